"""Octree evaluation on the MI355X path (reference: octree/evaluation.py): loads a tree npz and reports the
mean PSNR of its renders of the test split; test images are sharded over the GPUs.

    python -m plenoctree_amd.octree.evaluation --input tree_opt.npz --config blender --data_dir ... [--write_images DIR]
        [--keep_compressed]     (a tree written by octree.compression is rendered from its palette form, in place)
        [--keep_half]           (an uncompressed tree is rendered from the float16 data of its file, in place: the images of
                                 the float tree bit for bit; SH, SG and NDC scenes, --write_aux / --write_points on SH trees)
        [--max_depth L]         (the float tree rendered at level L in place, 2^(L+1) cells per axis, from the mean pyramid
                                 N3Tree.fill_internal_ writes into its unused rows; refused with --keep_half / --keep_compressed)
        [--lod_pixels P [--lod_min_depth M]]
                                (the float tree with every sample read at the first level whose cells are no wider than P
                                 pixels where the sample lies, never above depth M, from the same pyramid; composes with
                                 --max_depth, --write_aux and --write_points; refused with --keep_half / --keep_compressed
                                 and on an NDC scene)
        [--write_aux DIR]       (per view NNN_rgba.png, the render with its opacity as the alpha channel, and NNN_depth.npz
                                 with float32 depth / surface / alpha; distances are Euclidean, from the camera origin)
        [--write_points F.ply]  (every --points_stride-th pixel of every view whose transmittance falls to --surface_thresh,
                                 back-projected to its surface distance and coloured by the render)

An LLFF scene that is not --spherify is rendered in NDC (octree/nerf/utils.py:451-457); --keep_compressed, --write_aux and
--write_points are refused there by name, a compressed tree is re-inflated to floats and renders like any float tree.
"""
import os
import sys

import numpy as np

from .. import dist
from ..nerf_sh.nerf import llff, utils
from . import aux_io, extraction
from .._lib import TREE_MAX_DEPTH
from .svox import N3Tree


def define_flags():
    p = utils.define_flags()
    a = p.add_argument
    a("--input", type=str, default="./tree_opt.npz")            # octree/evaluation.py:54-58
    a("--write_vid", type=str, default=None)                     # :59-63 (mp4 through imageio there; GIF through PIL here)
    a("--write_images", type=str, default=None)                  # :64-68
    a("--renderer_step_size", type=float, default=1e-4)          # octree/nerf/utils.py:211-215
    a("--no_early_stop", action="store_true")
    a("--keep_compressed", action="store_true",
      help="evaluate a compressed tree (octree.compression) in its palette form instead of re-inflating it to float32")
    a("--keep_half", action="store_true",
      help="evaluate an uncompressed tree from the float16 data of its file, in place, instead of widening it to float32 "
           "(the same images bit for bit, half the device memory)")
    # not a reference flag: level of detail (VolumeRenderer(max_depth=...))
    a("--max_depth", type=int, default=None,
      help="render the float tree at this level in place, from the mean pyramid in its unused rows (0 = the root's 8 cells)")
    # not reference flags: a depth per sample from the pixel footprint (VolumeRenderer(lod_pixels=..., lod_min_depth=...))
    a("--lod_pixels", type=float, default=None,
      help="stop every sample's descent at the first cell no wider than this many pixels there (0 or unset: full depth)")
    a("--lod_min_depth", type=int, default=None, help=f"with --lod_pixels: never fold above this depth (0..{TREE_MAX_DEPTH}, default 0)")
    # not reference flags: the renderer's opacity / distance outputs (VolumeRenderer.render_persp_aux)
    a("--write_aux", type=str, default=None, help="directory for NNN_rgba.png and NNN_depth.npz of every test view")
    a("--write_points", type=str, default=None, help="binary PLY of the back-projected surface points of all test views")
    a("--points_stride", type=int, default=4, help="--write_points takes every n-th pixel along both image axes")
    a("--surface_thresh", type=float, default=0.5,
      help="transmittance at which a ray is taken to have reached the surface (above the early-stop threshold, below 1)")
    return p


def check_sg_flags(args):
    """An SG tree (data_format SG<K>) renders and is scored like an SH tree; its palette form and the extra outputs are not
    built, so the flags that need them are refused by name before anything is loaded onto the GPU."""
    with np.load(args.input) as z:
        fmt = str(z["data_format"]) if "data_format" in z.files else ""
    if not fmt.startswith("SG"):
        return
    bad = [f for f, on in (("--keep_compressed", args.keep_compressed), ("--write_aux", args.write_aux is not None),
                           ("--write_points", args.write_points is not None)) if on]
    if bad:
        raise NotImplementedError(f"{args.input} is an SG tree ({fmt}): {', '.join(bad)} not built for SG trees (palette-form "
                                  "rendering and the alpha / depth / surface outputs are SH only)")


def check_lod_flags(args):
    """--lod_pixels / --lod_min_depth: what they are refused with, by name, before anything is loaded."""
    if args.lod_pixels is None:
        if args.lod_min_depth is not None:
            raise ValueError("--lod_min_depth without --lod_pixels: it bounds the footprint render only")
        return
    if not 0 <= args.lod_pixels < float("inf"):
        raise ValueError(f"--lod_pixels {args.lod_pixels}: must be a finite number >= 0")
    if args.lod_min_depth is not None and not 0 <= args.lod_min_depth <= TREE_MAX_DEPTH:
        raise ValueError(f"--lod_min_depth {args.lod_min_depth}: must be in [0, {TREE_MAX_DEPTH}]")
    bad = [f for f, on in (("--keep_half", args.keep_half), ("--keep_compressed", args.keep_compressed)) if on]
    if bad:
        raise NotImplementedError(f"octree.evaluation: --lod_pixels together with {', '.join(bad)}: a footprint render reads "
                                  "the mean pyramid in the float tree's unused rows; the float16 and palette forms have none")
    if extraction.uses_ndc(args):
        raise NotImplementedError("octree.evaluation: --lod_pixels not built for an NDC scene (--dataset llff without "
                                  "--spherify): a ray parameter there is an NDC length, a pixel footprint along it has no "
                                  "meaning")


class _AuxSink:
    """Per-view consumer of eval_octree's aux_sink: writes the --write_aux files at once, collects the --write_points points."""

    def __init__(self, args, dataset):
        self.args, self.dataset = args, dataset
        self.xyz, self.colors = [], []
        if args.write_aux is not None:
            os.makedirs(args.write_aux, exist_ok=True)

    def __call__(self, idx, c2w, res):
        rgb, alpha, depth, surface = (res[k].cpu().numpy() for k in ("rgb", "alpha", "depth", "surface"))
        if self.args.write_aux is not None:
            aux_io.write_rgba_png(os.path.join(self.args.write_aux, f"{idx:03d}_rgba.png"), rgb, alpha)
            aux_io.write_depth_npz(os.path.join(self.args.write_aux, f"{idx:03d}_depth.npz"), depth, surface, alpha)
        if self.args.write_points is not None:
            xyz, col = aux_io.surface_points(c2w, self.dataset.focal, surface, rgb, self.args.points_stride)
            self.xyz.append(xyz)
            self.colors.append(col)

    def write_points(self, comm):
        path = self.args.write_points
        if comm.world > 1:
            path = os.path.splitext(path)[0] + f".rank{comm.rank}.ply"
        print("Writing to", path, flush=True)
        aux_io.write_ply(path, np.concatenate(self.xyz) if self.xyz else np.zeros((0, 3), np.float32),
                         np.concatenate(self.colors) if self.colors else np.zeros((0, 3), np.uint8))


def main(argv=None):
    args = define_flags().parse_args(argv)
    utils.update_flags(args)
    if args.write_vid is not None and os.path.splitext(args.write_vid)[1].lower() != ".gif":
        # checked BEFORE anything is rendered: imageio / ffmpeg are not installed, so only the animated GIF writer is built
        raise ValueError(f"--write_vid {args.write_vid}: only animated GIF output is built (no imageio/ffmpeg here); "
                         "give a .gif path")
    if args.keep_half and args.keep_compressed:
        raise ValueError("--keep_half together with --keep_compressed: a file holds either float16 data or the palette form; "
                         "give the flag that matches --input")
    if args.max_depth is not None:
        bad = [f for f, on in (("--keep_half", args.keep_half), ("--keep_compressed", args.keep_compressed)) if on]
        if bad:
            raise NotImplementedError(f"octree.evaluation: --max_depth together with {', '.join(bad)}: a capped render reads the "
                                      "mean pyramid in the float tree's unused rows; the float16 and palette forms have none")
        if args.max_depth < 0:
            raise ValueError(f"--max_depth {args.max_depth}: must be >= 0")
    check_lod_flags(args)
    extraction.check_octree_flags(args, "octree.evaluation", (("--keep_compressed", args.keep_compressed),
                                                              ("--write_aux", args.write_aux is not None),
                                                              ("--write_points", args.write_points is not None)))
    want_aux = args.write_aux is not None or args.write_points is not None
    if want_aux and args.points_stride < 1:
        raise ValueError(f"--points_stride {args.points_stride}: must be >= 1")
    comm, device, _ = dist.open_cli("octree.evaluation")
    dataset = llff.get_dataset("test", args, device)
    if comm.rank == 0:
        print("N3Tree load", args.input, flush=True)
    check_sg_flags(args)
    tree = N3Tree.load(args.input, map_location=device, keep_quantized=args.keep_compressed,   # not compressed + flag: ValueError
                       keep_half=args.keep_half)                                               # compressed + flag: ValueError
    if args.keep_compressed and comm.rank == 0:
        print(f"compressed tree kept in place: {tree.nbytes / 2 ** 20:.1f} MB on the device "
              f"(float form: {tree.float_nbytes / 2 ** 20:.1f} MB)", flush=True)
    if args.keep_half and comm.rank == 0:
        print(f"float16 tree kept in place: {tree.nbytes / 2 ** 20:.1f} MB on the device "
              f"(float form: {tree.float_nbytes / 2 ** 20:.1f} MB)", flush=True)
    want_frames = args.write_images is not None or args.write_vid is not None
    lod = {"lod_pixels": args.lod_pixels, "lod_min_depth": args.lod_min_depth or 0}
    if want_aux:
        sink = _AuxSink(args, dataset)
        psnr, ssim, frames = extraction.eval_octree(tree, dataset, args, comm, want_frames=want_frames, want_ssim=True,
                                                    aux_sink=sink, surface_thresh=args.surface_thresh, max_depth=args.max_depth,
                                                    **lod)
        if args.write_points is not None:
            sink.write_points(comm)
    else:
        psnr, ssim, frames = extraction.eval_octree(tree, dataset, args, comm, want_frames=want_frames, want_ssim=True,
                                                    max_depth=args.max_depth, **lod)
    if comm.rank == 0:
        print("Average PSNR", psnr, "SSIM", ssim, flush=True)
    if args.write_vid is not None and frames:
        # imageio / ffmpeg are not installed: this rank's frames (every world-th view) as an animated GIF
        from PIL import Image
        path = args.write_vid if comm.world == 1 else os.path.splitext(args.write_vid)[0] + f".rank{comm.rank}.gif"
        print("Writing to", path, flush=True)
        ims = [Image.fromarray(im.numpy()) for _, im in frames]
        ims[0].save(path, save_all=True, append_images=ims[1:], duration=50, loop=0)
    if args.write_images is not None:
        from PIL import Image
        os.makedirs(args.write_images, exist_ok=True)
        for idx, im in frames:
            Image.fromarray(im.numpy()).save(os.path.join(args.write_images, f"{idx:03d}.png"))
    comm.shutdown()
    return psnr


if __name__ == "__main__":
    main(sys.argv[1:])
