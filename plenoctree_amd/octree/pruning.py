"""Prunes (and optionally refines) a PlenOctree by the weight its leaves render the training views with.  No reference
counterpart: the reference stops at octree/optimization.py; the piece of svox this is built on is N3Tree.accumulate_weights.

    python -m plenoctree_amd.octree.pruning --config C --data_dir DATA --input tree_opt.npz --output tree_pruned.npz \\
        [--weight_thresh 0.001] [--no_collapse] [--refine_thresh W] [--renderer_step_size 1e-4] [--eval true]

The maximum compositing weight of every leaf over all pixels of the training cameras is accumulated with the exact march
(stop_thresh = 0, as the extraction's weight mask).  Leaves with weight <= --weight_thresh are zeroed; unless --no_collapse,
nodes left with nothing but such leaves are folded back into their parents.  With --refine_thresh W the surviving leaves
with weight >= W are then split once (children inherit the value), so that another round of octree.optimization has
resolution where the image comes from; the tree's depth_limit is raised by one for that split (up to the library's maximum
of 10), since the extraction leaves its finest leaves at the limit.  An LLFF scene that is not --spherify is marched in NDC.  --render_path and a
compressed input (octree.compression) are refused by name.
"""
import sys

import numpy as np
import torch

from .._lib import TREE_MAX_DEPTH
from ..nerf_sh.nerf import llff, utils
from . import extraction
from .svox import N3Tree, VolumeRenderer


def define_flags():
    p = utils.define_flags()
    a = p.add_argument
    a("--input", type=str, default="./tree_opt.npz")
    a("--output", type=str, default="./tree_pruned.npz")
    a("--weight_thresh", type=float, default=1e-3, help="a leaf is kept when its maximum compositing weight is above this")
    a("--no_collapse", action="store_true", help="only zero the dead leaves; keep the tree's structure")
    a("--refine_thresh", type=float, default=None, help="then split once every surviving leaf with weight >= this")
    a("--renderer_step_size", type=float, default=1e-4)
    a("--no_early_stop", action="store_true", help="--eval renders without the early-stopping preset")
    a("--eval", type=utils._bool, default=False, help="print the test-split PSNR of the tree before and after")
    return p


def check_flags(args):
    """Everything refused by name, before a GPU or a dataset is touched."""
    extraction.check_octree_flags(args, "octree.pruning")
    if not args.weight_thresh >= 0.0:
        raise ValueError(f"--weight_thresh {args.weight_thresh}: must be >= 0")
    if args.refine_thresh is not None and not args.refine_thresh > args.weight_thresh:
        raise ValueError(f"--refine_thresh {args.refine_thresh}: must be above --weight_thresh {args.weight_thresh} (only "
                         "surviving leaves are split)")
    if not args.renderer_step_size > 0.0:
        raise ValueError(f"--renderer_step_size {args.renderer_step_size}: must be > 0")


def check_input(path):
    with np.load(path) as z:
        if "quant_colors" in z.files:
            raise NotImplementedError(f"octree.pruning: {path} is a compressed tree (octree.compression): the palette form is "
                                      "read-only; prune the float tree and compress the result")


def tree_stats(tree):
    """(nodes, leaves, bytes of child + parent_depth + float32 data)."""
    n = tree.n_internal
    return n, tree.n_leaves, 4 * n * (8 + 2 + 8 * tree.data_dim)


@torch.no_grad()
def leaf_weights(tree, c2ws, H, W, focal, step_size, ndc=None, op="max"):
    """[n_internal, 2, 2, 2] weights of `tree`'s leaves over the cameras c2ws [n,4,4], exact march."""
    renderer = VolumeRenderer(tree, step_size=step_size, ndc=ndc)
    with tree.accumulate_weights(op=op) as accum:
        for c2w in c2ws:
            renderer.render_persp(c2w, width=W, height=H, fx=focal, fast=False)
    return accum.value


def main(argv=None):
    args = define_flags().parse_args(argv)
    utils.update_flags(args)
    check_flags(args)
    check_input(args.input)
    if not torch.cuda.is_available():
        raise SystemExit("octree.pruning needs a ROCm GPU; the HIP path has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    ds = llff.get_dataset("train", args, device)
    c2ws = torch.from_numpy(np.ascontiguousarray(ds.camtoworlds)).float().to(device)
    print("N3Tree load", args.input, flush=True)
    tree = N3Tree.load(args.input, map_location=device)
    tree.data.requires_grad_(False)
    ndc = extraction.ndc_config(args, ds)
    test = llff.get_dataset("test", args, device) if args.eval else None
    before = tree_stats(tree)
    print("before: nodes %d leaves %d bytes %d" % before, flush=True)
    if test is not None:
        print("before: test psnr", extraction.eval_octree(tree, test, args)[0], flush=True)

    weights = leaf_weights(tree, c2ws, ds.h, ds.w, ds.focal, args.renderer_step_size, ndc)
    keep = weights > args.weight_thresh
    leaves = tree.child == 0
    print(f"max weight over {c2ws.shape[0]} training cameras: {int((keep & leaves).sum())} of {tree.n_leaves} leaves above "
          f"{args.weight_thresh}", flush=True)
    removed = tree.prune_(keep, collapse=not args.no_collapse)
    print(f"pruned: {removed} nodes removed", flush=True)
    if args.refine_thresh is not None:
        # the collapse has moved the cells: weigh the pruned tree again rather than carry the old weights across
        weights = leaf_weights(tree, c2ws, ds.h, ds.w, ds.focal, args.renderer_step_size, ndc)
        if tree.depth_limit < TREE_MAX_DEPTH:
            # octree.extraction leaves depth_limit at the depth it built, so the finest leaves -- the ones that carry the
            # image -- sit at the limit: one more level is allowed for this one split
            tree.depth_limit += 1
            print("depth_limit raised to", tree.depth_limit, flush=True)
        added = tree.refine_leaves(weights >= args.refine_thresh)
        print(f"refined: {added} leaves with weight >= {args.refine_thresh} split", flush=True)
    after = tree_stats(tree)
    print("after: nodes %d leaves %d bytes %d" % after, flush=True)
    if test is not None:
        print("after: test psnr", extraction.eval_octree(tree, test, args)[0], flush=True)
    print("Saving to", args.output, flush=True)
    tree.save(args.output, compress=False)
    return before, after


if __name__ == "__main__":
    main(sys.argv[1:])
