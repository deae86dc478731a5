"""Writes a PlenOctree at coarser depths: every cell of level L takes the density-weighted mean of the subtree below it.  No
reference counterpart (the reference stops at octree/optimization.py), and the reduction is this project's definition, not
svox's (include/plenoctree_octree.h, "level of detail").

    python -m plenoctree_amd.octree.lod --input tree_opt.npz --output_dir lods/ --depths 6 7 \\
        [--eval true --config C --data_dir DATA] [--renderer_step_size 1e-4]

For every depth L it writes <output_dir>/<stem>_d<L>.npz with tree.lod(L).save(...): a tree every other tool takes as it is
(octree.optimization, octree.compression, octree.evaluation with or without --keep_half, octree.meshing, octree.pruning).
One line per depth and one for the source: nodes, leaves, the bytes of the float32 form (octree.pruning.tree_stats) and the
file size; with --eval also the test-split PSNR / SSIM.  The same table goes to <output_dir>/lod.json.  A compressed input
(octree.compression), --render_path and a depth outside [0, max_depth] are refused by name before a GPU or a dataset is
touched; without --eval no dataset flag is needed.
"""
import json
import os
import sys

import numpy as np
import torch

from ..nerf_sh.nerf import llff, utils
from . import extraction
from .pruning import tree_stats
from .svox import N3Tree, parent_depth_from_child


def define_flags():
    p = utils.define_flags()
    a = p.add_argument
    a("--input", type=str, default="./tree_opt.npz")
    a("--output_dir", type=str, default="./lods")
    a("--depths", type=int, nargs="+", required=True, help="levels to write: 0 (the root's 8 cells) .. the tree's max_depth")
    a("--renderer_step_size", type=float, default=1e-4)
    a("--no_early_stop", action="store_true", help="--eval renders without the early-stopping preset")
    a("--eval", type=utils._bool, default=False, help="also print the test-split PSNR / SSIM of the source and of every level")
    return p


def check_flags(args):
    extraction.check_octree_flags(args, "octree.lod")
    if not args.renderer_step_size > 0.0:
        raise ValueError(f"--renderer_step_size {args.renderer_step_size}: must be > 0")


def check_input(path, depths):
    """The file's own refusals, read from its header arrays on the host."""
    with np.load(path) as z:
        if "quant_colors" in z.files:
            raise NotImplementedError(f"octree.lod: {path} is a compressed tree (octree.compression): the palette form is "
                                      "read-only; coarsen the float tree and compress the result")
        n = int(z["n_internal"]) if "n_internal" in z.files else z["child"].shape[0]
        if "parent_depth" in z.files:
            max_depth = int(z["parent_depth"][:n, 1].max())
        else:
            max_depth = int(parent_depth_from_child(z["child"][:n])[:, 1].max())
    bad = [d for d in depths if not 0 <= d <= max_depth]
    if bad:
        raise ValueError(f"octree.lod: --depths {' '.join(map(str, bad))} outside [0, {max_depth}], the max_depth of {path}")
    return max_depth


def _row(name, tree, path, scores):
    nodes, leaves, nbytes = tree_stats(tree)
    row = {"name": name, "nodes": nodes, "leaves": leaves, "float32_bytes": nbytes, "file_bytes": os.path.getsize(path)}
    if scores is not None:
        row["psnr"], row["ssim"] = scores
    print(" ".join(f"{k} {v}" for k, v in row.items()), flush=True)
    return row


def main(argv=None):
    args = define_flags().parse_args(argv)
    utils.update_flags(args)
    check_flags(args)
    check_input(args.input, args.depths)
    if not torch.cuda.is_available():
        raise SystemExit("octree.lod needs a ROCm GPU; the HIP path has no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    test = llff.get_dataset("test", args, device) if args.eval else None
    score = (lambda t: extraction.eval_octree(t, test, args, want_ssim=True)[:2]) if args.eval else (lambda t: None)
    print("N3Tree load", args.input, flush=True)
    tree = N3Tree.load(args.input, map_location=device)
    tree.data.requires_grad_(False)
    os.makedirs(args.output_dir, exist_ok=True)
    stem = os.path.splitext(os.path.basename(args.input))[0]
    table = [_row("source", tree, args.input, score(tree))]
    for L in args.depths:
        path = os.path.join(args.output_dir, f"{stem}_d{L}.npz")
        level = tree.lod(L)                              # the first call fills the source's unused rows, the others reuse them
        level.save(path, compress=False)
        table.append(_row(f"d{L}", level, path, score(level)))
        table[-1]["path"] = path
    with open(os.path.join(args.output_dir, "lod.json"), "w") as f:
        json.dump(table, f, indent=1)
    return table


if __name__ == "__main__":
    main(sys.argv[1:])
