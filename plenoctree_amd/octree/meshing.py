"""Surface mesh of a PlenOctree: the sigma isosurface of the tree on its own dense cell grid, by marching cubes on the GPU.

    python -m plenoctree_amd.octree.meshing --input D/tree_opt.npz --output D/tree_mesh.obj \
        [--iso 10.0] [--depth D] [--color dc|view|none] [--normals]

No counterpart in the reference (octree.evaluation --write_points gives a point cloud, nerf_sh.gen_mesh meshes the NeRF).
Steps: the tree is loaded through N3Tree.load (a compressed file is re-inflated by the loader); sigma is sampled at the
centres of the 2^depth cells per axis with one layer of zeros around them (mesh_ops.tree_sigma_grid, an integer descent:
exact at every depth), so that with --iso > 0 a surface that touches the cube is closed; marching cubes runs on that grid on
the device (mesh_ops.marching_cubes, the definition of nerf_sh/isosurface.py); vertices go from padded index units v to tree
coordinates t = (v - 1/2) / 2^depth and to world space (t - offset) / invradius in float64; nerf_sh.gen_mesh.save_obj writes
the file (plenoctree_amd.mesh_io when normals are asked for or --output ends in .ply, which selects binary PLY).

--depth defaults to the tree's own finest grid (max_depth + 1) and may be coarser or finer, up to PXO_TREE_MAX_DEPTH + 1.
--color dc (the default for SH trees) gives every vertex the view-independent band of the leaf at the inside end of its edge,
sigmoid(0.28209479177387814 * data[leaf, c * K]) for c = 0, 1, 2 in float32; SG trees have no such band: --color dc is refused
for them by name and they mesh with --color none (their default).  --color view (SH and SG trees) shades the same leaf along
d = -n, the ray of a camera looking straight at the surface: sigmoid(sum_k Y_k(d) data[leaf, c * K + k]) with the basis the
renderer uses (pxo_shade_points, the leaves read in place).  n is the unit normal -(g / s) / |g / s| of the sigma gradient g at
the vertex (pxo_mc_vertex_gradients; s = 1 / (2^depth invradius), the world length of an index step per axis), float64, pointing
out of the solid; --normals writes it (`vn` records in an OBJ, nx ny nz in a PLY).  Where g = 0 the normal is (0, 0, 0) and the
shading direction (0, 0, 1).  The tree of a forward-facing (LLFF) scene lives in the NDC
cube and is meshed there: the vertices are NDC coordinates, nothing is converted back to world space -- normals and --color
view are then taken in NDC as well, where a direction has no world meaning (world-space normals for NDC trees are not built).
"""
import argparse
import os
import sys

import numpy as np
import torch

from .._lib import TREE_MAX_DEPTH
from ..mesh_io import save_mesh

SH_C0 = 0.28209479177387814
PAD = 1


def define_flags():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    a = p.add_argument
    a("--input", "-i", type=str, required=True, help="tree npz (float or compressed)")
    a("--output", "-o", type=str, required=True, help="OBJ file to write; binary PLY if the name ends in .ply")
    a("--iso", type=float, default=10.0, help="sigma isosurface, > 0")
    a("--depth", type=int, default=None,
      help=f"sample 2^depth cells per axis; default: the tree's finest grid (max_depth + 1); at most {TREE_MAX_DEPTH + 1}")
    a("--color", choices=("dc", "view", "none"), default=None,
      help="per-vertex colour: dc = the view-independent SH band, view = shaded along the inward normal (SH and SG trees); "
           "default: dc for SH trees, none for SG trees")
    a("--normals", action="store_true", help="write per-vertex unit normals (out of the solid) from the sigma gradient")
    return p


def index_to_world(vertices, depth, offset, invradius, pad=PAD):
    """Vertices in index units of the padded 2^depth grid -> world space, float64: sample v sits at the centre of cell
    v - pad, tree coordinate t = (v - pad + 1/2) / 2^depth; world = (t - offset) / invradius."""
    v = np.asarray(vertices, np.float64)
    t = (v - (pad - 0.5)) / float(1 << depth)
    return (t - np.asarray(offset, np.float64)) / np.asarray(invradius, np.float64)


def dc_colors(data, basis_dim, leaves):
    """sigmoid(SH_C0 * data[leaf, c * K]), c = 0, 1, 2: float32 [n, 3] on the device of `data` ([n_internal,2,2,2,3K+1])."""
    rows = data.reshape(-1, data.shape[-1])[leaves]
    return torch.sigmoid(rows[:, [0, basis_dim, 2 * basis_dim]] * np.float32(SH_C0))


def check_args(args):
    """Everything that can be refused without a GPU.  Returns the file's data format string."""
    if not args.iso > 0.0:
        raise SystemExit(f"--iso must be > 0 (got {args.iso}): the grid is padded with sigma 0, which has to lie outside")
    if args.depth is not None and not 1 <= args.depth <= TREE_MAX_DEPTH + 1:
        raise SystemExit(f"--depth {args.depth} outside [1, {TREE_MAX_DEPTH + 1}] (PXO_TREE_MAX_DEPTH + 1)")
    if not os.path.isfile(args.input):
        raise SystemExit(f"--input {args.input}: no such file")
    with np.load(args.input) as z:
        fmt = str(z["data_format"]) if "data_format" in z.files else "RGBA"
    if fmt.startswith("SG") and args.color == "dc":
        raise SystemExit(f"--color dc on an SG tree ({fmt}): a spherical-Gaussian tree has no view-independent (DC) band; "
                         "mesh it with --color none")
    return fmt


def index_step(depth, invradius):
    """World length of one index step of the 2^depth grid per axis, float64 [3]: 1 / (2^depth invradius)."""
    return 1.0 / (float(1 << depth) * np.asarray(invradius, np.float64))


def mesh_tree(tree, iso, depth, color, normals=False):
    """(world vertices float64 [V,3], triangles int64 [T,3], colours float32 [V,3] or None, unit normals float64 [V,3] or None)
    of a float N3Tree on the GPU.  The normals are computed for color == "view" too but only returned when asked for."""
    from .. import mesh_ops
    sigma, packed = mesh_ops.tree_sigma_grid(tree.view(), depth, pad=PAD, want_packed=color != "none", device=tree.device)
    nrm = None
    if normals or color == "view":
        v, f, inside, grad = mesh_ops.mesh_with_gradients(sigma, iso)
        nrm = mesh_ops.unit_normals(grad, index_step(depth, tree.invradius.numpy()))
    else:
        v, f, inside = mesh_ops.marching_cubes(sigma, iso)
    rgb = None
    if color == "dc":
        rgb = dc_colors(tree.data.data, tree.basis_dim, packed.reshape(-1)[inside]).cpu().numpy()
    elif color == "view":
        data = tree.data.data
        rgb = mesh_ops.shade_points(data.reshape(-1, data.shape[-1]), mesh_ops.shading_dirs(nrm), tree.basis_dim,
                                    rows=packed.reshape(-1)[inside], lobes=tree.extra_data).cpu().numpy()
    world = index_to_world(v.cpu().numpy(), depth, tree.offset.numpy(), tree.invradius.numpy())
    return world, f.cpu().numpy(), rgb, (nrm.cpu().numpy() if normals else None)


def main(argv=None):
    args = define_flags().parse_args(argv)
    fmt = check_args(args)
    color = args.color or ("none" if fmt.startswith("SG") else "dc")
    if not torch.cuda.is_available():
        raise SystemExit("octree.meshing needs a ROCm GPU; the HIP path has no CPU fallback")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    from .svox import N3Tree
    print("N3Tree load", args.input, flush=True)
    tree = N3Tree.load(args.input, map_location=device)
    depth = tree.max_depth + 1 if args.depth is None else args.depth
    print(f"* Sampling sigma at depth {depth} ({(1 << depth) + 2 * PAD}^3 with the pad), iso {args.iso}", flush=True)
    verts, faces, rgb, normals = mesh_tree(tree, args.iso, depth, color, normals=args.normals)
    print(f"* {len(verts)} vertices, {len(faces)} triangles -> {args.output}", flush=True)
    save_mesh(verts, faces, args.output, normals=normals, vert_rgb=rgb)
    return verts, faces, rgb


if __name__ == "__main__":
    main(sys.argv[1:])
