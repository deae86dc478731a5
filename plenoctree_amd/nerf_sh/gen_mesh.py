"""Mesh of a trained NeRF-SH's sigma isosurface (reference: nerf_sh/gen_mesh.py): sigma on a dense grid through the
HIP point evaluator (the sigma-only head pass, same kernel as the extraction grid), marching cubes, OBJ out.

    python -m plenoctree_amd.nerf_sh.gen_mesh --train_dir D --config blender --reso "300 300 300" --iso 6.0 [--mc host]
        [--color none|view] [--normals] [--format obj|ply]

PyMCubes is not installed here; `isosurface.marching_cubes` takes its place (same vertices, see that module).  By default
the sigma grid stays on the GPU and is meshed there (plenoctree_amd.mesh_ops, the same definition and output order, so
mesh.obj is byte-identical); `--mc host` copies the grid to the host and runs the numpy function instead.

The reference stops at geometry: its flags (gen_mesh.py:77-82) end with `coarse`, and save_obj (:133-158) takes a vert_rgb that
main never passes ("# TODO: implement color").  Here --normals adds the unit normal n = -(g / s) / |g / s| of the sigma
gradient g at every vertex (mesh_ops / isosurface.vertex_gradients on the grid that was meshed; s = (c2 - c1) / reso, the world
length of an index step under the reference's scaling; float64, out of the solid, (0, 0, 0) where g = 0), and --color view
evaluates raw_rgb at the vertices and shades it along d = -n, the ray of a camera looking straight at the surface
(pxo_shade_points: the SH basis, or the SG basis with the model's lobes).  --format ply writes mesh.ply (binary) instead of
mesh.obj.  Without these flags the file is today's, byte for byte.
"""
import os
import sys

import numpy as np
import torch

from . import isosurface
from .nerf import families, sg, utils

MC_CHOICES = ("device", "host")
COLOR_CHOICES = ("none", "view")
FORMAT_CHOICES = ("obj", "ply")

def define_flags():
    """nerf_sh/gen_mesh.py:49-76."""
    p = utils.define_flags()
    a = p.add_argument
    a("--reso", type=str, default="300 300 300", help="marching cubes resolution in each dimension: x y z")
    a("--c1", type=str, default="-2 -2 -2", help="lower corner, x y z or one number")
    a("--c2", type=str, default="2 2 2", help="upper corner, x y z or one number")
    a("--iso", type=float, default=6.0, help="sigma isosurface")
    a("--coarse", type=utils._bool, nargs="?", const=True, default=False, help="force the coarse network")
    a("--point_chunk", type=int, default=720720, help="points per evaluator launch (--chunk is ignored)")
    a("--mc", choices=MC_CHOICES, default="device",
      help="where marching cubes runs: on the GPU that holds the sigma grid, or on the host (same mesh.obj, byte for byte)")
    a("--color", choices=COLOR_CHOICES, default="none",
      help="per-vertex colour: view = raw_rgb at the vertex shaded along the inward normal (the reference has none)")
    a("--normals", action="store_true", help="write per-vertex unit normals (out of the solid) from the sigma gradient")
    a("--format", choices=FORMAT_CHOICES, default="obj", help="mesh.obj, or binary mesh.ply")
    return p


def sigma_grid(fn, c1, c2, reso, chunk, device):
    """:105-119: raw sigma at linspace(c1, c2, reso) per axis (end points included), ij order -> float32 [rx, ry, rz].
    `fn(points [n,3]) -> raw_sigma [n,1]`.  The axis coordinates are numpy float32 linspaces like the reference's; the
    point list is assembled per chunk on the device instead of materialising the [N,3] host array."""
    axes = [torch.from_numpy(np.linspace(lo, hi, sz, dtype=np.float32)).to(device) for lo, hi, sz in zip(c1, c2, reso)]
    ny, nz = reso[1], reso[2]
    total = reso[0] * ny * nz
    out = torch.empty(total, dtype=torch.float32, device=device)
    for s in range(0, total, chunk):
        idx = torch.arange(s, min(s + chunk, total), device=device)
        pts = torch.stack([axes[0][idx // (ny * nz)], axes[1][(idx // nz) % ny], axes[2][idx % nz]], 1)
        out[s:s + idx.numel()] = fn(pts.contiguous()).reshape(-1)
    return out.reshape(*reso)


def marching_cubes(fn, c1, c2, reso, isosurface_level, chunk, device, mc="device", normals=False):
    """:88-130.  Vertices are scaled by (c2 - c1) / reso exactly as the reference does (:127) - note the samples sit
    at spacing (c2 - c1) / (reso - 1), so the reference's mesh is shrunk by (reso-1)/reso towards c1; kept for parity.
    mc: "device" meshes a sigma grid that lives on a GPU there (mesh_ops.marching_cubes) and only the mesh comes back;
    "host", or a grid on the CPU, goes through isosurface.marching_cubes.  The two return identical arrays.
    normals=True returns a third array, the unit normals float64 [V,3] (see the module text), from the same grid by the path
    that meshed it: mesh_ops.mesh_with_gradients or isosurface.vertex_gradients, which agree element for element."""
    if mc not in MC_CHOICES:
        raise ValueError(f"mc must be one of {MC_CHOICES}, got {mc!r}")
    sigmas = sigma_grid(fn, c1, c2, reso, chunk, device)
    print("* Running marching cubes", flush=True)
    grad = None
    if mc == "device" and sigmas.is_cuda:
        from .. import mesh_ops
        if normals:
            vertices, triangles, _, grad = mesh_ops.mesh_with_gradients(sigmas, isosurface_level)
            grad = grad.cpu().numpy()
        else:
            vertices, triangles, _ = mesh_ops.marching_cubes(sigmas, isosurface_level)
        vertices, triangles = vertices.cpu().numpy(), triangles.cpu().numpy()
    else:
        host = sigmas.cpu().numpy()
        vertices, triangles = isosurface.marching_cubes(host, isosurface_level)
        if normals:
            grad = isosurface.vertex_gradients(host, isosurface_level)
    c1, c2 = np.array(c1), np.array(c2)
    step = (c2 - c1) / np.array(reso)
    vertices = vertices * step
    if normals:
        from ..mesh_ops import unit_normals
        return vertices + c1, triangles, unit_normals(grad, step)
    return vertices + c1, triangles


def save_obj(vertices, triangles, path, vert_rgb=None):
    """:133-158: `v x y z [r g b]` with four decimals, then 1-based `f a b c`."""
    with open(path, "w") as f:
        if vert_rgb is None:
            f.writelines("v %.4f %.4f %.4f\n" % tuple(v) for v in vertices)
        else:
            f.writelines("v %.4f %.4f %.4f %.4f %.4f %.4f\n" % (*v, *c) for v, c in zip(vertices, vert_rgb))
        f.writelines("f %d %d %d\n" % tuple(t) for t in (np.asarray(triangles) + 1))


def vertex_colors(model, state, vertices, normals, chunk, coarse=False):
    """--color view: raw_rgb of the network at the vertices (float32 positions, `chunk` points per evaluator launch), shaded
    along d = -n by pxo_shade_points with the model's basis -- SH, or SG with state.lobes.  float32 [V,3] on the host."""
    from .. import mesh_ops
    device = state.params.device
    K = (model.cfg.sh_deg + 1) ** 2
    pts = torch.from_numpy(np.ascontiguousarray(vertices, dtype=np.float32)).to(device)
    dirs = torch.from_numpy(mesh_ops.shading_dirs(normals)).to(device)
    out = torch.empty(len(pts), 3, dtype=torch.float32, device=device)
    for s in range(0, len(pts), chunk):
        raw_rgb = model.eval_points_raw(state, pts[s:s + chunk].contiguous(), coarse=coarse, want_rgb=True)[0]
        out[s:s + chunk] = mesh_ops.shade_points(raw_rgb.reshape(-1, 3 * K).contiguous(), dirs[s:s + chunk], K,
                                                 lobes=getattr(state, "lobes", None))
    return out.cpu().numpy()


def _triple(s, cast):
    v = [cast(x) for x in s.split()]
    return v * 3 if len(v) == 1 else v


def main(argv=None):
    """:161-194."""
    args = define_flags().parse_args(argv)
    utils.update_flags(args)
    sg.apply_cli(args, argv)                     # --sg_dim K --sh_deg -1 on the command line win over the preset's sh_deg
    if not torch.cuda.is_available():
        raise SystemExit("nerf_sh.gen_mesh needs a ROCm GPU; the HIP path has no CPU fallback")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    families.check(args, "mesh", require_data=False)
    reso, c1, c2 = _triple(args.reso, int), _triple(args.c1, float), _triple(args.c2, float)
    print("* Creating model", flush=True)
    model, state = families.restore(args, device, "mesh", require_data=False)
    print("* Eval reso", args.reso, "coarse?", args.coarse, flush=True)
    print("* Evaluating sigma @", reso[0] * reso[1] * reso[2], "points", flush=True)

    def fn(points):
        return model.eval_points_raw(state, points, coarse=args.coarse, want_rgb=False)[1]

    want_normals = args.normals or args.color == "view"
    out = marching_cubes(fn, c1, c2, reso, args.iso, args.point_chunk, device, mc=args.mc, normals=want_normals)
    verts, faces, normals = out if want_normals else (*out, None)
    mesh_path = os.path.join(args.train_dir, "mesh." + args.format)
    if args.color == "none" and not args.normals and args.format == "obj":          # the reference's output
        print(" Saving to", mesh_path, flush=True)
        save_obj(verts, faces, mesh_path)
        return verts, faces
    from .. import mesh_io
    rgb = None
    if args.color == "view":
        print("* Shading", len(verts), "vertices along their normals", flush=True)
        rgb = vertex_colors(model, state, verts, normals, args.point_chunk, coarse=args.coarse)
    print(" Saving to", mesh_path, flush=True)
    mesh_io.save_mesh(verts, faces, mesh_path, normals=normals if args.normals else None, vert_rgb=rgb, fmt=args.format)
    return verts, faces, rgb, (normals if args.normals else None)


if __name__ == "__main__":
    main(sys.argv[1:])
