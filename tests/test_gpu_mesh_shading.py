"""Normals and view-dependent colour of device meshes on the MI355X: pxo_mc_vertex_gradients against the host definition
isosurface.vertex_gradients (exact: np.array_equal on float64), pxo_shade_points against a float64 restatement of its sum, and the
two CLIs end to end.

Shading bound.  max |HIP - float64| <= 4 x floor, floor = max |the same restatement evaluated in float32 - its float64 self|.
One floor per (K, basis): it is taken over the case's whole point set (257 points x 3 channels, with the rows the run gathers),
and the runs at n = 1, 63, 64, 65 are prefixes of that set held to the same bound -- a floor estimated from the three numbers of
an n = 1 run would be noise, not the rounding level of the arithmetic.  Launch geometry of the two kernels: one vertex / point per
lane, 256 per workgroup; 63 / 64 / 65 straddle a wave, 257 is a second workgroup holding one point."""
import os

import numpy as np
import pytest
import torch

import _mesh_oracle as M
from _helpers import _gpu
from oracle import nerf_oracle as O
from plenoctree_amd import mesh_io, mesh_ops, octree_ops as oops
from plenoctree_amd.nerf_sh import gen_mesh, isosurface
from plenoctree_amd.octree import meshing, svox

pytestmark = pytest.mark.gpu

_worst = {}


# ---- gradients -------------------------------------------------------------------------------------------------------
def _same_gradients(vol, iso):
    """Host and device gradients of the float32 array `vol` must be equal; so must the mesh that comes with them."""
    dev = _gpu()
    assert vol.dtype == np.float32
    want = isosurface.vertex_gradients(vol, iso)
    dvol = torch.from_numpy(vol).to(dev)
    got = mesh_ops.vertex_gradients(dvol, iso)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), "gradients"
    v, f, inside, grad = mesh_ops.mesh_with_gradients(dvol, iso)
    hv, hf = isosurface.marching_cubes(vol, iso)
    assert np.array_equal(v.cpu().numpy(), hv) and np.array_equal(f.cpu().numpy(), hf) and torch.equal(grad, got)
    return got


def _all_cases_pattern():
    """bool [512, 2, 2]: cell 2c (corners x in {2c, 2c+1}) has corner pattern c, corner = dx + 2 dy + 4 dz."""
    pat = np.zeros((512, 2, 2), bool)
    for c in range(256):
        for corner in range(8):
            pat[2 * c + (corner & 1), (corner >> 1) & 1, (corner >> 2) & 1] = (c >> corner) & 1
    return pat


def test_gradients_on_all_256_cases_with_random_magnitudes():
    pat = _all_cases_pattern()
    mag = (np.random.RandomState(0).rand(*pat.shape) * 3.0 + 1e-3).astype(np.float32)
    vol = np.where(pat, np.float32(0.5) + mag, np.float32(0.5) - mag).astype(np.float32)
    assert np.array_equal(vol >= np.float32(0.5), pat)
    g = _same_gradients(vol, 0.5)
    assert len(g) > 1000 and bool(torch.isfinite(g).all())


# the launch-geometry list of test_gpu_mesh.py that the issue names: one workgroup exactly, one minus a point, a last workgroup of
# one point, z around the wave size, more than one scan tile
SHAPES = [(2, 2, 2), (4, 8, 8), (3, 5, 17), (3, 3, 57), (3, 4, 65), (65, 64, 66)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradients_on_shapes_around_the_launch_geometry(shape):
    n = int(np.prod(shape))
    vol = np.random.RandomState(n).standard_normal(shape).astype(np.float32)
    g = _same_gradients(vol, 0.1)
    assert len(g) > 0
    if shape == (65, 64, 66):
        assert len(g) > 256 * 256                                     # many workgroups of the one-vertex-per-lane kernel


def test_gradients_of_degenerate_fields():
    vol = np.zeros((5, 5, 5), np.float32)
    vol[2, 2, 2] = 1.0                                                # one point exactly at iso: f = 0 above it, f = 1 below
    g = _same_gradients(vol, 1.0)
    assert tuple(g.shape) == (6, 3) and bool((g == 0).all())
    # iso = 0.7 against float32(0.7) < 0.7: inside by the float32 comparison, f slightly outside [0, 1]
    vol = np.zeros((4, 4, 4), np.float32)
    vol[1, 2, 1] = np.float32(0.7)
    assert tuple(_same_gradients(vol, 0.7).shape) == (6, 3)
    # a thin slab: an inside point between two outside ones owns a vertex on either side along x
    vol = np.random.RandomState(3).rand(5, 6, 7).astype(np.float32)
    vol[2] += 2.0
    assert len(_same_gradients(vol, 1.5)) == 2 * 6 * 7
    # no crossing: empty output (the wrapper returns before the emit and gradient launches)
    for fill in (0.0, 2.0, 1.0):
        g = _same_gradients(np.full((6, 7, 9), fill, np.float32), 1.0)
        assert tuple(g.shape) == (0, 3)
    assert tuple(_same_gradients(np.zeros((1, 5, 5), np.float32), 0.5).shape) == (0, 3)
    bad = np.random.RandomState(2).standard_normal((9, 9, 9)).astype(np.float32)
    bad[4, 5, 6] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        mesh_ops.vertex_gradients(torch.from_numpy(bad).to(_gpu()), 0.0)


# ---- shading ---------------------------------------------------------------------------------------------------------
def _restate(coef, rows, dirs, K, lobes, dtype):
    """sigmoid(sum_k Y_k(d) coef[r, c K + k]) with every step in `dtype` (torch on the CPU), from the float32 inputs; a negative
    row gives 0.  Returns float64 numpy [n, 3]."""
    c = torch.from_numpy(coef)
    d = torch.from_numpy(dirs).to(dtype)
    r = torch.arange(len(dirs)) if rows is None else torch.from_numpy(rows)
    live = r >= 0
    c = c[r.clamp(min=0)][:, :3 * K].reshape(-1, 3, K).to(dtype)
    if lobes is None:
        Y = O.sh_basis(int(round(K ** 0.5)) - 1, d)
    else:
        L = torch.from_numpy(lobes).to(dtype)
        Y = torch.exp(L[:, 0] * (d @ L[:, 1:].T - 1.0)) / K
    s = (Y[:, None, :] * c).sum(-1)
    out = 1.0 / (1.0 + torch.exp(-s))
    return torch.where(live[:, None], out, torch.zeros_like(out)).double().numpy()


def _unit(rs, n):
    d = rs.standard_normal((n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _lobes(rs, K):
    return np.concatenate([rs.uniform(0.5, 6.0, (K, 1)), _unit(rs, K)], 1).astype(np.float32)


def _held(name, got, want64, floor):
    err = float(np.abs(got.astype(np.float64) - want64).max())
    ratio = err / floor
    _worst[name.split()[0]] = max(_worst.get(name.split()[0], 0.0), ratio)
    print(f"{name}: max |HIP - f64| {err:.3e}, float32 restatement {floor:.3e}, ratio {ratio:.2f} (worst "
          f"{name.split()[0]} so far {_worst[name.split()[0]]:.2f})")
    assert err <= 4 * floor, (name, err, floor)


N_POINTS = (1, 63, 64, 65, 257)


@pytest.mark.parametrize("basis", ["SH", "SG"])
@pytest.mark.parametrize("K", [1, 4, 9, 16, 25])
def test_shade_points_against_the_float64_restatement(K, basis):
    dev = _gpu()
    rs = np.random.RandomState(100 * K + (basis == "SG"))
    n_max, R = max(N_POINTS), 300
    lobes = _lobes(rs, K) if basis == "SG" else None
    dirs = _unit(rs, n_max)
    dirs[5] = (0.0, 0.0, 1.0)                                        # the direction of a vertex without a normal
    leaves = (rs.standard_normal((R, 3 * K + 1)) * 1.5).astype(np.float32)          # a tree's rows: 3 K coefficients, sigma
    leaves[:, -1] = 1e30                                             # read by nobody
    rows = rs.randint(0, R, n_max).astype(np.int64)
    rows[0] = R - 1                                                  # the last row
    rows[[3, 40, 64, 200, 256]] = -1                                 # no leaf: colour 0
    rows[[7, 8, 9, 70]] = rows[6]                                    # repeats
    raw = np.ascontiguousarray(leaves[:n_max, :3 * K])               # a NeRF's raw_rgb: stride 3 K, row i for point i
    d_leaves, d_raw, d_dirs = (torch.from_numpy(a).to(dev) for a in (leaves, raw, dirs))
    d_rows = torch.from_numpy(rows).to(dev)
    d_lobes = None if lobes is None else torch.from_numpy(lobes).to(dev)
    for tag, coef, d_coef, rw, d_rw in (("rows", leaves, d_leaves, rows, d_rows), ("direct", raw, d_raw, None, None)):
        want = _restate(coef, rw, dirs, K, lobes, torch.float64)
        floor = float(np.abs(_restate(coef, rw, dirs, K, lobes, torch.float32) - want).max())
        assert 1e-9 < floor < 1e-5, floor
        for n in N_POINTS:
            got = mesh_ops.shade_points(d_coef if rw is not None else d_coef[:n].contiguous(), d_dirs[:n], K,
                                        rows=None if rw is None else d_rw[:n], lobes=d_lobes)
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3)
            got = got.cpu().numpy()
            if rw is not None:
                dead = rows[:n] < 0
                assert (got[dead] == 0).all() and (got[~dead] > 0).all()
                if n > 70:
                    assert (got[[7, 8, 9]] != got[6]).any() or K == 1    # same row, other directions
            _held(f"{basis}{K} {tag} n={n}", got, want[:n], floor)
    # the same row along the same direction is the same colour, wherever it sits in the launch
    same = mesh_ops.shade_points(d_leaves, d_dirs[:1].repeat(257, 1), K, rows=d_rows[:1].repeat(257), lobes=d_lobes)
    assert bool((same == same[0]).all())


def test_shade_points_refusals():
    dev = _gpu()
    coef, dirs = torch.zeros(10, 13, device=dev), torch.zeros(4, 3, device=dev)
    with pytest.raises(mesh_ops.PxoError, match="basis_dim"):
        mesh_ops.shade_points(coef, dirs, 5)
    with pytest.raises(mesh_ops.PxoError, match="hold no"):
        mesh_ops.shade_points(coef, dirs, 9)
    with pytest.raises(mesh_ops.PxoError, match="outside"):
        mesh_ops.shade_points(coef, dirs, 4, rows=torch.tensor([0, 1, 10, 2], device=dev))
    with pytest.raises(mesh_ops.PxoError, match="coefficient rows"):
        mesh_ops.shade_points(coef[:3].contiguous(), dirs, 4)
    with pytest.raises(mesh_ops.PxoError, match="lobes"):
        mesh_ops.shade_points(coef, dirs, 4, lobes=torch.zeros(3, 4, device=dev))
    out = mesh_ops.shade_points(coef, dirs[:0], 4)                   # nothing to shade: no launch
    assert tuple(out.shape) == (0, 3)
    out = mesh_ops.shade_points(coef, dirs, 4, rows=torch.tensor([0, 9, -1, -7], device=dev))
    assert torch.equal(out, torch.tensor([[0.5] * 3, [0.5] * 3, [0.0] * 3, [0.0] * 3], device=dev))


# ---- octree.meshing --------------------------------------------------------------------------------------------------
AXIS_LOBES = np.array([[2.0, 1, 0, 0], [3.0, 0, 1, 0], [1.5, 0, 0, 1], [4.0, -1, 0, 0]], np.float32)


def _sphere_tree(depth, dev, fmt, seed=0):
    """The sphere tree of test_gpu_mesh.py (sigma 20 inside radius 0.6 on the 2^(depth+1) grid, 0 outside; random float16-
    representable coefficients), in an SH or SG data format."""
    K = int(fmt[2:])
    reso = 2 ** (depth + 1)
    ax = (torch.arange(reso, device=dev, dtype=torch.float32) + 0.5) / reso * 2 - 1
    r = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt()
    mask = r <= 0.6
    tree = svox.N3Tree(N=2, data_dim=3 * K + 1, depth_limit=depth, radius=1.0, center=[0, 0, 0], data_format=fmt,
                       extra_data=AXIS_LOBES[:K] if fmt.startswith("SG") else None,
                       map_location=dev).refine_from_mask(mask.to(torch.uint8).reshape(-1))
    assert tree.max_depth == depth
    gen = torch.Generator().manual_seed(seed)
    data = (torch.randn(tree.n_internal, 2, 2, 2, 3 * K + 1, generator=gen) * 1.5).half().float().to(dev)
    data[..., -1] = 0
    c = (torch.arange(reso, device=dev, dtype=torch.float32) + 0.5) / reso
    pts = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3) * 2 - 1
    leaf = oops.tree_query(tree.child, pts, tree.offset, tree.invradius)
    data.view(-1, 3 * K + 1)[leaf[mask.reshape(-1)], -1] = 20.0
    tree.data.data.copy_(data)
    return tree


@pytest.mark.parametrize("fmt", ["SH4", "SG4"])
def test_octree_meshing_view_colour_and_normals(tmp_path, fmt):
    dev = _gpu()
    K, depth, iso = 4, 6, 10.0
    tree = _sphere_tree(depth - 1, dev, fmt, seed=3)                  # the depth-5 sphere tree: finest grid 64^3
    src = str(tmp_path / "tree.npz")
    tree.save(src)
    plain, out, ply = (str(tmp_path / n) for n in ("plain.obj", "view.obj", "view.ply"))
    v0, f0, c0 = meshing.main(["--input", src, "--output", plain, "--color", "none"])
    verts, faces, rgb = meshing.main(["--input", src, "--output", out, "--color", "view", "--normals"])
    assert c0 is None and np.array_equal(verts, v0) and np.array_equal(faces, f0) and len(verts) > 1000
    assert rgb.dtype == np.float32 and rgb.shape == verts.shape and rgb.std() > 0.05
    # the host definition on the same sampled grid: normals, leaves, directions
    z = np.load(src)
    loaded = svox.N3Tree.load(src, map_location=dev)
    sigma, packed = mesh_ops.tree_sigma_grid(loaded.view(), depth, pad=1, device=dev)
    sig = sigma.cpu().numpy()
    step = 1.0 / ((1 << depth) * z["invradius3"].astype(np.float64))
    nrm = mesh_ops.unit_normals(isosurface.vertex_gradients(sig, iso), step)
    assert np.array_equal(meshing.index_step(depth, z["invradius3"]), step)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, rtol=0, atol=1e-12)
    assert ((nrm * verts).sum(1) > 0).all()                           # out of the ball around the origin
    leaf = packed.cpu().numpy().reshape(-1)[M.inside_index(sig, iso)]
    assert (leaf >= 0).all()
    dirs = mesh_ops.shading_dirs(nrm)
    lobes = z["extra_data"] if fmt.startswith("SG") else None
    assert (lobes is None) == fmt.startswith("SH")
    data = z["data"].astype(np.float32).reshape(-1, 3 * K + 1)
    want = mesh_ops.shade_points(torch.from_numpy(data).to(dev), torch.from_numpy(dirs).to(dev), K,
                                 rows=torch.from_numpy(leaf).to(dev),
                                 lobes=None if lobes is None else torch.from_numpy(lobes).to(dev))
    assert np.array_equal(rgb, want.cpu().numpy())                    # shade_points on the stated leaves, bit for bit
    ref = _restate(data, leaf, dirs, K, lobes, torch.float64)
    _held(f"{fmt} meshing colours", rgb, ref, float(np.abs(_restate(data, leaf, dirs, K, lobes, torch.float32) - ref).max()))
    # the OBJ: v with colours, vn, f a//a
    lines = open(out).read().splitlines()
    nv, nf = len(verts), len(faces)
    assert len(lines) == 2 * nv + nf and all(l.startswith("v ") for l in lines[:nv]) and lines[nv].startswith("vn ")
    assert lines[0] == "v %.4f %.4f %.4f %.4f %.4f %.4f" % (*verts[0], *rgb[0])
    assert lines[nv + 7] == "vn %.4f %.4f %.4f" % tuple(nrm[7])
    a, b, c = faces[-1] + 1
    assert lines[-1] == f"f {a}//{a} {b}//{b} {c}//{c}"
    # the same mesh as PLY
    v2, f2, c2 = meshing.main(["--input", src, "--output", ply, "--color", "view", "--normals"])
    pv, pf, pn, pc = mesh_io.load_ply(ply)
    assert np.array_equal(v2, verts) and np.array_equal(c2, rgb)
    assert np.array_equal(pv, verts.astype(np.float32)) and np.array_equal(pf, faces) and np.array_equal(pn, nrm.astype(np.float32))
    assert np.array_equal(pc, mesh_io.rgb_to_uchar(rgb))
    # without --normals a PLY carries colour only, an OBJ stays the old writer's
    meshing.main(["--input", src, "--output", ply, "--color", "view"])
    _, _, pn, pc = mesh_io.load_ply(ply)
    assert pn is None and np.array_equal(pc, mesh_io.rgb_to_uchar(rgb))
    meshing.main(["--input", src, "--output", out, "--color", "view"])
    ov, oc, of = M.read_obj(out)
    assert np.array_equal(of, faces) and np.abs(oc - rgb).max() <= 0.5e-4 + 1e-7


def test_octree_meshing_view_colour_of_sh1_is_the_dc_colour(tmp_path):
    """One band: Y_0 is the constant both rules multiply by, so the pre-activation is the same float32 number and the two
    sigmoids (torch's, and 1 / (1 + expf(-s)) in the kernel) each sit within a few float32 roundings of its exact value: 8 ulp of
    1 between them at most (expf <= 2 ulp, the sum and the quotient half an ulp each, per path)."""
    dev = _gpu()
    tree = _sphere_tree(4, dev, "SH1", seed=5)
    src, out = str(tmp_path / "tree.npz"), str(tmp_path / "m.obj")
    tree.save(src)
    v1, f1, dc = meshing.main(["--input", src, "--output", out])                       # the default: dc
    v2, f2, view = meshing.main(["--input", src, "--output", out, "--color", "view"])
    assert np.array_equal(v1, v2) and np.array_equal(f1, f2) and len(v1) > 500 and dc.std() > 0.05
    diff = float(np.abs(dc - view).max())
    print(f"SH1 view vs dc: max |difference| {diff:.3e} ({diff / 2.0 ** -24:.2f} ulp of 1)")
    assert diff <= 8 * 2.0 ** -24


# ---- nerf_sh.gen_mesh ------------------------------------------------------------------------------------------------
BOX = ["--reso", "40 36 32", "--c1", "-0.02", "--c2", "0.02", "--point_chunk", "7001"]


def _checkpoint(train_dir, dev, extra=()):
    """A tiny checkpoint without training: the freshly initialised SH9 model, saved the way nerf_sh.train saves."""
    from plenoctree_amd.nerf_sh.nerf import checkpoints, models, utils
    common = ["--train_dir", train_dir, "--sh_deg", "2", "--use_viewdirs", "false", *extra]
    args = gen_mesh.define_flags().parse_args(common)
    utils.update_flags(args)
    model, state = models.get_model_state(args, dev, restore=False)
    checkpoints.save_checkpoint(train_dir, state, 1)
    fn = lambda p: model.eval_points_raw(state, p, want_rgb=False)[1]
    sig = gen_mesh.sigma_grid(fn, [-0.02] * 3, [0.02] * 3, [40, 36, 32], 7001, dev)
    return common, model, state, fn, float(sig.median())


def test_gen_mesh_view_colour_device_and_host_paths_write_the_same_files(tmp_path):
    dev = _gpu()
    d = str(tmp_path)
    common, model, state, fn, iso = _checkpoint(d, dev)
    run = lambda *extra: gen_mesh.main(common + BOX + ["--iso", repr(iso), *extra])
    read = lambda name: open(os.path.join(d, name), "rb").read()
    # the defaults: (verts, faces), and mesh.obj is what save_obj writes for the mesh of the grid -- the file as it was
    verts, faces = run()
    v_ref, f_ref = gen_mesh.marching_cubes(fn, [-0.02] * 3, [0.02] * 3, [40, 36, 32], iso, 7001, dev)
    assert np.array_equal(verts, v_ref) and np.array_equal(faces, f_ref) and len(verts) > 100
    gen_mesh.save_obj(v_ref, f_ref, os.path.join(d, "ref.obj"))
    assert read("mesh.obj") == read("ref.obj")
    plain = read("mesh.obj")
    assert len(run("--color", "none", "--mc", "host")) == 2 and read("mesh.obj") == plain
    # view colour and normals: --mc device and --mc host write identical files, OBJ and PLY
    files = {}
    for mc in ("device", "host"):
        for fmt in ("obj", "ply"):
            v, f, rgb, nrm = run("--color", "view", "--normals", "--format", fmt, "--mc", mc)
            assert np.array_equal(v, verts) and np.array_equal(f, faces)
            files[mc, fmt] = read("mesh." + fmt)
    assert files["device", "obj"] == files["host", "obj"] and files["device", "ply"] == files["host", "ply"]
    assert files["device", "obj"] != plain
    pv, pf, pn, pc = mesh_io.load_ply(os.path.join(d, "mesh.ply"))
    assert np.array_equal(pv, verts.astype(np.float32)) and np.array_equal(pf, faces)
    assert np.array_equal(pn, nrm.astype(np.float32)) and np.array_equal(pc, mesh_io.rgb_to_uchar(rgb))
    # normals: the host definition under the reference's scaling; colours: raw_rgb at the vertices along -n, in float64
    sig = gen_mesh.sigma_grid(fn, [-0.02] * 3, [0.02] * 3, [40, 36, 32], 7001, dev).cpu().numpy()
    step = np.array([0.04] * 3) / np.array([40, 36, 32])
    assert np.array_equal(nrm, mesh_ops.unit_normals(isosurface.vertex_gradients(sig, iso), step))
    raw = model.eval_points_raw(state, torch.from_numpy(verts.astype(np.float32)).to(dev), want_rgb=True)[0].cpu().numpy()
    dirs = mesh_ops.shading_dirs(nrm)
    ref = _restate(raw, None, dirs, 9, None, torch.float64)
    _held("gen_mesh SH9 colours", rgb, ref, float(np.abs(_restate(raw, None, dirs, 9, None, torch.float32) - ref).max()))
    # --color view alone: colours in the OBJ, no vn records, main's four values with None for the normals
    v, f, rgb2, none = run("--color", "view")
    assert none is None and np.array_equal(rgb2, rgb)
    ov, oc, of = M.read_obj(os.path.join(d, "mesh.obj"))
    assert np.array_equal(of, faces) and np.abs(oc - rgb).max() <= 0.5e-4 + 1e-7


def test_gen_mesh_vertex_colours_of_an_sg_model_use_its_lobes(tmp_path):
    dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import sg, utils
    args = gen_mesh.define_flags().parse_args(["--train_dir", str(tmp_path), "--sg_dim", "4", "--sh_deg", "-1", "--use_viewdirs", "false"])
    utils.update_flags(args)
    model, state = sg.get_model_state(args, dev)
    rs = np.random.RandomState(4)
    verts = rs.uniform(-0.5, 0.5, (300, 3))
    nrm = _unit(rs, 300).astype(np.float64)
    nrm[17] = 0.0
    rgb = gen_mesh.vertex_colors(model, state, verts, nrm, 128)       # ragged chunks: 128 + 128 + 44
    raw = model.eval_points_raw(state, torch.from_numpy(verts.astype(np.float32)).to(dev), want_rgb=True)[0].cpu().numpy()
    dirs = mesh_ops.shading_dirs(nrm)
    assert np.array_equal(dirs[17], [0.0, 0.0, 1.0])
    lobes = state.lobes.cpu().numpy()
    ref = _restate(raw, None, dirs, 4, lobes, torch.float64)
    floor = float(np.abs(_restate(raw, None, dirs, 4, lobes, torch.float32) - ref).max())
    _held("gen_mesh SG4 colours", rgb, ref, floor)
    assert np.abs(ref - _restate(raw, None, dirs, 4, None, torch.float64)).max() > 8 * floor     # the SH basis would not pass
