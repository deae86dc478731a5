"""Host side of mesh normals and view-dependent colour (no GPU): the definition isosurface.vertex_gradients that
pxo_mc_vertex_gradients is held to, the unit normal and the shading direction made from it, the PLY / OBJ writers of mesh_io, the
new flags of octree.meshing and nerf_sh.gen_mesh beside their unchanged defaults and refusals, and the argument checks of the
two new entry points that return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import _mesh_oracle as M
from plenoctree_amd import _lib, build, mesh_io, mesh_ops
from plenoctree_amd.nerf_sh import gen_mesh, isosurface
from plenoctree_amd.octree import meshing


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def _edges(vol, iso):
    """(axis, lower end point [3]) of every vertex of isosurface.marching_cubes, in its order, written out independently."""
    inside = vol >= iso
    out = []
    for a in range(3):
        lo = tuple(slice(0, -1) if d == a else slice(None) for d in range(3))
        hi = tuple(slice(1, None) if d == a else slice(None) for d in range(3))
        out += [(a, p) for p in np.argwhere(inside[lo] != inside[hi])]
    return out


def _gradient_loop(vol, iso):
    """The definition of the issue, vertex by vertex in Python floats (IEEE doubles, one rounding per operation)."""
    def g(p, b):
        q, r = list(p), list(p)
        q[b] += 1
        r[b] -= 1
        if 0 < p[b] < vol.shape[b] - 1:
            return (float(vol[tuple(q)]) - float(vol[tuple(r)])) * 0.5
        if p[b] == 0:
            return float(vol[tuple(q)]) - float(vol[tuple(p)])
        return float(vol[tuple(p)]) - float(vol[tuple(r)])
    out = []
    for a, lo in _edges(vol, iso):
        hi = lo.copy()
        hi[a] += 1
        v0, v1 = float(vol[tuple(lo)]), float(vol[tuple(hi)])
        f = (iso - v0) / (v1 - v0)
        out.append([(1.0 - f) * g(lo, b) + f * g(hi, b) for b in range(3)])
    return np.asarray(out, np.float64).reshape(-1, 3)


def test_vertex_gradients_follow_the_vertex_order_of_marching_cubes():
    vol = np.random.RandomState(5 * 7 * 11).standard_normal((5, 7, 11)).astype(np.float32)
    v, _ = isosurface.marching_cubes(vol, 0.1)
    g = isosurface.vertex_gradients(vol, 0.1)
    assert g.dtype == np.float64 and g.shape == v.shape and len(v) > 100
    edges = _edges(vol, 0.1)
    assert len(edges) == len(v)
    for (a, lo), p in zip(edges, v):                  # the independent edge list is marching_cubes' vertex list
        others = [d for d in range(3) if d != a]
        assert np.array_equal(p[others], lo[others]) and lo[a] - 1e-6 <= p[a] <= lo[a] + 1 + 1e-6
    assert np.array_equal(g, _gradient_loop(vol, 0.1))
    # grids without a cell, and non-finite volumes, as marching_cubes treats them
    assert isosurface.vertex_gradients(np.zeros((1, 4, 4), np.float32), 0.5).shape == (0, 3)
    assert isosurface.vertex_gradients(np.zeros((4, 4, 4), np.float32), 0.5).shape == (0, 3)
    bad = vol.copy()
    bad[1, 2, 3] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        isosurface.vertex_gradients(bad, 0.1)
    with pytest.raises(ValueError, match="3-D"):
        isosurface.vertex_gradients(vol[0], 0.1)


def test_linear_field_gives_its_coefficients_exactly_borders_included():
    """a, b, c are powers of two and the samples small dyadic numbers, so every difference is exact and each product with a
    coefficient is a scaling; what is left is fl(fl(1 - f) + f), which is 1 for every f in [0, 1]: fl(1 - f) is off by at most
    2^-54, below half the spacing of doubles next to 1."""
    a, b, c = 2.0, -0.5, 4.0
    x, y, z = np.meshgrid(np.arange(5), np.arange(7), np.arange(11), indexing="ij")
    vol = (a * x + b * y + c * z).astype(np.float32)
    g = isosurface.vertex_gradients(vol, 7.3)
    v, _ = isosurface.marching_cubes(vol, 7.3)
    assert len(g) == len(v) > 40 and np.array_equal(g, np.broadcast_to([a, b, c], g.shape))
    on_border = ((v == 0) | (v == np.array(vol.shape) - 1)).any(1)
    assert on_border.sum() > 10 and (~on_border).sum() > 10          # both kinds of grid-point gradient were exercised
    # the smallest grid: every point is a border point along every axis
    g2 = isosurface.vertex_gradients(vol[:2, :2, :2].copy(), 1.0)
    assert len(g2) > 0 and np.array_equal(g2, np.broadcast_to([a, b, c], g2.shape))
    # general coefficients: to rounding
    vol = (3.0 * x - 0.7 * y + 1.3 * z).astype(np.float32)
    g = isosurface.vertex_gradients(vol, 7.3)
    assert np.abs(g - [3.0, -0.7, 1.3]).max() < 2e-6                 # float32 samples of magnitude <= 20: 1 ulp ~ 1e-6


def _sphere_field(n=48):
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (0.6 - np.sqrt(x * x + y * y + z * z) + 0.05 * np.sin(7 * x) * np.sin(5 * y + 1) * np.sin(6 * z + 2)).astype(np.float32)


def test_normals_point_out_of_the_smooth_sphere_field():
    n = 48
    vol = _sphere_field(n)                                            # the field of test_gpu_mesh.py
    v, _ = isosurface.marching_cubes(vol, 0.0)
    nrm = mesh_ops.unit_normals(isosurface.vertex_gradients(vol, 0.0), [2.0 / (n - 1)] * 3)
    radial = v / (n - 1) * 2 - 1
    assert len(v) > 3000 and nrm.dtype == np.float64
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, rtol=0, atol=1e-12)
    cos = (nrm * radial).sum(1) / np.linalg.norm(radial, axis=1)
    assert (cos > 0).all()
    # anisotropic steps rescale the gradient per axis before the normalisation
    g = np.array([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    got = mesh_ops.unit_normals(g, [1.0, 0.5, 4.0])
    want = np.array([[-1.0, -2.0, 0.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    want[0] /= np.sqrt(5.0)
    assert np.allclose(got, want, rtol=0, atol=1e-15) and np.array_equal(got[1], [0.0, 0.0, 0.0])
    assert torch.equal(mesh_ops.unit_normals(torch.from_numpy(g), [1.0, 0.5, 4.0]), torch.from_numpy(got))
    d = mesh_ops.shading_dirs(got)
    assert d.dtype == np.float32 and np.array_equal(d[1], [0.0, 0.0, 1.0]) and np.array_equal(d[[0, 2]], (-got[[0, 2]]).astype(np.float32))
    assert torch.equal(mesh_ops.shading_dirs(torch.from_numpy(got)), torch.from_numpy(d))


def test_single_point_at_iso_gives_six_equal_gradients():
    vol = np.zeros((5, 5, 5), np.float32)
    vol[2, 2, 2] = 1.0
    g = isosurface.vertex_gradients(vol, 1.0)
    # f = 1 on the three edges below the point and 0 on the three above: every vertex takes g(2,2,2), a central difference of
    # equal neighbours, and 0 * (the finite gradient of the other end)
    assert g.shape == (6, 3) and (g == g[0]).all() and np.array_equal(g[0], [0.0, 0.0, 0.0])
    assert np.array_equal(mesh_ops.unit_normals(g, [1.0] * 3), np.zeros((6, 3)))


# ---- writers ---------------------------------------------------------------------------------------------------------
def _mesh():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [0.0, 1.0, -2.5], [0.12345, 7.0, 1e-3]])
    f = np.array([[0, 1, 2], [2, 1, 3]])
    n = np.array([[0.0, 0.0, 1.0], [0.6, 0.0, 0.8], [0.0, -1.0, 0.0], [0.0, 0.0, 0.0]])
    c = np.array([[0.0, 1.0, 0.5], [0.498, 0.4981, 0.002], [1.0 / 255, 1.49 / 255, 1.51 / 255], [0.25, 0.75, 0.999]])
    return v, f, n, c


@pytest.mark.parametrize("with_n,with_c", [(False, False), (True, False), (False, True), (True, True)])
def test_ply_round_trip(tmp_path, with_n, with_c):
    v, f, n, c = _mesh()
    path = str(tmp_path / "m.ply")
    mesh_io.save_ply(v, f, path, normals=n if with_n else None, vert_rgb=c if with_c else None)
    blob = open(path, "rb").read()
    head, _, body = blob.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    props = ["property float x", "property float y", "property float z"]
    props += ["property float nx", "property float ny", "property float nz"] if with_n else []
    props += ["property uchar red", "property uchar green", "property uchar blue"] if with_c else []
    assert lines == ["ply", "format binary_little_endian 1.0", "element vertex 4"] + props + \
        ["element face 2", "property list uchar int vertex_indices"]
    assert len(body) == 4 * (12 + 12 * with_n + 3 * with_c) + 2 * (1 + 12)
    pv, pf, pn, pc = mesh_io.load_ply(path)
    assert pv.dtype == np.float32 and np.array_equal(pv, v.astype(np.float32)) and np.array_equal(pf, f)
    assert (pn is None) == (not with_n) and (pc is None) == (not with_c)
    if with_n:
        assert np.array_equal(pn, n.astype(np.float32))
    if with_c:                                                        # round(255 c), halves to even like np.rint
        assert pc.dtype == np.uint8
        assert np.array_equal(pc, [[0, 255, 128], [127, 127, 1], [1, 1, 2], [64, 191, 255]])
    # the face records as bytes: count 3, then three little-endian int32
    assert body[-26:] == b"\x03" + np.array([0, 1, 2], "<i4").tobytes() + b"\x03" + np.array([2, 1, 3], "<i4").tobytes()


def test_writers_refuse_mismatched_arrays_and_clip_colours(tmp_path):
    v, f, n, c = _mesh()
    path = str(tmp_path / "m.ply")
    with pytest.raises(ValueError, match="normals"):
        mesh_io.save_ply(v, f, path, normals=n[:3])
    with pytest.raises(ValueError, match="vert_rgb"):
        mesh_io.save_obj_normals(v, f, path, n, vert_rgb=c[:, :2])
    with pytest.raises(ValueError, match="indices"):
        mesh_io.save_ply(v, f + 2, path)
    assert np.array_equal(mesh_io.rgb_to_uchar([[-0.5, 1.5, 0.5]]), [[0, 255, 128]])
    mesh_io.save_ply(v[:0], f[:0], path, normals=n[:0], vert_rgb=c[:0])            # an empty mesh is a header
    pv, pf, pn, pc = mesh_io.load_ply(path)
    assert pv.shape == (0, 3) and pf.shape == (0, 3) and pn.shape == (0, 3) and pc.shape == (0, 3)


def test_obj_with_normals_and_save_mesh_dispatch(tmp_path):
    v, f, n, c = _mesh()
    path = str(tmp_path / "m.obj")
    mesh_io.save_obj_normals(v, f, path, n)
    lines = open(path).read().splitlines()
    assert lines[:4] == ["v %.4f %.4f %.4f" % tuple(p) for p in v] and lines[3] == "v 0.1235 7.0000 0.0010"
    assert lines[4:8] == ["vn 0.0000 0.0000 1.0000", "vn 0.6000 0.0000 0.8000", "vn 0.0000 -1.0000 0.0000", "vn 0.0000 0.0000 0.0000"]
    assert lines[8:] == ["f 1//1 2//2 3//3", "f 3//3 2//2 4//4"]
    mesh_io.save_obj_normals(v, f, path, n, vert_rgb=c)
    assert open(path).read().splitlines()[0] == "v 0.0000 0.0000 0.0000 0.0000 1.0000 0.5000"
    # save_mesh: without normals an OBJ is gen_mesh.save_obj's file, byte for byte; .ply or fmt="ply" selects PLY
    a, b = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
    for rgb in (None, c):
        mesh_io.save_mesh(v, f, a, vert_rgb=rgb)
        gen_mesh.save_obj(v, f, b, vert_rgb=rgb)
        assert open(a, "rb").read() == open(b, "rb").read()
        pv, pc, pf = M.read_obj(a)
        assert np.array_equal(pf, f) and (pc is None) == (rgb is None)
    mesh_io.save_mesh(v, f, a, normals=n)
    assert open(a).read().splitlines()[4].startswith("vn ")
    p1, p2 = str(tmp_path / "x.PLY"), str(tmp_path / "y.bin")
    mesh_io.save_mesh(v, f, p1, normals=n)
    mesh_io.save_mesh(v, f, p2, normals=n, fmt="ply")
    assert open(p1, "rb").read() == open(p2, "rb").read() and open(p1, "rb").read(4) == b"ply\n"


# ---- flags -----------------------------------------------------------------------------------------------------------
def _save_tree(path, fmt):
    from plenoctree_amd.octree.svox import N3Tree
    K = int(fmt[2:])
    extra = None
    if fmt.startswith("SG"):
        extra = np.concatenate([np.full((K, 1), 2.0), np.eye(3)[np.arange(K) % 3]], 1).astype(np.float32)
    N3Tree(N=2, data_dim=3 * K + 1, depth_limit=3, radius=1.0, center=[0, 0, 0], data_format=fmt, extra_data=extra).save(path)


def test_meshing_flags_defaults_and_the_sg_dc_refusal(tmp_path):
    sh, sg, out = str(tmp_path / "sh.npz"), str(tmp_path / "sg.npz"), str(tmp_path / "m.ply")
    _save_tree(sh, "SH4")
    _save_tree(sg, "SG4")
    flags = meshing.define_flags()
    args = flags.parse_args(["-i", sh, "-o", out])
    assert args.color is None and args.normals is False and args.iso == 10.0 and args.depth is None
    args = flags.parse_args(["-i", sg, "-o", out, "--color", "view", "--normals"])
    assert args.color == "view" and args.normals is True and meshing.check_args(args) == "SG4"
    args = flags.parse_args(["-i", sh, "-o", out, "--color", "view"])
    assert meshing.check_args(args) == "SH4"
    with pytest.raises(SystemExit):
        flags.parse_args(["-i", sh, "-o", out, "--color", "rainbow"])
    with pytest.raises(SystemExit, match=r"--color dc on an SG tree \(SG4\): a spherical-Gaussian tree has no view-independent "
                                         r"\(DC\) band; mesh it with --color none"):
        meshing.main(["--input", sg, "--output", out, "--color", "dc"])
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a ROCm GPU"):
            meshing.main(["--input", sg, "--output", out, "--color", "view", "--normals"])
    assert not (tmp_path / "m.ply").exists()
    assert np.array_equal(meshing.index_step(3, np.array([0.5, 0.25, 1.0], np.float32)), [0.25, 0.5, 0.125])


def test_gen_mesh_flags_and_host_normals():
    flags = gen_mesh.define_flags()
    args = flags.parse_args([])
    assert (args.color, args.normals, args.format, args.mc) == ("none", False, "obj", "device")
    args = flags.parse_args(["--color", "view", "--normals", "--format", "ply"])
    assert (args.color, args.normals, args.format) == ("view", True, "ply")
    for bad in (["--color", "dc"], ["--format", "stl"]):
        with pytest.raises(SystemExit):
            flags.parse_args(bad)
    # marching_cubes(normals=True) on a CPU grid: the host gradients, scaled by the reference's (c2 - c1) / reso
    c1, c2, reso = [-2.0, -1.0, -1.5], [2.0, 1.0, 1.5], [21, 17, 13]
    field = lambda p: (1.0 - p.norm(dim=-1, keepdim=True)) * 3.0
    cpu = torch.device("cpu")
    v0, f0 = gen_mesh.marching_cubes(field, c1, c2, reso, 0.25, 1000, cpu)
    v, f, n = gen_mesh.marching_cubes(field, c1, c2, reso, 0.25, 1000, cpu, normals=True)
    assert np.array_equal(v, v0) and np.array_equal(f, f0) and n.shape == v.shape and n.dtype == np.float64
    sig = gen_mesh.sigma_grid(field, c1, c2, reso, 1000, cpu).numpy()
    step = (np.array(c2) - np.array(c1)) / np.array(reso)
    assert np.array_equal(n, mesh_ops.unit_normals(isosurface.vertex_gradients(sig, 0.25), step))
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, rtol=0, atol=1e-12)
    # the field falls with the distance from the origin of the *sample* space; there the normals are radial to O(h^2)
    idx = (v - np.array(c1)) / step
    pos = np.array(c1) + idx * (np.array(c2) - np.array(c1)) / (np.array(reso) - 1)
    # a world normal is the gradient in the reference's (shrunk) vertex space: J^-T of the sample-space one, J = reso/(reso-1)
    radial = pos * (np.array(reso) / (np.array(reso) - 1.0))
    cos = (n * radial).sum(1) / np.linalg.norm(radial, axis=1)
    assert cos.min() > 0.97


# ---- the entry points' refusals, before any launch -------------------------------------------------------------------
def test_new_entry_points_refuse_what_emit_refuses(lib):
    counts = (ctypes.c_int64 * 4)()
    fn = lib.pxo_mc_vertex_gradients
    assert fn(None, 2048, 2048, 512, 1.0, None, 0, counts, None, None, None) == -1 and b"2^31" in lib.pxo_last_error()
    assert fn(None, -1, 4, 4, 1.0, None, 0, counts, None, None, None) == -1
    assert fn(None, 8, 8, 8, 1.0, None, 0, None, None, None, None) == -1
    counts[:] = [2 ** 30, 2 ** 30, 0, 5]
    assert fn(None, 8, 8, 8, 1.0, None, 0, counts, None, None, None) == -1 and b"vertices" in lib.pxo_last_error()
    counts[:] = [3, 3, 3, 2 ** 31]
    assert fn(None, 8, 8, 8, 1.0, None, 0, counts, None, None, None) == -1 and b"triangles" in lib.pxo_last_error()
    counts[:] = [-1, 0, 0, 0]
    assert fn(None, 8, 8, 8, 1.0, None, 0, counts, None, None, None) == -1
    counts[:] = [3, 3, 3, 4]
    assert fn(None, 8, 8, 8, 1.0, None, 0, counts, None, None, None) == -1 and b"null" in lib.pxo_last_error()
    # nothing to do: no launch, on a machine without a GPU too
    counts[:] = [0, 0, 0, 0]
    assert fn(None, 8, 8, 8, 1.0, None, 0, counts, None, None, None) == 0
    counts[:] = [9, 9, 9, 9]
    assert fn(None, 1, 5, 5, 1.0, None, 0, counts, None, None, None) == 0
    # a workspace that is too small for the grid (host pointers are never dereferenced: the check comes first)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    counts[:] = [1, 1, 1, 1]
    assert fn(p, 8, 8, 8, 1.0, p, 64, counts, p, p, None) != 0 and b"workspace" in lib.pxo_last_error()

    sh = lib.pxo_shade_points
    for k in (0, 2, 3, 5, 8, 10, 24, 26, 36, -1):
        assert sh(None, 3 * max(k, 1), None, None, 0, k, None, None, None) == -1 and b"basis_dim" in lib.pxo_last_error()
    assert sh(None, 11, None, None, 0, 4, None, None, None) == -1 and b"row_stride" in lib.pxo_last_error()
    assert sh(None, 12, None, None, -1, 4, None, None, None) == -1
    assert sh(None, 12, None, None, 2 ** 31, 4, None, None, None) == -1
    assert sh(None, 12, None, None, 5, 4, None, None, None) == -1 and b"null" in lib.pxo_last_error()
    for k in (1, 4, 9, 16, 25):
        assert sh(None, 3 * k, None, None, 0, k, None, None, None) == 0
        assert sh(None, 3 * k + 1, None, None, 0, k, None, None, None) == 0
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PxoError):
            mesh_ops.vertex_gradients(torch.zeros(4, 4, 4), 0.5)
        with pytest.raises(_lib.PxoError):
            mesh_ops.shade_points(torch.zeros(4, 12), torch.zeros(4, 3), 4)
