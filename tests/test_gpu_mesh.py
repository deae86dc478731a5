"""Device marching cubes (pxo_mc_count / pxo_mc_emit), the tree-to-grid sampler (pxo_tree_sigma_grid) and the octree.meshing
CLI on the MI355X.  The oracle is the host function nerf_sh/isosurface.py:marching_cubes; every comparison with it is exact
(np.array_equal on float64 vertices, int64 triangles, int64 inside end points): same definition, same output order.

Launch geometry of the implementation (mesh_kernels.hip), which the shapes below straddle: one grid point per lane, z fastest,
BLOCK = 256 points per workgroup (4 waves of 64), SCAN_TILE = 1024 workgroup sums per scan tile."""
import numpy as np
import pytest
import torch

import _mesh_oracle as M
import _octree_cases as C
from _helpers import _gpu
from plenoctree_amd import mesh_ops, octree_ops as oops
from plenoctree_amd.nerf_sh import gen_mesh, isosurface
from plenoctree_amd.octree import meshing, svox

pytestmark = pytest.mark.gpu

BLOCK, SCAN_TILE = 256, 1024
assert (BLOCK, SCAN_TILE) == (mesh_ops.MC_BLOCK, mesh_ops.MC_SCAN_TILE)


def _same_as_host(vol, iso, expect_empty=None):
    """Runs both paths on the float32 array `vol`; every output array must be equal.  Returns the device result."""
    dev = _gpu()
    assert vol.dtype == np.float32
    hv, hf = isosurface.marching_cubes(vol, iso)
    dv, df, di = mesh_ops.marching_cubes(torch.from_numpy(vol).to(dev), iso)
    assert dv.dtype == torch.float64 and df.dtype == torch.int64 and di.dtype == torch.int64
    assert dv.is_cuda and df.is_cuda and di.is_cuda
    assert tuple(dv.shape) == hv.shape and tuple(df.shape) == hf.shape and tuple(di.shape) == (len(hv),)
    assert np.array_equal(dv.cpu().numpy(), hv), "vertices"
    assert np.array_equal(df.cpu().numpy(), hf), "triangles"
    if min(vol.shape) >= 2:
        assert np.array_equal(di.cpu().numpy(), M.inside_index(vol, iso)), "inside_idx"
    if expect_empty is not None:
        assert (len(hv) == 0 and len(hf) == 0) == expect_empty
    return dv, df, di


def _all_cases_pattern():
    """bool [512, 2, 2]: cell 2c (corners x in {2c, 2c+1}) has corner pattern c, corner = dx + 2 dy + 4 dz."""
    pat = np.zeros((512, 2, 2), bool)
    for c in range(256):
        for corner in range(8):
            pat[2 * c + (corner & 1), (corner >> 1) & 1, (corner >> 2) & 1] = (c >> corner) & 1
    return pat


def test_all_256_cases_binary_and_random_magnitudes():
    pat = _all_cases_pattern()
    dv, df, _ = _same_as_host(pat.astype(np.float32), 0.5)
    assert len(df) >= int(isosurface.TRI_COUNT.sum())            # every case's row was emitted (odd cells add more)
    assert np.isin(dv.cpu().numpy() % 1.0, (0.0, 0.5)).all()    # values in {0, 1}: every vertex is an edge midpoint
    rs = np.random.RandomState(0)
    mag = (rs.rand(*pat.shape) * 3.0 + 1e-3).astype(np.float32)
    vol = np.where(pat, np.float32(0.5) + mag, np.float32(0.5) - mag).astype(np.float32)
    assert np.array_equal(vol >= np.float32(0.5), pat)
    _same_as_host(vol, 0.5)


SHAPES = [
    (2, 2, 2), (2, 3, 5), (5, 7, 11),
    (4, 8, 8),                    # 256 points: exactly one workgroup
    (3, 5, 17),                   # 255: one workgroup minus one point
    (2, 3, 43),                   # 258: 257 is prime, no grid with all sides >= 2 has BLOCK + 1 points
    (3, 3, 57),                   # 513 = 2 BLOCK + 1: a last workgroup holding one point
    (3, 4, 63), (3, 4, 64), (3, 4, 65),          # z extent around the wave size
    (65, 64, 66),                 # 1073 workgroups > SCAN_TILE: the second scan tile starts from the first one's sum
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_around_the_launch_geometry(shape):
    n = int(np.prod(shape))
    if shape == (4, 8, 8):
        assert n == BLOCK
    if shape == (65, 64, 66):
        assert -(-n // BLOCK) > SCAN_TILE
    vol = np.random.RandomState(n).standard_normal(shape).astype(np.float32)
    _same_as_host(vol, 0.1, expect_empty=False)


@pytest.mark.parametrize("shape", [(1, 5, 5), (5, 5, 1), (5, 1, 5)])
def test_grids_without_a_cell_give_empty_outputs(shape):
    vol = np.random.RandomState(1).standard_normal(shape).astype(np.float32)
    dv, df, di = _same_as_host(vol, 0.0, expect_empty=True)
    assert tuple(dv.shape) == (0, 3) and tuple(df.shape) == (0, 3) and tuple(di.shape) == (0,)


def test_degenerate_fields():
    _same_as_host(np.zeros((6, 7, 9), np.float32), 1.0, expect_empty=True)           # all below iso
    _same_as_host(np.full((6, 7, 9), 2.0, np.float32), 1.0, expect_empty=True)       # all above
    _same_as_host(np.ones((6, 7, 9), np.float32), 1.0, expect_empty=True)            # all equal to iso: inside
    vol = np.zeros((5, 5, 5), np.float32)
    vol[2, 2, 2] = 1.0                                                               # one point exactly at iso: inside, t = 0
    dv, df, di = _same_as_host(vol, 1.0, expect_empty=False)
    assert len(dv) == 6 and len(df) == 8 and (di == (2 * 5 + 2) * 5 + 2).all()
    assert torch.equal(dv, torch.full((6, 3), 2.0, dtype=torch.float64, device=dv.device))
    # iso = 0.7 (a double) against a grid point holding float32(0.7) < 0.7: the float32 comparison says inside
    vol = np.zeros((4, 4, 4), np.float32)
    vol[1, 2, 1] = np.float32(0.7)
    assert float(vol[1, 2, 1]) < 0.7 and not (vol.astype(np.float64) >= 0.7).any() and (vol >= 0.7).sum() == 1
    dv, df, _ = _same_as_host(vol, 0.7, expect_empty=False)
    assert len(dv) == 6 and len(df) == 8
    vol = np.random.RandomState(2).standard_normal((9, 9, 9)).astype(np.float32)
    vol[4, 5, 6] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        mesh_ops.marching_cubes(torch.from_numpy(vol).to(_gpu()), 0.0)
    with pytest.raises(ValueError, match="non-finite"):
        isosurface.marching_cubes(vol, 0.0)


def test_smooth_field_is_closed_on_the_device():
    n = 48
    ax = np.linspace(-1, 1, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.6 - np.sqrt(x * x + y * y + z * z) + 0.05 * np.sin(7 * x) * np.sin(5 * y + 1) * np.sin(6 * z + 2)).astype(np.float32)
    dv, df, _ = _same_as_host(vol, 0.0, expect_empty=False)
    # every edge is shared by exactly two triangles, counted on the device arrays
    e = torch.cat([df[:, [0, 1]], df[:, [1, 2]], df[:, [2, 0]]], 0)
    key = e.min(1).values * dv.shape[0] + e.max(1).values
    _, uses = torch.unique(key, return_counts=True)
    assert bool((uses == 2).all())
    assert dv.shape[0] - uses.numel() + df.shape[0] == 2          # one closed surface of genus 0
    assert int(df.min()) == 0 and int(df.max()) == dv.shape[0] - 1


# ---- pxo_tree_sigma_grid ---------------------------------------------------------------------------------------------
def _check_sigma_grid(child, data, depths, oracle_depths):
    """child [n,2,2,2] int32 / data [n,2,2,2,D] float32 device tensors of a tree.  Every depth in `depths` is held to
    pxo_tree_query at the cell centres; those in `oracle_depths` also to the numpy descent."""
    dev = child.device
    view = oops.tree_view(child, data, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    flat = data.reshape(-1, data.shape[-1])
    for depth in depths:
        if depth in oracle_depths:
            ws0, wp0 = M.sigma_grid(child.cpu().numpy(), data.cpu().numpy(), depth, 0)
        for pad in (1, 0, 3):
            sigma, packed = mesh_ops.tree_sigma_grid(view, depth, pad=pad, device=dev)
            g = 1 << depth
            assert tuple(sigma.shape) == tuple(packed.shape) == (g + 2 * pad,) * 3
            inner = (slice(pad, pad + g),) * 3
            if pad == 1:
                # tree_query at the cell centres (exact in float32; identity transform, so no rounding enters) plus a gather
                c = (torch.arange(g, device=dev, dtype=torch.float32) + 0.5) / g
                pts = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
                want = oops.tree_query(child, pts, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
                assert torch.equal(packed[inner].reshape(-1), want) and int(want.min()) >= 0
                assert torch.equal(sigma[inner].reshape(-1), flat[want, -1])
                pad_mask = torch.ones_like(packed, dtype=torch.bool)
                pad_mask[inner] = False
                assert bool((sigma[pad_mask] == 0).all()) and bool((packed[pad_mask] == -1).all())
                assert int(pad_mask.sum()) == (g + 2) ** 3 - g ** 3
            if depth in oracle_depths:                    # the numpy descent, padded with 0 / -1
                assert np.array_equal(sigma.cpu().numpy(), np.pad(ws0, pad))
                assert np.array_equal(packed.cpu().numpy(), np.pad(wp0, pad, constant_values=-1))
        # without the packed output
        s2, p2 = mesh_ops.tree_sigma_grid(view, depth, pad=1, want_packed=False, device=dev)
        assert p2 is None and torch.equal(s2, mesh_ops.tree_sigma_grid(view, depth, pad=1, device=dev)[0])


@pytest.mark.parametrize("family,tree_depth", [("shell", 4), ("chunked", 4), ("shell", 6)])
def test_sigma_grid_on_the_small_case_trees(family, tree_depth):
    dev = _gpu()
    t = C.make_tree(family, tree_depth, 1)
    child, data = torch.from_numpy(t.child).to(dev), torch.from_numpy(t.data).to(dev)
    finest = tree_depth + 1
    if tree_depth == 4:       # below, at and above the tree's own finest level
        _check_sigma_grid(child, data, (1, finest - 2, finest, finest + 1), (1, finest - 2, finest, finest + 1))
    else:
        _check_sigma_grid(child, data, (finest - 1, finest), (finest - 1,))


def _sphere_tree(depth, dev, K=1, radius_vox=None, seed=0):
    """N3Tree refined from a sphere mask on its 2^(depth+1) grid (centre 0, radius 1: world = 2 t - 1): sigma 20 in the masked
    finest cells and 0 elsewhere, random SH coefficients (float16-representable, so a saved file holds them exactly)."""
    reso = 2 ** (depth + 1)
    ax = (torch.arange(reso, device=dev, dtype=torch.float32) + 0.5) / reso * 2 - 1
    r = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt()
    mask = r <= 0.6
    tree = svox.N3Tree(N=2, data_dim=3 * K + 1, depth_limit=depth, radius=1.0, center=[0, 0, 0], data_format=f"SH{K}",
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
    return tree, mask


@pytest.mark.parametrize("depth", [4, 5])
def test_sigma_grid_on_a_tree_refined_from_a_sphere_mask(depth):
    dev = _gpu()
    tree, mask = _sphere_tree(depth, dev)
    finest = depth + 1                                   # the tree's finest grid: 2^finest cells per axis
    _check_sigma_grid(tree.child, tree.data.data, (finest - 1, finest, finest + 1), (finest - 1, finest))
    sigma, _ = mesh_ops.tree_sigma_grid(tree.view(), finest, pad=0, device=dev)
    assert torch.equal(sigma, torch.where(mask, 20.0, 0.0).float())


# ---- the CLI ---------------------------------------------------------------------------------------------------------
def test_octree_meshing_end_to_end(tmp_path):
    dev = _gpu()
    K, depth = 4, 6
    tree, _ = _sphere_tree(depth - 1, dev, K=K, seed=3)      # the depth-5 sphere tree: finest grid 64^3
    src, out = str(tmp_path / "tree.npz"), str(tmp_path / "tree_mesh.obj")
    tree.save(src)
    verts, faces, rgb = meshing.main(["--input", src, "--output", out, "--iso", "10.0"])
    pv, pc, pf = M.read_obj(out)                                                   # the OBJ parses
    assert len(pv) == len(verts) > 1000 and pc is not None and np.array_equal(pf, faces)
    assert np.abs(pv - verts).max() <= 0.5e-4 + 1e-12 and np.abs(pc - rgb).max() <= 0.5e-4 + 1e-7     # "%.4f"
    _, uses = M.edge_use(faces)
    assert (uses == 2).all() and len(verts) - uses.size + len(faces) == 2         # closed, Euler characteristic 2
    h = 2.0 / (1 << depth)                                                         # one finest cell in world units
    assert np.abs(np.linalg.norm(verts, axis=1) - 0.6).max() < h
    # host path on the same sampled grid
    z = np.load(src)
    loaded = svox.N3Tree.load(src, map_location=dev)
    sigma, packed = mesh_ops.tree_sigma_grid(loaded.view(), depth, pad=1, device=dev)
    hv, hf = isosurface.marching_cubes(sigma.cpu().numpy(), 10.0)
    assert np.array_equal(faces, hf)
    assert np.array_equal(verts, meshing.index_to_world(hv, depth, z["offset"], z["invradius3"]))
    # colours: the DC rule at the inside end point's leaf, float32, from the values the file holds
    leaf = packed.cpu().numpy().reshape(-1)[M.inside_index(sigma.cpu().numpy(), 10.0)]
    assert (leaf >= 0).all()
    dc = z["data"].astype(np.float32).reshape(-1, 3 * K + 1)[leaf][:, [0, K, 2 * K]]
    want = torch.sigmoid(torch.from_numpy(dc).to(dev) * np.float32(meshing.SH_C0)).cpu().numpy()
    assert rgb.dtype == np.float32 and np.array_equal(rgb, want)
    assert np.abs(rgb - 1.0 / (1.0 + np.exp(-0.28209479177387814 * dc.astype(np.float64)))).max() < 1e-6
    assert rgb.std() > 0.05                                                       # the leaves do differ in colour
    # --color none, a coarser --depth: still closed, no colours in the file
    out2 = str(tmp_path / "coarse.obj")
    v2, f2, c2 = meshing.main(["--input", src, "--output", out2, "--iso", "10", "--depth", str(depth - 1), "--color", "none"])
    pv2, pc2, pf2 = M.read_obj(out2)
    assert c2 is None and pc2 is None and len(pv2) == len(v2) > 100 and np.array_equal(pf2, f2)
    _, uses2 = M.edge_use(f2)
    assert (uses2 == 2).all() and np.abs(np.linalg.norm(v2, axis=1) - 0.6).max() < 2 * h


def test_gen_mesh_device_and_host_paths_agree(tmp_path):
    dev = _gpu()
    c1, c2, reso = [-2.0, -1.0, -1.5], [2.0, 1.0, 1.5], [37, 29, 23]
    field = lambda p: (1.0 - p.norm(dim=-1, keepdim=True)) * 3.0 + 0.2 * torch.sin(5.0 * p[:, :1])
    vd, fd = gen_mesh.marching_cubes(field, c1, c2, reso, 0.25, 5000, dev, mc="device")
    vh, fh = gen_mesh.marching_cubes(field, c1, c2, reso, 0.25, 5000, dev, mc="host")
    assert len(fd) > 500 and np.array_equal(vd, vh) and np.array_equal(fd, fh) and vd.dtype == np.float64
    a, b = str(tmp_path / "device.obj"), str(tmp_path / "host.obj")
    gen_mesh.save_obj(vd, fd, a)
    gen_mesh.save_obj(vh, fh, b)
    assert open(a, "rb").read() == open(b, "rb").read()
