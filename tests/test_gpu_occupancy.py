"""The occupancy-grid entry points on the MI355X, through the C ABI, each against its numpy restatement (tests/_occupancy_ref.py)
bit for bit: pxo_occ_pack, pxo_occ_cull, pxo_occ_expand, and pxo_render_fwd_culled against pxo_render_fwd (every sample live) and
against a twin composed from the per-stage entry points (a real mask)."""
import os

import numpy as np
import pytest
import torch

import _occupancy_ref as R
from _helpers import _gpu, _ops, make_params, make_rays, pxo_cfg, split_mlp
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

BLOCK = 256                                       # points per workgroup of the cull (occupancy_kernels.hip kOccBlock)
M_SET = (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17)
M_TILES = 1024 * BLOCK + 300                      # more than one scan tile of 1024 block counts
# the box [-2, 2)^3 in 4 cells per axis: scale a power of two, offset 0.5 -- t = p / 4 + 1/2 is exact for the points below
RESO, OFFSET, SCALE = 4, [0.5] * 3, [0.25] * 3
CELL_A, CELL_B = (2, 1, 3), (0, 0, 0)             # a cell every test grid sets / leaves empty


def _grid(ops, dev, mask, outside_live, reso=RESO, offset=OFFSET, scale=SCALE):
    bits = torch.from_numpy(R.bits_from_mask(mask)).to(dev)
    return ops.OccupancyGrid(bits, reso, offset, scale, outside_live=bool(outside_live))


# ---- pack -----------------------------------------------------------------------------------------------------------------------
def _pack_case(reso, seed):
    rs = np.random.RandomState(seed)
    s = np.zeros((reso, reso, reso), np.float32)
    s[rs.rand(reso, reso, reso) < 0.03] = 2.0
    s[rs.rand(reso, reso, reso) < 0.05] = 1.0                    # exactly the threshold: not occupied (strict >)
    s[rs.rand(reso, reso, reso) < 0.05] = 0.999
    h, e = reso // 2, reso - 1
    for c in ((0, 0, 0), (e, e, e), (0, e, 0), (0, 0, h), (e, h, e), (0, h, h), (h, e, h), (h, h, 0)):    # corners, edges, faces
        s[c] = 2.0
    s[h, 1, h] = 1.0
    s[1, h, 1] = np.nan
    return s


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("reso", [5, 32, 33])
def test_pack(reso, dilate):
    dev, ops = _gpu(), _ops()
    s = _pack_case(reso, reso)
    want = R.pack(s, reso, 1.0, dilate)
    bits = torch.full((R.words(reso),), -1, dtype=torch.int32, device=dev)          # every word must be written
    got = ops.occ_pack(torch.from_numpy(s.reshape(-1)).to(dev), reso, 1.0, dilate, bits=bits).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    tail = reso ** 3 % 32
    if tail:                                                      # reso 5: 125 bits, 29 in the last word
        assert int(got.view(np.uint32)[-1]) >> tail == 0
    m = R.mask_from_bits(got, reso).reshape(reso, reso, reso)
    if not dilate:
        assert m[1, reso // 2, 1] and not m[reso // 2, 1, reso // 2]             # the NaN cell is occupied, the == thresh cell is not
    g = ops.OccupancyGrid(torch.from_numpy(got).to(dev), reso, OFFSET, SCALE)
    assert g.count_occupied() == int(m.sum())


# ---- cull -----------------------------------------------------------------------------------------------------------------------
def _points_in(cells, rs):
    """One point per row of `cells` [M,3]: t = (cell + f) / 4 with f in {1/8 .. 7/8} -- exact in float32 and at least 1/8 of a cell
    away from every boundary."""
    f = rs.randint(1, 8, size=cells.shape) / 8.0
    t = (cells + f) / RESO
    return ((t - 0.5) * 4.0).astype(np.float32)


SPECIAL = np.array([[0.0, -1.0, 1.0],             # exactly on the lower boundaries of CELL_A: belongs to it
                    [1.0, -0.5, 1.5],             # exactly on its upper x boundary: cell (3,1,3)
                    [-2.0, -2.0, -2.0],           # t = 0 on all axes: inside, CELL_B
                    [0.5, -0.5, 2.0],             # t_z = 1: outside
                    [2.0, 2.0, 2.0],              # t = 1 on all axes
                    [-2.5, 0.5, 0.5],             # outside
                    [0.5, 7.0, 0.5],
                    [np.nan, 0.5, 0.5],
                    [0.5, -0.5, np.inf]], np.float32)


def _cull_case(pattern, M, seed):
    """(mask [4,4,4], outside_live, pts [M,3])."""
    rs = np.random.RandomState(seed)
    mask = rs.rand(RESO, RESO, RESO) < 0.4
    mask[CELL_A], mask[CELL_B] = True, False
    a, b = np.array(CELL_A), np.array(CELL_B)
    m = np.arange(M)
    outside_live = 0
    if pattern == "all_live":
        mask[:] = True
        outside_live = 1
        cells = rs.randint(0, RESO, size=(M, 3))
    elif pattern == "all_empty":
        mask[:] = False
        cells = rs.randint(0, RESO, size=(M, 3))
    elif pattern == "alternating":
        cells = np.where((m % 2 == 0)[:, None], a, b)
    elif pattern == "last_block":
        cells = np.where((m >= (max(M - 1, 0) // BLOCK) * BLOCK)[:, None], a, b)
    else:                                                         # "mixed_outside0" / "mixed_outside1"
        outside_live = int(pattern[-1])
        cells = rs.randint(0, RESO, size=(M, 3))
    pts = _points_in(cells, rs)
    if pattern.startswith("mixed"):
        n = min(len(SPECIAL), M)
        where = rs.permutation(M)[:n]                             # boundary, outside and non-finite points among the others
        pts[where] = SPECIAL[:n]
    return mask, outside_live, pts


PATTERNS = ("all_live", "all_empty", "alternating", "last_block", "mixed_outside0", "mixed_outside1")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("M", M_SET + (M_TILES,))
def test_cull(M, pattern):
    dev, ops = _gpu(), _ops()
    mask, outside_live, pts = _cull_case(pattern, M, 11 * M + len(pattern))
    bits = R.bits_from_mask(mask)
    want_live, want_slot, want_n = R.cull(bits, RESO, OFFSET, SCALE, outside_live, pts)
    if pattern == "all_live":
        assert want_n == M
    if pattern == "all_empty":
        assert want_n == 0
    g = _grid(ops, dev, mask, outside_live)
    live, slot, n = ops.occ_cull(g, torch.from_numpy(pts).to(dev))
    assert int(n.item()) == want_n
    assert slot.dtype == torch.int32 and np.array_equal(slot.cpu().numpy(), want_slot)
    got = live.cpu().numpy()[:want_n]
    assert np.array_equal(got.view(np.uint32), want_live.view(np.uint32))           # bit for bit, NaN rows included
    # deterministic: a second call gives the same arrays
    live2, slot2, n2 = ops.occ_cull(g, torch.from_numpy(pts).to(dev))
    assert torch.equal(slot, slot2) and torch.equal(n, n2)


def test_cull_special_points_are_all_present():
    """The mixed patterns at 3 blocks + 17 hold every boundary, outside and non-finite point (both treatments of the outside)."""
    for pattern in ("mixed_outside0", "mixed_outside1"):
        _, _, pts = _cull_case(pattern, 3 * BLOCK + 17, 11 * (3 * BLOCK + 17) + len(pattern))
        for sp in SPECIAL:
            assert (pts.view(np.uint32) == sp.view(np.uint32)).all(axis=1).any(), sp


def test_cull_across_the_tile_scan_loop():
    """More than 64 scan tiles (64 x 1024 blocks): the single wave that scans the tile sums carries from one round of 64 to the
    next.  The pattern (two live points in three) and its expected slots are made on the device."""
    dev, ops = _gpu(), _ops()
    M = 64 * 1024 * BLOCK + 3 * BLOCK + 5
    mask = np.zeros((RESO, RESO, RESO), bool)
    mask[CELL_A] = True
    m = torch.arange(M, device=dev)
    live = m % 3 != 0
    pa = torch.tensor([0.5, -0.5, 1.5], device=dev)              # the centre of CELL_A
    pb = torch.tensor([-1.5, -1.5, -1.5], device=dev)            # the centre of CELL_B
    pts = torch.where(live[:, None], pa, pb).contiguous()
    got_live, slot, n = ops.occ_cull(_grid(ops, dev, mask, 0), pts)
    want_n = int(live.sum())
    assert int(n.item()) == want_n
    want_slot = torch.where(live, torch.cumsum(live.to(torch.int32), 0, dtype=torch.int32) - 1, torch.full_like(m, -1, dtype=torch.int32))
    assert torch.equal(slot, want_slot)
    assert torch.equal(got_live[:want_n], pa.expand(want_n, 3))


# ---- expand ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 75, 5])             # 5: a width that is no SH head's, the kernel's general form
@pytest.mark.parametrize("M", M_SET)
def test_expand(M, C):
    dev, ops = _gpu(), _ops()
    rs = np.random.RandomState(7 * M + C)
    live = rs.rand(M) < 0.5
    if M > BLOCK:
        live[:BLOCK] = False                                      # a whole block of culled rows
    slot = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    n = int(live.sum())
    rgb_live = rs.randn(max(n, 1), C).astype(np.float32)
    sigma_live = rs.randn(max(n, 1)).astype(np.float32)
    want_rgb, want_sigma = R.expand(rgb_live[:n], sigma_live[:n], slot, C)
    rgb, sigma = ops.occ_expand(torch.from_numpy(rgb_live).to(dev), torch.from_numpy(sigma_live).to(dev),
                                torch.from_numpy(slot).to(dev), C)
    assert tuple(rgb.shape) == (M, C) and tuple(sigma.shape) == (M,)
    assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(sigma.cpu().numpy(), want_sigma)
    assert not rgb.cpu().numpy()[~live].any() and not sigma.cpu().numpy()[~live].any()          # culled rows: exactly zero


def test_expand_writes_every_element():
    dev, ops, lib = _gpu(), _ops(), __import__("plenoctree_amd")._lib.load()
    import ctypes
    M, C = 3 * BLOCK + 17, 75
    slot = torch.full((M,), -1, dtype=torch.int32, device=dev)
    slot[5], slot[M - 1] = 0, 1
    rgb_live = torch.arange(2 * C, dtype=torch.float32, device=dev).reshape(2, C) + 1
    sigma_live = torch.tensor([3.0, 4.0], device=dev)
    rgb = torch.full((M, C), float("nan"), device=dev)
    sigma = torch.full((M,), float("nan"), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.pxo_occ_expand(p(rgb_live), p(sigma_live), p(slot), M, C, p(rgb), p(sigma),
                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    assert not torch.isnan(rgb).any() and not torch.isnan(sigma).any()
    assert torch.equal(rgb[5], rgb_live[0]) and torch.equal(rgb[M - 1], rgb_live[1]) and float(sigma[M - 1]) == 4.0
    assert int((rgb != 0).any(dim=1).sum()) == 2


# ---- the culled render ------------------------------------------------------------------------------------------------------------
B, NC, NF, DEG = 37, 8, 16, 2


@pytest.fixture(scope="module")
def scene():
    dev, ops = _gpu(), _ops()
    ocfg = O.Cfg(num_coarse_samples=NC, num_fine_samples=NF, sh_deg=DEG, sparsity_npoints=16)
    flat = make_params(ocfg, seed=3).to(dev)
    rays = make_rays(B, seed=5)
    o, d, v = (x.to(dev).contiguous() for x in rays)
    gen = torch.Generator().manual_seed(9)
    lam = torch.rand(9, generator=gen) * 4 + 0.5
    mu = torch.randn(9, 3, generator=gen)
    lobes = torch.cat([lam[:, None], mu / mu.norm(dim=-1, keepdim=True)], dim=1).to(dev).contiguous()      # K = 9 = (DEG + 1)^2
    t_rand = torch.rand(B, NC, generator=gen).to(dev)
    u = torch.rand(B, NF, generator=gen).to(dev)
    packed = {}

    def images(cfg):
        key = cfg.mlp_precision
        if key not in packed:
            packed[key] = [ops.pack_weights(cfg, split_mlp(flat, ocfg, i), need_bwd=False)[0] for i in range(2)]
        return packed[key]
    return dict(dev=dev, ops=ops, ocfg=ocfg, o=o, d=d, v=v, lobes=lobes, t_rand=t_rand, u=u, images=images)


def _cfg(scene, white_bkgd, precision=0):
    cfg = pxo_cfg(scene["ops"], scene["ocfg"])
    cfg.white_bkgd, cfg.mlp_precision = int(white_bkgd), precision
    return cfg


def _flat(outs):
    return [t for level in outs for t in level]


NAMES = ("rgb_c", "disp_c", "acc_c", "rgb_f", "disp_f", "acc_f")


def _assert_same_bits(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        same = torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert same, f"{what}: {name} differs in rows {torch.nonzero((a != b).reshape(B, -1).any(dim=1)).reshape(-1).tolist()[:10]}"


@pytest.mark.parametrize("sg, white_bkgd, precision, randomized", [
    (False, 1, 0, False), (False, 0, 0, False), (True, 1, 0, False), (True, 0, 0, False), (False, 1, 2, False), (False, 1, 0, True)])
def test_render_all_ones_grid_is_the_dense_render(scene, sg, white_bkgd, precision, randomized):
    """Every sample live: the MLP launch sees the same rows in the same order, so all six outputs are pxo_render_fwd's bit for bit
    (a row of the fused MLP is its own dot products in a fixed k order: its value does not depend on the launch it sits in)."""
    ops, dev = scene["ops"], scene["dev"]
    cfg = _cfg(scene, white_bkgd, precision)
    pk = scene["images"](cfg)
    lobes = scene["lobes"] if sg else None
    kw = dict(randomized=randomized, t_rand=scene["t_rand"] if randomized else None, u=scene["u"] if randomized else None, lobes=lobes)
    want = _flat(ops.render_fwd(cfg, pk[0], pk[1], scene["o"], scene["d"], scene["v"], **kw))
    # a box of half side 8 holds every sample (the rays start 4 from the origin and end at most 6.6 further on)
    grid = _grid(ops, dev, np.ones((RESO, RESO, RESO), bool), 1, offset=[0.5] * 3, scale=[1.0 / 16] * 3)
    rows = []
    got = _flat(ops.render_fwd_culled(cfg, grid, pk[0], pk[1], scene["o"], scene["d"], scene["v"], live_rows=rows, **kw))
    assert rows == [B * NC, B * (NC + NF)]
    _assert_same_bits(got, want, "all-ones grid")
    assert all(torch.isfinite(t).all() for t in got)


def _twin(scene, cfg, pk, mask, outside_live):
    """The culled render composed from the per-stage entry points: every row through the MLP, the rows the numpy rule culls set to
    zero, then the existing compositing; the fine level samples from the coarse weights of that."""
    ops = scene["ops"]
    o, d, v = scene["o"], scene["d"], scene["v"]
    bits = R.bits_from_mask(mask)
    out, rows = [], []
    z, pts = ops.sample_along_rays(o, d, NC, cfg.near_, cfg.far_)
    for level in range(2):
        rgb, sigma = ops.mlp_fwd(cfg, pk[level], pts)
        live = torch.from_numpy(R.live_mask(bits, RESO, OFFSET, SCALE, outside_live, pts.reshape(-1, 3).cpu().numpy())).to(rgb.device)
        rows.append(int(live.sum()))
        rgb[~live] = 0.0
        sigma[~live] = 0.0
        comp, disp, acc, w = ops.shade_composite_fwd(cfg, rgb, sigma, z, d, v)
        out += [comp, disp, acc]
        if level == 0:
            z, pts = ops.sample_pdf(z, w, o, d, NF)
    return out, rows


def _masks():
    half = np.zeros((RESO, RESO, RESO), bool)
    half[:2] = True                                               # the half space x < 0
    x, y, z = np.meshgrid(*[np.arange(RESO)] * 3, indexing="ij")
    return {"half_space": half, "checkerboard": (x + y + z) % 2 == 0}


@pytest.mark.parametrize("outside_live", [0, 1])
@pytest.mark.parametrize("mask_name", ["half_space", "checkerboard"])
@pytest.mark.parametrize("white_bkgd", [1, 0])
def test_render_real_mask_sh(scene, white_bkgd, mask_name, outside_live):
    ops, dev = scene["ops"], scene["dev"]
    cfg = _cfg(scene, white_bkgd)
    pk = scene["images"](cfg)
    mask = _masks()[mask_name]
    want, want_rows = _twin(scene, cfg, pk, mask, outside_live)
    rows = []
    got = _flat(ops.render_fwd_culled(cfg, _grid(ops, dev, mask, outside_live), pk[0], pk[1], scene["o"], scene["d"], scene["v"],
                                      live_rows=rows))
    assert rows == want_rows
    assert 0 < rows[0] < B * NC and 0 < rows[1] < B * (NC + NF), rows          # the mask does cull, and not everything
    _assert_same_bits(got, want, f"{mask_name}, outside_live {outside_live}")


@pytest.mark.parametrize("outside_live", [0, 1])
@pytest.mark.parametrize("mask_name", ["half_space", "checkerboard"])
def test_render_real_mask_sg(scene, mask_name, outside_live):
    """The per-stage compositing entry point has no lobe argument, so the SG render has no bit-exact twin of its colours.  What
    does not depend on the basis -- the live rows, acc and disp of both levels (functions of sigma and z alone, and the fine
    samples follow from the coarse weights) -- equals the SH twin's bit for bit.  The colours are held to the SG training
    composite (pxo_sg_shade_composite_train: the same sums in another kernel, documented to agree to float32 round-off) on the
    culled rows: at most S = 24 terms weight * sigmoid <= 1 each, so 24 * 2^-23 = 3e-6 of round-off; bound 1e-5."""
    ops, dev = scene["ops"], scene["dev"]
    cfg = _cfg(scene, 1)
    pk = scene["images"](cfg)
    mask = _masks()[mask_name]
    want, want_rows = _twin(scene, cfg, pk, mask, outside_live)
    rows = []
    grid = _grid(ops, dev, mask, outside_live)
    got = _flat(ops.render_fwd_culled(cfg, grid, pk[0], pk[1], scene["o"], scene["d"], scene["v"], lobes=scene["lobes"], live_rows=rows))
    assert rows == want_rows
    for i in (1, 2, 4, 5):
        assert torch.equal(got[i], want[i]), NAMES[i]
    # colours of the coarse level against the training composite on the same culled rows
    o, d, v = scene["o"], scene["d"], scene["v"]
    z, pts = ops.sample_along_rays(o, d, NC, cfg.near_, cfg.far_)
    rgb, sigma = ops.mlp_fwd(cfg, pk[0], pts)
    live = torch.from_numpy(R.live_mask(R.bits_from_mask(mask), RESO, OFFSET, SCALE, outside_live, pts.reshape(-1, 3).cpu().numpy())).to(dev)
    rgb[~live] = 0.0
    sigma[~live] = 0.0
    tr = ops.sg_shade_composite_train(cfg, scene["lobes"], rgb, sigma, z, d, v, torch.zeros(B, 3, device=dev))
    err = float((tr["comp_rgb"] - got[0]).abs().max())
    print(f"SG {mask_name} outside {outside_live}: coarse colour vs the training composite, max abs diff {err:.3g}")
    assert err <= 1e-5
    assert not torch.equal(got[0], want[0])                       # and they are not the SH colours


@pytest.mark.parametrize("sg", [False, True])
@pytest.mark.parametrize("white_bkgd", [1, 0])
def test_render_all_empty_grid(scene, white_bkgd, sg):
    ops, dev = scene["ops"], scene["dev"]
    cfg = _cfg(scene, white_bkgd)
    pk = scene["images"](cfg)
    grid = _grid(ops, dev, np.zeros((RESO, RESO, RESO), bool), 0)
    torch.cuda.synchronize()
    ops.profile_enable(tags=[ops.PROF_MLP_FWD])
    try:
        ops.profile_read(ops.PROF_MLP_FWD)
        rows = []
        got = _flat(ops.render_fwd_culled(cfg, grid, pk[0], pk[1], scene["o"], scene["d"], scene["v"], live_rows=rows,
                                          lobes=scene["lobes"] if sg else None))
        launches, _, _ = ops.profile_read(ops.PROF_MLP_FWD)
    finally:
        ops.profile_enable(False)
    assert rows == [0, 0] and launches == 0                       # no MLP launch at all
    for i in (0, 3):
        assert torch.equal(got[i], torch.full((B, 3), float(white_bkgd), device=dev)), NAMES[i]      # the background
    for i in (2, 5):
        assert torch.equal(got[i], torch.zeros(B, device=dev)), NAMES[i]


def test_render_culled_refuses_noise_and_counts_launches(scene):
    ops, dev = scene["ops"], scene["dev"]
    cfg = _cfg(scene, 1)
    pk = scene["images"](cfg)
    grid = _grid(ops, dev, _masks()["half_space"], 0)
    ops.profile_enable(tags=[ops.PROF_MLP_FWD])
    try:
        ops.profile_read(ops.PROF_MLP_FWD)
        rows = []
        ops.render_fwd_culled(cfg, grid, pk[0], pk[1], scene["o"], scene["d"], scene["v"], live_rows=rows)
        launches, _, mlp_rows = ops.profile_read(ops.PROF_MLP_FWD)
    finally:
        ops.profile_enable(False)
    assert launches == 2 and mlp_rows == sum(rows)                # the existing launch, once per level, on the live rows only
    cfg.noise_std = 0.5
    with pytest.raises(ops.PxoError, match="resurrect"):
        ops.render_fwd_culled(cfg, grid, pk[0], pk[1], scene["o"], scene["d"], scene["v"], randomized=True)
    ops.render_fwd_culled(cfg, grid, pk[0], pk[1], scene["o"], scene["d"], scene["v"], randomized=False)      # noise is off: fine


# ---- grids from a model and from a tree -------------------------------------------------------------------------------------------
def test_grid_from_model_and_from_tree(scene, tmp_path):
    from plenoctree_amd.nerf_sh.nerf import models, occupancy
    from plenoctree_amd.octree import extraction, svox
    ops, dev = scene["ops"], scene["dev"]
    cfg = _cfg(scene, 1)
    pk = scene["images"](cfg)
    model = models.NerfModel(cfg)
    state = type("S", (models.Workspace,), {})()
    state.packed, state.params = [(pk[0], None), (pk[1], None)], pk[0]
    reso, radius = 12, [2.0, 1.0, 1.5]
    grid = occupancy.from_model(model, state, reso, center=[0.1, 0.0, -0.2], radius=radius, alpha_thresh=0.05, dilate=1)
    sigma = extraction.grid_sigma(model, state, reso, [0.1, 0.0, -0.2], radius).cpu().numpy()
    want = R.pack(sigma, reso, np.float32(occupancy.sigma_thresh(0.05, radius, reso)), 1)
    assert np.array_equal(grid.bits.cpu().numpy(), want)
    off, sc = extraction.tree_transform([0.1, 0.0, -0.2], radius)
    assert np.allclose(grid.offset, off) and np.allclose(grid.scale, sc) and not grid.outside_live
    assert 0.0 < grid.fraction_occupied() <= 1.0
    # model.apply routes to the culled entry and, without the argument, makes the dense call
    rays = O.Rays(scene["o"], scene["d"], scene["v"])
    rows = []
    culled = model.apply(state, rays, False, occupancy=grid, live_rows=rows)
    direct = ops.render_fwd_culled(cfg, grid, pk[0], pk[1], scene["o"], scene["d"], scene["v"])
    _assert_same_bits(_flat(culled), _flat(direct), "model.apply(occupancy=)")
    assert len(rows) == 2 and rows[0] <= B * NC
    dense = model.apply(state, rays, False)
    _assert_same_bits(_flat(dense), _flat(ops.render_fwd(cfg, pk[0], pk[1], scene["o"], scene["d"], scene["v"])), "model.apply")
    # a tree: occupied iff the leaf under the cell centre has sigma > 0, over the tree's own box
    from plenoctree_amd import octree_ops as oops
    rs = np.random.RandomState(4)
    tree = svox.N3Tree(N=2, data_dim=3 * 9 + 1, depth_limit=2, radius=[1.5, 1.0, 2.0], center=[0.0, 0.25, 0.0], data_format="SH9",
                       map_location=dev).refine_from_mask(torch.from_numpy((rs.rand(512) < 0.5).astype(np.uint8)).to(dev))
    assert tree.max_depth == 2
    with torch.no_grad():
        sig = torch.from_numpy(((rs.rand(tree.n_internal, 2, 2, 2) - 0.6) * 5).astype(np.float32)).clamp_(min=0.0)
        tree.data.data[..., -1] = sig.to(dev)
    for depth in (2, 3):
        g = occupancy.from_tree(tree, depth, dilate=0, outside="live")
        n = 1 << depth
        c = (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) / n
        t = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
        world = ((t - tree.offset.to(dev)) / tree.invradius.to(dev)).contiguous()
        leaf = oops.tree_query(tree.child, world, tree.offset, tree.invradius)
        want_mask = (tree.data.data.reshape(-1, 28)[leaf, -1] > 0).cpu().numpy()
        assert 0 < want_mask.sum() < want_mask.size
        assert np.array_equal(g.bits.cpu().numpy(), R.bits_from_mask(want_mask))
        assert g.reso == n and g.outside_live and np.allclose(g.offset, tree.offset.numpy()) and np.allclose(g.scale, tree.invradius.numpy())
    with pytest.raises(ValueError, match="finer than the tree"):
        occupancy.from_tree(tree, tree.max_depth + 2)
    path = os.path.join(str(tmp_path), "t.npz")
    tree.save(path)
    g2 = occupancy.from_tree(path, 3, dilate=0, outside="live", device=dev)
    assert g2.reso == 8 and g2.count_occupied() > 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_eval_cli_with_and_without_the_grid(tmp_path, capsys):
    """nerf_sh.eval on the small analytic dataset with a fresh model: --occupancy_reso 16 runs, reports and writes its outputs;
    --occupancy_reso 0 writes the files of the plain render (model.apply through utils.render_image, as before the flag)."""
    from PIL import Image
    from plenoctree_amd.nerf_sh import eval as nerf_eval
    from plenoctree_amd.nerf_sh.nerf import datasets, families, utils
    dev = _gpu()
    cfg_path = os.path.join(str(tmp_path), "tiny.yaml")
    with open(cfg_path, "w") as f:
        f.write("dataset: synthetic\nfactor: 20\nnum_coarse_samples: 16\nnum_fine_samples: 32\nuse_viewdirs: false\nwhite_bkgd: true\n"
                "sh_deg: 1\n")
    dirs = {}
    for name, extra in (("off", ["--occupancy_reso", "0"]), ("on", ["--occupancy_reso", "16", "--occupancy_radius", "1.5"])):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        dirs[name] = d
        psnrs = nerf_eval.main(["--train_dir", d, "--config", cfg_path, "--approx_eval_skip", "1000", "--chunk", "1000", *extra])
        assert len(psnrs) == 1 and np.isfinite(psnrs[0])
        out = capsys.readouterr().out
        assert ("occupancy grid 16^3 from model" in out and "live rows: coarse" in out) == (name == "on"), out
        assert sorted(os.listdir(os.path.join(d, "test_preds"))) == sorted(["000.png", "disp_000.png", "psnr.txt", "ssim.txt",
                                                                          "psnrs_0.txt", "ssims_0.txt"])
    # the plain render, made here the way eval made it before the flag existed
    argv = ["--train_dir", dirs["off"], "--config", cfg_path]
    args = utils.define_flags().parse_args(argv)
    utils.update_flags(args)
    model, state = families.restore(args, dev, "render", say=lambda *a, **k: None)
    ex = datasets.get_dataset("test", args, dev).get_image(0)
    rgb, disp, _ = utils.render_image(lambda r: model.apply(state, r, False), ex["rays"], chunk=1000)
    utils.save_img(rgb, os.path.join(str(tmp_path), "ref.png"))
    utils.save_img(disp[..., 0], os.path.join(str(tmp_path), "ref_disp.png"))
    for ours, ref in (("000.png", "ref.png"), ("disp_000.png", "ref_disp.png")):
        a = np.asarray(Image.open(os.path.join(dirs["off"], "test_preds", ours)))
        b = np.asarray(Image.open(os.path.join(str(tmp_path), ref)))
        assert a.shape == b.shape == ((40, 40, 3) if ours == "000.png" else (40, 40)) and np.array_equal(a, b), ours
