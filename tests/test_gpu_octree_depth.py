"""The octree marchers against oracle/octree_oracle.py at production depth and grid size.

tests/test_gpu_octree.py holds every kernel variant to the oracle on trees of depth <= 3 and weight grids of 12 / 16 / 64;
all renderer variants share one Marcher::find (11-bit quantisation, path reuse through a per-row stack, the depth stop), so a
defect there at depth > 3 would be reproduced by every variant alike.  Here: trees of depth 6 / 8 / 10 built without a dense
mask (tests/_octree_cases.py: shell = leaves at every depth, rod = thousands of consecutive deepest-level samples, chunked =
last level out of packed-parent order), rays aimed into leaves of every depth, ray arguments no other test passes (zero
direction components, origins on the boundary / on cell faces, viewdirs != dirs, fy != fx), and weight grids of 10, 13
(unbricked kernel), 20, 96 (bricked, not a power of two), 128, 256 (many slabs) and 1024 (no index tables).  That the cases
reach what they claim is asserted without a GPU in tests/test_octree_cases_cpu.py.

Bars (those of tests/test_gpu_octree.py): integers and bit-equalities exact; images atol 2e-5; weights rtol 1e-5, atol 1e-6;
gradients rtol 2e-3, atol 2e-6 max|g| + 1e-7.  No case needed more: the long marches (rod rays, up to ~4300 samples per
ray; grid 1024) stay inside the plain bars, so no bound here is derived from a measured floor.  The oracle's own
float32-vs-float64 deviation on the same sample sequence (no code under test involved) is printed next to the observed
error as a diagnostic only.  Every test prints its observed error next to its bound (pytest -s).

Out of scope: grid size 2048 (>= 96 GB of device buffers and 32 GB of host memory for sigma alone)."""
import functools
import time

import numpy as np
import pytest
import torch

import _octree_cases as C
from oracle import octree_oracle as T
from _helpers import _gpu, close

pytestmark = pytest.mark.gpu
f32 = np.float32
IMG_ATOL = 2e-5
CASES = [(f, d) for d in C.DEPTHS for f in C.FAMILIES]


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _device_tree(t, dev):
    """(view, the device tensors it points into: the caller keeps them alive for as long as it uses the view)."""
    child = torch.from_numpy(t.child).to(dev)
    data = torch.from_numpy(t.data).to(dev)
    return _oops().tree_view(child, data, t.offset, t.invradius), (child, data)


def _opts(opt):
    return _oops().render_opts(float(opt.step_size), float(opt.background_brightness), float(opt.sigma_thresh),
                               float(opt.stop_thresh))


def _packed(t, pts_world):
    out = []
    for p in np.asarray(pts_world, f32):
        n, i, j, k, _, _ = t.query(t.world2tree(p))
        out.append(((n * 2 + i) * 2 + j) * 2 + k)
    return np.asarray(out, np.int64)


@functools.lru_cache(maxsize=None)
def _explicit_rays(family, depth, K):
    """name -> (origins, dirs, viewdirs, step size)."""
    t = C.make_tree(family, depth, K)
    ao, ad = C.aimed_rays(t, 5)
    names, eo, ed, ev = C.edge_rays()
    sets = {"aimed": (ao, ad, ad, 1e-3), "edge": (eo, ed, ev, 1e-3)}
    if family == "rod":
        o1, d1 = C.rod_axis_rays(t)
        o2, d2 = C.rod_skew_rays(t, 3)
        o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        sets["rod"] = (o, d, d, C.ROD_STEP)
    return sets


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,depth", CASES)
def test_lookup_matches_oracle_exactly(family, depth):
    """tree_query == Tree.query (packed index, exact) at interior points of leaves of every depth, at points ON cell faces of
    every level (dyadic tree coordinates k 2^-(d+1), the volume's faces included) and outside the volume; every
    tree_sample_leaves sample of leaves of every depth queries back to its own leaf."""
    oops = _oops(); dev = _gpu()
    t = C.make_tree(family, depth, 4)
    rs = np.random.RandomState(depth)
    lv = t.leaves()
    dep = t.parent_depth[lv[:, 0], 1]
    pick = np.concatenate([rs.choice(np.nonzero(dep == d)[0], 150) for d in range(1, depth + 1)])
    corner, side = T.leaf_corners(t, lv[pick])
    interior = C.tree2world(t, corner + side[:, None] * (0.02 + 0.96 * rs.rand(len(pick), 3)))
    dyadic = []
    for d in range(depth + 1):
        n = 2 ** (d + 1)
        k = rs.randint(0, n + 1, (150, 3))
        k[:6] = [[0, 0, 0], [n, n, n], [n // 2, 1, n - 1], [n, 0, n // 2], [1, n, 0], [n // 2, n // 2, n // 2]]
        dyadic.append(C.tree2world(t, k / n))
    # faces of the leaves themselves: lower corners of picked leaves, which are dyadic at the leaf's own level
    dyadic.append(C.tree2world(t, corner))
    outside = rs.uniform(-6.0, 6.0, (400, 3))
    probe = np.concatenate([interior, *dyadic, outside]).astype(f32)
    child = torch.from_numpy(t.child).to(dev)
    got = oops.tree_query(child, torch.from_numpy(probe).to(dev), t.offset, t.invradius).cpu().numpy()
    want = _packed(t, probe)
    assert np.array_equal(got, want), (int((got != want).sum()), probe[got != want][:5])
    assert np.array_equal(want[:len(pick)], (lv[pick] * [8, 4, 2, 1]).sum(1))       # interior points: the leaf they were drawn in
    assert set(np.unique(t.parent_depth[want // 8, 1])) >= set(range(1, depth + 1))
    # samples of leaves of every depth
    S = 4
    packed = torch.from_numpy((lv[pick] * [8, 4, 2, 1]).sum(1).astype(np.int64)).to(dev)
    pd = torch.from_numpy(t.parent_depth).to(dev)
    pts = oops.tree_sample_leaves(pd, packed, S, t.offset, t.invradius, seed=depth)
    again = oops.tree_query(child, pts.view(-1, 3), t.offset, t.invradius).view(-1, S)
    assert torch.equal(again, packed[:, None].expand(-1, S))
    want_back = _packed(t, pts.view(-1, 3).cpu().numpy()).reshape(-1, S)
    assert np.array_equal(want_back, again.cpu().numpy())


@pytest.mark.parametrize("family,depth", CASES)
def test_march_counters_match_oracle_exactly(family, depth):
    """octree_count_work repeats the renderer's march; rays, samples, shaded samples, distinct leaves AND child-pointer
    loads equal what the oracle's sample sequence implies, exact and with the `fast` preset, on both camera views (the
    second has fy != fx) and, on the rod tree, on the camera along the rod (thousands of consecutive deepest-level
    samples).  The expected load count (tests/_octree_cases.py: tree_march_counts) restarts each descent at the deepest
    common ancestor of consecutive samples' nodes, so equality fails for one level less reuse as for one level more;
    it is itself strictly below the count without reuse (asserted), which is below depth + 1 per sample."""
    oops = _oops(); dev = _gpu()
    t = C.make_tree(family, depth, 4)
    view, _keep = _device_tree(t, dev)
    jobs = [(C.CAMERA_VIEWS[0], T.RenderOptions.for_renderer(1e-3, False)), (C.CAMERA_VIEWS[1], T.RenderOptions.for_renderer(1e-3, True)),
            (C.CAMERA_VIEWS[1], T.RenderOptions.for_renderer(1e-3, False))]
    if family == "rod":
        jobs.append((C.rod_view(t), T.RenderOptions(C.ROD_STEP)))
    for cam, opt in jobs:
        want, no_reuse = C.tree_march_counts(t, cam, opt)
        got = oops.octree_count_work(view, torch.from_numpy(cam["c2w"]).to(dev), cam["W"], cam["H"], cam["fx"], _opts(opt), fy=cam["fy"])
        print(f"\n{family} depth {depth} {cam['W']}x{cam['H']} stop {float(opt.stop_thresh):g}: {got}; "
              f"{got['child_loads'] / max(got['samples'], 1):.2f} loads per sample, {no_reuse} without reuse")
        assert got == want, (got, want)
        assert want["samples"] > 300 and want["shaded_samples"] > 100
        assert got["samples"] <= got["child_loads"] < no_reuse <= got["samples"] * (depth + 1)
        assert got["child_loads"] < got["samples"] * (depth + 1)


def _forward_Ks(depth):
    return (1, 4, 9, 16, 25) if depth == 8 else (4, 16)


@pytest.mark.parametrize("family,depth", CASES)
def test_forward_matches_oracle(family, depth):
    """Every lane variant (4 / 8 / 16) and SH format against the oracle: aimed, rod and edge rays through octree_render_rays
    (viewdirs != dirs on the edge set), both camera views through octree_render_persp (one with fy != fx), each exact and with
    the `fast` preset; aimed rays again with background 0 and a step of two deepest cells (at least 2e-3).  Bound 2e-5
    throughout.  Observed on an MI355X: <= 3.6e-7 in every case, the rod rays (up to ~4300 samples) included, whose
    oracle float32-vs-float64 floor (render_ray against render_rays_torch, printed) is <= 8e-7."""
    oops = _oops(); dev = _gpu()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    worst = {}
    t_oracle = t_gpu = 0.0
    for K in _forward_Ks(depth):
        t = C.make_tree(family, depth, K)
        view, _keep = _device_tree(t, dev)
        jobs = []                                        # (name, launch(), oracle image)
        t0 = time.time()
        for name, (o, d, v, step) in _explicit_rays(family, depth, K).items():
            for fast in (False, True):
                opt = T.RenderOptions.for_renderer(step, fast)
                want = np.stack([T.render_ray(t, oo, dd, vv, opt) for oo, dd, vv in zip(o, d, v)])
                if name == "rod" and not fast:            # diagnostic only: no bound depends on it
                    ref64 = T.render_rays_torch(t, torch.from_numpy(t.data), o, d, v, opt).numpy()
                    worst[f"SH{K} rod oracle float32 floor (diagnostic)"] = float(np.abs(want - ref64).max())
                jobs.append((f"SH{K} {name} fast={fast}",
                             functools.partial(oops.octree_render_rays, view, to(o), to(d), to(v), _opts(opt)), want))
                if name == "edge":
                    idx = [C.edge_rays()[0].index(n) for n in C.EDGE_BACKGROUND]
                    assert np.array_equal(want[idx], np.ones((3, 3), f32))
        o, d, v, _ = _explicit_rays(family, depth, K)["aimed"]
        opt = T.RenderOptions(max(2e-3, 2.0 ** -depth), background_brightness=0.0)     # two deepest cells, at least 2e-3
        assert float(opt.step_size) > 2.0 ** -(depth + 1)
        want = np.stack([T.render_ray(t, oo, dd, vv, opt) for oo, dd, vv in zip(o, d, v)])
        jobs.append((f"SH{K} aimed bg=0 big step",
                     functools.partial(oops.octree_render_rays, view, to(o), to(d), to(v), _opts(opt)), want))
        for cam, fast in ((C.CAMERA_VIEWS[0], False), (C.CAMERA_VIEWS[1], False), (C.CAMERA_VIEWS[1], True)):
            opt = T.RenderOptions.for_renderer(1e-3, fast)
            want = T.render_persp(t, cam["c2w"], cam["W"], cam["H"], cam["fx"], opt, fy=cam["fy"])
            # the view sees the tree (the rod tree is thin and kept translucent for its long marches: 50 x the image bar there)
            assert float(np.abs(want - 1.0).max()) > (1e-3 if family == "rod" else 0.2)
            jobs.append((f"SH{K} view fy={cam['fy']} fast={fast}",
                         functools.partial(oops.octree_render_persp, view, to(cam["c2w"]), cam["W"], cam["H"], cam["fx"],
                                           _opts(opt), fy=cam["fy"]), want))
        t_oracle += time.time() - t0
        t0 = time.time()
        try:
            for lanes in (4, 8, 16):
                oops.set_lanes_per_ray(lanes, lanes)
                for name, launch, want in jobs:
                    got = launch().cpu().numpy()
                    assert got.shape == want.shape and np.isfinite(got).all(), name
                    err = float(np.abs(got - want).max())
                    worst[name] = max(worst.get(name, 0.0), err)
                    assert err <= IMG_ATOL, (name, lanes, err)
        finally:
            oops.set_lanes_per_ray(0, 0)
        t_gpu += time.time() - t0
    print(f"\n{family} depth {depth}: oracle {t_oracle:.1f} s, device {t_gpu:.1f} s; max abs err over lanes 4/8/16 " +
          ", ".join(f"{k}: {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("depth", C.DEPTHS)
def test_far_origin_ends_by_the_stop_guard(depth):
    """Step size 1e-7 from 4e3 world units away: inside the fine cells t + delta_t == t, and the march ends by the kernels'
    `!(tn > t)` guard (tests/test_octree_cases_cpu.py shows that the guarded march of this ray ends that way).  The oracle's
    loop has no such guard and would not terminate on this ray, so there is no oracle image: asserted are termination,
    finiteness, a colour inside [0, 1] (background 1, sigmoid colours) and agreement of the three lane variants to the
    image bar."""
    oops = _oops(); dev = _gpu()
    t = C.make_tree("shell", depth, 4)
    view, keep = _device_tree(t, dev)
    o, d, opt, n = C.far_origin_ray(t)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a[None])).to(dev)
    out = {}
    try:
        for lanes in (4, 8, 16):
            oops.set_lanes_per_ray(lanes, lanes)
            out[lanes] = oops.octree_render_rays(view, to(o), to(d), to(d), _opts(opt)).cpu().numpy()
            grad = torch.zeros_like(keep[1])
            oops.octree_render_rays_bwd(view, to(o), to(d), to(d), _opts(opt), torch.ones(1, 3, device=dev), grad)
            assert bool(torch.isfinite(grad).all())
    finally:
        oops.set_lanes_per_ray(0, 0)
    for lanes, rgb in out.items():
        assert np.isfinite(rgb).all() and (rgb >= 0).all() and (rgb <= 1.0 + 1e-6).all(), (lanes, rgb)
        assert float(np.abs(rgb - out[16]).max()) <= IMG_ATOL, (lanes, rgb, out[16])


def _gradient_cases():
    """K = 4 everywhere (the run-time-K gradient kernel); at depth 8 also K = 16, the compiled SH16 instantiation."""
    return [(f, d, K) for f, d in CASES for K in ((4, 16) if d == 8 else (4,))]


@pytest.mark.parametrize("family,depth,K", _gradient_cases())
def test_gradient_matches_float64_oracle(family, depth, K):
    """d sum(rgb * g) / d data against render_rays_torch in float64 on aimed + rod-line rays (>= 64 rays: more than two
    full waves at 4 lanes per ray), for both PXO_TUNE_BWD_UPDATE forms x cache rows 0 / 4 / 16 x 4 and 16 lanes x with
    and without the forward image; exactly zero on every leaf no ray sampled.  Bound: rtol 2e-3, atol 2e-6 max|g| + 1e-7,
    in every case.  The float32-autograd-vs-float64 deviation of the oracle itself is printed as a diagnostic and enters
    no bound."""
    oops = _oops(); dev = _gpu()
    t = C.make_tree(family, depth, K)
    view, (_child, data) = _device_tree(t, dev)
    sets = _explicit_rays(family, depth, K)
    ao, ad = sets["aimed"][0], sets["aimed"][1]
    sel = np.arange(0, len(ao), max(1, len(ao) // 90))
    ro, rd = C.rod_axis_rays(t)
    so, sd = C.rod_skew_rays(t, 3)
    o, d = np.concatenate([ao[sel], ro, so]), np.concatenate([ad[sel], rd, sd])
    assert len(o) >= 64
    rs = np.random.RandomState(depth)
    v = rs.randn(len(o), 3); v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)     # viewdirs != dirs
    g = rs.randn(len(o), 3).astype(f32)
    opt = T.RenderOptions(C.ROD_STEP if family == "rod" else 1e-3)
    t0 = time.time()
    grads = {}
    for dtype in (torch.float64, torch.float32):
        dd = torch.tensor(t.data.astype(np.float64), requires_grad=True)
        out = T.render_rays_torch(t, dd, o, d, v, opt, dtype=dtype)
        (out * torch.from_numpy(g).to(dtype)).sum().backward()
        grads[dtype] = dd.grad.clone()
        if dtype == torch.float64:
            fwd64 = out.detach()
    want = grads[torch.float64].float()
    gmax = float(want.abs().max())
    oracle_f32_dev = float((grads[torch.float32] - grads[torch.float64]).abs().max())      # diagnostic only
    atol = 2e-6 * gmax + 1e-7
    sampled = np.zeros(t.data.shape[0] * 8, bool)
    sampled[list(C.sampled_leaves(t, o, d, opt))] = True
    assert gmax > 1e-3 and 50 < sampled.sum() < sampled.size
    untouched = torch.from_numpy(~sampled).to(dev)
    t_oracle = time.time() - t0
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    do, dd_, dv, dg = to(o), to(d), to(v), to(g)
    worst = 0.0
    default_upd, default_rows = oops.get_tuning(oops.TUNE_BWD_UPDATE), oops.get_tuning(oops.TUNE_BWD_CACHE_ROWS)
    try:
        for lanes in (4, 16):
            oops.set_lanes_per_ray(lanes, lanes)
            fwd = oops.octree_render_rays(view, do, dd_, dv, _opts(opt))
            for upd in (0, 1):
                for rows in (0, 4, 16):
                    oops.set_tuning(oops.TUNE_BWD_UPDATE, upd); oops.set_tuning(oops.TUNE_BWD_CACHE_ROWS, rows)
                    for out_rgb in (None, fwd):
                        grad = torch.zeros_like(data)
                        oops.octree_render_rays_bwd(view, do, dd_, dv, _opts(opt), dg, grad, out_rgb=out_rgb)
                        name = (f"{family} depth {depth} SH{K} lanes {lanes} update {upd} rows {rows} "
                                f"out_rgb {out_rgb is not None}")
                        assert not bool(grad.view(-1, t.data_dim)[untouched].any()), name
                        worst = max(worst, float((grad.cpu() - want).abs().max()))
                        close(name, grad, want, rtol=2e-3, atol=atol)
    finally:
        oops.set_lanes_per_ray(0, 0)
        oops.set_tuning(oops.TUNE_BWD_UPDATE, default_upd); oops.set_tuning(oops.TUNE_BWD_CACHE_ROWS, default_rows)
    print(f"\n{family} depth {depth} SH{K}: {len(o)} rays, oracle {t_oracle:.1f} s, max|g| {gmax:.3e}, atol {atol:.2e}, "
          f"max abs gradient err {worst:.2e} (rel. to max|g| {worst / gmax:.2e}); diagnostics: oracle float32 autograd "
          f"vs float64 {oracle_f32_dev:.2e}, forward vs float64 {float((fwd.cpu().double() - fwd64).abs().max()):.2e}")


@pytest.mark.parametrize("depth", C.DEPTHS)
def test_chunked_tree_renders_as_its_breadth_first_twin(depth):
    """Second, oracle-free check of the out-of-order last level: the breadth-first tree of the same geometry, its data rows
    fetched from the chunked tree through tree_query at the leaf centres, gives the same image and the same rays."""
    oops = _oops(); dev = _gpu()
    K = 16
    ch, one = C.make_tree("chunked", depth, K), C.make_tree("shell", depth, K)
    view_c, (child_c, data_c) = _device_tree(ch, dev)
    lv = one.leaves()
    corner, side = T.leaf_corners(one, lv)
    centres = torch.from_numpy(C.tree2world(one, corner + 0.5 * side[:, None]).astype(f32)).to(dev)
    rows = oops.tree_query(child_c, centres, ch.offset, ch.invradius)
    assert int(rows.min()) >= 0 and rows.unique().numel() == rows.numel()
    moved = torch.zeros(one.data.shape, device=dev).view(-1, one.data_dim)
    dst = torch.from_numpy((lv * [8, 4, 2, 1]).sum(1).astype(np.int64)).to(dev)
    moved[dst] = data_c.view(-1, ch.data_dim)[rows]
    assert not torch.equal(rows, dst)                                   # the node order really differs
    child_o = torch.from_numpy(one.child).to(dev)
    view_o = oops.tree_view(child_o, moved, one.offset, one.invradius)
    cam = C.CAMERA_VIEWS[1]
    args = (torch.from_numpy(cam["c2w"]).to(dev), cam["W"], cam["H"], cam["fx"], oops.render_opts(1e-3))
    im_c, im_o = oops.octree_render_persp(view_c, *args, fy=cam["fy"]), oops.octree_render_persp(view_o, *args, fy=cam["fy"])
    assert float((im_c - 1.0).abs().max()) > 0.2
    close("chunked vs breadth-first image", im_c, im_o, rtol=0, atol=IMG_ATOL)
    o, d = C.aimed_rays(ch, 5)
    to = lambda a: torch.from_numpy(a).to(dev)
    r_c = oops.octree_render_rays(view_c, to(o), to(d), to(d), oops.render_opts(1e-3))
    r_o = oops.octree_render_rays(view_o, to(o), to(d), to(d), oops.render_opts(1e-3))
    close("chunked vs breadth-first rays", r_c, r_o, rtol=0, atol=IMG_ATOL)
    print(f"\nchunked depth {depth}: image diff {float((im_c - im_o).abs().max()):.2e}, "
          f"rays diff {float((r_c - r_o).abs().max()):.2e}")


# ---------------------------------------------------------------------------------------------------------------
def _weights_close(name, got, want_dev):
    err = (got - want_dev).abs()
    tol = 1e-6 + 1e-5 * want_dev.abs()
    assert bool(torch.isfinite(got).all()), name
    worst = float(err.max())
    assert bool((err <= tol).all()), (name, int((err > tol).sum()), worst)
    return worst


@pytest.mark.parametrize("reso", C.GRID_SIZES)
def test_grid_weight_render_matches_oracle_at_every_kernel_path(reso):
    """grid_weight_render against T.grid_weight_render; default marcher choice, both forced marchers and (power-of-two grids)
    both tile orders bit-equal; camera-by-camera accumulation equal to one call; fy != fx; images wider than one tile and
    ragged from 20 up.  At 128 and 1024 the work counters equal the oracle's march."""
    oops = _oops(); dev = _gpu()
    W, H, fx, fy = C.grid_case(reso)
    t = C.new_tree(1, 3)
    opt = T.RenderOptions(step_size=1e-3)
    sigma = C.grid_sigma(reso)
    cams = C.GRID_CAMERAS
    t0 = time.time()
    want = np.zeros_like(sigma)
    for c in cams:
        T.grid_weight_render(sigma, c, W, H, fx, opt, t.offset, t.invradius, fy=fy, weight=want)
    t_oracle = time.time() - t0
    positive = int(np.count_nonzero(want))
    assert positive > 50
    sig_d, cams_d = torch.from_numpy(sigma).to(dev).reshape(-1), torch.from_numpy(cams).to(dev)
    want_d = torch.from_numpy(want).to(dev).reshape(-1)
    render = lambda cc=cams_d, acc=None: oops.grid_weight_render(sig_d, reso, cc, fx, fy, W, H, oops.render_opts(1e-3),
                                                                 t.offset, t.invradius, grid_weight=acc)
    got = render()
    worst = _weights_close(f"grid {reso}", got, want_d)
    assert int((got > 0).sum()) == positive
    occupied = float((sig_d > 0).float().mean())
    # the library does not report which marcher a default call ran; this restates its documented rule (slab-staged when
    # more than half of sigma is above the threshold) and is printed as such.  Coverage does not lean on it: both
    # forced marchers are held bit-equal to the default call below.
    by_rule = "slab-staged" if occupied > 0.5 else "per-sample"
    pow2 = reso % 4 == 0 and (reso & (reso - 1)) == 0
    default_order = oops.get_tuning(oops.TUNE_GW_TILE_ORDER)
    try:
        for order in ((0, 1) if pow2 else (default_order,)):
            oops.set_tuning(oops.TUNE_GW_TILE_ORDER, order)
            for mode in (0, 1):
                oops.set_tuning(oops.TUNE_GW_MARCHER, mode)
                w = render()
                assert torch.equal(w, got), (reso, order, mode, int((w != got).sum()))
                del w
    finally:
        oops.set_tuning(oops.TUNE_GW_TILE_ORDER, default_order); oops.set_tuning(oops.TUNE_GW_MARCHER, -1)
    acc = None
    for i in range(len(cams)):
        acc = render(cams_d[i:i + 1], acc)
    assert torch.equal(acc, got)
    del acc
    msg = ""
    if reso in (128, 1024):
        t0 = time.time()
        want_c = C.grid_march_counts(sigma, cams, W, H, fx, fy, opt, t.offset, t.invradius)
        t_oracle += time.time() - t0
        got_c = oops.grid_weight_count_work(sig_d, reso, cams_d, fx, fy, W, H, oops.render_opts(1e-3), t.offset, t.invradius)
        assert got_c == want_c, (got_c, want_c)
        msg = f", counters {got_c}"
    print(f"\ngrid {reso}: {W}x{H} x {len(cams)} cameras, {positive} voxels with weight, {100 * occupied:.2f} % of sigma "
          f"above threshold -> default marcher by the occupancy rule (not observed): {by_rule}; "
          f"max abs weight err {worst:.2e}; oracle {t_oracle:.1f} s{msg}")
