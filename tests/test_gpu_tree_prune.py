"""GPU tests of pruning a PlenOctree by the weight its leaves render with: pxo_octree_weight_accum_cams / _rays against
tests/_tree_prune_oracle.py, pxo_tree_collapse_mark / _emit against the numpy restatement of the definition, and
N3Tree.accumulate_weights / prune_ / refine_leaves and the octree.pruning CLI end to end.

Bounds of the weight cases (fixed before any GPU run; tests/test_tree_prune_cpu.py measures what they rest on):
  set    weights > 0 must be the oracle's set exactly.  Leaves whose float64 weight is below 1e-30 would be left out (at most
         2 % of the touched leaves per case); with fill_data's scales NO case leaves any out, so the sets are compared whole.
  max    the renderer's own bar for a compositing weight: atol 2e-5 against the float64 oracle.
  sum    for a leaf hit by c samples: (c - 1) 2^-24 (oracle sum), the error of c non-negative float32 additions in any order,
         plus c x 4 x the per-sample floor.  The floor, max |float32 restatement - float64 restatement| of one sample's weight
         over all of these inputs, was measured on the CPU as 1.247e-7 (PER_SAMPLE_FLOOR rounds it up to 1.25e-7); 4 x is the
         project's usual margin.  The observed maximum is printed.
Collapse: all four arrays equal the restatement exactly; the collapsed tree's render is held to the oracle's render of the same
collapsed tree at the renderer's atol 2e-5."""
import os

import numpy as np
import pytest
import torch

import _octree_cases as C
import _octree_ndc_oracle as N
import _tree_prune_oracle as P
from oracle import nerf_oracle as O
from oracle import octree_oracle as T
from _helpers import _gpu, close, make_params

pytestmark = pytest.mark.gpu
f32 = np.float32
PER_SAMPLE_FLOOR = 1.25e-7
OPS = ("max", "sum")


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _svox():
    from plenoctree_amd.octree import svox
    return svox


def _device_tree(t, dev):
    """(view, the device tensors it points into: the caller keeps them alive for as long as it uses the view)."""
    child, data = torch.from_numpy(t.child).to(dev), torch.from_numpy(t.data).to(dev)
    return _oops().tree_view(child, data, t.offset, t.invradius), (child, data)


def _opts(opt):
    return _oops().render_opts(float(opt.step_size), float(opt.background_brightness), float(opt.sigma_thresh),
                               float(opt.stop_thresh))


def _svox_tree(t, dev, fmt=None, extra=None):
    """The oracle tree `t` as an svox N3Tree on `dev`, float32 data as they are."""
    svox = _svox()
    K = (t.data_dim - 1) // 3
    z = {"data_dim": t.data_dim, "child": t.child, "parent_depth": t.parent_depth, "n_internal": t.n_internal,
         "invradius3": t.invradius, "offset": t.offset, "depth_limit": t.depth_limit, "data": t.data,
         "data_format": fmt or f"SH{K}"}
    if extra is not None:
        z["extra_data"] = extra
    tree = svox.N3Tree._from_npz(svox._NpzDict({k: np.asarray(v) for k, v in z.items()}), dev)
    tree.data.requires_grad_(False)
    return tree


def _oracle_tree(tree):
    """An svox N3Tree's arrays as an oracle Tree."""
    t = T.Tree.__new__(T.Tree)
    t.data_dim, t.depth_limit = tree.data_dim, tree.depth_limit
    t.invradius, t.offset = tree.invradius.numpy().copy(), tree.offset.numpy().copy()
    t.child, t.parent_depth = tree.child.cpu().numpy(), tree.parent_depth.cpu().numpy()
    t.data = tree.data.data.detach().cpu().numpy()
    return t


def _check_weights(name, got, lw, op, child):
    """The bounds of the module docstring.  `got`: device tensor [n*8]; lw: the oracle's LeafWeights."""
    got = got.detach().cpu().numpy().astype(np.float64).reshape(-1)
    assert np.isfinite(got).all() and (got >= 0).all(), name
    assert not got[np.asarray(child).reshape(-1) != 0].any(), f"{name}: a cell that is not a leaf was written"
    out = P.left_out(lw, op)
    assert not out.any(), f"{name}: the oracle leaves out {int(out.sum())} leaves; the cases were chosen so that none is"
    want_set = (lw.max32 if op == "max" else lw.sum32) > 0
    wrong = np.nonzero((got > 0) != want_set)[0]
    assert wrong.size == 0, f"{name}: touched set differs at {wrong.size} cells, first {wrong[:5]} (got {got[wrong[:5]]})"
    if op == "max":
        err = np.abs(got - lw.max64)
        print(f"{name} max: {int(want_set.sum())} leaves, max abs err {err.max() if err.size else 0:.3g} (bound 2e-5)")
        assert (err <= 2e-5).all(), f"{name}: max weight off by {err.max():.3g} at cell {int(err.argmax())}"
    else:
        err = np.abs(got - lw.sum64)
        c = lw.count.astype(np.float64)
        bound = np.maximum(c - 1, 0) * 2.0 ** -24 * lw.sum64 + c * 4 * PER_SAMPLE_FLOOR
        hit = np.nonzero(c > 0)[0]
        worst = int(hit[np.argmax(err[hit] / bound[hit])]) if hit.size else 0
        print(f"{name} sum: {int(want_set.sum())} leaves, max abs err {err.max() if err.size else 0:.3g}; closest to its bound: cell "
              f"{worst}, err {err[worst]:.3g} of {bound[worst]:.3g} ({int(c[worst])} samples)")
        assert (err <= bound).all(), f"{name}: summed weight off by more than its bound at cells {np.nonzero(err > bound)[0][:5]}"


def _c2ws(n, dev):
    return torch.from_numpy(np.stack([P.camera(i) for i in range(n)]) if n else np.zeros((0, 4, 4), f32)).to(dev)


# ---- weights: cameras ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("fast", (False, True))
@pytest.mark.parametrize("name,n_cams", [("shell1", 1), ("shell1", 3), ("chunked16", 3)])
def test_weight_accum_cams(name, n_cams, fast, op):
    """37 x 29 = 1,073 rays per camera: the last block is partial, and with three cameras a block's rays cross a camera boundary."""
    oops = _oops(); dev = _gpu()
    t = P.case_tree(name)
    view, keep = _device_tree(t, dev)
    got = oops.octree_weight_accum_cams(view, _c2ws(n_cams, dev), P.CAM_W, P.CAM_H, P.CAM_FX, _opts(P.options(name, fast)), op,
                                        fy=P.CAM_FY)
    _check_weights(f"cams {name} n{n_cams} fast{int(fast)}", got, P.camera_case(name, n_cams, fast), op, t.child)


@pytest.mark.parametrize("op", OPS)
def test_weight_accum_no_cameras_and_union_of_calls(op):
    """n_cams = 0 launches nothing and leaves the buffer as it is.  Camera 0, then cameras 1 and 2, into one buffer equal one
    call over all three: bit for bit for max (the order cannot matter), within the sum bound for sum."""
    oops = _oops(); dev = _gpu()
    t = P.case_tree("shell1")
    view, keep = _device_tree(t, dev)
    opts = _opts(P.options("shell1", False))
    args = (P.CAM_W, P.CAM_H, P.CAM_FX, opts, op)
    buf = torch.full((t.n_internal * 8,), 0.25, device=dev)
    oops.octree_weight_accum_cams(view, _c2ws(0, dev), *args, weights=buf, fy=P.CAM_FY)
    assert bool((buf == 0.25).all())
    c2ws = _c2ws(3, dev)
    whole = oops.octree_weight_accum_cams(view, c2ws, *args, fy=P.CAM_FY)
    parts = oops.octree_weight_accum_cams(view, c2ws[:1], *args, fy=P.CAM_FY)
    again = oops.octree_weight_accum_cams(view, c2ws[1:], *args, weights=parts, fy=P.CAM_FY)
    assert again.data_ptr() == parts.data_ptr()
    if op == "max":
        assert torch.equal(whole, parts)
    _check_weights("cams shell1 1+2", parts, P.camera_case("shell1", 3, False), op, t.child)


# ---- weights: explicit rays ------------------------------------------------------------------------------------------
def _rays(name, lo, hi, dev):
    o, d = P.ray_set(name)
    return torch.from_numpy(o[lo:hi].copy()).to(dev), torch.from_numpy(d[lo:hi].copy()).to(dev)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("B", P.BATCHES)
def test_weight_accum_rays_batch_sizes(B, op):
    """B = 0 (no launch), 1, and one below / at / above a block of 256; the first 13 rays are the edge rays (corner, away and
    miss write nothing)."""
    oops = _oops(); dev = _gpu()
    t = P.case_tree("shell1")
    view, keep = _device_tree(t, dev)
    o, d = _rays("shell1", 0, B, dev)
    got = oops.octree_weight_accum_rays(view, o, d, _opts(P.options("shell1", False)), op)
    _check_weights(f"rays shell1 B{B}", got, P.ray_case("shell1", 0, B, False), op, t.child)
    if B == 0:
        assert not bool(got.any())


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("fast", (False, True))
@pytest.mark.parametrize("name", ["shell1", "chunked16", "rod1"])
def test_weight_accum_rays_trees(name, fast, op):
    """Every ray of the set: sigma at offset 3 (K = 1) and 48 (K = 16); the depth-10 rod with its axis rays (kMaxD, the deepest
    stack entry) at ROD_STEP; exact and early-stop options."""
    oops = _oops(); dev = _gpu()
    t = P.case_tree(name)
    view, keep = _device_tree(t, dev)
    n = len(P.ray_set(name)[0])
    o, d = _rays(name, 0, n, dev)
    got = oops.octree_weight_accum_rays(view, o, d, _opts(P.options(name, fast)), op)
    _check_weights(f"rays {name} fast{int(fast)}", got, P.ray_case(name, 0, n, fast), op, t.child)


@pytest.mark.parametrize("op", OPS)
def test_weight_accum_rays_union_of_calls(op):
    oops = _oops(); dev = _gpu()
    t = P.case_tree("shell1")
    view, keep = _device_tree(t, dev)
    opts = _opts(P.options("shell1", False))
    o, d = _rays("shell1", 0, 257, dev)
    whole = oops.octree_weight_accum_rays(view, o, d, opts, op)
    parts = oops.octree_weight_accum_rays(view, o[:100].contiguous(), d[:100].contiguous(), opts, op)
    oops.octree_weight_accum_rays(view, o[100:].contiguous(), d[100:].contiguous(), opts, op, weights=parts)
    if op == "max":
        assert torch.equal(whole, parts)
    _check_weights("rays shell1 100+157", parts, P.ray_case("shell1", 0, 257, False), op, t.child)


def _sg_lobes(K):
    rs = np.random.RandomState(17)
    mu = rs.randn(K, 3)
    mu /= np.linalg.norm(mu, axis=1, keepdims=True)
    return np.concatenate([1.0 + 4.0 * rs.rand(K, 1), mu], 1).astype(f32)


@pytest.mark.parametrize("op", OPS)
def test_weight_accum_sg_tree_through_the_renderer(op):
    """An SG4 tree (data_dim 13) through VolumeRenderer.forward inside accumulate_weights: sigma is read at the row's last float,
    no lobes are needed, and the colours are bitwise those rendered outside the block."""
    svox = _svox(); dev = _gpu()
    t = P.case_tree("sg4")
    tree = _svox_tree(t, dev, fmt="SG4", extra=_sg_lobes(4))
    n = len(P.ray_set("sg4")[0])
    o, d = _rays("sg4", 0, n, dev)
    r = svox.VolumeRenderer(tree, step_size=P.STEP)
    with torch.no_grad():
        outside = r.forward(o, d, d)
        with tree.accumulate_weights(op=op) as accum:
            inside = r.forward(o, d, d)
    assert torch.equal(inside, outside)
    assert tuple(accum.value.shape) == (t.n_internal, 2, 2, 2)
    _check_weights("rays sg4", accum.value, P.ray_case("sg4", 0, n, False), op, t.child)


# ---- weights: NDC ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("mode", ("rays", "cams"))
def test_weight_accum_ndc(mode, op):
    """_octree_ndc_oracle's set-up.  rays: camera B's 140 rays and five with d_z >= 0, which are misses and write nothing;
    cams: cameras A (every NDC ray parallel to z) and B in one launch."""
    oops = _oops(); dev = _gpu()
    t = P.ndc_tree()
    view, keep = _device_tree(t, dev)
    opts, ndc = _opts(T.RenderOptions(P.STEP)), N.Ndc()
    lw, misses = P.ndc_case(mode)
    if mode == "rays":
        o, d = P.ndc_rays()
        assert misses >= 5 and (d[-5:, 2] >= 0).all()
        od, dd = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        got = oops.octree_weight_accum_rays(view, od, dd, opts, op, ndc=ndc)
        only_misses = oops.octree_weight_accum_rays(view, od[-5:].contiguous(), dd[-5:].contiguous(), opts, op, ndc=ndc)
        assert not bool(only_misses.any())
    else:
        c2ws = torch.from_numpy(np.stack([N.camera_a(), N.camera_b()])).to(dev)
        got = oops.octree_weight_accum_cams(view, c2ws, N.W, N.H, N.FX, opts, op, ndc=ndc)
    _check_weights(f"ndc {mode}", got, lw, op, t.child)


def test_weight_accum_refusals():
    import ctypes
    from plenoctree_amd import _lib
    oops = _oops(); dev = _gpu()
    t = P.case_tree("shell1")
    view, keep = _device_tree(t, dev)
    opts = _opts(P.options("shell1", False))
    o, d = _rays("shell1", 0, 4, dev)
    w = torch.zeros(t.n_internal * 8, device=dev)
    lib = _lib.load()
    st, f = oops._stream(), oops._f
    c2w = _c2ws(1, dev)[:, :3, :4].contiguous()
    rays = lambda op, B=4, weights=w, origins=o: lib.pxo_octree_weight_accum_rays(
        ctypes.byref(view), None if origins is None else f(origins), f(d), B, ctypes.byref(opts), op, f(weights), st, None)
    cams = lambda op, n=1, ptr=c2w: lib.pxo_octree_weight_accum_cams(
        ctypes.byref(view), None if ptr is None else f(ptr), n, 30.0, 30.0, 8, 6, ctypes.byref(opts), op, f(w), st, None)
    for bad, what in ((lambda: rays(2), "op 2"), (lambda: rays(-1), "op -1"), (lambda: cams(2), "op 2"),
                      (lambda: cams(0, n=-1), "n_cams -1"), (lambda: rays(0, weights=None), "null weights"),
                      (lambda: rays(0, origins=None), "null ray arrays"), (lambda: cams(0, ptr=None), "null c2w_all"),
                      (lambda: rays(0, B=-1), "B < 0")):
        assert bad() == -1, what                                       # PXO_ERR_ARG
        assert b"pxo_octree_weight_accum_" in lib.pxo_last_error(), (what, lib.pxo_last_error())     # refused by name
    assert rays(2, B=0) == -1                                          # a bad op is refused with no work as well
    assert rays(0, B=0, weights=None, origins=None) == 0 and cams(1, n=0, ptr=None) == 0      # no work: OK without a launch
    with pytest.raises(oops.PxoError, match="neither 'sum' nor 'max'"):
        oops.octree_weight_accum_rays(view, o, d, opts, "mean")
    torch.cuda.synchronize()
    assert not bool(w.any())


# ---- collapse --------------------------------------------------------------------------------------------------------
def _collapse_and_check(name, t, keep, view_spec, step, dev):
    """Device collapse == restatement on all four arrays, then the device render of the collapsed tree against the oracle's
    render of the same collapsed tree at atol 2e-5.  Returns (collapsed oracle tree, old2new)."""
    oops = _oops()
    child, pd, data = (torch.from_numpy(a).to(dev) for a in (t.child, t.parent_depth, t.data))
    got = oops.tree_collapse(child, pd, data, torch.from_numpy(np.ascontiguousarray(keep)).to(dev))
    ct, old2new = P.collapsed_tree(t, keep)
    names = ("child", "parent_depth", "data", "old2new")
    want = (ct.child, ct.parent_depth, ct.data, old2new)
    for nm, g, w_ in zip(names, got, want):
        g = g.cpu().numpy()
        assert g.shape == w_.shape and g.dtype == w_.dtype, (name, nm, g.shape, w_.shape, g.dtype, w_.dtype)
        assert np.array_equal(g, w_), f"{name}: {nm} differs from the restatement"
    assert P.valid_tree(ct.child, ct.parent_depth)
    opt = T.RenderOptions(step)
    V = view_spec
    view = oops.tree_view(got[0], got[2], t.offset, t.invradius)
    im = oops.octree_render_persp(view, torch.from_numpy(V["c2w"]).to(dev), V["W"], V["H"], V["fx"], _opts(opt), fy=V["fy"])
    ref = T.render_persp(ct, V["c2w"], V["W"], V["H"], V["fx"], opt, fy=V["fy"])
    print(f"{name}: {t.n_internal} -> {ct.n_internal} nodes; render max abs err "
          f"{float(np.abs(im.cpu().numpy() - ref).max()):.3g}")
    close(f"{name} render of the collapsed tree", im, torch.from_numpy(ref), rtol=0, atol=2e-5)
    return ct, old2new


NEST_VIEW = dict(c2w=C.look_at((2.9, 2.3, 2.1), target=(0.0, 0.0, 0.0)), W=13, H=11, fx=11.0, fy=12.5)


def _nest(seed=3):
    t = P.nest_tree(K=1, seed=seed)
    t.data[..., -1] = np.abs(t.data[..., -1]) * 3.0
    return t


def test_collapse_nothing_dead_is_the_identity():
    dev = _gpu()
    t = C.make_tree("shell", 6, 1)
    ct, old2new = _collapse_and_check("nothing dead", t, np.ones((t.n_internal, 8), bool), C.CAMERA_VIEWS[0], P.STEP, dev)
    assert np.array_equal(ct.child, t.child) and np.array_equal(ct.data, t.data) and np.array_equal(old2new, np.arange(t.n_internal))


def test_collapse_everything_dead_leaves_the_root():
    dev = _gpu()
    t = C.make_tree("shell", 6, 1)
    ct, old2new = _collapse_and_check("everything dead", t, np.zeros((t.n_internal, 8), bool), C.CAMERA_VIEWS[0], P.STEP, dev)
    assert ct.n_internal == 1 and not ct.child.any() and not ct.data.any() and (old2new[1:] == -1).all() and old2new[0] == 0


def test_collapse_cascade_and_seven_dead_siblings():
    dev = _gpu()
    t = _nest()
    ct, old2new = _collapse_and_check("cascade", t, P.nest_keep_cascade(t), NEST_VIEW, P.STEP, dev)
    assert np.array_equal(old2new, [0, -1, -1, -1, 1])
    ct, old2new = _collapse_and_check("seven dead", t, P.seven_dead_keep(t), NEST_VIEW, P.STEP, dev)
    assert np.array_equal(old2new, np.arange(5)) and np.array_equal(ct.child, t.child)
    assert np.count_nonzero(np.abs(ct.data.reshape(-1, 8, 4)[3]).sum(-1)) == 1


def test_collapse_tree_not_in_level_order():
    """A shallow leaf split with _refine_packed after deeper nodes exist: the new depth-2 node sits behind the depth-6 ones,
    and the mark pass still finds it by its stored depth."""
    dev = _gpu()
    tree = _svox_tree(C.make_tree("shell", 6, 1), dev)
    shallow = torch.nonzero((tree.child.view(-1) == 0) & (tree.parent_depth[:, 1].repeat_interleave(8) == 1)).reshape(-1)[:2]
    assert tree._refine_packed(shallow) == 2 and not tree._level_order
    t = _oracle_tree(tree)
    assert (np.diff(t.parent_depth[:, 1]) < 0).any()
    keep = np.random.RandomState(8).rand(t.n_internal, 8) < 0.25
    keep[-1] = False                                              # one of the late shallow nodes dies whole ...
    keep[-2, 3] = True                                            # ... the other keeps one leaf
    ct, old2new = _collapse_and_check("not level order", t, keep, C.CAMERA_VIEWS[1], P.STEP, dev)
    assert old2new[-1] == -1 and old2new[-2] == ct.n_internal - 1 and ct.n_internal < t.n_internal


def test_collapse_rod_keeps_the_axis():
    """Depth-10 rod, every leaf the axis rays do not sample dead: the rod's own depth-10 chain survives, everything beside it
    folds up, and a camera looking along the rod renders the collapsed tree as the oracle does."""
    dev = _gpu()
    t = C.make_tree("rod", 10, 1)
    opt = T.RenderOptions(C.ROD_STEP)
    on_axis = sorted(C.sampled_leaves(t, *C.rod_axis_rays(t), opt))
    keep = np.zeros(t.n_internal * 8, bool)
    keep[on_axis] = True
    view = dict(C.rod_view(t), W=2, H=1)
    ct, old2new = _collapse_and_check("rod", t, keep.reshape(-1, 8), view, C.ROD_STEP, dev)
    assert int(ct.parent_depth[:, 1].max()) == 10 and ct.n_internal < t.n_internal
    print(f"rod: {t.n_internal} -> {ct.n_internal} nodes")


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_prune_by_own_weights_is_bit_identical_without_collapse_and_matches_the_oracle_with():
    """max weights over a tree's own cameras through accumulate_weights around render_persp; prune_(weights > 0, collapse=False)
    must leave the same cameras' images bit-identical (a leaf with weight exactly 0 contributed exactly 0, and the sample
    sequence does not depend on data): the kernel's weight is the renderer's weight.  The rgb rendered inside the block is
    bitwise the rgb rendered outside.  With collapse the sample phase shifts where empty octants merge, so the images are held
    to the oracle on the collapsed tree instead (atol 2e-5); the difference to the uncollapsed image is printed."""
    svox = _svox(); dev = _gpu()
    t = C.make_tree("chunked", 6, 16)
    tree = _svox_tree(t, dev)
    r = svox.VolumeRenderer(tree, step_size=P.STEP)
    views = C.CAMERA_VIEWS
    render = lambda rr, V: rr.render_persp(torch.from_numpy(V["c2w"]), width=V["W"], height=V["H"], fx=V["fx"], fy=V["fy"])
    with torch.no_grad():
        before = [render(r, V) for V in views]
        with tree.accumulate_weights("max") as accum:
            inside = [render(r, V) for V in views]
        assert all(torch.equal(a, b) for a, b in zip(before, inside))
        keep = accum.value > 0
        assert 0 < int(keep.sum()) < int((tree.child == 0).sum())
        collapsed = tree.clone()
        assert tree.prune_(keep, collapse=False) == 0
        zeroed = int(((tree.data.data.abs().sum(-1) == 0) & (tree.child == 0)).sum())
        assert zeroed >= int(((tree.child == 0) & ~keep).sum()) > 0
        after = [render(r, V) for V in views]
        assert all(torch.equal(a, b) for a, b in zip(before, after))
        removed = collapsed.prune_(keep, collapse=True)
        assert removed > 0 and collapsed.n_internal == tree.n_internal - removed and collapsed._level_order == tree._level_order
        assert collapsed.level_nodes == np.bincount(collapsed.parent_depth[:, 1].cpu().numpy()).tolist()
        ct = _oracle_tree(collapsed)
        assert P.valid_tree(ct.child, ct.parent_depth)
        rc = svox.VolumeRenderer(collapsed, step_size=P.STEP)
        opt = T.RenderOptions(P.STEP)
        for V, ref_im in zip(views, before):
            im = render(rc, V)
            want = T.render_persp(ct, V["c2w"], V["W"], V["H"], V["fx"], opt, fy=V["fy"])
            close("collapsed render", im, torch.from_numpy(want), rtol=0, atol=2e-5)
            print(f"collapse removed {removed} of {tree.n_internal} nodes; image difference to the uncollapsed tree "
                  f"{float((im - ref_im).abs().max()):.3g}")


def test_accumulate_weights_on_the_differentiable_path():
    """render_persp with a tree that requires grad launches the weight kernel too; image and gradient are those without it."""
    svox = _svox(); dev = _gpu()
    t = C.make_tree("shell", 6, 1)
    V = C.CAMERA_VIEWS[0]
    c2w = torch.from_numpy(V["c2w"])
    outs = []
    for use in (False, True):
        tree = _svox_tree(t, dev)
        tree.data.requires_grad_(True)
        r = svox.VolumeRenderer(tree, step_size=P.STEP)
        if use:
            with tree.accumulate_weights("sum") as accum:
                im = r.render_persp(c2w, width=V["W"], height=V["H"], fx=V["fx"], fy=V["fy"])
        else:
            im = r.render_persp(c2w, width=V["W"], height=V["H"], fx=V["fx"], fy=V["fy"])
        (im * im).sum().backward()
        outs.append((im.detach(), tree.data.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    close("gradient with the accumulator active", outs[1][1], outs[0][1], rtol=1e-5, atol=1e-7)      # atomics: order only
    o, d = T.camera_rays(**V)
    lw = P.leaf_weights(t, P.march_rays(t, o, d, P.STEP), T.RenderOptions(P.STEP))
    _check_weights("differentiable path", accum.value, lw, "sum", t.child)


def test_pruning_cli_end_to_end(tmp_path):
    """Fixed-weight checkpoint with a known non-trivial density -> nerf_sh.train for a few steps -> octree.extraction at depth 4
    -> octree.pruning (with --eval) -> its output loads, has no more nodes than the input, and octree.evaluation and one epoch
    of octree.optimization accept it; --refine_thresh gives a tree with more leaves whose render matches the oracle on it."""
    dev = _gpu()
    from plenoctree_amd.nerf_sh import train
    from plenoctree_amd.nerf_sh.nerf import checkpoints, datasets, models, utils
    from plenoctree_amd.octree import evaluation, extraction, optimization, pruning, svox
    d = str(tmp_path)
    cfg_path = os.path.join(d, "tiny.yaml")
    with open(cfg_path, "w") as f:
        f.write("dataset: synthetic\nfactor: 16\nnum_coarse_samples: 64\nnum_fine_samples: 128\nuse_viewdirs: false\n"
                "white_bkgd: true\nbatch_size: 1024\nsh_deg: 3\nrandomized: true\nmax_steps: 8\nprint_every: 4\nsave_every: 8\n"
                "render_every: 0\n")
    common = ["--train_dir", d, "--config", cfg_path, "--synthetic_hw", "40", "40", "--synthetic_views", "3", "2"]
    args = utils.define_flags().parse_args(common)
    utils.update_flags(args)
    model, _ = models.construct_nerf(args, dev)
    checkpoints.save_checkpoint(d, models.TrainState(model.cfg, make_params(O.Cfg(), seed=11, bias_scale=0.2).to(dev)), step=0)
    trace = train.main(common)
    assert len(trace) == 2 and all(np.isfinite(s[1]) for s in trace) and os.path.exists(os.path.join(d, "checkpoint_8"))
    src = os.path.join(d, "tree.npz")
    tree = extraction.main(common + ["--output", src, "--init_grid_depth", "4", "--masking_mode", "sigma", "--samples_per_cell", "8",
                                     "--renderer_step_size", "1e-3", "--eval", "false"])
    assert tree.n_internal > 20
    out = os.path.join(d, "tree_pruned.npz")
    before, after = pruning.main(common + ["--input", src, "--output", out, "--renderer_step_size", "1e-3", "--eval", "true"])
    pruned = svox.N3Tree.load(out, map_location=dev)
    assert before[0] == tree.n_internal and after[0] == pruned.n_internal <= tree.n_internal and after[2] <= before[2]
    assert str(pruned.data_format) == "SH16" and P.valid_tree(pruned.child.cpu().numpy(), pruned.parent_depth.cpu().numpy())
    print(f"octree.pruning: nodes {before[0]} -> {after[0]}, leaves {before[1]} -> {after[1]}, bytes {before[2]} -> {after[2]}")
    # --no_collapse keeps the structure
    same = os.path.join(d, "tree_zeroed.npz")
    b2, a2 = pruning.main(common + ["--input", src, "--output", same, "--renderer_step_size", "1e-3", "--no_collapse"])
    assert a2 == b2 and torch.equal(svox.N3Tree.load(same, map_location=dev).child, tree.child)
    psnr = evaluation.main(common + ["--input", out, "--renderer_step_size", "1e-3"])
    assert np.isfinite(psnr)
    hist = optimization.main(common + ["--input", out, "--output", os.path.join(d, "tree_pruned_opt.npz"), "--num_epochs", "1",
                                       "--val_interval", "1", "--renderer_step_size", "1e-3", "--lr", "2e4",
                                       "--continue_on_decrease"])
    assert len(hist) == 2 and all(np.isfinite(h[2]) for h in hist)
    split = os.path.join(d, "tree_split.npz")
    _, a3 = pruning.main(common + ["--input", src, "--output", split, "--renderer_step_size", "1e-3", "--refine_thresh", "0.05"])
    refined = svox.N3Tree.load(split, map_location=dev)
    assert refined.n_leaves == a3[1] > pruned.n_leaves
    assert refined.depth_limit == tree.depth_limit + 1 == refined.max_depth       # the split went one level below the extraction's
    train_set = datasets.get_dataset("train", args, dev)
    rt = _oracle_tree(refined)
    assert P.valid_tree(rt.child, rt.parent_depth)
    W, H, fx = 16, 12, train_set.focal * 16 / train_set.w
    seen = 0.0
    for c2w in train_set.camtoworlds:                             # the cameras the weights came from: 16 x 12 views of each
        c2w = np.ascontiguousarray(c2w[:3, :4]).astype(f32)
        with torch.no_grad():
            im = svox.VolumeRenderer(refined, step_size=1e-3).render_persp(torch.from_numpy(c2w), width=W, height=H, fx=fx)
        want = T.render_persp(rt, c2w, W, H, fx, T.RenderOptions(1e-3))
        seen = max(seen, float(np.abs(want - 1.0).max()))
        close("render of the refined tree", im, torch.from_numpy(want), rtol=0, atol=2e-5)
    assert seen > 1e-3, seen                                      # leaves of weight >= 0.05 were split: some view sees them
