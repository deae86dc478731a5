"""GPU tests of octree fine-tuning (plenoctree_amd/octree/optimization.py) against its float64 twin (tests/_finetune_twin.py):
the clamped-MSE kernel and the SGD kernel at the sizes where their launches change shape, TreeOptimizer step by step for every
optimiser mode and tree family, and the epoch loop's decisions.

Bounds.  image_mse and sgd_step: derived from the roundings of the float32 arithmetic (stated at each test).  The step and the
loop: MARGIN (8) x the float32 twin's own deviation from the float64 twin (F.FLOOR, measured on the CPU oracle alone and
re-measured by tests/test_finetune_twin_cpu.py); the device differs from the float32 oracle by the order of its atomic adds,
its exp / sigmoid and contraction.  Every test prints observed / bound (pytest -s).

Observed on the MI355X, worst step of each case as a fraction of its bound (move in relative L2 / elementwise / sum of squares):
sh4 sgd 0.15 / 0.06 / 0.04, momentum 0.34 / 0.10 / 0.21, nesterov 0.23 / 0.09 / 0.08, adam 0.38 / - / 0.13; sh16 sgd 0.15 / 0.07 /
0.31, momentum 0.35 / 0.08 / 0.06, nesterov 0.23 / 0.07 / 0.19, adam 0.44 / - / 0.14; sg4 sgd 0.23 / 0.09 / 0.13, adam 0.31 / - /
0.10; ndc sgd 0.21 / 0.07 / 0.16, adam 0.20 / - / 0.02; the loop's data and its PSNRs 0.13 of their bounds.
Against the autograd float32 twin's floor alone the Adam cases miss: the first step of sh4 lands at 13 times that bound, all
of it on 79 sigmas whose gradient is below Adam's eps.  The renderer's backward (svox's rule: the colour behind a sample by
subtraction) leaves them an absolute error of some 1e-11, which Adam divides by |g| + 1e-8.  The float32 twin that follows the
same rule (F._loss_backward_one_sweep, CPU only) shows the same deviation, 2.9e-4 against the device's 2.7e-4 on that step,
so the Adam floors are the larger of the two float32 twins (F.measure_floor)."""
import math

import numpy as np
import pytest
import torch

import _finetune_twin as F
from _helpers import _gpu, close
from plenoctree_amd import octree_ops as oops

pytestmark = pytest.mark.gpu
f32 = np.float32
EPS = 2.0 ** -24                                  # half a float32 spacing, relative: one rounding

# the launch of pxo_image_mse, which the sizes below are built around
assert (oops.MSE_BLOCK, oops.MSE_BLOCK * oops.MSE_PER_THREAD, oops.MSE_MAX_BLOCKS) == (256, F.MSE_GROUP, F.MSE_CAP)
assert F.MSE_SIZES[-3:] == (F.MSE_CAP * F.MSE_GROUP, F.MSE_CAP * F.MSE_GROUP + 1, F.MSE_CAP * F.MSE_GROUP + 256 * F.MSE_CAP + 3)


# ---- image_mse ------------------------------------------------------------------------------------------------------------
def _mse64(im, gt):
    """torch in float64 on the same device tensors: (sum of squares, d mean / d im)."""
    x = im.double().requires_grad_(True)
    sq = (x.clamp(0.0, 1.0) - gt.double()) ** 2
    sq.mean().backward()
    return float(sq.sum().detach()), x.grad


def _sse_bound(n):
    """(T + 8 + G) 2^-24, relative: T terms per thread summed in order, 6 shuffle steps and 2 adds in the workgroup, G atomic
    adds -- the worst case of summing non-negative float32 terms in any order."""
    G = F.mse_groups(n)
    T = -(-n // (G * oops.MSE_BLOCK))
    return (T + 8 + G) * EPS


@pytest.mark.parametrize("n", F.MSE_SIZES)
def test_image_mse_matches_float64(n):
    """Gradient: 2 / n * (clamp(v) - gt) takes three float32 roundings -- the difference, the quotient 2 / n, the product --
    so against float64 autograd it is held to 3 * 2^-24 |g64|.  Two roundings, 2 * 2^-24, are not enough for any float32
    evaluation: numpy's float32 arithmetic of the same rule is off by 2.19 * 2^-24 |g64| at n = 63.  The difference is
    exact in float64 and correctly rounded in float32, so the two-rounding bound is held as well, against
    2 / n * float64(float32(clamp(v) - gt)): the quotient and the product, which is where a kernel has freedom."""
    dev = _gpu()
    edges = 0
    for seed in F.mse_seeds(n):
        im_h, gt_h = F.mse_inputs(n, seed)
        im, gt = torch.from_numpy(im_h).to(dev), torch.from_numpy(gt_h).to(dev)
        sse64, g64 = _mse64(im, gt)
        sse, g = oops.image_mse(im, gt)
        inside = (im >= 0) & (im <= 1)
        err = (g.double() - g64).abs()
        tol = 3.0 * EPS * g64.abs() + 1e-37
        g_two = torch.where(inside, (2.0 / n) * (im.clamp(0.0, 1.0) - gt).double(), torch.zeros_like(g64))
        err_two = (g.double() - g_two).abs()
        tol_two = 2.0 * EPS * g_two.abs() + 1e-37
        worst, worst_two = float((err / tol).max()), float((err_two / tol_two).max())
        print(f"image_mse n={n} seed={seed}: gradient error / bound {worst:.3f} (three roundings), {worst_two:.3f} (two, after "
              f"the float32 difference); sse {float(sse):.9g} vs {sse64:.9g}, "
              f"error / bound {abs(float(sse) - sse64) / (_sse_bound(n) * sse64):.3f}")
        assert bool((err <= tol).all()), (n, seed, worst)
        assert bool((err_two <= tol_two).all()), (n, seed, worst_two)
        assert int(torch.count_nonzero(g[~inside])) == 0
        edge = ((im == 0) | (im == 1)) & (gt != im.clamp(0.0, 1.0))
        edges += int(edge.sum())
        assert bool((g[edge] != 0).all())                                        # the gradient passes at v == 0 and v == 1
        assert abs(float(sse) - sse64) <= _sse_bound(n) * sse64
        # validation's call: no gradient, the same sum within the same bound
        sse_v, none = oops.image_mse(im, gt, want_grad=False)
        assert none is None and abs(float(sse_v) - sse64) <= _sse_bound(n) * sse64
    assert edges >= 3                                                            # 0.0, -0.0 and 1.0 each came up


@pytest.mark.parametrize("n", F.MSE_SIZES)
def test_image_mse_drops_no_element(n):
    """All error in one element (index 0, n - 1, the first of the last workgroup): the sum is float32(e * e) exactly, with and
    without the gradient, and repeated calls return each image's own sum."""
    dev = _gpu()
    seen = []
    for at in F.mse_hot_positions(n):
        im_h, gt_h, e = F.mse_single_hot(n, at)
        im, gt = torch.from_numpy(im_h).to(dev), torch.from_numpy(gt_h).to(dev)
        want = f32(e * e)
        sse, g = oops.image_mse(im, gt)
        sse_v, _ = oops.image_mse(im, gt, want_grad=False)
        assert float(sse) == float(want) and torch.equal(sse, sse_v), (n, at, float(sse), float(sse_v), float(want))
        assert int(torch.count_nonzero(g)) == 1 and float(g[at]) == float(f32(f32(f32(2.0) / f32(n)) * e))
        seen.append((im, gt))
    # nothing accumulates from call to call: a dense image in between, then the first single-hot image again
    im_h, gt_h = F.mse_inputs(n, 0)
    dense, _ = oops.image_mse(torch.from_numpy(im_h).to(dev), torch.from_numpy(gt_h).to(dev), want_grad=False)
    again, _ = oops.image_mse(*seen[0], want_grad=False)
    assert float(again) == float(f32(e * e))
    if n > 1:
        assert float(dense) != float(again)


def test_image_mse_nan_and_inf_follow_torch():
    """A NaN pixel makes the sum NaN (a diverged tree cannot score a finite PSNR) and gets torch's gradient, zero; +-inf clamp
    to 1 / 0 with a zero gradient.  Every other element's gradient is untouched."""
    dev = _gpu()
    n = 2 * F.MSE_GROUP + 1
    im_h, gt_h = F.mse_inputs(n, 0)
    for at in (0, 300, F.MSE_GROUP, n - 1):
        for bad in (float("nan"), float("inf"), -float("inf")):
            im_b = im_h.copy(); im_b[at] = bad
            im, gt = torch.from_numpy(im_b).to(dev), torch.from_numpy(gt_h).to(dev)
            sse64, g64 = _mse64(im, gt)
            for want_grad in (True, False):
                sse, g = oops.image_mse(im, gt, want_grad=want_grad)
                if math.isnan(bad):
                    assert math.isnan(sse64) and math.isnan(float(sse)), (at, want_grad, float(sse), sse64)
                else:
                    assert abs(float(sse) - sse64) <= _sse_bound(n) * sse64
                if want_grad:
                    assert float(g[at]) == float(g64[at]) == 0.0
                    assert bool(torch.isfinite(g).all())
                    assert bool(((g.double() - g64).abs() <= 3.0 * EPS * g64.abs() + 1e-37).all())


# ---- sgd_step -------------------------------------------------------------------------------------------------------------
SGD_MODES = [(0.0, False), (0.9, False), (0.9, True)]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
@pytest.mark.parametrize("mu,nesterov", SGD_MODES, ids=["plain", "momentum", "nesterov"])
def test_sgd_step_one_step_ahead_of_float64(n, mu, nesterov):
    """Before each of 4 steps the parameters and the buffer are taken from the device, torch.optim.SGD steps them in float64,
    and the kernel's step is held to
        |d buf| <= 2^-23 (|mu buf| + |g|)           (two roundings: the product and the sum)
        |d p|   <= 2^-23 (|p| + 2 lr G),  G = the sum of the magnitudes of the terms of g_eff
    (the product, the difference and what g_eff inherits from the buffer's roundings; fma only removes roundings).  With
    mu = 0, G = |g| = |g_eff|.  With momentum, G = |mu buf| + |g| (plain) or |g| + mu (|mu buf| + |g|) (Nesterov), not
    |g_eff| itself: where mu buf and g cancel, the roundings of the buffer are not small against |g_eff|, and plain float32
    arithmetic of the same rule, on the CPU, exceeds 2^-23 (|p| + 2 lr |g_eff|) 7.6 times at n = 100003.
    lr and mu are the float32 values the kernel is handed.  The buffer starts non-zero: first_step must overwrite it."""
    dev = _gpu()
    gen = torch.Generator().manual_seed(n + int(10 * mu) + int(nesterov))
    lr32, mu32 = float(f32(0.1)), float(f32(mu))
    p = torch.randn(n, generator=gen).to(dev)
    buf = torch.randn(n, generator=gen).to(dev) if mu else None
    worst_p = worst_b = 0.0
    for step in range(4):
        g = torch.randn(n, generator=gen).to(dev)
        g_before = g.clone()
        ref = torch.nn.Parameter(p.double())
        ref.grad = g.double()
        opt = torch.optim.SGD([ref], lr=lr32, momentum=mu32, nesterov=nesterov)
        if mu and step > 0:
            opt.state[ref]["momentum_buffer"] = buf.double()
        mag_buf = (mu32 * buf.double()).abs() if (mu and step > 0) else torch.zeros(n, dtype=torch.float64, device=dev)
        p_before = p.double()
        opt.step()
        oops.sgd_step(p, g, 0.1, mu, nesterov, buf, first_step=step == 0)
        assert torch.equal(g, g_before)                                        # the gradient is read, never written
        G = g.double().abs()
        if mu:
            b64 = opt.state[ref]["momentum_buffer"]
            tol_b = 2.0 ** -23 * (mag_buf + g.double().abs())
            if step == 0:
                assert torch.equal(buf, g)                                     # buffer := g, whatever it held
            assert bool(((buf.double() - b64).abs() <= tol_b).all())
            if n:
                worst_b = max(worst_b, float(((buf.double() - b64).abs() / tol_b).max()))
            G = G + mu32 * (mag_buf + G) if nesterov else mag_buf + G
        tol_p = 2.0 ** -23 * (p_before.abs() + 2.0 * lr32 * G)
        err = (p.double() - ref.data).abs()
        if n:
            worst_p = max(worst_p, float((err / tol_p).max()))
        assert bool((err <= tol_p).all()), (step, float((err / tol_p).max()))
    print(f"sgd_step n={n} mu={mu} nesterov={nesterov}: worst |d p| / bound {worst_p:.3f}, |d buf| / bound {worst_b:.3f}")


def test_sgd_step_buffer_protocol():
    dev = _gpu()
    from plenoctree_amd._lib import PxoError
    gen = torch.Generator().manual_seed(5)
    p, g, buf = (torch.randn(257, generator=gen).to(dev) for _ in range(3))
    p0, buf0 = p.clone(), buf.clone()
    oops.sgd_step(p, g, 0.1, 0.0, False, buf)                                  # mu = 0: a supplied buffer is untouched
    assert torch.equal(buf, buf0) and not torch.equal(p, p0)
    q = p0.clone()
    oops.sgd_step(q, g, 0.1, 0.0, False, None)                                 # ... and none is needed
    assert torch.equal(q, p)
    for nesterov in (False, True):
        with pytest.raises(PxoError, match="momentum needs a buffer"):
            oops.sgd_step(q, g, 0.1, 0.9, nesterov, None)
    assert torch.equal(q, p)


# ---- the step -------------------------------------------------------------------------------------------------------------
def _device_tree(c, dev):
    """The case's tree as the existing tests build it: svox.N3Tree holding the oracle's arrays."""
    from plenoctree_amd.octree import svox
    t = c.tree
    K = (t.data_dim - 1) // 3
    radius = 0.5 / t.invradius
    host = svox.N3Tree(N=2, data_dim=t.data_dim, depth_limit=int(t.parent_depth[:, 1].max()), radius=radius,
                       center=(1.0 - 2.0 * t.offset) * radius, data_format=f"SG{K}" if c.lobes is not None else f"SH{K}",
                       extra_data=c.lobes, map_location=dev)
    assert np.array_equal(host.offset.numpy(), t.offset) and np.array_equal(host.invradius.numpy(), t.invradius)
    host.child, host.parent_depth = torch.from_numpy(t.child).to(dev), torch.from_numpy(t.parent_depth).to(dev)
    host.data = torch.nn.Parameter(torch.from_numpy(c.data0.copy()).to(dev))
    host.level_nodes = [int(v) for v in np.bincount(t.parent_depth[:, 1])]
    host._leaves = None
    return host


def _renderer(c, tree):
    from plenoctree_amd.octree import svox
    ndc = None if c.ndc is None else svox.NDCConfig(c.ndc.width, c.ndc.height, c.ndc.focal, c.ndc.near)
    return svox.VolumeRenderer(tree, step_size=1e-3, ndc=ndc)


def _views(c, split, dev):
    return torch.from_numpy(c.poses[split]).to(dev), [torch.from_numpy(g).to(dev) for g in c.gt[split]]


def _run_steps(name, mode, ref, lr=None, grad_scale=1.0, label=""):
    """N_STEPS steps of zero_grad / train_image / step on the device, each held to ref = (data, sse, gradient) of the twin."""
    from plenoctree_amd.octree import optimization
    dev = _gpu()
    c = F.case(name)
    d64, sse64, g64 = ref
    tree = _device_tree(c, dev)
    renderer = _renderer(c, tree)
    opt = optimization.TreeOptimizer(tree, F.mode_args(mode, F.LR[name, mode] if lr is None else lr))
    c2w, gt = _views(c, "train", dev)
    start = F.start(c)
    untouched = (d64 == start[None]).all(0).all(-1)
    worst = dict(rel=0.0, elem=0.0, sse=0.0)
    for k in range(F.N_STEPS):
        j = k % len(gt)
        opt.zero_grad()
        sse = optimization.train_image(renderer, opt, c2w[j], gt[j], c.H, c.W, c.fx)
        opt.step(grad_scale)
        assert opt.step_count == k + 1
        rel_bound, atol, sse_bound = F.bounds(name, mode, d64[k])
        data = tree.data.data.cpu().double()
        rel = float((data - d64[k]).norm() / (d64[k] - start).norm())
        elem = float((data - d64[k]).abs().max())
        dsse = abs(float(sse) - sse64[k])
        worst = dict(rel=max(worst["rel"], rel / rel_bound), elem=max(worst["elem"], elem / atol), sse=max(worst["sse"], dsse / sse_bound))
        print(f"{name} {mode}{label} step {k}: move rel L2 {rel:.3g} / {rel_bound:.3g}, elementwise {elem:.3g} / {atol:.3g}, "
              f"sse {float(sse):.9g} vs {sse64[k]:.9g}: {dsse:.3g} / {sse_bound:.3g}")
        assert dsse <= sse_bound, (k, dsse, sse_bound)
        assert rel <= rel_bound, (k, rel, rel_bound)
        if mode != "adam":                     # Adam in L2 only: where a gradient cancels to rounding noise, g / sqrt(v) amplifies its sign
            close(f"{name} {mode}{label} data after step {k}", data, d64[k], rtol=0, atol=atol)
        # opt.grad holds this image's gradient alone (the twin's is already scaled): the bar of the single-launch gradient tests
        want = (g64[k] / grad_scale).float()
        close(f"{name} {mode}{label} gradient of step {k}", opt.grad, want, rtol=2e-3, atol=2e-6 * float(want.abs().max()) + 1e-7)
        # leaves no ray reaches
        if mode == "adam":
            assert not bool(opt.m.cpu()[untouched].any()) and not bool(opt.v.cpu()[untouched].any())
        else:
            assert torch.equal(tree.data.data.cpu()[untouched], torch.from_numpy(c.data0)[untouched])
    print(f"{name} {mode}{label}: worst observed / bound: move rel L2 {worst['rel']:.3f}, elementwise {worst['elem']:.3f}, sse {worst['sse']:.3f}")
    return tree, opt


def test_the_twin_tree_is_the_gradient_tests_tree():
    """F.random_tree restates test_gpu_octree.py:_random_tree; the sh4 case is its (2, 34, 4, p=0.3) but for the planted sigma."""
    from test_gpu_octree import _random_tree
    t, want = F.random_tree(2, 34, 4, p=0.3), _random_tree(2, 34, 4, p=0.3)
    assert np.array_equal(t.child, want.child) and np.array_equal(t.data, want.data) and np.array_equal(t.offset, want.offset)
    got = F.case("sh4").data0.reshape(-1, 13)
    differs = np.nonzero((got != want.data.reshape(-1, 13)).any(-1))[0]
    assert differs.tolist() == [F.PLANTED[0]] and got[F.PLANTED[0], -1] == f32(F.PLANTED[1])


@pytest.mark.parametrize("name,mode", F.CASE_MODES, ids=[f"{c}-{m}" for c, m in F.CASE_MODES])
def test_steps_match_the_float64_twin(name, mode):
    _run_steps(name, mode, F.steps64(name, mode))


def test_grad_scale_sgd_is_the_twin_at_half_the_lr():
    """TreeOptimizer at twice the case's lr with grad_scale 0.5 is the twin at the case's lr, whose floor is the recorded one."""
    ref = F.steps64("sh4", "sgd")
    # _run_steps divides the twin's gradient by grad_scale to get what opt.grad holds; this twin's gradient is unscaled already
    _run_steps("sh4", "sgd", (ref[0], ref[1], 0.5 * ref[2]), lr=2.0 * F.LR["sh4", "sgd"], grad_scale=0.5, label=" grad_scale 0.5")


def test_grad_scale_adam_is_the_twin_fed_half_the_gradient():
    _run_steps("sh4", "adam", F.steps64("sh4", "adam", grad_scale=0.5), grad_scale=0.5, label=" grad_scale 0.5")


# ---- the loop -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", list(F.FIT))
def test_fit_decides_as_the_twin(schedule):
    from plenoctree_amd import dist
    from plenoctree_amd.octree import optimization
    dev = _gpu()
    c = F.case("sh4")
    want = F.fit64(schedule)
    args = F.fit_args(schedule)
    tree = _device_tree(c, dev)
    train, val = _views(c, "train", dev), _views(c, F.FIT[schedule][0], dev)
    lines = []
    history, best = optimization.fit(args, tree, train, val, c.H, c.W, c.fx, dist.Comm(),
                                     say=lambda *a, **k: lines.append(" ".join(str(x) for x in a)))
    assert [h[0] for h in history] == [h[0] for h in want.history], (history, want.history)
    for h, w, (train_inv, val_inv) in zip(history, want.history, want.inv):
        assert (h[1] is None) == (w[1] is None)
        for what, got, ref, inv in (("train", h[1], w[1], train_inv), ("val", h[2], w[2], val_inv)):
            if got is not None:
                bound = F.psnr_bound(schedule, inv)
                print(f"fit {schedule} epoch {h[0]} {what} psnr {got:.7f} vs {ref:.7f}: {abs(got - ref):.3g} / {bound:.3g}")
                assert abs(got - ref) <= bound, (h, w, bound)
    stopped = any("Stop since overfitting" in line for line in lines)
    assert stopped == want.stopped, lines
    if schedule in ("to_the_end", "carry_on"):
        assert history[-1][0] == args.num_epochs
    rel_bound = F.MARGIN * F.FLOOR["fit", schedule][1]
    start = F.start(c)
    final = tree.data.data.cpu().double()
    rel = float((final - want.final).norm() / (want.final - start).norm())
    print(f"fit {schedule}: final data, move rel L2 {rel:.3g} / {rel_bound:.3g}")
    assert rel <= rel_bound
    if want.best is None:
        assert best is None
        return
    assert best is not tree and best.data.device.type == "cpu" and best.child.device.type == "cpu"
    assert torch.equal(best.child, tree.child.cpu())
    rel = float((best.data.data.double() - want.best).norm() / (want.best - start).norm())
    print(f"fit {schedule}: best data (epoch {want.best_epoch}), move rel L2 {rel:.3g} / {rel_bound:.3g}")
    assert rel <= rel_bound
    # ... and it is the device data as it was after that epoch: the same number of steps by hand
    hand = _device_tree(c, dev)
    renderer = _renderer(c, hand)
    opt = optimization.TreeOptimizer(hand, args)
    for _ in range(want.best_epoch):
        for j in range(len(train[1])):
            opt.zero_grad()
            optimization.train_image(renderer, opt, train[0][j], train[1][j], c.H, c.W, c.fx)
            opt.step(1.0)
    by_hand = hand.data.data.cpu().double()
    rel = float((best.data.data.double() - by_hand).norm() / (by_hand - start).norm())
    print(f"fit {schedule}: best data against {want.best_epoch} epochs by hand, move rel L2 {rel:.3g} / {rel_bound:.3g}")
    assert rel <= rel_bound                              # two device runs differ by the order of their atomic adds only
    if want.best_epoch < history[-1][0]:                 # the loop went on: the snapshot is a copy, not the live tree
        assert float((final - by_hand).norm() / (by_hand - start).norm()) >= 1000.0 * rel_bound
