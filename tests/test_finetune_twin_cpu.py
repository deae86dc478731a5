"""CPU conditions that keep tests/test_gpu_octree_finetune.py honest, on the float64 twin alone (tests/_finetune_twin.py): the
recorded float32 floors are what the oracle measures today, every case moves the data far beyond the bounds the GPU test
derives from them, the sigma threshold is part of what is compared, no decision of the epoch loop is a coin flip, and the
image_mse inputs hold the values their test speaks of.  No code under test runs here."""
import numpy as np
import pytest
import torch

import _finetune_twin as F

CASE_IDS = [f"{c}-{m}" for c, m in F.CASE_MODES]


@pytest.mark.parametrize("name,mode", F.CASE_MODES, ids=CASE_IDS)
def test_recorded_floor_and_signal(name, mode):
    c = F.case(name)
    rel, dloss = F.measure_floor(name, mode)
    want_rel, want_dloss = F.FLOOR[name, mode]
    print(f"{name} {mode}: float32 twin vs float64 twin, relative L2 of the move {rel:.3g} (recorded {want_rel:.3g}), "
          f"loss {dloss:.3g} (recorded {want_dloss:.3g})")
    assert rel <= want_rel and dloss <= want_dloss
    d64, sse64, g64 = F.steps64(name, mode)
    rel_bound, atol, sse_bound = F.bounds(name, mode, d64[-1])
    move = d64[-1] - F.start(c)
    # the move is >= 1000 x what the GPU test allows: in L2 (the bound is relative to the move, so this is a statement about the
    # floor), elementwise, and against the float32 spacing of the data itself
    assert float(move.norm()) >= 1000.0 * rel_bound * float(move.norm()) and rel_bound <= 1e-3
    assert float(move.abs().max()) >= 1000.0 * atol
    assert float(move.abs().max()) >= 1000.0 * 2.0 ** -24 * float(F.start(c).abs().max())
    # the loss answers to the steps by far more than its bound: each view's loss changes between its first two visits
    n_views = len(c.gt["train"])
    for j in range(n_views):
        assert abs(sse64[j + n_views] - sse64[j]) >= 100.0 * sse_bound, (j, sse64, sse_bound)
    # every sigma of every step stays clear of the threshold by 10 x the elementwise bound: the device is on the same side
    sig = torch.cat([F.start(c)[None], d64])[..., -1]
    assert float(sig.abs().min()) >= 10.0 * atol
    # leaves no ray reaches (or whose sigma is below the threshold) exist, and so do leaves that move
    untouched = (d64 == F.start(c)[None]).all(0).all(-1)
    assert 50 <= int(untouched.sum()) <= untouched.numel() - 50
    assert not bool(g64[:, untouched].any())


def test_a_sigma_crosses_the_threshold_in_the_sh4_sgd_case():
    c = F.case("sh4")
    d64, _, g64 = F.steps64("sh4", "sgd")
    sig = torch.cat([F.start(c)[None], d64])[..., -1].reshape(F.N_STEPS + 1, -1)
    crossed = torch.nonzero(((sig[1:] > 0) != (sig[:-1] > 0)).any(0)).flatten().tolist()
    assert F.PLANTED[0] in crossed
    s = sig[:, F.PLANTED[0]]
    k = int(torch.nonzero((s[1:] > 0) != (s[:-1] > 0)).flatten()[0])
    atol = F.bounds("sh4", "sgd", d64[-1])[1]
    assert 0 < k < F.N_STEPS - 1                                   # steps before and after the crossing are compared too
    assert float(s[k]) >= 100.0 * atol and float(s[k + 1]) <= -100.0 * atol
    # once below the threshold the leaf gets no gradient: the kink, not a smooth passage
    gs = g64[..., -1].reshape(F.N_STEPS, -1)[:, F.PLANTED[0]]
    assert float(gs[k].abs()) > 0 and not bool(gs[k + 1:].any())


@pytest.mark.parametrize("mode", ["sgd", "adam"])
def test_negative_controls_differ_by_far_more_than_the_bound(mode):
    """What the GPU test must be able to see, shown on the twin: a gradient buffer that is never cleared, and (SGD) a
    grad_scale applied twice, move the result by >= 100 x the bound of the honest run."""
    c = F.case("sh4")
    d64, _, _ = F.steps64("sh4", mode)
    rel_bound = F.bounds("sh4", mode, d64[-1])[0]
    dist = lambda d, k: float((d[k] - d64[k]).norm() / (d64[k] - F.start(c)).norm())
    stale, _, _ = F.twin_steps(c, mode, F.LR["sh4", mode], F.N_STEPS, torch.float64, zero_grad=False)
    assert torch.equal(stale[0], d64[0])                            # the first step has nothing stale to add
    for k in range(1, F.N_STEPS):
        assert dist(stale, k) >= 100.0 * rel_bound, (k, dist(stale, k), rel_bound)
    if mode == "sgd":
        half, _, _ = F.steps64("sh4", mode, grad_scale=0.5)
        quarter, _, _ = F.twin_steps(c, mode, F.LR["sh4", mode], F.N_STEPS, torch.float64, grad_scale=0.25)
        at_half_lr, _, _ = F.twin_steps(c, mode, 0.5 * F.LR["sh4", mode], F.N_STEPS, torch.float64)
        for k in range(F.N_STEPS):
            assert float((half[k] - at_half_lr[k]).norm() / (half[k] - F.start(c)).norm()) <= 1e-12
            assert float((quarter[k] - half[k]).norm() / (half[k] - F.start(c)).norm()) >= 100.0 * rel_bound
            assert dist(half, k) >= 100.0 * rel_bound


@pytest.mark.parametrize("schedule", list(F.FIT))
def test_fit_schedules_decide_clearly(schedule):
    r = F.fit64(schedule)
    a = F.fit_args(schedule)
    floor = F.measure_fit_floor(schedule)
    print(f"{schedule}: float32 loop vs float64 loop, largest |mse32 - mse64| {floor[0]:.3g}, relative L2 of the move {floor[1]:.3g} "
          f"(recorded {F.FLOOR['fit', schedule]}); history {r.history}")
    assert floor[0] <= F.FLOOR["fit", schedule][0] and floor[1] <= F.FLOOR["fit", schedule][1]
    assert F.MARGIN * F.FLOOR["fit", schedule][1] <= 1e-3               # the move is >= 1000 x the bound on the returned data
    assert len(r.decisions) >= 1
    for v, best, inv_v, inv_best in r.decisions:
        assert abs(v - best) >= 100.0 * (F.psnr_bound(schedule, inv_v) + F.psnr_bound(schedule, inv_best)), (v, best)
    epochs = [h[0] for h in r.history]
    if schedule == "to_the_end":
        assert not r.stopped and epochs == [0, 2, 4] and r.best_epoch == 4
    elif schedule == "early_stop":
        assert r.stopped and epochs == [0, 1, 2, 3, 4] and epochs[-1] < a.num_epochs and r.best_epoch == 3
    elif schedule == "carry_on":
        assert not r.stopped and epochs == list(range(a.num_epochs + 1)) and r.best_epoch == 3
        assert sum(d[0] <= d[1] for d in r.decisions) == 3          # three validations that would have stopped the loop
    else:
        assert r.stopped and epochs == [0, 1] and r.best is None and r.best_epoch is None
    # the training PSNR answers to the steps: it rises by far more than its bound from epoch to epoch
    train = [(h[1], i[0]) for h, i in zip(r.history, r.inv) if h[1] is not None]
    for (x, _), (y, inv) in zip(train, train[1:]):
        assert y - x >= 100.0 * F.psnr_bound(schedule, inv)


def test_mse_inputs_hold_the_planted_values():
    for n in F.MSE_SIZES[:11]:                                       # the sizes past the cap repeat the builder of 4096 * 2048
        seen = set()
        for seed in F.mse_seeds(n):
            im, gt = F.mse_inputs(n, seed)
            assert im.dtype == np.float32 and gt.dtype == np.float32 and im.shape == gt.shape == (n,)
            assert float(im.min()) >= -0.5 and float(im.max()) <= 1.5 and float(gt.min()) >= 0.0 and float(gt.max()) <= 1.0
            where = F.mse_boundaries(n)
            assert where[0] == 0 and where[-1] == n - 1
            planted = im[where]
            seen |= {"neg" for v in planted if v < 0} | {"big" for v in planted if v > 1}
            seen |= {"+0" for v in planted if v == 0 and not np.signbit(v)} | {"-0" for v in planted if v == 0 and np.signbit(v)}
            seen |= {"1" for v in planted if v == 1}
            for i in (0, n - 1):
                assert any(im[i].tobytes() == p.tobytes() for p in F.MSE_PLANTED)
        assert seen == {"neg", "big", "+0", "-0", "1"}, (n, seen)
    # every workgroup of a multi-workgroup launch has planted values at both ends of its first stretch
    n = 2 * 2048 + 1
    assert set(F.mse_boundaries(n).tolist()) == {0, 255, 256, 511, 512, 2047, 2048, 4095, 4096}
    assert F.mse_groups(2048) == 1 and F.mse_groups(2049) == 2 and F.mse_groups(4096 * 2048 + 1) == 4096
    # the single-hot inputs: zero error everywhere but one element
    for n in (1, 2049, 2 * 2048 + 1):
        for at in F.mse_hot_positions(n):
            im, gt, e = F.mse_single_hot(n, at)
            d = np.clip(im, 0, 1) - gt
            assert np.count_nonzero(d) == 1 and d[at] == e and 0 <= at < n
    assert F.mse_hot_positions(2 * 2048 + 1) == [0, 4096, 512]
