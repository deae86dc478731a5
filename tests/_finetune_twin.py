"""The float64 twin of octree fine-tuning (plenoctree_amd/octree/optimization.py; reference octree/optimization.py:176-243) and
the cases it is run on.  Shared by tests/test_finetune_twin_cpu.py (the conditions that keep the GPU tests honest, on the twin
alone) and tests/test_gpu_octree_finetune.py (the HIP path against the twin).  Nothing here touches the GPU or the code under
test: the renders are oracle/octree_oracle.py:render_rays_torch (SH, SG with lobes, NDC), the optimisers are torch.optim.SGD
and torch.optim.Adam.

The oracle's march (the sample sequence of a ray) depends on the tree's structure only, never on its data, so a case marches
every ray of a view once (Case.marches) and hands the marches to every render of that view.
"""
import functools
import math
import types

import numpy as np
import torch

import _octree_ndc_oracle as N
import _octree_sg_cases as G
from _octree_cases import pose, random_tree
from oracle import octree_oracle as T

f32 = np.float32
N_STEPS = 6                       # optimiser steps of every per-step case: two passes over three views, three over two
MODES = ("sgd", "momentum", "nesterov", "adam")
MOMENTUM = 0.9

# ---- recorded floors ------------------------------------------------------------------------------------------------------
# FLOOR[case, mode] = (relative L2 distance of the float32 twin's total move from the float64 twin's after N_STEPS steps,
#                      largest per-step |loss32 - loss64|), loss = the mean squared error of the step's image before the step.
# The oracle's own float32 deviation: no code under test enters it.  The Adam entries are the larger of two float32 twins,
# autograd's and the one-sweep backward's (measure_floor says why).  Measured on the CPU on 2026-10-20 with
#     PYTHONPATH=.:tests python tests/_finetune_twin.py
# and written down rounded up to two digits; tests/test_finetune_twin_cpu.py measures them again and holds them to these.
# FLOOR["fit", schedule] = the same two of the epoch loop (measure_fit_floor), the loss first: (largest |mse32 - mse64| over
# every image the loop scores, relative L2 of the total move).  At the loop's lr the move is fifty times that of the step
# cases, so the rounding of the stored float32 data, which sets the floor of the step cases, no longer shows.
FLOOR = {
    ("sh4", "sgd"): (2.5e-05, 1.6e-09),      # measured 2.44e-05, 1.55e-09
    ("sh4", "momentum"): (2.9e-05, 1.2e-09),      # measured 2.80e-05, 1.19e-09
    ("sh4", "nesterov"): (2.4e-05, 2.4e-09),      # measured 2.35e-05, 2.31e-09
    ("sh4", "adam"): (9.1e-05, 7.4e-09),      # measured 9.01e-05, 7.40e-09 (autograd twin alone: 2.57e-06, 1.42e-09)
    ("sh16", "sgd"): (4.5e-05, 1.2e-09),      # measured 4.43e-05, 1.16e-09
    ("sh16", "momentum"): (6.5e-05, 5.9e-09),      # measured 6.46e-05, 5.87e-09
    ("sh16", "nesterov"): (5.3e-05, 2.5e-09),      # measured 5.27e-05, 2.48e-09
    ("sh16", "adam"): (2.9e-05, 6.7e-09),      # measured 2.81e-05, 6.66e-09 (autograd twin alone: 1.91e-06, 2.17e-09)
    ("sg4", "sgd"): (4.0e-05, 9.7e-10),      # measured 3.91e-05, 9.67e-10
    ("sg4", "adam"): (3.0e-05, 7.5e-09),      # measured 2.93e-05, 7.50e-09 (autograd twin alone: 2.64e-06, 7.76e-10)
    ("ndc", "sgd"): (2.9e-05, 6.0e-10),      # measured 2.89e-05, 5.95e-10
    ("ndc", "adam"): (2.9e-06, 2.3e-09),      # measured 2.80e-06, 2.21e-09 (autograd twin alone: 2.23e-06, 5.95e-10)
    ("fit", "to_the_end"): (2.4e-09, 6.3e-07),      # measured 2.30e-09, 6.30e-07
    ("fit", "early_stop"): (2.4e-09, 6.3e-07),      # measured 2.30e-09, 6.30e-07
    ("fit", "carry_on"): (2.4e-09, 6.1e-07),      # measured 2.30e-09, 6.05e-07
    ("fit", "no_gain"): (2.4e-09, 6.7e-07),      # measured 2.30e-09, 6.67e-07
}
# lr per (case, mode): the twin's data moves by some 1e-1 in N_STEPS steps (tests/test_finetune_twin_cpu.py holds the move
# against the bounds of the GPU test)
LR = {
    ("sh4", "sgd"): 20.0, ("sh4", "momentum"): 5.0, ("sh4", "nesterov"): 5.0, ("sh4", "adam"): 1e-2,
    ("sh16", "sgd"): 20.0, ("sh16", "momentum"): 5.0, ("sh16", "nesterov"): 5.0, ("sh16", "adam"): 1e-2,
    ("sg4", "sgd"): 20.0, ("sg4", "adam"): 1e-2,
    ("ndc", "sgd"): 100.0, ("ndc", "adam"): 1e-2,
}
MARGIN = 8.0                      # the GPU tests' bounds are MARGIN x FLOOR (atomic order, exp / sigmoid, contraction)


def mode_args(mode, lr, **kw):
    """The argument namespace of optimization.TreeOptimizer / fit for an optimiser mode."""
    a = dict(sgd=mode != "adam", lr=float(lr), sgd_momentum=0.0 if mode in ("sgd", "adam") else MOMENTUM,
             sgd_nesterov=mode == "nesterov", renderer_step_size=1e-3, num_epochs=1, val_interval=1,
             continue_on_decrease=False, dp_grad_reduce="mean", render_interval=0)
    a.update(kw)
    return types.SimpleNamespace(**a)


# ---- cases ----------------------------------------------------------------------------------------------------------------
class Case:
    """tree: the oracle tree (its .data is the start); lobes / ndc: None or what the oracle takes for an SG tree / an NDC scene;
    poses, gt, rays, marches per split ("train", "val", "val_mid", "val_back"): c2w [n,3 or 4,4] float32, float32 [H,W,3]
    images, (origins, dirs) per view, and per view the oracle's march of every ray."""

    def __init__(self, name, family, tree, W, H, fx, lobes=None, ndc=None):
        self.name, self.family, self.tree, self.W, self.H, self.fx, self.lobes, self.ndc = name, family, tree, W, H, fx, lobes, ndc
        self.opt = T.RenderOptions(1e-3)
        self.data0 = tree.data.copy()
        self.poses, self.gt, self.rays, self.marches = {}, {}, {}, {}

    @property
    def n(self):
        return self.H * self.W * 3

    def add_views(self, split, poses, target, rays_of=None):
        """Views whose ground truth is the float64 render of the tree holding `target`, rounded to float32."""
        rays_of = rays_of or split
        if rays_of not in self.rays:
            self.rays[rays_of] = [T.camera_rays(c, self.W, self.H, self.fx) for c in poses]
            self.marches[rays_of] = [[T.march(self.tree, o, d, self.opt.step_size, ndc=self.ndc) for o, d in zip(*rays)]
                                     for rays in self.rays[rays_of]]
        self.poses[split], self.rays[split], self.marches[split] = np.stack(poses).astype(f32), self.rays[rays_of], self.marches[rays_of]
        with torch.no_grad():
            d = torch.from_numpy(target.astype(np.float64))
            self.gt[split] = [render(self, d, split, j, torch.float64).clamp(0.0, 1.0).float().numpy() for j in range(len(poses))]


def render(case, data, split, j, dtype):
    """[H,W,3] image of view j of a split from `data` (a torch tensor shaped like tree.data), composited in dtype."""
    o, d = case.rays[split][j]
    out = T.render_rays_torch(case.tree, data, o, d, d, case.opt, dtype=dtype, lobes=case.lobes, marches=case.marches[split][j])
    return out.reshape(case.H, case.W, 3)


def _target(t, seed, colour=1.5, sigma=4.0):
    """The data the ground truth is rendered from: the start plus noise, so that every channel has somewhere to go."""
    rs = np.random.RandomState(seed)
    d = t.data.astype(np.float64) + colour * rs.randn(*t.data.shape)
    d[..., -1] = t.data[..., -1] + sigma * rs.randn(*t.data.shape[:-1])
    return d


TRAIN_POSES = ((40.0, 25.0), (160.0, -10.0), (280.0, 40.0))
VAL_POSES = ((100.0, 10.0), (220.0, 30.0))
# where the ground truth of the "val_mid" views lies between the start (0) and the target (1): validation improves while the
# tree approaches that point and gets worse once it has passed it; "val_back" lies behind the start: every step makes it worse
VAL_MID, VAL_BACK = 0.25, -0.5


@functools.lru_cache(maxsize=None)
def case(name):
    """sh4: depth 2, SH4, three 12 x 9 training views (fx 11) and two validation views; sh16: depth 3, SH16, the same views;
    sg4: depth 2, four lobes; ndc: tests/_octree_ndc_oracle.py's depth-3 SH4 tree in its second box, cameras A and B, 14 x 10."""
    if name in ("sh4", "sh16", "sg4"):
        depth, seed, K, p = {"sh4": (2, 34, 4, 0.3), "sh16": (3, 46, 16, 0.15), "sg4": (2, 35, 4, 0.3)}[name]
        t = random_tree(depth, seed, K, p=p)
        if name == "sh4":
            _plant_sigma(t)
        c = Case(name, "sg" if name == "sg4" else "sh", t, 12, 9, 11.0, lobes=G.lobes(4) if name == "sg4" else None)
        target = _target(t, seed + 200)
        c.add_views("train", [pose(*a) for a in TRAIN_POSES], target)
        if name == "sh4":
            val = [pose(*a) for a in VAL_POSES]
            d0 = t.data.astype(np.float64)
            c.add_views("val", val, target)
            c.add_views("val_mid", val, d0 + VAL_MID * (target - d0), rays_of="val")
            c.add_views("val_back", val, d0 + VAL_BACK * (target - d0), rays_of="val")
        return c
    if name == "ndc":
        t = N.box_tree(4, 1)
        c = Case(name, "ndc", t, N.W, N.H, N.FX, ndc=N.Ndc())
        c.add_views("train", [N.camera_a(), N.camera_b()], _target(t, 300))
        return c
    raise KeyError(name)


# No learning rate of the table moves a sigma of the random tree through 0 in N_STEPS steps (the smallest |sigma| is 8e-3, the
# largest move of a sigma 1e-2), so one leaf starts just above 0: leaf 547 (flat index) is seen by the third view, whose step
# lowers its sigma by 6e-3.  It crosses between steps 2 and 3 and then stays below the threshold, without a gradient.
PLANTED = (547, 0.003)


def _plant_sigma(t):
    t.data.reshape(-1, t.data_dim)[PLANTED[0], -1] = f32(PLANTED[1])


CASE_MODES = [(c, m) for c in ("sh4", "sh16") for m in MODES] + [(c, m) for c in ("sg4", "ndc") for m in ("sgd", "adam")]


# ---- the twin -------------------------------------------------------------------------------------------------------------
def _optimizer(p, mode, lr):
    if mode == "adam":
        return torch.optim.Adam([p], lr=lr, eps=1e-8)
    mu = 0.0 if mode == "sgd" else MOMENTUM
    return torch.optim.SGD([p], lr=lr, momentum=mu, nesterov=mode == "nesterov")


def _loss_backward(c, p, split, j, dtype):
    """render -> clamp(0, 1) -> mean((. - gt)^2) -> backward (reference :216-219); returns the sum of squares."""
    im = render(c, p, split, j, dtype)
    sq = (im.clamp(0.0, 1.0) - torch.from_numpy(c.gt[split][j]).to(dtype)) ** 2
    sq.mean().backward()
    return float(sq.sum().detach())


def _loss_backward_one_sweep(c, p, split, j):
    """The same loss and gradient in float32 by the renderer's own backward rule, the one of svox's trace_ray_backward that
    the HIP kernels follow: one forward sweep per ray, then one sweep that carries accum = sum_c g_c out_c, takes each
    sample's share off it and writes d / d sigma = dt (total * light - accum), the colour behind the sample by subtraction.
    Autograd differentiates the cumulative product instead.  The two agree to rounding, but not to the same rounding: a
    sigma deep behind an opaque leaf has a gradient of 1e-11 that this rule leaves with the absolute error of accum (some
    1e-11 at gradients of 1e-3), autograd with a relative one -- and Adam divides by |g| + 1e-8.  Sets p.grad, returns the
    sum of squares."""
    t, D = c.tree, c.tree.data_dim
    K = (D - 1) // 3
    flat = p.detach().numpy().reshape(-1, D)
    grad = np.zeros_like(flat)
    _, d = c.rays[split][j]
    gt = c.gt[split][j].reshape(-1, 3)
    scale = f32(f32(2.0) / f32(c.n))
    one, bg = f32(1.0), f32(c.opt.background_brightness)
    sse = f32(0.0)
    for r, m in enumerate(c.marches[split][j]):
        basis = T.view_basis(t, d[r], c.lobes)
        live = []
        out, light = np.zeros(3, f32), one
        for leaf, dtw in (() if m is None else zip(m.flat.tolist(), m.dtw)):
            val = flat[leaf]
            if val[-1] > 0:
                att = f32(np.exp(f32(-dtw * val[-1]), dtype=f32))
                weight = f32(light * f32(one - att))
                col = (one / (one + np.exp(-(val[:-1].reshape(3, K) * basis).sum(-1, dtype=f32), dtype=f32))).astype(f32)
                out = (out + weight * col).astype(f32)
                light = f32(light * att)
                live.append((leaf, dtw, att, weight, col))
        out = (out + f32(light * bg)).astype(f32)
        clamped = np.clip(out, f32(0.0), one)
        e = (clamped - gt[r]).astype(f32)
        sse = f32(sse + f32(f32(f32(e[0] * e[0]) + f32(e[1] * e[1])) + f32(e[2] * e[2])))
        g = np.where((out >= 0) & (out <= 1), scale * e, f32(0.0)).astype(f32)
        accum = f32(f32(f32(g[0] * out[0]) + f32(g[1] * out[1])) + f32(g[2] * out[2]))
        light = one
        for leaf, dtw, att, weight, col in live:
            total = f32(f32(f32(g[0] * col[0]) + f32(g[1] * col[1])) + f32(g[2] * col[2]))
            dcol = (weight * g * col * (one - col)).astype(f32)
            grad[leaf, :-1] += (dcol[:, None] * basis[None, :]).astype(f32).reshape(-1)
            light = f32(light * att)
            accum = f32(accum - f32(weight * total))
            grad[leaf, -1] += f32(dtw * f32(f32(total * light) - accum))
    g_new = torch.from_numpy(grad.reshape(p.shape))
    p.grad = g_new if p.grad is None else p.grad + g_new
    return float(sse)


def twin_steps(c, mode, lr, n_steps, dtype, grad_scale=1.0, zero_grad=True, one_sweep=False):
    """The reference's step, one training image per step, cycling.  Returns (data after every step [n_steps, ...] float64,
    pre-step sum of squares of every step [n_steps], the gradient of every step as the optimiser saw it [n_steps, ...]).
    grad_scale multiplies the gradient before the optimiser, which is what TreeOptimizer.step does with it.  zero_grad=False
    is the negative control: the gradient buffer is never cleared.  one_sweep (float32 only): the gradient comes from
    _loss_backward_one_sweep, not from autograd -- a second float32 realisation of the same step."""
    assert not one_sweep or dtype == torch.float32
    p = torch.nn.Parameter(torch.from_numpy(c.data0.copy()).to(dtype))
    opt = _optimizer(p, mode, lr)
    datas, sses, grads = [], [], []
    for s in range(n_steps):
        if zero_grad:
            p.grad = None
        j = s % len(c.gt["train"])
        sses.append(_loss_backward_one_sweep(c, p, "train", j) if one_sweep else _loss_backward(c, p, "train", j, dtype))
        held = p.grad.clone()
        if grad_scale != 1.0:
            p.grad.mul_(grad_scale)
        grads.append(p.grad.detach().double().clone())
        opt.step()
        p.grad.copy_(held)                     # what accumulates without zero_grad is the unscaled gradient
        datas.append(p.detach().double().clone())
    return torch.stack(datas), np.asarray(sses, np.float64), torch.stack(grads)


@functools.lru_cache(maxsize=None)
def steps64(name, mode, lr=None, n_steps=N_STEPS, grad_scale=1.0):
    """twin_steps in float64, once per process."""
    return twin_steps(case(name), mode, LR[name, mode] if lr is None else lr, n_steps, torch.float64, grad_scale)


def measure_floor(name, mode, one_sweep=None):
    """(relative L2 of the float32 twin's total move from the float64 twin's, largest per-step |loss32 - loss64|).
    For Adam the larger of two float32 twins, autograd's and the one-sweep backward's (_loss_backward_one_sweep): Adam
    turns the absolute error the second leaves on gradients below its eps into moves of its own size; on the device the
    autograd twin's floor alone is exceeded 13 times by the first step of the sh4 case, all of it on 79 such sigmas.
    The SGD modes, where this error is scaled by lr like any other, keep the autograd twin's floor."""
    c = case(name)
    d64, s64, _ = steps64(name, mode)
    move = d64[-1] - torch.from_numpy(c.data0).double()
    out = (0.0, 0.0)
    for sweep in ((False, True) if mode == "adam" else (False,)) if one_sweep is None else (one_sweep,):
        d32, s32, _ = twin_steps(c, mode, LR[name, mode], N_STEPS, torch.float32, one_sweep=sweep)
        out = (max(out[0], float((d32[-1] - d64[-1]).norm() / move.norm())), max(out[1], float(np.abs(s32 - s64).max() / c.n)))
    return out


def start(c):
    return torch.from_numpy(c.data0).double()


def bounds(name, mode, data64):
    """What the GPU test allows after a step whose float64 twin data is data64: (relative L2 of the move, elementwise atol,
    absolute sum-of-squares deviation) = MARGIN x the recorded floors, the atol scaled by the largest move of an element
    and the loss deviation by the number of elements of an image."""
    rel, dloss = FLOOR[name, mode]
    return MARGIN * rel, MARGIN * rel * float((data64 - start(case(name))).abs().max()), MARGIN * dloss * case(name).n


def _psnr(sse, n):
    return -10.0 * math.log10(sse / n)


def _validate(c, p, split, dtype, mses):
    with torch.no_grad():
        tot = 0.0
        for j in range(len(c.gt[split])):
            sq = (render(c, p, split, j, dtype).clamp(0.0, 1.0) - torch.from_numpy(c.gt[split][j]).to(dtype)) ** 2
            mses.append(float(sq.sum()) / c.n)
            tot += _psnr(float(sq.sum()), c.n)
    k = len(c.gt[split])
    return tot / k, sum(1.0 / m for m in mses[-k:]) / k


def twin_fit(c, args, dtype, val="val"):
    """The epoch loop of the reference (:189-243) on the case's training views and the validation views `val`: initial
    validation; per epoch the mean over the images of -10 log10(sse / n), each taken before its step; validation every
    val_interval epochs and after the last; the best snapshot; "Stop since overfitting" unless continue_on_decrease.
    Returns a namespace: history [(epoch, train psnr or None, val psnr)] as optimization.fit's, best (data float64 or None),
    best_epoch (or None), stopped (bool), final (the data the loop ends with), mses (every image's mean squared error,
    validation and training, in the order they were taken), inv [(mean over the training images of 1 / mse or None, the same
    over the validation images)] per history entry -- what turns a bound on the mse into one on the averaged PSNR --, and
    decisions [(val psnr, best before it, its inv, the best's inv)] of every validation after the first."""
    mode = "adam" if not args.sgd else ("sgd" if args.sgd_momentum == 0.0 else ("nesterov" if args.sgd_nesterov else "momentum"))
    p = torch.nn.Parameter(torch.from_numpy(c.data0.copy()).to(dtype))
    opt = _optimizer(p, mode, args.lr)
    mses = []
    best, best_inv = _validate(c, p, val, dtype, mses)
    out = types.SimpleNamespace(history=[(0, None, best)], best=None, best_epoch=None, stopped=False, decisions=[], mses=mses,
                                inv=[(None, best_inv)])
    n_train = len(c.gt["train"])
    for epoch in range(args.num_epochs):
        tpsnr = 0.0
        for j in range(n_train):
            p.grad = None
            sse = _loss_backward(c, p, "train", j, dtype)
            mses.append(sse / c.n)
            tpsnr += _psnr(sse, c.n)
            opt.step()
        if epoch % args.val_interval == args.val_interval - 1 or epoch == args.num_epochs - 1:
            train_inv = sum(1.0 / m for m in mses[-n_train:]) / n_train
            v, v_inv = _validate(c, p, val, dtype, mses)
            out.history.append((epoch + 1, tpsnr / n_train, v))
            out.inv.append((train_inv, v_inv))
            out.decisions.append((v, best, v_inv, best_inv))
            if v > best:
                best, best_inv, out.best, out.best_epoch = v, v_inv, p.detach().double().clone(), epoch + 1
            elif not args.continue_on_decrease:
                out.stopped = True
                break
    out.final = p.detach().double().clone()
    return out


# the schedules of the loop test, all on sh4 with plain SGD: (validation split, fit arguments)
FIT = {
    "to_the_end": ("val", dict(num_epochs=4, val_interval=2)),
    "early_stop": ("val_mid", dict(num_epochs=6, val_interval=1)),
    "carry_on": ("val_mid", dict(num_epochs=6, val_interval=1, continue_on_decrease=True)),
    "no_gain": ("val_back", dict(num_epochs=3, val_interval=1)),
}
FIT_LR = 1000.0


def fit_args(schedule):
    return mode_args("sgd", FIT_LR, **FIT[schedule][1])


@functools.lru_cache(maxsize=None)
def fit64(schedule):
    return twin_fit(case("sh4"), fit_args(schedule), torch.float64, val=FIT[schedule][0])


def measure_fit_floor(schedule):
    """FLOOR["fit", schedule]: (largest |mse32 - mse64| over every image the loop scores, training and validation; relative L2
    distance of the float32 loop's total move from the float64 loop's)."""
    r32 = twin_fit(case("sh4"), fit_args(schedule), torch.float32, val=FIT[schedule][0])
    r64 = fit64(schedule)
    assert len(r32.mses) == len(r64.mses) and [h[0] for h in r32.history] == [h[0] for h in r64.history]
    c = case("sh4")
    return (float(np.abs(np.asarray(r32.mses) - np.asarray(r64.mses)).max()),
            float((r32.final - r64.final).norm() / (r64.final - start(c)).norm()))


def psnr_bound(schedule, inv):
    """The bound on an averaged PSNR that follows from the bound on each image's sum of squares: 10 / ln 10 * delta sse / sse
    per image, delta sse / n = MARGIN x the schedule's recorded floor, averaged: `inv` is the mean of 1 / mse (twin_fit)."""
    return 10.0 / math.log(10.0) * MARGIN * FLOOR["fit", schedule][0] * inv


# ---- the inputs of the image_mse tests ------------------------------------------------------------------------------------
MSE_GROUP = 2048                  # elements per workgroup of pxo_image_mse's launch below its cap (the GPU test asserts it)
MSE_CAP = 4096                    # workgroups at most
MSE_SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 1, 4096 * 2048, 4096 * 2048 + 1,
             4096 * 2048 + 256 * 4096 + 3)
_ONE = f32(1.0)
MSE_PLANTED = (f32(0.0), f32(-0.0), _ONE, np.nextafter(f32(0.0), f32(-1.0)), np.nextafter(f32(0.0), f32(1.0)),
               np.nextafter(_ONE, f32(0.0)), np.nextafter(_ONE, f32(2.0)))


def mse_groups(n):
    return min((n + MSE_GROUP - 1) // MSE_GROUP, MSE_CAP)


def mse_boundaries(n):
    """Index 0, n - 1 and the first and last element of every workgroup's first stretch of the grid-stride loop (a workgroup
    takes 256 consecutive elements per iteration; the launcher sizes the grid for eight iterations)."""
    idx = {0, n - 1}
    for g in range(1, mse_groups(n)):
        for i in (g * 256 - 1, g * 256, g * MSE_GROUP - 1, g * MSE_GROUP):
            if 0 <= i < n:
                idx.add(i)
    return np.fromiter(sorted(idx), np.int64)


def mse_inputs(n, seed=0):
    """(im, gt) float32 [n]: im uniform in [-0.5, 1.5] with the exact values 0.0, -0.0, 1.0 and their neighbours on both sides
    planted, in turn, at index 0, n - 1 and every workgroup boundary that exists for n; gt uniform in [0, 1]."""
    rs = np.random.RandomState(seed + n % 1000003)
    im = (rs.rand(n).astype(f32) * f32(2.0) - f32(0.5)).astype(f32)
    gt = rs.rand(n).astype(f32)
    where = mse_boundaries(n)
    im[where] = np.asarray(MSE_PLANTED, f32)[(np.arange(len(where)) + seed) % len(MSE_PLANTED)]
    return im, gt


def mse_seeds(n):
    """Seeds of mse_inputs the tests run for a size: seven for the small sizes, so that every planted value takes every
    boundary in turn, one for the sizes with thousands of boundaries."""
    return range(len(MSE_PLANTED)) if n <= 2 * MSE_GROUP + 1 else range(1)


def mse_hot_positions(n):
    """Index 0, n - 1 and the first element of the last workgroup (workgroup g starts at element 256 g)."""
    return [0, n - 1, (mse_groups(n) - 1) * 256]


def mse_single_hot(n, at):
    """(im, gt, e): the clamped error is exactly zero everywhere (im == gt inside [0, 1], or im beyond the end of the range
    gt sits on) except at `at`, where it is the float32 e: the sum of squares is float32(e * e), whatever the order."""
    rs = np.random.RandomState(n % 1000003 + at % 9973)
    gt = rs.rand(n).astype(f32)
    gt[::7], gt[3::11] = f32(1.0), f32(0.0)
    im = gt.copy()
    im[::7], im[3::11] = f32(1.25), f32(-0.25)
    im[at], gt[at] = f32(0.9), f32(0.3)
    return im, gt, f32(f32(0.9) - f32(0.3))


if __name__ == "__main__":
    import time
    for name, mode in CASE_MODES:
        t0 = time.time()
        rel, dl = measure_floor(name, mode)
        d64 = steps64(name, mode)[0]
        move = float((d64[-1] - torch.from_numpy(case(name).data0).double()).abs().max())
        print(f'    ("{name}", "{mode}"): ({rel:.2e}, {dl:.2e}),      # max move {move:.3g}, {time.time() - t0:.1f} s', flush=True)
    for schedule in FIT:
        r = fit64(schedule)
        print(f'    ("fit", "{schedule}"): {measure_fit_floor(schedule)},      # stopped {r.stopped}, best epoch {r.best_epoch}, '
              f'history {[(h[0], None if h[1] is None else round(h[1], 3), round(h[2], 3)) for h in r.history]}', flush=True)
