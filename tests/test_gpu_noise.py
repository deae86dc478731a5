"""-m gpu tests of the density-noise branch of the whole-path entry points (PxoCfg.noise_std > 0 with randomized != 0:
pxo_train_fwd_bwd, pxo_sg_train_fwd_bwd, pxo_render_fwd, pxo_sg_render_fwd, pxo_vd_render_fwd) and of lindisp = 1 through the
whole path, against the float64 oracle.

The whole path draws its normals from Philox streams 3 (coarse, B*Nc elements) and 4 (fine, B*(Nc+Nf)) of the call's seed.
Each test draws the two streams once through pxo_add_gaussian_noise on zeros, holds them to the host restatement
(_helpers.philox_normal, 2e-6: the bar of test_gaussian_noise_against_reference) and hands them as float64 to the oracle.  The
rule -- which stream, seed and element -- is pinned by the restatement, the arithmetic by the oracle at the numbers drawn.

Groups (the worst ratio of an observed error to its bound is printed per group; run with -s):
  a  the SH training step: loss / loss_c rtol 1e-5 + atol 1e-7, PSNR rtol 2e-5 + atol 1e-6, gradient rel L2 per MLP
     <= max(1e-3, 3 e_f32) against the float64 loss_fn at the device's own positions and normals, e_f32 = the float32
     oracle's error there (<= 4e-3); bit identities: loss_sp and weight_l2 against the noise-free call, skip_zero_rows,
     a repeated call, randomized = 0; seed + 1 changes the gradient
  b  bucketed entry and coarse reverse on the side stream, bit-identical under noise
  c  the NeRF-SG training step against the float64 twin, the rules of test_sg_train_step_past_64_ray_blocks_at_every_lobe_count
  d  forward against the oracle, the form of test_render_fwd_matches_oracle (max <= 3 e_cpu + 3e-5, mean <= 3 m_cpu + 2e-6)
  e  forward against its public pieces, bit for bit, and the view-conditioned path against its float64 restatement
  f  lindisp = 1: render under d's bounds, training under a's
tests/test_noise_cpu.py shows on the oracle alone that e_f32 stays under its cap for these cases and that each mistake this
file exists for moves an asserted quantity by >= 10 x its bound."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _noise_cases as C                                              # noqa: E402
import _octree_sg_cases as G                                          # noqa: E402
import _sg_train_cases as SC                                          # noqa: E402
import _sg_train_oracle as T                                          # noqa: E402
from _helpers import (_gpu, _ops, hip_sample_positions, make_params, make_rays, philox_normal, pxo_cfg,  # noqa: E402
                      split_mlp)
from _viewdirs_render_helpers import Rays, check_level, fixture, fixture_state_dict, host_render_f64, render_cfg  # noqa: E402
from oracle import nerf_oracle as O                                   # noqa: E402

pytestmark = pytest.mark.gpu
_worst = {}


def _show(group, what, err, bound, device=True):
    """Prints an observed error beside its bound and the group's worst ratio so far; returns whether the bound holds.
    device=False: a figure of the oracle alone (e_f32 against its cap), kept out of the group's worst ratio."""
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    _worst[group] = max(_worst.get(group, 0.0), ratio if device else 0.0)
    print(f"[{group}] {what}: {err:.3e} (bound {bound:.3e}, ratio {ratio:.2f}; worst of group {group} so far {_worst[group]:.2f})")
    return err <= bound


def _same(group, what, ok):
    print(f"[{group}] {what}: bit-identical {bool(ok)}")
    return bool(ok)


def _device_normals(ops, dev, group, B, Nc, Nf, seed=C.SEED):
    """(N_c [B*Nc], N_f [B*(Nc+Nf)] or None) as the device draws streams 3 and 4 of `seed`, held to the host restatement."""
    out = []
    for sid, n in ((C.STREAM_COARSE, B * Nc), (C.STREAM_FINE, B * (Nc + Nf) if Nf > 0 else 0)):
        if n == 0:
            out.append(None)
            continue
        got = ops.add_gaussian_noise(torch.zeros(n, device=dev), 1.0, seed=seed, stream_id=sid)
        err = float(np.abs(got.cpu().double().numpy() - philox_normal(seed, sid, n)).max())
        assert _show(group, f"normals of stream {sid}, {n} elements, against philox_normal", err, C.NORMAL_ATOL)
        out.append(got)
    return out


def _host(n, B):
    return None if n is None else n.cpu().reshape(B, -1)


# ---- a / b / f: the SH training step ------------------------------------------------------------------------------------------
class _Step:
    """One case's inputs on the device, and pxo_train_fwd_bwd on them with a NaN-poisoned workspace."""

    def __init__(self, ops, dev, c):
        self.ops, self.dev, self.c = ops, dev, c
        self.inputs = C.train_inputs(c, dev)
        self.cfg, self.flat, self.rays, self.px, self.t_rand, self.u, self.sp = self.inputs
        self.fd = self.flat.to(dev)
        self.rays_dev = tuple(r.to(dev) for r in self.rays)
        self.on_dev = [x.to(dev) for x in (self.px, self.t_rand, self.u, self.sp)]

    def pcfg(self, std, skip=0):
        cfg = copy.copy(self.cfg)
        cfg.noise_std = std
        p = pxo_cfg(self.ops, cfg)
        p.mlp_precision, p.skip_zero_rows = self.c["prec"], skip
        return p

    def packed(self, pcfg):
        return [self.ops.pack_weights(pcfg, split_mlp(self.fd, self.cfg, i)) for i in range(2)]

    def run(self, std, seed=C.SEED, skip=0, randomized=True, entry="ops"):
        ops, dev = self.ops, self.dev
        pcfg = self.pcfg(std, skip)
        packed = self.packed(pcfg)
        px, t_rand, u, sp = self.on_dev
        B = px.shape[0]
        grads = torch.full_like(self.fd, float("nan")); stats = torch.zeros(6, device=dev)
        ws = torch.empty(ops.train_workspace_bytes(pcfg, B), dtype=torch.uint8, device=dev)
        ws.fill_(0xFF)                               # skipped tiles leave dz unwritten: NaN patterns there must never be read
        t_rand, u = (t_rand, u) if randomized else (None, None)
        if entry == "plain":                         # pxo_train_fwd_bwd itself; ops.train_fwd_bwd goes through the bucketed entry
            from plenoctree_amd import _lib
            P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
            (f0, b0), (f1, b1) = packed
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            rc = _lib.load().pxo_train_fwd_bwd(ctypes.byref(pcfg), P(self.fd), P(f0), P(b0), P(f1), P(b1), *[P(r) for r in self.rays_dev],
                                               P(px), B, int(randomized), P(t_rand), P(u), P(sp), seed, P(grads), P(stats), P(ws),
                                               ws.numel(), stream)
            _lib.check(rc, "pxo_train_fwd_bwd")
        else:
            event = ops.Event() if entry == "bucketed" else None          # kept until the call's kernels are done
            ops.train_fwd_bwd(pcfg, self.fd, packed, *self.rays_dev, px, grads, stats, ws, randomized=randomized, t_rand=t_rand, u=u,
                              sp_points=sp, seed=seed, grads0_ready=event)
        torch.cuda.synchronize()
        return grads.cpu(), stats.cpu()


def _check_step_against_the_oracle(group, name):
    """The value checks of group a on one case; returns (_Step, gradient, stats) of the checked call."""
    ops = _ops(); dev = _gpu()
    c = C.case(name)
    B, Nc, Nf, std = c["B"], c["Nc"], c["Nf"], c["std"]
    fine = Nf > 0
    st = _Step(ops, dev, c)
    n_c, n_f = _device_normals(ops, dev, group, B, Nc, Nf) if std else (None, None)
    g, s = st.run(std)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(s).all())
    pcfg = st.pcfg(std)
    z_c, z_f = hip_sample_positions(ops, pcfg, st.packed(pcfg), st.rays_dev, st.on_dev[1], st.on_dev[2], noise_c=n_c, noise_f=n_f)
    z_c, z_f = z_c.cpu(), None if z_f is None else z_f.cpu()
    hn_c, hn_f = _host(n_c, B), _host(n_f, B)
    l64, lc64, g64 = C.oracle_at(st.inputs, z_c, z_f, hn_c, hn_f)
    l32, lc32, g32 = C.oracle_at(st.inputs, z_c, z_f, hn_c, hn_f, dtype=torch.float32)
    e_f32 = C.rel_l2_per_mlp(g32, g64, fine)
    e_hip = C.rel_l2_per_mlp(g, g64, fine)
    n = g64.numel() // 2
    print(f"[{group}] {name}: loss HIP {float(s[0]):.9g} f64 {l64:.9g} f32 oracle {l32:.9g}; loss_c HIP {float(s[2]):.9g} f64 {lc64:.9g} "
          f"f32 oracle {lc32:.9g}")
    ok = [_show(group, f"{name} loss vs f64", abs(float(s[0]) - l64), C.LOSS_ATOL + C.LOSS_RTOL * abs(l64))]
    psnr64 = -10.0 * np.log10(l64)
    ok.append(_show(group, f"{name} psnr vs f64", abs(float(s[1]) - psnr64), C.PSNR_ATOL + C.PSNR_RTOL * abs(psnr64)))
    if fine:
        ok.append(_show(group, f"{name} loss_c vs f64", abs(float(s[2]) - lc64), C.LOSS_ATOL + C.LOSS_RTOL * abs(lc64)))
        psnr_c64 = -10.0 * np.log10(lc64)
        ok.append(_show(group, f"{name} psnr_c vs f64", abs(float(s[4]) - psnr_c64), C.PSNR_ATOL + C.PSNR_RTOL * abs(psnr_c64)))
    for mi in range(2 if fine else 1):
        norm = float(g64[mi * n:(mi + 1) * n].norm())
        assert norm > 1e-4, f"degenerate test: the oracle's MLP_{mi} gradient vanishes ({norm:.3g})"
        ok.append(_show(group, f"{name} e_f32 of MLP_{mi} (the float32 oracle vs f64, same positions and normals)", e_f32[mi],
                        C.E_F32_CAP, device=False))
        ok.append(_show(group, f"{name} MLP_{mi} gradient rel L2 vs f64 (float32 oracle {e_f32[mi]:.3e})", e_hip[mi],
                        C.grad_bound(e_f32[mi])))
    if not fine and c["wd"] == 0.0:
        assert float(g[n:].abs().max()) == 0.0
    assert all(ok), name
    return st, g, s


@pytest.mark.parametrize("name", list(C.TRAIN_CASES))
def test_train_step_with_noise_matches_the_oracle(name):
    """Group a.  pxo_train_fwd_bwd with noise_std > 0, explicit t_rand / u / sp_points and seed 7, against the float64 loss_fn
    with the device's own normals injected, at the device's own sample positions (which the coarse noise moves); then the bit
    identities of the branch."""
    st, g, s = _check_step_against_the_oracle("a", name)
    std = st.c["std"]
    g0, s0 = st.run(0.0)
    ok = [_same("a", f"{name} loss_sp and weight_l2 against the call with noise_std = 0 (no noise reaches the sparsity rows)",
                torch.equal(s[3], s0[3]) and torch.equal(s[5], s0[5]))]
    assert not torch.equal(g, g0), "the noise changed nothing"
    g1, s1 = st.run(std, skip=1)
    ok.append(_same("a", f"{name} skip_zero_rows 1 against 0 (noise decides which rows are exactly zero)",
                    torch.equal(g1, g) and torch.equal(s1, s)))
    g2, s2 = st.run(std)
    ok.append(_same("a", f"{name} a repeated call", torch.equal(g2, g) and torch.equal(s2, s)))
    g3, _ = st.run(std, seed=C.SEED + 1)
    assert bool(torch.isfinite(g3).all()) and not torch.equal(g3, g), "seed + 1 must change the gradient"
    g4, s4 = st.run(std, randomized=False)
    g5, s5 = st.run(0.0, randomized=False)
    ok.append(_same("a", f"{name} randomized = 0 with noise_std {std} against noise_std = 0",
                    torch.equal(g4, g5) and torch.equal(s4, s5)))
    assert bool(torch.isfinite(g1).all()) and bool(torch.isfinite(g4).all()) and all(ok), name


def test_bucketed_entry_and_side_stream_are_bit_identical_under_noise():
    """Group b, on case i: pxo_train_fwd_bwd, pxo_train_fwd_bwd_bucketed with an event, and the coarse reverse pass on the
    library's side stream (PXO_TUNE_COARSE_REVERSE_STREAM, as test_coarse_reverse_side_stream_is_bit_identical sets it) give
    the same bits, dense and skipping."""
    ops = _ops(); dev = _gpu()
    st = _Step(ops, dev, C.case("i-48x64+128-std0.3"))
    std = st.c["std"]
    g, s = st.run(std)
    assert bool(torch.isfinite(g).all()) and not torch.equal(g, st.run(0.0)[0])
    ok = []
    for entry in ("plain", "bucketed"):
        ge, se = st.run(std, entry=entry)
        ok.append(_same("b", f"{entry} entry against ops.train_fwd_bwd", torch.equal(ge, g) and torch.equal(se, s)))
    default = ops.get_tuning(ops.TUNE_COARSE_REVERSE_STREAM)
    assert default == 0
    try:
        ops.set_tuning(ops.TUNE_COARSE_REVERSE_STREAM, 1)
        assert ops.get_tuning(ops.TUNE_COARSE_REVERSE_STREAM) == 1
        side = [st.run(std, skip=skip) for skip in (0, 1)]
    finally:
        ops.set_tuning(ops.TUNE_COARSE_REVERSE_STREAM, default)
    for skip, (gs, ss) in enumerate(side):
        ok.append(_same("b", f"coarse reverse on the side stream, skip_zero_rows {skip}", torch.equal(gs, g) and torch.equal(ss, s)))
    assert all(ok)


@pytest.mark.parametrize("name", list(C.LINDISP_CASES))
def test_train_step_with_lindisp_matches_the_oracle(name):
    """Group f.  near 0.5 / far 4.0 (the stage test's values), samples linear in disparity, noise off and std 0.3: group a's bounds."""
    _check_step_against_the_oracle("f", name)


# ---- c: the NeRF-SG training step ---------------------------------------------------------------------------------------------
SG_STD = 0.5
SG_STEP_CASES = (SC.STEP_CASES[1], SC.STEP_CASES[0])          # (16, 257, 8, 0, 0.0): no fine level; (9, 260, 8, 8, 0.05): 65 ray blocks


def _sg_step(ops, dev, case, cfg, skip=0):
    _, flat, sgp, rays, px, t_rand, u, sp = SC.step_inputs(case)
    pcfg = pxo_cfg(ops, cfg)
    pcfg.skip_zero_rows = skip
    flat, sgp = flat.to(dev), sgp.to(dev)
    n = flat.numel() // 2
    packed = [ops.pack_weights(pcfg, flat[i * n:(i + 1) * n].contiguous()) for i in range(2)]
    o, d, v = (x.contiguous().to(dev) for x in rays)
    B = o.shape[0]
    grads, sg_grads, stats = torch.zeros_like(flat), torch.full_like(sgp, 7.0), torch.zeros(6, device=dev)
    ws = torch.empty(ops.sg_train_workspace_bytes(pcfg, B), dtype=torch.uint8, device=dev)
    ops.sg_train_fwd_bwd(pcfg, flat, sgp, packed, o, d, v, px.to(dev), grads, sg_grads, stats, ws, randomized=True,
                         t_rand=t_rand.to(dev), u=u.to(dev) if cfg.num_fine_samples > 0 else None, sp_points=sp.to(dev), seed=C.SEED)
    torch.cuda.synchronize()
    from plenoctree_amd.nerf_sh.nerf import utils
    return dict(zip(utils.Stats._fields, stats.cpu().tolist())), grads.cpu(), sg_grads.cpu()


@pytest.mark.parametrize("case", SG_STEP_CASES, ids=SC.step_id)
def test_sg_train_step_with_noise_matches_the_float64_twin(case):
    """Group c.  pxo_sg_train_fwd_bwd with noise_std 0.5 against T.loss_and_grad in float64 with the device's normals injected;
    the floors are the float32 twin's figures on the same normals.  SG gradient <= 4 x floor, each MLP's <= 2 x floor, the
    Stats to rel 2e-5 (loss_sp rel 5e-3), skip 0 / 1 and a repeated call bitwise equal."""
    ops = _ops(); dev = _gpu()
    K, B, Nc, Nf, wd = case
    n_c, n_f = _device_normals(ops, dev, "c", B, Nc, Nf)
    cfg = copy.copy(SC.step_inputs(case)[0])
    cfg.noise_std = SG_STD

    def twin(dtype):
        _, flat, sgp, rays, px, t_rand, u, sp = SC.step_inputs(case, dtype)
        cast = lambda t: None if t is None else t.to(dtype)
        _, stats, grad, sg_grad = T.loss_and_grad(flat, sgp, rays, px, cfg, t_rand, u if Nf > 0 else None, sp,
                                                  noise_c=cast(_host(n_c, B)), noise_f=cast(_host(n_f, B)))
        return {k: float(v) for k, v in stats.items()}, grad.double(), sg_grad.double()

    want_stats, want, want_sg = twin(torch.float64)
    _, g32, sg32 = twin(torch.float32)
    n = want.numel() // 2
    rel = lambda a, b: float((a.double() - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.double().norm())
    floors = (rel(sg32, want_sg), rel(g32[:n], want[:n]), rel(g32[n:], want[n:]))
    st, grad, sg_grad = _sg_step(ops, dev, case, cfg)
    plain_cfg = copy.copy(cfg); plain_cfg.noise_std = None
    assert not torch.equal(_sg_step(ops, dev, case, plain_cfg)[2], sg_grad), "the noise changed nothing"
    assert float(want_sg.norm()) > 0 and not bool((sg_grad == 7.0).any())
    tag = SC.step_id(case)
    ok = [_show("c", f"{tag} SG gradient rel L2 vs the float64 twin (float32 twin {floors[0]:.3e})", rel(sg_grad, want_sg), 4 * floors[0]),
          _show("c", f"{tag} MLP_0 gradient (float32 twin {floors[1]:.3e})", rel(grad[:n], want[:n]), 2 * floors[1]),
          _show("c", f"{tag} MLP_1 gradient (float32 twin {floors[2]:.3e})", rel(grad[n:], want[n:]), 2 * floors[2])]
    for k in ("loss", "loss_c", "weight_l2", "psnr", "psnr_c"):
        ok.append(_show("c", f"{tag} stats/{k}", abs(st[k] - want_stats[k]), 2e-5 * abs(want_stats[k])))
    ok.append(_show("c", f"{tag} stats/loss_sp", abs(st["loss_sp"] - want_stats["loss_sp"]), 1e-9 + 5e-3 * abs(want_stats["loss_sp"])))
    st1, grad1, sg1 = _sg_step(ops, dev, case, cfg, skip=1)
    st2, grad2, sg2 = _sg_step(ops, dev, case, cfg)
    ok.append(_same("c", f"{tag} skip_zero_rows 1 against 0", torch.equal(grad1, grad) and torch.equal(sg1, sg_grad) and st1 == st))
    ok.append(_same("c", f"{tag} a repeated call", torch.equal(grad2, grad) and torch.equal(sg2, sg_grad) and st2 == st))
    assert all(ok)


# ---- d / f: the forward pass against the oracle -------------------------------------------------------------------------------
RENDER_CASES = {
    "sh16-200x64+128-std0.3": dict(group="d", B=200, Nc=64, Nf=128, deg=3, std=0.3),
    "sg16-200x64+128-std0.3": dict(group="d", B=200, Nc=64, Nf=128, deg=3, std=0.3, sg=True),
    "sh4-5x13+20-std1": dict(group="d", B=5, Nc=13, Nf=20, deg=1, std=1.0),          # case iv's shape: both streams end inside a quad
    "lindisp-48x64+128-noise-off": dict(group="f", B=48, Nc=64, Nf=128, deg=3, std=None, near=0.5, far=4.0, lindisp=True),
    "lindisp-48x64+128-std0.3": dict(group="f", B=48, Nc=64, Nf=128, deg=3, std=0.3, near=0.5, far=4.0, lindisp=True),
}


@pytest.mark.parametrize("name", list(RENDER_CASES))
def test_render_fwd_with_noise_matches_the_oracle(name):
    """Groups d and f.  pxo_render_fwd / pxo_sg_render_fwd (through lobes=) with explicit t_rand / u and seed 7 against O.render /
    the SG twin's render in float64 with the device's normals injected: rgb and acc of both levels, max error <= 3 e_cpu + 3e-5
    and mean error <= 3 m_cpu + 2e-6, e_cpu / m_cpu the float32 oracle's with the same normals."""
    ops = _ops(); dev = _gpu()
    c = dict(dict(near=2.0, far=6.0, lindisp=False, sg=False), **RENDER_CASES[name])
    group, B, Nc, Nf = c["group"], c["B"], c["Nc"], c["Nf"]
    cfg = O.Cfg(sh_deg=c["deg"], num_coarse_samples=Nc, num_fine_samples=Nf, near=c["near"], far=c["far"], lindisp=c["lindisp"],
                noise_std=c["std"])
    pcfg = pxo_cfg(ops, cfg)
    flat = make_params(cfg, bias_scale=0.2)
    rays = make_rays(B, 41)
    gen = torch.Generator().manual_seed(43)
    t_rand, u = torch.rand(B, Nc, generator=gen), torch.rand(B, Nf, generator=gen)
    n_c, n_f = _device_normals(ops, dev, group, B, Nc, Nf) if c["std"] else (None, None)
    pk = [ops.pack_weights(pcfg, split_mlp(flat, cfg, i).to(dev), need_bwd=False)[0] for i in range(2)]
    sgp = lobes = None
    if c["sg"]:
        fx = G.fixture()
        K = cfg.sh_dim
        sgp = torch.cat([torch.tensor(fx[f"sg_lambda_{K}"]).float(), torch.tensor(fx[f"sg_mu_spher_{K}"]).float().reshape(-1)])
        lobes = ops.sg_lobes(sgp.to(dev), K)
    out = ops.render_fwd(pcfg, pk[0], pk[1], *[r.to(dev) for r in rays], randomized=True, t_rand=t_rand.to(dev), u=u.to(dev),
                         seed=C.SEED, lobes=lobes)

    def oracle(dtype):
        cast = lambda t: None if t is None else t.to(dtype)
        r = O.Rays(*[cast(x) for x in rays])
        kw = dict(noise_c=cast(_host(n_c, B)), noise_f=cast(_host(n_f, B)))
        with torch.no_grad():
            params = O.unflatten_params(cast(flat), cfg)
            if c["sg"]:
                return T.render(params, cast(sgp), r, cfg, cast(t_rand), cast(u), **kw)
            return O.render(params, r, cfg, cast(t_rand), cast(u), **kw)

    ref, ref64 = oracle(torch.float32), oracle(torch.float64)
    if c["std"]:
        plain = copy.copy(cfg); plain.noise_std = None
        clean = ops.render_fwd(pxo_cfg(ops, plain), pk[0], pk[1], *[r.to(dev) for r in rays], randomized=True, t_rand=t_rand.to(dev),
                               u=u.to(dev), seed=C.SEED, lobes=lobes)
        assert float((clean[1][0] - out[1][0]).abs().max()) > 1e-3, "the noise changed nothing"
    ok = []
    for lvl, tag in ((0, "coarse"), (1, "fine")):
        for j, q in ((0, "rgb"), (2, "acc")):
            got, r32, r64 = out[lvl][j].cpu().double(), ref[lvl][j].double(), ref64[lvl][j]
            assert bool(torch.isfinite(got).all())
            e_hip, e_cpu = float((got - r64).abs().max()), float((r32 - r64).abs().max())
            m_hip, m_cpu = float((got - r64).abs().mean()), float((r32 - r64).abs().mean())
            ok.append(_show(group, f"{name} {tag}/{q} max err vs f64 (float32 oracle {e_cpu:.3e})", e_hip, 3 * e_cpu + 3e-5))
            ok.append(_show(group, f"{name} {tag}/{q} mean err vs f64 (float32 oracle {m_cpu:.3e})", m_hip, 3 * m_cpu + 2e-6))
    assert all(ok), name


# ---- e: the forward pass against its public pieces ----------------------------------------------------------------------------
def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for la, lb in zip(a, b) for x, y in zip(la, lb))


def test_sh_whole_path_equals_its_public_pieces_bit_for_bit_under_noise():
    """Group e, pxo_render_fwd against the chain test_gaussian_noise_against_reference spells out (pxo_sample_along_rays ->
    pxo_mlp_fwd -> pxo_add_gaussian_noise with the injected normals -> pxo_shade_composite_fwd -> pxo_sample_pdf -> ...).  The
    noise-free comparison is the control: with it bit-identical, the noisy one must be too."""
    ops = _ops(); dev = _gpu()
    for B, Nc, Nf, deg, std in ((48, 64, 128, 3, 0.3), (5, 13, 20, 1, 1.0)):
        cfg = O.Cfg(sh_deg=deg, num_coarse_samples=Nc, num_fine_samples=Nf)
        flat = make_params(cfg, bias_scale=0.2)
        pk = [ops.pack_weights(pxo_cfg(ops, cfg), split_mlp(flat, cfg, i).to(dev), need_bwd=False)[0] for i in range(2)]
        o, d, v = (r.to(dev) for r in make_rays(B, 41))
        gen = torch.Generator().manual_seed(43)
        t_rand, u = torch.rand(B, Nc, generator=gen).to(dev), torch.rand(B, Nf, generator=gen).to(dev)
        normals = _device_normals(ops, dev, "e", B, Nc, Nf)
        for noise_std in (None, std):
            cfg.noise_std = noise_std
            pcfg = pxo_cfg(ops, cfg)
            whole = ops.render_fwd(pcfg, pk[0], pk[1], o, d, v, randomized=True, t_rand=t_rand, u=u, seed=C.SEED)
            z, pts = ops.sample_along_rays(o, d, Nc, pcfg.near_, pcfg.far_, t_rand)
            pieces = []
            for lvl in (0, 1):
                raw_rgb, raw_sigma = ops.mlp_fwd(pcfg, pk[lvl], pts)
                if noise_std:
                    ops.add_gaussian_noise(raw_sigma, noise_std, noise=normals[lvl])
                comp, disp, acc, w = ops.shade_composite_fwd(pcfg, raw_rgb, raw_sigma, z, d, v)
                pieces.append((comp, disp, acc))
                if lvl == 0:
                    z, pts = ops.sample_pdf(z, w, o, d, Nf, u)
            what = "control, noise off" if not noise_std else f"noise_std {noise_std}"
            assert _same("e", f"pxo_render_fwd against its pieces, {B} x {Nc}+{Nf}, {what}", _equal(whole, pieces))


@pytest.fixture(scope="module")
def vd():
    from plenoctree_amd import ops
    from plenoctree_amd.nerf_sh.nerf import checkpoints, viewdirs
    dev = _gpu()
    sd = fixture_state_dict(fixture())
    flat = checkpoints.vd_tree_to_arena(checkpoints.vd_torch_state_dict_to_tree(sd))
    return dict(ops=ops, viewdirs=viewdirs, dev=dev, sd=sd, state=viewdirs.ViewdirsState(torch.from_numpy(flat).to(dev)))


def _vd_rays(n, seed, norms=(0.5, 1.0, 1.5)):
    """n rays from cameras on a sphere of radius 4 towards the origin, |directions| cycling through `norms` (the rays of
    tests/test_gpu_viewdirs_render.py)."""
    g = torch.Generator().manual_seed(seed)
    cam = torch.randn(n, 3, generator=g)
    cam = 4 * cam / cam.norm(dim=-1, keepdim=True)
    v = -cam / 4 + 0.08 * torch.randn(n, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True)
    d = v * torch.tensor([norms[i % len(norms)] for i in range(n)])[:, None]
    return Rays(cam.contiguous(), d.contiguous(), v.contiguous())


VD_STD = 0.3


@pytest.mark.timeout(60)
@pytest.mark.parametrize("nc,nf,B", [(12, 20, 7), (64, 128, 5), (13, 20, 7)])
def test_vd_whole_path_equals_its_public_pieces_and_the_float64_restatement_under_noise(vd, nc, nf, B):
    """Group e, pxo_vd_render_fwd with noise_std 0.3: test_whole_path_equals_its_public_pieces_bit_for_bit with
    pxo_add_gaussian_noise (injected normals) between pxo_vd_eval_points_raw and pxo_vd_composite_fwd, with the default ray block
    and with PXO_TUNE_VD_RAY_BLOCK = 5.  At (12, 20) and (64, 128) every block of 5 rays starts on a quad of the streams
    (5 x 12, 5 x 32, ...); (13, 20, 7) is here so that one starts inside a quad (elements 65 and 165) and the `first` offset of
    the blocked launch matters.  Then host_render_f64 with the same normals under check_level's bounds."""
    ops, dev, st = vd["ops"], vd["dev"], vd["state"]
    host_rays = _vd_rays(B, 300 + B)
    rays = Rays(*[x.to(dev) for x in host_rays])
    g = torch.Generator().manual_seed(8)
    t_rand, u = torch.rand(B, nc, generator=g), torch.rand(B, nf, generator=g)
    normals = _device_normals(ops, dev, "e", B, nc, nf)
    model = vd["viewdirs"].ViewdirsModel(nc, nf, noise_std=VD_STD)
    whole = model.apply(st, rays, True, t_rand=t_rand.to(dev), u=u.to(dev), seed=C.SEED)
    clean = vd["viewdirs"].ViewdirsModel(nc, nf).apply(st, rays, True, t_rand=t_rand.to(dev), u=u.to(dev), seed=C.SEED)
    assert not torch.equal(whole[0][0], clean[0][0]) and not torch.equal(whole[1][0], clean[1][0]), "the noise changed nothing"
    z, pts = ops.sample_along_rays(rays.origins, rays.directions, nc, 2.0, 6.0, t_rand.to(dev))
    pieces = []
    for lvl, S in ((0, nc), (1, nc + nf)):
        dirs = rays.viewdirs[:, None, :].expand(B, S, 3).reshape(-1, 3).contiguous()
        raw_rgb, raw_sigma = ops.vd_eval_points_raw(st.packed[lvl][0], pts.reshape(-1, 3), dirs)
        ops.add_gaussian_noise(raw_sigma, VD_STD, noise=normals[lvl])
        comp, disp, acc, w = ops.vd_composite_fwd(model.cfg, raw_rgb, raw_sigma, z, rays.directions)
        pieces.append((comp, disp, acc))
        if lvl == 0:
            z, pts = ops.sample_pdf(z, w, rays.origins, rays.directions, nf, u.to(dev))
    ok = [_same("e", f"pxo_vd_render_fwd against its pieces, ({nc},{nf}) B={B}, default ray block", _equal(whole, pieces))]
    default = ops.get_tuning(ops.TUNE_VD_RAY_BLOCK)
    try:
        ops.set_tuning(ops.TUNE_VD_RAY_BLOCK, 5)
        blocked = model.apply(st, rays, True, t_rand=t_rand.to(dev), u=u.to(dev), seed=C.SEED)
    finally:
        ops.set_tuning(ops.TUNE_VD_RAY_BLOCK, default)
    ok.append(_same("e", f"pxo_vd_render_fwd against its pieces, ({nc},{nf}) B={B}, ray block 5", _equal(blocked, pieces)))
    want = host_render_f64(vd["sd"], host_rays, render_cfg(nc, nf, noise_std=VD_STD), t_rand, u, noise_c=_host(normals[0], B),
                           noise_f=_host(normals[1], B))
    for lvl, got, w64 in zip(("coarse", "fine"), whole, want):
        check_level(f"[e] pxo_vd_render_fwd vs host_render_f64 with the normals injected, ({nc},{nf}) B={B} {lvl}", got, w64)
    assert all(ok)
