"""The conditions under which tests/test_gpu_noise.py means something, checked on the oracle alone (no GPU).

1. _helpers.philox_normal, the host restatement of the normals pxo_add_gaussian_noise draws, against known answers.
2. For every training case of tests/_noise_cases.py, at the float32 oracle's own sample positions (standing in for the
   device's) and the restated normals of Philox(7, 3 | 4): e_f32, the float32 oracle's gradient error against the float64
   oracle at the same positions and normals (relative L2 per MLP), is <= 4e-3, so the GPU test's gradient bound
   max(1e-3, 3 e_f32) stays <= 1.2e-2; the float64 gradient norm is > 1e-4.
3. Each mistake the GPU test exists to catch moves at least one quantity it asserts by >= 10 x that quantity's bound there
   (loss and loss_c: 1e-7 + 1e-5 |value|; an MLP's gradient: max(1e-3, 3 e_f32) relative L2; loss_sp: asserted bit-identical
   to the noise-free call, so its bound is one float32 ulp, 1.2e-7 relative):
     roll    the last level's normals rolled by one element (an element index off by one)
     stream3 the fine level given stream 3's normals
     no-c / no-f   the noise left out of the coarse / the fine level
     sparsity      the noise also added to the sparsity sigmas (the next 300 elements of the last level's stream)
   A case that fails 2 or 3 is to be replaced by another seed or ray count, never loosened.

Measured here.  Under each mistake: the move as a multiple of the GPU test's bound, the largest over loss, loss_c and both
gradients.  Under `sparsity`: loss_sp's move in float32 ulps, and in brackets the largest gradient multiple, which stays below
10: the sparsity term is 1e-3 of the loss, so only loss_sp's bit identity sees that mistake.

  case                       loss f32 vs f64  e_f32 MLP_0 / MLP_1   roll     stream3  no-c     no-f     sparsity
  i-48x64+128-std0.3         8.7e-08          9.5e-05 / 6.1e-04     4.0e+02  1.0e+02  4.1e+02  7.8e+01  1.8e+04 [0.1]
  ii-llff-ndc-64x16+32-std1  9.5e-08          3.3e-05 / 2.7e-05     1.7e+02  2.4e+02  5.7e+02  8.2e+02  1.8e+06 [0.1]
  iii-coarse-only            2.2e-07          9.5e-05 / -           3.3e+02  -        4.1e+02  -        1.0e+05 [0.1]
  iv-5x13+20-sh4-std1        2.6e-07          1.8e-03 / 8.6e-05     5.1e+02  2.4e+03  6.7e+02  5.1e+03  7.0e+05 [0.4]
  v-bf16x6                   the host inputs of case i
  vi-weight-decay            8.7e-08          9.5e-05 / 6.1e-04     4.0e+02  1.0e+02  4.1e+02  7.8e+01  1.8e+04 [0.1]
  lindisp-noise-off          1.8e-07          9.9e-04 / 1.6e-04     (no noise: condition 2 only)
  lindisp-std0.3             2.3e-07          9.7e-04 / 2.6e-04     7.0e+02  7.5e+02  4.2e+02  5.4e+02  1.8e+04 [0.1]

Case ii draws its 64 NDC rays of llff_tiny through the CPU stand-in of the feeder; case iv's MLP_0 is why a flat 1e-3 cannot
be asked of the gradient (5 rays: the oracle's own float32 is 1.8e-3 away).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _noise_cases as C                                              # noqa: E402
from _helpers import philox_normal                                    # noqa: E402
from oracle import nerf_oracle as O                                   # noqa: E402

F32_ULP = 2.0 ** -23


@pytest.fixture(autouse=True, scope="module")
def _llff_cpu_feeder():
    """LLFF datasets on a CPU device get the stand-in with the NDC methods (as in tests/test_llff_cpu.py)."""
    from _llff_cpu_feeder import feeder_for
    from plenoctree_amd.nerf_sh.nerf import llff
    llff.LLFF.feeder_factory = staticmethod(feeder_for)
    yield
    del llff.LLFF.feeder_factory


def test_philox_normal_known_answers():
    """Elements 0..3 of stream (seed 0, stream 0) are Box-Muller of the first Random123 vector (counter 0, key 0; the words
    test_host_cpu.py pins philox4x32_10 to), spelt out here with `math` on the literal words; a slice that starts inside a quad
    equals the same slice of the whole draw, bit for bit, for a 64-bit seed and stream as well."""
    w = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    want = []
    for h in range(2):
        u1, u2 = ((w[2 * h] >> 8) + 1) / 2.0 ** 24, (w[2 * h + 1] >> 8) / 2.0 ** 24
        r = math.sqrt(-2.0 * math.log(u1))
        want += [r * math.cos(2 * math.pi * u2), r * math.sin(2 * math.pi * u2)]
    got = philox_normal(0, 0, 4)
    assert got.dtype == np.float64 and got.shape == (4,)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    # the same four numbers as literals (first pair: u1 = 0.399046, r = 1.3555, u2 = 0.880520, angle 5.5325 rad)
    np.testing.assert_allclose(got, [0.9911374751458971, -0.9246627803544332, -0.6176090549848544, -0.4820683472644963], rtol=0,
                               atol=1e-12)
    assert np.array_equal(philox_normal(0, 0, 3), got[:3]) and np.array_equal(philox_normal(0, 0, 1, first=3), got[3:])
    for seed, sid in ((C.SEED, C.STREAM_FINE), (0x1234567_89ABCDEF, (1 << 40) + 5)):
        whole = philox_normal(seed, sid, 50)
        for first, n in ((6, 37), (1, 3), (5, 1), (8, 42), (47, 3)):
            assert np.array_equal(philox_normal(seed, sid, n, first=first), whole[first:first + n]), (first, n)
    assert abs(float(philox_normal(9, 3, 4096).mean())) < 0.06 and abs(float(philox_normal(9, 3, 4096).std()) - 1.0) < 0.05


def _key(name):
    c = C.case(name)
    return tuple(sorted((k, v) for k, v in c.items() if k != "prec"))      # bf16x6 changes nothing on the host


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(case, inputs, z_c, z_f, N_c, N_f, float64 (loss, loss_c, grad), float32 the same) at the float32 oracle's own positions."""
    c = dict(key)
    inputs = C.train_inputs(c)
    cfg, flat, rays, px, t_rand, u, sp = inputs
    n_c, n_f = C.host_normals(c["B"], c["Nc"], c["Nf"]) if c["std"] else (None, None)
    with torch.no_grad():
        _, aux = O.render(O.unflatten_params(flat, cfg), rays, cfg, t_rand, u if c["Nf"] > 0 else None, return_aux=True,
                          noise_c=n_c, noise_f=n_f)
    z_c, z_f = aux["z_c"], aux.get("z_f")
    r64 = C.oracle_at(inputs, z_c, z_f, n_c, n_f)
    r32 = C.oracle_at(inputs, z_c, z_f, n_c, n_f, dtype=torch.float32)
    return c, inputs, z_c, z_f, n_c, n_f, r64, r32


ALL = list(C.TRAIN_CASES) + list(C.LINDISP_CASES)


@pytest.mark.parametrize("name", ALL)
def test_float32_oracle_stays_under_the_cap(name):
    c, inputs, z_c, z_f, n_c, n_f, (l64, lc64, g64), (l32, lc32, g32) = _reference(_key(name))
    fine = c["Nf"] > 0
    e = C.rel_l2_per_mlp(g32, g64, fine)
    n = g64.numel() // 2
    norms = [float(g64[:n].norm())] + ([float(g64[n:].norm())] if fine else [])
    print(f"{name}: loss f32 vs f64 {abs(l32 - l64) / l64:.1e}; e_f32 MLP_0 {e[0]:.1e}" + (f" / MLP_1 {e[1]:.1e}" if fine else "")
          + f" (cap {C.E_F32_CAP:.0e}); float64 gradient norms {norms}")
    assert all(x > 1e-4 for x in norms), norms
    assert all(x <= C.E_F32_CAP for x in e if x is not None), e
    assert abs(l32 - l64) <= 0.1 * (C.LOSS_ATOL + C.LOSS_RTOL * abs(l64))        # the oracle's float32 leaves the loss bound 90 %


def _sparsity_term(inputs, noise):
    """(loss_sp, its gradient) in float64 with `noise` [300] (or None) added, times noise_std, to the sparsity points' raw sigma."""
    cfg, flat, rays, px, t_rand, u, sp = inputs
    p = flat.double().requires_grad_(True)
    _, sig = O.eval_points_raw(O.unflatten_params(p, cfg), sp.double(), cfg)
    if noise is not None:
        sig = sig + cfg.noise_std * noise.double().reshape(sig.shape)
    loss = cfg.sparsity_weight * (1.0 - torch.exp(-cfg.sparsity_length * torch.relu(sig)).mean())
    loss.backward()
    return float(loss), p.grad


@pytest.mark.parametrize("name", [k for k in ALL if C.case(k)["std"]])
def test_each_mistake_moves_an_asserted_quantity_by_ten_bounds(name):
    c, inputs, z_c, z_f, n_c, n_f, (l64, lc64, g64), (l32, lc32, g32) = _reference(_key(name))
    B, Nc, Nf = c["B"], c["Nc"], c["Nf"]
    fine = Nf > 0
    S = Nc + Nf
    e_f32 = C.rel_l2_per_mlp(g32, g64, fine)
    roll = lambda t: torch.roll(t.reshape(-1), 1).reshape(t.shape)
    mutations = {"roll": (n_c, roll(n_f)) if fine else (roll(n_c), None), "no-c": (None, n_f)}
    if fine:
        mutations["stream3"] = (n_c, torch.from_numpy(philox_normal(C.SEED, C.STREAM_COARSE, B * S)).float().reshape(B, S))
        mutations["no-f"] = (n_c, None)
    report = []
    for tag, (mc, mf) in mutations.items():
        l, lc, g = C.oracle_at(inputs, z_c, z_f, mc, mf)
        moved = [abs(l - l64) / (C.LOSS_ATOL + C.LOSS_RTOL * abs(l64))]
        if fine:
            moved.append(abs(lc - lc64) / (C.LOSS_ATOL + C.LOSS_RTOL * abs(lc64)))
        moved += [d / C.grad_bound(e) for d, e in zip(C.rel_l2_per_mlp(g, g64, fine), e_f32) if d is not None]
        report.append(f"{tag} {max(moved):.1e}")
        assert max(moved) >= 10.0, (tag, moved)
    # noise on the sparsity rows that share the last pass's buffer: elements B*S .. B*S + 300 of that level's stream
    last_stream, n_ray = (C.STREAM_FINE, B * S) if fine else (C.STREAM_COARSE, B * Nc)
    n_sp = torch.from_numpy(philox_normal(C.SEED, last_stream, C.N_SPARSITY, first=n_ray)).float()
    (sp0, gs0), (sp1, gs1) = _sparsity_term(inputs, None), _sparsity_term(inputs, n_sp)
    ulps = abs(sp1 - sp0) / (F32_ULP * sp0)
    g_moved = max(d / C.grad_bound(e) for d, e in zip(C.rel_l2_per_mlp(g64 + gs1 - gs0, g64, fine), e_f32) if d is not None)
    report.append(f"sparsity {ulps:.1e} [{g_moved:.1f}]")
    print(f"{name}: " + "  ".join(report))
    assert sp0 > 0 and ulps >= 10.0, (sp0, sp1)
