"""-m gpu tests of NeRF-SG training (sg_dim > 0 on the HIP path): the fused shading kernel with the lobe gradient against the
float64 twin (tests/_sg_train_oracle.py), pxo_sg_lobes against the host expression, the whole step against the reference's own
train_step with the SG leaves (G1-SG: tests/golden/sg_train_grad.npz), the update wiring of models.train_step on an SgState, resume from a
checkpoint, nerf_sh.train end to end with eval and extraction on its checkpoint, and two ranks sharing the GPU."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _octree_sg_cases as G                                          # noqa: E402
import _sg_train_cases as C                                           # noqa: E402
import _sg_train_oracle as T                                          # noqa: E402
from _helpers import _gpu, _ops, close, make_params, make_rays, pxo_cfg   # noqa: E402
from oracle import nerf_oracle as O                                   # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
PRECISIONS = [("f32", 0), ("bf16x6", 2)]
_worst = {"ratio": 0.0, "edges": 0.0, "partition": 0.0, "step_sg": 0.0, "step_mlp": 0.0}


# ---- 1. the stage kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sp", [0, 257])
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("B,S", [(1, 64), (7, 40), (41, 192), (5, 255)])
@pytest.mark.parametrize("K", [1, 4, 25])
def test_sg_shade_composite_train_against_the_float64_twin(K, B, S, white, n_sp):
    """pxo_sg_shade_composite_train on the lobes of sg_reference.npz (the sharp lobe, raw lambda 30, included) against the twin
    in float64: a partial ray block (B = 1, 7, 5), a partial chunk (S = 40), three chunks (192) and the last-lane edge (255).
    comp_rgb, weights, ray_sse, d_raw_rgb, d_raw_sigma and the sparsity rows: the bounds of test_shade_composite_train_fused,
    unchanged.  d_lobes: relative L2 over [K,4] <= 4 x the relative L2 of the twin run in float32 on the CPU, computed here (4
    rather than G1's 2: a floor estimated from <= 100 entries in one summation order is itself noisy).  Two identical calls
    give bitwise-equal outputs."""
    ops = _ops(); dev = _gpu()
    deg = int(round(np.sqrt(K))) - 1
    cfg = O.Cfg(sh_deg=deg, white_bkgd=white, sparsity_length=0.07, sparsity_weight=2e-3)
    pcfg = pxo_cfg(ops, cfg)
    rays, raw_rgb, raw_sigma, z, px, sp_sigma, sp_rgb = C.stage_inputs(K, B, S, n_sp, C.stage_seed(K, S))
    lobes = torch.from_numpy(G.lobes(K))
    all_rgb = torch.cat([raw_rgb.reshape(B * S, 3 * K), sp_rgb]).to(dev)
    all_sigma = torch.cat([raw_sigma.reshape(-1), sp_sigma]).to(dev)
    args = (pcfg, lobes.to(dev), all_rgb, all_sigma, z.to(dev), rays.directions.to(dev), rays.viewdirs.to(dev), px.to(dev))
    out = ops.sg_shade_composite_train(*args, n_sp=n_sp)
    again = ops.sg_shade_composite_train(*args, n_sp=n_sp)
    ref = T.stage(cfg, rays, raw_rgb, raw_sigma, z, px, lobes, sp_sigma, torch.float64)
    close("comp_rgb", out["comp_rgb"], ref["comp_rgb"], rtol=1e-5, atol=2e-6)
    close("weights", out["weights"], ref["weights"], rtol=1e-4, atol=2e-6)
    close("ray_sse", out["ray_sse"], ref["ray_sse"], rtol=1e-4, atol=1e-7)
    close("d_raw_rgb", out["d_raw_rgb"][:B * S], ref["d_raw_rgb"].reshape(B * S, -1), rtol=1e-4, atol=1e-8)
    close("d_raw_sigma", out["d_raw_sigma"][:B * S], ref["d_raw_sigma"].reshape(-1), rtol=2e-4,
          atol=1e-6 * max(1.0, float(ref["d_raw_sigma"].abs().max())))
    if n_sp:
        close("sparsity d_raw_sigma", out["d_raw_sigma"][B * S:], ref["d_sp_sigma"], rtol=1e-5, atol=1e-12)
        close("sparsity exp", out["sp_exp"][:n_sp], torch.exp(-cfg.sparsity_length * torch.relu(sp_sigma.double())), rtol=1e-6, atol=1e-7)
        assert bool((out["d_raw_rgb"][B * S:] == 0).all())
    want = ref["d_lobes"]
    assert float(want.norm()) > 0
    floor = float((T.stage(cfg, rays, raw_rgb, raw_sigma, z, px, lobes, sp_sigma, torch.float32)["d_lobes"].double() - want).norm()
                  / want.norm())
    rel = float((out["d_lobes"].cpu().double() - want).norm() / want.norm())
    _worst["ratio"] = max(_worst["ratio"], rel / floor)
    print(f"SG{K} B={B} S={S} white={int(white)} n_sp={n_sp}: d_lobes rel L2 {rel:.3e}, float32 twin {floor:.3e}, ratio "
          f"{rel / floor:.2f} (worst so far {_worst['ratio']:.2f})")
    assert rel <= 4 * floor, (rel, floor)
    for k in ("d_lobes", "comp_rgb", "d_raw_rgb", "d_raw_sigma", "ray_sse"):
        assert torch.equal(out[k], again[k]), k


def _run_stage(ops, dev, cfg, inputs, lobes, n_sp, **kw):
    rays, raw_rgb, raw_sigma, z, px, sp_sigma, sp_rgb = inputs
    B, S = z.shape
    all_rgb = torch.cat([raw_rgb.reshape(B * S, -1), sp_rgb]).to(dev)
    all_sigma = torch.cat([raw_sigma.reshape(-1), sp_sigma]).to(dev)
    return ops.sg_shade_composite_train(pxo_cfg(ops, cfg), lobes.to(dev), all_rgb, all_sigma, z.to(dev).contiguous(),
                                        rays.directions.to(dev).contiguous(), rays.viewdirs.to(dev).contiguous(),
                                        px.to(dev).contiguous(), n_sp=n_sp, **kw)


@pytest.mark.parametrize("case", C.STAGE_CASES, ids=C.stage_id)
def test_sg_shade_composite_train_at_lobe_count_chunk_and_stride_edges(case):
    """The edges the product above leaves out (tests/_sg_train_cases.py): K = 9 and 16 (shade_composite_train_kernel<2,true> and
    <3,true>), S = 1, 63, 65 and 256, and 64, 65 and 129 ray blocks (the second stage of the lobe gradient adds the per-block
    partials 64 blocks at a time).  The checks of the test above, unchanged, except that the floor of d_lobes is max(float32
    twin, 1.5e-7): 4 x floor was measured at floors of 1.5e-7 .. 4.1e-7, and a floor estimated from a six-term sum (S = 1 gives
    8e-8 .. 1e-7) is noisier than that.  tests/test_sg_train_cpu.py holds every case to a gradient norm > 1e-4, no all-zero lobe
    row, a float32-twin error < 1e-6, and shows that leaving out the last ray block moves d_lobes by > 10 x the bound.
    Two cases run once more with comp_rgb == weights == NULL (what the fine pass of the step does): bitwise-equal gradients.
    Two run as rows [:256] and [256:]: the pixel-loss scale is 2 / (3B), so d_lobes = (B1 d1 + B2 d2) / B within the same bound
    (against the float64 value of the whole batch), and comp_rgb of each part equals the whole's rows bit for bit."""
    ops = _ops(); dev = _gpu()
    K, B, S, white, n_sp = case
    cfg, inputs, lobes, ref, floor, twin32 = C.stage_reference(case)
    rays, raw_rgb, raw_sigma, z, px, sp_sigma, sp_rgb = inputs
    out = _run_stage(ops, dev, cfg, inputs, lobes, n_sp)
    again = _run_stage(ops, dev, cfg, inputs, lobes, n_sp)
    close("comp_rgb", out["comp_rgb"], ref["comp_rgb"], rtol=1e-5, atol=2e-6)
    close("weights", out["weights"], ref["weights"], rtol=1e-4, atol=2e-6)
    close("ray_sse", out["ray_sse"], ref["ray_sse"], rtol=1e-4, atol=1e-7)
    close("d_raw_rgb", out["d_raw_rgb"][:B * S], ref["d_raw_rgb"].reshape(B * S, -1), rtol=1e-4, atol=1e-8)
    close("d_raw_sigma", out["d_raw_sigma"][:B * S], ref["d_raw_sigma"].reshape(-1), rtol=2e-4,
          atol=1e-6 * max(1.0, float(ref["d_raw_sigma"].abs().max())))
    if n_sp:
        close("sparsity d_raw_sigma", out["d_raw_sigma"][B * S:], ref["d_sp_sigma"], rtol=1e-5, atol=1e-12)
        close("sparsity exp", out["sp_exp"][:n_sp], torch.exp(-cfg.sparsity_length * torch.relu(sp_sigma.double())), rtol=1e-6, atol=1e-7)
        assert bool((out["d_raw_rgb"][B * S:] == 0).all())
    want = ref["d_lobes"]
    assert float(want.norm()) > 0
    rel = float((out["d_lobes"].cpu().double() - want).norm() / want.norm())
    _worst["edges"] = max(_worst["edges"], rel / floor)
    print(f"SG{K} B={B} S={S} white={int(white)} n_sp={n_sp}: d_lobes rel L2 {rel:.3e}, float32 twin {twin32:.3e}, floor {floor:.3e}, "
          f"ratio {rel / floor:.2f} (worst so far {_worst['edges']:.2f})")
    assert rel <= 4 * floor, (rel, floor)
    for k in ("d_lobes", "comp_rgb", "d_raw_rgb", "d_raw_sigma", "ray_sse"):
        assert torch.equal(out[k], again[k]), k
    if (K, B, S) in C.STAGE_NULL_OUTPUTS:
        bare = _run_stage(ops, dev, cfg, inputs, lobes, n_sp, want_rgb=False, want_weights=False)
        assert bare["comp_rgb"] is None and bare["weights"] is None
        for k in ("d_raw_rgb", "d_raw_sigma", "ray_sse", "d_lobes"):
            assert torch.equal(out[k], bare[k]), k
    if (K, B, S) in C.STAGE_PARTITION:
        cut = C.PARTITION_AT
        parts = [_run_stage(ops, dev, cfg, C.stage_rows(inputs, rows), lobes, n_sp) for rows in (slice(0, cut), slice(cut, B))]
        joined = (cut * parts[0]["d_lobes"].cpu().double() + (B - cut) * parts[1]["d_lobes"].cpu().double()) / B
        gap = float((out["d_lobes"].cpu().double() - joined).norm() / want.norm())
        _worst["partition"] = max(_worst["partition"], gap / floor)
        print(f"SG{K} B={B} S={S}: d_lobes whole vs rows [:{cut}] + [{cut}:] {gap:.3e} of the float64 norm, ratio to the floor "
              f"{gap / floor:.2f} (worst so far {_worst['partition']:.2f})")
        assert gap <= 4 * floor, (gap, floor)
        assert torch.equal(parts[0]["comp_rgb"], out["comp_rgb"][:cut]) and torch.equal(parts[1]["comp_rgb"], out["comp_rgb"][cut:])


def test_sg_shade_composite_train_refuses_more_samples_than_its_chunks_hold():
    """S = 257 is one sample past the four chunks of 64: PxoError naming the sample range, nothing launched."""
    ops = _ops(); dev = _gpu()
    from plenoctree_amd._lib import PxoError
    K, B, S = 4, 2, 257
    cfg = C.stage_cfg(K, True)
    with pytest.raises(PxoError, match=r"samples per ray 257 not in \[1,256\]"):
        _run_stage(ops, dev, cfg, C.stage_inputs(K, B, S, 0, C.stage_seed(K, S)), torch.from_numpy(G.lobes(K)), 0)


@pytest.mark.parametrize("K,Nc", [(25, 64), (4, 100), (25, 128)])
def test_fused_forward_equals_the_sg_render_composite(K, Nc):
    """The fused kernel's forward values against pxo_sg_render_fwd's composite of the SAME samples (coarse level of a model
    without a fine level: its sample positions and raw outputs are bit for bit those of pxo_sample_along_rays / pxo_eval_points):
    rtol 1e-6 / atol 1e-7, one and two chunks."""
    ops = _ops(); dev = _gpu()
    deg = int(round(np.sqrt(K))) - 1
    cfg = ops.make_cfg(sh_deg=deg, num_coarse_samples=Nc, num_fine_samples=0)
    flat = make_params(O.Cfg(sh_deg=deg), seed=20 + K, bias_scale=0.2).to(dev)
    n = flat.numel() // 2
    pk0 = ops.pack_weights(cfg, flat[:n].contiguous(), need_bwd=False)[0]
    lobes = torch.from_numpy(G.lobes(K)).to(dev)
    B = 7
    rays = make_rays(B, 3)
    o, d, v = (x.to(dev).contiguous() for x in rays)
    t_rand = torch.rand(B, Nc, generator=torch.Generator().manual_seed(K)).to(dev)
    rgb = ops.render_fwd(cfg, pk0, None, o, d, v, randomized=True, t_rand=t_rand, lobes=lobes)[0][0]
    z, pts = ops.sample_along_rays(o, d, Nc, cfg.near_, cfg.far_, t_rand)
    raw_rgb, raw_sigma = ops.eval_points(cfg, pk0, pts.reshape(-1, 3))
    px = torch.rand(B, 3, generator=torch.Generator().manual_seed(1)).to(dev)
    out = ops.sg_shade_composite_train(cfg, lobes, raw_rgb, raw_sigma.reshape(-1).contiguous(), z, d, v, px)
    assert float((rgb - 1.0).abs().max()) > 0.05                          # the rays see the model
    close("fused vs pxo_sg_render_fwd comp_rgb", out["comp_rgb"], rgb, rtol=1e-6, atol=1e-7)


# ---- 2. the lobes on the device -------------------------------------------------------------------------------------
def test_sg_lobes_kernel_against_the_host_expression():
    """pxo_sg_lobes against sg.lobes_from_params on the parameters of the two fixtures: mu to 4 float32 ulp of 1 (two libm
    calls and a product of values <= 1), lambda to rtol 1e-6; the sharp lobe (30, theta 0) comes out as (30, 0, 0, 1) exactly."""
    ops = _ops(); dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import sg
    g = np.load(os.path.join(GOLDEN, "sg_train_grad.npz"))
    fx = G.fixture()
    cases = [(25, g["sg_lambda"], g["sg_mu_spher"])] + [(K, fx[f"sg_lambda_{K}"], fx[f"sg_mu_spher_{K}"]) for K in G.KS]
    for K, lam, mu in cases:
        lam, mu = torch.tensor(lam).float(), torch.tensor(mu).float()
        got = ops.sg_lobes(torch.cat([lam, mu.reshape(-1)]).to(dev), K).cpu()
        want = sg.lobes_from_params(lam, mu)
        assert tuple(got.shape) == (K, 4)
        np.testing.assert_allclose(got[:, 0].numpy(), want[:, 0].numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(got[:, 1:].numpy(), want[:, 1:].numpy(), rtol=0, atol=4 * 2.0 ** -23)
        if float(lam[0]) == 30.0:
            assert got[0].tolist() == [30.0, 0.0, 0.0, 1.0]


# ---- 3. the whole step (G1-SG) --------------------------------------------------------------------------------------
def _fixture():
    return np.load(os.path.join(GOLDEN, "sg_train_grad.npz")), np.load(os.path.join(GOLDEN, "eval_points_sh25.npz"))


def _step_once(ops, dev, prec=0, skip=0, rows=slice(None)):
    g, gw = _fixture()
    cfg, flat, sgp, rays, px, t_rand, u, sp = T.fixture_inputs(g, gw, torch.float32)
    pcfg = pxo_cfg(ops, cfg)
    pcfg.mlp_precision, pcfg.skip_zero_rows = prec, skip
    flat, sgp = flat.to(dev), sgp.to(dev)
    n = flat.numel() // 2
    packed = [ops.pack_weights(pcfg, flat[i * n:(i + 1) * n].contiguous()) for i in range(2)]
    o, d, v = (x[rows].contiguous().to(dev) for x in rays)
    B = o.shape[0]
    grads, sg_grads, stats = torch.zeros_like(flat), torch.full_like(sgp, 7.0), torch.zeros(6, device=dev)
    ws = torch.empty(ops.sg_train_workspace_bytes(pcfg, B), dtype=torch.uint8, device=dev)
    ops.sg_train_fwd_bwd(pcfg, flat, sgp, packed, o, d, v, px[rows].contiguous().to(dev), grads, sg_grads, stats, ws, randomized=True,
                         t_rand=t_rand[rows].contiguous().to(dev), u=u[rows].contiguous().to(dev), sp_points=sp.to(dev))
    torch.cuda.synchronize()
    from plenoctree_amd.nerf_sh.nerf import utils
    return cfg, dict(zip(utils.Stats._fields, stats.cpu().tolist())), grads.cpu(), sg_grads.cpu()


@pytest.mark.parametrize("prec_name,prec", PRECISIONS)
def test_sg_train_step_against_the_references_train_step(prec_name, prec):
    """G1-SG.  sg_train_grad.npz: float64 reverse-mode AD through the reference's own train_step with sg_dim = 25 (24 rays, 500
    sparsity points, weight decay on; make_golden_sg_grad.py).  Stats: G1's tolerances (rel 2e-5 against the float64 run).  MLP
    gradients: relative L2 per MLP, over the entries the fixture keeps, <= 2 x the reference's own float32-vs-float64 figure
    recorded there, and every leaf within 10 x its MLP's bound (G1's rule).  SG gradient: relative L2 over the 75 entries <= 4 x
    its recorded floor.  skip_zero_rows 0 / 1 and repeated calls: bitwise-equal gradients, SG tail included."""
    ops = _ops(); dev = _gpu()
    g, _ = _fixture()
    cfg, st, grad, sg_grad = _step_once(ops, dev, prec)
    idx, ranges, owner = T.fixture_index(cfg, int(g["grad_stride"]))
    want, got = torch.tensor(g["grad"]).double(), grad.double()[idx]
    n = grad.numel() // 2
    sel = idx < n
    ref32 = (float(g["grad_f32_vs_f64_rel_l2_mlp0"]), float(g["grad_f32_vs_f64_rel_l2_mlp1"]))
    bounds = (2 * ref32[0], 2 * ref32[1])
    rels = [float((got[m] - want[m]).norm() / want[m].norm()) for m in (sel, ~sel)]
    want_sg = torch.tensor(g["sg_grad"])
    rel_sg, floor_sg = float((sg_grad.double() - want_sg).norm() / want_sg.norm()), float(g["grad_f32_vs_f64_rel_l2_sg"])
    print(f"HIP ({prec_name}) vs reference-autograd, SG25: MLP_0 rel L2 {rels[0]:.2e}, MLP_1 {rels[1]:.2e} (the reference's own "
          f"float32: {ref32[0]:.2e} / {ref32[1]:.2e}); SG gradient {rel_sg:.2e} (floor {floor_sg:.2e}, ratio {rel_sg / floor_sg:.2f})")
    for k in ("loss", "loss_c", "weight_l2", "psnr", "psnr_c"):
        assert st[k] == pytest.approx(float(g[k + "_f64"]), rel=2e-5), (k, st[k], float(g[k + "_f64"]))
    assert st["loss_sp"] == pytest.approx(float(g["loss_sp_f64"]), rel=5e-3, abs=1e-9)
    assert rels[0] <= bounds[0] and rels[1] <= bounds[1], rels
    for li, (a0, cnt) in enumerate(ranges):
        a, b = got[a0:a0 + cnt], want[a0:a0 + cnt]
        assert float((a - b).norm()) <= 10 * bounds[owner[li]] * float(b.norm()) + 1e-9, (li, cnt)
    assert rel_sg <= 4 * floor_sg, (rel_sg, floor_sg)
    _, st1, grad1, sg1 = _step_once(ops, dev, prec, skip=1)
    _, st2, grad2, sg2 = _step_once(ops, dev, prec)
    assert torch.equal(grad1, grad) and torch.equal(sg1, sg_grad) and st1 == st
    assert torch.equal(grad2, grad) and torch.equal(sg2, sg_grad) and st2 == st


def _step_case_once(ops, dev, case, prec=0, skip=0):
    """_step_once's calling pattern on the inputs of a tests/_sg_train_cases.py case."""
    cfg, flat, sgp, rays, px, t_rand, u, sp = C.step_inputs(case)
    pcfg = pxo_cfg(ops, cfg)
    pcfg.mlp_precision, pcfg.skip_zero_rows = prec, skip
    flat, sgp = flat.to(dev), sgp.to(dev)
    n = flat.numel() // 2
    packed = [ops.pack_weights(pcfg, flat[i * n:(i + 1) * n].contiguous()) for i in range(2)]
    o, d, v = (x.contiguous().to(dev) for x in rays)
    B = o.shape[0]
    grads, sg_grads, stats = torch.zeros_like(flat), torch.full_like(sgp, 7.0), torch.zeros(6, device=dev)
    ws = torch.empty(ops.sg_train_workspace_bytes(pcfg, B), dtype=torch.uint8, device=dev)
    ops.sg_train_fwd_bwd(pcfg, flat, sgp, packed, o, d, v, px.to(dev), grads, sg_grads, stats, ws, randomized=True,
                         t_rand=t_rand.to(dev), u=u.to(dev) if cfg.num_fine_samples > 0 else None, sp_points=sp.to(dev))
    torch.cuda.synchronize()
    from plenoctree_amd.nerf_sh.nerf import utils
    return dict(zip(utils.Stats._fields, stats.cpu().tolist())), grads.cpu(), sg_grads.cpu()


@pytest.mark.parametrize("case,prec_name,prec", [(c, "f32", 0) for c in C.STEP_CASES] + [(c, "bf16x6", 2) for c in C.STEP_BF16X6],
                         ids=lambda v: C.step_id(v) if isinstance(v, tuple) else None)
def test_sg_train_step_past_64_ray_blocks_at_every_lobe_count(case, prec_name, prec):
    """pxo_sg_train_fwd_bwd against the float64 twin (T.loss_and_grad, computed here once per case) where the fixture of the test
    above does not reach: every lobe count, 65 and 129 ray blocks per pass (the two-pass lobe reduction takes a second and a
    third stride), Nf = 0 (the second pass NULL), weight decay on and off.  Inputs: tests/_sg_train_cases.py.  Stats: G1's
    tolerances.  SG gradient: relative L2 over [3K] <= 4 x the float32 twin's own figure for the case (the rule of the test
    above); each MLP's gradient: relative L2 <= 2 x the float32 twin's (G1's rule; MLP_1 without a fine level and without weight
    decay is exactly zero on both sides).  tests/test_sg_train_cpu.py caps those floors (SG 1e-4, MLP 5e-3) and shows that
    leaving out the last ray block, or either pass, moves the SG gradient by > 10 x the bound.  skip_zero_rows 0 / 1 and a
    repeated call: bitwise equal; no entry of sg_grads keeps its pre-fill."""
    ops = _ops(); dev = _gpu()
    K = case[0]
    want_stats, want, want_sg, floors = C.step_reference(case)
    st, grad, sg_grad = _step_case_once(ops, dev, case, prec)
    n = grad.numel() // 2
    rel = lambda a, b: float((a.double() - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.double().norm())
    rel_sg, rels = rel(sg_grad, want_sg), (rel(grad[:n], want[:n]), rel(grad[n:], want[n:]))
    ratio = lambda a, f: a / f if f > 0 else (0.0 if a == 0 else float("inf"))
    _worst["step_sg"] = max(_worst["step_sg"], ratio(rel_sg, floors[0]))
    _worst["step_mlp"] = max(_worst["step_mlp"], ratio(rels[0], floors[1]), ratio(rels[1], floors[2]))
    print(f"HIP ({prec_name}) vs float64 twin, {C.step_id(case)}: SG gradient {rel_sg:.2e} (float32 twin {floors[0]:.2e}, ratio "
          f"{ratio(rel_sg, floors[0]):.2f}); MLP_0 {rels[0]:.2e} ({floors[1]:.2e}, {ratio(rels[0], floors[1]):.2f}), MLP_1 "
          f"{rels[1]:.2e} ({floors[2]:.2e}, {ratio(rels[1], floors[2]):.2f}); worst so far SG {_worst['step_sg']:.2f}, MLP "
          f"{_worst['step_mlp']:.2f}")
    for k in ("loss", "loss_c", "weight_l2", "psnr", "psnr_c"):
        assert st[k] == pytest.approx(want_stats[k], rel=2e-5), (k, st[k], want_stats[k])
    assert st["loss_sp"] == pytest.approx(want_stats["loss_sp"], rel=5e-3, abs=1e-9)
    assert float(want_sg.norm()) > 0 and not bool((sg_grad == 7.0).any())
    assert rel_sg <= 4 * floors[0], (rel_sg, floors[0])
    assert rels[0] <= 2 * floors[1] and rels[1] <= 2 * floors[2], (rels, floors)
    st1, grad1, sg1 = _step_case_once(ops, dev, case, prec, skip=1)
    st2, grad2, sg2 = _step_case_once(ops, dev, case, prec)
    assert torch.equal(grad1, grad) and torch.equal(sg1, sg_grad) and st1 == st
    assert torch.equal(grad2, grad) and torch.equal(sg2, sg_grad) and st2 == st


# ---- 4. the update and the resume -----------------------------------------------------------------------------------
def _fixture_state(ops, dev, prec=0):
    from plenoctree_amd.nerf_sh.nerf import sg, utils
    g, gw = _fixture()
    cfg, flat, sgp, rays, px, t_rand, u, sp = T.fixture_inputs(g, gw, torch.float32)
    pcfg = pxo_cfg(ops, cfg)
    pcfg.mlp_precision = prec
    K = cfg.sh_dim
    state = sg.SgState(pcfg, flat.to(dev), sgp[:K], sgp[K:].reshape(K, 2))
    batch = {"rays": utils.Rays(*[x.to(dev) for x in rays]), "pixels": px.to(dev)}
    kw = dict(t_rand=t_rand.to(dev), u=u.to(dev), sp_points=sp.to(dev))
    return sg.SgModel(pcfg), state, batch, kw, sgp


def test_train_step_moves_the_sg_parameters_and_refreshes_the_lobes():
    """One models.train_step on an SgState from zero moments is Adam's first step: m_hat = g, v_hat = g^2, so every SG parameter
    moves by lr g / (|g| + 1e-8) -- lr against the sign of its gradient, to the eps of the denominator (1 % at |g| = 1e-6, which is why
    the expected move is written with it) -- checked to rtol 1e-3 wherever |g| > 1e-6; lr = 1e-2 keeps the float32 spacing of the
    parameters (<= 4.8e-7) below that tolerance.  Afterwards the device lobes are pxo_sg_lobes of the new parameters, and the
    host copies behind state.sg_lambda / sg_mu_spher are read back on demand."""
    ops = _ops(); dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import models, sg
    model, state, batch, kw, sgp = _fixture_state(ops, dev)
    K, lr = state.sg_dim, 1e-2
    before, lobes_before = state.sg_params.clone(), state.lobes.clone()
    assert torch.equal(before.cpu(), sgp) and not state.sg_m.any() and not state.sg_v.any()
    models.train_step(model, state, batch, lr, **kw)
    torch.cuda.synchronize()
    gr = state.sg_grads.cpu().double()
    moved = (state.sg_params.cpu().double() - before.cpu().double())
    big = gr.abs() > 1e-6
    assert int(big.sum()) >= 50, int(big.sum())
    expect = -lr * gr / (gr.abs() + 1e-8)
    assert bool((torch.sign(moved[big]) == -torch.sign(gr[big])).all())
    np.testing.assert_allclose(moved[big].numpy(), expect[big].numpy(), rtol=1e-3, atol=0)
    assert float(moved.abs().max()) <= lr * (1 + 1e-3)
    assert state.step == 1 and float(state.sg_m.abs().max()) > 0 and float(state.sg_v.abs().max()) > 0
    assert torch.equal(state.lobes, ops.sg_lobes(state.sg_params, K)) and not torch.equal(state.lobes, lobes_before)
    assert torch.equal(state.sg_lambda, state.sg_params[:K].cpu())
    assert torch.equal(state.sg_mu_spher, state.sg_params[K:].reshape(K, 2).cpu())
    assert state._sg_stale is False


@pytest.mark.parametrize("prec_name,prec", PRECISIONS)
def test_resume_from_a_checkpoint_continues_bit_for_bit(tmp_path, prec_name, prec):
    """Three steps, save, restore into a fresh state, then the same fourth step on both: parameters, SG parameters, every Adam
    moment, the lobes and the stats agree bit for bit (one GPU, the same batch -- through nerf_sh.train a resumed run draws its
    batches from the start of the sampler's stream again, as the reference's does, so the equality is stated here, at the
    step)."""
    ops = _ops(); dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import checkpoints, models, sg
    model, live, batch, kw, _ = _fixture_state(ops, dev, prec)
    for _ in range(3):
        models.train_step(model, live, batch, 5e-4, **kw)
    checkpoints.save_checkpoint(str(tmp_path), live, step=live.step)
    _, back, _, _, _ = _fixture_state(ops, dev, prec)
    back.params.zero_()
    checkpoints.restore_checkpoint(str(tmp_path), back)
    assert back.step == 3 and float(back.sg_m.abs().max()) > 0
    for st in (live, back):
        models.train_step(model, st, batch, 5e-4, **kw)
    torch.cuda.synchronize()
    for name in ("params", "m", "v", "sg_params", "sg_m", "sg_v", "lobes", "stats", "sg_grads", "grads"):
        assert torch.equal(getattr(live, name), getattr(back, name)), name
    for i in range(2):
        assert torch.equal(live.packed[i][0], back.packed[i][0]) and torch.equal(live.packed[i][1], back.packed[i][1])


# ---- 5. nerf_sh.train end to end ------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
def test_train_cli_converges_and_its_checkpoint_feeds_eval_and_extraction(tmp_path):
    """nerf_sh.train.main on the analytic synthetic scene (32 x 32 views), SG25, 256 rays, 60 steps.  The preset is a file with
    the blender preset's values and dataset / batch_size / max_steps set for this run: utils.update_flags lets a preset win
    over the command line, so `--config blender` itself would select the Blender loader, 1024 rays and 2,000,000 steps whatever
    the command line says.  Checked: the mean loss of the last 20 steps is below that of the first 20; the checkpoint holds the
    SG keys and non-zero moments for them; the lobes left init_lobe_params; nerf_sh.eval and octree.extraction (depth 4) run on
    that checkpoint; a second run with max_steps 61 resumes at step 61 and writes checkpoint_61 with moved SG parameters."""
    dev = _gpu()
    from plenoctree_amd.nerf_sh import eval as nerf_eval, train
    from plenoctree_amd.nerf_sh.nerf import checkpoints, sg
    from plenoctree_amd.octree import extraction, svox
    d = str(tmp_path)
    cfg_path = os.path.join(d, "sg_tiny.yaml")

    def write_cfg(max_steps):
        with open(cfg_path, "w") as f:
            f.write("dataset: synthetic\nimage_batching: false\nfactor: 0\nnum_coarse_samples: 64\nnum_fine_samples: 128\n"
                    f"use_viewdirs: false\nwhite_bkgd: true\nbatch_size: 256\nsh_deg: 3\nrandomized: true\nmax_steps: {max_steps}\n")
    write_cfg(60)
    common = ["--train_dir", d, "--config", cfg_path, "--synthetic_hw", "32", "32", "--synthetic_views", "4", "1",
              "--sg_dim", "25", "--sh_deg", "-1"]
    train_flags = ["--print_every", "20", "--save_every", "60", "--render_every", "0"]
    trace = train.main(common + train_flags)
    assert [t[0] for t in trace] == [20, 40, 60]
    first, last = trace[0][4], trace[-1][4]
    print(f"SG25 training, 60 steps x 256 rays: mean loss of steps 1-20 {first:.5f}, of steps 41-60 {last:.5f}")
    assert np.isfinite(last) and last < first, (first, last)
    tree = checkpoints.restore_checkpoint(os.path.join(d, "checkpoint_60"))["optimizer"]
    params, ps = tree["target"]["params"], tree["state"]["param_states"]["params"]
    assert int(np.asarray(tree["state"]["step"]).reshape(-1)[0]) == 60
    lam0, mu0 = sg.init_lobe_params(25)
    assert params["sg_lambda"].shape == (25,) and params["sg_mu_spher"].shape == (25, 2)
    assert np.abs(params["sg_lambda"] - lam0.numpy()).max() > 1e-4 and np.abs(params["sg_mu_spher"] - mu0.numpy()).max() > 1e-4
    for k in ("sg_lambda", "sg_mu_spher"):
        assert np.abs(ps[k]["grad_ema"]).max() > 0 and np.abs(ps[k]["grad_sq_ema"]).max() > 0, k
    psnrs = nerf_eval.main(common + ["--chunk", "1024"])
    assert len(psnrs) == 1 and np.isfinite(psnrs[0])
    out = os.path.join(d, "tree.npz")
    extraction.main(common + ["--output", out, "--init_grid_depth", "4", "--masking_mode", "sigma", "--alpha_thresh", "1e-4",
                              "--samples_per_cell", "8", "--renderer_step_size", "1e-3", "--eval", "false"])
    loaded = svox.N3Tree.load(out, map_location=dev)
    assert str(loaded.data_format) == "SG25" and tuple(loaded.extra_data.shape) == (25, 4)
    want = sg.lobes_from_params(torch.from_numpy(params["sg_lambda"]), torch.from_numpy(params["sg_mu_spher"]))
    assert torch.equal(loaded.extra_data.cpu(), want)
    write_cfg(61)
    trace = train.main(common + ["--print_every", "1", "--save_every", "100", "--render_every", "0"])
    assert [t[0] for t in trace] == [61]
    after = checkpoints.restore_checkpoint(os.path.join(d, "checkpoint_61"))["optimizer"]
    assert int(np.asarray(after["state"]["step"]).reshape(-1)[0]) == 61
    assert not np.array_equal(after["target"]["params"]["sg_lambda"], params["sg_lambda"])
    step = np.abs(after["target"]["params"]["sg_lambda"] - params["sg_lambda"]).max()
    assert step < 1e-4, step                  # one step at the end of the schedule (lr -> 5e-6)


# ---- 6. two ranks on one GPU ----------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_step(rank, world, comm, dev):
    from plenoctree_amd import dist, ops
    from plenoctree_amd.nerf_sh.nerf import models, sg, utils
    model, state, batch, kw, _ = _fixture_state(ops, dev)
    per = 24 // world
    sl = slice(rank * per, (rank + 1) * per)
    batch = {"rays": utils.Rays(*[r[sl].contiguous() for r in batch["rays"]]), "pixels": batch["pixels"][sl].contiguous()}
    reducer = dist.GradReducer(comm, dev) if world > 1 else None
    models.train_step(model, state, batch, 5e-4, t_rand=kw["t_rand"][sl].contiguous(), u=kw["u"][sl].contiguous(),
                  sp_points=kw["sp_points"], world_size=world, reducer=reducer)
    torch.cuda.synchronize()
    s = 1.0 / world
    return dict(sg_grads=state.sg_grads.cpu() * s, grads=state.grads.cpu() * s, sg_params=state.sg_params.cpu(),
                params=state.params.cpu(), stats=state.stats.cpu(), lobes=state.lobes.cpu())


def _worker(rank, world, port, outdir):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from plenoctree_amd import dist
    torch.cuda.set_device(0)
    comm = dist.init_from_env(backend="gloo")
    assert comm.world == world
    torch.save(_rank_step(rank, world, comm, torch.device("cuda", 0)), os.path.join(outdir, f"rank{rank}.pt"))
    comm.barrier()
    comm.shutdown()


@pytest.mark.timeout(600)
def test_two_ranks_on_one_gpu_average_the_sg_gradient_in_bucket1():
    """In the manner of tests/test_gpu_two_ranks_one_gpu.py: 2 x 12 rays of the fixture against 1 x 24, collectives through gloo.
    The replicas are bit-identical after the step (SG parameters and lobes included: the SG gradient went through the exchange,
    inside bucket 1); the averaged SG gradient equals the single-process one to the reorder tolerance that test uses for the MLP
    halves (relative L2 2e-3), as do the MLP halves here."""
    from plenoctree_amd import dist
    world = 2
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(world, _free_port(), outdir), nprocs=world, join=True)
        res = [torch.load(os.path.join(outdir, f"rank{r}.pt")) for r in range(world)]
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    single = _rank_step(0, 1, dist.Comm(), torch.device("cuda", 0))
    for k in ("sg_grads", "grads"):
        a, b = res[0][k].double(), single[k].double()
        rel = float((a - b).norm() / b.norm())
        print(f"2 ranks x 12 rays vs 1 x 24: {k} rel L2 {rel:.2e}")
        assert rel < 2e-3, (k, rel)
    assert float(single["sg_grads"].norm()) > 0
    np.testing.assert_allclose(res[0]["stats"][0].item(), single["stats"][0].item(), rtol=2e-3)
