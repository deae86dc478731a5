"""CPU tests of NeRF-SG training: the new ABI symbols and their argument checks, the flag route of nerf_sh.train, checkpoints
that carry the SG leaves' Adam moments, the layout of the gradient arena, the lobe chain rule of the float64 twin
(tests/_sg_train_oracle.py) against central differences, the twin against the reference's own train_step
(tests/golden/sg_train_grad.npz, written by tests/golden/make_golden_sg_grad.py), and the conditions on the twin that keep the
GPU tests over tests/_sg_train_cases.py from passing vacuously."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _octree_sg_cases as G
import _sg_train_cases as C
import _sg_train_oracle as T
from oracle import nerf_oracle as O
from plenoctree_amd import _lib, build
from plenoctree_amd.nerf_sh.nerf import checkpoints, families, models, sg, utils

NEW_SYMBOLS = ("pxo_sg_lobes", "pxo_sg_shade_composite_train", "pxo_sg_train_workspace_bytes", "pxo_sg_train_fwd_bwd_bucketed",
               "pxo_sg_train_fwd_bwd")


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_sg_training_symbols_in_header_ctypes_table_and_library():
    build.build(verbose=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "plenoctree_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES and re.search(rf"\bT {name}\b", nm), name
    # entry points only: the version, the struct and the sizes every SH caller sees are what they were
    assert int(re.search(r"#define PXO_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.pxo_version() == 9 and lib.pxo_cfg_bytes() == ctypes.sizeof(_lib.PxoCfg) == 17 * 4
    assert int(re.search(r"#define PXO_SG_RAYS_PER_BLOCK (\d+)", hdr).group(1)) == _lib.SG_RAYS_PER_BLOCK
    cfg = _lib.make_cfg(sh_deg=4)
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for B in (1, 24, 4096):
        assert lib.pxo_train_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(a)) == 0
        assert lib.pxo_sg_train_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(b)) == 0
        blocks = -(-B // _lib.SG_RAYS_PER_BLOCK)
        assert a.value < b.value <= a.value + 4 * (100 + 2 * blocks * 100) + 3 * 256, (B, a.value, b.value)


def test_sg_training_argument_checks_need_no_gpu():
    """Null sg_params / sg_grads / lobes: PXO_ERR_ARG (-1) with a message that names the argument; bf16x3: PXO_ERR_UNSUPPORTED (-4);
    a short workspace: PXO_ERR_WORKSPACE (-3) -- all before anything is launched."""
    build.build(verbose=False)
    lib = _lib.load()
    cfg = _lib.make_cfg(sh_deg=4)
    d = ctypes.c_void_p(256)                      # a non-null pointer that is never dereferenced
    assert lib.pxo_sg_lobes(None, 25, d, None) == -1 and b"null sg_params" in lib.pxo_last_error()
    assert lib.pxo_sg_lobes(d, 25, None, None) == -1 and b"null lobes" in lib.pxo_last_error()
    assert lib.pxo_sg_lobes(d, 26, d, None) == -1 and b"K 26" in lib.pxo_last_error()

    def stage(lobes, d_lobes, partials):
        return lib.pxo_sg_shade_composite_train(ctypes.byref(cfg), lobes, d, d, d, d, d, d, 4, 64, None, None, d, d, d, 0, None,
                                                d_lobes, partials, None)
    assert stage(None, d, d) == -1 and b"null lobes" in lib.pxo_last_error()
    assert stage(d, None, d) == -1 and b"null d_lobes" in lib.pxo_last_error()
    assert stage(d, d, None) == -1 and b"lobe_partials" in lib.pxo_last_error()

    def step(sg_params, sg_grads, c=cfg, bucketed=True, ws_bytes=16):
        args = [ctypes.byref(c), d, sg_params, d, d, d, d, d, d, d, d, 4, 1, None, None, None, 0, d, sg_grads, d, d, ws_bytes]
        return lib.pxo_sg_train_fwd_bwd_bucketed(*args, None, None) if bucketed else lib.pxo_sg_train_fwd_bwd(*args, None)
    for bucketed in (True, False):
        assert step(None, d, bucketed=bucketed) == -1 and b"null sg_params" in lib.pxo_last_error()
        assert step(d, None, bucketed=bucketed) == -1 and b"null sg_grads" in lib.pxo_last_error()
    x3 = _lib.make_cfg(sh_deg=4, mlp_precision=_lib.MLP_BF16X3)
    assert step(d, d, x3) == -4 and b"pxo_sg_train_fwd_bwd: training runs in float32" in lib.pxo_last_error()
    assert step(d, d) == -3 and b"pxo_sg_train_fwd_bwd: workspace 16 <" in lib.pxo_last_error()
    # the SH entry point keeps its own name in its messages
    assert lib.pxo_train_fwd_bwd(ctypes.byref(x3), d, d, d, d, d, d, d, d, d, 4, 1, None, None, None, 0, d, d, d, 16, None) == -4
    assert b"pxo_train_fwd_bwd: training runs in float32" in lib.pxo_last_error()


# ---- flags ----------------------------------------------------------------------------------------------------------
def _sg_args(extra=()):
    argv = ["--train_dir", "x", "--config", "blender", "--sg_dim", "25", "--sh_deg", "-1", *extra]
    a = utils.define_flags().parse_args(argv)
    utils.update_flags(a)
    sg.apply_cli(a, argv)
    a.dataset = "synthetic"
    return a


def test_train_flag_check_accepts_the_preset_and_rejects_the_rest_by_name():
    a = _sg_args()
    families.check_flags(families.SG, a, "train")
    families.check(a, "train", world_size=2)
    for mutate, word in ((dict(sg_dim=7), r"sg_dim=7 \(need one of \(1, 4, 9, 16, 25\)"),
                         (dict(sh_deg=3), r"sh_deg=3 \(need -1"),
                         (dict(use_viewdirs=True), "use_viewdirs=true"),
                         (dict(sg_dim=-1), "sg_dim=-1"),
                         (dict(legacy_posenc_order=True), "legacy_posenc_order"),
                         (dict(render_path=True), "LLFF")):
        b = _sg_args()
        vars(b).update(mutate)
        with pytest.raises(NotImplementedError, match="training a NeRF-SG.*" + word):
            families.check_flags(families.SG, b, "train")
        with pytest.raises(NotImplementedError, match="training a NeRF-SG"):
            utils.check_dirs(b, require_batch_size_div=True)          # the directory checks, then the SG row's own
            families.check_flags(families.SG, b, "train")
    with pytest.raises(ValueError, match="Batch size must be divisible"):
        b = _sg_args(); b.batch_size = 1023
        families.check(b, "train", world_size=2)
    with pytest.raises(ValueError, match="train_dir"):
        b = _sg_args(); b.train_dir = None
        families.check(b, "train")
    # the generic check is what it was: it refuses the SG preset by name (nerf_sh.train routes around it for sg_dim > 0)
    with pytest.raises(NotImplementedError, match=r"sg_dim>0 \(spherical gaussians\)"):
        utils.check_flags(_sg_args(), require_batch_size_div=True)


# ---- checkpoints ----------------------------------------------------------------------------------------------------
def _sg_state(K, seed=3, moments=True):
    """An SgState without a GPU, built the way tests/test_sg_cpu.py builds it (object.__new__ and the fields a checkpoint
    touches)."""
    cfg = _lib.make_cfg(sh_deg=sg.head_degree(K))
    g = torch.Generator().manual_seed(seed)
    params = models.init_params(cfg, seed) + 0.01 * torch.randn(models.init_params(cfg, seed).shape, generator=g)
    state = object.__new__(sg.SgState)
    state.cfg, state.params, state.step = cfg, params, 7
    state.m, state.v = torch.zeros_like(params), torch.zeros_like(params)
    state.repack = lambda *a, **k: None
    lam, mu = torch.randn(K, generator=g), torch.rand(K, 2, generator=g) * 3.0
    if moments:
        state.set_lobe_params(lam, mu, torch.randn(3 * K, generator=g) * 1e-3, torch.rand(3 * K, generator=g) * 1e-6)
    else:
        state.set_lobe_params(lam, mu)
    return state


@pytest.mark.parametrize("K", [4, 25])
def test_checkpoint_carries_the_sg_moments_flax(tmp_path, K):
    src = _sg_state(K)
    assert float(src.sg_m.abs().max()) > 0 and float(src.sg_v.abs().max()) > 0
    checkpoints.save_checkpoint(str(tmp_path), src, step=7)
    ps = checkpoints.restore_checkpoint(str(tmp_path))["optimizer"]["state"]["param_states"]["params"]
    assert ps["sg_lambda"]["grad_ema"].shape == (K,) and ps["sg_mu_spher"]["grad_sq_ema"].shape == (K, 2)
    assert np.array_equal(ps["sg_mu_spher"]["grad_ema"].reshape(-1), src.sg_m[K:].numpy())
    assert set(ps["MLP_0"]["Dense_0"]["kernel"]) == set(ps["sg_lambda"]) == {"grad_ema", "grad_sq_ema"}     # same tree shape
    dst = _sg_state(K, seed=99, moments=False)
    checkpoints.restore_checkpoint(str(tmp_path), dst)
    for name in ("params", "sg_params", "sg_m", "sg_v", "sg_lambda", "sg_mu_spher", "lobes"):
        assert torch.equal(getattr(dst, name), getattr(src, name)), name
    assert dst.step == 7 and torch.equal(dst.sg_params, torch.cat([src.sg_lambda, src.sg_mu_spher.reshape(-1)]))
    # a file without the SG moments (what the tree held before training existed: parameters only) loads with zeros
    tree = checkpoints.state_to_tree(src)
    for k in ("sg_lambda", "sg_mu_spher"):
        del tree["optimizer"]["state"]["param_states"]["params"][k]
    old = _sg_state(K, seed=5)
    checkpoints.load_tree_into_state(checkpoints.msgpack_restore(checkpoints.msgpack_serialize(tree)), old)
    assert torch.equal(old.sg_params, src.sg_params) and not old.sg_m.any() and not old.sg_v.any()
    del tree["optimizer"]["state"]
    checkpoints.load_tree_into_state(tree, old)
    assert torch.equal(old.sg_lambda, src.sg_lambda) and not old.sg_m.any() and old.step == 0
    # moments of the wrong shape are refused by name
    tree = checkpoints.state_to_tree(src)
    tree["optimizer"]["state"]["param_states"]["params"]["sg_lambda"]["grad_ema"] = np.zeros(K + 1, np.float32)
    with pytest.raises(ValueError, match="grad_ema of sg_lambda"):
        checkpoints.load_tree_into_state(tree, _sg_state(K))


def test_checkpoint_torch_dict_has_no_moments_and_states_without_them_round_trip(tmp_path):
    K = 25
    src = _sg_state(K)
    torch.save({"model": checkpoints.torch_state_dict_from_state(src)}, str(tmp_path / "nerf.ckpt"))
    dst = _sg_state(K, seed=99)
    assert checkpoints.restore_torch_checkpoint(str(tmp_path), dst).endswith("nerf.ckpt")
    assert torch.equal(dst.sg_params, src.sg_params) and torch.equal(dst.params, src.params)
    assert not dst.sg_m.any() and not dst.sg_v.any()                       # a state dict carries no optimizer state
    # a state that never saw set_lobe_params' moment fields (built by hand, as older callers do) still saves: zeros
    bare = _sg_state(K, moments=False)
    del bare.sg_m, bare.sg_v
    checkpoints.save_checkpoint(str(tmp_path / "bare"), bare, step=1)
    back = _sg_state(K, seed=5)
    checkpoints.restore_checkpoint(str(tmp_path / "bare"), back)
    assert torch.equal(back.sg_lambda, bare.sg_lambda) and not back.sg_m.any() and not back.sg_v.any()


# ---- the gradient arena ---------------------------------------------------------------------------------------------
def test_sg_gradient_lies_inside_bucket1_and_bucket0_is_unchanged(monkeypatch):
    monkeypatch.setattr(models.TrainState, "repack", lambda self, need_bwd=True: None)      # no GPU: no weight images
    K = 25
    cfg = _lib.make_cfg(sh_deg=sg.head_degree(K))
    params = models.init_params(cfg)
    lam, mu = sg.init_lobe_params(K)
    st, plain = sg.SgState(cfg, params, lam, mu), models.TrainState(cfg, params.clone())
    n, e = params.numel(), 4
    assert st.n_mlp == plain.n_mlp == n // 2 and st.params.numel() == n                      # the MLP arena is the MLPs' only
    assert st.bucket0.data_ptr() == st.reduce_buf.data_ptr() and st.bucket0.numel() == plain.bucket0.numel() == n // 2
    assert st.grads.data_ptr() == st.reduce_buf.data_ptr() and st.grads.numel() == plain.grads.numel() == n
    b1 = (st.bucket1.data_ptr(), st.bucket1.data_ptr() + e * st.bucket1.numel())
    assert st.bucket1.data_ptr() == st.reduce_buf.data_ptr() + e * (n // 2)
    assert st.sg_grads.numel() == 3 * K and st.sg_grads.data_ptr() == st.reduce_buf.data_ptr() + e * n
    assert b1[0] <= st.sg_grads.data_ptr() and st.sg_grads.data_ptr() + e * 3 * K <= st.stats.data_ptr()
    assert st.stats.numel() == 6 and st.stats.data_ptr() + e * 6 <= b1[1]
    assert st.bucket1.numel() == plain.bucket1.numel() + 3 * K
    assert st.sg_params.shape == st.sg_m.shape == st.sg_v.shape == (3 * K,)
    assert torch.equal(st.sg_params, torch.cat([lam, mu.reshape(-1)])) and torch.equal(st.sg_lambda, lam)
    # the host copies follow the device parameters once a step has marked them stale
    st.sg_params[0] = 2.5
    st._sg_stale = True
    assert float(st.sg_lambda[0]) == 2.5 and st._sg_stale is False


# ---- the twin -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", G.KS)
def test_lobe_chain_rule_matches_central_differences(K):
    """d lobes / d sg_params of the twin (autograd through softplus and spher2cart) and the closed form the kernel evaluates
    (T.chain_rule) against float64 central differences at the parameters of sg_reference.npz, the sharp lobe (raw lambda = 30,
    theta = 0) included.  f = sum(w * lobes) with random w.  Bound of the central difference with step h = 1e-5: truncation
    h^2 / 6 * |d3f| with the third derivative |d3f| <= 4 max|w| (third derivatives of products of two sines / cosines are
    <= 4, of softplus <= 0.13), plus round-off: each of the two evaluations carries at most ~8 roundings (libm calls,
    products, the 4K-term sum), each <= 2^-52 of S = sum |w * lobes|, divided by h."""
    fx = G.fixture()
    p = torch.cat([torch.tensor(fx[f"sg_lambda_{K}"]).double(), torch.tensor(fx[f"sg_mu_spher_{K}"]).double().reshape(-1)])
    assert float(p[0]) == 30.0 and float(p[K]) == 0.0
    w = torch.randn(K, 4, generator=torch.Generator().manual_seed(K), dtype=torch.float64)
    f = lambda q: float((T.lobes_from_params(q, K) * w).sum())
    q = p.clone().requires_grad_(True)
    (T.lobes_from_params(q, K) * w).sum().backward()
    h = 1e-5
    fd = torch.tensor([(f(p + h * e) - f(p - h * e)) / (2 * h) for e in torch.eye(3 * K, dtype=torch.float64)], dtype=torch.float64)
    tol = h * h / 6 * 4 * float(w.abs().max()) + 8 * 2.0 ** -52 * float((T.lobes_from_params(p, K) * w).abs().sum()) / h
    print(f"K={K}: autograd vs central differences {float((q.grad - fd).abs().max()):.3g} (bound {tol:.3g})")
    assert float((q.grad - fd).abs().max()) <= tol, (float((q.grad - fd).abs().max()), tol)
    assert float((T.chain_rule(w, p) - q.grad).abs().max()) < 1e-14
    assert abs(float(q.grad[0]) - float(w[0, 0])) < 1e-12                   # sigmoid(30) = 1 - 9e-14: the sharp lobe is not clipped


def test_twin_against_the_references_train_step_with_sg_leaves(golden_dir):
    """tests/golden/sg_train_grad.npz: reverse-mode AD (torch) through the REFERENCE'S OWN train_step / loss_fn / NerfModel.
    __call__ / eval_sg bodies with sg_dim = 25 (tests/golden/make_golden_sg_grad.py).  The twin must give the same gradient in
    float64: 2e-7 leaf by leaf (G1's float64 bound; the MLP entries are stored as float32, 6e-8 per element, over the entries
    T.fixture_index keeps), the two SG leaves included, and the same six stats."""
    g = np.load(os.path.join(golden_dir, "sg_train_grad.npz"))
    gw = np.load(os.path.join(golden_dir, "eval_points_sh25.npz"))
    cfg, flat, sgp, rays, px, t_rand, u, sp = T.fixture_inputs(g, gw, torch.float64)
    K = cfg.sh_dim
    assert K == 25 and sgp.numel() == 75
    _, stats, grad, sg_grad = T.loss_and_grad(flat, sgp, rays, px, cfg, t_rand, u, sp)
    idx, ranges, _ = T.fixture_index(cfg, int(g["grad_stride"]))
    want, got = torch.tensor(g["grad"]).double(), grad[idx]
    assert want.numel() == idx.numel() == 194200
    assert float(grad.norm()) == pytest.approx(float(g["grad_norm_f64"]), rel=1e-6)
    for li, (a0, cnt) in enumerate(ranges):
        a, b = got[a0:a0 + cnt], want[a0:a0 + cnt]
        assert float(b.norm()) > 0, li
        assert float((a - b).norm()) <= 2e-7 * float(b.norm()) + 1e-12, (li, float((a - b).norm() / b.norm()))
    want_sg = torch.tensor(g["sg_grad"])
    assert want_sg.dtype == torch.float64
    for name, sl in (("sg_lambda", slice(0, K)), ("sg_mu_spher", slice(K, 3 * K))):
        a, b = sg_grad[sl], want_sg[sl]
        assert float((a - b).norm()) <= 2e-7 * float(b.norm()), (name, float((a - b).norm() / b.norm()))
    for k in ("loss", "loss_c", "loss_sp", "weight_l2", "psnr", "psnr_c"):
        assert float(stats[k]) == pytest.approx(float(g[k + "_f64"]), rel=1e-9), k
    # the fixture cannot be vacuous: weight_l2 counts the 75 SG entries, and the loss reaches (nearly) every lobe
    n_all = flat.numel() + 3 * K
    assert float(g["weight_l2_f64"]) == pytest.approx(float((flat ** 2).sum() + (sgp ** 2).sum()) / n_all, rel=1e-12)
    per_lobe = (want_sg[:K] ** 2 + (want_sg[K:].reshape(K, 2) ** 2).sum(-1)).sqrt()
    assert int((per_lobe > 1e-4 * per_lobe.max()).sum()) >= 20
    # the twin in float32 is no further from float64 than the reference's own float32 run (3 x, as G1's CPU test allows)
    cfg, flat, sgp, rays, px, t_rand, u, sp = T.fixture_inputs(g, gw, torch.float32)
    _, _, _, sg32 = T.loss_and_grad(flat, sgp, rays, px, cfg, t_rand, u, sp)
    rel = float((sg32.double() - want_sg).norm() / want_sg.norm())
    print(f"twin float32 SG gradient vs float64: {rel:.3e} (the reference's own float32: {float(g['grad_f32_vs_f64_rel_l2_sg']):.3e})")
    assert rel < 3 * float(g["grad_f32_vs_f64_rel_l2_sg"])


# ---- the cases of tests/test_gpu_sg_train.py cannot pass vacuously --------------------------------------------------------------
def test_stage_case_lists_name_cases_that_exist():
    have = {c[:3] for c in C.STAGE_CASES}
    assert len(have) == len(C.STAGE_CASES) == 12 and set(C.STAGE_NULL_OUTPUTS) <= have and set(C.STAGE_PARTITION) <= have
    assert {c[0] for c in C.STAGE_CASES} == set(G.KS) and {c[2] for c in C.STAGE_CASES} >= {1, 63, 65, 256}
    assert {-(-c[1] // C.RAYS_PER_BLOCK) for c in C.STAGE_CASES} >= {64, 65, 129}
    assert {c[3] for c in C.STAGE_CASES} == {True, False} and {c[4] for c in C.STAGE_CASES} == {0, 257}
    assert all(c[1] > C.PARTITION_AT for c in C.STAGE_CASES if c[:3] in C.STAGE_PARTITION)
    assert not any(c[0] == 1 and c[2] == 1 for c in C.STAGE_CASES)       # K = 1 at S = 1: the sharp lobe alone, |d_lobes| = 6e-11
    assert C.RAYS_PER_BLOCK == _lib.SG_RAYS_PER_BLOCK
    assert {c[0] for c in C.STEP_CASES} == set(G.KS) and all(-(-c[1] // C.RAYS_PER_BLOCK) in (65, 129) for c in C.STEP_CASES)
    assert any(c[3] == 0 for c in C.STEP_CASES) and {c[4] > 0 for c in C.STEP_CASES} == {True, False}


@pytest.mark.parametrize("case", C.STAGE_CASES, ids=C.stage_id)
def test_stage_cases_have_a_lobe_gradient_worth_comparing(case):
    """On the twin alone: |d_lobes| > 1e-4, no all-zero lobe row, and the float32 twin within 1e-6 of the float64 one (so that
    4 x floor stays a bound that a wrong kernel misses).  Past 64 ray blocks, d_lobes without the last ray block's rays (the
    loss scale of the full batch kept) differs from the full one by >= 10 x the bound of the GPU test: a second stage that drops
    its last block fails there."""
    K, B, S, white, n_sp = case
    cfg, inputs, lobes, ref, floor, twin32 = C.stage_reference(case)
    d = ref["d_lobes"]
    assert tuple(d.shape) == (K, 4) and float(d.norm()) > 1e-4, float(d.norm())
    assert bool((d.abs().amax(dim=-1) > 0).all())
    assert twin32 < 1e-6 and C.LOBE_FLOOR <= floor < 1e-6, (twin32, floor)
    nb = -(-B // C.RAYS_PER_BLOCK)
    if nb > 64:
        rows = C.last_block(B)
        assert rows.start == (nb - 1) * C.RAYS_PER_BLOCK and 1 <= B - rows.start <= C.RAYS_PER_BLOCK
        share = C.stage_twin(cfg, C.stage_rows(inputs, rows), lobes, torch.float64)["d_lobes"] * ((B - rows.start) / B)
        head = C.stage_twin(cfg, C.stage_rows(inputs, slice(0, rows.start)), lobes, torch.float64)["d_lobes"] * (rows.start / B)
        assert float((head + share - d).norm()) <= 1e-12 * float(d.norm())            # the loss is a sum over rays
        print(f"{C.stage_id(case)}: the last ray block carries {float(share.norm() / d.norm()):.3e} of d_lobes, 10 x bound {40 * floor:.3e}")
        assert float(share.norm()) >= 10 * 4 * floor * float(d.norm())


@pytest.mark.parametrize("case", C.STEP_CASES, ids=C.step_id)
def test_step_cases_keep_their_bounds_tight_and_see_a_dropped_block_or_pass(case):
    """On the twin alone.  Caps (not tolerances) on the float32 twin's own error, which the GPU test multiplies by 4 (SG) and 2
    (MLP): SG <= 1e-4, each MLP <= 5e-3.  The float64 SG gradient with the last ray block left out (the loss scale of the full B
    kept), with the first pass left out and with the second pass left out each differ from the full gradient by >= 10 x the SG
    bound of the GPU test: a reduction that drops its last block, part_a or part_b fails there."""
    K, B, Nc, Nf, wd = case
    stats, grad, sg_grad, floors = C.step_reference(case)
    print(f"{C.step_id(case)}: float32 twin vs float64: SG {floors[0]:.3e}, MLP_0 {floors[1]:.3e}, MLP_1 {floors[2]:.3e}")
    assert 0 < floors[0] <= 1e-4 and 0 < floors[1] <= 5e-3 and floors[2] <= 5e-3, floors
    n = grad.numel() // 2
    assert float(grad[:n].norm()) > 0 and (float(grad[n:].norm()) > 0) == (Nf > 0 or wd > 0)
    bound = 4 * floors[0] * float(sg_grad.norm())
    first, second = C.step_pass_gradients(case)
    assert (second is None) == (Nf == 0)
    cfg, flat, sgp, *_ = C.step_inputs(case, torch.float64)
    decay = wd * 2.0 * sgp / (flat.numel() + sgp.numel())
    total = first + (0 if second is None else second) + decay
    assert float((total - sg_grad).norm()) <= 1e-12 * float(sg_grad.norm())           # the passes and the decay are all there is
    last = C.step_rows_gradient(case, C.last_block(B))
    print(f"{C.step_id(case)}: shares of the SG gradient: last ray block {float(last.norm() / sg_grad.norm()):.3e}, first pass "
          f"{float(first.norm() / sg_grad.norm()):.3e}, second pass "
          f"{'-' if second is None else format(float(second.norm() / sg_grad.norm()), '.3e')}; 10 x bound {40 * floors[0]:.3e}")
    assert float(last.norm()) >= 10 * bound and float(first.norm()) >= 10 * bound
    assert second is None or float(second.norm()) >= 10 * bound
    if wd > 0:
        assert float(decay.norm()) >= 10 * bound                                      # the weight-decay term would be missed too
