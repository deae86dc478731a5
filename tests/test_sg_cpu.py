"""CPU tests of the spherical-Gaussian (SG) chain: the basis against the reference's own eval_sg (fixture
tests/golden/sg_reference.npz, written by tests/golden/make_golden_sg.py), checkpoints with the SG keys in both wire formats,
SG trees in the svox mirror (construction, save / load, compression pass-through, refusals), the flag checks, the ABI symbols,
and the conditions that keep the GPU forward test (tests/test_gpu_sg.py) from passing vacuously."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _octree_sg_cases as G
from oracle import octree_oracle as T
from plenoctree_amd import _lib, build
from plenoctree_amd.nerf_sh.nerf import checkpoints, families, models, sg, utils
from plenoctree_amd.octree import compression, evaluation, extraction, svox

f32 = np.float32
EPS = 2.0 ** -24                 # float32 unit round-off


# ---- the basis ------------------------------------------------------------------------------------------------------
def test_lobes_from_params_match_the_references_expression():
    """float32 softplus / sin / cos on the host against the float64 fixture (extraction.py:439-442).  Bound: lambda is one
    correctly rounded libm call on an exact input plus the rounding of the result, <= 2 ulp relative -> 4 EPS * lambda; a
    component of mu is at most two roundings of values <= 1 and one product, <= 3 ulp(1) absolute -> 6 EPS."""
    fx = G.fixture()
    for K in G.KS:
        got = sg.lobes_from_params(torch.from_numpy(fx[f"sg_lambda_{K}"]), torch.from_numpy(fx[f"sg_mu_spher_{K}"]))
        assert got.dtype == torch.float32 and tuple(got.shape) == (K, 4)
        want = fx[f"lobes_{K}"]
        err = np.abs(got.numpy().astype(np.float64) - want)
        assert (err[:, 0] <= 4 * EPS * want[:, 0]).all(), (K, err[:, 0].max())
        assert err[:, 1:].max() <= 6 * EPS, (K, err[:, 1:].max())
        assert np.abs(np.linalg.norm(got.numpy().astype(np.float64)[:, 1:], axis=1) - 1.0).max() < 4 * EPS
        assert float(got[0, 0]) == 30.0 and got[0, 1:].tolist() == [0.0, 0.0, 1.0]          # the sharp lobe sits on +z exactly
        if K >= 4:
            assert abs(float(got[1, 0]) - 0.0067153485) < 1e-8                              # softplus(-5)
    with pytest.raises(ValueError, match="sg_mu_spher"):
        sg.lobes_from_params(torch.zeros(4), torch.zeros(3, 2))


def test_sg_basis_matches_the_references_eval_sg():
    """sg_basis_np (float32, the kernels' order) and the colour sums built on it against eval_sg in float64.

    Bound, from K, the lobes and the coefficient range alone.  With the same float32 lobes and direction the float32 basis
    differs from the exact one by: the dot product (three products, two sums of values <= 1: <= 5 EPS absolute, times lambda
    in the exponent), the subtraction and the product with lambda (<= 2 EPS relative on an exponent a = lambda (dot - 1) <= 0),
    expf and the final product (<= 3 EPS relative).  Relative to 1/K that is at most
        lambda * 5 EPS * e^a + |a| e^a * 2 EPS + 3 EPS <= (5 lambda_max + 2 / e + 3) EPS,
    because e^a <= 1 and |a| e^a <= 1 / e.  Rounding the float64 lobes of the fixture to float32 adds lambda_max * 3 EPS (mu) and
    |a| e^a EPS (lambda) in the same units.  The sharp lobe (lambda = 30) sits on +z exactly, mu = (0, 0, 1): its dot product
    is d_z with no rounding at all, so the lambda that multiplies the dot-product error is the largest one among the OTHER
    lobes, lambda_eff <= softplus(4) = 4.02.  A colour sum has K terms of at most c / K each plus K - 1 additions of partial
    sums <= c:  bound = c * ((8 lambda_eff + 5) EPS + K EPS) = 7.4e-6 for K = 25, c = 2: a few float32 ulps (1.2e-7 at c) per
    term of the sum."""
    fx = G.fixture()
    c = float(fx["coef_range"])
    dirs = fx["dirs"]
    for K in G.KS:
        lobes = G.lobes(K)
        assert lobes[0].tolist() == [30.0, 0.0, 0.0, 1.0] and float(np.abs(fx[f"coeffs_{K}"]).max()) <= c
        lam_max = float(lobes[1:, 0].max()) if K > 1 else 0.0          # lambda_eff: the lobes whose dot product is rounded
        assert lam_max <= 4.02
        basis = np.stack([T.sg_basis_np(lobes, d) for d in dirs])
        assert basis.dtype == f32
        tol_basis = (8 * lam_max + 5) * EPS / K
        err = np.abs(basis.astype(np.float64) - fx[f"basis_{K}"])
        print(f"K={K}: basis err {err.max():.3g} (bound {tol_basis:.3g})")
        assert err.max() <= tol_basis, (K, err.max(), tol_basis)
        assert np.abs(T.sg_basis_f64(lobes, dirs) - fx[f"basis_{K}"]).max() <= tol_basis
        # parallel to the sharp lobe: exactly 1/K; anti-parallel: exp(-60), towards 0 without becoming inf / nan
        assert basis[0, 0] == f32(1.0) / f32(K) and 0.0 <= basis[1, 0] < 1e-25
        if K >= 4:                                                  # the nearly flat lobe: 1/K everywhere to 1.4 %
            assert np.abs(basis[:, 1] * K - 1.0).max() < 0.014
        out = np.zeros((len(dirs), 3), f32)
        for n in range(len(dirs)):
            for ch in range(3):
                acc = f32(0.0)
                for i in range(K):
                    acc = f32(acc + f32(basis[n, i] * fx[f"coeffs_{K}"][n, ch, i]))
                out[n, ch] = acc
        tol = c * ((8 * lam_max + 5) * EPS + K * EPS)
        err = np.abs(out.astype(np.float64) - fx[f"out_{K}"])
        print(f"K={K}: colour err {err.max():.3g} (bound {tol:.3g})")
        assert err.max() <= tol, (K, err.max(), tol)


# ---- checkpoints ----------------------------------------------------------------------------------------------------
def _sg_args(extra=()):
    argv = ["--train_dir", "x", "--config", "blender", "--sg_dim", "25", "--sh_deg", "-1", *extra]
    a = utils.define_flags().parse_args(argv)
    utils.update_flags(a)
    assert a.sh_deg == 3                    # the preset wins in update_flags ...
    sg.apply_cli(a, argv)                   # ... and the SG flags of the command line are applied again
    a.dataset = "synthetic"
    return a


def _sg_state(K, seed=3):
    cfg = _lib.make_cfg(sh_deg=sg.head_degree(K))
    g = torch.Generator().manual_seed(seed)
    params = models.init_params(cfg, seed) + 0.01 * torch.randn(models.init_params(cfg, seed).shape, generator=g)
    lam = torch.randn(K, generator=g)
    mu = torch.rand(K, 2, generator=g) * 3.0
    state = object.__new__(sg.SgState)       # no GPU here: the fields a checkpoint touches, without the packed images
    state.cfg, state.params, state.step = cfg, params, 7
    state.m, state.v = torch.zeros_like(params), torch.zeros_like(params)
    state.repack = lambda *a, **k: None
    state.set_lobe_params(lam, mu)
    return state


def _plain_state(K):
    s = _sg_state(K)
    t = object.__new__(models.TrainState)
    t.cfg, t.params, t.step, t.m, t.v = s.cfg, s.params.clone(), 0, s.m.clone(), s.v.clone()
    t.repack = lambda *a, **k: None
    return t


@pytest.mark.parametrize("K", [4, 25])
def test_checkpoint_round_trip_with_sg_keys_flax(tmp_path, K):
    src = _sg_state(K)
    path = checkpoints.save_checkpoint(str(tmp_path), src, step=7)
    raw = checkpoints.restore_checkpoint(str(tmp_path))["optimizer"]["target"]["params"]
    assert raw["sg_lambda"].shape == (K,) and raw["sg_mu_spher"].shape == (K, 2) and raw["sg_lambda"].dtype == np.float32
    dst = _sg_state(K, seed=99)
    assert not torch.equal(dst.sg_lambda, src.sg_lambda)
    assert checkpoints.restore_checkpoint(str(tmp_path), dst) == path
    assert torch.equal(dst.params, src.params) and dst.step == 7
    assert torch.equal(dst.sg_lambda, src.sg_lambda) and torch.equal(dst.sg_mu_spher, src.sg_mu_spher)
    assert torch.equal(dst.lobes, sg.lobes_from_params(src.sg_lambda, src.sg_mu_spher))
    # a model without SG refuses the file by the key's name; an SG model refuses a file without the keys
    with pytest.raises(ValueError, match="sg_lambda"):
        checkpoints.restore_checkpoint(str(tmp_path), _plain_state(K))
    plain_dir = tmp_path / "plain"
    checkpoints.save_checkpoint(str(plain_dir), _plain_state(K), step=1)
    with pytest.raises(ValueError, match="sg_lambda.*not a NeRF-SG checkpoint"):
        checkpoints.restore_checkpoint(str(plain_dir), _sg_state(K))
    # the lobe count must be the model's
    with pytest.raises(ValueError, match="sg_dim"):
        other = _sg_state(K)
        other.cfg = _lib.make_cfg(sh_deg=sg.head_degree(K))
        tree = checkpoints.state_to_tree(src)
        tree["optimizer"]["target"]["params"]["sg_lambda"] = np.zeros(K + 1, f32)
        checkpoints.load_tree_into_state(tree, other)


@pytest.mark.parametrize("K", [4, 25])
def test_checkpoint_round_trip_with_sg_keys_torch_dict(tmp_path, K):
    src = _sg_state(K)
    sd = checkpoints.torch_state_dict_from_state(src)
    assert tuple(sd["sg_lambda"].shape) == (K,) and tuple(sd["sg_mu_spher"].shape) == (K, 2)
    assert tuple(sd["MLP_1.rgb_layer.weight"].shape) == (3 * K, 256)                 # Linear weights are [out, in]
    torch.save({"model": sd}, str(tmp_path / "nerf.ckpt"))
    dst = _sg_state(K, seed=99)
    assert checkpoints.restore_torch_checkpoint(str(tmp_path), dst).endswith("nerf.ckpt")
    assert torch.equal(dst.params, src.params)
    assert torch.equal(dst.sg_lambda, src.sg_lambda) and torch.equal(dst.sg_mu_spher, src.sg_mu_spher)
    # a non-SG model still rejects the keys with the message it always had
    with pytest.raises(ValueError, match=r"torch checkpoint key 'sg_lambda': the view-conditioned head / SG basis is not built"):
        checkpoints.restore_torch_checkpoint(str(tmp_path), _plain_state(K))
    with pytest.raises(ValueError, match="SG basis is not built"):
        checkpoints.torch_state_dict_to_tree(sd)
    with pytest.raises(ValueError, match="SG basis is not built"):
        checkpoints.vd_torch_state_dict_to_tree(sd)
    del sd["sg_mu_spher"]
    torch.save({"model": sd}, str(tmp_path / "nerf.ckpt"))
    with pytest.raises(ValueError, match="sg_mu_spher"):
        checkpoints.restore_torch_checkpoint(str(tmp_path), _sg_state(K))


# ---- the svox mirror ------------------------------------------------------------------------------------------------
def _sg_tree(K=25, depth=2, seed=0):
    lobes = torch.from_numpy(G.lobes(K))
    t = svox.N3Tree(N=2, data_dim=3 * K + 1, depth_limit=4, data_format=f"SG{K}", extra_data=lobes, radius=[1.0, 2.0, 1.0],
                    center=[0.5, 0.0, 0.5])
    g = torch.Generator().manual_seed(seed)
    for _ in range(depth):
        t._refine_packed(t._leaf_packed()[::3])
    with torch.no_grad():
        t.data.copy_(torch.randn(t.data.shape, generator=g))
        t.data[..., -1] = torch.rand(t.data.shape[:-1], generator=g) * 20.0
    return t


def test_n3tree_sg_construction_save_load_clone(tmp_path):
    t = _sg_tree(25)
    assert str(t.data_format) == "SG25" and t.data_format.format == svox.DataFormat.SG and t.basis_dim == 25 and t.data_dim == 76
    assert t.data_format == "SG25" and t.data_format != "SH25"
    assert t.extra_data.dtype == torch.float32 and tuple(t.extra_data.shape) == (25, 4)
    assert not isinstance(t.extra_data, torch.nn.Parameter) and not t.extra_data.requires_grad
    assert len(t.parameters()) == 1 and t.parameters()[0] is t.data                      # a buffer: svox does not optimise it
    assert "SG25" in repr(t)
    assert t.basis_kwargs()["lobes"] is t.extra_data
    path = str(tmp_path / "sg.npz")
    t.save(path, compress=False)
    z = np.load(path)
    assert str(z["data_format"]) == "SG25" and z["extra_data"].shape == (25, 4) and z["extra_data"].dtype == np.float32
    back = svox.N3Tree.load(path)
    assert str(back.data_format) == "SG25" and torch.equal(back.extra_data, t.extra_data)
    assert torch.equal(back.child, t.child) and torch.equal(back.data.data, t.data.data.half().float())
    for c in (t.clone(), t.clone(device="cpu"), t.to("cpu")):
        assert torch.equal(c.extra_data, t.extra_data) and c.extra_data is not t.extra_data and str(c.data_format) == "SG25"
    # an SH tree has the attribute too, empty
    sh = svox.N3Tree(N=2, data_dim=49, data_format="SH16")
    assert sh.extra_data is None and sh.clone().extra_data is None and sh.basis_kwargs() == {}
    # the file is validated: shape against data_format
    bad = {k: z[k] for k in z.files}
    bad["extra_data"] = bad["extra_data"][:24]
    np.savez(str(tmp_path / "bad.npz"), **bad)
    with pytest.raises(ValueError, match=r"extra_data has shape \(24, 4\), data_format SG25 needs \(25, 4\)"):
        svox.N3Tree.load(str(tmp_path / "bad.npz"))
    del bad["extra_data"]
    np.savez(str(tmp_path / "bad.npz"), **bad)
    with pytest.raises(NotImplementedError, match="SG25 without extra_data"):
        svox.N3Tree.load(str(tmp_path / "bad.npz"))


def test_n3tree_sg_refusals_by_message():
    lobes = torch.from_numpy(G.lobes(4))
    with pytest.raises(NotImplementedError, match="SG7.*sg_dim 1, 4, 9, 16 and 25"):
        svox.N3Tree(N=2, data_dim=22, data_format="SG7", extra_data=torch.ones(7, 4))
    with pytest.raises(NotImplementedError, match="without extra_data"):
        svox.N3Tree(N=2, data_dim=13, data_format="SG4")
    with pytest.raises(ValueError, match=r"extra_data has shape \(4, 3\)"):
        svox.N3Tree(N=2, data_dim=13, data_format="SG4", extra_data=lobes[:, :3])
    with pytest.raises(ValueError, match="only the SG formats carry extra_data"):
        svox.N3Tree(N=2, data_dim=13, data_format="SH4", extra_data=lobes)
    with pytest.raises(ValueError, match="lambda"):
        svox.N3Tree(N=2, data_dim=13, data_format="SG4", extra_data=-lobes)
    with pytest.raises(ValueError, match="data_dim 14 does not match data_format SG4"):
        svox.N3Tree(N=2, data_dim=14, data_format="SG4", extra_data=lobes)
    with pytest.raises(NotImplementedError, match="ASG"):
        svox.N3Tree(N=2, data_dim=13, data_format="ASG4", extra_data=lobes)
    t = _sg_tree(4)
    r = svox.VolumeRenderer(t)
    o = torch.zeros(1, 3)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="render_persp_aux on an SG tree"):
            r.render_persp_aux(torch.eye(4), width=4, height=4, fx=4.0)
        with pytest.raises(NotImplementedError, match="forward_aux on an SG tree"):
            r.forward_aux(o, o, o)


def test_compression_keeps_extra_data_and_the_file_reloads_as_an_sg_tree(tmp_path):
    assert "extra_data" not in compression._DROPPED
    t = _sg_tree(4, depth=2)
    src = str(tmp_path / "sg.npz")
    t.save(src, compress=False)
    for flags, name in ((["--noquant"], "deflate"), (["--bits", "4", "--sigma_thresh", "2.0"], "palette"),
                        (["--bits", "4", "--retain", "1"], "retain")):
        out_dir = str(tmp_path / name)
        done = compression.main([src, "--out_dir", out_dir, "--overwrite", *flags])
        z = np.load(done[0])
        assert np.array_equal(z["extra_data"], t.extra_data.numpy()) and str(z["data_format"]) == "SG4", name
        back = svox.N3Tree.load(done[0])                            # the decompressing path
        assert isinstance(back, svox.N3Tree) and str(back.data_format) == "SG4" and torch.equal(back.extra_data, t.extra_data)
        assert tuple(back.data.shape) == tuple(t.data.shape)
        if name != "deflate":
            assert "quant_colors" in z.files
            with pytest.raises(NotImplementedError, match="keep_quantized=True on an SG tree"):
                svox.N3Tree.load(done[0], keep_quantized=True)
    # octree.evaluation: the flags that need the palette form or the extra outputs are refused for an SG file, by name
    base = ["--input", src, "--dataset", "synthetic"]
    for flag, extra in (("--keep_compressed", []), ("--write_aux", [str(tmp_path / "aux")]), ("--write_points", [str(tmp_path / "p.ply")])):
        with pytest.raises(NotImplementedError, match=rf"SG tree \(SG4\): {flag}"):
            evaluation.check_sg_flags(evaluation.define_flags().parse_args(base + [flag] + extra))
    evaluation.check_sg_flags(evaluation.define_flags().parse_args(base))
    sh = svox.N3Tree(N=2, data_dim=13, data_format="SH4")
    sh.save(str(tmp_path / "sh.npz"), compress=False)
    evaluation.check_sg_flags(evaluation.define_flags().parse_args(["--input", str(tmp_path / "sh.npz"), "--write_aux", "d"]))


# ---- flags ----------------------------------------------------------------------------------------------------------
def test_flag_checks_accept_the_preset_and_reject_the_rest_by_name():
    a = _sg_args()
    assert a.sg_dim == 25 and a.sh_deg == -1 and a.use_viewdirs is False
    families.check_flags(families.SG, a, "render")
    families.check_flags(families.SG, a, "extract")
    families.check(a, "render")
    assert sg.make_cfg(a).sh_deg == 4 and a.sh_deg == -1
    for K, deg in ((1, 0), (4, 1), (9, 2), (16, 3), (25, 4)):
        assert sg.head_degree(K) == deg
    for purpose, what in (("render", "rendering a NeRF-SG"), ("extract", "extraction of an SG PlenOctree")):
        for mutate, word in ((dict(sg_dim=7), r"sg_dim=7 \(need one of \(1, 4, 9, 16, 25\)"),
                             (dict(sh_deg=3), r"sh_deg=3 \(need -1"),
                             (dict(use_viewdirs=True), "use_viewdirs=true"),
                             (dict(sg_dim=-1), "sg_dim=-1"),
                             (dict(legacy_posenc_order=True), "legacy_posenc_order"),
                             (dict(render_path=True), "LLFF")):
            b = _sg_args()
            vars(b).update(mutate)
            with pytest.raises(NotImplementedError, match=what + ".*" + word):
                families.check_flags(families.SG, b, purpose)
    with pytest.raises(NotImplementedError, match="sg_dim=7"):
        sg.head_degree(7)
    with pytest.raises(ValueError, match="train_dir"):
        b = _sg_args(); b.train_dir = None
        families.check(b, "render")
    # training stays unbuilt: nerf_sh.train's flag check (utils.check_flags) refuses the SG preset by name ...
    with pytest.raises(NotImplementedError, match=r"sg_dim>0 \(spherical gaussians\)"):
        utils.check_flags(_sg_args(), require_batch_size_div=True)
    # ... and the reference never defines sg_global: no such flag here either
    with pytest.raises(SystemExit):
        utils.define_flags().parse_args(["--train_dir", "x", "--sg_global", "true"])
    assert not hasattr(extraction.define_flags().parse_args([]), "sg_global")


# ---- ABI ------------------------------------------------------------------------------------------------------------
def test_sg_symbols_in_header_ctypes_table_and_library():
    build.build(verbose=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = {"pxo_sg_render_fwd": "plenoctree_hip.h", "pxo_octree_render_sg_fwd": "plenoctree_octree.h",
             "pxo_octree_render_sg_bwd": "plenoctree_octree.h"}
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, header in names.items():
        src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", header)).read(), flags=re.S)
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES and re.search(rf"\bT {name}\b", nm), name
    hdr = open(os.path.join(root, "include", "plenoctree_hip.h")).read()
    assert int(re.search(r"#define PXO_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.pxo_version() == 9
    # argument checks that need no GPU: K outside the list, data_dim, null lobes -- PXO_ERR_ARG with a message
    import ctypes
    opts = _lib.PxoRenderOpts(1e-3, 1.0, 0.0, 0.0)
    dummy = ctypes.c_void_p(16)

    def call(basis_dim, data_dim, lobes):
        t = _lib.PxoTree()
        t.child, t.data, t.n_internal, t.data_dim, t.basis_dim = 16, 16, 1, data_dim, basis_dim
        return lib.pxo_octree_render_sg_fwd(ctypes.byref(t), lobes, None, None, None, None, 0, ctypes.byref(opts), None, None)

    assert call(4, 13, dummy) == 0                                   # B = 0: nothing is launched
    for args, word in (((7, 22, dummy), b"basis_dim 7 is not a supported SG format"), ((4, 14, dummy), b"data_dim 14 != 3*basis_dim+1"),
                       ((4, 13, None), b"null lobes")):
        assert call(*args) == -1 and word in lib.pxo_last_error(), lib.pxo_last_error()
    cfg = _lib.make_cfg(sh_deg=4)
    assert lib.pxo_sg_render_fwd(ctypes.byref(cfg), None, *([None] * 5), 0, 0, None, None, 0, *([None] * 7), 0, None) == -1
    assert b"null lobes" in lib.pxo_last_error()


# ---- the scenes of the GPU forward test -----------------------------------------------------------------------------
@pytest.mark.parametrize("K", G.KS)
def test_gpu_scenes_cannot_pass_vacuously(K):
    """On the CPU helper alone: at least half of the view's rays accumulate alpha > 0.1; the SG image differs from the same
    data read as SH by more than 1e-2 (a dispatch that silently takes the SH basis fails); the early-stop options change the
    image (some rays do stop) and some pixels see only the background; the helper's own float32 round-off is far below the
    renderer bound of tests/test_gpu_sg.py."""
    alpha = G.view_alphas(K)
    assert (alpha > 0.1).mean() >= 0.5, (alpha > 0.1).mean()
    assert (alpha > 0.99).sum() >= 1 and (alpha == 0.0).sum() >= 1
    im, sh, fast = G.want_image(K, False), G.sh_image(K), G.want_image(K, True)
    assert im.shape == (12, 16, 3) and im.dtype == f32
    assert np.abs(im - sh).max() > 1e-2, np.abs(im - sh).max()
    assert 1e-5 < np.abs(fast - im).max() < 0.03
    own = np.abs(im.astype(np.float64) - G.want_image(K, False, "f64")).max()
    print(f"K={K}: helper float32 vs its float64 compositing {own:.3g}")
    assert own < 2e-6
    o, d, v = G.ray_batch(K)
    rays = G.want_rays(K, False)
    assert (np.abs(rays - 1.0).max(axis=1) == 0).sum() == 3              # corner, away, miss: background only
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-6 and np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-6
