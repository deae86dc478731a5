"""Host side of NDC on the octree side (no GPU): the test oracle's conversion is the reference's convert_to_ndc bit for bit, the
composition "convert, then march" gives a closed-form answer that does not come from the composition, misses give the
background, and the Python surface accepts, checks and refuses what the documents say it does."""
import argparse
import os
import types

import numpy as np
import pytest
import torch

import _octree_ndc_oracle as N
import _quant_cases as Q
from oracle import octree_oracle as T
from plenoctree_amd import _lib, build
from plenoctree_amd.octree import evaluation, extraction, optimization, svox

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = os.path.join(GOLDEN, "llff_tiny")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "octree_ndc.npz"))


def test_restatement_is_the_reference_convert_to_ndc(golden):
    """Bit for bit the reference's float32 output; within 4 x the reference's own float32-against-float64 error of its float64
    output (the fixture holds both, tests/golden/README_octree_ndc.md)."""
    z = golden
    ndc = N.Ndc(int(z["width"]), int(z["height"]), float(z["focal"]))
    assert (ndc.width, ndc.height, ndc.focal) == (N.W, N.H, N.FX) and z["origins"].shape[0] == 2 * N.W * N.H + 6
    got = [T.convert_to_ndc_f32(o, d, ndc) for o, d in zip(z["origins"], z["directions"])]
    go, gd = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    assert go.dtype == np.float32 and np.array_equal(go, z["o32"]) and np.array_equal(gd, z["d32"])
    e_o, e_d = float(z["e_ref_o"]), float(z["e_ref_d"])
    assert 0 < e_o < 1e-5 and 0 < e_d < 1e-5
    assert np.abs(go - z["o64"]).max() <= 4 * e_o and np.abs(gd - z["d64"]).max() <= 4 * e_d
    # the fixture's camera rays are the ones the tests render
    o, d = T.camera_rays(N.camera_b(), N.W, N.H, N.FX)
    assert np.array_equal(z["origins"][N.W * N.H: 2 * N.W * N.H], o) and np.array_equal(z["directions"][N.W * N.H: 2 * N.W * N.H], d)
    # item 3: the direction that marches is a unit vector and every ray of a forward-facing camera is a hit
    for oo, dd in zip(o[::7], d[::7]):
        no, nd, ok = T.ndc_ray(oo, dd, ndc)
        assert ok and abs(float(np.linalg.norm(nd.astype(np.float64))) - 1.0) < 1e-6 and nd[2] > 0


def test_shared_views_have_hits_and_misses():
    """The eight views of the GPU tests: at least 20 hits each, at least one miss each except camera A on the radius-1 box,
    which fills the frustum by construction; at most 21 samples per ray; every image far from the background."""
    ndc = N.Ndc()
    for box in (0, 1):
        t = N.box_tree(16, box)
        for cam in "AB":
            o, d = T.camera_rays(N.CAMERAS[cam](), N.W, N.H, N.FX)
            for fast in (False, True):
                opt = T.RenderOptions.for_renderer(1e-3, fast)
                seqs = [T.march(t, oo, dd, opt.step_size, ndc=ndc) for oo, dd in zip(o, d)]
                hits = sum(s is not None for s in seqs)
                assert hits >= 20 and max(len(s) for s in seqs if s is not None) <= 21
                assert (hits == N.W * N.H) if (box, cam) == (0, "A") else (hits < N.W * N.H), (box, cam, hits)
                img = T.render_rays(t, o, d, d, opt, ndc=ndc)
                assert float(np.abs(img - 1.0).max()) > 0.5


def test_known_answer_chord_and_world_space_shading():
    worst, bound = N.known_answer_check(lambda t, o, d, opt: T.render_rays(t, o, d, d, opt, ndc=N.Ndc()))
    print(f"known answer: max error {worst:.3g}, bound {bound:.3g}")
    assert bound < 5e-3


def test_rays_that_cannot_be_converted_give_the_background():
    ndc = N.Ndc()
    t = N.box_tree(4, 0)
    opt = T.RenderOptions(1e-3, background_brightness=0.25)
    for dz in (0.0, 0.5, -1e-38):
        d = np.array([0.1, -0.2, dz], f32)
        for o in ([0.0, 0.0, 0.0], [0.2, 0.1, -0.5]):
            assert T.march(t, np.array(o, f32), d, opt.step_size, ndc=ndc) is None
            assert np.array_equal(T.render_ray(t, np.array(o, f32), d, d, opt, ndc=ndc), np.full(3, 0.25, f32))
    # ... while the same origins looking down -z are hits that see the tree
    assert T.march(t, np.zeros(3, f32), np.array([0.0, 0.0, -1.0], f32), opt.step_size, ndc=ndc) is not None


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def _sh_tree(K=4):
    return svox.N3Tree(N=2, data_dim=3 * K + 1, data_format=f"SH{K}", depth_limit=4, radius=1.0, center=[0.0, 0.0, 0.0])


def test_volume_renderer_takes_an_ndc_config_and_only_that():
    cfg = svox.NDCConfig(width=12, height=8, focal=10.5)
    assert (cfg.width, cfg.height, cfg.focal, cfg.near) == (12, 8, 10.5, 1.0)
    r = svox.VolumeRenderer(_sh_tree(), step_size=1e-3, ndc=cfg)
    assert r.ndc is cfg and r._basis_kwargs() == {"ndc": cfg}
    assert svox.VolumeRenderer(_sh_tree())._basis_kwargs() == {}
    for bad in (object(), (12, 8, 10.5), {"width": 12}):
        with pytest.raises(NotImplementedError, match="NDC"):
            svox.VolumeRenderer(_sh_tree(), ndc=bad)
    with pytest.raises(ValueError, match="NDCConfig"):
        svox.NDCConfig(0, 8, 10.5)
    with pytest.raises(ValueError, match="NDCConfig"):
        svox.NDCConfig(12, 8, 0.0)


def test_render_persp_checks_the_camera_against_the_config():
    r = svox.VolumeRenderer(_sh_tree(), ndc=svox.NDCConfig(12, 8, 10.5))
    c2w = np.eye(4, dtype=f32)
    for kw in (dict(width=13, height=8, fx=10.5), dict(width=12, height=9, fx=10.5), dict(width=12, height=8, fx=10.0),
               dict(width=12, height=8, fx=10.5, fy=11.0)):
        with pytest.raises(ValueError, match="NDCConfig"):
            r.render_persp(c2w, **kw)
    r._check_ndc_camera(12, 8, 10.5, None)            # the matching camera passes the check (rendering needs a GPU)
    r._check_ndc_camera(12, 8, 10.5, 10.5)


def test_refusals_carry_their_names(tmp_path):
    cfg = svox.NDCConfig(12, 8, 10.5)
    r = svox.VolumeRenderer(_sh_tree(), ndc=cfg)
    z = torch.zeros(2, 3)
    with pytest.raises(NotImplementedError, match="render_persp_aux with NDC"):
        r.render_persp_aux(np.eye(4, dtype=f32), width=12, height=8, fx=10.5)
    with pytest.raises(NotImplementedError, match="forward_aux with NDC"):
        r.forward_aux(z, z, z)
    q = svox.N3Tree.load(Q.make_case(4, 0, 8, depth=2).save(str(tmp_path / "q.npz")), keep_quantized=True)
    with pytest.raises(NotImplementedError, match="QuantizedN3Tree.*NDC"):
        svox.VolumeRenderer(q, ndc=cfg)
    lobes = np.array([[2.0, 1.0, 0.0, 0.0], [2.0, 0.0, 1.0, 0.0], [2.0, 0.0, 0.0, 1.0], [2.0, 0.0, 0.6, 0.8]], f32)
    sg = svox.N3Tree(N=2, data_dim=13, data_format="SG4", extra_data=lobes, depth_limit=4)
    with pytest.raises(NotImplementedError, match="SG tree.*NDC"):
        svox.VolumeRenderer(sg, ndc=cfg)
    svox.VolumeRenderer(sg)                          # ... and without ndc an SG tree is taken as before
    # a compressed tree that N3Tree.load has expanded to floats is a float tree like any other
    f = svox.N3Tree.load(str(tmp_path / "q.npz"))
    assert svox.VolumeRenderer(f, ndc=cfg).ndc is cfg
    # the octree_ops layer names it too, whoever calls it
    from plenoctree_amd import octree_ops as oops
    with pytest.raises(NotImplementedError, match="NDC rendering of an SG tree"):
        oops._no_sg_ndc(torch.zeros(4, 4), cfg)


def _flags(mod, extra):
    from plenoctree_amd.nerf_sh.nerf import utils
    args = mod.define_flags().parse_args(["--train_dir", "/nonexistent", "--data_dir", TINY] + extra)
    utils.update_flags(args)
    return args


@pytest.mark.parametrize("mod", [extraction, optimization, evaluation], ids=["extraction", "optimization", "evaluation"])
def test_entry_points_decide_ndc_by_dataset_and_spherify(mod):
    """NDC is on for `--dataset llff` without --spherify, in all three entry points (the reference's optimization leaves the
    spherify test out)."""
    ds = types.SimpleNamespace(w=12, h=8, focal=10.5)
    a = _flags(mod, ["--config", "llff"])
    assert a.dataset == "llff" and extraction.uses_ndc(a)
    cfg = extraction.ndc_config(a, ds)
    assert isinstance(cfg, svox.NDCConfig) and (cfg.width, cfg.height, cfg.focal, cfg.near) == (12, 8, 10.5, 1.0)
    a = _flags(mod, ["--config", "llff", "--spherify", "true"])
    assert not extraction.uses_ndc(a) and extraction.ndc_config(a, ds) is None
    a = _flags(mod, ["--config", "blender"])
    assert not extraction.uses_ndc(a) and extraction.ndc_config(a, ds) is None
    assert not extraction.uses_ndc(argparse.Namespace())                       # callers with a bare namespace: world space
    extraction.check_octree_flags(a, "x", (("--write_aux", True),))            # not an NDC scene: nothing to refuse
    # every entry point refuses --render_path by name before it looks for a GPU
    with pytest.raises(NotImplementedError, match="--render_path"):
        mod.main(["--config", "llff", "--data_dir", TINY, "--train_dir", "/nonexistent", "--render_path", "true"])


def test_evaluation_refuses_aux_and_palette_flags_on_an_ndc_scene(tmp_path):
    common = ["--config", "llff", "--data_dir", TINY, "--input", str(tmp_path / "none.npz")]
    for flag, extra in (("--write_aux", ["--write_aux", str(tmp_path / "aux")]),
                        ("--write_points", ["--write_points", str(tmp_path / "p.ply")]),
                        ("--keep_compressed", ["--keep_compressed"])):
        with pytest.raises(NotImplementedError, match=f"{flag}.*NDC scene"):
            evaluation.main(common + extra)
    assert not os.path.exists(str(tmp_path / "aux"))


def test_llff_dataset_reaches_the_octree_entry_points_only_through_their_own_loader(monkeypatch):
    """The three entry points call llff.get_dataset, which builds the LLFF class; the plain table keeps refusing the name."""
    from _llff_cpu_feeder import feeder_for
    from plenoctree_amd.nerf_sh.nerf import datasets, llff
    monkeypatch.setattr(llff.LLFF, "feeder_factory", staticmethod(feeder_for))
    a = _flags(extraction, ["--config", "llff", "--factor", "2"])
    a.factor = 2
    for mod in (extraction, optimization, evaluation):
        assert mod.llff is llff and not hasattr(mod, "datasets")
    ds = llff.get_dataset("test", a, torch.device("cpu"))
    assert isinstance(ds, llff.LLFF) and (ds.w, ds.h) == (12, 8)
    cfg = extraction.ndc_config(a, ds)
    assert (cfg.width, cfg.height, cfg.focal) == (12, 8, float(ds.focal))
    with pytest.raises(NotImplementedError):
        datasets.get_dataset("test", a, torch.device("cpu"))


def test_a_library_without_the_ndc_symbols_is_refused_by_name(monkeypatch):
    build.build(verbose=False)
    real = _lib.load()
    new = ("pxo_octree_render_ndc_fwd", "pxo_octree_render_ndc_bwd", "pxo_grid_weight_render_ndc")
    assert all(n in _lib.SIGNATURES and hasattr(real, n) for n in new)
    assert _lib.ABI_VERSION == real.pxo_version()                    # the ABI grew by additions only

    class Old:
        def __getattr__(self, name):
            if name in new:
                raise AttributeError(name)
            return getattr(real, name)

    import ctypes
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: Old())
    with pytest.raises(_lib.PxoError, match="does not export pxo_octree_render_ndc_fwd.*rebuild"):
        _lib.load()
    assert _lib._lib is None


def test_c_abi_rejects_bad_ndc_arguments():
    """PXO_ERR_ARG on a null ndc, width / height < 1, focal / near <= 0 and a basis_dim outside the SH formats, before any
    launch (host-side checks: no GPU needed)."""
    import ctypes
    build.build(verbose=False)
    lib = _lib.load()
    tree = _lib.PxoTree(1, 1, 1, 13, 4, (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.5, 0.5, 0.5))
    opts = _lib.PxoRenderOpts(1e-3, 1.0, 0.0, 0.0)
    fwd = lambda t, n: lib.pxo_octree_render_ndc_fwd(ctypes.byref(t), None, None, None, None, 0, ctypes.byref(opts), None, None, n)
    bwd = lambda t, n: lib.pxo_octree_render_ndc_bwd(ctypes.byref(t), None, None, None, None, 0, ctypes.byref(opts), None, None,
                                                     None, None, n)
    gw = lambda n: lib.pxo_grid_weight_render_ndc(None, 16, None, 0, 10.0, 10.0, 12, 8, ctypes.byref(opts), None, None, None, None,
                                                  0, None, n)
    good = _lib.PxoNdc(12, 8, 10.5, 1.0)
    assert fwd(tree, ctypes.byref(good)) == 0 and bwd(tree, ctypes.byref(good)) == 0 and gw(ctypes.byref(good)) == 0   # B = 0
    for bad in (None, _lib.PxoNdc(0, 8, 10.5, 1.0), _lib.PxoNdc(12, 0, 10.5, 1.0), _lib.PxoNdc(12, 8, 0.0, 1.0),
                _lib.PxoNdc(12, 8, 10.5, 0.0), _lib.PxoNdc(12, 8, -1.0, 1.0)):
        arg = None if bad is None else ctypes.byref(bad)
        assert fwd(tree, arg) != 0 and b"ndc" in lib.pxo_last_error()
        assert bwd(tree, arg) != 0 and gw(arg) != 0
    odd = _lib.PxoTree(1, 1, 1, 7, 2, (ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.5, 0.5, 0.5))
    assert fwd(odd, ctypes.byref(good)) != 0 and b"basis_dim" in lib.pxo_last_error()
    assert bwd(odd, ctypes.byref(good)) != 0
