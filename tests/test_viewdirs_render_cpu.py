"""Ray rendering with the view-conditioned head, the parts that need no GPU: the float64 restatement against the fixture of the
reference's own NerfModel.__call__ (tests/golden/viewdirs_render.npz), the ABI surface and the flag checks of the CLIs."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from plenoctree_amd import _lib, build
from plenoctree_amd.nerf_sh.nerf import families, utils, viewdirs
from _viewdirs_render_helpers import check_level, fixture, fixture_rays, fixture_state_dict, host_render_f64, render_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pxo_vd_render_workspace_bytes", "pxo_vd_render_fwd", "pxo_vd_composite_fwd")


def test_fixture_covers_transparent_and_opaque_rays():
    fx = fixture()
    assert fx["origins"].shape == (12, 3) and fx["t_rand"].shape == (12, 64) and fx["u"].shape == (12, 128)
    norms = np.linalg.norm(fx["directions"], axis=-1)
    assert norms.min() < 1e-11 and norms.max() / norms.min() > 1e11 and np.allclose(np.linalg.norm(fx["viewdirs"], axis=-1), 1, atol=1e-6)
    for r in (0, 1):
        acc = fx[f"acc_fine_r{r}"]
        assert acc.min() < 0.05 and acc.max() > 0.95
    assert not any("weight" in k or "kernel" in k or "bias" in k for k in fx.files)       # the file holds no weights


def test_float64_restatement_reproduces_the_reference_run():
    """The measured maxima printed here are the reference-float32 floor of each quantity (recorded in DESIGN.md section 11):
    the fixture is the reference's float32 run, the restatement is float64."""
    fx = fixture()
    sd = fixture_state_dict(fx)
    rays = fixture_rays(fx)
    for r in (0, 1):
        out = host_render_f64(sd, rays, render_cfg(), torch.from_numpy(fx["t_rand"]) if r else None,
                              torch.from_numpy(fx["u"]) if r else None)
        for lvl, got in zip(("coarse", "fine"), out):
            check_level(f"f64 restatement vs reference f32, {lvl} r{r}", got,
                        (fx[f"rgb_{lvl}_r{r}"], fx[f"disp_{lvl}_r{r}"], fx[f"acc_{lvl}_r{r}"]))


def test_new_symbols_are_declared_bound_and_exported():
    build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "plenoctree_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (pxo_[a-z0-9_]+)", nm))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and name in exported, name
    assert "PXO_TUNE_VD_RAY_BLOCK" in header
    lib = _lib.load()
    assert lib.pxo_version() == _lib.ABI_VERSION
    from plenoctree_amd import ops
    assert all(hasattr(ops, n) for n in ("vd_render_workspace_bytes", "vd_render_fwd", "vd_composite_fwd", "TUNE_VD_RAY_BLOCK"))


def test_workspace_is_one_block_and_errors_are_reported():
    """Host-only entry points: the workspace stops growing at the ray block (apart from the draws' 4 bytes per sample), sh_deg is
    ignored, the split precisions are refused."""
    import ctypes
    build.build(verbose=False)
    lib = _lib.load()
    n = ctypes.c_size_t(0)

    def size(B, **kw):
        cfg = _lib.make_cfg(**kw)
        assert lib.pxo_vd_render_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(n)) == 0, lib.pxo_last_error()
        return n.value
    per_ray_draws = 4 * (64 + 128)
    a, b, c = size(1024), size(8192), size(512)
    assert 0 <= b - a - 7168 * per_ray_draws < 4096 and c < 0.6 * a
    rows = 1024 * 192
    assert 8 * rows * 1024 < a < 1.15 * 8 * rows * 1024            # dominated by the trunk's saved activations
    cfg = _lib.make_cfg()
    cfg.sh_deg = -1                                                # the reference's rendering presets
    assert lib.pxo_vd_render_workspace_bytes(ctypes.byref(cfg), 1024, ctypes.byref(n)) == 0 and n.value == a
    for prec in (_lib.MLP_BF16X3, _lib.MLP_BF16X6):
        cfg = _lib.make_cfg(mlp_precision=prec)
        assert lib.pxo_vd_render_workspace_bytes(ctypes.byref(cfg), 8, ctypes.byref(n)) == -4
    v = ctypes.c_int(0)
    assert lib.pxo_get_tuning(5, ctypes.byref(v)) == 0 and v.value == 1024
    assert lib.pxo_set_tuning(5, 0) == -1 and lib.pxo_set_tuning(5, 4097) == -1
    try:
        assert lib.pxo_set_tuning(5, 512) == 0 and size(1024) == c + 512 * per_ray_draws
    finally:
        assert lib.pxo_set_tuning(5, 1024) == 0


def _args(extra=()):
    return utils.define_flags().parse_args(["--train_dir", "x", "--dataset", "synthetic", *extra])


def test_render_flag_check_accepts_the_references_presets_and_names_the_rest():
    og_nerf = ["--num_coarse_samples", "64", "--num_fine_samples", "128", "--use_viewdirs", "true", "--white_bkgd", "true",
               "--sparsity_weight", "0.0"]                                   # config/misc/og_nerf.yaml: sh_deg stays -1
    proj = og_nerf[:-2] + ["--sh_deg", "4"]                                  # config/misc/proj.yaml
    assert _args(og_nerf).sh_deg == -1
    families.check_flags(families.VIEWDIRS, _args(og_nerf), "render")
    families.check_flags(families.VIEWDIRS, _args(proj), "render")
    families.check(_args(og_nerf), "render")
    for extra, word in ((["--net_width_condition", "256"], "net_width_condition=256"),
                        (["--deg_view", "3"], "deg_view=3"),
                        (["--sg_dim", "8"], "sg_dim>0"),
                        (["--mlp_precision", "bf16x6"], "mlp_precision=bf16x6"),
                        (["--net_depth_condition", "2"], "net_depth_condition=2"),
                        (["--use_viewdirs", "false"], "use_viewdirs=false")):
        with pytest.raises(NotImplementedError, match=word):
            families.check_flags(families.VIEWDIRS, _args(og_nerf + extra), "render")
    with pytest.raises(ValueError, match="train_dir"):
        a = _args(og_nerf); a.train_dir = None
        families.check(a, "render")
    # the projection keeps its own clauses, and the generic check (training, gen_mesh) keeps rejecting the head
    with pytest.raises(NotImplementedError, match="sh_deg=-1"):
        families.check_flags(families.VIEWDIRS, _args(og_nerf), "extract")
    with pytest.raises(NotImplementedError, match="use_viewdirs=true"):
        utils.check_flags(_args(og_nerf))
    with pytest.raises(NotImplementedError, match="use_viewdirs=true"):
        utils.check_flags(_args(proj))


def test_clis_parse_the_checkpoint_flags_of_extraction():
    from plenoctree_amd.nerf_sh import gen_video
    a = gen_video.define_flags().parse_args(["--train_dir", "x", "--is_jaxnerf_ckpt", "--trust_ckpt_pickle", "true"])
    assert a.is_jaxnerf_ckpt is True and a.trust_ckpt_pickle is True
    a = viewdirs.add_checkpoint_flags(utils.define_flags()).parse_args(["--train_dir", "x"])
    assert a.is_jaxnerf_ckpt is False and a.trust_ckpt_pickle is False
