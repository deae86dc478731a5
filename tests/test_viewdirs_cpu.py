"""Host side of the view-conditioned NeRF path (no GPU): parameter layout, both checkpoint formats, flag checks, direction draw,
and the fixture's own consistency with the float64 restatement the GPU tests use."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from plenoctree_amd import _lib, build, ops
from plenoctree_amd.nerf_sh.nerf import checkpoints, families, utils, viewdirs
from plenoctree_amd.octree import extraction

from _viewdirs_helpers import (EDGE_CROSS_N, EDGE_CROSS_R, EDGE_DIR_N, EDGE_DIR_R, EDGE_PER_POINT_N, EDGE_POINT_N, EDGE_POINT_R,
                               EdgeReference, edge_check, fixture, host_model_f64, host_project_f64, seeded_state_dict)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def test_layout_is_twelve_layers_per_mlp_with_the_twins_shapes(lib):
    fx = fixture()
    leaves, n = ops.vd_param_layout()
    assert len(leaves) == 24 == _lib.VD_NUM_LEAVES and n == 595844
    assert n == 493056 + 257 + 65792 + 36352 + 387
    # the twin's state dict lists MLP_0 then MLP_1, each layer weight [out,in] then bias [out], in the arena's layer order
    shapes = [tuple(int(v) for v in s[:int(nd)]) for s, nd in zip(fx["shapes"], fx["ndim"])]
    assert len(shapes) == 48
    off = 0
    for i, (layer, is_bias, o, rows, cols) in enumerate(leaves):
        assert (layer, is_bias, o) == (i // 2, i % 2, off)
        assert shapes[i] == ((rows,) if is_bias else (cols, rows)) == shapes[24 + i], str(fx["keys"][i])
        off += rows * cols
    assert off == n
    k = ctypes.c_int64(0)
    assert lib.pxo_vd_packed_floats(ctypes.byref(k)) == 0
    a = ctypes.c_int64(0)
    assert lib.pxo_packed_sizes(ctypes.byref(_lib.make_cfg(sh_deg=0)), ctypes.byref(a), None) == 0
    assert k.value == a.value + (n - 493056)          # an SH-degree-0 forward image, then Dense_8..11
    # the SH layout is what it was
    assert lib.pxo_param_layout(ctypes.byref(_lib.make_cfg(sh_deg=3)), None, ctypes.byref(k)) == 0 and k.value == 505649


def test_workspace_does_not_grow_with_points_times_directions(lib):
    w = ops.vd_project_workspace_bytes
    assert w(0, 1000) < w(0, 10000) < w(0, 1000) + 9001 * (128 + 25 + 8) * 4 + 4096
    per_point = (w(1 << 16, 10000) - w(0, 10000)) / (1 << 16)
    assert per_point == pytest.approx((w(1 << 16, 10) - w(0, 10)) / (1 << 16), rel=1e-3)     # independent of R
    assert 8 * 1024 < per_point < 10 * 1024                                                  # saved trunk activations dominate
    nbytes = ctypes.c_size_t(0)
    assert lib.pxo_vd_project_workspace_bytes(16, 0, ctypes.byref(nbytes)) == -1


def test_both_checkpoint_formats_land_in_the_same_arena(tmp_path):
    fx = fixture()
    sd = seeded_state_dict(fx)
    flat = checkpoints.vd_tree_to_arena(checkpoints.vd_torch_state_dict_to_tree(sd))
    leaves, n = ops.vd_param_layout()
    assert flat.shape == (2 * n,)
    # kernels are the transposed Linear weights: spot values at both ends of every leaf
    for mi in range(2):
        for li, name in enumerate(checkpoints._VD_TORCH_NAMES):
            w = sd[f"MLP_{mi}.{name}.weight"].numpy()
            _, _, off, rows, cols = leaves[2 * li]
            assert np.array_equal(flat[mi * n + off: mi * n + off + rows * cols].reshape(rows, cols), w.T)
            assert np.array_equal(flat[mi * n + leaves[2 * li + 1][2]:][:cols], sd[f"MLP_{mi}.{name}.bias"].numpy())
    # torch *.ckpt
    d1 = tmp_path / "torch"; d1.mkdir()
    torch.save({"model": sd}, str(d1 / "model.ckpt"))
    got, path, fmt = checkpoints.load_viewdirs_arena(str(d1))
    assert fmt == "torch state dict" and np.array_equal(got, flat)
    assert checkpoints.vd_state_dict_from_arena(flat).keys() == sd.keys()
    # flax msgpack checkpoint_<step>, Dense_0..11 with kernels [in,out]
    d2 = tmp_path / "flax"; d2.mkdir()
    tree = checkpoints.vd_arena_to_tree(flat)
    assert sorted(tree["MLP_1"], key=lambda k: int(k.split("_")[1])) == [f"Dense_{i}" for i in range(12)]
    assert tree["MLP_0"]["Dense_10"]["kernel"].shape == (283, 128) and tree["MLP_0"]["Dense_11"]["kernel"].shape == (128, 3)
    with open(d2 / "checkpoint_5", "wb") as f:
        f.write(checkpoints.msgpack_serialize({"optimizer": {"target": {"params": tree}}}))
    got2, _, fmt2 = checkpoints.load_viewdirs_arena(str(d2), is_jaxnerf_ckpt=True)
    assert fmt2 == "flax msgpack" and np.array_equal(got2, flat)
    got3, _, fmt3 = checkpoints.load_viewdirs_arena(str(d2))            # no *.ckpt: falls through to the flax file
    assert fmt3 == "flax msgpack" and np.array_equal(got3, flat)


def test_wrong_shapes_name_the_first_mismatching_leaf(tmp_path):
    fx = fixture()
    sd = seeded_state_dict(fx)
    bad = dict(sd)
    bad["MLP_0.condition_layers.0.weight"] = torch.zeros(64, 283)
    torch.save({"model": bad}, str(tmp_path / "a.ckpt"))
    with pytest.raises(ValueError, match=r"MLP_0/Dense_10/kernel has shape \(283, 64\).*\(283, 128\)"):
        checkpoints.load_viewdirs_arena(str(tmp_path))
    # an SH model's file (no view-conditioned head) fits neither: named, with the hint
    sh = {k: v for k, v in sd.items() if "bottleneck" not in k and "condition" not in k}
    torch.save({"model": sh}, str(tmp_path / "b.ckpt"))
    with pytest.raises(ValueError, match=r"MLP_0\.bottleneck_layer\.weight.*missing"):
        checkpoints.load_viewdirs_arena(str(tmp_path))
    tree = checkpoints.vd_arena_to_tree(checkpoints.vd_tree_to_arena(checkpoints.vd_torch_state_dict_to_tree(sd)))
    del tree["MLP_1"]["Dense_11"]
    with pytest.raises(ValueError, match=r"MLP_1/Dense_11/kernel is missing"):
        checkpoints.vd_tree_to_arena(tree)
    # and the SH loader still refuses a view-conditioned file
    with pytest.raises(ValueError, match="bottleneck_layer"):
        checkpoints.torch_state_dict_to_tree(sd)


def _args(extra=()):
    a = extraction.define_flags().parse_args(["--train_dir", "x", "--dataset", "synthetic", "--use_viewdirs", "true", "--sh_deg", "2",
                                              *extra])
    return a


def test_extraction_flag_check_accepts_the_built_combination_and_names_the_rest():
    families.check(_args(), "extract")
    for extra, word in ((["--net_depth_condition", "2"], "net_depth_condition=2"),
                        (["--net_width_condition", "256"], "net_width_condition=256"),
                        (["--deg_view", "3"], "deg_view=3"),
                        (["--sh_deg", "-1"], "sh_deg=-1"),
                        (["--sh_deg", "5"], "sh_deg=5"),
                        (["--sg_dim", "8"], "sg_dim>0"),
                        (["--legacy_posenc_order", "true"], "legacy_posenc_order"),
                        (["--mlp_precision", "bf16x3"], "mlp_precision=bf16x3")):
        with pytest.raises(NotImplementedError, match=word):
            families.check(_args(extra), "extract")
    # the generic check (training, NeRF rendering) keeps rejecting the head, with the reference's default flag values
    ref_defaults = utils.define_flags().parse_args(["--train_dir", "x", "--dataset", "synthetic"])
    assert ref_defaults.use_viewdirs is True
    with pytest.raises(NotImplementedError, match="use_viewdirs=true"):
        utils.check_flags(ref_defaults)
    with pytest.raises(NotImplementedError, match="use_viewdirs=true"):
        utils.check_flags(_args())


def test_direction_draw_is_the_references_formula_on_unit_vectors():
    g = torch.Generator().manual_seed(3)
    u, v = torch.rand(1000, generator=g), torch.rand(1000, generator=g)
    d = viewdirs.sphere_directions(u, v)
    assert d.dtype == torch.float32 and d.shape == (1000, 3)
    assert float((d.double().norm(dim=-1) - 1).abs().max()) < 2e-7
    theta = np.arccos(2.0 * u.double().numpy() - 1.0)
    phi = 2.0 * math.pi * v.double().numpy()
    want = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)
    assert np.abs(d.numpy() - want).max() < 1e-7
    # the fixture's directions are the reference's spher2cart of its own theta / phi
    fx = fixture()
    got = viewdirs.sphere_directions((torch.cos(torch.from_numpy(fx["theta"]).double()) + 1) / 2, torch.from_numpy(fx["phi"]).double() / (2 * math.pi))
    assert np.abs(got.numpy() - fx["dirs"]).max() < 1e-6


def test_fixture_agrees_with_the_float64_restatement():
    """The host model the GPU tests compare with IS the reference's twin in float64 (1e-12: both float64, different order)."""
    fx = fixture()
    sd = seeded_state_dict(fx)
    pts, dirs = torch.from_numpy(fx["points"]), torch.from_numpy(fx["dirs"])
    rgb, sigma = host_model_f64(sd, pts, dirs, cross=True)
    assert np.abs(rgb.numpy() - fx["rgb_cross"]).max() < 1e-12 and np.abs(sigma.numpy() - fx["sigma"]).max() < 1e-12
    rgbp, _ = host_model_f64(sd, pts, dirs[:40])
    assert np.abs(rgbp.numpy() - fx["rgb_point"]).max() < 1e-12
    for d in range(5):
        assert np.abs(host_project_f64(rgb, dirs, d).numpy() - fx[f"coeffs_{d}"]).max() < 1e-12
        assert 0 < float(fx[f"floor_coeffs_{d}"]) < 1e-5
    assert 0 < float(fx["floor_rgb_cross"]) < 1e-5 and 0 < float(fx["floor_sigma"]) < 1e-5
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "viewdirs_projection.npz")) < 1 << 20


def test_reference_arithmetic_stays_inside_the_edge_bounds():
    """The bound of tests/test_gpu_viewdirs_edges.py, 4 x floor x max(1, range of the case / range of the fixture), leaves room
    for the reference arithmetic itself: the float32 host restatement of every (N, R, degree) case of that file stays within it
    of the float64 one.  What is left of the factor 4 is the kernels' allowance for their different summation order."""
    ref = EdgeReference()
    f32 = torch.float32
    pts = ref.inp["points"]
    worst = {}

    def projection(N, R):
        dirs = ref.dirs(R)
        rgb, sigma = host_model_f64(ref.sd, pts[:N], dirs, cross=True, dtype=f32)
        assert rgb.dtype == f32 and sigma.dtype == f32
        for deg in range(5) if R != "special" else (4,):
            want = ref.coeffs(N, R, deg)
            got = host_project_f64(rgb, dirs, deg, dtype=f32)
            assert got.dtype == f32
            edge_check(f"coeffs_{deg} N={N} R={R}", got, want, ref.bound(f"coeffs_{deg}", want), worst)
        edge_check(f"sigma N={N} R={R}", sigma, ref.sigma[:N], ref.bound("sigma", ref.sigma[:N]), worst)

    for N in EDGE_POINT_N:
        projection(N, EDGE_POINT_R)
    for R in EDGE_DIR_R + ("special",):
        projection(EDGE_DIR_N, R)
    for N in EDGE_CROSS_N:
        for R in EDGE_CROSS_R:
            rgb, _ = host_model_f64(ref.sd, pts[:N], ref.dirs(R), cross=True, dtype=f32)
            want = ref.cross(N, R)
            edge_check(f"rgb_cross N={N} R={R}", rgb, want, ref.bound("rgb_cross", want), worst)
    for N in EDGE_PER_POINT_N:
        rgb, _ = host_model_f64(ref.sd, pts[:N], ref.dirs(N), dtype=f32)
        want = ref.rgb_per_point[:N]
        edge_check(f"rgb_point N={N}", rgb, want, ref.bound("rgb_point", want), worst)
    print("worst float32-restatement multiple of the scaled floor:", {k: round(v, 2) for k, v in sorted(worst.items())})
