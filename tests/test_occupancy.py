"""The occupancy grid of the NeRF ray renderer on the CPU: the numpy restatements the GPU tests compare against (pack with
dilation, point -> cell -> live, expand) on hand-made cases, the sigma threshold, and every refusal -- each raised before a GPU is
touched."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

import _occupancy_ref as R
from plenoctree_amd import _lib, ops
from plenoctree_amd.nerf_sh.nerf import families, occupancy, utils


# ---- the restatements on cases worked out by hand ---------------------------------------------------------------------------
def test_bits_layout_and_partial_last_word():
    mask = np.zeros(125, bool)
    mask[[0, 31, 32, 124]] = True
    bits = R.bits_from_mask(mask).view(np.uint32)
    assert bits.size == R.words(5) == 4
    assert bits.tolist() == [1 | 1 << 31, 1, 0, 1 << (124 - 96)]
    assert bits[3] >> 29 == 0                                     # 125 bits: positions 29..31 of the last word stay zero
    assert np.array_equal(R.mask_from_bits(bits.view(np.int32), 5), mask)


def test_pack_dilation_clamps_at_the_faces():
    s = np.zeros((4, 4, 4), np.float32)
    s[0, 0, 0] = 2.0                                              # a corner: its neighbourhood is cut to 2 x 2 x 2
    s[3, 1, 2] = 2.0                                              # a face cell: 2 x 3 x 3
    m0 = R.pack_mask(s, 4, 1.0, 0)
    assert m0.sum() == 2 and m0[0, 0, 0] and m0[3, 1, 2]
    m1 = R.pack_mask(s, 4, 1.0, 1)
    want = np.zeros((4, 4, 4), bool)
    want[0:2, 0:2, 0:2] = True
    want[2:4, 0:3, 1:4] = True
    assert np.array_equal(m1, want)
    # strictly above the threshold; NaN is occupied
    s2 = np.array([1.0, np.nan, 0.5, 1.0000001, 0, 0, 0, 0], np.float32)
    assert R.pack_mask(s2, 2, 1.0, 0).reshape(-1).tolist() == [False, True, False, True, False, False, False, False]
    assert R.pack(s2, 2, 1.0, 0).view(np.uint32).tolist() == [0b1010]


def test_point_rule():
    reso, offset, scale = 4, [0.5] * 3, [0.25] * 3               # the box [-2, 2)^3; cell side 1
    mask = np.zeros((4, 4, 4), bool)
    mask[2, 1, 3] = True                                          # x in [0,1), y in [-1,0), z in [1,2)
    bits = R.bits_from_mask(mask)
    pts = np.array([[0.5, -0.5, 1.5],       # inside the set cell
                    [0.0, -1.0, 1.0],       # exactly on its lower boundaries: belongs to it
                    [1.0, -0.5, 1.5],       # exactly on its upper x boundary: the next cell
                    [0.5, -0.5, 2.0],       # t_z = 1: outside
                    [-2.0, -2.0, -2.0],     # t = 0: inside, cell (0,0,0), empty
                    [0.5, -0.5, -2.5],      # outside
                    [np.nan, 0.0, 0.0],
                    [0.5, np.inf, 1.5]], np.float32)
    assert R.live_mask(bits, reso, offset, scale, 0, pts).tolist() == [True, True, False, False, False, False, True, True]
    assert R.live_mask(bits, reso, offset, scale, 1, pts).tolist() == [True, True, False, True, False, True, True, True]
    live, slot, n = R.cull(bits, reso, offset, scale, 0, pts)
    assert n == 4 and slot.tolist() == [0, 1, -1, -1, -1, -1, 2, 3]
    assert np.array_equal(live[:2], pts[:2]) and np.isnan(live[2, 0]) and np.isinf(live[3, 1])


def test_expand_restatement():
    slot = np.array([-1, 0, -1, 1, 2], np.int32)
    rgb_live = np.arange(9, dtype=np.float32).reshape(3, 3) + 1
    rgb, sigma = R.expand(rgb_live, np.array([5, 6, 7], np.float32), slot, 3)
    assert rgb.tolist() == [[0, 0, 0], [1, 2, 3], [0, 0, 0], [4, 5, 6], [7, 8, 9]] and sigma.tolist() == [0, 5, 0, 6, 7]


# ---- the threshold ------------------------------------------------------------------------------------------------------------
def test_sigma_thresh_formula():
    assert occupancy.sigma_thresh(0.0, 1.5, 128) == 0.0
    assert occupancy.sigma_thresh(0.01, 1.5, 256) == pytest.approx(-math.log(0.99) / (3.0 / 256), rel=1e-15)
    assert occupancy.sigma_thresh(0.01, [2.0, 1.0, 3.0], 64) == pytest.approx(-math.log(0.99) / (2.0 / 64), rel=1e-15)   # min(radius)
    # a cell of that side at that sigma has exactly that alpha
    a, r, n = 0.2, 1.25, 32
    assert 1.0 - math.exp(-occupancy.sigma_thresh(a, r, n) * 2 * r / n) == pytest.approx(a, rel=1e-12)
    for bad in (-0.1, 1.0):
        with pytest.raises(ValueError, match="alpha_thresh"):
            occupancy.sigma_thresh(bad, 1.5, 8)
    with pytest.raises(ValueError, match="radius"):
        occupancy.sigma_thresh(0.01, [1.0, 0.0, 1.0], 8)


# ---- refusals: command line ---------------------------------------------------------------------------------------------------
def _args(*argv):
    a = utils.define_flags().parse_args(["--train_dir", "x", "--dataset", "synthetic", "--use_viewdirs", "false", "--sh_deg", "2",
                                         *argv])
    return a


def test_flags_parse_and_defaults():
    a = _args()
    assert (a.occupancy_reso, a.occupancy_center, a.occupancy_radius, a.occupancy_alpha_thresh, a.occupancy_dilate,
            a.occupancy_outside, a.occupancy_tree) == (0, [0.0, 0.0, 0.0], [1.5, 1.5, 1.5], 0.01, 1, "empty", "")
    a = _args("--occupancy_reso", "64", "--occupancy_center", "0.5 0 -1", "--occupancy_radius", "2", "--occupancy_outside", "live",
              "--occupancy_dilate", "0")
    assert a.occupancy_center == [0.5, 0.0, -1.0] and a.occupancy_radius == [2.0, 2.0, 2.0]
    assert not occupancy.wanted(_args()) and occupancy.wanted(a) and occupancy.clauses(a) == []
    families.check(a, "render")                                  # built: no refusal
    families.check(_args(), "train")


@pytest.mark.parametrize("argv, words", [
    (["--use_viewdirs", "true"], "occupancy_reso with use_viewdirs=true"),
    (["--dataset", "llff", "--data_dir", "d"], "forward-facing scene without --spherify (NDC"),
    (["--noise_std", "1.0", "--randomized", "true"], "noise_std and randomized rendering"),
    (["--occupancy_tree", "t.npz", "--occupancy_reso", "48"], "need a power of two"),
    (["--occupancy_reso", "2048"], "occupancy_reso=2048 (need 1..1024"),
    (["--occupancy_alpha_thresh", "1.0"], "occupancy_alpha_thresh=1"),
])
def test_render_refusals_by_name(argv, words):
    a = _args("--occupancy_reso", "32", *argv)
    with pytest.raises(NotImplementedError) as e:
        families.check(a, "render")
    assert words in str(e.value), str(e.value)
    # the same flags without the grid are not refused for it
    a.occupancy_reso, a.occupancy_tree = 0, ""
    try:
        families.check(a, "render")
    except NotImplementedError as e2:
        assert "occupancy" not in str(e2)


def test_noise_without_randomized_and_spherified_llff_pass_the_occupancy_clause():
    assert occupancy.clauses(_args("--occupancy_reso", "32", "--noise_std", "1.0", "--randomized", "false")) == []
    assert occupancy.clauses(_args("--occupancy_reso", "32", "--dataset", "llff", "--spherify", "true")) == []
    assert occupancy.clauses(_args("--occupancy_tree", "t.npz")) != []


@pytest.mark.parametrize("purpose", ["train", "extract", "mesh"])
@pytest.mark.parametrize("family", [[], ["--sg_dim", "9", "--sh_deg", "-1"]])
def test_every_other_entry_point_refuses_the_grid(purpose, family):
    a = _args("--occupancy_reso", "32", *family)
    with pytest.raises(NotImplementedError, match="culling inside training"):
        families.check(a, purpose)


def test_render_fn_without_the_flag_is_model_apply(capsys):
    calls = []
    model = types.SimpleNamespace(apply=lambda *a, **k: calls.append((a, k)) or "out", cfg=ops.make_cfg())
    fn, live = occupancy.render_fn(_args(), model, "state", say=print)
    assert live is None and fn("rays") == "out"
    assert calls == [(("state", "rays", False), {})]             # today's call, no occupancy argument
    assert capsys.readouterr().out == ""


def test_live_rows_bookkeeping():
    live = occupancy.LiveRows(ops.make_cfg(num_coarse_samples=8, num_fine_samples=16))
    live.add([40, 60], 10)
    live.add([0, 60], 10)
    assert live.fractions() == [40 / 160, 120 / 480]
    assert live.line() == "live rows: coarse 25.00 %, fine 25.00 %"
    live.reset()
    assert live.fractions() == [0.0, 0.0]


# ---- refusals: grids ------------------------------------------------------------------------------------------------------------
def test_grid_holder_refusals():
    bits = torch.zeros(R.words(5), dtype=torch.int32)
    g = ops.OccupancyGrid(bits, 5, [0.5] * 3, [0.25] * 3)
    assert g.fraction_occupied() == 0.0 and not g.outside_live
    bits[3] = 1 << 28
    bits[0] = -1                                                  # 32 bits, sign bit included
    assert g.count_occupied() == 33 and g.fraction_occupied() == 33 / 125
    for kw, words in ((dict(reso=0), "reso 0"), (dict(reso=1025), "reso 1025"), (dict(scale=[0.25, 0.0, 0.25]), "zero or non-finite"),
                      (dict(scale=[0.25, float("inf"), 0.25]), "zero or non-finite"),
                      (dict(scale=[float("nan")] * 3), "zero or non-finite"), (dict(bits=bits[:3]), "4 words"),
                      (dict(bits=bits.float()), "int32"), (dict(bits=None), "int32")):
        args = dict(bits=bits, reso=5, offset=[0.5] * 3, scale=[0.25] * 3)
        args.update(kw)
        with pytest.raises(_lib.PxoError, match=words):
            ops.OccupancyGrid(**args)
    for kw, words in ((dict(reso=0), "reso"), (dict(dilate=2), "dilate"), (dict(outside="maybe"), "outside")):
        args = dict(reso=8, dilate=1, outside="empty")
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            occupancy.check_grid_args(**args)


def test_from_tree_refuses_compressed_and_ndc_trees(tmp_path):
    from plenoctree_amd.octree import svox
    with pytest.raises(NotImplementedError, match="NDC tree"):
        occupancy.from_tree("whatever.npz", 3, ndc=svox.NDCConfig(8, 8, 10.0))
    p = str(tmp_path / "q.npz")
    np.savez(p, quant_colors=np.zeros(1), data_format="SH9")
    with pytest.raises(NotImplementedError, match="compressed tree"):
        occupancy.from_tree(p, 3)
    q = object.__new__(svox.QuantizedN3Tree)
    with pytest.raises(NotImplementedError, match="compressed tree"):
        occupancy.from_tree(q, 3)


# ---- refusals: the C ABI, all before the first HIP call ---------------------------------------------------------------------
def _grid_struct(bits=1, reso=8, scale=(0.25, 0.25, 0.25), outside=0):
    g = _lib.PxoOccGrid()
    g.bits = bits                                                 # never dereferenced: every call below is refused first
    g.reso = reso
    g.offset = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    g.scale = (ctypes.c_float * 3)(*scale)
    g.outside_live = outside
    return g


def _render_culled(lib, cfg, occ, randomized=0):
    nil = [None] * 5
    return lib.pxo_render_fwd_culled(ctypes.byref(cfg), occ, None, *nil, 4, randomized, None, None, 0, *([None] * 6), None, None, 0,
                                     None)


def test_c_abi_refusals():
    lib = _lib.load()
    cfg = ops.make_cfg(num_coarse_samples=8, num_fine_samples=16, sh_deg=2)
    err = lambda: lib.pxo_last_error().decode()
    assert _render_culled(lib, cfg, None) == -1 and "occ is NULL" in err()
    assert _render_culled(lib, cfg, ctypes.byref(_grid_struct(bits=None))) == -1 and "occ->bits is NULL" in err()
    for reso in (0, -3, 1025):
        assert _render_culled(lib, cfg, ctypes.byref(_grid_struct(reso=reso))) == -1 and f"reso {reso} outside [1,1024]" in err()
    for sc in ((0.25, 0.0, 0.25), (float("nan"), 0.25, 0.25), (0.25, 0.25, float("inf")), (0.25, float("-inf"), 0.25)):
        assert _render_culled(lib, cfg, ctypes.byref(_grid_struct(scale=sc))) == -1 and "zero or not finite" in err(), sc
    noisy = ops.make_cfg(num_coarse_samples=8, num_fine_samples=16, sh_deg=2, noise_std=0.5)
    assert _render_culled(lib, noisy, ctypes.byref(_grid_struct()), randomized=1) == -4 and "resurrect" in err()   # PXO_ERR_UNSUPPORTED
    # the cull takes the same grid checks; pack and expand their own
    n = ctypes.c_size_t(0)
    assert lib.pxo_occ_cull(None, None, 4, None, None, None, None, 0, None) == -1 and "occ is NULL" in err()
    assert lib.pxo_occ_cull(ctypes.byref(_grid_struct(reso=2000)), None, 4, None, None, None, None, 0, None) == -1 and "reso" in err()
    assert lib.pxo_occ_cull(ctypes.byref(_grid_struct()), None, 1 << 31, None, None, None, None, 0, None) == -1 and "2^31" in err()
    assert lib.pxo_occ_cull_workspace_bytes(1 << 31, ctypes.byref(n)) == -1
    assert lib.pxo_occ_cull_workspace_bytes(1000, ctypes.byref(n)) == 0 and 1000 <= n.value <= 1000 + 3 * 256
    assert lib.pxo_occ_pack(None, 0, 0.0, 0, None, None) == -1 and "reso 0" in err()
    assert lib.pxo_occ_pack(None, 8, 0.0, 2, None, None) == -1 and "dilate 2" in err()
    assert lib.pxo_occ_pack(None, 8, 0.0, 1, None, None) == -1 and "null" in err()
    assert lib.pxo_occ_expand(None, None, None, 4, 0, None, None, None) == -1 and "C = 0" in err()
    assert lib.pxo_occ_expand(None, None, None, 4, 3, None, None, None) == -1 and "null" in err()
    assert lib.pxo_occ_expand(None, None, None, 0, 3, None, None, None) == 0                       # no row: nothing is touched
    assert lib.pxo_version() == _lib.ABI_VERSION                                                    # new entry points, same ABI
