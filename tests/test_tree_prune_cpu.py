"""Host side of pruning a PlenOctree by its leaves' weights (no GPU): the test oracle against closed forms, the numpy
restatement of the collapse on hand-built trees, what the GPU tests' bounds rest on (per-sample float32 floor, left-out
share), the flags and by-name refusals of octree.pruning, and N3Tree.accumulate_weights / prune_ / refine_leaves with
octree_ops stubbed.

Measured here (tests/_tree_prune_oracle.py::all_cases, every input the GPU weight tests use): the largest |float32 - float64|
of one sample's weight is 1.247e-7 (camera case, three cameras on the depth-6 shell); PER_SAMPLE_FLOOR rounds it up to 1.25e-7.
No case leaves out a single leaf: every float64 weight that is positive is above 1e-30."""
import math
import os

import numpy as np
import pytest
import torch

import _octree_cases as C
import _quant_cases as Q
import _tree_prune_oracle as P
from oracle import octree_oracle as T
from plenoctree_amd import _lib, build
from plenoctree_amd.octree import pruning, svox

f32 = np.float32
PER_SAMPLE_FLOOR = 1.25e-7


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return _lib.load()


# ---- the oracle against closed forms ------------------------------------------------------------------------------------
def _two_cell_tree(sigma_a, sigma_b):
    """Root only, world cube [-1, 1]^3: the ray along +x at (y, z) = (0.3, 0.4) crosses cells (0,1,1) then (1,1,1), 1.0 each."""
    t = T.Tree(4, 1, [0.0, 0.0, 0.0], 1.0)
    t.data[0, 0, 1, 1, -1] = sigma_a
    t.data[0, 1, 1, 1, -1] = sigma_b
    return t, 0 * 8 + 3, 0 * 8 + 7


STEP_KNOWN = 1e-4
ORIGIN, ALONG_X = np.array([-3.0, 0.3, 0.4], f32), np.array([1.0, 0.0, 0.0], f32)


def test_oracle_single_uniform_leaf():
    """One occupied leaf of length L = 1: w = 1 - exp(-sigma L).  The march's sample is longer than the chord by the step
    (world length 2e-4 here), so |w - closed form| <= sigma * 2e-4."""
    sigma = 1.5
    t, a, b = _two_cell_tree(sigma, 0.0)
    lw = P.single_ray_weights(t, ORIGIN, ALONG_X, T.RenderOptions(STEP_KNOWN))
    want = 1.0 - math.exp(-sigma * 1.0)
    assert lw.count[a] == 1 and lw.count.sum() == 1
    assert abs(lw.max64[a] - want) <= sigma * 2e-4 and abs(float(lw.max32[a]) - want) <= sigma * 2e-4 + 1e-6
    assert lw.sum64[a] == lw.max64[a] and np.count_nonzero(lw.max64) == 1


def test_oracle_two_leaves_in_a_row():
    """The second leaf's weight is exp(-s1 L1) (1 - exp(-s2 L2)); the step overshoot moves each factor by at most s * 2e-4."""
    s1, s2 = 1.5, 0.8
    t, a, b = _two_cell_tree(s1, s2)
    lw = P.single_ray_weights(t, ORIGIN, ALONG_X, T.RenderOptions(STEP_KNOWN))
    want_a = 1.0 - math.exp(-s1)
    want_b = math.exp(-s1) * (1.0 - math.exp(-s2))
    assert lw.count[a] == 1 and lw.count[b] == 1
    assert abs(lw.max64[a] - want_a) <= s1 * 2e-4
    assert abs(lw.max64[b] - want_b) <= (s1 + s2) * 2e-4
    # the early-stop preset's sigma threshold takes a thin second leaf out of the set
    t.data[0, 1, 1, 1, -1] = 5e-3
    fast = P.single_ray_weights(t, ORIGIN, ALONG_X, T.RenderOptions(STEP_KNOWN, 1.0, 1e-2, 1e-2))
    assert fast.count[b] == 0 and fast.max64[b] == 0.0 and fast.count[a] == 1


def test_oracle_max_against_sum_over_two_rays():
    """Two rays through the same two leaves (the second enters at another height, same lengths): sum = 2 w, max = w."""
    s1, s2 = 1.5, 0.8
    t, a, b = _two_cell_tree(s1, s2)
    opt = T.RenderOptions(STEP_KNOWN)
    o2 = np.array([-3.0, 0.6, 0.7], f32)
    one = P.single_ray_weights(t, ORIGIN, ALONG_X, opt)
    two = P.leaf_weights(t, P.march_rays(t, [ORIGIN, o2], [ALONG_X, ALONG_X], STEP_KNOWN), opt)
    for leaf in (a, b):
        assert two.count[leaf] == 2
        assert abs(two.sum64[leaf] - 2.0 * one.max64[leaf]) <= 1e-6
        assert abs(two.max64[leaf] - one.max64[leaf]) <= 1e-6
        assert two.sum64[leaf] > 1.9 * two.max64[leaf]
    assert two.floor <= PER_SAMPLE_FLOOR


def test_gpu_bounds_rest_on_what_is_measured_here():
    """Over every input of the GPU weight tests: the per-sample float32 floor is within PER_SAMPLE_FLOOR (the figure the sum
    bound multiplies by 4), no case leaves out more than 2 % of its touched leaves (none leaves out any), and the float32
    restatement touches exactly the leaves the float64 one does."""
    worst = 0.0
    for name, lw in P.all_cases().items():
        worst = max(worst, lw.floor)
        touched = int((lw.max32 > 0).sum())
        for op in ("max", "sum"):
            out = int(P.left_out(lw, op).sum())
            assert out <= 0.02 * touched, (name, op, out, touched)
            assert out == 0, (name, op, out)                       # stated in the GPU tests: no case leaves any out
        assert np.array_equal(lw.max32 > 0, lw.max64 > 0) and np.array_equal(lw.sum32 > 0, lw.count > 0), name
    print(f"per-sample floor over all cases: {worst:.4g}")
    assert worst <= PER_SAMPLE_FLOOR
    lw, misses = P.ndc_case("rays")
    assert misses >= 5 and int((lw.max32 > 0).sum()) > 100         # the d_z >= 0 rays are misses; the others see the tree
    assert lw.count[P.ndc_tree().child.reshape(-1) != 0].sum() == 0


# ---- the collapse restatement on hand-built trees ---------------------------------------------------------------------------
def test_collapse_nothing_dead_is_the_identity():
    t = P.nest_tree()
    child, pd, data, old2new = P.collapse(t.child, t.parent_depth, t.data, np.ones((t.n_internal, 8), bool))
    assert np.array_equal(child, t.child) and np.array_equal(pd, t.parent_depth) and np.array_equal(data, t.data)
    assert np.array_equal(old2new, np.arange(t.n_internal))


def test_collapse_everything_dead_leaves_the_root():
    t = P.nest_tree()
    child, pd, data, old2new = P.collapse(t.child, t.parent_depth, t.data, np.zeros((t.n_internal, 8), bool))
    assert child.shape == (1, 2, 2, 2) and not child.any() and not data.any() and np.array_equal(pd, [[0, 0]])
    assert np.array_equal(old2new, [0, -1, -1, -1, -1])


def test_collapse_cascade_of_three_levels():
    t = P.nest_tree()
    child, pd, data, old2new = P.collapse(t.child, t.parent_depth, t.data, P.nest_keep_cascade(t))
    assert np.array_equal(old2new, [0, -1, -1, -1, 1])             # nodes 3, 2, 1 went; node 4 moved up
    flat = child.reshape(-1, 8)
    assert flat[0, 5] == 0 and flat[0, 1] == 1 and np.count_nonzero(flat) == 1
    assert np.array_equal(pd, [[0, 0], [1, 1]])
    rows, src = data.reshape(-1, 8, 4), t.data.reshape(-1, 8, 4)
    assert not rows[0, 5].any()                                    # the cell that pointed to the nest is a dead leaf now
    keep_rows = [c for c in range(8) if c != 5]
    assert np.array_equal(rows[0, keep_rows], src[0, keep_rows]) and np.array_equal(rows[1], src[4])
    assert P.valid_tree(child, pd)


def test_collapse_seven_dead_siblings_and_one_live():
    t = P.nest_tree()
    child, pd, data, old2new = P.collapse(t.child, t.parent_depth, t.data, P.seven_dead_keep(t))
    assert np.array_equal(child, t.child) and np.array_equal(pd, t.parent_depth)
    assert np.array_equal(old2new, np.arange(t.n_internal))
    rows, src = data.reshape(-1, 8, 4), t.data.reshape(-1, 8, 4)
    assert np.array_equal(rows[3, 4], src[3, 4]) and not rows[3, [0, 1, 2, 3, 5, 6, 7]].any()
    assert np.array_equal(rows[[0, 1, 2, 4]], src[[0, 1, 2, 4]])


def test_collapse_of_a_deep_tree_stays_a_tree_in_level_order():
    """shell, depth 6, leaves kept at random: the collapsed tree is valid (every child points forward to a node whose record
    points back), level order survives, and the survivors are renumbered in their storage order."""
    t = C.make_tree("shell", 6, 1)
    keep = np.random.RandomState(4).rand(t.n_internal, 8) < 0.3
    ct, old2new = P.collapsed_tree(t, keep)
    assert P.valid_tree(ct.child, ct.parent_depth) and ct.n_internal < t.n_internal
    assert not (np.diff(ct.parent_depth[:, 1]) < 0).any()
    survivors = np.nonzero(old2new >= 0)[0]
    assert np.array_equal(old2new[survivors], np.arange(len(survivors)))


# ---- octree.pruning: flags and refusals ---------------------------------------------------------------------------------
def _cfg(tmp_path):
    path = os.path.join(str(tmp_path), "tiny.yaml")
    with open(path, "w") as f:
        f.write("dataset: synthetic\nfactor: 16\nwhite_bkgd: true\nsh_deg: 1\n")
    return path


def test_pruning_flags_parse(tmp_path):
    cfg = _cfg(tmp_path)
    a = pruning.define_flags().parse_args(["--config", cfg])
    assert (a.input, a.output, a.weight_thresh, a.no_collapse, a.refine_thresh, a.renderer_step_size, a.eval) == \
        ("./tree_opt.npz", "./tree_pruned.npz", 1e-3, False, None, 1e-4, False)
    a = pruning.define_flags().parse_args(["--config", cfg, "--data_dir", "D", "--input", "a.npz", "--output", "b.npz",
                                           "--weight_thresh", "0.01", "--no_collapse", "--refine_thresh", "0.2",
                                           "--renderer_step_size", "1e-3", "--eval", "true"])
    assert (a.input, a.output, a.weight_thresh, a.no_collapse, a.refine_thresh, a.renderer_step_size, a.eval, a.data_dir) == \
        ("a.npz", "b.npz", 0.01, True, 0.2, 1e-3, True, "D")
    pruning.check_flags(a)
    # the five existing entry points keep their flags: none of the new ones leaks into them
    from plenoctree_amd.octree import evaluation, extraction, optimization
    for mod in (evaluation, extraction, optimization):
        with pytest.raises(SystemExit):
            mod.define_flags().parse_args(["--config", cfg, "--no_collapse"])


def test_pruning_refusals_by_name(tmp_path):
    cfg = _cfg(tmp_path)
    with pytest.raises(NotImplementedError, match="octree.pruning: --render_path"):
        pruning.main(["--config", cfg, "--render_path", "true"])
    with pytest.raises(ValueError, match="--refine_thresh 0.0005"):
        pruning.main(["--config", cfg, "--refine_thresh", "0.0005"])
    with pytest.raises(ValueError, match="--weight_thresh -1"):
        pruning.main(["--config", cfg, "--weight_thresh", "-1"])
    packed = Q.case(4, 1, 8).save(str(tmp_path / "compressed.npz"))
    with pytest.raises(NotImplementedError, match="compressed tree"):
        pruning.main(["--config", cfg, "--input", packed])


# ---- N3Tree.accumulate_weights / prune_ / refine_leaves with octree_ops stubbed -------------------------------------------
def _cpu_tree():
    t = svox.N3Tree(N=2, data_dim=4, data_format="SH1", depth_limit=3)
    t._refine_packed(torch.tensor([2, 5]))
    t.data.requires_grad_(False)
    return t


@pytest.fixture
def stubbed(monkeypatch):
    """octree_ops without a device: the launches record their arguments and return zeros."""
    calls = []
    oops = svox.oops

    def weight_cams(view, c2w_all, width, height, fx, opts, op, weights, fy=None, ndc=None):
        calls.append(("weights_cams", op, tuple(c2w_all.shape), width, height, fx, fy, ndc,
                      (opts.step_size, opts.sigma_thresh, opts.stop_thresh), weights))
        weights += 1.0

    def weight_rays(view, origins, dirs, opts, op, weights, ndc=None):
        calls.append(("weights_rays", op, origins.shape[0], ndc, (opts.step_size, opts.sigma_thresh, opts.stop_thresh), weights))
        weights += 1.0

    def render_persp(view, c2w, width, height, fx, opts, fy=None, **kw):
        calls.append(("rgb_persp", (opts.step_size, opts.sigma_thresh, opts.stop_thresh)))
        return torch.zeros(height, width, 3)

    def render_rays(view, origins, dirs, viewdirs, opts, **kw):
        calls.append(("rgb_rays",))
        return torch.zeros(origins.shape[0], 3)

    monkeypatch.setattr(oops, "tree_view", lambda *a, **k: "view")
    monkeypatch.setattr(oops, "octree_weight_accum_cams", weight_cams)
    monkeypatch.setattr(oops, "octree_weight_accum_rays", weight_rays)
    monkeypatch.setattr(oops, "octree_render_persp", render_persp)
    monkeypatch.setattr(oops, "octree_render_rays", render_rays)
    return calls


def test_accumulator_launches_only_inside_the_block(stubbed):
    t = _cpu_tree()
    r = svox.VolumeRenderer(t, step_size=1e-3)
    rays = torch.zeros(5, 3)
    with torch.no_grad():
        r.render_persp(torch.eye(4), width=6, height=4, fx=5.0)
        r.forward(rays, rays, rays)
        assert [c[0] for c in stubbed] == ["rgb_persp", "rgb_rays"]
        del stubbed[:]
        with t.accumulate_weights(op="max") as accum:
            assert accum.value.shape == (t.n_internal, 2, 2, 2) and accum() is accum.value and not accum.value.any()
            r.render_persp(torch.eye(4), width=6, height=4, fx=5.0, fast=True)
            r.forward(rays, rays, rays)
        kinds = [c[0] for c in stubbed]
        assert kinds == ["weights_cams", "rgb_persp", "weights_rays", "rgb_rays"]
        cams, rgb = stubbed[0], stubbed[1]
        assert cams[1:8] == ("max", (1, 4, 4), 6, 4, 5.0, None, None)
        assert cams[8] == rgb[1] and cams[8][1:] == (pytest.approx(1e-2), pytest.approx(1e-2))    # the same _opts(fast)
        assert stubbed[2][1:4] == ("max", 5, None)
        assert cams[9].data_ptr() == accum.value.data_ptr() and stubbed[2][5].data_ptr() == accum.value.data_ptr()
        assert float(accum.value.min()) == 2.0                    # both launches accumulated into the one buffer
        del stubbed[:]
        r.render_persp(torch.eye(4), width=6, height=4, fx=5.0)      # the block is over: nothing but rgb
        assert [c[0] for c in stubbed] == ["rgb_persp"] and t._weight_accum is None
        assert float(accum.value.min()) == 2.0                    # still readable after the block


def test_accumulator_differentiable_path_and_default_op(stubbed):
    t = _cpu_tree()
    t.data.requires_grad_(True)
    r = svox.VolumeRenderer(t, step_size=1e-3)
    with t.accumulate_weights() as accum:
        assert accum.op == "sum"
        im = r.render_persp(torch.eye(4), width=6, height=4, fx=5.0)
        assert im.requires_grad
        with pytest.raises(svox.PxoError, match="not differentiable"):
            r.render_persp(torch.eye(4), width=6, height=4, fx=5.0, fast=True)
    assert [c[0] for c in stubbed] == ["weights_cams", "rgb_persp"]
    assert stubbed[0][1] == "sum" and stubbed[0][8][1:] == (0.0, 0.0)


def test_accumulator_nesting_and_structure_change_raise(stubbed):
    t = _cpu_tree()
    r = svox.VolumeRenderer(t)
    with pytest.raises(ValueError, match="'sum' or 'max'"):
        t.accumulate_weights(op="mean")
    with torch.no_grad():
        with t.accumulate_weights("max"):
            with pytest.raises(svox.PxoError, match="do not nest"):
                with t.accumulate_weights("sum"):
                    pass
            assert t._weight_accum is not None                   # the failed inner block did not close the outer one
            r.render_persp(torch.eye(4), width=4, height=4, fx=4.0)
            t.refine_leaves(torch.ones(t.n_internal, 2, 2, 2, dtype=torch.bool))
            with pytest.raises(svox.PxoError, match="structure changed inside the block"):
                r.render_persp(torch.eye(4), width=4, height=4, fx=4.0)
            with pytest.raises(svox.PxoError, match="structure changed inside the block"):
                r.forward(torch.zeros(1, 3), torch.zeros(1, 3), torch.zeros(1, 3))
        assert t._weight_accum is None
        with t.accumulate_weights("max"):                         # a new block on the refined tree is fine
            r.render_persp(torch.eye(4), width=4, height=4, fx=4.0)
        # a clone does not inherit the open block
        with t.accumulate_weights("max"):
            assert t.clone()._weight_accum is None


def test_refine_leaves_and_prune_without_collapse_on_the_host():
    t = _cpu_tree()
    n0, leaves0 = t.n_internal, t.n_leaves
    with torch.no_grad():
        t.data.copy_(torch.arange(t.data.numel(), dtype=torch.float32).reshape(t.data.shape) + 1.0)
    mask = torch.zeros(n0, 2, 2, 2, dtype=torch.bool)
    mask.view(-1)[[2, 3, 8 + 1]] = True                          # cell 2 is internal (ignored), 3 and 9 are leaves
    assert t.refine_leaves(mask) == 2 and t.n_internal == n0 + 2 and t.n_leaves == leaves0 + 14
    assert not t._level_order                                    # a depth-0 leaf was split after depth-1 nodes existed
    d = t.data.data.view(-1, 4)
    assert torch.equal(d[n0 * 8:(n0 + 1) * 8], d[3].expand(8, 4))  # children inherit the value
    # at depth_limit nothing splits
    deep = svox.N3Tree(N=2, data_dim=4, data_format="SH1", depth_limit=1)
    deep._refine_packed(torch.tensor([0]))
    assert deep.refine_leaves(torch.ones(2, 2, 2, 2, dtype=torch.bool)) == 7        # the root's leaves; node 1's are at the limit
    assert deep.refine_leaves(torch.ones(deep.n_internal, 2, 2, 2, dtype=torch.bool)) == 0
    assert int(deep.parent_depth[:, 1].max()) == 1 and deep.n_internal == 9
    # prune_ without collapse: dead leaves zeroed, internal cells and kept leaves untouched, nothing removed
    keep = torch.ones(t.n_internal, 2, 2, 2, dtype=torch.bool)
    keep.view(-1)[[2, 4, 9]] = False                             # 2 and 9 are internal now, 4 is a leaf
    ref = t.data.data.clone()
    assert t.prune_(keep, collapse=False) == 0
    ref.view(-1, 4)[4] = 0
    assert torch.equal(t.data.data, ref)
    with pytest.raises(ValueError, match="bool over the tree's"):
        t.prune_(torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool over the tree's"):
        t.refine_leaves(torch.ones(t.n_internal, 2, 2, 2))


def test_quantized_tree_refuses_all_three(tmp_path):
    q = svox.N3Tree.load(Q.case(4, 1, 8).save(str(tmp_path / "tree.npz")), keep_quantized=True)
    mask = torch.ones(q.n_internal, 2, 2, 2, dtype=torch.bool)
    for name, op in (("accumulate_weights", lambda: q.accumulate_weights("max")), ("prune_", lambda: q.prune_(mask)),
                     ("refine_leaves", lambda: q.refine_leaves(mask))):
        with pytest.raises(svox.PxoError, match=name + r".*dequantize\(\)"):
            op()
