"""Host side of the level of detail of a PlenOctree (no GPU): the oracle's known answers on a hand-written two-level tree,
N3Tree.lod(L, fill=False) / lod_child on CPU trees whose internal rows the test wrote itself (one source in level order, one
not), the npz round trip and octree.compression on the result, the filled mark, and the by-name refusals of octree.lod,
octree.evaluation --max_depth and VolumeRenderer(max_depth=...)."""
import argparse
import os

import numpy as np
import pytest
import torch

import _lod_oracle as L
import _quant_cases as Q
from plenoctree_amd import _lib, build
from plenoctree_amd.octree import compression, evaluation, lod, svox

f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return _lib.load()


# ---- the entry point's argument checks (host side: nothing is launched) ---------------------------------------------------
def test_lod_fill_argument_checks(lib):
    import ctypes
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    fill = lambda child=ptr, pd=ptr, data=ptr, n=5, D=49, depth=3: lib.pxo_tree_lod_fill(child, pd, data, n, D, depth, None)
    for bad, what in ((dict(D=48), b"data_dim 48"), (dict(D=0), b"data_dim 0"), (dict(D=3 * 36 + 1), b"data_dim 109"),
                      (dict(depth=-1), b"max_depth -1"), (dict(depth=_lib.TREE_MAX_DEPTH + 1), b"max_depth 11"),
                      (dict(n=0), b"n_internal 0"), (dict(n=1 << 28), b"n_internal"), (dict(child=None), b"null pointer"),
                      (dict(pd=None), b"null pointer"), (dict(data=None), b"null pointer")):
        assert fill(**bad) == -1, bad                                    # PXO_ERR_ARG
        err = lib.pxo_last_error()
        assert b"pxo_tree_lod_fill" in err and what in err, (bad, err)
    # a root-only tree is a no-op: returns before anything is launched, for every width the formats allow
    for D in (4, 13, 28, 49, 76):
        assert fill(n=1, D=D, depth=0) == 0 and fill(n=1, D=D, depth=3) == 0 and fill(n=5, D=D, depth=0) == 0
    assert not any(buf)


# ---- the oracle's known answers -------------------------------------------------------------------------------------------
def _rows(sigmas, D=4):
    """Eight rows with distinct coefficients c_j[k] = 10 (j + 1) + k and the given sigmas."""
    rows = np.zeros((8, D))
    rows[:, :-1] = 10.0 * (np.arange(8)[:, None] + 1) + np.arange(D - 1)[None, :]
    rows[:, -1] = sigmas
    return rows


def test_oracle_value_of_a_node_with_two_dense_cells():
    """sigmas [1, 3, 0, ...]: S = 4, sigma = 0.5, c[k] = (1 (10 + k) + 3 (20 + k)) / 4 = 17.5 + k; the six empty cells, whose
    coefficients are 30 .. 80, do not enter."""
    v = L.node_value(_rows([1, 3, 0, 0, 0, 0, 0, 0]))
    assert np.array_equal(v, [17.5, 18.5, 19.5, 0.5])
    b = L.node_bound(_rows([1, 3, 0, 0, 0, 0, 0, 0]))
    assert b[-1] == 8 * 2.0 ** -24 * 0.5 and np.allclose(b[:-1], 16 * 2.0 ** -24 * (17.5 + np.arange(3)), rtol=1e-12)


def test_oracle_value_of_an_empty_node_is_an_all_zero_row():
    for sig in ([0.0] * 8, [-1.0, -0.5, 0, 0, -3, 0, 0, -1e-3]):
        v = L.node_value(_rows(sig))
        assert not v.any() and not np.signbit(v).any()
        assert L.node_bound(_rows(sig))[-1] == 0.0


def test_oracle_negative_sigma_enters_as_weight_zero():
    """-5 beside 2: without the clamp S would be -3 (or the mean would be pulled towards cell 0); with it the node is cell 1's
    colour at an eighth of its density."""
    v = L.node_value(_rows([-5, 2, 0, 0, 0, 0, 0, 0]))
    assert np.array_equal(v, [20.0, 21.0, 22.0, 0.25])


def test_oracle_fill_on_a_two_level_tree():
    """Root with one child at cell 5; the child's cells are leaves.  The fill writes the child's value into root row 5 and
    nothing else."""
    child = np.zeros((2, 2, 2, 2), np.int32)
    child.reshape(-1)[5] = 1
    pd = np.array([[0, 0], [5, 1]], np.int32)
    data = np.random.RandomState(0).randn(2, 2, 2, 2, 4).astype(f32)
    data[1].reshape(8, 4)[:] = _rows([1, 3, 0, 0, 0, 0, 0, 0])
    out = L.fill(child, pd, data)
    want = data.astype(np.float64)
    want.reshape(-1, 4)[5] = [17.5, 18.5, 19.5, 0.5]
    assert np.array_equal(out, want)
    c0, pd0, d0 = L.lod(child, pd, out, 0)
    assert c0.shape == (1, 2, 2, 2) and not c0.any() and np.array_equal(pd0, [[0, 0]]) and np.array_equal(d0[0], out[0])
    c1, pd1, d1 = L.lod(child, pd, out, 1)
    assert np.array_equal(c1, child) and np.array_equal(pd1, pd)
    assert not d1.reshape(-1, 4)[5].any() and np.array_equal(np.delete(d1.reshape(-1, 4), 5, 0), np.delete(out.reshape(-1, 4), 5, 0))


# ---- N3Tree.lod / lod_child on CPU trees ----------------------------------------------------------------------------------
def _marked(tree):
    """Every row written by the test: row r holds r + 1 + k / 16 (exact in float16 as well, up to 2047), internal rows too."""
    n, D = tree.n_internal, tree.data_dim
    with torch.no_grad():
        tree.data.copy_((torch.arange(n * 8, dtype=torch.float32)[:, None] + 1.0 +
                         torch.arange(D, dtype=torch.float32)[None, :] / 16.0).reshape(n, 2, 2, 2, D))
    tree.data.requires_grad_(False)
    return tree


def _level_order_tree():
    """Depth 3, 1 + 2 + 3 + 2 nodes, whole levels refined one at a time."""
    t = svox.N3Tree(N=2, data_dim=4, data_format="SH1", depth_limit=4)
    t._refine_packed(torch.tensor([2, 5]))                               # depth 1: nodes 1, 2
    t._refine_packed(torch.tensor([8 + 1, 8 + 6, 16 + 3]))               # depth 2: nodes 3, 4, 5
    t._refine_packed(torch.tensor([24 + 0, 40 + 7]))                     # depth 3: nodes 6, 7
    assert t._level_order and t.level_nodes == [1, 2, 3, 2]
    return _marked(t)


def _out_of_order_tree():
    """The same, then a shallow leaf (root cell 7, then a cell of the new depth-1 node) split after the deeper nodes exist."""
    t = _level_order_tree()
    t._refine_packed(torch.tensor([7]))                                  # node 8 at depth 1
    t._refine_packed(torch.tensor([64 + 2]))                             # node 9 at depth 2
    assert not t._level_order and t.level_nodes == [1, 3, 4, 2]
    assert (np.diff(t.parent_depth[:, 1].numpy()) < 0).any()
    return _marked(t)


SOURCES = {"level_order": _level_order_tree, "out_of_order": _out_of_order_tree}


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_lod_without_fill_on_a_cpu_tree(source):
    src = SOURCES[source]()
    child0, pd0, data0 = src.child.numpy().copy(), src.parent_depth.numpy().copy(), src.data.data.numpy().copy()
    D = src.data_dim
    for lvl in range(src.max_depth + 1):
        t = src.lod(lvl, fill=False)
        assert isinstance(t, svox.N3Tree) and t is not src and not src._lod_filled
        child, pd, data = t.child.numpy(), t.parent_depth.numpy(), t.data.data.numpy()
        assert t.n_internal == sum(src.level_nodes[:lvl + 1]) and t.level_nodes == src.level_nodes[:lvl + 1]
        assert t.max_depth == lvl and child.dtype == np.int32 and pd.dtype == np.int32 and data.dtype == np.float32
        assert child.shape == (t.n_internal, 2, 2, 2) and data.shape == (t.n_internal, 2, 2, 2, D)
        assert not child[pd[:, 1] == lvl].any()                          # the depth-L pointers are zero
        assert L.valid_tree(child, pd)                                   # each node's parent cell points back at it
        want = L.lod(child0, pd0, data0, lvl)
        for got, ref in zip((child, pd, data), want):
            assert got.dtype == ref.dtype and np.array_equal(got, ref)
        # told apart by what the test wrote: row r of the source holds r + 1 in its first channel
        kept = np.nonzero(pd0[:, 1] <= lvl)[0]
        rows, src_rows = data.reshape(-1, 8, D), data0.reshape(-1, 8, D)[kept]
        src_child = child0.reshape(-1, 8)[kept]
        at_cut = (pd0[kept, 1] == lvl)[:, None]
        leaf = src_child == 0
        assert np.array_equal(rows[leaf].view(np.uint32), src_rows[leaf].view(np.uint32))          # surviving leaves, bit for bit
        cut = ~leaf & at_cut
        assert np.array_equal(rows[cut], src_rows[cut]) and (rows[cut][:, 0] >= 1).all()          # former internal rows at L
        assert not rows[~leaf & ~at_cut].any()                                                     # rows above are zero
        if lvl < src.max_depth:
            assert cut.any() and (~leaf & ~at_cut).any() == (lvl > 0)
        assert t._level_order == (not (np.diff(pd[:, 1]) < 0).any())
        assert torch.equal(t.offset, src.offset) and torch.equal(t.invradius, src.invradius) and t.offset is not src.offset
        assert (str(t.data_format), t.depth_limit, t.geom_resize_fact, t.extra_data) == ("SH1", 4, 1.0, None)
    # the source is untouched
    assert np.array_equal(src.child.numpy(), child0) and np.array_equal(src.data.data.numpy(), data0)


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_lod_at_max_depth_is_the_identity_on_structure_and_leaves(source):
    src = SOURCES[source]()
    t = src.lod(src.max_depth, fill=False)
    assert torch.equal(t.child, src.child) and torch.equal(t.parent_depth, src.parent_depth)
    leaf = src.child == 0
    assert torch.equal(t.data.data[leaf], src.data.data[leaf]) and not t.data.data[~leaf].any()
    assert t.child.data_ptr() != src.child.data_ptr() and t.level_nodes == src.level_nodes


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_lod_child(source):
    src = SOURCES[source]()
    depth = src.parent_depth[:, 1]
    for lvl in range(src.max_depth + 1):
        c = src.lod_child(lvl)
        assert c.dtype == torch.int32 and c.shape == src.child.shape and c.data_ptr() != src.child.data_ptr()
        assert not c[depth >= lvl].any() and torch.equal(c[depth < lvl], src.child[depth < lvl])
    assert torch.equal(src.lod_child(src.max_depth), src.child * (depth < src.max_depth).int()[:, None, None, None])
    assert not src.lod_child(0).any()


def test_lod_depth_out_of_range_is_a_value_error():
    src = _level_order_tree()
    for bad in (-1, 4, 2.0, True, None):
        with pytest.raises(ValueError, match=r"outside \[0, 3\]"):
            src.lod(bad, fill=False)
        with pytest.raises(ValueError, match=r"outside \[0, 3\]"):
            src.lod_child(bad)


def test_lod_with_fill_on_a_cpu_tree_has_no_fallback():
    with pytest.raises(svox.PxoError):
        _level_order_tree().lod(1)


def test_lod_carries_sg_lobes_as_a_copy():
    lobes = np.array([[2.0, 0, 0, 1], [3.0, 0, 1, 0], [1.5, 1, 0, 0], [4.0, 0, 0, -1]], f32)
    t = svox.N3Tree(N=2, data_dim=13, data_format="SG4", depth_limit=3, extra_data=lobes, geom_resize_fact=2.0)
    t._refine_packed(torch.tensor([1]))
    c = _marked(t).lod(0, fill=False)
    assert str(c.data_format) == "SG4" and torch.equal(c.extra_data, t.extra_data) and c.extra_data is not t.extra_data
    assert c.extra_data.data_ptr() != t.extra_data.data_ptr() and c.geom_resize_fact == 2.0 and c.n_internal == 1
    assert torch.equal(c.data.data[0], t.data.data[0])


@pytest.mark.parametrize("source", sorted(SOURCES))
def test_lod_save_load_round_trip_and_compression(source, tmp_path):
    src = SOURCES[source]()
    t = src.lod(2, fill=False)
    path = str(tmp_path / "tree_d2.npz")
    t.save(path, compress=False)
    back = svox.N3Tree.load(path)
    assert torch.equal(back.child, t.child) and torch.equal(back.parent_depth, t.parent_depth)
    assert torch.equal(back.data.data, t.data.data.half().float()) and torch.equal(back.data.data, t.data.data)   # exact in float16
    assert back.level_nodes == t.level_nodes and back.depth_limit == t.depth_limit and back._level_order == t._level_order
    assert torch.equal(back.offset, t.offset) and torch.equal(back.invradius, t.invradius)
    half = svox.N3Tree.load(path, keep_half=True)
    assert half.n_internal == t.n_internal and torch.equal(half.to_float().data.data, t.data.data)
    dst = str(tmp_path / "tree_d2_min.npz")
    args = argparse.Namespace(noquant=False, bits=4, sigma_thresh=2.0, retain=0, weighted=False)
    assert compression.compress_file(path, dst, args) is True
    q = svox.N3Tree.load(dst)
    assert torch.equal(q.child, t.child) and q.n_internal == t.n_internal


# ---- the filled mark ------------------------------------------------------------------------------------------------------
def test_every_editing_method_clears_the_filled_mark(monkeypatch):
    monkeypatch.setattr(svox.oops, "tree_relu_sigma", lambda data: None)
    monkeypatch.setattr(svox.oops, "tree_lod_fill", lambda child, pd, data, max_depth: data)
    edits = {
        "refine": lambda t: t._refine_packed(torch.tensor([3])),
        "refine_leaves": lambda t: t.refine_leaves(torch.ones(t.n_internal, 2, 2, 2, dtype=torch.bool)),
        "prune_ without collapse": lambda t: t.prune_(torch.zeros(t.n_internal, 2, 2, 2, dtype=torch.bool), collapse=False),
        "tree[:] = value": lambda t: t.__setitem__(slice(None), 0.5),
        "tree[leaves, -1:] = value": lambda t: t.__setitem__((torch.tensor([0, 1]), slice(-1, None)), 0.5),
        "tree[:, -1:].relu_()": lambda t: t[:, -1:].relu_(),
        "tree[:, :2].relu_()": lambda t: t[:, :2].relu_(),
        "relu_sigma_": lambda t: t.relu_sigma_(),
        "max_depth_data": lambda t: t.max_depth_data(),
    }
    for name, edit in edits.items():
        t = _level_order_tree()
        assert not t._lod_filled
        assert t.fill_internal_() is t and t._lod_filled
        assert t.clone()._lod_filled                                     # a clone copies the rows, so it stays filled
        edit(t)
        assert not t._lod_filled, name
    t = _level_order_tree().fill_internal_()
    assert not t.lod(1)._lod_filled and t._lod_filled                    # the cut tree has zero rows, not a pyramid
    fresh = svox.N3Tree(N=2, data_dim=4, data_format="SH1")
    assert not fresh._lod_filled


def test_lod_fills_an_unmarked_source_once(monkeypatch):
    calls = []
    monkeypatch.setattr(svox.oops, "tree_lod_fill", lambda child, pd, data, max_depth: calls.append(max_depth))
    t = _level_order_tree()
    t.lod(1); t.lod(2); t.lod(0, fill=False)
    assert calls == [3]
    t[:] = 1.0
    t.lod(1, fill=False)
    assert calls == [3]
    t.lod(1)
    assert calls == [3, 3]


def test_capped_renderer_on_a_stubbed_device(monkeypatch):
    """The capped view is child-with-zeroed-pointers over the tree's own data; it is rebuilt after a structure edit and the
    tree refilled after a data edit; max_depth >= the tree's depth is the plain view; the refusals come before any launch."""
    seen = []
    fills = []
    monkeypatch.setattr(svox.oops, "tree_lod_fill", lambda child, pd, data, max_depth: fills.append(max_depth))
    monkeypatch.setattr(svox.oops, "tree_view", lambda child, data, offset, invradius: (child, data))
    monkeypatch.setattr(svox.oops, "octree_render_persp", lambda view, *a, **k: seen.append(view) or torch.zeros(2, 2, 3))
    monkeypatch.setattr(svox.oops, "octree_render_rays", lambda view, *a, **k: seen.append(view) or torch.zeros(1, 3))
    monkeypatch.setattr(svox.oops, "octree_weight_accum_cams", lambda *a, **k: seen.append("weights"))
    t = _level_order_tree()
    r = svox.VolumeRenderer(t, max_depth=1)
    assert fills == [] and r.max_depth == 1                              # nothing happens before the first render
    rays = torch.zeros(1, 3)
    r.render_persp(torch.eye(4), width=2, height=2, fx=2.0)
    r.forward(rays, rays, rays)
    assert fills == [3] and len(seen) == 2 and seen[0][0] is seen[1][0]  # filled once, the capped array cached
    assert torch.equal(seen[0][0], t.lod_child(1)) and seen[0][1].data_ptr() == t.data.data_ptr()
    t[:] = 2.0                                                           # a data edit through the class
    r.render_persp(torch.eye(4), width=2, height=2, fx=2.0)
    assert fills == [3, 3] and seen[2][0] is seen[0][0]                  # refilled; same structure, same capped array
    t.refine_leaves(torch.ones(t.n_internal, 2, 2, 2, dtype=torch.bool))
    r.render_persp(torch.eye(4), width=2, height=2, fx=2.0)
    assert fills == [3, 3, 4] and seen[3][0] is not seen[0][0] and torch.equal(seen[3][0], t.lod_child(1))
    # the identity case: no fill, the tree's own child
    del seen[:], fills[:]
    t2 = _level_order_tree()
    for cap in (3, 7):
        svox.VolumeRenderer(t2, max_depth=cap).render_persp(torch.eye(4), width=2, height=2, fx=2.0)
    assert fills == [] and all(v[0] is t2.child for v in seen)
    # refusals, before a launch
    del seen[:]
    t2.data.requires_grad_(True)
    capped = svox.VolumeRenderer(t2, max_depth=1)
    for call in (lambda: capped.render_persp(torch.eye(4), width=2, height=2, fx=2.0), lambda: capped.forward(rays, rays, rays),
                 lambda: capped.render_persp_aux(torch.eye(4), width=2, height=2, fx=2.0),
                 lambda: capped.forward_aux(rays, rays, rays)):
        with pytest.raises(NotImplementedError, match=r"fine-tune tree\.lod\(1\) instead"):
            call()
    t2.data.requires_grad_(False)
    with t2.accumulate_weights("max"):
        with pytest.raises(NotImplementedError, match="max_depth=1 inside accumulate_weights"):
            capped.render_persp(torch.eye(4), width=2, height=2, fx=2.0)
        with pytest.raises(NotImplementedError, match="max_depth=1 inside accumulate_weights"):
            capped.forward(rays, rays, rays)
    assert seen == [] and fills == []
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="max_depth"):
            svox.VolumeRenderer(t2, max_depth=bad)


# ---- refusals by name -----------------------------------------------------------------------------------------------------
def _cfg(tmp_path):
    path = os.path.join(str(tmp_path), "tiny.yaml")
    with open(path, "w") as f:
        f.write("dataset: synthetic\nfactor: 16\nwhite_bkgd: true\nsh_deg: 1\n")
    return path


def _saved(tmp_path):
    path = str(tmp_path / "tree.npz")
    _level_order_tree().save(path, compress=False)
    return path


def test_volume_renderer_max_depth_refuses_half_and_palette_trees(tmp_path):
    half = svox.N3Tree.load(_saved(tmp_path), keep_half=True)
    with pytest.raises(NotImplementedError, match=r"max_depth=\.\.\.\) on a HalfN3Tree.*to_float\(\)"):
        svox.VolumeRenderer(half, max_depth=1)
    quant = svox.N3Tree.load(Q.case(4, 1, 8).save(str(tmp_path / "compressed.npz")), keep_quantized=True)
    with pytest.raises(NotImplementedError, match=r"max_depth=\.\.\.\) on a QuantizedN3Tree.*dequantize\(\)"):
        svox.VolumeRenderer(quant, max_depth=1)
    svox.VolumeRenderer(half)                                            # without a cap both are taken as before
    svox.VolumeRenderer(quant, max_depth=None)


def test_lod_cli_flags_and_refusals(tmp_path):
    cfg, src = _cfg(tmp_path), _saved(tmp_path)
    a = lod.define_flags().parse_args(["--input", src, "--output_dir", "o", "--depths", "1", "2"])
    assert (a.input, a.output_dir, a.depths, a.eval, a.renderer_step_size, a.config, a.data_dir) == \
        (src, "o", [1, 2], False, 1e-4, None, None)                      # no dataset flag is needed without --eval
    lod.check_flags(a)
    assert lod.check_input(src, [0, 3]) == 3
    out = str(tmp_path / "lods")
    with pytest.raises(NotImplementedError, match="octree.lod: --render_path"):
        lod.main(["--config", cfg, "--input", src, "--output_dir", out, "--depths", "1", "--render_path", "true"])
    with pytest.raises(ValueError, match=r"--depths 4 outside \[0, 3\]"):
        lod.main(["--input", src, "--output_dir", out, "--depths", "1", "4"])
    with pytest.raises(ValueError, match=r"--depths -1 outside \[0, 3\]"):
        lod.main(["--input", src, "--output_dir", out, "--depths", "-1"])
    packed = Q.case(4, 1, 8).save(str(tmp_path / "compressed.npz"))
    with pytest.raises(NotImplementedError, match="octree.lod: .* is a compressed tree"):
        lod.main(["--input", packed, "--output_dir", out, "--depths", "1"])
    with pytest.raises(ValueError, match="--renderer_step_size"):
        lod.main(["--input", src, "--output_dir", out, "--depths", "1", "--renderer_step_size", "0"])
    assert not os.path.exists(out)                                       # refused before anything was written
    with pytest.raises(SystemExit):
        lod.define_flags().parse_args(["--input", src])                  # --depths is required


def test_evaluation_max_depth_flag_and_refusals(tmp_path):
    cfg, src = _cfg(tmp_path), _saved(tmp_path)
    a = evaluation.define_flags().parse_args(["--config", cfg])
    assert a.max_depth is None
    assert evaluation.define_flags().parse_args(["--config", cfg, "--max_depth", "2"]).max_depth == 2
    with pytest.raises(NotImplementedError, match="octree.evaluation: --max_depth together with --keep_half"):
        evaluation.main(["--config", cfg, "--input", src, "--max_depth", "2", "--keep_half"])
    with pytest.raises(NotImplementedError, match="octree.evaluation: --max_depth together with --keep_compressed"):
        evaluation.main(["--config", cfg, "--input", src, "--max_depth", "2", "--keep_compressed"])
    with pytest.raises(ValueError, match="--max_depth -1"):
        evaluation.main(["--config", cfg, "--input", src, "--max_depth", "-1"])
    # the other entry points do not grow the flag
    from plenoctree_amd.octree import extraction, optimization, pruning
    for mod in (extraction, optimization, pruning):
        with pytest.raises(SystemExit):
            mod.define_flags().parse_args(["--config", cfg, "--max_depth", "2"])


def test_eval_octree_passes_the_cap_to_the_renderer(monkeypatch):
    from plenoctree_amd.octree import extraction
    seen = []

    class Renderer:
        def __init__(self, tree, step_size, ndc, max_depth=None):
            seen.append(max_depth)

    monkeypatch.setattr(extraction, "VolumeRenderer", Renderer)
    ds = argparse.Namespace(size=0, w=4, h=4, focal=4.0)
    args = argparse.Namespace(renderer_step_size=1e-3, dataset="synthetic", spherify=False, no_early_stop=False)
    tree = _level_order_tree()
    with np.errstate(all="ignore"):
        extraction.eval_octree(tree, ds, args)
        extraction.eval_octree(tree, ds, args, max_depth=2)
    assert seen == [None, 2]
