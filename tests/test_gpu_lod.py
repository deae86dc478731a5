"""GPU tests of the level of detail of a PlenOctree: pxo_tree_lod_fill against tests/_lod_oracle.py, the capped view of
VolumeRenderer(max_depth=L) against the standalone tree N3Tree.lod(L), trees out of prune_ / refine_leaves, staleness after
edits, and the octree.lod command line.

Bounds of the fill (derived in tests/_lod_oracle.py, fixed before any GPU run): every row the device wrote for a node is
compared with the float64 value computed from the DEVICE's own eight rows of that node, so rounding does not compound over the
levels; a coefficient may be off by 16 * 2^-24 * (sum w_j |c_j[k]|) / S + 2^-126, sigma by 8 * 2^-24 * S / 8.  On top of the
bounds every row must equal a float32 numpy twin of the definition bit for bit (IEEE operations in a fixed order have one
result; first run on the MI355X: all rows equal, the worst error 0.32 of its bound).  Everything about rendering is torch.equal: a capped view and
the standalone tree of the same level hold the same rows behind the same pointers, so the same launches give the same bits."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

import _lod_oracle as L
import _octree_cases as C
import _octree_ndc_oracle as N
from _helpers import _gpu
from oracle import octree_oracle as T

pytestmark = pytest.mark.gpu
f32 = np.float32
STEP = 1e-3
LANES = (4, 8, 16)
VIEW = dict(c2w=C.look_at((3.4, 3.1, 2.6)), W=24, H=20, fx=17.0, fy=18.5)
N_RAYS = 300
FIXTURES = [(family, depth, K) for family in C.FAMILIES for depth in (3, 4) for K in (1, 9, 16)] + [("sg4", 4, 4)]


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _svox():
    from plenoctree_amd.octree import svox
    return svox


@pytest.fixture(autouse=True)
def _default_lanes():
    yield
    _oops().set_lanes_per_ray(0, 0)


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def _sg_lobes(K):
    rs = np.random.RandomState(17)
    mu = rs.randn(K, 3)
    mu /= np.linalg.norm(mu, axis=1, keepdims=True)
    return np.concatenate([1.0 + 4.0 * rs.rand(K, 1), mu], 1).astype(f32)


@functools.lru_cache(maxsize=None)
def _case(family, depth, K):
    """A copy of the shared case tree (make_tree's is cached and stays as it is) in which one deepest node has no density at
    all: its value is the S == 0 branch.  fill_data wrote random numbers into EVERY row, so the rows of cells that have a
    child start as garbage the fill has to overwrite, and 35 % of the sigmas are negative."""
    t = copy.deepcopy(C.make_tree("shell" if family == "sg4" else family, depth, K))
    deepest = np.nonzero(t.parent_depth[:, 1] == t.parent_depth[:, 1].max())[0]
    assert int(t.parent_depth[:, 1].max()) == depth and not t.child[deepest].any()
    t.data[deepest[0], ..., -1] = -np.abs(t.data[deepest[0], ..., -1]) - f32(0.25)
    return t


def _svox_tree(t, dev, sg=False):
    """The oracle tree `t` as an svox N3Tree on `dev`, float32 data as they are, not requiring grad."""
    svox = _svox()
    K = (t.data_dim - 1) // 3
    z = {"data_dim": t.data_dim, "child": t.child, "parent_depth": t.parent_depth, "n_internal": t.n_internal,
         "invradius3": t.invradius, "offset": t.offset, "depth_limit": t.depth_limit, "data": t.data,
         "data_format": f"SG{K}" if sg else f"SH{K}"}
    if sg:
        z["extra_data"] = _sg_lobes(K)
    tree = svox.N3Tree._from_npz(svox._NpzDict({k: np.asarray(v) for k, v in z.items()}), dev)
    tree.data.requires_grad_(False)
    return tree


@functools.lru_cache(maxsize=None)
def _rays():
    """300 unit rays from a sphere around the volume towards random points inside it (world box of _octree_cases)."""
    rs = np.random.RandomState(5)
    v = rs.randn(N_RAYS, 3)
    o = np.array(C.CENTER) + 5.0 * v / np.linalg.norm(v, axis=1, keepdims=True)
    target = np.array(C.CENTER) + (rs.rand(N_RAYS, 3) - 0.5) * 1.8 * np.array(C.RADIUS)
    d = target - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    return o.astype(f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def _renders(r, dev, aux=True, view=VIEW, rays=None):
    """Every output of renderer `r` the capped view has to reproduce: the image (exact march), the explicit rays (early-stop
    preset) and, on SH trees in world space, both aux calls."""
    o, d = (torch.from_numpy(a).to(dev) for a in (rays or _rays()))
    c2w = torch.from_numpy(view["c2w"])
    cam = dict(width=view["W"], height=view["H"], fx=view["fx"], fy=view.get("fy"))
    with torch.no_grad():
        out = {"persp": r.render_persp(c2w, **cam), "rays": r.forward(o, d, d, fast=True)}
        if aux:
            for k, v in r.render_persp_aux(c2w, fast=True, **cam).items():
                out["persp_aux." + k] = v
            for k, v in r.forward_aux(o, d, d, surface_thresh=0.3).items():
                out["rays_aux." + k] = v
    return out


def _same(name, a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), f"{name}: {k} differs in " \
            f"{int((a[k] != b[k]).sum())} of {a[k].numel()} values"


def _check_fill(name, tree):
    """Check 1 on a filled tree: every node of depth >= 1 against the float64 value of its own device rows."""
    D = tree.data_dim
    child, pd = tree.child.cpu().numpy().reshape(-1), tree.parent_depth.cpu().numpy()
    rows32 = tree.data.data.cpu().numpy().reshape(-1, 8, D)
    flat32 = rows32.reshape(-1, D)
    worst, empty, twin_equal = 0.0, 0, 0
    for n in range(1, tree.n_internal):
        p = int(pd[n, 0])
        assert child[p] != 0 and p // 8 + child[p] == n
        want, bound = L.node_value(rows32[n]), L.node_bound(rows32[n])
        err = np.abs(flat32[p].astype(np.float64) - want)
        assert np.isfinite(flat32[p]).all() and (err <= bound).all(), \
            f"{name}: node {n} (depth {pd[n, 1]}) row off by {err.max():.3g}, bound {bound[err.argmax()]:.3g}"
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        empty += not (rows32[n, :, -1] > 0).any()
        if not (rows32[n, :, -1] > 0).any():
            assert not flat32[p].any()                                   # S == 0: an all-zero row
        twin_equal += np.array_equal(flat32[p].view(np.uint32), _twin32(rows32[n]).view(np.uint32))
    print(f"{name}: {tree.n_internal - 1} filled rows, worst err / bound {worst:.3f}, {empty} nodes with S == 0, "
          f"{twin_equal} rows bit-equal to the float32 twin")
    # stricter than the bounds, and what the definition says: IEEE operations in a fixed order have one result
    assert twin_equal == tree.n_internal - 1, f"{name}: {tree.n_internal - 1 - twin_equal} rows differ from the float32 twin"
    return empty


def _twin32(rows):
    """The definition in numpy float32, operation by operation."""
    w = np.maximum(rows[:, -1], f32(0))
    S = f32(w[0] + w[1])
    for j in range(2, 8):
        S = f32(S + w[j])
    out = np.zeros(rows.shape[1], f32)
    out[-1] = f32(S * f32(0.125))
    if S > 0:
        acc = (w[0] * rows[0, :-1]).astype(f32)
        for j in range(1, 8):
            acc = (acc + (w[j] * rows[j, :-1]).astype(f32)).astype(f32)
        with np.errstate(all="ignore"):
            out[:-1] = (acc / S).astype(f32)
    return out


def _check_capped_equals_standalone(name, tree, dev, aux, lanes=LANES, **render_kw):
    """Check 2 on `tree`: for every lane count and every L the capped view renders what tree.lod(L) renders; L = max_depth is
    the uncapped render as well, L = 0 the 8-cell tree of the root's rows; below max_depth the image differs from the full."""
    svox, oops = _svox(), _oops()
    ndc = render_kw.pop("ndc", None)
    make = lambda tr, **kw: svox.VolumeRenderer(tr, step_size=STEP, ndc=ndc, **kw)
    depth = tree.parent_depth[:, 1]
    for lanes_per_ray in lanes:
        oops.set_lanes_per_ray(lanes_per_ray, 0)
        full = _renders(make(tree), dev, aux, **render_kw)
        for lvl in range(tree.max_depth + 1):
            capped = _renders(make(tree, max_depth=lvl), dev, aux, **render_kw)
            level = tree.lod(lvl)
            assert level.n_internal == sum(tree.level_nodes[:lvl + 1]) and level.max_depth == lvl
            _same(f"{name} lanes {lanes_per_ray} L {lvl}", capped, _renders(make(level), dev, aux, **render_kw))
            if lvl == tree.max_depth:
                _same(f"{name} lanes {lanes_per_ray} L = max_depth", capped, full)
            else:
                assert bool((tree.child[depth == lvl] != 0).any()), f"{name}: no node of depth {lvl} has a child"
                assert not torch.equal(capped["persp"], full["persp"]), f"{name}: level {lvl} renders the full image"
            if lvl == 0:
                assert level.n_internal == 1 and not bool(level.child.any())
                assert torch.equal(level.data.data[0], tree.data.data[0])
    # a cap above the tree's depth is no cap
    _same(f"{name} cap above the depth", _renders(make(tree, max_depth=tree.max_depth + 3), dev, aux, **render_kw), full)


# ---- 1 + 2: every fixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,depth,K", FIXTURES)
def test_fill_and_capped_view(family, depth, K):
    svox = _svox(); dev = _gpu()
    sg = family == "sg4"
    t = _case(family, depth, K)
    name = f"{family} depth {depth} K {K}"
    assert (t.data[..., -1][t.child == 0] < 0).any()                     # some leaves have negative sigma
    tree = _svox_tree(t, dev, sg)
    assert tree.max_depth == depth and not tree._lod_filled
    before = tree.data.data.clone()
    leaf = tree.child == 0
    r = svox.VolumeRenderer(tree, step_size=STEP)
    full_before = _renders(r, dev, aux=not sg)
    assert tree.fill_internal_() is tree and tree._lod_filled
    assert torch.equal(tree.data.data[leaf], before[leaf])               # leaf rows are never written
    assert not torch.equal(tree.data.data[~leaf], before[~leaf])         # the garbage rows were
    _same(f"{name} uncapped render after the fill", _renders(r, dev, aux=not sg), full_before)
    assert _check_fill(name, tree) >= 1                                  # the emptied node took the S == 0 branch
    # the fill is idempotent: a second pass reads the same leaf rows and the rows it wrote itself
    filled = tree.data.data.clone()
    tree.fill_internal_()
    assert torch.equal(tree.data.data, filled)
    _check_capped_equals_standalone(name, tree, dev, aux=not sg)


def test_fill_widest_rows():
    """K = 25 (76 floats per row, more than a wave): the one width the fixtures do not have."""
    dev = _gpu()
    tree = _svox_tree(_case("chunked", 3, 25), dev)
    tree.fill_internal_()
    assert _check_fill("chunked depth 3 K 25", tree) >= 1


def test_ndc_capped_view():
    """A tree in the NDC cube (tests/test_gpu_octree_ndc.py's set-up): render_persp and forward with ndc=..."""
    svox = _svox(); dev = _gpu()
    tree = _svox_tree(N.box_tree(4, 1, depth=3, seed=77, p=0.2), dev)
    view = dict(c2w=N.camera_b(), W=N.W, H=N.H, fx=N.FX)
    _check_capped_equals_standalone("ndc", tree, dev, aux=False, ndc=svox.NDCConfig(N.W, N.H, N.FX), view=view,
                                    rays=T.camera_rays(N.camera_b(), N.W, N.H, N.FX))
    _check_fill("ndc", tree)


# ---- 3: trees out of the other tools --------------------------------------------------------------------------------------
def test_pruned_and_collapsed_tree():
    dev = _gpu()
    tree = _svox_tree(_case("shell", 4, 9), dev)
    keep = torch.from_numpy(np.random.RandomState(4).rand(tree.n_internal, 2, 2, 2) < 0.3).to(dev)
    removed = tree.prune_(keep, collapse=True)
    assert removed > 0 and tree.max_depth == 4 and not tree._lod_filled
    tree.fill_internal_()
    _check_fill("collapsed", tree)
    _check_capped_equals_standalone("collapsed", tree, dev, aux=True, lanes=(4,))


def test_refined_tree_not_in_level_order():
    dev = _gpu()
    tree = _svox_tree(_case("shell", 4, 1), dev)
    tree.depth_limit = 5
    shallow = (tree.child == 0) & (tree.parent_depth[:, 1] <= 1)[:, None, None, None]
    deep = (tree.child == 0) & (tree.parent_depth[:, 1] == 4)[:, None, None, None]
    deep.view(-1)[1::2] = False                                          # every second leaf of the deepest level
    n0, added = tree.n_internal, int(shallow.sum()) + int(deep.sum())
    assert tree.refine_leaves(shallow | deep) == added and not tree._level_order and tree.max_depth == 5
    assert bool((tree.parent_depth[1:, 1] < tree.parent_depth[:-1, 1]).any())
    # the new cells inherited their parent's row, and a node of eight equal rows has (nearly) its cells' value: give them rows
    # of their own, written past the class as an optimizer would, before the fill
    rs = np.random.RandomState(21)
    rows = (rs.randn(added, 2, 2, 2, tree.data_dim) * 0.7).astype(f32)
    rows[..., -1] = (rs.rand(added, 2, 2, 2) - 0.35) * 0.12 * 2.0 ** (tree.parent_depth[n0:, 1].cpu().numpy()[:, None, None, None] + 1)
    tree.data.data[n0:] = torch.from_numpy(rows).to(dev)
    tree.fill_internal_()
    _check_fill("refined", tree)
    _check_capped_equals_standalone("refined", tree, dev, aux=True, lanes=(4,))
    level = tree.lod(2)
    assert L.valid_tree(level.child.cpu().numpy(), level.parent_depth.cpu().numpy())
    want = L.lod(tree.child.cpu().numpy(), tree.parent_depth.cpu().numpy(), tree.data.data.cpu().numpy(), 2)
    for got, ref in zip((level.child, level.parent_depth, level.data.data), want):
        assert np.array_equal(got.cpu().numpy(), ref)


# ---- 4: staleness and refusals --------------------------------------------------------------------------------------------
def test_a_stale_pyramid_is_never_rendered():
    svox = _svox(); dev = _gpu()
    tree = _svox_tree(_case("chunked", 4, 9), dev)
    lvl = 2
    r = svox.VolumeRenderer(tree, step_size=STEP, max_depth=lvl)
    first = _renders(r, dev)
    assert tree._lod_filled

    def fresh_level():
        """lod(L) of a copy whose pyramid is rebuilt from its leaves, whatever the copy's unused rows held."""
        other = tree.clone()
        other._lod_filled = False
        return svox.VolumeRenderer(other.lod(lvl), step_size=STEP)

    rs = np.random.RandomState(9)
    new = (rs.randn(tree.n_internal * 8, tree.data_dim) * 0.6).astype(f32)
    new[:, -1] = (rs.rand(tree.n_internal * 8) - 0.3) * 6.0
    tree[:] = torch.from_numpy(new).to(dev)
    assert not tree._lod_filled
    second = _renders(r, dev)
    assert tree._lod_filled                                              # the render refilled
    _same("after tree[:] = ...", second, _renders(fresh_level(), dev))
    assert not torch.equal(second["persp"], first["persp"])
    tree.relu_sigma_()
    assert not tree._lod_filled and not bool((tree.data.data[..., -1] < 0).any())
    third = _renders(r, dev)
    assert tree._lod_filled
    _same("after relu_sigma_", third, _renders(fresh_level(), dev))
    # a structure edit: the capped child array is rebuilt as well
    added = tree.refine_leaves((tree.child == 0) & (tree.parent_depth[:, 1] == 1)[:, None, None, None])
    assert added > 0
    _same("after refine_leaves", _renders(r, dev), _renders(fresh_level(), dev))
    _check_fill("after the edits", tree)


def test_refusals_by_name_before_a_launch(tmp_path):
    svox = _svox(); dev = _gpu()
    tree = _svox_tree(_case("shell", 3, 1), dev)
    path = str(tmp_path / "tree.npz")
    tree.save(path, compress=False)
    with pytest.raises(NotImplementedError, match="on a HalfN3Tree"):
        svox.VolumeRenderer(svox.N3Tree.load(path, map_location=dev, keep_half=True), max_depth=1)
    from plenoctree_amd.octree import compression
    import argparse
    packed = str(tmp_path / "tree_min.npz")
    compression.compress_file(path, packed, argparse.Namespace(noquant=False, bits=4, sigma_thresh=0.0, retain=0, weighted=False))
    with pytest.raises(NotImplementedError, match="on a QuantizedN3Tree"):
        svox.VolumeRenderer(svox.N3Tree.load(packed, map_location=dev, keep_quantized=True), max_depth=1)
    r = svox.VolumeRenderer(tree, step_size=STEP, max_depth=1)
    o, d = (torch.from_numpy(a).to(dev) for a in _rays())
    c2w = torch.from_numpy(VIEW["c2w"])
    before = tree.data.data.clone()
    tree.data.requires_grad_(True)
    for call in (lambda: r.render_persp(c2w, width=8, height=6, fx=7.0), lambda: r.forward(o, d, d),
                 lambda: r.render_persp_aux(c2w, width=8, height=6, fx=7.0), lambda: r.forward_aux(o, d, d)):
        with pytest.raises(NotImplementedError, match=r"fine-tune tree\.lod\(1\) instead"):
            call()
    tree.data.requires_grad_(False)
    with torch.no_grad(), tree.accumulate_weights("max") as accum:
        with pytest.raises(NotImplementedError, match="inside accumulate_weights"):
            r.render_persp(c2w, width=8, height=6, fx=7.0)
        with pytest.raises(NotImplementedError, match="inside accumulate_weights"):
            r.forward(o, d, d)
        assert not bool(accum.value.any())
    assert not tree._lod_filled and torch.equal(tree.data.data, before)  # nothing was launched, not even the fill
    tree.data.requires_grad_(True)
    with torch.no_grad():                                                # the same tree under no_grad renders
        assert r.render_persp(c2w, width=8, height=6, fx=7.0).shape == (6, 8, 3)


# ---- 5: the command line --------------------------------------------------------------------------------------------------
def test_lod_cli_pipeline(tmp_path):
    svox = _svox(); dev = _gpu()
    from plenoctree_amd.octree import lod
    from plenoctree_amd.octree.pruning import tree_stats
    src = str(tmp_path / "tree_opt.npz")
    _svox_tree(_case("chunked", 4, 16), dev).save(src, compress=False)
    out = str(tmp_path / "lods")
    table = lod.main(["--input", src, "--output_dir", out, "--depths", "1", "3", "4"])
    with open(os.path.join(out, "lod.json")) as f:
        assert json.load(f) == table
    source = svox.N3Tree.load(src, map_location=dev)
    source.data.requires_grad_(False)
    assert [row["name"] for row in table] == ["source", "d1", "d3", "d4"]
    assert (table[0]["nodes"], table[0]["leaves"], table[0]["float32_bytes"]) == tree_stats(source)
    assert table[0]["file_bytes"] == os.path.getsize(src)
    for row, lvl in zip(table[1:], (1, 3, 4)):
        path = os.path.join(out, f"tree_opt_d{lvl}.npz")
        assert row["path"] == path and row["file_bytes"] == os.path.getsize(path)
        assert row["nodes"] == sum(source.level_nodes[:lvl + 1]) and row["leaves"] == 7 * row["nodes"] + 1
        got = svox.N3Tree.load(path, map_location=dev)
        got.data.requires_grad_(False)
        half = svox.N3Tree.load(path, map_location=dev, keep_half=True)
        want = source.lod(lvl)
        with torch.no_grad():
            want.data.copy_(want.data.data.half().float())               # what save does to the rows
        assert torch.equal(got.child, want.child) and torch.equal(got.parent_depth, want.parent_depth)
        assert torch.equal(got.data.data, want.data.data) and got.level_nodes == want.level_nodes
        ref = _renders(svox.VolumeRenderer(want, step_size=STEP), dev)
        _same(f"octree.lod d{lvl} float", _renders(svox.VolumeRenderer(got, step_size=STEP), dev), ref)
        _same(f"octree.lod d{lvl} half", _renders(svox.VolumeRenderer(half, step_size=STEP), dev), ref)
    assert table[1]["float32_bytes"] < table[2]["float32_bytes"] < table[3]["float32_bytes"] == table[0]["float32_bytes"]


# ---- a tree whose rows lie past 2^31 floats ---------------------------------------------------------------------------------
def test_fill_past_2_31_floats():
    """3.7 M nodes of 8 x 76 floats: 2.2e9 floats, so the rows of the last nodes and of their parents' cells start beyond
    2^31 elements (9 GB of data).  The nodes with the highest indices and those whose parent row lies past 2^31 are held to
    the bounds, here by a float64 restatement in torch on the device (the numpy oracle would walk 3.6 M nodes)."""
    svox = _svox(); dev = _gpu()
    D = 76
    tree = svox.N3Tree(N=2, data_dim=D, data_format="SH25", depth_limit=10, device=dev)
    tree.data.requires_grad_(False)
    tree[:].refine(repeats=7)                                            # complete to depth 7: 2,396,745 nodes
    first_deep = tree.n_internal - tree.level_nodes[-1]
    leaves = tree._leaf_packed()
    pick = leaves[(leaves >> 3) >= first_deep][-1_250_000:]              # the last depth-7 nodes' cells: high row indices
    assert tree._refine_packed(pick) == 1_250_000
    # and the cells of the last 5,000 of those: 40,000 nodes of depth 9 whose PARENT rows (the writes) lie past 2^31 as well
    assert tree._refine_packed(torch.arange((tree.n_internal - 5000) * 8, tree.n_internal * 8, device=dev)) == 40_000
    n = tree.n_internal
    assert n * 8 * D > 2 ** 31 and tree.max_depth == 9
    data = tree.data.data
    gen = torch.Generator(device=dev).manual_seed(3)
    for a in range(0, n, 1 << 18):                                       # random rows, a third of the sigmas negative
        b = min(n, a + (1 << 18))
        data[a:b] = torch.randn(b - a, 2, 2, 2, D, device=dev, generator=gen) * 0.7
        data[a:b, ..., -1] = (torch.rand(b - a, 2, 2, 2, device=dev, generator=gen) - 0.33) * 5.0
    leaf = tree.child == 0
    sample = torch.nonzero(leaf.view(-1))[:: 4099].reshape(-1)
    before = data.view(-1, D)[sample].clone()
    tree.fill_internal_()
    torch.cuda.synchronize()
    assert torch.equal(data.view(-1, D)[sample], before)
    parent_cell = tree.parent_depth[:, 0].long()
    past = torch.nonzero(parent_cell * D >= 2 ** 31).reshape(-1)
    assert past.numel() > 1000
    nodes = torch.unique(torch.cat([past[:: max(1, past.numel() // 20000)], torch.arange(n - 20000, n, device=dev),
                                    torch.arange(1, 20000, device=dev)]))
    rows = data.view(-1, 8, D)[nodes].double()
    w = rows[..., -1].clamp_min(0.0)
    S = w.sum(1)
    want = torch.zeros(nodes.numel(), D, dtype=torch.float64, device=dev)
    want[:, -1] = S * 0.125
    pos = S > 0
    want[pos, :-1] = (w[pos][:, :, None] * rows[pos][:, :, :-1]).sum(1) / S[pos][:, None]
    bound = torch.full_like(want, 2.0 ** -126)
    bound[pos, :-1] += 16 * 2.0 ** -24 * (w[pos][:, :, None] * rows[pos][:, :, :-1].abs()).sum(1) / S[pos][:, None]
    bound[:, -1] = 8 * 2.0 ** -24 * S / 8
    got = data.view(-1, D)[parent_cell[nodes]].double()
    err = (got - want).abs()
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements outside the bound, worst {float(err.max()):.3g}"
    print(f"{n} nodes, {past.numel()} parent rows past 2^31 floats, {nodes.numel()} nodes checked, "
          f"worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
