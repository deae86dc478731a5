"""GPU tests of the footprint render (VolumeRenderer(lod_pixels=...), pxo_octree_render_foot_fwd / _foot_aux_fwd; the
definition: include/plenoctree_octree.h, "footprint") on the fixtures of tests/test_gpu_lod.py -- copies of the shared case trees
in which EVERY row is random, so a sample that reads a row nothing filled, or a fine row under a cap, shows.

What pins the kernel, in this order: a cap that never binds is the existing render bit for bit; a constant cap is the capped view
of VolumeRenderer(max_depth=L) and the standalone tree.lod(L) bit for bit; a cap that varies along the rays is held to the numpy
twin (oracle/octree_oracle.py's march with a footprint), which descends from the root for every sample and so cannot share the kernel's path-reuse trap.
The twin is given the DEVICE's filled rows, so the rounding of the fill plays no part.  Bounds of the third check (fixed before
any GPU run): rgb rtol 0, atol 2e-5, what tests/test_gpu_octree.py holds the uncapped forward to, for the same reason -- the
steps are identical, only exp, sigmoid and the order of the K-term sums differ; alpha atol 2e-5, depth atol 2e-5 s_max, surface
rtol 1e-6 leaving out at most 2 % of the rays (tests/test_gpu_octree_aux.py's bounds and exclusion rule).

So that the third check cannot pass empty, the twin's counters must all be > 0 on every fixture and both ray sets: samples the
cap stopped at a cell that has a child, clamp cases of the path reuse, rays whose cap changes.  They are > 0 at depth 3 as well
(tests/test_footprint_cpu.py pins the figures of three fixtures), so no fixture is left out."""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

import _footprint_oracle as F
import _octree_cases as C
import test_gpu_lod as LOD
from _helpers import _gpu, close
from oracle import octree_oracle as T

pytestmark = pytest.mark.gpu
f32 = np.float32
STEP, LANES, VIEW = LOD.STEP, LOD.LANES, LOD.VIEW
FMAX = max(VIEW["fx"], VIEW["fy"])
CAM = dict(width=VIEW["W"], height=VIEW["H"], fx=VIEW["fx"], fy=VIEW["fy"])
GEOMETRIES = [(family, depth) for family in C.FAMILIES for depth in (3, 4)] + [("chunked", 6)]
FIXTURES = [(family, depth, K) for family, depth in GEOMETRIES for K in (1, 9, 16, 25)] + [("sg4", 4, 4)]
# cone 0.1 both ways: explicit rays 2 pixels x 0.05 rad, the camera 1.85 pixels / max(fx, fy) = 18.5
VARYING = dict(lod_pixels=1.85, pixel_angle=0.1 / 1.85)
SURFACE = 0.5


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


def _tree(family, depth, K, dev):
    return LOD._svox_tree(LOD._case(family, depth, K), dev, sg=family == "sg4")


def _renders(r, dev, aux, pixel_angle, fast=(False, True)):
    """Every output of renderer `r`: image and explicit rays, `fast` both ways, and on SH trees both aux calls.  pixel_angle is
    handed to the plain renderers too: without lod_pixels it is not looked at."""
    o, d = (torch.from_numpy(a).to(dev) for a in LOD._rays())
    c2w = torch.from_numpy(VIEW["c2w"])
    out = {}
    with torch.no_grad():
        for fa in fast:
            out[f"persp.{fa}"] = r.render_persp(c2w, fast=fa, **CAM)
            out[f"rays.{fa}"] = r.forward(o, d, d, fast=fa, pixel_angle=pixel_angle)
            if aux:
                for k, v in r.render_persp_aux(c2w, fast=fa, surface_thresh=SURFACE, **CAM).items():
                    out[f"persp_aux.{fa}.{k}"] = v
                for k, v in r.forward_aux(o, d, d, fast=fa, surface_thresh=SURFACE, pixel_angle=pixel_angle).items():
                    out[f"rays_aux.{fa}.{k}"] = v
    return out


def _make(tree, **kw):
    return _svox().VolumeRenderer(tree, step_size=STEP, **kw)


# ---- 1: a cap that never binds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,depth,K", FIXTURES)
def test_cap_that_never_binds_is_the_plain_render(family, depth, K):
    dev = _gpu()
    tree = _tree(family, depth, K, dev)
    aux = family != "sg4"
    name = f"{family} depth {depth} K {K}"
    tiny = dict(lod_pixels=FMAX * 2.0 ** -40, pixel_angle=1.0 / FMAX)    # cone 2^-40 both ways: f stays far below 2^-11
    for lanes in LANES:
        _oops().set_lanes_per_ray(lanes, 0)
        plain = _renders(_make(tree), dev, aux, 1.0)
        r = _make(tree, lod_pixels=tiny["lod_pixels"])
        LOD._same(f"{name} lanes {lanes} cone 2^-40", _renders(r, dev, aux, tiny["pixel_angle"]), plain)
        assert tree._lod_filled                                          # the footprint render filled the tree on the way
        for lod_pixels, angle in ((VARYING["lod_pixels"], VARYING["pixel_angle"]), (1e9 * FMAX, 1.0 / FMAX)):
            r = _make(tree, lod_pixels=lod_pixels, lod_min_depth=tree.max_depth)
            LOD._same(f"{name} lanes {lanes} lod_pixels {lod_pixels:g} held at max_depth", _renders(r, dev, aux, angle), plain)


# ---- 2: a constant cap -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,depth,K", FIXTURES)
def test_constant_cap_is_the_capped_view(family, depth, K):
    dev = _gpu()
    tree = _tree(family, depth, K, dev)
    aux = family != "sg4"
    name = f"{family} depth {depth} K {K}"
    huge = dict(lod_pixels=1e9 * FMAX, pixel_angle=1.0 / FMAX)           # cone 1e9 both ways: f >= 0.5 at every sample
    tree.fill_internal_()
    levels = {lvl: tree.lod(lvl) for lvl in range(tree.max_depth + 1)}
    for lanes in LANES:
        _oops().set_lanes_per_ray(lanes, 0)
        for lvl in range(tree.max_depth + 1):
            got = _renders(_make(tree, lod_pixels=huge["lod_pixels"], lod_min_depth=lvl), dev, aux, huge["pixel_angle"])
            LOD._same(f"{name} lanes {lanes} L {lvl} against max_depth=L", got, _renders(_make(tree, max_depth=lvl), dev, aux, 1.0))
            LOD._same(f"{name} lanes {lanes} L {lvl} against tree.lod(L)", got, _renders(_make(levels[lvl]), dev, aux, 1.0))


# ---- 3: the varying cap against the twin -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ray_sets():
    co, cd = T.camera_rays(**VIEW)
    return {"rays": LOD._rays(), "persp": (co.astype(f32), cd.astype(f32))}


def _cone(which):
    """The cone exactly as VolumeRenderer forms it, in Python floats; the entry point takes it as a float32."""
    return VARYING["lod_pixels"] * VARYING["pixel_angle"] if which == "rays" else VARYING["lod_pixels"] / FMAX


def _march_all(child, offset, invradius, which, min_depth=0):
    o, d = _ray_sets()[which]
    return [T.march((child, offset, invradius), o[i], d[i], STEP, foot=(_cone(which), min_depth)) for i in range(o.shape[0])]


@functools.lru_cache(maxsize=None)
def _fixture_marches(family, depth, which):
    """The march does not read the data: one per geometry and ray set, shared by the formats."""
    t = LOD._case("shell" if family == "sg4" else family, depth, 1)
    return _march_all(t.child, t.offset, t.invradius, which)


def _bases(which, K, lobes):
    _, d = _ray_sets()[which]
    return [T.sh_basis_np(K, v) if lobes is None else T.sg_basis_np(lobes, v) for v in d]


def _check_against_twin(name, got, data, marches_of, K, lobes, aux, min_surface=0):
    """`got`: _renders of a footprint renderer; data: the device's filled rows [n_cells, D] as numpy; marches_of(which)."""
    for which in ("rays", "persp"):
        marches = marches_of(which)
        counts = F.case_counts(marches)
        assert all(v > 0 for v in counts.values()), f"{name} {which}: the case is empty somewhere: {counts}"
        bases = _bases(which, K, lobes)
        for fast in (False, True):
            b32, b64 = T.composite_batches(data, marches, bases, T.RenderOptions.for_renderer(STEP, fast), SURFACE)
            what = f"{name} {which} fast={fast}"
            rgb = got[f"{which}.{fast}"].reshape(-1, 3)
            print(f"{what}: max |rgb - twin| {np.abs(rgb.cpu().numpy() - b32.rgb).max():.3g} (bound 2e-5), {counts}")
            close(f"{what} rgb", rgb, torch.from_numpy(b32.rgb), rtol=0, atol=2e-5)
            if not aux:
                continue
            assert torch.equal(got[f"{which}_aux.{fast}.rgb"].reshape(-1, 3), rgb), what
            alpha, depth, surface = (got[f"{which}_aux.{fast}.{k}"].reshape(-1).cpu().numpy() for k in ("alpha", "depth", "surface"))
            close(f"{what} alpha", torch.from_numpy(alpha), torch.from_numpy(b32.aux[:, 0]), rtol=0, atol=2e-5)
            close(f"{what} depth", torch.from_numpy(depth), torch.from_numpy(b32.aux[:, 1]), rtol=0, atol=2e-5 * b32.s_max)
            left_out = T.surface_excluded(b32, b64, SURFACE)
            assert left_out.mean() <= 0.02, what
            want = b32.aux[:, 2]
            inf = np.isinf(want)
            assert np.array_equal(np.isinf(surface[~left_out]), inf[~left_out]) and not np.isnan(surface).any(), what
            cmp = ~left_out & ~inf
            # few rays lose half their light in these sparse trees (4 of the 169 camera rays that meet shell depth 3, none in the
            # nearly transparent rods): the comparison must not be empty where the caller says it cannot be
            print(f"{what}: {int(cmp.sum())} finite surface distances compared, {int(left_out.sum())} rays left out")
            assert cmp.sum() >= (min_surface if which == "rays" else 0), what
            assert np.allclose(surface[cmp], want[cmp], rtol=1e-6, atol=0), (what, np.abs(surface[cmp] / want[cmp] - 1).max())


@pytest.mark.parametrize("family,depth,K", FIXTURES)
def test_varying_cap_matches_the_twin(family, depth, K):
    dev = _gpu()
    tree = _tree(family, depth, K, dev)
    sg = family == "sg4"
    name = f"{family} depth {depth} K {K}"
    r = _make(tree, lod_pixels=VARYING["lod_pixels"])
    by_lanes = {}
    for lanes in LANES:
        _oops().set_lanes_per_ray(lanes, 0)
        by_lanes[lanes] = _renders(r, dev, not sg, VARYING["pixel_angle"])
    assert tree._lod_filled
    data = tree.data.data.cpu().numpy().reshape(-1, tree.data_dim)       # the device's own filled rows
    lobes = LOD._sg_lobes(K) if sg else None
    for lanes in LANES:
        _check_against_twin(f"{name} lanes {lanes}", by_lanes[lanes], data, lambda w: _fixture_marches(family, depth, w), K, lobes,
                            aux=not sg, min_surface=0 if family == "rod" else 1)
    # neither the full render nor any one level
    _oops().set_lanes_per_ray(0, 0)
    got = by_lanes[4]
    others = [_renders(_make(tree), dev, False, 1.0)] + \
             [_renders(_make(tree, max_depth=lvl), dev, False, 1.0) for lvl in range(tree.max_depth)]
    for i, other in enumerate(others):
        for k in other:
            assert not torch.equal(got[k], other[k]), f"{name}: {k} is the {'full render' if i == 0 else f'level {i - 1}'}"


# ---- 4: composition and staleness --------------------------------------------------------------------------------------------
def _twin_of(tree):
    """marches_of(which) and the rows of a device tree as it stands (any node order)."""
    child = tree.child.cpu().numpy()
    offset, invradius = tree.offset.numpy().astype(f32), tree.invradius.numpy().astype(f32)
    cache = {}
    marches_of = lambda which: cache.setdefault(which, _march_all(child, offset, invradius, which))
    return marches_of, tree.data.data.cpu().numpy().reshape(-1, tree.data_dim)


def test_composes_with_max_depth():
    dev = _gpu()
    tree = _tree("chunked", 4, 9, dev)
    for lanes in LANES:
        _oops().set_lanes_per_ray(lanes, 0)
        for lvl in (1, 2, 3, 4, 7):
            both = _make(tree, max_depth=lvl, lod_pixels=VARYING["lod_pixels"], lod_min_depth=1)
            level = tree.lod(min(lvl, tree.max_depth))
            alone = _make(level, lod_pixels=VARYING["lod_pixels"], lod_min_depth=1)
            LOD._same(f"lanes {lanes} max_depth {lvl} with lod_pixels", _renders(both, dev, True, VARYING["pixel_angle"]),
                      _renders(alone, dev, True, VARYING["pixel_angle"]))


def test_pruned_and_refined_trees_match_the_twin():
    dev = _gpu()
    tree = _tree("shell", 4, 9, dev)
    keep = torch.from_numpy(np.random.RandomState(4).rand(tree.n_internal, 2, 2, 2) < 0.3).to(dev)
    assert tree.prune_(keep, collapse=True) > 0 and tree.max_depth == 4 and not tree._lod_filled
    r = _make(tree, lod_pixels=VARYING["lod_pixels"])
    got = _renders(r, dev, True, VARYING["pixel_angle"])
    assert tree._lod_filled
    marches_of, data = _twin_of(tree)
    _check_against_twin("collapsed", got, data, marches_of, 9, None, aux=True)
    # refine_leaves: the new nodes are appended, so the tree is no longer in level order
    tree = _tree("shell", 4, 1, dev)
    tree.depth_limit = 5
    shallow = (tree.child == 0) & (tree.parent_depth[:, 1] <= 1)[:, None, None, None]
    deep = (tree.child == 0) & (tree.parent_depth[:, 1] == 4)[:, None, None, None]
    deep.view(-1)[1::2] = False
    n0 = tree.n_internal
    assert tree.refine_leaves(shallow | deep) > 0 and not tree._level_order and tree.max_depth == 5
    rs = np.random.RandomState(21)
    rows = (rs.randn(tree.n_internal - n0, 2, 2, 2, tree.data_dim) * 0.7).astype(f32)
    rows[..., -1] = (rs.rand(tree.n_internal - n0, 2, 2, 2) - 0.35) * 0.12 * 2.0 ** (tree.parent_depth[n0:, 1].cpu().numpy()[:, None, None, None] + 1)
    tree.data.data[n0:] = torch.from_numpy(rows).to(dev)                 # written past the class: the mark is already clear
    assert not tree._lod_filled
    got = _renders(_make(tree, lod_pixels=VARYING["lod_pixels"]), dev, True, VARYING["pixel_angle"])
    marches_of, data = _twin_of(tree)
    _check_against_twin("refined", got, data, marches_of, 1, None, aux=True)


def test_a_stale_pyramid_is_never_rendered():
    svox = _svox(); dev = _gpu()
    tree = _tree("chunked", 4, 9, dev)
    r = _make(tree, lod_pixels=VARYING["lod_pixels"])
    first = _renders(r, dev, True, VARYING["pixel_angle"])
    assert tree._lod_filled

    def fresh():
        other = tree.clone()
        other.data.requires_grad_(False)
        other._lod_filled = False
        rr = _make(other, lod_pixels=VARYING["lod_pixels"])
        out = _renders(rr, dev, True, VARYING["pixel_angle"])
        assert other._lod_filled
        return out

    rs = np.random.RandomState(9)
    new = (rs.randn(tree.n_internal * 8, tree.data_dim) * 0.6).astype(f32)
    new[:, -1] = (rs.rand(tree.n_internal * 8) - 0.3) * 6.0
    tree[:] = torch.from_numpy(new).to(dev)
    assert not tree._lod_filled
    second = _renders(r, dev, True, VARYING["pixel_angle"])
    assert tree._lod_filled                                              # the render refilled
    LOD._same("after tree[:] = ...", second, fresh())
    assert not torch.equal(second["persp.False"], first["persp.False"])
    marches_of, data = _twin_of(tree)
    _check_against_twin("after tree[:] = ...", second, data, marches_of, 9, None, aux=True)
    assert tree.refine_leaves((tree.child == 0) & (tree.parent_depth[:, 1] == 1)[:, None, None, None]) > 0
    assert not tree._lod_filled
    LOD._same("after refine_leaves", _renders(r, dev, True, VARYING["pixel_angle"]), fresh())


# ---- 5: refusals by name, before any launch ----------------------------------------------------------------------------------
def test_refusals_by_name_before_a_launch(tmp_path):
    svox, oops = _svox(), _oops()
    dev = _gpu()
    tree = _tree("shell", 3, 1, dev)
    path = str(tmp_path / "tree.npz")
    tree.save(path, compress=False)
    before = tree.data.data.clone()

    @contextlib.contextmanager
    def refused(exc, match):
        """The block raises `exc` with `match`, and leaves the tree as it was: not filled, not a byte of data changed."""
        with pytest.raises(exc, match=match):
            yield
        assert not tree._lod_filled and torch.equal(tree.data.data, before), match

    with refused(NotImplementedError, r"lod_pixels=\.\.\.\) on a HalfN3Tree"):
        svox.VolumeRenderer(svox.N3Tree.load(path, map_location=dev, keep_half=True), lod_pixels=1.0)
    from plenoctree_amd.octree import compression
    import argparse
    packed = str(tmp_path / "tree_min.npz")
    compression.compress_file(path, packed, argparse.Namespace(noquant=False, bits=4, sigma_thresh=0.0, retain=0, weighted=False))
    with refused(NotImplementedError, r"lod_pixels=\.\.\.\) on a QuantizedN3Tree"):
        svox.VolumeRenderer(svox.N3Tree.load(packed, map_location=dev, keep_quantized=True), lod_pixels=1.0)
    with refused(NotImplementedError, r"lod_pixels=\.\.\.\) with ndc"):
        svox.VolumeRenderer(tree, ndc=svox.NDCConfig(8, 6, 7.0), lod_pixels=1.0)
    for kw in (dict(lod_pixels=-1.0), dict(lod_pixels="1"), dict(lod_pixels=1.0, lod_min_depth=11), dict(lod_pixels=1.0, lod_min_depth=-1),
               dict(lod_pixels=1.0, lod_min_depth=1.5)):
        with refused(ValueError, "lod_pixels|lod_min_depth"):
            svox.VolumeRenderer(tree, **kw)
    r = _make(tree, lod_pixels=2.0)
    o, d = (torch.from_numpy(a).to(dev) for a in LOD._rays())
    c2w = torch.from_numpy(VIEW["c2w"])
    small = dict(width=8, height=6, fx=7.0)
    calls = (lambda: r.render_persp(c2w, **small), lambda: r.forward(o, d, d, pixel_angle=0.05),
             lambda: r.render_persp_aux(c2w, **small), lambda: r.forward_aux(o, d, d, pixel_angle=0.05))
    with torch.no_grad():
        for call in (lambda: r.forward(o, d, d), lambda: r.forward_aux(o, d, d)):
            with refused(ValueError, "needs pixel_angle"):
                call()
    tree.data.requires_grad_(True)
    for call in calls:
        with refused(NotImplementedError, "lod_pixels=2 on a tree that requires grad"):
            call()
    tree.data.requires_grad_(False)
    with torch.no_grad(), tree.accumulate_weights("max") as accum:
        for call in calls[:2]:
            with refused(NotImplementedError, "lod_pixels=2 inside accumulate_weights"):
                call()
        assert not bool(accum.value.any())
    # the entry points' own checks, through the wrappers: the message is the library's
    view = tree.view()
    opts = oops.render_opts(STEP, 1.0, 0.0, 0.0)
    for kw, text in ((dict(cone=-0.1), "cone -0.1 must be finite and >= 0"), (dict(cone=float("nan")), "must be finite and >= 0"),
                     (dict(cone=float("inf")), "cone inf must be finite"), (dict(cone=0.1, min_depth=11), r"min_depth 11 is outside \[0, 10\]"),
                     (dict(cone=0.1, min_depth=-1), "min_depth -1 is outside")):
        for surface_thresh in (None, 0.5):
            with refused(oops.PxoError, text):
                oops.octree_render_foot_rays(view, o, d, d, opts, surface_thresh=surface_thresh, **kw)
            with refused(oops.PxoError, text):
                oops.octree_render_foot_persp(view, c2w.to(dev), 8, 6, 7.0, opts, surface_thresh=surface_thresh, **kw)
    sg = _tree("sg4", 4, 4, dev)
    with refused(NotImplementedError, r"of an SG tree \(lobes\) is not built for a PxoTree"):
        oops.octree_render_foot_rays(sg.view(), o, d, d, opts, 0.1, lobes=sg.extra_data, surface_thresh=0.5)
    with torch.no_grad(), refused(NotImplementedError, "on an SG tree"):
        _make(sg, lod_pixels=2.0).forward_aux(o, d, d, pixel_angle=0.05)
    assert not sg._lod_filled
    assert not tree._lod_filled and torch.equal(tree.data.data, before)  # nothing was launched, not even the fill
    tree.data.requires_grad_(True)
    with torch.no_grad():                                                # the same tree under no_grad renders
        assert r.render_persp(c2w, **small).shape == (6, 8, 3) and tree._lod_filled


# ---- 6: the command line -----------------------------------------------------------------------------------------------------
def test_evaluation_lod_pixels(tmp_path, monkeypatch):
    """octree.evaluation --lod_pixels 4 on 4 views of the synthetic scene (factor 16: 50 x 50 pixels) and a depth-6 tree: the
    images are those of VolumeRenderer(lod_pixels=4) on the file's tree, and not those of the run without the flag."""
    svox = _svox(); dev = _gpu()
    from plenoctree_amd.octree import evaluation
    src = str(tmp_path / "tree_opt.npz")
    _tree("chunked", 6, 16, dev).save(src, compress=False)
    cfg_path = os.path.join(str(tmp_path), "tiny.yaml")
    with open(cfg_path, "w") as fh:
        fh.write("dataset: synthetic\nfactor: 16\nnum_coarse_samples: 64\nnum_fine_samples: 128\nuse_viewdirs: false\n"
                 "white_bkgd: true\nbatch_size: 1024\nsh_deg: 3\nrandomized: true\n")
    common = ["--train_dir", str(tmp_path), "--config", cfg_path, "--synthetic_views", "4", "4", "--renderer_step_size", str(STEP),
              "--input", src]
    seen = []
    for name in ("render_persp", "render_persp_aux"):
        def recording(self, c2w, *a, _plain=getattr(svox.VolumeRenderer, name), _name=name, **k):
            res = _plain(self, c2w, *a, **k)
            seen.append((_name, self.lod_pixels, self.lod_min_depth, self.max_depth, torch.as_tensor(c2w).clone(), dict(k),
                         (res["rgb"] if isinstance(res, dict) else res).detach().cpu()))
            return res
        monkeypatch.setattr(svox.VolumeRenderer, name, recording)
    psnr_plain = evaluation.main(common)
    plain, seen[:] = list(seen), []
    psnr = evaluation.main(common + ["--lod_pixels", "4"])
    foot, seen[:] = list(seen), []
    assert len(plain) == len(foot) == 4 and np.isfinite(psnr) and np.isfinite(psnr_plain)
    assert all(s[1] is None for s in plain) and all(s[:4] == ("render_persp", 4.0, 0, None) for s in foot)
    assert any(not torch.equal(a[-1], b[-1]) for a, b in zip(plain, foot))       # the flag reached the march
    tree = svox.N3Tree.load(src, map_location=dev)
    tree.data.requires_grad_(False)
    api = svox.VolumeRenderer(tree, step_size=STEP, lod_pixels=4)
    with torch.no_grad():
        for _, _, _, _, c2w, kw, image in foot:
            assert kw["fast"] is True
            assert torch.equal(api.render_persp(c2w, **kw).cpu(), image)
    # with the flags it is allowed with: the aux call, a cap and a floor
    out_dir = str(tmp_path / "aux")
    seen[:] = []                                                         # (the API's own calls above were recorded too)
    evaluation.main(common + ["--lod_pixels", "4", "--lod_min_depth", "2", "--max_depth", "5", "--write_aux", out_dir])
    both, seen[:] = list(seen), []
    assert len(both) == 4 and all(s[:4] == ("render_persp_aux", 4.0, 2, 5) for s in both)
    api = svox.VolumeRenderer(tree, step_size=STEP, lod_pixels=4, lod_min_depth=2, max_depth=5)
    with torch.no_grad():
        for _, _, _, _, c2w, kw, image in both:
            assert torch.equal(api.render_persp_aux(c2w, **kw)["rgb"].cpu(), image)
    assert sorted(os.listdir(out_dir))[:2] == ["000_depth.npz", "000_rgba.png"]
    seen[:] = []
    # the refused pairs leave with their message
    tiny_llff = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llff_tiny")
    for argv, text in ((common + ["--keep_half"], "--lod_pixels together with --keep_half"),
                       (common + ["--keep_compressed"], "--lod_pixels together with --keep_compressed"),
                       (["--config", "llff", "--data_dir", tiny_llff, "--input", src], "--lod_pixels not built for an NDC scene")):
        with pytest.raises(NotImplementedError, match=text):
            evaluation.main(argv + ["--lod_pixels", "4"])
    assert not seen
