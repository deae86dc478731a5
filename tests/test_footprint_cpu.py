"""The footprint render without a GPU: known answers of the cap, a hand-marched tree, the conditions the GPU fixtures must
meet (asserted on the twin, oracle/octree_oracle.py's march with a footprint, and tests/_footprint_oracle.py's counts), every refusal that comes before a launch -- VolumeRenderer's by name,
the entry points' own with pointers nothing reads -- and the flags of octree.evaluation."""
import ctypes

import numpy as np
import pytest
import torch

import _footprint_oracle as F
import test_gpu_lod as LOD
from oracle import octree_oracle as T

f32 = np.float32
PTR = 0x10000                                    # a 256-byte aligned address nothing reads


# ---- the cap ---------------------------------------------------------------------------------------------------------------
def test_cap_known_answers():
    assert T.MAX_DEPTH == 10
    assert T.cap_of(f32(2.0 ** -5)) == 4                                  # side 2^-(4+1) <= f
    assert T.cap_of(np.nextafter(f32(2.0 ** -5), f32(0))) == 5            # the float just below: one level deeper
    assert T.cap_of(f32(0.0)) == T.MAX_DEPTH and T.cap_of(f32(1e-40)) == T.MAX_DEPTH      # 0 and a denormal: no cap
    assert f32(1e-40) > 0 and f32(1e-40) < np.finfo(f32).tiny
    assert T.cap_of(f32(0.5)) == 0 and T.cap_of(f32(1e30)) == 0 and T.cap_of(f32(np.inf)) == 0
    assert T.cap_of(np.nextafter(f32(0.5), f32(0))) == 1
    for d in range(T.MAX_DEPTH + 1):                                      # every cell side, and the float below it
        side = f32(2.0 ** -(d + 1))
        assert T.cap_of(side) == d and T.cap_of(np.nextafter(side, f32(0))) == min(d + 1, T.MAX_DEPTH)
    # the clamp from below
    assert T.cap_of(f32(0.5), min_depth=3) == 3 and T.cap_of(f32(2.0 ** -5), min_depth=3) == 4
    assert T.cap_of(f32(0.0), min_depth=T.MAX_DEPTH) == T.MAX_DEPTH and T.cap_of(f32(np.inf), min_depth=T.MAX_DEPTH) == T.MAX_DEPTH


# ---- a tree of three levels, one axis-parallel ray, by hand -----------------------------------------------------------------
def _hand_tree():
    """Unit volume (offset 0, invradius 1: tree coordinates are world coordinates).  Node 0 = the root; its cells 0 = (0,0,0) and
    4 = (1,0,0) are nodes 1 and 2 (depth 1, cells of side 1/4); cell 0 of node 1 is node 3 (depth 2, cells of side 1/8)."""
    t = T.Tree(4, 5, 0.5, 0.5)
    assert np.array_equal(t.offset, np.zeros(3, f32)) and np.array_equal(t.invradius, np.ones(3, f32))
    assert t.refine_leaves([0, 4]) == 2 and t.refine_leaves([8]) == 1
    assert t.child.reshape(-1)[[0, 4, 8]].tolist() == [1, 2, 2] and t.parent_depth[:, 1].tolist() == [0, 1, 1, 2]
    return t


def test_hand_marched_ray():
    """The ray (-7.5, 1/32, 1/32) + t (1, 0, 0), step 2^-10, cone 2^-4: it is inside the volume for t in [7.5, 8.5), x = t - 7.5,
    delta_scale = 1, k = 2^-4, so f = t / 16 passes 0.5 at t = 8: cap 1 for x < 0.5, cap 0 from there.  Every number is dyadic.
      t = 7.5          x = 0          f = 0.46875  cap 1: root cell 0 has a child (node 1); node 1's cell 0 has one too (node 3),
                                      but depth 1 >= cap: stop at node 1 cell 0 = flat 8.  Exit of a 1/4 cell from its face: 1/4.
      t = 7.7509765625 x = 0.2509..   f = 0.4844   cap 1: node 1's cell (1,0,0) = flat 12, a leaf.  local x = 2^-8 of the cell's
                                      1/4, exit (1 - 2^-8) / 4 = 0.2490234375; + 2^-10 = 0.25.
      t = 8.0009765625 x = 0.5009..   f = 0.50006  cap 0: root cell 4 has a child (node 2), depth 0 >= cap: flat 4.  local x =
                                      2^-9 of 1/2, exit (1 - 2^-9) / 2 = 0.4990234375; + 2^-10 = 0.5.
      t = 8.5009765625 >= tmax = 8.5: the march ends."""
    t = _hand_tree()
    o, d = np.array([-7.5, 1 / 32, 1 / 32], f32), np.array([1.0, 0.0, 0.0], f32)
    step = 2.0 ** -10
    tree, foot = (t.child, t.offset, t.invradius), lambda cone, min_depth=0: (cone, min_depth)
    m = T.march(tree, o, d, step, foot=foot(2.0 ** -4))
    assert m.delta_scale == 1.0 and not m.guard
    assert m.flat.tolist() == [8, 12, 4]
    assert m.t.tolist() == [7.5, 7.7509765625, 8.0009765625]
    assert m.delta.tolist() == [0.2509765625, 0.25, 0.5]
    assert m.dtw.tolist() == [0.2509765625, 0.25, 0.5]
    assert m.depth.tolist() == [1, 1, 0] and m.cap.tolist() == [1, 1, 0]
    assert m.has_child.tolist() == [True, False, True]
    assert F.reuse_counts(m) == (3, 2, 0, True)
    # no cone: the plain march of the oracle, down to the depth-2 cells of node 3 (flat 24 .., side 1/8)
    plain = T.march(tree, o, d, step, foot=foot(0.0))
    want = T.march_tree(t, o, d, T.RenderOptions(step))
    assert list(zip(plain.flat.tolist(), plain.dtw)) == want and plain.flat.tolist()[:2] == [24, 28]
    assert plain.delta.tolist()[:2] == [0.1259765625, 0.125]
    assert not plain.has_child.any() and set(plain.cap.tolist()) == {T.MAX_DEPTH}
    # min_depth holds the cap up: at 2 the ray is the plain one, at 1 only the last sample differs from cone 2^-4
    held = T.march(tree, o, d, step, foot=foot(2.0 ** -4, 2))
    assert held.flat.tolist() == plain.flat.tolist() and held.delta.tolist() == plain.delta.tolist()
    one = T.march(tree, o, d, step, foot=foot(2.0 ** -4, 1))
    assert one.flat.tolist()[:2] == [8, 12] and one.flat[2] == 2 * 8 + 0 and one.depth[2] == 1
    # a huge cone is the constant cap min_depth
    flat0 = T.march(tree, o, d, step, foot=foot(1e9))
    assert flat0.flat.tolist() == [0, 4] and flat0.delta.tolist() == [0.5009765625, 0.5]
    # compositing: sigma chosen so that exp is exact (0), colour sigmoid(0) = 1/2 from the stopped cell's own row
    data = np.zeros((4 * 8, 4), f32)
    data[8, -1] = np.inf
    basis = T.sh_basis_np(1, d)
    r = T.composite(data, m, basis, T.RenderOptions(step), surface_thresh=0.5)
    assert r.rgb.tolist() == [0.5, 0.5, 0.5] and r.alpha == 1.0 and r.pick == 0
    assert float(r.depth) == float(r.surface) == 7.5 + 0.5 * 0.2509765625
    assert T.composite(data, None, basis, T.RenderOptions(step, 0.25), surface_thresh=0.5).rgb.tolist() == [0.25] * 3


# ---- the conditions of the GPU fixtures -------------------------------------------------------------------------------------
# cone 0.1, the first 60 of the 300 rays, step 1e-3 (the march does not read the data: K plays no part)
TABLE = {("shell", 4): (581, 43, 4, 48), ("rod", 4): (412, 28, 5, 46), ("chunked", 6): (588, 69, 5, 48)}


@pytest.mark.parametrize("family,depth", sorted(TABLE))
def test_fixture_conditions(family, depth):
    """Every situation the GPU test is there for occurs on its fixtures: samples the cap stopped at a cell that has a child, the
    clamp case of the path reuse, rays whose cap changes.  The figures were worked out before the kernel ran."""
    t = LOD._case(family, depth, 1)
    o, d = LOD._rays()
    marches = [T.march((t.child, t.offset, t.invradius), o[i], d[i], LOD.STEP, foot=(0.1, 0)) for i in range(60)]
    c = F.case_counts(marches)
    print(family, depth, c)
    assert all(v > 0 for v in c.values()), c
    assert (c["samples"], c["cap_stopped"], c["clamp_cases"], c["rays_changing_cap"]) == TABLE[(family, depth)]


# ---- refusals by name, before any launch -------------------------------------------------------------------------------------
def _svox():
    from plenoctree_amd.octree import svox
    return svox


def _cpu_tree():
    svox = _svox()
    tree = LOD._svox_tree(LOD._case("shell", 3, 1), torch.device("cpu"))
    assert isinstance(tree, svox.N3Tree) and not tree._lod_filled
    return tree


def test_constructor_refusals():
    svox = _svox()
    tree = _cpu_tree()
    for bad in (-1, -0.5, float("nan"), float("inf"), "2", True, [1.0]):
        with pytest.raises(ValueError, match="lod_pixels"):
            svox.VolumeRenderer(tree, lod_pixels=bad)
    for bad in (-1, 11, 1.0, "1", True, None):
        with pytest.raises(ValueError, match="lod_min_depth"):
            svox.VolumeRenderer(tree, lod_pixels=1.0, lod_min_depth=bad)
    with pytest.raises(ValueError, match="lod_min_depth"):                # checked whether or not lod_pixels is set
        svox.VolumeRenderer(tree, lod_min_depth=11)
    for cls, name in ((svox.HalfN3Tree, "on a HalfN3Tree"), (svox.QuantizedN3Tree, "on a QuantizedN3Tree")):
        other = object.__new__(cls)                                      # refused by its form, before anything of it is read
        with pytest.raises(NotImplementedError, match=r"VolumeRenderer\(lod_pixels=\.\.\.\) " + name):
            svox.VolumeRenderer(other, lod_pixels=1.0)
    with pytest.raises(NotImplementedError, match=r"lod_pixels=\.\.\.\) with ndc"):
        svox.VolumeRenderer(tree, ndc=svox.NDCConfig(8, 6, 7.0), lod_pixels=1.0)
    # None and 0 are today's renderer: nothing is refused that was not, nothing is asked for
    for off in (None, 0, 0.0):
        r = svox.VolumeRenderer(tree, ndc=svox.NDCConfig(8, 6, 7.0), lod_pixels=off, lod_min_depth=3)
        assert r.lod_pixels is None
    r = svox.VolumeRenderer(tree, lod_pixels=np.float32(1.5), lod_min_depth=np.int64(2))
    assert r.lod_pixels == 1.5 and r.lod_min_depth == 2


def test_call_refusals_leave_the_tree_alone():
    svox = _svox()
    tree = _cpu_tree()
    before = tree.data.data.clone()
    r = svox.VolumeRenderer(tree, step_size=1e-3, lod_pixels=2.0)
    o, d = (torch.from_numpy(a) for a in LOD._rays())
    c2w = torch.from_numpy(LOD.VIEW["c2w"])
    cam = dict(width=8, height=6, fx=7.0)
    with torch.no_grad():
        for call in (lambda: r.forward(o, d, d), lambda: r(o, d, d), lambda: r.forward_aux(o, d, d)):
            with pytest.raises(ValueError, match="needs pixel_angle"):
                call()
        for bad in (-1e-3, float("nan"), float("inf"), "0.1", True):
            with pytest.raises(ValueError, match="pixel_angle"):
                r.forward(o, d, d, pixel_angle=bad)
    tree.data.requires_grad_(True)
    for call in (lambda: r.render_persp(c2w, **cam), lambda: r.forward(o, d, d, pixel_angle=0.05),
                 lambda: r.render_persp_aux(c2w, **cam), lambda: r.forward_aux(o, d, d, pixel_angle=0.05)):
        with pytest.raises(NotImplementedError, match="lod_pixels=2 on a tree that requires grad"):
            call()
    tree.data.requires_grad_(False)
    tree._weight_accum = object()                                         # what accumulate_weights sets for its duration
    with torch.no_grad():
        for call in (lambda: r.render_persp(c2w, **cam), lambda: r.forward(o, d, d, pixel_angle=0.05)):
            with pytest.raises(NotImplementedError, match="lod_pixels=2 inside accumulate_weights"):
                call()
    tree._weight_accum = None
    # together with max_depth the capped view's own refusals come first, in its words
    capped = svox.VolumeRenderer(tree, step_size=1e-3, max_depth=1, lod_pixels=2.0)
    tree.data.requires_grad_(True)
    with pytest.raises(NotImplementedError, match=r"fine-tune tree\.lod\(1\) instead"):
        capped.render_persp(c2w, **cam)
    tree.data.requires_grad_(False)
    # an SG tree has no aux outputs, footprint or not
    sg = LOD._svox_tree(LOD._case("sg4", 4, 4), torch.device("cpu"), sg=True)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="on an SG tree"):
        svox.VolumeRenderer(sg, lod_pixels=2.0).render_persp_aux(c2w, **cam)
    assert not sg._lod_filled
    assert not tree._lod_filled and torch.equal(tree.data.data, before)  # nothing was launched, not even the fill


def _entry(name, aux, tree=True, lobes=None, cone=0.1, min_depth=0, tree_kw=(), surface_thresh=0.5, B=5):
    from plenoctree_amd import _lib
    lib = _lib.load()
    t = _lib.PxoTree()
    fields = dict(child=PTR, data=PTR, n_internal=9, data_dim=49, basis_dim=16, offset=(0.5,) * 3, invradius=(0.5,) * 3)
    fields.update(dict(tree_kw))
    for k, v in fields.items():
        setattr(t, k, (ctypes.c_float * 3)(*v) if isinstance(v, tuple) else v)
    opts = _lib.PxoRenderOpts()
    opts.step_size, opts.background_brightness, opts.sigma_thresh, opts.stop_thresh = 1e-3, 1.0, 0.0, 0.0
    args = (ctypes.byref(t) if tree else None,) + (() if aux else (lobes,)) + (None, PTR, PTR, PTR, B, ctypes.byref(opts),
                                                                               cone, min_depth)
    args += (surface_thresh, PTR, PTR, None) if aux else (PTR, None)
    rc = getattr(lib, name)(*args)
    return rc, "" if rc == 0 else lib.pxo_last_error().decode()


@pytest.mark.parametrize("name,aux", [("pxo_octree_render_foot_fwd", False), ("pxo_octree_render_foot_aux_fwd", True)])
def test_entry_point_refusals(name, aux):
    """The entry points' own checks, in the project's error text; they run before any HIP call, so no pointer is read."""
    assert _entry(name, aux, tree=False) == (-1, f"{name}: null tree")
    assert _entry(name, aux, tree_kw={"child": None}) == (-1, f"{name}: null tree")
    assert _entry(name, aux, tree_kw={"data": None}) == (-1, f"{name}: null tree")
    assert _entry(name, aux, cone=-1e-6) == (-1, f"{name}: cone -1e-06 must be finite and >= 0")
    assert _entry(name, aux, cone=float("inf")) == (-1, f"{name}: cone inf must be finite and >= 0")
    rc, text = _entry(name, aux, cone=float("nan"))
    assert rc == -1 and text.startswith(f"{name}: cone ") and text.endswith("must be finite and >= 0")
    assert _entry(name, aux, min_depth=-1) == (-1, f"{name}: min_depth -1 is outside [0, 10]")
    assert _entry(name, aux, min_depth=11) == (-1, f"{name}: min_depth 11 is outside [0, 10]")
    # order: the footprint's arguments are looked at before the options, the format and the rays
    assert _entry(name, aux, cone=-1.0, tree_kw={"basis_dim": 7, "data_dim": 22})[1] == f"{name}: cone -1 must be finite and >= 0"
    # and what the uncapped entry points refuse is refused in the same words
    assert _entry(name, aux, tree_kw={"basis_dim": 7, "data_dim": 22}) == \
        (-1, f"{name}: basis_dim 7 is not an SH format (1,4,9,16,25)")
    assert _entry(name, aux, tree_kw={"n_internal": 0}) == (-1, f"{name}: n_internal out of range")
    assert _entry(name, aux, B=-1)[0] == -1
    if aux:
        assert _entry(name, aux, surface_thresh=1.5)[1].startswith(f"{name}: surface_thresh 1.5 must lie in (stop_thresh")
    else:
        assert _entry(name, aux, lobes=PTR, tree_kw={"basis_dim": 7, "data_dim": 22}) == \
            (-1, f"{name}: basis_dim 7 is not a supported SG format (sg_dim 1,4,9,16,25)")
    assert _entry(name, aux, B=0) == (0, "")                              # nothing to do is not an error, and launches nothing


def test_sg_tree_on_the_aux_entry_is_refused():
    """The aux entry takes no lobes; the one door to it refuses an SG tree by name."""
    from plenoctree_amd import _lib, octree_ops
    t = _lib.PxoTree()
    with pytest.raises(NotImplementedError, match=r"alpha / depth / surface at a depth per sample.* of an SG tree \(lobes\) is "
                                                  "not built for a PxoTree"):
        octree_ops._call(t, "foot_aux", object(), None, (), None, ())
    with pytest.raises(NotImplementedError, match=r"of an NDC scene \(ndc\) is not built for a PxoTree"):
        octree_ops._call(t, "foot", None, octree_ops.ndc_spec(8, 6, 7.0), (), None, ())
    for form in (_lib.PxoHalfTree, _lib.PxoQuantTree):
        with pytest.raises(NotImplementedError, match="is not built for a " + form.__name__):
            octree_ops._call(form(), "foot", None, None, (), None, ())


# ---- the command line ------------------------------------------------------------------------------------------------------
def _flags(*argv):
    from plenoctree_amd.octree import evaluation
    return evaluation, evaluation.define_flags().parse_args(list(argv))


def test_evaluation_flags():
    ev, a = _flags()
    assert a.lod_pixels is None and a.lod_min_depth is None
    ev.check_lod_flags(a)
    ev, a = _flags("--lod_pixels", "4")
    assert a.lod_pixels == 4.0 and a.lod_min_depth is None
    ev.check_lod_flags(a)
    ev, a = _flags("--lod_pixels", "1.5", "--lod_min_depth", "3", "--max_depth", "5", "--write_aux", "x", "--write_points", "y.ply")
    assert (a.lod_pixels, a.lod_min_depth, a.max_depth) == (1.5, 3, 5)
    ev.check_lod_flags(a)                                                 # allowed together
    with pytest.raises(SystemExit):
        _flags("--lod_pixels", "many")
    with pytest.raises(SystemExit):
        _flags("--lod_min_depth", "1.5")
    for argv, exc, text in (
            (("--lod_min_depth", "2"), ValueError, "--lod_min_depth without --lod_pixels"),
            (("--lod_pixels", "-1"), ValueError, "--lod_pixels -1.0: must be a finite number >= 0"),
            (("--lod_pixels", "nan"), ValueError, "--lod_pixels nan"),
            (("--lod_pixels", "2", "--lod_min_depth", "11"), ValueError, r"--lod_min_depth 11: must be in \[0, 10\]"),
            (("--lod_pixels", "2", "--lod_min_depth", "-1"), ValueError, "--lod_min_depth -1"),
            (("--lod_pixels", "2", "--keep_half"), NotImplementedError, "--lod_pixels together with --keep_half"),
            (("--lod_pixels", "2", "--keep_compressed"), NotImplementedError, "--lod_pixels together with --keep_compressed"),
            (("--lod_pixels", "2", "--dataset", "llff"), NotImplementedError, "--lod_pixels not built for an NDC scene")):
        ev, a = _flags(*argv)
        with pytest.raises(exc, match=text):
            ev.check_lod_flags(a)
    ev, a = _flags("--lod_pixels", "2", "--dataset", "llff", "--spherify", "true")     # a spherified LLFF scene is in world space
    ev.check_lod_flags(a)
    # and through main, before anything is loaded (the input does not exist)
    import os
    tiny_llff = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llff_tiny")
    for argv, text in ((["--config", "blender", "--keep_half"], "--lod_pixels together with --keep_half"),
                       (["--config", "blender", "--keep_compressed"], "--lod_pixels together with --keep_compressed"),
                       (["--config", "llff", "--data_dir", tiny_llff], "--lod_pixels not built for an NDC scene")):
        with pytest.raises(NotImplementedError, match=text):
            ev.main(argv + ["--input", "/nonexistent/tree.npz", "--lod_pixels", "2"])
    with pytest.raises(ValueError, match="--lod_min_depth without --lod_pixels"):
        ev.main(["--config", "blender", "--input", "/nonexistent/tree.npz", "--lod_min_depth", "2"])
