"""Coverage conditions of tests/_octree_cases.py, asserted on the oracle alone (no GPU): the deep-tree GPU module
(tests/test_gpu_octree_depth.py) compares kernels with the oracle on these cases, and it can only catch a defect at depth d
if the rays put shaded, still-visible samples into leaves of depth d.  These are conditions on the cases, not measurements
of any kernel; the counts are printed (pytest -s) for the record."""
import numpy as np
import pytest

import _octree_cases as C
from oracle import octree_oracle as T

OPT = T.RenderOptions(1e-3)


@pytest.mark.parametrize("depth", C.DEPTHS)
@pytest.mark.parametrize("family", ["shell", "chunked"])
def test_aimed_rays_shade_every_leaf_depth(family, depth):
    """Every leaf depth 1..depth receives >= 30 samples with sigma > sigma_thresh and transmittance > 1e-2 on arrival."""
    t = C.make_tree(family, depth, 4)
    assert t.n_internal < 10000
    leaf_d = np.bincount(t.depths(), minlength=depth + 1)
    assert (leaf_d[1:] > 0).all(), leaf_d
    o, d = C.aimed_rays(t, 5)
    samples, live, _ = C.depth_coverage(t, o, d, OPT)
    print(f"\n{family} depth {depth}: {t.n_internal} nodes, {len(o)} aimed rays; samples per depth {samples.tolist()}, "
          f"shaded with T > 1e-2 per depth {live.tolist()}")
    assert (live[1:] >= 30).all(), live
    sig = t.data[..., -1][t.child == 0]
    assert 0.2 < float((sig <= 0).mean()) < 0.5                      # a mix of empty and occupied leaves


@pytest.mark.parametrize("depth", C.DEPTHS)
def test_rod_rays_stay_in_the_deepest_level(depth):
    """Each ray along the rod takes >= 1000 samples, >= 80 % of them in deepest-level leaves, >= 1000 of them
    consecutive.  A depth-6 tree has 128 finest cells per axis and a straight line crosses fewer than 3 * 128 of them,
    so 1000 cannot be asked there: >= 300 (the rod's |dx| + |dy| + |dz| = 2.65 times 128, less the samples the step
    size merges)."""
    t = C.make_tree("rod", depth, 4)
    assert t.n_internal < 10000
    o, d = C.rod_axis_rays(t)
    opt = T.RenderOptions(C.ROD_STEP)
    samples, live, per_ray = C.depth_coverage(t, o, d, opt)
    need = 1000 if depth >= 8 else 300
    for ds in per_ray:
        deepest = sum(1 for x in ds if x == depth)
        run = best = 0
        for x in ds:
            run = run + 1 if x == depth else 0
            best = max(best, run)
        print(f"\nrod depth {depth}: {len(ds)} samples, {deepest} at depth {depth}, longest consecutive run {best}")
        assert len(ds) >= need and deepest >= 0.8 * len(ds) and best >= need, (len(ds), deepest, best)
    assert live[depth] >= 30                                        # and the ray still sees what it samples there
    so, sd = C.rod_skew_rays(t, 3)
    _, _, skew = C.depth_coverage(t, so, sd, opt)
    assert all(len(ds) > 50 for ds in skew)


@pytest.mark.parametrize("depth", C.DEPTHS)
def test_rod_view_reuses_the_path(depth):
    """The camera along the rod (the view octree_count_work is given): its axis pixel marches the deepest level like the
    rod rays do, and the expected child-pointer loads, derived from the leaf sequence, lie strictly between one per
    sample and the count without path reuse -- so equality with the device counter says that reuse happened, and by
    how much."""
    t = C.make_tree("rod", depth, 4)
    view = C.rod_view(t)
    opt = T.RenderOptions(C.ROD_STEP)
    o, d = T.camera_rays(**view)
    axis = view["W"] * (view["H"] // 2) + view["W"] // 2
    _, _, per_ray = C.depth_coverage(t, o[axis:axis + 1], d[axis:axis + 1], opt)
    need = 1000 if depth >= 8 else 300
    assert len(per_ray[0]) >= need and sum(1 for x in per_ray[0] if x == depth) >= 0.8 * len(per_ray[0])
    c, no_reuse = C.tree_march_counts(t, view, opt)
    print(f"\nrod view depth {depth}: {c}, loads without reuse {no_reuse}, axis pixel {len(per_ray[0])} samples")
    assert c["rays"] == view["W"] * view["H"] and c["samples"] >= 2 * need
    assert c["samples"] < c["child_loads"] < no_reuse < c["samples"] * (depth + 1)
    assert no_reuse > 2 * c["child_loads"]                          # most levels of most lookups are reused


@pytest.mark.parametrize("depth", C.DEPTHS)
def test_chunked_tree_is_the_same_tree_in_another_node_order(depth):
    one, ch = C.make_tree("shell", depth, 4), C.make_tree("chunked", depth, 4)
    last = ch.parent_depth[:, 1] == depth
    assert last.sum() > 3 and not (np.diff(ch.parent_depth[last, 0]) > 0).all()
    assert (np.diff(one.parent_depth[one.parent_depth[:, 1] == depth, 0]) > 0).all()      # the one-shot tree is in order
    assert (np.diff(ch.parent_depth[:, 1]) >= 0).all()                                   # levels themselves stay in order
    assert ch.n_internal == one.n_internal and C.leaf_set(ch) == C.leaf_set(one)
    assert not np.array_equal(ch.child, one.child)


@pytest.mark.parametrize("family,depth", [("shell", 8), ("rod", 10), ("chunked", 6)])
def test_edge_rays_are_finite_and_background_where_they_see_nothing(family, depth):
    t = C.make_tree(family, depth, 4)
    names, o, d, v = C.edge_rays()
    assert not np.allclose(d, v)
    assert sum(int((np.abs(x) == 0).sum() == 1) for x in d) >= 2 and sum(int((np.abs(x) == 0).sum() == 2) for x in d) >= 3
    opt = T.RenderOptions(1e-3, background_brightness=0.25)
    for name, oo, dd, vv in zip(names, o, d, v):
        rgb = T.render_ray(t, oo, dd, vv, opt)
        n = len(T.march_tree(t, oo, dd, opt) or [])
        assert np.isfinite(rgb).all(), name
        if name in C.EDGE_BACKGROUND:
            assert n == 0 and np.array_equal(rgb, np.full(3, 0.25, np.float32)), (name, rgb)
        else:
            assert n >= 3, (name, n)
    i = names.index("corner")
    ot, dt, invdir, _ = T._to_tree_ray(o[i], d[i], t.offset, t.invradius)
    tmin, tmax = T._dda_unit(ot, invdir)
    assert tmin == tmax and tmin > 0                                 # touches the volume in one point
    i = names.index("in_plane_x_half")
    ot, dt, _, _ = T._to_tree_ray(o[i], d[i], t.offset, t.invradius)
    assert ot[0] == 0.5 and dt[0] == 0.0
    for nm in ("on_boundary", "on_boundary_axis"):
        ot = T._to_tree_ray(o[names.index(nm)], d[names.index(nm)], t.offset, t.invradius)[0]
        assert (ot == 0.0).sum() == 1 and ((ot >= 0) & (ot <= 1)).all()


def test_camera_views_and_far_origin_case():
    """The camera views see the tree (and not only it: some rays miss the volume); the far-origin ray can only end by the
    stop guard, which the plain oracle loop does not have -- the GPU test of that ray asserts what it can without one."""
    for family in C.FAMILIES:
        t = C.make_tree(family, 8, 4)
        for view in C.CAMERA_VIEWS:
            c, no_reuse = C.tree_march_counts(t, view, OPT)
            assert c["samples"] <= c["child_loads"] < no_reuse
            assert 50 < c["rays"] < view["W"] * view["H"] and c["shaded_samples"] > 200 and c["distinct_leaves"] > 100, c
    assert C.CAMERA_VIEWS[1]["fx"] != C.CAMERA_VIEWS[1]["fy"]
    for depth in C.DEPTHS:
        o, d, opt, n = C.far_origin_ray(C.make_tree("shell", depth, 4))
        assert n >= 5 and np.linalg.norm(o) > 3000


def test_grid_cases():
    for reso in C.GRID_SIZES:
        W, H, fx, fy = C.grid_case(reso)
        assert fx != fy
        if reso > 13:
            assert W > 16 and (W % 16 or H % 16)
    sg = C.grid_sigma(128)
    assert 0.3 < float((sg > 0).mean()) < 0.5
