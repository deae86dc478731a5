"""The numpy twin of the scene renderer (tests/_scene_oracle.py) against oracle/octree_oracle.py: the exact identities the
definition is built to keep (include/plenoctree_octree.h, "scene"), pinned on the CPU before any GPU run."""
import functools

import numpy as np
import pytest

import _octree_cases as C
import _scene_cases as SC
import _scene_oracle as S
from oracle import octree_oracle as T

f32 = np.float32
TREES = {"d3_sh4": (3, 5, 4), "d2_sh1": (2, 9, 1)}
OPTS = {"exact": T.RenderOptions.for_renderer(1e-3, False), "fast": T.RenderOptions.for_renderer(1e-3, True)}
CASES = [(t, v, o) for t in TREES for v in range(len(C.CAMERA_VIEWS)) for o in OPTS]


@functools.lru_cache(maxsize=None)
def tree(name):
    return C.random_tree(TREES[name][0], TREES[name][1], K=TREES[name][2])


@functools.lru_cache(maxsize=None)
def plain(name, v, o):
    img = T.render_persp(tree(name), opt=OPTS[o], **C.CAMERA_VIEWS[v])
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("name,v,o", CASES)
def test_one_identity_instance_is_the_plain_render(name, v, o):
    cnt = S.Counts()
    img = S.render_persp([S.Instance(tree(name))], opt=OPTS[o], counts=cnt, **C.CAMERA_VIEWS[v])
    assert cnt.rounds > 0 and cnt.non_leader == 0 and cnt.gap_steps == 0
    assert np.array_equal(img, plain(name, v, o))


@pytest.mark.parametrize("name,v,o", CASES)
def test_complementary_halves_are_the_whole(name, v, o):
    a, b = S.split_by_x(tree(name))
    assert (a.data[..., -1] != tree(name).data[..., -1]).any() and (b.data[..., -1] != tree(name).data[..., -1]).any()
    cnt = S.Counts()
    img = S.render_persp([S.Instance(a), S.Instance(b)], opt=OPTS[o], counts=cnt, **C.CAMERA_VIEWS[v])
    assert cnt.non_leader == 0                        # identical structure: lockstep
    assert np.array_equal(img, plain(name, v, o))


@pytest.mark.parametrize("name,v,o", CASES)
def test_rotated_scaled_instance_from_the_carried_camera(name, v, o):
    view = dict(C.CAMERA_VIEWS[v])
    view["c2w"] = S.transformed_camera(view["c2w"], S.CYCLIC, 2.0)
    img = S.render_persp([S.Instance(tree(name), S.CYCLIC, scale=2.0)], opt=OPTS[o], **view)
    assert np.array_equal(img, plain(name, v, o))
    if o == "exact":                                   # the guard: a transposed matrix is seen
        wrong = S.render_persp([S.Instance(tree(name), S.CYCLIC.T, scale=2.0)], opt=OPTS[o], **view)
        assert np.abs(wrong - plain(name, v, o)).max() > 0.1


def overlapping(name, k=3):
    t = tree(name)
    poses = [(S.axis_angle((0.2, 0.3, 1.0), 35.0), (0.3, -0.2, 0.1), 0.8),
             (S.axis_angle((1.0, -0.4, 0.2), -50.0), (-0.2, 0.3, -0.1), 1.3),
             (S.axis_angle((0.1, 1.0, 0.1), 80.0), (0.1, 0.1, 0.4), 1.0)]
    return [S.Instance(t, *p) for p in poses[:k]]


@pytest.mark.parametrize("name,o", [(t, o) for t in TREES for o in OPTS])
def test_overlapping_instances_either_order(name, o):
    two = overlapping(name, 2)
    cnt = S.Counts()
    a = S.render_persp(two, opt=OPTS[o], counts=cnt, **C.CAMERA_VIEWS[0])
    b = S.render_persp(two[::-1], opt=OPTS[o], **C.CAMERA_VIEWS[0])
    assert cnt.multi_live > 0 and cnt.non_leader > 0
    print("order gap", np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-6


@pytest.mark.parametrize("name,o", [(t, o) for t in TREES for o in OPTS])
def test_three_overlapping_instances_terminate(name, o):
    cnt = S.Counts()
    img = S.render_persp(overlapping(name, 3), opt=OPTS[o], counts=cnt, **C.CAMERA_VIEWS[0])
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0 + 1e-5
    assert cnt.multi_live > 0 and cnt.non_leader > 0
    assert (img != OPTS[o].background_brightness).any()


def test_instance_validates_on_the_host():
    """svox.Instance: what it accepts, what it raises by name; nothing here touches a GPU."""
    import torch
    from plenoctree_amd.octree import svox
    tree = svox.N3Tree(N=2, data_dim=13, depth_limit=3, data_format="SH4")
    R = S.axis_angle((0.3, -0.2, 1.0), 40.0)
    i = svox.Instance(tree, R, (1.0, 2.0, 3.0), 1.5)
    assert np.array_equal(i.rotation, R) and i.scale == 1.5 and i.translation.tolist() == [1.0, 2.0, 3.0]
    d = svox.Instance(tree)
    assert np.array_equal(d.rotation, np.eye(3)) and d.scale == 1.0 and not d.translation.any()
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = 1.5 * R, (1.0, 2.0, 3.0)
    for mat, trans in ((m, [1.0, 2.0, 3.0]), (m[:3, :3], [0.0, 0.0, 0.0])):
        j = svox.Instance(tree, matrix=mat)
        assert abs(j.scale - 1.5) < 1e-12 and np.abs(j.rotation - R).max() < 1e-12 and j.translation.tolist() == trans
    for bad in (1.5 * R, np.diag([1.0, 1.0, -1.0]), R + 1e-3, np.eye(4), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError, match="rotation"):
            svox.Instance(tree, bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-46, "2", True):
        with pytest.raises(ValueError, match="scale"):
            svox.Instance(tree, R, scale=bad)
    for bad in ((0.0, float("nan"), 0.0), (0.0, 0.0), (float("inf"), 0.0, 0.0)):
        with pytest.raises(ValueError, match="translation"):
            svox.Instance(tree, R, bad)
    shear = np.eye(3)
    shear[0, 1] = 0.2
    for bad, word in ((shear, "rotation"), (np.diag([1.0, 2.0, 1.0]), "rotation"), (np.diag([1.0, 1.0, -1.0]), "determinant"),
                      (np.zeros((3, 3)), "determinant"), (np.eye(2), "3x3 or 4x4"), (2.0 * np.eye(4), "last row")):
        with pytest.raises(ValueError, match=word):
            svox.Instance(tree, matrix=bad)
    with pytest.raises(ValueError, match="excludes"):
        svox.Instance(tree, R, matrix=m)
    sg = svox.N3Tree(N=2, data_dim=13, depth_limit=3, data_format="SG4",
                     extra_data=torch.tensor([[2.0, 0.0, 0.0, 1.0]] * 4))
    with pytest.raises(NotImplementedError, match="SG tree"):
        svox.Instance(sg)
    for cls in (svox.QuantizedN3Tree, svox.HalfN3Tree):
        with pytest.raises(NotImplementedError, match=f"{cls.NOUN}.*{cls.WAY_OUT}"):
            svox.Instance(cls.__new__(cls))
    with pytest.raises(TypeError, match="N3Tree"):
        svox.Instance(object())
    with pytest.raises(TypeError, match="svox.Instance"):
        svox.SceneRenderer([tree])


@pytest.mark.parametrize("name,opt", SC.CASE_OPTS)
def test_gpu_cases_exercise_what_they_are_for(name, opt):
    """No case of tests/test_gpu_scene.py is vacuous: the twin counts, on the case's own rays, at least one of each event the
    case is there for (a gap step, a round with two live instances, a non-leader advance; for the cubes in a line a jump; for
    the camera inside an instance an origin with tmin = 0), every instance is hit by some ray, and the image is not flat."""
    img, cnt = SC.reference(name, opt)
    for what in SC.CASES[name][2]:
        assert getattr(cnt, what) > 0, (name, what, vars(cnt))
    n = len(SC.instances(name))
    assert {i for key in cnt.hits for i in key} == set(range(n)), cnt.hits
    assert np.isfinite(img).all() and img.reshape(-1, 3).std(0).min() > 0.01
    if name == "last_only_and_none":
        assert cnt.hits.get((n - 1,), 0) > 0 and cnt.hits.get((), 0) > 0, cnt.hits
    if name == "two_in_a_line":
        assert cnt.hits.get((0, 1), 0) > 20, cnt.hits
    if name == "eight_on_a_ring":
        assert n == S.MAX_INSTANCES


@pytest.mark.parametrize("name,opt", SC.CASE_OPTS)
def test_twin_float32_compositing_gap_is_under_half_the_gpu_bound(name, opt):
    """tests/test_gpu_scene.py holds the kernel to the float32 twin within atol 2e-5 (the single-tree forward's bound).  That
    is sound only while the twin's own float32 round-off on these inputs, measured against the same rounds composited in
    float64, stays below half of it.  Measured: at most 2.3e-7 over the eight cases."""
    a, _ = SC.reference(name, opt)
    b, _ = SC.reference(name, opt, np.float64)
    gap = np.abs(a - b).max()
    print(name, opt, "float32 - float64 compositing gap", gap)
    assert gap < 1e-5
