"""Scenes for the scene renderer's tests, shared by tests/test_scene_cpu.py (the twin alone: every case exercises what it is
there for, and the twin's own float32-to-float64 compositing gap) and tests/test_gpu_scene.py (HIP against the twin).

Every case is at most about 300 rays of small trees, so the numpy twin renders it in a few seconds; the reference of a case is
computed once per process and handed out read-only."""
import functools

import numpy as np

import _octree_cases as C
import _scene_oracle as S
from oracle import octree_oracle as T

f32 = np.float32
ORIGIN_VIEW = dict(c2w=C.look_at((3.6, 2.9, 2.4), target=(0.0, 0.0, 0.0)), W=19, H=13, fx=14.0, fy=12.5)
SMALL_VIEW = dict(c2w=C.look_at((-4.1, 3.3, 2.2), target=(0.0, 0.0, 0.0)), W=13, H=9, fx=8.0, fy=9.0)
LINE_VIEW = dict(c2w=C.look_at((6.0, 0.35, 0.25), target=(0.0, 0.0, 0.0)), W=17, H=11, fx=22.0, fy=22.0)
INSIDE_VIEW = dict(c2w=C.look_at((0.1, 0.0, -0.2), target=(2.0, 0.4, 0.1)), W=15, H=11, fx=9.0, fy=9.0)
WIDE_VIEW = dict(c2w=C.look_at((0.0, -7.0, 1.0), target=(0.5, 0.0, 0.0)), W=23, H=9, fx=11.0, fy=11.0)


@functools.lru_cache(maxsize=None)
def tree(K, depth=2, seed=None):
    return C.random_tree(depth, 20 + K if seed is None else seed, K=K)


def _inst(K, axis, angle, trans, scale, **kw):
    return S.Instance(tree(K, **kw), S.axis_angle(axis, angle), trans, scale)


def _ring(n, K_of):
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        out.append(_inst(K_of(k), (0.3, 0.2 + 0.1 * k, 1.0), 40.0 * k, (1.6 * np.cos(a), 1.6 * np.sin(a), 0.15 * (k % 3)),
                         0.55 + 0.05 * (k % 4)))
    return out


def _same_tree_twice():
    t = tree(4)
    return [S.Instance(t, S.axis_angle((0, 0, 1), 30.0), (0.4, 0.0, 0.0), 0.9),
            S.Instance(t, S.axis_angle((1, 1, 0), -70.0), (-0.3, 0.2, 0.1), 1.1)]


# name -> (instances, view, the counters of S.Counts the case must exercise)
OVERLAP = ("gap_steps", "multi_live", "non_leader")
CASES = {
    "two_overlap_scaled": (lambda: [_inst(4, (0.2, 0.3, 1.0), 35.0, (0.3, -0.2, 0.1), 0.8),
                                    _inst(9, (1.0, -0.4, 0.2), -50.0, (-0.2, 0.3, -0.1), 1.3)], ORIGIN_VIEW, OVERLAP),
    "three_mixed_formats": (lambda: [_inst(1, (0.1, 1.0, 0.1), 80.0, (0.2, 0.1, 0.3), 1.0),
                                     _inst(16, (0.2, 0.3, 1.0), 20.0, (-0.3, -0.2, 0.0), 0.9),
                                     _inst(25, (1.0, 0.2, -0.3), -35.0, (0.1, 0.4, -0.2), 1.1)], ORIGIN_VIEW, OVERLAP),
    "eight_on_a_ring": (lambda: _ring(8, lambda k: (1, 4, 9, 4)[k % 4]), SMALL_VIEW, OVERLAP),
    # two cubes apart along the view: nothing is inside between them, w jumps and the transmittance is carried across
    "two_in_a_line": (lambda: [_inst(4, (0, 0, 1), 15.0, (1.6, 0.0, 0.0), 0.5), _inst(4, (0, 1, 0), -25.0, (-1.6, 0.0, 0.0), 0.5)],
                      LINE_VIEW, ("jumps",)),
    "small_inside_large": (lambda: [_inst(9, (0, 0, 1), 10.0, (0.0, 0.0, 0.0), 1.0),
                                    _inst(4, (1, 0, 1), 45.0, (0.15, 0.05, -0.1), 0.3)], ORIGIN_VIEW, OVERLAP),
    "camera_inside": (lambda: [S.Instance(tree(4)), _inst(9, (0, 1, 1), 30.0, (1.9, 0.4, 0.2), 0.6)], INSIDE_VIEW,
                      ("inside_origin", "gap_steps", "multi_live")),
    # rays that hit only the last-listed instance, and rays that hit none
    "last_only_and_none": (lambda: [_inst(4, (0, 0, 1), 20.0, (-1.2, 0.0, 0.0), 0.6), _inst(1, (0, 1, 0), 40.0, (-0.9, 0.3, 0.2), 0.6),
                                    _inst(9, (1, 0, 0), 60.0, (3.2, 0.0, 0.3), 0.4)], WIDE_VIEW, OVERLAP),
    "same_tree_twice": (_same_tree_twice, ORIGIN_VIEW, OVERLAP),
}
OPT = {"exact": T.RenderOptions.for_renderer(1e-3, False), "fast": T.RenderOptions(1e-3, 0.0, 1e-2, 1e-2)}
CASE_OPTS = [(name, "fast" if k % 2 else "exact") for k, name in enumerate(CASES)]      # both presets, background 1 and 0


@functools.lru_cache(maxsize=None)
def instances(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name, opt, dtype=f32):
    """(image [H,W,3] of the twin, its Counts), read-only."""
    cnt = S.Counts()
    img = S.render_persp(instances(name), opt=OPT[opt], dtype=dtype, counts=cnt, **CASES[name][1])
    img.setflags(write=False)
    return img, cnt
