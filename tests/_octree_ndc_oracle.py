"""The shapes the tests of the NDC launches of the octree side share (pxo_octree_render_ndc_fwd / _bwd,
pxo_grid_weight_render_ndc), and a known answer.  The oracle is oracle/octree_oracle.py with its `ndc=` argument: "convert
(ndc_ray: items 2, 3 and 5 of the definition, include/plenoctree_octree.h), then the existing march".

The 14 x 10 image whose edge pixels land on NDC x = +-1, camera A (identity: every NDC ray parallel to z, the degenerate
invdir case), camera B (translated and rotated), and depth-3 random trees in two boxes.
"""
import math

import numpy as np

import _octree_cases as C
from oracle import octree_oracle as T

f32 = np.float32
W, H, FX = 14, 10, 13.0
NEAR = 1.0
BOXES = (((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.1, 0.0, -0.2), (0.8, 0.9, 0.7)))


class Ndc:
    """width / height / focal / near: what octree_ops takes as `ndc`."""

    def __init__(self, width=W, height=H, focal=FX, near=NEAR):
        self.width, self.height, self.focal, self.near = width, height, focal, near


def camera_a():
    return np.eye(4, dtype=f32)[:3]


def camera_b():
    yaw, pitch = 0.15, -0.1
    ry = np.array([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]])
    rx = np.array([[1, 0, 0], [0, math.cos(pitch), -math.sin(pitch)], [0, math.sin(pitch), math.cos(pitch)]])
    return np.concatenate([ry @ rx, np.array([[0.2], [-0.1], [0.05]])], 1).astype(f32)


CAMERAS = {"A": camera_a, "B": camera_b}


def box_tree(K, box, depth=3, seed=None, p=0.15):
    """_octree_cases.random_tree (random mask, random SH data, about a third of the leaves empty) in one of the NDC boxes."""
    return C.random_tree(depth, 40 + K if seed is None else seed, K, p, *BOXES[box])


# ---- known answer, independent of the oracle's compositing ---------------------------------------------------------------
KNOWN_SIGMA, KNOWN_STEP = 1.5, 1e-4


def known_tree():
    """Full depth-1 tree (4^3 cells) on the cube [-1, 1]^3: sigma 1.5 everywhere, SH4 with one degree-1 coefficient in each of
    two channels (z in red, x in green), blue constant."""
    t = T.build_from_mask(np.ones((4, 4, 4), bool), 1, 13, [0.0, 0.0, 0.0], 1.0)
    t.data[:] = 0.0
    t.data[..., 0 * 4 + 2] = 2.0          # red: Y_1,0 (z)
    t.data[..., 1 * 4 + 3] = -1.5         # green: Y_1,1 (x)
    t.data[..., 1 * 4 + 0] = 0.4
    t.data[..., -1] = KNOWN_SIGMA
    return t


def chord_f64(o, d):
    """Length of the ray o + t d (unit d, t >= 0) inside [-1, 1]^3, float64 slab test; 0 if it misses."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    lo, hi = 0.0, np.inf
    for a in range(3):
        if d[a] == 0.0:
            if abs(o[a]) > 1.0:
                return 0.0
            continue
        t1, t2 = (-1.0 - o[a]) / d[a], (1.0 - o[a]) / d[a]
        lo, hi = max(lo, min(t1, t2)), min(hi, max(t1, t2))
    return max(hi - lo, 0.0)


def known_answer(tree, o, d, shade_dir, ndc):
    """(1 - exp(-sigma L)) sigmoid(c . Y(shade_dir)) with L the float64 chord of the NDC ray of (o, d); None for a miss."""
    no, nd, ok = T.ndc_ray(o, d, ndc)
    if not ok:
        return None
    L = chord_f64(no, nd / np.linalg.norm(nd.astype(np.float64)))
    basis = T.sh_basis_np(4, shade_dir).astype(np.float64)
    coef = tree.data.reshape(-1, 13)[0, :12].reshape(3, 4).astype(np.float64)
    return (1.0 - math.exp(-KNOWN_SIGMA * L)) / (1.0 + np.exp(-(coef @ basis)))


def known_answer_check(render):
    """Known answer 2 (shared with the device test): `render(tree, origins, dirs, opt)` -> [B,3] of camera B's rays on
    known_tree() must be (1 - exp(-sigma L)) sigmoid(c . Y(vdir_world)), L the float64 chord of the NDC ray in the cube, within
    sigma * n_samples * step_size * delta_scale + 1e-5 (delta_scale = 2 for this box): how far the summed step lengths can
    exceed the chord.  The same formula on the NDC direction must be off by more than 0.03.  Returns (max error, max bound)."""
    ndc = Ndc()
    t = known_tree()
    opt = T.RenderOptions(step_size=KNOWN_STEP, background_brightness=0.0)
    o, d = T.camera_rays(camera_b(), W, H, FX)
    got = np.asarray(render(t, o, d, opt), np.float64)
    worst, worst_bound, wrong, hits = 0.0, 0.0, 0.0, 0
    for i, (oo, dd) in enumerate(zip(o, d)):
        seq = T.march(t, oo, dd, opt.step_size, ndc=ndc)
        if seq is None:
            assert np.array_equal(got[i], np.zeros(3))
            continue
        hits += 1
        want = known_answer(t, oo, dd, dd, ndc)
        bound = KNOWN_SIGMA * len(seq) * KNOWN_STEP * 2.0 + 1e-5
        err = float(np.abs(got[i] - want).max())
        assert err <= bound, (i, err, bound, len(seq))
        worst, worst_bound = max(worst, err), max(worst_bound, bound)
        _, nd, _ = T.ndc_ray(oo, dd, ndc)
        wrong = max(wrong, float(np.abs(known_answer(t, oo, dd, nd, ndc) - got[i]).max()))
    assert hits >= 20 and wrong > 0.03, (hits, wrong)
    return worst, worst_bound
