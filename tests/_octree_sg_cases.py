"""Scenes of the SG tree tests, shared by tests/test_sg_cpu.py (the conditions that keep the GPU test from passing vacuously,
on the CPU helper alone) and tests/test_gpu_sg.py (HIP vs the helper).  Trees come from tests/_octree_cases.py at depth 3..5,
lobes from the fixture tests/golden/sg_reference.npz (a sharp lobe, a nearly flat one, random ones).  Every reference image is
computed once per process (lru_cache) and shared."""
import copy
import functools
import os

import numpy as np

import _octree_cases as C
from oracle import octree_oracle as T

f32 = np.float32
KS = (1, 4, 9, 16, 25)
# depth and family per K: every depth 3..5 and both node orders occur
CASE_OF = {1: ("shell", 3), 4: ("chunked", 4), 9: ("shell", 5), 16: ("chunked", 3), 25: ("shell", 5)}
# 16 x 12: 12 rows leave the last tile row partial at every lanes-per-ray value (tiles are 8x8, 8x4 and 4x4 pixels)
# fx 22: 89 % of the pixels enter the volume, the rest see only the background
VIEW = dict(c2w=C.look_at((3.4, 3.1, 2.6)), W=16, H=12, fx=22.0, fy=22.0)
# the shells of _octree_cases are thin (a cell crossing has an optical depth of 0.12); sigma is scaled in a COPY of the tree
# so that most rays accumulate visible opacity and a few saturate (the early stop and its rescale are reached)
SIGMA_SCALE = 6.0
STEP = 1e-3
N_RAYS = 37                     # no multiple of any rays-per-block (64, 32, 16)


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sg_reference.npz"))
    return {k: z[k] for k in z.files}


def lobes(K):
    """The fixture's lobes (the reference's own extraction.py:439-442 expression, float64) rounded to float32."""
    return np.ascontiguousarray(fixture()[f"lobes_{K}"].astype(f32))


@functools.lru_cache(maxsize=None)
def tree(K):
    family, depth = CASE_OF[K]
    t = copy.deepcopy(C.make_tree(family, depth, K))
    t.data[..., -1] *= f32(SIGMA_SCALE)
    return t


def options(fast):
    return T.RenderOptions.for_renderer(STEP, fast)


@functools.lru_cache(maxsize=None)
def ray_batch(K):
    """37 explicit rays: 30 aimed at leaves of every depth, 7 edge cases (inside the volume, on its boundary, axis-parallel,
    and three that see only the background: corner, away, miss).  viewdirs = dirs for the aimed rays, unrelated unit vectors
    for the rest."""
    t = tree(K)
    o, d = C.aimed_rays(t, seed=40 + K)
    names, eo, ed, ev = C.edge_rays()
    pick = [names.index(n) for n in ("inside", "on_boundary", "two_zero_x", "one_zero", "corner", "away", "miss")]
    o = np.concatenate([o[:30], eo[pick]]).astype(f32)
    v = np.concatenate([d[:30], ev[pick]]).astype(f32)
    d = np.concatenate([d[:30], ed[pick]]).astype(f32)
    assert o.shape == (N_RAYS, 3)
    return o, d, v


@functools.lru_cache(maxsize=None)
def want_image(K, fast, dtype="f32"):
    return T.render_persp(tree(K), VIEW["c2w"], VIEW["W"], VIEW["H"], VIEW["fx"], options(fast), VIEW["fy"], lobes=lobes(K),
                          dtype=f32 if dtype == "f32" else np.float64)


@functools.lru_cache(maxsize=None)
def want_rays(K, fast, dtype="f32"):
    o, d, v = ray_batch(K)
    return T.render_rays(tree(K), o, d, v, options(fast), lobes=lobes(K), dtype=f32 if dtype == "f32" else np.float64)


@functools.lru_cache(maxsize=None)
def sh_image(K):
    """The same data read as SH: what a dispatch that silently takes the SH basis would render."""
    return T.render_persp(tree(K), VIEW["c2w"], VIEW["W"], VIEW["H"], VIEW["fx"], options(False), VIEW["fy"])


@functools.lru_cache(maxsize=None)
def view_alphas(K):
    """Accumulated opacity 1 - light of every ray of the view (float64 over march's samples, no early stop); 0 for a miss."""
    t, opt = tree(K), options(False)
    rows = t.data.reshape(-1, t.data_dim)
    o, d = T.camera_rays(**VIEW)
    return np.array([1.0 - T.composite(rows, T.march(t, oo, dd, opt.step_size), None, opt, np.float64).light for oo, dd in zip(o, d)])
