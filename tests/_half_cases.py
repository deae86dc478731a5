"""Trees kept in the float16 of their files (`N3Tree.load(path, keep_half=True)`), shared by tests/test_half_tree_cpu.py and
tests/test_gpu_half_tree.py.

Every tree is one of the existing fixtures -- tests/_octree_sg_cases.py (depth 3..5, both node orders, sigma scaled so that
the early stop is reached; rendered as SH and, with the fixture's lobes, as SG), tests/_octree_aux_cases.py (depth 3, a third
of the leaves empty) and the NDC trees of tests/_octree_ndc_oracle.py -- written with N3Tree.save, which rounds the data to
float16, and loaded from that file: once as a float tree, once with keep_half.  The oracle references are taken on the
WIDENED data (the values both trees hold) and computed once per process.
"""
import copy
import functools

import numpy as np

import _octree_aux_cases as A
import _octree_cases as C
import _octree_sg_cases as G
from oracle import octree_oracle as T

f32, f16 = np.float32, np.float16
KS = (1, 4, 9, 16, 25)
ROW_STRIDE = {1: 4, 4: 16, 9: 28, 16: 52, 25: 76}         # include/plenoctree_octree.h, PxoHalfTree
VIEW = G.VIEW                                             # 16 x 12: no multiple of any lane variant's patch, 11 % background
STEP = G.STEP
LANES = (0, 4, 8, 16)                                     # 0: the default


def host_tree(t, fmt, lobes=None):
    """The svox N3Tree (CPU) holding the oracle tree `t`: its child, parent_depth, transform and float32 data."""
    import torch
    from plenoctree_amd.octree import svox
    radius = f32(0.5) / t.invradius
    host = svox.N3Tree(N=2, data_dim=t.data_dim, depth_limit=max(int(t.parent_depth[:, 1].max()), 1), radius=radius,
                       center=(f32(1.0) - f32(2.0) * t.offset) * radius, data_format=fmt, extra_data=lobes)
    # the transform is the oracle's own, bit for bit, not the constructor's rounding of radius / center
    host._set_transform(t.invradius, t.offset)
    host.child, host.parent_depth = torch.from_numpy(t.child.copy()), torch.from_numpy(t.parent_depth.copy())
    host.data = torch.nn.Parameter(torch.from_numpy(t.data.copy()))
    host.level_nodes = [int(c) for c in np.bincount(t.parent_depth[:, 1])]
    host._leaves = None
    return host


def save(path, t, fmt, lobes=None):
    """Writes `t` with N3Tree.save (float16 data) and returns the path."""
    host_tree(t, fmt, lobes).save(path)
    return path


def widened(t):
    """A copy of the oracle tree whose data went through float16: what both loads of the saved file hold."""
    w = copy.deepcopy(t)
    w.data[:] = t.data.astype(f16).astype(f32)
    assert np.isfinite(w.data).all()
    return w


def packed_layout(data16, n, D):
    """The documented device layout of the first n nodes of the file's data: float16 [n*8, row_stride], zeros in the padding."""
    stride = (D + 3) // 4 * 4
    out = np.zeros((n * 8, stride), f16)
    out[:, :D] = data16[:n].reshape(n * 8, D)
    return out, stride


# ---- SH and SG renders of the _octree_sg_cases trees -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sg_tree(K):
    return widened(G.tree(K))


def options(fast):
    return T.RenderOptions.for_renderer(STEP, fast)


@functools.lru_cache(maxsize=None)
def rays(K):
    """37 rays aimed at leaves of every depth with unrelated view directions, then the 13 edge rays of _octree_cases (three of
    which see only the background): (origins, dirs, viewdirs, indices of the background rays)."""
    o, d = C.aimed_rays(G.tree(K), seed=70 + K, per_depth=lambda depth: 13)      # >= 39 rays for a depth-3 tree
    assert len(o) >= 37
    rs = np.random.RandomState(700 + K)
    v = rs.randn(37, 3)
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)
    names, eo, ed, ev = C.edge_rays()
    miss = [37 + names.index(n) for n in C.EDGE_BACKGROUND]
    return (np.concatenate([o[:37], eo]).astype(f32), np.concatenate([d[:37], ed]).astype(f32),
            np.concatenate([v, ev]).astype(f32), miss)


@functools.lru_cache(maxsize=None)
def want(kind, K, fast):
    """(image [H,W,3], rays [50,3]) of the oracle on the widened data; kind "SH" or "SG" (oracle/octree_oracle.py with the
    fixture's lobes)."""
    t, opt = sg_tree(K), options(fast)
    o, d, v, _ = rays(K)
    lobes = G.lobes(K) if kind == "SG" else None
    img = T.render_persp(t, VIEW["c2w"], VIEW["W"], VIEW["H"], VIEW["fx"], opt, VIEW["fy"], lobes=lobes)
    return img, T.render_rays(t, o, d, v, opt, lobes=lobes)


# ---- aux: the _octree_aux_cases configurations --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def aux_tree(K):
    return widened(A.tree(K))
