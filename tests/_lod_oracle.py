"""Level of detail of a PlenOctree, restated in numpy float64 (include/plenoctree_octree.h, "level of detail"): the value of a
node, the bottom-up fill and the truncated tree `N3Tree.lod(L)`.  Everything walks the tree by child / parent_depth, node by
node; no device code, nothing shared with plenoctree_amd.  Used by tests/test_lod_cpu.py and tests/test_gpu_lod.py.

Bounds of the device fill against node_value on the device's own rows (derived, to first order, not measured):
  a coefficient   16 * 2^-24 * (sum_j w_j |c_j[k]|) / S + 2^-126    8 product roundings, 7 additions in each of the two sums,
                                                                    one division; 2^-126 for a result that underflows
  sigma           8 * 2^-24 * S / 8                                 7 additions; the scaling by 1/8 is exact
"""
import numpy as np

EPS = 2.0 ** -24


def node_value(rows):
    """Value [D] (float64) of a node from the rows [8, D] of its cells in storage order: w_j = max(s_j, 0), sigma = sum(w) / 8,
    c[k] = sum(w_j c_j[k]) / sum(w) where sum(w) > 0, else 0."""
    rows = np.asarray(rows, np.float64)
    w = np.maximum(rows[:, -1], 0.0)
    S = 0.0
    for j in range(8):
        S = S + w[j]
    out = np.zeros(rows.shape[1], np.float64)
    out[-1] = S * 0.125
    if S > 0.0:
        acc = np.zeros(rows.shape[1] - 1, np.float64)
        for j in range(8):
            acc = acc + w[j] * rows[j, :-1]
        out[:-1] = acc / S
    return out


def node_bound(rows):
    """Per element [D]: how far the float32 evaluation of node_value(rows) may be from it (module docstring)."""
    rows = np.asarray(rows, np.float64)
    w = np.maximum(rows[:, -1], 0.0)
    S = w.sum()
    out = np.full(rows.shape[1], 2.0 ** -126, np.float64)
    if S > 0.0:
        out[:-1] += 16.0 * EPS * (w[:, None] * np.abs(rows[:, :-1])).sum(0) / S
    out[-1] = 8.0 * EPS * S / 8.0
    return out


def max_depth(parent_depth):
    return int(np.asarray(parent_depth)[:, 1].max())


def nodes_by_depth(parent_depth, d):
    return np.nonzero(np.asarray(parent_depth)[:, 1] == d)[0]


def fill(child, parent_depth, data):
    """The whole pyramid in float64: a copy of data [n, 2,2,2, D] with, deepest level first, the value of every node of depth
    >= 1 written into the row of its parent cell."""
    D = data.shape[-1]
    out = np.asarray(data, np.float64).copy()
    rows = out.reshape(-1, D)
    flat_child = np.asarray(child).reshape(-1)
    for d in range(max_depth(parent_depth), 0, -1):
        for n in nodes_by_depth(parent_depth, d):
            p = int(parent_depth[n, 0])
            assert flat_child[p] != 0 and p // 8 + flat_child[p] == n, "parent cell does not point back"
            rows[p] = node_value(rows[n * 8:n * 8 + 8])
    return out


def lod(child, parent_depth, data, L):
    """(child, parent_depth, data) of the tree cut at depth L, from `data` as it stands (already filled, or not): the nodes of
    depth <= L in their original order; a depth-L node's cells are all leaves and keep their rows; a cell that still has a
    child gets a zero row; parent_depth is remapped, the root's record is (0, 0)."""
    child, parent_depth = np.asarray(child), np.asarray(parent_depth)
    n, D = child.shape[0], data.shape[-1]
    new_of = {}
    for old in range(n):
        if parent_depth[old, 1] <= L:
            new_of[old] = len(new_of)
    m = len(new_of)
    c = np.zeros((m, 8), child.dtype)
    pd = np.zeros((m, 2), parent_depth.dtype)
    rows = np.zeros((m, 8, D), data.dtype)
    flat_child, src = child.reshape(n, 8), np.asarray(data).reshape(n, 8, D)
    for old, new in new_of.items():
        depth = int(parent_depth[old, 1])
        pd[new, 1] = depth
        if old != 0:
            p = int(parent_depth[old, 0])
            pd[new, 0] = new_of[p // 8] * 8 + p % 8
        for j in range(8):
            skip = int(flat_child[old, j])
            if skip != 0 and depth < L:
                c[new, j] = new_of[old + skip] - new
            else:
                rows[new, j] = src[old, j]
    return c.reshape(m, 2, 2, 2), pd, rows.reshape(m, 2, 2, 2, D)


def valid_tree(child, parent_depth):
    """Every child pointer leads forward to a node whose record names that cell and the next depth; node 0 is the root."""
    child, parent_depth = np.asarray(child), np.asarray(parent_depth)
    n = child.shape[0]
    flat = child.reshape(n, 8)
    if tuple(parent_depth[0]) != (0, 0):
        return False
    seen = np.zeros(n, bool)
    seen[0] = True
    for node in range(n):
        for j in range(8):
            if flat[node, j]:
                tgt = node + int(flat[node, j])
                if not 0 < tgt < n or seen[tgt] or tuple(parent_depth[tgt]) != (node * 8 + j, parent_depth[node, 1] + 1):
                    return False
                seen[tgt] = True
    return bool(seen.all())
