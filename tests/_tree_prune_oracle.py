"""Test-side oracle of the per-leaf weight accumulation (pxo_octree_weight_accum_*) and of the structural collapse
(pxo_tree_collapse_*): numpy only, built on oracle/octree_oracle.py's march and composite.

Weights.  A ray's compositing weights are composite's, taken twice: in float32 (the operation order of oracle.render_ray,
stop once light <= stop_thresh), and in float64 over the SAME samples (the float32 compositing decides where an
early-stopped ray ends, so that both see the same samples).  Per leaf: max and sum of either, and the sample count.

Collapse.  A recursion on the definition (include/plenoctree_octree.h): dead(node) = every cell is a leaf with keep == 0 or
points to a dead node; the root survives; survivors are renumbered in storage order.
"""
import functools

import numpy as np

import _octree_cases as C
import _octree_ndc_oracle as N
from oracle import octree_oracle as T

f32 = np.float32


class LeafWeights:
    """Per flat cell index: max32 / sum32 (float32 compositing), max64 / sum64 (float64), count (shaded samples); floor = the
    largest |float32 - float64| of a single sample's weight."""

    def __init__(self, cells):
        self.max32, self.sum32 = np.zeros(cells, f32), np.zeros(cells, f32)
        self.max64, self.sum64 = np.zeros(cells, np.float64), np.zeros(cells, np.float64)
        self.count = np.zeros(cells, np.int64)
        self.floor = 0.0

    def add_ray(self, rows, m, opt):
        if m is None:
            return
        r32 = T.composite(rows, m, None, opt)
        r64 = T.composite(rows, m, None, T.RenderOptions(opt.step_size, 1.0, opt.sigma_thresh, 0.0), np.float64)
        leaf, w32, w64 = m.flat[r32.shaded], r32.weight[r32.shaded], r64.weight[r32.shaded]
        if not len(leaf):
            return
        np.maximum.at(self.max32, leaf, w32)
        np.add.at(self.sum32, leaf, w32)                 # unbuffered and in sample order: one float32 rounding per sample
        np.maximum.at(self.max64, leaf, w64)
        np.add.at(self.sum64, leaf, w64)
        np.add.at(self.count, leaf, 1)
        self.floor = max(self.floor, float(np.abs(w32.astype(np.float64) - w64).max()))


def march_rays(tree, origins, dirs, step_size, ndc=None):
    """The March of every ray (None for a miss); it depends on the step size only, not on the thresholds."""
    return [T.march(tree, o, d, step_size, ndc=ndc) for o, d in zip(np.asarray(origins, f32), np.asarray(dirs, f32))]


def leaf_weights(tree, marches, opt):
    """LeafWeights of the given per-ray marches (march_rays) under the thresholds of `opt`."""
    rows = tree.data.reshape(-1, tree.data_dim)
    lw = LeafWeights(tree.n_internal * 8)
    for m in marches:
        lw.add_ray(rows, m, opt)
    return lw


def single_ray_weights(tree, origin, direction, opt):
    return leaf_weights(tree, march_rays(tree, [origin], [direction], opt.step_size), opt)


# ---- collapse -------------------------------------------------------------------------------------------------------
def collapse(child, parent_depth, data, keep):
    """(child, parent_depth, data, old2new) of the collapsed tree, by the definition."""
    n = child.shape[0]
    ch = np.asarray(child).reshape(n, 8)
    keep = np.asarray(keep).reshape(n, 8).astype(bool)
    rows = np.asarray(data).reshape(n, 8, -1)

    @functools.lru_cache(maxsize=None)
    def dead(node):
        return all((not keep[node, c]) if ch[node, c] == 0 else dead(node + int(ch[node, c])) for c in range(8))

    survivors = [node for node in range(n) if node == 0 or not dead(node)]
    old2new = np.full(n, -1, np.int64)
    old2new[survivors] = np.arange(len(survivors))
    new_child = np.zeros((len(survivors), 8), np.int32)
    new_pd = np.zeros((len(survivors), 2), np.int32)
    new_data = np.zeros((len(survivors), 8, rows.shape[-1]), f32)
    for m, node in enumerate(survivors):
        for c in range(8):
            sub = node + int(ch[node, c])
            if ch[node, c] != 0 and not dead(sub):
                new_child[m, c] = old2new[sub] - m
                new_data[m, c] = rows[node, c]
            elif ch[node, c] == 0 and keep[node, c]:
                new_data[m, c] = rows[node, c]
        p = int(parent_depth[node, 0])
        assert old2new[p >> 3] >= 0, "a survivor's parent survives"
        new_pd[m] = (old2new[p >> 3] * 8 + (p & 7), parent_depth[node, 1])
    return (new_child.reshape(-1, 2, 2, 2), new_pd, new_data.reshape((-1, 2, 2, 2, rows.shape[-1])), old2new)


def collapsed_tree(tree, keep):
    """An oracle Tree holding collapse() of `tree` (same transform), and old2new."""
    child, pd, data, old2new = collapse(tree.child, tree.parent_depth, tree.data, keep)
    t = T.Tree.__new__(T.Tree)
    t.data_dim, t.depth_limit = tree.data_dim, tree.depth_limit
    t.invradius, t.offset = tree.invradius.copy(), tree.offset.copy()
    t.child, t.parent_depth, t.data = child, pd, data
    return t, old2new


def valid_tree(child, parent_depth):
    """Structural invariants every consumer relies on: children point forward to nodes whose record points back."""
    n = child.shape[0]
    ch = np.asarray(child).reshape(n, 8)
    seen = np.zeros(n, bool)
    seen[0] = True
    for node in range(n):
        for c in range(8):
            if ch[node, c]:
                sub = node + int(ch[node, c])
                if not (0 < sub < n) or seen[sub] or parent_depth[sub, 0] != node * 8 + c or \
                        parent_depth[sub, 1] != parent_depth[node, 1] + 1:
                    return False
                seen[sub] = True
    return bool(seen.all()) and tuple(parent_depth[0]) == (0, 0)


# ---- hand-built trees for the collapse cases --------------------------------------------------------------------------
def _filled(t, seed):
    rs = np.random.RandomState(seed)
    t.data[:] = rs.randn(*t.data.shape).astype(f32)
    return t


def nest_tree(K=1, seed=3):
    """Root -> cell 5 -> cell 2 -> cell 7: a three-level nest below the root, and a one-level branch at root cell 1."""
    t = T.Tree(3 * K + 1, 5, [0.0, 0.0, 0.0], 1.0)
    t.refine_leaves([5])                          # node 1
    t.refine_leaves([1 * 8 + 2])                  # node 2
    t.refine_leaves([2 * 8 + 7])                  # node 3
    t.refine_leaves([1])                          # node 4 (depth 1, stored after deeper nodes)
    return _filled(t, seed)


def nest_keep_cascade(t):
    """Everything below root cell 5 dead: nodes 3, 2, 1 go in cascade; the rest stays."""
    keep = np.ones((t.n_internal, 8), bool)
    keep[1:4] = False
    return keep


def seven_dead_keep(t):
    """Node 3's cells: seven dead, one live -> nothing collapses, seven rows zeroed."""
    keep = np.ones((t.n_internal, 8), bool)
    keep[3] = False
    keep[3, 4] = True
    return keep


# ---- the weight cases shared by tests/test_tree_prune_cpu.py (floor, left-out share) and tests/test_gpu_tree_prune.py ----
STEP = 1e-3
CAM_W, CAM_H, CAM_FX, CAM_FY = 37, 29, 30.0, 33.0      # 1,073 rays per camera: no multiple of 256
CAM_EYES = ((3.4, 3.1, 2.6), (-2.2, -4.0, 1.9), (1.2, 4.4, -1.6))
BATCHES = (0, 1, 255, 256, 257)
# name -> (family, depth, K, step); "sg4" is shell's geometry with 13 floats per cell, rendered as an SG4 tree on the device
TREES = {"shell1": ("shell", 6, 1, STEP), "chunked16": ("chunked", 6, 16, STEP), "rod1": ("rod", 10, 1, C.ROD_STEP),
         "sg4": ("shell", 6, 4, STEP)}


def case_tree(name):
    family, depth, K, _ = TREES[name]
    return C.make_tree(family, depth, K)


def options(name, fast):
    return T.RenderOptions.for_renderer(TREES[name][3], fast)


def camera(i):
    return C.look_at(CAM_EYES[i])


@functools.lru_cache(maxsize=None)
def ray_set(name):
    """(origins, dirs) float32: the 13 edge rays first (corner, away and miss among them), then for the rod its two axis rays,
    then rays aimed at leaves of every depth -- at least 257 in all."""
    t = case_tree(name)
    _, eo, ed, _ = C.edge_rays()
    o, d = [eo], [ed]
    if TREES[name][0] == "rod":
        ao, ad = C.rod_axis_rays(t)
        o.append(ao); d.append(ad)
    for seed in (5, 6):
        ao, ad = C.aimed_rays(t, seed)
        o.append(ao); d.append(ad)
    return np.concatenate(o).astype(f32), np.concatenate(d).astype(f32)


@functools.lru_cache(maxsize=None)
def ray_marches(name):
    o, d = ray_set(name)
    return tuple(march_rays(case_tree(name), o, d, TREES[name][3]))


@functools.lru_cache(maxsize=None)
def camera_marches(name, cam):
    view = dict(c2w=camera(cam), W=CAM_W, H=CAM_H, fx=CAM_FX, fy=CAM_FY)
    o, d = T.camera_rays(**view)
    return tuple(march_rays(case_tree(name), o, d, TREES[name][3]))


@functools.lru_cache(maxsize=None)
def ray_case(name, lo, hi, fast):
    """LeafWeights of rays [lo, hi) of ray_set(name)."""
    return leaf_weights(case_tree(name), ray_marches(name)[lo:hi], options(name, fast))


@functools.lru_cache(maxsize=None)
def camera_case(name, n_cams, fast):
    marches = [m for cam in range(n_cams) for m in camera_marches(name, cam)]
    return leaf_weights(case_tree(name), marches, options(name, fast))


# NDC: tests/_octree_ndc_oracle.py's set-up (14 x 10 image, cameras A and B, a depth-3 tree in the second box)
NDC_K, NDC_BOX = 4, 1


def ndc_tree():
    return N.box_tree(NDC_K, NDC_BOX)


@functools.lru_cache(maxsize=None)
def ndc_rays():
    """Camera B's rays, then five rays with d_z >= 0 (NDC misses) aimed at the tree's box from either side."""
    o, d = T.camera_rays(N.camera_b(), N.W, N.H, N.FX)
    back_d = np.array([[0.0, 0.0, 1.0], [0.3, 0.1, 0.9], [0.6, -0.8, 0.0], [-0.2, 0.4, 0.5], [1.0, 0.0, 0.0]], np.float64)
    back_d = (back_d / np.linalg.norm(back_d, axis=1, keepdims=True)).astype(f32)
    back_o = (np.array(N.BOXES[NDC_BOX][0], f32) - 3.0 * back_d).astype(f32)
    return np.concatenate([o, back_o]).astype(f32), np.concatenate([d, back_d]).astype(f32)


@functools.lru_cache(maxsize=None)
def ndc_case(mode):
    """mode "rays": ndc_rays(); mode "cams": cameras A and B in one launch."""
    t, ndc, opt = ndc_tree(), N.Ndc(), T.RenderOptions(STEP)
    if mode == "rays":
        o, d = ndc_rays()
    else:
        oa, da = T.camera_rays(N.camera_a(), N.W, N.H, N.FX)
        ob, db = T.camera_rays(N.camera_b(), N.W, N.H, N.FX)
        o, d = np.concatenate([oa, ob]), np.concatenate([da, db])
    marches = march_rays(t, o, d, STEP, ndc)
    return leaf_weights(t, marches, opt), sum(m is None for m in marches)


def all_cases():
    """Every LeafWeights the GPU tests compare against, by name (the CPU test measures the floor and the left-out share)."""
    out = {}
    for fast in (False, True):
        for n_cams in (1, 3):
            out[f"cams shell1 n{n_cams} fast{int(fast)}"] = camera_case("shell1", n_cams, fast)
        out[f"cams chunked16 n3 fast{int(fast)}"] = camera_case("chunked16", 3, fast)
        for name in TREES:
            out[f"rays {name} all fast{int(fast)}"] = ray_case(name, 0, len(ray_set(name)[0]), fast)
    for B in BATCHES:
        out[f"rays shell1 B{B}"] = ray_case("shell1", 0, B, False)
    out["ndc rays"], out["ndc cams"] = ndc_case("rays")[0], ndc_case("cams")[0]
    return out


def left_out(lw, op):
    """Cells whose float64 weight is positive but below 1e-30: float32 underflow decides whether they show up."""
    w64 = lw.max64 if op == "max" else lw.sum64
    return (w64 > 0) & (w64 < 1e-30)
