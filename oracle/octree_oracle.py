"""CPU restatement of the PlenOctree side of the path: N3Tree build / sample / assign, the dense
grid weight render and the octree volume renderer (forward + gradient w.r.t. the tree data).

TEST INFRASTRUCTURE -- the checker, never the product.  Only tests/, __graft_entry__.smoke()
and bench.py's cpu_baseline leg may import this.

PARITY UNPINNED.  These algorithms live in the third-party package `svox` (pin `svox>=0.2.28`,
/root/reference/environment.yml), which is NOT in /root/reference and not installed here.  What
is restated is svox's published algorithm (PlenOctrees, Yu et al. 2021, sec. 4.1-4.3 and the svox
0.2.28 semantics of N3Tree / VolumeRenderer / _C.grid_weight_render), anchored on the reference's
own call sites:

  N3Tree(N, data_dim, init_refine=0, depth_limit, radius, center, data_format)   octree/extraction.py:476-486
  tree[grid].refine()                                                            octree/extraction.py:341-350
  tree.depths / tree.max_depth / tree[inds].sample(S) / tree[inds] = rgba        octree/extraction.py:358-394
  tree[:, -1:].relu_(), tree.shrink_to_fit(), tree.save(path, compress=False)    octree/extraction.py:503-509
  _C.grid_weight_render(grid, cam, opts, offset, invradius)                      octree/extraction.py:181-214
  VolumeRenderer(t, step_size, ndc).render_persp(c2w, width, height, fx, fast)   octree/nerf/utils.py:456-474,
                                                                                 octree/optimization.py:174-216
  npz keys                                                                        octree/compression.py:76-86
It is pinned only by closed-form known answers (tests/test_octree_oracle.py).

One of each: `march` is the only ray march through a tree (NDC conversion and the footprint cap are arguments of it),
`composite` the only numpy compositing loop (SH or SG basis, float32 or float64, the aux sums), `render_rays_torch` the only
differentiable compositor, `grid_march` the only march through a dense grid.  march_tree, render_ray, render_persp and
grid_weight_render are views of these; what the tests measure besides (leaf weights, work counts, coverage) are reductions
over the records `march` and `composite` return.

Conventions (svox): world -> tree coordinates x_t = offset + invradius * x_w with
invradius = 0.5 / radius, offset = 0.5 * (1 - center / radius) (same formulas the reference uses at
octree/extraction.py:250-251); `child[n,i,j,k]` = index(child node) - n, 0 for a leaf;
`parent_depth[n]` = (packed index of the parent cell ((p*N+i)*N+j)*N+k, depth of n); leaves are ordered by
packed cell index.  All marching arithmetic is float32, one rounding per operation, in the order written
here (the HIP kernels are compiled without fused contraction so the two traversals take identical steps).
"""
import math

import numpy as np
import torch

from . import nerf_oracle as O

f32 = np.float32
N = 2
MAX_DEPTH = 10                                   # PXO_TREE_MAX_DEPTH


class RenderOptions:
    """svox RenderOptions as set by VolumeRenderer._get_options / extraction.calculate_grid_weights."""

    def __init__(self, step_size=1e-3, background_brightness=1.0, sigma_thresh=0.0, stop_thresh=0.0):
        self.step_size = f32(step_size)
        self.background_brightness = f32(background_brightness)
        self.sigma_thresh = f32(sigma_thresh)
        self.stop_thresh = f32(stop_thresh)

    @classmethod
    def for_renderer(cls, step_size, fast):
        """fast=True is svox's early-stopping preset (eval_octree passes fast=not no_early_stop)."""
        return cls(step_size, 1.0, 1e-2 if fast else 0.0, 1e-2 if fast else 0.0)


class Tree:
    def __init__(self, data_dim, depth_limit, center, radius):
        radius = np.broadcast_to(np.asarray(radius, f32), (3,)).astype(f32)
        center = np.broadcast_to(np.asarray(center, f32), (3,)).astype(f32)
        self.data_dim = data_dim
        self.depth_limit = depth_limit
        self.invradius = (f32(0.5) / radius).astype(f32)
        self.offset = (f32(0.5) * (f32(1.0) - center / radius)).astype(f32)
        self.child = np.zeros((1, N, N, N), np.int32)
        self.parent_depth = np.zeros((1, 2), np.int32)
        self.data = np.zeros((1, N, N, N, data_dim), f32)

    @property
    def n_internal(self):
        return self.child.shape[0]

    # -- structure ---------------------------------------------------------------------------
    def world2tree(self, p):
        return (self.offset + self.invradius * np.asarray(p, f32)).astype(f32)

    def find(self, p_tree, cap=None):
        """svox query_single_from_root with a depth counter: (node, i, j, k, cube_sz, local position inside the cell, depth)
        of the first cell on the way down that is a leaf or, with `cap`, sits at depth >= cap."""
        x = np.clip(np.asarray(p_tree, f32), f32(0.0), f32(1.0 - 1e-6)).astype(f32)
        node, depth, cube = 0, 0, f32(N)
        while True:
            x = (x * f32(N)).astype(f32)
            u = np.floor(x).astype(np.int64)
            x = (x - u.astype(f32)).astype(f32)
            skip = int(self.child[node, u[0], u[1], u[2]])
            if skip == 0 or (cap is not None and depth >= cap):
                return node, int(u[0]), int(u[1]), int(u[2]), cube, x, depth
            cube = f32(cube * f32(N))
            node += skip
            depth += 1

    def query(self, p_tree, cap=None):
        """find() without the depth (cube_sz = 2^(depth+1) says it): (node, i, j, k, cube_sz, local position)."""
        return self.find(p_tree, cap)[:6]

    def leaves(self):
        """All leaves in packed-index order: [n_leaves, 4] (node, i, j, k)."""
        return np.argwhere(self.child == 0)

    def depths(self):
        lv = self.leaves()
        return self.parent_depth[lv[:, 0], 1]

    def refine_leaves(self, packed):
        """N3Tree.refine(sel=...): split the given leaves (unique, ascending packed index)."""
        packed = np.unique(np.asarray(packed, np.int64))
        node, cell = packed // 8, packed % 8
        keep = self.parent_depth[node, 1] < self.depth_limit
        packed, node, cell = packed[keep], node[keep], cell[keep]
        n0, k = self.n_internal, packed.shape[0]
        if k == 0:
            return 0
        self.child = np.concatenate([self.child, np.zeros((k, N, N, N), np.int32)])
        self.data = np.concatenate([self.data, np.zeros((k, N, N, N, self.data_dim), f32)])
        self.parent_depth = np.concatenate([self.parent_depth, np.zeros((k, 2), np.int32)])
        new = np.arange(n0, n0 + k)
        self.child.reshape(-1)[packed] = (new - node).astype(np.int32)
        self.data[n0:] = self.data.reshape(-1, self.data_dim)[packed][:, None, None, None, :]
        self.parent_depth[n0:, 0] = packed
        self.parent_depth[n0:, 1] = self.parent_depth[node, 1] + 1
        return k

    def refine_at(self, pts_world):
        """tree[pts].refine() (octree/extraction.py:341-350)."""
        packed = []
        for p in np.asarray(pts_world, f32):
            n, i, j, k, _, _ = self.query(self.world2tree(p))
            packed.append(((n * 2 + i) * 2 + j) * 2 + k)
        return self.refine_leaves(packed)

    def node_corners(self):
        """Lower corner (tree coords, exact dyadic) and integer depth of every node."""
        corner = np.zeros((self.n_internal, 3), np.float64)
        for n in range(1, self.n_internal):
            packed, d = self.parent_depth[n]
            p, c = packed // 8, packed % 8
            ijk = np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1], np.float64)
            corner[n] = corner[p] + ijk * 0.5 ** d
        return corner


def grid_points(reso, offset, invradius):
    """Cell centres of the reso^3 grid in world coordinates, x slowest (octree/extraction.py:294-303)."""
    arr = ((np.arange(reso, dtype=f32) + f32(0.5)) / f32(reso)).astype(f32)
    ax = [((arr - offset[a]) / invradius[a]).astype(f32) for a in range(3)]
    g = np.stack(np.meshgrid(*ax, indexing="ij"), -1)
    return g.reshape(-1, 3)


def build_from_mask(mask, depth, data_dim, center, radius):
    """Step 1's tree build, literally as the reference does it (octree/extraction.py:337-350):
    `depth` rounds of tree[grid].refine() with grid = centres of the masked voxels of the 2^(depth+1) grid."""
    reso = 2 ** (depth + 1)
    assert mask.shape == (reso, reso, reso)
    tree = Tree(data_dim, depth, center, radius)
    pts = grid_points(reso, tree.offset, tree.invradius)[mask.reshape(-1)]
    for _ in range(depth):
        tree.refine_at(pts)
    return tree


def leaf_corners(tree, leaves):
    """Lower corner and side length (tree coords) of leaves given as rows (node, i, j, k)."""
    corner = tree.node_corners()
    d = tree.parent_depth[leaves[:, 0], 1].astype(np.float64)
    side = 0.5 ** (d + 1)
    return corner[leaves[:, 0]] + leaves[:, 1:4] * side[:, None], side


# -- SH basis (svox calc_sh_basis == nerf_sh/nerf/sh.py:54-109 polynomials) ------------------------
def sh_basis_np(basis_dim, d):
    deg = int(round(math.sqrt(basis_dim))) - 1
    return O.sh_basis(deg, torch.tensor(np.asarray(d, f32))[None])[0].numpy().astype(f32)


# -- SG basis (svox data_format SG<K>): lobes [K,4] rows (lambda_i, mu_i), basis_i(d) = exp(lambda_i (mu_i . d - 1)) / K;
# anchored to the reference's own eval_sg by tests/golden/sg_reference.npz (tests/test_sg_cpu.py) --------------------------
def sg_basis_np(lobes, d):
    """float32 [K]: dot, minus 1, times lambda, exp, times 1/K -- every step rounded to float32, the order the kernels use."""
    lobes, d = np.asarray(lobes, f32), np.asarray(d, f32)
    K = lobes.shape[0]
    out = np.zeros(K, f32)
    inv_k = f32(f32(1.0) / f32(K))
    for i in range(K):
        lam, mx, my, mz = lobes[i]
        dot = f32(f32(f32(mx * d[0]) + f32(my * d[1])) + f32(mz * d[2]))
        out[i] = f32(np.exp(f32(lam * f32(dot - f32(1.0))), dtype=f32) * inv_k)
    return out


def sg_basis_f64(lobes, d):
    """The same in float64 on the float32 inputs, vectorised over directions: [..., K]."""
    lobes, d = np.asarray(lobes, np.float64), np.asarray(d, np.float64)
    return np.exp(lobes[:, 0] * (d @ lobes[:, 1:].T - 1.0)) / lobes.shape[0]


def view_basis(tree, vdir, lobes=None, dtype=f32):
    """The [K] basis a ray is shaded with: SH without lobes, else SG; float32, or for dtype float64 the SG basis in double."""
    basis_dim = (tree.data_dim - 1) // 3
    if lobes is None:
        return sh_basis_np(basis_dim, vdir)
    assert np.asarray(lobes).shape == (basis_dim, 4)
    return sg_basis_np(lobes, vdir) if dtype == f32 else sg_basis_f64(lobes, np.asarray(vdir, f32))


# -- ray set-up --------------------------------------------------------------------------------
def cam2world_ray(ix, iy, c2w, W, H, fx, fy):
    """svox cam2world_ray: pixel centres at integer coordinates, -z forward (same convention as
    generate_rays, nerf_sh/nerf/utils.py:567-588); returns (origin, unit direction)."""
    c2w = np.asarray(c2w, f32)
    x = f32((f32(ix) - f32(0.5) * f32(W)) / f32(fx))
    y = f32(-(f32(iy) - f32(0.5) * f32(H)) / f32(fy))
    z = f32(np.sqrt(f32(f32(x * x) + f32(y * y)) + f32(1.0)))
    x = f32(x / z); y = f32(y / z); z = f32(f32(-1.0) / z)
    d = np.array([f32(f32(f32(c2w[a, 0] * x) + f32(c2w[a, 1] * y)) + f32(c2w[a, 2] * z)) for a in range(3)], f32)
    return c2w[:3, 3].astype(f32), d


def camera_rays(c2w, W, H, fx, fy=None):
    """World-space (origins, unit directions) float32 [H*W, 3] of cam2world_ray, row-major."""
    fy = fx if fy is None else fy
    rays = [cam2world_ray(ix, iy, c2w, W, H, fx, fy) for iy in range(H) for ix in range(W)]
    return np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])


# -- NDC (include/plenoctree_octree.h items 2, 3 and 5; `ndc` is any record with width / height / focal / near); pinned to
# the reference's own convert_to_ndc by tests/golden/octree_ndc.npz (tests/test_octree_ndc_cpu.py) -------------------------
def convert_to_ndc_f32(o, d, ndc):
    """Item 2: (o', d') of convert_to_ndc, float32, one rounding per operation, before the normalisation."""
    o = [f32(v) for v in o]
    d = [f32(v) for v in d]
    near, focal = f32(ndc.near), f32(ndc.focal)
    with np.errstate(all="ignore"):
        t = f32(f32(-f32(near + o[2])) / d[2])
        o = [f32(o[a] + f32(t * d[a])) for a in range(3)]
        cw = f32(f32(f32(2.0) * focal) / f32(ndc.width))
        ch = f32(f32(f32(2.0) * focal) / f32(ndc.height))
        ox_oz, oy_oz = f32(o[0] / o[2]), f32(o[1] / o[2])
        no = [f32(f32(-cw) * ox_oz), f32(f32(-ch) * oy_oz), f32(f32(1.0) + f32(f32(f32(2.0) * near) / o[2]))]
        nd = [f32(f32(-cw) * f32(f32(d[0] / d[2]) - ox_oz)), f32(f32(-ch) * f32(f32(d[1] / d[2]) - oy_oz)),
              f32(f32(f32(-2.0) * near) / o[2])]
    return np.array(no, f32), np.array(nd, f32)


def ndc_ray(o, d, ndc):
    """Items 2, 3 and 5: (o', unit d', hit).  A miss: d_z >= 0, a non-finite component, or a direction without a length."""
    no, nd = convert_to_ndc_f32(o, d, ndc)
    with np.errstate(all="ignore"):
        n = f32(np.sqrt(f32(f32(f32(nd[0] * nd[0]) + f32(nd[1] * nd[1])) + f32(nd[2] * nd[2]))))
        ok = bool(f32(d[2]) < 0) and bool(np.isfinite(no).all()) and bool(np.isfinite(nd).all()) and bool(n > 0) and \
            bool(np.isfinite(n))
        unit = np.array([f32(nd[a] / n) for a in range(3)], f32)
    return no, unit, ok


def _dda_unit(cen, invdir):
    tmin, tmax = f32(0.0), f32(1e9)
    for a in range(3):
        t1 = f32(-cen[a] * invdir[a])
        t2 = f32(t1 + invdir[a])
        tmin = max(tmin, min(t1, t2))
        tmax = min(tmax, max(t1, t2))
    return f32(tmin), f32(tmax)


def _to_tree_ray(origin, direction, offset, invradius):
    o = np.array([f32(offset[a] + f32(invradius[a] * origin[a])) for a in range(3)], f32)
    d = np.array([f32(direction[a] * invradius[a]) for a in range(3)], f32)
    nrm = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
    delta_scale = f32(f32(1.0) / nrm)
    d = (d * delta_scale).astype(f32)
    invdir = (f32(1.0) / (d + f32(1e-9)).astype(f32)).astype(f32)
    return o, d, invdir, delta_scale


# -- the footprint cap (include/plenoctree_octree.h, "footprint") ---------------------------------------------------------
def cap_of(f, min_depth=0):
    """clamp(126 - (bits(f) >> 23), min_depth, MAX_DEPTH): the smallest depth d with 2^-(d+1) <= f, from the exponent field."""
    e = int(np.array(f, f32).view(np.uint32) >> np.uint32(23))
    return max(int(min_depth), min(126 - e, MAX_DEPTH))


def launch_g(cone, invradius):
    """g = fl(cone * min(invradius)), once per launch."""
    return f32(f32(cone) * f32(min(f32(v) for v in invradius)))


def tree_view(child, offset, invradius):
    """A Tree that holds a structure and a transform only: what `march` reads."""
    t = Tree.__new__(Tree)
    t.child, t.offset, t.invradius = np.asarray(child).reshape(-1, N, N, N), offset, invradius
    return t


class March:
    """The sample sequence of one ray that meets the volume.  delta_scale; guard: the kernels' `!(tn > t)` stop ended the march
    (a step below the resolution of t); per sample, as arrays: flat = node * 8 + cell of the cell the descent stopped at, t and
    delta = the sample's own parameter and step (tree units, float32), dtw = fl(delta * delta_scale), depth.  Marched with a
    footprint also cap, has_child (the cap stopped the descent above a leaf) and pos (the clamped position, [n,3])."""

    def __len__(self):
        return len(self.flat)


def march(tree, origin, direction, step_size, ndc=None, foot=None):
    """svox trace_ray's sample sequence, all float32, one rounding per operation: None for a ray that misses the volume, else
    a March.  tree: a Tree or (child, offset, invradius).  ndc: the world ray is converted first (ndc_ray); one that cannot be
    converted is a miss.  foot = (cone, min_depth): the descent also stops at the depth the sample's footprint allows,
    cap_of(fl(t * fl(delta_scale * g)), min_depth).  The twin descends from the root for every sample: it has no path to
    reuse, so it cannot share the kernels' trap."""
    if not isinstance(tree, Tree):
        tree = tree_view(*tree)
    if ndc is not None:
        origin, direction, hit = ndc_ray(origin, direction, ndc)
        if not hit:
            return None
    step = f32(step_size)
    with np.errstate(over="ignore"):             # a ray converted to 1e37 overflows the slab test to inf: a plain miss
        o, d, invdir, delta_scale = _to_tree_ray(origin, direction, tree.offset, tree.invradius)
        tmin, tmax = _dda_unit(o, invdir)
        if tmax < 0 or tmin > tmax:
            return None
        k = None if foot is None else f32(delta_scale * launch_g(foot[0], tree.invradius))
        m = March()
        m.delta_scale, m.guard = delta_scale, False
        flat, ts, deltas, depths, caps, poss = [], [], [], [], [], []
        t = tmin
        while t < tmax:
            pos = np.array([f32(o[a] + f32(t * d[a])) for a in range(3)], f32)
            cap = None if foot is None else cap_of(f32(t * k), foot[1])
            n, i, j, kk, cube, local, depth = tree.find(pos, cap)
            s0, s1 = _dda_unit(local, invdir)
            delta = f32(f32(f32(s1 - s0) / cube) + step)
            flat.append(((n * 2 + i) * 2 + j) * 2 + kk); ts.append(t); deltas.append(delta); depths.append(depth)
            if foot is not None:
                caps.append(cap); poss.append(pos)
            tn = f32(t + delta)
            if not tn > t:
                m.guard = True
                break
            t = tn
    m.flat, m.depth = np.array(flat, np.int64), np.array(depths, np.int64)
    m.t, m.delta = np.array(ts, f32), np.array(deltas, f32)
    m.dtw = (m.delta * delta_scale).astype(f32)
    if foot is not None:
        m.cap = np.array(caps, np.int64)
        m.has_child = tree.child.reshape(-1)[m.flat] != 0
        m.pos = np.clip(np.array(poss, f32).reshape(-1, 3), f32(0.0), f32(1.0 - 1e-6)).astype(f32)
    return m


def march_tree(tree, origin, direction, opt):
    """Sample sequence of svox trace_ray: list of (flat leaf index, dt_world), None for a miss."""
    m = march(tree, origin, direction, opt.step_size)
    return None if m is None else list(zip(m.flat.tolist(), m.dtw))


class Rendered:
    """One composited ray.  rgb[3] (None without a basis); alpha, depth, surface (include/plenoctree_octree.h, aux); light = the
    transmittance left when the march ended (before any rescale); stopped = the early stop ended it; used = the samples
    looked at up to there; s_max = the largest sample distance among them (0 without any).  With a surface_thresh: pick =
    index (into the march) of the sample that set `surface`, -1 if none; light_at_pick = the transmittance after it; margin =
    the smallest |light - surface_thresh| / surface_thresh over the transmittances after every shaded sample (inf without any).
    Per sample, [n]: shaded (sigma > sigma_thresh, before the stop), weight and light_in (the transmittance on arrival) in
    the compositing dtype, 0 and 1 where not shaded."""


def composite(rows, marched, basis, opt, dtype=f32, surface_thresh=None):
    """svox trace_ray's compositing over a March (None: the ray sees the background), with the sums of
    pxo_octree_render_aux_fwd.  rows: [n_cells, D] float32; basis: [K], SH or SG, the caller's choice (None: weights only).
      float32  operation by operation in the kernels' order, one rounding each:
                 att = exp(-dtw sigma), w = light (1 - att), logit_c = sum_q basis_q coef_cq (q ascending from 0),
                 out_c += w sigmoid(logit_c), alpha += w, s = (t + 0.5 delta) delta_scale, depth += w s, light *= att;
                 once light <= stop_thresh: everything times 1 / (1 - light) and the march ends.
      float64  the same float32 samples composited in double, the logit summed in the same order: the yardstick for how
               much of a difference is float32 round-off.  The step is the sample's float32 dtw, as march_tree hands it
               out; with a surface_thresh (the aux definition, whose samples are t_i and delta_i) it is delta delta_scale
               in double."""
    R = Rendered()
    one, bg = dtype(1.0), dtype(opt.background_brightness)
    R.stopped, R.used, R.s_max, R.pick, R.light_at_pick, R.margin = False, 0, 0.0, -1, None, np.inf
    R.alpha, R.depth, R.surface, R.light = dtype(0.0), dtype(0.0), dtype(np.inf), one
    n = 0 if marched is None else len(marched)
    R.shaded, R.weight, R.light_in = np.zeros(n, bool), np.zeros(n, dtype), np.ones(n, dtype)
    if marched is None:
        R.rgb = None if basis is None else np.full(3, bg, dtype)
        return R
    delta_scale = dtype(marched.delta_scale)
    delta = marched.delta.astype(dtype)
    s = (marched.t.astype(dtype) + dtype(0.5) * delta) * delta_scale
    dtw = marched.dtw.astype(dtype) if surface_thresh is None else delta * delta_scale
    val = rows[marched.flat]
    live = np.nonzero(val[:, -1] > opt.sigma_thresh)[0]
    att = np.exp(-dtw[live] * val[live, -1].astype(dtype))
    if basis is not None:
        K = basis.shape[0]
        coef, b = val[live, :-1].reshape(-1, 3, K).astype(dtype), basis.astype(dtype)
        logit = np.zeros((len(live), 3), dtype)
        for q in range(K):
            logit = logit + b[q] * coef[:, :, q]
        col = one / (one + np.exp(-logit))
    thresh = None if surface_thresh is None else dtype(f32(surface_thresh))
    out, light, alpha, depth = np.zeros(3, dtype), one, dtype(0.0), dtype(0.0)
    R.used = n
    for j, i in enumerate(live):
        weight = light * (one - att[j])
        R.shaded[i], R.weight[i], R.light_in[i] = True, weight, light
        if basis is not None:
            out = out + weight * col[j]
        alpha = alpha + weight
        depth = depth + weight * s[i]
        light = light * att[j]
        if thresh is not None:
            R.margin = min(R.margin, abs(float(light) - float(thresh)) / float(thresh))
            if light <= thresh and R.pick < 0:
                R.surface, R.pick, R.light_at_pick = s[i], int(i), float(light)
        if light <= opt.stop_thresh:
            R.stopped, R.used = True, int(i) + 1
            break
    R.light = light
    R.s_max = float(s[:R.used].max()) if R.used else 0.0
    if R.stopped:
        scale = one / (one - light)
        R.rgb, R.alpha, R.depth = out * scale, alpha * scale, depth * scale
    else:
        R.rgb, R.alpha, R.depth = out + light * bg, alpha, depth
    if basis is None:
        R.rgb = None
    return R


class Batch:
    """Per-ray results stacked: rgb [n,3], aux [n,3] = (alpha, depth, surface), light, stopped, pick, light_at_pick (nan
    where nothing was picked), margin [n]; s_max = the largest sample distance over all rays."""

    def __init__(self, rays):
        self.rgb = np.stack([x.rgb for x in rays])
        self.aux = np.stack([np.array([x.alpha, x.depth, x.surface], self.rgb.dtype) for x in rays])
        self.light = np.array([x.light for x in rays])
        self.stopped = np.array([x.stopped for x in rays])
        self.pick = np.array([x.pick for x in rays])
        self.light_at_pick = np.array([np.nan if x.light_at_pick is None else x.light_at_pick for x in rays])
        self.margin = np.array([x.margin for x in rays])
        self.s_max = max(x.s_max for x in rays)


def composite_batches(rows, marches, bases, opt, surface_thresh=0.5):
    """(float32 Batch, float64 Batch) of the marches of a ray set; bases: one [K] basis per ray."""
    return tuple(Batch([composite(rows, m, b, opt, dtype, surface_thresh) for m, b in zip(marches, bases)])
                 for dtype in (f32, np.float64))


def surface_excluded(b32, b64, surface_thresh=0.5):
    """Rays left out of the surface comparison: the float64 transmittance after the chosen sample lies within a relative
    1e-4 of the threshold, or the two precisions already choose different samples."""
    near = np.abs(b64.light_at_pick - surface_thresh) <= 1e-4 * surface_thresh        # nan (no pick) compares False
    return near | (b32.pick != b64.pick)


def render_ray(tree, origin, direction, vdir, opt, want_samples=False, lobes=None, ndc=None, dtype=f32):
    """svox trace_ray: returns rgb[3].  SH format, or SG with `lobes`; with `ndc` the ray is marched in NDC and shaded with
    the world-space vdir; dtype float64 composites the same float32 sample sequence in double."""
    m = march(tree, origin, direction, opt.step_size, ndc=ndc)
    return composite(tree.data.reshape(-1, tree.data_dim), m, view_basis(tree, vdir, lobes, dtype), opt, dtype).rgb


def render_rays(tree, origins, dirs, vdirs, opt, **kw):
    return np.stack([render_ray(tree, o, d, v, opt, **kw) for o, d, v in
                     zip(np.asarray(origins, f32), np.asarray(dirs, f32), np.asarray(vdirs, f32))])


def render_persp(tree, c2w, W, H, fx, opt, fy=None, **kw):
    o, d = camera_rays(c2w, W, H, fx, fy)
    return render_rays(tree, o, d, d, opt, **kw).reshape(H, W, 3)


def render_rays_torch(tree, data, origins, dirs, vdirs, opt, dtype=torch.float64, lobes=None, ndc=None, marches=None):
    """Differentiable (w.r.t. `data`, a torch tensor shaped like tree.data) compositing over the sample sequences of
    `march`, in `dtype`.  No early stop (training uses stop_thresh = 0).  SH, or SG with `lobes`; `ndc` as in march: a ray
    that cannot be converted is the constant background.  marches: the rays' March records (None for a miss) where the
    caller has them already -- they depend on the tree's structure, never on `data`."""
    basis_dim = (tree.data_dim - 1) // 3
    flat = data.reshape(-1, tree.data_dim).to(dtype)
    origins, dirs, vdirs = np.asarray(origins, f32), np.asarray(dirs, f32), np.asarray(vdirs, f32)
    if marches is None:
        marches = [march(tree, o, d, opt.step_size, ndc=ndc) for o, d in zip(origins, dirs)]
    outs = []
    for m, v in zip(marches, vdirs):
        bg = float(opt.background_brightness)
        if m is None:
            outs.append(torch.full((3,), bg, dtype=dtype))
            continue
        idx = torch.from_numpy(m.flat)
        dtw = torch.from_numpy(m.dtw.astype(np.float64)).to(dtype)
        val = flat[idx]
        sigma = val[:, -1]
        live = sigma > float(opt.sigma_thresh)
        att = torch.where(live, torch.exp(-dtw * sigma), torch.ones_like(sigma))
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=dtype), att]), 0)
        w = T[:-1] * (1.0 - att)
        basis = sh_basis_np(basis_dim, v).astype(np.float64) if lobes is None else sg_basis_f64(lobes, v)
        basis = torch.tensor(basis, dtype=dtype)
        rgb = torch.sigmoid((val[:, :-1].reshape(-1, 3, basis_dim) * basis).sum(-1))
        outs.append((w[:, None] * rgb).sum(0) + T[-1] * bg)
    return torch.stack(outs)


def grid_march(sigma_grid, c2w, W, H, fx, opt, offset, invradius, fy=None, ndc=None):
    """The march of svox _C.grid_weight_render over a dense reso^3 grid: for every ray of the camera that meets the volume
    (in NDC with `ndc`), row-major, (voxels [n,3] of the samples it takes, indices of the shaded ones among them, their
    compositing weights, float32).  The early stop ends a ray after the sample that reaches it."""
    fy = fx if fy is None else fy
    cube = f32(sigma_grid.shape[0])
    for iy in range(H):
        for ix in range(W):
            origin, direction = cam2world_ray(ix, iy, c2w, W, H, fx, fy)
            if ndc is not None:
                origin, direction, hit = ndc_ray(origin, direction, ndc)
                if not hit:
                    continue
            o, d, invdir, delta_scale = _to_tree_ray(origin, direction, offset, invradius)
            tmin, tmax = _dda_unit(o, invdir)
            if tmax < 0 or tmin > tmax:
                continue
            voxels, shaded, weights = [], [], []
            t, light = tmin, f32(1.0)
            while t < tmax:
                pos = np.array([f32(o[a] + f32(t * d[a])) for a in range(3)], f32)
                pos = np.clip(pos, f32(0.0), f32(1.0 - 1e-6)).astype(f32)
                pos = (pos * cube).astype(f32)
                u = np.floor(pos).astype(np.int64)
                local = (pos - u.astype(f32)).astype(f32)
                s0, s1 = _dda_unit(local, invdir)
                delta_t = f32(f32(f32(s1 - s0) / cube) + opt.step_size)
                sigma = sigma_grid[u[0], u[1], u[2]]
                voxels.append(u)
                if sigma > opt.sigma_thresh:
                    att = f32(np.exp(f32(-f32(delta_t * delta_scale) * sigma), dtype=f32))
                    shaded.append(len(voxels) - 1); weights.append(f32(light * f32(f32(1.0) - att)))
                    light = f32(light * att)
                    if light <= opt.stop_thresh:
                        break
                t = f32(t + delta_t)
            yield np.array(voxels, np.int64).reshape(-1, 3), np.array(shaded, np.int64), np.array(weights, f32)


def grid_weight_render(sigma_grid, c2w, W, H, fx, opt, offset, invradius, fy=None, weight=None, ndc=None):
    """svox _C.grid_weight_render: per-voxel maximum compositing weight over the rays of one camera."""
    weight = np.zeros_like(sigma_grid, dtype=f32) if weight is None else weight
    for voxels, shaded, w in grid_march(sigma_grid, c2w, W, H, fx, opt, offset, invradius, fy, ndc):
        np.maximum.at(weight, tuple(voxels[shaded].T), w)
    return weight
