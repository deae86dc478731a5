"""Deep, sparse octrees and the ray sets that reach their deep leaves: case builders shared by
tests/test_octree_cases_cpu.py (coverage conditions, oracle only) and tests/test_gpu_octree_depth.py (HIP vs oracle).

Everything here is oracle/octree_oracle.py plus numpy: no GPU, no dense mask (a depth-10 mask would be 2048^3), every
case generated from a seed.  Trees are built with Tree.refine_at / refine_leaves and stay at a few thousand nodes so
that the Python oracle marches them in seconds.

Volume: center (0.5, 0, 0.5), radius (1, 2, 1) -> offset (0.25, 0.5, 0.25), invradius (0.5, 0.25, 0.5): exact powers of
two and anisotropic, so world points with dyadic tree coordinates (cell faces, the plane x_tree = 0.5, the volume's
corners) are representable exactly.  "Depth" of a leaf is the depth of the node that holds it (parent_depth[:, 1]), the
quantity the kernels' Marcher::find counts: the finest cells of a depth-d tree have side 2^-(d+1).
"""
import functools

import numpy as np

from oracle import octree_oracle as T

f32 = np.float32
CENTER = (0.5, 0.0, 0.5)
RADIUS = (1.0, 2.0, 1.0)
DEPTHS = (6, 8, 10)
FAMILIES = ("shell", "rod", "chunked")
# rod end points (tree coordinates): an almost full space diagonal, |dx| + |dy| + |dz| = 2.65, so the line crosses about
# 2.65 * 2^(depth+1) finest cells (depth 8: ~1350, depth 10: ~5400; a straight line cannot cross more than 3 * 2^(depth+1))
ROD_A = np.array([0.04, 0.07, 0.09])
ROD_B = np.array([0.96, 0.93, 0.94])
ROD2_A = np.array([0.9, 0.12, 0.3])
ROD2_B = np.array([0.15, 0.8, 0.35])
ROD_STEP = 1e-4            # the production renderer step (1e-3 would step over two finest cells of a depth-10 tree)


def new_tree(K, depth):
    t = T.Tree(3 * K + 1, depth, CENTER, RADIUS)
    assert np.array_equal(t.offset, np.array([0.25, 0.5, 0.25], f32))
    assert np.array_equal(t.invradius, np.array([0.5, 0.25, 0.5], f32))
    return t


def tree2world(t, p_tree):
    """World coordinates (float64) of tree-coordinate points; exact for dyadic p_tree."""
    return (np.asarray(p_tree, np.float64) - t.offset.astype(np.float64)) / t.invradius.astype(np.float64)


def leaf_depths(t):
    """Depth of every cell's node, shaped like t.child (meaningful where child == 0)."""
    return np.broadcast_to(t.parent_depth[:, 1][:, None, None, None], t.child.shape)


def leaf_set(t):
    """The tree's geometry, independent of node order: {(x, y, z, depth)} with integer corners on the 2^-(depth+1) grid."""
    lv = t.leaves()
    corner, side = T.leaf_corners(t, lv)
    d = t.parent_depth[lv[:, 0], 1]
    ijk = np.rint(corner / side[:, None]).astype(np.int64)
    return set(map(tuple, np.concatenate([ijk, d[:, None]], 1).tolist()))


# -- trees -------------------------------------------------------------------------------------------------------
def _shell_points(n, seed):
    rs = np.random.RandomState(seed)
    v = rs.randn(n, 3)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return 0.5 + v * (0.31 + 0.004 * rs.randn(n, 1)) * np.array([1.0, 1.1, 0.9])


def _round_sizes(depth, n_first=150, n_last=40):
    return [int(round(n_first * (n_last / n_first) ** (r / max(depth - 1, 1)))) for r in range(depth)]


def _refine_rounds(t, pts_tree, sizes, last_chunks=1):
    world = tree2world(t, pts_tree).astype(f32)
    for r, m in enumerate(sizes):
        if r == len(sizes) - 1 and last_chunks > 1:
            for c in range(last_chunks):                 # interleaved chunks: parents of one chunk lie between the other's
                t.refine_at(world[:m][c::last_chunks])
        else:
            t.refine_at(world[:m])


def fill_data(t, seed, sigma_scale):
    """Random SH coefficients; sigma: 35 % of the cells empty (<= 0), the rest scaled with 2^depth so that one cell crossing
    has an optical depth of about sigma_scale whatever the cell's size: transmittance survives to the deepest leaves."""
    rs = np.random.RandomState(seed)
    t.data[:] = (rs.randn(*t.data.shape) * 0.7).astype(f32)
    u = rs.rand(*t.child.shape) - 0.35
    t.data[..., -1] = (u * sigma_scale * 2.0 ** (leaf_depths(t) + 1)).astype(f32)
    return t


def shell(depth, K, seed=0):
    """Points on a thin ellipsoidal shell; round r refines at the first n_r of them with n_r shrinking 150 -> 40, so the
    leaves that drop out of the subset stay behind at every depth 1..depth."""
    t = new_tree(K, depth)
    _refine_rounds(t, _shell_points(150, seed), _round_sizes(depth))
    return fill_data(t, seed + 1000 * K + depth, 0.12)


def chunked(depth, K, seed=0, chunks=3):
    """shell's geometry with the last level appended in `chunks` separate refine calls (extraction's "last layer in
    chunks"): that level's nodes are not in packed-parent order."""
    t = new_tree(K, depth)
    _refine_rounds(t, _shell_points(150, seed), _round_sizes(depth), last_chunks=chunks)
    return fill_data(t, seed + 1000 * K + depth + 7, 0.12)


def _segment_points(a, b, depth_now):
    """Points on the segment a-b, four per finest-cell width at this level."""
    n = int(4 * 2 ** (depth_now + 1) * np.abs(b - a).sum()) + 2
    s = np.linspace(0.0, 1.0, n)[:, None]
    return a + s * (b - a)


def rod(depth, K, seed=0):
    """Refined to full depth along two line segments: a ray along the first stays in deepest-level leaves for its whole
    length, and the quantised position changes its leading bits at every level on the way."""
    t = new_tree(K, depth)
    for r in range(depth):
        pts = np.concatenate([_segment_points(ROD_A, ROD_B, r), _segment_points(ROD2_A, ROD2_B, r)])
        cells = np.unique(np.floor(pts * 2 ** (r + 1)).astype(np.int64), axis=0)      # one point per cell of this level
        t.refine_at(tree2world(t, (cells + 0.5) / 2 ** (r + 1)).astype(f32))
    # the cells whose corner the line only clips are still coarse: refine whatever the axis rays themselves sample between
    # the rod's ends until all of it is at full depth, so that the run of deepest-level samples is unbroken
    opt = T.RenderOptions(ROD_STEP)
    lo, hi = np.minimum(ROD_A, ROD_B) + 0.01, np.maximum(ROD_A, ROD_B) - 0.01
    for _ in range(3 * depth):
        shallow = set()
        for o, d in zip(*rod_axis_rays(t)):
            for leaf, _dt in T.march_tree(t, o, d, opt):
                if t.parent_depth[leaf // 8, 1] < depth:
                    shallow.add(leaf)
        if shallow:
            lv = np.array([[q // 8, (q >> 2) & 1, (q >> 1) & 1, q & 1] for q in sorted(shallow)])
            corner, side = T.leaf_corners(t, lv)
            inside = ((corner + side[:, None] > lo) & (corner < hi)).all(1)
            shallow = [q for q, ok in zip(sorted(shallow), inside) if ok]
        if not shallow:
            break
        t.refine_leaves(shallow)
    return fill_data(t, seed + 1000 * K + depth + 13, 0.004)


@functools.lru_cache(maxsize=None)
def make_tree(family, depth, K, seed=0):
    return {"shell": shell, "rod": rod, "chunked": chunked}[family](depth, K, seed)


# -- rays --------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def aimed_per_depth(d):
    return 12 if d < 5 else 64


def aimed_rays(t, seed, per_depth=aimed_per_depth):
    """For every leaf depth 1..max: rays from outside the volume through a jittered interior point of leaves of that depth
    (occupied ones where there are any).  Returns (origins, unit dirs) float32."""
    rs = np.random.RandomState(seed)
    lv = t.leaves()
    dep = t.parent_depth[lv[:, 0], 1]
    corner, side = T.leaf_corners(t, lv)
    sig = t.data[lv[:, 0], lv[:, 1], lv[:, 2], lv[:, 3], -1]
    o, d = [], []
    for depth in range(1, int(dep.max()) + 1):
        cand = np.nonzero(dep == depth)[0]
        occ = cand[sig[cand] > 0]
        cand = occ if occ.size else cand
        for q in rs.choice(cand, per_depth(depth)):
            p = tree2world(t, corner[q] + side[q] * (0.2 + 0.6 * rs.rand(3)))
            v = _unit(rs.randn(3))
            o.append(p - v * (6.0 + rs.rand()))
            d.append(v)
    d = np.asarray(d, f32)
    return np.asarray(o, f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def rod_axis_rays(t):
    """Along the first rod, both ways: origins outside the volume on the rod's line."""
    out_o, out_d = [], []
    for a, b in ((ROD_A, ROD_B), (ROD_B, ROD_A)):
        wa, wb = tree2world(t, a), tree2world(t, b)
        v = _unit(wb - wa)
        out_o.append(wa - 4.0 * v); out_d.append(v)
    d = np.asarray(out_d, f32)
    return np.asarray(out_o, f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def rod_skew_rays(t, seed):
    """Through the rod's midpoint at 1e-3 .. 5e-2 rad to it: they run inside the rod for a while, then through its coarse
    surroundings.  The last ray runs along the second, shorter rod."""
    rs = np.random.RandomState(seed)
    wa, wb = tree2world(t, ROD_A), tree2world(t, ROD_B)
    mid, v = 0.5 * (wa + wb), _unit(wb - wa)
    w2 = _unit(tree2world(t, ROD2_B) - tree2world(t, ROD2_A))
    o, d = [tree2world(t, ROD2_A) - 4.0 * w2], [w2]
    for ang in (1e-3, 3e-3, 1e-2, 2e-2, 5e-2):
        n = _unit(np.cross(v, rs.randn(3)))
        w = _unit(v * np.cos(ang) + n * np.sin(ang))
        o.append(mid - 5.0 * w); d.append(w)
    d = np.asarray(d, f32)
    return np.asarray(o, f32), (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


def look_at(eye, target=CENTER, up=(0.0, 0.0, 1.0)):
    """4x4 camera-to-world matrix, -z forward, as the renderer's cam2world_ray expects."""
    eye = np.asarray(eye, np.float64)
    z = _unit(eye - np.asarray(target, np.float64))
    x = _unit(np.cross(np.asarray(up, np.float64), z))
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m.astype(f32)


# a ragged view (21 x 13 is no multiple of any lane variant's patch) and one with fy != fx
CAMERA_VIEWS = (
    dict(c2w=look_at((3.4, 3.1, 2.6)), W=21, H=13, fx=15.0, fy=15.0),
    dict(c2w=look_at((-2.2, -4.0, 1.9)), W=19, H=14, fx=13.0, fy=17.5),
)


def rod_view(t):
    """A camera on the first rod's line looking along it, 4 x 2 pixels at a focal length of 400: pixel (2, 1) is the
    rod's axis (pixel centres sit at integer coordinates, so its camera-space direction is exactly -z), the others
    leave it at 2.5e-3 .. 5.6e-3 rad.  Meant for ROD_STEP."""
    wa, wb = tree2world(t, ROD_A), tree2world(t, ROD_B)
    v = _unit(wb - wa)
    return dict(c2w=look_at(wa - 4.0 * v, target=wb), W=4, H=2, fx=400.0, fy=400.0)


def pose(theta, phi, radius=4.0):
    from plenoctree_amd.nerf_sh.nerf.datasets import pose_spherical
    return pose_spherical(theta, phi, radius)


def random_tree(depth, seed, K, p=0.15, center=(0.1, 0.0, -0.2), radius=(1.4, 1.5, 1.3)):
    """The shallow dense case of the render tests: a tree from a random mask with random data, about a third of the leaves
    empty (sigma <= 0)."""
    reso = 2 ** (depth + 1)
    mask = np.random.RandomState(seed).rand(reso, reso, reso) < p
    t = T.build_from_mask(mask, depth, 3 * K + 1, center, radius)
    rs = np.random.RandomState(seed + 100)
    t.data[:] = (rs.randn(*t.data.shape) * 0.7).astype(f32)
    t.data[..., -1] = ((rs.rand(*t.data.shape[:-1]) - 0.35) * 12.0).astype(f32)
    return t


EDGE_BACKGROUND = ("corner", "away", "miss")


def edge_rays():
    """(names, origins, dirs, viewdirs): the ray arguments no other test passes.  World volume: x in [-0.5, 1.5],
    y in [-2, 2], z in [-0.5, 1.5].  viewdirs are unit vectors unrelated to dirs."""
    a = f32(1.0 / np.sqrt(5.0))
    cases = [
        ("one_zero", (-2.0, -3.1, 0.3), (0.6, 0.8, 0.0)),
        ("one_zero_neg", (0.7, 3.0, 2.9), (0.0, -0.6, -0.8)),
        ("two_zero_x", (-3.0, 0.37, 0.61), (1.0, 0.0, 0.0)),
        ("two_zero_y", (0.21, 5.0, 0.83), (0.0, -1.0, 0.0)),
        ("two_zero_z", (1.13, -1.7, -2.0), (0.0, 0.0, 1.0)),
        ("inside", (0.4, 0.3, 0.7), (0.48, -0.6, 0.64)),
        ("inside_on_cell_face", (0.5, -1.0, 0.25), (-0.36, 0.48, 0.8)),        # tree (0.5, 0.25, 0.375)
        ("on_boundary", (-0.5, 0.2, 0.4), (0.8, 0.36, 0.48)),                  # x_tree = 0 exactly
        ("on_boundary_axis", (0.3, -2.0, 0.9), (0.0, 1.0, 0.0)),               # y_tree = 0, two zero components
        ("in_plane_x_half", (0.5, -3.0, 0.1), (0.0, 0.96, 0.28)),              # x_tree = 0.5 for every t
        # through the corner (0,0,0)_tree only: tree direction (1,-1,0)/sqrt2, z_tree = 0 -> tmin == tmax, no sample
        ("corner", (-1.5, 0.0, -0.5), (a, -2 * a, 0.0)),
        ("away", (3.0, 0.0, 0.5), (1.0, 0.0, 0.0)),
        ("miss", (-3.0, -6.0, 0.5), (0.25, 0.97, 0.0)),
    ]
    names = [c[0] for c in cases]
    o = np.asarray([c[1] for c in cases], f32)
    d = np.asarray([c[2] for c in cases], np.float64)
    exact = [names.index("corner")]                       # its components are constructed exactly; do not renormalise
    dn = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    dn[exact] = d[exact].astype(f32)
    v = _unit(np.random.RandomState(99).randn(len(cases), 3)).astype(f32)
    return names, o, dn, v


# -- oracle-side measurements ------------------------------------------------------------------------------------
def depth_coverage(t, origins, dirs, opt):
    """Per leaf depth: (samples, samples with sigma > sigma_thresh and transmittance > 1e-2 on arrival), and per ray the
    list of sampled depths."""
    rows = t.data.reshape(-1, t.data_dim)
    nd = t.depth_limit + 1
    samples, live = np.zeros(nd, np.int64), np.zeros(nd, np.int64)
    per_ray = []
    no_stop = T.RenderOptions(opt.step_size, opt.background_brightness, opt.sigma_thresh, 0.0)
    for o, d in zip(origins, dirs):
        m = T.march(t, o, d, opt.step_size)
        if m is None:
            per_ray.append([])
            continue
        r = T.composite(rows, m, None, no_stop, np.float64)
        samples += np.bincount(m.depth, minlength=nd)
        live += np.bincount(m.depth[r.shaded & (r.light_in > 1e-2)], minlength=nd)
        per_ray.append(m.depth.tolist())
    return samples, live, per_ray


def sampled_leaves(t, origins, dirs, opt):
    out = set()
    for o, d in zip(origins, dirs):
        m = T.march(t, o, d, opt.step_size)
        out.update(() if m is None else m.flat.tolist())
    return out


def _node_paths(t):
    """Per node: the nodes from the root down to it (node n sits at depth len(path) - 1)."""
    paths = [[0]]
    for n in range(1, t.n_internal):
        parent = int(t.parent_depth[n, 0]) // 8
        assert parent < n
        paths.append(paths[parent] + [n])
    return paths


def tree_march_counts(t, view, opt):
    """What pxo_octree_count_work counts, from the sample sequence march_tree returns: (counts, child-pointer loads a
    lookup without path reuse would take).

    child_loads is the load count of a descent that restarts at the deepest node of the previous sample's path which
    still contains the new position.  Those nodes exist in the tree and contain the new position, so they are exactly
    the common ancestors of the two samples' nodes: the restart depth follows from the leaf sequence alone, with no
    position arithmetic of the kernel's repeated here.  Sample i in a leaf of depth d_i costs d_i - restart_i + 1 loads
    (restart = 0 for a ray's first sample), against d_i + 1 without reuse."""
    rows = t.data.reshape(-1, t.data_dim)
    paths = _node_paths(t)
    rays = samples = shaded = loads = loads_no_reuse = 0
    leaves = set()
    for o, d in zip(*T.camera_rays(**view)):
        m = T.march(t, o, d, opt.step_size)
        if m is None:
            continue
        r = T.composite(rows, m, None, opt)
        rays += 1
        samples += r.used
        shaded += int(r.shaded.sum())
        leaves.update(m.flat[r.shaded].tolist())
        prev = None
        for leaf in m.flat[:r.used].tolist():
            path = paths[leaf // 8]
            shared = 0 if prev is None else sum(1 for a, b in zip(prev, path) if a == b) - 1
            loads += len(path) - shared
            loads_no_reuse += len(path)
            prev = path
    counts = dict(rays=rays, samples=samples, shaded_samples=shaded, child_loads=loads, distinct_leaves=len(leaves))
    return counts, loads_no_reuse


def far_origin_ray(t, seed=0):
    """A ray from 4e3 world units away aimed at a deepest leaf, step size 1e-7: at t ~ 1e3 .. 2e3 one ulp of t is 1.2e-4, so
    a clipped corner of a fine cell (crossing + step below half an ulp) leaves t + delta_t == t and the march can only end
    by the `!(tn > t)` guard.  Returns (origin, dir, opt, samples) of the first seeded candidate whose guarded oracle march
    ends that way after at least five samples."""
    opt = T.RenderOptions(1e-7)
    lv = t.leaves()
    dep = t.parent_depth[lv[:, 0], 1]
    corner, side = T.leaf_corners(t, lv)
    rs = np.random.RandomState(seed)
    for q in rs.choice(np.nonzero(dep == dep.max())[0], 40):
        p = tree2world(t, corner[q] + 0.5 * side[q])
        v = _unit(rs.randn(3))
        o, d = (p - 4.0e3 * v).astype(f32), v.astype(f32)
        d = (d / np.linalg.norm(d)).astype(f32)
        m = T.march(t, o, d, opt.step_size)
        if m is not None and m.guard and len(m) >= 5:
            return o, d, opt, len(m)
    raise AssertionError("no far-origin candidate reaches the stop guard")


# -- weight mask -------------------------------------------------------------------------------------------------
GRID_SIZES = (10, 13, 20, 96, 128, 256, 1024)
GRID_CAMERAS = np.stack([look_at((3.3, 2.9, 2.7)), look_at((-2.4, -3.6, -1.5))])


def grid_case(reso):
    """(W, H, fx, fy): fy != fx everywhere; ragged and wider than one 16x16 tile, except 10 / 13 where the kernel has no
    tiles to speak of; ~150 rays per camera at 1024 (the oracle takes ~1000 samples per ray there)."""
    if reso == 1024:
        return 17, 9, 12.0, 9.5
    if reso <= 13:
        return 13, 11, 14.0, 11.0
    return 19, 18, 17.0, 14.0


def grid_sigma(reso, seed=0):
    """Up to 256: dense random, 40 % above the threshold (as the existing weight-mask test).  1024: zeros (allocated,
    not drawn) with a six-voxel ellipsoidal shell (the 1e-3 step spans a voxel: a thinner one is mostly stepped over)
    and a few occupied blocks filled in."""
    rs = np.random.RandomState(seed)
    if reso < 1024:
        scale = 30.0 * max(1.0, reso / 64.0)              # keeps the optical depth per voxel as at 64
        return ((rs.rand(reso, reso, reso) - 0.6) * scale).astype(f32)
    sigma = np.zeros((reso, reso, reso), f32)
    ax = (np.arange(reso, dtype=np.float64) + 0.5) / reso - 0.5
    r_yz2 = (ax[:, None] * 1.1) ** 2 + (ax[None, :] * 0.9) ** 2
    for ix in range(reso):
        r = np.sqrt(ax[ix] ** 2 + r_yz2)
        m = np.abs(r - 0.3) < 3.0 / reso
        if m.any():
            sigma[ix][m] = ((rs.rand(int(m.sum())) - 0.3) * 300.0).astype(f32)
    for _ in range(12):
        c = rs.randint(reso // 8, reso - reso // 8 - 48, 3)
        sigma[c[0]:c[0] + 48, c[1]:c[1] + 48, c[2]:c[2] + 48] = ((rs.rand(48, 48, 48) - 0.3) * 300.0).astype(f32)
    return sigma


def grid_march_counts(sigma, cams, W, H, fx, fy, opt, offset, invradius):
    """What pxo_grid_weight_count_work counts, from the sample sequences of the march behind T.grid_weight_render."""
    rays = samples = occ = 0
    seen = set()
    for c in cams:
        for voxels, shaded, _ in T.grid_march(sigma, c, W, H, fx, opt, offset, invradius, fy):
            rays += 1
            samples += len(voxels)
            occ += len(shaded)
            seen.update(map(tuple, voxels[shaded].tolist()))
    return dict(rays=rays, samples=samples, occupied_samples=occ, distinct_voxels=len(seen))
