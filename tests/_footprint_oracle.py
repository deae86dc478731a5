"""CPU twin of the footprint render (pxo_octree_render_foot_fwd / _foot_aux_fwd; the definition: include/plenoctree_octree.h,
"footprint"), in numpy float32, one rounding per operation.  TEST INFRASTRUCTURE, shared by tests/test_footprint_cpu.py and
tests/test_gpu_footprint.py.

`march` is octree_oracle.march_tree's loop (its _to_tree_ray and _dda_unit, Tree.query's iterated doubling with a depth
counter) in which the descent also stops at the depth the sample's footprint allows; `composite` composites a sample list in
the arithmetic of octree_oracle.render_ray, with the aux sums of tests/_octree_aux_oracle.py, for the SH or the SG basis;
`reuse_counts` replays the kernel's integer path reuse over the twin's samples and counts the situations the tests must not
miss.  The twin descends from the root for every sample: it has no path to reuse, so it cannot share the kernel's trap.
"""
import numpy as np

from oracle import octree_oracle as T

f32 = np.float32
MAX_DEPTH = 10                                   # PXO_TREE_MAX_DEPTH
BITS = MAX_DEPTH + 1                             # bits per axis of the kernel's quantised position


def cap_of(f, min_depth=0):
    """clamp(126 - (bits(f) >> 23), min_depth, MAX_DEPTH): the smallest depth d with 2^-(d+1) <= f, from the exponent field."""
    e = int(np.array(f, f32).view(np.uint32) >> np.uint32(23))
    return max(int(min_depth), min(126 - e, MAX_DEPTH))


def launch_g(cone, invradius):
    """g = fl(cone * min(invradius)), once per launch."""
    return f32(f32(cone) * f32(min(f32(v) for v in invradius)))


def query_capped(child, p_tree, cap):
    """Tree.query with a depth counter: (node, cell, depth, cube, local) of the first cell with child == 0 or depth >= cap."""
    x = np.clip(np.asarray(p_tree, f32), f32(0.0), f32(1.0 - 1e-6)).astype(f32)
    node, depth, cube = 0, 0, f32(2.0)
    while True:
        x = (x * f32(2.0)).astype(f32)
        u = np.floor(x).astype(np.int64)
        x = (x - u.astype(f32)).astype(f32)
        cell = int((u[0] * 2 + u[1]) * 2 + u[2])
        skip = int(child[node * 8 + cell])
        if skip == 0 or depth >= cap:
            return node, cell, depth, cube, x
        cube = f32(cube * f32(2.0))
        node += skip
        depth += 1


class Sample:
    """flat = node * 8 + cell of the cell the descent stopped at; t, delta: the sample's own parameter and step (tree units);
    dtw = fl(delta * delta_scale); depth, cap; has_child: the cap stopped the descent above a leaf; pos: the clamped position."""
    __slots__ = ("flat", "t", "delta", "dtw", "depth", "cap", "has_child", "pos")


def march(child, offset, invradius, origin, direction, step_size, cone, min_depth=0):
    """None for a ray that misses the volume, else (samples, delta_scale).  child: int32, any shape with 8 cells per node."""
    child = np.asarray(child).reshape(-1)
    o, d, invdir, delta_scale = T._to_tree_ray(origin, direction, offset, invradius)
    tmin, tmax = T._dda_unit(o, invdir)
    if tmax < 0 or tmin > tmax:
        return None
    k = f32(delta_scale * launch_g(cone, invradius))
    out, t = [], tmin
    while t < tmax:
        pos = np.array([f32(o[a] + f32(t * d[a])) for a in range(3)], f32)
        cap = cap_of(f32(t * k), min_depth)
        node, cell, depth, cube, local = query_capped(child, pos, cap)
        s0, s1 = T._dda_unit(local, invdir)
        s = Sample()
        s.flat, s.t, s.depth, s.cap = node * 8 + cell, f32(t), depth, cap
        s.delta = f32(f32(f32(s1 - s0) / cube) + f32(step_size))
        s.dtw = f32(s.delta * delta_scale)
        s.has_child = bool(child[s.flat] != 0)
        s.pos = np.clip(pos, f32(0.0), f32(1.0 - 1e-6)).astype(f32)
        out.append(s)
        tn = f32(t + s.delta)
        if not tn > t:                           # the kernels' guard: a step below the resolution of t ends the march
            break
        t = tn
    return out, delta_scale


def reuse_counts(marched):
    """Replays Marcher::find's integer path reuse over one ray's samples: (samples, cap-stopped samples -- the descent ended
    at a cell that has a child --, clamp cases -- min(common, last_depth) > cap, where resuming from the previous path
    without the clamp by cap would start below the cap --, whether the cap takes more than one value on the ray)."""
    if marched is None:
        return 0, 0, 0, False
    samples, _ = marched
    stopped = clamp = 0
    prev, last_depth = None, 0
    for s in samples:
        q = tuple(int(f32(c * f32(1 << BITS))) for c in s.pos)       # exact: a power of two; >= 0, so int() is the floor
        if prev is not None:
            diff = (q[0] ^ prev[0]) | (q[1] ^ prev[1]) | (q[2] ^ prev[2])
            common = BITS - diff.bit_length()                          # leading bit-levels shared
            clamp += min(common, last_depth) > s.cap
        stopped += s.has_child
        prev, last_depth = q, s.depth
    return len(samples), stopped, clamp, len({s.cap for s in samples}) > 1


def case_counts(rays_marched):
    """The per-case figures: dict(samples, cap_stopped, clamp_cases, rays_changing_cap) over the marches of a ray set."""
    tot = np.zeros(4, np.int64)
    for m in rays_marched:
        tot += np.array(reuse_counts(m), np.int64)
    return dict(samples=int(tot[0]), cap_stopped=int(tot[1]), clamp_cases=int(tot[2]), rays_changing_cap=int(tot[3]))


class RayOut:
    """rgb[3]; alpha, depth, surface; pick: index of the sample that set surface (-1: none); light_at_pick; s_max."""


def composite(data, marched, basis, opt, surface_thresh=0.5, dtype=np.float32):
    """octree_oracle.render_ray's compositing over `marched` (float32: operation by operation; float64: the same float32
    samples composited in double, the yardstick for the surface comparison), with the aux sums of pxo_octree_render_aux_fwd.
    data: [n_cells, D] rows (the device's own filled rows); basis: float32 [K], SH or SG."""
    R = RayOut()
    bg = opt.background_brightness
    R.pick, R.light_at_pick, R.s_max = -1, None, 0.0
    if marched is None:
        R.rgb = np.full(3, bg, dtype)
        R.alpha, R.depth, R.surface = dtype(0.0), dtype(0.0), dtype(np.inf)
        return R
    samples, delta_scale = marched
    K = basis.shape[0]
    exact = dtype == np.float32
    r = (lambda x: f32(x)) if exact else (lambda x: np.float64(x))
    out, light = np.zeros(3, dtype), dtype(1.0)
    alpha, depth, surface = dtype(0.0), dtype(0.0), dtype(np.inf)
    thresh = dtype(f32(surface_thresh))
    for i, smp in enumerate(samples):
        val = data[smp.flat]
        sigma = val[-1]
        s = r(r(r(smp.t) + r(dtype(0.5) * r(smp.delta))) * r(delta_scale))
        R.s_max = max(R.s_max, float(s))
        if sigma > opt.sigma_thresh:
            dtw = r(r(smp.delta) * r(delta_scale))
            att = r(np.exp(r(-dtw * r(sigma)), dtype=dtype))
            weight = r(light * r(dtype(1.0) - att))
            coef = val[:-1].reshape(3, K)
            if exact:
                tmp = np.zeros(3, f32)
                for q in range(K):
                    tmp = (tmp + (basis[q] * coef[:, q]).astype(f32)).astype(f32)
                col = T._sigmoid(tmp)
            else:
                col = 1.0 / (1.0 + np.exp(-(coef.astype(np.float64) @ basis.astype(np.float64))))
            out = (out + (weight * col).astype(dtype)).astype(dtype)
            alpha = r(alpha + weight)
            depth = r(depth + r(weight * s))
            light = r(light * att)
            if light <= thresh and R.pick < 0:
                surface, R.pick, R.light_at_pick = s, i, float(light)
            if light <= opt.stop_thresh:
                scale = r(dtype(1.0) / r(dtype(1.0) - light))
                R.rgb = (out * scale).astype(dtype)
                R.alpha, R.depth, R.surface = r(alpha * scale), r(depth * scale), surface
                return R
    R.rgb = (out + r(light * dtype(bg))).astype(dtype)
    R.alpha, R.depth, R.surface = alpha, depth, surface
    return R


class Batch:
    """Stacked per-ray results: rgb [n,3], aux [n,3] = (alpha, depth, surface), pick, light_at_pick (nan: none), s_max."""

    def __init__(self, rays):
        self.rgb = np.stack([x.rgb for x in rays])
        self.aux = np.stack([np.array([x.alpha, x.depth, x.surface], self.rgb.dtype) for x in rays])
        self.pick = np.array([x.pick for x in rays])
        self.light_at_pick = np.array([np.nan if x.light_at_pick is None else x.light_at_pick for x in rays])
        self.s_max = max(x.s_max for x in rays)


def render(data, marches, bases, opt, surface_thresh=0.5):
    """(float32 Batch, float64 Batch) of the marches of a ray set; bases: one float32 [K] basis per ray."""
    both = [(composite(data, m, b, opt, surface_thresh, np.float32), composite(data, m, b, opt, surface_thresh, np.float64))
            for m, b in zip(marches, bases)]
    return Batch([x[0] for x in both]), Batch([x[1] for x in both])


def surface_excluded(b32, b64, surface_thresh=0.5):
    """tests/_octree_aux_oracle.surface_excluded: rays whose float64 transmittance after the chosen sample lies within a
    relative 1e-4 of the threshold, or where the two precisions choose different samples."""
    near = np.abs(b64.light_at_pick - surface_thresh) <= 1e-4 * surface_thresh
    return near | (b32.pick != b64.pick)
