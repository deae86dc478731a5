"""CPU restatement of the extra outputs of the octree renderer (pxo_octree_render_aux_fwd: alpha, depth, surface), built on
oracle/octree_oracle.py.  TEST INFRASTRUCTURE, shared by tests/test_octree_aux_cpu.py and tests/test_gpu_octree_aux.py.

`march` repeats the loop of `octree_oracle.march_tree` but keeps every sample's own t_i and delta_i (float32, the same
operations in the same order, hence the same sample sequence).  `composite` then follows the definitions of
include/plenoctree_octree.h in a selectable precision:

  float32  mirrors `octree_oracle.render_ray` operation by operation (its rgb is render_ray's bit for bit) and rounds the
           added quantities once per operation, in the order the kernels evaluate them:
             s_i = f32(f32(t_i + f32(0.5 delta_i)) delta_scale),  alpha += w_i,  depth += f32(w_i s_i)
  float64  the same sample sequence (t_i, delta_i, delta_scale and the tree data are the float32 values) composited in
           float64: the yardstick for how much of a difference is float32 round-off.
"""
import numpy as np

from oracle import octree_oracle as T

f32 = np.float32


def march(tree, origin, direction, opt):
    """None for a ray that misses the volume, else (samples, delta_scale) with samples = [(flat leaf index, t_i, delta_i)]."""
    o, d, invdir, delta_scale = T._to_tree_ray(origin, direction, tree.offset, tree.invradius)
    tmin, tmax = T._dda_unit(o, invdir)
    if tmax < 0 or tmin > tmax:
        return None
    out, t = [], tmin
    while t < tmax:
        pos = np.array([f32(o[a] + f32(t * d[a])) for a in range(3)], f32)
        n, i, j, k, cube, local = tree.query(pos)
        s0, s1 = T._dda_unit(local, invdir)
        delta_t = f32(f32(f32(s1 - s0) / cube) + opt.step_size)
        out.append((((n * 2 + i) * 2 + j) * 2 + k, f32(t), delta_t))
        t = f32(t + delta_t)
    return out, delta_scale


class RayAux:
    """rgb[3]; alpha, depth, surface; light = the transmittance left when the march ended (before any rescale); stopped;
    s_max = the largest sample distance of the ray (0 without samples); pick = index (into the sample list) of the sample
    that set `surface`, -1 if none; light_at_pick = transmittance after that sample; margin = the smallest relative distance
    |light - surface_thresh| / surface_thresh over the transmittances after every shaded sample (inf without any)."""


def composite(tree, marched, vdir, opt, surface_thresh, dtype=np.float32):
    R = RayAux()
    bg = opt.background_brightness
    R.stopped, R.s_max, R.pick, R.light_at_pick, R.margin = False, 0.0, -1, None, np.inf
    if marched is None:
        R.rgb = np.full(3, bg, dtype)
        R.alpha, R.depth, R.surface, R.light = dtype(0.0), dtype(0.0), dtype(np.inf), dtype(1.0)
        return R
    samples, delta_scale = marched
    basis_dim = (tree.data_dim - 1) // 3
    basis = T.sh_basis_np(basis_dim, vdir)
    flat = tree.data.reshape(-1, tree.data_dim)
    exact = dtype == np.float32
    r = (lambda x: f32(x)) if exact else (lambda x: np.float64(x))
    out, light = np.zeros(3, dtype), dtype(1.0)
    alpha, depth, surface = dtype(0.0), dtype(0.0), dtype(np.inf)
    thresh = dtype(f32(surface_thresh))
    for i, (leaf, t, delta) in enumerate(samples):
        val = flat[leaf]
        sigma = val[-1]
        s = r(r(r(t) + r(dtype(0.5) * r(delta))) * r(delta_scale))
        R.s_max = max(R.s_max, float(s))
        if sigma > opt.sigma_thresh:
            dtw = r(r(delta) * r(delta_scale))
            att = r(np.exp(r(-dtw * r(sigma)), dtype=dtype))
            weight = r(light * r(dtype(1.0) - att))
            for c in range(3):
                if exact:
                    tmp = f32(0.0)
                    for q in range(basis_dim):
                        tmp = f32(tmp + f32(basis[q] * val[c * basis_dim + q]))
                    col = T._sigmoid(tmp)
                else:
                    tmp = np.dot(basis.astype(np.float64), val[c * basis_dim:(c + 1) * basis_dim].astype(np.float64))
                    col = 1.0 / (1.0 + np.exp(-tmp))
                out[c] = r(out[c] + r(weight * col))
            alpha = r(alpha + weight)
            depth = r(depth + r(weight * s))
            light = r(light * att)
            R.margin = min(R.margin, abs(float(light) - float(thresh)) / float(thresh))
            if light <= thresh and R.pick < 0:
                surface, R.pick, R.light_at_pick = s, i, float(light)
            if light <= opt.stop_thresh:
                scale = r(dtype(1.0) / r(dtype(1.0) - light))
                R.rgb = (out * scale).astype(dtype)
                R.alpha, R.depth, R.surface, R.light, R.stopped = r(alpha * scale), r(depth * scale), surface, light, True
                return R
    R.rgb = (out + r(light * dtype(bg))).astype(dtype)
    R.alpha, R.depth, R.surface, R.light = alpha, depth, surface, light
    return R


def render_ray_aux(tree, origin, direction, vdir, opt, surface_thresh=0.5):
    """(float32 RayAux, float64 RayAux) of one ray from one march."""
    m = march(tree, origin, direction, opt)
    return composite(tree, m, vdir, opt, surface_thresh, np.float32), composite(tree, m, vdir, opt, surface_thresh, np.float64)


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


def render_rays_aux(tree, origins, dirs, vdirs, opt, surface_thresh=0.5):
    """(float32 Batch, float64 Batch) of explicit rays."""
    both = [render_ray_aux(tree, o, d, v, opt, surface_thresh) for o, d, v in zip(origins, dirs, vdirs)]
    return Batch([b[0] for b in both]), Batch([b[1] for b in both])


def render_persp_aux(tree, c2w, W, H, fx, opt, surface_thresh=0.5, fy=None):
    """(float32 Batch, float64 Batch) of a pinhole camera, rays in row-major pixel order (reshape to [H,W,..])."""
    fy = fx if fy is None else fy
    rays = [T.cam2world_ray(ix, iy, c2w, W, H, fx, fy) for iy in range(H) for ix in range(W)]
    o = [x[0] for x in rays]; d = [x[1] for x in rays]
    return render_rays_aux(tree, o, d, d, opt, surface_thresh)


def surface_excluded(b32, b64, surface_thresh=0.5):
    """Rays left out of the surface comparison: the float64 transmittance after the chosen sample lies within a relative
    1e-4 of the threshold, or the two precisions already choose different samples."""
    near = np.abs(b64.light_at_pick - surface_thresh) <= 1e-4 * surface_thresh        # nan (no pick) compares False
    return near | (b32.pick != b64.pick)
