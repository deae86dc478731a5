"""Test-side oracle of the NDC launches of the octree side (pxo_octree_render_ndc_fwd / _bwd, pxo_grid_weight_render_ndc).

A numpy-float32 restatement of items 2, 3 and 5 of the definition (include/plenoctree_octree.h): the
reference's convert_to_ndc in its operation order, the normalisation of the NDC direction, and the miss rule.  Everything
after it is oracle/octree_oracle.py unchanged -- cam2world_ray before, march_tree / render_ray / render_rays_torch and the
body of grid_weight_render after -- so what is checked is exactly "convert, then the existing march".  The restatement itself
is pinned to the reference's own convert_to_ndc by tests/golden/octree_ndc.npz (tests/test_octree_ndc_cpu.py).

The shapes every test shares live here too: the 14 x 10 image whose edge pixels land on NDC x = +-1, camera A (identity: every
NDC ray parallel to z, the degenerate invdir case), camera B (translated and rotated), and depth-3 random trees in two boxes.
"""
import math

import numpy as np
import torch

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


def random_tree(K, box, depth=3, seed=None, p=0.15):
    """The trees of tests/test_gpu_octree.py::_random_tree (random mask, random SH data, about a third of the leaves empty) in
    one of the NDC boxes."""
    seed = 40 + K if seed is None else seed
    center, radius = BOXES[box]
    reso = 2 ** (depth + 1)
    mask = np.random.RandomState(seed).rand(reso, reso, reso) < p
    t = T.build_from_mask(mask, depth, 3 * K + 1, center, radius)
    rs = np.random.RandomState(seed + 100)
    t.data[:] = (rs.randn(*t.data.shape) * 0.7).astype(f32)
    t.data[..., -1] = ((rs.rand(*t.data.shape[:-1]) - 0.35) * 12.0).astype(f32)
    return t


def camera_rays(c2w, width=W, height=H, fx=FX):
    """World-space (origins, unit directions) [H*W, 3] of svox's cam2world_ray, row-major."""
    rays = [T.cam2world_ray(ix, iy, c2w, width, height, fx, fx) for iy in range(height) for ix in range(width)]
    return np.stack([r[0] for r in rays]).astype(f32), np.stack([r[1] for r in rays]).astype(f32)


def march(tree, o, d, opt, ndc):
    """march_tree over the NDC ray of the world ray (o, d): the sample list, or None for a miss."""
    no, nd, ok = ndc_ray(o, d, ndc)
    with np.errstate(over="ignore"):             # a ray converted to 1e37 overflows the slab test to inf: a plain miss
        return T.march_tree(tree, no, nd, opt) if ok else None


def render_ray(tree, o, d, vdir, opt, ndc):
    """render_ray of the converted ray, shaded with the WORLD-space vdir (item 1); the background for a miss."""
    no, nd, ok = ndc_ray(o, d, ndc)
    if not ok:
        return np.full(3, opt.background_brightness, f32)
    with np.errstate(over="ignore"):
        return T.render_ray(tree, no, nd, vdir, opt)


def render_rays(tree, origins, dirs, vdirs, opt, ndc):
    return np.stack([render_ray(tree, o, d, v, opt, ndc) for o, d, v in zip(origins, dirs, vdirs)])


def render_persp(tree, c2w, opt, ndc, width=W, height=H, fx=FX):
    o, d = camera_rays(c2w, width, height, fx)
    return render_rays(tree, o, d, d, opt, ndc).reshape(height, width, 3)


def render_rays_torch(tree, data, origins, dirs, vdirs, opt, ndc, dtype=torch.float64):
    """float64 autograd through oracle.render_rays_torch over the NDC sample sequence; a miss is the constant background.
    dtype: the compositing precision, handed on to oracle.render_rays_torch."""
    conv = [ndc_ray(o, d, ndc) for o, d in zip(origins, dirs)]
    hit = np.array([c[2] for c in conv])
    out = torch.full((len(conv), 3), float(opt.background_brightness), dtype=dtype)
    if hit.any():
        no = np.stack([c[0] for c in conv])[hit]
        nd = np.stack([c[1] for c in conv])[hit]
        res = T.render_rays_torch(tree, data, no, nd, np.asarray(vdirs, f32)[hit], opt, dtype=dtype)
        out = out.index_put((torch.from_numpy(np.nonzero(hit)[0]),), res)
    return out


def grid_weight_render(sigma_grid, c2w, width, height, fx, opt, offset, invradius, ndc, weight=None):
    """The body of oracle.grid_weight_render with the NDC conversion between cam2world_ray and _to_tree_ray."""
    reso = sigma_grid.shape[0]
    weight = np.zeros_like(sigma_grid, dtype=f32) if weight is None else weight
    cube = f32(reso)
    for iy in range(height):
        for ix in range(width):
            origin, direction = T.cam2world_ray(ix, iy, c2w, width, height, fx, fx)
            origin, direction, ok = ndc_ray(origin, direction, ndc)
            if not ok:
                continue
            o, d, invdir, delta_scale = T._to_tree_ray(origin, direction, offset, invradius)
            tmin, tmax = T._dda_unit(o, invdir)
            if tmax < 0 or tmin > tmax:
                continue
            t, light = tmin, f32(1.0)
            while t < tmax:
                pos = np.array([f32(o[a] + f32(t * d[a])) for a in range(3)], f32)
                pos = np.clip(pos, f32(0.0), f32(1.0 - 1e-6)).astype(f32)
                pos = (pos * cube).astype(f32)
                u = np.floor(pos).astype(np.int64)
                local = (pos - u.astype(f32)).astype(f32)
                s0, s1 = T._dda_unit(local, invdir)
                delta_t = f32(f32(f32(s1 - s0) / cube) + opt.step_size)
                sigma = sigma_grid[u[0], u[1], u[2]]
                if sigma > opt.sigma_thresh:
                    att = f32(np.exp(f32(-f32(delta_t * delta_scale) * sigma), dtype=f32))
                    w = f32(light * f32(f32(1.0) - att))
                    light = f32(light * att)
                    weight[u[0], u[1], u[2]] = max(weight[u[0], u[1], u[2]], w)
                    if light <= opt.stop_thresh:
                        break
                t = f32(t + delta_t)
    return weight


# ---- known answer, independent of the composition above -----------------------------------------------------------------
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
    no, nd, ok = ndc_ray(o, d, ndc)
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
    o, d = camera_rays(camera_b())
    got = np.asarray(render(t, o, d, opt), np.float64)
    worst, worst_bound, wrong, hits = 0.0, 0.0, 0.0, 0
    for i, (oo, dd) in enumerate(zip(o, d)):
        seq = march(t, oo, dd, opt, ndc)
        if seq is None:
            assert np.array_equal(got[i], np.zeros(3))
            continue
        hits += 1
        want = known_answer(t, oo, dd, dd, ndc)
        bound = KNOWN_SIGMA * len(seq) * KNOWN_STEP * 2.0 + 1e-5
        err = float(np.abs(got[i] - want).max())
        assert err <= bound, (i, err, bound, len(seq))
        worst, worst_bound = max(worst, err), max(worst_bound, bound)
        _, nd, _ = ndc_ray(oo, dd, ndc)
        wrong = max(wrong, float(np.abs(known_answer(t, oo, dd, nd, ndc) - got[i]).max()))
    assert hits >= 20 and wrong > 0.03, (hits, wrong)
    return worst, worst_bound
