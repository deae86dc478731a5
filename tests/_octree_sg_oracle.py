"""CPU restatement of the spherical-Gaussian (SG) tree renderer, beside oracle/octree_oracle.py (which holds the SH one).

The rule (svox data_format SG<K>, restated from the published package; anchored to the reference's own eval_sg by
tests/golden/sg_reference.npz, see tests/test_sg_cpu.py):
    lobes [K,4] rows (lambda_i, mu_i),  basis_i(d) = exp(lambda_i (mu_i . d - 1)) / K,
    colour_c = sigmoid(sum_i data[c*K + i] basis_i(d))
Everything else -- ray set-up, the sample sequence, compositing, early stop and its rescale -- is octree_oracle's: render_ray
below takes march_tree's samples and composites exactly like octree_oracle.render_ray, with this basis.
"""
import numpy as np
import torch

from oracle import octree_oracle as T

f32 = np.float32


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


def render_ray(tree, lobes, origin, direction, vdir, opt, dtype=f32):
    """octree_oracle.render_ray with the SG basis; dtype float64 composites the SAME float32 sample sequence in float64 (the
    helper's own round-off is the difference of the two)."""
    basis_dim = (tree.data_dim - 1) // 3
    assert np.asarray(lobes).shape == (basis_dim, 4)
    samples = T.march_tree(tree, origin, direction, opt)
    bg = opt.background_brightness
    r = dtype
    if samples is None:
        return np.full(3, bg, dtype)
    basis = sg_basis_np(lobes, vdir) if dtype is f32 else sg_basis_f64(lobes, np.asarray(vdir, f32))
    flat = tree.data.reshape(-1, tree.data_dim)
    out, light = np.zeros(3, dtype), r(1.0)
    for leaf, dtw in samples:
        val = flat[leaf].astype(dtype)
        sigma = val[-1]
        if sigma > opt.sigma_thresh:
            att = r(np.exp(r(-r(dtw) * sigma), dtype=dtype))
            weight = r(light * r(r(1.0) - att))
            for c in range(3):
                tmp = r(0.0)
                for q in range(basis_dim):
                    tmp = r(tmp + r(basis[q] * val[c * basis_dim + q]))
                out[c] = r(out[c] + r(weight * (r(1.0) / (r(1.0) + np.exp(-tmp, dtype=dtype)))))
            light = r(light * att)
            if light <= opt.stop_thresh:
                scale = r(r(1.0) / r(r(1.0) - light))
                return (out * scale).astype(dtype)
    return (out + r(light * r(bg))).astype(dtype)


def render_rays(tree, lobes, origins, dirs, vdirs, opt, dtype=f32):
    return np.stack([render_ray(tree, lobes, o, d, v, opt, dtype) for o, d, v in
                     zip(np.asarray(origins, f32), np.asarray(dirs, f32), np.asarray(vdirs, f32))])


def camera_rays(c2w, W, H, fx, fy=None):
    fy = fx if fy is None else fy
    rays = [T.cam2world_ray(ix, iy, c2w, W, H, fx, fy) for iy in range(H) for ix in range(W)]
    return np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])


def render_persp(tree, lobes, c2w, W, H, fx, opt, fy=None, dtype=f32):
    o, d = camera_rays(c2w, W, H, fx, fy)
    return render_rays(tree, lobes, o, d, d, opt, dtype).reshape(H, W, 3)


def ray_alpha(tree, origin, direction, opt):
    """Accumulated opacity 1 - light of a ray (float64 over march_tree's samples, no early stop); 0 for a miss."""
    samples = T.march_tree(tree, origin, direction, opt)
    if samples is None:
        return 0.0
    flat = tree.data.reshape(-1, tree.data_dim)
    light = 1.0
    for leaf, dtw in samples:
        sigma = float(flat[leaf][-1])
        if sigma > opt.sigma_thresh:
            light *= np.exp(-float(dtw) * sigma)
    return 1.0 - light


def render_rays_torch(tree, lobes, data, origins, dirs, vdirs, opt, dtype=torch.float64):
    """octree_oracle.render_rays_torch with the SG basis: differentiable w.r.t. `data`, no early stop."""
    basis_dim = (tree.data_dim - 1) // 3
    flat = data.reshape(-1, tree.data_dim).to(dtype)
    outs = []
    for o, d, v in zip(np.asarray(origins, f32), np.asarray(dirs, f32), np.asarray(vdirs, f32)):
        samples = T.march_tree(tree, o, d, opt)
        bg = float(opt.background_brightness)
        if samples is None:
            outs.append(torch.full((3,), bg, dtype=dtype))
            continue
        idx = torch.tensor([s[0] for s in samples], dtype=torch.long)
        dtw = torch.tensor([float(s[1]) for s in samples], dtype=dtype)
        val = flat[idx]
        sigma = val[:, -1]
        live = sigma > float(opt.sigma_thresh)
        att = torch.where(live, torch.exp(-dtw * sigma), torch.ones_like(sigma))
        Tr = torch.cumprod(torch.cat([torch.ones(1, dtype=dtype), att]), 0)
        w = Tr[:-1] * (1.0 - att)
        basis = torch.tensor(sg_basis_f64(lobes, v), dtype=dtype)
        rgb = torch.sigmoid((val[:, :-1].reshape(-1, 3, basis_dim) * basis).sum(-1))
        outs.append((w[:, None] * rgb).sum(0) + Tr[-1] * bg)
    return torch.stack(outs)
