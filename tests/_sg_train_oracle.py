"""Host twin of NeRF-SG training: the pieces of oracle.nerf_oracle (sampling, MLP, compositing, the loss of nerf_sh/train.py:
68-114) composed with the spherical-Gaussian basis of nerf_sh/nerf/sg.py:35-66 in place of eval_sh, in any torch dtype, and
differentiated by torch autograd.  The SG leaves travel as one array sg_params [3K] = (sg_lambda [K], sg_mu_spher [K,2]
row-major), the layout of pxo_sg_lobes; they are counted in weight_l2 (train.py:101-108 reduces over the whole params tree)."""
import torch

from oracle import nerf_oracle as O


def split_params(sg_params, K):
    return sg_params[:K], sg_params[K:].reshape(K, 2)


def lobes_from_params(sg_params, K):
    """[K,4] = (softplus(sg_lambda), spher2cart(1, theta, phi)) (sg.py:27-32, :54-58), differentiable."""
    lam, mu = split_params(sg_params, K)
    theta, phi = mu[:, 0], mu[:, 1]
    st = torch.sin(theta)
    return torch.stack([torch.logaddexp(lam, torch.zeros_like(lam)), st * torch.cos(phi), st * torch.sin(phi), torch.cos(theta)], -1)


def basis(lobes, viewdirs):
    """exp(lambda_i (mu_i . v - 1)) / K for viewdirs [B,3] -> [B,K] (sg.py:59-65; the division by K folded into the basis)."""
    dot = viewdirs @ lobes[:, 1:].T
    return torch.exp(lobes[:, 0] * (dot - 1.0)) / lobes.shape[0]


def shade(raw_rgb, lobes, viewdirs):
    """raw_rgb [B,S,3K] channel-major -> sigmoid(eval_sg) [B,S,3] (models.py:273-280)."""
    K = lobes.shape[0]
    Y = basis(lobes, viewdirs)
    return torch.sigmoid((raw_rgb.reshape(*raw_rgb.shape[:-1], 3, K) * Y[:, None, None, :]).sum(-1))


def composite(cfg, rays, raw_rgb, raw_sigma, z, lobes):
    """(comp_rgb, disp, acc, weights) of B rays of S samples: raw_rgb [B,S,3K], raw_sigma [B,S,1]."""
    return O.volumetric_rendering(shade(raw_rgb, lobes, rays.viewdirs), torch.relu(raw_sigma), z, rays.directions, cfg.white_bkgd)


def stage(cfg, rays, raw_rgb, raw_sigma, z, px, lobes, sp_sigma=None, dtype=torch.float64):
    """What pxo_sg_shade_composite_train computes, in `dtype`: the pixel loss of train.py:89 (plus the sparsity term :81-83 on
    sp_sigma) and its gradients with respect to raw_rgb, raw_sigma, the lobes [K,4] and sp_sigma."""
    c = lambda t: t.detach().to(dtype)
    rr, rs, lb = c(raw_rgb).requires_grad_(True), c(raw_sigma).requires_grad_(True), c(lobes).requires_grad_(True)
    r = O.Rays(*[c(x) for x in rays])
    comp, _, _, w = composite(cfg, r, rr, rs, c(z), lb)
    loss = ((comp - c(px)) ** 2).mean()
    sps = None
    if sp_sigma is not None and sp_sigma.numel():
        sps = c(sp_sigma).requires_grad_(True)
        loss = loss + cfg.sparsity_weight * (1.0 - torch.exp(-cfg.sparsity_length * torch.relu(sps)).mean())
    loss.backward()
    return dict(comp_rgb=comp.detach(), weights=w.detach(), ray_sse=((comp - c(px)) ** 2).sum(-1).detach(), d_raw_rgb=rr.grad,
                d_raw_sigma=rs.grad, d_lobes=lb.grad, d_sp_sigma=None if sps is None else sps.grad)


def _level(mlp, lobes, samples, viewdirs, z, directions, cfg, noise=None):
    raw_rgb, raw_sigma = O.mlp_forward(mlp, O.posenc(samples, cfg.min_deg_point, cfg.max_deg_point), cfg)
    raw_sigma = O.add_gaussian_noise(raw_sigma, cfg.noise_std, noise)      # models.py:258-264 / :318-324, before the relu
    return O.volumetric_rendering(shade(raw_rgb, lobes, viewdirs), torch.relu(raw_sigma), z, directions, cfg.white_bkgd)


def render(params, sg_params, rays, cfg, t_rand=None, u=None, noise_c=None, noise_f=None):
    """NerfModel.__call__ with sg_dim = cfg.sh_dim (models.py:216-348): [(rgb, disp, acc)_coarse, (rgb, disp, acc)_fine].
    noise_c [B,Nc] / noise_f [B,Nc+Nf]: the standard-normal draws of add_gaussian_noise when cfg.noise_std is set."""
    lobes = lobes_from_params(sg_params, cfg.sh_dim)
    z, samples = O.sample_along_rays(rays.origins, rays.directions, cfg.num_coarse_samples, cfg.near, cfg.far, t_rand, cfg.lindisp)
    comp, disp, acc, w = _level(params[0], lobes, samples, rays.viewdirs, z, rays.directions, cfg, noise_c)
    ret = [(comp, disp, acc)]
    if cfg.num_fine_samples > 0:
        z_mid = 0.5 * (z[..., 1:] + z[..., :-1])
        z, samples = O.sample_pdf(z_mid, w[..., 1:-1], rays.origins, rays.directions, z, cfg.num_fine_samples, u)
        comp, disp, acc, _ = _level(params[1], lobes, samples, rays.viewdirs, z, rays.directions, cfg, noise_f)
        ret.append((comp, disp, acc))
    return ret


def loss_fn(params, sg_params, rays, pixels, cfg, t_rand, u, sp_points, noise_c=None, noise_f=None):
    """train.py:68-114 with the SG leaves in the params tree.  Returns (total, stats dict)."""
    ret = render(params, sg_params, rays, cfg, t_rand, u, noise_c, noise_f)
    zero = torch.zeros((), dtype=pixels.dtype)
    loss_sp = zero
    if cfg.sparsity_weight > 0.0:
        _, sp_sigma = O.eval_points_raw(params, sp_points, cfg)
        loss_sp = cfg.sparsity_weight * (1.0 - torch.exp(-cfg.sparsity_length * torch.relu(sp_sigma)).mean())
    loss = ((ret[-1][0] - pixels) ** 2).mean()
    loss_c, psnr_c = zero, zero
    if len(ret) > 1:
        loss_c = ((ret[0][0] - pixels) ** 2).mean()
        psnr_c = O.compute_psnr(loss_c)
    leaves = [t for mlp in params for pair in mlp for t in pair] + [sg_params]
    weight_l2 = sum((x ** 2).sum() for x in leaves) / sum(x.numel() for x in leaves)
    stats = dict(loss=loss, psnr=O.compute_psnr(loss), loss_c=loss_c, loss_sp=loss_sp, psnr_c=psnr_c, weight_l2=weight_l2)
    return loss + loss_c + loss_sp + cfg.weight_decay_mult * weight_l2, stats


def loss_and_grad(flat_params, sg_params, rays, pixels, cfg, t_rand, u, sp_points, noise_c=None, noise_f=None):
    """jax.value_and_grad(loss_fn) (train.py:116): (total, stats, MLP gradient [2 n_mlp], SG gradient [3K])."""
    flat = flat_params.detach().clone().requires_grad_(True)
    sgp = sg_params.detach().clone().requires_grad_(True)
    total, stats = loss_fn(O.unflatten_params(flat, cfg), sgp, rays, pixels, cfg, t_rand, u, sp_points, noise_c, noise_f)
    total.backward()
    return total.detach(), {k: v.detach() for k, v in stats.items()}, flat.grad.detach(), sgp.grad.detach()


def fixture_index(cfg, stride=8):
    """Which entries of the flat 2-MLP gradient tests/golden/sg_train_grad.npz keeps (a committed file is limited to 1 MiB; the
    whole float32 gradient of two sh_deg-4 MLPs is 4.1 MB): every bias, every kernel of at most 20,000 entries (Dense_0, the two
    heads) whole, and every `stride`-th input row of the 256-wide trunk kernels, all columns.  Every leaf is represented.
    Returns (index into the flat arena [int64], per-leaf (start, count) ranges within the kept vector, per-leaf MLP number)."""
    idx, ranges, owner, off, kept = [], [], [], 0, 0
    for mi in range(2):
        for fi, fo in O.layer_shapes(cfg):
            rows = torch.arange(fi) if fi * fo <= 20000 else torch.arange(0, fi, stride)
            k = (off + rows[:, None] * fo + torch.arange(fo)[None, :]).reshape(-1)
            idx.append(k); ranges.append((kept, k.numel())); owner.append(mi)
            kept += k.numel(); off += fi * fo
            b = off + torch.arange(fo)
            idx.append(b); ranges.append((kept, fo)); owner.append(mi)
            kept += fo; off += fo
    return torch.cat(idx), ranges, owner


def chain_rule(d_lobes, sg_params):
    """d loss / d sg_params [3K] from d loss / d lobes [K,4] in closed form (what sg_lobe_grad_kernel evaluates): sigmoid for the
    softplus, the derivatives of (sin t cos p, sin t sin p, cos t) for spher2cart."""
    K = d_lobes.shape[0]
    lam, mu = split_params(sg_params, K)
    st, ct, sp, cp = torch.sin(mu[:, 0]), torch.cos(mu[:, 0]), torch.sin(mu[:, 1]), torch.cos(mu[:, 1])
    g_lam = d_lobes[:, 0] * torch.sigmoid(lam)
    g_theta = d_lobes[:, 1] * ct * cp + d_lobes[:, 2] * ct * sp - d_lobes[:, 3] * st
    g_phi = d_lobes[:, 2] * st * cp - d_lobes[:, 1] * st * sp
    return torch.cat([g_lam, torch.stack([g_theta, g_phi], -1).reshape(-1)])


def fixture_inputs(g, gw, dtype):
    """Inputs of tests/golden/sg_train_grad.npz in `dtype`: (cfg, flat MLP arena, sg_params, rays, pixels, t_rand, u, sparsity
    points).  Weights of eval_points_sh25.npz with the sigma-head biases shifted in float32, as the generator did."""
    cfg = O.Cfg(sh_deg=4, sparsity_npoints=int(g["sparsity_npoints"]), weight_decay_mult=float(g["weight_decay_mult"]))
    params = [[(torch.tensor(gw[f"MLP_{mi}.Dense_{li}.kernel"]), torch.tensor(gw[f"MLP_{mi}.Dense_{li}.bias"]))
               for li in range(cfg.net_depth + 2)] for mi in range(2)]
    flat = O.flatten_params(params)
    n, C = flat.numel() // 2, cfg.num_rgb_channels
    for mi in range(2):                                   # Dense_8 bias = the float just before Dense_9's kernel + bias
        flat[(mi + 1) * n - C - C * 256 - 1] += float(g["sigma_bias_shift"])
    t = lambda k: torch.tensor(g[k]).to(dtype)
    sg_params = torch.cat([t("sg_lambda"), t("sg_mu_spher").reshape(-1)])
    rays = O.Rays(t("origins"), t("directions"), t("viewdirs"))
    return cfg, flat.to(dtype), sg_params, rays, t("pixels"), t("t_rand"), t("u"), -1.5 + 3.0 * t("sp_u")
