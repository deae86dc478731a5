"""float64 restatement of the loss a culled train step minimises (pxo_train_fwd_bwd_culled, include/plenoctree_hip.h), built from
the oracle's functions: the raw outputs of the culled rows are replaced by the constants 0 (no gradient flows into them),
everything else -- shading, compositing, the pixel losses of both levels, the sparsity term on the always-live sparsity points,
weight decay -- is O.loss_fn.  The sample positions are given (no gradient flows through them, model_utils.py:286), as in
_helpers.oracle_loss_and_grad_given_z; with every row live this IS that function."""
import torch

from oracle import nerf_oracle as O


def _level(mlp, z, live, o, d, v, cfg):
    """comp_rgb [B,3] of one level; live bool [B,S]: False = the sample's raw colour and raw sigma are the constants 0."""
    raw_rgb, raw_sigma = O.mlp_forward(mlp, O.posenc(O.cast_rays(z, o, d), cfg.min_deg_point, cfg.max_deg_point), cfg)
    raw_rgb = torch.where(live[..., None], raw_rgb, torch.zeros_like(raw_rgb))
    raw_sigma = torch.where(live[..., None], raw_sigma, torch.zeros_like(raw_sigma))      # [B,S,1]
    raw = O.eval_sh(cfg.sh_deg, raw_rgb.reshape(*raw_rgb.shape[:-1], -1, cfg.sh_dim), v[:, None])
    return O.volumetric_rendering(torch.sigmoid(raw), torch.relu(raw_sigma), z, d, cfg.white_bkgd)[0]


def masked_loss_and_grad(flat, rays, px, cfg, z_c, z_f, live_c, live_f, sp_points, dtype=torch.float64):
    """(stats dict of floats: loss, psnr, loss_c, loss_sp, psnr_c, weight_l2; gradient on the flat arena).  z_c [B,Nc], z_f
    [B,Nc+Nf]: the sample positions; live_c / live_f: bool masks of the same shapes; sp_points [n,3] or None."""
    cast = lambda t: t.detach().cpu().to(dtype)
    p = cast(flat).clone().requires_grad_(True)
    params = O.unflatten_params(p, cfg)
    o, d, v = [cast(x) for x in rays]
    tgt = cast(px)
    assert cfg.num_fine_samples > 0
    loss_c = ((_level(params[0], cast(z_c), live_c.cpu(), o, d, v, cfg) - tgt) ** 2).mean()
    loss = ((_level(params[1], cast(z_f), live_f.cpu(), o, d, v, cfg) - tgt) ** 2).mean()
    loss_sp = torch.zeros((), dtype=dtype)
    if cfg.sparsity_weight > 0.0 and cfg.sparsity_npoints > 0:
        _, sig = O.eval_points_raw(params, cast(sp_points), cfg)
        loss_sp = cfg.sparsity_weight * (1.0 - torch.exp(-cfg.sparsity_length * torch.relu(sig)).mean())
    leaves = [t for mlp in params for pair in mlp for t in pair]
    weight_l2 = sum((x ** 2).sum() for x in leaves) / sum(x.numel() for x in leaves)
    (loss + loss_c + loss_sp + cfg.weight_decay_mult * weight_l2).backward()
    loss, loss_c, loss_sp, weight_l2 = (x.detach() for x in (loss, loss_c, loss_sp, weight_l2))
    stats = dict(loss=float(loss), psnr=float(O.compute_psnr(loss)), loss_c=float(loss_c), loss_sp=float(loss_sp),
                 psnr_c=float(O.compute_psnr(loss_c)), weight_l2=float(weight_l2))
    return stats, p.grad.detach()


STAT_NAMES = ("loss", "psnr", "loss_c", "loss_sp", "psnr_c", "weight_l2")
