"""NeRF-SG: the reference's spherical-Gaussian output basis (nerf_sh/config/misc/sg.yaml, sg_dim: 25), read, ray-rendered and
baked into an SG PlenOctree.

Host-side mirror of the sg_dim > 0 branches of nerf_sh/nerf/models.py (:107-117 the two model-level parameters sg_lambda [K]
and sg_mu_spher [K,2]; :204-210, :273-292, :331-348 the shading through eval_sg, nerf_sh/nerf/sg.py:35-66) and of
octree/extraction.py:436-442 (the lobes handed to the tree as extra_data).

A NeRF-SG is the SH network with 3 * sg_dim + 1 outputs.  For sg_dim in {1, 4, 9, 16, 25} that is the MLP shape the kernels
run for sh_deg = sqrt(sg_dim) - 1, so the model keeps a PxoCfg of that degree and shares packing, pxo_eval_points,
pxo_grid_sigma and pxo_mean_over_samples with the SH path; only the shading differs (pxo_sg_render_fwd).  Lobes are one
global set per model (the reference asserts a flag `sg_global` that it defines nowhere).  Training a NeRF-SG is not built:
nerf_sh.train keeps rejecting sg_dim > 0 (utils.check_supported); nerf_sh.eval, nerf_sh.gen_video and octree.extraction opt
in through check_render_flags / check_extraction_flags.
"""
import math

import numpy as np
import torch

from . import models

SUPPORTED_DIMS = (1, 4, 9, 16, 25)


def head_degree(sg_dim):
    """sh_deg of the SH model whose MLP head has the width of a NeRF-SG with `sg_dim` lobes."""
    if sg_dim not in SUPPORTED_DIMS:
        raise NotImplementedError(f"sg_dim={sg_dim}: SG is built for sg_dim in {SUPPORTED_DIMS} only (the widths the MLP head "
                                  "and the renderers are instantiated for)")
    return int(round(math.sqrt(sg_dim))) - 1


def lobes_from_params(sg_lambda, sg_mu_spher):
    """cat(softplus(sg_lambda)[:, None], spher2cart(theta, phi)) (octree/extraction.py:439-442; eval_sg, sg.py:54-58):
    float32 [K,4] rows (lambda, mu.x, mu.y, mu.z) with mu = (sin theta cos phi, sin theta sin phi, cos theta), evaluated on the
    host in float32."""
    lam = np.asarray(sg_lambda.detach().cpu() if torch.is_tensor(sg_lambda) else sg_lambda, np.float32).reshape(-1)
    mu = np.asarray(sg_mu_spher.detach().cpu() if torch.is_tensor(sg_mu_spher) else sg_mu_spher, np.float32)
    if mu.shape != (lam.shape[0], 2):
        raise ValueError(f"sg_mu_spher has shape {mu.shape}, sg_lambda {lam.shape}: expected [K,2] and [K]")
    theta, phi = mu[:, 0], mu[:, 1]
    soft = np.logaddexp(np.float32(0.0), lam).astype(np.float32)              # softplus, stable for large |x|
    st = np.sin(theta, dtype=np.float32)
    out = np.stack([soft, st * np.cos(phi, dtype=np.float32), st * np.sin(phi, dtype=np.float32),
                    np.cos(theta, dtype=np.float32)], -1).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(out))


def init_lobe_params(sg_dim, seed=20200823):
    """nerf_sh/nerf/models.py:107-117: sg_lambda = 1, theta uniform in [0, pi), phi uniform in [0, 2 pi) (host RNG)."""
    gen = torch.Generator().manual_seed(seed + 1)
    u = torch.rand(sg_dim, 2, generator=gen, dtype=torch.float64)
    return torch.ones(sg_dim), (u * torch.tensor([math.pi, 2.0 * math.pi], dtype=torch.float64)).float()


class SgState(models.TrainState):
    """TrainState of the two MLPs plus the model-level SG parameters (host) and the lobes the kernels read (device)."""

    def __init__(self, cfg, params, sg_lambda, sg_mu_spher, step=0):
        super().__init__(cfg, params, step)
        self.set_lobe_params(sg_lambda, sg_mu_spher)

    @property
    def sg_dim(self):
        return (self.cfg.sh_deg + 1) ** 2

    def set_lobe_params(self, sg_lambda, sg_mu_spher):
        sg_lambda = torch.as_tensor(sg_lambda, dtype=torch.float32).detach().cpu().reshape(-1).clone()
        sg_mu_spher = torch.as_tensor(sg_mu_spher, dtype=torch.float32).detach().cpu().clone()
        K = self.sg_dim
        if tuple(sg_lambda.shape) != (K,) or tuple(sg_mu_spher.shape) != (K, 2):
            raise ValueError(f"sg_lambda {tuple(sg_lambda.shape)} / sg_mu_spher {tuple(sg_mu_spher.shape)}: a model with "
                             f"sg_dim={K} needs ({K},) and ({K}, 2)")
        self.sg_lambda, self.sg_mu_spher = sg_lambda, sg_mu_spher
        self.lobes = lobes_from_params(sg_lambda, sg_mu_spher).to(self.params.device)


class SgModel(models.NerfModel):
    """NerfModel with sg_dim > 0: eval_points_raw (the raw SG coefficients, channel-major like SH) is inherited; apply shades
    with the lobes of the state."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.sg_dim = (cfg.sh_deg + 1) ** 2

    def apply(self, state, rays, randomized, t_rand=None, u=None, seed=0):
        from ... import ops
        ws = state.workspace(ops.render_workspace_bytes(self.cfg, rays.origins.shape[0]))
        return ops.render_fwd(self.cfg, state.packed[0][0], state.packed[1][0], rays.origins, rays.directions, rays.viewdirs,
                              randomized=randomized, t_rand=t_rand, u=u, seed=seed, ws=ws, lobes=state.lobes)

    __call__ = apply


def apply_cli(args, argv=None):
    """utils.update_flags lets the preset win over the command line (as the reference's does), and every in-tree preset says
    sh_deg.  So that `--config blender --sg_dim 25 --sh_deg -1` selects a NeRF-SG without a preset file of its own, an
    explicit --sg_dim K > 0 on the command line, and --sh_deg beside it, are applied again after the preset.  Command lines
    without --sg_dim are left exactly as update_flags made them."""
    import argparse
    import sys
    p = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    p.add_argument("--sg_dim", type=int, default=None)
    p.add_argument("--sh_deg", type=int, default=None)
    given, _ = p.parse_known_args(sys.argv[1:] if argv is None else list(argv))
    if given.sg_dim is not None and given.sg_dim > 0:
        args.sg_dim = given.sg_dim
        if given.sh_deg is not None:
            args.sh_deg = given.sh_deg
    return args


def _unbuilt_flags(args):
    """Names of the flags of an sg_dim > 0 model that the MI355X path does not build."""
    bad = []
    if args.sg_dim <= 0:
        bad.append(f"sg_dim={args.sg_dim} (an SH model: the plain path)")
    elif args.sg_dim not in SUPPORTED_DIMS:
        bad.append(f"sg_dim={args.sg_dim} (need one of {SUPPORTED_DIMS}: the widths of the MLP head and the renderers)")
    if args.sh_deg != -1:
        bad.append(f"sh_deg={args.sh_deg} (need -1: you can only use up to one of SH or SG)")
    if args.use_viewdirs:
        bad.append("use_viewdirs=true (an SG model has no view-conditioned head)")
    if (args.net_depth, args.net_width, args.skip_layer) != (8, 256, 4):
        bad.append("net_depth/net_width/skip_layer != 8/256/4")
    if (args.min_deg_point, args.max_deg_point) != (0, 10):
        bad.append("min/max_deg_point != 0/10")
    if args.num_rgb_channels != 3 or args.num_sigma_channels != 1:
        bad.append("num_rgb_channels/num_sigma_channels != 3/1")
    if args.noise_std is not None and args.noise_std < 0:
        bad.append("noise_std < 0")
    if getattr(args, "render_path", False) or getattr(args, "spherify", False):
        bad.append("render_path / spherify (LLFF scenes)")
    if args.legacy_posenc_order:
        bad.append("legacy_posenc_order")
    if (args.net_activation.lower(), args.rgb_activation.lower(), args.sigma_activation.lower()) != ("relu", "sigmoid", "relu"):
        bad.append("activations other than relu/sigmoid/relu")
    return bad


def check_render_flags(args):
    """What nerf_sh.eval / gen_video build of an sg_dim > 0 model; everything else is rejected by name."""
    bad = _unbuilt_flags(args)
    if bad:
        raise NotImplementedError("rendering a NeRF-SG, not built on the MI355X path: " + "; ".join(bad))


def check_extraction_flags(args):
    """What octree.extraction builds of an sg_dim > 0 model; everything else is rejected by name."""
    bad = _unbuilt_flags(args)
    if bad:
        raise NotImplementedError("extraction of an SG PlenOctree, not built on the MI355X path: " + "; ".join(bad))


def check_dirs(args, require_data=True, extraction=False):
    """utils.check_flags' directory checks, then the SG flag check."""
    if args.train_dir is None:
        raise ValueError("train_dir must be set. None set now.")
    if require_data and args.data_dir is None and args.dataset != "synthetic":
        raise ValueError("data_dir must be set. None set now.")
    (check_extraction_flags if extraction else check_render_flags)(args)


def make_cfg(args):
    """PxoCfg of the SH model with the same head width (sh_deg = sqrt(sg_dim) - 1); args is left as it is."""
    import copy
    a = copy.copy(args)
    a.sh_deg = head_degree(args.sg_dim)
    return models.make_cfg(a)


def get_model_state(args, device, extraction=False):
    """Model + state with freshly initialised parameters (the caller restores a checkpoint)."""
    (check_extraction_flags if extraction else check_render_flags)(args)
    cfg = make_cfg(args)
    params = models.init_params(cfg, args.seed).to(device)
    lam, mu = init_lobe_params(args.sg_dim, args.seed)
    return SgModel(cfg), SgState(cfg, params, lam, mu)


def restore(args, device, say=print, require_data=True, extraction=False):
    """The --sg_dim K branch of nerf_sh.eval / gen_video / octree.extraction: flag checks, model + state, newest checkpoint of
    train_dir in either of the reference's formats (extraction.load_nerf_checkpoint's choice)."""
    from ...octree.extraction import load_nerf_checkpoint
    check_dirs(args, require_data, extraction)
    say(f"* Loading NeRF (SG{args.sg_dim})", flush=True)
    model, state = get_model_state(args, device, extraction)
    say(load_nerf_checkpoint(args, state), flush=True)
    return model, state
