"""NeRF-SG: the reference's spherical-Gaussian output basis (nerf_sh/config/misc/sg.yaml, sg_dim: 25), trained, read,
ray-rendered and baked into an SG PlenOctree.

Host-side mirror of the sg_dim > 0 branches of nerf_sh/nerf/models.py (:107-117 the two model-level parameters sg_lambda [K]
and sg_mu_spher [K,2]; :204-210, :273-292, :331-348 the shading through eval_sg, nerf_sh/nerf/sg.py:35-66) and of
octree/extraction.py:436-442 (the lobes handed to the tree as extra_data).

A NeRF-SG is the SH network with 3 * sg_dim + 1 outputs.  For sg_dim in {1, 4, 9, 16, 25} that is the MLP shape the kernels
run for sh_deg = sqrt(sg_dim) - 1, so the model keeps a PxoCfg of that degree and shares packing, pxo_eval_points,
pxo_grid_sigma and pxo_mean_over_samples with the SH path; only the shading differs (pxo_sg_render_fwd).  Lobes are one
global set per model (the reference asserts a flag `sg_global` that it defines nowhere).  utils.check_supported keeps
rejecting sg_dim > 0; what nerf_sh.train, nerf_sh.eval, nerf_sh.gen_video, nerf_sh.gen_mesh and octree.extraction build of such
a model, and which checkpoints they read, is the SG row of families.py.

Training (models.train_step with the SgState below; nerf_sh/nerf/models.py:107-117 puts sg_lambda and sg_mu_spher into the
"params" collection, so train.py:101-119 differentiates, averages, decays and Adam-updates them like any other leaf): the raw parameters live on the
device as one array sg_params [3K] = (sg_lambda [K], sg_mu_spher [K,2]) with their Adam moments; their gradient sits behind
the two MLPs' in the state's reduce buffer, inside bucket 1, so the gradient exchange needs no collective of its own.
pxo_sg_train_fwd_bwd derives the lobes from sg_params on the device, the update is pxo_adam_step on the 3K tail and pxo_sg_lobes
refreshes state.lobes: nothing in a step waits for the host.  state.sg_lambda / state.sg_mu_spher are host copies, read back
from the device when they are asked for after a step.  A state restored from a checkpoint takes its lobes from the host
expression (lobes_from_params), which can differ from the device kernel's in the last float32 bit; training never reads them.
"""
import math

import numpy as np
import torch

from ... import ops
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
    """TrainState of the two MLPs plus the model-level SG parameters: raw parameters, Adam moments and gradient on the device
    of `params` (sg_params / sg_m / sg_v / sg_grads, [3K] each), host copies behind sg_lambda / sg_mu_spher, and the lobes the
    kernels read."""

    def __init__(self, cfg, params, sg_lambda, sg_mu_spher, step=0):
        super().__init__(cfg, params, step)
        # gradient arena [MLP_0 | MLP_1 | SG (3K) | 6 stats | pad]: bucket 0 is unchanged, the SG gradient rides in bucket 1
        n, k3 = params.numel(), 3 * self.sg_dim
        self.reduce_buf = torch.zeros(n + k3 + 8, dtype=torch.float32, device=params.device)
        self.grads = self.reduce_buf[:n]
        self.sg_grads = self.reduce_buf[n:n + k3]
        self.stats = self.reduce_buf[n + k3:n + k3 + 6]
        self.bucket0 = self.reduce_buf[:self.n_mlp]
        self.bucket1 = self.reduce_buf[self.n_mlp:]
        self.set_lobe_params(sg_lambda, sg_mu_spher)

    @property
    def sg_dim(self):
        return (self.cfg.sh_deg + 1) ** 2

    def _sync_host(self):
        """The host copies follow the device parameters when a train step has moved them (one copy, when somebody asks)."""
        if getattr(self, "_sg_stale", False):
            K = self.sg_dim
            p = self.sg_params.detach().cpu()
            self._sg_lambda, self._sg_mu_spher = p[:K].clone(), p[K:].reshape(K, 2).clone()
            self._sg_stale = False

    @property
    def sg_lambda(self):
        self._sync_host()
        return self._sg_lambda

    @property
    def sg_mu_spher(self):
        self._sync_host()
        return self._sg_mu_spher

    def set_lobe_params(self, sg_lambda, sg_mu_spher, m=None, v=None):
        """Raw parameters (and, from a checkpoint, their Adam moments as flat [3K] arrays; zeros otherwise) into the state."""
        sg_lambda = torch.as_tensor(sg_lambda, dtype=torch.float32).detach().cpu().reshape(-1).clone()
        sg_mu_spher = torch.as_tensor(sg_mu_spher, dtype=torch.float32).detach().cpu().clone()
        K = self.sg_dim
        if tuple(sg_lambda.shape) != (K,) or tuple(sg_mu_spher.shape) != (K, 2):
            raise ValueError(f"sg_lambda {tuple(sg_lambda.shape)} / sg_mu_spher {tuple(sg_mu_spher.shape)}: a model with "
                             f"sg_dim={K} needs ({K},) and ({K}, 2)")
        dev = self.params.device
        self._sg_lambda, self._sg_mu_spher, self._sg_stale = sg_lambda, sg_mu_spher, False
        self.sg_params = torch.cat([sg_lambda, sg_mu_spher.reshape(-1)]).to(dev)
        self.sg_m, self.sg_v = (torch.zeros(3 * K, dtype=torch.float32, device=dev) if a is None else
                                torch.as_tensor(a, dtype=torch.float32).reshape(3 * K).clone().to(dev) for a in (m, v))
        self.lobes = lobes_from_params(sg_lambda, sg_mu_spher).to(dev)

    def train_workspace_bytes(self, cfg, B):
        return ops.sg_train_workspace_bytes(cfg, B)

    def fwd_bwd(self, cfg, rays, pixels, ws, **kw):
        """pxo_sg_train_fwd_bwd_bucketed leaves the SG gradient behind the MLPs' in the reduce buffer (inside bucket 1, so the
        step's reducer averages it with the rest)."""
        ops.sg_train_fwd_bwd(cfg, self.params, self.sg_params, self.packed, rays.origins, rays.directions, rays.viewdirs, pixels,
                             self.grads, self.sg_grads, self.stats, ws, **kw)

    def update(self, cfg, lr, grad_scale):
        """Adam over the two MLPs with the re-pack, Adam over the 3K SG tail at the same learning rate and step (train.py:119)
        and the refresh of the lobes -- all on the stream; the host copies are stale from here on."""
        super().update(cfg, lr, grad_scale)
        ops.adam_step(self.sg_params, self.sg_m, self.sg_v, self.sg_grads, lr, self.step, grad_scale=grad_scale)
        ops.sg_lobes(self.sg_params, self.sg_dim, self.lobes)
        self._sg_stale = True

    def sg_moments(self):
        """((m of sg_lambda [K], m of sg_mu_spher [K,2]), (v ...)) on the host, for a checkpoint."""
        K = self.sg_dim
        zero = torch.zeros(3 * K)
        return tuple((a[:K].clone(), a[K:].reshape(K, 2).clone())
                     for a in (getattr(self, n, zero).detach().cpu() for n in ("sg_m", "sg_v")))


class SgModel(models.NerfModel):
    """NerfModel with sg_dim > 0: eval_points_raw (the raw SG coefficients, channel-major like SH) is inherited; apply shades
    with the lobes of the state."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.sg_dim = (cfg.sh_deg + 1) ** 2

    def apply(self, state, rays, randomized, t_rand=None, u=None, seed=0, occupancy=None, live_rows=None):
        if occupancy is not None:
            return self._apply_culled(state, rays, randomized, t_rand, u, seed, occupancy, live_rows, state.lobes)
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


def make_cfg(args):
    """PxoCfg of the SH model with the same head width (sh_deg = sqrt(sg_dim) - 1); args is left as it is."""
    import copy
    a = copy.copy(args)
    a.sh_deg = head_degree(args.sg_dim)
    return models.make_cfg(a)


def get_model_state(args, device, purpose="render"):
    """Model + state with freshly initialised parameters (the caller restores a checkpoint), after the flag check of the
    `purpose` they are built for (families.SG)."""
    from . import families
    families.check_flags(families.SG, args, purpose)
    cfg = make_cfg(args)
    params = models.init_params(cfg, args.seed).to(device)
    lam, mu = init_lobe_params(args.sg_dim, args.seed)
    return SgModel(cfg), SgState(cfg, params, lam, mu)
