"""The view-conditioned ("vanilla") NeRF of the reference: extraction by SH projection, and ray rendering (eval, gen_video).

Host-side mirror of the torch twin with use_viewdirs=True (octree/nerf/models.py:116-252 over octree/nerf/model_utils.py:64-158,
net_depth_condition 1, net_width_condition 128, deg_view 4): per MLP twelve dense layers in flax key order -- Dense_0..7 trunk,
Dense_8 sigma, Dense_9 bottleneck, Dense_10 condition, Dense_11 rgb -- in one flat float32 arena (MLP_0 then MLP_1).  All
arithmetic is done by libplenoctree_hip.so (csrc/viewdirs_kernels.hip) through plenoctree_amd.ops.  Training with this head is
not built: nerf_sh.train keeps rejecting use_viewdirs=true (utils.check_supported); what nerf_sh.eval, nerf_sh.gen_video and
octree.extraction build of such a model, and which checkpoints they read, is the view-conditioned row of families.py.
"""
import math

import torch

from ... import ops
from . import models

DIRECTION_STREAM = 16        # Philox stream id of the projection's direction draw (0..4: the train step's draws)


class ViewdirsState(models.Workspace):
    """Parameters of the two MLPs and the images the kernels stream.  `packed[i][0]` starts with the forward image of an SH model
    of degree 0 (trunk + Dense_8), so the sigma-only consumers of a TrainState (extraction.grid_sigma) take this state as it is."""

    def __init__(self, params):
        self.params = params
        self.step = 0                # no optimiser state is restored: what eval names its per-step summary files with
        self.n_mlp = params.numel() // 2
        self.packed = [None, None]
        self.repack()

    def mlp_params(self, i):
        return self.params[i * self.n_mlp:(i + 1) * self.n_mlp]

    def repack(self):
        for i in range(2):
            img = self.packed[i][0] if self.packed[i] is not None else None
            self.packed[i] = (ops.vd_pack_weights(self.mlp_params(i), img), None)


class ViewdirsModel:
    def __init__(self, num_coarse_samples=64, num_fine_samples=128, mlp_precision=0, near=2.0, far=6.0, white_bkgd=True,
                 lindisp=False, noise_std=None):
        # the SH model of degree 0 whose forward image opens the packed image: what pxo_grid_sigma is called with; the ray
        # renderer reads its sample counts, near / far, lindisp, white_bkgd and noise_std
        self.cfg = ops.make_cfg(num_coarse_samples=num_coarse_samples, num_fine_samples=num_fine_samples, sh_deg=0, near_=near,
                                far_=far, white_bkgd=int(bool(white_bkgd)), lindisp=int(bool(lindisp)),
                                noise_std=0.0 if noise_std is None else noise_std, mlp_precision=mlp_precision)
        self.num_coarse_samples = num_coarse_samples
        self.num_fine_samples = num_fine_samples
        self.mlp_precision = mlp_precision

    def _which(self, coarse):
        return 1 if (self.num_fine_samples > 0 and not coarse) else 0

    def apply(self, state, rays, randomized, t_rand=None, u=None, seed=0):
        """model.apply(variables, key_0, key_1, rays, randomized) with use_viewdirs (nerf_sh/nerf/models.py:216-348): returns
        [(rgb, disp, acc)_coarse, (rgb, disp, acc)_fine].  The jax keys are replaced by explicit uniforms (t_rand [B,Nc],
        u [B,Nf]) or a Philox `seed`, as in NerfModel.apply."""
        ws = state.workspace(ops.vd_render_workspace_bytes(self.cfg, rays.origins.shape[0]))
        return ops.vd_render_fwd(self.cfg, state.packed[0][0], state.packed[1][0], rays.origins, rays.directions, rays.viewdirs,
                                 randomized=randomized, t_rand=t_rand, u=u, seed=seed, ws=ws)

    __call__ = apply

    def eval_points_raw(self, state, points, viewdirs=None, coarse=False, cross_broadcast=False):
        """octree/nerf/models.py:211-252: raw_rgb [N,3] (viewdirs [N,3]) or [N,R,3] (cross_broadcast, viewdirs [R,3]), raw
        sigma [N,1]."""
        N = points.reshape(-1, 3).shape[0]
        R = viewdirs.shape[0] if viewdirs is not None else 0
        ws = state.workspace(ops.vd_eval_workspace_bytes(N, R, cross_broadcast))
        rgb, sigma = ops.vd_eval_points_raw(state.packed[self._which(coarse)][0], points, viewdirs, cross_broadcast, ws=ws,
                                            mlp_precision=self.mlp_precision)
        return rgb, sigma.view(-1, 1)

    def project_sh(self, state, points, dirs, sh_deg, coarse=False, coeffs=None, raw_sigma=None):
        """project_nerf_to_sh (octree/extraction.py:217-241) for a given direction set: coeffs [N,3K], raw sigma [N]."""
        N = points.reshape(-1, 3).shape[0]
        ws = state.workspace(ops.vd_project_workspace_bytes(N, dirs.shape[0]))
        return ops.vd_project_sh(state.packed[self._which(coarse)][0], points, dirs, sh_deg, ws=ws, coeffs=coeffs,
                                 raw_sigma=raw_sigma, mlp_precision=self.mlp_precision)


def init_params(seed=20200823):
    """Glorot-uniform kernels, zero biases, host RNG (as nerf.models.init_params)."""
    return models.glorot_arena(*ops.vd_param_layout(), seed)


def get_model_state(args, device, purpose="extract"):
    """Model + state with freshly initialised parameters (the caller restores a checkpoint), after the flag check of the
    `purpose` they are built for (families.VIEWDIRS): the SH projection's, or the ray renderer's."""
    from . import families
    families.check_flags(families.VIEWDIRS, args, purpose)
    model = ViewdirsModel(args.num_coarse_samples, args.num_fine_samples, near=args.near, far=args.far,
                          white_bkgd=args.white_bkgd, lindisp=args.lindisp, noise_std=args.noise_std)
    return model, ViewdirsState(init_params(args.seed).to(device))


def add_checkpoint_flags(parser):
    """The checkpoint flags of octree.extraction (same names) for the CLIs that render a view-conditioned model."""
    from . import utils
    parser.add_argument("--is_jaxnerf_ckpt", type=utils._bool, nargs="?", const=True, default=False)
    parser.add_argument("--trust_ckpt_pickle", type=utils._bool, nargs="?", const=True, default=False)
    return parser


def sphere_directions(u, v):
    """spherical_uniform_sampling + spher2cart (octree/nerf/sh_proj.py:241-245, 28-33) for given uniforms u, v in [0,1):
    theta = acos(2u - 1), phi = 2 pi v -> unit vectors [R,3] (float64 arithmetic, rounded once to float32)."""
    u, v = u.double(), v.double()
    theta = torch.acos(2.0 * u - 1.0)
    phi = 2.0 * math.pi * v
    r = torch.sin(theta)
    return torch.stack([r * torch.cos(phi), r * torch.sin(phi), torch.cos(theta)], dim=-1).float().contiguous()


def draw_directions(seed, count, device):
    """The run's ONE direction set: 2 * count uniforms of Philox stream (seed, DIRECTION_STREAM), u first, then v."""
    uv = ops.uniform(seed, DIRECTION_STREAM, 2 * count, device=device)
    return sphere_directions(uv[:count], uv[count:])
