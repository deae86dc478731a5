"""Cases, input builders and bounds of the density-noise tests (PxoCfg.noise_std > 0, and lindisp through the whole path),
shared by tests/test_noise_cpu.py (the conditions that keep the GPU tests from passing vacuously, on the oracle alone) and
tests/test_gpu_noise.py (HIP vs the oracle), so that the two cannot drift apart.

The normals.  The whole path draws them from Philox streams 3 (coarse, B*Nc elements) and 4 (fine, B*(Nc+Nf) elements) of the
step's seed.  A GPU test draws the same streams once through pxo_add_gaussian_noise on zeros, holds them to the host
restatement _helpers.philox_normal (2e-6, the bar of test_gaussian_noise_against_reference) and hands them, as float64, to
the oracle: the rule (stream, seed, element) is pinned by the restatement, the arithmetic by the oracle at the numbers drawn.
The CPU test uses the restatement itself, rounded to float32."""
import os

import torch

from _helpers import make_params, make_rays, oracle_loss_and_grad_given_z, philox_normal
from oracle import nerf_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 7                        # the step's seed; the streams are (SEED, 3) and (SEED, 4)
STREAM_COARSE, STREAM_FINE = 3, 4
NORMAL_ATOL = 2e-6              # device normals against philox_normal (values up to ~5, float32 log / sincos)
# the bounds of test_gpu_parity.py::test_train_fwd_bwd_matches_oracle
LOSS_RTOL, LOSS_ATOL = 1e-5, 1e-7
PSNR_RTOL, PSNR_ATOL = 2e-5, 1e-6
GRAD_FLOOR, GRAD_FACTOR, E_F32_CAP = 1e-3, 3.0, 4e-3      # gradient rel L2 <= max(1e-3, 3 e_f32), e_f32 <= 4e-3: at most 1.2e-2

# ---- the training step: every field other than the ones a case names keeps its default -----------------------------------------
_DEFAULT = dict(B=48, Nc=64, Nf=128, deg=3, white=True, near=2.0, far=6.0, lindisp=False, std=0.3, wd=0.0, prec=0, rays="synthetic")
TRAIN_CASES = {
    "i-48x64+128-std0.3": {},
    "ii-llff-ndc-64x16+32-std1": dict(B=64, Nc=16, Nf=32, near=0.0, far=1.0, white=False, std=1.0, rays="llff"),   # config/llff.yaml
    "iii-coarse-only": dict(Nf=0),
    "iv-5x13+20-sh4-std1": dict(B=5, Nc=13, Nf=20, deg=1, std=1.0),        # B*Nc = 65 and B*(Nc+Nf) = 165 end inside a Philox quad
    "v-bf16x6": dict(prec=2),
    "vi-weight-decay": dict(wd=0.05),
}
LINDISP_CASES = {
    "lindisp-noise-off": dict(near=0.5, far=4.0, lindisp=True, std=None),
    "lindisp-std0.3": dict(near=0.5, far=4.0, lindisp=True, std=0.3),
}
N_SPARSITY = 300


def case(name):
    return dict(_DEFAULT, **{**TRAIN_CASES, **LINDISP_CASES}[name])


def oracle_cfg(c):
    return O.Cfg(sh_deg=c["deg"], num_coarse_samples=c["Nc"], num_fine_samples=c["Nf"], near=c["near"], far=c["far"],
                 white_bkgd=c["white"], lindisp=c["lindisp"], noise_std=c["std"], weight_decay_mult=c["wd"],
                 sparsity_npoints=N_SPARSITY, sparsity_weight=1e-3)


def llff_args():
    from plenoctree_amd.nerf_sh.nerf import utils
    a = utils.define_flags().parse_args(["--config", "llff", "--train_dir", "x", "--data_dir", os.path.join(HERE, "golden", "llff_tiny")])
    utils.update_flags(a)
    a.factor = 0
    return a


def train_inputs(c, device=torch.device("cpu")):
    """(cfg, flat MLP arena, rays, pixels, t_rand, u, sparsity points) of a case, on the host in float32.  `device`: where the
    LLFF dataset draws its NDC batch (the GPU in the GPU tests, as test_one_training_step_in_the_ndc_regime obtains it)."""
    cfg = oracle_cfg(c)
    B, Nc, Nf = c["B"], c["Nc"], c["Nf"]
    flat = make_params(cfg, bias_scale=0.2)
    gen = torch.Generator().manual_seed(53)
    if c["rays"] == "llff":
        from plenoctree_amd.nerf_sh.nerf import llff
        batch = next(llff.get_dataset("train", llff_args(), device, batch_size=B, seed=3))
        rays = O.Rays(*[r.cpu().contiguous() for r in batch["rays"]])
        px = batch["pixels"].cpu().contiguous()
    else:
        rays = make_rays(B, 51)
        px = torch.rand(B, 3, generator=gen)
    t_rand = torch.rand(B, Nc, generator=gen)
    u = torch.rand(B, max(Nf, 1), generator=gen)
    sp = (torch.rand(N_SPARSITY, 3, generator=gen) * 2 - 1) * 1.5
    return cfg, flat, rays, px, t_rand, u, sp


def host_normals(B, Nc, Nf, seed=SEED):
    """(N_c [B,Nc], N_f [B,Nc+Nf] or None): the host restatement of the two streams, rounded to float32 as the device holds them."""
    n_c = torch.from_numpy(philox_normal(seed, STREAM_COARSE, B * Nc)).float().reshape(B, Nc)
    n_f = torch.from_numpy(philox_normal(seed, STREAM_FINE, B * (Nc + Nf))).float().reshape(B, Nc + Nf) if Nf > 0 else None
    return n_c, n_f


def rel_l2_per_mlp(g, ref, fine=True):
    """Relative L2 of each MLP's half of the flat gradient against `ref` (float64); the second entry is None without a fine level."""
    n = ref.numel() // 2
    halves = [(0, n)] + ([(n, 2 * n)] if fine else [])
    out = [float((g[lo:hi].double() - ref[lo:hi]).norm() / ref[lo:hi].norm()) for lo, hi in halves]
    return out + [None] * (2 - len(out))


def oracle_at(inputs, z_c, z_f, n_c, n_f, dtype=torch.float64):
    """(loss, loss_c, gradient) of the oracle's loss_fn in `dtype` at the given positions and normals (None: no noise)."""
    cfg, flat, rays, px, t_rand, u, sp = inputs
    d = lambda t: None if t is None else t.double()
    return oracle_loss_and_grad_given_z(flat, rays, px, cfg, z_c, z_f, sp, dtype=dtype, noise_c=d(n_c), noise_f=d(n_f))


def grad_bound(e_f32):
    return max(GRAD_FLOOR, GRAD_FACTOR * e_f32)
