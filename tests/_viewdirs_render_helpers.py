"""Shared by tests/test_viewdirs_render_cpu.py and tests/test_gpu_viewdirs_render.py: the ray-rendering fixture of the
view-conditioned model (tests/golden/viewdirs_render.npz), its seeded weights and a float64 restatement of
NerfModel.__call__ with use_viewdirs (nerf_sh/nerf/models.py:216-348) composed of the oracle's pieces."""
import os
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from oracle import nerf_oracle as O
from _viewdirs_helpers import fixture as projection_fixture, host_model_f64, seeded_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viewdirs_render.npz")
Rays = namedtuple("Rays", ("origins", "directions", "viewdirs"))

# the project's R1 bounds for rendered quantities against the reference's own float32 run (tests/test_gpu_reference_fixtures.py)
RGB_ATOL, ACC_ATOL, DISP_RTOL, DISP_ATOL = 2e-5, 2e-5, 2e-3, 1e-6


def fixture():
    return np.load(GOLDEN)


def fixture_state_dict(fx=None):
    """The seeded weights of the fixture: _viewdirs_helpers.seeded_state_dict plus the stored shift of both sigma biases."""
    fx = fixture() if fx is None else fx
    sd = seeded_state_dict(projection_fixture())
    for mi in range(2):
        sd[f"MLP_{mi}.sigma_layer.bias"] = sd[f"MLP_{mi}.sigma_layer.bias"] + torch.tensor(fx["sigma_shift"])
    return sd


def fixture_rays(fx, dtype=torch.float32):
    return Rays(*[torch.from_numpy(fx[k]).to(dtype) for k in ("origins", "directions", "viewdirs")])


def render_cfg(num_coarse_samples=64, num_fine_samples=128, near=2.0, far=6.0, white_bkgd=True, lindisp=False, noise_std=None):
    return SimpleNamespace(num_coarse_samples=num_coarse_samples, num_fine_samples=num_fine_samples, near=near, far=far,
                           white_bkgd=white_bkgd, lindisp=lindisp, noise_std=noise_std)


def host_render_f64(sd, rays, cfg, t_rand=None, u=None, noise_c=None, noise_f=None):
    """[(rgb, disp, acc)_coarse, (rgb, disp, acc)_fine] in float64: sample_along_rays, volumetric_rendering and sample_pdf of the
    oracle around host_model_f64 in its per-point form (viewdirs repeated per sample), sigmoid and relu.  noise_c [B,Nc] /
    noise_f [B,Nc+Nf]: the standard-normal draws of add_gaussian_noise on raw sigma (cfg.noise_std set), before the relu."""
    o, d, v = (r.double() for r in rays)
    t_rand = None if t_rand is None else t_rand.double()
    u = None if u is None else u.double()

    def shade(mlp, samples, noise):
        B, S = samples.shape[:2]
        raw_rgb, raw_sigma = host_model_f64(sd, samples.reshape(-1, 3), v[:, None, :].expand(B, S, 3).reshape(-1, 3), mlp=mlp)
        raw_sigma = O.add_gaussian_noise(raw_sigma, cfg.noise_std, None if noise is None else noise.double())
        return torch.sigmoid(raw_rgb).reshape(B, S, 3), torch.relu(raw_sigma).reshape(B, S, 1)

    z, samples = O.sample_along_rays(o, d, cfg.num_coarse_samples, cfg.near, cfg.far, t_rand, cfg.lindisp)
    rgb, sigma = shade(0, samples, noise_c)
    comp, disp, acc, weights = O.volumetric_rendering(rgb, sigma, z, d, cfg.white_bkgd)
    ret = [(comp, disp, acc)]
    if cfg.num_fine_samples > 0:
        z_mid = 0.5 * (z[..., 1:] + z[..., :-1])
        z, samples = O.sample_pdf(z_mid, weights[..., 1:-1], o, d, z, cfg.num_fine_samples, u)
        rgb, sigma = shade(1, samples, noise_f)
        comp, disp, acc, _ = O.volumetric_rendering(rgb, sigma, z, d, cfg.white_bkgd)
        ret.append((comp, disp, acc))
    return ret


def errors(got, want):
    """(max |rgb diff|, max |acc diff|, max of |disp diff| - DISP_RTOL |want disp|) of one level; inputs: (rgb, disp, acc)."""
    g = [np.asarray(x.detach().cpu() if hasattr(x, "detach") else x, np.float64) for x in got]
    w = [np.asarray(x.detach().cpu() if hasattr(x, "detach") else x, np.float64) for x in want]
    return (float(np.abs(g[0] - w[0]).max()), float(np.abs(g[2] - w[2]).max()),
            float((np.abs(g[1] - w[1]) - DISP_RTOL * np.abs(w[1])).max()))


def check_level(name, got, want):
    """Prints the measured errors of one level, then holds them to the R1 bounds."""
    e_rgb, e_acc, e_disp = errors(got, want)
    print(f"{name}: max |rgb| err {e_rgb:.3e} (bound {RGB_ATOL:.0e}), |acc| err {e_acc:.3e} (bound {ACC_ATOL:.0e}), "
          f"disp excess over rtol {DISP_RTOL:.0e}: {e_disp:.3e} (bound {DISP_ATOL:.0e})")
    assert e_rgb <= RGB_ATOL, f"{name}: rgb {e_rgb:.3e}"
    assert e_acc <= ACC_ATOL, f"{name}: acc {e_acc:.3e}"
    assert e_disp <= DISP_ATOL, f"{name}: disp {e_disp:.3e}"
