"""Shared by tests/test_viewdirs_cpu.py and tests/test_gpu_viewdirs.py: the fixture, its seeded state dict and a float64 host
restatement of the view-conditioned model (octree/nerf/model_utils.py:112-158, octree/nerf/sh_proj.py:278-306)."""
import math
import os

import numpy as np
import torch

from oracle import nerf_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "viewdirs_projection.npz")


def fixture():
    return np.load(GOLDEN)


def seeded_state_dict(fx, scale=1.0):
    """tests/golden/make_golden_consumers.py twin_state_dict: weights ~ N(0, 1 / fan_in), biases ~ N(0, 0.01^2), generator
    seeded 1000 + position of the key."""
    out = {}
    for i, (k, s, nd) in enumerate(zip(fx["keys"], fx["shapes"], fx["ndim"])):
        s = tuple(int(n) for n in s[:int(nd)])
        t = torch.randn(s, generator=torch.Generator().manual_seed(1000 + i))
        out[str(k)] = (t / float(np.sqrt(s[1])) if len(s) == 2 else 0.01 * t) * scale
    return out


def host_model_f64(sd, points, dirs=None, cross=False, mlp=1):
    """float64 restatement: raw_rgb ([N,R,3] cross / [N,3] / None without dirs) and raw_sigma [N]."""
    g = lambda name: (sd[f"MLP_{mlp}.{name}.weight"].double(), sd[f"MLP_{mlp}.{name}.bias"].double())
    inputs = O.posenc(points.double(), 0, 10)
    x = inputs
    for i in range(8):
        w, b = g(f"input_layers.{i}")
        x = torch.relu(x @ w.T + b)
        if i % 4 == 0 and i > 0:
            x = torch.cat([x, inputs], -1)
    w, b = g("sigma_layer")
    sigma = (x @ w.T + b).reshape(-1)
    if dirs is None:
        return None, sigma
    w, b = g("bottleneck_layer")
    bott = x @ w.T + b
    denc = O.posenc(dirs.double(), 0, 4)
    w10, b10 = g("condition_layers.0")
    w11, b11 = g("rgb_layer")
    if cross:
        h = torch.relu((bott @ w10[:, :256].T)[:, None, :] + (denc @ w10[:, 256:].T + b10)[None, :, :])
    else:
        h = torch.relu(torch.cat([bott, denc], -1) @ w10.T + b10)
    return h @ w11.T + b11, sigma


def host_project_f64(rgb_cross, dirs, sh_deg):
    """coeffs [N, 3K] = 4 pi / R sum_r rgb[p,r,c] Y_k(d_r) in float64, channel-major."""
    Y = O.sh_basis(sh_deg, dirs.double())                                   # [R,K]
    co = torch.einsum("prc,rk->pck", rgb_cross.double(), Y) * (4.0 * math.pi / dirs.shape[0])
    return co.reshape(co.shape[0], -1)
