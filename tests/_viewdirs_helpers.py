"""Shared by tests/test_viewdirs_cpu.py, tests/test_gpu_viewdirs.py and tests/test_gpu_viewdirs_edges.py: the fixture, its seeded
state dict, a host restatement of the view-conditioned model (octree/nerf/model_utils.py:112-158, octree/nerf/sh_proj.py:278-306;
float64, or float32 to measure the reference arithmetic's own round-off) and the shared inputs, cases and bounds of the edge tests."""
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


def host_model_f64(sd, points, dirs=None, cross=False, mlp=1, dtype=torch.float64):
    """Host restatement, in float64 unless `dtype` says float32 (the same statements, to measure their own round-off): raw_rgb
    ([N,R,3] cross / [N,3] / None without dirs) and raw_sigma [N]."""
    g = lambda name: (sd[f"MLP_{mlp}.{name}.weight"].to(dtype), sd[f"MLP_{mlp}.{name}.bias"].to(dtype))
    inputs = O.posenc(points.to(dtype), 0, 10)
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
    denc = O.posenc(dirs.to(dtype), 0, 4)
    w10, b10 = g("condition_layers.0")
    w11, b11 = g("rgb_layer")
    if cross:
        h = torch.relu((bott @ w10[:, :256].T)[:, None, :] + (denc @ w10[:, 256:].T + b10)[None, :, :])
    else:
        h = torch.relu(torch.cat([bott, denc], -1) @ w10.T + b10)
    return h @ w11.T + b11, sigma


def host_project_f64(rgb_cross, dirs, sh_deg, dtype=torch.float64):
    """coeffs [N, 3K] = 4 pi / R sum_r rgb[p,r,c] Y_k(d_r), channel-major, in float64 unless `dtype` says float32."""
    Y = O.sh_basis(sh_deg, dirs.to(dtype))                                  # [R,K]
    co = torch.einsum("prc,rk->pck", rgb_cross.to(dtype), Y) * (4.0 * math.pi / dirs.shape[0])
    return co.reshape(co.shape[0], -1)


# ---- the edge tests (tests/test_gpu_viewdirs_edges.py; their bound is shown to hold for the reference arithmetic alone by
# tests/test_viewdirs_cpu.py) ---------------------------------------------------------------------------------------------------
EDGE_POINT_N, EDGE_POINT_R = (1, 15, 16, 17, 63, 65, 255, 256, 257, 300), 65     # vd_head groups of 16, vd_pair blocks of 256
EDGE_DIR_N, EDGE_DIR_R = 17, (1, 7, 8, 9, 63, 64, 65, 1001)                      # direction blocks of 8
EDGE_CROSS_N, EDGE_CROSS_R = (1, 17, 257), (1, 7, 9, 65)
EDGE_PER_POINT_N = (1, 7, 8, 9, 255, 256, 257)


def edge_inputs():
    """points [300,3] seeded in [-1.5, 1.5]^3 like the fixture's, dirs [1001,3] seeded unit directions, special [9,3]: the axes
    (where most basis functions vanish) and directions with one or no zero component."""
    from plenoctree_amd.nerf_sh.nerf import viewdirs
    g = torch.Generator().manual_seed(23)
    points = (torch.rand(300, 3, generator=g) * 2 - 1) * 1.5
    dirs = viewdirs.sphere_directions(torch.rand(1001, generator=g), torch.rand(1001, generator=g))
    s = 1.0 / math.sqrt(3.0)
    special = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [0, 0.6, -0.8],
                            [s, s, s]], dtype=torch.float32)
    return dict(points=points, dirs=dirs, special=special)


class EdgeReference:
    """The float64 side of every edge case, computed once: raw colour of the 300 points under the first 65 directions, of the
    first 17 points under all 1001 and under the special ones, point i under direction i, and sigma.  Cases are slices."""

    def __init__(self):
        self.fx = fixture()
        self.sd = seeded_state_dict(self.fx)
        self.inp = edge_inputs()
        p, d, sp = self.inp["points"], self.inp["dirs"], self.inp["special"]
        self.rgb_points, self.sigma = host_model_f64(self.sd, p, d[:EDGE_POINT_R], cross=True)     # [300,65,3], [300]
        self.rgb_dirs, _ = host_model_f64(self.sd, p[:EDGE_DIR_N], d, cross=True)                  # [17,1001,3]
        self.rgb_special, _ = host_model_f64(self.sd, p[:EDGE_DIR_N], sp, cross=True)              # [17,9,3]
        n = max(EDGE_PER_POINT_N)
        self.rgb_per_point, _ = host_model_f64(self.sd, p[:n], d[:n])                              # [257,3]

    def dirs(self, R):
        return self.inp["special"] if R == "special" else self.inp["dirs"][:R].contiguous()

    def cross(self, N, R):
        """float64 raw colour [N,R,3] of points[:N] under dirs(R)."""
        if R == "special":
            return self.rgb_special[:N]
        return self.rgb_points[:N, :R] if R <= EDGE_POINT_R else self.rgb_dirs[:N, :R]

    def coeffs(self, N, R, deg):
        return host_project_f64(self.cross(N, R), self.dirs(R), deg)

    def bound(self, floor, want):
        """4 x floor x max(1, max |want| / max |the fixture's value of that quantity|): the rule of test_extraction_end_to_end for
        inputs other than the fixture's.  floor: "rgb_cross", "rgb_point", "sigma" or "coeffs_<d>"."""
        ref = float(np.abs(self.fx[floor]).max())
        return 4.0 * float(self.fx[f"floor_{floor}"]) * max(1.0, float(torch.as_tensor(want).abs().max()) / ref)


def edge_check(name, got, want, bound, worst=None):
    """max |got - want| <= bound, printed as a multiple of the (scaled) floor; `worst` collects the largest multiple per quantity."""
    err = float((got.detach().cpu().double() - torch.as_tensor(want).double()).abs().max())
    ratio = err / bound * 4
    print(f"{name}: max |got - f64| = {err:.3e}, bound {bound:.3e} ({ratio:.2f} x floor)")
    if worst is not None:
        key = name.split(" ")[0].split("_")[0] if name.startswith("coeffs") else name.split(" ")[0]
        worst[key] = max(worst.get(key, 0.0), ratio)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values"
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
    return ratio
