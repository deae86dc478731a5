"""Fixture of the reference's view-conditioned torch twin and of its SH projection, written by running the reference's own code:

  keys / shapes / ndim   state dict of octree/nerf/models.py NerfModel(use_viewdirs=True); its contents follow the seeded rule of
                         make_golden_consumers.twin_state_dict (the tests rebuild them from the seed: the file holds no weights)
  points [40,3]          seeded, inside [-1.5, 1.5]^3
  theta, phi, dirs       256 directions from octree/nerf/sh_proj.py spherical_uniform_sampling under torch.manual_seed(7),
                         dirs = spher2cart(theta, phi)
  rgb_cross [40,256,3], rgb_point [40,3] (point i under direction i), sigma [40]
                         eval_points_raw of the twin in FLOAT64 (model.double())
  coeffs_<d> [40, 3K]    d = 0..4: 4 pi / R * sum_r rgb_cross[p,r,c] * EvalSH(l, m, dirs)[r] in float64 with sh_proj's own EvalSH /
                         GetIndex (ProjectFunctionNeRF itself keeps its result in a float32 tensor)
  floor_rgb_cross, floor_rgb_point, floor_sigma, floor_coeffs_<d>
                         max |float32 twin - float64 twin| per quantity: the reference's own round-off.  For the coefficients the
                         float32 side is sh_proj.ProjectFunctionNeRF over the float32 twin, with spherical_uniform_sampling
                         replaced by the stored theta / phi.

Run in the authoring container only, with the reference tree's root as the argument:
    python tests/golden/make_golden_viewdirs.py REFERENCE_TREE
Writes tests/golden/viewdirs_projection.npz.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_consumers import twin_state_dict  # noqa: E402

N_POINTS, N_DIRS = 40, 256
TWIN_KW = dict(num_coarse_samples=64, num_fine_samples=128, use_viewdirs=True, sh_deg=-1, sg_dim=-1, num_rgb_channels=3,
               num_sigma_channels=1)


def points():
    return (torch.rand(N_POINTS, 3, generator=torch.Generator().manual_seed(5)) * 2 - 1) * 1.5


def main(ref):
    sys.path.insert(0, ref)
    from octree.nerf import models as ref_models
    from octree.nerf import sh_proj
    out = {}
    model = ref_models.NerfModel(**TWIN_KW)
    sd = model.state_dict()
    keys, shapes = list(sd), [tuple(v.shape) for v in sd.values()]
    model.load_state_dict(twin_state_dict(keys, shapes))
    out["keys"] = np.array(keys)
    out["shapes"] = np.array([list(s) + [0] * (2 - len(s)) for s in shapes], np.int64)
    out["ndim"] = np.array([len(s) for s in shapes], np.int64)
    pts = points()
    torch.manual_seed(7)
    theta, phi = sh_proj.spherical_uniform_sampling(N_DIRS)
    dirs = sh_proj.spher2cart(theta, phi)
    out["points"], out["theta"], out["phi"], out["dirs"] = pts.numpy(), theta.numpy(), phi.numpy(), dirs.numpy()
    with torch.no_grad():
        rgb32, sig32 = model.eval_points_raw(pts, dirs, cross_broadcast=True)
        rgbp32, _ = model.eval_points_raw(pts, dirs[:N_POINTS])
        sh_proj.spherical_uniform_sampling = lambda count, device="cpu": (theta, phi)
        co32 = {d: sh_proj.ProjectFunctionNeRF(d, lambda v: model.eval_points_raw(pts, v, cross_broadcast=True), N_POINTS, N_DIRS)[0]
                .reshape(N_POINTS, -1).numpy() for d in range(5)}
        m64 = ref_models.NerfModel(**TWIN_KW).double()
        m64.load_state_dict({k: v.double() for k, v in twin_state_dict(keys, shapes).items()})
        rgb64, sig64 = m64.eval_points_raw(pts.double(), dirs.double(), cross_broadcast=True)
        rgbp64, _ = m64.eval_points_raw(pts.double(), dirs[:N_POINTS].double())
    out["rgb_cross"], out["rgb_point"], out["sigma"] = rgb64.numpy(), rgbp64.numpy(), sig64.reshape(-1).numpy()
    out["floor_rgb_cross"] = np.array(float((rgb32.double() - rgb64).abs().max()))
    out["floor_rgb_point"] = np.array(float((rgbp32.double() - rgbp64).abs().max()))
    out["floor_sigma"] = np.array(float((sig32.reshape(-1).double() - sig64.reshape(-1)).abs().max()))
    d64 = dirs.double()
    for d in range(5):
        K = (d + 1) ** 2
        co = torch.zeros(N_POINTS, 3, K, dtype=torch.float64)
        for l in range(d + 1):
            for m in range(-l, l + 1):
                co[:, :, sh_proj.GetIndex(l, m)] = torch.einsum("bsc,s->bc", rgb64, sh_proj.EvalSH(l, m, d64))
        co *= 4.0 * math.pi / N_DIRS
        out[f"coeffs_{d}"] = co.reshape(N_POINTS, -1).numpy()
        out[f"floor_coeffs_{d}"] = np.array(float(np.abs(co32[d].astype(np.float64) - out[f"coeffs_{d}"]).max()))
    dst = os.path.join(HERE, "viewdirs_projection.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes", {k: (getattr(v, "shape", None) if getattr(v, "ndim", 0) else float(v))
                                                       for k, v in out.items() if k.startswith(("floor", "rgb", "coeffs_3"))})


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "octree")):
        raise SystemExit(__doc__)
    main(sys.argv[1])
