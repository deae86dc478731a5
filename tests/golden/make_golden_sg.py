"""Generate tests/golden/sg_reference.npz by IMPORTING the reference's own spherical-Gaussian code (method of make_golden.py).

Run in the authoring container only (needs /root/reference):
    python tests/golden/make_golden_sg.py
Reference code executed, in place:
  nerf_sh/nerf/sg.py        eval_sg, spher2cart -- with numpy standing in for `jax.numpy` and a numpy softplus for
                            `jax.nn.softplus`, i.e. the REFERENCE'S OWN FUNCTION BODIES run by numpy, in float64
  octree/nerf/sh_proj.py    spher2cart (torch), for the lobes expression of octree/extraction.py:439-442, restated here
                            verbatim on float64 tensors: cat(softplus(sg_lambda[:, None]), spher2cart(theta, phi))
Inputs are float32-representable numbers (what a checkpoint holds), outputs are float64.

Per K in {1, 4, 9, 16, 25}:
  sg_lambda_K [K] f32, sg_mu_spher_K [K,2] f32   raw parameters; lobe 0: raw lambda 30 (sharp) at theta = 0, i.e. mu = +z
                                                 exactly; lobe 1 (K >= 4): raw lambda -5 (softplus 0.0067: basis ~ 1/K
                                                 everywhere); the rest random, raw lambda in [-2, 4]
  coeffs_K [16,3,K] f32                          uniform in [-2, 2]
  out_K [16,3] f64                               eval_sg(sg_lambda, sg_mu_spher, coeffs, dirs)
  basis_K [16,K] f64                             eval_sg with identity coefficients: exp(lambda_i (mu_i . d - 1)) / K
  lobes_K [K,4] f64                              the extraction.py:439-442 expression
dirs [16,3] f32: dirs[0] = +z (parallel to lobe 0: basis exactly 1/K), dirs[1] = -z (anti-parallel: exp(-60)), the rest
random unit vectors (normalised in float64, rounded to float32).
"""
import os
import sys
import types
import importlib.util

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
KS = (1, 4, 9, 16, 25)
N_DIRS = 16
COEF_RANGE = 2.0
SHARP_RAW, SOFT_RAW = 30.0, -5.0


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _numpy_jax():
    """`jax` / `jax.numpy` stand-ins: numpy, and softplus(x) = log(1 + exp(x)) evaluated stably."""
    jax, nn = types.ModuleType("jax"), types.ModuleType("jax.nn")
    nn.softplus = lambda x: np.logaddexp(np.asarray(x), 0.0)
    jax.nn, jax.numpy = nn, np
    return {"jax": jax, "jax.nn": nn, "jax.numpy": np}


def main():
    saved = {k: sys.modules.get(k) for k in ("jax", "jax.nn", "jax.numpy")}
    sys.modules.update(_numpy_jax())
    try:
        ref_sg = _load("ref_sg", os.path.join(REF, "nerf_sh/nerf/sg.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    ref_proj = _load("ref_sh_proj", os.path.join(REF, "octree/nerf/sh_proj.py"))

    rng = np.random.default_rng(25)
    d = rng.normal(size=(N_DIRS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[0] = [0.0, 0.0, 1.0]
    d[1] = [0.0, 0.0, -1.0]
    dirs = d.astype(np.float32)
    out = {"dirs": dirs, "coef_range": np.float64(COEF_RANGE)}
    for K in KS:
        lam = rng.uniform(-2.0, 4.0, size=K).astype(np.float32)
        mu = np.stack([rng.uniform(0.0, np.pi, size=K), rng.uniform(0.0, 2.0 * np.pi, size=K)], -1).astype(np.float32)
        lam[0], mu[0] = SHARP_RAW, (0.0, 0.7)
        if K >= 4:
            lam[1] = SOFT_RAW
        coeffs = rng.uniform(-COEF_RANGE, COEF_RANGE, size=(N_DIRS, 3, K)).astype(np.float32)
        lam64, mu64, dirs64 = lam.astype(np.float64), mu.astype(np.float64), dirs.astype(np.float64)
        out[f"sg_lambda_{K}"], out[f"sg_mu_spher_{K}"], out[f"coeffs_{K}"] = lam, mu, coeffs
        out[f"out_{K}"] = np.asarray(ref_sg.eval_sg(lam64, mu64, coeffs.astype(np.float64), dirs64), np.float64)
        eye = np.broadcast_to(np.eye(K), (N_DIRS, K, K))
        out[f"basis_{K}"] = np.asarray(ref_sg.eval_sg(lam64, mu64, eye, dirs64), np.float64)
        tl, tm = torch.from_numpy(lam64), torch.from_numpy(mu64)
        lobes = torch.cat((torch.nn.functional.softplus(tl[:, None]), ref_proj.spher2cart(tm[:, 0], tm[:, 1])), dim=-1)
        out[f"lobes_{K}"] = lobes.numpy().astype(np.float64)
        # the two ways the reference turns (theta, phi) into a vector agree
        assert np.abs(np.asarray(ref_sg.spher2cart(1.0, mu64[:, 0], mu64[:, 1])) - out[f"lobes_{K}"][:, 1:]).max() < 1e-15
        assert out[f"basis_{K}"][0, 0] == 1.0 / K and out[f"basis_{K}"][1, 0] < 1e-25
    np.savez_compressed(os.path.join(HERE, "sg_reference.npz"), **out)
    print("wrote", os.path.join(HERE, "sg_reference.npz"), os.path.getsize(os.path.join(HERE, "sg_reference.npz")), "bytes")


if __name__ == "__main__":
    main()
