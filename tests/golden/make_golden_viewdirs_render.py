"""Fixture of ray rendering with the view-conditioned head, written by running the reference's own NerfModel.__call__
(nerf_sh/nerf/models.py:216-348) with use_viewdirs=True, sh_deg=-1: numpy (float32 defaults) stands in for `jax.numpy`, the
random draws are passed in through the `key` arguments, `lax.stop_gradient` is the identity and flax's Dense layers take their
(kernel, bias) from a queue in creation order -- the same kind of shim as make_golden.py uses for nerf_model.npz, restated
here.  Dense creation order inside MLP.__call__ (nerf_sh/nerf/model_utils.py:43-94 with a condition): Dense_0..7 trunk, 8 sigma,
9 bottleneck, 10 condition, 11 rgb -- the arena's order.

  sigma_shift            added to both sigma biases; chosen below so that the fine-level acc spans (< 0.05, > 0.95).  The seeded
                         model's raw sigma is about -0.1 +- 0.05 near the origin and falls with distance, so the list starts
                         well above 0.1: a shift that leaves sigma straddling zero along a ray (0.1 was tried) makes
                         sample_pdf amplify float32 round-off, and the reference's own float32 run then sits 2.9e-5 from
                         float64 on acc -- a fixture no float32 implementation could be held to 2e-5 on
  origins, directions, viewdirs [12,3]
                         cameras on a sphere of radius 4 looking at the origin; viewdirs are unit vectors and
                         directions = viewdirs * norm with norm = 1e-12 / 1e-10 / 1 (four rays each): random weights under a
                         2^10 positional encoding give every ray statistically the same density, so only |directions| (it
                         scales the sample distances, the last one's 1e10 included, model_utils.py:196) makes rays
                         transparent (acc ~ 4e-3), half transparent or opaque.  Norms above 1 are not used: they carry the
                         samples to coordinates of 100 and more, where float32 rounds the argument of the top encoding
                         frequency by ~1e-2 and the reference's own float32 run is 3e-5 off float64 on rgb
  t_rand [12,64], u [12,128]
  {rgb,disp,acc}_{coarse,fine}_r{0,1}
                         the reference's float32 results, randomized false / true, white_bkgd true, near 2, far 6

The weights follow the seeded rule of make_golden_consumers.twin_state_dict over the keys / shapes stored in
viewdirs_projection.npz (tests/_viewdirs_helpers.seeded_state_dict rebuilds them: the file holds no weights).

Run in the authoring container only, with the reference tree's root as the argument:
    python tests/golden/make_golden_viewdirs_render.py REFERENCE_TREE
Writes tests/golden/viewdirs_render.npz.
"""
import dataclasses
import importlib.util
import os
import sys
import types
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_consumers import twin_state_dict  # noqa: E402

NC, NF, NEAR, FAR = 64, 128, 2.0, 6.0
NORMS = (1e-12, 1e-10, 1.0)
SHIFTS = (0.5, 1.0, 2.0, 0.25, 0.0)       # tried in this order
TORCH_NAMES = [f"input_layers.{i}" for i in range(8)] + ["sigma_layer", "bottleneck_layer", "condition_layers.0", "rgb_layer"]
f32 = np.float32


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def rays():
    rng = np.random.default_rng(11)
    cam = rng.normal(size=(12, 3))
    cam = 4.0 * cam / np.linalg.norm(cam, axis=-1, keepdims=True)
    v = -cam / 4.0 + 0.08 * rng.normal(size=(12, 3))
    v = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(f32)
    d = (v * np.repeat(np.array(NORMS, f32), 4)[:, None]).astype(f32)
    t_rand, u = rng.uniform(size=(12, NC)).astype(f32), rng.uniform(size=(12, NF)).astype(f32)
    return cam.astype(f32), d, v, t_rand, u


def install_shim(ref):
    """numpy for jax.numpy, keys = lists of pre-drawn arrays, a flax.linen whose Dense pops (kernel, bias) from a queue."""
    jnp = types.ModuleType("jax.numpy")
    jnp.__dict__.update({k: v for k, v in np.__dict__.items() if not k.startswith("__")})
    jnp.linspace = lambda a, b, n: np.linspace(a, b, n, dtype=f32)          # jax's default dtype is float32
    jnp.zeros = lambda shape, dtype=f32: np.zeros(shape, dtype)
    jnp.ones = lambda shape, dtype=f32: np.ones(shape, dtype)
    jnp.array = lambda x, dtype=None: np.array(x, dtype=dtype or f32)        # int32 * float32 -> float32 in jax
    # jax turns a python list of floats into float32 (model_utils.py:196 broadcasts [1e10]); numpy would make it float64
    jnp.broadcast_to = lambda a, shape: np.broadcast_to(a if isinstance(a, np.ndarray) else np.asarray(a, f32), shape)
    jax = types.ModuleType("jax")
    jrandom, lax, jnn = types.ModuleType("jax.random"), types.ModuleType("jax.lax"), types.ModuleType("jax.nn")
    jrandom.uniform = lambda key, shape: np.asarray(key, f32).reshape(shape)   # the draw IS the key
    jrandom.normal = lambda key, shape, dtype=f32: np.asarray(key, dtype).reshape(shape)
    jrandom.split = lambda key, num=2: (key[0], key[1:])
    lax.stop_gradient = lambda x: x
    jnn.initializers = types.SimpleNamespace(glorot_uniform=lambda: None)
    jax.numpy, jax.random, jax.lax, jax.nn = jnp, jrandom, lax, jnn

    class Module:
        def __init_subclass__(cls, **kw):
            super().__init_subclass__(**kw)
            dataclasses.dataclass(cls, eq=False)

        def __post_init__(self):
            if hasattr(self, "setup"):
                self.setup()

    queue = []

    class Dense:
        def __init__(self, features, kernel_init=None):
            self.features = features

        def __call__(self, x):
            kernel, bias = queue.pop(0)
            assert kernel.shape == (x.shape[-1], self.features), (kernel.shape, x.shape, self.features)
            assert x.dtype == f32 and kernel.dtype == f32 and bias.dtype == f32
            return x @ kernel + bias

    flax, linen = types.ModuleType("flax"), types.ModuleType("flax.linen")
    linen.Module, linen.Dense, linen.compact = Module, Dense, (lambda f: f)
    linen.relu = lambda x: np.maximum(x, 0)
    linen.sigmoid = lambda x: (1.0 / (1.0 + np.exp(-x))).astype(f32)
    flax.linen = linen
    sys.modules.update({"jax": jax, "jax.numpy": jnp, "jax.random": jrandom, "jax.lax": lax, "jax.nn": jnn, "flax": flax,
                        "flax.linen": linen})
    ref_sh = types.ModuleType("nerf_sh.nerf.sh")          # not reached with sh_deg = -1
    ref_jmu = _load("nerf_sh.nerf.model_utils", os.path.join(ref, "nerf_sh/nerf/model_utils.py"))
    Rays = namedtuple("Rays", ("origins", "directions", "viewdirs"))
    pkg, pkg_nerf = types.ModuleType("nerf_sh"), types.ModuleType("nerf_sh.nerf")
    utils_stub, sg_stub = types.ModuleType("nerf_sh.nerf.utils"), types.ModuleType("nerf_sh.nerf.sg")
    utils_stub.Rays = Rays
    pkg.nerf = pkg_nerf
    pkg_nerf.model_utils, pkg_nerf.utils, pkg_nerf.sh, pkg_nerf.sg = ref_jmu, utils_stub, ref_sh, sg_stub
    sys.modules.update({"nerf_sh": pkg, "nerf_sh.nerf": pkg_nerf, "nerf_sh.nerf.utils": utils_stub, "nerf_sh.nerf.sg": sg_stub,
                        "nerf_sh.nerf.sh": ref_sh})
    ref_models = _load("nerf_sh.nerf.models", os.path.join(ref, "nerf_sh/nerf/models.py"))
    return ref_models, linen, queue, Rays


def main(ref):
    ref_models, linen, queue, Rays = install_shim(ref)
    fx = np.load(os.path.join(HERE, "viewdirs_projection.npz"))
    shapes = [tuple(int(n) for n in s[:int(nd)]) for s, nd in zip(fx["shapes"], fx["ndim"])]
    sd = twin_state_dict(list(fx["keys"]), shapes)
    model = ref_models.NerfModel(
        num_coarse_samples=NC, num_fine_samples=NF, use_viewdirs=True, sh_deg=-1, sg_dim=-1, near=NEAR, far=FAR, noise_std=None,
        net_depth=8, net_width=256, net_depth_condition=1, net_width_condition=128, net_activation=linen.relu, skip_layer=4,
        num_rgb_channels=3, num_sigma_channels=1, white_bkgd=True, min_deg_point=0, max_deg_point=10, deg_view=4, lindisp=False,
        rgb_activation=linen.sigmoid, sigma_activation=linen.relu, legacy_posenc_order=False)
    cam, d, v, t_rand, u = rays()
    out = None
    for shift in SHIFTS:
        weights = []
        for mi in range(2):
            for li, name in enumerate(TORCH_NAMES):
                kernel = np.ascontiguousarray(sd[f"MLP_{mi}.{name}.weight"].numpy().T.astype(f32))
                bias = sd[f"MLP_{mi}.{name}.bias"].numpy().astype(f32)
                weights.append((kernel, bias + f32(shift) if li == 8 else bias))
        cur = dict(origins=cam, directions=d, viewdirs=v, t_rand=t_rand, u=u, sigma_shift=np.array(shift, f32),
                   near=np.array(NEAR, f32), far=np.array(FAR, f32))
        for randomized in (False, True):
            queue[:] = list(weights)
            ret = model(*([t_rand, None], [u, None], Rays(cam, d, v), randomized))
            assert not queue
            for lvl, (rgb_, disp_, acc_) in zip(("coarse", "fine"), ret):
                for name, val in (("rgb", rgb_), ("disp", disp_), ("acc", acc_)):
                    assert np.asarray(val).dtype == f32, (name, np.asarray(val).dtype)
                    cur[f"{name}_{lvl}_r{int(randomized)}"] = np.asarray(val, f32)
        spans = [(float(cur[f"acc_fine_r{r}"].min()), float(cur[f"acc_fine_r{r}"].max())) for r in (0, 1)]
        print(f"sigma shift {shift}: fine acc spans {spans}")
        if all(lo < 0.05 and hi > 0.95 for lo, hi in spans):
            out = cur
            break
    assert out is not None, "no listed sigma shift gives a fine-level acc spanning (< 0.05, > 0.95): widen the norm spread"
    dst = os.path.join(HERE, "viewdirs_render.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; acc_fine_r0 =", np.round(out["acc_fine_r0"], 4))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "nerf_sh")):
        raise SystemExit(__doc__)
    main(sys.argv[1])
