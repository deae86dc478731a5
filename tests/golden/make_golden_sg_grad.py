"""NeRF-SG gradient fixture from the REFERENCE'S OWN train_step, by the method of make_golden_grad.py: nerf_sh/train.py:51-121
with nerf_sh/nerf/models.py (NerfModel.__call__ and eval_points_raw with sg_dim = 25, sh_deg = -1), model_utils.py and
nerf_sh/nerf/sg.py (eval_sg, spher2cart) imported from the reference checkout (make_golden_grad.REF) at run time and executed by the torch-backed stand-ins
of make_golden_grad.Shim, extended here by what the SG branch needs:

  * flax's Module.variable("params", name, init, ...) -> a holder whose .value is the leaf tensor fed in (no init call),
  * jnp.einsum / jnp.cos -> torch.einsum / torch.cos, jax.nn.softplus -> torch.logaddexp(x, 0),
  * random.split of the constant key that setup() derives for the SG initialiser -> placeholders (the initialiser never runs),
  * the SG leaves ride in optimizer.target as a third (sg_lambda, sg_mu_spher) pair beside the two MLPs' (kernel, bias) pairs,
    so the shim's jax.value_and_grad and jax.tree_util.tree_reduce differentiate and count them like any other leaf.

So the stored gradients -- the MLPs' and d loss / d(sg_lambda, sg_mu_spher) -- are reverse-mode AD through the reference's
function bodies.  Run where the reference checkout is present:
    python tests/golden/make_golden_sg_grad.py
Writes tests/golden/sg_train_grad.npz.  MLP weights: those of eval_points_sh25.npz (the head width of sg_dim 25) with the
sigma-head bias of both MLPs raised by 0.5, as in train_grad.npz.  SG parameters: float32 draws, stored.  Rays, pixels, t_rand,
u and sp_u have the shapes of train_grad.npz (24 rays, 64 + 128 samples, 500 sparsity points).

Size.  A committed file is limited to 1 MiB and the float32 gradient of the two MLPs is 4.1 MB, so the file keeps the entries
selected by tests/_sg_train_oracle.fixture_index (every bias, Dense_0 and the heads whole, every 8th input row of the trunk
kernels: 194,200 of 1,025,176 floats, every leaf represented) of the float64 run, rounded once to float32; the float32-vs-
float64 floors of the MLPs are taken over the same entries.  The SG gradient is kept whole, in float64.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_grad as G                      # noqa: E402
import _sg_train_oracle as T                      # noqa: E402
from oracle import nerf_oracle as O               # noqa: E402

K = 25


class SgShim(G.Shim):
    def __init__(self, dtype):
        super().__init__(dtype)
        jnp, jax, jrandom = sys.modules["jax.numpy"], sys.modules["jax"], sys.modules["jax.random"]
        jnp.cos, jnp.einsum = torch.cos, torch.einsum
        jax.nn.softplus = lambda x: torch.logaddexp(x, torch.zeros_like(x))      # jax's definition: no linear branch
        split = jrandom.split
        jrandom.split = lambda key, num=2: (None,) * num if key is None else split(key, num)
        self.linen.Module.variable = lambda self_, col, name, init, *a: types.SimpleNamespace(value=None)
        self.sg = G._load("nerf_sh.nerf.sg", os.path.join(G.REF, "nerf_sh/nerf/sg.py"))
        sys.modules["nerf_sh.nerf"].sg = self.sg
        self.models.sg = self.sg                  # models.py bound the name at import

    def sg_model(self):
        return self.models.NerfModel(
            num_coarse_samples=64, num_fine_samples=128, use_viewdirs=False, sh_deg=-1, sg_dim=K, near=2.0, far=6.0,
            noise_std=None, net_depth=8, net_width=256, net_depth_condition=1, net_width_condition=128,
            net_activation=self.linen.relu, skip_layer=4, num_rgb_channels=3 * K, num_sigma_channels=1,
            white_bkgd=True, min_deg_point=0, max_deg_point=10, deg_view=4, lindisp=False,
            rgb_activation=self.linen.sigmoid, sigma_activation=self.linen.relu, legacy_posenc_order=False)

    def sg_train_step(self, weights_np, sg_lambda, sg_mu_spher, batch_np, t_rand, u, sp_u, fl):
        """The reference's train_step on one replica.  Returns (stats dict, MLP gradient tree, (d sg_lambda, d sg_mu_spher))."""
        Tn, queue = self.T, self.weight_queue
        self.flags.FLAGS.__dict__.update(fl)
        model = self.sg_model()
        mk = lambda a: torch.tensor(a, dtype=self.dtype, requires_grad=True)
        target = [[(mk(k), mk(b)) for k, b in mlp] for mlp in weights_np] + [[(mk(sg_lambda), mk(sg_mu_spher))]]

        class ModelApply:
            def apply(self_, variables, *args, method=None):
                model.sg_lambda.value, model.sg_mu_spher.value = variables[2][0]
                if method is not None:
                    queue[:] = list(variables[1])
                    res = method(*args)
                else:
                    queue[:] = [wb for mlp in variables[:2] for wb in mlp]
                    res = model(*args)
                assert not queue
                return res
            eval_points_raw = model.eval_points_raw

        got = {}
        state = types.SimpleNamespace(optimizer=types.SimpleNamespace(
            target=target, apply_gradient=lambda grad, learning_rate: got.setdefault("grad", grad)),
            replace=lambda optimizer: None)
        rays = self.Rays(*[Tn(batch_np[k]) for k in ("origins", "directions", "viewdirs")])
        keys = [None, [t_rand, None], [u, None], [None, sp_u]]
        _, stats, _ = self.train.train_step(ModelApply(), keys, state, {"rays": rays, "pixels": Tn(batch_np["pixels"])}, 5e-4)
        grad = [[(k.detach().numpy(), b.detach().numpy()) for k, b in mlp] for mlp in got["grad"]]
        return {k: float(getattr(stats, k)) for k in self.Stats._fields}, grad[:2], grad[2][0]


def main():
    sys.path.insert(0, G.REF)
    gw = np.load(os.path.join(HERE, "eval_points_sh25.npz"))
    weights = [[(gw[f"MLP_{mi}.Dense_{li}.kernel"].copy(), gw[f"MLP_{mi}.Dense_{li}.bias"].copy()) for li in range(10)]
               for mi in range(2)]
    for mi in range(2):
        weights[mi][8][1][:] += 0.5
    rng = np.random.default_rng(20211018)
    f32 = np.float32
    B, n_sp = 24, 500
    cam = rng.normal(size=(B, 3)); cam = (4.0 * cam / np.linalg.norm(cam, axis=-1, keepdims=True)).astype(f32)
    d = (-cam / 4.0 + 0.08 * rng.normal(size=(B, 3))).astype(f32)
    v = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(f32)
    batch = dict(origins=cam, directions=d, viewdirs=v, pixels=rng.uniform(size=(B, 3)).astype(f32))
    t_rand, u = rng.uniform(size=(B, 64)).astype(f32), rng.uniform(size=(B, 128)).astype(f32)
    sp_u = rng.uniform(size=(n_sp, 3)).astype(f32)
    sg_lambda = rng.normal(1.0, 0.7, size=K).astype(f32)
    sg_mu_spher = (rng.uniform(size=(K, 2)) * np.array([np.pi, 2 * np.pi])).astype(f32)
    fl = dict(randomized=True, sparsity_weight=1e-3, sparsity_npoints=n_sp, sparsity_radius=1.5, sparsity_length=0.05,
              weight_decay_mult=0.1)
    out = dict(batch, t_rand=t_rand, u=u, sp_u=sp_u, sg_lambda=sg_lambda, sg_mu_spher=sg_mu_spher, sigma_bias_shift=0.5,
               **{k: np.float64(val) for k, val in fl.items()})
    idx, _, owner_of_leaf = T.fixture_index(O.Cfg(sh_deg=4))
    idx = idx.numpy()

    def run(dt):
        stats, grad, (dl, dm) = SgShim(dt).sg_train_step(weights, sg_lambda, sg_mu_spher, batch, t_rand, u, sp_u, fl)
        return stats, G.flat_grad(grad).astype(np.float64), np.concatenate([dl.reshape(-1), dm.reshape(-1)]).astype(np.float64)

    stats64, g64, s64 = run(torch.float64)
    n = g64.size // 2
    for k, val in stats64.items():
        out[f"{k}_f64"] = np.float64(val)
    # weight_l2 counts the 3K SG entries, in the sum and in the element count (train.py:101-108)
    sq = sum(float((a.astype(np.float64) ** 2).sum()) for mlp in weights for pair in mlp for a in pair)
    sq += float((sg_lambda.astype(np.float64) ** 2).sum() + (sg_mu_spher.astype(np.float64) ** 2).sum())
    assert abs(stats64["weight_l2"] - sq / (2 * n + 3 * K)) <= 1e-12 * stats64["weight_l2"], (stats64["weight_l2"], sq / (2 * n + 3 * K))
    assert abs(stats64["weight_l2"] - sq / (2 * n)) > 1e-6 * stats64["weight_l2"]
    per_lobe = np.sqrt(s64[:K] ** 2 + (s64[K:].reshape(K, 2) ** 2).sum(-1))
    assert np.linalg.norm(s64) > 0 and (per_lobe > 1e-4 * per_lobe.max()).sum() >= 20, per_lobe
    floors = np.zeros(3)
    threads0 = torch.get_num_threads()
    for nt in (1, 5, 8):                           # the float32 result depends on the summation order of the host BLAS
        torch.set_num_threads(nt)
        stats32, g32, s32 = run(torch.float32)
        sel = idx < n
        rels = [np.linalg.norm(g32[idx[m]] - g64[idx[m]]) / np.linalg.norm(g64[idx[m]]) for m in (sel, ~sel)]
        rels.append(np.linalg.norm(s32 - s64) / np.linalg.norm(s64))
        print(f"threads {nt}: reference-f32 vs reference-f64 rel L2  MLP_0 {rels[0]:.3e}  MLP_1 {rels[1]:.3e}  SG {rels[2]:.3e}")
        floors = np.maximum(floors, rels)
        if nt == 1:
            for k, val in stats32.items():
                out[f"{k}_f32"] = np.float64(val)
    torch.set_num_threads(threads0)
    out["grad"] = g64[idx].astype(f32)
    out["grad_norm_f64"] = np.float64(np.linalg.norm(g64))
    out["grad_stride"] = np.int64(8)
    out["sg_grad"] = s64
    out["grad_f32_vs_f64_rel_l2_mlp0"], out["grad_f32_vs_f64_rel_l2_mlp1"], out["grad_f32_vs_f64_rel_l2_sg"] = map(np.float64, floors)
    print(f"|g_mlp| {np.linalg.norm(g64):.6e}  |g_sg| {np.linalg.norm(s64):.6e}  lobes above 1e-4 of the largest: "
          f"{int((per_lobe > 1e-4 * per_lobe.max()).sum())} / {K}")
    path = os.path.join(HERE, "sg_train_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
