"""What tests/test_gpu_api_sequences.py holds the render and train sequences of pxo_api.hip to: for a grid of small configurations,
the five workspace sizes, the launches and rows each sequence puts under every profiler tag, and the bits a culled render followed
by a culled step leave when both use one workspace.  measure() is run once on the commit BEFORE a change of the sequences to write
tests/golden/api_sequences.json (python tests/_api_sequences.py, on the MI355X), and by the test on the tree under test."""
import json
import os
import sys

import numpy as np
import torch

NC, NF = 8, 16                                    # the sizes of tests/test_gpu_occ_train.py
RESO = 4
TAGS = ("MLP_FWD", "MLP_BWD_DATA", "WGRAD_MAIN", "WGRAD_OTHER")
PRECISIONS = (0, 2)                               # float32, bf16x6: the two a train step runs in
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_sequences.json")


def configs():
    return [(deg, nf, n_sp, B) for deg in (0, 2) for nf in (0, NF) for n_sp in (0, 16) for B in (1, 257)]


def key(deg, nf, n_sp, B):
    return f"deg{deg}_nf{nf}_sp{n_sp}_B{B}"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _checksum(t):
    return int(_bits(t).to(torch.int64).sum())


def _profiled(ops, call):
    """{tag: [launches, rows]} of one call."""
    tags = [getattr(ops, "PROF_" + t) for t in TAGS]
    torch.cuda.synchronize()
    ops.profile_enable(tags=tags)
    try:
        for t in tags:
            ops.profile_read(t)
        call()
        torch.cuda.synchronize()
        return {name: list(ops.profile_read(t)[::2]) for name, t in zip(TAGS, tags)}
    finally:
        ops.profile_enable(False)


_PARAMS = {}                                      # per sh_deg (the parameters do not depend on the other sizes)


def measure_one(ops, dev, deg, nf, n_sp, B):
    import _occupancy_ref as R
    from _helpers import make_params, make_rays, pxo_cfg, split_mlp
    from oracle import nerf_oracle as O
    ocfg = O.Cfg(num_coarse_samples=NC, num_fine_samples=nf, sh_deg=deg, sparsity_npoints=n_sp)
    if deg not in _PARAMS:
        _PARAMS[deg] = make_params(ocfg, seed=3)
    fd = _PARAMS[deg].to(dev)
    o, d, v = (x.to(dev).contiguous() for x in make_rays(B, seed=5))
    gen = torch.Generator().manual_seed(9)
    px = torch.rand(B, 3, generator=gen).to(dev)
    t_rand = torch.rand(B, NC, generator=gen).to(dev)
    u = torch.rand(B, max(nf, 1), generator=gen).to(dev) if nf else None
    sp = ((torch.rand(16, 3, generator=gen) * 2 - 1) * ocfg.sparsity_radius)[:n_sp].contiguous().to(dev) if n_sp else None
    K = (deg + 1) ** 2
    sgp = (0.5 + torch.rand(3 * K, generator=gen)).to(dev)
    lobes = ops.sg_lobes(sgp, K)
    half = np.zeros((RESO, RESO, RESO), bool)
    half[:2] = True                                               # the half space x < 0 of the box [-2, 2)^3
    grids = {"all_ones": ops.OccupancyGrid(torch.from_numpy(R.bits_from_mask(np.ones((RESO,) * 3, bool))).to(dev), RESO, [0.5] * 3,
                                           [1.0 / 16] * 3, outside_live=True),
             "half_space": ops.OccupancyGrid(torch.from_numpy(R.bits_from_mask(half)).to(dev), RESO, [0.5] * 3, [0.25] * 3,
                                             outside_live=False)}
    out = {}
    for precision in PRECISIONS:
        pcfg = pxo_cfg(ops, ocfg)
        pcfg.mlp_precision = precision
        pk = [ops.pack_weights(pcfg, split_mlp(fd, ocfg, i)) for i in range(2)]
        fwd = [p[0] for p in pk]
        sizes = {"render": ops.render_workspace_bytes(pcfg, B), "render_culled": ops.render_culled_workspace_bytes(pcfg, B),
                 "train": ops.train_workspace_bytes(pcfg, B), "sg_train": ops.sg_train_workspace_bytes(pcfg, B),
                 "train_culled": ops.train_culled_workspace_bytes(pcfg, B)}
        draws = dict(randomized=True, t_rand=t_rand, u=u, sp_points=sp)

        def train(fn, nbytes, *head, ws=None, extra=(), **kw):
            grads = torch.full_like(fd, float("nan"))
            stats = torch.full((6,), float("nan"), device=dev)
            if ws is None:
                ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
            fn(pcfg, *head, pk, o, d, v, px, grads, *extra, stats, ws, **draws, **kw)
            return grads, stats

        rec = {"workspace_bytes": sizes, "launches": {}}
        L = rec["launches"]
        L["render_fwd"] = _profiled(ops, lambda: ops.render_fwd(pcfg, fwd[0], fwd[1], o, d, v))
        L["train_fwd_bwd"] = _profiled(ops, lambda: train(ops.train_fwd_bwd, sizes["train"], fd))
        sg_grads = torch.zeros_like(sgp)
        L["sg_train_fwd_bwd"] = _profiled(ops, lambda: train(ops.sg_train_fwd_bwd, sizes["sg_train"], fd, sgp, extra=(sg_grads,)))
        for name, grid in grids.items():
            rows = []
            L["render_fwd_culled/" + name] = _profiled(
                ops, lambda: ops.render_fwd_culled(pcfg, grid, fwd[0], fwd[1], o, d, v, live_rows=rows))
            L["render_fwd_culled/" + name]["live_rows"] = list(rows)
            rows = []
            L["train_fwd_bwd_culled/" + name] = _profiled(
                ops, lambda: train(ops.train_fwd_bwd_culled, sizes["train_culled"], grid, fd, live_rows=rows))
            L["train_fwd_bwd_culled/" + name]["live_rows"] = list(rows)
        # a culled render, then a culled step, in ONE workspace: arrays of the cull block that lay on one another would show here
        ws = torch.full((max(sizes["train_culled"], sizes["render_culled"]),), 0xFF, dtype=torch.uint8, device=dev)
        outs = ops.render_fwd_culled(pcfg, grids["half_space"], fwd[0], fwd[1], o, d, v, ws=ws, lobes=lobes)
        grads, stats = train(ops.train_fwd_bwd_culled, 0, grids["half_space"], fd, ws=ws)
        torch.cuda.synchronize()
        rec["shared_workspace"] = {"render_checksum": sum(_checksum(x) for lvl in outs for x in lvl),
                                   "stats_bits": _bits(stats).cpu().tolist(), "grads_checksum": _checksum(grads)}
        out[f"precision{precision}"] = rec
    return out


def measure(ops, dev):
    return {"cus": torch.cuda.get_device_properties(dev).multi_processor_count,
            "configs": {key(*c): measure_one(ops, dev, *c) for c in configs()}}


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from plenoctree_amd import ops as _ops
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(measure(_ops, torch.device("cuda:0")), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
