#!/usr/bin/env python
"""Ray rendering of a trained NeRF-SH through an occupancy grid (pxo_render_fwd_culled) against the dense path (pxo_render_fwd)
of the same build, on bench.py's analytic scene at a trained state.  Needs the MI355X; bench.py is not involved.

    python scripts/occ_render_bench.py [--params DIR/params.npy | --train-steps 1500] [--views 2] [--windows 3] [--chunk 8192]
                                       [--reso 128,256,512] [--alpha 0,0.01] [--out FILE.json]

--params: the parameter arena `bench.py --dump-outputs DIR` writes; without it the script trains the fixed-seed initialisation
itself for --train-steps steps of 4096 rays (the bench's step).

Per grid (reso x alpha_thresh, dilate 1, outside empty, box centre 0 radius 1.5): held-out 800 x 800 views of the test split are
rendered in windows that ALTERNATE dense and culled in one process; a window is all --views views, timed by a host clock around
work that ends in a device synchronise.  Reported per grid: the median and the min..max of the windows of both paths (rays/s),
the live-row fraction per level, PSNR of dense and of culled against ground truth and of culled against dense, the grid's build
time and occupied fraction; and once: the fused-MLP time per image of both paths from HIP events (a pass of its own), cull +
expand on one chunk's fine level beside their HBM floor (bytes moved / 6.3 TB/s achievable), and the round trip of one host read.
The model the result is held against:  t_culled ~ (t_dense - t_mlp_dense) + f_live * t_mlp_dense + t_cull+expand + host reads.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12       # bytes/s, float4 copy on the MI355X


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--params", default=None, help="params.npy of `bench.py --dump-outputs DIR`")
    p.add_argument("--train-steps", type=int, default=1500)
    p.add_argument("--views", type=int, default=2)
    p.add_argument("--windows", type=int, default=3)
    p.add_argument("--chunk", type=int, default=8192)
    p.add_argument("--factor", type=int, default=0, help="image down-scaling of the analytic scene (0: 800 x 800)")
    p.add_argument("--reso", default="128,256,512")
    p.add_argument("--alpha", default="0,0.01")
    p.add_argument("--out", default=None)
    return p.parse_args(argv)


def trained_state(a, device):
    from plenoctree_amd.nerf_sh.nerf import datasets, models, utils
    args = utils.define_flags().parse_args([])
    args.config = "synthetic"
    utils.update_flags(args)
    args.dataset, args.factor, args.batch_size, args.train_dir = "synthetic", a.factor, 4096, "/tmp/pxo_occ_bench"
    model, params = models.construct_nerf(args, device)
    state = models.TrainState(model.cfg, params)
    if a.params:
        flat = torch.from_numpy(np.load(a.params)).to(device)
        if flat.numel() != state.params.numel():
            raise SystemExit(f"{a.params}: {flat.numel()} floats, the preset's two MLPs have {state.params.numel()}")
        state.params.copy_(flat)
        state.repack(need_bwd=False)
        source = a.params
    else:
        ds = datasets.Synthetic("train", args, device, batch_size=4096, seed=20201473)
        for step in range(a.train_steps):
            lr = utils.learning_rate_decay(step, args.lr_init, args.lr_final, args.max_steps)
            models.train_step(model, state, next(ds), lr, randomized=True, seed=step << 8)
        source = f"{a.train_steps} steps x 4096 rays from the fixed-seed initialisation"
    torch.cuda.synchronize()
    return args, model, state, source


def render_views(model, state, views, chunk, grid=None, live=None):
    from plenoctree_amd.nerf_sh.nerf import utils
    out = []
    for ex in views:
        if grid is None:
            fn = lambda r: model.apply(state, r, False)
        else:
            def fn(r):
                rows = []
                res = model.apply(state, r, False, occupancy=grid, live_rows=rows)
                if live is not None:
                    live.add(rows, r.origins.shape[0])
                return res
        out.append(utils.render_image(fn, ex["rays"], chunk=chunk)[0])
    torch.cuda.synchronize()
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def psnr(a, b):
    return float(-10.0 * torch.log10(((a.double() - b.double()) ** 2).mean()))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def mlp_ms(ops, fn):
    """Fused-MLP time of fn() from HIP events (a pass of its own: the brackets are off in the timed windows)."""
    ops.profile_enable(tags=[ops.PROF_MLP_FWD])
    ops.profile_read(ops.PROF_MLP_FWD)
    fn()
    n, ms, rows = ops.profile_read(ops.PROF_MLP_FWD)
    ops.profile_enable(False)
    return {"launches": n, "ms": ms, "rows": rows}


def stage_times(ops, model, state, grid, rays, reps=20):
    """cull and expand of one chunk's fine level, device events, beside their HBM floors; and one host read's round trip."""
    cfg = model.cfg
    o, d = rays.origins, rays.directions
    B, C = o.shape[0], ops.rgb_channels(cfg)
    z, pts = ops.sample_along_rays(o, d, cfg.num_coarse_samples + cfg.num_fine_samples, cfg.near_, cfg.far_)
    M = pts.numel() // 3
    live, slot, n = ops.occ_cull(grid, pts)
    n_live = int(n.item())
    rgb_live = torch.zeros(max(n_live, 1), C, device=o.device)
    sig_live = torch.zeros(max(n_live, 1), device=o.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(3):
        ops.occ_cull(grid, pts)
        ops.occ_expand(rgb_live, sig_live, slot, C)
    torch.cuda.synchronize()
    # the wrappers allocate their outputs from torch's caching allocator: no device malloc inside the brackets after the warm-up
    ev[0].record()
    for _ in range(reps):
        ops.occ_cull(grid, pts)
    ev[1].record()
    for _ in range(reps):
        ops.occ_expand(rgb_live, sig_live, slot, C)
    ev[2].record()
    torch.cuda.synchronize()
    t_cull, t_expand = ev[0].elapsed_time(ev[1]) / reps * 1e-3, ev[1].elapsed_time(ev[2]) / reps * 1e-3
    # bytes: classify reads the points and writes a flag; emit reads flag + points of the live rows' lines (all, at this density),
    # writes slot and the live points; expand reads slot and the live rows, writes every dense element
    cull_bytes = M * (12 + 1) + M * (1 + 12 + 4) + n_live * 12
    expand_bytes = M * 4 + n_live * (C + 1) * 4 + M * (C + 1) * 4
    pinned = torch.empty(1, dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        pinned.copy_(n, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    t_read = (time.perf_counter() - t0) / 200
    return {"rays": B, "rows": M, "live_rows": n_live, "cull_us": 1e6 * t_cull, "cull_hbm_floor_us": 1e6 * cull_bytes / HBM_ACHIEVABLE,
            "expand_us": 1e6 * t_expand, "expand_hbm_floor_us": 1e6 * expand_bytes / HBM_ACHIEVABLE,
            "host_read_round_trip_us": 1e6 * t_read}


def main(argv=None):
    a = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("occ_render_bench.py needs the MI355X; there is no CPU fallback and no CPU timing")
    from plenoctree_amd import ops
    from plenoctree_amd.nerf_sh.nerf import datasets, occupancy, utils
    device = torch.device("cuda:0")
    t0 = time.perf_counter()
    args, model, state, source = trained_state(a, device)
    test = datasets.Synthetic("test", args, device)
    idx = [(i * test.size) // a.views + test.size // (2 * a.views) for i in range(a.views)]
    views = [test.get_image(i) for i in idx]
    h, w = views[0]["pixels"].shape[:2]
    rays_per_window = a.views * h * w
    chunks_per_image = -(-h * w // a.chunk)
    dense_img = render_views(model, state, views, a.chunk)                      # warm-up of the dense shapes, and the reference images
    psnr_dense = [psnr(im, ex["pixels"]) for im, ex in zip(dense_img, views)]
    head = {"record": "setup", "state": source, "views": idx, "image": [h, w], "chunk": a.chunk, "windows": a.windows,
            "psnr_dense_vs_gt": psnr_dense, "setup_s": time.perf_counter() - t0}
    print(json.dumps(head), flush=True)
    records = [head]
    mlp_dense = mlp_ms(ops, lambda: render_views(model, state, views, a.chunk))
    one_chunk = utils.namedtuple_map(lambda r: r.reshape(-1, 3)[:a.chunk].contiguous(), views[0]["rays"])
    for reso in [int(r) for r in a.reso.split(",")]:
        for alpha in [float(x) for x in a.alpha.split(",")]:
            t_build, grid = timed(lambda: occupancy.from_model(model, state, reso, alpha_thresh=alpha, dilate=1, outside="empty"))
            live = occupancy.LiveRows(model.cfg)
            culled_img = render_views(model, state, views, a.chunk, grid, live)     # warm-up of the culled path
            fractions = live.fractions()
            t_dense, t_culled = [], []
            for _ in range(a.windows):                                          # alternating, one process
                t_dense.append(timed(lambda: render_views(model, state, views, a.chunk))[0])
                t_culled.append(timed(lambda: render_views(model, state, views, a.chunk, grid))[0])
            mlp_culled = mlp_ms(ops, lambda: render_views(model, state, views, a.chunk, grid))
            st = stage_times(ops, model, state, grid, one_chunk)
            td, tc = statistics.median(t_dense), statistics.median(t_culled)
            f_live = mlp_culled["rows"] / mlp_dense["rows"]
            reads = 2 * chunks_per_image * a.views * st["host_read_round_trip_us"] * 1e-6
            # cull + expand per window: the measured fine-level chunk scaled by rows (coarse + fine = 256 / 192 of the fine rows)
            ce = (st["cull_us"] + st["expand_us"]) * 1e-6 * chunks_per_image * a.views * (
                (model.cfg.num_coarse_samples * 2 + model.cfg.num_fine_samples) / (model.cfg.num_coarse_samples + model.cfg.num_fine_samples))
            model_t = (td - mlp_dense["ms"] * 1e-3) + f_live * mlp_dense["ms"] * 1e-3 + ce + reads
            rec = {"record": "grid", "reso": reso, "alpha_thresh": alpha, "build_s": t_build,
                   "fraction_occupied": grid.fraction_occupied(), "live_fraction": {"coarse": fractions[0], "fine": fractions[1]},
                   "dense_rays_per_s": spread([rays_per_window / t for t in t_dense]),
                   "culled_rays_per_s": spread([rays_per_window / t for t in t_culled]),
                   "dense_s_per_window": spread(t_dense), "culled_s_per_window": spread(t_culled), "speedup_median": td / tc,
                   "mlp_ms_per_window": {"dense": mlp_dense["ms"], "culled": mlp_culled["ms"], "row_fraction": f_live},
                   "stages_one_fine_chunk": st, "host_reads_s_per_window": reads, "cull_expand_s_per_window": ce,
                   "model_s_per_window": model_t, "measured_over_model": tc / model_t,
                   "psnr_dense_vs_gt": psnr_dense, "psnr_culled_vs_gt": [psnr(im, ex["pixels"]) for im, ex in zip(culled_img, views)],
                   "psnr_culled_vs_dense": [None if torch.equal(c, dn) else psnr(c, dn) for c, dn in zip(culled_img, dense_img)]}
            print(json.dumps(rec), flush=True)
            records.append(rec)
            del grid
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
