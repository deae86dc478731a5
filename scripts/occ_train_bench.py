#!/usr/bin/env python
"""The train step through an occupancy grid (pxo_train_fwd_bwd_culled) against the dense step (pxo_train_fwd_bwd_bucketed,
skip_zero_rows on: the CLI default) of the same build, on bench.py's analytic scene.  Needs the MI355X; bench.py is not involved.

    python scripts/occ_train_bench.py [--steps 2000] [--snapshot 1500] [--reso 128,256] [--precisions f32,bf16x6]
                                      [--window-steps 20] [--windows 5] [--views 2] [--skip-psnr | --skip-steps] [--out FILE.json]

Two runs of --steps steps x 4096 rays x 64 + 128 samples from ONE seed: dense, and with an occupancy.TrainingGrid of the flags'
defaults (--cull-reso, --cull-warmup-steps, --cull-update-every, --cull-alpha-thresh, --cull-dilate).  Both are rendered DENSE on
held-out 800 x 800 views: PSNR against ground truth (the pair the project's 0.1 dB bar is held to), and the culled run's live
fractions and rebuild times.

The step time is measured on the dense run's parameters after --snapshot steps.  Per precision and grid resolution, windows of
--window-steps whole train steps (models.train_step with lr = 0: fwd_bwd, Adam, re-pack; the parameters do not move) ALTERNATE
dense and culled in one process, each timed by a host clock around work that ends in a device synchronise.  Reported: rays/s of
both (median, min..max of the windows), the live fractions, the grid's build time and what it costs per step at
--cull-update-every, the fused kernels' HIP-event times of both steps (a pass of its own), cull + expand + gather on one fine
level beside their HBM floor, one host read's round trip, and the model the result is held against:

    t_culled ~ (t_dense - t_fwd - t_bwd - t_wgrad) + f_live (t_fwd + t_bwd + t_wgrad) + t_cull+expand+gather + 2 host reads

with f_live the rows through the culled step's MLPs over the dense step's.  What the model leaves unexplained is, beside the
dense reverse pass already skipping zero rows, the cost of the two stream synchronisations: the device idles while the host,
woken by the count, enqueues the rest of the level."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HBM_ACHIEVABLE = 6.3e12       # bytes/s, float4 copy on the MI355X
B = 4096                      # rays per step: the bench's step


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--snapshot", type=int, default=1500, help="the dense run's step whose parameters the step time is measured at")
    p.add_argument("--reso", default="128,256")
    p.add_argument("--precisions", default="f32,bf16x6")
    p.add_argument("--window-steps", type=int, default=20)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--views", type=int, default=2)
    p.add_argument("--chunk", type=int, default=8192)
    p.add_argument("--factor", type=int, default=0, help="image down-scaling of the analytic scene (0: 800 x 800)")
    p.add_argument("--cull-reso", type=int, default=128)
    p.add_argument("--cull-warmup-steps", type=int, default=500)
    p.add_argument("--cull-update-every", type=int, default=32)
    p.add_argument("--cull-alpha-thresh", type=float, default=0.01)
    p.add_argument("--cull-dilate", type=int, default=1)
    p.add_argument("--skip-psnr", action="store_true", help="only the dense run to --snapshot and the step times")
    p.add_argument("--skip-steps", action="store_true", help="only the two runs and their PSNR")
    p.add_argument("--out", default=None)
    return p.parse_args(argv)


def fresh(a, device):
    from plenoctree_amd.nerf_sh.nerf import datasets, models, utils
    args = utils.define_flags().parse_args([])
    args.config = "synthetic"
    utils.update_flags(args)
    args.dataset, args.factor, args.batch_size, args.train_dir = "synthetic", a.factor, B, "/tmp/pxo_occ_train_bench"
    model, params = models.construct_nerf(args, device)
    state = models.TrainState(model.cfg, params)
    ds = datasets.Synthetic("train", args, device, batch_size=B, seed=20201473)
    return args, model, state, ds


def train(a, device, cull, snapshot_at=None):
    """--steps steps from the fixed-seed initialisation; cull: a TrainingGrid or None.  Returns (args, model, state, the parameters
    after snapshot_at steps or None, seconds, [(step, live fractions, occupied fraction, rebuild seconds)] per rebuild)."""
    from plenoctree_amd.nerf_sh.nerf import models, occupancy, utils
    args, model, state, ds = fresh(a, device)
    snap, trace = None, []
    live = occupancy.LiveRows(model.cfg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(1, a.steps + 1):
        lr = utils.learning_rate_decay(step, args.lr_init, args.lr_final, args.max_steps)
        grid, rows = (cull.before_step(step, model, state), []) if cull is not None else (None, None)
        if cull is not None and cull.built_at == step:
            if live.total[0]:
                trace[-1]["live_fraction"] = live.fractions()
                live.reset()
            trace.append({"step": step, "fraction_occupied": cull.fraction, "rebuild_s": cull.rebuild_seconds})
        if grid is None:
            models.train_step(model, state, next(ds), lr, randomized=True, seed=step << 8)
        else:
            models.train_step(model, state, next(ds), lr, randomized=True, seed=step << 8, occupancy=grid, live_rows=rows)
            live.add(rows, B)
        if step == snapshot_at:
            snap = state.params.clone()
    torch.cuda.synchronize()
    if trace and live.total[0]:
        trace[-1]["live_fraction"] = live.fractions()
    return args, model, state, snap, time.perf_counter() - t0, trace


def with_precision(model, params, precision):
    """(model, state) on a copy of `params` with cfg.mlp_precision = precision (0 f32, 2 bf16x6)."""
    from plenoctree_amd.nerf_sh.nerf import models
    cfg = type(model.cfg).from_buffer_copy(model.cfg)
    cfg.mlp_precision = precision
    return models.NerfModel(cfg), models.TrainState(cfg, params.clone())


def kernel_ms(ops, fn, steps):
    """HIP-event time per step of the four fused-kernel tags over fn() (a pass of its own: the brackets are off in the timed windows)."""
    names = {"fwd": ops.PROF_MLP_FWD, "bwd": ops.PROF_MLP_BWD_DATA, "wgrad_main": ops.PROF_WGRAD_MAIN, "wgrad_other": ops.PROF_WGRAD_OTHER}
    ops.profile_enable(tags=list(names.values()))
    for t in names.values():
        ops.profile_read(t)
    fn()
    torch.cuda.synchronize()
    out = {}
    for k, t in names.items():
        n, ms, rows = ops.profile_read(t)
        out[k] = {"launches_per_step": n / steps, "ms_per_step": ms / steps, "rows_per_step": rows / steps}
    ops.profile_enable(False)
    return out


def stage_times(ops, cfg, grid, rays, reps=20):
    """cull, expand and gather of one fine level (4096 rays x 192 samples, uniform along the rays), device events, beside their HBM
    floors; and one host read's round trip."""
    o, d = rays.origins, rays.directions
    C = ops.rgb_channels(cfg)
    _, pts = ops.sample_along_rays(o, d, cfg.num_coarse_samples + cfg.num_fine_samples, cfg.near_, cfg.far_)
    M = pts.numel() // 3
    _, slot, n = ops.occ_cull(grid, pts)
    n_live = int(n.item())
    rgb_live, sig_live = torch.zeros(M, C, device=o.device), torch.zeros(M, device=o.device)
    d_rgb, d_sig = torch.zeros(M, C, device=o.device), torch.zeros(M, device=o.device)
    for _ in range(3):
        ops.occ_cull(grid, pts)
        ops.occ_expand(rgb_live, sig_live, slot, C)
        ops.occ_gather(d_rgb, d_sig, slot, rgb_live, sig_live)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(reps):
        ops.occ_cull(grid, pts)
    ev[1].record()
    for _ in range(reps):
        ops.occ_expand(rgb_live, sig_live, slot, C)
    ev[2].record()
    for _ in range(reps):
        ops.occ_gather(d_rgb, d_sig, slot, rgb_live, sig_live)
    ev[3].record()
    torch.cuda.synchronize()
    t = [ev[i].elapsed_time(ev[i + 1]) / reps * 1e-3 for i in range(3)]
    cull_bytes = M * (12 + 1) + M * (1 + 12 + 4) + n_live * 12
    expand_bytes = M * 4 + n_live * (C + 1) * 4 + M * (C + 1) * 4
    gather_bytes = M * 4 + 2 * n_live * (C + 1) * 4            # slot, the live rows read and written (dead rows' lines are not read)
    pinned = torch.empty(1, dtype=torch.int64).pin_memory()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        pinned.copy_(n, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    t_read = (time.perf_counter() - t0) / 200
    return {"rows": M, "live_rows": n_live, "cull_us": 1e6 * t[0], "cull_hbm_floor_us": 1e6 * cull_bytes / HBM_ACHIEVABLE,
            "expand_us": 1e6 * t[1], "expand_hbm_floor_us": 1e6 * expand_bytes / HBM_ACHIEVABLE, "gather_us": 1e6 * t[2],
            "gather_hbm_floor_us": 1e6 * gather_bytes / HBM_ACHIEVABLE, "host_read_round_trip_us": 1e6 * t_read}


def step_times(a, ops, model, params, batches, emit):
    from plenoctree_amd.nerf_sh.nerf import models, occupancy
    from occ_render_bench import spread, timed
    n = a.window_steps
    for name in a.precisions.split(","):
        m, st = with_precision(model, params, {"f32": 0, "bf16x6": 2}[name])
        cfg = m.cfg

        def steps(grid, live=None):
            for i in range(n):
                if grid is None:
                    models.train_step(m, st, batches[i % len(batches)], 0.0, randomized=True, seed=i << 8)
                else:
                    rows = []
                    models.train_step(m, st, batches[i % len(batches)], 0.0, randomized=True, seed=i << 8, occupancy=grid, live_rows=rows)
                    if live is not None:
                        live.add(rows, B)
        steps(None)                                               # warm-up of the dense shapes
        k_dense = kernel_ms(ops, lambda: steps(None), n)
        for reso in [int(r) for r in a.reso.split(",")]:
            t_build, grid = timed(lambda: occupancy.from_model(m, st, reso, alpha_thresh=a.cull_alpha_thresh, dilate=a.cull_dilate,
                                                               outside="empty"))
            t_build = min(t_build, timed(lambda: occupancy.from_model(m, st, reso, alpha_thresh=a.cull_alpha_thresh,
                                                                      dilate=a.cull_dilate, outside="empty"))[0])      # the second: warm
            live = occupancy.LiveRows(cfg)
            steps(grid, live)                                     # warm-up of the culled path
            t_d, t_c = [], []
            for _ in range(a.windows):                            # alternating, one process
                t_d.append(timed(lambda: steps(None))[0] / n)
                t_c.append(timed(lambda: steps(grid))[0] / n)
            k_culled = kernel_ms(ops, lambda: steps(grid), n)
            stg = stage_times(ops, cfg, grid, batches[0]["rays"])
            td, tc = statistics.median(t_d), statistics.median(t_c)
            mlp_d = sum(k_dense[k]["ms_per_step"] for k in k_dense) * 1e-3
            mlp_c = sum(k_culled[k]["ms_per_step"] for k in k_culled) * 1e-3
            f_live = k_culled["fwd"]["rows_per_step"] / k_dense["fwd"]["rows_per_step"]
            levels = (cfg.num_coarse_samples * 2 + cfg.num_fine_samples) / (cfg.num_coarse_samples + cfg.num_fine_samples)
            ceg = (stg["cull_us"] + stg["expand_us"] + stg["gather_us"]) * 1e-6 * levels
            reads = 2 * stg["host_read_round_trip_us"] * 1e-6
            model_t = (td - mlp_d) + f_live * mlp_d + ceg + reads
            emit({"record": "step", "precision": name, "reso": reso, "alpha_thresh": a.cull_alpha_thresh, "dilate": a.cull_dilate,
                  "fraction_occupied": grid.fraction_occupied(), "live_fraction": dict(zip(("coarse", "fine"), live.fractions())),
                  "dense_rays_per_s": spread([B / t for t in t_d]), "culled_rays_per_s": spread([B / t for t in t_c]),
                  "dense_ms_per_step": spread([1e3 * t for t in t_d]), "culled_ms_per_step": spread([1e3 * t for t in t_c]),
                  "speedup_median": td / tc, "grid_build_s": t_build, "grid_build_ms_per_step_amortised": 1e3 * t_build / a.cull_update_every,
                  "culled_rays_per_s_with_rebuilds": B / (tc + t_build / a.cull_update_every),
                  "kernels_dense": k_dense, "kernels_culled": k_culled, "mlp_row_fraction": f_live,
                  "stages_one_fine_level": stg, "cull_expand_gather_ms_per_step": 1e3 * ceg, "host_reads_ms_per_step": 1e3 * reads,
                  "model_ms_per_step": 1e3 * model_t, "measured_over_model": tc / model_t,
                  "unexplained_ms_per_step": 1e3 * (tc - ((td - mlp_d) + mlp_c + ceg + reads))})
            del grid


def main(argv=None):
    a = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("occ_train_bench.py needs the MI355X; there is no CPU fallback and no CPU timing")
    from plenoctree_amd import ops
    from plenoctree_amd.nerf_sh.nerf import datasets, occupancy
    from occ_render_bench import psnr, render_views
    device = torch.device("cuda:0")
    records = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        records.append(rec)
    if a.skip_psnr:
        a.steps = a.snapshot
    args, model, state, snap, t_dense, _ = train(a, device, None, snapshot_at=a.snapshot)
    emit({"record": "run", "mode": "dense", "steps": a.steps, "seconds": t_dense, "rays_per_s": a.steps * B / t_dense})
    if not a.skip_psnr:
        test = datasets.Synthetic("test", args, device)
        idx = [(i * test.size) // a.views + test.size // (2 * a.views) for i in range(a.views)]
        views = [test.get_image(i) for i in idx]
        psnr_dense = [psnr(im, ex["pixels"]) for im, ex in zip(render_views(model, state, views, a.chunk), views)]
        cull = occupancy.TrainingGrid(a.cull_reso, alpha_thresh=a.cull_alpha_thresh, dilate=a.cull_dilate,
                                      warmup_steps=a.cull_warmup_steps, update_every=a.cull_update_every)
        _, model_c, state_c, _, t_culled, trace = train(a, device, cull)
        emit({"record": "run", "mode": "culled", "steps": a.steps, "seconds": t_culled, "rays_per_s": a.steps * B / t_culled,
              "cull_reso": a.cull_reso, "warmup_steps": a.cull_warmup_steps, "update_every": a.cull_update_every,
              "alpha_thresh": a.cull_alpha_thresh, "dilate": a.cull_dilate, "rebuilds": len(trace),
              "rebuild_s_median": statistics.median(t["rebuild_s"] for t in trace) if trace else None,
              "first_rebuild": trace[0] if trace else None, "last_rebuild": trace[-1] if trace else None})
        psnr_culled = [psnr(im, ex["pixels"]) for im, ex in zip(render_views(model_c, state_c, views, a.chunk), views)]
        psnr_culled_grid = None
        if cull.grid is not None:                                 # the culled run's model through its own last grid
            psnr_culled_grid = [psnr(im, ex["pixels"]) for im, ex in zip(render_views(model_c, state_c, views, a.chunk, cull.grid), views)]
        mean = lambda xs: sum(xs) / len(xs)
        emit({"record": "psnr", "views": idx, "image": list(views[0]["pixels"].shape[:2]), "steps": a.steps,
              "dense_vs_gt": psnr_dense, "culled_vs_gt": psnr_culled, "culled_through_its_grid_vs_gt": psnr_culled_grid,
              "mean_dense": mean(psnr_dense), "mean_culled": mean(psnr_culled), "culled_minus_dense_db": mean(psnr_culled) - mean(psnr_dense)})
        del state_c
    if not a.skip_steps:
        _, _, _, ds = fresh(a, device)
        batches = [next(ds) for _ in range(8)]
        step_times(a, ops, model, snap if snap is not None else state.params, batches, emit)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
