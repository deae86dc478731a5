"""Ray-rendering throughput of the view-conditioned model beside the SH16 model (nothing here is a pass/fail number).

Renders one 800x800 view, deterministic sampling, in chunks of --chunk rays: the view-conditioned model (seeded weights) through
pxo_vd_render_fwd and, in the same process, the SH16 model through pxo_render_fwd.  Best of --repeats after one warm-up each.
The trunk work per sample is the same, so the ratio is what the head, the trunk's saved-tensor writes and the blocking cost.

    python scripts/vd_render_bench.py [--chunk 8192] [--ray_block N] [--size 800] [--repeats 3] [--only vd|sh]

--ray_block sets PXO_TUNE_VD_RAY_BLOCK (A/B of the internal block).  For the per-kernel split run it under
`rocprofv3 --kernel-trace --stats -- python scripts/vd_render_bench.py --repeats 1`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plenoctree_amd import ops  # noqa: E402
from plenoctree_amd.nerf_sh.nerf import models, utils, viewdirs  # noqa: E402


def timed_view(render, rays, chunk, repeats):
    best = float("inf")
    for i in range(repeats + 1):                      # the first pass warms up (workspace allocation, code load)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        utils.render_image(render, rays, chunk=chunk)
        torch.cuda.synchronize()
        if i:
            best = min(best, time.perf_counter() - t0)
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=8192)
    ap.add_argument("--ray_block", type=int, default=None)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["vd", "sh"], default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if a.ray_block is not None:
        ops.set_tuning(ops.TUNE_VD_RAY_BLOCK, a.ray_block)
    H = W = a.size
    focal = 0.5 * W / np.tan(0.5 * 0.6911112070083618)
    c2w = torch.from_numpy(utils.pose_spherical(30.0, -30.0, 4.0)[:3, :4].copy()).to(dev)
    rays = utils.Rays(*[r.reshape(H, W, 3) for r in ops.generate_rays(c2w, W, H, focal)])
    n = H * W
    rec = {"rays": n, "chunk": a.chunk, "ray_block": ops.get_tuning(ops.TUNE_VD_RAY_BLOCK)}
    if a.only != "sh":
        model = viewdirs.ViewdirsModel()
        state = viewdirs.ViewdirsState(viewdirs.init_params(1).to(dev))
        rec["vd_workspace_gb"] = ops.vd_render_workspace_bytes(model.cfg, min(a.chunk, n)) / 2 ** 30
        t = timed_view(lambda r: model.apply(state, r, False), rays, a.chunk, a.repeats)
        rec.update(vd_seconds=t, vd_rays_per_s=n / t)
        del state
    if a.only != "vd":
        cfg = ops.make_cfg(sh_deg=3)
        sh_model = models.NerfModel(cfg)
        sh_state = models.TrainState(cfg, models.init_params(cfg, 1).to(dev))
        t = timed_view(lambda r: sh_model.apply(sh_state, r, False), rays, a.chunk, a.repeats)
        rec.update(sh16_seconds=t, sh16_rays_per_s=n / t)
    if "vd_rays_per_s" in rec and "sh16_rays_per_s" in rec:
        rec["vd_over_sh16"] = rec["vd_rays_per_s"] / rec["sh16_rays_per_s"]
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
