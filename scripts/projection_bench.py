"""Times the fused SH projection of a view-dependent NeRF (pxo_vd_project_sh) against the reference's algorithm stated with
torch ops: cross-broadcast concat [bottleneck | posenc(dir)] -> Linear -> ReLU -> Linear -> einsum with the SH basis, chunked to
fit memory (octree/nerf/model_utils.py:139-157, octree/nerf/sh_proj.py:293-305).  The baseline is not the code under test; both
start from the same points and directions and both include the trunk.

    python scripts/projection_bench.py [--points 1048576] [--dirs 10000] [--sh_deg 3] [--baseline_points 16384]

Prints one JSON line: point-direction pairs/s of both, their ratio, the fused pair kernel's fraction of the vector-ALU bound of
its cost model (640 + 3K lane operations per pair at CUs x 64 lanes x clock), the workspace bytes (which do
not grow with points x directions) and the largest difference between the two results on the baseline's points.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from plenoctree_amd import ops  # noqa: E402
from plenoctree_amd.nerf_sh.nerf import checkpoints, viewdirs  # noqa: E402


def _timed(fn, warmup=1, iters=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def torch_baseline(sd, pts, dirs, sh_deg, Y, pair_budget=1 << 22):
    """The materialising algorithm: per chunk of points an [n, R, 283] input and an [n, R, 3] colour tensor in HBM."""
    g = lambda n: (sd[f"MLP_1.{n}.weight"], sd[f"MLP_1.{n}.bias"])
    R = dirs.shape[0]
    scales = 2.0 ** torch.arange(4, device=dirs.device)
    xb = (dirs[:, None, :] * scales[:, None]).reshape(R, -1)
    denc = torch.cat([dirs, torch.sin(torch.cat([xb, xb + 0.5 * math.pi], -1))], -1)
    pscales = 2.0 ** torch.arange(10, device=pts.device)
    out = []
    step = max(pair_budget // R, 1)
    for i in range(0, pts.shape[0], step):
        p = pts[i:i + step]
        pb = (p[:, None, :] * pscales[:, None]).reshape(p.shape[0], -1)
        inputs = torch.cat([p, torch.sin(torch.cat([pb, pb + 0.5 * math.pi], -1))], -1)
        x = inputs
        for l in range(8):
            w, b = g(f"input_layers.{l}")
            x = torch.relu(torch.nn.functional.linear(x, w, b))
            if l == 4:
                x = torch.cat([x, inputs], -1)
        bott = torch.nn.functional.linear(x, *g("bottleneck_layer"))
        z = torch.cat([bott[:, None, :].expand(-1, R, -1), denc[None].expand(p.shape[0], -1, -1)], -1).reshape(-1, 283)
        h = torch.relu(torch.nn.functional.linear(z, *g("condition_layers.0")))
        rgb = torch.nn.functional.linear(h, *g("rgb_layer")).view(p.shape[0], R, 3)
        out.append(torch.einsum("prc,rk->pck", rgb, Y).reshape(p.shape[0], -1) * (4.0 * math.pi / R))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--dirs", type=int, default=10000)
    ap.add_argument("--sh_deg", type=int, default=3)
    ap.add_argument("--baseline_points", type=int, default=1 << 14)
    ap.add_argument("--chunk_points", type=int, default=1 << 16)
    ap.add_argument("--clock_ghz", type=float, default=2.4)       # peak engine clock the vector bound is stated at (MI355X)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    flat = viewdirs.init_params(seed=1)
    state = viewdirs.ViewdirsState(flat.to(dev))
    model = viewdirs.ViewdirsModel()
    sd = {k: v.to(dev) for k, v in checkpoints.vd_state_dict_from_arena(flat.numpy()).items()}
    g = torch.Generator().manual_seed(2)
    pts = ((torch.rand(args.points, 3, generator=g) * 2 - 1) * 1.5).to(dev)
    dirs = viewdirs.sphere_directions(torch.rand(args.dirs, generator=g), torch.rand(args.dirs, generator=g)).to(dev)
    K = (args.sh_deg + 1) ** 2
    coeffs = torch.empty(args.points, 3 * K, device=dev)
    sigma = torch.empty(args.points, device=dev)

    def fused():
        for i in range(0, args.points, args.chunk_points):
            j = min(i + args.chunk_points, args.points)
            model.project_sh(state, pts[i:j], dirs, args.sh_deg, coeffs=coeffs[i:j], raw_sigma=sigma[i:j])

    t_fused = _timed(fused)
    from oracle import nerf_oracle as O
    Y = O.sh_basis(args.sh_deg, dirs)
    nb = min(args.baseline_points, args.points)
    t_base = _timed(lambda: torch_baseline(sd, pts[:nb], dirs, args.sh_deg, Y), warmup=1, iters=2)
    diff = float((torch_baseline(sd, pts[:nb], dirs, args.sh_deg, Y) - coeffs[:nb]).abs().max())
    prop = torch.cuda.get_device_properties(dev)
    lanes_per_s = prop.multi_processor_count * 64 * args.clock_ghz * 1e9
    pairs_fused = args.points * args.dirs / t_fused
    print(json.dumps({
        "points": args.points, "dirs": args.dirs, "sh_deg": args.sh_deg,
        "fused_s": t_fused, "fused_pairs_per_s": pairs_fused,
        "baseline_points": nb, "baseline_s": t_base, "baseline_pairs_per_s": nb * args.dirs / t_base,
        "ratio": pairs_fused / (nb * args.dirs / t_base),
        "valu_bound_pairs_per_s": lanes_per_s / (640 + 3 * K), "fraction_of_valu_bound": pairs_fused / (lanes_per_s / (640 + 3 * K)),
        "workspace_bytes_per_chunk": ops.vd_project_workspace_bytes(min(args.chunk_points, args.points), args.dirs),
        "max_abs_diff_vs_baseline": diff}))


if __name__ == "__main__":
    main()
