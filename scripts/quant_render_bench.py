#!/usr/bin/env python
"""Float renderer against the palette renderer on the same compressed tree (profiles/EXPERIMENTS.md).

Scene: scripts/octree_bench.py's analytic one (three fuzzy spheres on a 2^(depth+1) grid, weight-masked by --cams training
views, random SH16 leaves), saved as octree.extraction saves it and compressed by the octree.compression CLI with its
defaults (16 bits, sigma_thresh 2, retain 0).  Measured, one JSON line:

  load_s            np.load -> first rendered image on the device, `N3Tree.load(path)` and `keep_quantized=True`
  device_bytes      both forms
  render ms         one --size x --size view, exact and early-stop, float kernel on the dequantised tree and palette kernel
                    on the packed one: HIP events around --renders back-to-back renders after a warm-up, the two kernels
                    alternating, --windows windows each, best and median
  bytes per sample  algorithmic (nothing cached), from pxo_octree_count_work on the float tree (same sample sequence):
                    float 4 (3K+1) per shaded sample; palette 2 idx_stride + 4 + 8 Kq palette lookups + 8 r
  image difference  max |palette - float| over the timed views

Nothing here is asserted; bench.py is not involved.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_scene(a, dev, path):
    from plenoctree_amd import octree_ops as oops
    from plenoctree_amd.nerf_sh.nerf.datasets import pose_spherical
    from plenoctree_amd.octree.svox import N3Tree
    depth, reso, K = a.depth, 2 ** (a.depth + 1), a.basis
    tree = N3Tree(N=2, data_dim=3 * K + 1, depth_limit=depth, radius=1.5, center=[0, 0, 0], data_format=f"SH{K}", map_location=dev)
    ax = ((torch.arange(reso, device=dev, dtype=torch.float32) + 0.5) / reso - 0.5) * 3.0
    sig = torch.zeros(reso, reso, reso, device=dev)
    for c, r in (((0.0, 0.0, 0.0), 0.6), ((0.7, 0.3, 0.2), 0.3), ((-0.5, -0.4, 0.5), 0.35)):
        d2 = (ax[:, None, None] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2
        sig += 40.0 * torch.sigmoid((r - d2.sqrt()) * 60.0)
    sig = sig.reshape(-1).contiguous()
    W = H = a.size
    focal = 0.5 * W / np.tan(0.5 * 0.6911112)
    rs = np.random.RandomState(7)
    cams = torch.from_numpy(np.stack([pose_spherical(rs.uniform(0, 360), rs.uniform(-10, 60), 4.0311) for _ in range(a.cams)])).to(dev)
    wt = oops.grid_weight_render(sig, reso, cams, focal, focal, W, H, oops.render_opts(a.step), tree.offset, tree.invradius)
    tree.refine_from_mask(oops.threshold_mask(wt, 1e-3))
    node0, count = tree.max_depth_nodes()
    pts = tree.sample_max_depth_cells(1, u=torch.full((count * 8, 3), 0.5, device=dev)).view(-1, 3)
    idx = ((pts / 3.0 + 0.5) * reso).long().clamp_(0, reso - 1)
    leaf = tree.max_depth_data()
    leaf.copy_(torch.randn(leaf.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 0.5)
    leaf[:, -1] = sig[(idx[:, 0] * reso + idx[:, 1]) * reso + idx[:, 2]]
    tree.save(path, compress=False)
    return cams, focal, tree.n_internal


def window(fn, renders):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(renders):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / renders


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--step", type=float, default=1e-4)
    p.add_argument("--cams", type=int, default=8)
    p.add_argument("--basis", type=int, default=16)
    p.add_argument("--renders", type=int, default=100, help="back-to-back renders per timed window")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--lanes", type=int, nargs="*", default=[0], help="lanes per ray of the palette kernel to time (0 = default)")
    p.add_argument("--workdir", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quant_render_bench needs a ROCm GPU: nothing here can be measured on a CPU")
    from plenoctree_amd import build, octree_ops as oops
    from plenoctree_amd.octree import compression
    from plenoctree_amd.octree.svox import N3Tree, VolumeRenderer
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    work = a.workdir or tempfile.mkdtemp(prefix="quant_bench_")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "tree.npz")
    t0 = time.perf_counter()
    cams, focal, n_internal = build_scene(a, dev, src)
    out = {"basis_dim": a.basis, "depth": a.depth, "image": [a.size, a.size], "step_size": a.step, "n_internal": n_internal,
           "scene_s": time.perf_counter() - t0}
    t0 = time.perf_counter()
    dst = compression.main([src, "--out_dir", os.path.join(work, "min"), "--overwrite"])[0]        # the CLI's defaults
    out["compress_s"] = time.perf_counter() - t0
    out["file_MB"] = {"float16": os.path.getsize(src) / 2 ** 20, "compressed": os.path.getsize(dst) / 2 ** 20}
    print(json.dumps(out), flush=True)

    W = H = a.size
    c2w = cams[0]

    def first_image(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tree = N3Tree.load(dst, map_location=dev, **kw)
        t1 = time.perf_counter()
        with torch.no_grad():
            im = VolumeRenderer(tree, step_size=a.step).render_persp(c2w, width=W, height=H, fx=focal, fast=True)
        torch.cuda.synchronize()
        return tree, im, {"load_s": t1 - t0, "to_first_image_s": time.perf_counter() - t0}

    # second pass of each: the first one also pays for the file cache and the code objects
    first_image(); first_image(keep_quantized=True)
    ftree, _, out["load_float"] = first_image()
    qtree, _, out["load_palette"] = first_image(keep_quantized=True)
    out["device_bytes"] = {"float": qtree.float_nbytes, "palette": qtree.nbytes, "float_measured": ftree.data.numel() * 4 +
                           4 * (ftree.child.numel() + ftree.parent_depth.numel())}
    out["bits"], out["n_retained"] = qtree.bits, qtree.n_retained
    rf, rq = VolumeRenderer(ftree, step_size=a.step), VolumeRenderer(qtree, step_size=a.step)
    K, r, Kq = qtree.basis_dim, qtree.n_retained, qtree.basis_dim - qtree.n_retained
    for fast in (False, True):
        key = "fast" if fast else "exact"
        with torch.no_grad():
            fn_f = lambda: rf.render_persp(c2w, width=W, height=H, fx=focal, fast=fast)
            fn_q = lambda: rq.render_persp(c2w, width=W, height=H, fx=focal, fast=fast)
            res = {"float_ms": []}
            for lanes in a.lanes:
                res[f"palette_lanes{lanes}_ms"] = []
            for fn in (fn_f, fn_q):
                window(fn, 10)                                              # warm-up
            for _ in range(a.windows):                                      # alternate the kernels inside every round
                res["float_ms"].append(window(fn_f, a.renders))
                for lanes in a.lanes:
                    oops.set_lanes_per_ray(lanes, 0)
                    res[f"palette_lanes{lanes}_ms"].append(window(fn_q, a.renders))
                oops.set_lanes_per_ray(0, 0)
            diff = max(float((rq.render_persp(c, width=W, height=H, fx=focal, fast=fast) -
                              rf.render_persp(c, width=W, height=H, fx=focal, fast=fast)).abs().max()) for c in cams)
        cw = oops.octree_count_work(ftree.view(), c2w, W, H, focal, rf._opts(fast))
        shaded, other = cw["shaded_samples"], cw["samples"] - cw["shaded_samples"]
        common = other * 4 + cw["child_loads"] * 4 + W * H * 12
        alg_f = shaded * 4 * (3 * K + 1) + common
        alg_q = shaded * (2 * qtree._layout.idx_stride + 4 + 8 * Kq + 8 * r) + common
        summary = {k: {"best": min(v), "median": float(np.median(v)), "all": v} for k, v in res.items()}
        best_q = min(summary[k]["best"] for k in summary if k.startswith("palette"))
        out[f"render_{key}"] = dict(summary, palette_over_float=best_q / summary["float_ms"]["best"], work=cw,
                                    bytes_per_shaded_sample={"float": 4 * (3 * K + 1),
                                                             "palette_leaf": 2 * qtree._layout.idx_stride + 4 + 8 * r,
                                                             "palette_lookups": 8 * Kq},
                                    algorithmic_bytes={"float": alg_f, "palette": alg_q},
                                    algorithmic_GBps={"float": alg_f / summary["float_ms"]["best"] / 1e6, "palette": alg_q / best_q / 1e6},
                                    max_abs_image_diff=diff)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
