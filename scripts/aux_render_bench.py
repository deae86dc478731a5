#!/usr/bin/env python
"""What the renderer's extra outputs (alpha, depth, surface distance) cost: render with them against render without, on the
float tree and on a palette-form tree, next to the time of a march that reads sigma only (pxo_octree_count_work).

Scene: scripts/quant_render_bench.py's (= scripts/octree_bench.py's analytic one: three fuzzy spheres on a 2^(depth+1) grid,
weight-masked by --cams views, random SH leaves).  The palette form is NOT made by octree.compression (minutes of host time
at this size): it carries the float tree's sigma (rounded to float16, so the float tree it is compared with is the dequantised
one), --bits-bit palettes of random float16 colours and random indices -- the geometry, the sample sequence and the bytes per
sample of a compressed tree, with less locality in its palette lookups than a real one has.

One JSON line.  Per preset (exact, early-stop): HIP events around --renders back-to-back renders of one --size x --size view,
--windows windows per variant after a warm-up, the variants alternating inside every round; best, median and all windows.
A library without the aux entry points (an older build, for A/B runs of the rgb-only kernels) is timed without them.
Nothing here is asserted except that the rgb beside aux is bit-equal to the rgb without; bench.py is not involved.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


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
    p.add_argument("--bits", type=int, default=16)
    p.add_argument("--renders", type=int, default=100, help="back-to-back renders per timed window")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--surface_thresh", type=float, default=0.5)
    p.add_argument("--workdir", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aux_render_bench needs a ROCm GPU: nothing here can be measured on a CPU")
    from plenoctree_amd import build, octree_ops as oops
    from plenoctree_amd.octree import svox
    from quant_render_bench import build_scene
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    work = a.workdir or tempfile.mkdtemp(prefix="aux_bench_")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "tree.npz")
    cams, focal, n = build_scene(a, dev, src)
    z = np.load(src)
    K, P = a.basis, 1 << a.bits
    rs = np.random.RandomState(0)
    files = {k: z[k] for k in ("data_dim", "child", "parent_depth", "n_internal", "depth_limit", "invradius3", "offset", "data_format")}
    sigma = np.ascontiguousarray(z["data"][:n, ..., -1]).astype(np.float16)
    files.update(sigma=sigma, quant_colors=(rs.randn(K, P, 3) * 0.5).astype(np.float16),
                 quant_map=rs.randint(0, P, size=(K, n, 2, 2, 2)).astype(np.uint16))
    q = svox.QuantizedN3Tree(svox._NpzDict(files), dev)
    f = q.dequantize()
    del z, files
    have_aux = hasattr(oops, "octree_render_aux_persp")
    out = {"basis_dim": K, "depth": a.depth, "image": [a.size, a.size], "step_size": a.step, "n_internal": int(n), "bits": a.bits,
           "renders_per_window": a.renders, "windows": a.windows, "aux_entry_points": have_aux,
           "device_bytes": {"float": q.float_nbytes, "palette": q.nbytes}}
    W = H = a.size
    c2w = cams[0]
    fv, qv = f.view(), q.quant_view()
    for fast in (False, True):
        thr = 1e-2 if fast else 0.0
        opts = oops.render_opts(a.step, 1.0, thr, thr)
        variants = {"float_rgb": lambda: oops.octree_render_persp(fv, c2w, W, H, focal, opts),
                    "palette_rgb": lambda: oops.octree_render_quant_persp(qv, c2w, W, H, focal, opts),
                    # the renderer's march reading sigma only, one thread per ray (no leaf flags: count_leaves=False)
                    "sigma_only_march": lambda: oops.octree_count_work(fv, c2w, W, H, focal, opts, count_leaves=False)}
        if have_aux:
            variants["float_aux"] = lambda: oops.octree_render_aux_persp(fv, c2w, W, H, focal, opts, surface_thresh=a.surface_thresh)
            variants["palette_aux"] = lambda: oops.octree_render_aux_persp(qv, c2w, W, H, focal, opts, surface_thresh=a.surface_thresh)
        res = {k: [] for k in variants}
        with torch.no_grad():
            for fn in variants.values():
                window(fn, 5)                                               # warm-up
            for _ in range(a.windows):
                for k, fn in variants.items():
                    res[k].append(window(fn, a.renders if k != "sigma_only_march" else max(a.renders // 10, 1)))
        rec = {k: {"best": min(v), "median": float(np.median(v)), "spread": (max(v) - min(v)) / min(v), "all": v}
               for k, v in res.items()}
        if have_aux:
            for kind, view in (("float", fv), ("palette", qv)):
                rgb, aux = oops.octree_render_aux_persp(view, c2w, W, H, focal, opts, surface_thresh=a.surface_thresh)
                plain = variants[f"{kind}_rgb"]()
                assert torch.equal(rgb, plain), f"{kind}: rgb beside aux differs from the rgb-only render"
                rec[f"{kind}_aux_over_rgb"] = rec[f"{kind}_aux"]["median"] / rec[f"{kind}_rgb"]["median"]
                rec[f"{kind}_aux_extra_ms"] = rec[f"{kind}_aux"]["median"] - rec[f"{kind}_rgb"]["median"]
                fin = torch.isfinite(aux[..., 2])
                rec[f"{kind}_aux_summary"] = {"alpha_mean": float(aux[..., 0].mean()), "depth_mean": float(aux[..., 1].mean()),
                                              "surface_finite_fraction": float(fin.float().mean()),
                                              "surface_mean": float(aux[..., 2][fin].mean())}
        # sigma_only_march syncs once per call (it returns host counters): its time is an upper bound of that march's
        out["fast" if fast else "exact"] = rec
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
