#!/usr/bin/env python
"""Float, float16 and palette renderers on the same tree, alternating in one process (profiles/EXPERIMENTS.md).

Scene: scripts/quant_render_bench.py's (= scripts/octree_bench.py's analytic one: three fuzzy spheres on a 2^(depth+1) grid,
weight-masked by --cams views, random SH leaves; depth 8 gives about 923 k nodes), saved as N3Tree.save writes it: float16.
That file is loaded twice, as `N3Tree.load(path)` and with `keep_half=True`, so the two trees hold the same values and the two
images must be equal bit for bit (checked on every camera, reported, not timed).  The palette form is the one of
scripts/aux_render_bench.py -- the tree's sigma, --bits-bit palettes of random colours and random indices: the bytes per
sample of a compressed tree, not its picture; --no_palette leaves it out.

Measured, one JSON line: per form the device bytes and, for the exact and the early-stop preset, the milliseconds per
--size x --size view (HIP events around --renders back-to-back renders after a warm-up, the forms alternating inside every
one of --windows rounds; best, median and the spread (max - min) / min over the windows), and half / float of the medians.
--lanes sets the lanes per ray of every form (0 = default 4).

On a checkout without the float16 entry points only the float and palette forms are timed: the same script measures the
parent commit's float renderer.  Nothing here is asserted beyond the image equality; bench.py is not involved.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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
    p.add_argument("--lanes", type=int, default=0)
    p.add_argument("--renders", type=int, default=100, help="back-to-back renders per timed window")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--no_palette", action="store_true")
    p.add_argument("--workdir", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("half_render_bench needs a ROCm GPU: nothing here can be measured on a CPU")
    from plenoctree_amd import build, octree_ops as oops
    from plenoctree_amd.octree import svox
    from quant_render_bench import build_scene
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    work = a.workdir or tempfile.mkdtemp(prefix="half_bench_")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "tree.npz")
    cams, focal, n = build_scene(a, dev, src)
    have_half = hasattr(oops, "octree_render_half_persp")
    K = a.basis
    f = svox.N3Tree.load(src, map_location=dev)
    geometry = 4 * (f.child.numel() + f.parent_depth.numel())
    out = {"basis_dim": K, "depth": a.depth, "image": [a.size, a.size], "step_size": a.step, "n_internal": int(n), "lanes": a.lanes,
           "renders_per_window": a.renders, "windows": a.windows, "half_entry_points": have_half,
           "device_bytes": {"float": f.data.numel() * 4 + geometry}}
    fv = f.view()
    if have_half:
        h = svox.N3Tree.load(src, map_location=dev, keep_half=True)
        hv = h.half_view()
        out["device_bytes"]["half"] = h.nbytes
        out["row_stride"] = h.row_stride
    if not a.no_palette:
        z = np.load(src)
        P = 1 << a.bits
        rs = np.random.RandomState(0)
        files = {k: z[k] for k in ("data_dim", "child", "parent_depth", "n_internal", "depth_limit", "invradius3", "offset", "data_format")}
        files.update(sigma=np.ascontiguousarray(z["data"][:n, ..., -1]), quant_colors=(rs.randn(K, P, 3) * 0.5).astype(np.float16),
                     quant_map=rs.randint(0, P, size=(K, n, 2, 2, 2)).astype(np.uint16))
        q = svox.QuantizedN3Tree(svox._NpzDict(files), dev)
        qv = q.quant_view()
        out["device_bytes"]["palette"] = q.nbytes
        del z, files
    W = H = a.size
    c2w = cams[0]
    oops.set_lanes_per_ray(a.lanes, 0)
    for fast in (False, True):
        thr = 1e-2 if fast else 0.0
        opts = oops.render_opts(a.step, 1.0, thr, thr)
        variants = {"float": lambda: oops.octree_render_persp(fv, c2w, W, H, focal, opts)}
        if have_half:
            variants["half"] = lambda: oops.octree_render_half_persp(hv, c2w, W, H, focal, opts)
        if not a.no_palette:
            variants["palette"] = lambda: oops.octree_render_quant_persp(qv, c2w, W, H, focal, opts)
        res = {k: [] for k in variants}
        with torch.no_grad():
            for fn in variants.values():
                window(fn, 10)                                              # warm-up
            for _ in range(a.windows):                                      # the forms alternate inside every round
                for k, fn in variants.items():
                    res[k].append(window(fn, a.renders))
            rec = {k: {"best": min(v), "median": float(np.median(v)), "spread": (max(v) - min(v)) / min(v), "all": v}
                   for k, v in res.items()}
            rec["image_sum"] = float(variants["float"]().double().sum())
            if have_half:
                rec["half_over_float"] = rec["half"]["median"] / rec["float"]["median"]
                equal = [bool(torch.equal(oops.octree_render_half_persp(hv, c, W, H, focal, opts),
                                          oops.octree_render_persp(fv, c, W, H, focal, opts))) for c in cams]
                rec["half_equals_float_bit_for_bit"] = all(equal)
                assert all(equal), "the float16 render differs from the float render of the same file"
        out["fast" if fast else "exact"] = rec
    oops.set_lanes_per_ray(0, 0)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
