#!/usr/bin/env python
"""Timing of the device meshing path against the host marching cubes it replaces, and of the tree-to-grid sampler.

    python scripts/mesh_bench.py [--sizes 256 512] [--reps 5 3] [--tree_depth 8] [--attrs] [--json out.json]

Field: "noise on a sphere", vol = 0.6 - |x| + 0.02 * N(0,1) on [-1,1]^3 (seeded, made on the GPU where gen_mesh's sigma grid
lives), iso 0: a thick shell of cells that exercises every case.  Per size, alternating and warmed:
  (a) device   mesh_ops.marching_cubes (finite check, workspace, count, emit) + the copy of the mesh to the host, host clock
               around work that ends in a synchronise
  (b) host     the copy of the volume to the host + isosurface.marching_cubes
and, with device events around the two library calls, pxo_mc_count and pxo_mc_emit on their own against the bytes they must
move (computed from the shapes below).  The meshes of (a) and (b) are compared for equality at every size that is timed.
--attrs adds, after each round's emit and outside its events, the two per-vertex stages on the mesh just emitted:
pxo_mc_vertex_gradients, and pxo_shade_points with SH16 rows gathered at random from a 2^18-row table (a tree's leaves in place)
along the normalised negative gradients.
Then pxo_tree_sigma_grid at depth tree_depth + 1 on a tree of three fuzzy spheres refined from its 2^(tree_depth+1) mask (the
scene of scripts/octree_bench.py).  Needs the GPU: there is nothing to time without one.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12        # bytes/s: MI355X HBM3E peak, and what a float4 copy achieves


def noise_sphere(n, device, seed=0):
    ax = torch.linspace(-1.0, 1.0, n, device=device)
    r = (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2).sqrt()
    noise = torch.randn(n, n, n, device=device, generator=torch.Generator(device=device).manual_seed(seed))
    return (0.6 - r + 0.02 * noise).contiguous()


def floors(n_points, n_vert, n_tri):
    """Least bytes each call must move through HBM (reads + writes), from the shapes alone.
    count: the volume once (4 B/point), a case and a flag byte per point out; the block sums are 16 B per 256 points.
    emit:  vertices: a flag byte per point in, per vertex 24 B position + 8 B inside index + 4 B id out (the two float32 end
           values come from lines the pass shares with its neighbours: not counted); triangles: a flag byte per point in (the
           case bytes of the cells that emit are not counted), every vertex id read at least once (4 B), 24 B per triangle out."""
    nb = -(-n_points // 256)
    k = {"mc_classify_kernel": 6 * n_points + 16 * nb, "scan kernels": 16 * nb,
         "mc_vertex_kernel": n_points + 36 * n_vert + 12 * nb, "mc_triangle_kernel": n_points + 4 * n_vert + 24 * n_tri + 4 * nb}
    return {"count": k["mc_classify_kernel"] + k["scan kernels"], "emit": k["mc_vertex_kernel"] + k["mc_triangle_kernel"],
            "kernels": k}


def spread(xs):
    return {"min_ms": min(xs) * 1e3, "median_ms": statistics.median(xs) * 1e3, "max_ms": max(xs) * 1e3, "n": len(xs)}


def bench_size(n, reps, dev, attrs=False):
    from plenoctree_amd import _lib, mesh_ops
    from plenoctree_amd.nerf_sh import isosurface
    from plenoctree_amd.ops import _f, _p, _stream
    vol = noise_sphere(n, dev)

    def device_path():
        v, f, _ = mesh_ops.marching_cubes(vol, 0.0)
        return v.cpu().numpy(), f.cpu().numpy()

    def host_path():
        return isosurface.marching_cubes(vol.cpu().numpy(), 0.0)

    dv, df = device_path()                      # warm both (code objects, allocator, numpy pages) and compare once
    hv, hf = host_path()
    equal = bool(np.array_equal(dv, hv) and np.array_equal(df, hf))
    t_dev, t_host = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); device_path(); t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); host_path(); t_host.append(time.perf_counter() - t0)
    # the two library calls on their own, device events
    lib = _lib.load()
    table, count = mesh_ops._device_tables(dev)
    nbytes = mesh_ops.mc_workspace_bytes(n, n, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = (ctypes.c_int64 * 4)()
    t_count, t_emit, t_grad, t_shade = [], [], [], []
    K, R = 16, 1 << 18
    if attrs:
        gen = torch.Generator(device=dev).manual_seed(1)
        leaves = torch.randn(R, 3 * K + 1, device=dev, generator=gen)
    for i in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        _lib.check(lib.pxo_mc_count(_f(vol), n, n, n, 0.0, _p(count), _p(ws), nbytes, counts, _stream()), "pxo_mc_count")
        e[1].record()
        nv, nt = counts[0] + counts[1] + counts[2], counts[3]
        v = torch.empty(nv, 3, dtype=torch.float64, device=dev)
        f = torch.empty(nt, 3, dtype=torch.int64, device=dev)
        ii = torch.empty(nv, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        e[2].record()
        _lib.check(lib.pxo_mc_emit(_f(vol), n, n, n, 0.0, _p(table), _p(ws), nbytes, counts, _p(v), _p(f), _p(ii), _stream()),
                   "pxo_mc_emit")
        e[3].record()
        torch.cuda.synchronize()
        if attrs:                               # after the emit's events have been read off the stream
            g = torch.empty(nv, 3, dtype=torch.float64, device=dev)
            rows = torch.randint(0, R, (nv,), device=dev, generator=gen)
            a = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            a[0].record()
            _lib.check(lib.pxo_mc_vertex_gradients(_f(vol), n, n, n, 0.0, _p(ws), nbytes, counts, _p(ii), _p(g), _stream()),
                       "pxo_mc_vertex_gradients")
            a[1].record()
            dirs = mesh_ops.shading_dirs(mesh_ops.unit_normals(g, [1.0] * 3))
            rgb = torch.empty(nv, 3, device=dev)
            a[2].record()
            _lib.check(lib.pxo_shade_points(_f(leaves), 3 * K + 1, _p(rows), _f(dirs), nv, K, None, _f(rgb), _stream()),
                       "pxo_shade_points")
            a[3].record()
            torch.cuda.synchronize()
            if i:
                t_grad.append(a[0].elapsed_time(a[1]) * 1e-3)
                t_shade.append(a[2].elapsed_time(a[3]) * 1e-3)
        if i:                                   # the first round warms
            t_count.append(e[0].elapsed_time(e[1]) * 1e-3)
            t_emit.append(e[2].elapsed_time(e[3]) * 1e-3)
    fl = floors(n ** 3, len(dv), len(df))
    out = {"size": n, "vertices": len(dv), "triangles": len(df), "device_equals_host": equal,
           "workspace_MB": nbytes / 1e6, "device_end_to_end": spread(t_dev), "host_end_to_end": spread(t_host),
           "speedup_median": statistics.median(t_host) / statistics.median(t_dev),
           "kernel_floor_bytes": fl["kernels"]}     # per kernel, for the times of a `rocprofv3 --kernel-trace --stats` run
    for name, ts in (("count", t_count), ("emit", t_emit)):
        # pxo_mc_count's time includes its device-to-host copy of the four totals and the synchronise
        med = statistics.median(ts)
        out[f"pxo_mc_{name}"] = dict(spread(ts), floor_bytes=fl[name], achieved_TB_per_s=fl[name] / med / 1e12,
                                     floor_ms_at_measured_peak=fl[name] / HBM_MEASURED * 1e3,
                                     share_of_measured_peak=fl[name] / med / HBM_MEASURED, share_of_spec_peak=fl[name] / med / HBM_SPEC)
    if attrs:
        # least traffic per vertex.  gradients: 8 B inside index + 1 B flag + 4 B id in, 24 B out (the float32 samples around the
        # edge share lines with the neighbouring vertices: not counted).  shade: 8 B row + 12 B direction in, 12 B out, and the
        # 3 K coefficients of a row picked at random (192 B; whole 32-byte sectors: 7 of them for a 196-byte row)
        for name, ts, fb in (("pxo_mc_vertex_gradients", t_grad, 37 * len(dv)), ("pxo_shade_points_sh16", t_shade, (32 + 224) * len(dv))):
            med = statistics.median(ts)
            out[name] = dict(spread(ts), floor_bytes=fb, achieved_TB_per_s=fb / med / 1e12, share_of_measured_peak=fb / med / HBM_MEASURED)
    return out


def bench_sigma_grid(tree_depth, reps, dev):
    from plenoctree_amd import mesh_ops, octree_ops as oops
    from plenoctree_amd.octree.svox import N3Tree
    reso = 2 ** (tree_depth + 1)
    ax = ((torch.arange(reso, device=dev, dtype=torch.float32) + 0.5) / reso - 0.5) * 3.0
    sig = torch.zeros(reso, reso, reso, device=dev)
    for c, r in (((0.0, 0.0, 0.0), 0.6), ((0.7, 0.3, 0.2), 0.3), ((-0.5, -0.4, 0.5), 0.35)):
        d2 = (ax[:, None, None] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2
        sig += 40.0 * torch.sigmoid((r - d2.sqrt()) * 60.0)
    tree = N3Tree(N=2, data_dim=49, depth_limit=tree_depth, radius=1.5, center=[0, 0, 0], data_format="SH16", map_location=dev)
    tree.refine_from_mask(oops.threshold_mask(sig.reshape(-1), 1.0))
    pts = tree.sample_max_depth_cells(1, u=torch.full((tree.max_depth_nodes()[1] * 8, 3), 0.5, device=dev)).view(-1, 3)
    idx = ((pts / 3.0 + 0.5) * reso).long().clamp_(0, reso - 1)
    tree.max_depth_data()[:, -1] = sig[idx[:, 0], idx[:, 1], idx[:, 2]]
    del sig, pts, idx
    depth = tree.max_depth + 1
    out = {"tree_depth": tree.max_depth, "n_internal": tree.n_internal, "grid_depth": depth, "side": (1 << depth) + 2}
    view = tree.view()
    for want_packed in (False, True):
        ts = []
        for i in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            s, p = mesh_ops.tree_sigma_grid(view, depth, pad=1, want_packed=want_packed, device=dev)
            e1.record()
            torch.cuda.synchronize()
            if i:
                ts.append(e0.elapsed_time(e1) * 1e-3)
            del s, p
        # least traffic: the grid out (4 B sigma, 8 B packed index per sample); in, the child array (32 B per node) and, per
        # cell, the 32-byte sector that holds its sigma (every cell's sigma ends its own 196-byte data row)
        floor = out["side"] ** 3 * (12 if want_packed else 4) + tree.n_internal * (32 + 8 * 32)
        med = statistics.median(ts)
        out["with_packed" if want_packed else "sigma_only"] = dict(
            spread(ts), floor_bytes=floor, achieved_TB_per_s=floor / med / 1e12, share_of_measured_peak=floor / med / HBM_MEASURED,
            share_of_spec_peak=floor / med / HBM_SPEC)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    p.add_argument("--reps", type=int, nargs="+", default=[5, 3], help="timed repeats per size (the last value repeats)")
    p.add_argument("--tree_depth", type=int, default=8, help="0 skips the tree-to-grid timing")
    p.add_argument("--attrs", action="store_true", help="also time pxo_mc_vertex_gradients and pxo_shade_points per size")
    p.add_argument("--json", type=str, default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench needs a ROCm GPU: a timing taken without one says nothing")
    from plenoctree_amd import build
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"marching_cubes": []}
    for i, n in enumerate(a.sizes):
        r = bench_size(n, a.reps[min(i, len(a.reps) - 1)], dev, attrs=a.attrs)
        out["marching_cubes"].append(r)
        print(json.dumps(r), flush=True)
    if a.tree_depth:
        out["tree_sigma_grid"] = bench_sigma_grid(a.tree_depth, 5, dev)
        print(json.dumps(out["tree_sigma_grid"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
