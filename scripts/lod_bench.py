#!/usr/bin/env python
"""Level of detail at the reference's sizes, on the tree scripts/octree_bench.py builds (512^3 grid, 800x800 views, SH16):

  fill      pxo_tree_lod_fill with device events, and its share of the memory floor: every node but the root reads its
            eight rows and writes one, 4 * D * 9 * (n_internal - 1) bytes, over the 6.3 TB/s a streaming kernel reaches
  full      the full-depth render of the tree before the fill (its unused rows zero, as on a tree that was never filled) and
            after it, alternating: the fill must not move it
  levels    for every L the render through the capped view (VolumeRenderer(max_depth=L)) and of the standalone tree
            (tree.lod(L)), alternating; nodes, float32 bytes, and the PSNR of the level's images against the full-depth
            ones (the analytic scene has no photographs to score against)

Prints one JSON line.  Secondary measurement for profiles/EXPERIMENTS.md -- bench.py's headline stays the training metric.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_HBM_ACHIEVABLE_GBPS = 6300.0        # as scripts/octree_bench.py


def build_tree(a, dev):
    """The scene of scripts/octree_bench.py:measure: three fuzzy spheres on the grid, the weight mask of `cams` views, the tree
    of that mask, sigma from the grid and random SH in its deepest leaves.  Returns (tree, cams, focal)."""
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
    focal = 0.5 * a.size / np.tan(0.5 * 0.6911112)
    rs = np.random.RandomState(7)
    cams = torch.from_numpy(np.stack([pose_spherical(rs.uniform(0, 360), rs.uniform(-10, 60), 4.0311) for _ in range(a.cams)])).to(dev)
    wt = torch.zeros(reso ** 3, device=dev)
    oops.grid_weight_render(sig, reso, cams, focal, focal, a.size, a.size, oops.render_opts(a.step), tree.offset, tree.invradius,
                            grid_weight=wt)
    tree.refine_from_mask(oops.threshold_mask(wt, 1e-3))
    _, count = tree.max_depth_nodes()
    pts = tree.sample_max_depth_cells(1, u=torch.full((count * 8, 3), 0.5, device=dev)).view(-1, 3)
    idx = ((pts / 3.0 + 0.5) * reso).long().clamp_(0, reso - 1)
    leaf = tree.max_depth_data()
    leaf.copy_(torch.randn(leaf.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 0.5)
    leaf[:, -1] = sig[(idx[:, 0] * reso + idx[:, 1]) * reso + idx[:, 2]]
    tree.data.requires_grad_(False)
    return tree, cams, focal


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(fns, reps):
    """Each of `fns` warmed once, then timed `reps` times in turn (A B A B ...): {name: [ms, ...]}."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(event_ms(fn))
    return out


def spread(ms, per):
    ms = np.asarray(ms) / per
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max())}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--step", type=float, default=1e-4)
    p.add_argument("--cams", type=int, default=8)
    p.add_argument("--basis", type=int, default=16)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lod_bench needs a ROCm GPU: a timing without one is not a measurement")
    from plenoctree_amd import build
    from plenoctree_amd.octree.pruning import tree_stats
    from plenoctree_amd.octree.svox import VolumeRenderer
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    tree, cams, focal = build_tree(a, dev)
    W = H = a.size
    n, D = tree.n_internal, tree.data_dim
    out = {"depth": a.depth, "image": [H, W], "basis_dim": a.basis, "step_size": a.step, "cams": a.cams, "reps": a.reps,
           "n_internal": n, "level_nodes": tree.level_nodes, "tree_data_MB": tree.data.numel() * 4 / 1e6}

    def renders(renderer, fast):
        with torch.no_grad():
            return [renderer.render_persp(c, width=W, height=H, fx=focal, fast=fast) for c in cams]

    unfilled = tree.clone()                                              # the rows no renderer reads stay zero in this one
    fill = alternate({"fill": lambda: tree.fill_internal_()}, a.reps)["fill"]     # idempotent: every pass does the same work
    floor_bytes = 4 * D * 9 * (n - 1)
    floor_ms = floor_bytes / (PEAK_HBM_ACHIEVABLE_GBPS * 1e9) * 1e3
    out["fill"] = {"ms": spread(fill, 1), "floor_bytes": floor_bytes, "floor_ms": floor_ms, "launches": tree.max_depth,
                   "share_of_floor": floor_ms / float(np.median(fill)), "GBps": floor_bytes / float(np.median(fill)) / 1e6}
    # where the gap to the floor goes: the same call without its first launch (the deepest level, most of the nodes) is the
    # cost of the launches that find few nodes of their depth among all n; then the whole fill again, which repairs the rows
    from plenoctree_amd import octree_ops as oops
    if tree.max_depth > 1:
        upper = alternate({"upper": lambda: oops.tree_lod_fill(tree.child, tree.parent_depth, tree.data.data, tree.max_depth - 1)},
                          a.reps)["upper"]
        tree.fill_internal_()
        moved = 4 * D * 9 * (n - 1 - tree.level_nodes[-1])
        out["fill"]["without_deepest_level"] = {"ms": spread(upper, 1), "launches": tree.max_depth - 1, "floor_bytes": moved,
                                                "nodes": n - 1 - tree.level_nodes[-1]}
    leaf = tree.child == 0
    out["fill"]["leaf_rows_untouched"] = bool(torch.equal(tree.data.data[leaf], unfilled.data.data[leaf]))

    r_full, r_unfilled = VolumeRenderer(tree, step_size=a.step), VolumeRenderer(unfilled, step_size=a.step)
    out["full"] = {}
    for fast in (True, False):
        t = alternate({"unfilled": lambda: renders(r_unfilled, fast), "filled": lambda: renders(r_full, fast)}, a.reps)
        same = all(torch.equal(x, y) for x, y in zip(renders(r_unfilled, fast), renders(r_full, fast)))
        out["full"]["fast" if fast else "exact"] = {"unfilled_ms_per_image": spread(t["unfilled"], a.cams),
                                                    "filled_ms_per_image": spread(t["filled"], a.cams), "bit_identical": same}
    del unfilled, r_unfilled
    full_images = renders(r_full, True)
    out["levels"] = []
    for lvl in range(tree.max_depth + 1):
        level = tree.lod(lvl)
        r_cap, r_own = VolumeRenderer(tree, step_size=a.step, max_depth=lvl), VolumeRenderer(level, step_size=a.step)
        t = alternate({"capped": lambda: renders(r_cap, True), "standalone": lambda: renders(r_own, True)}, a.reps)
        images = renders(r_cap, True)
        same = all(torch.equal(x, y) for x, y in zip(images, renders(r_own, True)))
        mse = float(torch.stack([((x.clamp(0, 1) - y.clamp(0, 1)).double() ** 2).mean() for x, y in zip(images, full_images)]).mean())
        nodes, leaves, nbytes = tree_stats(level)
        out["levels"].append({"L": lvl, "cells_per_axis": 2 ** (lvl + 1), "nodes": nodes, "leaves": leaves, "float32_bytes": nbytes,
                              "capped_ms_per_image": spread(t["capped"], a.cams),
                              "standalone_ms_per_image": spread(t["standalone"], a.cams), "capped_equals_standalone": same,
                              "psnr_vs_full_depth": None if mse == 0 else -10.0 * float(np.log10(mse))})     # None: identical
        del level, r_own
    print(json.dumps(out))


if __name__ == "__main__":
    main()
