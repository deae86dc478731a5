#!/usr/bin/env python
"""Timing of the per-leaf weight accumulation and of the structural collapse on the scene of scripts/octree_bench.py
(three fuzzy spheres on a 512^3 grid, random SH16 leaves, 800x800 views), and what pruning by weight does to that tree.

Prints one JSON line:
  weight_{max,sum}_ms_per_view   pxo_octree_weight_accum_cams, one view per launch, beside
  count_work_ms_per_view         pxo_octree_count_work (the same march, counting) and
  render_exact_ms_per_view       the rgb forward render of the same views, all in this process
  weight_max_all_views_ms        the same views in ONE launch
  collapse_ms                    pxo_tree_collapse_mark + the scan + pxo_tree_collapse_emit at --weight_thresh
  before / after                 nodes, leaves, bytes and render times of the tree before and after pruning
  psnr_*                         held-out views of the pruned tree (and of the pruned tree with its heavy leaves split once)
                                 against the renders of the unpruned tree: the scene is analytic, there are no photographs, so
                                 the unpruned tree is the reference and has no figure of its own

A secondary measurement: bench.py's headline stays the training metric.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def build_scene(a, dev):
    """The tree of scripts/octree_bench.py: weight mask of `cams` training views at 1e-3, sigma from the grid, random SH."""
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
    poses = [pose_spherical(rs.uniform(0, 360), rs.uniform(-10, 60), 4.0311) for _ in range(a.cams + a.test_cams)]
    cams = torch.from_numpy(np.stack(poses)).to(dev)
    train, test = cams[:a.cams], cams[a.cams:]
    opts = oops.render_opts(a.step)
    wt = oops.grid_weight_render(sig, reso, train, focal, focal, W, H, opts, tree.offset, tree.invradius)
    tree.refine_from_mask(oops.threshold_mask(wt, 1e-3))
    node0, count = tree.max_depth_nodes()
    pts = tree.sample_max_depth_cells(1, u=torch.full((count * 8, 3), 0.5, device=dev)).view(-1, 3)
    idx = ((pts / 3.0 + 0.5) * reso).long().clamp_(0, reso - 1)
    leaf = tree.max_depth_data()
    leaf.copy_(torch.randn(leaf.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 0.5)
    leaf[:, -1] = sig[(idx[:, 0] * reso + idx[:, 1]) * reso + idx[:, 2]]
    tree.data.requires_grad_(False)
    return tree, train, test, W, H, focal


def tree_stats(tree):
    n = tree.n_internal
    return {"nodes": n, "leaves": tree.n_leaves, "bytes": 4 * n * (8 + 2 + 8 * tree.data_dim)}


def psnr(a, b):
    return float(-10.0 * torch.log10(((a.clamp(0, 1).double() - b.clamp(0, 1).double()) ** 2).mean()))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--step", type=float, default=1e-4)
    p.add_argument("--cams", type=int, default=8)
    p.add_argument("--test-cams", dest="test_cams", type=int, default=4)
    p.add_argument("--basis", type=int, default=16)
    p.add_argument("--weight-thresh", dest="weight_thresh", type=float, default=1e-3)
    p.add_argument("--refine-thresh", dest="refine_thresh", type=float, default=0.1)
    p.add_argument("--reps", type=int, default=3)
    a = p.parse_args()
    from plenoctree_amd import build, octree_ops as oops
    from plenoctree_amd.octree.svox import VolumeRenderer
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    tree, train, test, W, H, focal = build_scene(a, dev)
    out = {"depth": a.depth, "image": [H, W], "step_size": a.step, "cams": a.cams, "test_cams": a.test_cams, "basis_dim": a.basis,
           "weight_thresh": a.weight_thresh, "refine_thresh": a.refine_thresh, "before": tree_stats(tree)}
    r = VolumeRenderer(tree, step_size=a.step)
    exact, view = r._opts(False), tree.view()

    def render_all(rr, cams, fast):
        with torch.no_grad():
            return [rr.render_persp(c, width=W, height=H, fx=focal, fast=fast) for c in cams]

    n = a.cams
    for op in ("max", "sum"):
        buf = torch.zeros(tree.n_internal * 8, device=dev)
        out[f"weight_{op}_ms_per_view"] = timed(lambda: [oops.octree_weight_accum_cams(view, c[None], W, H, focal, exact, op, buf)
                                                         for c in train], a.reps) / n
    buf = torch.zeros(tree.n_internal * 8, device=dev)
    out["weight_max_all_views_ms"] = timed(lambda: oops.octree_weight_accum_cams(view, train, W, H, focal, exact, "max", buf), a.reps)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    import ctypes
    from plenoctree_amd import _lib

    def count_all():
        for c in train:
            cam, keep = oops._camera(c, W, H, focal, None)
            _lib.check(_lib.load().pxo_octree_count_work(ctypes.byref(view), ctypes.byref(cam), ctypes.byref(exact), oops._p(counts),
                                                         None, oops._stream()), "pxo_octree_count_work")
    out["count_work_ms_per_view"] = timed(count_all, a.reps) / n
    for fast in (False, True):
        out["before"][f"render_{'fast' if fast else 'exact'}_ms_per_view"] = timed(lambda: render_all(r, train, fast), a.reps) / n
    out["render_exact_ms_per_view"] = out["before"]["render_exact_ms_per_view"]

    weights = torch.zeros(tree.n_internal * 8, device=dev)
    oops.octree_weight_accum_cams(view, train, W, H, focal, exact, "max", weights)
    keep = weights > a.weight_thresh
    leaves = tree.child.view(-1) == 0
    out["leaves_kept"] = int((keep & leaves).sum())
    out["collapse_ms"] = timed(lambda: oops.tree_collapse(tree.child, tree.parent_depth, tree.data.data, keep), a.reps)
    ref_test = render_all(r, test, False)
    pruned = tree.clone()
    out["nodes_removed"] = pruned.prune_(keep.view(-1, 2, 2, 2), collapse=True)
    out["after"] = tree_stats(pruned)
    rp = VolumeRenderer(pruned, step_size=a.step)
    for fast in (False, True):
        out["after"][f"render_{'fast' if fast else 'exact'}_ms_per_view"] = timed(lambda: render_all(rp, train, fast), a.reps) / n
    out["psnr_pruned_vs_unpruned_train_views"] = float(np.mean([psnr(x, y) for x, y in zip(render_all(rp, train, False),
                                                                                             render_all(r, train, False))]))
    out["psnr_pruned_vs_unpruned_test_views"] = float(np.mean([psnr(x, y) for x, y in zip(render_all(rp, test, False), ref_test)]))
    # pruning followed by one split of the heavy leaves (children inherit the value: the function is unchanged, the sample
    # positions are not)
    with pruned.accumulate_weights("max") as accum:
        render_all(rp, train, False)
    if pruned.depth_limit < 10:
        pruned.depth_limit += 1
    out["split_nodes_added"] = pruned.refine_leaves(accum.value >= a.refine_thresh)
    out["after_split"] = tree_stats(pruned)
    out["psnr_split_vs_unpruned_test_views"] = float(np.mean([psnr(x, y) for x, y in zip(render_all(rp, test, False), ref_test)]))
    out["after_split"]["render_exact_ms_per_view"] = timed(lambda: render_all(rp, train, False), a.reps) / n
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
