#!/usr/bin/env python
"""The scene renderer against the plain renderer on the same tree, alternating in one process (DESIGN 8.9,
profiles/EXPERIMENTS.md).

Scene: scripts/quant_render_bench.py's tree (= scripts/octree_bench.py's analytic one: three fuzzy spheres on a 2^(depth+1)
grid, weight-masked by --cams views, random SH leaves; depth 8 gives about 923 k nodes; world radius 1.5), --size x --size,
the early-stop preset.  Variants, timed in turn inside every one of --windows rounds (HIP events around --renders
back-to-back renders after a warm-up; best, median and the spread (max - min) / min over the windows):
  plain       VolumeRenderer.render_persp of the tree
  scene1      a one-instance identity scene (bit for bit the plain image: checked, reported)
  disjoint2/4 2 / 4 instances of the tree at scale 0.45 side by side along x, none overlapping
  overlap2/4  2 / 4 instances at scale 0.8, rotated, their centres 0.35 apart: every ray through the middle has all of them live
One JSON line: per variant the milliseconds per image, each over plain, and the kernel's LDS per workgroup at 1 / 2 / 4 / 8
instances.  On a checkout without the scene entry points only `plain` is timed: the same script measures the parent commit.
Nothing is asserted beyond the one-instance equality; bench.py is not involved.
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


def rot_z(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--step", type=float, default=1e-4)
    p.add_argument("--cams", type=int, default=8)
    p.add_argument("--basis", type=int, default=16)
    p.add_argument("--renders", type=int, default=200, help="back-to-back renders per timed window")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--workdir", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scene_bench needs a ROCm GPU: nothing here can be measured on a CPU")
    from plenoctree_amd import build, octree_ops as oops
    from plenoctree_amd.octree import svox
    from quant_render_bench import build_scene, window
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    work = a.workdir or tempfile.mkdtemp(prefix="scene_bench_")
    os.makedirs(work, exist_ok=True)
    src = os.path.join(work, "tree.npz")
    cams, focal, n = build_scene(a, dev, src)
    tree = svox.N3Tree.load(src, map_location=dev)
    tree.data.requires_grad_(False)
    have_scene = hasattr(svox, "SceneRenderer")
    W = H = a.size
    c2w = cams[0]
    plain = svox.VolumeRenderer(tree, a.step)
    variants = {"plain": lambda: plain.render_persp(c2w, W, H, focal, fast=True)}
    out = {"basis_dim": a.basis, "depth": a.depth, "image": [W, H], "step_size": a.step, "n_internal": int(n),
           "renders_per_window": a.renders, "windows": a.windows, "scene_entry_points": have_scene}
    if have_scene:
        def scene(poses):
            r = svox.SceneRenderer([svox.Instance(tree, R, t, s) for R, t, s in poses], a.step)
            return lambda: r.render_persp(c2w, W, H, focal, fast=True)
        side = lambda k: [(rot_z(25.0 * i), ((i - 0.5 * (k - 1)) * 1.4, 0.0, 0.0), 0.45) for i in range(k)]
        over = lambda k: [(rot_z(37.0 * i), (0.35 * np.cos(2 * np.pi * i / k), 0.35 * np.sin(2 * np.pi * i / k), 0.0), 0.8)
                          for i in range(k)]
        variants.update(scene1=scene([(np.eye(3), (0.0, 0.0, 0.0), 1.0)]), disjoint2=scene(side(2)), overlap2=scene(over(2)),
                        disjoint4=scene(side(4)), overlap4=scene(over(4)))
        out["lds_bytes_per_workgroup"] = {str(k): oops.scene_lds_bytes(k) for k in (1, 2, 4, 8)}
    res = {k: [] for k in variants}
    with torch.no_grad():
        for fn in variants.values():
            window(fn, 5)                                                   # warm-up
        for _ in range(a.windows):                                          # the variants alternate inside every round
            for k, fn in variants.items():
                res[k].append(window(fn, a.renders))
        for k, v in res.items():
            out[k] = {"best": min(v), "median": float(np.median(v)), "spread": (max(v) - min(v)) / min(v), "all": v,
                      "over_plain": float(np.median(v)) / float(np.median(res["plain"]))}
        if have_scene:
            equal = [bool(torch.equal(svox.SceneRenderer([svox.Instance(tree)], a.step).render_persp(c, W, H, focal, fast=True),
                                      plain.render_persp(c, W, H, focal, fast=True))) for c in cams]
            out["scene1_equals_plain_bit_for_bit"] = all(equal)
            assert all(equal), "the one-instance identity scene differs from the plain render"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
