#!/usr/bin/env python
"""The footprint render (VolumeRenderer(lod_pixels=P)) against the plain full-depth render on the tree scripts/octree_bench.py
builds (512^3 grid, SH16, 922,817 nodes), from its 8 views at 800, 400, 200 and 100 pixels square with fx scaled so that the
field of view is kept:

  time      per size and preset the plain render and the footprint renders (lod_pixels 1 and 2) alternate in one process,
            `reps` repetitions of the 8 views each, device events: ms per image as median and range
  quality   PSNR against the 800 x 800 full-depth render of the same preset box-averaged down to the size -- the antialiased
            image of the same tree -- for the plain low-resolution render and for the footprint renders, side by side.  A
            pixel's centre sits at an integer coordinate (camera_ray), so pixel j of the small image looks where pixel f j of
            the large one does, f = 800 / size: the box is the f large pixels centred THERE (f + 1 taps, half weight on the two
            outer ones, the border repeated), not the block f j .. f j + f - 1, which sits half a small pixel to the side.
  samples   pxo_octree_count_work marches at full depth only (it is not extended by the footprint): not reported

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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from lod_bench import alternate, build_tree, spread          # noqa: E402


def box_down(image, f):
    """[H,W,3] -> [H/f,W/f,3]: the mean over the f x f large pixels centred on each small pixel's centre (see the header)."""
    if f == 1:
        return image
    x = image.permute(2, 0, 1)[None].double()
    w = torch.ones(f + 1, dtype=torch.float64, device=x.device)
    w[0] = w[-1] = 0.5
    w /= f
    x = torch.nn.functional.pad(x, (f // 2, f // 2, f // 2, f // 2), mode="replicate")
    k = (w[:, None] * w[None, :])[None, None].expand(3, 1, f + 1, f + 1)
    y = torch.nn.functional.conv2d(x, k, stride=f, groups=3)
    return y[0].permute(1, 2, 0)


def psnr(images, truths):
    mse = float(torch.stack([((x.double().clamp(0, 1) - y.clamp(0, 1)) ** 2).mean() for x, y in zip(images, truths)]).mean())
    return None if mse == 0 else -10.0 * float(np.log10(mse))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--size", type=int, default=800)
    p.add_argument("--sizes", type=int, nargs="+", default=[800, 400, 200, 100])
    p.add_argument("--lod_pixels", type=float, nargs="+", default=[1.0, 2.0])
    p.add_argument("--step", type=float, default=1e-4)
    p.add_argument("--cams", type=int, default=8)
    p.add_argument("--basis", type=int, default=16)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("footprint_bench needs a ROCm GPU: a timing without one is not a measurement")
    if any(a.size % s for s in a.sizes):
        raise SystemExit("--sizes must divide --size")
    from plenoctree_amd import build
    from plenoctree_amd.octree.svox import VolumeRenderer
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    tree, cams, focal = build_tree(a, dev)
    tree.fill_internal_()
    out = {"depth": a.depth, "basis_dim": a.basis, "step_size": a.step, "cams": a.cams, "reps": a.reps, "n_internal": tree.n_internal,
           "focal_at_%d" % a.size: focal, "camera_distance": 4.0311, "radius": 1.5, "sizes": {}}
    plain = VolumeRenderer(tree, step_size=a.step)
    foots = {P: VolumeRenderer(tree, step_size=a.step, lod_pixels=P) for P in a.lod_pixels}

    def renders(renderer, size, fast):
        fx = focal * size / a.size
        with torch.no_grad():
            return [renderer.render_persp(c, width=size, height=size, fx=fx, fast=fast) for c in cams]

    for fast in (True, False):
        preset = "fast" if fast else "exact"
        full = renders(plain, a.size, fast)
        for size in a.sizes:
            fns = {"plain": lambda: renders(plain, size, fast)}
            for P, r in foots.items():
                fns[f"lod_pixels_{P:g}"] = (lambda r=r: renders(r, size, fast))
            t = alternate(fns, a.reps)
            truth = [box_down(im, a.size // size) for im in full]
            row = {}
            plain_images = renders(plain, size, fast)
            for name in fns:
                images = plain_images if name == "plain" else renders(foots[float(name.split("_")[-1])], size, fast)
                row[name] = {"ms_per_image": spread(t[name], a.cams), "psnr_vs_box_averaged_full": psnr(images, truth),
                             "equals_plain": all(torch.equal(x, y) for x, y in zip(images, plain_images))}
            out["sizes"].setdefault(str(size), {})[preset] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
