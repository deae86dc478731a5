#!/usr/bin/env python
"""Timing of the NDC launches of the PlenOctree side on the exported forward-facing rig (scripts/export_scene.py llff: 20
views, 1008 x 756 after --factor 4), at the extraction's sizes (init_grid_depth 8 -> 512^3 grid over the NDC cube).

The scene is octree_bench.py's -- three fuzzy spheres' density, random SH16 coefficients -- placed in front of the rig and
sampled on the grid of the NDC cube through the inverse of convert_to_ndc.  Prints one JSON line: time per view of the NDC
weight mask, the NDC forward (exact and early stop) and the NDC backward.  For information: there is no world-space
counterpart of the same scene to hold these against (octree_bench.py times the world-space launches on its own rig).
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--size", type=int, nargs=2, default=[756, 1008], metavar=("H", "W"))
    p.add_argument("--views", type=int, default=20)
    p.add_argument("--step", type=float, default=1e-4)
    p.add_argument("--reps", type=int, default=2)
    a = p.parse_args()
    import export_scene
    from octree_bench import timed
    from plenoctree_amd import build, octree_ops as oops
    from plenoctree_amd.nerf_sh.nerf import llff, utils
    from plenoctree_amd.octree.svox import N3Tree, NDCConfig, VolumeRenderer
    build.build(verbose=False)
    dev = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as tmp:
        export_scene.write_llff(tmp, a.size[0], a.size[1], a.views, 4, dev)
        args = utils.define_flags().parse_args(["--config", "llff", "--data_dir", tmp, "--train_dir", tmp])
        utils.update_flags(args)
        ds = llff.get_dataset("train", args, dev)
    H, W, focal = ds.h, ds.w, ds.focal
    ndc = NDCConfig(W, H, focal)
    cams = torch.from_numpy(np.ascontiguousarray(ds.camtoworlds)).to(dev)
    depth, reso, K = a.depth, 2 ** (a.depth + 1), 16
    # the grid of the NDC cube, back in the rig's own frame: z_w = 2 / (z' - 1), x_w = -x' z_w / cw, y_w = -y' z_w / ch undo the
    # projection (near = 1); the loader divided lengths by 0.75 x the nearest bound and moved the origin to the mean camera, (0, 0, 4)
    ax = ((torch.arange(reso, device=dev, dtype=torch.float32) + 0.5) / reso - 0.5) * 2.0
    scale = 1.0 / (export_scene.LLFF_NEAR * 0.75)
    zw = 2.0 / (ax - 1.0)
    xw = -ax[:, None] * zw[None, :] / (2.0 * focal / W)                 # [x, z]
    yw = -ax[:, None] * zw[None, :] / (2.0 * focal / H)                 # [y, z]
    X, Y, Z = xw[:, None, :] / scale, yw[None, :, :] / scale, zw[None, None, :] / scale + 4.0
    sig = torch.zeros(reso, reso, reso, device=dev)
    for c, r in (((0.0, 0.0, 0.0), 0.6), ((0.7, 0.3, 0.2), 0.3), ((-0.5, -0.4, 0.5), 0.35)):
        d2 = (X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2
        sig += 40.0 * torch.sigmoid((r - d2.sqrt()) * 60.0)
    sig = sig.reshape(-1).contiguous()
    tree = N3Tree(N=2, data_dim=3 * K + 1, depth_limit=depth, radius=1.0, center=[0, 0, 0], data_format=f"SH{K}", map_location=dev)
    out = {"image": [H, W], "views": int(cams.shape[0]), "reso": reso, "step_size": a.step, "focal": focal,
           "sigma_positive_fraction": float((sig > 1.0).float().mean())}
    opts = oops.render_opts(a.step)
    wt = torch.zeros(reso ** 3, device=dev)
    gw = lambda: oops.grid_weight_render(sig, reso, cams, focal, focal, W, H, opts, tree.offset, tree.invradius, grid_weight=wt, ndc=ndc)
    out["ndc_grid_weight_ms_per_view"] = timed(gw, reps=1) / cams.shape[0]
    mask = oops.threshold_mask(wt, 1e-3)
    out["mask_voxels"] = int(mask.sum())
    tree.refine_from_mask(mask)
    out["n_internal"] = tree.n_internal
    node0, count = tree.max_depth_nodes()
    pts = tree.sample_max_depth_cells(1, u=torch.full((count * 8, 3), 0.5, device=dev)).view(-1, 3)
    idx = ((pts / 2.0 + 0.5) * reso).long().clamp_(0, reso - 1)
    leaf = tree.max_depth_data()
    leaf.copy_(torch.randn(leaf.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 0.5)
    leaf[:, -1] = sig[(idx[:, 0] * reso + idx[:, 1]) * reso + idx[:, 2]]
    r = VolumeRenderer(tree, step_size=a.step, ndc=ndc)

    def render_all(fast):
        with torch.no_grad():
            return [r.render_persp(c, width=W, height=H, fx=focal, fast=fast) for c in cams]

    for fast in (False, True):
        out[f"ndc_render_{'fast' if fast else 'exact'}_ms_per_view"] = timed(lambda: render_all(fast), reps=a.reps) / cams.shape[0]
    ims = render_all(False)
    out["image_mean"] = float(torch.stack(ims).mean())
    out["seen_fraction"] = float(((torch.stack(ims) - 1.0).abs().amax(-1) > 1e-3).float().mean())
    gt = torch.rand_like(ims[0])
    grad = torch.zeros_like(tree.data)

    def bwd():
        for c, imc in zip(cams, ims):
            _, g = oops.image_mse(imc, gt)
            oops.octree_render_persp_bwd(tree.view(), c, W, H, focal, r._opts(False), g, grad, out_rgb=imc, ndc=ndc)

    out["ndc_render_bwd_reusing_fwd_ms_per_view"] = timed(bwd, reps=a.reps) / cams.shape[0]
    out["grad_abs_sum"] = float(grad.double().abs().sum())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
