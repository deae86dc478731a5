"""Object insertion: renders several PlenOctrees placed in one scene, each under its own rotation, uniform scale and
translation (svox.SceneRenderer; the definition: include/plenoctree_octree.h, "scene").  No reference counterpart.

    python -m plenoctree_amd.octree.compose --scene S.json --output_dir OUT
        --orbit RADIUS ELEV_DEG N [--width W --height H --focal F]     N cameras on a circle around the world origin
      | --config C --data_dir DATA [flags of the dataset's parser]      the test-split poses of a dataset
        [--write_vid F.gif] [--renderer_step_size 1e-4] [--no_early_stop]

Scene file (paths relative to the file; rotation, scale and translation are optional):
    {"background": 1.0,
     "instances": [{"tree": "a.npz", "rotation": [[..3x3..]] | {"axis": [x, y, z], "angle_deg": a}, "scale": 1.0,
                    "translation": [x, y, z]}, ...]}
Writes OUT/NNN.png per camera; prints the node count of every instance and the milliseconds per frame.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from ..nerf_sh.nerf.datasets import pose_spherical
from .svox import Instance, N3Tree, SceneRenderer


def define_flags():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    a = p.add_argument
    a("--scene", type=str, required=True)
    a("--output_dir", type=str, required=True)
    a("--orbit", type=float, nargs=3, default=None, metavar=("RADIUS", "ELEV_DEG", "N"))
    a("--width", type=int, default=800)
    a("--height", type=int, default=800)
    a("--focal", type=float, default=1111.111)
    a("--config", type=str, default=None)
    a("--data_dir", type=str, default=None)
    a("--write_vid", type=str, default=None)
    a("--renderer_step_size", type=float, default=1e-4)
    a("--no_early_stop", action="store_true")
    return p


def rotation_of(spec):
    """3x3 float64 of a scene file's "rotation": a matrix, or {"axis", "angle_deg"} (Rodrigues)."""
    if spec is None:
        return np.eye(3)
    if isinstance(spec, dict):
        if set(spec) != {"axis", "angle_deg"}:
            raise ValueError(f'"rotation": expected a 3x3 matrix or {{"axis", "angle_deg"}}, got keys {sorted(spec)}')
        axis = np.asarray(spec["axis"], np.float64)
        if axis.shape != (3,) or not np.isfinite(axis).all() or not np.linalg.norm(axis) > 0:
            raise ValueError(f'"rotation": axis {spec["axis"]!r} is not a non-zero 3-vector')
        axis = axis / np.linalg.norm(axis)
        th = np.deg2rad(float(spec["angle_deg"]))
        K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
    return np.asarray(spec, np.float64)


def load_scene(path, device):
    """(instances, background) of a scene file; a tree named twice is loaded once."""
    with open(path) as f:
        spec = json.load(f)
    unknown = set(spec) - {"background", "instances"}
    if unknown or not isinstance(spec.get("instances"), list) or not spec["instances"]:
        raise ValueError(f'{path}: expected {{"background", "instances": [..]}} with at least one instance'
                         + (f", unknown keys {sorted(unknown)}" if unknown else ""))
    base, trees, instances = os.path.dirname(os.path.abspath(path)), {}, []
    for k, item in enumerate(spec["instances"]):
        unknown = set(item) - {"tree", "rotation", "scale", "translation"}
        if unknown or "tree" not in item:
            raise ValueError(f"{path}: instance {k}: expected tree[, rotation, scale, translation], got {sorted(item)}")
        file = os.path.join(base, item["tree"])
        if file not in trees:
            trees[file] = N3Tree.load(file, map_location=device)
        instances.append(Instance(trees[file], rotation_of(item.get("rotation")), item.get("translation"), item.get("scale")))
    return instances, float(spec.get("background", 1.0))


def cameras(args, device, dataset_flags=()):
    """(list of c2w [4,4] float32, width, height, focal).  dataset_flags: what the command line holds beyond this tool's own
    flags; with --config they go to the dataset's parser (nerf_sh/nerf/utils.py), with --orbit there must be none."""
    if (args.orbit is None) == (args.config is None):
        raise ValueError("octree.compose: give either --orbit RADIUS ELEV_DEG N or --config C --data_dir DATA")
    if args.orbit is not None:
        if dataset_flags:
            raise ValueError(f"octree.compose: unknown flags {list(dataset_flags)} (dataset flags go with --config)")
        radius, elev, n = args.orbit
        if not (radius > 0 and n >= 1 and n == int(n)):
            raise ValueError(f"--orbit {radius} {elev} {n}: RADIUS must be > 0 and N a whole number >= 1")
        if args.width < 1 or args.height < 1 or not args.focal > 0:
            raise ValueError("--width / --height must be >= 1 and --focal > 0")
        return [pose_spherical(360.0 * k / int(n), elev, radius) for k in range(int(n))], args.width, args.height, args.focal
    from ..nerf_sh.nerf import llff, utils
    from . import extraction
    flags = ["--config", args.config] + (["--data_dir", args.data_dir] if args.data_dir else [])
    dargs = utils.define_flags().parse_args(flags + list(dataset_flags))
    utils.update_flags(dargs)
    if extraction.uses_ndc(dargs):
        raise NotImplementedError("octree.compose: the cameras of an NDC scene (--dataset llff without --spherify) are not built: "
                                  "a scene is composed in world space")
    dataset = llff.get_dataset("test", dargs, device)
    return [dataset.camtoworlds[i] for i in range(dataset.size)], dataset.w, dataset.h, dataset.focal


@torch.no_grad()
def main(argv=None):
    args, dataset_flags = define_flags().parse_known_args(argv)
    if args.write_vid is not None and os.path.splitext(args.write_vid)[1].lower() != ".gif":
        raise ValueError(f"--write_vid {args.write_vid}: only animated GIF output is built; give a .gif path")
    if not torch.cuda.is_available():
        raise RuntimeError("octree.compose needs a ROCm GPU: there is no CPU fallback")
    device = torch.device("cuda", torch.cuda.current_device())
    cams, width, height, focal = cameras(args, device, dataset_flags)
    instances, background = load_scene(args.scene, device)
    for k, i in enumerate(instances):
        print(f"instance {k}: {i.tree.n_internal} nodes, {i.tree.data_format}, scale {i.scale:g}", flush=True)
    renderer = SceneRenderer(instances, step_size=args.renderer_step_size, background_brightness=background)
    from PIL import Image
    os.makedirs(args.output_dir, exist_ok=True)
    frames, spent = [], 0.0
    for idx, c2w in enumerate(cams):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        im = renderer.render_persp(torch.as_tensor(np.asarray(c2w, np.float32)), width=width, height=height, fx=focal,
                                   fast=not args.no_early_stop)
        torch.cuda.synchronize()
        spent += time.perf_counter() - t0
        frames.append(Image.fromarray((im.clamp(0, 1) * 255).to(torch.uint8).cpu().numpy()))
        path = os.path.join(args.output_dir, f"{idx:03d}.png")
        frames[-1].save(path)
        print("Wrote", path, flush=True)
    print(f"{len(cams)} frames of {width} x {height}, {1e3 * spent / len(cams):.3f} ms per frame", flush=True)
    if args.write_vid is not None:
        print("Writing to", args.write_vid, flush=True)
        frames[0].save(args.write_vid, save_all=True, append_images=frames[1:], duration=50, loop=0)
    return len(cams)


if __name__ == "__main__":
    main(sys.argv[1:])
