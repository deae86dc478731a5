"""Generate the LLFF fixtures by IMPORTING the reference's own loader (method of make_golden.py).

Run in the authoring container only (needs /root/reference):
    python tests/golden/make_golden_llff.py
Writes
  llff_tiny/             a forward-facing capture of the analytic three-sphere scene (scripts/export_scene.py `llff`): 9 poses,
                         images/ at 24 x 16 and images_2/ at 12 x 8 -- a few KB of PNGs, read by the tests through OUR loader
  llff_reference.npz     what the reference's `LLFF` class (nerf_sh/nerf/datasets.py:235-489) makes of that directory

Reference modules executed in place: nerf_sh/nerf/datasets.py (LLFF, convert_to_ndc) and nerf_sh/nerf/utils.py
(generate_rays, Rays), with stand-ins for `absl.flags`, `cv2`, `flax`, `jax` (host_count() = 1; no arithmetic goes through
them: the loader is numpy).  The loader's prefetch thread is a daemon and is never read from.

Per case `<split>_s<spherify>_f<factor>_h<llffhold>` (split in train / test, spherify 0 / 1, factor 0 / 2, llffhold 8 / 4):
camtoworlds, focal, h, w, images, render_poses (test) and the hold-out `indices`; for llffhold 8 also the rays of the cameras
`ray_cams` (first, middle, last of the split) and of the path poses `render_ray_poses` (0, 59, 119) -- a subset, to stay
well under the size limit of a committed file; every ray enters e_ref below.

ndc64_*: the reference's generate_rays and convert_to_ndc BODIES run on float64 copies of the same float32 poses (numpy
promotes: the float32 pixel grid is exact), for the same subset.  e_ref_origins / e_ref_directions: max |float32 reference
- float64 reference| over ALL NDC rays of all llffhold-8 cases -- the reference's own float32 error, the unit of the bounds
in tests/test_llff_cpu.py and tests/test_gpu_llff.py."""
import importlib.util
import os
import shutil
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
RENDER_RAY_POSES = np.array([0, 59, 119])


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _reference_modules():
    absl, flags, cv2 = types.ModuleType("absl"), types.ModuleType("absl.flags"), types.ModuleType("cv2")
    flags.FLAGS = types.SimpleNamespace()
    absl.flags = flags
    flax = types.ModuleType("flax")
    flax.struct = types.SimpleNamespace(dataclass=lambda cls: cls)
    flax.optim = types.SimpleNamespace(Optimizer=object)
    jax = types.ModuleType("jax")
    jax.host_count = lambda: 1
    for name in ("jax.dlpack", "jax.numpy", "jax.scipy"):
        sys.modules[name] = types.ModuleType(name)
    jax.dlpack, jax.numpy, jax.scipy = sys.modules["jax.dlpack"], sys.modules["jax.numpy"], sys.modules["jax.scipy"]
    pkg, pkg_nerf = types.ModuleType("nerf_sh"), types.ModuleType("nerf_sh.nerf")
    ds_stub = types.ModuleType("nerf_sh.nerf.datasets")        # utils imports datasets and the other way round
    pkg.nerf, pkg_nerf.datasets = pkg_nerf, ds_stub
    sys.modules.update({"absl": absl, "absl.flags": flags, "cv2": cv2, "flax": flax, "jax": jax, "nerf_sh": pkg,
                        "nerf_sh.nerf": pkg_nerf, "nerf_sh.nerf.datasets": ds_stub})
    ref_utils = _load("nerf_sh.nerf.utils", os.path.join(REF, "nerf_sh/nerf/utils.py"))
    pkg_nerf.utils = ref_utils
    ref_datasets = _load("nerf_sh.nerf.datasets", os.path.join(REF, "nerf_sh/nerf/datasets.py"))
    return ref_utils, ref_datasets


def main():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    sys.path.insert(0, ROOT)
    import export_scene
    tiny = os.path.join(HERE, "llff_tiny")
    shutil.rmtree(tiny, ignore_errors=True)
    cpu = torch.device("cpu")
    export_scene.write_llff(tiny, 16, 24, 9, 0, cpu)
    export_scene.write_llff(tiny, 8, 12, 9, 2, cpu)          # the same poses_bounds.npy: the full-size capture is 16 x 24

    ref_utils, ref_datasets = _reference_modules()
    out = {"render_ray_poses": RENDER_RAY_POSES}
    e_o = e_d = 0.0
    for hold in (8, 4):
        for split in ("train", "test"):
            for spherify in (False, True):
                for factor in (0, 2):
                    key = f"{split}_s{int(spherify)}_f{factor}_h{hold}_"
                    args = types.SimpleNamespace(data_dir=tiny, factor=factor, spherify=spherify, llffhold=hold,
                                                 render_path=False, batch_size=4, image_batching=False)
                    ds = ref_datasets.LLFF(split, args)
                    n = 9
                    held = np.arange(n)[::hold]
                    out[key + "indices"] = held if split == "test" else np.array([i for i in range(n) if i not in held])
                    out[key + "camtoworlds"] = np.asarray(ds.camtoworlds)
                    out[key + "focal"], out[key + "h"], out[key + "w"] = np.float64(ds.focal), ds.h, ds.w
                    assert ds.images.shape[0] == len(out[key + "indices"])
                    if hold != 8:
                        continue
                    out[key + "images"] = np.asarray(ds.images, np.float32).reshape(-1, ds.h, ds.w, 3)
                    n_cam = ds.camtoworlds.shape[0]
                    cams = np.unique([0, n_cam // 2, n_cam - 1])
                    out[key + "ray_cams"] = cams
                    rays = [np.asarray(r).reshape(n_cam, ds.h * ds.w, 3) for r in ds.rays]
                    for name, r in zip(("origins", "directions", "viewdirs"), rays):
                        out[key + "rays_" + name] = r[cams].astype(np.float32)
                    c2w_all, all_rays = np.asarray(ds.camtoworlds), rays
                    if split == "test":
                        out[key + "render_poses"] = np.asarray(ds.render_poses)
                        rrays = [np.asarray(r).reshape(120, ds.h * ds.w, 3) for r in ds.render_rays]
                        for name, r in zip(("origins", "directions", "viewdirs"), rrays):
                            out[key + "render_rays_" + name] = r[RENDER_RAY_POSES].astype(np.float32)
                        c2w_all = np.concatenate([np.asarray(ds.render_poses), c2w_all], 0)
                        all_rays = [np.concatenate([a, b], 0) for a, b in zip(rrays, rays)]
                    if spherify:
                        continue
                    # the reference's own bodies on float64 copies of the float32 poses
                    assert c2w_all.dtype == np.float32
                    r64 = ref_utils.generate_rays(ds.w, ds.h, np.float64(ds.focal), c2w_all.astype(np.float64))
                    o64, d64 = ref_datasets.convert_to_ndc(r64.origins, r64.directions, np.float64(ds.focal), ds.w, ds.h)
                    assert o64.dtype == np.float64 and d64.dtype == np.float64
                    o64, d64 = o64.reshape(len(c2w_all), -1, 3), d64.reshape(len(c2w_all), -1, 3)
                    e_o = max(e_o, float(np.abs(all_rays[0] - o64).max()))
                    e_d = max(e_d, float(np.abs(all_rays[1] - d64).max()))
                    first = 120 if split == "test" else 0
                    out[key + "ndc64_origins"], out[key + "ndc64_directions"] = o64[first + cams], d64[first + cams]
                    if split == "test":
                        out[key + "ndc64_render_origins"] = o64[RENDER_RAY_POSES]
                        out[key + "ndc64_render_directions"] = d64[RENDER_RAY_POSES]
    out["e_ref_origins"], out["e_ref_directions"] = np.float64(e_o), np.float64(e_d)
    np.savez_compressed(os.path.join(HERE, "llff_reference.npz"), **out)
    print(f"e_ref_origins {e_o:.3e}  e_ref_directions {e_d:.3e}")
    print("written:", tiny, os.path.getsize(os.path.join(HERE, "llff_reference.npz")), "bytes")


if __name__ == "__main__":
    main()
