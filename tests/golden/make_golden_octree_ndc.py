"""Generate the NDC fixture of the octree side by IMPORTING the reference's own convert_to_ndc (method of make_golden.py).

Run in the authoring container only (needs /root/reference):
    python tests/golden/make_golden_octree_ndc.py
Writes octree_ndc.npz (a few kB).

Reference module executed in place: octree/nerf/datasets.py (convert_to_ndc, :37-57, pure numpy), with empty stand-ins for `cv2`,
`tqdm` and `octree.nerf.utils` (its module-level imports; convert_to_ndc touches none of them).

Inputs: the svox cam2world_ray rays (oracle/octree_oracle.py) of the two cameras of tests/_octree_ndc_oracle.py at W, H, fx =
14, 10, 13.0 -- A the identity pose, B translation (0.2, -0.1, 0.05) with R = Ry(0.15) Rx(-0.1) -- plus a handful of explicit rays
(unnormalised directions, origins in front of and behind the near plane).  Outputs: convert_to_ndc of those rays evaluated in
float32 (`o32`, `d32`) and on float64 copies of the same float32 inputs (`o64`, `d64`), and e_ref_o / e_ref_d = max |float32 -
float64| over all of them: the reference's own float32 error, the unit of the bound in tests/test_octree_ndc_cpu.py."""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _reference_convert_to_ndc():
    for name in ("cv2", "tqdm", "octree", "octree.nerf", "octree.nerf.utils"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["tqdm"].tqdm = getattr(sys.modules["tqdm"], "tqdm", lambda it, *a, **k: it)
    sys.modules["octree"].nerf = sys.modules["octree.nerf"]
    sys.modules["octree.nerf"].utils = sys.modules["octree.nerf.utils"]
    spec = importlib.util.spec_from_file_location("octree.nerf.datasets", os.path.join(REF, "octree/nerf/datasets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.convert_to_ndc


def main():
    import _octree_ndc_oracle as N
    from oracle import octree_oracle as T
    convert = _reference_convert_to_ndc()
    W, H, fx = N.W, N.H, N.FX
    o, d = [], []
    for c2w in (N.camera_a(), N.camera_b()):
        for iy in range(H):
            for ix in range(W):
                oo, dd = T.cam2world_ray(ix, iy, c2w, W, H, fx, fx)
                o.append(oo); d.append(dd)
    extra_o = [[0.0, 0.0, 0.0], [0.3, -0.2, 0.5], [-0.4, 0.1, -0.5], [0.05, 0.07, 2.0], [1.0, 1.0, -0.99], [0.0, 0.0, -3.0]]
    extra_d = [[0.0, 0.0, -1.0], [0.1, 0.2, -2.0], [-0.3, 0.05, -0.7], [0.5, -0.5, -0.1], [0.01, -0.02, -1e-3], [0.2, 0.1, -1.0]]
    o = np.concatenate([np.stack(o), np.asarray(extra_o, np.float32)]).astype(np.float32)
    d = np.concatenate([np.stack(d), np.asarray(extra_d, np.float32)]).astype(np.float32)
    o32, d32 = convert(o, d, fx, W, H)
    assert o32.dtype == np.float32 and d32.dtype == np.float32
    o64, d64 = convert(o.astype(np.float64), d.astype(np.float64), fx, W, H)
    out = dict(width=W, height=H, focal=np.float32(fx), origins=o, directions=d, o32=o32, d32=d32, o64=o64, d64=d64,
               e_ref_o=np.abs(o32 - o64).max(), e_ref_d=np.abs(d32 - d64).max())
    path = os.path.join(HERE, "octree_ndc.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; e_ref_o", out["e_ref_o"], "e_ref_d", out["e_ref_d"])


if __name__ == "__main__":
    main()
