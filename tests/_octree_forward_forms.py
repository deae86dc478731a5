"""What tests/test_gpu_octree_forward_forms.py holds the forward renderers of the three storage forms to: SHA-256 of the bytes
of every output over float, float16 and palette trees, SH / SG / NDC / aux, a 13 x 7 camera and 67 explicit rays, exact and
fast options, at 4, 8 and 16 lanes per ray.  The forward kernels use no atomics, so the bits are reproducible.  measure() is run
once on the commit BEFORE a change of the forward path to write tests/golden/octree_forward_forms.json
(python tests/_octree_forward_forms.py, on the MI355X), and by the test on the tree under test."""
import copy
import functools
import hashlib
import json
import os
import sys

import numpy as np
import torch

f32, f16 = np.float32, np.float16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "octree_forward_forms.json")
LANES = (4, 8, 16)
W, H, FX = 13, 7, 11.0             # partial 2x2-patch tiles in both axes at every lanes-per-ray value (tiles 4x4, 8x4, 8x8)
N_RAYS = 67                        # no multiple of the 64, 32 or 16 rays of a block
STEP = 1e-3
SIGMA_SCALE = 6.0                  # as tests/_octree_sg_cases.py: some rays saturate, so the early stop is reached
# (kind, K) of the float and float16 trees; the palette trees: (K, retained, bits)
TREE_CASES = [("sh", K) for K in (1, 4, 9, 16, 25)] + [("sg", 4), ("sg", 16), ("ndc", 9), ("aux", 4), ("aux", 16)]
QUANT_CASES = ((16, 0, 8), (16, 1, 4), (4, 3, 2))


@functools.lru_cache(maxsize=None)
def tree(K):
    """The depth-3 shell of tests/_octree_cases.py (leaves at depths 1..3), its data rounded through float16: what the float
    and the float16 form both hold."""
    import _octree_cases as C
    t = copy.deepcopy(C.make_tree("shell", 3, K))
    t.data[..., -1] *= f32(SIGMA_SCALE)
    t.data[:] = t.data.astype(f16).astype(f32)
    assert np.isfinite(t.data).all() and len(set(t.parent_depth[t.leaves()[:, 0], 1].tolist())) == 3
    return t


def _rays(t, seed):
    import _octree_cases as C
    o, d = C.aimed_rays(t, seed, per_depth=lambda depth: 23)
    assert len(o) >= N_RAYS
    v = np.random.RandomState(seed + 1).randn(N_RAYS, 3)
    return o[:N_RAYS].copy(), d[:N_RAYS].copy(), (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _outputs(out):
    rgb = out[0] if isinstance(out, tuple) else out
    assert float(rgb.std()) > 1e-2, "a flat image: the rays miss the tree"
    return {"rgb": _sha(out[0]), "aux": _sha(out[1])} if isinstance(out, tuple) else {"rgb": _sha(out)}


def _tree_renders(oops, dev, kind, K):
    """{form: (persp, rays)}: the two renders of the float and the float16 tree of one case, as functions of the options."""
    import _octree_cases as C
    import _octree_ndc_oracle as N
    import _octree_sg_cases as G
    t = tree(K)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    child, data = up(t.child), up(t.data)
    packed, _ = oops.half_pack(up(t.data.astype(f16)), t.n_internal)
    views = {"float": oops.tree_view(child, data, t.offset, t.invradius),
             "half": oops.half_tree_view(child, packed, t.data_dim, t.offset, t.invradius)}
    keep = (child, data, packed)
    c2w = up(N.camera_b() if kind == "ndc" else C.look_at((3.4, 3.1, 2.6)))
    o, d, v = (up(a) for a in _rays(t, 40 + K))
    kw = {"sg": dict(lobes=up(G.lobes(K))), "ndc": dict(ndc=oops.ndc_spec(W, H, FX)), "sh": {}, "aux": {}}[kind]
    fns = {"float": (oops.octree_render_aux_persp, oops.octree_render_aux_rays) if kind == "aux" else
                    (oops.octree_render_persp, oops.octree_render_rays),
           "half": (oops.octree_render_half_aux_persp, oops.octree_render_half_aux_rays) if kind == "aux" else
                   (oops.octree_render_half_persp, oops.octree_render_half_rays)}
    return {form: (lambda opts, p=fns[form][0], tv=views[form]: (keep, p(tv, c2w, W, H, FX, opts, **kw))[1],
                   lambda opts, r=fns[form][1], tv=views[form]: (keep, r(tv, o, d, v, opts, **kw))[1]) for form in views}


def _quant_renders(oops, dev, K, retain, bits):
    import _octree_cases as C
    import _quant_cases as Q
    c = Q.case(K, retain, bits)
    t, n = c.tree, c.tree.n_internal
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    child = up(t.child)
    packed, lay = oops.quant_pack(up(c.quant_map.view(np.int16)), up(c.quant_colors), up(c.sigma.reshape(n * 8)),
                                  up(None if not retain else c.data_retained.reshape(retain, n * 8, 3)), n, K, retain, bits)
    view = oops.quant_tree_view(child, packed, lay, K, retain, bits, t.offset, t.invradius)
    keep = (child, packed)
    c2w = up(C.look_at((3.4, 3.1, 2.6), target=Q.CENTER))
    o, d, v = (up(a) for a in _rays(t, 60 + K + bits))
    return {"plain": (lambda opts: (keep, oops.octree_render_quant_persp(view, c2w, W, H, FX, opts))[1],
                      lambda opts: (keep, oops.octree_render_quant_rays(view, o, d, v, opts))[1]),
            "aux": (lambda opts: (keep, oops.octree_render_aux_persp(view, c2w, W, H, FX, opts))[1],
                    lambda opts: (keep, oops.octree_render_aux_rays(view, o, d, v, opts))[1])}


def measure(oops, dev):
    """{"<form>/<case>/lanes<L>/<exact|fast>/<persp|rays>": {"rgb": sha256[, "aux": sha256]}}."""
    renders = {}
    for kind, K in TREE_CASES:
        for form, fns in _tree_renders(oops, dev, kind, K).items():
            renders[f"{form}/{kind}{K}"] = fns
    for K, retain, bits in QUANT_CASES:
        for what, fns in _quant_renders(oops, dev, K, retain, bits).items():
            renders[f"quant/{what}_K{K}_r{retain}_b{bits}"] = fns
    options = {"exact": oops.render_opts(STEP), "fast": oops.render_opts(STEP, 1.0, 1e-2, 1e-2)}
    out = {}
    try:
        for lanes in LANES:
            oops.set_lanes_per_ray(lanes, 0)
            for name, (persp, rays) in renders.items():
                for oname, opts in options.items():
                    out[f"{name}/lanes{lanes}/{oname}/persp"] = _outputs(persp(opts))
                    out[f"{name}/lanes{lanes}/{oname}/rays"] = _outputs(rays(opts))
    finally:
        oops.set_lanes_per_ray(0, 0)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from plenoctree_amd import octree_ops as _oops
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(measure(_oops, torch.device("cuda:0")), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
