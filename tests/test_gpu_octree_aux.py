"""The octree renderer's extra outputs on the device (pxo_octree_render_aux_fwd / pxo_octree_render_quant_aux_fwd: alpha, depth,
surface distance) against the CPU restatement of their definitions, oracle/octree_oracle.py's composite.

Cases (tests/_octree_aux_cases.py): the shapes of test_gpu_octree.py::test_octree_render_matches_oracle -- depth-3 trees with a
third of their leaves empty, a 14 x 10 camera (exact options and the early-stopping preset), 25 explicit rays with background
0.5, origins inside the volume and one ray that misses -- for every SH format at the default lanes per ray and SH16 at 8 and 16.

Bounds.  alpha is the sum of the weights that rgb is a weighted sum of: the renderer's own bound against the oracle, atol 2e-5,
rtol 0.  depth is the same sum with the "colours" bounded by s_max (the largest sample distance of the case, from the helper)
instead of 1: atol 2e-5 s_max.  What float32 round-off alone does to the definitions, measured on the CPU for exactly these
inputs as float32 helper against float64 helper (tests/test_octree_aux_cpu.py asserts < 1e-6 / < 1e-6 s_max): at most 2.5e-7 for
alpha and 1.5e-7 s_max for depth over all 15 cases -- 80 and 130 times inside the bounds, so neither is widened.
surface is a choice of sample: rtol 1e-6 against the float32 helper, leaving out only rays whose float64 transmittance after the
chosen sample is within a relative 1e-4 of the threshold or where the two helpers already choose different samples (1 ray of
140 in the SH16 early-stop case, none elsewhere; the cap is 2 %).
"""
import os

import numpy as np
import pytest
import torch

import _octree_aux_cases as C
import _quant_cases as Q
from _helpers import _gpu, close
from oracle import octree_oracle as T

pytestmark = pytest.mark.gpu
f32 = np.float32


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _svox():
    from plenoctree_amd.octree import svox
    return svox


def _device_tree(t, dev):
    oops = _oops()
    child = torch.from_numpy(t.child).to(dev)
    data = torch.from_numpy(t.data).to(dev)
    return oops.tree_view(child, data, t.offset, t.invradius), (child, data)


def _render(oops, view, K, config, dev):
    """(rgb, aux, rgb of the renderer without the extra outputs), flattened to [n,3]."""
    cam, step, bg, fast = C.CONFIGS[config]
    thr = 1e-2 if fast else 0.0
    opts = oops.render_opts(step, bg, thr, thr)
    if cam is None:
        o, d = (torch.from_numpy(a).to(dev) for a in C.explicit_rays(K))
        rgb, aux = oops.octree_render_aux_rays(view, o, d, d, opts, C.SURFACE_THRESH)
        plain = oops.octree_render_rays(view, o, d, d, opts)
        assert rgb.shape == (25, 3) and aux.shape == (25, 3)
    else:
        c2w = torch.from_numpy(C.pose(*cam)).to(dev)
        rgb, aux = oops.octree_render_aux_persp(view, c2w, C.W, C.H, C.FX, opts, surface_thresh=C.SURFACE_THRESH)
        plain = oops.octree_render_persp(view, c2w, C.W, C.H, C.FX, opts)
        assert rgb.shape == (C.H, C.W, 3) and aux.shape == (C.H, C.W, 3)
    return rgb.reshape(-1, 3), aux.reshape(-1, 3), plain.reshape(-1, 3)


def _check_case(K, lanes, dev):
    oops = _oops()
    view, keep = _device_tree(C.tree(K), dev)
    for config, (cam, _, bg, fast) in C.CONFIGS.items():
        b32, b64 = C.reference(K, config)
        rgb, aux, plain = _render(oops, view, K, config, dev)
        what = f"SH{K} {config} lanes={lanes}"
        # 3. rgb is untouched
        assert torch.equal(rgb, plain), what
        got = aux.cpu().numpy()
        alpha, depth, surface = got.T
        print(f"{what}: max |alpha - helper| {np.abs(alpha - b32.aux[:, 0]).max():.3g} (bound 2e-5), max |depth - helper| / s_max "
              f"{np.abs(depth - b32.aux[:, 1]).max() / b32.s_max:.3g} (bound 2e-5), s_max {b32.s_max:.4g}")
        # 1. parity of alpha and depth
        assert alpha.max() > 0.5 and (alpha == 0).any(), what               # the view sees the tree, and some rays see nothing
        close(f"{what} alpha", aux[:, 0], torch.from_numpy(b32.aux[:, 0]), rtol=0, atol=2e-5)
        close(f"{what} depth", aux[:, 1], torch.from_numpy(b32.aux[:, 1]), rtol=0, atol=2e-5 * b32.s_max)
        if fast:
            assert b32.stopped.any() and (np.abs(alpha[b32.stopped] - 1.0) <= 2e-5).all(), what     # rays that stopped early
        else:
            assert not b32.stopped.any()
        # 2. surface distance
        left_out = T.surface_excluded(b32, b64, C.SURFACE_THRESH)
        assert left_out.mean() <= 0.02, what
        want = b32.aux[:, 2]
        inf = np.isinf(want)
        assert np.array_equal(np.isinf(surface[~left_out]), inf[~left_out]), what
        assert (surface[np.isinf(surface)] > 0).all() and not np.isnan(surface).any()
        cmp = ~left_out & ~inf
        assert cmp.sum() >= 20
        assert np.allclose(surface[cmp], want[cmp], rtol=1e-6, atol=0), (what, np.abs(surface[cmp] / want[cmp] - 1).max())
        assert (alpha[inf & ~left_out] <= 0.5 + 2e-5).all()                 # never crossed: at least half the light is left
        if cam is None:                                                    # the ray that misses: (0, 0, +inf), rgb = background
            assert not left_out[-1] and tuple(got[-1]) == (0.0, 0.0, np.inf)
            assert torch.equal(rgb[-1].cpu(), torch.full((3,), bg))


@pytest.mark.parametrize("K", C.KS)
def test_aux_matches_the_definitions(K):
    _check_case(K, "default", _gpu())


@pytest.mark.parametrize("lanes", [8, 16])
def test_aux_matches_the_definitions_at_every_lanes_per_ray(lanes):
    oops = _oops(); dev = _gpu()
    try:
        oops.set_lanes_per_ray(lanes, 0)
        _check_case(16, lanes, dev)
    finally:
        oops.set_lanes_per_ray(0, 0)


def test_aux_rejects_a_threshold_the_early_stop_could_pass():
    oops = _oops(); dev = _gpu()
    from plenoctree_amd import _lib
    view, keep = _device_tree(C.tree(4), dev)
    c2w = torch.from_numpy(C.pose(20.0, 30.0)).to(dev)
    for thresh in (1e-2, 5e-3, 1.0):
        with pytest.raises(_lib.PxoError, match="surface_thresh"):
            oops.octree_render_aux_persp(view, c2w, C.W, C.H, C.FX, oops.render_opts(1e-3, 1.0, 1e-2, 1e-2), surface_thresh=thresh)
    with pytest.raises(_lib.PxoError, match="PxoTree"):
        oops.octree_render_aux_persp(object(), c2w, C.W, C.H, C.FX, oops.render_opts(1e-3))


# ---- 4. compressed trees ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(16, 0, 8), (9, 1, 8)], ids=lambda k: "SH%d-retain%d-bits%d" % k)
def test_palette_form_gives_the_float_trees_aux(tmp_path, key):
    """aux depends on sigma and the geometry only, and the packed sigma is the file's float16 widened exactly -- the value the
    float tree of N3Tree.load carries: bit-equal aux from the two kernels, at every lanes-per-ray variant; rgb is that of the
    palette renderer without the extra outputs."""
    svox = _svox(); oops = _oops(); dev = _gpu()
    path = Q.case(*key).save(os.path.join(str(tmp_path), "tree.npz"))
    q, f = svox.N3Tree.load(path, map_location=dev, keep_quantized=True), svox.N3Tree.load(path, map_location=dev)
    qv, fv = q.quant_view(), f.view()
    W, H, FX = 13, 9, 12.0
    rs = np.random.RandomState(37)
    o = np.concatenate([rs.randn(20, 3) * 3.0, rs.rand(4, 3) * 0.5, [[9.0, 9.0, 9.0]]]).astype(f32)
    d = (np.asarray(Q.CENTER) - o + rs.randn(25, 3) * 0.4).astype(f32)
    d[-1] = [1.0, 0.0, 0.0]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = torch.from_numpy(o).to(dev), torch.from_numpy(d.astype(f32)).to(dev)
    stopped = 0
    try:
        for lanes in (0, 8, 16):
            oops.set_lanes_per_ray(lanes, 0)
            for (theta, phi), fast in (((20.0, 30.0), False), ((250.0, -5.0), True)):
                thr = 1e-2 if fast else 0.0
                opts = oops.render_opts(1e-3, 1.0, thr, thr)
                c2w = torch.from_numpy(C.pose(theta, phi)).to(dev)
                rgb_q, aux_q = oops.octree_render_aux_persp(qv, c2w, W, H, FX, opts)
                _, aux_f = oops.octree_render_aux_persp(fv, c2w, W, H, FX, opts)
                assert torch.equal(aux_q, aux_f), (lanes, fast)
                assert torch.equal(rgb_q, oops.octree_render_quant_persp(qv, c2w, W, H, FX, opts))
                alpha = aux_q[..., 0]
                assert float(alpha.max()) > 0.5 and bool((alpha == 0).any()) and bool(torch.isfinite(aux_q[..., 2]).any())
                if fast:
                    stopped += int(((alpha - 1.0).abs() <= 2e-5).sum())
                ray_q, raux_q = oops.octree_render_aux_rays(qv, o, d, d, opts, 0.25)
                _, raux_f = oops.octree_render_aux_rays(fv, o, d, d, opts, 0.25)
                assert torch.equal(raux_q, raux_f) and torch.equal(ray_q, oops.octree_render_quant_rays(qv, o, d, d, opts))
                assert tuple(raux_q[-1].tolist()) == (0.0, 0.0, float("inf"))
    finally:
        oops.set_lanes_per_ray(0, 0)
    assert stopped > 0


# ---- 5. the svox surface ------------------------------------------------------------------------------------------------
def test_svox_render_persp_aux_on_device(tmp_path):
    svox = _svox(); oops = _oops(); dev = _gpu()
    from plenoctree_amd import _lib
    K = 4
    t = C.tree(K)
    path = os.path.join(str(tmp_path), "tree.npz")
    np.savez(path, data_dim=np.int64(3 * K + 1), child=t.child, parent_depth=t.parent_depth, invradius3=t.invradius,
             offset=t.offset, data_format=f"SH{K}", data=t.data)
    tree = svox.N3Tree.load(path, map_location=dev)
    r = svox.VolumeRenderer(tree, step_size=1e-3)
    c2w = C.pose(20.0, 30.0)
    assert tree.data.requires_grad and torch.is_grad_enabled()
    with pytest.raises(_lib.PxoError, match="not differentiable"):
        r.render_persp_aux(c2w, width=C.W, height=C.H, fx=C.FX)
    o, d = (torch.from_numpy(a).to(dev) for a in C.explicit_rays(K))
    with pytest.raises(_lib.PxoError, match="not differentiable"):
        r.forward_aux(o, d, d)
    with torch.no_grad():
        res = r.render_persp_aux(c2w, width=C.W, height=C.H, fx=C.FX)
        plain = r.render_persp(c2w, width=C.W, height=C.H, fx=C.FX)
        rays = r.forward_aux(o, d, d, fast=True, surface_thresh=0.3)
    assert sorted(res) == ["alpha", "depth", "rgb", "surface"]
    assert res["rgb"].shape == (C.H, C.W, 3) and all(res[k].shape == (C.H, C.W) for k in ("alpha", "depth", "surface"))
    assert torch.equal(res["rgb"], plain)
    b32, _ = C.reference(K, "exact")
    close("svox alpha", res["alpha"], torch.from_numpy(b32.aux[:, 0]), rtol=0, atol=2e-5)
    assert rays["rgb"].shape == (25, 3) and all(rays[k].shape == (25,) for k in ("alpha", "depth", "surface"))
    tree.data.requires_grad_(False)                                         # nothing to differentiate: grad mode may stay on
    again = r.render_persp_aux(c2w, width=C.W, height=C.H, fx=C.FX)
    assert all(torch.equal(again[k], res[k]) for k in res)


# ---- 6. the command line ------------------------------------------------------------------------------------------------
def test_evaluation_writes_aux_files_and_points(tmp_path, monkeypatch):
    """octree.evaluation --write_aux / --write_points on 4 views of the synthetic scene (factor 16: 50 x 50 pixels) and a
    depth-3 tree: files for every view, the PNG's alpha is the archive's quantised, every vertex lies inside the tree's
    bounding box (a sample's middle can lie half a renderer step outside it), and the PSNR is that of the run without."""
    _gpu()
    from PIL import Image
    from plenoctree_amd.octree import aux_io, evaluation
    c = Q.case(16, 4, 16)
    path = c.save(os.path.join(str(tmp_path), "tree_min.npz"))
    cfg_path = os.path.join(str(tmp_path), "tiny.yaml")
    with open(cfg_path, "w") as fh:
        fh.write("dataset: synthetic\nfactor: 16\nnum_coarse_samples: 64\nnum_fine_samples: 128\nuse_viewdirs: false\n"
                 "white_bkgd: true\nbatch_size: 1024\nsh_deg: 3\nrandomized: true\n")
    step = 1e-3
    common = ["--train_dir", str(tmp_path), "--config", cfg_path, "--synthetic_views", "4", "4", "--renderer_step_size", str(step),
              "--input", path]
    out_dir, ply = os.path.join(str(tmp_path), "aux"), os.path.join(str(tmp_path), "points.ply")
    svox = _svox()
    images = {"render_persp": [], "render_persp_aux": []}
    for name in images:
        def recording(self, *a, _plain=getattr(svox.VolumeRenderer, name), _into=images[name], **k):
            res = _plain(self, *a, **k)
            _into.append((res["rgb"] if isinstance(res, dict) else res).detach().cpu())
            return res
        monkeypatch.setattr(svox.VolumeRenderer, name, recording)
    psnr = evaluation.main(common)
    assert not os.path.exists(out_dir) and not os.path.exists(ply)
    assert (len(images["render_persp"]), len(images["render_persp_aux"])) == (4, 0)       # without the flags: today's entry point
    psnr_aux = evaluation.main(common + ["--write_aux", out_dir, "--write_points", ply, "--points_stride", "3"])
    assert (len(images["render_persp"]), len(images["render_persp_aux"])) == (4, 4)
    assert all(torch.equal(a, b) for a, b in zip(images["render_persp"], images["render_persp_aux"]))     # the same rgb ...
    # ... hence the same PSNR, up to the order of the float32 atomic sum of the 7500 squared errors of a view (pxo_image_mse):
    # relative 7500 x 2^-24 = 4.5e-4 of the mse at the very worst, 2e-3 dB
    assert abs(psnr_aux - psnr) < 2e-3 and np.isfinite(psnr)
    n_points = 0
    for idx in range(4):
        png, npz = os.path.join(out_dir, f"{idx:03d}_rgba.png"), os.path.join(out_dir, f"{idx:03d}_depth.npz")
        assert os.path.exists(png) and os.path.exists(npz), idx
        z = np.load(npz)
        im = np.asarray(Image.open(png))
        assert im.shape == z["alpha"].shape + (4,) and all(z[k].dtype == np.float32 for k in ("alpha", "depth", "surface"))
        assert np.array_equal(im[..., 3], np.rint(255.0 * np.clip(z["alpha"], 0, 1)).astype(np.uint8))
        assert z["alpha"].max() > 0.5                                      # (the tree fills these views: no pixel misses it)
        # the surface is reached exactly where half the light is gone (alpha = 1 - light up to round-off)
        assert (np.isfinite(z["surface"]) != (z["alpha"] >= 0.5)).mean() < 0.01
        n_points += int(np.isfinite(z["surface"][::3, ::3]).sum())
    xyz, col = C.read_ply(ply)
    assert xyz.shape == (n_points, 3) and n_points > 50 and col.shape == (n_points, 3)
    radius, center = np.asarray(Q.RADIUS), np.asarray(Q.CENTER)
    slack = step * 2.0 * radius                                             # one renderer step (tree units) in world units, per axis
    assert (np.abs(xyz - center) <= radius + slack).all()
