"""Trees rendered in place from the float16 of their files (pxo_octree_render_half_fwd / _aux_fwd, HalfN3Tree).

Bars.  (1) The pack kernel's buffer is the documented layout byte for byte.  (2) torch.equal with the float renderer on
`N3Tree.load(path)` of the same file: widening float16 to float32 is exact and the half instantiations own the same logical
coefficients per lane and add them in the same order, so there is no tolerance.  (3) Independently of the float kernel: the
CPU oracles on the widened data at the float renderer's own bar, atol 2e-5, rtol 0 (tests/test_gpu_octree.py,
tests/test_gpu_sg.py); background pixels and rays equal the background exactly.

Cases (tests/_half_cases.py): the depth 3..5 trees of tests/_octree_sg_cases.py as SH and as SG at K = 1, 4, 9, 16, 25, a
16 x 12 camera (no multiple of any lane variant's patch, 11 % of the pixels miss), 37 aimed rays with unrelated view
directions plus the 13 edge rays, exact and early-stop presets, lanes 0 (default), 4, 8, 16 with both renderers at the same
setting; one NDC case built as tests/test_gpu_octree_ndc.py builds its own; the aux configurations of
tests/_octree_aux_cases.py.  Each file is written with N3Tree.save and loaded twice.
"""
import os

import numpy as np
import pytest
import torch

import _half_cases as H
import _octree_aux_cases as A
import _octree_ndc_oracle as N
import _octree_sg_cases as G
from oracle import octree_oracle as T
from _helpers import _gpu, close

pytestmark = pytest.mark.gpu
f32 = np.float32


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _svox():
    from plenoctree_amd.octree import svox
    return svox


def _load_both(tmp_path, t, fmt, lobes=None):
    svox = _svox(); dev = _gpu()
    path = H.save(os.path.join(str(tmp_path), "tree.npz"), t, fmt, lobes)
    h, f = svox.N3Tree.load(path, map_location=dev, keep_half=True), svox.N3Tree.load(path, map_location=dev)
    assert isinstance(h, svox.HalfN3Tree) and isinstance(f, svox.N3Tree) and h.device.type == "cuda"
    return h, f


@pytest.mark.parametrize("K", H.KS)
def test_pack_kernel_writes_the_documented_layout(K):
    """n_internal smaller than the file's row count: the rows behind it are not read; zero padding included."""
    oops = _oops(); dev = _gpu()
    t = G.tree(K)
    D = 3 * K + 1
    data16 = t.data.astype(np.float16)
    n = t.n_internal - 3
    src = torch.from_numpy(data16).to(dev)
    packed, stride = oops.half_pack(src[:n], n)
    want, s = H.packed_layout(data16, n, D)
    assert stride == s == H.ROW_STRIDE[K] and packed.shape == (n * 8, stride) and packed.dtype == torch.float16
    got = packed.cpu().numpy()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    assert stride == D or (got[:, D:] == 0).all()
    assert np.abs(want[:, :D].astype(f32)).max() > 1.0
    with pytest.raises(oops.PxoError):
        oops.half_pack(src[:n].float(), n)
    with pytest.raises(oops.PxoError):
        oops.half_pack(src[:n], n + 1)


def _render_pair(rh, rf, c2w, o, d, v, fast):
    V = H.VIEW
    with torch.no_grad():
        img_f = rf.render_persp(c2w, width=V["W"], height=V["H"], fx=V["fx"], fast=fast)
        ray_f = rf.forward(o, d, v, fast=fast)
    img_h = rh.render_persp(c2w, width=V["W"], height=V["H"], fx=V["fx"], fast=fast)       # grad mode on: nothing requires grad
    ray_h = rh.forward(o, d, v, fast=fast)
    assert img_h.shape == (V["H"], V["W"], 3) and not img_h.requires_grad and not ray_h.requires_grad
    return img_h, ray_h, img_f, ray_f


@pytest.mark.parametrize("K", H.KS)
@pytest.mark.parametrize("kind", ["SH", "SG"])
def test_half_render_is_the_float_render_and_matches_the_oracle(tmp_path, kind, K):
    svox = _svox(); oops = _oops(); dev = _gpu()
    t = G.tree(K)
    assert (t.data[..., -1] <= 0).any() and len(set(t.parent_depth[:, 1].tolist())) >= 3      # sigma-0 leaves, mixed depths
    h, f = _load_both(tmp_path, t, f"{kind}{K}", G.lobes(K) if kind == "SG" else None)
    assert torch.equal(h.to_float().data.data, f.data.data)
    rh, rf = svox.VolumeRenderer(h, step_size=H.STEP), svox.VolumeRenderer(f, step_size=H.STEP)
    c2w = torch.from_numpy(H.VIEW["c2w"])
    o, d, v, miss = H.rays(K)
    o, d, v = (torch.from_numpy(a).to(dev) for a in (o, d, v))
    try:
        for fast in (False, True):
            want_img, want_ray = (torch.from_numpy(a) for a in H.want(kind, K, fast))
            bg = (want_img == 1.0).all(-1)
            assert float((want_img - 1.0).abs().max()) > 0.2 and bg.any()     # the view sees the tree, some pixels miss it
            for lanes in H.LANES:
                oops.set_lanes_per_ray(lanes, 0)
                img_h, ray_h, img_f, ray_f = _render_pair(rh, rf, c2w, o, d, v, fast)
                what = f"{kind}{K} fast={fast} lanes={lanes}"
                e_img, e_ray = float((img_h.cpu() - want_img).abs().max()), float((ray_h.cpu() - want_ray).abs().max())
                d_img, d_ray = float((img_h - img_f).abs().max()), float((ray_h - ray_f).abs().max())
                print(f"{what}: max |half - float kernel| image {d_img:.3g} rays {d_ray:.3g}; max |half - oracle| image "
                      f"{e_img:.3g} rays {e_ray:.3g} (bound 2e-5)")
                # 2. bit identity with the float renderer
                assert torch.equal(img_h, img_f), what
                assert torch.equal(ray_h, ray_f), what
                # 3. independent of the float kernel
                close(f"{what} image against the oracle", img_h, want_img, rtol=0, atol=2e-5)
                close(f"{what} rays against the oracle", ray_h, want_ray, rtol=0, atol=2e-5)
                assert torch.equal(img_h.cpu()[bg], torch.ones(int(bg.sum()), 3)), what
                assert torch.equal(ray_h.cpu()[miss], torch.ones(len(miss), 3)) and bool((want_ray[miss] == 1.0).all()), what
    finally:
        oops.set_lanes_per_ray(0, 0)
    if kind == "SG":
        # the lobes are used: the same data shaded with the SH basis is another image
        sh = oops.octree_render_half_persp(h.half_view(), c2w.to(dev), H.VIEW["W"], H.VIEW["H"], H.VIEW["fx"],
                                           oops.render_opts(H.STEP))
        if K > 1:
            assert float((sh - img_h).abs().max()) > 1e-2


def test_half_render_ndc(tmp_path):
    """An SH16 tree in the second NDC box, camera B (some pixels miss): VolumeRenderer(ndc=...) on the half tree equals the
    float tree bit for bit at every lane count and the composed NDC oracle on the widened data to 2e-5."""
    svox = _svox(); oops = _oops(); dev = _gpu()
    K = 16
    t = N.box_tree(K, 1)
    h, f = _load_both(tmp_path, t, f"SH{K}")
    w = H.widened(t)
    ndc = svox.NDCConfig(N.W, N.H, N.FX)
    rh, rf = svox.VolumeRenderer(h, step_size=1e-3, ndc=ndc), svox.VolumeRenderer(f, step_size=1e-3, ndc=ndc)
    c2w = torch.from_numpy(N.camera_b())
    co, cd = T.camera_rays(N.camera_b(), N.W, N.H, N.FX)
    rs = np.random.RandomState(5)
    cv = rs.randn(*cd.shape)
    cv = (cv / np.linalg.norm(cv, axis=1, keepdims=True)).astype(f32)
    o, d, v = (torch.from_numpy(np.ascontiguousarray(a[:37], dtype=f32)).to(dev) for a in (co[50:], cd[50:], cv))
    try:
        for fast in (False, True):
            opt = T.RenderOptions.for_renderer(1e-3, fast)
            want = torch.from_numpy(T.render_persp(w, N.camera_b(), N.W, N.H, N.FX, opt, ndc=N.Ndc()))
            want_r = torch.from_numpy(T.render_rays(w, co[50:87], cd[50:87], cv[:37], opt, ndc=N.Ndc()))
            bg = (want == 1.0).all(-1)
            assert float((want - 1.0).abs().max()) > 0.5 and bg.any()
            for lanes in H.LANES:
                oops.set_lanes_per_ray(lanes, 0)
                with torch.no_grad():
                    img_f = rf.render_persp(c2w, width=N.W, height=N.H, fx=N.FX, fast=fast)
                    ray_f = rf.forward(o, d, v, fast=fast)
                img_h = rh.render_persp(c2w, width=N.W, height=N.H, fx=N.FX, fast=fast)
                ray_h = rh.forward(o, d, v, fast=fast)
                what = f"NDC SH{K} fast={fast} lanes={lanes}"
                print(f"{what}: max |half - oracle| image {float((img_h.cpu() - want).abs().max()):.3g} rays "
                      f"{float((ray_h.cpu() - want_r).abs().max()):.3g} (bound 2e-5)")
                assert torch.equal(img_h, img_f) and torch.equal(ray_h, ray_f), what
                close(f"{what} image against the oracle", img_h, want, rtol=0, atol=2e-5)
                close(f"{what} rays against the oracle", ray_h, want_r, rtol=0, atol=2e-5)
                assert torch.equal(img_h.cpu()[bg], torch.ones(int(bg.sum()), 3)), what
    finally:
        oops.set_lanes_per_ray(0, 0)
    world = svox.VolumeRenderer(h, step_size=1e-3).render_persp(c2w, width=N.W, height=N.H, fx=N.FX)
    assert float((world - img_h).abs().max()) > 0.1                            # and it is not the world-space image


@pytest.mark.parametrize("K", H.KS)
def test_half_aux_is_the_float_aux(tmp_path, K):
    svox = _svox(); oops = _oops(); dev = _gpu()
    h, f = _load_both(tmp_path, A.tree(K), f"SH{K}")
    try:
        for lanes in H.LANES if K == 16 else (0,):
            oops.set_lanes_per_ray(lanes, 0)
            for config, (cam, step, bg, fast) in A.CONFIGS.items():
                rh = svox.VolumeRenderer(h, step_size=step, background_brightness=bg)
                rf = svox.VolumeRenderer(f, step_size=step, background_brightness=bg)
                if cam is None:
                    o, d = (torch.from_numpy(a).to(dev) for a in A.explicit_rays(K))
                    got = rh.forward_aux(o, d, d, fast=fast, surface_thresh=A.SURFACE_THRESH)
                    with torch.no_grad():
                        ref = rf.forward_aux(o, d, d, fast=fast, surface_thresh=A.SURFACE_THRESH)
                        plain = rh.forward(o, d, d, fast=fast)
                else:
                    c2w = torch.from_numpy(A.pose(*cam))
                    kw = dict(width=A.W, height=A.H, fx=A.FX, fast=fast)
                    got = rh.render_persp_aux(c2w, surface_thresh=A.SURFACE_THRESH, **kw)
                    with torch.no_grad():
                        ref = rf.render_persp_aux(c2w, surface_thresh=A.SURFACE_THRESH, **kw)
                        plain = rh.render_persp(c2w, **kw)
                what = f"SH{K} {config} lanes={lanes}"
                for k in ("rgb", "alpha", "depth", "surface"):
                    assert torch.equal(got[k], ref[k]), f"{what} {k}"           # +inf == +inf: the entries without a surface too
                assert torch.equal(got["rgb"], plain), what
                assert bool(torch.isinf(got["surface"]).any()) and bool(torch.isfinite(got["surface"]).any()), what
                assert float(got["alpha"].max()) > 0.5 and bool((got["alpha"] == 0).any()), what
    finally:
        oops.set_lanes_per_ray(0, 0)


def test_half_refusals_are_the_float_trees(tmp_path):
    svox = _svox(); oops = _oops(); dev = _gpu()
    K = 9
    V = H.VIEW
    c2w = torch.from_numpy(V["c2w"])
    sub = tmp_path / "sg"; sub.mkdir()
    hs, fs = _load_both(sub, G.tree(K), f"SG{K}", G.lobes(K))
    hh, fh = _load_both(tmp_path, A.tree(K), f"SH{K}")
    ndc = svox.NDCConfig(V["W"], V["H"], V["fx"])

    def message(fn):
        with pytest.raises(NotImplementedError) as e:
            fn()
        return str(e.value)

    kw = dict(width=V["W"], height=V["H"], fx=V["fx"])
    o, d = (torch.from_numpy(a).to(dev) for a in A.explicit_rays(K))
    with torch.no_grad():
        # aux on an SG tree, aux with NDC, SG with NDC: the float tree's words
        for half, flt in ((hs, fs),):
            assert message(lambda: svox.VolumeRenderer(half).render_persp_aux(c2w, **kw)) == \
                message(lambda: svox.VolumeRenderer(flt).render_persp_aux(c2w, **kw))
            assert message(lambda: svox.VolumeRenderer(half).forward_aux(o, d, d)) == \
                message(lambda: svox.VolumeRenderer(flt).forward_aux(o, d, d))
            assert message(lambda: svox.VolumeRenderer(half, ndc=ndc)) == message(lambda: svox.VolumeRenderer(flt, ndc=ndc))
        assert message(lambda: svox.VolumeRenderer(hh, ndc=ndc).render_persp_aux(c2w, **kw)) == \
            message(lambda: svox.VolumeRenderer(fh, ndc=ndc).render_persp_aux(c2w, **kw))
        assert "SG" in message(lambda: svox.VolumeRenderer(hs).render_persp_aux(c2w, **kw))
        assert "NDC" in message(lambda: svox.VolumeRenderer(hh, ndc=ndc).forward_aux(o, d, d))
    # the C entry point: lobes together with ndc, a wrong stride, a misaligned buffer
    view = hs.half_view()
    with pytest.raises(NotImplementedError, match="NDC rendering of an SG tree"):
        oops.octree_render_half_persp(view, c2w.to(dev), V["W"], V["H"], V["fx"], oops.render_opts(1e-3), lobes=hs.extra_data,
                                      ndc=oops.ndc_spec(V["W"], V["H"], V["fx"]))
    view.row_stride += 4
    with pytest.raises(oops.PxoError, match="row_stride"):
        oops.octree_render_half_persp(view, c2w.to(dev), V["W"], V["H"], V["fx"], oops.render_opts(1e-3), lobes=hs.extra_data)
    view = hs.half_view()
    view.data += 2
    with pytest.raises(oops.PxoError, match="8-byte aligned"):
        oops.octree_render_half_persp(view, c2w.to(dev), V["W"], V["H"], V["fx"], oops.render_opts(1e-3), lobes=hs.extra_data)
    with pytest.raises(oops.PxoError, match="null lobes|SG|lobes"):
        oops.octree_render_half_persp(hs.half_view(), c2w.to(dev), V["W"], V["H"], V["fx"], oops.render_opts(1e-3),
                                      lobes=torch.zeros(K + 1, 4, device=dev))


def test_evaluation_keep_half(tmp_path, capsys, monkeypatch):
    """octree.evaluation on 4 views of the synthetic scene, with and without --keep_half: the same PSNR, the same rendered
    images bit for bit and the same written frames byte for byte (SH with --write_aux, SG for rgb); the size line is printed;
    a compressed file is refused.

    25 x 25 views (factor 32): 1875 values per image are ONE workgroup of pxo_image_mse, so the squared error the PSNR comes
    from is summed in a fixed order.  Larger images take several workgroups, which add their partial sums with float atomics
    in whatever order they finish: at 50 x 50 six runs on the SAME float tree gave 7.220636101 dB five times and 7.220636187
    dB once, with identical images in all six (profiles/EXPERIMENTS.md); at 25 x 25 every run gives the same digits."""
    svox = _svox(); _gpu()
    from plenoctree_amd.octree import evaluation
    import _quant_cases as Q
    cfg_path = os.path.join(str(tmp_path), "tiny.yaml")
    with open(cfg_path, "w") as fh:
        fh.write("dataset: synthetic\nfactor: 32\nnum_coarse_samples: 64\nnum_fine_samples: 128\nuse_viewdirs: false\n"
                 "white_bkgd: true\nbatch_size: 1024\nsh_deg: 3\nrandomized: true\n")
    common = ["--train_dir", str(tmp_path), "--config", cfg_path, "--synthetic_views", "4", "4", "--renderer_step_size", "1e-3"]
    images = []
    plain, plain_aux = svox.VolumeRenderer.render_persp, svox.VolumeRenderer.render_persp_aux

    def recording(self, *a, **k):
        im = plain(self, *a, **k)
        images.append((type(self.tree).__name__, im.detach().cpu()))
        return im

    def recording_aux(self, *a, **k):
        res = plain_aux(self, *a, **k)
        images.append((type(self.tree).__name__, torch.cat([res["rgb"], res["alpha"][..., None], res["depth"][..., None],
                                                            res["surface"][..., None]], -1).cpu()))
        return res

    monkeypatch.setattr(svox.VolumeRenderer, "render_persp", recording)
    monkeypatch.setattr(svox.VolumeRenderer, "render_persp_aux", recording_aux)

    def files(d):
        return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}

    K = 16
    for kind, t, lobes, aux in (("SH", Q.case(K, 4, 16).tree, None, True), ("SG", Q.case(K, 0, 8).tree, G.lobes(K), False)):
        path = H.save(os.path.join(str(tmp_path), f"tree_{kind}.npz"), t, f"{kind}{K}", lobes)
        out = {}
        del images[:]
        for flag in ((), ("--keep_half",)):
            tag = kind + ("_half" if flag else "_float")
            dirs = [os.path.join(str(tmp_path), f"{tag}_{w}") for w in ("images", "aux")]
            argv = common + ["--input", path, "--write_images", dirs[0]] + (["--write_aux", dirs[1]] if aux else []) + list(flag)
            psnr = evaluation.main(argv)
            out[bool(flag)] = (psnr, files(dirs[0]), files(dirs[1]) if aux else {}, capsys.readouterr().out)
        (p_f, im_f, aux_f, txt_f), (p_h, im_h, aux_h, txt_h) = out[False], out[True]
        print(f"{kind}{K}: PSNR float {p_f!r} dB, kept in float16 {p_h!r} dB")
        assert np.isfinite(p_f) and p_f == p_h
        assert [t for t, _ in images] == ["N3Tree"] * 4 + ["HalfN3Tree"] * 4
        for (_, a), (_, b) in zip(images[:4], images[4:]):
            assert float((a[..., :3] - 1.0).abs().max()) > 0.2 and torch.equal(a, b)
        assert len(im_f) == 4 and im_f == im_h and aux_f == aux_h and (len(aux_f) == 8) == aux
        h = svox.N3Tree.load(path, keep_half=True)
        line = f"float16 tree kept in place: {h.nbytes / 2 ** 20:.1f} MB on the device (float form: {h.float_nbytes / 2 ** 20:.1f} MB)"
        assert line in txt_h and "kept in place" not in txt_f
    comp = Q.case(K, 4, 16).save(os.path.join(str(tmp_path), "compressed.npz"))
    with pytest.raises(ValueError, match="keep_half"):
        evaluation.main(common + ["--input", comp, "--keep_half"])
