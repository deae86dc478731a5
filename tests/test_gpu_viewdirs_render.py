"""Ray rendering with the view-conditioned head on the GPU (pxo_vd_render_fwd, pxo_vd_composite_fwd, ViewdirsModel.apply and the
--use_viewdirs true branch of nerf_sh.eval / gen_video).  Accuracy bounds are the project's R1 bounds for rendered quantities
(tests/test_gpu_reference_fixtures.py): rgb and acc atol 2e-5, disp rtol 2e-3 + atol 1e-6, against the reference's own run
(tests/golden/viewdirs_render.npz) and against the float64 restatement; everything else is bit equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _viewdirs_render_helpers import (Rays, check_level, fixture, fixture_rays, fixture_state_dict, host_render_f64, render_cfg)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from plenoctree_amd import ops
    from plenoctree_amd.nerf_sh.nerf import checkpoints, viewdirs
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    fx = fixture()
    sd = fixture_state_dict(fx)
    flat = checkpoints.vd_tree_to_arena(checkpoints.vd_torch_state_dict_to_tree(sd))
    state = viewdirs.ViewdirsState(torch.from_numpy(flat).to(dev))
    return dict(ops=ops, viewdirs=viewdirs, dev=dev, fx=fx, sd=sd, state=state)


def _rays(n, seed, dev=None, norms=(0.5, 1.0, 1.5)):
    """n rays from cameras on a sphere of radius 4 towards the origin, |directions| cycling through `norms`."""
    g = torch.Generator().manual_seed(seed)
    cam = torch.randn(n, 3, generator=g)
    cam = 4 * cam / cam.norm(dim=-1, keepdim=True)
    v = -cam / 4 + 0.08 * torch.randn(n, 3, generator=g)
    v = v / v.norm(dim=-1, keepdim=True)
    d = v * torch.tensor([norms[i % len(norms)] for i in range(n)])[:, None]
    r = Rays(cam.contiguous(), d.contiguous(), v.contiguous())
    return r if dev is None else Rays(*[x.to(dev) for x in r])


def _model(ctx, nc=64, nf=128, **kw):
    return ctx["viewdirs"].ViewdirsModel(nc, nf, **kw)


def _equal(a, b):
    return all(torch.equal(x, y) for la, lb in zip(a, b) for x, y in zip(la, lb)) and len(a) == len(b)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("randomized", [0, 1])
def test_fixture_parity(ctx, randomized):
    fx, dev = ctx["fx"], ctx["dev"]
    rays = Rays(*[x.to(dev) for x in fixture_rays(fx)])
    t_rand = torch.from_numpy(fx["t_rand"]).to(dev) if randomized else None
    u = torch.from_numpy(fx["u"]).to(dev) if randomized else None
    out = _model(ctx).apply(ctx["state"], rays, bool(randomized), t_rand=t_rand, u=u)
    assert len(out) == 2
    for lvl, got in zip(("coarse", "fine"), out):
        check_level(f"HIP vs reference f32, {lvl} r{randomized}", got,
                    tuple(fx[f"{q}_{lvl}_r{randomized}"] for q in ("rgb", "disp", "acc")))


@pytest.mark.timeout(60)
@pytest.mark.parametrize("nc,nf,B,white,lindisp", [(12, 20, 7, True, False), (40, 60, 5, True, False), (64, 0, 3, True, False),
                                                   (12, 20, 1, True, False), (12, 20, 7, False, False), (12, 20, 7, True, True)])
def test_odd_shapes_against_the_float64_restatement(ctx, nc, nf, B, white, lindisp):
    """(12,20) x 7: M = 84 and 224 rows are no multiples of 16 x S, so head groups straddle rays, and S = 32 is a partial chunk;
    (40,60): one full + one partial chunk; (64,0): coarse only (fine pointers NULL); B = 1; black background; lindisp."""
    dev = ctx["dev"]
    rays = _rays(B, 100 + B + nc)
    g = torch.Generator().manual_seed(7)
    t_rand, u = torch.rand(B, nc, generator=g), torch.rand(B, max(nf, 1), generator=g)[:, :nf].contiguous()
    model = _model(ctx, nc, nf, white_bkgd=white, lindisp=lindisp)
    for r in (0, 1):
        out = model.apply(ctx["state"], Rays(*[x.to(dev) for x in rays]), bool(r), t_rand=t_rand.to(dev) if r else None,
                          u=u.to(dev) if (r and nf) else None)
        want = host_render_f64(ctx["sd"], rays, render_cfg(nc, nf, white_bkgd=white, lindisp=lindisp), t_rand if r else None,
                               u if (r and nf) else None)
        assert len(out) == len(want) == (2 if nf else 1)
        for lvl, got, w in zip(("coarse", "fine"), out, want):
            check_level(f"({nc},{nf}) B={B} white={white} lindisp={lindisp} {lvl} r{r}", got, w)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("nc,nf,B", [(12, 20, 7), (64, 128, 5)])
def test_whole_path_equals_its_public_pieces_bit_for_bit(ctx, nc, nf, B):
    ops, dev, st = ctx["ops"], ctx["dev"], ctx["state"]
    rays = _rays(B, 300 + B, dev)
    g = torch.Generator().manual_seed(8)
    t_rand, u = torch.rand(B, nc, generator=g).to(dev), torch.rand(B, nf, generator=g).to(dev)
    model = _model(ctx, nc, nf)
    for r in (0, 1):
        whole = model.apply(st, rays, bool(r), t_rand=t_rand if r else None, u=u if r else None)
        z, pts = ops.sample_along_rays(rays.origins, rays.directions, nc, 2.0, 6.0, t_rand if r else None)
        pieces = []
        for lvl, S in ((0, nc), (1, nc + nf)):
            vd = rays.viewdirs[:, None, :].expand(B, S, 3).reshape(-1, 3).contiguous()
            raw_rgb, raw_sigma = ops.vd_eval_points_raw(st.packed[lvl][0], pts.reshape(-1, 3), vd)
            comp, disp, acc, w = ops.vd_composite_fwd(model.cfg, raw_rgb, raw_sigma, z, rays.directions)
            pieces.append((comp, disp, acc))
            if lvl == 0:
                z, pts = ops.sample_pdf(z, w, rays.origins, rays.directions, nf, u if r else None)
        assert _equal(whole, pieces), (nc, nf, B, r)


@pytest.mark.timeout(60)
def test_block_and_chunk_invariance_bit_for_bit(ctx):
    ops, dev, st = ctx["ops"], ctx["dev"], ctx["state"]
    rays = _rays(23, 400, dev)
    model = _model(ctx, 12, 20)
    default = ops.get_tuning(ops.TUNE_VD_RAY_BLOCK)
    assert default == 1024
    want = model.apply(st, rays, False)
    want_r = model.apply(st, rays, True, seed=5)                      # draws from the Philox streams of the whole batch
    try:
        ops.set_tuning(ops.TUNE_VD_RAY_BLOCK, 8)                      # blocks of 8, 8, 7 rays
        assert ops.get_tuning(ops.TUNE_VD_RAY_BLOCK) == 8
        assert _equal(model.apply(st, rays, False), want)
        assert _equal(model.apply(st, rays, True, seed=5), want_r)
    finally:
        ops.set_tuning(ops.TUNE_VD_RAY_BLOCK, default)
    parts = [model.apply(st, Rays(*[x[a:b].contiguous() for x in rays]), False) for a, b in ((0, 7), (7, 23))]
    glued = [tuple(torch.cat([p[lvl][q] for p in parts]) for q in range(3)) for lvl in range(2)]
    assert _equal(glued, want)


@pytest.mark.timeout(60)
def test_noise(ctx):
    ops, dev, st = ctx["ops"], ctx["dev"], ctx["state"]
    rays = _rays(23, 500, dev)
    g = torch.Generator().manual_seed(9)
    t_rand, u = torch.rand(23, 13, generator=g).to(dev), torch.rand(23, 20, generator=g).to(dev)
    plain, noisy = _model(ctx, 13, 20), _model(ctx, 13, 20, noise_std=0.3)     # 13 and 33 samples: blocks start inside a Philox quad
    a = noisy.apply(st, rays, True, t_rand=t_rand, u=u, seed=11)
    assert _equal(a, noisy.apply(st, rays, True, t_rand=t_rand, u=u, seed=11))           # deterministic per seed
    assert not torch.equal(a[1][0], noisy.apply(st, rays, True, t_rand=t_rand, u=u, seed=12)[1][0])
    ref = plain.apply(st, rays, True, t_rand=t_rand, u=u, seed=11)
    assert not torch.equal(a[0][0], ref[0][0]) and not torch.equal(a[1][0], ref[1][0])   # differs from the noise-free render
    assert all(bool(torch.isfinite(x).all()) for lvl in a for x in lvl)
    assert _equal(noisy.apply(st, rays, False), plain.apply(st, rays, False))            # untouched when randomized = 0
    default = ops.get_tuning(ops.TUNE_VD_RAY_BLOCK)
    try:                                                                                  # a sample's draw does not depend on the block
        ops.set_tuning(ops.TUNE_VD_RAY_BLOCK, 5)
        assert _equal(noisy.apply(st, rays, True, t_rand=t_rand, u=u, seed=11), a)
    finally:
        ops.set_tuning(ops.TUNE_VD_RAY_BLOCK, default)


@pytest.mark.timeout(60)
def test_error_paths(ctx):
    from plenoctree_amd import _lib
    lib = _lib.load()
    ops, dev, st = ctx["ops"], ctx["dev"], ctx["state"]
    rays = _rays(4, 600, dev)
    for prec in (_lib.MLP_BF16X3, _lib.MLP_BF16X6):
        with pytest.raises(_lib.PxoError, match=r"\(-4\)"):
            _model(ctx, 12, 20, mlp_precision=prec).apply(st, rays, False)
    cfg = ops.make_cfg(num_coarse_samples=12, num_fine_samples=20, sh_deg=0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rgb, disp, acc = (torch.empty(4, 3, device=dev), torch.empty(4, device=dev), torch.empty(4, device=dev))
    rgb2, disp2, acc2 = torch.empty_like(rgb), torch.empty_like(disp), torch.empty_like(acc)
    ws = torch.empty(max(ops.vd_render_workspace_bytes(cfg, 4), 16), dtype=torch.uint8, device=dev)

    def call(packed1, ws_bytes, B=4):
        return lib.pxo_vd_render_fwd(ctypes.byref(cfg), P(st.packed[0][0]), packed1, P(rays.origins), P(rays.directions),
                                     P(rays.viewdirs), B, 0, None, None, 0, P(rgb), P(disp), P(acc), P(rgb2), P(disp2), P(acc2),
                                     P(ws), ws_bytes, None)
    assert call(P(st.packed[1][0]), 1024) == -3                                          # a short workspace
    assert call(None, ws.numel()) == -1                                                  # NULL packed1 with Nf > 0
    assert lib.pxo_vd_render_fwd(ctypes.byref(cfg), None, None, None, None, None, 0, 0, None, None, 0, None, None, None, None,
                                 None, None, None, 0, None) == 0                         # B = 0 touches no pointer
    assert lib.pxo_vd_composite_fwd(ctypes.byref(cfg), None, None, None, None, 0, 32, None, None, None, None, None) == 0
    assert call(P(st.packed[1][0]), ws.numel()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rgb2).all())


@pytest.mark.timeout(300)
def test_eval_and_gen_video_cli(ctx, tmp_path):
    from plenoctree_amd import ops
    from plenoctree_amd.nerf_sh import eval as nerf_eval, gen_video
    from plenoctree_amd.nerf_sh.nerf import datasets, families, utils
    from PIL import Image
    dev = ctx["dev"]
    torch.save({"model": ctx["sd"]}, os.path.join(str(tmp_path), "model.ckpt"))
    argv = ["--train_dir", str(tmp_path), "--use_viewdirs", "true", "--dataset", "synthetic", "--factor", "16", "--chunk", "1000"]
    args = ctx["viewdirs"].add_checkpoint_flags(utils.define_flags()).parse_args(argv)
    dataset = datasets.get_dataset("test", args, dev)
    skip = max(dataset.size - 1, 1)                                        # images 0 and size - 1: at most 2 render
    psnrs = nerf_eval.main(argv + ["--approx_eval_skip", str(skip)])
    assert 1 <= len(psnrs) <= 2 and all(np.isfinite(p) for p in psnrs)
    out_dir = os.path.join(str(tmp_path), "test_preds")
    assert os.path.exists(os.path.join(out_dir, "000.png")) and os.path.exists(os.path.join(out_dir, "disp_000.png"))
    assert np.isfinite(float(open(os.path.join(out_dir, "psnr.txt")).read()))
    # image 0 == model.apply on the same rays in ONE call, bit for bit (1000 is no multiple of the ray block, and the image's
    # last chunk is shorter still): compared through the PNG's 8-bit quantisation of the same float32 values
    ex = dataset.get_image(0)
    H, W = ex["rays"].origins.shape[:2]
    model, state = families.restore(args, dev, "render", say=lambda *a, **k: None)
    flat = Rays(*[r.reshape(-1, 3).contiguous() for r in ex["rays"]])
    rgb = model.apply(state, flat, False)[-1][0].reshape(H, W, 3)
    chunked = utils.render_image(lambda r: model.apply(state, r, False), ex["rays"], chunk=1000)[0]
    assert torch.equal(chunked, rgb)
    want_png = (np.clip(rgb.cpu().numpy(), 0.0, 1.0) * 255.0).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, "000.png"))), want_png)
    frames = gen_video.main(["--train_dir", str(tmp_path), "--use_viewdirs", "true", "--num_views", "2", "--height", "40",
                             "--width", "40", "--chunk", "1000"])
    assert len(frames) == 2 and frames[0].shape == (40, 40, 3)
    fdir = os.path.join(str(tmp_path), "video", "e300", "frames")
    assert os.path.exists(os.path.join(fdir, "0000.png")) and os.path.exists(os.path.join(fdir, "0001.png"))
