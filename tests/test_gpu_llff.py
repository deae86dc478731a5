"""Forward-facing (LLFF) scenes on the device: the NDC ray kernels (pxo_generate_rays_ndc, pxo_sample_batch_ndc) against the
float64 evaluation of the host formula llff.convert_to_ndc -- itself held to the reference's float64 evaluation by
tests/test_llff_cpu.py --, their exact relations to the existing launches, one training step in the NDC regime against the
float64 oracle, and the three entry points on tests/golden/llff_tiny.

The ray bound is 4 x e_ref, e_ref read from tests/golden/llff_reference.npz: the reference's OWN float32 distance from its
float64 evaluation (4.8e-7 for origins and directions); the factor covers the kernel's freedom in FMA contraction and
operation order relative to numpy's float32.  Measured kernel deviations: tests/golden/README_llff.md."""
import os

import numpy as np
import pytest
import torch
import yaml

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

from _helpers import (_gpu, _ops, close, hip_sample_positions, make_params, oracle_loss_and_grad_given_z,  # noqa: E402
                      pxo_cfg, split_mlp)

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "llff_tiny")
W, H, FOCAL, N_CAMS = 11, 7, 9.5, 3          # odd and non-square: p % W, p / W and the half-pixel centre all matter
HW = W * H


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(HERE, "golden", "llff_reference.npz")))


@pytest.fixture(scope="module")
def cams(ref):
    """The first three recentred training poses of llff_tiny as the reference's loader produced them, float32 [3,3,4]."""
    c2w = np.ascontiguousarray(ref["train_s0_f0_h8_camtoworlds"][:N_CAMS])
    assert c2w.dtype == np.float32 and c2w.shape == (N_CAMS, 3, 4)
    return c2w


@pytest.fixture(scope="module")
def truth(cams):
    """float64 NDC rays of every pixel of the three cameras, from the same float32 poses: (origins, directions) [3*HW,3]."""
    from plenoctree_amd.nerf_sh.nerf import llff, utils
    rays = utils.generate_rays(W, H, np.float64(FOCAL), cams.astype(np.float64))
    o, d = llff.convert_to_ndc(rays.origins, rays.directions, np.float64(FOCAL), W, H)
    assert o.dtype == np.float64
    return o.reshape(-1, 3), d.reshape(-1, 3)


def _check(tag, o, d, ids, truth, ref):
    eo, ed = float(ref["e_ref_origins"]), float(ref["e_ref_directions"])
    o, d = o.cpu().double().numpy(), d.cpu().double().numpy()
    assert np.isfinite(o).all() and np.isfinite(d).all()
    dev_o, dev_d = np.abs(o - truth[0][ids]).max(), np.abs(d - truth[1][ids]).max()
    plane = max(np.abs(o[:, 2] + 1.0).max(), np.abs(o[:, 2] + d[:, 2] - 1.0).max())
    print(f"{tag}: |kernel - f64| origins {dev_o:.3e} directions {dev_d:.3e}; |o_z + 1|, |o_z + d_z - 1| {plane:.3e} "
          f"(bound {4 * eo:.3e})")
    assert dev_o <= 4 * eo, f"{tag}: origins {dev_o:.3e} > 4 e_ref = {4 * eo:.3e}"
    assert dev_d <= 4 * ed, f"{tag}: directions {dev_d:.3e} > 4 e_ref = {4 * ed:.3e}"
    # known answers: every origin on the near plane z = -1, every ray ends on z = +1
    assert plane <= 4 * max(eo, ed)


@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_generate_rays_ndc_against_float64_at_block_edges(B, cams, truth, ref):
    ops = _ops(); dev = _gpu()
    ids = (torch.arange(B, dtype=torch.int64) * 37 + 5) % (N_CAMS * HW)
    o, d, v = ops.generate_rays_multi_ndc(torch.from_numpy(cams).to(dev), W, H, FOCAL, ids.to(dev))
    assert o.shape == d.shape == v.shape == (B, 3)
    _check(f"B={B}", o, d, ids.numpy(), truth, ref)
    if B > 1:
        assert len(torch.unique(torch.div(ids, HW, rounding_mode="floor"))) == N_CAMS


def test_generate_rays_ndc_whole_images_and_explicit_ids(cams, truth, ref):
    ops = _ops(); dev = _gpu()
    cd = torch.from_numpy(cams).to(dev)
    for c in range(N_CAMS):                                   # pixel ids NULL: a whole image
        o, d, v = ops.generate_rays_ndc(cd[c], W, H, FOCAL)
        assert o.shape == (HW, 3)
        _check(f"camera {c}, whole image", o, d, np.arange(c * HW, (c + 1) * HW), truth, ref)
    # explicit ids into the [3, H*W] table: first and last pixel of every camera, the last camera's included
    ids = torch.tensor([0, HW - 1, HW, 2 * HW - 1, 2 * HW, N_CAMS * HW - 1, W - 1, W, 2 * HW + W], dtype=torch.int64)
    o, d, v = ops.generate_rays_multi_ndc(cd, W, H, FOCAL, ids.to(dev))
    _check("explicit ids", o, d, ids.numpy(), truth, ref)
    last = torch.tensor([0, HW - 1], dtype=torch.int64, device=dev)
    o, d, v = ops.generate_rays_ndc(cd[N_CAMS - 1], W, H, FOCAL, last)
    _check("last camera, first and last pixel", o, d, np.array([2 * HW, 3 * HW - 1]), truth, ref)


def test_exact_relations_to_the_existing_launches(cams):
    ops = _ops(); dev = _gpu()
    cd = torch.from_numpy(cams).to(dev)
    gids = ops.randint(9, 1, 1003, N_CAMS * HW, device=dev)
    before = ops.generate_rays_multi(cd, W, H, FOCAL, gids)
    image = torch.rand(HW, 3, device=dev)
    before_batch = ops.sample_batch(12345, 9, cd[1], W, H, FOCAL, image, 300, want_ids=True)
    # multi-camera call == per-camera calls
    o, d, v = ops.generate_rays_multi_ndc(cd, W, H, FOCAL, gids)
    cam = torch.div(gids, HW, rounding_mode="floor")
    assert len(torch.unique(cam)) == N_CAMS
    for c in range(N_CAMS):
        sel = cam == c
        o1, d1, v1 = ops.generate_rays_ndc(cd[c], W, H, FOCAL, (gids[sel] - c * HW).contiguous())
        assert torch.equal(o[sel], o1) and torch.equal(d[sel], d1) and torch.equal(v[sel], v1)
    # viewdirs == those of pxo_generate_rays: the world-space unit directions
    assert torch.equal(v, before[2])
    assert not torch.equal(o, before[0]) and not torch.equal(d, before[1])
    # sample_batch_ndc == randint + generate_rays_ndc + gather, the slice of the whole draw included
    whole = ops.randint(12345, 9, 100 + 777, HW, device=dev)
    for first in (0, 100):
        for B in (1, 257, 777):
            o, d, v, px, ids = ops.sample_batch_ndc(12345, 9, cd[1], W, H, FOCAL, image, B, want_ids=True, first=first)
            assert torch.equal(ids, whole[first:first + B])
            o2, d2, v2 = ops.generate_rays_ndc(cd[1], W, H, FOCAL, ids)
            assert torch.equal(o, o2) and torch.equal(d, d2) and torch.equal(v, v2)
            assert torch.equal(px, image[ids])
            assert ops.sample_batch_ndc(12345, 9, cd[1], W, H, FOCAL, image, B, first=first)[3].equal(px)   # ids NULL
    # the non-NDC entry points give the same bits after the NDC ones ran
    after = ops.generate_rays_multi(cd, W, H, FOCAL, gids)
    after_batch = ops.sample_batch(12345, 9, cd[1], W, H, FOCAL, image, 300, want_ids=True)
    for a, b in zip(before + before_batch, after + after_batch):
        assert torch.equal(a, b)
    # another near plane is another ray
    o3, d3, _ = ops.generate_rays_ndc(cd[0], W, H, FOCAL, ndc_near=0.5)
    assert float((o3[:, 2] + 1.0).abs().max()) < 2e-6 and not torch.equal(o3, ops.generate_rays_ndc(cd[0], W, H, FOCAL)[0])
    from plenoctree_amd._lib import PxoError
    with pytest.raises(PxoError, match="pxo_generate_rays_ndc"):
        ops.generate_rays_ndc(cd[0], W, H, FOCAL, ndc_near=0.0)


def _llff_args(extra=()):
    from plenoctree_amd.nerf_sh.nerf import utils
    a = utils.define_flags().parse_args(["--config", "llff", "--train_dir", "x", "--data_dir", TINY, *extra])
    utils.update_flags(a)
    a.factor = 0
    return a


def test_dataset_feeds_ndc_batches_on_the_device(ref):
    """LLFF on the device: the fused launch, the three separate ones and the image-batching table give NDC rays of the
    recorded images; shards are contiguous rows of the whole draw."""
    ops = _ops(); dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import llff
    e = 4 * max(float(ref["e_ref_origins"]), float(ref["e_ref_directions"]))
    k = "train_s0_f0_h8_"
    ds = llff.get_dataset("train", _llff_args(), dev, batch_size=256)
    np.testing.assert_array_equal(ds.images.cpu().numpy().reshape(-1, ds.h, ds.w, 3), ref[k + "images"])
    for j, cam in enumerate(ref[k + "ray_cams"]):
        ex = ds.get_image(int(cam))
        o, d, v = [r.reshape(-1, 3).cpu().double().numpy() for r in ex["rays"]]
        assert np.abs(o - ref[k + "ndc64_origins"][j]).max() <= e and np.abs(d - ref[k + "ndc64_directions"][j]).max() <= e
        np.testing.assert_allclose(v, ref[k + "rays_viewdirs"][j], rtol=1e-5, atol=1e-6)
    whole = llff.get_dataset("train", _llff_args(), dev, batch_size=256, seed=5)
    shards = [llff.get_dataset("train", _llff_args(), dev, batch_size=64, seed=5, shard=(r, 4)) for r in range(4)]
    for _ in range(2):
        want = next(whole)
        assert float((want["rays"].origins[:, 2] + 1.0).abs().max()) <= e
        for r, sd in enumerate(shards):
            got = next(sd)
            assert torch.equal(got["pixels"], want["pixels"][r * 64:(r + 1) * 64])
            for a, b in zip(got["rays"], want["rays"]):
                assert torch.equal(a, b[r * 64:(r + 1) * 64])
    args = _llff_args(); args.image_batching = True
    tab = llff.get_dataset("train", args, dev, batch_size=300, seed=5)
    b = next(tab)
    ids = ops.randint(5, 1, 300, tab.size * tab.h * tab.w, device=dev)
    o, d, v = ops.generate_rays_multi_ndc(tab._c2w_dev, tab.w, tab.h, tab.focal, ids)
    assert torch.equal(b["rays"].origins, o) and torch.equal(b["rays"].directions, d) and torch.equal(b["rays"].viewdirs, v)
    assert torch.equal(b["pixels"], tab.images.reshape(-1, 3)[ids])
    # --spherify: world-space rays through the existing launches
    args = _llff_args(); args.spherify = True
    sph = llff.get_dataset("train", args, dev, batch_size=64)
    bs = next(sph)
    cam_pos = torch.from_numpy(sph.camtoworlds[:, :, 3]).to(dev)
    assert float((bs["rays"].origins[:, None] - cam_pos[None]).abs().sum(-1).min(dim=1).values.max()) == 0.0


def test_one_training_step_in_the_ndc_regime():
    """pxo_train_fwd_bwd on 256 NDC rays of llff_tiny (near 0, far 1, black background, 16 + 32 samples, SH16) against
    oracle/nerf_oracle.py in float64, at the bounds tests/test_gpu_parity.py::test_train_fwd_bwd_matches_oracle asserts: loss and
    coarse loss rtol 1e-5 / atol 1e-7 and gradient rel L2 per MLP <= 1e-3 against the float64 loss_fn evaluated at the HIP
    path's own sample positions; PSNR rtol 2e-5 / atol 1e-6 (its bound for the Stats)."""
    ops = _ops(); dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import llff
    B = 256
    batch = next(llff.get_dataset("train", _llff_args(), dev, batch_size=B, seed=3))
    rays_dev = tuple(batch["rays"])
    rays = O.Rays(*[r.cpu() for r in rays_dev])
    px = batch["pixels"].cpu()
    assert float(px.max()) > 0.2 and float((px.sum(-1) == 0).float().mean()) > 0.05          # spheres and background
    cfg = O.Cfg(sh_deg=3, num_coarse_samples=16, num_fine_samples=32, near=0.0, far=1.0, white_bkgd=False,
                sparsity_npoints=300, sparsity_weight=1e-3)
    pcfg = pxo_cfg(ops, cfg)
    flat = make_params(cfg, bias_scale=0.2)
    gen = torch.Generator().manual_seed(53)
    t_rand, u = torch.rand(B, 16, generator=gen), torch.rand(B, 32, generator=gen)
    sp_pts = (torch.rand(300, 3, generator=gen) * 2 - 1) * 1.5
    fd = flat.to(dev)
    packed = [ops.pack_weights(pcfg, split_mlp(fd, cfg, i)) for i in range(2)]
    grads = torch.full_like(fd, float("nan"))
    stats = torch.zeros(6, device=dev)
    ws = torch.empty(ops.train_workspace_bytes(pcfg, B), dtype=torch.uint8, device=dev)
    ops.train_fwd_bwd(pcfg, fd, packed, *rays_dev, batch["pixels"], grads, stats, ws, randomized=True, t_rand=t_rand.to(dev),
                      u=u.to(dev), sp_points=sp_pts.to(dev))
    s = stats.cpu()
    z_c, z_f = hip_sample_positions(ops, pcfg, packed, rays_dev, t_rand.to(dev), u.to(dev))
    assert float(z_c.min()) >= 0.0 and float(z_f.max()) <= 1.0                               # the NDC depth range
    l64, lc64, g64 = oracle_loss_and_grad_given_z(flat, rays, px, cfg, z_c.cpu(), z_f.cpu(), sp_pts)
    l32, lc32, g32 = oracle_loss_and_grad_given_z(flat, rays, px, cfg, z_c.cpu(), z_f.cpu(), sp_pts, dtype=torch.float32)
    psnr64 = -10.0 * np.log10(l64)
    n = flat.numel() // 2
    e_hip = [float((grads[lo:lo + n].cpu().double() - g64[lo:lo + n]).norm() / g64[lo:lo + n].norm()) for lo in (0, n)]
    e_f32 = [float((g32[lo:lo + n].double() - g64[lo:lo + n]).norm() / g64[lo:lo + n].norm()) for lo in (0, n)]
    print(f"loss HIP {float(s[0]):.9g} f64 {l64:.9g} f32 oracle {l32:.9g}; loss_c HIP {float(s[2]):.9g} f64 {lc64:.9g} "
          f"f32 oracle {lc32:.9g}; psnr HIP {float(s[1]):.7g} f64 {psnr64:.7g}")
    print(f"gradient rel L2 vs f64 at the same positions: HIP {e_hip[0]:.3e} / {e_hip[1]:.3e}, float32 oracle "
          f"{e_f32[0]:.3e} / {e_f32[1]:.3e}")
    assert torch.isfinite(grads).all() and torch.isfinite(s).all()
    close("loss vs f64 at the same positions", s[0], torch.tensor(l64), rtol=1e-5, atol=1e-7)
    close("loss_c vs f64 at the same positions", s[2], torch.tensor(lc64), rtol=1e-5, atol=1e-7)
    close("psnr vs f64 at the same positions", s[1], torch.tensor(psnr64), rtol=2e-5, atol=1e-6)
    for i, lo in enumerate((0, n)):
        assert float(g64[lo:lo + n].norm()) > 1e-4, "degenerate test: oracle gradient vanishes"
        assert e_hip[i] <= 1e-3, f"MLP_{i}: rel L2 err vs the f64 oracle at the same sample positions {e_hip[i]:.3g}"


def test_cli_train_eval_render_path(tmp_path):
    """nerf_sh.train / eval / eval --render_path / gen_video --render_path on llff_tiny with the values of the llff preset.  A
    preset overrides the command line for the keys it holds (as in the reference), so the short schedule -- factor 2, batch
    256, 4 steps -- lives in a copy of config/llff.yaml, like the schedule of test_gpu_parity.py::test_cli_train_eval_extraction."""
    _gpu()
    from plenoctree_amd.nerf_sh import eval as eval_mod, gen_video, train
    import plenoctree_amd.nerf_sh as pkg
    with open(os.path.join(os.path.dirname(pkg.__file__), "config", "llff.yaml")) as f:
        preset = yaml.safe_load(f)
    assert preset["dataset"] == "llff" and preset["factor"] == 4 and preset["near"] == 0.0 and preset["far"] == 1.0
    preset.update(factor=2, batch_size=256, max_steps=4, print_every=1, save_every=4, render_every=4)
    cfg_path = os.path.join(str(tmp_path), "llff_short.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(preset, f)
    common = ["--train_dir", str(tmp_path), "--config", cfg_path, "--data_dir", TINY]
    trace = train.main(common)
    assert len(trace) == 4 and all(np.isfinite(t[1]) and np.isfinite(t[2]) and t[1] > 0 for t in trace), trace
    assert os.path.exists(os.path.join(str(tmp_path), "checkpoint_4"))
    assert os.path.exists(os.path.join(str(tmp_path), "render", "0000000004.png"))
    psnrs = eval_mod.main(common)
    assert len(psnrs) == 2 and all(np.isfinite(psnrs))
    preds = os.path.join(str(tmp_path), "test_preds")
    assert sorted(os.listdir(preds)) == sorted(["000.png", "001.png", "disp_000.png", "disp_001.png", "psnr.txt", "ssim.txt",
                                                "psnrs_4.txt", "ssims_4.txt"])
    from PIL import Image
    assert Image.open(os.path.join(preds, "000.png")).size == (12, 8)
    disp = np.asarray(Image.open(os.path.join(preds, "disp_000.png")))
    assert disp.min() == 0 and disp.max() == 255                       # normalize_disp: the map spans the whole range
    assert eval_mod.main(common + ["--render_path", "true"]) == []
    renders = os.path.join(str(tmp_path), "path_renders")
    names = sorted(os.listdir(renders))
    assert names == sorted([f"{i:03d}.png" for i in range(120)] + [f"disp_{i:03d}.png" for i in range(120)]), names
    frames = gen_video.main(common + ["--render_path", "true"])
    assert len(frames) == 120 and frames[0].shape == (8, 12, 3)
    assert os.path.exists(os.path.join(str(tmp_path), "video", "path", "frames", "0119.png"))
    with pytest.raises(ValueError, match="render_path"):
        gen_video.main(common)
