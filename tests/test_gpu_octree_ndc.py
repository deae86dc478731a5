"""GPU tests of the NDC launches of the octree side (pxo_octree_render_ndc_fwd / _bwd, pxo_grid_weight_render_ndc) against the
oracle's `ndc=` argument on the shapes of tests/_octree_ndc_oracle.py: the reference's convert_to_ndc (pinned by
tests/golden/octree_ndc.npz), then the oracle's march unchanged.  Bounds are those of the world-space tests in tests/test_gpu_octree.py: the march takes
identical steps, only exp / sigmoid and the summation order differ."""
import os

import numpy as np
import pytest
import torch
import yaml

import _octree_ndc_oracle as N
from oracle import nerf_oracle as O
from oracle import octree_oracle as T
from _helpers import _gpu, close, make_params

pytestmark = pytest.mark.gpu
f32 = np.float32
TINY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llff_tiny")


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _device_tree(t, dev):
    child = torch.from_numpy(t.child).to(dev)
    data = torch.from_numpy(t.data).to(dev)
    return _oops().tree_view(child, data, t.offset, t.invradius), (child, data)


def _dopts(opt):
    return _oops().render_opts(float(opt.step_size), float(opt.background_brightness), float(opt.sigma_thresh), float(opt.stop_thresh))


_WANT = {}


def _want_image(K, box, cam, fast):
    """The oracle image of one of the shared views, computed once per session."""
    key = (K, box, cam, fast)
    if key not in _WANT:
        t = N.box_tree(K, box)
        opt = T.RenderOptions.for_renderer(1e-3, fast)
        o, d = T.camera_rays(N.CAMERAS[cam](), N.W, N.H, N.FX)
        hits = sum(T.march(t, oo, dd, opt.step_size, ndc=N.Ndc()) is not None for oo, dd in zip(o, d))
        img = T.render_persp(t, N.CAMERAS[cam](), N.W, N.H, N.FX, opt, ndc=N.Ndc())
        assert hits >= 20 and float(np.abs(img - 1.0).max()) > 0.5
        assert (hits == N.W * N.H) if (box, cam) == (0, "A") else (hits < N.W * N.H)         # misses are in the picture too
        _WANT[key] = (t, opt, img)
    return _WANT[key]


VIEWS = {1: [(0, "B")], 4: [(1, "A")], 9: [(1, "B")], 16: [(0, "A"), (0, "B"), (1, "A"), (1, "B")], 25: [(0, "A")]}


@pytest.mark.parametrize("K", [1, 4, 9, 16, 25])
def test_ndc_forward_camera_mode_matches_oracle(K):
    """Every SH format, exact and early stop; both cameras and both boxes for SH16, one pair each otherwise; for SH16 and SH25
    every lanes-per-ray instantiation takes the NDC set-up (none may run the world-space march)."""
    oops = _oops(); dev = _gpu()
    for box, cam in VIEWS[K]:
        for fast in (False, True):
            t, opt, want = _want_image(K, box, cam, fast)
            view, keep = _device_tree(t, dev)
            c2w = torch.from_numpy(N.CAMERAS[cam]()).to(dev)
            got = oops.octree_render_persp(view, c2w, N.W, N.H, N.FX, _dopts(opt), ndc=N.Ndc())
            assert got.shape == (N.H, N.W, 3)
            close(f"SH{K} NDC image box {box} camera {cam} fast={fast}", got, torch.from_numpy(want), rtol=0, atol=2e-5)
            world = oops.octree_render_persp(view, c2w, N.W, N.H, N.FX, _dopts(opt))
            assert float((world - got).abs().max()) > 0.1                  # and it is not the world-space image
            if K in (16, 25):
                try:
                    for lanes in (4, 8, 16):
                        oops.set_lanes_per_ray(lanes, lanes)
                        got_l = oops.octree_render_persp(view, c2w, N.W, N.H, N.FX, _dopts(opt), ndc=N.Ndc())
                        close(f"SH{K} NDC image, {lanes} lanes", got_l, torch.from_numpy(want), rtol=0, atol=2e-5)
                finally:
                    oops.set_lanes_per_ray(0, 0)


def _frustum_rays(n, seed):
    """World rays from near camera B's position aimed at points inside the forward frustum; unit directions."""
    rs = np.random.RandomState(seed)
    o = (rs.randn(n, 3) * 0.1 + [0.1, 0.0, 0.1]).astype(f32)
    z = -rs.uniform(1.5, 8.0, n)
    target = np.stack([rs.uniform(-0.5, 0.5, n) * -z, rs.uniform(-0.35, 0.35, n) * -z, z], 1)
    d = target - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)


@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_ndc_forward_explicit_rays(B):
    """Explicit world-space rays around the 64-rays-per-block edge, two of them unconvertible (d_z = 0, d_z > 0: background,
    finite); and the camera's own rays give the camera-mode image bit for bit."""
    oops = _oops(); dev = _gpu()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t = N.box_tree(16, 1)
    view, keep = _device_tree(t, dev)
    opt = T.RenderOptions(2e-3, background_brightness=0.5)
    o, d = _frustum_rays(B, 7)
    want = T.render_rays(t, o, d, d, opt, ndc=N.Ndc())
    got = oops.octree_render_rays(view, to(o), to(d), to(d), _dopts(opt), ndc=N.Ndc())
    close(f"NDC rays B={B}", got, torch.from_numpy(want), rtol=0, atol=2e-5)
    if B > 1:
        assert float(np.abs(want - 0.5).max()) > 0.2
        # the last two rays replaced by rays that cannot be converted
        o2, d2 = o.copy(), d.copy()
        d2[-2] = [0.6, 0.8, 0.0]
        d2[-1] = [0.0, 0.6, 0.8]
        got2 = oops.octree_render_rays(view, to(o2), to(d2), to(d2), _dopts(opt), ndc=N.Ndc())
        assert bool(torch.isfinite(got2).all()) and torch.equal(got2[-2:].cpu(), torch.full((2, 3), 0.5))
        assert torch.equal(got2[:-2], got[:-2])
        want2 = T.render_rays(t, o2[-2:], d2[-2:], d2[-2:], opt, ndc=N.Ndc())
        assert np.array_equal(want2, np.full((2, 3), 0.5, f32))
    if B == 65:
        for cam in "AB":
            co, cd = T.camera_rays(N.CAMERAS[cam](), N.W, N.H, N.FX)
            img = oops.octree_render_persp(view, to(N.CAMERAS[cam]()), N.W, N.H, N.FX, _dopts(opt), ndc=N.Ndc())
            rays = oops.octree_render_rays(view, to(co), to(cd), to(cd), _dopts(opt), ndc=N.Ndc())
            assert torch.equal(rays.reshape(N.H, N.W, 3), img), cam


@pytest.fixture(params=[0, 1], ids=["wave_per_sample", "ray_parallel"])
def bwd_update(request):
    oops = _oops()
    default = oops.get_tuning(oops.TUNE_BWD_UPDATE)
    oops.set_tuning(oops.TUNE_BWD_UPDATE, request.param)
    yield request.param
    oops.set_tuning(oops.TUNE_BWD_UPDATE, default)


@pytest.fixture(params=[0, 16], ids=["direct_scatter", "cache16"])
def bwd_cache(request):
    oops = _oops()
    default = oops.get_tuning(oops.TUNE_BWD_CACHE_ROWS)
    oops.set_tuning(oops.TUNE_BWD_CACHE_ROWS, request.param)
    yield request.param
    oops.set_tuning(oops.TUNE_BWD_CACHE_ROWS, default)


_WANT_GRAD = {}


def _want_grad(K):
    """float64 autograd through render_rays_torch over the NDC sample sequence of camera B's rays (hits and misses) on a
    depth-2 tree in the off-centre box; once per K."""
    if K not in _WANT_GRAD:
        t = N.box_tree(K, 1, depth=2, seed=30 + K, p=0.3)
        o, d = T.camera_rays(N.camera_b(), N.W, N.H, N.FX)
        g = np.random.RandomState(K + 1).randn(o.shape[0], 3).astype(f32)
        opt = T.RenderOptions(1e-3)
        dd = torch.tensor(t.data.astype(np.float64), requires_grad=True)
        out = T.render_rays_torch(t, dd, o, d, d, opt, ndc=N.Ndc())
        (out * torch.from_numpy(g.astype(np.float64))).sum().backward()
        hit = np.array([T.march(t, oo, dd_, opt.step_size, ndc=N.Ndc()) is not None for oo, dd_ in zip(o, d)])
        assert 20 <= hit.sum() < hit.size
        _WANT_GRAD[K] = (t, o, d, g, opt, dd.grad.float(), out.detach(), hit)
    return _WANT_GRAD[K]


@pytest.mark.parametrize("K", [4, 16, 25])
def test_ndc_gradient_matches_oracle(K, bwd_update, bwd_cache):
    oops = _oops(); dev = _gpu()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    t, o, d, g, opt, want, want_img, hit = _want_grad(K)
    view, (child, data) = _device_tree(t, dev)
    assert float(want.abs().max()) > 1e-3
    atol = 2e-6 * float(want.abs().max()) + 1e-7
    grad = torch.zeros_like(data)
    oops.octree_render_rays_bwd(view, to(o), to(d), to(d), _dopts(opt), to(g), grad, ndc=N.Ndc())
    close(f"SH{K} NDC d/d data", grad, want, rtol=2e-3, atol=atol)
    # accumulation: a second call doubles the gradient; handing over the forward result skips one march
    fwd = oops.octree_render_rays(view, to(o), to(d), to(d), _dopts(opt), ndc=N.Ndc())
    close("NDC forward of the gradient's rays", fwd, want_img.float(), rtol=0, atol=2e-5)
    oops.octree_render_rays_bwd(view, to(o), to(d), to(d), _dopts(opt), to(g), grad, out_rgb=fwd, ndc=N.Ndc())
    close("accumulated", grad, 2 * want, rtol=2e-3, atol=2 * atol)
    # camera mode is the same gradient
    gc = torch.zeros_like(data)
    oops.octree_render_persp_bwd(view, to(N.camera_b()), N.W, N.H, N.FX, _dopts(opt), to(g).reshape(N.H, N.W, 3), gc, ndc=N.Ndc())
    close("camera mode", gc, want, rtol=2e-3, atol=atol)
    # a miss contributes an exact zero: the box misses of this camera, a ray with d_z = 0 and one looking backwards
    mo = np.concatenate([o[~hit], o[:2]])
    md = np.concatenate([d[~hit], np.array([[0.6, 0.8, 0.0], [0.0, 0.6, 0.8]], f32)])
    mg = np.concatenate([g[~hit], g[:2]])
    gm = torch.zeros_like(data)
    oops.octree_render_rays_bwd(view, to(mo), to(md), to(md), _dopts(opt), to(mg), gm, ndc=N.Ndc())
    assert int(torch.count_nonzero(gm)) == 0


@pytest.mark.parametrize("K", [4, 16])
def test_ndc_svox_bridge_equals_the_direct_call(K):
    """render_persp(..., fast=False) on a tree whose data requires grad, then backward: the image and tree.data.grad are those
    of the direct calls (the gradient to the round-off of float32 atomics in another order)."""
    oops = _oops(); dev = _gpu()
    from plenoctree_amd.octree import svox
    t, o, d, g, opt, want, want_img, hit = _want_grad(K)
    view, (child, data) = _device_tree(t, dev)
    c2w = torch.from_numpy(N.camera_b()).to(dev)
    radius = 0.5 / t.invradius
    host = svox.N3Tree(N=2, data_dim=t.data_dim, depth_limit=2, radius=radius, center=(1.0 - 2.0 * t.offset) * radius,
                       data_format=f"SH{K}", map_location=dev)
    host.child, host.parent_depth = child, torch.from_numpy(t.parent_depth).to(dev)
    host.data = data.clone().requires_grad_(True)
    host.level_nodes = np.bincount(t.parent_depth[:, 1]).tolist()
    r = svox.VolumeRenderer(host, step_size=1e-3, ndc=svox.NDCConfig(N.W, N.H, N.FX))
    im = r.render_persp(c2w, width=N.W, height=N.H, fx=N.FX, fast=False)
    direct = oops.octree_render_persp(view, c2w, N.W, N.H, N.FX, _dopts(opt), ndc=N.Ndc())
    assert torch.equal(im.detach(), direct)
    gd = torch.from_numpy(g).to(dev).reshape(N.H, N.W, 3)
    (im * gd).sum().backward()
    grad = torch.zeros_like(data)
    oops.octree_render_persp_bwd(view, c2w, N.W, N.H, N.FX, _dopts(opt), gd.contiguous(), grad, out_rgb=direct, ndc=N.Ndc())
    close("bridge grad", host.data.grad, grad, rtol=1e-4, atol=2e-6 * float(grad.abs().max()) + 1e-7)
    close("bridge grad against the oracle", host.data.grad, want, rtol=2e-3, atol=2e-6 * float(want.abs().max()) + 1e-7)
    with pytest.raises(ValueError, match="NDCConfig"):
        r.render_persp(c2w, width=N.W + 1, height=N.H, fx=N.FX)
    with torch.no_grad():
        rays = r.forward(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), torch.from_numpy(d).to(dev))
    assert torch.equal(rays.reshape(N.H, N.W, 3), direct)


@pytest.mark.parametrize("reso", [16, 64, 12])
def test_ndc_grid_weight_render_matches_oracle(reso):
    """reso 16: the whole grid sits in the slab marcher's window; 64 at 13 x 11 pixels: most samples take its out-of-window path;
    12: not a power of two, the plain bricked kernel.  Camera A's NDC rays are all parallel to z."""
    oops = _oops(); dev = _gpu()
    W, H, fx = 13, 11, 14.0
    ndc = N.Ndc(W, H, fx)
    sigma = ((np.random.RandomState(0).rand(reso, reso, reso) - 0.6) * 30.0).astype(f32)
    t = T.Tree(4, 3, [0.0, 0.0, 0.0], 1.0)
    cams = np.stack([N.camera_a(), N.camera_b()])
    opt = T.RenderOptions(step_size=1e-3)
    want = np.zeros_like(sigma)
    for c in cams:
        T.grid_weight_render(sigma, c, W, H, fx, opt, t.offset, t.invradius, weight=want, ndc=ndc)
    sig_d, cams_d = torch.from_numpy(sigma).to(dev), torch.from_numpy(cams).to(dev)
    call = lambda c=cams_d, acc=None: oops.grid_weight_render(sig_d, reso, c, fx, fx, W, H, oops.render_opts(1e-3), t.offset,
                                                              t.invradius, grid_weight=acc, ndc=ndc)
    got = call()
    assert (want > 0).sum() > 50
    close("NDC grid weights", got, torch.from_numpy(want), rtol=1e-5, atol=1e-6)
    world = oops.grid_weight_render(sig_d, reso, cams_d, fx, fx, W, H, oops.render_opts(1e-3), t.offset, t.invradius)
    assert not torch.equal(world, got)
    # both marchers and both tile orders: the same samples, the same arithmetic, bit-equal
    default_order = oops.get_tuning(oops.TUNE_GW_TILE_ORDER)
    try:
        for order in (0, 1):
            for mode in (0, 1):
                oops.set_tuning(oops.TUNE_GW_TILE_ORDER, order); oops.set_tuning(oops.TUNE_GW_MARCHER, mode)
                assert torch.equal(call(), got), (order, mode)
    finally:
        oops.set_tuning(oops.TUNE_GW_TILE_ORDER, default_order); oops.set_tuning(oops.TUNE_GW_MARCHER, -1)
    # accumulating camera by camera == one call
    acc = None
    for i in range(cams.shape[0]):
        acc = call(cams_d[i:i + 1], acc)
    assert torch.equal(acc, got)


def test_ndc_known_answer_on_the_device():
    """Known answer 2 of tests/test_octree_ndc_cpu.py, rendered by the device: the chord of the NDC ray and world-space shading,
    same bound."""
    oops = _oops(); dev = _gpu()
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def render(t, o, d, opt):
        view, keep = _device_tree(t, dev)
        rays = oops.octree_render_rays(view, to(o), to(d), to(d), _dopts(opt), ndc=N.Ndc())
        img = oops.octree_render_persp(view, to(N.camera_b()), N.W, N.H, N.FX, _dopts(opt), ndc=N.Ndc())
        assert torch.equal(rays.reshape(N.H, N.W, 3), img)
        return rays.cpu().numpy()

    worst, bound = N.known_answer_check(render)
    print(f"known answer on the device: max error {worst:.3g}, bound {bound:.3g}")


def test_world_space_launches_are_untouched_by_an_ndc_call():
    """One SH16 view and its gradient through the existing entry points, before and after NDC calls in the same process:
    bit-equal.  The gradient view is 4 x 4 pixels -- one wave, whose atomics execute in program order -- so that bit equality
    is a property of the code and not of the order in which waves happen to run."""
    oops = _oops(); dev = _gpu()
    t = N.box_tree(16, 1)
    view, (child, data) = _device_tree(t, dev)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    from plenoctree_amd.nerf_sh.nerf.datasets import pose_spherical
    c2w = to(pose_spherical(20.0, 30.0, 3.0)[:3].astype(f32))
    opts = oops.render_opts(1e-3)
    g = to(np.random.RandomState(3).randn(4, 4, 3).astype(f32))

    def world():
        img = oops.octree_render_persp(view, c2w, N.W, N.H, N.FX, opts)
        small = oops.octree_render_persp(view, c2w, 4, 4, 3.0, opts)
        grad = torch.zeros_like(data)
        oops.octree_render_persp_bwd(view, c2w, 4, 4, 3.0, opts, g, grad, out_rgb=small)
        return img, grad

    img0, grad0 = world()
    assert float((img0 - 1.0).abs().max()) > 0.2 and float(grad0.abs().max()) > 0
    ndc_img = oops.octree_render_persp(view, to(N.camera_b()), N.W, N.H, N.FX, opts, ndc=N.Ndc())
    gn = torch.zeros_like(data)
    oops.octree_render_persp_bwd(view, to(N.camera_b()), N.W, N.H, N.FX, opts, torch.ones_like(ndc_img), gn, ndc=N.Ndc())
    sigma = torch.rand(16 ** 3, device=dev) * 10.0
    oops.grid_weight_render(sigma, 16, to(N.camera_b())[None], N.FX, N.FX, N.W, N.H, opts, t.offset, t.invradius, ndc=N.Ndc())
    img1, grad1 = world()
    assert torch.equal(img0, img1) and torch.equal(grad0, grad1)
    assert not torch.equal(ndc_img, img0)


def test_llff_extraction_pipeline_end_to_end(tmp_path, monkeypatch):
    """octree.extraction -> evaluation -> optimization through their CLIs on tests/golden/llff_tiny (factor 2: 12 x 8 images; the
    llff preset shortened as tests/test_gpu_llff.py::test_cli_train_eval_render_path does), in NDC; then the same directory with
    --spherify true, which must take the world-space path.
    Learning rate: the reference's 1e7 is tuned for the mean over 800 x 800 pixels; test_extraction_pipeline_end_to_end scales it
    by the pixel count and halves it (2e4 at 50 x 50 ~ 1e7 * 2500 / 640000 / 2).  The same rule at 12 x 8 gives 1e7 * 96 / 640000
    / 2 = 750."""
    oops = _oops(); dev = _gpu()
    import plenoctree_amd.nerf_sh as pkg
    from plenoctree_amd.nerf_sh.nerf import checkpoints, models, utils
    from plenoctree_amd.octree import evaluation, extraction, optimization, svox
    with open(os.path.join(os.path.dirname(pkg.__file__), "config", "llff.yaml")) as f:
        preset = yaml.safe_load(f)
    preset.update(factor=2, batch_size=256)
    cfg_path = os.path.join(str(tmp_path), "llff_short.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(preset, f)
    common = ["--train_dir", str(tmp_path), "--config", cfg_path, "--data_dir", TINY]
    args = utils.define_flags().parse_args(common)
    utils.update_flags(args)
    model, _ = models.construct_nerf(args, dev)
    state = models.TrainState(model.cfg, make_params(O.Cfg(), seed=11, bias_scale=0.2).to(dev))
    checkpoints.save_checkpoint(str(tmp_path), state, step=0)

    seen = {"gw": [], "renderer": []}
    real_gw, real_vr = oops.grid_weight_render, svox.VolumeRenderer
    monkeypatch.setattr(oops, "grid_weight_render", lambda *a, **k: (seen["gw"].append(k.get("ndc")), real_gw(*a, **k))[1])

    class Recorder(real_vr):
        def __init__(self, tree, *a, **k):
            seen["renderer"].append(k.get("ndc"))
            super().__init__(tree, *a, **k)

    monkeypatch.setattr(extraction, "VolumeRenderer", Recorder)
    monkeypatch.setattr(optimization, "VolumeRenderer", Recorder)
    out = os.path.join(str(tmp_path), "tree.npz")
    box = ["--init_grid_depth", "4", "--radius", "1 1 1", "--center", "0 0 0", "--samples_per_cell", "8",
           "--renderer_step_size", "1e-3"]
    trees = {}
    for mode in ("sigma", "weight"):
        tree = extraction.main(common + box + ["--output", out, "--masking_mode", mode, "--eval", "false"])
        assert tree.max_depth == 4 and tree.n_internal > 20
        assert bool((tree.data[..., -1] >= 0).all())
        trees[mode] = tree
    assert len(seen["gw"]) == 1 and isinstance(seen["gw"][0], svox.NDCConfig)
    cfg = seen["gw"][0]
    assert (cfg.width, cfg.height) == (12, 8)
    # the weight mask of the run is the NDC one, and the world-space mask of the same grid is another
    from plenoctree_amd.nerf_sh.nerf import llff
    train = llff.get_dataset("train", args, dev)
    center, radius = extraction.tree_center_radius(trees["weight"])
    sig = extraction.grid_sigma(model, state, 32, center, radius)
    masks = {}
    for name, ndc in (("ndc", cfg), ("world", None)):
        w = extraction.calculate_grid_weights(train, sig, 32, trees["weight"].invradius, trees["weight"].offset, 1e-3, ndc=ndc)
        masks[name] = oops.threshold_mask(w, 0.001)
    assert not torch.equal(masks["ndc"], masks["world"])
    rebuilt = svox.N3Tree(N=2, data_dim=49, depth_limit=4, radius=[1, 1, 1], center=[0, 0, 0], data_format="SH16",
                          map_location=dev).refine_from_mask(masks["ndc"])
    assert torch.equal(rebuilt.child, trees["weight"].child)
    # evaluation: NDC renderer, finite PSNR, the GIF
    vid = os.path.join(str(tmp_path), "eval.gif")
    psnr = evaluation.main(common + ["--input", out, "--renderer_step_size", "1e-3", "--write_vid", vid])
    assert np.isfinite(psnr) and os.path.exists(vid)
    assert isinstance(seen["renderer"][-1], svox.NDCConfig) and seen["renderer"][-1].focal == cfg.focal
    # optimisation: three epochs in NDC improve the training PSNR
    hist = optimization.main(common + ["--input", out, "--output", os.path.join(str(tmp_path), "tree_opt.npz"),
                                       "--num_epochs", "3", "--val_interval", "1", "--renderer_step_size", "1e-3",
                                       "--lr", "750", "--continue_on_decrease"])
    train_psnrs = [h[1] for h in hist if h[1] is not None]
    assert len(train_psnrs) == 3 and train_psnrs[-1] > train_psnrs[0], hist
    assert isinstance(seen["renderer"][-1], svox.NDCConfig)
    # --spherify true: the same directory as a world-space scene
    seen["gw"].clear(); seen["renderer"].clear()
    out_s = os.path.join(str(tmp_path), "tree_sph.npz")
    ts = extraction.main(common + ["--spherify", "true", "--init_grid_depth", "4", "--samples_per_cell", "8",
                                   "--renderer_step_size", "1e-3", "--output", out_s, "--masking_mode", "weight", "--eval", "true"])
    assert ts.max_depth == 4 and seen["gw"] == [None] and seen["renderer"] == [None]
    psnr_s = evaluation.main(common + ["--spherify", "true", "--input", out_s, "--renderer_step_size", "1e-3"])
    assert np.isfinite(psnr_s) and seen["renderer"] == [None, None]
