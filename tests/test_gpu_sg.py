"""GPU tests of the spherical-Gaussian (SG) chain: pxo_octree_render_sg_fwd / _bwd against oracle/octree_oracle.py with the
fixture's lobes, pxo_sg_render_fwd against the fixture-pinned eval_sg restatement over the kernel's own samples, and
checkpoint -> octree.extraction -> octree.evaluation -> octree.optimization end to end.

Bounds are those of the corresponding SH tests, taken over unchanged: colours atol 2e-5 (tests/test_gpu_octree.py: the march
takes identical steps, only exp / sigmoid and the summation order differ; the helper's own float32 round-off against its
float64 compositing of the same samples is 1.5e-7 on these scenes, tests/test_sg_cpu.py), gradients rtol 2e-3 with atol 2e-6 of
the largest entry against float64 autograd; NeRF-SG render rgb / acc atol 2e-5, disp rtol 2e-3
(test_render_fwd_against_reference_nerf_model_call)."""
import os

import numpy as np
import pytest
import torch

import _octree_sg_cases as G
from oracle import nerf_oracle as O
from oracle import octree_oracle as T
from _helpers import _gpu, _psnr, close, make_params

pytestmark = pytest.mark.gpu
f32 = np.float32


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _device_tree(K, dev):
    oops = _oops()
    t = G.tree(K)
    child, data = torch.from_numpy(t.child).to(dev), torch.from_numpy(t.data).to(dev)
    lobes = torch.from_numpy(G.lobes(K)).to(dev)
    return t, oops.tree_view(child, data, t.offset, t.invradius), lobes, (child, data)


def _ropts(oops, fast, bg=1.0):
    o = G.options(fast)
    return oops.render_opts(G.STEP, bg, float(o.sigma_thresh), float(o.stop_thresh))


@pytest.fixture
def lanes_reset():
    yield
    _oops().set_lanes_per_ray(0, 0)


# ---- octree forward -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", G.KS)
def test_sg_octree_forward_matches_the_helper(K, lanes_reset):
    """Every K at 4, 8 and 16 lanes per ray, exact and early-stop options: the 16 x 12 camera view (partial last tile row at
    every lane count) and 37 explicit rays (no multiple of a block's rays; three see only the background)."""
    oops = _oops(); dev = _gpu()
    t, view, lobes, keep = _device_tree(K, dev)
    V = G.VIEW
    c2w = torch.from_numpy(V["c2w"]).to(dev)
    o, d, v = (torch.from_numpy(a).to(dev) for a in G.ray_batch(K))
    for lanes in (4, 8, 16):
        oops.set_lanes_per_ray(lanes, lanes)
        for fast in (False, True):
            got = oops.octree_render_persp(view, c2w, V["W"], V["H"], V["fx"], _ropts(oops, fast), V["fy"], lobes=lobes)
            want = G.want_image(K, fast)
            err = float((got.cpu() - torch.from_numpy(want)).abs().max())
            print(f"SG{K} image, {lanes} lanes, fast={fast}: max err {err:.3g}")
            close(f"SG{K} image, {lanes} lanes, fast={fast}", got, torch.from_numpy(want), rtol=0, atol=2e-5)
            # the SH entry point on the same data is a different image: the dispatch is not vacuous
            assert float((got.cpu() - torch.from_numpy(G.sh_image(K))).abs().max()) > 1e-2
            rays = oops.octree_render_rays(view, o, d, v, _ropts(oops, fast), lobes=lobes)
            close(f"SG{K} rays, {lanes} lanes, fast={fast}", rays, torch.from_numpy(G.want_rays(K, fast)), rtol=0, atol=2e-5)
            assert torch.equal(rays[-3:].cpu(), torch.ones(3, 3))                        # corner, away, miss: background, exactly
    # the SH entry point itself is untouched by the lobes argument being absent
    sh = oops.octree_render_persp(view, c2w, V["W"], V["H"], V["fx"], _ropts(oops, False), V["fy"])
    close(f"SH{K} image of the same data", sh, torch.from_numpy(G.sh_image(K)), rtol=0, atol=2e-5)


def test_sg_octree_argument_checks():
    oops = _oops(); dev = _gpu()
    from plenoctree_amd._lib import PxoError
    t, view, lobes, keep = _device_tree(4, dev)
    o, d, v = (torch.from_numpy(a).to(dev) for a in G.ray_batch(4))
    with pytest.raises(PxoError, match=r"lobes must be a contiguous float32 \[4, 4\]"):
        oops.octree_render_rays(view, o, d, v, _ropts(oops, False), lobes=lobes[:3])
    with pytest.raises(PxoError, match="lobes"):
        oops.octree_render_rays(view, o, d, v, _ropts(oops, False), lobes=lobes.cpu())
    bad = oops.tree_view(keep[0], keep[1], t.offset, t.invradius)
    bad.basis_dim = 3
    with pytest.raises(PxoError, match="SG lobes|not a supported SG format"):
        oops.octree_render_rays(bad, o, d, v, _ropts(oops, False), lobes=lobes)
    grad = torch.zeros_like(keep[1])
    g = torch.ones(o.shape[0], 3, device=dev)
    fwd = oops.octree_render_rays(view, o, d, v, _ropts(oops, True), lobes=lobes)
    with pytest.raises(PxoError, match="pxo_octree_render_sg_bwd: out_rgb must come from an exact march"):
        oops.octree_render_rays_bwd(view, o, d, v, _ropts(oops, True), g, grad, out_rgb=fwd, lobes=lobes)
    assert float(grad.abs().max()) == 0.0


# ---- octree backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 9, 25])
def test_sg_octree_gradient_matches_float64_autograd(K, lanes_reset):
    """grad_data against float64 autograd of the helper on the 37 rays and on the camera view, 4 and 16 lanes, with the forward
    image handed over and without; leaves no sample touches (and leaves with sigma <= 0) keep an exactly zero gradient."""
    oops = _oops(); dev = _gpu()
    t, view, lobes, (child, data) = _device_tree(K, dev)
    opt = G.options(False)
    rs = np.random.RandomState(70 + K)
    o, d, v = G.ray_batch(K)
    V = G.VIEW
    co, cd = T.camera_rays(**V)
    cases = {"rays": (o, d, v, rs.randn(len(o), 3).astype(f32)), "view": (co, cd, cd, rs.randn(len(co), 3).astype(f32))}
    want = {}
    for name, (oo, dd, vv, g) in cases.items():
        x = torch.tensor(t.data.astype(np.float64), requires_grad=True)
        out = T.render_rays_torch(t, x, oo, dd, vv, opt, lobes=G.lobes(K))
        (out * torch.from_numpy(g.astype(np.float64))).sum().backward()
        want[name] = x.grad.float()
        assert float(want[name].abs().max()) > 1e-3
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ropts = _ropts(oops, False)
    c2w = to(V["c2w"])
    for lanes in (4, 16):
        oops.set_lanes_per_ray(lanes, lanes)
        for with_out in (False, True):
            oo, dd, vv, g = cases["rays"]
            fwd = oops.octree_render_rays(view, to(oo), to(dd), to(vv), ropts, lobes=lobes) if with_out else None
            grad = torch.zeros_like(data)
            oops.octree_render_rays_bwd(view, to(oo), to(dd), to(vv), ropts, to(g), grad, out_rgb=fwd, lobes=lobes)
            w = want["rays"]
            close(f"SG{K} d/d data, rays, {lanes} lanes, out_rgb={with_out}", grad, w, rtol=2e-3,
                  atol=2e-6 * float(w.abs().max()) + 1e-7)
            untouched = (w == 0).all(dim=-1)
            assert int(untouched.sum()) > 0 and float(grad.cpu()[untouched].abs().max()) == 0.0
            g = cases["view"][3]
            img = oops.octree_render_persp(view, c2w, V["W"], V["H"], V["fx"], ropts, V["fy"], lobes=lobes) if with_out else None
            grad = torch.zeros_like(data)
            oops.octree_render_persp_bwd(view, c2w, V["W"], V["H"], V["fx"], ropts, to(g).reshape(V["H"], V["W"], 3), grad, V["fy"],
                                         out_rgb=img, lobes=lobes)
            w = want["view"]
            close(f"SG{K} d/d data, view, {lanes} lanes, out_rgb={with_out}", grad, w, rtol=2e-3,
                  atol=2e-6 * float(w.abs().max()) + 1e-7)
            assert float(grad.cpu()[(w == 0).all(dim=-1)].abs().max()) == 0.0


def test_sg_tree_renders_and_backpropagates_through_the_svox_mirror():
    """VolumeRenderer on an SG N3Tree: render_persp / forward dispatch to the SG entry points, autograd reaches tree.data, the
    lobes get no gradient and do not move, and the aux outputs stay refused."""
    oops = _oops(); dev = _gpu()
    from plenoctree_amd.octree import svox
    K = 9
    t = G.tree(K)
    V = G.VIEW
    host = svox.N3Tree(N=2, data_dim=3 * K + 1, depth_limit=5, data_format=f"SG{K}", extra_data=G.lobes(K), radius=[1.0, 2.0, 1.0],
                       center=[0.5, 0.0, 0.5], map_location=dev)
    host.child, host.parent_depth = torch.from_numpy(t.child).to(dev), torch.from_numpy(t.parent_depth).to(dev)
    host.data = torch.nn.Parameter(torch.from_numpy(t.data).to(dev))
    host.level_nodes = [int(c) for c in np.bincount(t.parent_depth[:, 1])]
    host._leaves = None
    assert host.extra_data.device.type == "cuda"
    r = svox.VolumeRenderer(host, step_size=G.STEP)
    c2w = torch.from_numpy(V["c2w"])
    with torch.no_grad():
        im = r.render_persp(c2w, width=V["W"], height=V["H"], fx=V["fx"], fast=False)
        close("svox SG image", im, torch.from_numpy(G.want_image(K, False)), rtol=0, atol=2e-5)
        o, d, v = (torch.from_numpy(a).to(dev) for a in G.ray_batch(K))
        close("svox SG rays", r(o, d, v, fast=True), torch.from_numpy(G.want_rays(K, True)), rtol=0, atol=2e-5)
        with pytest.raises(NotImplementedError, match="SG"):
            r.render_persp_aux(c2w, width=V["W"], height=V["H"], fx=V["fx"])
    gt = torch.rand(V["H"], V["W"], 3, device=dev)
    before = host.extra_data.clone()
    loss = ((r.render_persp(c2w, width=V["W"], height=V["H"], fx=V["fx"], fast=False) - gt) ** 2).mean()
    loss.backward()
    x = torch.tensor(t.data.astype(np.float64), requires_grad=True)
    co, cd = T.camera_rays(**V)
    ref = ((T.render_rays_torch(t, x, co, cd, cd, G.options(False), lobes=G.lobes(K)).reshape(V["H"], V["W"], 3) - gt.cpu().double()) ** 2).mean()
    ref.backward()
    assert abs(float(loss) - float(ref)) < 1e-6
    close("svox SG grad", host.data.grad, x.grad.float(), rtol=2e-3, atol=2e-6 * float(x.grad.abs().max()) + 1e-9)
    assert torch.equal(host.extra_data, before) and host.extra_data.grad is None
    moved = host.to("cpu")
    assert moved.extra_data.device.type == "cpu" and torch.equal(moved.extra_data, before.cpu())


# ---- NeRF-SG ray rendering ------------------------------------------------------------------------------------------
def _sg_shade_f64(raw_rgb, raw_sigma, lobes, viewdirs, z, dirs, white):
    """eval_sg (the fixture-pinned restatement T.sg_basis_f64) -> sigmoid / relu -> oracle volumetric rendering, float64."""
    B, Sn = z.shape
    K = lobes.shape[0]
    basis = torch.from_numpy(T.sg_basis_f64(lobes, viewdirs.numpy()))                       # [B,K]
    pre = (raw_rgb.double().reshape(B, Sn, 3, K) * basis[:, None, None, :]).sum(-1)
    return O.volumetric_rendering(torch.sigmoid(pre), torch.relu(raw_sigma.double().reshape(B, Sn, 1)), z.double(), dirs.double(), white)


# (K, precision, Nc, Nf, B); the fine level of the added sample counts has 63, 65 and 256 samples
_SG_FWD_EDGES = [(K, 0, Nc, Nf, 5) for K in (9, 16) for Nc, Nf in ((20, 43), (20, 45), (128, 128))]
_SG_FWD_CASES = [(25, 0, 64, 128, 24), (4, 0, 64, 128, 24), (25, 2, 64, 128, 24), (1, 0, 64, 128, 24), (9, 0, 64, 128, 24),
                 (16, 0, 64, 128, 24)] + _SG_FWD_EDGES
_SG_FWD_IDS = ["sg25-f32", "sg4-f32", "sg25-bf16x6", "sg1-f32", "sg9-f32", "sg16-f32"] + [f"sg{c[0]}-f32-{c[2]}+{c[3]}-B{c[4]}"
                                                                                          for c in _SG_FWD_EDGES]


@pytest.mark.parametrize("K,precision,Nc,Nf,B", _SG_FWD_CASES, ids=_SG_FWD_IDS)
def test_sg_render_fwd_against_eval_sg_over_the_kernels_own_samples(K, precision, Nc, Nf, B):
    """24 rays, 64 + 128 samples, t_rand / u supplied, every lobe count (shade_composite_fwd_kernel<DEG, true> for DEG 0..4);
    K = 9 and 16 also on 5 rays (a partial ray block) whose fine level has 63 samples (the lane-63 carry without a second
    chunk), 65 (one live row in the second chunk) and 256 (all four chunks).  The raw outputs of pxo_eval_points at the kernel's
    own sample points (pxo_sample_along_rays, then pxo_sample_pdf on the host-composited coarse weights) go through eval_sg and
    the oracle's volumetric rendering in float64."""
    from plenoctree_amd import ops
    dev = _gpu()
    deg = int(round(np.sqrt(K))) - 1
    ocfg = O.Cfg(sh_deg=deg)
    cfg = ops.make_cfg(sh_deg=deg, mlp_precision=precision, num_coarse_samples=Nc, num_fine_samples=Nf)
    flat = make_params(ocfg, seed=20 + K, bias_scale=0.2).to(dev)
    n = flat.numel() // 2
    pk = [ops.pack_weights(cfg, flat[i * n:(i + 1) * n].contiguous(), need_bwd=False)[0] for i in range(2)]
    lobes = torch.from_numpy(G.lobes(K)).to(dev)
    gen = torch.Generator().manual_seed(K)
    cam = torch.randn(B, 3, generator=gen); cam = 4.0 * cam / cam.norm(dim=-1, keepdim=True)
    dirs = 0.5 * (torch.rand(B, 3, generator=gen) - 0.5) - cam
    dirs = dirs / dirs.norm(dim=-1, keepdim=True) * (1.0 + 0.1 * torch.rand(B, 1, generator=gen))
    vdirs = dirs / dirs.norm(dim=-1, keepdim=True)
    t_rand, u = torch.rand(B, Nc, generator=gen), torch.rand(B, Nf, generator=gen)
    o, d, v, t_rand_d, u_d = (x.to(dev).contiguous() for x in (cam, dirs, vdirs, t_rand, u))
    out = ops.render_fwd(cfg, pk[0], pk[1], o, d, v, randomized=True, t_rand=t_rand_d, u=u_d, lobes=lobes)
    sh = ops.render_fwd(cfg, pk[0], pk[1], o, d, v, randomized=True, t_rand=t_rand_d, u=u_d)
    assert float((out[1][0] - sh[1][0]).abs().max()) > 1e-2                     # not the SH shading of the same weights
    z_c, pts = ops.sample_along_rays(o, d, Nc, 2.0, 6.0, t_rand_d)
    raw_rgb, raw_sigma = ops.eval_points(cfg, pk[0], pts.reshape(-1, 3), want_rgb=True)
    rgb_c, disp_c, acc_c, w = _sg_shade_f64(raw_rgb.cpu(), raw_sigma.cpu(), G.lobes(K), vdirs, z_c.cpu(), dirs, True)
    z_f, pts_f = ops.sample_pdf(z_c, w.float().to(dev).contiguous(), o, d, Nf, u_d)
    raw_rgb, raw_sigma = ops.eval_points(cfg, pk[1], pts_f.reshape(-1, 3), want_rgb=True)
    rgb_f, disp_f, acc_f, _ = _sg_shade_f64(raw_rgb.cpu(), raw_sigma.cpu(), G.lobes(K), vdirs, z_f.cpu(), dirs, True)
    assert 0.05 < float(acc_f.mean()) and float(acc_f.min()) < 0.999            # the rays see translucent and empty space
    for lvl, got, want in (("coarse", out[0], (rgb_c, disp_c, acc_c)), ("fine", out[1], (rgb_f, disp_f, acc_f))):
        for name, g, w_, rtol, atol in (("rgb", got[0], want[0], 0, 2e-5), ("acc", got[2], want[2], 0, 2e-5),
                                        ("disp", got[1], want[1], 2e-3, 1e-6)):
            print(f"SG{K} p{precision} {name} {lvl}: max err {float((g.cpu().double() - w_).abs().max()):.3g}")
            close(f"SG{K} {name} {lvl}", g, w_, rtol=rtol, atol=atol)


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_sg_pipeline_end_to_end(tmp_path):
    """SG25 checkpoint (fixed random weights, the fixture's lobes) on the analytic three-sphere scene -> octree.extraction at
    init_grid_depth 5 -> octree.evaluation on a 32 x 32 view -> octree.optimization for one epoch on two 32 x 32 images.

    The tree's render of the test view is held to pxo_sg_render_fwd of the same checkpoint by the PSNR the SH pipeline reaches
    at the same sizes: no SH test asserts such a figure, so the SH pipeline is run here on the SAME MLP weights (read as an SH25
    model), same grid, same samples, same view, and the SG tree may be at most 3 dB (a factor 2 in the mean squared error)
    below it.  Both errors are dominated by what the two runs share -- the density field and its 64^3 discretisation -- and
    the SG basis (<= 1/K) weighs the leaf-averaged coefficients no more than the SH basis does; a dispatch that shades an SG
    tree with SH (or the reverse) changes the image by > 0.1 and falls far below."""
    dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import checkpoints, datasets, families, models, sg, utils
    from plenoctree_amd.octree import evaluation, extraction, optimization, svox
    fx = G.fixture()
    flat = make_params(O.Cfg(sh_deg=4), seed=11, bias_scale=0.2)
    sizes = ["--synthetic_hw", "32", "32", "--synthetic_views", "2", "1"]
    psnr = {}
    for kind in ("sg", "sh"):
        d = os.path.join(str(tmp_path), kind)
        os.makedirs(d)
        cfg_path = os.path.join(d, "tiny.yaml")
        with open(cfg_path, "w") as f:
            f.write("dataset: synthetic\nfactor: 16\nnum_coarse_samples: 64\nnum_fine_samples: 128\nuse_viewdirs: false\n"
                    "white_bkgd: true\nbatch_size: 1024\nsh_deg: 4\nrandomized: true\n")
        common = ["--train_dir", d, "--config", cfg_path, *sizes] + (["--sg_dim", "25", "--sh_deg", "-1"] if kind == "sg" else [])
        args = extraction.define_flags().parse_args(common)
        utils.update_flags(args)
        sg.apply_cli(args, common)
        if kind == "sg":
            assert (args.sg_dim, args.sh_deg) == (25, -1)
            model, state = sg.get_model_state(args, dev)
            state.params.copy_(flat.to(dev)); state.repack()
            state.set_lobe_params(torch.from_numpy(fx["sg_lambda_25"]), torch.from_numpy(fx["sg_mu_spher_25"]))
        else:
            model, params = models.construct_nerf(args, dev)
            state = models.TrainState(model.cfg, flat.to(dev))
        checkpoints.save_checkpoint(d, state, step=0)
        out = os.path.join(d, "tree.npz")
        tree = extraction.main(common + ["--output", out, "--init_grid_depth", "5", "--masking_mode", "sigma", "--samples_per_cell", "8",
                                         "--renderer_step_size", "1e-3", "--eval", "false"])
        assert tree.max_depth == 5 and tree.n_internal > 50 and bool((tree.data[..., -1] >= 0).all())
        loaded = svox.N3Tree.load(out, map_location=dev)
        test = datasets.get_dataset("test", args, dev)
        ex = test.get_image(0)
        nerf_rgb, _, _ = utils.render_image(lambda r: model.apply(state, r, False), ex["rays"], chunk=1024)
        with torch.no_grad():
            im = svox.VolumeRenderer(loaded, step_size=1e-3).render_persp(torch.from_numpy(test.camtoworlds[0]), width=test.w,
                                                                           height=test.h, fx=test.focal, fast=False)
        psnr[kind] = _psnr(im.cpu(), nerf_rgb.reshape(test.h, test.w, 3).cpu())
        assert float((nerf_rgb - 1.0).abs().max()) > 0.2                    # the view sees the model
        if kind == "sh":
            assert str(loaded.data_format) == "SH25" and loaded.extra_data is None
            continue
        # the SG file: format, lobes, leaf data = mean of the network's raw output over the leaf's samples
        assert str(loaded.data_format) == "SG25" and str(tree.data_format) == "SG25"
        assert torch.equal(loaded.extra_data, state.lobes) and torch.equal(tree.extra_data, state.lobes)
        assert torch.equal(state.lobes.cpu(), sg.lobes_from_params(fx["sg_lambda_25"], fx["sg_mu_spher_25"]))
        node0, count = tree.max_depth_nodes()
        pts = tree.sample_max_depth_cells(8, first=0, count=count, seed=args.seed)
        rgb, sigma = model.eval_points_raw(state, pts.view(-1, 3))
        want = torch.cat([rgb, sigma], -1).reshape(-1, 8, 76).mean(1)
        want[:, -1].clamp_(min=0)
        # chunk boundaries reuse stream ids per `first`, so compare the first chunk only (as the SH pipeline test does)
        close("SG leaf data", tree.max_depth_data()[: 64 * 8], want[: 64 * 8], rtol=1e-5, atol=1e-6)
        # the flax file is read back by the CLI's own restore (both SG keys), and the evaluation CLI scores the tree
        _, again = families.restore(args, dev, "extract", say=lambda *a, **k: None)
        assert torch.equal(again.lobes, state.lobes) and torch.equal(again.params, state.params)
        ev = evaluation.main(common + ["--input", out, "--renderer_step_size", "1e-3"])
        assert np.isfinite(ev)
        for flag, extra in (("--keep_compressed", []), ("--write_aux", [os.path.join(d, "aux")])):
            with pytest.raises(NotImplementedError, match="SG"):
                evaluation.main(common + ["--input", out, flag] + extra)
        # one epoch of fine-tuning on the two training images: the CLI runs, and the training loss does not go up
        opt_args = ["--input", out, "--output", os.path.join(d, "tree_opt.npz"), "--num_epochs", "1", "--val_interval", "1",
                    "--renderer_step_size", "1e-3", "--lr", "5e3", "--continue_on_decrease"]
        hist = optimization.main(common + opt_args)
        assert len(hist) == 2 and all(np.isfinite(h[2]) for h in hist) and np.isfinite(hist[1][1])
        train = datasets.get_dataset("train", args, dev)
        c2ws = torch.from_numpy(np.ascontiguousarray(train.camtoworlds)).float().to(dev)
        gts = [train.get_image(i)["pixels"].contiguous() for i in range(train.size)]
        assert len(gts) == 2 and tuple(gts[0].shape) == (32, 32, 3)

        def train_loss(tr):
            r = svox.VolumeRenderer(tr, step_size=1e-3)
            with torch.no_grad():
                return sum(float(((r.render_persp(c2ws[j], width=32, height=32, fx=train.focal, fast=False).clamp(0, 1) - gts[j]) ** 2)
                                 .mean()) for j in range(2)) / 2

        tuned = svox.N3Tree.load(out, map_location=dev)
        loss0 = train_loss(tuned)
        oargs = optimization.define_flags().parse_args(common + opt_args)
        utils.update_flags(oargs)
        from plenoctree_amd import dist
        optimization.fit(oargs, tuned, (c2ws, gts), (c2ws, gts), 32, 32, train.focal, dist.Comm(), say=lambda *a, **k: None)
        loss1 = train_loss(tuned)
        print(f"SG25 fine-tuning: training loss {loss0:.6g} -> {loss1:.6g}")
        assert loss1 <= loss0, (loss0, loss1)
        assert torch.equal(tuned.extra_data, state.lobes)                    # the lobes are not optimised
        tuned.save(os.path.join(d, "tuned.npz"), compress=False)
        assert str(svox.N3Tree.load(os.path.join(d, "tuned.npz")).data_format) == "SG25"
    print(f"tree vs NeRF render, 32 x 32 view, depth 5: SG25 {psnr['sg']:.2f} dB, SH25 {psnr['sh']:.2f} dB")
    assert psnr["sg"] >= psnr["sh"] - 3.0, psnr
