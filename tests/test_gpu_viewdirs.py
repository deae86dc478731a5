"""The view-conditioned NeRF head and its fused SH projection on the GPU, against the float64 fixture of the reference's torch twin
(tests/golden/viewdirs_projection.npz).  Bounds: max |HIP - float64| <= 4 x floor, floor = the reference's own measured
float32 deviation from float64 for that quantity; the factor 4 covers a different summation order over the 256..283-term and
R-term sums."""
import os
import time

import numpy as np
import pytest
import torch

from _viewdirs_helpers import fixture, host_model_f64, host_project_f64, seeded_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from plenoctree_amd import ops
    from plenoctree_amd.nerf_sh.nerf import checkpoints, viewdirs
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    fx = fixture()
    sd = seeded_state_dict(fx)
    flat = checkpoints.vd_tree_to_arena(checkpoints.vd_torch_state_dict_to_tree(sd))
    state = viewdirs.ViewdirsState(torch.from_numpy(flat).to(dev))
    model = viewdirs.ViewdirsModel()
    return dict(ops=ops, dev=dev, fx=fx, sd=sd, state=state, model=model, flat=flat,
                pts=torch.from_numpy(fx["points"]).to(dev), dirs=torch.from_numpy(fx["dirs"]).to(dev))


def _check(name, got, want, bound):
    err = float(np.abs(got.detach().cpu().double().numpy() - np.asarray(want, np.float64)).max())
    print(f"{name}: max |HIP - f64| = {err:.3e}, bound {bound:.3e} ({err / bound * 4:.2f} x floor)")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"


@pytest.mark.timeout(60)
def test_eval_points_raw_against_the_float64_twin(ctx):
    fx, m, st = ctx["fx"], ctx["model"], ctx["state"]
    rgb, sigma = m.eval_points_raw(st, ctx["pts"], ctx["dirs"], cross_broadcast=True)
    assert rgb.shape == (40, 256, 3) and sigma.shape == (40, 1)
    _check("raw_rgb cross", rgb, fx["rgb_cross"], 4 * float(fx["floor_rgb_cross"]))
    _check("raw_sigma", sigma.view(-1), fx["sigma"], 4 * float(fx["floor_sigma"]))
    rgbp, sigp = m.eval_points_raw(st, ctx["pts"], ctx["dirs"][:40].contiguous())
    assert rgbp.shape == (40, 3)
    _check("raw_rgb per point", rgbp, fx["rgb_point"], 4 * float(fx["floor_rgb_point"]))
    assert torch.equal(sigp, sigma)
    none, sig0 = m.eval_points_raw(st, ctx["pts"])
    assert none is None and torch.equal(sig0, sigma)
    # the coarse MLP is MLP_0
    _, sc = m.eval_points_raw(st, ctx["pts"], coarse=True)
    _, want = host_model_f64(ctx["sd"], ctx["pts"].cpu(), mlp=0)
    _check("raw_sigma coarse", sc.view(-1), want.numpy(), 4 * float(fx["floor_sigma"]))


@pytest.mark.timeout(60)
@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_fused_projection_against_the_float64_twin(ctx, deg):
    fx, m, st = ctx["fx"], ctx["model"], ctx["state"]
    co, sigma = m.project_sh(st, ctx["pts"], ctx["dirs"], deg)
    assert co.shape == (40, 3 * (deg + 1) ** 2)
    bound = 4 * float(fx[f"floor_coeffs_{deg}"])
    _check(f"coeffs SH{(deg + 1) ** 2}", co, fx[f"coeffs_{deg}"], bound)
    # == eval_points_raw(cross_broadcast) followed by the SH sum in float64 on the host; sigma bit-equal
    rgb, sig_e = m.eval_points_raw(st, ctx["pts"], ctx["dirs"], cross_broadcast=True)
    _check("coeffs vs host sum of the HIP raw_rgb", co, host_project_f64(rgb.cpu(), ctx["dirs"].cpu(), deg).numpy(), bound)
    assert torch.equal(sigma, sig_e.view(-1))


@pytest.mark.timeout(60)
def test_grid_sigma_serves_the_view_conditioned_model(ctx):
    """Step 1 / auto-scale reuse pxo_grid_sigma on the image's leading SH-degree-0 part; it forms its coordinates in the kernel,
    so the comparison is to the float64 model at the grid's own points, not bit equality."""
    from plenoctree_amd.octree import extraction
    fx, m, st = ctx["fx"], ctx["model"], ctx["state"]
    reso = 8
    sig = extraction.grid_sigma(m, st, reso, [0.0, 0.0, 0.0], [1.5, 1.5, 1.5])
    # the grid's own points: the kernel's float32 arithmetic ((i + .5) / reso - offset) / scale, then exact in float64
    arr = (torch.arange(reso, dtype=torch.float32) + 0.5) / torch.tensor(float(reso), dtype=torch.float32)
    offset, scale = extraction.tree_transform([0.0] * 3, [1.5] * 3)
    axes = [(arr - torch.tensor(np.float32(offset[a]))) / torch.tensor(np.float32(scale[a])) for a in range(3)]
    assert all(a.dtype == torch.float32 for a in axes)
    g = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    _, want = host_model_f64(ctx["sd"], g)
    scale_up = max(1.0, float(want.abs().max()) / float(np.abs(fx["sigma"]).max()))
    _check("grid sigma", sig, want.numpy(), 4 * float(fx["floor_sigma"]) * scale_up)
    _, sig_pts = m.eval_points_raw(st, g.to(ctx["dev"]))
    _check("grid sigma vs eval_points_raw", sig, sig_pts.view(-1).cpu().double().numpy(), 4 * float(fx["floor_sigma"]) * scale_up)


@pytest.mark.timeout(120)
def test_a_points_coefficients_do_not_depend_on_its_batch(ctx):
    m, st, dev = ctx["model"], ctx["state"], ctx["dev"]
    g = torch.Generator().manual_seed(9)
    pts = ((torch.rand(1000, 3, generator=g) * 2 - 1) * 1.5).to(dev)
    u, v = torch.rand(1000, generator=g), torch.rand(1000, generator=g)
    from plenoctree_amd.nerf_sh.nerf import viewdirs
    dirs_all = viewdirs.sphere_directions(u, v).to(dev)
    for R in (1, 63, 64, 65, 1000):
        dirs = dirs_all[:R].contiguous()
        full, sig_full = m.project_sh(st, pts, dirs, 2)
        assert bool(torch.isfinite(full).all())
        for N in (1, 127, 128, 129, 1000):
            part, sig = m.project_sh(st, pts[:N].contiguous(), dirs, 2)
            assert torch.equal(part, full[:N]) and torch.equal(sig, sig_full[:N]), (R, N)
        alone, _ = m.project_sh(st, pts[500:501].contiguous(), dirs, 2)            # a point from the middle, alone
        assert torch.equal(alone[0], full[500]), R
        a, _ = m.project_sh(st, pts[:333].contiguous(), dirs, 2)                  # split over two calls
        b, _ = m.project_sh(st, pts[333:].contiguous(), dirs, 2)
        assert torch.equal(torch.cat([a, b]), full), R
    # R = 1: the projection of one direction is its raw colour times the basis
    rgb, _ = m.eval_points_raw(st, pts[:5].contiguous(), dirs_all[:1].contiguous(), cross_broadcast=True)
    co, _ = m.project_sh(st, pts[:5].contiguous(), dirs_all[:1].contiguous(), 1)
    want = host_project_f64(rgb.cpu(), dirs_all[:1].cpu(), 1)
    assert float((co.cpu().double() - want).abs().max()) < 1e-5


@pytest.mark.timeout(60)
def test_error_paths(ctx):
    import ctypes
    from plenoctree_amd import _lib
    lib = _lib.load()
    ops, st = ctx["ops"], ctx["state"]
    for prec in (_lib.MLP_BF16X3, _lib.MLP_BF16X6):
        with pytest.raises(_lib.PxoError, match=r"\(-4\)"):
            ops.vd_project_sh(st.packed[1][0], ctx["pts"], ctx["dirs"], 2, mlp_precision=prec)
        with pytest.raises(_lib.PxoError, match=r"\(-4\)"):
            ops.vd_eval_points_raw(st.packed[1][0], ctx["pts"], ctx["dirs"], True, mlp_precision=prec)
    with pytest.raises(_lib.PxoError, match=r"\(-1\).*sh_deg"):
        ops.vd_project_sh(st.packed[1][0], ctx["pts"], ctx["dirs"], 5)
    assert b"sh_deg" in lib.pxo_last_error()
    # N = 0 returns 0 without touching a pointer; a short workspace is refused
    assert lib.pxo_vd_project_sh(0, None, None, 0, None, 256, 2, None, None, None, 0, None) == 0
    assert lib.pxo_vd_eval_points_raw(0, None, None, 0, None, 0, 1, None, None, None, 0, None) == 0
    ws = torch.empty(1024, dtype=torch.uint8, device=ctx["dev"])
    co = torch.empty(40, 27, device=ctx["dev"]); sg = torch.empty(40, device=ctx["dev"])
    rc = lib.pxo_vd_project_sh(0, ctypes.c_void_p(st.packed[1][0].data_ptr()), ctypes.c_void_p(ctx["pts"].data_ptr()), 40,
                               ctypes.c_void_p(ctx["dirs"].data_ptr()), 256, 2, ctypes.c_void_p(co.data_ptr()),
                               ctypes.c_void_p(sg.data_ptr()), ctypes.c_void_p(ws.data_ptr()), 1024, None)
    assert rc == -3


@pytest.mark.timeout(300)
def test_extraction_end_to_end(ctx, tmp_path):
    from plenoctree_amd.nerf_sh.nerf import checkpoints
    from plenoctree_amd.octree import extraction, svox
    fx, dev = ctx["fx"], ctx["dev"]
    # a seeded model with a density field that crosses the mask threshold: the fixture's weights with a raised sigma bias
    sd = {k: v.clone() for k, v in ctx["sd"].items()}
    for mi in range(2):
        sd[f"MLP_{mi}.sigma_layer.bias"] += 4.0
    torch.save({"model": sd}, os.path.join(str(tmp_path), "model.ckpt"))
    out = os.path.join(str(tmp_path), "tree.npz")
    argv = ["--train_dir", str(tmp_path), "--use_viewdirs", "true", "--sh_deg", "2", "--projection_samples", "256",
            "--masking_mode", "sigma", "--init_grid_depth", "5", "--dataset", "synthetic", "--factor", "16", "--eval", "false", "--output", out]
    t0 = time.time()
    tree = extraction.main(argv + ["--chunk", "128"], record_projection=True)
    print(f"extraction: {time.time() - t0:.1f} s, {tree.n_internal} internal nodes")
    assert tree.max_depth == 5 and tree.data_dim == 28 and tree.data_format.format == tree.data_format.SH
    rec = tree.projection_record
    dirs = rec["dirs"]
    assert dirs.shape == (256, 3)
    # >= 200 leaves: stored row == float64 restatement (trunk, head, SH sum, mean over the cell's samples, relu on sigma)
    n0, cnt, pts = rec["points"][0]
    S = 8
    cells = min(cnt * 8, 200)
    assert cells >= 200
    p = pts[: cells * S]
    rgb, sigma = host_model_f64(sd, p, dirs, cross=True)
    co = host_project_f64(rgb, dirs, 2)
    want = torch.cat([co, sigma[:, None]], -1).reshape(cells, S, 28).mean(1)
    want[:, -1].clamp_(min=0)
    got = tree.max_depth_data()[n0 * 8: n0 * 8 + cells].cpu().double()
    rng = max(1.0, float(co.abs().max()) / float(np.abs(fx["coeffs_2"]).max()))
    rng_s = max(1.0, float(sigma.abs().max()) / float(np.abs(fx["sigma"]).max()))
    _check("leaf coefficients", got[:, :-1], want[:, :-1].numpy(), 4 * float(fx["floor_coeffs_2"]) * rng)
    _check("leaf sigma", got[:, -1], want[:, -1].numpy(), 4 * float(fx["floor_sigma"]) * rng_s)
    # the file loads and renders through the octree renderer
    loaded = svox.N3Tree.load(out, map_location=dev)
    assert torch.equal(loaded.child, tree.child)
    assert torch.equal(loaded.data.data, tree.data.data.half().float())          # the file keeps `data` in half precision
    from plenoctree_amd.nerf_sh.nerf import utils
    c2w = torch.from_numpy(utils.pose_spherical(30.0, -30.0, 4.0))
    im = svox.VolumeRenderer(loaded, step_size=1e-3).render_persp(c2w, width=100, height=100, fx=110.0)
    assert im.shape[:2] == (100, 100) and bool(torch.isfinite(im).all())
    # half the chunk: the same tree, bit for bit
    tree2 = extraction.main(argv[:-1] + [os.path.join(str(tmp_path), "tree2.npz"), "--chunk", "64"])
    assert torch.equal(tree2.child, tree.child) and torch.equal(tree2.data.data, tree.data.data)
