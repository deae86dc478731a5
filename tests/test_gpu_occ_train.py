"""Training through the occupancy grid on the MI355X: pxo_occ_gather against its numpy restatement bit for bit; the culled train
step (pxo_train_fwd_bwd_culled) against the dense step bit for bit when every sample is live, against a float64 restatement of the
masked loss (tests/_occ_train_ref.py) and a twin composed from the per-stage entry points when a real mask culls; its refusals;
and occupancy.TrainingGrid / nerf_sh.train --cull_reso end to end."""
import os

import numpy as np
import pytest
import torch

import _occ_train_ref as T
import _occupancy_ref as R
from _helpers import _gpu, _ops, close, make_params, make_rays, pxo_cfg, split_mlp
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

BLOCK = 256                                       # elements a lane strides by in the expand / gather kernels
M_SET = (0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17)
RESO, OFFSET, SCALE = 4, [0.5] * 3, [0.25] * 3    # the box [-2, 2)^3 in 4 cells per axis (tests/test_gpu_occupancy.py)
B, NC, NF, DEG = 37, 8, 16, 2                     # 296 and 888 (+16) rows: ragged against the 128-row tile, the 32-row split, the 16-row chunk
N_SP = 16


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- gather ---------------------------------------------------------------------------------------------------------------------
def gather_ref(d_rgb, d_sigma, slot, rgb_live, sigma_live):
    """pxo_occ_gather as the header states it, on copies of the pre-filled outputs."""
    rgb_live, sigma_live = rgb_live.copy(), sigma_live.copy()
    M = slot.size
    for m in range(M):
        s = int(slot[m])
        if 0 <= s < M:
            rgb_live[s] = d_rgb[m]
            sigma_live[s] = d_sigma[m]
    return rgb_live, sigma_live


def _slots(pattern, M, rs):
    m = np.arange(M)
    if pattern == "all_live":
        live = np.ones(M, bool)
    elif pattern == "none":
        live = np.zeros(M, bool)
    elif pattern == "alternating":
        live = m % 2 == 0
    else:                                                         # "last_block"
        live = m >= (max(M - 1, 0) // BLOCK) * BLOCK
    return np.where(live, np.cumsum(live) - 1, -1).astype(np.int32), int(live.sum())


@pytest.mark.parametrize("pattern", ["all_live", "none", "alternating", "last_block"])
@pytest.mark.parametrize("C", [3, 75, 5])             # 5: a width that is no SH head's, the kernel's general form
@pytest.mark.parametrize("M", M_SET)
def test_gather(M, C, pattern):
    dev, ops = _gpu(), _ops()
    rs = np.random.RandomState(13 * M + C)
    slot, n = _slots(pattern, M, rs)
    d_rgb = rs.randn(M, C).astype(np.float32)
    d_sigma = rs.randn(M).astype(np.float32)
    pre_rgb = np.full((M, C), np.nan, np.float32)
    pre_sigma = np.full(M, np.nan, np.float32)
    want_rgb, want_sigma = gather_ref(d_rgb, d_sigma, slot, pre_rgb, pre_sigma)
    outs = []
    for _ in range(2):                                            # two calls: the same bits
        got_rgb, got_sigma = torch.from_numpy(pre_rgb).to(dev), torch.from_numpy(pre_sigma).to(dev)
        r = ops.occ_gather(torch.from_numpy(d_rgb).to(dev), torch.from_numpy(d_sigma).to(dev), torch.from_numpy(slot).to(dev),
                           got_rgb, got_sigma)
        assert r[0] is got_rgb and r[1] is got_sigma
        outs.append((got_rgb.cpu().numpy(), got_sigma.cpu().numpy()))
    for got_rgb, got_sigma in outs:
        assert np.array_equal(got_rgb.view(np.uint32), want_rgb.view(np.uint32))
        assert np.array_equal(got_sigma.view(np.uint32), want_sigma.view(np.uint32))
        assert not np.isnan(got_rgb[:n]).any() and not np.isnan(got_sigma[:n]).any()     # every compact element written
        assert np.isnan(got_rgb[n:]).all() and np.isnan(got_sigma[n:]).all()             # rows >= n_live untouched


def test_gather_is_the_inverse_of_expand():
    dev, ops = _gpu(), _ops()
    M, C = 3 * BLOCK + 17, 27
    rs = np.random.RandomState(1)
    live = rs.rand(M) < 0.4
    slot = torch.from_numpy(np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)).to(dev)
    n = int(live.sum())
    rgb_live = torch.from_numpy(rs.randn(n, C).astype(np.float32)).to(dev)
    sigma_live = torch.from_numpy(rs.randn(n).astype(np.float32)).to(dev)
    rgb, sigma = ops.occ_expand(rgb_live, sigma_live, slot, C)
    back_rgb, back_sigma = ops.occ_gather(rgb, sigma, slot)
    assert torch.equal(back_rgb[:n], rgb_live) and torch.equal(back_sigma[:n], sigma_live)


# ---- the culled train step ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    dev, ops = _gpu(), _ops()
    ocfg = O.Cfg(num_coarse_samples=NC, num_fine_samples=NF, sh_deg=DEG, sparsity_npoints=N_SP)
    flat = make_params(ocfg, seed=3)
    rays = make_rays(B, seed=5)
    gen = torch.Generator().manual_seed(9)
    px = torch.rand(B, 3, generator=gen)
    t_rand = torch.rand(B, NC, generator=gen)
    u = torch.rand(B, NF, generator=gen)
    sp = (torch.rand(N_SP, 3, generator=gen) * 2 - 1) * ocfg.sparsity_radius
    fd = flat.to(dev)
    packed = {}

    def images(pcfg):
        if pcfg.mlp_precision not in packed:
            packed[pcfg.mlp_precision] = [ops.pack_weights(pcfg, split_mlp(fd, ocfg, i)) for i in range(2)]
        return packed[pcfg.mlp_precision]
    o, d, v = (x.to(dev).contiguous() for x in rays)
    return dict(dev=dev, ops=ops, ocfg=ocfg, flat=flat, fd=fd, rays=rays, o=o, d=d, v=v, px=px, pxd=px.to(dev), t_rand=t_rand.to(dev),
                u=u.to(dev), sp=sp, spd=sp.to(dev), images=images, ref={})


def _pcfg(scene, precision=0, skip=0, wd=0.0, n_sp=N_SP):
    pcfg = pxo_cfg(scene["ops"], scene["ocfg"])
    pcfg.mlp_precision, pcfg.skip_zero_rows, pcfg.weight_decay_mult, pcfg.sparsity_npoints = precision, skip, wd, n_sp
    return pcfg


def _grid(scene, mask, outside_live, offset=OFFSET, scale=SCALE):
    bits = torch.from_numpy(R.bits_from_mask(mask)).to(scene["dev"])
    return scene["ops"].OccupancyGrid(bits, RESO, offset, scale, outside_live=bool(outside_live))


def _all_live_grid(scene):
    # a box of half side 8 holds every sample (the rays start 4 from the origin and end at most 6.6 further on)
    return _grid(scene, np.ones((RESO, RESO, RESO), bool), 1, offset=[0.5] * 3, scale=[1.0 / 16] * 3)


def _masks():
    half = np.zeros((RESO, RESO, RESO), bool)
    half[:2] = True                                               # the half space x < 0
    x, y, z = np.meshgrid(*[np.arange(RESO)] * 3, indexing="ij")
    return {"half_space": half, "checkerboard": (x + y + z) % 2 == 0}


def _draws(scene, pcfg, randomized):
    return dict(randomized=randomized, t_rand=scene["t_rand"] if randomized else None, u=scene["u"] if randomized else None,
                sp_points=scene["spd"][:pcfg.sparsity_npoints].contiguous() if pcfg.sparsity_npoints else None)


def _step(scene, pcfg, grid, randomized=False, ws=None, poison=0xFF, images=None):
    """One step: through the grid, or (grid None) the dense entry point.  A fresh workspace is filled with `poison` bytes (0xFF: every
    float a NaN, every count and slot -1)."""
    ops, dev = scene["ops"], scene["dev"]
    grads = torch.full_like(scene["fd"], float("nan"))
    stats = torch.full((6,), float("nan"), device=dev)
    rows = []
    if ws is None:
        nbytes = ops.train_workspace_bytes(pcfg, B) if grid is None else ops.train_culled_workspace_bytes(pcfg, B)
        ws = torch.full((nbytes,), poison, dtype=torch.uint8, device=dev)
    args = (scene["fd"], images or scene["images"](pcfg), scene["o"], scene["d"], scene["v"], scene["pxd"], grads, stats, ws)
    if grid is None:
        ops.train_fwd_bwd(pcfg, *args, **_draws(scene, pcfg, randomized))
    else:
        ops.train_fwd_bwd_culled(pcfg, grid, *args, live_rows=rows, **_draws(scene, pcfg, randomized))
    return grads, stats, rows, ws


@pytest.mark.parametrize("randomized", [False, True])
@pytest.mark.parametrize("n_sp", [N_SP, 0])
@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("precision", [0, 2])
def test_every_sample_live_is_the_dense_step(scene, precision, skip, wd, n_sp, randomized):
    """The compact rows are the dense rows in the dense order, the sparsity points behind them, and the weight-gradient split of
    the compact M is the dense one: the same launches on the same values, so gradients and stats are the dense step's bits."""
    pcfg = _pcfg(scene, precision, skip, wd, n_sp)
    assert scene["ops"].train_culled_workspace_bytes(pcfg, B) > scene["ops"].train_workspace_bytes(pcfg, B)
    want_g, want_s, _, _ = _step(scene, pcfg, None, randomized)
    got_g, got_s, rows, _ = _step(scene, pcfg, _all_live_grid(scene), randomized)
    assert rows == [B * NC, B * (NC + NF)]
    assert torch.isfinite(want_g).all() and torch.isfinite(want_s).all() and float(want_g.abs().max()) > 0
    assert torch.equal(_bits(got_s), _bits(want_s)), (got_s.tolist(), want_s.tolist())
    assert torch.equal(_bits(got_g), _bits(want_g)), int((got_g != want_g).sum())


def _twin(scene, pcfg, mask, outside_live):
    """The culled step composed from the existing per-stage entry points on ALL rows: mlp_fwd(save=True), culled rows of raw_* zeroed,
    shade_composite_train, culled rows of d_raw_* zeroed, mlp_bwd_data, mlp_bwd_weights.  Returns (grads, z_c, z_f, live_c, live_f):
    the positions and the numpy rule's masks are what the float64 restatement is evaluated at."""
    ops, dev, ocfg = scene["ops"], scene["dev"], scene["ocfg"]
    o, d, v = scene["o"], scene["d"], scene["v"]
    bits = R.bits_from_mask(mask)
    n_sp = pcfg.sparsity_npoints
    n_all = scene["fd"].numel()
    wd_coef = np.float32(2.0) * np.float32(pcfg.weight_decay_mult) / np.float32(n_all)
    z, pts = ops.sample_along_rays(o, d, NC, pcfg.near_, pcfg.far_)
    grads, zs, lives = [], [], []
    for level in range(2):
        f, b = scene["images"](pcfg)[level]
        live = torch.from_numpy(R.live_mask(bits, RESO, OFFSET, SCALE, outside_live, pts.reshape(-1, 3).cpu().numpy())).to(dev)
        extra = n_sp if level == 1 else 0
        rows = pts.reshape(-1, 3)
        if extra:
            rows = torch.cat([rows, scene["spd"][:n_sp]]).contiguous()
            live_all = torch.cat([live, torch.ones(n_sp, dtype=torch.bool, device=dev)])
        else:
            live_all = live
        rgb, sigma, (acts, enc, relu) = ops.mlp_fwd(pcfg, f, rows, save=True)
        rgb[~live_all] = 0.0
        sigma[~live_all] = 0.0
        out = ops.shade_composite_train(pcfg, rgb, sigma, z, d, v, scene["pxd"], n_sp=extra)
        d_rgb, d_sigma = out["d_raw_rgb"], out["d_raw_sigma"]
        d_rgb[~live_all] = 0.0
        d_sigma[~live_all] = 0.0
        dz, dbias = ops.mlp_bwd_data(pcfg, b, d_rgb, d_sigma, relu)
        g = ops.mlp_bwd_weights(pcfg, acts, enc, dz, d_rgb, d_sigma, dbias)
        grads.append(g + float(wd_coef) * split_mlp(scene["fd"], ocfg, level))
        zs.append(z)
        lives.append(live.reshape(z.shape))
        if level == 0:
            z, pts = ops.sample_pdf(z, out["weights"], o, d, NF)
    return torch.cat(grads), zs[0], zs[1], lives[0], lives[1]


ACCURACY_CASES = [("half_space", 0, 0, N_SP), ("half_space", 1, 0, N_SP), ("checkerboard", 0, 0, N_SP), ("checkerboard", 1, 0, N_SP),
                  ("half_space", 0, 0, 0), ("checkerboard", 1, 2, N_SP)]


@pytest.mark.parametrize("mask_name, outside_live, precision, n_sp", ACCURACY_CASES)
def test_real_mask_against_the_float64_restatement(scene, mask_name, outside_live, precision, n_sp):
    """Measured on the MI355X (relative L2 error of the gradient against float64: culled step / per-stage twin), see
    profiles/EXPERIMENTS.md "Training through the occupancy grid"."""
    pcfg = _pcfg(scene, precision, skip=1, wd=0.05, n_sp=n_sp)
    ocfg = O.Cfg(num_coarse_samples=NC, num_fine_samples=NF, sh_deg=DEG, sparsity_npoints=n_sp, weight_decay_mult=0.05)
    mask = _masks()[mask_name]
    g_twin, z_c, z_f, live_c, live_f = _twin(scene, pcfg, mask, outside_live)
    want_rows = [int(live_c.sum()), int(live_f.sum())]
    got_g, got_s, rows, _ = _step(scene, pcfg, _grid(scene, mask, outside_live))
    assert rows == want_rows                                      # the live rows are the numpy rule's
    assert 0 < rows[0] < B * NC and 0 < rows[1] < B * (NC + NF), rows
    st, g_ref = T.masked_loss_and_grad(scene["flat"], scene["rays"], scene["px"], ocfg, z_c, z_f, live_c, live_f,
                                       scene["sp"][:n_sp] if n_sp else None)
    for i, k in enumerate(T.STAT_NAMES):
        print(f"stats/{k}: got {float(got_s[i]):.8g} want {st[k]:.8g}")
        close(f"stats/{k}", got_s.cpu()[i], torch.tensor(st[k]), rtol=3e-4, atol=2e-6)
    norm = float(g_ref.norm())
    assert norm > 0
    e_culled = float((got_g.cpu().double() - g_ref).norm()) / norm
    e_twin = float((g_twin.cpu().double() - g_ref).norm()) / norm
    print(f"{mask_name} outside_live {outside_live} precision {precision} n_sp {n_sp}: live rows {rows}, "
          f"e_culled {e_culled:.4g} e_twin {e_twin:.4g} ratio {e_culled / e_twin:.3f}")
    # the same float32 terms summed in another row order (forward rows bit-identical, so relu flips are shared): margin 1.5;
    # 2e-3 is the project's kink-flip bound (tests/test_gpu_parity.py)
    assert e_culled <= 1.5 * e_twin
    assert e_culled < 2e-3


@pytest.mark.parametrize("outside_live", [0, 1])
@pytest.mark.parametrize("mask_name", ["half_space", "checkerboard"])
def test_real_mask_two_calls_give_the_same_bits(scene, mask_name, outside_live):
    pcfg = _pcfg(scene, skip=1, wd=0.05)
    grid = _grid(scene, _masks()[mask_name], outside_live)
    g1, s1, r1, _ = _step(scene, pcfg, grid, randomized=True)
    g2, s2, r2, _ = _step(scene, pcfg, grid, randomized=True)
    assert r1 == r2 and torch.isfinite(g1).all() and torch.isfinite(s1).all()
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(s1), _bits(s2))


@pytest.mark.parametrize("precision, skip", [(0, 0), (0, 1), (2, 1)])
def test_stale_compact_rows_are_never_read(scene, precision, skip):
    """A step with every row live, then one with a real mask on the same workspace: the second step's compact arrays still hold
    the first step's rows behind its own n_live.  Its bits are those of the same step on a fresh, NaN-poisoned workspace."""
    pcfg = _pcfg(scene, precision, skip, wd=0.05)
    masks = _masks()
    _, _, rows1, ws = _step(scene, pcfg, _all_live_grid(scene))
    second = _grid(scene, masks["half_space"], 0)
    g_a, s_a, rows_a, _ = _step(scene, pcfg, second, ws=ws)
    g_b, s_b, rows_b, _ = _step(scene, pcfg, second)
    assert rows_a == rows_b and rows_a[0] < rows1[0] and rows_a[1] < rows1[1]
    assert torch.isfinite(g_b).all() and torch.isfinite(s_b).all()
    assert torch.equal(_bits(g_a), _bits(g_b)) and torch.equal(_bits(s_a), _bits(s_b))
    # and with another real mask before it
    _, _, _, ws = _step(scene, pcfg, _grid(scene, masks["checkerboard"], 1))
    g_c, s_c, _, _ = _step(scene, pcfg, second, ws=ws)
    assert torch.equal(_bits(g_c), _bits(g_b)) and torch.equal(_bits(s_c), _bits(s_b))


@pytest.mark.parametrize("n_sp", [0, N_SP])
def test_all_empty_grid(scene, n_sp):
    ops, dev = scene["ops"], scene["dev"]
    pcfg = _pcfg(scene, skip=1, wd=0.05, n_sp=n_sp)
    grid = _grid(scene, np.zeros((RESO, RESO, RESO), bool), 0)
    torch.cuda.synchronize()
    ops.profile_enable(tags=[ops.PROF_MLP_FWD, ops.PROF_MLP_BWD_DATA])
    try:
        ops.profile_read(ops.PROF_MLP_FWD)
        ops.profile_read(ops.PROF_MLP_BWD_DATA)
        g, s, rows, _ = _step(scene, pcfg, grid)
        fwd, _, fwd_rows = ops.profile_read(ops.PROF_MLP_FWD)
        bwd, _, bwd_rows = ops.profile_read(ops.PROF_MLP_BWD_DATA)
    finally:
        ops.profile_enable(False)
    assert rows == [0, 0]
    assert torch.isfinite(s).all(), s.tolist()
    n_mlp = g.numel() // 2
    coef = np.float32(2.0) * np.float32(0.05) / np.float32(g.numel())
    decay = scene["fd"] * torch.tensor(coef, device=dev)
    assert torch.equal(g[:n_mlp], decay[:n_mlp])                  # the coarse level: the fill plus the weight-decay term
    if n_sp == 0:
        assert fwd == 0 and bwd == 0                              # no MLP launch at all
        assert torch.equal(g, decay)
    else:
        assert (fwd, fwd_rows) == (1, n_sp) and (bwd, bwd_rows) == (1, n_sp)       # the fine level, on the sparsity points only
        assert torch.isfinite(g).all() and not torch.equal(g[n_mlp:], decay[n_mlp:])


def test_refusals(scene):
    ops = scene["ops"]
    grid = _grid(scene, _masks()["half_space"], 0)
    pcfg = _pcfg(scene)
    pcfg.noise_std = 0.5
    with pytest.raises(ops.PxoError, match="resurrect"):
        _step(scene, pcfg, grid, randomized=True)
    _step(scene, pcfg, grid, randomized=False)                    # noise is off without randomized: fine
    with pytest.raises(ops.PxoError, match="bf16x3"):
        _step(scene, _pcfg(scene, precision=1), grid, images=scene["images"](_pcfg(scene)))      # refused before any image is read
    pcfg = _pcfg(scene)
    with pytest.raises(ops.PxoError, match="occ is NULL"):
        g = torch.zeros_like(scene["fd"])
        ws = torch.zeros(ops.train_culled_workspace_bytes(pcfg, B), dtype=torch.uint8, device=scene["dev"])
        ops.train_fwd_bwd_culled(pcfg, None, scene["fd"], scene["images"](pcfg), scene["o"], scene["d"], scene["v"], scene["pxd"], g,
                                 torch.zeros(6, device=scene["dev"]), ws)
    small = torch.zeros(ops.train_workspace_bytes(pcfg, B), dtype=torch.uint8, device=scene["dev"])      # the dense step's size
    with pytest.raises(ops.PxoError, match="workspace"):
        _step(scene, pcfg, grid, ws=small)
    _, _, _, ws = _step(scene, pcfg, grid)
    with pytest.raises(ops.PxoError, match="pxo_train_fwd_bwd_culled"):
        ops.train_backward_work(pcfg, B, ws)
    _step(scene, pcfg, None, ws=ws)                               # a dense step on the same block leaves its own record again
    live, total = ops.train_backward_work(pcfg, B, ws)
    assert 0 < live <= total


# ---- TrainingGrid and nerf_sh.train --cull_reso -----------------------------------------------------------------------------------
CULL_FLAGS = ["--cull_reso", "16", "--cull_warmup_steps", "4", "--cull_update_every", "4"]


def _write_cfg(path, max_steps=12):
    with open(path, "w") as f:
        f.write("dataset: synthetic\nimage_batching: false\nfactor: 0\nnum_coarse_samples: 16\nnum_fine_samples: 32\nuse_viewdirs: false\n"
                f"white_bkgd: true\nbatch_size: 256\nsh_deg: 1\nrandomized: true\nmax_steps: {max_steps}\nsparsity_npoints: 100\n")


def _loop(args, dev, first, last, state=None, record=None, save_at=None):
    """Steps first..last of nerf_sh.train's loop (its dataset, learning rate, seeds and TrainingGrid) on one GPU; a run that starts
    after step 1 first draws the batches of the steps before it, so that it sees the batches the uninterrupted run sees."""
    from plenoctree_amd.nerf_sh.nerf import checkpoints, families, llff, models, occupancy, utils
    dataset = llff.get_dataset("train", args, dev, batch_size=args.batch_size, seed=20201473)
    if state is None:
        model, state = families.restore(args, dev, "train", say=lambda *a, **k: None)
    else:
        model = models.NerfModel(state.cfg)
    cull = occupancy.TrainingGrid.from_args(args, say=lambda *a, **k: None)
    for _ in range(1, first):
        next(dataset)
    for step in range(first, last + 1):
        batch = next(dataset)
        lr = utils.learning_rate_decay(step, args.lr_init, args.lr_final, args.max_steps, args.lr_delay_steps, args.lr_delay_mult)
        grid, rows = cull.before_step(step, model, state), []
        models.train_step(model, state, batch, lr, randomized=args.randomized, seed=step << 8, occupancy=grid, live_rows=rows)
        if record is not None:
            record.append((step, grid is not None, list(rows), cull.fraction))
        if step == save_at:
            checkpoints.save_checkpoint(args.train_dir, state, step)
    torch.cuda.synchronize()
    return state, cull


def test_training_grid_follows_the_schedule_and_a_resume_continues_bit_for_bit(tmp_path):
    """12 steps with a grid from step 5 on, rebuilt before step 9.  A checkpoint of step 8 (a multiple of cull_update_every) restored
    into a fresh state, with a fresh TrainingGrid and the batches of steps 9..12, ends with the bits of the uninterrupted run: the
    schedule depends on the step alone and the grid of step 9 is built from the restored parameters."""
    dev = _gpu()
    from plenoctree_amd.nerf_sh.nerf import families, utils
    cfg_path = os.path.join(str(tmp_path), "tiny.yaml")
    _write_cfg(cfg_path)
    argv = ["--train_dir", str(tmp_path), "--config", cfg_path, "--synthetic_hw", "32", "32", "--synthetic_views", "4", "1", *CULL_FLAGS]
    args = utils.define_flags().parse_args(argv)
    utils.update_flags(args)
    record = []
    state, cull = _loop(args, dev, 1, 12, record=record, save_at=8)
    print("step, culled, live rows, occupied fraction:", record)
    assert cull.rebuilds == [5, 9] and [r[1] for r in record] == [False] * 4 + [True] * 8
    per_ray = (16, 48)
    for step, culled, rows, _ in record[4:]:
        assert all(0 < rows[i] <= 256 * per_ray[i] for i in range(2)), (step, rows)
    for name in ("params", "m", "v"):
        assert torch.isfinite(getattr(state, name)).all(), name
    _, fresh = families.restore(args, dev, "train", say=lambda *a, **k: None)          # reads checkpoint_8
    assert fresh.step == 8
    resumed, cull2 = _loop(args, dev, 9, 12, state=fresh)
    assert cull2.rebuilds == [9]
    for name in ("params", "m", "v", "stats"):
        assert torch.equal(_bits(getattr(resumed, name)), _bits(getattr(state, name))), name


def test_train_cli_with_the_grid_and_with_it_off(tmp_path, capsys, monkeypatch):
    """nerf_sh.train on the small analytic scene: --cull_reso 16 rebuilds at the scheduled steps only, prints the live fractions,
    renders its test view through the grid and leaves finite parameters; --cull_reso 0 ends with the bits of a run without the
    flag."""
    dev = _gpu()
    from plenoctree_amd.nerf_sh import train
    from plenoctree_amd.nerf_sh.nerf import checkpoints, occupancy
    grids, applied = [], []
    orig = occupancy.TrainingGrid.from_args.__func__
    monkeypatch.setattr(occupancy.TrainingGrid, "from_args",
                        classmethod(lambda cls, args, say=print: grids.append(orig(cls, args, say)) or grids[-1]))
    ends = {}
    for name, extra in (("on", CULL_FLAGS), ("zero", ["--cull_reso", "0"]), ("plain", [])):
        d = os.path.join(str(tmp_path), name)
        os.makedirs(d)
        cfg_path = os.path.join(d, "tiny.yaml")
        _write_cfg(cfg_path)
        trace = train.main(["--train_dir", d, "--config", cfg_path, "--synthetic_hw", "32", "32", "--synthetic_views", "4", "1",
                            "--print_every", "4", "--save_every", "12", "--render_every", "12", "--chunk", "512", *extra])
        assert [t[0] for t in trace] == [4, 8, 12] and all(np.isfinite(t[1]) for t in trace)
        out = capsys.readouterr().out
        tree = checkpoints.restore_checkpoint(os.path.join(d, "checkpoint_12"))["optimizer"]["target"]["params"]
        ends[name] = tree
        if name == "on":
            assert grids[-1] is not None and grids[-1].rebuilds == [5, 9]
            lines = [l for l in out.splitlines() if "rays/sec" in l and "i_loss" in l]
            assert "cull: dense until step 5" in lines[0], lines[0]
            assert "live rows: coarse" in lines[1] and "rebuilt before step 5" in lines[1], lines[1]
            assert "live rows: coarse" in lines[2] and "rebuilt before step 9" in lines[2], lines[2]
            assert "Eval 12:" in out and "PSNR" in out
        else:
            assert grids[-1] is None and "cull" not in out and "live rows" not in out

    def leaves(t):
        return [np.asarray(v) for k in sorted(t) for v in (leaves(t[k]) if isinstance(t[k], dict) else [t[k]])]
    for a, b, c in zip(leaves(ends["zero"]), leaves(ends["plain"]), leaves(ends["on"])):
        assert a.tobytes() == b.tobytes()                         # --cull_reso 0: the run without the flag, bit for bit
        assert np.isfinite(c).all()
    assert any(a.tobytes() != c.tobytes() for a, c in zip(leaves(ends["plain"]), leaves(ends["on"])))      # the grid did act
