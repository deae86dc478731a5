"""The phases between the GEMMs of the fused float32 MLP kernels -- accumulator start, ReLU, relu mask, staging of the
upstream gradient, head bias sum -- at the smallest shapes at which they can go wrong (-m gpu), through pxo_mlp_fwd /
pxo_mlp_bwd_data.  The reference is the oracle MLP in float64 on the host, at the bars of test_gpu_mlp_boundaries.py
(forward 2e-4 |want| + 2e-5, dz 5e-4 |want| + 2e-6, rows with a pre-activation within float32 round-off of 0 get a zero
upstream gradient); what is exact by construction is compared bit for bit.

  row counts       M in {1, 33, 64, 65, 128, 129, 192, 257}, SH16 and SH25: one row, a partial row block, half a tile, a full
                   tile, a full tile + 1, one and a half tiles, two tiles + 1 (below one round of tiles every tile runs at full
                   height; the half-height tiles of a ragged last round are test_gpu_mlp_boundaries.py's "round+..." sizes)
  bias start       one layer at a time with a zero kernel and large biases: its saved activation is relu(bias) exactly, layer 5
                   (two K segments: the second must not start from the bias again) included
  mask semantics   pre-activations of layer 1 that are exactly +0, -0, a positive denormal, a negative denormal, positive and
                   negative, at known rows of a 128-row tile (both half-waves, both register halves of a fragment, every row
                   block) and columns of several waves: the saved activation is +0 (all bits) unless the pre-activation is
                   positive, dz is exactly 0 there (relu'(0) = 0) and carries the gradient through the positive denormal
  fresh start      backward at M = 129 into buffers full of NaN: no NaN in dz, bias partials against float64 column sums
  head bias sum    the head's bias partial of a tile is the float32 sum of the staged upstream gradient, rows 0 -> 127 in turn
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from _helpers import _gpu, _ops, make_params, pxo_cfg, split_mlp

pytestmark = pytest.mark.gpu

ROWS = (1, 33, 64, 65, 128, 129, 192, 257)
TILE = 128


@pytest.fixture(autouse=True)
def _poisoned_buffers(monkeypatch):
    """every buffer the ops wrappers allocate starts with all bits set (NaN), the dz and bias-partial workspaces included"""
    ops = _ops()
    new = ops._new

    def poisoned(*shape, device=None, dtype=torch.float32):
        t = new(*shape, device=device, dtype=dtype)
        t.view(torch.uint8).fill_(0xFF)
        return t

    monkeypatch.setattr(ops, "_new", poisoned)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _offsets(cfg):
    """{(layer, is_bias): (offset, rows, cols)} inside ONE MLP's flat parameters (O.flatten_params order)"""
    out, off = {}, 0
    for l, (fi, fo) in enumerate(O.layer_shapes(cfg)):
        out[(l, 0)] = (off, fi, fo); off += fi * fo
        out[(l, 1)] = (off, 1, fo); off += fo
    return out


def _kernel(flat, cfg, l):
    o, r, c = _offsets(cfg)[(l, 0)]
    return flat[o:o + r * c].view(r, c)


def _bias(flat, cfg, l):
    o, _, c = _offsets(cfg)[(l, 1)]
    return flat[o:o + c]


@functools.lru_cache(maxsize=None)
def _mlp_flat(deg):
    cfg = O.Cfg(sh_deg=deg)
    return split_mlp(make_params(cfg, bias_scale=0.1), cfg, 1)


def _mlp64(flat, cfg):
    return O.unflatten_params(torch.cat([flat, flat]).double(), cfg)[0]


def _inputs(M, C, seed):
    gen = torch.Generator().manual_seed(seed)
    pts = (torch.rand(M, 3, generator=gen) * 2 - 1) * 2.0
    return pts, torch.randn(M, C, generator=gen) * 0.1, torch.randn(M, generator=gen) * 0.1


def _reference(flat, cfg, pts, d_rgb, d_sigma, skip_ambiguity=None):
    """float64 on the host, on the float32 encoding: (raw_rgb, raw_sigma, acts[8], dz[8], ambiguous rows).  The upstream
    gradient of an ambiguous row (a pre-activation within 1e-5 of 0, `skip_ambiguity(layer)` -> columns left out) is zero."""
    mlp = _mlp64(flat, cfg)
    x = O.posenc(pts.float(), 0, 10).double().requires_grad_(True)
    with torch.enable_grad():
        rr, rs, acts = O.mlp_forward(mlp, x, cfg, return_acts=True)
    ambiguous = torch.zeros(pts.shape[0], dtype=torch.bool)
    with torch.no_grad():
        for l in range(8):
            inp = x if l == 0 else (torch.cat([acts[4], x], -1) if l == 5 else acts[l - 1])
            near0 = (inp @ mlp[l][0] + mlp[l][1]).abs() < 1e-5
            if skip_ambiguity is not None:
                near0[:, skip_ambiguity(l)] = False
            ambiguous |= near0.any(dim=1)
    d_rgb, d_sigma = d_rgb.clone(), d_sigma.clone()
    d_rgb[ambiguous] = 0.0
    d_sigma[ambiguous] = 0.0
    with torch.enable_grad():
        loss = (rr * d_rgb.double()).sum() + (rs[:, 0] * d_sigma.double()).sum()
        g = torch.autograd.grad(loss, acts)
    dz = [(g[l] * (acts[l] > 0)).detach() for l in range(8)]
    return rr.detach(), rs[:, 0].detach(), [a.detach() for a in acts], dz, ambiguous, d_rgb, d_sigma


def _outside(got, want, rtol, atol):
    d = (got.detach().cpu().double() - want).abs()
    bad = ~(d <= atol + rtol * want.abs())       # a NaN counts as outside
    return int(bad.sum()), float(d.max()) if d.numel() else 0.0


def _run(ops, deg, flat, pts, d_rgb, d_sigma):
    """forward with saved tensors, then backward(data), on the device"""
    dev = _gpu()
    pcfg = pxo_cfg(ops, O.Cfg(sh_deg=deg))
    pf, pb = ops.pack_weights(pcfg, flat.to(dev))
    rgb, sig, (acts, enc, mask) = ops.mlp_fwd(pcfg, pf, pts.to(dev), save=True)
    dz, dbias = ops.mlp_bwd_data(pcfg, pb, d_rgb.to(dev).contiguous(), d_sigma.to(dev).contiguous(), mask)
    torch.cuda.synchronize()
    return rgb, sig, acts, enc, dz, dbias


def _check_vs_f64(tag, got, ref, fails, layers=range(8)):
    rgb, sig, acts, enc, dz, _ = got
    rr, rs, racts, rdz = ref[:4]
    checks = [("raw_rgb", rgb, rr, 2e-4, 2e-5), ("raw_sigma", sig, rs, 2e-4, 2e-5)]
    checks += [(f"acts[{l}]", acts[l], racts[l], 2e-4, 2e-5) for l in layers]
    checks += [(f"dz[{l}]", dz[l], rdz[l], 5e-4, 2e-6) for l in layers]
    for name, g, w, rtol, atol in checks:
        bad, mx = _outside(g, w, rtol, atol)
        print(f"{tag} {name}: max |err| {mx:.3e}, outside {bad}/{w.numel()}")
        if bad:
            fails.append(f"{tag} {name}: {bad}/{w.numel()} outside {rtol} |want| + {atol} (max |err| {mx:.3e})")


# ---------------------------------------------------------------------------------------------------------------------
# row counts
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows_reference(deg):
    """one float64 evaluation of max(ROWS) rows per degree; every row count is a prefix of it (rows are independent)"""
    cfg = O.Cfg(sh_deg=deg)
    pts, d_rgb, d_sigma = _inputs(max(ROWS), cfg.num_rgb_channels, 700 + deg)
    return (pts, *_reference(_mlp_flat(deg), cfg, pts, d_rgb, d_sigma))


@pytest.mark.parametrize("deg", (3, 4))
@pytest.mark.parametrize("M", ROWS)
def test_rows_vs_f64(deg, M):
    ops = _ops()
    pts, rr, rs, racts, rdz, _, d_rgb, d_sigma = _rows_reference(deg)
    got = _run(ops, deg, _mlp_flat(deg), pts[:M].contiguous(), d_rgb[:M], d_sigma[:M])
    fails = []
    enc_bad, enc_max = _outside(got[3][:, :63], O.posenc(pts[:M].float(), 0, 10).double(), 0.0, 2e-6)
    if enc_bad or not bool((got[3][:, 63] == 0).all()):
        fails.append(f"enc: {enc_bad} outside 2e-6 (max {enc_max:.3e}) or a non-zero pad column")
    _check_vs_f64(f"deg {deg} M {M}", got, (rr[:M], rs[:M], [a[:M] for a in racts], [z[:M] for z in rdz]), fails)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# bias start and skip segment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layer", (0, 3, 5, 7))
def test_zero_kernel_layer_outputs_its_bias_exactly(layer):
    """A layer with a zero kernel returns relu(bias) whatever it reads: every product is an exact zero, so the accumulator
    must hold exactly the value it started from -- the bias, once (layer 5 runs two K segments)."""
    ops = _ops()
    deg, M = 3, 129
    cfg = O.Cfg(sh_deg=deg)
    flat = _mlp_flat(deg).clone()
    _kernel(flat, cfg, layer).zero_()
    n = torch.arange(256, dtype=torch.float32)
    bias = torch.where(n.long() % 3 == 1, -1.0, 1.0) * (17.0 + n * 0.37109375)      # large, both signs, all different
    _bias(flat, cfg, layer).copy_(bias)
    pts, d_rgb, d_sigma = _inputs(M, cfg.num_rgb_channels, 800 + layer)
    ref = _reference(flat, cfg, pts, d_rgb, d_sigma, skip_ambiguity=lambda l: slice(None) if l == layer else slice(0, 0))
    got = _run(ops, deg, flat, pts, ref[5], ref[6])
    want = torch.relu(bias).expand(M, 256)
    diff = int((_bits(got[2][layer]) != _bits(want)).sum())
    fails = [f"acts[{layer}] is not relu(bias) bit for bit: {diff} of {want.numel()} elements differ"] if diff else []
    _check_vs_f64(f"zero kernel in layer {layer}", got, ref, fails)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# mask semantics, ReLU of signed zeros and denormals
# ---------------------------------------------------------------------------------------------------------------------
DENORMAL = float(np.float32(1e-40))
KINDS = (0.0, DENORMAL, 0.75, 3.0)                      # t[row] = the first coordinate of the row's point
PASS_COLS = (3, 100, 255)                               # pre-activation of layer 1 = +t   (waves 0, 3, 7)
NEG_COLS = (40, 200)                                    # pre-activation of layer 1 = -t   (-0 where t = +0; waves 1, 6)


def _row_kinds():
    """index into KINDS per row of a 128-row tile: within every (row block, half-wave, register half) class of rows --
    accumulator register reg of lane l holds row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of its row block -- each kind twice"""
    kind = np.zeros(TILE, np.int64)
    seen = {}
    for row in range(TILE):
        cls = (row // 32, (row % 8) // 4, (row % 32) // 16)
        kind[row] = (seen.get(cls, 0) + sum(cls)) % len(KINDS)
        seen[cls] = seen.get(cls, 0) + 1
    assert all(v == 8 for v in seen.values()) and len(seen) == 16
    return kind


def test_relu_mask_at_signed_zeros_and_denormals():
    ops = _ops()
    deg, M = 3, TILE
    cfg = O.Cfg(sh_deg=deg)
    flat = _mlp_flat(deg).clone()
    # layer 0: column 0 = relu(1 * p0) = t, columns 1 and 2 = relu(p1), relu(p2) (rows with the same t differ further on),
    # every other column relu(+0) = +0
    w0 = _kernel(flat, cfg, 0)
    w0.zero_(); w0[0, 0] = w0[1, 1] = w0[2, 2] = 1.0
    _bias(flat, cfg, 0).zero_()
    # layer 1: +0 + t * 1 + (>= +0)(+0) ... = t in PASS_COLS, -0 + t * (-1) + (>= +0)(-0) ... = -t in NEG_COLS (-0 for t = +0)
    w1, b1 = _kernel(flat, cfg, 1), _bias(flat, cfg, 1)
    for n in PASS_COLS:
        w1[:, n] = 0.0; w1[0, n] = 1.0; b1[n] = 0.0
    for n in NEG_COLS:
        w1[:, n] = -0.0; w1[0, n] = -1.0; b1[n] = -0.0
    kind = _row_kinds()
    t = torch.tensor([KINDS[k] for k in kind], dtype=torch.float32)
    assert float(t[kind == 1][0]) == DENORMAL and 0.0 < DENORMAL < float(np.finfo(np.float32).tiny)
    pts, d_rgb, d_sigma = _inputs(M, cfg.num_rgb_channels, 900)
    pts[:, 0] = t
    special = list(PASS_COLS + NEG_COLS)
    ref = _reference(flat, cfg, pts, d_rgb, d_sigma,
                     skip_ambiguity=lambda l: slice(None) if l == 0 else (special if l == 1 else slice(0, 0)))
    clear = ~ref[4]                                        # rows that keep their upstream gradient
    assert all(int((clear & torch.from_numpy(kind == k)).sum()) >= 8 for k in range(len(KINDS))), "too many ambiguous rows"
    rgb, sig, acts, enc, dz, _ = got = _run(ops, deg, flat, pts, ref[5], ref[6])

    fails = []
    a0, a1, z1 = _bits(acts[0]), _bits(acts[1]), dz[1].cpu()
    tb = _bits(t)
    if not (torch.equal(a0[:, :3], _bits(torch.relu(pts))) and int((a0[:, 3:] != 0).sum()) == 0):
        fails.append("construction: acts[0] is not [t, relu(p1), relu(p2) | +0 ...] bit for bit (a denormal or a zero did not "
                     "survive layer 0)")
    positive = t > 0
    for n in PASS_COLS:
        if not torch.equal(a1[:, n], tb):
            fails.append(f"acts[1][:, {n}]: {int((a1[:, n] != tb).sum())} rows are not t bit for bit "
                         f"(+0 rows {a1[:, n][~positive].unique().tolist()}, denormal rows {a1[:, n][torch.from_numpy(kind == 1)].unique().tolist()})")
        if int((z1[:, n][~positive] != 0).sum()):
            fails.append(f"dz[1][:, {n}]: a gradient passes where the pre-activation is +0")
        through = positive & clear
        if int((z1[:, n][through] == 0).sum()):
            fails.append(f"dz[1][:, {n}]: no gradient through {int((z1[:, n][through] == 0).sum())} positive pre-activations "
                         f"(of them denormal: {int((z1[:, n][through & torch.from_numpy(kind == 1)] == 0).sum())})")
    for n in NEG_COLS:
        if int((a1[:, n] != 0).sum()):
            fails.append(f"acts[1][:, {n}]: {int((a1[:, n] != 0).sum())} rows are not +0 (all bits) for -0 / negative pre-activations")
        if int((z1[:, n] != 0).sum()):
            fails.append(f"dz[1][:, {n}]: a gradient passes where the pre-activation is -0 or negative")
    _check_vs_f64("mask semantics", got, ref, fails)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# backward into NaN-filled buffers, bias partials, head bias sum
# ---------------------------------------------------------------------------------------------------------------------
def _staged(d_rgb, d_sigma, rows, NH):
    """the head's upstream-gradient tile as the kernel stages it: [rgb | sigma | 0 ...], rows past M zero"""
    C = d_rgb.shape[1]
    out = torch.zeros(TILE, NH, dtype=torch.float32)
    out[:rows.stop - rows.start, :C] = d_rgb[rows]
    out[:rows.stop - rows.start, C] = d_sigma[rows]
    return out


@pytest.mark.parametrize("deg", (3, 4))
def test_bwd_fresh_accumulators_and_bias_partials(deg):
    ops = _ops()
    M = 129
    cfg = O.Cfg(sh_deg=deg)
    C = cfg.num_rgb_channels
    NH = 32 * ((C + 1 + 31) // 32)
    pts, d_rgb, d_sigma = _inputs(M, C, 950 + deg)
    ref = _reference(_mlp_flat(deg), cfg, pts, d_rgb, d_sigma)
    d_rgb, d_sigma = ref[5], ref[6]
    got = _run(ops, deg, _mlp_flat(deg), pts, d_rgb, d_sigma)
    dz, dbias = got[4].cpu(), got[5].cpu()
    fails = []
    if bool(torch.isnan(dz).any()):
        fails.append(f"{int(torch.isnan(dz).sum())} NaN in dz: an accumulator or a row was not started afresh")
    _check_vs_f64(f"deg {deg} M {M} into NaN-filled buffers", got, ref, fails)
    part = dbias[:2 * 9 * 256].view(2, 9, 256)
    eps = 2.0 ** -24
    for slot, rows in enumerate((slice(0, TILE), slice(TILE, M))):
        for l in range(8):
            col = dz[l, rows].double()
            want, bound = col.sum(0), TILE * eps * col.abs().sum(0)            # (n - 1) u sum |x| of a float32 sum of n terms
            err = (part[slot, l].double() - want).abs()
            if not bool((err <= bound).all()):
                fails.append(f"bias partial slot {slot} layer {l}: max |err| {float(err.max()):.3e} beyond 128 x 2^-24 x sum |dz|")
        # the head: the staged tile summed row 0 -> 127 in float32, one add at a time -- the order fixes the bits
        staged = _staged(d_rgb, d_sigma, rows, NH).numpy()
        acc = np.zeros(NH, np.float32)
        for r in range(TILE):
            acc = (acc + staged[r]).astype(np.float32)
        head = part[slot, 8].numpy()
        diff = int((head[:NH].view(np.int32) != acc.view(np.int32)).sum()) + int((head[NH:].view(np.int32) != 0).sum())
        print(f"deg {deg} slot {slot}: head bias partial differs from the row-ordered float32 sum in {diff} columns")
        if diff:
            fails.append(f"head bias partial of slot {slot}: {diff} of 256 columns differ from the float32 sum over rows 0 -> 127")
    assert not fails, "\n".join(fails)
