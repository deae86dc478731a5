"""The fused MLP kernels at every tile and split boundary, in every precision, against float64 (-m gpu).

What decides a launch's work split is a function of M (rows) and of the CU count:
  tile_sched (pxo_common.h)      whole rounds of full tiles (pxo_tile_rows() rows, one workgroup per CU), then a ragged
                                 last round that runs as half-height tiles only if it fits one round at half height
  mlp_grid                       one workgroup per CU, or one per tile when there are fewer tiles than CUs
  bf16x3                         half-height tiles, two workgroups per CU: a round is the same pxo_tile_rows() * CUs rows
  wgrad_split (wgrad_kernels)    256x256 products: one row range per CU from 1024 rows per CU, 4 CUs / 7 below;
                                 skinny products (enc-based pair, heads): 2 CUs ranges from 512 rows per CU, CUs below
Every row count below is derived from the device's CU count and pxo_tile_rows() at run time, and every SH degree
(head_blocks(deg) = 1, 1, 1, 2, 3) sees the small and tile-schedule sizes; the wgrad_split thresholds and the BASELINE
passes (4096 rays x 64 / 192 samples + 10,000 sparsity points) run at degrees 3 and 4.

  forward          raw_rgb, raw_sigma and the saved acts of every layer against the oracle MLP in float64 (rocBLAS on the
                   device, row chunks), at the bars of test_mlp_fwd_saved_tensors / test_mlp_fwd_x6_vs_f64_and_f32_kernel /
                   test_eval_points_x3_vs_f64
  row independence every row's outputs, saved tensors and dz are bit for bit those of the same rows in launches of at most
                   one round of full tiles (the invariant of test_half_height_tail_tiles)
  launch variants  eval_points with / without rgb, mlp_fwd with / without save, save without rgb: the same bits
  backward(data)   dz of all 8 layers against float64 autograd through the oracle MLP (ReLU-ambiguous rows zeroed)
  weight gradients every leaf of mlp_bwd_weights against float64 X^T dZ / column sums on the kernels' own float32
                   operands; bf16x6 with PXO_TUNE_X6_WGRAD = 1 and 0 (the leaves the knob does not touch: same bits)

Every buffer the ops wrappers allocate starts with all bits set (NaN): a row a kernel leaves unwritten cannot pass by
holding the right values of an earlier launch.
"""
import functools

import pytest
import torch

from oracle import nerf_oracle as O
from _helpers import _gpu, _ops, make_params, pxo_cfg, split_mlp

pytestmark = pytest.mark.gpu
F32, X3, X6 = 0, 1, 2

# row counts: name -> rows(c = CUs, T = pxo_tile_rows()); one round of full tiles is T * c rows
SMALL = {
    "1": lambda c, T: 1,
    "T/4-1": lambda c, T: T // 4 - 1,
    "T/2-1": lambda c, T: T // 2 - 1,
    "T/2": lambda c, T: T // 2,
    "T/2+1": lambda c, T: T // 2 + 1,
    "T-1": lambda c, T: T - 1,
    "T": lambda c, T: T,
    "T+1": lambda c, T: T + 1,
}
SCHED = {
    "round-T+5": lambda c, T: T * (c - 1) + 5,           # fewer tiles than CUs: one workgroup per tile
    "round-1": lambda c, T: T * c - 1,                   # one round, its last tile ragged; bf16x3: one row below a round
    "round": lambda c, T: T * c,                         # exactly one round
    "round+1": lambda c, T: T * c + 1,                   # + one half tile; bf16x3: one row above a round
    "round+T/2": lambda c, T: T * c + T // 2,            # + one whole half tile
    "round+half_round": lambda c, T: T * c + T // 2 * c,         # the largest half round
    "round+half_round+1": lambda c, T: T * c + T // 2 * c + 1,   # does not fit at half height: full tiles
    "2round+17": lambda c, T: 2 * T * c + 17,            # two rounds + one half tile
}
LARGE = {
    "skinny_split-1": lambda c, T: 512 * c - 1,          # wgrad_split: skinny products on c ranges ...
    "skinny_split": lambda c, T: 512 * c,                # ... and on 2 c from here
    "main_split-1": lambda c, T: 1024 * c - 1,           # 256x256 products on 4 c / 7 ranges ...
    "main_split": lambda c, T: 1024 * c,                 # ... and on c from here
    "baseline_coarse": lambda c, T: 4096 * 64 + 10000,
    "baseline_fine": lambda c, T: 4096 * 192 + 10000,
}
SIZES = {**SMALL, **SCHED, **LARGE}
CASES = [(d, s) for d in range(5) for s in list(SMALL) + list(SCHED)] + [(d, s) for d in (3, 4) for s in LARGE]
CHUNK = 32768            # rows per float64 reference chunk (bounds device memory at the BASELINE sizes)


def _geometry(dev):
    from plenoctree_amd import _lib
    return torch.cuda.get_device_properties(dev).multi_processor_count, _lib.load().pxo_tile_rows()


def _rows(dev, size):
    return SIZES[size](*_geometry(dev))


def _round_rows(dev):
    cus, T = _geometry(dev)
    return cus * T


def _chunks(M, n=CHUNK):
    return [slice(i, min(i + n, M)) for i in range(0, M, n)]


@functools.lru_cache(maxsize=None)
def _mlp_flat(deg, bias_scale):
    cfg = O.Cfg(sh_deg=deg)
    return split_mlp(make_params(cfg, bias_scale=bias_scale), cfg, 1)


def _mlp64(mlp_flat, cfg, dev):
    return [(w.to(dev), b.to(dev)) for w, b in O.unflatten_params(torch.cat([mlp_flat, mlp_flat]).double(), cfg)[0]]


def _inputs(M, C, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    pts = (torch.rand(M, 3, device=dev, generator=gen) * 2 - 1) * 2.0
    d_rgb = torch.randn(M, C, device=dev, generator=gen) * 0.1
    d_sigma = torch.randn(M, device=dev, generator=gen) * 0.1
    return pts, d_rgb, d_sigma


def _posenc(pts, dtype):
    """the oracle's encoding, computed on the host in `dtype`, on the device"""
    return torch.cat([O.posenc(pts[sl].cpu().to(dtype), 0, 10) for sl in _chunks(pts.shape[0], 1 << 18)]).to(pts.device)


def _cfgs(ops, deg, precisions):
    out = {}
    for tag, p in precisions:
        c = pxo_cfg(ops, O.Cfg(sh_deg=deg))
        c.mlp_precision = p
        out[tag] = c
    return out


@pytest.fixture(autouse=True)
def _poisoned_buffers(monkeypatch):
    ops = _ops()
    new = ops._new

    def poisoned(*shape, device=None, dtype=torch.float32):
        t = new(*shape, device=device, dtype=dtype)
        t.view(torch.uint8).fill_(0xFF)
        return t

    monkeypatch.setattr(ops, "_new", poisoned)


class _Err:
    """|got - want| accumulated over row chunks on the device: max, mean and the number of elements outside
    atol + rtol |want| (a NaN counts as outside)."""

    def __init__(self, rtol=0.0, atol=0.0):
        self.rtol, self.atol = rtol, atol
        self.mx = self.sum = self.bad = 0
        self.n = 0

    def add(self, got, want):
        d = (got.double() - want).abs()
        self.mx = torch.maximum(torch.as_tensor(self.mx, device=d.device, dtype=d.dtype), d.max()) if d.numel() else self.mx
        self.sum = self.sum + d.sum()
        self.bad = self.bad + (~(d <= self.atol + self.rtol * want.abs())).sum()
        self.n += d.numel()

    @property
    def max(self):
        return float(self.mx)

    @property
    def mean(self):
        return float(self.sum) / max(self.n, 1)

    def __repr__(self):
        out = f"max {self.max:.3e} mean {self.mean:.3e}"
        return out + (f" outside {int(self.bad)}/{self.n}" if self.rtol or self.atol else "")


def _same(what, got, want):
    assert got.shape == want.shape and torch.equal(got, want), \
        f"{what}: not bit-identical ({int((got != want).sum())} of {want.numel()} elements differ)"


# ---------------------------------------------------------------------------------------------------------------------
# float32 and bf16x6: forward, row independence, launch variants, backward(data)
# ---------------------------------------------------------------------------------------------------------------------
FWD_NAMES = [f"acts[{l}]" for l in range(8)] + ["raw_rgb", "raw_sigma"]


@pytest.mark.parametrize("deg,size", CASES)
def test_mlp_fwd_bwd_data_vs_f64(deg, size):
    ops = _ops(); dev = _gpu()
    M = _rows(dev, size)
    cfg = O.Cfg(sh_deg=deg)
    mlp_flat = _mlp_flat(deg, 0.1)
    cfgs = _cfgs(ops, deg, (("f32", F32), ("x6", X6)))
    pts, d_rgb, d_sigma = _inputs(M, cfg.num_rgb_channels, dev, 1000 + deg)
    packed = {t: ops.pack_weights(c, mlp_flat.to(dev)) for t, c in cfgs.items()}
    fwd = {t: ops.mlp_fwd(c, packed[t][0], pts, save=True) for t, c in cfgs.items()}

    # forward against float64, on the f32 encoding the kernels evaluate (pinned separately: "enc", atol 2e-6)
    mlp64 = _mlp64(mlp_flat, cfg, dev)
    e32 = _posenc(pts, torch.float32)
    err = {t: {n: _Err(2e-4, 2e-5) for n in FWD_NAMES} for t in cfgs}
    for t in cfgs:
        err[t]["enc"] = _Err(0.0, 2e-6)
        err[t]["dz"] = [_Err(5e-4, 2e-6) for _ in range(8)]
    ambiguous = torch.zeros(M, dtype=torch.bool, device=dev)
    with torch.no_grad():
        for sl in _chunks(M):
            x = e32[sl].double()
            rr, rs, acts = O.mlp_forward(mlp64, x, cfg, return_acts=True)
            for l in range(8):
                inp = x if l == 0 else (torch.cat([acts[4], x], -1) if l == 5 else acts[l - 1])
                ambiguous[sl] |= ((inp @ mlp64[l][0] + mlp64[l][1]).abs() < 1e-5).any(dim=1)
            for t, (rgb, sig, (a, enc, _)) in fwd.items():
                for l in range(8):
                    err[t][f"acts[{l}]"].add(a[l, sl], acts[l])
                err[t]["raw_rgb"].add(rgb[sl], rr)
                err[t]["raw_sigma"].add(sig[sl], rs[:, 0])
                err[t]["enc"].add(enc[sl], torch.cat([x, torch.zeros_like(x[:, :1])], -1))

    # backward(data) against float64 autograd; rows with a pre-activation within float32 round-off of 0 (either ReLU
    # branch is a correct float32 evaluation) get a zero upstream gradient everywhere
    d_rgb[ambiguous] = 0.0
    d_sigma[ambiguous] = 0.0
    bwd = {t: ops.mlp_bwd_data(c, packed[t][1], d_rgb, d_sigma, fwd[t][2][2]) for t, c in cfgs.items()}
    for sl in _chunks(M):
        x = e32[sl].double().requires_grad_(True)
        with torch.enable_grad():
            rr, rs, acts = O.mlp_forward(mlp64, x, cfg, return_acts=True)
            loss = (rr * d_rgb[sl].double()).sum() + (rs[:, 0] * d_sigma[sl].double()).sum()
            g = torch.autograd.grad(loss, acts)
        with torch.no_grad():
            for l in range(8):
                ref = g[l] * (acts[l] > 0)
                for t in cfgs:
                    err[t]["dz"][l].add(bwd[t][0][l, sl], ref)
        del acts, g, rr, rs, loss

    report = {t: {n: e for n, e in err[t].items() if n != "dz"} for t in cfgs}
    for t in cfgs:
        report[t].update({f"dz[{l}]": err[t]["dz"][l] for l in range(8)})
    names = FWD_NAMES + [f"dz[{l}]" for l in range(8)]
    ratio = lambda n, k: getattr(report["x6"][n], k) / max(getattr(report["f32"][n], k), 1e-300)
    print(f"\nBOUNDARY fwd/bwd deg={deg} M={M} ({size}) x6/f32 mean: "
          + " ".join(f"{n}={ratio(n, 'mean'):.3f}" for n in names)
          + " | max: " + " ".join(f"{n}={ratio(n, 'max'):.3f}" for n in names)
          + f" | f32 mean raw_rgb {report['f32']['raw_rgb'].mean:.2e} dz[0] {report['f32']['dz[0]'].mean:.2e}")
    fails = [f"{t}/{n}: {e}" for t in cfgs for n, e in report[t].items() if int(e.bad)]
    # bf16x6 at least as close to float64 as the float32 kernel: mean (5 % for ties) and worst element (x 3, the tail of a
    # max of two round-off patterns); over fewer than 64 rows the ratios are coin tosses and the element-wise bars hold alone
    if M >= 64:
        for n in names:
            a, b = report["f32"][n], report["x6"][n]
            eps_mean, eps_max = (1e-9, 1e-7) if n in FWD_NAMES else (1e-12, 1e-9)
            if not (b.mean <= 1.05 * a.mean + eps_mean and b.max <= 3.0 * a.max + eps_max):
                fails.append(f"x6 vs f32 {n}: x6 {b} / f32 {a}")
    assert not fails, f"deg {deg}, M {M} ({size}):\n" + "\n".join(fails)

    # launch variants: the same bits
    for t, c in cfgs.items():
        pf = packed[t][0]
        rgb, sig, (acts, enc, _) = fwd[t]
        r, s = ops.eval_points(c, pf, pts)
        _same(f"{t} eval_points rgb", r, rgb); _same(f"{t} eval_points sigma", s[:, 0], sig)
        _, s = ops.eval_points(c, pf, pts, want_rgb=False)
        _same(f"{t} eval_points sigma-only", s[:, 0], sig)
        r, s = ops.mlp_fwd(c, pf, pts, save=False)
        _same(f"{t} mlp_fwd(save=False) rgb", r, rgb); _same(f"{t} mlp_fwd(save=False) sigma", s, sig)
        _, s = ops.mlp_fwd(c, pf, pts, save=False, want_rgb=False)
        _same(f"{t} mlp_fwd(save=False, want_rgb=False) sigma", s, sig)
        _, s, (a2, e2, _) = ops.mlp_fwd(c, pf, pts, save=True, want_rgb=False)
        _same(f"{t} acts-only sigma", s, sig); _same(f"{t} acts-only acts", a2, acts); _same(f"{t} acts-only enc", e2, enc)
        del a2, e2, r, s

    # row independence: the same rows in launches of at most one round of full tiles
    if M > _round_rows(dev):
        for t, c in cfgs.items():
            pf, pb = packed[t]
            rgb, sig, (acts, enc, _) = fwd[t]
            dz = bwd[t][0]
            for sl in _chunks(M, _round_rows(dev)):
                r2, s2, (a2, e2, m2) = ops.mlp_fwd(c, pf, pts[sl].contiguous(), save=True)
                what = f"{t} rows [{sl.start},{sl.stop}) of {M}"
                _same(f"{what}: raw_rgb", r2, rgb[sl]); _same(f"{what}: raw_sigma", s2, sig[sl])
                _same(f"{what}: acts", a2, acts[:, sl]); _same(f"{what}: enc", e2, enc[sl])
                dz2, _ = ops.mlp_bwd_data(c, pb, d_rgb[sl].contiguous(), d_sigma[sl].contiguous(), m2)
                _same(f"{what}: dz", dz2, dz[:, sl])


# ---------------------------------------------------------------------------------------------------------------------
# bf16x3 (forward only)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg,size", CASES)
def test_mlp_x3_fwd_vs_f64(deg, size):
    ops = _ops(); dev = _gpu()
    M = _rows(dev, size)
    cfg = O.Cfg(sh_deg=deg)
    mlp_flat = _mlp_flat(deg, 0.2)
    cfgs = _cfgs(ops, deg, (("f32", F32), ("x3", X3)))
    pts, _, _ = _inputs(M, cfg.num_rgb_channels, dev, 2000 + deg)
    packed = {t: ops.pack_weights(c, mlp_flat.to(dev), need_bwd=False)[0] for t, c in cfgs.items()}
    out = {t: ops.eval_points(c, packed[t], pts) for t, c in cfgs.items()}
    # as test_eval_points_x3_vs_f64: the float64 oracle on the float64 encoding
    mlp64 = _mlp64(mlp_flat, cfg, dev)
    e64 = _posenc(pts, torch.float64)
    err = {t: {"rgb": _Err(), "sigma": _Err()} for t in cfgs}
    s_rgb = s_sig = torch.zeros((), dtype=torch.float64, device=dev)
    with torch.no_grad():
        for sl in _chunks(M):
            rr, rs = O.mlp_forward(mlp64, e64[sl], cfg)
            s_rgb = torch.maximum(s_rgb, rr.abs().max()); s_sig = torch.maximum(s_sig, rs.abs().max())
            for t, (rgb, sig) in out.items():
                err[t]["rgb"].add(rgb[sl], rr)
                err[t]["sigma"].add(sig[sl], rs)
    s_rgb, s_sig = max(float(s_rgb), 1.0), max(float(s_sig), 1.0)
    x3, f32 = err["x3"], err["f32"]
    print(f"\nBOUNDARY x3 deg={deg} M={M} ({size}) max rgb {x3['rgb'].max / s_rgb:.2e} sigma {x3['sigma'].max / s_sig:.2e} "
          f"(x output scale), mean rgb x3/f32 {x3['rgb'].mean / max(f32['rgb'].mean, 1e-300):.2f}")
    assert x3["rgb"].max <= 5e-5 * s_rgb and x3["sigma"].max <= 5e-5 * s_sig, (x3, s_rgb, s_sig)
    if M >= 100:
        assert x3["rgb"].mean <= 12 * f32["rgb"].mean + 1e-7, (x3, f32)

    c, px3 = cfgs["x3"], packed["x3"]
    rgb, sig = out["x3"]
    _, s = ops.eval_points(c, px3, pts, want_rgb=False)
    _same("x3 eval_points sigma-only", s, sig)
    r, s = ops.mlp_fwd(c, px3, pts, save=False)
    _same("x3 mlp_fwd rgb", r, rgb); _same("x3 mlp_fwd sigma", s, sig[:, 0])
    _, s = ops.mlp_fwd(c, px3, pts, save=False, want_rgb=False)
    _same("x3 mlp_fwd sigma-only", s, sig[:, 0])
    if M > _round_rows(dev):
        for sl in _chunks(M, _round_rows(dev)):
            r2, s2 = ops.eval_points(c, px3, pts[sl].contiguous())
            _same(f"x3 rows [{sl.start},{sl.stop}) of {M}: rgb", r2, rgb[sl])
            _same(f"x3 rows [{sl.start},{sl.stop}) of {M}: sigma", s2, sig[sl])


# ---------------------------------------------------------------------------------------------------------------------
# weight and bias gradients, per leaf
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad_ref64(acts, enc, dz, d_rgb, d_sigma, C):
    """{(layer, is_bias): float64 [rows, cols]}: X^T dZ and column sums over the rows, on the kernels' own float32 operands;
    {layer: [rows, 1]}: the root-sum-square of each bias's summands"""
    M = d_sigma.shape[0]
    dev = d_sigma.device
    z = lambda r, c: torch.zeros(r, c, dtype=torch.float64, device=dev)
    ref = {(l, 0): z(63 if l == 0 else (256 + 63 if l == 5 else 256), 256) for l in range(8)}
    ref.update({(l, 1): z(256, 1) for l in range(8)})
    ref.update({(8, 0): z(256, 1), (8, 1): z(1, 1), (9, 0): z(256, C), (9, 1): z(C, 1)})
    rss = {l: z(256, 1) for l in range(8)}
    rss.update({8: z(1, 1), 9: z(C, 1)})
    for sl in _chunks(M):
        e = enc[sl, :63].double()
        A, Z = acts[:, sl].double(), dz[:, sl].double()
        dr, ds = d_rgb[sl].double(), d_sigma[sl].double()[:, None]
        ref[(0, 0)] += e.T @ Z[0]
        for l in range(1, 8):
            ref[(l, 0)][:256] += A[l - 1].T @ Z[l]
        ref[(5, 0)][256:] += e.T @ Z[5]
        ref[(8, 0)] += A[7].T @ ds
        ref[(9, 0)] += A[7].T @ dr
        for l, col in [(l, Z[l]) for l in range(8)] + [(8, ds), (9, dr)]:
            ref[(l, 1)] += col.sum(0)[:, None]
            rss[l] += (col * col).sum(0)[:, None]
        del A, Z
    return ref, {l: r.sqrt() for l, r in rss.items()}


@pytest.mark.parametrize("deg,size", CASES)
def test_mlp_bwd_weights_per_leaf_vs_f64(deg, size):
    ops = _ops(); dev = _gpu()
    M = _rows(dev, size)
    T = _geometry(dev)[1]
    cfg = O.Cfg(sh_deg=deg)
    C = cfg.num_rgb_channels
    mlp_flat = _mlp_flat(deg, 0.2)
    cfgs = _cfgs(ops, deg, (("f32", F32), ("x6", X6)))
    pts, d_rgb, d_sigma = _inputs(M, C, dev, 3000 + deg)
    lay, _ = ops.param_layout(cfgs["f32"])
    assert ops.get_tuning(ops.TUNE_X6_WGRAD) == 1
    fails, lines = [], []
    for t, c in cfgs.items():
        pf, pb = ops.pack_weights(c, mlp_flat.to(dev))
        _, _, (acts, enc, mask) = ops.mlp_fwd(c, pf, pts, save=True)
        dz, dbias = ops.mlp_bwd_data(c, pb, d_rgb, d_sigma, mask)
        g = {}
        try:
            for knob in ((1, 0) if t == "x6" else (1,)):
                ops.set_tuning(ops.TUNE_X6_WGRAD, knob)
                g[knob] = ops.mlp_bwd_weights(c, acts, enc, dz, d_rgb, d_sigma, dbias)
        finally:
            ops.set_tuning(ops.TUNE_X6_WGRAD, 1)
        ref, rss = _wgrad_ref64(acts, enc, dz, d_rgb, d_sigma, C)
        del acts, enc, dz, mask, dbias
        same = torch.ones(g[1].numel(), dtype=torch.bool, device=dev)
        for layer, is_bias, o, rows, cols in lay:
            r = ref[(layer, is_bias)]
            scale = float(r.abs().max())
            if is_bias:
                # a column sum is judged on the size of what it sums as well: the sigma head's bias gradient is ONE sum of
                # random-sign terms (|sum| ~ 1e-4 of its root-sum-square at some sizes)
                scale = max(scale, float(rss[layer].max()))
            for knob, gk in g.items():
                e = _Err(); e.add(gk[o:o + rows * cols].view(rows, cols), r)
                tag = f"{t}{'' if t == 'f32' else f'/knob{knob}'} {'b' if is_bias else 'W'}{layer}"
                lines.append(f"{tag}={e.max / max(scale, 1e-300):.1e}")
                if not (scale > 0 and e.max <= 1e-5 * scale):
                    fails.append(f"{tag}: max |err| {e.max:.3e} > 1e-5 x scale {scale:.3e} ({e})")
            if t == "x6" and not is_bias and 1 <= layer <= 7:
                # the 256x256 products on the bf16 pipe against the float32-MFMA kernel on the same operands
                ea, eb = _Err(), _Err()
                ea.add(g[1][o:o + 256 * 256].view(256, 256), r[:256]); eb.add(g[0][o:o + 256 * 256].view(256, 256), r[:256])
                lines.append(f"x6/f32mfma W{layer} mean {ea.mean / max(eb.mean, 1e-300):.3f} max {ea.max / max(eb.max, 1e-300):.3f}")
                # 4096 rows and more (test_wgrad_x6_vs_f64_and_f32_kernel, 40,000 rows): 1.05, measured 0.49 - 0.83 from one round
                # of tiles up.  Below, every row range is one partial chunk and the six-MFMA chain meets 1.25 x at 597 rows;
                # fewer than 2 tiles of rows (measured 1.22 - 1.38) and ONE row (each element is one product: the float32 MFMA
                # rounds it once, the chain of the six twice and leaves the three smallest out; measured 1.96, max 3.9 x)
                # keep a ~20 % margin over what was measured
                slack, max_slack = (1.05, 3.0) if M >= 4096 else (1.25, 3.0) if M >= 2 * T else (1.6, 3.0) if M > 1 else (2.4, 4.8)
                if not (ea.mean <= slack * eb.mean + 1e-12 and ea.max <= max_slack * eb.max + 1e-12):
                    fails.append(f"x6 W{layer} vs the float32-MFMA kernel: {ea} / {eb}")
                same[o:o + 256 * 256] = False
        if t == "x6":
            bad = int((g[1][same] != g[0][same]).sum())
            if bad:
                fails.append(f"x6: {bad} elements of the leaves PXO_TUNE_X6_WGRAD does not touch differ between knob 1 and 0")
    print(f"\nBOUNDARY wgrad deg={deg} M={M} ({size}) max|err|/scale: " + " ".join(lines))
    assert not fails, f"deg {deg}, M {M} ({size}):\n" + "\n".join(fails)
