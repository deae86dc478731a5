"""The view-conditioned head, its fused SH projection and its compositing kernel at the edges of their blocks, against float64.

vd_head_kernel works in groups of 16 points, vd_pair_kernel in blocks of 256 points (lanes past N redo point N - 1 and store
nothing) and of 8 directions (padded rows of C and of the basis that vd_dir_kernel must write as zeros), vd_point_kernel takes one
direction per point (so the padding of C depends on N), and vd_composite_fwd_kernel runs four rays per workgroup in chunks of 64
samples.  Every case is compared with the float64 host restatement of tests/_viewdirs_helpers.py on seeded inputs.

Bounds.  Projection and head: 4 x floor x max(1, max |want| / max |the fixture's value of that quantity|), floor = the reference's
own float32 round-off stored in tests/golden/viewdirs_projection.npz: the rule test_extraction_end_to_end uses for inputs other
than the fixture's.  tests/test_viewdirs_cpu.py (test_reference_arithmetic_stays_inside_the_edge_bounds) measures how much of
that factor 4 a float32 host restatement uses on these inputs and prints it; the rest is the kernels' allowance.  Compositing:
the rtol / atol test_shade_composite_fwd_bwd holds the SH kernel to, which shares sample_alpha and chunk_transmittance with this
one."""
import ctypes

import pytest
import torch

from oracle import nerf_oracle as O

from _helpers import make_rays
from _viewdirs_helpers import (EDGE_CROSS_N, EDGE_CROSS_R, EDGE_DIR_N, EDGE_DIR_R, EDGE_PER_POINT_N, EDGE_POINT_N, EDGE_POINT_R,
                               EdgeReference, edge_check)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 64                 # floats: 256 bytes


@pytest.fixture(scope="module")
def ctx():
    from plenoctree_amd import _lib, ops
    from plenoctree_amd.nerf_sh.nerf import checkpoints, viewdirs
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    ref = EdgeReference()
    flat = checkpoints.vd_tree_to_arena(checkpoints.vd_torch_state_dict_to_tree(ref.sd))
    state = viewdirs.ViewdirsState(torch.from_numpy(flat).to(dev))
    worst = {}
    yield dict(ops=ops, lib=_lib.load(), dev=dev, ref=ref, state=state, model=viewdirs.ViewdirsModel(), packed=state.packed[1][0],
               pts=ref.inp["points"].to(dev), worst=worst)
    print("\nworst multiple of the scaled floor per quantity:", {k: round(v, 2) for k, v in sorted(worst.items())})


def _dirs(ctx, R):
    return ctx["ref"].dirs(R).to(ctx["dev"])


def _project_case(ctx, N, R, deg):
    ref, m = ctx["ref"], ctx["model"]
    K = (deg + 1) ** 2
    co, sigma = m.project_sh(ctx["state"], ctx["pts"][:N].contiguous(), _dirs(ctx, R), deg)
    assert co.shape == (N, 3 * K) and sigma.shape == (N,)
    want = ref.coeffs(N, R, deg)
    edge_check(f"coeffs_{deg} N={N} R={R}", co, want, ref.bound(f"coeffs_{deg}", want), ctx["worst"])
    edge_check(f"sigma N={N} R={R}", sigma, ref.sigma[:N], ref.bound("sigma", ref.sigma[:N]), ctx["worst"])


# ---- a. b. the projection -----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(60)
@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("N", EDGE_POINT_N)
def test_projection_at_the_point_edges(ctx, N, deg):
    _project_case(ctx, N, EDGE_POINT_R, deg)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("R", EDGE_DIR_R)
def test_projection_at_the_direction_edges(ctx, R, deg):
    _project_case(ctx, EDGE_DIR_N, R, deg)


@pytest.mark.timeout(60)
def test_projection_of_the_special_directions(ctx):
    """The axes, where all but a few basis functions vanish, and directions with one or no zero component; R = 9 pads 7 rows."""
    _project_case(ctx, EDGE_DIR_N, "special", 4)


# ---- c. d. the head alone -----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(60)
@pytest.mark.parametrize("R", EDGE_CROSS_R)
@pytest.mark.parametrize("N", EDGE_CROSS_N)
def test_cross_evaluation(ctx, N, R):
    ref = ctx["ref"]
    rgb, sigma = ctx["model"].eval_points_raw(ctx["state"], ctx["pts"][:N].contiguous(), _dirs(ctx, R), cross_broadcast=True)
    assert rgb.shape == (N, R, 3) and sigma.shape == (N, 1)
    want = ref.cross(N, R)
    edge_check(f"rgb_cross N={N} R={R}", rgb, want, ref.bound("rgb_cross", want), ctx["worst"])
    edge_check(f"sigma N={N} R={R}", sigma.view(-1), ref.sigma[:N], ref.bound("sigma", ref.sigma[:N]), ctx["worst"])


@pytest.mark.timeout(60)
@pytest.mark.parametrize("N", EDGE_PER_POINT_N)
def test_per_point_form(ctx, N):
    """Point i under direction i: C has N rows here, padded to the next multiple of 8."""
    ref = ctx["ref"]
    rgb, sigma = ctx["model"].eval_points_raw(ctx["state"], ctx["pts"][:N].contiguous(), _dirs(ctx, N))
    assert rgb.shape == (N, 3) and sigma.shape == (N, 1)
    want = ref.rgb_per_point[:N]
    edge_check(f"rgb_point N={N}", rgb, want, ref.bound("rgb_point", want), ctx["worst"])
    edge_check(f"sigma N={N}", sigma.view(-1), ref.sigma[:N], ref.bound("sigma", ref.sigma[:N]), ctx["worst"])


# ---- e. nothing is written outside the result ---------------------------------------------------------------------------------
class _Guarded:
    """`count` floats at a 256-byte-aligned offset inside a larger buffer filled with a sentinel."""

    def __init__(self, count, dev):
        self.count = count
        tail = -count % PAD + PAD
        self.buf = torch.full((PAD + count + tail,), SENTINEL, dtype=torch.float32, device=dev)
        self.out = self.buf[PAD:PAD + count]
        assert self.out.data_ptr() % 256 == 0 and self.out.is_contiguous()

    def intact(self):
        s = torch.tensor(SENTINEL, dtype=torch.float32, device=self.buf.device)
        return bool((self.buf[:PAD] == s).all()) and bool((self.buf[PAD + self.count:] == s).all())

    def written(self):
        return bool((self.out != torch.tensor(SENTINEL, dtype=torch.float32, device=self.buf.device)).all())


@pytest.mark.timeout(60)
@pytest.mark.parametrize("N,R", [(257, 9), (1, 1)])
def test_nothing_is_written_outside_the_result(ctx, N, R):
    ops, lib, dev, packed = ctx["ops"], ctx["lib"], ctx["dev"], ctx["packed"]
    pts, dirs = ctx["pts"][:N].contiguous(), _dirs(ctx, R)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    # the projection, every degree (the stores are unrolled per instantiation)
    for deg in range(5):
        K = (deg + 1) ** 2
        co, sg = _Guarded(N * 3 * K, dev), _Guarded(N, dev)
        ops.vd_project_sh(packed, pts, dirs, deg, coeffs=co.out.view(N, 3 * K), raw_sigma=sg.out)
        plain_co, plain_sg = ops.vd_project_sh(packed, pts, dirs, deg)
        torch.cuda.synchronize()
        assert co.intact() and sg.intact(), deg
        assert co.written() and sg.written(), deg
        assert torch.equal(co.out.view(N, 3 * K), plain_co) and torch.equal(sg.out, plain_sg), deg
    # the head: cross form (R directions) and per-point form (N directions)
    for cross, dd in ((1, dirs), (0, _dirs(ctx, N))):
        n_dirs = dd.shape[0]
        rgb, sg = _Guarded(N * n_dirs * 3 if cross else N * 3, dev), _Guarded(N, dev)
        ws = torch.empty(ops.vd_eval_workspace_bytes(N, n_dirs, cross), dtype=torch.uint8, device=dev)
        rc = lib.pxo_vd_eval_points_raw(0, vp(packed), vp(pts), N, vp(dd), n_dirs, cross, vp(rgb.out), vp(sg.out), vp(ws), ws.numel(),
                                        ops._stream())
        assert rc == 0, lib.pxo_last_error()
        plain_rgb, plain_sg = ops.vd_eval_points_raw(packed, pts, dd, bool(cross))
        torch.cuda.synchronize()
        assert rgb.intact() and sg.intact(), cross
        assert rgb.written() and sg.written(), cross
        assert torch.equal(rgb.out, plain_rgb.reshape(-1)) and torch.equal(sg.out, plain_sg), cross


# ---- f. the workspace carries nothing in --------------------------------------------------------------------------------------
@pytest.mark.timeout(60)
@pytest.mark.parametrize("N,R", [(17, 9), (257, 65)])
def test_the_workspace_carries_nothing_in(ctx, N, R):
    """One workspace, larger than any of the calls needs and reused as it is: zero-filled, then filled with 0xFF bytes (a NaN in
    every float, all bits set in every mask word).  The padded rows of C and of the basis must be the kernels' own zeros.
    Degree 4 stands for all five: every degree reads a prefix of the same rows of C and of the basis."""
    ops, dev, packed = ctx["ops"], ctx["dev"], ctx["packed"]
    pts, dirs, dirs_n = ctx["pts"][:N].contiguous(), _dirs(ctx, R), _dirs(ctx, N)
    need = max(ops.vd_project_workspace_bytes(N, R), ops.vd_eval_workspace_bytes(N, R, True), ops.vd_eval_workspace_bytes(N, N, False))
    ws = torch.empty(2 * need + 4096, dtype=torch.uint8, device=dev)
    calls = {"project": lambda: ops.vd_project_sh(packed, pts, dirs, 4, ws=ws),
             "cross": lambda: ops.vd_eval_points_raw(packed, pts, dirs, True, ws=ws),
             "per point": lambda: ops.vd_eval_points_raw(packed, pts, dirs_n, False, ws=ws)}
    for name, call in calls.items():
        outs = []
        for fill in (0x00, 0xFF):
            ws.fill_(fill)
            ptr = ws.data_ptr()
            outs.append([t.clone() for t in call()])
            assert ws.data_ptr() == ptr
        for a, b in zip(*outs):
            assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
            assert torch.equal(a, b), name


# ---- g. compositing -----------------------------------------------------------------------------------------------------------
def _composite_inputs(B, S, seed, opaque):
    """As tests/test_gpu_parity.py _composite_inputs with three raw colour channels: randomised z in [2, 6], raw sigma ~ 3 N(0,1)
    (30 N(0,1): most samples saturate), directions of length 1 .. 1.1."""
    gen = torch.Generator().manual_seed(seed)
    rays = make_rays(B, seed)
    raw_rgb = torch.randn(B, S, 3, generator=gen)
    raw_sigma = torch.randn(B, S, 1, generator=gen) * (30.0 if opaque else 3.0)
    z, _ = O.sample_along_rays(rays.origins, rays.directions, S, 2.0, 6.0, torch.rand(B, S, generator=gen))
    assert float((rays.directions.norm(dim=-1) - 1).abs().min()) > 1e-4
    return rays.directions, raw_rgb, raw_sigma, z


def _close(name, got, want, rtol, atol):
    got, want = got.detach().cpu().double().reshape(-1), want.double().reshape(-1)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
    excess = ((got - want).abs() / (atol + rtol * want.abs())).max()
    print(f"{name}: worst |HIP - f64| / (atol + rtol |f64|) = {float(excess):.3f}")
    assert float(excess) <= 1.0, f"{name}: {float(excess):.3f} x the tolerance"


def _composite_raw(ctx, cfg, raw_rgb, raw_sigma, z, d, B, S, with_weights=True):
    dev = ctx["dev"]
    vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    comp, disp, acc = torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)
    w = torch.empty(B, S, device=dev) if with_weights else None
    rc = ctx["lib"].pxo_vd_composite_fwd(ctypes.byref(cfg), vp(raw_rgb), vp(raw_sigma), vp(z), vp(d), B, S, vp(comp), vp(disp), vp(acc),
                                         vp(w), ctx["ops"]._stream())
    return rc, comp, disp, acc, w


@pytest.mark.timeout(60)
@pytest.mark.parametrize("opaque", [False, True])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 255, 256])
def test_composite_against_the_float64_oracle(ctx, S, opaque):
    ops, dev = ctx["ops"], ctx["dev"]
    for B in (1, 4, 5, 37):
        d, raw_rgb, raw_sigma, z = _composite_inputs(B, S, 100 * S + B, opaque)
        args = (raw_rgb.reshape(B * S, 3).to(dev), raw_sigma.reshape(-1).to(dev), z.to(dev), d.to(dev))
        for white in (True, False):
            cfg = ops.make_cfg(white_bkgd=int(white))
            comp, disp, acc, w = ops.vd_composite_fwd(cfg, *args)
            c_ref, d_ref, a_ref, w_ref = O.volumetric_rendering(torch.sigmoid(raw_rgb.double()), torch.relu(raw_sigma.double()),
                                                                z.double(), d.double(), white)
            tag = f"S={S} B={B} white={white} opaque={opaque}"
            _close(f"comp {tag}", comp, c_ref, 1e-5, 2e-6)
            _close(f"acc {tag}", acc, a_ref, 1e-5, 2e-6)
            _close(f"weights {tag}", w, w_ref, 1e-4, 2e-6)
            _close(f"disp {tag}", disp, d_ref, 1e-4, 1e-6)
            # weights = NULL: the same comp, disp and acc
            rc, comp0, disp0, acc0, _ = _composite_raw(ctx, cfg, *args, B, S, with_weights=False)
            assert rc == 0
            assert torch.equal(comp0, comp) and torch.equal(disp0, disp) and torch.equal(acc0, acc), tag


@pytest.mark.timeout(60)
@pytest.mark.parametrize("S", [1, 63, 64, 65, 255, 256])
def test_composite_of_empty_space_is_the_background(ctx, S):
    ops, dev = ctx["ops"], ctx["dev"]
    B = 5
    d, raw_rgb, raw_sigma, z = _composite_inputs(B, S, 7 + S, False)
    raw_sigma = -raw_sigma.abs() - 1e-3
    for white in (True, False):
        comp, disp, acc, w = ops.vd_composite_fwd(ops.make_cfg(white_bkgd=int(white)), raw_rgb.reshape(B * S, 3).to(dev),
                                                  raw_sigma.reshape(-1).to(dev), z.to(dev), d.to(dev))
        assert torch.equal(comp.cpu(), torch.full((B, 3), 1.0 if white else 0.0))
        assert torch.equal(disp.cpu(), torch.full((B,), 1e10, dtype=torch.float32))
        assert torch.equal(acc.cpu(), torch.zeros(B)) and torch.equal(w.cpu(), torch.zeros(B, S))


@pytest.mark.timeout(60)
def test_composite_refuses_sample_counts_it_has_no_chunks_for(ctx):
    """S = 0 and S = 257 (a fifth chunk): PXO_ERR_ARG, and no launch -- the outputs keep their sentinel."""
    ops, dev = ctx["ops"], ctx["dev"]
    B = 4
    cfg = ops.make_cfg(white_bkgd=1)
    buf = torch.zeros(B * 257 * 3, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for S in (0, 257):
        outs = [torch.full((n,), SENTINEL, device=dev) for n in (B * 3, B, B, B * 257)]
        rc = ctx["lib"].pxo_vd_composite_fwd(ctypes.byref(cfg), vp(buf), vp(buf), vp(buf), vp(buf), B, S, *[vp(t) for t in outs],
                                             ops._stream())
        torch.cuda.synchronize()
        assert rc == -1, S
        assert b"samples per ray" in ctx["lib"].pxo_last_error()
        assert all(bool((t == SENTINEL).all()) for t in outs), S
