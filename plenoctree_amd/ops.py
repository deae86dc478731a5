"""torch-tensor front end of the C ABI (include/plenoctree_hip.h).

torch is used for device storage and the current HIP stream only; all arithmetic happens in
libplenoctree_hip.so.  Every tensor must be a contiguous float32 ROCm tensor.
"""
import ctypes

import torch

from . import _lib
from ._lib import NET_DEPTH, NET_WIDTH, ENC_PAD, PxoError, check, make_cfg  # noqa: F401


def _require_gpu():
    if not torch.cuda.is_available():
        raise PxoError("plenoctree_amd needs a ROCm GPU (gfx950); there is no CPU fallback")


def _p(t):
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise PxoError("tensor must be a contiguous ROCm tensor")
    return ctypes.c_void_p(t.data_ptr())


def _f(t):
    if t is not None and t.dtype != torch.float32:
        raise PxoError(f"expected float32, got {t.dtype}")
    return _p(t)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _new(*shape, device=None, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device=device or torch.device("cuda", torch.cuda.current_device()))


def sh_dim(cfg):
    return (cfg.sh_deg + 1) ** 2


def rgb_channels(cfg):
    return 3 * sh_dim(cfg)


def param_layout(cfg):
    """[(layer, is_bias, offset, rows, cols)] of ONE MLP's sub-arena and its size in floats."""
    lib = _lib.load()
    leaves = (_lib.PxoLeaf * _lib.NUM_LEAVES)()
    n = ctypes.c_int64(0)
    check(lib.pxo_param_layout(ctypes.byref(cfg), leaves, ctypes.byref(n)), "pxo_param_layout")
    return [(l.layer, l.is_bias, l.offset, l.rows, l.cols) for l in leaves], n.value


def packed_sizes(cfg):
    lib = _lib.load()
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    check(lib.pxo_packed_sizes(ctypes.byref(cfg), ctypes.byref(a), ctypes.byref(b)), "pxo_packed_sizes")
    return a.value, b.value


def pack_weights(cfg, mlp_params, packed_fwd=None, packed_bwd=None, need_bwd=True):
    _require_gpu()
    lib = _lib.load()
    nf, nb = packed_sizes(cfg)
    if packed_fwd is None:
        packed_fwd = _new(nf, device=mlp_params.device)
    if need_bwd and packed_bwd is None:
        packed_bwd = _new(nb, device=mlp_params.device)
    check(lib.pxo_pack_weights(ctypes.byref(cfg), _f(mlp_params), _f(packed_fwd),
                               _f(packed_bwd) if need_bwd else None, _stream()), "pxo_pack_weights")
    return packed_fwd, packed_bwd


def sample_along_rays(origins, directions, num_samples, near, far, t_rand=None, lindisp=False):
    _require_gpu()
    lib = _lib.load()
    B = origins.shape[0]
    z = _new(B, num_samples, device=origins.device)
    pts = _new(B, num_samples, 3, device=origins.device)
    check(lib.pxo_sample_along_rays(_f(origins), _f(directions), B, num_samples, near, far, int(lindisp),
                                    _f(t_rand), _f(z), _f(pts), _stream()), "pxo_sample_along_rays")
    return z, pts


def posenc(x):
    _require_gpu()
    lib = _lib.load()
    lead = x.shape[:-1]
    x2 = x.reshape(-1, 3).contiguous()
    enc = _new(x2.shape[0], _lib.ENC_DIM, device=x.device)
    check(lib.pxo_posenc(_f(x2), x2.shape[0], _f(enc), _stream()), "pxo_posenc")
    return enc.reshape(*lead, _lib.ENC_DIM)


def relu_mask_bytes(M):
    return _lib.load().pxo_relu_mask_bytes(M)


def dbias_partial_bytes(M):
    return _lib.load().pxo_dbias_partial_bytes(M)


def mlp_fwd(cfg, packed_fwd, pts, save=False, want_rgb=True):
    """-> raw_rgb [M,3K] (or None), raw_sigma [M], and if save: (acts [8,M,256], enc [M,64], mask)."""
    _require_gpu()
    lib = _lib.load()
    pts = pts.reshape(-1, 3)
    M = pts.shape[0]
    dev = pts.device
    raw_rgb = _new(M, rgb_channels(cfg), device=dev) if want_rgb else None
    raw_sigma = _new(M, device=dev)
    acts = enc = mask = None
    if save:
        acts = _new(NET_DEPTH, M, NET_WIDTH, device=dev)
        enc = _new(M, ENC_PAD, device=dev)
        mask = _new(max(relu_mask_bytes(M), 16), device=dev, dtype=torch.uint8)
    check(lib.pxo_mlp_fwd(ctypes.byref(cfg), _f(packed_fwd), _f(pts), M, _f(raw_rgb), _f(raw_sigma),
                          _f(acts), _f(enc), _p(mask), _stream()), "pxo_mlp_fwd")
    if save:
        return raw_rgb, raw_sigma, (acts, enc, mask)
    return raw_rgb, raw_sigma


def mlp_bwd_data(cfg, packed_bwd, d_raw_rgb, d_raw_sigma, mask):
    _require_gpu()
    lib = _lib.load()
    M = d_raw_sigma.shape[0]
    dev = d_raw_sigma.device
    dz = _new(NET_DEPTH, M, NET_WIDTH, device=dev)
    dbias = _new(max(dbias_partial_bytes(M) // 4, 4), device=dev)
    check(lib.pxo_mlp_bwd_data(ctypes.byref(cfg), _f(packed_bwd), _f(d_raw_rgb), _f(d_raw_sigma), _p(mask), M,
                               _f(dz), _f(dbias), _stream()), "pxo_mlp_bwd_data")
    return dz, dbias


def mlp_bwd_weights(cfg, acts, enc, dz, d_raw_rgb, d_raw_sigma, dbias):
    _require_gpu()
    lib = _lib.load()
    M = d_raw_sigma.shape[0]
    dev = d_raw_sigma.device
    _, n = param_layout(cfg)
    grads = _new(n, device=dev)
    nbytes = ctypes.c_size_t(0)
    check(lib.pxo_wgrad_workspace_bytes(ctypes.byref(cfg), M, ctypes.byref(nbytes)), "pxo_wgrad_workspace_bytes")
    ws = _new(max(nbytes.value, 16), device=dev, dtype=torch.uint8)
    check(lib.pxo_mlp_bwd_weights(ctypes.byref(cfg), _f(acts), _f(enc), _f(dz), _f(d_raw_rgb), _f(d_raw_sigma),
                                  _f(dbias), M, _f(grads), _p(ws), nbytes.value, _stream()),
          "pxo_mlp_bwd_weights")
    return grads


def shade_composite_fwd(cfg, raw_rgb, raw_sigma, z_vals, directions, viewdirs):
    _require_gpu()
    lib = _lib.load()
    B, S = z_vals.shape
    dev = z_vals.device
    comp, disp, acc, w = _new(B, 3, device=dev), _new(B, device=dev), _new(B, device=dev), _new(B, S, device=dev)
    check(lib.pxo_shade_composite_fwd(ctypes.byref(cfg), _f(raw_rgb), _f(raw_sigma), _f(z_vals), _f(directions),
                                      _f(viewdirs), B, S, _f(comp), _f(disp), _f(acc), _f(w), _stream()),
          "pxo_shade_composite_fwd")
    return comp, disp, acc, w


def shade_composite_bwd(cfg, raw_rgb, raw_sigma, z_vals, directions, viewdirs, d_comp_rgb):
    _require_gpu()
    lib = _lib.load()
    B, S = z_vals.shape
    dev = z_vals.device
    d_rgb = _new(B * S, rgb_channels(cfg), device=dev)
    d_sigma = _new(B * S, device=dev)
    check(lib.pxo_shade_composite_bwd(ctypes.byref(cfg), _f(raw_rgb), _f(raw_sigma), _f(z_vals), _f(directions),
                                      _f(viewdirs), _f(d_comp_rgb), B, S, _f(d_rgb), _f(d_sigma), _stream()),
          "pxo_shade_composite_bwd")
    return d_rgb, d_sigma


def sample_pdf(z_coarse, w_coarse, origins, directions, num_fine, u=None):
    _require_gpu()
    lib = _lib.load()
    B, Nc = z_coarse.shape
    dev = z_coarse.device
    z = _new(B, Nc + num_fine, device=dev)
    pts = _new(B, Nc + num_fine, 3, device=dev)
    check(lib.pxo_sample_pdf(_f(z_coarse), _f(w_coarse), _f(origins), _f(directions), B, Nc, num_fine, _f(u),
                             _f(z), _f(pts), _stream()), "pxo_sample_pdf")
    return z, pts


def add_gaussian_noise(raw, noise_std, noise=None, seed=0, stream_id=0):
    """model_utils.add_gaussian_noise in place: raw += noise_std * N(0,1) (`noise`: injected draws, else Philox)."""
    _require_gpu()
    check(_lib.load().pxo_add_gaussian_noise(_f(raw), raw.numel(), float(noise_std), _f(noise), seed, stream_id, _stream()),
          "pxo_add_gaussian_noise")
    return raw


def uniform(seed, stream_id, n, lo=0.0, hi=1.0, device=None):
    _require_gpu()
    lib = _lib.load()
    out = _new(n, device=device)
    check(lib.pxo_uniform(seed, stream_id, n, lo, hi, _f(out), _stream()), "pxo_uniform")
    return out


def adam_step(params, m, v, grads, lr, step, grad_scale=1.0):
    _require_gpu()
    lib = _lib.load()
    check(lib.pxo_adam_step(_f(params), _f(m), _f(v), _f(grads), params.numel(), float(lr), int(step),
                            float(grad_scale), _stream()), "pxo_adam_step")


def adam_pack_step(cfg, params, m, v, grads, lr, step, packed, grad_scale=1.0):
    """Adam on the whole arena + refresh of the weight images `packed` = [(fwd0, bwd0), (fwd1, bwd1)] in one launch."""
    _require_gpu()
    lib = _lib.load()
    (f0, b0), (f1, b1) = packed
    check(lib.pxo_adam_pack_step(ctypes.byref(cfg), _f(params), _f(m), _f(v), _f(grads), float(lr), int(step),
                                 float(grad_scale), _f(f0), _f(b0), _f(f1), _f(b1), _stream()), "pxo_adam_pack_step")


def _train_outputs(raw_rgb, B, S, n_sp, want_rgb, want_weights):
    """The output dict of the *_shade_composite_train wrappers for raw_rgb [B*S + n_sp, 3K]."""
    C = raw_rgb.shape[-1]
    dev = raw_rgb.device
    return {"comp_rgb": _new(B, 3, device=dev) if want_rgb else None,
            "weights": _new(B, S, device=dev) if want_weights else None,
            "ray_sse": _new(B, device=dev), "d_raw_rgb": _new(B * S + n_sp, C, device=dev),
            "d_raw_sigma": _new(B * S + n_sp, device=dev), "sp_exp": _new(max(n_sp, 1), device=dev)}


def shade_composite_train(cfg, raw_rgb, raw_sigma, z_vals, directions, viewdirs, pixels, n_sp=0, want_rgb=True,
                          want_weights=True):
    """Forward compositing + pixel loss + reverse in one launch: returns dict(comp_rgb, weights, ray_sse, d_raw_rgb,
    d_raw_sigma, sp_exp).  raw_rgb [B*S + n_sp, 3K], raw_sigma [B*S + n_sp]."""
    _require_gpu()
    lib = _lib.load()
    B, S = z_vals.shape
    out = _train_outputs(raw_rgb, B, S, n_sp, want_rgb, want_weights)
    check(lib.pxo_shade_composite_train(ctypes.byref(cfg), _f(raw_rgb), _f(raw_sigma), _f(z_vals), _f(directions),
                                        _f(viewdirs), _f(pixels), B, S, _f(out["comp_rgb"]), _f(out["weights"]),
                                        _f(out["ray_sse"]), _f(out["d_raw_rgb"]), _f(out["d_raw_sigma"]), n_sp,
                                        _f(out["sp_exp"]), _stream()), "pxo_shade_composite_train")
    return out


def render_workspace_bytes(cfg, B):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_render_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(n)), "pxo_render_workspace_bytes")
    return n.value


def train_workspace_bytes(cfg, B):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_train_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(n)), "pxo_train_workspace_bytes")
    return n.value


def _check_lobes(cfg, lobes):
    if lobes is not None:
        K = (cfg.sh_deg + 1) ** 2
        if lobes.dtype != torch.float32 or tuple(lobes.shape) != (K, 4) or not lobes.is_contiguous() or not lobes.is_cuda:
            raise PxoError(f"SG lobes must be a contiguous float32 [{K}, 4] tensor on the GPU")


def _render_outputs(cfg, B, dev):
    """The [(rgb, disp, acc)] list of the levels a render returns, and the six pointers the library takes (NULL without a fine level)."""
    outs = [(_new(B, 3, device=dev), _new(B, device=dev), _new(B, device=dev)) for _ in range(2 if cfg.num_fine_samples > 0 else 1)]
    return outs, [_f(x) for lvl in outs for x in lvl] + [None] * (6 - 3 * len(outs))


def _train_args(packed, origins, directions, viewdirs, pixels, randomized, t_rand, u, sp_points, seed, grads, stats, ws, grads0_ready):
    """What the three train entry points share: the arguments from the packed images to `grads`, and those from `stats` on."""
    (f0, b0), (f1, b1) = packed
    head = (_f(f0), _f(b0), _f(f1), _f(b1), _f(origins), _f(directions), _f(viewdirs), _f(pixels), origins.shape[0], int(randomized),
            _f(t_rand), _f(u), _f(sp_points), seed, _f(grads))
    return head, (_f(stats), _p(ws), ws.numel(), grads0_ready.handle if grads0_ready is not None else None, _stream())


def render_fwd(cfg, packed_fwd0, packed_fwd1, origins, directions, viewdirs, randomized=False, t_rand=None, u=None,
               seed=0, ws=None, lobes=None):
    """NerfModel.__call__ forward: [(rgb,disp,acc)_coarse, (rgb,disp,acc)_fine].  lobes [K,4] with K = (cfg.sh_deg+1)^2: the
    model is a NeRF-SG with sg_dim = K (pxo_sg_render_fwd) and is shaded with that basis instead of SH."""
    _require_gpu()
    _check_lobes(cfg, lobes)
    lib = _lib.load()
    B = origins.shape[0]
    dev = origins.device
    nbytes = render_workspace_bytes(cfg, B)
    if ws is None or ws.numel() < nbytes:
        ws = _new(max(nbytes, 16), device=dev, dtype=torch.uint8)
    outs, out_ptrs = _render_outputs(cfg, B, dev)
    tail = (_f(packed_fwd0), _f(packed_fwd1), _f(origins), _f(directions), _f(viewdirs), B, int(randomized), _f(t_rand), _f(u),
            seed, *out_ptrs, _p(ws), ws.numel(), _stream())
    if lobes is None:
        check(lib.pxo_render_fwd(ctypes.byref(cfg), *tail), "pxo_render_fwd")
    else:
        check(lib.pxo_sg_render_fwd(ctypes.byref(cfg), _f(lobes), *tail), "pxo_sg_render_fwd")
    return outs


def train_fwd_bwd(cfg, params, packed, origins, directions, viewdirs, pixels, grads, stats, ws, randomized=True,
                  t_rand=None, u=None, sp_points=None, seed=0, grads0_ready=None):
    """loss_fn + value_and_grad on this device's shard; fills grads (2-MLP arena) and stats[6].
    grads0_ready: an `Event` recorded on the current stream once MLP_0's half of `grads` is final (the coarse level is
    reversed before the fine level starts), or None."""
    _require_gpu()
    head, tail = _train_args(packed, origins, directions, viewdirs, pixels, randomized, t_rand, u, sp_points, seed, grads, stats, ws,
                             grads0_ready)
    check(_lib.load().pxo_train_fwd_bwd_bucketed(ctypes.byref(cfg), _f(params), *head, *tail), "pxo_train_fwd_bwd_bucketed")


# ---- training a NeRF-SG: the pxo_sg_* entry points beside the three above -----------------------------------------------------
def sg_lobes(sg_params, K, lobes=None):
    """pxo_sg_lobes: raw sg_params [3K] (sg_lambda [K], then sg_mu_spher [K,2]) -> lobes [K,4] on the device, on the stream."""
    _require_gpu()
    if sg_params.numel() != 3 * K:
        raise PxoError(f"sg_params has {sg_params.numel()} floats, sg_dim={K} needs {3 * K}")
    if lobes is None:
        lobes = _new(K, 4, device=sg_params.device)
    check(_lib.load().pxo_sg_lobes(_f(sg_params), int(K), _f(lobes), _stream()), "pxo_sg_lobes")
    return lobes


def sg_shade_composite_train(cfg, lobes, raw_rgb, raw_sigma, z_vals, directions, viewdirs, pixels, n_sp=0, want_rgb=True,
                             want_weights=True):
    """shade_composite_train with the SG basis of `lobes` [K,4]; the dict gains d_lobes [K,4], the gradient of the launch's pixel
    loss with respect to (lambda, mu)."""
    _require_gpu()
    lib = _lib.load()
    B, S = z_vals.shape
    K = sh_dim(cfg)
    dev = raw_rgb.device
    out = _train_outputs(raw_rgb, B, S, n_sp, want_rgb, want_weights)
    out["d_lobes"] = _new(K, 4, device=dev)
    partials = _new(max(-(-B // _lib.SG_RAYS_PER_BLOCK), 1) * K * 4, device=dev)
    check(lib.pxo_sg_shade_composite_train(ctypes.byref(cfg), _f(lobes), _f(raw_rgb), _f(raw_sigma), _f(z_vals), _f(directions),
                                           _f(viewdirs), _f(pixels), B, S, _f(out["comp_rgb"]), _f(out["weights"]),
                                           _f(out["ray_sse"]), _f(out["d_raw_rgb"]), _f(out["d_raw_sigma"]), n_sp,
                                           _f(out["sp_exp"]), _f(out["d_lobes"]), _f(partials), _stream()),
          "pxo_sg_shade_composite_train")
    return out


def sg_train_workspace_bytes(cfg, B):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_sg_train_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(n)), "pxo_sg_train_workspace_bytes")
    return n.value


def sg_train_fwd_bwd(cfg, params, sg_params, packed, origins, directions, viewdirs, pixels, grads, sg_grads, stats, ws,
                     randomized=True, t_rand=None, u=None, sp_points=None, seed=0, grads0_ready=None):
    """train_fwd_bwd of a NeRF-SG: sg_params [3K] in, sg_grads [3K] out (d total loss / d raw SG parameters, weight decay
    included); stats[5] counts the SG leaves."""
    _require_gpu()
    head, tail = _train_args(packed, origins, directions, viewdirs, pixels, randomized, t_rand, u, sp_points, seed, grads, stats, ws,
                             grads0_ready)
    check(_lib.load().pxo_sg_train_fwd_bwd_bucketed(ctypes.byref(cfg), _f(params), _f(sg_params), *head, _f(sg_grads), *tail),
          "pxo_sg_train_fwd_bwd_bucketed")


def train_backward_work(cfg, B, ws):
    """(live, total) 16-row chunks of the reverse pass of the last train_fwd_bwd call on workspace `ws` (synchronises)."""
    _require_gpu()
    live, total = ctypes.c_int64(0), ctypes.c_int64(0)
    check(_lib.load().pxo_train_backward_work(ctypes.byref(cfg), B, _p(ws), ws.numel(), ctypes.byref(live), ctypes.byref(total),
                                              _stream()), "pxo_train_backward_work")
    return live.value, total.value


class Event:
    """hipEvent_t owned through the C ABI (pxo_event_create): recorded by pxo_train_fwd_bwd_bucketed, waited for by
    `wait(stream)`."""

    def __init__(self):
        _require_gpu()
        h = ctypes.c_void_p(None)
        check(_lib.load().pxo_event_create(ctypes.byref(h)), "pxo_event_create")
        self.handle = h

    def wait(self, stream):
        """`stream` (a torch.cuda.Stream) continues once the last record of this event has completed."""
        check(_lib.load().pxo_stream_wait_event(ctypes.c_void_p(stream.cuda_stream), self.handle), "pxo_stream_wait_event")

    def __del__(self):
        try:
            if self.handle:
                _lib.load().pxo_event_destroy(self.handle)
        except Exception:
            pass


def eval_points(cfg, packed_fwd, points, want_rgb=True):
    """NerfModel.eval_points_raw: raw_rgb [N,3K] (or None), raw_sigma [N,1]."""
    _require_gpu()
    lib = _lib.load()
    points = points.reshape(-1, 3)
    N = points.shape[0]
    dev = points.device
    raw_rgb = _new(N, rgb_channels(cfg), device=dev) if want_rgb else None
    raw_sigma = _new(N, 1, device=dev)
    check(lib.pxo_eval_points(ctypes.byref(cfg), _f(packed_fwd), _f(points), N, _f(raw_rgb), _f(raw_sigma), _stream()),
          "pxo_eval_points")
    return raw_rgb, raw_sigma


def grid_sigma(cfg, packed_fwd, reso, x0, x1, offset, scale, out=None):
    """sigma on the dense grid slab x in [x0,x1) (octree/extraction.py:290-320)."""
    _require_gpu()
    lib = _lib.load()
    n = (x1 - x0) * reso * reso
    if out is None:
        out = _new(n, device=packed_fwd.device)
    off = (ctypes.c_float * 3)(*[float(v) for v in offset])
    sc = (ctypes.c_float * 3)(*[float(v) for v in scale])
    check(lib.pxo_grid_sigma(ctypes.byref(cfg), _f(packed_fwd), reso, x0, x1, off, sc, _f(out), _stream()),
          "pxo_grid_sigma")
    return out


PROF_MLP_FWD, PROF_MLP_BWD_DATA, PROF_WGRAD_MAIN, PROF_WGRAD_OTHER, PROF_NUM_TAGS = 0, 1, 2, 3, 4


TUNE_TILE_SCHED, TUNE_WGRAD_RANGES, TUNE_WGRAD_SKINNY_RANGES, TUNE_COARSE_REVERSE_STREAM, TUNE_X6_WGRAD = 0, 1, 2, 3, 4        # PXO_TUNE_* of include/plenoctree_hip.h
TUNE_VD_RAY_BLOCK = 5               # rays per internal block of vd_render_fwd (1 .. 4096, default 1024)


def set_tuning(knob, value):
    """pxo_set_tuning: choose between implementations of the same result (A/B sessions, equality tests)."""
    check(_lib.load().pxo_set_tuning(int(knob), int(value)), "pxo_set_tuning")


def get_tuning(knob):
    v = ctypes.c_int(0)
    check(_lib.load().pxo_get_tuning(int(knob), ctypes.byref(v)), "pxo_get_tuning")
    return v.value


def occupy_cus(blocks, threads, micros, stream=None, lds_bytes=0):
    """pxo_occupy_cus: `blocks` idle workgroups (each with `lds_bytes` of LDS) for `micros` us on `stream` (a torch.cuda.Stream;
    default: the current one)."""
    _require_gpu()
    h = ctypes.c_void_p(stream.cuda_stream) if stream is not None else _stream()
    check(_lib.load().pxo_occupy_cus(int(blocks), int(threads), float(micros), int(lds_bytes), h), "pxo_occupy_cus")


def profile_enable(on=True, tags=None):
    """HIP-event brackets around the tagged kernel launches: all tags (on=True), none (False), or the listed `tags`.
    Every bracket costs the stream two event records (~5 us each between kernels that would otherwise run back to back)."""
    mask = 0
    if tags is not None:
        for t in tags:
            mask |= 1 << int(t)
    elif on:
        mask = (1 << PROF_NUM_TAGS) - 1
    check(_lib.load().pxo_profile_enable(mask), "pxo_profile_enable")


def profile_read(tag):
    """(launches, total_ms, total_rows) of the kernels tagged `tag` since the last read."""
    n, ms, rows = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_int64(0)
    check(_lib.load().pxo_profile_read(tag, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(rows)), "pxo_profile_read")
    return n.value, ms.value, rows.value



def randint(seed, stream_id, count, n, device=None):
    """count uniform integers in [0, n) (int64) from the Philox stream."""
    _require_gpu()
    out = _new(count, device=device, dtype=torch.int64)
    check(_lib.load().pxo_randint(seed, stream_id, count, n, _p(out), _stream()), "pxo_randint")
    return out


def generate_rays(c2w, W, H, focal, pixel_ids=None, count=None):
    """Rays of the given pixels (or of pixels 0..count-1) of one camera: (origins, directions, viewdirs)."""
    _require_gpu()
    c2w = c2w[:3, :4].contiguous()
    B = pixel_ids.shape[0] if pixel_ids is not None else (count if count is not None else W * H)
    dev = c2w.device
    o, d, v = _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev)
    if pixel_ids is not None and pixel_ids.dtype != torch.int64:
        raise PxoError("pixel_ids must be int64")
    check(_lib.load().pxo_generate_rays(_f(c2w), W, H, float(focal), _p(pixel_ids), B, _f(o), _f(d), _f(v), _stream()),
          "pxo_generate_rays")
    return o, d, v


def sample_batch(seed, stream_id, c2w, W, H, focal, image_rgb, B, want_ids=False, first=0):
    """One training batch of one image in one launch: (origins, directions, viewdirs, pixels[, pixel_ids]); `first`: the B rows
    are elements first .. first + B - 1 of the stream (a rank's shard of one global draw)."""
    _require_gpu()
    c2w = c2w[:3, :4].contiguous()
    dev = c2w.device
    o, d, v, px = _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev)
    ids = _new(B, device=dev, dtype=torch.int64) if want_ids else None
    check(_lib.load().pxo_sample_batch(seed, stream_id, _f(c2w), W, H, float(focal), _f(image_rgb), B, int(first), _p(ids), _f(o), _f(d),
                                       _f(v), _f(px), _stream()), "pxo_sample_batch")
    return (o, d, v, px, ids) if want_ids else (o, d, v, px)


def generate_rays_multi(c2w_all, W, H, focal, ray_ids):
    """Rays of ids into the flattened [n_cams, H*W] table (image_batching): (origins, directions, viewdirs)."""
    _require_gpu()
    if ray_ids.dtype != torch.int64:
        raise PxoError("ray_ids must be int64")
    c2w_all = c2w_all[:, :3, :4].contiguous()
    B = ray_ids.shape[0]
    dev = c2w_all.device
    o, d, v = _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev)
    check(_lib.load().pxo_generate_rays_multi(_f(c2w_all), c2w_all.shape[0], W, H, float(focal), _p(ray_ids), B,
                                              _f(o), _f(d), _f(v), _stream()), "pxo_generate_rays_multi")
    return o, d, v


def generate_rays_ndc(c2w, W, H, focal, pixel_ids=None, count=None, ndc_near=1.0):
    """generate_rays taken through the reference's convert_to_ndc (forward-facing scenes): (origins, directions) in normalised
    device coordinates, viewdirs the world-space unit directions."""
    _require_gpu()
    c2w = c2w[:3, :4].contiguous()
    B = pixel_ids.shape[0] if pixel_ids is not None else (count if count is not None else W * H)
    dev = c2w.device
    o, d, v = _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev)
    if pixel_ids is not None and pixel_ids.dtype != torch.int64:
        raise PxoError("pixel_ids must be int64")
    check(_lib.load().pxo_generate_rays_ndc(_f(c2w), 1, W, H, float(focal), float(ndc_near), _p(pixel_ids), B, _f(o), _f(d),
                                            _f(v), _stream()), "pxo_generate_rays_ndc")
    return o, d, v


def generate_rays_multi_ndc(c2w_all, W, H, focal, ray_ids, ndc_near=1.0):
    """generate_rays_multi taken through convert_to_ndc (image_batching over a forward-facing scene)."""
    _require_gpu()
    if ray_ids.dtype != torch.int64:
        raise PxoError("ray_ids must be int64")
    c2w_all = c2w_all[:, :3, :4].contiguous()
    B = ray_ids.shape[0]
    dev = c2w_all.device
    o, d, v = _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev)
    check(_lib.load().pxo_generate_rays_ndc(_f(c2w_all), c2w_all.shape[0], W, H, float(focal), float(ndc_near), _p(ray_ids), B,
                                            _f(o), _f(d), _f(v), _stream()), "pxo_generate_rays_ndc")
    return o, d, v


def sample_batch_ndc(seed, stream_id, c2w, W, H, focal, image_rgb, B, want_ids=False, first=0, ndc_near=1.0):
    """sample_batch with NDC rays, in one launch: (origins, directions, viewdirs, pixels[, pixel_ids])."""
    _require_gpu()
    c2w = c2w[:3, :4].contiguous()
    dev = c2w.device
    o, d, v, px = _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev), _new(B, 3, device=dev)
    ids = _new(B, device=dev, dtype=torch.int64) if want_ids else None
    check(_lib.load().pxo_sample_batch_ndc(seed, stream_id, _f(c2w), W, H, float(focal), float(ndc_near), _f(image_rgb), B,
                                           int(first), _p(ids), _f(o), _f(d), _f(v), _f(px), _stream()), "pxo_sample_batch_ndc")
    return (o, d, v, px, ids) if want_ids else (o, d, v, px)


def mean_over_samples(cfg, raw_rgb, raw_sigma, samples_per_cell, out=None):
    _require_gpu()
    n = raw_sigma.numel() // samples_per_cell
    if out is None:
        out = _new(n, rgb_channels(cfg) + 1, device=raw_sigma.device)
    elif out.numel() != n * (rgb_channels(cfg) + 1):
        raise PxoError("mean_over_samples: `out` has the wrong size")
    check(_lib.load().pxo_mean_over_samples(ctypes.byref(cfg), _f(raw_rgb), _f(raw_sigma.reshape(-1)), n,
                                            samples_per_cell, _f(out), _stream()), "pxo_mean_over_samples")
    return out


# ---- view-conditioned NeRF (use_viewdirs = true): the pxo_vd_* entry points -------------------------------------------------
def vd_param_layout():
    """[(layer, is_bias, offset, rows, cols)] of ONE view-conditioned MLP's sub-arena (Dense_0..11) and its size in floats."""
    leaves = (_lib.PxoLeaf * _lib.VD_NUM_LEAVES)()
    n = ctypes.c_int64(0)
    check(_lib.load().pxo_vd_param_layout(leaves, ctypes.byref(n)), "pxo_vd_param_layout")
    return [(l.layer, l.is_bias, l.offset, l.rows, l.cols) for l in leaves], n.value


def vd_packed_floats():
    n = ctypes.c_int64(0)
    check(_lib.load().pxo_vd_packed_floats(ctypes.byref(n)), "pxo_vd_packed_floats")
    return n.value


def vd_pack_weights(mlp_params, packed=None):
    _require_gpu()
    if packed is None:
        packed = _new(vd_packed_floats(), device=mlp_params.device)
    check(_lib.load().pxo_vd_pack_weights(_f(mlp_params), _f(packed), _stream()), "pxo_vd_pack_weights")
    return packed


def _ws(ws, nbytes, device):
    if ws is None or ws.numel() < nbytes:
        ws = _new(max(nbytes, 16), device=device, dtype=torch.uint8)
    return ws


def vd_eval_workspace_bytes(N, R, cross_broadcast):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_vd_eval_workspace_bytes(N, R, int(bool(cross_broadcast)), ctypes.byref(n)), "pxo_vd_eval_workspace_bytes")
    return n.value


def vd_eval_points_raw(packed, points, viewdirs=None, cross_broadcast=False, ws=None, mlp_precision=0):
    """eval_points_raw of the view-conditioned model: raw_rgb [N,R,3] (cross_broadcast) or [N,3] (or None without viewdirs),
    raw_sigma [N]."""
    _require_gpu()
    points = points.reshape(-1, 3)
    N, dev = points.shape[0], points.device
    R = viewdirs.shape[0] if viewdirs is not None else 0
    raw_rgb = None
    if viewdirs is not None:
        raw_rgb = _new(N, R, 3, device=dev) if cross_broadcast else _new(N, 3, device=dev)
    raw_sigma = _new(N, device=dev)
    nbytes = vd_eval_workspace_bytes(N, R, cross_broadcast)
    ws = _ws(ws, nbytes, dev)
    check(_lib.load().pxo_vd_eval_points_raw(int(mlp_precision), _f(packed), _f(points), N, _f(viewdirs), R,
                                             int(bool(cross_broadcast)), _f(raw_rgb), _f(raw_sigma), _p(ws), ws.numel(),
                                             _stream()), "pxo_vd_eval_points_raw")
    return raw_rgb, raw_sigma


def vd_project_workspace_bytes(N, R):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_vd_project_workspace_bytes(N, R, ctypes.byref(n)), "pxo_vd_project_workspace_bytes")
    return n.value


def vd_project_sh(packed, points, dirs, sh_deg, ws=None, coeffs=None, raw_sigma=None, mlp_precision=0):
    """Fused SH projection: coeffs [N, 3K] (channel-major) and raw_sigma [N] for unit directions dirs [R,3]."""
    _require_gpu()
    points = points.reshape(-1, 3)
    N, dev = points.shape[0], points.device
    R = dirs.shape[0]
    K = (int(sh_deg) + 1) ** 2
    if coeffs is None:
        coeffs = _new(N, 3 * max(K, 1), device=dev)
    if raw_sigma is None:
        raw_sigma = _new(N, device=dev)
    n = ctypes.c_size_t(0)
    lib = _lib.load()
    if lib.pxo_vd_project_workspace_bytes(N, R, ctypes.byref(n)) != 0:
        n.value = 16                                       # the call below reports what is wrong with the arguments
    ws = _ws(ws, n.value, dev)
    check(lib.pxo_vd_project_sh(int(mlp_precision), _f(packed), _f(points), N, _f(dirs), R, int(sh_deg), _f(coeffs),
                                _f(raw_sigma), _p(ws), ws.numel(), _stream()), "pxo_vd_project_sh")
    return coeffs, raw_sigma


def vd_render_workspace_bytes(cfg, B):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_vd_render_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(n)), "pxo_vd_render_workspace_bytes")
    return n.value


def vd_render_fwd(cfg, packed0, packed1, origins, directions, viewdirs, randomized=False, t_rand=None, u=None, seed=0, ws=None):
    """NerfModel.__call__ of the view-conditioned model, forward: [(rgb,disp,acc)_coarse, (rgb,disp,acc)_fine] (the fine entry
    only with num_fine_samples > 0).  packed0/1: the vd_pack_weights images of MLP_0 / MLP_1."""
    _require_gpu()
    B, dev = origins.shape[0], origins.device
    ws = _ws(ws, vd_render_workspace_bytes(cfg, B), dev)
    outs = [(_new(B, 3, device=dev), _new(B, device=dev), _new(B, device=dev))]
    fine = cfg.num_fine_samples > 0
    if fine:
        outs.append((_new(B, 3, device=dev), _new(B, device=dev), _new(B, device=dev)))
    f = outs[1] if fine else (None, None, None)
    check(_lib.load().pxo_vd_render_fwd(ctypes.byref(cfg), _f(packed0), _f(packed1), _f(origins), _f(directions), _f(viewdirs), B,
                                        int(randomized), _f(t_rand), _f(u), seed, _f(outs[0][0]), _f(outs[0][1]),
                                        _f(outs[0][2]), _f(f[0]), _f(f[1]), _f(f[2]), _p(ws), ws.numel(), _stream()),
          "pxo_vd_render_fwd")
    return outs


def vd_composite_fwd(cfg, raw_rgb, raw_sigma, z_vals, directions):
    """sigmoid + relu + volumetric_rendering of the view-conditioned model: raw_rgb [B*S,3] -> (comp_rgb [B,3], disp [B], acc [B],
    weights [B,S])."""
    _require_gpu()
    B, S = z_vals.shape
    dev = z_vals.device
    comp, disp, acc, w = _new(B, 3, device=dev), _new(B, device=dev), _new(B, device=dev), _new(B, S, device=dev)
    check(_lib.load().pxo_vd_composite_fwd(ctypes.byref(cfg), _f(raw_rgb), _f(raw_sigma), _f(z_vals), _f(directions), B, S,
                                           _f(comp), _f(disp), _f(acc), _f(w), _stream()), "pxo_vd_composite_fwd")
    return comp, disp, acc, w


# ---- occupancy grid: ray rendering that skips empty samples (the pxo_occ_* entry points and pxo_render_fwd_culled) -----------
def occ_words(reso):
    """Words of the bit image of a reso^3 grid."""
    return (int(reso) ** 3 + 31) // 32


class OccupancyGrid:
    """One bit per cell of a reso^3 grid over the box t = p * scale + offset in [0,1)^3 (PxoOccGrid): `bits` int32 [occ_words(reso)] on
    the GPU, cell (x, y, z) at bit (x * reso + y) * reso + z.  outside_live: a sample outside the box is evaluated (True) or empty."""

    def __init__(self, bits, reso, offset, scale, outside_live=False):
        reso = int(reso)
        offset = [float(v) for v in offset]
        scale = [float(v) for v in scale]
        if not 1 <= reso <= _lib.OCC_MAX_RESO:
            raise PxoError(f"occupancy grid: reso {reso} outside [1, {_lib.OCC_MAX_RESO}]")
        if len(offset) != 3 or len(scale) != 3:
            raise PxoError("occupancy grid: offset and scale take three values each")
        if any(s == 0.0 or s != s or s in (float("inf"), float("-inf")) for s in scale):
            raise PxoError(f"occupancy grid: scale {scale} has a zero or non-finite entry")
        if bits is None or bits.dtype != torch.int32 or bits.numel() != occ_words(reso) or not bits.is_contiguous():
            raise PxoError(f"occupancy grid: bits must be a contiguous int32 tensor of {occ_words(reso)} words (reso {reso})")
        self.bits, self.reso, self.offset, self.scale, self.outside_live = bits, reso, offset, scale, bool(outside_live)

    def struct(self):
        g = _lib.PxoOccGrid()
        g.bits = self.bits.data_ptr()
        g.reso = self.reso
        g.offset = (ctypes.c_float * 3)(*self.offset)
        g.scale = (ctypes.c_float * 3)(*self.scale)
        g.outside_live = int(self.outside_live)
        return g

    def count_occupied(self):
        b = self.bits.to(torch.int64) & 0xFFFFFFFF
        n = 0
        for shift in range(0, 32, 8):                      # popcount by bytes through a 256-entry table
            n += int(_POPCOUNT8.to(b.device)[(b >> shift) & 0xFF].sum())
        return n

    def fraction_occupied(self):
        return self.count_occupied() / float(self.reso ** 3)


_POPCOUNT8 = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64)


def occ_pack(sigma, reso, sigma_thresh, dilate=1, bits=None):
    """pxo_occ_pack: sigma [reso^3] (grid_sigma's order) -> the bit image (int32 [occ_words(reso)]); a cell is occupied iff a cell of
    the grid within Chebyshev distance `dilate` has sigma > sigma_thresh (or NaN)."""
    _require_gpu()
    reso = int(reso)
    if not 1 <= reso <= _lib.OCC_MAX_RESO:
        raise PxoError(f"occ_pack: reso {reso} outside [1, {_lib.OCC_MAX_RESO}]")
    if sigma.numel() != reso ** 3:
        raise PxoError(f"occ_pack: sigma has {sigma.numel()} values, reso {reso} needs {reso ** 3}")
    if bits is None:
        bits = _new(occ_words(reso), device=sigma.device, dtype=torch.int32)
    elif bits.numel() != occ_words(reso) or bits.dtype != torch.int32:
        raise PxoError("occ_pack: `bits` has the wrong size or type")
    check(_lib.load().pxo_occ_pack(_f(sigma), reso, float(sigma_thresh), int(dilate), _p(bits), _stream()), "pxo_occ_pack")
    return bits


def occ_cull(occ, pts):
    """pxo_occ_cull: (pts_live [M,3] whose first n_live rows are the live points in order, slot int32 [M], n_live int64 [1] on the
    device)."""
    _require_gpu()
    pts = pts.reshape(-1, 3)
    M, dev = pts.shape[0], pts.device
    pts_live = _new(M, 3, device=dev)
    slot = _new(M, device=dev, dtype=torch.int32)
    n_live = _new(1, device=dev, dtype=torch.int64)
    n = ctypes.c_size_t(0)
    lib = _lib.load()
    check(lib.pxo_occ_cull_workspace_bytes(M, ctypes.byref(n)), "pxo_occ_cull_workspace_bytes")
    ws = _new(max(n.value, 16), device=dev, dtype=torch.uint8)
    g = occ.struct()
    check(lib.pxo_occ_cull(ctypes.byref(g), _f(pts), M, _f(pts_live), _p(slot), _p(n_live), _p(ws), ws.numel(), _stream()),
          "pxo_occ_cull")
    return pts_live, slot, n_live


def occ_expand(raw_rgb_live, raw_sigma_live, slot, C):
    """pxo_occ_expand: dense raw_rgb [M,C] / raw_sigma [M] from the compact rows; a culled row is zero."""
    _require_gpu()
    if slot.dtype != torch.int32:
        raise PxoError("occ_expand: slot must be int32")
    M, dev = slot.numel(), slot.device
    raw_rgb, raw_sigma = _new(M, C, device=dev), _new(M, device=dev)
    check(_lib.load().pxo_occ_expand(_f(raw_rgb_live), _f(raw_sigma_live), _p(slot), M, int(C), _f(raw_rgb), _f(raw_sigma),
                                     _stream()), "pxo_occ_expand")
    return raw_rgb, raw_sigma


def render_culled_workspace_bytes(cfg, B):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_render_culled_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(n)), "pxo_render_culled_workspace_bytes")
    return n.value


def render_fwd_culled(cfg, occ, packed_fwd0, packed_fwd1, origins, directions, viewdirs, randomized=False, t_rand=None, u=None,
                      seed=0, ws=None, lobes=None, live_rows=None):
    """render_fwd with each level's MLP run only on the samples `occ` (an OccupancyGrid) calls live.  Returns render_fwd's list;
    live_rows (a list, optional) receives the rows that went through MLP_0 and MLP_1.  Synchronises the stream twice."""
    _require_gpu()
    if not isinstance(occ, OccupancyGrid):
        raise PxoError("render_fwd_culled: occ must be an ops.OccupancyGrid")
    _check_lobes(cfg, lobes)
    B, dev = origins.shape[0], origins.device
    ws = _ws(ws, render_culled_workspace_bytes(cfg, B), dev)
    outs, out_ptrs = _render_outputs(cfg, B, dev)
    rows = (ctypes.c_int64 * 2)(0, 0)
    g = occ.struct()
    check(_lib.load().pxo_render_fwd_culled(ctypes.byref(cfg), ctypes.byref(g), _f(lobes), _f(packed_fwd0), _f(packed_fwd1),
                                            _f(origins), _f(directions), _f(viewdirs), B, int(randomized), _f(t_rand), _f(u), seed,
                                            *out_ptrs, rows, _p(ws), ws.numel(), _stream()), "pxo_render_fwd_culled")
    if live_rows is not None:
        live_rows[:] = [rows[0], rows[1]]
    return outs


# ---- training through the occupancy grid ---------------------------------------------------------------------------------------
def occ_gather(d_raw_rgb, d_raw_sigma, slot, d_rgb_live=None, d_sigma_live=None):
    """pxo_occ_gather, the inverse of occ_expand: dense row m of d_raw_rgb [M,C] / d_raw_sigma [M] with slot[m] >= 0 goes to row
    slot[m] of (d_rgb_live [M,C], d_sigma_live [M]); rows with slot[m] < 0 are dropped, compact rows no slot names are left as
    they were (the outputs are allocated uninitialised unless given)."""
    _require_gpu()
    if slot.dtype != torch.int32:
        raise PxoError("occ_gather: slot must be int32")
    M, dev = slot.numel(), slot.device
    d_raw_rgb = d_raw_rgb.reshape(M, -1) if M else d_raw_rgb.reshape(0, max(d_raw_rgb.shape[-1], 1))
    C = d_raw_rgb.shape[1]
    if d_raw_sigma.numel() != M:
        raise PxoError(f"occ_gather: d_raw_sigma has {d_raw_sigma.numel()} rows, slot {M}")
    if d_rgb_live is None:
        d_rgb_live = _new(M, C, device=dev)
    if d_sigma_live is None:
        d_sigma_live = _new(M, device=dev)
    if d_rgb_live.numel() != M * C or d_sigma_live.numel() != M:
        raise PxoError("occ_gather: the compact outputs must have room for all M rows")
    check(_lib.load().pxo_occ_gather(_f(d_raw_rgb), _f(d_raw_sigma), _p(slot), M, int(C), _f(d_rgb_live), _f(d_sigma_live),
                                     _stream()), "pxo_occ_gather")
    return d_rgb_live, d_sigma_live


def train_culled_workspace_bytes(cfg, B):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_train_culled_workspace_bytes(ctypes.byref(cfg), B, ctypes.byref(n)), "pxo_train_culled_workspace_bytes")
    return n.value


def train_fwd_bwd_culled(cfg, occ, params, packed, origins, directions, viewdirs, pixels, grads, stats, ws, randomized=True,
                         t_rand=None, u=None, sp_points=None, seed=0, grads0_ready=None, live_rows=None):
    """train_fwd_bwd with both levels' MLPs, forward and reverse, run only on the samples `occ` (an OccupancyGrid; None is refused
    by the library) calls live; ws of train_culled_workspace_bytes.  live_rows (a list, optional) receives the live sample rows
    of the two levels.  Synchronises the stream twice."""
    _require_gpu()
    if occ is not None and not isinstance(occ, OccupancyGrid):
        raise PxoError("train_fwd_bwd_culled: occ must be an ops.OccupancyGrid")
    head, tail = _train_args(packed, origins, directions, viewdirs, pixels, randomized, t_rand, u, sp_points, seed, grads, stats, ws,
                             grads0_ready)
    rows = (ctypes.c_int64 * 2)(0, 0)
    g = occ.struct() if occ is not None else None
    check(_lib.load().pxo_train_fwd_bwd_culled(ctypes.byref(cfg), ctypes.byref(g) if g is not None else None, _f(params), *head,
                                               *tail, rows), "pxo_train_fwd_bwd_culled")
    if live_rows is not None:
        live_rows[:] = [rows[0], rows[1]]
