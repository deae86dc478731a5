"""Host side of the octree renderer's extra outputs (alpha, depth, surface distance; no GPU): the names exist at every
layer, the two C entry points decide their argument errors on the host before any launch, the CPU restatement the GPU
tests compare against (tests/_octree_aux_oracle.py) is consistent with oracle/octree_oracle.py and with the definitions,
the cases of the GPU tests stay under their cap of rays left out of the surface comparison, and the file writers of
octree.evaluation (--write_aux, --write_points) write what they document."""
import ctypes
import os

import numpy as np
import pytest

import _octree_aux_cases as C
import _octree_aux_oracle as A
from oracle import octree_oracle as T
from plenoctree_amd import _lib, build

f32 = np.float32
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "plenoctree_octree.h")
NEW = ("pxo_octree_render_aux_fwd", "pxo_octree_render_quant_aux_fwd")


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


# ---- names ----------------------------------------------------------------------------------------------------------
def test_names_exist_at_every_layer(lib):
    with open(HEADER) as f:
        header = f.read()
    for name in NEW:
        assert f"int {name}(" in header and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the extra arguments: surface_thresh (float) before the outputs, out_aux after out_rgb
    assert _lib.SIGNATURES[NEW[0]][1][7] is ctypes.c_float and len(_lib.SIGNATURES[NEW[0]][1]) == 11
    assert _lib.SIGNATURES[NEW[1]][1][7] is ctypes.c_float and len(_lib.SIGNATURES[NEW[1]][1]) == 11
    from plenoctree_amd import octree_ops
    from plenoctree_amd.octree import evaluation, svox
    assert callable(octree_ops.octree_render_aux_persp) and callable(octree_ops.octree_render_aux_rays)
    assert callable(svox.VolumeRenderer.render_persp_aux) and callable(svox.VolumeRenderer.forward_aux)
    args = evaluation.define_flags().parse_args([])
    assert (args.write_aux, args.write_points, args.points_stride, args.surface_thresh) == (None, None, 4, 0.5)
    args = evaluation.define_flags().parse_args(["--write_aux", "d", "--write_points", "p.ply", "--points_stride", "3",
                                                 "--surface_thresh", "0.25"])
    assert (args.write_aux, args.write_points, args.points_stride, args.surface_thresh) == ("d", "p.ply", 3, 0.25)


def test_eval_octree_keyword_defaults_to_off():
    import inspect
    from plenoctree_amd.octree import extraction
    sig = inspect.signature(extraction.eval_octree)
    assert sig.parameters["aux_sink"].default is None and sig.parameters["surface_thresh"].default == 0.5


# ---- argument errors decided on the host ----------------------------------------------------------------------------
def _float_tree():
    t = _lib.PxoTree()
    t.child, t.data, t.n_internal, t.data_dim, t.basis_dim = 256, 256, 5, 49, 16       # never dereferenced
    t.offset = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    t.invradius = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    return t


def _quant_tree():
    t = _lib.PxoQuantTree()
    t.child, t.idx, t.palette, t.sigma, t.retained = 256, 256, 256, 256, 256
    t.n_internal, t.idx_stride, t.ret_stride = 5, 16, 0
    t.basis_dim, t.n_retained, t.bits = 16, 0, 8
    return t


@pytest.mark.parametrize("which", [0, 1], ids=["float", "palette"])
def test_c_abi_rejects_bad_arguments(lib, which):
    """PXO_ERR_ARG (-1), all decided on the host before any launch: the pointers below are never dereferenced."""
    fn = getattr(lib, NEW[which])
    tree = (_float_tree, _quant_tree)[which]()
    p = ctypes.c_void_p(256)
    exact, fast = _lib.PxoRenderOpts(1e-3, 1.0, 0.0, 0.0), _lib.PxoRenderOpts(1e-3, 1.0, 1e-2, 1e-2)
    call = lambda opts, thresh, B=0, out=p, aux=p, tr=tree: fn(ctypes.byref(tr) if tr is not None else None, None, p, p, p, B,
                                                                 ctypes.byref(opts) if opts is not None else None, thresh, out,
                                                                 aux, None)
    assert call(exact, 0.5) == 0 and call(fast, 0.5) == 0                    # B = 0 returns ok
    assert call(exact, 0.5, aux=None) == 0                                  # ... before the outputs are looked at, as for out_rgb
    assert call(exact, 0.5, B=4, aux=None) == -1                            # null out_aux
    assert b"null output" in lib.pxo_last_error()
    assert call(exact, 0.5, B=4, out=None) == -1
    assert call(fast, 1e-2) == -1                                           # surface_thresh equal to stop_thresh
    assert b"surface_thresh" in lib.pxo_last_error()
    assert call(exact, 0.0) == -1
    assert call(fast, 5e-3) == -1                                           # below stop_thresh
    assert call(exact, -0.1) == -1
    assert call(exact, 1.0) == -1 and call(exact, 1.5) == -1                # surface_thresh = 1 and above
    assert call(exact, float("nan")) == -1
    # the checks of the renderer without the extra outputs
    assert call(None, 0.5) == -1 and call(exact, 0.5, tr=None) == -1 and call(exact, 0.5, B=-1) == -1
    assert call(_lib.PxoRenderOpts(0.0, 1.0, 0.0, 0.0), 0.5) == -1          # step_size 0
    bad = (_float_tree, _quant_tree)[which]()
    bad.basis_dim = 7
    assert call(exact, 0.5, tr=bad) == -1
    cam = _lib.PxoCamera(256, 10.0, 10.0, 4, 3)
    assert fn(ctypes.byref(tree), ctypes.byref(cam), None, None, None, 11, ctypes.byref(exact), 0.5, p, p, None) == -1   # B != W*H


# ---- the CPU restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", C.KS)
def test_helper_is_consistent_with_the_oracle_and_the_definitions(K):
    t = C.tree(K)
    for config, (cam, _, bg, fast) in C.CONFIGS.items():
        b32, b64 = C.reference(K, config)
        opt = C.options(config)
        if cam is None:
            o, d = C.explicit_rays(K)
            want = np.stack([T.render_ray(t, oo, dd, dd, opt) for oo, dd in zip(o, d)])
        else:
            want = T.render_persp(t, C.pose(*cam), C.W, C.H, C.FX, opt).reshape(-1, 3)
        assert np.array_equal(b32.rgb, want)                                 # bit for bit
        for b, eps in ((b32, 2.0 ** -24), (b64, 2.0 ** -53)):
            alpha, depth, surface = b.aux.T
            miss = b.light == 1.0
            # alpha = 1 - light: a sum of at most a few hundred terms <= 1 each rounded once (the rescaled ray: / (1 - light))
            want_alpha = np.where(b.stopped, 1.0, 1.0 - b.light)
            assert np.abs(alpha - want_alpha).max() <= 512 * eps
            assert (depth <= alpha * b.s_max * (1 + 512 * eps)).all() and (depth >= 0).all()
            assert (alpha[miss] == 0).all() and (depth[miss] == 0).all() and np.isinf(surface[miss]).all()
            # surface is finite exactly where the transmittance fell to the threshold, and is one of the ray's distances
            assert np.array_equal(np.isfinite(surface), b.light <= C.SURFACE_THRESH)
            assert (surface[np.isfinite(surface)] <= b.s_max).all() and (surface > 0).all()
        assert np.array_equal(b32.stopped, b64.stopped) and b32.stopped.any() == fast
        # round-off of the definitions in float32, far inside the bounds of the GPU test (2e-5, 2e-5 s_max)
        assert np.abs(b32.aux[:, 0] - b64.aux[:, 0]).max() < 1e-6
        assert np.abs(b32.aux[:, 1] - b64.aux[:, 1]).max() < 1e-6 * b32.s_max
        # the case shows what the GPU test wants to see, and leaves at most 2 % of its rays out of the surface comparison
        assert b32.aux[:, 0].max() > 0.5 and (b32.aux[:, 0] == 0).any()
        left_out = T.surface_excluded(b32, b64, C.SURFACE_THRESH)
        assert left_out.mean() <= 0.02, (config, int(left_out.sum()))
        assert np.isfinite(b32.aux[~left_out, 2]).sum() >= 20
    o, d = C.explicit_rays(K)
    r32, r64 = A.render_ray_aux(t, o[-1], d[-1], d[-1], C.options("rays"))      # the ray that misses
    for r in (r32, r64):
        assert (float(r.alpha), float(r.depth), float(r.surface)) == (0.0, 0.0, np.inf) and (r.rgb == 0.5).all()
    assert b32.light[-1] == 1.0 and np.isinf(b32.aux[-1, 2])


def test_helper_sample_distance_is_measured_from_the_origin():
    """One opaque slab: a tree whose root cells all hold a huge sigma; a ray along +x from x = -3 enters the volume
    (radius 1, centre 0) at distance 2, so the first sample's middle lies at 2 + delta_0 / 2 in world units."""
    t = T.Tree(4, 1, [0.0, 0.0, 0.0], 1.0)
    t.data[..., -1] = 1e4
    opt = T.RenderOptions(1e-3)
    o, d = np.array([-3.0, 0.1, 0.2], f32), np.array([1.0, 0.0, 0.0], f32)
    m = T.march(t, o, d, opt.step_size)
    r32, r64 = A.render_ray_aux(t, o, d, d, opt)
    first = 2.0 + 0.5 * float(m.delta[0]) * float(m.delta_scale)
    for r in (r32, r64):
        assert abs(float(r.surface) - first) < 1e-6 and r.pick == 0
        assert abs(float(r.alpha) - 1.0) < 1e-6 and abs(float(r.depth) - first) < 1e-5
    assert [(leaf, float(dt * m.delta_scale)) for leaf, dt in zip(m.flat.tolist(), m.delta)] == \
        [(leaf, float(dtw)) for leaf, dtw in T.march_tree(t, o, d, opt)]


# ---- writers ------------------------------------------------------------------------------------------------------------
def _fake_view(seed=0, H=9, W=11):
    rs = np.random.RandomState(seed)
    rgb = rs.rand(H, W, 3).astype(f32) * 1.2 - 0.1                          # some values outside [0,1]
    alpha = rs.rand(H, W).astype(f32)
    alpha[0, 0], alpha[0, 1], alpha[0, 2] = 0.0, 1.0, 1.0 + 3e-7
    surface = (2.0 + 3.0 * rs.rand(H, W)).astype(f32)
    surface[rs.rand(H, W) < 0.4] = np.inf
    surface[0, 0], surface[0, 4] = 2.5, np.inf
    depth = (alpha * 3.0).astype(f32)
    return rgb, alpha, depth, surface


def test_rgba_png_round_trips(tmp_path):
    from PIL import Image
    from plenoctree_amd.octree import aux_io
    rgb, alpha, _, _ = _fake_view()
    path = str(tmp_path / "000_rgba.png")
    aux_io.write_rgba_png(path, rgb, alpha)
    im = Image.open(path)
    assert im.mode == "RGBA" and im.size == (11, 9)
    got = np.asarray(im)
    assert got.dtype == np.uint8
    assert np.array_equal(got[..., 3], np.round(255.0 * np.clip(alpha, 0, 1)).astype(np.uint8))
    assert np.array_equal(got[..., :3], (np.clip(rgb, 0, 1) * 255).astype(np.uint8))      # the colours as --write_images writes them
    assert got[0, 0, 3] == 0 and got[0, 1, 3] == 255 and got[0, 2, 3] == 255


def test_depth_npz_holds_three_float32_arrays(tmp_path):
    from plenoctree_amd.octree import aux_io
    _, alpha, depth, surface = _fake_view()
    path = str(tmp_path / "000_depth.npz")
    aux_io.write_depth_npz(path, depth.astype(np.float64), surface, alpha)
    z = np.load(path)
    assert sorted(z.files) == ["alpha", "depth", "surface"]
    for k, want in (("alpha", alpha), ("depth", depth), ("surface", surface)):
        assert z[k].dtype == np.float32 and np.array_equal(z[k], want)
    assert np.isinf(z["surface"]).any()


@pytest.mark.parametrize("stride", [1, 4])
def test_ply_holds_the_finite_surface_pixels_at_the_stride(tmp_path, stride):
    from plenoctree_amd.octree import aux_io
    H, W, fx = 9, 11, 10.0
    views = [(C.pose(30.0, 20.0), _fake_view(1)), (C.pose(200.0, -40.0), _fake_view(2))]
    xyz, col = zip(*[aux_io.surface_points(c2w, fx, v[3], v[0], stride) for c2w, v in views])
    path = str(tmp_path / "points.ply")
    aux_io.write_ply(path, np.concatenate(xyz), np.concatenate(col))
    n = sum(int(np.isfinite(v[3][::stride, ::stride]).sum()) for _, v in views)
    with open(path, "rb") as f:
        raw = f.read()
    head, body = raw.split(b"end_header\n", 1)
    assert head.decode("ascii").split("\n")[:-1] == [
        "ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y",
        "property float z", "property uchar red", "property uchar green", "property uchar blue"]
    assert len(body) == 15 * n
    # the first vertex: pixel (0, 0) of the first view (its surface is finite), by the oracle's own camera ray
    c2w, (rgb, _, _, surface) = views[0]
    o, d = T.cam2world_ray(0, 0, c2w, W, H, fx, fx)
    first = np.frombuffer(body[:12], "<f4")
    assert np.allclose(first, o + surface[0, 0] * d, rtol=0, atol=1e-5)
    assert tuple(body[12:15]) == tuple((np.clip(rgb[0, 0], 0, 1) * 255).astype(np.uint8))
    got_xyz, got_col = C.read_ply(path)
    assert got_xyz.shape == (n, 3) and np.array_equal(got_xyz, np.concatenate(xyz)) and np.array_equal(got_col, np.concatenate(col))
    # every vertex is origin + surface * unit direction of its own pixel
    k = 0
    for c2w, (rgb, _, _, surface) in views:
        for iy in range(0, H, stride):
            for ix in range(0, W, stride):
                if np.isfinite(surface[iy, ix]):
                    o, d = T.cam2world_ray(ix, iy, c2w, W, H, fx, fx)
                    assert np.allclose(got_xyz[k], o + surface[iy, ix] * d, rtol=0, atol=1e-5)
                    k += 1
    assert k == n
    with pytest.raises(ValueError):
        aux_io.write_ply(path, np.zeros((2, 3)), np.zeros((3, 3)))
