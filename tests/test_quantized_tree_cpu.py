"""Host side of rendering compressed trees in place (no GPU): `N3Tree.load(path, keep_quantized=True)` keeps the
palette form of octree/compression.py, `dequantize()` gives exactly the tree `N3Tree.load(path)` gives, the device
footprint is the documented layout, every inconsistency of the file is a ValueError naming the array before anything
could reach the GPU, and the float-only operations refuse with a pointer to `dequantize()`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _quant_cases as Q
from plenoctree_amd import _lib, build
from plenoctree_amd.octree import compression, svox
from plenoctree_amd.octree.svox import N3Tree, QuantizedN3Tree

CPU_CASES = ((1, 0, 8), (4, 1, 8), (9, 0, 16), (16, 4, 3), (25, 1, 1))


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return _lib.load()


def _case(K, retain, bits):
    return Q.case(K, retain, bits) if (K, retain, bits) in Q.CASES else Q.make_case(K, retain, bits, depth=2)


@pytest.mark.parametrize("K,retain,bits", CPU_CASES)
def test_dequantize_equals_plain_load(tmp_path, K, retain, bits):
    c = _case(K, retain, bits)
    path = c.save(str(tmp_path / "tree.npz"))
    q = N3Tree.load(path, keep_quantized=True)
    assert isinstance(q, QuantizedN3Tree) and (q.bits, q.n_retained, q.basis_dim) == (bits, retain, K)
    f = N3Tree.load(path)
    d = q.dequantize()
    assert isinstance(f, N3Tree) and isinstance(d, N3Tree)
    assert torch.equal(d.data.data, f.data.data) and d.data.dtype == torch.float32
    assert torch.equal(d.child, f.child) and torch.equal(d.parent_depth, f.parent_depth)
    # ... and both are what the format says, and the geometry is the tree's
    assert np.array_equal(f.data.data.numpy(), c.dequantized())
    assert np.array_equal(q.child.numpy(), c.tree.child) and np.array_equal(q.parent_depth.numpy(), c.tree.parent_depth)
    assert np.array_equal(q.offset.numpy(), c.tree.offset) and np.array_equal(q.invradius.numpy(), c.tree.invradius)
    assert (q.n_internal, q.max_depth, q.depth_limit, str(q.data_format)) == (f.n_internal, f.max_depth, f.depth_limit, f"SH{K}")
    assert q.device == torch.device("cpu")


@pytest.mark.parametrize("K,retain,bits", CPU_CASES)
def test_nbytes_is_the_documented_layout(tmp_path, K, retain, bits):
    c = _case(K, retain, bits)
    q = N3Tree.load(c.save(str(tmp_path / "tree.npz")), keep_quantized=True)
    n = c.tree.n_internal
    sections, stride = Q.layout_bytes(n, K, retain, bits)
    geometry = n * 8 * 4 + n * 2 * 4                                   # child + parent_depth, int32
    assert q.nbytes == sum(sections) + geometry
    assert q.float_nbytes == n * 8 * (3 * K + 1) * 4 + geometry
    lay = _lib.PxoQuantLayout()
    assert _lib.load().pxo_octree_quant_pack_bytes(n, K, retain, bits, ctypes.byref(lay)) == 0
    offs = np.concatenate([[0], np.cumsum(sections)])
    assert [lay.idx_offset, lay.palette_offset, lay.sigma_offset, lay.retained_offset, lay.total_bytes] == offs.tolist()
    assert (lay.idx_stride, lay.ret_stride) == (stride, 4 * retain)
    assert stride % 4 == 0 and stride >= K - retain                    # no 8-byte index load is misaligned for odd counts


def test_validation_errors_name_the_array(tmp_path):
    c = Q.case(4, 1, 8)
    p = str(tmp_path / "bad.npz")
    load = lambda **over: N3Tree.load(c.save(p, **over), keep_quantized=True)
    bad = c.quant_map.copy()
    bad[2, -1, 1, 0, 1] = 256                                           # == 2^bits: one past its palette
    with pytest.raises(ValueError, match="quant_map.*256"):
        load(quant_map=bad)
    with pytest.raises(ValueError, match="quant_map.*300"):
        wide = c.quant_map.astype(np.int32)
        wide[0, 0, 0, 0, 0] = 300
        load(quant_map=wide)
    with pytest.raises(ValueError, match="quant_map"):                  # planes != palettes
        load(quant_map=c.quant_map[:2])
    with pytest.raises(ValueError, match="data_retained"):              # retained + quantised != K
        load(data_retained=np.concatenate([c.data_retained, c.data_retained]))
    with pytest.raises(ValueError, match="quant_colors"):               # ... the same without retained planes
        load(data_retained=None)
    with pytest.raises(ValueError, match="quant_colors"):               # not a power of two
        load(quant_colors=c.quant_colors[:, :200])
    with pytest.raises(ValueError, match="quant_map"):                  # leaf counts
        load(quant_map=c.quant_map[:, :-1])
    with pytest.raises(ValueError, match="sigma"):
        load(sigma=c.sigma[:-1])
    with pytest.raises(ValueError, match="data_retained"):
        load(data_retained=c.data_retained[:, :-1])
    with pytest.raises(ValueError, match="sigma"):
        load(sigma=c.sigma.astype(np.float64))
    assert isinstance(load(), QuantizedN3Tree)                          # the unmodified file is fine
    # a file that is not compressed
    flat = str(tmp_path / "float.npz")
    z = c.files()
    for k in ("quant_colors", "quant_map", "sigma", "data_retained"):
        z.pop(k)
    np.savez(flat, data=c.dequantized().astype(np.float16), **z)
    with pytest.raises(ValueError, match="keep_quantized"):
        N3Tree.load(flat, keep_quantized=True)
    assert isinstance(N3Tree.load(flat), N3Tree) and isinstance(N3Tree.load(flat, keep_quantized=False), N3Tree)


def test_float_only_operations_raise(tmp_path):
    c = Q.case(4, 1, 8)
    q = N3Tree.load(c.save(str(tmp_path / "tree.npz")), keep_quantized=True)
    ops = {
        "data": lambda: q.data,
        "parameters": lambda: q.parameters(),
        "refine": lambda: q.refine(),
        "view refine": lambda: q[:].refine(),
        "assign": lambda: q.__setitem__(slice(None), 0.0),
        "save": lambda: q.save(str(tmp_path / "out.npz")),
        "relu": lambda: q.relu_sigma_(),
    }
    for name, op in ops.items():
        with pytest.raises(svox.PxoError, match=r"dequantize\(\)"):
            op()
    assert not os.path.exists(str(tmp_path / "out.npz"))
    # without a GPU there is nothing to render with, and the message says so (no silent CPU path)
    if not torch.cuda.is_available():
        with pytest.raises(svox.PxoError):
            svox.VolumeRenderer(q).render_persp(torch.eye(4), width=4, height=4, fx=4.0)


@pytest.mark.parametrize("retain,bits", [(0, 4), (2, 6)])
def test_file_from_the_compression_tool_round_trips(tmp_path, retain, bits):
    """The repository's own octree.compression on a small SH4 tree, then both ways of loading its output."""
    c = Q.case(4, 1, 8)
    t = c.tree
    n = t.n_internal
    rs = np.random.RandomState(5)
    data = (rs.randn(n, 2, 2, 2, 13) * 0.7).astype(np.float16)
    data[..., -1] = (rs.rand(n, 2, 2, 2) * 8.0 - 2.0).astype(np.float16)
    src = str(tmp_path / "tree.npz")
    np.savez(src, data_dim=13, child=t.child, parent_depth=t.parent_depth, n_internal=n, n_free=0, invradius3=t.invradius,
             offset=t.offset, depth_limit=t.depth_limit, geom_resize_fact=1.0, data=data, data_format="SH4")
    out = compression.main([src, "--out_dir", str(tmp_path / "min"), "--overwrite", "--bits", str(bits), "--retain", str(retain),
                            "--sigma_thresh", "1.0"])
    assert len(out) == 1
    z = np.load(out[0])
    assert "quant_colors" in z.files and "data" not in z.files and ("data_retained" in z.files) == bool(retain)
    q = N3Tree.load(out[0], keep_quantized=True)
    f = N3Tree.load(out[0])
    d = q.dequantize()
    assert (q.bits, q.n_retained) == (bits, retain)
    assert torch.equal(d.data.data, f.data.data) and torch.equal(d.child, f.child) and torch.equal(d.parent_depth, f.parent_depth)
    assert np.array_equal(f.parent_depth.numpy(), t.parent_depth)       # the tool drops it; rebuilt from child
    sig = f.data.data[..., -1].numpy()
    assert ((sig == 0) | (sig > 1.0)).all() and (sig == 0).any() and (sig > 1.0).any()
    assert q.nbytes < q.float_nbytes


def test_c_abi_rejects_bad_arguments(lib):
    """PXO_ERR_ARG (-1) like the float renderer's entry points; all decided on the host, before any launch."""
    lay = _lib.PxoQuantLayout()
    pack_bytes = lambda n, K, r, b, out=lay: lib.pxo_octree_quant_pack_bytes(n, K, r, b, ctypes.byref(out) if out is not None else None)
    assert pack_bytes(5, 16, 0, 8) == 0
    for args in ((5, 7, 0, 8), (5, 16, 16, 8), (5, 16, -1, 8), (5, 16, 0, 0), (5, 16, 0, 17), (0, 16, 0, 8)):
        assert pack_bytes(*args) == -1, args
    assert b"bits" in (pack_bytes(5, 16, 0, 17), lib.pxo_last_error())[1]
    assert lib.pxo_octree_quant_pack_bytes(5, 16, 0, 8, None) == -1
    assert lib.pxo_octree_quant_pack(None, None, None, 2, None, 5, 16, 0, 8, None, 0, None) == -1
    opts = _lib.PxoRenderOpts(1e-3, 1.0, 0.0, 0.0)
    out = ctypes.c_void_p(256)                                          # never dereferenced: every call below fails first
    assert lib.pxo_octree_render_quant_fwd(None, None, None, None, None, 0, ctypes.byref(opts), out, None) == -1
    t = _lib.PxoQuantTree()                                             # all-null tree
    assert lib.pxo_octree_render_quant_fwd(ctypes.byref(t), None, None, None, None, 0, ctypes.byref(opts), out, None) == -1
    t.child, t.idx, t.palette, t.sigma, t.retained = 256, 256, 256, 256, 256
    t.n_internal, t.idx_stride, t.ret_stride = 5, 16, 0
    for K, r, b in ((7, 0, 8), (16, 16, 8), (16, 0, 0), (16, 0, 17)):
        t.basis_dim, t.n_retained, t.bits = K, r, b
        assert lib.pxo_octree_render_quant_fwd(ctypes.byref(t), None, None, None, None, 0, ctypes.byref(opts), out, None) == -1
    t.basis_dim, t.n_retained, t.bits = 16, 0, 8
    assert lib.pxo_octree_render_quant_fwd(ctypes.byref(t), None, None, None, None, 0, None, out, None) == -1      # null options
    t.idx_stride = 15                                                   # not the packed stride
    assert lib.pxo_octree_render_quant_fwd(ctypes.byref(t), None, None, None, None, 0, ctypes.byref(opts), out, None) == -1
    t.idx_stride = 16
    assert lib.pxo_octree_render_quant_fwd(ctypes.byref(t), None, None, None, None, 0, ctypes.byref(opts), out, None) == 0   # B = 0
