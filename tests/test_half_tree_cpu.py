"""Host side of rendering trees from the float16 of their files (no GPU): `N3Tree.load(path, keep_half=True)` keeps the data
as it is, `to_float()` gives exactly the tree `N3Tree.load(path)` gives, the device footprint is the documented layout, the
three refusals of the load name the file and the reason before anything could reach the GPU, and the float-only operations
refuse with a pointer to `to_float()`."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _half_cases as H
import _octree_sg_cases as G
import _quant_cases as Q
from plenoctree_amd import _lib, build, octree_ops
from plenoctree_amd.octree import svox
from plenoctree_amd.octree.svox import HalfN3Tree, N3Tree


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build(verbose=False)
    return _lib.load()


def _saved(tmp_path, K, kind):
    t = G.tree(K) if kind == "SG" else H.A.tree(K)
    return t, H.save(str(tmp_path / "tree.npz"), t, f"{kind}{K}", G.lobes(K) if kind == "SG" else None)


@pytest.mark.parametrize("K", H.KS)
@pytest.mark.parametrize("kind", ["SH", "SG"])
def test_load_keeps_the_halves_and_to_float_equals_plain_load(tmp_path, kind, K):
    t, path = _saved(tmp_path, K, kind)
    h = N3Tree.load(path, keep_half=True)
    f = N3Tree.load(path)
    assert isinstance(h, HalfN3Tree) and isinstance(f, N3Tree) and h.device == torch.device("cpu")
    assert torch.equal(h.child, f.child) and torch.equal(h.parent_depth, f.parent_depth)
    assert np.array_equal(h.child.numpy(), t.child) and np.array_equal(h.parent_depth.numpy(), t.parent_depth)
    assert torch.equal(h.offset, f.offset) and torch.equal(h.invradius, f.invradius)
    assert np.array_equal(h.offset.numpy(), t.offset) and np.array_equal(h.invradius.numpy(), t.invradius)
    assert (h.n_internal, h.max_depth, h.depth_limit, str(h.data_format), h.basis_dim, h.data_dim) == \
        (f.n_internal, f.max_depth, f.depth_limit, f"{kind}{K}", K, 3 * K + 1)
    if kind == "SG":
        assert torch.equal(h.extra_data, f.extra_data) and np.array_equal(h.extra_data.numpy(), G.lobes(K))
        assert set(h.basis_kwargs()) == {"lobes"}
    else:
        assert h.extra_data is None and h.basis_kwargs() == {}
    w = h.to_float()
    assert isinstance(w, N3Tree) and w.data.dtype == torch.float32
    assert torch.equal(w.data.data, f.data.data) and w.data.shape == f.data.shape
    assert np.array_equal(w.data.data.numpy(), t.data.astype(np.float16).astype(np.float32))
    assert torch.equal(w.child, f.child) and torch.equal(w.parent_depth, f.parent_depth)
    assert str(w.data_format) == str(f.data_format) and w.level_nodes == f.level_nodes and w.depth_limit == f.depth_limit
    assert (w.extra_data is None) == (f.extra_data is None)
    w.refine_leaves(torch.zeros(w.n_internal, 2, 2, 2, dtype=torch.bool))          # an editable tree of its own
    assert "HalfN3Tree" in repr(h)


@pytest.mark.parametrize("K", H.KS)
def test_strides_and_nbytes_are_the_documented_layout(tmp_path, K):
    t, path = _saved(tmp_path, K, "SH")
    h = N3Tree.load(path, keep_half=True)
    n, D = t.n_internal, 3 * K + 1
    stride, nbytes = ctypes.c_int32(0), ctypes.c_int64(0)
    assert _lib.load().pxo_octree_half_pack_bytes(n, D, ctypes.byref(stride), ctypes.byref(nbytes)) == 0
    assert stride.value == H.ROW_STRIDE[K] == (D + 3) // 4 * 4 and nbytes.value == n * 8 * stride.value * 2
    assert octree_ops.half_layout(n, D) == (stride.value, nbytes.value) and h.row_stride == stride.value
    geometry = n * 8 * 4 + n * 2 * 4                                   # child + parent_depth, int32
    assert h.nbytes == nbytes.value + geometry
    assert h.float_nbytes == n * 8 * D * 4 + geometry
    want, s = H.packed_layout(t.data.astype(np.float16), n, D)
    assert want.nbytes == nbytes.value and s == stride.value


def test_pack_bytes_refuses_other_formats():
    stride, nbytes = ctypes.c_int32(0), ctypes.c_int64(0)
    lib = _lib.load()
    for D in (0, 3, 5, 48, 50, 7, 3 * 36 + 1):
        assert lib.pxo_octree_half_pack_bytes(10, D, ctypes.byref(stride), ctypes.byref(nbytes)) == -1, D
    assert lib.pxo_octree_half_pack_bytes(0, 49, ctypes.byref(stride), ctypes.byref(nbytes)) == -1
    assert lib.pxo_octree_half_pack_bytes(1 << 28, 49, ctypes.byref(stride), ctypes.byref(nbytes)) == -1
    assert lib.pxo_octree_half_pack_bytes(10, 49, None, ctypes.byref(nbytes)) == -1
    with pytest.raises(svox.PxoError):
        octree_ops.half_layout(10, 50)


def test_float_only_operations_raise(tmp_path):
    _, path = _saved(tmp_path, 4, "SH")
    h = N3Tree.load(path, keep_half=True)
    mask = torch.zeros(h.n_internal, 2, 2, 2, dtype=torch.bool)
    ops = {
        "tree.data": lambda: h.data,
        "tree.parameters()": lambda: h.parameters(),
        "tree[...]": lambda: h[:],
        "tree[...] = value": lambda: h.__setitem__(slice(None), 0.0),
        "refine": lambda: h.refine(),
        "refine_from_mask": lambda: h.refine_from_mask(mask),
        "relu_sigma_": lambda: h.relu_sigma_(),
        "accumulate_weights": lambda: h.accumulate_weights("sum"),
        "prune_": lambda: h.prune_(mask),
        "refine_leaves": lambda: h.refine_leaves(mask),
        "view()": lambda: h.view(),
        "save": lambda: h.save(str(tmp_path / "out.npz")),
    }
    for what, op in ops.items():
        with pytest.raises(svox.PxoError) as e:
            op()
        assert str(e.value) == f"{what}: a HalfN3Tree is read-only and has no float leaf data; call to_float() for an N3Tree"
    assert not os.path.exists(str(tmp_path / "out.npz"))
    # on the CPU the object loads, and rendering refuses like the palette form does
    with pytest.raises(svox.PxoError, match="ROCm device only"):
        h.half_view()
    if not torch.cuda.is_available():
        with pytest.raises(svox.PxoError):
            svox.VolumeRenderer(h).render_persp(torch.eye(4)[:3], width=4, height=4, fx=4.0)


def test_load_refusals_name_the_file_and_the_reason(tmp_path):
    t, path = _saved(tmp_path, 4, "SH")
    with pytest.raises(ValueError, match=r"tree\.npz.*keep_half.*keep_quantized"):
        N3Tree.load(path, keep_half=True, keep_quantized=True)
    comp = Q.case(4, 1, 8).save(str(tmp_path / "compressed.npz"))              # the palette form: no `data`
    with pytest.raises(ValueError, match=r"compressed\.npz.*keep_half.*compressed"):
        N3Tree.load(comp, keep_half=True)
    with pytest.raises(ValueError, match=r"compressed\.npz.*keep_half.*keep_quantized"):
        N3Tree.load(comp, keep_half=True, keep_quantized=True)
    z = dict(np.load(path))
    wide = str(tmp_path / "float32.npz")
    np.savez(wide, **{**z, "data": z["data"].astype(np.float32)})
    with pytest.raises(ValueError, match=r"float32\.npz.*float16.*float32"):
        N3Tree.load(wide, keep_half=True)
    assert isinstance(N3Tree.load(wide), N3Tree)                               # the float load takes it, as before
    short = str(tmp_path / "short.npz")
    np.savez(short, **{**z, "data": z["data"][:-1]})
    with pytest.raises(ValueError, match="data"):
        N3Tree.load(short, keep_half=True)
    assert isinstance(N3Tree.load(path, keep_half=True), HalfN3Tree) and isinstance(N3Tree.load(path, keep_half=False), N3Tree)


def test_evaluation_refuses_keep_half_with_keep_compressed(tmp_path, monkeypatch):
    """... before a device is opened: the refusal comes although opening one would fail."""
    from plenoctree_amd.octree import evaluation
    from plenoctree_amd import dist

    def no_device(*a, **k):
        raise AssertionError("a device was opened before the flags were checked")

    monkeypatch.setattr(dist, "open_cli", no_device)
    cfg_path = os.path.join(str(tmp_path), "tiny.yaml")
    with open(cfg_path, "w") as fh:
        fh.write("dataset: synthetic\nfactor: 16\nnum_coarse_samples: 64\nnum_fine_samples: 128\nuse_viewdirs: false\n"
                 "white_bkgd: true\nbatch_size: 1024\nsh_deg: 3\nrandomized: true\n")
    argv = ["--train_dir", str(tmp_path), "--config", cfg_path, "--input", str(tmp_path / "none.npz")]
    with pytest.raises(ValueError, match="--keep_half together with --keep_compressed"):
        evaluation.main(argv + ["--keep_half", "--keep_compressed"])
    args = evaluation.define_flags().parse_args(argv + ["--keep_half"])
    assert args.keep_half and not args.keep_compressed
    assert not evaluation.define_flags().parse_args(argv).keep_half
