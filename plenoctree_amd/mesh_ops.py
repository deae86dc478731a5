"""torch-tensor front end of the isosurface entry points of include/plenoctree_octree.h: marching cubes on a device grid
(pxo_mc_count / pxo_mc_emit) and the sampler of a PlenOctree's sigma onto its dense cell grid (pxo_tree_sigma_grid).

The definition is that of nerf_sh/isosurface.py:marching_cubes, output order included: the device arrays equal the host
function's element for element.  The case table is uploaded from that module (once per device); the library holds none.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import PxoError, check
from .ops import _f, _new, _p, _require_gpu, _stream

TRI_MAX = 5                        # row length of the case table the kernels index (kMcTriMax)
MC_BLOCK = 256                     # grid points per workgroup (kMcBlock)
MC_SCAN_TILE = 1024                # workgroup sums per scan tile (kMcScanTile)

_tables = {}


def case_tables():
    """(tri_table int8 [256, 5, 3], tri_count uint8 [256]) in the form the kernels read, from isosurface.TRI_TABLE / TRI_COUNT /
    _EDGES: an entry names a cell edge as axis << 3 | corner offset of its lower end (host arrays)."""
    from .nerf_sh import isosurface
    table, count = isosurface.TRI_TABLE, isosurface.TRI_COUNT
    if table.shape != (256, TRI_MAX, 3) or int(count.max()) > TRI_MAX:
        raise PxoError(f"isosurface.TRI_TABLE has shape {table.shape}; the kernels index rows of {TRI_MAX} triangles")
    code = np.array([(a << 3) | o for a, o in isosurface._EDGES], np.int8)
    coded = np.where(table >= 0, code[np.maximum(table, 0)], np.int8(-1)).astype(np.int8)
    return np.ascontiguousarray(coded), np.ascontiguousarray(count.astype(np.uint8))


def _device_tables(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _tables:
        table, count = case_tables()
        _tables[key] = (torch.from_numpy(table).to(device), torch.from_numpy(count).to(device))
    return _tables[key]


def mc_workspace_bytes(nx, ny, nz):
    """pxo_mc_workspace_bytes (host only).  PxoError for a grid of 2^31 points or more."""
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_mc_workspace_bytes(int(nx), int(ny), int(nz), ctypes.byref(n)), "pxo_mc_workspace_bytes")
    return n.value


def marching_cubes(vol, iso):
    """vol: float32 [nx, ny, nz] on the GPU -> (vertices [V,3] float64 in index units, triangles [T,3] int64, inside_idx [V]
    int64), device tensors equal to isosurface.marching_cubes(vol.cpu().numpy(), iso); inside_idx is the linear grid index of
    the end point of each vertex's edge whose value is >= iso.  ValueError for a volume with non-finite values."""
    _require_gpu()
    if vol.dim() != 3:
        raise ValueError("marching_cubes expects a 3-D array")
    if not vol.is_cuda or vol.dtype != torch.float32:
        raise PxoError("mesh_ops.marching_cubes takes a float32 volume on the GPU (the host function is isosurface.marching_cubes)")
    dev = vol.device
    nx, ny, nz = (int(s) for s in vol.shape)
    iso = float(iso)

    def empty(n_vert=0):
        return (torch.zeros(n_vert, 3, dtype=torch.float64, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev),
                torch.zeros(n_vert, dtype=torch.int64, device=dev))

    if min(nx, ny, nz) < 2:
        return empty()
    vol = vol.contiguous()
    if not bool(torch.isfinite(vol).all()):
        raise ValueError("marching_cubes: the volume holds non-finite values (NaN/inf sigma would give NaN vertices)")
    lib = _lib.load()
    table, count = _device_tables(dev)
    nbytes = mc_workspace_bytes(nx, ny, nz)
    ws = _new(nbytes, device=dev, dtype=torch.uint8)
    counts = (ctypes.c_int64 * 4)()
    check(lib.pxo_mc_count(_f(vol), nx, ny, nz, iso, _p(count), _p(ws), nbytes, counts, _stream()), "pxo_mc_count")
    n_vert, n_tri = counts[0] + counts[1] + counts[2], counts[3]
    if n_vert == 0 and n_tri == 0:
        return empty()
    vertices = _new(n_vert, 3, device=dev, dtype=torch.float64)
    triangles = _new(n_tri, 3, device=dev, dtype=torch.int64)
    inside_idx = _new(n_vert, device=dev, dtype=torch.int64)
    check(lib.pxo_mc_emit(_f(vol), nx, ny, nz, iso, _p(table), _p(ws), nbytes, counts, _p(vertices), _p(triangles),
                          _p(inside_idx), _stream()), "pxo_mc_emit")
    return vertices, triangles, inside_idx


def tree_sigma_grid(tree_view, depth, pad=1, want_packed=True, device=None):
    """(sigma float32 [S,S,S], packed int64 [S,S,S] or None), S = 2^depth + 2 pad: the tree's sigma at the centres of the 2^depth
    cells per axis with `pad` layers of 0 around them, and the packed leaf index node*8 + cell of every sample (-1 in the
    pad).  tree_view: a PxoTree (octree_ops.tree_view / N3Tree.view()); its tensors must stay alive during the call.  device: the
    tree's device (default: the current one)."""
    _require_gpu()
    depth, pad = int(depth), int(pad)
    if not 1 <= depth <= _lib.TREE_MAX_DEPTH + 1:
        raise PxoError(f"tree_sigma_grid: depth {depth} outside [1, {_lib.TREE_MAX_DEPTH + 1}]")
    if not 0 <= pad <= 64:
        raise PxoError(f"tree_sigma_grid: pad {pad} outside [0, 64]")
    side = (1 << depth) + 2 * pad
    sigma = _new(side, side, side, device=device)
    packed = _new(side, side, side, device=device, dtype=torch.int64) if want_packed else None
    check(_lib.load().pxo_tree_sigma_grid(ctypes.byref(tree_view), depth, pad, _f(sigma), _p(packed), _stream()),
          "pxo_tree_sigma_grid")
    return sigma, packed
