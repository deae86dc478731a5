"""torch-tensor front end of the isosurface entry points of include/plenoctree_octree.h: marching cubes on a device grid
(pxo_mc_count / pxo_mc_emit), the sampler of a PlenOctree's sigma onto its dense cell grid (pxo_tree_sigma_grid), and the two
stages that give a mesh normals and view-dependent colour (pxo_mc_vertex_gradients, pxo_shade_points).

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


def _mesh(vol, iso, who, gradients):
    """The count -> emit (-> gradient) sequence behind marching_cubes, mesh_with_gradients and vertex_gradients."""
    _require_gpu()
    if vol.dim() != 3:
        raise ValueError(f"{who} expects a 3-D array")
    if not vol.is_cuda or vol.dtype != torch.float32:
        raise PxoError(f"mesh_ops.{who} takes a float32 volume on the GPU (the host function is isosurface.{who})")
    dev = vol.device
    nx, ny, nz = (int(s) for s in vol.shape)
    iso = float(iso)

    def empty(n_vert=0):
        return (torch.zeros(n_vert, 3, dtype=torch.float64, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev),
                torch.zeros(n_vert, dtype=torch.int64, device=dev), torch.zeros(n_vert, 3, dtype=torch.float64, device=dev))

    if min(nx, ny, nz) < 2:
        return empty()
    vol = vol.contiguous()
    if not bool(torch.isfinite(vol).all()):
        raise ValueError(f"{who}: the volume holds non-finite values (NaN/inf sigma would give NaN vertices)")
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
    grad = None
    if gradients:
        grad = _new(n_vert, 3, device=dev, dtype=torch.float64)
        check(lib.pxo_mc_vertex_gradients(_f(vol), nx, ny, nz, iso, _p(ws), nbytes, counts, _p(inside_idx), _p(grad), _stream()),
              "pxo_mc_vertex_gradients")
    return vertices, triangles, inside_idx, grad


def marching_cubes(vol, iso):
    """vol: float32 [nx, ny, nz] on the GPU -> (vertices [V,3] float64 in index units, triangles [T,3] int64, inside_idx [V]
    int64), device tensors equal to isosurface.marching_cubes(vol.cpu().numpy(), iso); inside_idx is the linear grid index of
    the end point of each vertex's edge whose value is >= iso.  ValueError for a volume with non-finite values."""
    return _mesh(vol, iso, "marching_cubes", False)[:3]


def mesh_with_gradients(vol, iso):
    """marching_cubes(vol, iso) plus the sigma gradient at every vertex (float64 [V,3], index units, on the device; equal to
    isosurface.vertex_gradients(vol.cpu().numpy(), iso)): one count, one emit, one gradient launch on the same workspace."""
    return _mesh(vol, iso, "marching_cubes", True)


def vertex_gradients(vol, iso):
    """pxo_mc_vertex_gradients: float64 [V,3] on the device, equal to isosurface.vertex_gradients(vol.cpu().numpy(), iso)
    element for element.  A field without a crossing gives an empty array and launches nothing."""
    return _mesh(vol, iso, "vertex_gradients", True)[3]


def unit_normals(gradients, step):
    """n = -(grad / s) / |grad / s| in float64 (torch tensor or numpy array in, the same kind out): `step` is the world length
    of one index step per axis; the normal points towards lower sigma, out of the solid.  A zero gradient gives (0, 0, 0)."""
    if torch.is_tensor(gradients):
        g = gradients.double() / torch.as_tensor(step, dtype=torch.float64, device=gradients.device)
        length = g.norm(dim=1, keepdim=True)
        return torch.where(length > 0, -g / torch.where(length > 0, length, torch.ones_like(length)), torch.zeros_like(g))
    g = np.asarray(gradients, np.float64) / np.asarray(step, np.float64)
    length = np.sqrt((g * g).sum(1, keepdims=True))
    return np.where(length > 0, -g / np.where(length > 0, length, 1.0), 0.0)


def shading_dirs(normals):
    """d = -n in float32, the ray direction of a camera looking straight at the surface (what both renderers feed their basis);
    (0, 0, 1) where n = 0.  numpy or torch in, the same kind out."""
    if torch.is_tensor(normals):
        d = (-normals).float()
        d[(normals == 0).all(1)] = torch.tensor([0.0, 0.0, 1.0], device=d.device)
        return d.contiguous()
    d = (-np.asarray(normals)).astype(np.float32)
    d[(np.asarray(normals) == 0).all(1)] = (0.0, 0.0, 1.0)
    return np.ascontiguousarray(d)


SHADE_DIMS = (1, 4, 9, 16, 25)


def shade_points(coef, dirs, basis_dim, rows=None, lobes=None):
    """pxo_shade_points: out[i, c] = sigmoid(sum_k Y_k(dirs[i]) coef[r, c K + k]), r = rows[i] if rows is given else i; float32
    [n, 3] on the device.  coef: float32 [R, S] with S >= 3 K (a tree's leaves [n_internal * 8, 3 K + 1] are read in place, a
    NeRF's raw_rgb [n, 3 K] likewise); dirs float32 [n, 3]; rows int64 [n], a negative row gives colour 0 and a row >= R is
    refused; lobes float32 [K, 4] selects the SG basis, None the SH basis."""
    _require_gpu()
    K = int(basis_dim)
    if K not in SHADE_DIMS:
        raise PxoError(f"shade_points: basis_dim {K} not in {SHADE_DIMS}")
    if coef.dim() != 2 or coef.dtype != torch.float32 or not coef.is_cuda or not coef.is_contiguous():
        raise PxoError("shade_points takes contiguous float32 coefficients [R, S] on the GPU")
    if coef.shape[1] < 3 * K:
        raise PxoError(f"shade_points: rows of {coef.shape[1]} floats hold no 3 x {K} coefficients")
    dev = coef.device
    dirs = dirs.to(device=dev, dtype=torch.float32).contiguous()
    n = int(dirs.shape[0])
    if dirs.dim() != 2 or dirs.shape[1] != 3:
        raise PxoError("shade_points: dirs must be [n, 3]")
    if rows is None:
        if n > coef.shape[0]:
            raise PxoError(f"shade_points: {n} points but {coef.shape[0]} coefficient rows")
    else:
        rows = rows.to(device=dev, dtype=torch.int64).contiguous()
        if tuple(rows.shape) != (n,):
            raise PxoError(f"shade_points: rows has shape {tuple(rows.shape)}, dirs {tuple(dirs.shape)}")
        if n and int(rows.max()) >= coef.shape[0]:
            raise PxoError(f"shade_points: row {int(rows.max())} outside the {coef.shape[0]} coefficient rows")
    if lobes is not None:
        lobes = lobes.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(lobes.shape) != (K, 4):
            raise PxoError(f"shade_points: lobes of shape {tuple(lobes.shape)}, basis_dim {K} needs ({K}, 4)")
    out = _new(n, 3, device=dev)
    check(_lib.load().pxo_shade_points(_f(coef), int(coef.shape[1]), _p(rows), _f(dirs), n, K, _p(lobes), _f(out), _stream()),
          "pxo_shade_points")
    return out


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
