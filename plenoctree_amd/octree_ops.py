"""torch-tensor front end of include/plenoctree_octree.h (tree build, weight mask, octree renderer).

As in ops.py, torch only provides device storage and the current HIP stream; every operation runs in
libplenoctree_hip.so and there is no CPU fallback.
"""
import ctypes

import torch

from . import _lib
from ._lib import PxoError, check
from .ops import _f, _new, _p, _require_gpu, _stream


def _vec3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def render_opts(step_size=1e-3, background_brightness=1.0, sigma_thresh=0.0, stop_thresh=0.0):
    return _lib.PxoRenderOpts(float(step_size), float(background_brightness), float(sigma_thresh), float(stop_thresh))


def threshold_mask(value, thresh):
    """uint8 mask = value >= thresh (octree/extraction.py:322-331)."""
    _require_gpu()
    value = value.reshape(-1)
    mask = _new(value.numel(), device=value.device, dtype=torch.uint8)
    check(_lib.load().pxo_threshold_mask(_f(value), value.numel(), float(thresh), _p(mask), _stream()),
          "pxo_threshold_mask")
    return mask


def tree_workspace_bytes(depth):
    n = ctypes.c_size_t(0)
    check(_lib.load().pxo_tree_workspace_bytes(depth, ctypes.byref(n)), "pxo_tree_workspace_bytes")
    return n.value


def tree_from_mask(mask, depth):
    """Octree of the masked voxels of a 2^(depth+1) grid: (child [n,2,2,2] int32, parent_depth [n,2] int32,
    level_nodes list).  Equivalent of `depth` rounds of tree[grid].refine() (octree/extraction.py:341-350)."""
    _require_gpu()
    lib = _lib.load()
    reso = 2 ** (depth + 1)
    if mask.dtype != torch.uint8 or mask.numel() != reso ** 3:
        raise PxoError(f"mask must be uint8 with {reso}^3 entries")
    nbytes = tree_workspace_bytes(depth)
    ws = _new(nbytes, device=mask.device, dtype=torch.uint8)
    levels = (ctypes.c_int64 * (depth + 1))()
    check(lib.pxo_tree_count_nodes(_p(mask.reshape(-1)), depth, _p(ws), nbytes, levels, _stream()),
          "pxo_tree_count_nodes")
    level_nodes = [int(v) for v in levels]
    n = sum(level_nodes)
    child = _new(n, 2, 2, 2, device=mask.device, dtype=torch.int32)
    parent_depth = _new(n, 2, device=mask.device, dtype=torch.int32)
    check(lib.pxo_tree_build(_p(ws), nbytes, depth, levels, _p(child), _p(parent_depth), _stream()), "pxo_tree_build")
    return child, parent_depth, level_nodes


def tree_sample_cells(parent_depth, node0, n_nodes, samples, offset, invradius, u=None, seed=0, stream_id=0):
    """World-space sample points [n_nodes*8, samples, 3] of the 8 cells of nodes [node0, node0+n_nodes)."""
    _require_gpu()
    lib = _lib.load()
    n = n_nodes * 8 * samples
    dev = parent_depth.device
    if u is None:
        u = _new(max(n * 3, 1), device=dev)
        check(lib.pxo_uniform(seed, stream_id, n * 3, 0.0, 1.0, _f(u), _stream()), "pxo_uniform")
    pts = _new(n_nodes * 8, samples, 3, device=dev)
    check(lib.pxo_tree_sample_cells(_p(parent_depth), node0, n_nodes, samples, _f(u), _vec3(offset), _vec3(invradius),
                                    _f(pts), _stream()), "pxo_tree_sample_cells")
    return pts


def tree_sample_leaves(parent_depth, packed, samples, offset, invradius, u=None, seed=0, stream_id=0):
    """World-space sample points [n, samples, 3] inside the leaves `packed` (int64 node*8+cell)."""
    _require_gpu()
    lib = _lib.load()
    if packed.dtype != torch.int64:
        raise PxoError("packed leaf indices must be int64")
    n_cells = packed.numel()
    n = n_cells * samples
    dev = parent_depth.device
    if u is None:
        u = _new(max(n * 3, 1), device=dev)
        check(lib.pxo_uniform(seed, stream_id, n * 3, 0.0, 1.0, _f(u), _stream()), "pxo_uniform")
    pts = _new(n_cells, samples, 3, device=dev)
    check(lib.pxo_tree_sample_leaves(_p(parent_depth), _p(packed.contiguous()), n_cells, samples, _f(u), _vec3(offset),
                                     _vec3(invradius), _f(pts), _stream()), "pxo_tree_sample_leaves")
    return pts


def tree_query(child, points, offset, invradius):
    """Packed index (node*8 + cell, int64 [n]) of the leaf containing each world-space point [n,3]."""
    _require_gpu()
    points = points.reshape(-1, 3).contiguous().float()
    out = _new(points.shape[0], device=points.device, dtype=torch.int64)
    check(_lib.load().pxo_tree_query(_p(child), _f(points), points.shape[0], _vec3(offset), _vec3(invradius), _p(out),
                                     _stream()), "pxo_tree_query")
    return out


def tree_relu_sigma(data):
    _require_gpu()
    dim = data.shape[-1]
    check(_lib.load().pxo_tree_relu_sigma(_f(data), data.numel() // dim, dim, _stream()), "pxo_tree_relu_sigma")


def ndc_spec(width, height, focal, near=1.0):
    """PxoNdc: the projection an LLFF scene was trained with (include/plenoctree_octree.h, "forward-facing scenes")."""
    return _lib.PxoNdc(int(width), int(height), float(focal), float(near))


def _ndc(ndc):
    """PxoNdc of anything that carries width / height / focal (and optionally near): a PxoNdc, an svox NDCConfig."""
    if isinstance(ndc, _lib.PxoNdc):
        return ndc
    return ndc_spec(ndc.width, ndc.height, ndc.focal, getattr(ndc, "near", 1.0))


def grid_weight_render(sigma_grid, reso, c2w_all, fx, fy, width, height, opts, offset, invradius, grid_weight=None, ndc=None):
    """Per-voxel maximum compositing weight over all pixels of the given cameras (c2w_all [n,3,4] or [n,4,4]).  ndc: None for
    a world-space grid, or the projection (ndc_spec / NDCConfig) of a forward-facing scene whose grid spans the NDC cube
    (pxo_grid_weight_render_ndc)."""
    _require_gpu()
    lib = _lib.load()
    dev = sigma_grid.device
    c2w = c2w_all[:, :3, :4].contiguous().to(device=dev, dtype=torch.float32)
    if grid_weight is None:
        grid_weight = torch.zeros(reso ** 3, dtype=torch.float32, device=dev)
    nbytes = ctypes.c_size_t(0)
    check(lib.pxo_grid_weight_workspace_bytes(reso, ctypes.byref(nbytes)), "pxo_grid_weight_workspace_bytes")
    ws = _new(max(nbytes.value, 16), device=dev, dtype=torch.uint8)
    args = (_f(sigma_grid.reshape(-1)), reso, _f(c2w), c2w.shape[0], float(fx), float(fy), int(width), int(height),
            ctypes.byref(opts), _vec3(offset), _vec3(invradius), _f(grid_weight), _p(ws), nbytes.value, _stream())
    if ndc is None:
        check(lib.pxo_grid_weight_render(*args), "pxo_grid_weight_render")
    else:
        check(lib.pxo_grid_weight_render_ndc(*args, ctypes.byref(_ndc(ndc))), "pxo_grid_weight_render_ndc")
    return grid_weight


def _tree_fields(t, child, offset, invradius):
    """What the three tree structs share: the child array, n_internal and the transform."""
    if child.dtype != torch.int32:
        raise PxoError("child must be int32")
    t.child = _p(child).value
    t.n_internal = child.shape[0]
    t.offset = _vec3(offset)
    t.invradius = _vec3(invradius)
    return t


def tree_view(child, data, offset, invradius):
    """PxoTree struct over torch storage (keeps no reference: the caller owns the tensors)."""
    data_dim = data.shape[-1]
    if (data_dim - 1) % 3:
        raise PxoError(f"data_dim {data_dim} is not 3*basis_dim+1")
    t = _tree_fields(_lib.PxoTree(), child, offset, invradius)
    t.data = _f(data).value
    t.data_dim = data_dim
    t.basis_dim = (data_dim - 1) // 3
    return t


def _lobes(lobes, tree):
    """Device pointer of an SG tree's lobes [basis_dim, 4] (float32, contiguous, on the tree's device), checked on the host."""
    if not torch.is_tensor(lobes) or lobes.dtype != torch.float32 or tuple(lobes.shape) != (tree.basis_dim, 4) or \
            not lobes.is_contiguous() or not lobes.is_cuda:
        raise PxoError(f"SG lobes must be a contiguous float32 [{tree.basis_dim}, 4] tensor on the GPU")
    return _f(lobes)


def _no_sg_ndc(lobes, ndc):
    if lobes is not None and ndc is not None:
        raise NotImplementedError("NDC rendering of an SG tree is not built: the NDC launches (pxo_octree_render_ndc_*) take SH "
                                  "trees only")


# The renderer entry points: (struct type, what) -> {shading: (name, takes lobes, takes ndc)}; what: "fwd", "aux" (forward with
# the extra outputs) or "bwd"; shading: "" for SH in world space, "sg" with an SG tree's lobes, "ndc" with a scene's projection.
# "foot" / "foot_aux" are "fwd" / "aux" at a depth per sample from the pixel footprint (float trees in world space only).
# Every one takes, in this order: the tree[, lobes], the camera and rays of _rays, the options[, cone, min_depth][,
# surface_thresh], out_rgb[, out_aux] (backward: out_rgb, grad_out, grad_data), the stream[, ndc].  What a form has no row or shading for is not built.
_ENTRIES = {
    (_lib.PxoTree, "fwd"): {"": ("pxo_octree_render_fwd", False, False), "sg": ("pxo_octree_render_sg_fwd", True, False),
                            "ndc": ("pxo_octree_render_ndc_fwd", False, True)},
    (_lib.PxoTree, "bwd"): {"": ("pxo_octree_render_bwd", False, False), "sg": ("pxo_octree_render_sg_bwd", True, False),
                            "ndc": ("pxo_octree_render_ndc_bwd", False, True)},
    (_lib.PxoTree, "aux"): {"": ("pxo_octree_render_aux_fwd", False, False)},
    (_lib.PxoTree, "foot"): dict.fromkeys(("", "sg"), ("pxo_octree_render_foot_fwd", True, False)),
    (_lib.PxoTree, "foot_aux"): {"": ("pxo_octree_render_foot_aux_fwd", False, False)},
    (_lib.PxoQuantTree, "fwd"): {"": ("pxo_octree_render_quant_fwd", False, False)},
    (_lib.PxoQuantTree, "aux"): {"": ("pxo_octree_render_quant_aux_fwd", False, False)},
    (_lib.PxoHalfTree, "fwd"): dict.fromkeys(("", "sg", "ndc"), ("pxo_octree_render_half_fwd", True, True)),
    (_lib.PxoHalfTree, "aux"): {"": ("pxo_octree_render_half_aux_fwd", False, False)},
}
_WHAT = {"fwd": "rendering", "aux": "rendering alpha / depth / surface", "bwd": "the gradient",
         "foot": "rendering at a depth per sample from the pixel footprint",
         "foot_aux": "rendering alpha / depth / surface at a depth per sample from the pixel footprint"}
_SHADING = {"": "an SH tree in world space", "sg": "an SG tree (lobes)", "ndc": "an NDC scene (ndc)"}


def _call(tree, what, lobes, ndc, rays, opts, outputs):
    """Calls the renderer entry point of `tree`'s form; outputs: the arguments between the options and the stream."""
    _no_sg_ndc(lobes, ndc)
    if not isinstance(tree, (_lib.PxoTree, _lib.PxoQuantTree, _lib.PxoHalfTree)):
        raise PxoError(f"expected a PxoTree, a PxoQuantTree or a PxoHalfTree, got {type(tree).__name__}")
    shading = "ndc" if ndc is not None else ("" if lobes is None else "sg")
    row = _ENTRIES.get((type(tree), what), {})
    if shading not in row:
        raise NotImplementedError(f"{_WHAT[what]} of {_SHADING[shading]} is not built for a {type(tree).__name__}")
    name, takes_lobes, takes_ndc = row[shading]
    lead = (None if lobes is None else _lobes(lobes, tree),) if takes_lobes else ()
    trail = (None if ndc is None else ctypes.byref(_ndc(ndc)),) if takes_ndc else ()
    check(getattr(_lib.load(), name)(ctypes.byref(tree), *lead, *rays, ctypes.byref(opts), *outputs, _stream(), *trail), name)


def _forward(tree, opts, camera=None, rays=None, lobes=None, ndc=None, surface_thresh=None, foot=None):
    """The forward render of a PxoTree, a PxoQuantTree or a PxoHalfTree from camera = (c2w, width, height, fx, fy) or rays =
    (origins, dirs, viewdirs): rgb [H,W,3] or [B,3], and with surface_thresh (rgb, aux), aux of rgb's shape.  foot: None, or
    (cone, min_depth) of the footprint launches (include/plenoctree_octree.h, "footprint"); the tree's data must be filled."""
    _require_gpu()
    if camera is not None:
        cam, keep = _camera(*camera)
        shape, device, rays = (cam.height, cam.width, 3), keep.device, _rays(cam)
    else:
        shape, device, rays = (rays[0].shape[0], 3), rays[0].device, _rays(None, *rays)
    aux = surface_thresh is not None
    outs = [_new(*shape, device=device) for _ in range(2 if aux else 1)]
    what = ("aux" if aux else "fwd") if foot is None else ("foot_aux" if aux else "foot")
    _call(tree, what, lobes, ndc, rays, opts, (() if foot is None else (float(foot[0]), int(foot[1]))) +
          ((float(surface_thresh),) if aux else ()) + tuple(_f(o) for o in outs))
    return tuple(outs) if aux else outs[0]


def _render_bwd(tree, lobes, rays, opts, out_rgb, grad_out, grad_data, ndc=None):
    _call(tree, "bwd", lobes, ndc, rays, opts, (_f(out_rgb), _f(grad_out), _f(grad_data)))
    return grad_data


def _rays(cam=None, origins=None, dirs=None, viewdirs=None):
    """(camera, origins, dirs, viewdirs, B) as every renderer entry point takes them: a PxoCamera with its pixel count, or
    three [B,3] ray arrays."""
    if cam is not None:
        return ctypes.byref(cam), None, None, None, cam.width * cam.height
    return None, _f(origins), _f(dirs), _f(viewdirs), origins.shape[0]


def _camera(c2w, width, height, fx, fy):
    c2w = c2w[:3, :4].contiguous().float()
    cam = _lib.PxoCamera(_f(c2w).value, float(fx), float(fx if fy is None else fy), int(width), int(height))
    return cam, c2w          # keep c2w alive for the duration of the call


def set_lanes_per_ray(forward=0, backward=0):
    """Lanes per ray of the renderer launches (4 / 8 / 16; 0 = measured default 4)."""
    check(_lib.load().pxo_octree_set_lanes_per_ray(int(forward), int(backward)), "pxo_octree_set_lanes_per_ray")


TUNE_GW_MARCHER, TUNE_BWD_CACHE_ROWS, TUNE_BWD_UPDATE, TUNE_GW_TILE_ORDER = 0, 1, 2, 3


def get_tuning(knob):
    v = ctypes.c_int(0)
    check(_lib.load().pxo_octree_get_tuning(int(knob), ctypes.byref(v)), "pxo_octree_get_tuning")
    return v.value


def set_tuning(knob, value):
    """pxo_octree_set_tuning: choose between kernels that compute the same result (A/B sessions, equality tests)."""
    check(_lib.load().pxo_octree_set_tuning(int(knob), int(value)), "pxo_octree_set_tuning")


def octree_render_persp(tree, c2w, width, height, fx, opts, fy=None, lobes=None, ndc=None):
    """[H,W,3] image of a pinhole camera (VolumeRenderer.render_persp).  lobes: the [K,4] extra_data of an SG tree (the
    spherical-Gaussian basis instead of SH), None for an SH tree.  ndc: the projection (ndc_spec / NDCConfig) of a
    forward-facing scene whose tree lives in the NDC cube, None for a world-space tree.  tree: a PxoTree, or the struct of
    another storage form (PxoQuantTree: SH in world space only; PxoHalfTree), rendered in place."""
    return _forward(tree, opts, camera=(c2w, width, height, fx, fy), lobes=lobes, ndc=ndc)


def octree_render_persp_bwd(tree, c2w, width, height, fx, opts, grad_out, grad_data, fy=None, out_rgb=None, lobes=None,
                            ndc=None):
    """Accumulates d sum(image * grad_out) / d data into grad_data; `out_rgb` = the exact forward image of the same
    camera (saves one of the two marches) or None.  lobes, ndc: as in octree_render_persp."""
    _require_gpu()
    cam, keep = _camera(c2w, width, height, fx, fy)
    return _render_bwd(tree, lobes, _rays(cam), opts, out_rgb, grad_out, grad_data, ndc=ndc)


def octree_count_work(tree, c2w, width, height, fx, opts, fy=None, count_leaves=True):
    """Work counters of one render of `tree` from camera c2w (pxo_octree_count_work: the renderer's own march, counting):
    dict(rays, samples, shaded_samples, child_loads, distinct_leaves).  A roofline / debug pass, not on the product path."""
    _require_gpu()
    cam, keep = _camera(c2w, width, height, fx, fy)
    counts = torch.zeros(4, dtype=torch.int64, device=keep.device)
    seen = torch.zeros(tree.n_internal * 8, dtype=torch.uint8, device=keep.device) if count_leaves else None
    check(_lib.load().pxo_octree_count_work(ctypes.byref(tree), ctypes.byref(cam), ctypes.byref(opts), _p(counts), _p(seen),
                                            _stream()), "pxo_octree_count_work")
    c = counts.tolist()
    return {"rays": c[0], "samples": c[1], "shaded_samples": c[2], "child_loads": c[3],
            "distinct_leaves": int(seen.sum(dtype=torch.int64)) if count_leaves else None}


def grid_weight_count_work(sigma_grid, reso, c2w_all, fx, fy, width, height, opts, offset, invradius, count_voxels=True):
    """Work counters of pxo_grid_weight_render on the same cameras: dict(rays, samples, occupied_samples, distinct_voxels)."""
    _require_gpu()
    dev = sigma_grid.device
    c2w = c2w_all[:, :3, :4].contiguous().to(device=dev, dtype=torch.float32)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    seen = torch.zeros(reso ** 3, dtype=torch.uint8, device=dev) if count_voxels else None
    check(_lib.load().pxo_grid_weight_count_work(_f(sigma_grid.reshape(-1)), reso, _f(c2w), c2w.shape[0], float(fx), float(fy),
                                                 int(width), int(height), ctypes.byref(opts), _vec3(offset), _vec3(invradius),
                                                 _p(counts), _p(seen), _stream()), "pxo_grid_weight_count_work")
    c = counts.tolist()
    return {"rays": c[0], "samples": c[1], "occupied_samples": c[2],
            "distinct_voxels": int(seen.sum(dtype=torch.int64)) if count_voxels else None}


WEIGHT_OPS = {"max": 0, "sum": 1}


def _weight_op(op):
    if op not in WEIGHT_OPS:
        raise PxoError(f"weight accumulation op {op!r} is neither 'sum' nor 'max'")
    return WEIGHT_OPS[op]


def _weights_buffer(tree, weights, dev):
    """The [n_internal*8] float32 accumulator of the weight launches: a fresh zeroed one, or the caller's, checked."""
    cells = tree.n_internal * 8
    if weights is None:
        return torch.zeros(cells, dtype=torch.float32, device=dev)
    if weights.dtype != torch.float32 or weights.numel() != cells or not weights.is_contiguous() or not weights.is_cuda:
        raise PxoError(f"weights must be a contiguous float32 tensor of {cells} cells on the GPU")
    return weights


def octree_weight_accum_cams(tree, c2w_all, width, height, fx, opts, op="max", weights=None, fy=None, ndc=None):
    """Accumulates, per leaf of `tree` (a PxoTree), the compositing weights the forward renderer gives its samples over every
    pixel of the cameras c2w_all ([n,3,4] or [n,4,4]) into `weights` ([n_internal*8] float32, zeros when None): op "max" or
    "sum" (pxo_octree_weight_accum_cams).  ndc: as in octree_render_persp.  Returns `weights`."""
    _require_gpu()
    c2w = c2w_all[:, :3, :4].contiguous().to(dtype=torch.float32)
    weights = _weights_buffer(tree, weights, c2w.device)
    check(_lib.load().pxo_octree_weight_accum_cams(ctypes.byref(tree), _f(c2w), c2w.shape[0], float(fx),
                                                   float(fx if fy is None else fy), int(width), int(height), ctypes.byref(opts),
                                                   _weight_op(op), _f(weights), _stream(),
                                                   None if ndc is None else ctypes.byref(_ndc(ndc))),
          "pxo_octree_weight_accum_cams")
    return weights


def octree_weight_accum_rays(tree, origins, dirs, opts, op="max", weights=None, ndc=None):
    """octree_weight_accum_cams for explicit world-space rays [B,3] with unit dirs (pxo_octree_weight_accum_rays)."""
    _require_gpu()
    weights = _weights_buffer(tree, weights, origins.device)
    check(_lib.load().pxo_octree_weight_accum_rays(ctypes.byref(tree), _f(origins), _f(dirs), origins.shape[0],
                                                   ctypes.byref(opts), _weight_op(op), _f(weights), _stream(),
                                                   None if ndc is None else ctypes.byref(_ndc(ndc))),
          "pxo_octree_weight_accum_rays")
    return weights


def tree_collapse(child, parent_depth, data, keep):
    """Removes every node all of whose cells are dead (keep == 0 leaves, or children that are themselves removed; the root
    stays) and zeroes the rows of dead leaf cells: (child, parent_depth, data, old2new) of the collapsed tree, old2new int64
    [n] with -1 for removed nodes (pxo_tree_collapse_mark, a scan, pxo_tree_collapse_emit).  keep: bool / uint8 over cells."""
    _require_gpu()
    lib = _lib.load()
    n, D, dev = child.shape[0], data.shape[-1], child.device
    if child.dtype != torch.int32 or parent_depth.dtype != torch.int32 or data.dtype != torch.float32:
        raise PxoError("tree_collapse: child / parent_depth must be int32, data float32")
    if keep.numel() != n * 8 or data.numel() != n * 8 * D or parent_depth.numel() != n * 2:
        raise PxoError(f"tree_collapse: keep / data / parent_depth do not match the {n} nodes of child")
    child, parent_depth, data = child.contiguous(), parent_depth.contiguous(), data.detach().contiguous()
    keep = keep.reshape(-1).to(torch.uint8).contiguous()
    node_dead = _new(n, device=dev, dtype=torch.uint8)
    check(lib.pxo_tree_collapse_mark(_p(child), _p(parent_depth), _p(keep), n, int(parent_depth[:, 1].max()), _p(node_dead),
                                     _stream()), "pxo_tree_collapse_mark")
    alive = (node_dead == 0).to(torch.int64)
    new_index = (torch.cumsum(alive, 0) - alive).contiguous()            # exclusive scan of the survivors
    n_new = int(alive.sum())
    new_child = _new(n_new, 2, 2, 2, device=dev, dtype=torch.int32)
    new_pd = _new(n_new, 2, device=dev, dtype=torch.int32)
    new_data = _new(n_new, 2, 2, 2, D, device=dev)
    old2new = _new(n, device=dev, dtype=torch.int64)
    check(lib.pxo_tree_collapse_emit(_p(child), _p(parent_depth), _f(data), D, _p(keep), _p(node_dead), _p(new_index), n, n_new,
                                     _p(new_child), _p(new_pd), _f(new_data), _p(old2new), _stream()), "pxo_tree_collapse_emit")
    return new_child, new_pd, new_data, old2new


def tree_lod_fill(child, parent_depth, data, max_depth):
    """Writes into the row of every cell that has a child the density-weighted mean of that child's eight rows, deepest level
    first, in place (pxo_tree_lod_fill; the definition is in include/plenoctree_octree.h, "level of detail").  Leaf rows are
    not touched.  max_depth: the deepest node's depth.  Returns `data`."""
    _require_gpu()
    n, D = child.shape[0], data.shape[-1]
    if child.dtype != torch.int32 or parent_depth.dtype != torch.int32 or data.dtype != torch.float32:
        raise PxoError("tree_lod_fill: child / parent_depth must be int32, data float32")
    if child.numel() != n * 8 or data.numel() != n * 8 * D or parent_depth.numel() != n * 2:
        raise PxoError(f"tree_lod_fill: data / parent_depth do not match the {n} nodes of child")
    check(_lib.load().pxo_tree_lod_fill(_p(child), _p(parent_depth), _f(data), n, D, int(max_depth), _stream()),
          "pxo_tree_lod_fill")
    return data


def octree_render_rays(tree, origins, dirs, viewdirs, opts, lobes=None, ndc=None):
    """[B,3] colours of explicit world-space rays with unit dirs (VolumeRenderer.forward).  lobes, ndc: as in
    octree_render_persp (with ndc the rays are still given in world space; they are converted per ray)."""
    return _forward(tree, opts, rays=(origins, dirs, viewdirs), lobes=lobes, ndc=ndc)


# ---- compressed trees rendered in place (the palette form of octree/compression.py:88-139) ----
def quant_layout(n_internal, basis_dim, n_retained, bits):
    """PxoQuantLayout of the packed form (host only: no GPU needed)."""
    lay = _lib.PxoQuantLayout()
    check(_lib.load().pxo_octree_quant_pack_bytes(int(n_internal), int(basis_dim), int(n_retained), int(bits),
                                                  ctypes.byref(lay)), "pxo_octree_quant_pack_bytes")
    return lay


def quant_pack(quant_map, quant_colors, sigma, data_retained, n_internal, basis_dim, n_retained, bits):
    """The file's arrays, uploaded as they are (quant_map int16 holding the uint16 bits [Kq, n*8], quant_colors float16
    [Kq, 2^bits, 3], sigma float16 / float32 [n*8], data_retained float16 [r, n*8, 3] or None) -> the packed uint8 buffer."""
    _require_gpu()
    if quant_map.dtype != torch.int16 or quant_colors.dtype != torch.float16 or sigma.dtype not in (torch.float16, torch.float32):
        raise PxoError("quant_pack: quant_map must be int16 (uint16 bits), quant_colors float16, sigma float16 or float32")
    if data_retained is not None and data_retained.dtype != torch.float16:
        raise PxoError("quant_pack: data_retained must be float16")
    Kq, cells = basis_dim - n_retained, n_internal * 8
    if quant_map.numel() != Kq * cells or quant_colors.numel() != Kq * (3 << bits) or sigma.numel() != cells or \
            (data_retained.numel() if data_retained is not None else 0) != n_retained * cells * 3:
        raise PxoError("quant_pack: array sizes do not match (n_internal, basis_dim, n_retained, bits)")
    lay = quant_layout(n_internal, basis_dim, n_retained, bits)
    packed = torch.zeros(lay.total_bytes, dtype=torch.uint8, device=quant_map.device)
    check(_lib.load().pxo_octree_quant_pack(_p(quant_map), _p(quant_colors), _p(sigma), sigma.element_size(),
                                            _p(data_retained), n_internal, basis_dim, n_retained, bits, _p(packed),
                                            lay.total_bytes, _stream()), "pxo_octree_quant_pack")
    return packed, lay


def quant_tree_view(child, packed, lay, basis_dim, n_retained, bits, offset, invradius):
    """PxoQuantTree struct over torch storage (keeps no reference: the caller owns the tensors)."""
    t = _tree_fields(_lib.PxoQuantTree(), child, offset, invradius)
    if packed.dtype != torch.uint8 or packed.numel() < lay.total_bytes:
        raise PxoError("packed buffer is smaller than its layout")
    base = _p(packed).value
    t.idx = base + lay.idx_offset
    t.palette = base + lay.palette_offset
    t.sigma = base + lay.sigma_offset
    t.retained = base + lay.retained_offset
    t.basis_dim, t.n_retained, t.bits = int(basis_dim), int(n_retained), int(bits)
    t.idx_stride, t.ret_stride = lay.idx_stride, lay.ret_stride
    return t


def octree_render_quant_persp(qtree, c2w, width, height, fx, opts, fy=None):
    """octree_render_persp on a PxoQuantTree."""
    return _forward(qtree, opts, camera=(c2w, width, height, fx, fy))


def octree_render_quant_rays(qtree, origins, dirs, viewdirs, opts):
    """octree_render_rays on a PxoQuantTree."""
    return _forward(qtree, opts, rays=(origins, dirs, viewdirs))


# ---- float16 trees rendered in place (the data array of the files N3Tree.save writes) ----
def half_layout(n_internal, data_dim):
    """(row_stride in halves, bytes) of the packed form (host only: no GPU needed)."""
    stride, nbytes = ctypes.c_int32(0), ctypes.c_int64(0)
    check(_lib.load().pxo_octree_half_pack_bytes(int(n_internal), int(data_dim), ctypes.byref(stride), ctypes.byref(nbytes)),
          "pxo_octree_half_pack_bytes")
    return stride.value, nbytes.value


def half_pack(data, n_internal):
    """The file's data[:n_internal], uploaded as it is (float16 [n, 2,2,2, D] or [n*8, D]) -> (the packed float16 buffer
    [n*8, row_stride], row_stride)."""
    _require_gpu()
    if data.dtype != torch.float16 or not data.is_contiguous():
        raise PxoError("half_pack: data must be a contiguous float16 tensor")
    data_dim = data.shape[-1]
    if data.numel() != n_internal * 8 * data_dim:
        raise PxoError("half_pack: array size does not match (n_internal, data_dim)")
    stride, nbytes = half_layout(n_internal, data_dim)
    packed = torch.empty(n_internal * 8, stride, dtype=torch.float16, device=data.device)
    check(_lib.load().pxo_octree_half_pack(_p(data), n_internal, data_dim, _p(packed), nbytes, _stream()),
          "pxo_octree_half_pack")
    return packed, stride


def half_tree_view(child, packed, data_dim, offset, invradius):
    """PxoHalfTree struct over torch storage (keeps no reference: the caller owns the tensors)."""
    t = _tree_fields(_lib.PxoHalfTree(), child, offset, invradius)
    stride, nbytes = half_layout(child.shape[0], data_dim)
    if packed.dtype != torch.float16 or not packed.is_contiguous() or packed.numel() * 2 < nbytes:
        raise PxoError("packed buffer is smaller than its layout")
    t.data = _p(packed).value
    t.data_dim = int(data_dim)
    t.basis_dim = (int(data_dim) - 1) // 3
    t.row_stride = stride
    return t


def octree_render_half_persp(htree, c2w, width, height, fx, opts, fy=None, lobes=None, ndc=None):
    """octree_render_persp on a PxoHalfTree: bit for bit the image of the float tree with the widened data."""
    return _forward(htree, opts, camera=(c2w, width, height, fx, fy), lobes=lobes, ndc=ndc)


def octree_render_half_rays(htree, origins, dirs, viewdirs, opts, lobes=None, ndc=None):
    """octree_render_rays on a PxoHalfTree."""
    return _forward(htree, opts, rays=(origins, dirs, viewdirs), lobes=lobes, ndc=ndc)


def _half_only(htree):
    if not isinstance(htree, _lib.PxoHalfTree):
        raise PxoError(f"expected a PxoHalfTree, got {type(htree).__name__}")


def octree_render_half_aux_persp(htree, c2w, width, height, fx, opts, fy=None, surface_thresh=0.5):
    """octree_render_aux_persp on a PxoHalfTree (SH, world space): rgb and aux bit for bit those of the float tree."""
    _half_only(htree)
    return octree_render_aux_persp(htree, c2w, width, height, fx, opts, fy, surface_thresh)


def octree_render_half_aux_rays(htree, origins, dirs, viewdirs, opts, surface_thresh=0.5):
    """octree_render_aux_rays on a PxoHalfTree (SH, world space)."""
    _half_only(htree)
    return octree_render_aux_rays(htree, origins, dirs, viewdirs, opts, surface_thresh)


def octree_render_aux_persp(tree, c2w, width, height, fx, opts, fy=None, surface_thresh=0.5):
    """(rgb [H,W,3], aux [H,W,3]) of a pinhole camera from one march, for a PxoTree, a PxoQuantTree or a PxoHalfTree: rgb is
    octree_render_persp's, aux = (alpha, depth, surface) as defined at pxo_octree_render_aux_fwd.  Not differentiable."""
    return _forward(tree, opts, camera=(c2w, width, height, fx, fy), surface_thresh=surface_thresh)


def octree_render_aux_rays(tree, origins, dirs, viewdirs, opts, surface_thresh=0.5):
    """(rgb [B,3], aux [B,3]) of explicit world-space rays with unit dirs; see octree_render_aux_persp."""
    return _forward(tree, opts, rays=(origins, dirs, viewdirs), surface_thresh=surface_thresh)


def octree_render_foot_persp(tree, c2w, width, height, fx, opts, cone, min_depth=0, fy=None, lobes=None, surface_thresh=None):
    """octree_render_persp (surface_thresh None) or octree_render_aux_persp of a PxoTree whose data tree_lod_fill has filled,
    every sample at the depth its pixel footprint allows (pxo_octree_render_foot_fwd / _foot_aux_fwd).  cone: world-space
    width of a pixel per unit of distance along the ray; min_depth: no sample is folded above this depth."""
    return _forward(tree, opts, camera=(c2w, width, height, fx, fy), lobes=lobes, surface_thresh=surface_thresh,
                    foot=(cone, min_depth))


def octree_render_foot_rays(tree, origins, dirs, viewdirs, opts, cone, min_depth=0, lobes=None, surface_thresh=None):
    """octree_render_foot_persp for explicit world-space rays [B,3] with unit dirs."""
    return _forward(tree, opts, rays=(origins, dirs, viewdirs), lobes=lobes, surface_thresh=surface_thresh,
                    foot=(cone, min_depth))


def octree_render_rays_bwd(tree, origins, dirs, viewdirs, opts, grad_out, grad_data, out_rgb=None, lobes=None, ndc=None):
    _require_gpu()
    return _render_bwd(tree, lobes, _rays(None, origins, dirs, viewdirs), opts, out_rgb, grad_out, grad_data, ndc=ndc)


# ---- scene: several float SH trees in one world, each under a similarity transform (include/plenoctree_octree.h, "scene") ----
class SceneInstances:
    """The device array of a scene's PxoInstance records (`records`: uint8 on the trees' device) and their count.  Keeps no
    reference to the trees' tensors: the caller owns them for as long as the scene is rendered."""

    def __init__(self, records, n):
        self.records, self.n = records, n


def scene_instances(instances, device=None):
    """instances: a sequence of (PxoTree, rotation 3x3, translation 3, scale) with rotation R of x_w = scale R x_o +
    translation (float64 on the host; orthonormality is the caller's to check, svox.Instance does).  Checked by
    pxo_scene_check -- count, tree formats, scales -- and uploaded: a SceneInstances."""
    import numpy as np
    n = len(instances)
    if not 1 <= n <= _lib.SCENE_MAX_INSTANCES:
        raise PxoError(f"a scene takes 1 .. {_lib.SCENE_MAX_INSTANCES} instances, got {n}")
    host = (_lib.PxoInstance * n)()
    for rec, (tree, rotation, translation, scale) in zip(host, instances):
        if not isinstance(tree, _lib.PxoTree):
            raise NotImplementedError(f"a scene instance must be a float SH tree (PxoTree), got {type(tree).__name__}: float16, "
                                      "palette and SG instances are not built")
        rec.tree = tree
        rot_t = np.asarray(rotation, np.float64).reshape(3, 3).T.astype(np.float32)
        rec.rot_t = (ctypes.c_float * 9)(*rot_t.reshape(-1).tolist())
        rec.trans = _vec3(np.asarray(translation, np.float64).reshape(3))
        s = np.float32(scale)
        rec.scale = float(s)
        with np.errstate(all="ignore"):
            rec.inv_scale = float(np.float32(1.0) / s)
    check(_lib.load().pxo_scene_check(host, n), "pxo_scene_check")
    _require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    records = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    return SceneInstances(records, n)


def _scene_forward(scene, opts, camera=None, rays=None):
    _require_gpu()
    if not isinstance(scene, SceneInstances):
        raise PxoError(f"expected the SceneInstances of scene_instances(), got {type(scene).__name__}")
    if camera is not None:
        cam, keep = _camera(*camera)
        shape, rays = (cam.height, cam.width, 3), _rays(cam)
    else:
        shape, rays = (rays[0].shape[0], 3), _rays(None, *rays)
    out = _new(*shape, device=scene.records.device)
    check(_lib.load().pxo_scene_render_fwd(_p(scene.records), scene.n, *rays, ctypes.byref(opts), _f(out), _stream()),
          "pxo_scene_render_fwd")
    return out


def scene_render_persp(scene, c2w, width, height, fx, opts, fy=None):
    """[H,W,3] image of the scene (a SceneInstances) from a pinhole camera.  Always the scene kernel, also for one instance."""
    return _scene_forward(scene, opts, camera=(c2w, width, height, fx, fy))


def scene_render_rays(scene, origins, dirs, viewdirs, opts):
    """[B,3] colours of explicit world-space rays with unit dirs through the scene."""
    return _scene_forward(scene, opts, rays=(origins, dirs, viewdirs))


def scene_lds_bytes(n):
    """Dynamic LDS per workgroup of the scene kernel at n instances (host only)."""
    v = ctypes.c_size_t(0)
    check(_lib.load().pxo_scene_lds_bytes(int(n), ctypes.byref(v)), "pxo_scene_lds_bytes")
    return v.value


MSE_BLOCK, MSE_PER_THREAD, MSE_MAX_BLOCKS = 256, 8, 4096     # pxo_image_mse's launch (kMseBlock, kMsePerThread, kMseMaxBlocks)


def image_mse(im, gt, want_grad=True):
    """(sse device scalar, grad or None) of mean((clamp(im,0,1)-gt)^2)  (octree/optimization.py:217-219)."""
    _require_gpu()
    n = im.numel()
    grad = torch.empty_like(im) if want_grad else None
    sse = _new(1, device=im.device)
    check(_lib.load().pxo_image_mse(_f(im), _f(gt), n, _f(grad), _f(sse), _stream()), "pxo_image_mse")
    return sse, grad


def sgd_step(params, grads, lr, momentum=0.0, nesterov=False, buf=None, first_step=False):
    _require_gpu()
    check(_lib.load().pxo_sgd_step(_f(params), _f(grads), _f(buf), params.numel(), float(lr), float(momentum), int(nesterov),
                                   int(first_step), _stream()), "pxo_sgd_step")
