"""The extra outputs of the octree renderer (pxo_octree_render_aux_fwd: alpha, depth, surface) from oracle/octree_oracle.py, in
the shape tests/test_octree_aux_cpu.py and tests/test_gpu_octree_aux.py compare against: one march per ray (`march`),
composited twice (`composite` with a surface_thresh) -- in float32, whose rgb is render_ray's bit for bit, and in float64 over
the same float32 samples, the yardstick for how much of a difference is float32 round-off.  TEST INFRASTRUCTURE."""
import numpy as np

from oracle import octree_oracle as T


def render_rays_aux(tree, origins, dirs, vdirs, opt, surface_thresh=0.5):
    """(float32 Batch, float64 Batch) of explicit rays."""
    marches = [T.march(tree, o, d, opt.step_size) for o, d in zip(origins, dirs)]
    bases = [T.view_basis(tree, v) for v in vdirs]
    return T.composite_batches(tree.data.reshape(-1, tree.data_dim), marches, bases, opt, surface_thresh)


def render_ray_aux(tree, origin, direction, vdir, opt, surface_thresh=0.5):
    """(float32 Rendered, float64 Rendered) of one ray from one march."""
    m, rows = T.march(tree, origin, direction, opt.step_size), tree.data.reshape(-1, tree.data_dim)
    return tuple(T.composite(rows, m, T.view_basis(tree, vdir), opt, dtype, surface_thresh) for dtype in (np.float32, np.float64))


def render_persp_aux(tree, c2w, W, H, fx, opt, surface_thresh=0.5, fy=None):
    """(float32 Batch, float64 Batch) of a pinhole camera, rays in row-major pixel order (reshape to [H,W,..])."""
    o, d = T.camera_rays(c2w, W, H, fx, fy)
    return render_rays_aux(tree, o, d, d, opt, surface_thresh)
