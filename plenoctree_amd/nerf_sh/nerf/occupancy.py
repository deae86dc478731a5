"""Occupancy grids for ray rendering of a trained NeRF (no reference counterpart: the reference's NerfModel.__call__ sends every
sample of every ray through the MLP, nerf_sh/nerf/models.py:242-264, :308-330).

A grid is one bit per cell of a reso^3 grid over the box a PlenOctree of the scene would span (extraction.tree_transform: a world
point p has grid coordinate t = p * scale + offset, inside iff t in [0,1)^3).  model.apply(..., occupancy=grid) then evaluates
only the samples in occupied cells (ops.render_fwd_culled); the others get raw sigma 0, hence weight 0.  Two sources:

  from_model  the fine MLP's sigma on the grid (extraction.grid_sigma, sharded over the ranks), a cell occupied iff a cell within
              `dilate` of it has sigma > sigma_thresh(alpha_thresh, radius, reso) -- the threshold of the extraction's step 1
  from_tree   a finished float SH or SG tree sampled at 2^depth cells per axis (pxo_tree_sigma_grid), occupied iff sigma > 0, over
              the tree's own box

Forward-only and opt-in (nerf_sh.eval / nerf_sh.gen_video --occupancy_reso R); not built: culling inside training or its test
renders, the view-conditioned head, NDC scenes, a grid that follows a model while it trains.
"""
import math
import time

import numpy as np

from ... import ops

OUTSIDE = ("empty", "live")


def sigma_thresh(alpha_thresh, radius, reso):
    """The sigma above which a cell of side 2 min(radius) / reso has alpha > alpha_thresh: -ln(1 - alpha_thresh) / (2 min(radius) /
    reso) (octree/extraction.py:322-326 with the box's shortest side for approx_delta).  alpha_thresh = 0 gives 0: sigma > 0."""
    alpha_thresh = float(alpha_thresh)
    if not 0.0 <= alpha_thresh < 1.0:
        raise ValueError(f"occupancy alpha_thresh {alpha_thresh} outside [0, 1)")
    rmin = float(np.min(np.broadcast_to(np.asarray(radius, np.float64), (3,))))
    if not rmin > 0.0:
        raise ValueError(f"occupancy radius {radius} must be > 0")
    if alpha_thresh == 0.0:
        return 0.0
    return -math.log(1.0 - alpha_thresh) / (2.0 * rmin / int(reso))


def check_grid_args(reso, dilate, outside):
    """What a grid can be refused for before a GPU is touched."""
    if not 1 <= int(reso) <= ops._lib.OCC_MAX_RESO:
        raise ValueError(f"occupancy reso {reso} outside [1, {ops._lib.OCC_MAX_RESO}]")
    if int(dilate) not in (0, 1):
        raise ValueError(f"occupancy dilate {dilate} is not 0 or 1")
    if outside not in OUTSIDE:
        raise ValueError(f"occupancy outside {outside!r} is not one of {OUTSIDE}")


def from_model(model, state, reso, center=(0.0, 0.0, 0.0), radius=1.5, alpha_thresh=0.01, dilate=1, outside="empty", comm=None):
    """The grid of a trained SH or SG model: sigma of the fine MLP at the reso^3 cell centres of the box (center, radius)."""
    from ...octree import extraction
    check_grid_args(reso, dilate, outside)
    thresh = sigma_thresh(alpha_thresh, radius, reso)
    offset, scale = extraction.tree_transform(center, radius)
    sigma = extraction.grid_sigma(model, state, int(reso), center, radius, comm)
    bits = ops.occ_pack(sigma, reso, thresh, dilate)
    return ops.OccupancyGrid(bits, reso, offset, scale, outside_live=outside == "live")


def from_tree(path_or_tree, depth, dilate=1, outside="empty", device=None, ndc=None):
    """The grid of a finished float SH or SG PlenOctree (a path or an N3Tree), 2^depth cells per axis, depth <= the tree's own
    finest grid (max_depth + 1); occupied iff the leaf at the cell's centre has sigma > 0."""
    from ... import mesh_ops
    from ...octree import svox
    depth = int(depth)
    if ndc is not None:
        raise NotImplementedError("occupancy grid from an NDC tree (a forward-facing scene without --spherify): not built -- "
                                  "its box is the NDC cube, the NeRF's samples are culled in world space")
    if isinstance(path_or_tree, svox.QuantizedN3Tree):
        raise NotImplementedError("occupancy grid from a compressed tree (QuantizedN3Tree): not built -- load the float tree")
    if isinstance(path_or_tree, svox.N3Tree):
        tree = path_or_tree
    else:
        with np.load(path_or_tree) as z:
            if "quant_colors" in z.files:
                raise NotImplementedError(f"occupancy grid from a compressed tree ({path_or_tree}): not built -- pass the float "
                                          "tree the compression started from")
        tree = svox.N3Tree.load(path_or_tree, device=device if device is not None else "cuda")
    if depth < 1:
        raise ValueError(f"occupancy tree depth {depth} < 1")
    check_grid_args(1 << depth, dilate, outside)
    if depth > tree.max_depth + 1:
        raise ValueError(f"occupancy tree depth {depth} (reso {1 << depth}) is finer than the tree's own grid: its depth is "
                         f"{tree.max_depth + 1} (reso {1 << (tree.max_depth + 1)})")
    sigma, _ = mesh_ops.tree_sigma_grid(tree.view(), depth, pad=0, want_packed=False, device=tree.device)
    bits = ops.occ_pack(sigma.reshape(-1), 1 << depth, 0.0, dilate)
    return ops.OccupancyGrid(bits, 1 << depth, tree.offset.tolist(), tree.invradius.tolist(), outside_live=outside == "live")


# ---- command line (nerf_sh.eval, nerf_sh.gen_video) ----------------------------------------------------------------------------
def _floats(n):
    def parse(text):
        vals = [float(v) for v in str(text).replace(",", " ").split()]
        if len(vals) not in (1, n):
            raise ValueError(f"expected 1 or {n} numbers, got {text!r}")
        return vals * n if len(vals) == 1 else vals
    return parse


def add_flags(parser):
    """The --occupancy_* flags of the renderers' command lines."""
    a = parser.add_argument
    a("--occupancy_reso", type=int, default=0,
      help="cells per axis of an occupancy grid that skips empty samples while rendering; 0 = off (every sample is evaluated)")
    a("--occupancy_center", type=_floats(3), default=[0.0, 0.0, 0.0], help='centre of the grid\'s box, "x y z"')
    a("--occupancy_radius", type=_floats(3), default=[1.5, 1.5, 1.5], help='half side of the grid\'s box, "r" or "rx ry rz"')
    a("--occupancy_alpha_thresh", type=float, default=0.01,
      help="a cell is occupied if its alpha over one cell side exceeds this (the extraction's --alpha_thresh); 0: sigma > 0")
    a("--occupancy_dilate", type=int, choices=(0, 1), default=1, help="also occupy the cells next to an occupied one")
    a("--occupancy_outside", choices=OUTSIDE, default="empty", help="samples outside the grid's box: skipped, or evaluated")
    a("--occupancy_tree", type=str, default="", help="take the grid from this float PlenOctree (npz) instead of the model; "
                                                      "--occupancy_reso must then be a power of two")
    return parser


def wanted(args):
    return int(getattr(args, "occupancy_reso", 0) or 0) != 0


def clauses(args):
    """What the --occupancy_* flags ask for that is not built, in words (the families table's `render` clauses call this)."""
    if not wanted(args):
        if getattr(args, "occupancy_tree", ""):
            return ["occupancy_tree without occupancy_reso (give the grid's resolution, a power of two)"]
        return []
    bad = []
    reso = int(args.occupancy_reso)
    if not 1 <= reso <= ops._lib.OCC_MAX_RESO:
        bad.append(f"occupancy_reso={reso} (need 1..{ops._lib.OCC_MAX_RESO}, or 0 = off)")
    if getattr(args, "use_viewdirs", False):
        bad.append("occupancy_reso with use_viewdirs=true (the occupancy grid is not built for the view-conditioned head)")
    if getattr(args, "dataset", None) == "llff" and not getattr(args, "spherify", False):
        bad.append("occupancy_reso on a forward-facing scene without --spherify (NDC: the grid is not built for NDC rays)")
    if getattr(args, "noise_std", None) and getattr(args, "randomized", False):
        bad.append("occupancy_reso with noise_std and randomized rendering (noise on a culled sample's zero sigma would resurrect it)")
    if getattr(args, "occupancy_tree", "") and reso >= 1 and reso & (reso - 1):
        bad.append(f"occupancy_reso={reso} with occupancy_tree (a tree's grid has 2^depth cells per axis: need a power of two)")
    alpha = float(getattr(args, "occupancy_alpha_thresh", 0.01))
    if not 0.0 <= alpha < 1.0:
        bad.append(f"occupancy_alpha_thresh={alpha:g} (need 0 <= a < 1)")
    radius = getattr(args, "occupancy_radius", [1.5])
    if min(radius) <= 0.0:
        bad.append(f"occupancy_radius={radius} (need > 0)")
    return bad


def from_args(args, model, state, comm=None, say=print):
    """The grid the --occupancy_* flags describe, or None without --occupancy_reso; says its occupied fraction and build time."""
    if not wanted(args):
        return None
    t0 = time.time()
    if args.occupancy_tree:
        grid = from_tree(args.occupancy_tree, int(args.occupancy_reso).bit_length() - 1, args.occupancy_dilate,
                         args.occupancy_outside, device=state.params.device)
        source = f"tree {args.occupancy_tree}"
    else:
        grid = from_model(model, state, args.occupancy_reso, args.occupancy_center, args.occupancy_radius,
                          args.occupancy_alpha_thresh, args.occupancy_dilate, args.occupancy_outside, comm)
        source = f"model, alpha_thresh {args.occupancy_alpha_thresh:g}"
    frac = grid.fraction_occupied()                                      # reads the bits back: the build is complete
    say(f"* occupancy grid {grid.reso}^3 from {source}, dilate {args.occupancy_dilate}, outside {args.occupancy_outside}: "
        f"{100.0 * frac:.2f} % of the cells occupied, built in {time.time() - t0:.3f} s", flush=True)
    return grid


def render_fn(args, model, state, comm=None, say=print):
    """(the chunk renderer utils.render_image takes, a LiveRows or None) of a deterministic render: without --occupancy_reso
    model.apply as it is; with it the grid is built here, once, and every chunk goes through it."""
    grid = from_args(args, model, state, comm, say)
    if grid is None:
        return (lambda r: model.apply(state, r, False)), None
    live = LiveRows(model.cfg)

    def fn(r):
        rows = []
        out = model.apply(state, r, False, occupancy=grid, live_rows=rows)
        live.add(rows, r.origins.shape[0])
        return out
    return fn, live


class LiveRows:
    """Rows that went through MLP_0 / MLP_1 over the chunks of one image, against all sample rows."""

    def __init__(self, cfg):
        self.per_ray = (cfg.num_coarse_samples, cfg.num_coarse_samples + cfg.num_fine_samples if cfg.num_fine_samples > 0 else 0)
        self.reset()

    def reset(self):
        self.live, self.total = [0, 0], [0, 0]

    def add(self, rows, n_rays):
        for i in range(2):
            self.live[i] += int(rows[i])
            self.total[i] += n_rays * self.per_ray[i]

    def fractions(self):
        return [self.live[i] / self.total[i] if self.total[i] else 0.0 for i in range(2)]

    def line(self):
        c, f = self.fractions()
        return f"live rows: coarse {100.0 * c:.2f} %, fine {100.0 * f:.2f} %"
