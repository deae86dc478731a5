"""Occupancy grids for ray rendering of a trained NeRF (no reference counterpart: the reference's NerfModel.__call__ sends every
sample of every ray through the MLP, nerf_sh/nerf/models.py:242-264, :308-330).

A grid is one bit per cell of a reso^3 grid over the box a PlenOctree of the scene would span (extraction.tree_transform: a world
point p has grid coordinate t = p * scale + offset, inside iff t in [0,1)^3).  model.apply(..., occupancy=grid) then evaluates
only the samples in occupied cells (ops.render_fwd_culled); the others get raw sigma 0, hence weight 0.  Two sources:

  from_model  the fine MLP's sigma on the grid (extraction.grid_sigma, sharded over the ranks), a cell occupied iff a cell within
              `dilate` of it has sigma > sigma_thresh(alpha_thresh, radius, reso) -- the threshold of the extraction's step 1
  from_tree   a finished float SH or SG tree sampled at 2^depth cells per axis (pxo_tree_sigma_grid), occupied iff sigma > 0, over
              the tree's own box

Rendering: opt-in, nerf_sh.eval / nerf_sh.gen_video --occupancy_reso R.  Training: opt-in, nerf_sh.train --cull_reso R -- a
TrainingGrid follows the model (rebuilt from the fine MLP every --cull_update_every steps after --cull_warmup_steps dense steps),
models.train_step(..., occupancy=grid) runs both levels' MLPs, forward and reverse, on the live samples only
(ops.train_fwd_bwd_culled), and the periodic test render goes through the same grid.  Not built: SG and view-conditioned training
through the grid, NDC scenes, culling in extraction and meshing, a device-side row count.
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
    # nerf_sh.train: the grid that follows the model while it trains (TrainingGrid)
    a("--cull_reso", type=int, default=0,
      help="nerf_sh.train: cells per axis of an occupancy grid rebuilt from the fine MLP while training; the train step and the test "
           "renders then run the MLPs on the samples in occupied cells only; 0 = off (every sample is evaluated)")
    a("--cull_center", type=_floats(3), default=[0.0, 0.0, 0.0], help='centre of the training grid\'s box, "x y z"')
    a("--cull_radius", type=_floats(3), default=[1.5, 1.5, 1.5], help='half side of the training grid\'s box, "r" or "rx ry rz"')
    a("--cull_alpha_thresh", type=float, default=0.01,
      help="a cell of the training grid is occupied if its alpha over one cell side exceeds this; 0: sigma > 0")
    a("--cull_dilate", type=int, choices=(0, 1), default=1, help="also occupy the cells next to an occupied one")
    a("--cull_warmup_steps", type=int, default=500, help="steps that run dense before the first grid is built")
    a("--cull_update_every", type=int, default=32,
      help="the grid is rebuilt from scratch before every step s > cull_warmup_steps with (s - 1) %% cull_update_every == 0 (and "
           "whenever there is none: at the first culled step and after a resume).  The schedule depends on the step alone: a run "
           "resumed from a checkpoint whose step is a multiple of cull_update_every continues bit for bit")
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


# ---- nerf_sh.train --cull_reso: the grid that follows the model ------------------------------------------------------------------
def cull_wanted(args):
    return int(getattr(args, "cull_reso", 0) or 0) != 0


def cull_clauses(args):
    """What the --cull_* flags ask of nerf_sh.train that is not built, in words (the SH family's `train` clauses call this)."""
    if not cull_wanted(args):
        return []
    bad = []
    reso = int(args.cull_reso)
    if not 1 <= reso <= ops._lib.OCC_MAX_RESO:
        bad.append(f"cull_reso={reso} (need 1..{ops._lib.OCC_MAX_RESO}, or 0 = off)")
    if getattr(args, "use_viewdirs", False):
        bad.append("cull_reso with use_viewdirs=true (training through the occupancy grid is not built for the view-conditioned head)")
    if getattr(args, "dataset", None) == "llff" and not getattr(args, "spherify", False):
        bad.append("cull_reso on a forward-facing scene without --spherify (NDC: the grid is not built for NDC rays)")
    if getattr(args, "noise_std", None) and getattr(args, "randomized", False):
        bad.append("cull_reso with noise_std and randomized sampling (noise on a culled sample's zero sigma would resurrect it)")
    alpha = float(getattr(args, "cull_alpha_thresh", 0.01))
    if not 0.0 <= alpha < 1.0:
        bad.append(f"cull_alpha_thresh={alpha:g} (need 0 <= a < 1)")
    if min(getattr(args, "cull_radius", [1.5])) <= 0.0:
        bad.append(f"cull_radius={args.cull_radius} (need > 0)")
    if int(getattr(args, "cull_warmup_steps", 0)) < 0:
        bad.append(f"cull_warmup_steps={args.cull_warmup_steps} (need >= 0)")
    if int(getattr(args, "cull_update_every", 1)) < 1:
        bad.append(f"cull_update_every={args.cull_update_every} (need >= 1)")
    return bad


class TrainingGrid:
    """The occupancy grid of a training run.  before_step(step, model, state) gives the grid step `step` runs through, or None
    for a dense step:

      * the first `warmup_steps` steps run dense;
      * from then on the grid is rebuilt before every step s with (s - 1) % update_every == 0, and whenever there is none (the
        first culled step; the first step after a resume) -- from scratch, never as a running maximum: `build` evaluates the
        fine MLP in EVERY cell, so density that grows into a culled cell by the network's continuity turns the cell back on;
      * between rebuilds the grid is reused;
      * a rebuild that finds no occupied cell makes the steps up to the next rebuild dense, and says so once.

    The schedule is a function of the step alone, and every rank builds the same grid from the same parameters (no
    communication; the ranks' live-row counts differ, the gradient all-reduces do not change).  build(model, state) -> a grid
    with fraction_occupied(); the default is from_model over the box (center, radius)."""

    def __init__(self, reso, center=(0.0, 0.0, 0.0), radius=1.5, alpha_thresh=0.01, dilate=1, warmup_steps=500, update_every=32,
                 build=None, say=print):
        check_grid_args(reso, dilate, "empty")
        if int(update_every) < 1 or int(warmup_steps) < 0:
            raise ValueError(f"TrainingGrid: update_every {update_every} < 1 or warmup_steps {warmup_steps} < 0")
        self.reso, self.warmup_steps, self.update_every = int(reso), int(warmup_steps), int(update_every)
        self.build = build or (lambda model, state: from_model(model, state, reso, center, radius, alpha_thresh, dilate, "empty"))
        self.say = say
        self.grid = None                  # the grid in use (None: none built yet, or the last build was empty)
        self.built_at = None              # the step before which the last rebuild ran
        self.rebuilds = []                # every such step, in order
        self.fraction = None              # the last build's occupied fraction
        self.rebuild_seconds = 0.0        # and its time
        self.live = None                  # LiveRows since the last line()
        self._said_empty = False

    @classmethod
    def from_args(cls, args, say=print):
        """The TrainingGrid of the --cull_* flags, or None without --cull_reso."""
        if not cull_wanted(args):
            return None
        return cls(args.cull_reso, args.cull_center, args.cull_radius, args.cull_alpha_thresh, args.cull_dilate,
                   args.cull_warmup_steps, args.cull_update_every, say=say)

    def due(self, step):
        """Whether a rebuild runs before step `step` (1-based, the step about to be taken)."""
        if step <= self.warmup_steps:
            return False
        return self.built_at is None or (step - 1) % self.update_every == 0

    def before_step(self, step, model, state):
        if step <= self.warmup_steps:
            return None
        if self.due(step) and self.built_at != step:
            import torch
            t0 = time.time()
            grid = self.build(model, state)
            self.fraction = float(grid.fraction_occupied())              # reads the bits back: the build is complete
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            self.rebuild_seconds = time.time() - t0
            self.built_at = step
            self.rebuilds.append(step)
            self.grid = grid if self.fraction > 0.0 else None
            if self.grid is None and not self._said_empty:
                self._said_empty = True
                self.say(f"* training grid {self.reso}^3 rebuilt before step {step}: no occupied cell -- the steps run dense until a "
                         "rebuild finds one", flush=True)
        return self.grid

    def count(self, cfg, rows, n_rays):
        """Add one culled step's live rows (train_step's live_rows) to the fractions of the next line()."""
        if self.live is None:
            self.live = LiveRows(cfg)
        self.live.add(rows, n_rays)

    def line(self):
        """What the progress line gains: the live-row fractions since the last call and the last rebuild's time."""
        if self.built_at is None:
            return f"cull: dense until step {self.warmup_steps + 1}"
        if self.live is None or not self.live.total[0]:
            return f"cull: dense (grid {100.0 * (self.fraction or 0.0):.2f} % occupied)"
        text = (f"{self.live.line()}, grid {100.0 * self.fraction:.2f} % occupied, rebuilt before step {self.built_at} in "
                f"{self.rebuild_seconds:.3f} s")
        self.live.reset()
        return text


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
