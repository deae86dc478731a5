"""numpy twin of the scene renderer (include/plenoctree_octree.h, "scene"): several trees in one world, each
under its own similarity transform x_w = s R x_o + t, marched together.

Built on oracle/octree_oracle.py (Tree.find, _to_tree_ray, _dda_unit, sh_basis_np): float32, one rounding per operation, in
the order the header pins.  Every sample descends from the root (Tree.find), so the twin cannot share the kernel's
path-reuse trap.  `render_ray(..., dtype=np.float64)` marches the same float32 rounds and composites them in double.
"""
import numpy as np

from oracle import octree_oracle as T

f32 = np.float32
MAX_INSTANCES = 8                    # PXO_SCENE_MAX_INSTANCES
DONE, WAITING, INSIDE = 0, 1, 2


class Instance:
    """A tree placed in the world: x_w = scale * rotation @ x_o + translation."""

    def __init__(self, tree, rotation=None, translation=(0.0, 0.0, 0.0), scale=1.0):
        self.tree = tree
        rot = np.eye(3) if rotation is None else np.asarray(rotation, np.float64)
        self.rot_t = rot.T.astype(f32).copy()                  # what the device record carries: R^T, row-major
        self.trans = np.asarray(translation, np.float64).astype(f32)
        self.scale = f32(scale)
        self.inv_scale = f32(f32(1.0) / self.scale)
        self.rows = tree.data.reshape(-1, tree.data_dim)
        self.basis_dim = (tree.data_dim - 1) // 3


def _rot(m, v):
    return np.array([f32(f32(f32(m[a, 0] * v[0]) + f32(m[a, 1] * v[1])) + f32(m[a, 2] * v[2])) for a in range(3)], f32)


class _Ray:
    """Ray constants of one instance (the per-instance set-up of the header)."""

    def __init__(self, inst, origin, direction, vdir):
        q = np.array([f32(origin[a] - inst.trans[a]) for a in range(3)], f32)
        o = (_rot(inst.rot_t, q) * inst.inv_scale).astype(f32)
        d = _rot(inst.rot_t, direction)
        self.vdir = _rot(inst.rot_t, vdir)
        with np.errstate(over="ignore", invalid="ignore"):
            self.o, self.d, self.invdir, delta_scale = T._to_tree_ray(o, d, inst.tree.offset, inst.tree.invradius)
            self.tmin, self.tmax = T._dda_unit(self.o, self.invdir)
        self.hit = (not (self.tmax < 0 or self.tmin > self.tmax)) and bool(self.tmin < self.tmax)
        self.c = f32(inst.scale * delta_scale)
        self.enter = f32(self.tmin * self.c)


class Counts:
    """What a ray's march went through: rounds, gap steps (a round whose step was a waiting instance's gap), rounds with two
    or more live instances, non-leader advances (an inside instance carried by another's step), jumps (nothing inside: w
    moved to the next entry), rays whose tmin is 0 for some instance (an origin inside it), and per set of hit instances the
    number of rays (`hits`: {tuple of instance indices: rays})."""

    def __init__(self):
        self.rounds = self.gap_steps = self.multi_live = self.non_leader = self.jumps = self.inside_origin = 0
        self.hits = {}


def render_ray(instances, origin, direction, vdir, opt, dtype=f32, counts=None):
    """rgb[3] of one world ray through the scene.  dtype float64: the float32 march, composited in double."""
    assert 1 <= len(instances) <= MAX_INSTANCES
    origin, direction, vdir = (np.asarray(v, f32) for v in (origin, direction, vdir))
    n = len(instances)
    rays = [_Ray(I, origin, direction, vdir) for I in instances]
    basis = [T.sh_basis_np(I.basis_dim, r.vdir).astype(dtype) for I, r in zip(instances, rays)]
    state = [WAITING if r.hit else DONE for r in rays]
    one, bg = dtype(1.0), dtype(opt.background_brightness)
    if counts is not None:
        key = tuple(i for i, s in enumerate(state) if s == WAITING)
        counts.hits[key] = counts.hits.get(key, 0) + 1
        counts.inside_origin += any(s == WAITING and r.tmin == 0 for r, s in zip(rays, state))
    if WAITING not in state:
        return np.full(3, bg, dtype)
    w = min(r.enter for r, s in zip(rays, state) if s == WAITING)
    tt = [r.tmin for r in rays]
    light, out, stopped = one, np.zeros(3, dtype), False
    cnt = Counts() if counts is None else counts
    leaf, delta, step = [0] * n, [f32(0)] * n, [f32(0)] * n
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        while True:
            d_min, any_inside, next_enter = f32(np.inf), False, f32(np.inf)
            for i, (I, r) in enumerate(zip(instances, rays)):
                if state[i] == WAITING and r.enter <= w:
                    state[i] = INSIDE
                if state[i] == INSIDE:
                    pos = np.array([f32(r.o[a] + f32(tt[i] * r.d[a])) for a in range(3)], f32)
                    nd, ci, cj, ck, cube, local, _ = I.tree.find(pos)
                    s0, s1 = T._dda_unit(local, r.invdir)
                    delta[i] = f32(f32(f32(s1 - s0) / cube) + opt.step_size)
                    leaf[i] = ((nd * 2 + ci) * 2 + cj) * 2 + ck
                    step[i] = f32(delta[i] * r.c)
                    d_min = min(d_min, step[i])
                    any_inside = True
                elif state[i] == WAITING:
                    step[i] = f32(r.enter - w)
                    d_min = min(d_min, step[i])
                    next_enter = min(next_enter, r.enter)
            if not any_inside:
                if not np.isfinite(next_enter):
                    break
                w = next_enter
                cnt.jumps += 1
                continue
            cnt.rounds += 1
            # one sample
            tau_i, tau = [None] * n, f32(0.0)
            for i, I in enumerate(instances):
                if state[i] == INSIDE:
                    sigma = I.rows[leaf[i], -1]
                    if sigma > opt.sigma_thresh:
                        tau_i[i] = f32(f32(d_min * I.inv_scale) * sigma)
                        tau = f32(tau + tau_i[i])
            live = [i for i in range(n) if tau_i[i] is not None]
            cnt.multi_live += len(live) >= 2
            if live and tau > 0:
                if dtype == f32:
                    att = f32(np.exp(f32(-tau), dtype=f32))
                    tau_c, tau_ic = tau, tau_i
                else:                                     # the same rounds, composited in double from the float32 inputs
                    tau_ic = [None if tau_i[i] is None else
                              float(d_min) * float(instances[i].inv_scale) * float(instances[i].rows[leaf[i], -1])
                              for i in range(n)]
                    tau_c = sum(v for v in tau_ic if v is not None)
                    att = np.exp(-tau_c)
                weight = dtype(light * dtype(one - att))
                for i in live:
                    I = instances[i]
                    share = dtype(weight * dtype(dtype(tau_ic[i]) / dtype(tau_c)))
                    coef = I.rows[leaf[i], :-1].reshape(3, I.basis_dim).astype(dtype)
                    logit = np.zeros(3, dtype)
                    for q in range(I.basis_dim):
                        logit = (logit + basis[i][q] * coef[:, q]).astype(dtype)
                    out = (out + share * (one / (one + np.exp(-logit)))).astype(dtype)
                light = dtype(light * att)
                if light <= opt.stop_thresh:
                    stopped = True
                    break
            # advance
            snap = None
            for i, r in enumerate(rays):
                if state[i] == INSIDE:
                    if step[i] == d_min:
                        tn = f32(tt[i] + delta[i])
                    else:
                        tn = f32(tt[i] + f32(d_min / r.c))
                        cnt.non_leader += 1
                    if not tn > tt[i] or tn >= r.tmax:
                        state[i] = DONE
                    else:
                        tt[i] = tn
                elif state[i] == WAITING and step[i] == d_min:
                    snap = r.enter if snap is None else max(snap, r.enter)
            if snap is not None:
                cnt.gap_steps += 1
                w = snap
            else:
                w = f32(w + d_min)
    if stopped:
        return (out * (one / (one - light))).astype(dtype)
    return (out + light * bg).astype(dtype)


def render_rays(instances, origins, dirs, vdirs, opt, dtype=f32, counts=None):
    return np.stack([render_ray(instances, o, d, v, opt, dtype, counts) for o, d, v in
                     zip(np.asarray(origins, f32), np.asarray(dirs, f32), np.asarray(vdirs, f32))])


def render_persp(instances, c2w, W, H, fx, opt, fy=None, dtype=f32, counts=None):
    o, d = T.camera_rays(c2w, W, H, fx, fy)
    return render_rays(instances, o, d, d, opt, dtype, counts).reshape(H, W, 3)


# -- helpers for the tests -----------------------------------------------------------------------------------------------
def axis_angle(axis, angle_deg):
    """Rotation matrix (float64) about `axis` by angle_deg (Rodrigues)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


CYCLIC = np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # x -> y -> -z -> x: det +1, not an involution


def split_by_x(tree):
    """(a, b): two copies of `tree` sharing its structure; a has sigma zeroed in the leaves whose lower corner has x < 0.5
    (tree coordinates), b in the rest."""
    import copy
    lv = tree.leaves()
    corner, _ = T.leaf_corners(tree, lv)
    low = corner[:, 0] < 0.5
    a, b = copy.deepcopy(tree), copy.deepcopy(tree)
    for t, sel in ((a, low), (b, ~low)):
        s = lv[sel]
        t.data[s[:, 0], s[:, 1], s[:, 2], s[:, 3], -1] = 0.0
    return a, b


def transformed_camera(c2w, rot, scale):
    """c2w' = [R c2w_rot | scale R c2w_pos]: the camera that sees an instance (R, scale, t = 0) as c2w sees the tree."""
    c2w = np.asarray(c2w, np.float64)
    out = np.eye(4)
    out[:3, :3] = rot @ c2w[:3, :3]
    out[:3, 3] = scale * (rot @ c2w[:3, 3])
    return out.astype(f32)
