"""NeRF-SH -> PlenOctree extraction on the MI355X path (reference: octree/extraction.py).

  step 0  auto_scale (:244-286)            sigma on a 2^depth grid -> bounding box
  step 1  grid eval (:288-320)             sigma of MLP_1 on the 2^(depth+1) grid, x-slabs sharded over the GPUs
          masking (:322-335)               "sigma": sigma >= thresh; "weight": max compositing weight over the
                                           training views (calculate_grid_weights :181-214), cameras sharded
          tree build (:337-352)            N3Tree.refine_from_mask (Morton pyramid + scans)
  step 2  3-D antialiasing (:355-394)      S samples per deepest-level cell -> MLP_1 -> mean -> tree data,
                                           nodes sharded over the GPUs
  finish  relu on sigma, save npz, evaluate (:503-516)
  --config llff (forward-facing scene, not --spherify): the grid and the tree span the NDC cube (--radius 1 1 1 --center 0 0 0,
          --z_min / --z_max to drop planes); the weight mask and the evaluation convert every world-space camera ray to NDC
          (svox.NDCConfig).  With --spherify the scene is an ordinary world-space one.
  --sg_dim K --sh_deg -1 (a NeRF-SG, :436-442, :481-499): the same steps with the MLP head of K lobes; the tree is `SG<K>` and
  carries the lobes (softplus(sg_lambda), spher2cart(sg_mu_spher)) as extra_data

    python -m plenoctree_amd.octree.extraction --train_dir D --config blender --data_dir ... --output tree.npz
    python -m torch.distributed.run --nproc-per-node 8 -m plenoctree_amd.octree.extraction ...
"""
import os
import sys
import time

import numpy as np
import torch

from .. import dist, ops
from .. import octree_ops as oops
from ..nerf_sh.nerf import families, llff, sg, utils
from .svox import N3Tree, NDCConfig, VolumeRenderer


def uses_ndc(args):
    """Whether the octree of this run lives in NDC: an LLFF scene that is not --spherify (octree/extraction.py:187,
    octree/nerf/utils.py:451; octree/optimization.py:170 leaves the spherify test out, which would render a spherified scene
    in a space its NeRF never saw -- all three entry points here use this one rule)."""
    return getattr(args, "dataset", None) == "llff" and not getattr(args, "spherify", False)


def ndc_config(args, dataset):
    """svox.NDCConfig of the run's dataset (octree/extraction.py:187-191), or None for a world-space scene."""
    return NDCConfig(width=dataset.w, height=dataset.h, focal=dataset.focal) if uses_ndc(args) else None


def check_octree_flags(args, who, ndc_refused=()):
    """What the octree entry points refuse by name on LLFF scenes: --render_path (the camera path has no ground truth and
    no octree-side writer), and on an NDC scene the flags in `ndc_refused` (name, is-set pairs)."""
    if getattr(args, "render_path", False):
        raise NotImplementedError(f"{who}: --render_path is not built on the octree side (render the camera path with "
                                  "nerf_sh.eval / nerf_sh.gen_video)")
    bad = [name for name, on in ndc_refused if on]
    if bad and uses_ndc(args):
        raise NotImplementedError(f"{who}: {', '.join(bad)} not built for an NDC scene (--dataset llff without --spherify): "
                                  "palette-form rendering and the alpha / depth / surface outputs have no NDC form")


def tree_transform(center, radius):
    """N3Tree's offset / invradius (octree/extraction.py:250-251)."""
    radius = np.broadcast_to(np.asarray(radius, np.float32), (3,)).copy()
    center = np.broadcast_to(np.asarray(center, np.float32), (3,)).copy()
    return 0.5 * (1.0 - center / radius), 0.5 / radius


def grid_sigma(model, state, reso, center, radius, comm=None):
    """sigma of MLP_1 (fine) on the reso^3 grid, x slowest (extraction.py:294-320), evaluated in
    x-slabs sharded over the ranks of `comm` and all-gathered (every rank returns the full grid)."""
    comm = comm or dist.Comm()
    offset, scale = tree_transform(center, radius)
    which = 1 if model.num_fine_samples > 0 else 0
    x0, x1 = dist.slab_range(reso, comm.world, comm.rank)
    dev = state.params.device
    plane = reso * reso
    if reso % comm.world == 0:
        # equal slabs (the 8-way split of the 512^3 grid): every rank evaluates straight into its rows of the final
        # buffer and the all-gather lands in place -- no padded staging buffer, no second 537 MB concatenation
        full = torch.empty(reso * plane, dtype=torch.float32, device=dev)
        mine = full[x0 * plane: x1 * plane]
        ops.grid_sigma(model.cfg, state.packed[which][0], reso, x0, x1, offset, scale, out=mine)
        if comm.is_dist:
            comm.all_gather_into(full, mine)
        return full
    base, rem = divmod(reso, comm.world)
    width = base + 1                                      # ragged slabs: equal-size padded buffers for all_gather
    slab = torch.zeros(width * plane, dtype=torch.float32, device=dev)
    if x1 > x0:
        ops.grid_sigma(model.cfg, state.packed[which][0], reso, x0, x1, offset, scale, out=slab[: (x1 - x0) * plane])
    full = comm.all_gather_cat(slab).reshape(comm.world, width * plane)
    parts = []
    for r in range(comm.world):
        a, b = dist.slab_range(reso, comm.world, r)
        parts.append(full[r, : (b - a) * plane])
    return torch.cat(parts)


def auto_scale(model, state, center, radius, init_grid_depth=8, scale_alpha_thresh=0.01, comm=None, z_min=None,
               z_max=None):
    """Bounding box of sigma >= thresh on a 2^depth grid (extraction.py:244-286)."""
    reso = 2 ** init_grid_depth
    sig = grid_sigma(model, state, reso, center, radius, comm)
    sigma_thresh = -np.log(1.0 - scale_alpha_thresh) / (2.0 / reso)
    offset, scale = tree_transform(center, radius)
    mask = z_range_mask((sig >= sigma_thresh), reso, offset, scale, z_min, z_max).reshape(reso, reso, reso)
    arr = (torch.arange(reso, dtype=torch.float32, device=sig.device) + 0.5) / reso
    lc, uc = [], []
    for ax in range(3):
        other = tuple(a for a in range(3) if a != ax)
        occ = mask.any(dim=other)
        if not bool(occ.any()):
            raise RuntimeError("auto_scale: no voxel above the sigma threshold")
        coords = ((arr - float(offset[ax])) / float(scale[ax]))[occ]
        lc.append(float(coords.min()) - 0.5 / reso)
        uc.append(float(coords.max()) + 0.5 / reso)
    lc, uc = np.array(lc), np.array(uc)
    return ((lc + uc) * 0.5).tolist(), ((uc - lc) * 0.5).tolist()


def eval_leaf_samples(model, state, points, samples_per_cell):
    """Step 2 (extraction.py:367-393, SH/SG formats): [n_cells*S, 3] points -> mean over the S
    samples of cat([raw_rgb, raw_sigma]) -> [n_cells, 3K+1]."""
    rgb, sigma = model.eval_points_raw(state, points)
    return ops.mean_over_samples(model.cfg, rgb, sigma, samples_per_cell)


def calculate_grid_weights(dataset, sigmas, reso, invradius, offset, step_size, comm=None, ndc=None):
    """calculate_grid_weights (:181-214): per-voxel maximum over the training cameras, camera-sharded.  ndc: the NDCConfig of a
    forward-facing scene (the grid then spans the NDC cube and every camera ray is converted), None otherwise."""
    comm = comm or dist.Comm()
    opts = oops.render_opts(step_size=step_size, sigma_thresh=0.0, stop_thresh=0.0)
    cams = torch.from_numpy(np.ascontiguousarray(dataset.camtoworlds[comm.rank::comm.world, :3, :4])).to(sigmas.device)
    weight = torch.zeros(reso ** 3, dtype=torch.float32, device=sigmas.device)
    if cams.shape[0]:
        oops.grid_weight_render(sigmas, reso, cams, dataset.focal, dataset.focal, dataset.w, dataset.h, opts, offset,
                                invradius, grid_weight=weight, **({} if ndc is None else {"ndc": ndc}))
    return comm.all_reduce_max(weight)


def z_range_mask(mask, reso, offset, scale, z_min, z_max):
    """The reference drops grid planes with world z outside [z_min, z_max] before it builds the point list
    (:257-260, :298-301; NDC scenes); on the dense mask (x slowest, z fastest) that is clearing those planes."""
    if z_min is None and z_max is None:
        return mask
    arr = (torch.arange(reso, dtype=torch.float32, device=mask.device) + 0.5) / reso
    zz = (arr - float(offset[2])) / float(scale[2])
    keep = torch.ones(reso, dtype=torch.bool, device=mask.device)
    if z_min is not None:
        keep &= zz >= z_min
    if z_max is not None:
        keep &= zz <= z_max
    m = mask.view(reso, reso, reso)
    m &= keep.to(m.dtype).view(1, 1, reso) if m.dtype != torch.bool else keep.view(1, 1, reso)
    return mask


def step1(args, tree, model, state, dataset, comm):
    """Grid evaluation, masking and tree build (:288-352)."""
    reso = 2 ** (args.init_grid_depth + 1)
    center, radius = tree_center_radius(tree)
    sig = grid_sigma(model, state, reso, center, radius, comm)
    approx_delta = 2.0 / reso
    if args.masking_mode == "sigma":
        mask = oops.threshold_mask(sig, -np.log(1.0 - args.alpha_thresh) / approx_delta)
    elif args.masking_mode == "weight":
        weights = calculate_grid_weights(dataset, sig, reso, tree.invradius, tree.offset, args.renderer_step_size, comm,
                                         ndc=ndc_config(args, dataset))
        mask = oops.threshold_mask(weights, args.weight_thresh)
        del weights
    else:
        raise ValueError(args.masking_mode)
    del sig
    offset, scale = tree_transform(center, radius)
    mask = z_range_mask(mask, reso, offset, scale, getattr(args, "z_min", None), getattr(args, "z_max", None))
    tree.refine_from_mask(mask)
    if tree.max_depth != args.init_grid_depth:
        raise RuntimeError(f"empty mask: the tree has depth {tree.max_depth}, expected {args.init_grid_depth} "
                           "(lower --weight_thresh / --alpha_thresh or check the bounding box)")
    return mask


def step2(args, tree, model, state, comm, seed=0):
    """3-D antialiasing (:355-394, SH formats): every deepest-level cell gets the mean of the network output
    at `samples_per_cell` uniform points inside it.  Nodes are sharded over the ranks and all-gathered."""
    S = args.samples_per_cell
    _, total = tree.max_depth_nodes()
    per = (total + comm.world - 1) // comm.world
    a, b = min(comm.rank * per, total), min((comm.rank + 1) * per, total)
    chunk_nodes = max(args.chunk // (8 * S), 1) * 64
    block = torch.zeros(per * 8, tree.data_dim, dtype=torch.float32, device=tree.device)
    for n0 in range(a, b, chunk_nodes):
        cnt = min(chunk_nodes, b - n0)
        pts = tree.sample_max_depth_cells(S, first=n0, count=cnt, seed=seed)
        rgb, sigma = model.eval_points_raw(state, pts.view(-1, 3))
        ops.mean_over_samples(model.cfg, rgb, sigma, S, out=block[(n0 - a) * 8:(n0 - a + cnt) * 8])
    if comm.is_dist:
        block = comm.all_gather_cat(block)
    tree.max_depth_data().copy_(block[: total * 8])


def projection_chunk_points(n_dirs, budget_bytes=1 << 30, samples_per_cell=8):
    """Points per call of the fused projection: as many as fit `budget_bytes` of its workspace (the saved trunk activations,
    about 9 KB per point; the directions' share does not grow with the points), in whole groups of 64 nodes' samples.  The
    reference's `chunk // (S * R // 10)` (:363) bounds its [points x directions x 283] tensors, which do not exist here."""
    base = ops.vd_project_workspace_bytes(0, n_dirs)
    per_point = (ops.vd_project_workspace_bytes(4096, n_dirs) - base) / 4095.0
    group = 64 * 8 * samples_per_cell
    return max(int((budget_bytes - base) / per_point) // group, 1) * group


SAMPLE_GROUP = 64


def sample_cells_by_group(tree, S, n0, cnt, total, seed):
    """The sample points of nodes [n0, n0 + cnt) drawn per aligned group of 64 nodes (N3Tree.sample_max_depth_cells seeds a
    draw by its first node): a node's points then depend on the node alone, not on the chunk or the rank it is evaluated in."""
    parts = []
    for g0 in range(n0 // SAMPLE_GROUP * SAMPLE_GROUP, n0 + cnt, SAMPLE_GROUP):
        pts = tree.sample_max_depth_cells(S, first=g0, count=min(SAMPLE_GROUP, total - g0), seed=seed)
        lo, hi = max(n0, g0) - g0, min(n0 + cnt, g0 + SAMPLE_GROUP) - g0
        parts.append(pts.view(-1, 8 * S, 3)[lo:hi])
    return torch.cat(parts).reshape(-1, S, 3)


def step2_projection(args, tree, model, state, comm, dirs, seed=0, record=None):
    """Step 2 for a view-dependent NeRF (:362-375 with project_nerf_to_sh :217-241): the S samples of every deepest-level cell
    go through the fused SH projection under ONE direction set `dirs` for the whole run (the reference draws one per chunk),
    then the mean over the samples.  --chunk caps the points per call (above the workspace-derived size it has no effect); no
    result depends on it.  record: a dict that receives the sample points per node range (tests)."""
    S = args.samples_per_cell
    _, total = tree.max_depth_nodes()
    per = (total + comm.world - 1) // comm.world
    a, b = min(comm.rank * per, total), min((comm.rank + 1) * per, total)
    pts_per_call = min(projection_chunk_points(dirs.shape[0], samples_per_cell=S), max(args.chunk // (8 * S), 1) * 64 * 8 * S)
    chunk_nodes = max(pts_per_call // (8 * S), 1)
    block = torch.zeros(per * 8, tree.data_dim, dtype=torch.float32, device=tree.device)
    for n0 in range(a, b, chunk_nodes):
        cnt = min(chunk_nodes, b - n0)
        pts = sample_cells_by_group(tree, S, n0, cnt, total, seed)
        if record is not None:
            record.setdefault("points", []).append((n0, cnt, pts.view(-1, 3).detach().cpu()))
        coeffs, sigma = model.project_sh(state, pts.view(-1, 3), dirs, args.sh_deg)
        ops.mean_over_samples(ops.make_cfg(sh_deg=args.sh_deg), coeffs, sigma, S, out=block[(n0 - a) * 8:(n0 - a + cnt) * 8])
    if comm.is_dist:
        block = comm.all_gather_cat(block)
    tree.max_depth_data().copy_(block[: total * 8])


def tree_center_radius(tree):
    radius = 0.5 / tree.invradius
    center = (1.0 - 2.0 * tree.offset) * radius
    return center.tolist(), radius.tolist()


@torch.no_grad()
def eval_octree(tree, dataset, args, comm=None, want_frames=False, want_ssim=False, aux_sink=None, surface_thresh=0.5,
                max_depth=None, lod_pixels=None, lod_min_depth=0):
    """eval_octree (octree/nerf/utils.py:448-497): mean PSNR (and SSIM if asked) of the octree renders of a split;
    images are sharded over the ranks.  LPIPS needs pretrained VGG weights, which cannot be fetched here.
    aux_sink (off by default): called as aux_sink(idx, c2w, res) for every view of this rank with the dict of
    VolumeRenderer.render_persp_aux; the view is then rendered by that call (same rgb) instead of render_persp.
    An LLFF scene that is not --spherify is rendered in NDC (octree/nerf/utils.py:451-457).
    max_depth (off by default): the level the float tree is rendered at, in place (VolumeRenderer(max_depth=...)).
    lod_pixels, lod_min_depth (off by default): every sample at the depth its pixel footprint allows
    (VolumeRenderer(lod_pixels=...))."""
    comm = comm or dist.Comm()
    foot = {"lod_pixels": lod_pixels, "lod_min_depth": lod_min_depth} if lod_pixels else {}    # unset: the call of before
    r = VolumeRenderer(tree, step_size=args.renderer_step_size, ndc=ndc_config(args, dataset), max_depth=max_depth, **foot)
    acc = torch.zeros(3, dtype=torch.float64, device=tree.device)
    frames = []
    for idx in range(comm.rank, dataset.size, comm.world):
        gt = dataset.get_image(idx)["pixels"]
        if aux_sink is None:
            im = r.render_persp(torch.from_numpy(dataset.camtoworlds[idx]), width=dataset.w, height=dataset.h,
                                fx=dataset.focal, fast=not args.no_early_stop)
        else:
            res = r.render_persp_aux(torch.from_numpy(dataset.camtoworlds[idx]), width=dataset.w, height=dataset.h,
                                     fx=dataset.focal, fast=not args.no_early_stop, surface_thresh=surface_thresh)
            im = res["rgb"]
            aux_sink(idx, dataset.camtoworlds[idx], res)
        sse, _ = oops.image_mse(im, gt.contiguous(), want_grad=False)
        acc[0] += utils.compute_psnr(float(sse) / im.numel())
        acc[1] += 1
        if want_ssim:
            acc[2] += float(utils.compute_ssim(im.clamp(0.0, 1.0), gt, max_val=1.0))
        if want_frames:
            frames.append((idx, (im.clamp(0, 1) * 255).to(torch.uint8).cpu()))   # 1.9 MB per 800x800 view
    comm.all_reduce_sum(acc)
    if want_ssim:
        return float(acc[0] / acc[1]), float(acc[2] / acc[1]), frames
    return float(acc[0] / acc[1]), frames


def _floats(text, name):
    vals = [float(v) for v in str(text).split()]
    if len(vals) == 1:
        vals *= 3
    if len(vals) != 3:
        raise ValueError(f"--{name} takes one or three numbers")
    return vals


def define_flags():
    """Flag names and defaults of octree/extraction.py:43-176 and octree/nerf/utils.py:211-219."""
    p = utils.define_flags()
    a = p.add_argument
    a("--output", type=str, default="./tree.npz")
    a("--center", type=str, default="0 0 0")
    a("--radius", type=str, default="1.5")
    a("--alpha_thresh", type=float, default=0.01)
    a("--init_grid_depth", type=int, default=8)
    a("--samples_per_cell", "-S", type=int, default=8)
    a("--masking_mode", type=str, default="weight", choices=["sigma", "weight"])
    a("--weight_thresh", type=float, default=0.001)
    a("--bbox_from_data", action="store_true")
    a("--data_bbox_scale", type=float, default=1.0)
    a("--autoscale", action="store_true")
    a("--bbox_cube", action="store_true")
    a("--bbox_scale", type=float, default=1.0)
    a("--scale_alpha_thresh", type=float, default=0.01)
    a("--tree_branch_n", type=int, default=2)
    a("--eval", type=utils._bool, default=True)
    a("--max_refine_prop", type=float, default=0.5)          # defined by the reference (:86-90), read nowhere
    a("--z_min", type=float, default=None)                   # :91-100: keep only grid points with z_min <= z <= z_max
    a("--z_max", type=float, default=None)
    a("--is_jaxnerf_ckpt", type=utils._bool, nargs="?", const=True, default=False)   # :117-121; see main()
    # not a reference flag: a `*.ckpt` holding more than tensors (argparse.Namespace, numpy scalars ...) is unpickled in full, like
    # the reference's plain torch.load, only when this says so (the default reads tensors only and explains itself otherwise)
    a("--trust_ckpt_pickle", type=utils._bool, nargs="?", const=True, default=False)
    a("--projection_samples", type=int, default=10000)       # :133-137: directions of the SH projection (--use_viewdirs true)
    a("--renderer_step_size", type=float, default=1e-4)
    a("--no_early_stop", action="store_true")
    return p


load_nerf_checkpoint = families.load_nerf_checkpoint      # the name scripts and tests know it by


def main(argv=None, record_projection=False):
    """record_projection: keep the run's direction set and step-2 sample points on the returned tree (`projection_record`)."""
    args = define_flags().parse_args(argv)
    utils.update_flags(args)
    sg.apply_cli(args, argv)                 # --sg_dim K --sh_deg -1 on the command line win over the preset's sh_deg
    args._record_projection = bool(record_projection)
    check_octree_flags(args, "octree.extraction")
    comm, device, say = dist.open_cli("octree.extraction")
    family = families.select(args)
    model, state = families.restore(args, device, "extract", say=say)
    dirs = family.projection(args, device) if family.projection else None
    dataset = llff.get_dataset("train", args, device)      # `llff` is built there, every other name by the plain table
    if args.bbox_from_data:                                  # :447-451 (NSVF datasets carry bbox.txt)
        bbox = getattr(dataset, "bbox", None)
        if bbox is None:
            raise ValueError("--bbox_from_data needs a dataset with bbox.txt (NSVF format)")
        center = ((bbox[:3] + bbox[3:6]) * 0.5).tolist()
        radius = ((bbox[3:6] - bbox[:3]) * 0.5 * args.data_bbox_scale).tolist()
        say("Bounding box from data: c", center, "r", radius, flush=True)
    else:
        center, radius = _floats(args.center, "center"), _floats(args.radius, "radius")
    if args.autoscale:
        say("* Step 0: Auto scale", flush=True)
        center, radius = auto_scale(model, state, center, radius, args.init_grid_depth, args.scale_alpha_thresh, comm,
                                    args.z_min, args.z_max)
        say("Autoscale result center", center, "radius", radius, flush=True)
    radius = [r * args.bbox_scale for r in radius]
    if args.bbox_cube:
        radius = [max(radius)] * 3
    data_format, basis_dim, extra_data = family.tree(args, state)
    data_dim = 1 + args.num_rgb_channels * basis_dim
    say("data dim is", data_dim, flush=True)
    tree = N3Tree(N=args.tree_branch_n, data_dim=data_dim, init_refine=0, depth_limit=args.init_grid_depth,
                  radius=radius, center=center, data_format=data_format, extra_data=extra_data, map_location=device)
    reso = 2 ** (args.init_grid_depth + 1)
    say("* Step 1: Grid eval", reso, flush=True)
    torch.cuda.synchronize(); comm.barrier(); t0 = time.time()
    mask = step1(args, tree, model, state, dataset, comm)
    torch.cuda.synchronize(); comm.barrier(); t1 = time.time()
    say(f"  {int(mask.sum())} / {reso ** 3} voxels kept ({args.masking_mode} mask); step 1 took {t1 - t0:.2f} s", flush=True)
    say(tree, flush=True)
    say("* Step 2: AA", args.samples_per_cell, flush=True)
    if dirs is not None:
        say(f"  SH projection: {dirs.shape[0]} directions, one set for the run", flush=True)
        record = {"dirs": dirs.detach().cpu()} if getattr(args, "_record_projection", False) else None
        step2_projection(args, tree, model, state, comm, dirs, seed=args.seed, record=record)
        tree.projection_record = record
    else:
        step2(args, tree, model, state, comm, seed=args.seed)
    tree.relu_sigma_()
    tree.shrink_to_fit()
    torch.cuda.synchronize(); comm.barrier(); t2 = time.time()
    say(f"  step 2 took {t2 - t1:.2f} s", flush=True)
    say(tree, flush=True)
    if comm.rank == 0:
        base = os.path.dirname(args.output)
        if base:
            os.makedirs(base, exist_ok=True)
        print("* Saving", args.output, flush=True)
        tree.save(args.output, compress=False)
    if args.eval:
        test = llff.get_dataset("test", args, device)
        say("* Evaluation (before fine tune)", flush=True)
        psnr, _ = eval_octree(tree, test, args, comm)
        say("Average PSNR", psnr, flush=True)
    comm.shutdown()
    return tree


if __name__ == "__main__":
    main(sys.argv[1:])
