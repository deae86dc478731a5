"""Turntable renderer of a trained NeRF-SH (reference: nerf_sh/gen_video.py): poses on a circle at the given
elevation -> rays -> deterministic render -> PNG frames under <train_dir>/video/e<elev>/frames (+ an animated GIF;
the reference writes an mp4 through imageio, which is not installed here).

    python -m plenoctree_amd.nerf_sh.gen_video --train_dir D --config blender --num_views 40 [--write_poses poses.txt]

A forward-facing scene has no turntable: its model lives in normalised device coordinates, inside the frustum of the capture.
`--config llff --data_dir DATA --render_path true` renders the scene's own camera path instead (the 120-pose spiral of the LLFF
loader, or the circle of `--spherify`), at the size of the loaded images, to <train_dir>/video/path/frames.
"""
import os
import sys

import numpy as np
import torch

from .. import dist, ops
from .nerf import families, llff, occupancy, sg, utils, viewdirs


def define_flags():
    """nerf_sh/gen_video.py:52-105."""
    p = viewdirs.add_checkpoint_flags(utils.define_flags())
    a = p.add_argument
    a("--elevation", type=float, default=-30.0)
    a("--num_views", type=int, default=40)
    a("--height", type=int, default=800)
    a("--width", type=int, default=800)
    a("--camera_angle_x", "-A", type=float, default=0.7)
    a("--intrin", type=str, default=None)
    a("--radius", type=float, default=4.0)
    a("--fps", type=int, default=20)
    a("--up_axis", type=int, default=1)
    a("--write_poses", type=str, default=None)
    return p


def render_poses(args):
    """:113-120: num_views poses on a circle, angles linspace(-180, 180, n+1)[:-1]."""
    return np.stack([utils.pose_spherical(angle, args.elevation, args.radius, args.up_axis - 1)
                     for angle in np.linspace(-180, 180, args.num_views + 1)[:-1]], 0)


def main(argv=None):
    args = define_flags().parse_args(argv)
    utils.update_flags(args)
    sg.apply_cli(args, argv)                     # --sg_dim K --sh_deg -1 on the command line win over the preset's sh_deg
    comm, device, say = dist.open_cli("nerf_sh.gen_video")
    families.check(args, "render", require_data=False, world_size=comm.world)
    path_ds = None
    if args.dataset == "llff":
        if not args.render_path or args.data_dir is None:
            raise ValueError("gen_video on an llff scene renders the scene's camera path: pass --render_path true and --data_dir "
                             "(turntable poses lie outside the frustum an NDC model is trained in)")
        say("* Loading the camera path", flush=True)
        path_ds = llff.get_dataset("test", args, device)
        poses, args.num_views = path_ds.render_poses, path_ds.size
        args.height, args.width, focal = path_ds.h, path_ds.w, path_ds.focal
    else:
        say("* Generating poses", flush=True)
        poses = render_poses(args)
        focal = 0.5 * args.width / np.tan(0.5 * args.camera_angle_x)
        if args.intrin is not None:
            K = np.loadtxt(args.intrin)
            focal = (K[0, 0] + K[1, 1]) * 0.5
    if args.write_poses and comm.rank == 0:
        np.savetxt(args.write_poses, poses.reshape(-1, 4))
        print("Saved poses to", args.write_poses, flush=True)
    say("* Creating model", flush=True)
    model, state = families.restore(args, device, "render", say=say, require_data=False)
    video_dir = os.path.join(args.train_dir, "video", "path" if path_ds is not None else "e{:03}".format(int(-args.elevation * 10)))
    frames_dir = os.path.join(video_dir, "frames")
    say(" Saving to", video_dir, flush=True)
    if comm.rank == 0:
        os.makedirs(frames_dir, exist_ok=True)
    c2w = None if path_ds is not None else torch.from_numpy(np.ascontiguousarray(poses[:, :3, :4])).to(device)
    frames = []
    render_fn, live = occupancy.render_fn(args, model, state, comm, say)      # without --occupancy_reso: model.apply, as ever
    for i in range(args.num_views):
        say(f"** View {i + 1}/{args.num_views} = {i / args.num_views * 100}%", flush=True)
        if path_ds is not None:
            rays = path_ds.get_image(i)["rays"]
        else:
            rays = utils.Rays(*[r.reshape(args.height, args.width, 3)
                                for r in ops.generate_rays(c2w[i], args.width, args.height, focal)])
        rgb, disp, acc = utils.render_image(render_fn, rays,
                                            normalize_disp=(args.dataset == "llff"), chunk=args.chunk,     # gen_video.py:158
                                            world_size=comm.world, rank=comm.rank, gather=comm.all_gather_cat)
        if live is not None:
            say(live.line(), flush=True)
            live.reset()
        if comm.rank == 0:
            utils.save_img(rgb, os.path.join(frames_dir, f"{i:04}.png"))
            frames.append((np.clip(rgb.cpu().numpy(), 0.0, 1.0) * 255).astype(np.uint8))
    if comm.rank == 0 and frames:
        from PIL import Image
        vid_path = os.path.join(video_dir, "video.gif")
        print("* Writing", vid_path, flush=True)
        ims = [Image.fromarray(f) for f in frames]
        ims[0].save(vid_path, save_all=True, append_images=ims[1:], duration=int(1000 / max(args.fps, 1)), loop=0)
        print("* Done", flush=True)
    comm.shutdown()
    return frames


if __name__ == "__main__":
    main(sys.argv[1:])
