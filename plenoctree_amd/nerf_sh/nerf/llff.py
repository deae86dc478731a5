"""Forward-facing captures (LLFF format) for the NeRF-SH trainer and renderers: the loader of the reference's `LLFF` class
(nerf_sh/nerf/datasets.py:235-489) and its rays in normalised device coordinates (`convert_to_ndc`, :40-60).

On disk: `poses_bounds.npy` ([n, 17]: a 3 x 5 pose block `[R | t | (h, w, f)]` in LLFF's (down, right, backwards) axis order
and the near / far depth bounds of every view) and `images[_<factor>]/` with the views as jpg / JPG / png, in the order of
the poses.  The scene is rescaled so that the nearest bound sits at 1 / 0.75, the poses are expressed in the frame of their
average, and -- unless `--spherify` -- every ray is moved to the plane z = -1 and projected, after which the whole scene in
front of that plane lies between ray depths 0 and 1 (the preset's near / far).  With `--spherify` (inward-facing 360 degree
captures) the poses are put on a unit sphere instead and the rays stay in world space.

The images are resident on the device like the other loaders'; NDC rays are computed on the device inside the launches
that feed a step (pxo_generate_rays_ndc, pxo_sample_batch_ndc).  The octree entry points (octree.extraction / optimization /
evaluation) take their dataset from `get_dataset` below as well; what they use of it is world-space -- `camtoworlds`, `focal`,
`h`, `w` and the images -- because the octree marchers convert each camera ray to NDC themselves (svox.NDCConfig; DESIGN
section 13.1).  `datasets.get_dataset` keeps refusing `llff`."""
import functools
import os

import numpy as np
import torch

from . import datasets, utils

NDC_NEAR = 1.0          # the reference calls convert_to_ndc with its default near (datasets.py:338-340)
N_PATH_VIEWS = 120      # poses of the spiral / circle a --render_path run renders (:404, :462)


def convert_to_ndc(origins, directions, focal, w, h, near=1.0):
    """Rays o + t d in front of a pinhole camera at the origin looking down -z  ->  rays in normalised device coordinates
    (datasets.py:40-60; the derivation is in the NeRF paper's appendix C).  numpy arrays or torch tensors [..., 3] of any
    float type, evaluated in that type in the reference's operation order; the device kernels do the same in float32."""
    stack = torch.stack if torch.is_tensor(origins) else np.stack
    t = -(near + origins[..., 2]) / directions[..., 2]          # to the plane z = -near
    origins = origins + t[..., None] * directions
    ox, oy, oz = origins[..., 0], origins[..., 1], origins[..., 2]
    dx, dy, dz = directions[..., 0], directions[..., 1], directions[..., 2]
    cw, ch = (2 * focal) / w, (2 * focal) / h
    o = stack([-cw * (ox / oz), -ch * (oy / oz), 1 + 2 * near / oz], -1)
    d = stack([-cw * (dx / dz - ox / oz), -ch * (dy / dz - oy / oz), -2 * near / oz], -1)
    return o, d


def _unit(x):
    return x / np.linalg.norm(x)


def _look_along(z, up, pos):
    """[3,4] camera-to-world with the given backward axis z, the up hint and the position (:377-384)."""
    z = _unit(z)
    x = _unit(np.cross(up, z))
    return np.stack([x, _unit(np.cross(z, x)), z, pos], 1)


def _average_pose(poses):
    """[3,5]: mean position, summed backward and up axes, hwf of the first pose (:368-375)."""
    pose = _look_along(_unit(poses[:, :3, 2].sum(0)), poses[:, :3, 1].sum(0), poses[:, :3, 3].mean(0))
    return np.concatenate([pose, poses[0, :3, -1:]], 1)


def _homogeneous(p34):
    """[n,3,4] -> [n,4,4] (float64)."""
    last = np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (p34.shape[0], 1, 4))
    return np.concatenate([p34, last], 1)


def _recenter_poses(poses):
    """The poses in the frame of their average pose (:355-366); the hwf column stays."""
    frame = _homogeneous(_average_pose(poses)[None, :3, :4])[0]
    out = poses.copy()
    out[:, :3, :4] = (np.linalg.inv(frame) @ _homogeneous(poses[:, :3, :4]))[:, :3, :4]
    return out


def _generate_spiral_poses(poses, bds):
    """120 poses [120,3,4] float32 on two turns of a spiral around the average pose, all looking at a point at the scene's
    "focus depth" (:390-423)."""
    avg = _average_pose(poses)
    up = _unit(poses[:, :3, 1].sum(0))
    # the depth the path looks at: the harmonic mix (1/4 near, 3/4 far) of just inside the nearest and far beyond the farthest bound
    focus = 1.0 / (0.25 / (0.9 * bds.min()) + 0.75 / (5.0 * bds.max()))
    rads = np.array(list(np.percentile(np.abs(poses[:, :3, 3]), 90, 0)) + [1.0])
    target = np.dot(avg[:3, :4], np.array([0, 0, -focus, 1.0]))
    out = []
    for theta in np.linspace(0.0, 2.0 * np.pi * 2, N_PATH_VIEWS + 1)[:-1]:
        pos = np.dot(avg[:3, :4], np.array([np.cos(theta), -np.sin(theta), -np.sin(theta * 0.5), 1.0]) * rads)
        out.append(_look_along(pos - target, up, pos))
    return np.array(out).astype(np.float32)


def _generate_spherical_poses(poses, bds):
    """--spherify (:425-489): the frame is moved to the point nearest to all optical axes with the mean camera offset as
    +z, the scene (poses and, in place, `bds`) scaled so that the cameras sit at RMS distance 1.  Returns (the poses
    [n,3,5] float64, the 120 poses [120,3,4] of a circle at the cameras' mean height)."""
    axes, centers = poses[:, :3, 2:3], poses[:, :3, 3:4]
    # least-squares point nearest to the lines centers + s * axes
    proj = np.eye(3) - axes * np.transpose(axes, [0, 2, 1])
    center = np.squeeze(-np.linalg.inv((np.transpose(proj, [0, 2, 1]) @ proj).mean(0)) @ (-proj @ centers).mean(0))
    z = _unit((poses[:, :3, 3] - center).mean(0))
    x = _unit(np.cross([0.1, 0.2, 0.3], z))
    frame = np.stack([x, _unit(np.cross(z, x)), z, center], 1)
    reset = np.linalg.inv(_homogeneous(frame[None])) @ _homogeneous(poses[:, :3, :4])
    scale = 1.0 / np.sqrt((reset[:, :3, 3] ** 2).sum(-1).mean())        # the cameras' RMS distance from the centre -> 1
    reset[:, :3, 3] *= scale
    bds *= scale
    height = np.mean(reset[:, :3, 3], 0)[2]
    circle = np.sqrt(1.0 - height ** 2)                                   # radius of the unit sphere's circle at that height
    path = []
    for th in np.linspace(0.0, 2.0 * np.pi, N_PATH_VIEWS):
        pos = np.array([circle * np.cos(th), circle * np.sin(th), height])
        back = _unit(pos)
        right = _unit(np.cross(back, np.array([0, 0, -1.0])))
        path.append(np.stack([right, _unit(np.cross(back, right)), back, pos], 1))
    hwf = poses[0, :3, -1:]
    reset = np.concatenate([reset[:, :3, :4], np.broadcast_to(hwf, reset[:, :3, -1:].shape)], -1)
    return reset, np.stack(path, 0)


class _NdcFeeder:
    """A feeder whose rays are NDC rays: the base sampler's calls (generate_rays, generate_rays_multi, sample_batch) go to the
    wrapped feeder's *_ndc methods; everything else, and a method the wrapped feeder lacks, is the wrapped feeder's."""
    _NDC = {"generate_rays": "generate_rays_ndc", "generate_rays_multi": "generate_rays_multi_ndc",
            "sample_batch": "sample_batch_ndc"}

    def __init__(self, feeder, ndc_near):
        self._feeder, self._ndc_near = feeder, ndc_near

    def __getattr__(self, name):
        target = getattr(self._feeder, self._NDC.get(name, name))
        return functools.partial(target, ndc_near=self._ndc_near) if name in self._NDC else target


class LLFF(datasets.Dataset):
    """Forward-facing scene (reference nerf_sh/nerf/datasets.py:235-353).  `test` holds every `llffhold`-th view, `train` the
    rest.  With `--render_path` the test split iterates the 120 `render_poses` and its examples carry rays only."""

    def _load(self, args):
        from PIL import Image
        root = os.path.expanduser(args.data_dir)
        factor = args.factor if args.factor > 0 else 1
        imgdir = os.path.join(root, "images" + (f"_{args.factor}" if args.factor > 0 else ""))
        if not os.path.isdir(imgdir):
            raise ValueError(f"LLFF {root}: no image folder {imgdir} (factor {args.factor})")
        names = [f for f in sorted(os.listdir(imgdir)) if f.endswith(("JPG", "jpg", "png"))]
        images = np.stack([np.asarray(Image.open(os.path.join(imgdir, f)), dtype=np.float32) / 255.0 for f in names], 0)
        poses_arr = np.load(os.path.join(root, "poses_bounds.npy"))
        poses = poses_arr[:, :-2].reshape(-1, 3, 5).astype(np.float64)
        bds = poses_arr[:, -2:].astype(np.float32)
        if poses.shape[0] != images.shape[0]:
            raise RuntimeError(f"LLFF {root}: {images.shape[0]} images in {imgdir} but {poses.shape[0]} poses")
        # hwf column: the size of the images that were loaded, the focal length of the full-size capture / factor (:276-278)
        poses[:, 0, 4], poses[:, 1, 4] = images.shape[1], images.shape[2]
        poses[:, 2, 4] = poses[:, 2, 4] * 1.0 / factor
        # LLFF's (down, right, backwards) columns -> (right, up, backwards) (:280-284)
        poses = np.concatenate([poses[:, :, 1:2], -poses[:, :, 0:1], poses[:, :, 2:]], 2).astype(np.float32)
        scale = 1.0 / (bds.min() * 0.75)               # the nearest depth bound at 1 / 0.75 (:288-291)
        poses[:, :3, 3] *= scale
        bds *= scale
        poses = _recenter_poses(poses)
        self.spherify = bool(args.spherify)
        self.render_poses = None
        if self.spherify:
            poses, path = _generate_spherical_poses(poses, bds)
            if self.split == "test":
                self.render_poses = path
        elif self.split == "test":
            self.render_poses = _generate_spiral_poses(poses, bds)
        held = np.arange(images.shape[0])[::args.llffhold]
        keep = held if self.split != "train" else np.array([i for i in range(images.shape[0]) if i not in held])
        images, poses = images[keep], poses[keep]
        self.indices = keep
        self.camtoworlds = np.ascontiguousarray(poses[:, :3, :4])
        self.focal = float(poses[0, -1, -1])
        self.h, self.w = images.shape[1:3]
        self.render_path = bool(args.render_path)
        if self.render_path:
            if self.render_poses is None:
                raise ValueError("render_path is an option of the test split (the train split has no render_poses)")
            self.n_examples = self.render_poses.shape[0]
            self._render_c2w_dev = torch.from_numpy(self.render_poses.astype(np.float32)).to(self.device)
        else:
            self.n_examples = images.shape[0]
        self.images = torch.from_numpy(np.ascontiguousarray(images[..., :3]).reshape(images.shape[0], -1, 3)).to(self.device)
        self.camtoworlds = self.camtoworlds.astype(np.float32)
        if not self.spherify:
            self.feeder = _NdcFeeder(self.feeder, NDC_NEAR)

    def _pixels_for(self, image_index, ray_indices, rays):
        return self.images[image_index][ray_indices].contiguous()

    def get_image(self, idx):
        if not self.render_path:
            return super().get_image(idx)
        rays = utils.Rays(*self.feeder.generate_rays(self._render_c2w_dev[idx], self.w, self.h, self.focal,
                                                     torch.arange(self.h * self.w, device=self.device)))
        return {"rays": utils.namedtuple_map(lambda r: r.reshape(self.h, self.w, 3), rays)}


def get_dataset(split, args, device, batch_size=None, seed=20201473, shard=None):
    """datasets.get_dataset for the NeRF entry points: `llff` is built here, every other name goes to the plain table."""
    if args.dataset == "llff":
        return LLFF(split, args, device, batch_size=batch_size, seed=seed, shard=shard)
    return datasets.get_dataset(split, args, device, batch_size=batch_size, seed=seed, shard=shard)
