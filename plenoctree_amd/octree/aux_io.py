"""Writers for the extra outputs of the octree renderer (VolumeRenderer.render_persp_aux): cut-out images, depth archives
and point clouds.  Everything here takes plain numpy arrays and runs on the host, so it is tested without a GPU.
"""
import numpy as np


def rgba_image(rgb, alpha):
    """uint8 [H,W,4]: the colours as the image writers of the drivers quantise them (clamp to [0,1], x255, truncate) and
    round(255 alpha) as the fourth channel."""
    rgb = np.asarray(rgb, np.float32)
    alpha = np.asarray(alpha, np.float32)
    out = np.empty(rgb.shape[:2] + (4,), np.uint8)
    out[..., :3] = (np.clip(rgb, 0.0, 1.0) * np.float32(255)).astype(np.uint8)
    out[..., 3] = np.rint(np.clip(alpha, 0.0, 1.0) * np.float32(255)).astype(np.uint8)
    return out


def write_rgba_png(path, rgb, alpha):
    from PIL import Image
    Image.fromarray(rgba_image(rgb, alpha), "RGBA").save(path)


def write_depth_npz(path, depth, surface, alpha):
    """float32 arrays `depth` (sum of weight x distance, not divided by alpha), `surface` (+inf where the transmittance never
    falls to the threshold) and `alpha`."""
    np.savez_compressed(path, depth=np.asarray(depth, np.float32), surface=np.asarray(surface, np.float32),
                        alpha=np.asarray(alpha, np.float32))


def camera_rays(c2w, width, height, fx, fy=None):
    """(origin [3], unit dirs [H,W,3]) of the renderer's pinhole camera: pixel centres at integer coordinates, -z forward."""
    c2w = np.asarray(c2w, np.float32)
    fy = fx if fy is None else fy
    x = (np.arange(width, dtype=np.float32) - np.float32(0.5 * width)) / np.float32(fx)
    y = -(np.arange(height, dtype=np.float32) - np.float32(0.5 * height)) / np.float32(fy)
    x, y = np.meshgrid(x, y)                                       # [H,W]
    z = np.sqrt(x * x + y * y + np.float32(1.0))
    d_cam = np.stack([x / z, y / z, -1.0 / z], -1).astype(np.float32)
    return c2w[:3, 3].copy(), d_cam @ c2w[:3, :3].T


def surface_points(c2w, fx, surface, rgb, stride=4, fy=None):
    """Back-projects every `stride`-th pixel (both axes, starting at pixel 0) whose `surface` distance is finite:
    (xyz float32 [n,3] = origin + surface * dir, colours uint8 [n,3])."""
    surface = np.asarray(surface, np.float32)
    height, width = surface.shape
    origin, dirs = camera_rays(c2w, width, height, fx, fy)
    sub = (slice(None, None, int(stride)), slice(None, None, int(stride)))
    s, d, col = surface[sub], dirs[sub], np.asarray(rgb, np.float32)[sub]
    keep = np.isfinite(s)
    xyz = origin[None, :] + s[keep][:, None] * d[keep]
    return xyz.astype(np.float32), (np.clip(col[keep], 0.0, 1.0) * np.float32(255)).astype(np.uint8)


PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def write_ply(path, xyz, colors):
    """Binary little-endian PLY of vertices `x y z red green blue`."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    if xyz.shape[0] != colors.shape[0]:
        raise ValueError(f"{xyz.shape[0]} points but {colors.shape[0]} colours")
    v = np.empty(xyz.shape[0], PLY_VERTEX)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = colors[:, 0], colors[:, 1], colors[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {xyz.shape[0]}\n"
              "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())

