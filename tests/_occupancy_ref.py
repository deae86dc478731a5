"""numpy restatements of the occupancy-grid entry points (include/plenoctree_hip.h, "occupancy grid"), written from the header's
definitions: tests/test_occupancy.py checks them against hand-made cases, tests/test_gpu_occupancy.py holds the kernels to them
bit for bit."""
import itertools

import numpy as np


def words(reso):
    return (reso ** 3 + 31) // 32


def bits_from_mask(mask):
    """bool [reso^3] (x slowest) -> int32 words: bit i in word i >> 5 at position i & 31, the last word's unused bits zero."""
    flat = np.asarray(mask, bool).reshape(-1)
    pad = np.zeros(((flat.size + 31) // 32) * 32, bool)
    pad[:flat.size] = flat
    w = (pad.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1)
    return w.astype(np.uint32).view(np.int32)


def mask_from_bits(bits, reso):
    w = np.asarray(bits).view(np.uint32).astype(np.uint64)
    flat = ((w[:, None] >> np.arange(32, dtype=np.uint64)) & 1).astype(bool).reshape(-1)
    return flat[:reso ** 3]


def pack_mask(sigma, reso, thresh, dilate):
    """bool [reso,reso,reso]: cell c is occupied iff a cell c' of the grid with Chebyshev distance <= dilate has
    !(sigma[c'] <= thresh) -- strictly above, or NaN."""
    s = np.asarray(sigma, np.float32).reshape(reso, reso, reso)
    with np.errstate(invalid="ignore"):
        above = ~(s <= np.float32(thresh))
    if not dilate:
        return above
    out = np.zeros_like(above)
    r = range(-dilate, dilate + 1)
    for dx, dy, dz in itertools.product(r, r, r):
        # out[x, y, z] |= above[x + dx, y + dy, z + dz] wherever that neighbour lies inside the grid
        xs = slice(max(0, -dx), reso - max(0, dx)); xn = slice(max(0, dx), reso - max(0, -dx))
        ys = slice(max(0, -dy), reso - max(0, dy)); yn = slice(max(0, dy), reso - max(0, -dy))
        zs = slice(max(0, -dz), reso - max(0, dz)); zn = slice(max(0, dz), reso - max(0, -dz))
        out[xs, ys, zs] |= above[xn, yn, zn]
    return out


def pack(sigma, reso, thresh, dilate):
    return bits_from_mask(pack_mask(sigma, reso, thresh, dilate))


def live_mask(bits, reso, offset, scale, outside_live, pts):
    """The point -> cell -> live rule in float64 (the tests choose points whose float32 t = fmaf(p, scale, offset) is exact)."""
    p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    occ = mask_from_bits(bits, reso)
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p * np.asarray(scale, np.float64) + np.asarray(offset, np.float64)
        inside = ((t >= 0.0) & (t < 1.0)).all(axis=1) & finite
        cell = np.minimum(np.where(inside[:, None], t * reso, 0.0).astype(np.int64), reso - 1)
    idx = (cell[:, 0] * reso + cell[:, 1]) * reso + cell[:, 2]
    return np.where(~finite, True, np.where(inside, occ[idx], bool(outside_live)))


def cull(bits, reso, offset, scale, outside_live, pts):
    """(pts_live [n_live,3], slot int32 [M], n_live)."""
    p = np.asarray(pts, np.float32).reshape(-1, 3)
    live = live_mask(bits, reso, offset, scale, outside_live, p)
    slot = np.where(live, np.cumsum(live) - 1, -1).astype(np.int32)
    return p[live], slot, int(live.sum())


def expand(rgb_live, sigma_live, slot, C):
    slot = np.asarray(slot)
    rgb = np.zeros((slot.size, C), np.float32)
    sigma = np.zeros(slot.size, np.float32)
    keep = slot >= 0
    rgb[keep] = np.asarray(rgb_live, np.float32).reshape(-1, C)[slot[keep]]
    sigma[keep] = np.asarray(sigma_live, np.float32).reshape(-1)[slot[keep]]
    return rgb, sigma
