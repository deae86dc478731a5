"""Synthetic compressed trees in the file format of octree/compression.py, shared by tests/test_quantized_tree_cpu.py
and tests/test_gpu_quantized_tree.py.

Everything here is oracle/octree_oracle.py plus numpy.  A case is a small tree from `build_from_mask` (leaves at every
depth 1..depth: the cells the mask leaves unrefined stay behind as coarse leaves), random float16 palettes, random
indices, float16 sigma with the non-positive share set to 0 (compression's `sigma_thresh`), and optionally retained
planes.  Magnitudes are those of tests/_octree_cases.py `fill_data` (coefficients 0.7 * randn, sigma (u - 0.35) * scale *
2^(depth + 1) per leaf depth), rounded to float16; the scale is 0.8, so that the finest leaves of a depth-3 tree reach the
sigma range of tests/test_gpu_octree.py (12) and the early-stopping preset does stop some rays.
"""
import functools

import numpy as np

from oracle import octree_oracle as T
from _octree_cases import leaf_depths

f32, f16 = np.float32, np.float16
CENTER, RADIUS = (0.1, 0.0, -0.2), (1.4, 1.5, 1.3)
SIGMA_SCALE = 0.8

# (basis_dim, retain, bits): every SH format with and without retained planes (odd and even counts of quantised planes),
# two-colour, 8-bit and full 16-bit palettes
CASES = ((1, 0, 8), (4, 0, 1), (4, 1, 8), (9, 0, 16), (9, 1, 8), (16, 0, 8), (16, 4, 16), (25, 0, 8), (25, 1, 1))


class QuantCase:
    """tree: oracle Tree holding the dequantised float32 data.  The file arrays are attributes named like the npz keys."""

    def files(self):
        z = dict(data_dim=np.int64(3 * self.K + 1), child=self.tree.child, invradius3=self.tree.invradius, offset=self.tree.offset,
                 data_format=f"SH{self.K}", quant_colors=self.quant_colors, quant_map=self.quant_map, sigma=self.sigma)
        if self.retain:
            z["data_retained"] = self.data_retained
        return z

    def save(self, path, **override):
        z = self.files()
        z.update(override)
        np.savez(path, **{k: v for k, v in z.items() if v is not None})
        return path

    def dequantized(self):
        """float32 [n,2,2,2,3K+1]: a restatement of the format (channel-major coefficients, sigma last)."""
        K, r = self.K, self.retain
        n = self.tree.n_internal
        data = np.zeros((n, 2, 2, 2, 3 * K + 1), f32)
        for c in range(3):
            for b in range(K):
                if b < r:
                    data[..., c * K + b] = self.data_retained[b][..., c].astype(f32)
                else:
                    data[..., c * K + b] = self.quant_colors[b - r][self.quant_map[b - r].astype(np.int64), c].astype(f32)
        data[..., -1] = self.sigma.astype(f32)
        return data

    def refresh(self):
        self.tree.data[:] = self.dequantized()
        return self


def make_case(K, retain, bits, depth=3, seed=0, p=0.04):
    rs = np.random.RandomState(1000 * K + 10 * retain + bits + seed)
    reso = 2 ** (depth + 1)
    tree = T.build_from_mask(rs.rand(reso, reso, reso) < p, depth, 3 * K + 1, CENTER, RADIUS)
    n = tree.n_internal
    c = QuantCase()
    c.K, c.retain, c.bits, c.tree = K, retain, bits, tree
    Kq, P = K - retain, 1 << bits
    c.quant_colors = (rs.randn(Kq, P, 3) * 0.7).astype(f16)
    c.quant_map = rs.randint(0, P, size=(Kq, n, 2, 2, 2)).astype(np.uint16)
    if bits == 16:                      # a quarter of the cells take the last entry of palette 0 (half of the rest is >= 32768)
        c.quant_map[0][rs.rand(n, 2, 2, 2) < 0.25] = 65535
    sigma = ((rs.rand(n, 2, 2, 2) - 0.35) * SIGMA_SCALE * 2.0 ** (leaf_depths(tree) + 1)).astype(f16)
    sigma[sigma <= 0] = 0
    c.sigma = sigma
    c.data_retained = (rs.randn(retain, n, 2, 2, 2, 3) * 0.7).astype(f16) if retain else None
    return c.refresh()


@functools.lru_cache(maxsize=None)
def case(K, retain, bits):
    return make_case(K, retain, bits)


def layout_bytes(n, K, retain, bits):
    """The documented device layout (include/plenoctree_octree.h, PxoQuantLayout): section sizes in bytes, each rounded
    up to 256, in the order idx, palette, sigma, retained."""
    cells, Kq = n * 8, K - retain
    stride = (Kq + 3) // 4 * 4
    up = lambda v: (v + 255) // 256 * 256
    return [up(cells * stride * 2), up(Kq * (1 << bits) * 8), up(cells * 4), up(cells * retain * 4 * 2)], stride
