"""What the footprint tests (tests/test_footprint_cpu.py, tests/test_gpu_footprint.py) add to the twin of the footprint render,
which is oracle/octree_oracle.py's `march(..., foot=(cone, min_depth))` and `composite`: `reuse_counts` replays the kernel's
integer path reuse over the twin's samples and counts the situations the tests must not miss.  TEST INFRASTRUCTURE."""
import numpy as np

from oracle import octree_oracle as T

f32 = np.float32
BITS = T.MAX_DEPTH + 1                           # bits per axis of the kernel's quantised position


def reuse_counts(marched):
    """Replays Marcher::find's integer path reuse over one ray's samples: (samples, cap-stopped samples -- the descent ended
    at a cell that has a child --, clamp cases -- min(common, last_depth) > cap, where resuming from the previous path
    without the clamp by cap would start below the cap --, whether the cap takes more than one value on the ray)."""
    if marched is None:
        return 0, 0, 0, False
    clamp = 0
    prev, last_depth = None, 0
    for pos, depth, cap in zip(marched.pos, marched.depth.tolist(), marched.cap.tolist()):
        q = tuple(int(f32(c * f32(1 << BITS))) for c in pos)         # exact: a power of two; >= 0, so int() is the floor
        if prev is not None:
            diff = (q[0] ^ prev[0]) | (q[1] ^ prev[1]) | (q[2] ^ prev[2])
            common = BITS - diff.bit_length()                          # leading bit-levels shared
            clamp += min(common, last_depth) > cap
        prev, last_depth = q, depth
    return len(marched), int(marched.has_child.sum()), clamp, len(set(marched.cap.tolist())) > 1


def case_counts(rays_marched):
    """The per-case figures: dict(samples, cap_stopped, clamp_cases, rays_changing_cap) over the marches of a ray set."""
    tot = np.zeros(4, np.int64)
    for m in rays_marched:
        tot += np.array(reuse_counts(m), np.int64)
    return dict(samples=int(tot[0]), cap_stopped=int(tot[1]), clamp_cases=int(tot[2]), rays_changing_cap=int(tot[3]))
