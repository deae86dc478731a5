"""numpy restatements for the meshing tests (tests/test_mesh_cpu.py, tests/test_gpu_mesh.py): the integer-bit descent of
pxo_tree_sigma_grid, the inside end point of every marching-cubes vertex, and small mesh-topology helpers.  No GPU."""
import numpy as np

MAX_DEPTH = 10                       # PXO_TREE_MAX_DEPTH


def sigma_grid(child, data, depth, pad):
    """(sigma float32 [S,S,S], packed int64 [S,S,S]), S = 2^depth + 2 pad, of the tree (child [n,2,2,2], data [n,2,2,2,D]).
    The centre of cell i is (i + 1/2) / 2^depth: binary digits = the bits of i, a one, then zeros; the descent takes the child
    cell from those digits."""
    g = 1 << depth
    i, j, k = (a.reshape(-1) for a in np.meshgrid(*[np.arange(g, dtype=np.int64)] * 3, indexing="ij"))
    flat = np.asarray(child).reshape(-1).astype(np.int64)
    node = np.zeros(i.size, np.int64)
    leaf = np.full(i.size, -1, np.int64)
    active = np.ones(i.size, bool)
    for lvl in range(MAX_DEPTH + 2):
        b = depth - 1 - lvl
        if b >= 0:
            cell = (((i >> b) & 1) * 2 + ((j >> b) & 1)) * 2 + ((k >> b) & 1)
        else:
            cell = np.full(i.size, 7 if b == -1 else 0, np.int64)
        at = node * 8 + cell
        skip = flat[np.where(active, at, 0)]
        done = active & (skip == 0)
        leaf[done] = at[done]
        active &= skip != 0
        node = np.where(active, node + skip, node)
        if not active.any():
            break
    assert not active.any(), "descent did not reach a leaf"
    sig = np.asarray(data).reshape(-1, np.asarray(data).shape[-1])[leaf, -1].astype(np.float32)
    s = g + 2 * pad
    sigma = np.zeros((s, s, s), np.float32)
    packed = np.full((s, s, s), -1, np.int64)
    sl = (slice(pad, pad + g),) * 3
    sigma[sl] = sig.reshape(g, g, g)
    packed[sl] = leaf.reshape(g, g, g)
    return sigma, packed


def inside_index(vol, iso):
    """Per vertex of isosurface.marching_cubes(vol, iso), in its order: the linear index of the end point of the vertex's grid
    edge whose value is >= iso (float32 comparison for a float32 volume, as the host function compares)."""
    vol = np.ascontiguousarray(vol)
    inside = vol >= iso
    lin = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    out = []
    for a in range(3):
        lo = tuple(slice(0, -1) if d == a else slice(None) for d in range(3))
        hi = tuple(slice(1, None) if d == a else slice(None) for d in range(3))
        idx = np.nonzero(inside[lo] != inside[hi])
        out.append(np.where(inside[lo][idx], lin[lo][idx], lin[hi][idx]))
    return np.concatenate(out)


def edge_use(faces):
    """(undirected edge keys, how many triangles use each)."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    e.sort(1)
    return np.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1], return_counts=True)


def read_obj(path):
    """(vertices float64 [V,3], colours float64 [V,3] or None, faces int64 [T,3], 0-based) of a file written by save_obj."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if tok[0] == "v":
                v.append([float(x) for x in tok[1:]])
            elif tok[0] == "f":
                f.append([int(x) - 1 for x in tok[1:]])
            else:
                raise AssertionError(f"unexpected OBJ line {line!r}")
    v = np.asarray(v, np.float64).reshape(len(v), -1)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    assert v.shape[1] in (3, 6)
    return v[:, :3], (v[:, 3:] if v.shape[1] == 6 else None), f
