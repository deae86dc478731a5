"""Host side of the device meshing path (no GPU): the workspace formula of DESIGN.md 8.7 and its overflow refusal, what
octree.meshing refuses before it needs a GPU, its index-to-world mapping, the numpy restatement of pxo_tree_sigma_grid's
integer descent against the oracle's point query, the uploaded case table, and gen_mesh's --mc flag with its CPU fallback."""
import ctypes

import numpy as np
import pytest
import torch

import _mesh_oracle as M
import _octree_cases as C
from plenoctree_amd import _lib, build, mesh_ops
from plenoctree_amd.nerf_sh import gen_mesh, isosurface
from plenoctree_amd.octree import meshing


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.load()


def _formula(nx, ny, nz):
    """DESIGN.md 8.7, written out once more: bytes = 3 r(4N) + 2 r(N) + r(16 nb) + r(32 nt) + 256."""
    r = lambda b: (b + 255) // 256 * 256
    n = nx * ny * nz
    nb = (n + 255) // 256
    nt = (nb + 1023) // 1024
    return 3 * r(4 * n) + 2 * r(n) + r(16 * nb) + r(32 * nt) + 256


@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 3, 5), (4, 8, 8), (3, 5, 17), (65, 64, 66), (300, 300, 300), (512, 512, 512),
                                   (1024, 1024, 1024), (2047, 1024, 1024)])
def test_workspace_bytes_match_the_documented_formula(lib, shape):
    n = ctypes.c_size_t(0)
    assert lib.pxo_mc_workspace_bytes(*shape, ctypes.byref(n)) == 0
    assert n.value == _formula(*shape)
    assert mesh_ops.mc_workspace_bytes(*shape) == n.value


def test_workspace_bytes_empty_grids_and_overflow(lib):
    n = ctypes.c_size_t(7)
    for shape in ((1, 5, 5), (5, 5, 1), (0, 4, 4)):
        assert lib.pxo_mc_workspace_bytes(*shape, ctypes.byref(n)) == 0 and n.value == 0
    # 2^31 grid points: the crossing edges of one axis alone could leave the int32 id range
    for shape in ((2048, 2048, 512), (2048, 2048, 2048), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.pxo_mc_workspace_bytes(*shape, ctypes.byref(n)) == -1
        assert b"2^31" in lib.pxo_last_error()
        with pytest.raises(_lib.PxoError, match="int32"):
            mesh_ops.mc_workspace_bytes(*shape)
    assert lib.pxo_mc_workspace_bytes(-1, 4, 4, ctypes.byref(n)) == -1
    assert lib.pxo_mc_workspace_bytes(4, 4, 4, None) == -1
    # the counting and emitting entry points refuse the same grids, and emit refuses counts of 2^31, before any launch
    counts = (ctypes.c_int64 * 4)()
    assert lib.pxo_mc_count(None, 2048, 2048, 512, 1.0, None, None, 0, counts, None) == -1
    counts[:] = [2 ** 30, 2 ** 30, 0, 5]
    assert lib.pxo_mc_emit(None, 8, 8, 8, 1.0, None, None, 0, counts, None, None, None, None) ==-1
    assert b"vertices" in lib.pxo_last_error()
    counts[:] = [3, 3, 3, 2 ** 31]
    assert lib.pxo_mc_emit(None, 8, 8, 8, 1.0, None, None, 0, counts, None, None, None, None) ==-1
    assert b"triangles" in lib.pxo_last_error()
    # grids with a side below 2 hold no cell: zero counts without a launch, on a machine without a GPU too
    counts[:] = [9, 9, 9, 9]
    assert lib.pxo_mc_count(None, 1, 5, 5, 1.0, None, None, 0, counts, None) == 0 and list(counts) == [0, 0, 0, 0]
    assert lib.pxo_mc_emit(None, 1, 5, 5, 1.0, None, None, 0, counts, None, None, None, None) ==0


def test_sigma_grid_argument_checks(lib):
    t = _lib.PxoTree()
    assert lib.pxo_tree_sigma_grid(None, 3, 1, None, None, None) == -1
    child, data = torch.zeros(1, 2, 2, 2, dtype=torch.int32), torch.zeros(1, 2, 2, 2, 4)
    t.child, t.data, t.n_internal, t.data_dim, t.basis_dim = child.data_ptr(), data.data_ptr(), 1, 4, 1
    out = torch.zeros(8)
    for depth, pad in ((0, 1), (_lib.TREE_MAX_DEPTH + 2, 1), (3, -1), (3, 65)):
        assert lib.pxo_tree_sigma_grid(ctypes.byref(t), depth, pad, out.data_ptr(), None, None) == -1
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PxoError):
            mesh_ops.tree_sigma_grid(t, 3)
        with pytest.raises(_lib.PxoError):
            mesh_ops.marching_cubes(torch.zeros(4, 4, 4), 0.5)


def test_uploaded_case_table_names_the_edges_of_the_host_table():
    table, count = mesh_ops.case_tables()
    assert table.dtype == np.int8 and table.shape == (256, 5, 3) and count.dtype == np.uint8
    assert np.array_equal(count, isosurface.TRI_COUNT)
    for case in (1, 23, 105, 254):
        for t in range(5):
            for k in range(3):
                e = isosurface.TRI_TABLE[case, t, k]
                if e < 0:
                    assert table[case, t, k] == -1
                else:
                    a, o = isosurface._EDGES[e]
                    assert table[case, t, k] >> 3 == a and table[case, t, k] & 7 == o and not (o >> a) & 1


# ---- octree.meshing: refusals that need no GPU, and the vertex mapping -----------------------------------------------
def _save_tree(path, fmt):
    from plenoctree_amd.octree.svox import N3Tree
    K = int(fmt[2:])
    extra = None
    if fmt.startswith("SG"):
        mu = np.random.RandomState(0).randn(K, 3)
        extra = np.concatenate([np.full((K, 1), 2.0), mu / np.linalg.norm(mu, axis=1, keepdims=True)], 1).astype(np.float32)
    N3Tree(N=2, data_dim=3 * K + 1, depth_limit=3, radius=1.0, center=[0, 0, 0], data_format=fmt, extra_data=extra).save(path)


def test_meshing_refuses_bad_input_before_touching_a_gpu(tmp_path):
    sh, sg, out = str(tmp_path / "sh.npz"), str(tmp_path / "sg.npz"), str(tmp_path / "m.obj")
    _save_tree(sh, "SH4")
    _save_tree(sg, "SG4")
    with pytest.raises(SystemExit, match=r"--color dc on an SG tree \(SG4\).*--color none"):
        meshing.main(["--input", sg, "--output", out, "--color", "dc"])
    for iso in ("0", "-3.5", "nan"):
        with pytest.raises(SystemExit, match="--iso must be > 0"):
            meshing.main(["--input", sh, "--output", out, "--iso", iso])
    for depth in ("0", "-1", str(_lib.TREE_MAX_DEPTH + 2)):
        with pytest.raises(SystemExit, match=rf"--depth {depth} outside \[1, {_lib.TREE_MAX_DEPTH + 1}\]"):
            meshing.main(["--input", sh, "--output", out, "--depth", depth])
    with pytest.raises(SystemExit, match="no such file"):
        meshing.main(["--input", str(tmp_path / "missing.npz"), "--output", out])
    # what passes these checks: an SG tree without --color (meshes uncoloured) and an SH tree with the largest depth
    args = meshing.define_flags().parse_args(["--input", sg, "--output", out])
    assert meshing.check_args(args) == "SG4" and args.color is None and args.iso == 10.0 and args.depth is None
    args = meshing.define_flags().parse_args(["--input", sh, "--output", out, "--depth", str(_lib.TREE_MAX_DEPTH + 1), "--color", "dc"])
    assert meshing.check_args(args) == "SH4"
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="needs a ROCm GPU"):
            meshing.main(["--input", sh, "--output", out])
    assert not (tmp_path / "m.obj").exists()


def test_index_to_world_on_a_hand_made_transform():
    # depth 3, pad 1: padded sample v is the centre of cell v - 1, tree coordinate (v - 1/2) / 8
    offset, invradius = np.array([0.25, 0.5, 0.25], np.float32), np.array([0.5, 0.25, 0.5], np.float32)
    v = np.array([[0.5, 0.5, 0.5],        # tree (0, 0, 0): the cube's lower corner
                  [8.5, 8.5, 8.5],        # tree (1, 1, 1)
                  [1.0, 1.0, 1.0],        # the centre of cell 0: tree 1/16
                  [4.5, 2.5, 6.5]])       # tree (1/2, 1/4, 3/4)
    want = np.array([[-0.5, -2.0, -0.5], [1.5, 2.0, 1.5], [-0.375, -1.75, -0.375], [0.5, -1.0, 1.0]])
    got = meshing.index_to_world(v, 3, offset, invradius)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    # pad 0: sample v is the centre of cell v
    assert np.array_equal(meshing.index_to_world(np.array([[3.5, 3.5, 3.5]]), 3, offset, invradius, pad=0),
                          np.array([[0.5, 0.0, 0.5]]))
    # float64 throughout: a float32 evaluation would lose the 2^-30 step
    step = meshing.index_to_world(np.array([[1.0 + 2.0 ** -30, 1.0, 1.0]]), 3, offset, invradius)[0, 0]
    assert step == -0.375 + 2.0 ** -32


# ---- the integer descent ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,tree_depth", [("shell", 4), ("chunked", 4), ("shell", 6)])
def test_numpy_descent_agrees_with_the_oracle_point_query(family, tree_depth):
    t = C.make_tree(family, tree_depth, 1)
    rs = np.random.RandomState(tree_depth)
    finest = int(t.parent_depth[:, 1].max()) + 1
    assert finest == tree_depth + 1
    for depth in (finest - 2, finest, finest + 1) if tree_depth == 4 else (finest,):
        sigma, packed = M.sigma_grid(t.child, t.data, depth, 1)
        g = 1 << depth
        assert sigma.shape == packed.shape == (g + 2,) * 3
        inner = (slice(1, -1),) * 3
        pad_mask = np.ones(sigma.shape, bool)
        pad_mask[inner] = False
        assert (sigma[pad_mask] == 0).all() and (packed[pad_mask] == -1).all() and (packed[inner] >= 0).all()
        # cell centres: random cells plus the cells around the deepest leaves' corners
        cells = rs.randint(0, g, (300, 3))
        lv = t.leaves()
        corner, _ = C.T.leaf_corners(t, lv[t.parent_depth[lv[:, 0], 1] == tree_depth][:100])
        cells = np.concatenate([cells, np.clip(np.floor(corner * g).astype(np.int64), 0, g - 1)])
        for i, j, k in cells:
            centre = ((np.array([i, j, k], np.float64) + 0.5) / g).astype(np.float32)      # exact
            node, ci, cj, ck, _, _ = t.query(centre)
            want = node * 8 + (ci * 2 + cj) * 2 + ck
            assert packed[i + 1, j + 1, k + 1] == want
            assert sigma[i + 1, j + 1, k + 1] == t.data[node, ci, cj, ck, -1]


# ---- gen_mesh --mc ---------------------------------------------------------------------------------------------------
def test_gen_mesh_mc_flag_and_cpu_fallback():
    flags = gen_mesh.define_flags()
    assert flags.parse_args([]).mc == "device"
    assert flags.parse_args(["--mc", "host"]).mc == "host"
    with pytest.raises(SystemExit):
        flags.parse_args(["--mc", "fpga"])
    c1, c2, reso = [-2.0, -1.0, -1.5], [2.0, 1.0, 1.5], [21, 17, 13]
    field = lambda p: (1.0 - p.norm(dim=-1, keepdim=True)) * 3.0
    cpu = torch.device("cpu")
    sig = gen_mesh.sigma_grid(field, c1, c2, reso, 1000, cpu)
    vi, fi = isosurface.marching_cubes(sig.numpy(), 0.25)
    scale = (np.array(c2) - np.array(c1)) / np.array(reso)
    for mc in ("device", "host"):                      # a grid on the CPU is meshed by the host function either way
        v, f = gen_mesh.marching_cubes(field, c1, c2, reso, 0.25, 1000, cpu, mc=mc)
        assert np.array_equal(f, fi) and np.array_equal(v, vi * scale + np.array(c1)) and len(f) > 100
    with pytest.raises(ValueError, match="mc must be one of"):
        gen_mesh.marching_cubes(field, c1, c2, reso, 0.25, 1000, cpu, mc="fpga")
