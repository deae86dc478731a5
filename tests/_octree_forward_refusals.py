"""What tests/test_octree_forward_refusals_cpu.py holds the argument checks of the octree renderers to: for each of the eight
forward entry points, the three backward ones and pxo_octree_count_work, one call per bad argument (and a few ordered pairs of
two), with the return code and the full pxo_last_error() text.  The checks run before any HIP call, so the pointers are never
dereferenced and no GPU is needed.  record() is run once on the commit BEFORE a change of the host layer to write
tests/golden/octree_forward_refusals.json (python tests/_octree_forward_refusals.py), and by the test on the tree under test."""
import copy
import ctypes
import json
import os
import sys

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "octree_forward_refusals.json")
PTR = 0x10000                                     # a 256-byte aligned address nothing reads

# entry point -> (tree form, takes lobes, takes ndc, aux, backward)
ENTRIES = {
    "pxo_octree_render_fwd": ("float", False, False, False, False),
    "pxo_octree_render_sg_fwd": ("float", True, False, False, False),
    "pxo_octree_render_ndc_fwd": ("float", False, True, False, False),
    "pxo_octree_render_aux_fwd": ("float", False, False, True, False),
    "pxo_octree_render_quant_fwd": ("quant", False, False, False, False),
    "pxo_octree_render_quant_aux_fwd": ("quant", False, False, True, False),
    "pxo_octree_render_half_fwd": ("half", True, True, False, False),
    "pxo_octree_render_half_aux_fwd": ("half", False, False, True, False),
    "pxo_octree_render_bwd": ("float", False, False, False, True),
    "pxo_octree_render_sg_bwd": ("float", True, False, False, True),
    "pxo_octree_render_ndc_bwd": ("float", False, True, False, True),
    "pxo_octree_count_work": ("float", False, False, False, False),
}
COUNT = "pxo_octree_count_work"

TREES = {
    "float": dict(child=PTR, data=PTR, n_internal=9, data_dim=49, basis_dim=16, offset=(0.5,) * 3, invradius=(0.5,) * 3),
    "half": dict(child=PTR, data=PTR, n_internal=9, data_dim=49, basis_dim=16, row_stride=52, offset=(0.5,) * 3,
                 invradius=(0.5,) * 3),
    "quant": dict(child=PTR, idx=PTR, palette=PTR, sigma=PTR, retained=PTR, n_internal=9, basis_dim=16, n_retained=1, bits=4,
                  idx_stride=16, ret_stride=4, offset=(0.5,) * 3, invradius=(0.5,) * 3),
}
CAMERA = dict(c2w=PTR, fx=10.0, fy=10.0, width=4, height=3)
NDC = dict(width=4, height=3, focal=10.0, near=1.0)


def good(entry):
    """A call of `entry` that every check accepts: 5 explicit rays (pxo_octree_count_work: a 4x3 camera)."""
    form, lobes, ndc, aux, bwd = ENTRIES[entry]
    s = dict(tree=dict(TREES[form]), opts=dict(step_size=1e-3, background_brightness=1.0, sigma_thresh=0.0, stop_thresh=0.0),
             cam=None, origins=PTR, dirs=PTR, viewdirs=PTR, B=5, out_rgb=PTR)
    if entry == COUNT:
        return dict(tree=s["tree"], opts=s["opts"], cam=dict(CAMERA), counts=PTR, leaf_seen=PTR)
    if lobes:
        s["lobes"] = PTR if form == "float" else None          # the half entry point takes SH trees without lobes
    if ndc:
        s["ndc"] = dict(NDC) if form == "float" else None
    if aux:
        s["surface_thresh"], s["out_aux"] = 0.5, PTR
    if bwd:
        s["out_rgb"], s["grad_out"], s["grad_data"] = None, PTR, PTR
    return s


def _set(path, value):
    def apply(s):
        d = s
        for k in path[:-1]:
            d = d[k]
        d[path[-1]] = value
    return apply


def _camera(**kw):
    def apply(s):
        s["cam"] = dict(CAMERA, **kw)
        if "B" in s:
            s["origins"] = s["dirs"] = s["viewdirs"] = None
            s["B"] = 12
    return apply


def _all(*fs):
    def apply(s):
        for f in fs:
            f(s)
    return apply


def _format(K, D):
    """basis_dim K / data_dim D with the strides that go with them, so that the format is the only thing wrong."""
    def apply(s):
        t = s["tree"]
        t["basis_dim"] = K
        if "data_dim" in t:
            t["data_dim"] = D
        if "row_stride" in t:
            t["row_stride"] = (D + 3) & ~3
        if "idx_stride" in t:
            t["idx_stride"] = (K - t["n_retained"] + 3) & ~3
    return apply


def _no_outputs(s):
    for k in ("out_rgb", "out_aux", "grad_out", "grad_data"):
        if k in s:
            s[k] = None


def mutations(entry):
    """[(case name, mutation of good(entry))]: one bad argument each, then the ordered pairs."""
    form, lobes, ndc, aux, bwd = ENTRIES[entry]
    count = entry == COUNT
    m = [("null_options", _set(("opts",), None)),
         ("step_size_0", _set(("opts", "step_size"), 0.0)),
         ("null_tree", _set(("tree",), None)),
         ("basis_dim_7", _format(7, 22)),
         ("n_internal_0", _set(("tree", "n_internal"), 0)),
         ("n_internal_2^28", _set(("tree", "n_internal"), 1 << 28)),
         ("camera_null_c2w", _camera(c2w=None)),
         ("camera_width_0", _camera(width=0)),
         ("camera_height_0", _camera(height=0)),
         ("camera_fx_0", _camera(fx=0.0))]
    m += [(f"null_{k}", _set(("tree", k), None)) for k in TREES[form] if TREES[form][k] == PTR and k != "retained"]
    if form != "quant":
        m.append(("data_dim_50", _format(16, 50)))
    if count:
        m += [("null_camera", _set(("cam",), None)), ("null_counts", _set(("counts",), None))]
        return m
    m += [("B_-1", _set(("B",), -1)),
          ("camera_B_11", _all(_camera(), _set(("B",), 11))),
          ("B_0_null_outputs_ok", _all(_set(("B",), 0), _no_outputs)),
          ("camera_ok_B_0_refused", _all(_camera(), _set(("B",), 0)))]
    m += [(f"null_{k}", _set((k,), None)) for k in ("origins", "dirs", "viewdirs")]
    m += [(f"null_{k}", _set((k,), None)) for k in ("out_rgb", "out_aux", "grad_out", "grad_data") if k in good(entry) and
          not (bwd and k == "out_rgb")]
    if bwd:
        m.append(("out_rgb_of_a_fast_march", _all(_set(("out_rgb",), PTR), _set(("opts", "stop_thresh"), 0.01))))
    if form == "half":
        m += [("row_stride_49", _set(("tree", "row_stride"), 49)), ("row_stride_56", _set(("tree", "row_stride"), 56)),
              ("data_misaligned", _set(("tree", "data"), PTR + 4))]
    if form == "quant":
        m += [("n_retained_K", _all(_set(("tree", "n_retained"), 16), _set(("tree", "idx_stride"), 0), _set(("tree", "ret_stride"), 64))),
              ("bits_0", _set(("tree", "bits"), 0)), ("bits_17", _set(("tree", "bits"), 17)),
              ("idx_stride_15", _set(("tree", "idx_stride"), 15)), ("ret_stride_3", _set(("tree", "ret_stride"), 3)),
              ("null_retained", _set(("tree", "retained"), None)), ("idx_misaligned", _set(("tree", "idx"), PTR + 4)),
              ("palette_misaligned", _set(("tree", "palette"), PTR + 2)), ("retained_misaligned", _set(("tree", "retained"), PTR + 1))]
    bad_thresh = _set(("surface_thresh",), 1.5)
    if aux:
        stop = _set(("opts", "stop_thresh"), 0.01)
        m += [("surface_thresh_at_stop_thresh", _all(stop, _set(("surface_thresh",), 0.01))),
              ("surface_thresh_below", _all(stop, _set(("surface_thresh",), 0.001))),
              ("surface_thresh_at_1", _set(("surface_thresh",), 1.0)),
              ("surface_thresh_above", bad_thresh),
              ("surface_thresh_nan", _set(("surface_thresh",), float("nan"))),
              # order: the tree and ray checks, then surface_thresh, then B == 0
              ("pair_surface_thresh_null_tree", _all(bad_thresh, _set(("tree",), None))),
              ("pair_surface_thresh_n_internal_0", _all(bad_thresh, _set(("tree", "n_internal"), 0))),
              ("pair_surface_thresh_null_dirs", _all(bad_thresh, _set(("dirs",), None))),
              ("pair_surface_thresh_B_-1", _all(bad_thresh, _set(("B",), -1))),
              ("pair_surface_thresh_B_0", _all(bad_thresh, _set(("B",), 0), _no_outputs)),
              ("pair_surface_thresh_null_out_aux", _all(bad_thresh, _set(("out_aux",), None)))]
    bad_ndc = _set(("ndc",), dict(NDC, width=0))
    if ndc:
        m += [("ndc_width_0", bad_ndc), ("ndc_height_0", _set(("ndc",), dict(NDC, height=0))),
              ("ndc_focal_0", _set(("ndc",), dict(NDC, focal=0.0))), ("ndc_near_0", _set(("ndc",), dict(NDC, near=0.0))),
              # order: the ndc checks come before the options and the tree checks
              ("pair_ndc_null_options", _all(bad_ndc, _set(("opts",), None))),
              ("pair_ndc_null_tree", _all(bad_ndc, _set(("tree",), None))),
              ("pair_ndc_basis_dim_7", _all(bad_ndc, _format(7, 22)))]
        if form == "float":
            m.append(("null_ndc", _set(("ndc",), None)))
    if lobes:
        sg7 = _all(_set(("lobes",), PTR), _format(7, 22))
        m += [("sg_basis_dim_7", sg7), ("sg_data_dim_50", _all(_set(("lobes",), PTR), _format(16, 50))),
              # order: an SG entry point names SG for a bad basis_dim whatever else is wrong
              ("pair_sg_basis_dim_7_step_size_0", _all(sg7, _set(("opts", "step_size"), 0.0)))]
        if form == "float":
            m += [("null_lobes", _set(("lobes",), None)),
                  ("pair_sg_basis_dim_7_null_options", _all(sg7, _set(("opts",), None))),
                  ("pair_sg_basis_dim_7_null_lobes", _all(_format(7, 22), _set(("lobes",), None))),
                  ("pair_null_lobes_null_options", _all(_set(("lobes",), None), _set(("opts",), None)))]
    if form == "half" and lobes and ndc:
        both = _all(_set(("lobes",), PTR), _set(("ndc",), dict(NDC)))
        m += [("lobes_with_ndc", both),
              # order: lobes && ndc, then the ndc checks, then the tree checks
              ("pair_lobes_with_ndc_bad_ndc", _all(_set(("lobes",), PTR), bad_ndc)),
              ("pair_lobes_with_ndc_null_tree", _all(both, _set(("tree",), None))),
              ("pair_lobes_with_ndc_null_options", _all(both, _set(("opts",), None)))]
    return m


def _struct(cls, fields):
    if fields is None:
        return None
    s = cls()
    for k, v in fields.items():
        setattr(s, k, (ctypes.c_float * 3)(*v) if isinstance(v, tuple) else v)
    return ctypes.byref(s)


def call(_lib, entry, s):
    """(return code, pxo_last_error() text or "" for PXO_OK) of one call of `entry` with the arguments of spec `s`."""
    form = ENTRIES[entry][0]
    lib = _lib.load()
    tree = _struct({"float": _lib.PxoTree, "half": _lib.PxoHalfTree, "quant": _lib.PxoQuantTree}[form], s["tree"])
    cam, opts = _struct(_lib.PxoCamera, s["cam"]), _struct(_lib.PxoRenderOpts, s["opts"])
    if entry == COUNT:
        args = (tree, cam, opts, s["counts"], s["leaf_seen"], None)
    else:
        args = (tree,) + ((s["lobes"],) if "lobes" in s else ()) + (cam, s["origins"], s["dirs"], s["viewdirs"], s["B"], opts)
        if "surface_thresh" in s:
            args += (s["surface_thresh"], s["out_rgb"], s["out_aux"])
        elif "grad_out" in s:
            args += (s["out_rgb"], s["grad_out"], s["grad_data"])
        else:
            args += (s["out_rgb"],)
        args += (None,)                           # the stream
        if "ndc" in s:
            args += (_struct(_lib.PxoNdc, s["ndc"]),)
    rc = getattr(lib, entry)(*args)
    return rc, "" if rc == 0 else (lib.pxo_last_error() or b"").decode()


def cases():
    """[(row id, entry point, spec)]."""
    out = []
    for entry in ENTRIES:
        for name, mutate in mutations(entry):
            s = copy.deepcopy(good(entry))
            mutate(s)
            out.append((f"{entry}/{name}", entry, s))
    assert len({c[0] for c in out}) == len(out)
    return out


def record(_lib):
    rows = {}
    for rid, entry, s in cases():
        rc, text = call(_lib, entry, s)
        # a row that passed every check would launch on pointers nothing backs: only refusals, and B == 0, belong here
        assert (rc, text) == (0, "") and s.get("B") == 0 or rc == -1 and text.startswith(entry + ": "), (rid, rc, text)
        rows[rid] = {"rc": rc, "error": text}
    return rows


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from plenoctree_amd import _lib as lib_module
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(path, "w") as f:
        json.dump(record(lib_module), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
