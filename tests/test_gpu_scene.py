"""The scene renderer (pxo_scene_render_fwd, svox.SceneRenderer) on the GPU.

Exact identities, torch.equal, no twin: one instance under the identity, a tree cut into two complementary instances, and an
instance under a signed permutation with scale 2 seen from the camera carried along, each against VolumeRenderer on the same
tree.  Against the float32 twin (tests/_scene_oracle.py) on the cases of tests/_scene_cases.py: rgb within rtol 0, atol 2e-5,
the bound tests/test_gpu_octree.py holds the single-tree forward to for the same reason (identical steps; only exp, sigmoid
and the order of the K-term sums differ).  tests/test_scene_cpu.py shows on the CPU that the twin's own float32-to-float64
compositing gap on these inputs (at most 2.3e-7) is far below half of that bound, and that no case is vacuous."""
import json
import os

import numpy as np
import pytest
import torch

import _octree_cases as C
import _scene_cases as SC
import _scene_oracle as S
from _helpers import _gpu, close
from oracle import octree_oracle as T

pytestmark = pytest.mark.gpu
f32 = np.float32
FORMATS = (1, 4, 9, 16, 25)
PRESETS = ((False, 1.0), (True, 0.0), (False, 0.0), (True, 1.0))           # (fast, background)


def _oops():
    from plenoctree_amd import octree_ops
    return octree_ops


def _svox():
    from plenoctree_amd.octree import svox
    return svox


def _svox_tree(t, dev):
    """The oracle tree `t` as an svox N3Tree on `dev`, float32 data as they are."""
    svox = _svox()
    z = {"data_dim": t.data_dim, "child": t.child, "parent_depth": t.parent_depth, "n_internal": t.n_internal,
         "invradius3": t.invradius, "offset": t.offset, "depth_limit": t.depth_limit, "data": t.data,
         "data_format": f"SH{(t.data_dim - 1) // 3}"}
    tree = svox.N3Tree._from_npz(svox._NpzDict({k: np.asarray(v) for k, v in z.items()}), dev)
    tree.data.requires_grad_(False)
    return tree


def _edge_tree(K):
    return C.random_tree(2, 40 + K, K, center=C.CENTER, radius=C.RADIUS)      # the volume C.edge_rays() is written for


def _ray_set(dev):
    """Explicit rays: C.edge_rays() plus the rays of a camera, with view directions unrelated to the directions."""
    _, o, d, v = C.edge_rays()
    co, cd = T.camera_rays(C.CAMERA_VIEWS[0]["c2w"], 9, 7, 6.0, 7.0)
    cv = np.roll(cd, 5, axis=0)
    return tuple(torch.from_numpy(np.ascontiguousarray(np.concatenate(p))).to(dev) for p in ((o, co), (d, cd), (v, cv)))


def _both_ways(plain, scene, dev, views, rays):
    """torch.equal of VolumeRenderer `plain(bg)` and SceneRenderer `scene(bg)` over both presets, both backgrounds, the camera
    views (plain view, scene view) and explicit rays (plain rays, scene rays)."""
    for fast, bg in PRESETS:
        p, s = plain(bg), scene(bg)
        for pv, sv in views:
            a = p.render_persp(torch.from_numpy(pv["c2w"]), pv["W"], pv["H"], pv["fx"], pv["fy"], fast=fast)
            b = s.render_persp(torch.from_numpy(sv["c2w"]), sv["W"], sv["H"], sv["fx"], sv["fy"], fast=fast)
            assert a.shape == b.shape == (pv["H"], pv["W"], 3)
            assert torch.equal(a, b), (fast, bg, float((a - b).abs().max()))
            assert float(a.std()) > 0.01
        if rays is not None:
            a, b = p.forward(*rays[0], fast=fast), s.forward(*rays[1], fast=fast)
            assert torch.equal(a, b), (fast, bg, float((a - b).abs().max()))


@pytest.mark.parametrize("K", FORMATS)
def test_one_identity_instance_equals_volume_renderer(K):
    svox, dev = _svox(), _gpu()
    views = [(v, v) for v in C.CAMERA_VIEWS]
    tree = _svox_tree(C.random_tree(3 if K <= 9 else 2, 5 + K, K), dev)
    _both_ways(lambda bg: svox.VolumeRenderer(tree, 1e-3, bg), lambda bg: svox.SceneRenderer([svox.Instance(tree)], 1e-3, bg),
               dev, views, None)
    edge = _svox_tree(_edge_tree(K), dev)
    rays = _ray_set(dev)
    _both_ways(lambda bg: svox.VolumeRenderer(edge, 1e-3, bg), lambda bg: svox.SceneRenderer([svox.Instance(edge)], 1e-3, bg),
               dev, [], (rays, rays))


@pytest.mark.parametrize("K,deep", [(K, False) for K in FORMATS] + [(4, True)])
def test_complementary_halves_equal_the_whole(K, deep):
    """deep: C.shell(5, 4), uneven down to depth 5, so that every instance reuses its own path across many levels."""
    svox, dev = _svox(), _gpu()
    whole = C.shell(5, 4) if deep else C.random_tree(3 if K <= 9 else 2, 5 + K, K)
    a, b = S.split_by_x(whole)
    assert (a.data[..., -1] != whole.data[..., -1]).any() and (b.data[..., -1] != whole.data[..., -1]).any()
    tw, ta, tb = (_svox_tree(t, dev) for t in (whole, a, b))
    rays = _ray_set(dev) if deep else None               # C.shell lives in the volume of C.edge_rays()
    _both_ways(lambda bg: svox.VolumeRenderer(tw, 1e-3, bg),
               lambda bg: svox.SceneRenderer([svox.Instance(ta), svox.Instance(tb)], 1e-3, bg), dev,
               [(v, v) for v in C.CAMERA_VIEWS], None if rays is None else (rays, rays))


@pytest.mark.parametrize("K", FORMATS)
def test_permuted_scaled_instance_from_the_carried_camera(K):
    svox, dev = _svox(), _gpu()
    tree = _svox_tree(_edge_tree(K), dev)
    views = []
    for v in C.CAMERA_VIEWS:
        moved = dict(v)
        moved["c2w"] = S.transformed_camera(v["c2w"], S.CYCLIC, 2.0)
        views.append((v, moved))
    o, d, vd = _ray_set(dev)
    turn = lambda a, s: torch.from_numpy((s * (a.cpu().numpy().astype(np.float64) @ S.CYCLIC.T)).astype(f32)).to(dev)
    carried = (turn(o, 2.0), turn(d, 1.0), turn(vd, 1.0))                     # a permutation, signs and x2: exact
    _both_ways(lambda bg: svox.VolumeRenderer(tree, 1e-3, bg),
               lambda bg: svox.SceneRenderer([svox.Instance(tree, S.CYCLIC, scale=2.0)], 1e-3, bg), dev, views,
               ((o, d, vd), carried))
    # the guard: a transposed matrix is seen
    v, moved = views[0]
    good = svox.VolumeRenderer(tree, 1e-3).render_persp(torch.from_numpy(v["c2w"]), v["W"], v["H"], v["fx"], v["fy"])
    bad = svox.SceneRenderer([svox.Instance(tree, S.CYCLIC.T, scale=2.0)], 1e-3).render_persp(
        torch.from_numpy(moved["c2w"]), v["W"], v["H"], v["fx"], v["fy"])
    assert float((good - bad).abs().max()) > 0.1


# ---- against the float32 twin ------------------------------------------------------------------------------------------
def _svox_scene(name, opt, dev):
    svox = _svox()
    trees = {}
    inst = []
    for I in SC.instances(name):
        if id(I.tree) not in trees:
            trees[id(I.tree)] = _svox_tree(I.tree, dev)
        inst.append(svox.Instance(trees[id(I.tree)], I.rot_t.T.astype(np.float64), I.trans.astype(np.float64), float(I.scale)))
    o = SC.OPT[opt]
    assert float(o.sigma_thresh) == float(o.stop_thresh) and float(o.sigma_thresh) in (0.0, float(f32(1e-2)))
    return svox.SceneRenderer(inst, float(o.step_size), float(o.background_brightness)), float(o.sigma_thresh) > 0


@pytest.mark.parametrize("name,opt", SC.CASE_OPTS)
def test_scene_matches_the_float32_twin(name, opt):
    """rgb within rtol 0, atol 2e-5 of the twin (the module docstring has the bound's reason)."""
    dev = _gpu()
    want = SC.reference(name, opt)[0].copy()            # the shared reference is read-only
    r, fast = _svox_scene(name, opt, dev)
    v = SC.CASES[name][1]
    got = r.render_persp(torch.from_numpy(v["c2w"]), v["W"], v["H"], v["fx"], v["fy"], fast=fast)
    print(name, opt, "max abs err", float((got.cpu() - torch.from_numpy(want)).abs().max()))
    close(f"scene {name} {opt}", got, torch.from_numpy(want), rtol=0.0, atol=2e-5)
    if name == "same_tree_twice":
        assert r.instances[0].tree is r.instances[1].tree


def test_one_pixel_image_and_ray_counts_around_a_block():
    """A 1 x 1 image, and explicit rays one short of and one past the 64 rays of a workgroup (kRaysPerBlock), through the
    C ABI front end (octree_ops) directly."""
    oops, dev = _oops(), _gpu()
    name = "two_overlap_scaled"
    inst = SC.instances(name)
    keep = [(torch.from_numpy(I.tree.child).to(dev), torch.from_numpy(I.tree.data).to(dev)) for I in inst]
    scene = oops.scene_instances([(oops.tree_view(c, d, I.tree.offset, I.tree.invradius), I.rot_t.T, I.trans, float(I.scale))
                                  for I, (c, d) in zip(inst, keep)], dev)
    opts = oops.render_opts(1e-3, 1.0, 0.0, 0.0)
    view = SC.CASES[name][1]
    want = torch.from_numpy(SC.reference(name, "exact")[0].reshape(-1, 3).copy())     # the shared reference is read-only
    o, d = T.camera_rays(view["c2w"], view["W"], view["H"], view["fx"], view["fy"])
    for count in (63, 64, 65):
        rays = [torch.from_numpy(np.ascontiguousarray(a[:count])).to(dev) for a in (o, d, d)]
        got = oops.scene_render_rays(scene, *rays, opts)
        assert got.shape == (count, 3)
        close(f"{count} rays", got, want[:count], rtol=0.0, atol=2e-5)
    one = dict(c2w=view["c2w"], W=1, H=1, fx=3.0, fy=3.0)
    ref = S.render_persp(inst, opt=SC.OPT["exact"], **one)
    got = oops.scene_render_persp(scene, torch.from_numpy(one["c2w"]).to(dev), 1, 1, 3.0, opts, 3.0)
    assert got.shape == (1, 1, 3) and float(np.abs(ref - 1.0).max()) > 0.01
    close("1 x 1 image", got, torch.from_numpy(ref), rtol=0.0, atol=2e-5)
    empty = oops.scene_render_rays(scene, *[torch.zeros(0, 3, device=dev)] * 3, opts)
    assert empty.shape == (0, 3)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    import ctypes
    from plenoctree_amd import _lib
    oops, dev = _oops(), _gpu()
    lib = _lib.load()
    t = SC.tree(4)
    child, data = torch.from_numpy(t.child).to(dev), torch.from_numpy(t.data).to(dev)
    view = oops.tree_view(child, data, t.offset, t.invradius)
    good = (view, np.eye(3), np.zeros(3), 1.0)
    for n in (0, 9):
        with pytest.raises(oops.PxoError, match="1 .. 8"):
            oops.scene_instances([good] * n, dev)
        host = (_lib.PxoInstance * max(n, 1))()
        assert lib.pxo_scene_check(host, n) != 0 and b"1 .. 8" in lib.pxo_last_error()
    scene = oops.scene_instances([good], dev)
    opts = oops.render_opts(1e-3)
    out = torch.zeros(4, 3, device=dev)
    rays = [torch.zeros(4, 3, device=dev)] * 3
    for n in (0, 9, -1):
        rc = lib.pxo_scene_render_fwd(scene.records.data_ptr(), n, None, *[r.data_ptr() for r in rays], 4, ctypes.byref(opts),
                                      out.data_ptr(), None)
        assert rc != 0 and b"1 .. 8" in lib.pxo_last_error()
    for scale, word in ((0.0, "scale"), (-2.0, "scale"), (float("inf"), "scale"), (float("nan"), "scale"), (1e-46, "scale")):
        with pytest.raises(oops.PxoError, match=word):
            oops.scene_instances([good, (view, np.eye(3), np.zeros(3), scale)], dev)
    with pytest.raises(oops.PxoError, match="finite"):
        oops.scene_instances([(view, np.eye(3), [0.0, float("nan"), 0.0], 1.0)], dev)
    bad = oops.tree_view(child, data, t.offset, t.invradius)
    bad.basis_dim, bad.data_dim = 7, 22
    with pytest.raises(oops.PxoError, match="basis_dim 7"):
        oops.scene_instances([good, (bad, np.eye(3), np.zeros(3), 1.0)], dev)
    null = oops.tree_view(child, data, t.offset, t.invradius)
    null.data = None
    with pytest.raises(oops.PxoError, match="null tree"):
        oops.scene_instances([(null, np.eye(3), np.zeros(3), 1.0)], dev)
    with pytest.raises(NotImplementedError, match="float SH tree"):
        oops.scene_instances([(_lib.PxoHalfTree(), np.eye(3), np.zeros(3), 1.0)], dev)
    with pytest.raises(oops.PxoError, match="step_size"):
        oops.scene_render_rays(scene, *rays, oops.render_opts(0.0))


def test_renderer_refusals():
    svox, dev = _svox(), _gpu()
    tree = _svox_tree(SC.tree(4), dev)
    inst = svox.Instance(tree)
    with pytest.raises(NotImplementedError, match="ndc"):
        svox.SceneRenderer([inst], ndc=svox.NDCConfig(8, 8, 10.0))
    with pytest.raises(NotImplementedError, match="max_depth"):
        svox.SceneRenderer([inst], max_depth=1)
    with pytest.raises(NotImplementedError, match="lod_pixels"):
        svox.SceneRenderer([inst], lod_pixels=2.0)
    with pytest.raises(ValueError, match="1 .. 8"):
        svox.SceneRenderer([])
    with pytest.raises(ValueError, match="1 .. 8"):
        svox.SceneRenderer([inst] * 9)
    r = svox.SceneRenderer([inst, svox.Instance(tree, translation=(0.5, 0, 0))], 1e-3)
    c2w = torch.from_numpy(C.CAMERA_VIEWS[0]["c2w"])
    tree.data.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="requires grad"):
        r.render_persp(c2w, 8, 6, 7.0)
    with torch.no_grad():
        assert r.render_persp(c2w, 8, 6, 7.0).shape == (6, 8, 3)
    tree.data.requires_grad_(False)
    with tree.accumulate_weights(op="max"):
        with pytest.raises(NotImplementedError, match="accumulate_weights"):
            r.render_persp(c2w, 8, 6, 7.0)
        with pytest.raises(NotImplementedError, match="accumulate_weights"):
            r.forward(*[torch.zeros(2, 3, device=dev)] * 3)
    assert r.render_persp(c2w, 8, 6, 7.0).shape == (6, 8, 3)


# ---- changes to an instanced tree ---------------------------------------------------------------------------------------
def test_tree_edits_are_followed_by_the_next_render():
    svox, dev = _svox(), _gpu()
    tree = _svox_tree(C.random_tree(2, 31, 4), dev)
    scene = svox.SceneRenderer([svox.Instance(tree)], 1e-3)
    plain = svox.VolumeRenderer(tree, 1e-3)
    v = C.CAMERA_VIEWS[0]
    shot = lambda r: r.render_persp(torch.from_numpy(v["c2w"]), v["W"], v["H"], v["fx"], v["fy"])
    first = shot(scene)
    assert torch.equal(first, shot(plain))
    records = scene._scene
    assert torch.equal(shot(scene), first) and scene._scene is records            # nothing changed: nothing rebuilt
    # a data replacement: a new parameter over new storage
    tree.data = torch.nn.Parameter(tree.data.data.flip(0).roll(1, 1).contiguous(), requires_grad=False)
    second = shot(scene)
    assert scene._scene is not records and not torch.equal(second, first)
    assert torch.equal(second, shot(plain))
    # a structure edit: every fourth leaf is split; child and data are new tensors
    mask = torch.zeros(tree.n_internal * 8, dtype=torch.bool, device=dev)
    mask[::4] = True
    n0, records = tree.n_internal, scene._scene
    assert tree.refine_leaves(mask) > 0 and tree.n_internal > n0
    third = shot(scene)
    assert scene._scene is not records
    assert torch.equal(third, shot(plain))
    # an edit in place is read through the same records
    tree.data.data[..., -1] *= 0.5
    assert torch.equal(shot(scene), shot(plain)) and not torch.equal(shot(scene), third)


# ---- the command-line tool ----------------------------------------------------------------------------------------------
def test_compose_cli_writes_its_frames(tmp_path, capsys):
    from plenoctree_amd.octree import compose
    dev = _gpu()
    _svox_tree(SC.tree(4), dev).save(str(tmp_path / "a.npz"))
    _svox_tree(SC.tree(9), dev).save(str(tmp_path / "b.npz"))
    scene = {"background": 0.5, "instances": [
        {"tree": "a.npz", "rotation": {"axis": [0, 0, 1], "angle_deg": 30.0}, "scale": 0.8, "translation": [0.6, 0.0, 0.0]},
        {"tree": "b.npz", "rotation": S.axis_angle((1, 0, 0), 20.0).tolist(), "translation": [-0.7, 0.1, 0.0]}]}
    with open(tmp_path / "scene.json", "w") as f:
        json.dump(scene, f)
    out = tmp_path / "out"
    n = compose.main(["--scene", str(tmp_path / "scene.json"), "--output_dir", str(out), "--orbit", "4.0", "25", "3",
                      "--width", "16", "--height", "12", "--focal", "14", "--renderer_step_size", "1e-3",
                      "--write_vid", str(tmp_path / "orbit.gif")])
    said = capsys.readouterr().out
    assert n == 3 and "ms per frame" in said and "instance 1:" in said
    from PIL import Image
    frames = []
    for k in range(3):
        path = out / f"{k:03d}.png"
        assert f"Wrote {path}" in said and path.exists()
        frames.append(np.asarray(Image.open(path)))
        assert frames[-1].shape == (12, 16, 3) and frames[-1].std() > 2.0
    assert not np.array_equal(frames[0], frames[1])
    assert os.path.getsize(tmp_path / "orbit.gif") > 0
    with pytest.raises(ValueError, match="--orbit"):
        compose.main(["--scene", str(tmp_path / "scene.json"), "--output_dir", str(out)])
    with pytest.raises(ValueError, match="unknown flags"):
        compose.main(["--scene", str(tmp_path / "scene.json"), "--output_dir", str(out), "--orbit", "4", "25", "3", "--factor", "8"])
    # the other camera source: the test poses of a dataset (the analytic scene of the `synthetic` preset); not rendered here
    args, rest = compose.define_flags().parse_known_args(["--scene", "s", "--output_dir", "o", "--config", "synthetic"])
    cams, w, h, focal = compose.cameras(args, dev, rest)
    assert w >= 1 and h >= 1 and focal > 0 and len(cams) >= 1 and all(np.asarray(c).shape in ((4, 4), (3, 4)) for c in cams)
