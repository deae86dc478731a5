"""Host side of the forward-facing (LLFF) scenes: the loader against what the REFERENCE's `LLFF` class makes of the same
directory (tests/golden/llff_tiny + llff_reference.npz, written by tests/golden/make_golden_llff.py), the host
convert_to_ndc against the reference's float64 evaluation, the rays a dataset hands out, flags and sharding.

Bounds.  Poses, focal, size: rtol 1e-5 / atol 1e-6, what test_host_cpu.py uses for the other loaders.  NDC rays against the
float64 reference (`ndc64_*`): 4 x e_ref, where e_ref (from the fixture, 4.8e-7) is the reference's OWN float32 distance from
its float64 evaluation over every ray of the fixture; the factor covers a different operation order / contraction.  NDC
rays against the reference's recorded float32 rays: one e_ref more (5 x e_ref), since the recording carries its own error.
World-space rays and viewdirs: rtol 1e-5 / atol 1e-6 as for the other loaders."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

from plenoctree_amd.nerf_sh.nerf import datasets, families, llff, utils, viewdirs

HERE = os.path.dirname(os.path.abspath(__file__))
TINY = os.path.join(HERE, "golden", "llff_tiny")
CPU = torch.device("cpu")
CASES = [(split, s, f, hold) for hold in (8, 4) for split in ("train", "test") for s in (0, 1) for f in (0, 2)]
CASES8 = [c for c in CASES if c[3] == 8]


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(HERE, "golden", "llff_reference.npz")))


@pytest.fixture(autouse=True, scope="module")
def _llff_cpu_feeder():
    """LLFF datasets on a CPU device get the stand-in with the NDC methods (the session-wide one of conftest.py has none)."""
    sys.path.insert(0, HERE)
    from _llff_cpu_feeder import feeder_for
    llff.LLFF.feeder_factory = staticmethod(feeder_for)
    yield
    del llff.LLFF.feeder_factory


def _args(extra=(), **over):
    a = utils.define_flags().parse_args(["--config", "llff", "--train_dir", "x", "--data_dir", TINY, *extra])
    utils.update_flags(a)
    a.factor = 0
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _key(split, s, f, hold):
    return f"{split}_s{s}_f{f}_h{hold}_"


def _dataset(split, s, f, hold, **kw):
    over = {k: kw.pop(k) for k in ("render_path", "image_batching") if k in kw}
    return llff.get_dataset(split, _args(spherify=bool(s), factor=f, llffhold=hold, **over), CPU, **kw)


@pytest.mark.parametrize("split,s,f,hold", CASES)
def test_loader_matches_the_reference(ref, split, s, f, hold):
    k = _key(split, s, f, hold)
    ds = _dataset(split, s, f, hold)
    assert isinstance(ds, llff.LLFF)
    np.testing.assert_array_equal(ds.indices, ref[k + "indices"])
    assert (ds.h, ds.w) == (int(ref[k + "h"]), int(ref[k + "w"])) == ((8, 12) if f == 2 else (16, 24))
    np.testing.assert_allclose(ds.focal, float(ref[k + "focal"]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ds.camtoworlds, ref[k + "camtoworlds"], rtol=1e-5, atol=1e-6)
    assert ds.size == len(ref[k + "indices"]) == ds.images.shape[0]
    if split == "test":
        assert list(ds.indices) == ([0, 8] if hold == 8 else [0, 4, 8])
    if hold == 8:
        np.testing.assert_array_equal(ds.images.numpy().reshape(-1, ds.h, ds.w, 3), ref[k + "images"])
        if split == "test":
            assert ds.render_poses.shape == (120, 3, 4)
            np.testing.assert_allclose(ds.render_poses, ref[k + "render_poses"], rtol=1e-5, atol=1e-6)
        else:
            assert ds.render_poses is None


def test_loader_rejects_inconsistent_directories(tmp_path):
    with pytest.raises(ValueError, match="images_3"):
        llff.get_dataset("train", _args(factor=3), CPU)
    broken = tmp_path / "scene"
    shutil.copytree(TINY, broken)
    os.remove(broken / "images" / "image008.png")
    with pytest.raises(RuntimeError, match="8 images in .* but 9 poses"):
        llff.get_dataset("train", _args(data_dir=str(broken)), CPU)
    with pytest.raises(ValueError, match="render_path"):
        llff.get_dataset("train", _args(render_path=True), CPU)


@pytest.mark.parametrize("split,f", [("train", 0), ("train", 2), ("test", 0), ("test", 2)])
def test_host_convert_to_ndc_against_the_float64_reference(ref, split, f):
    k = _key(split, 0, f, 8)
    h, w, focal = int(ref[k + "h"]), int(ref[k + "w"]), np.float32(ref[k + "focal"])
    eo, ed = float(ref["e_ref_origins"]), float(ref["e_ref_directions"])
    assert 1e-7 < eo < 1e-6 and 1e-7 < ed < 1e-6          # a float32 error of values of order 1
    sets = [(ref[k + "camtoworlds"][ref[k + "ray_cams"]], ref[k + "ndc64_origins"], ref[k + "ndc64_directions"])]
    if split == "test":
        sets.append((ref[k + "render_poses"][ref["render_ray_poses"]], ref[k + "ndc64_render_origins"],
                     ref[k + "ndc64_render_directions"]))
    for c2w, o64, d64 in sets:
        assert c2w.dtype == np.float32
        rays = utils.generate_rays(w, h, focal, c2w)
        o, d = llff.convert_to_ndc(rays.origins, rays.directions, focal, w, h)
        assert o.dtype == np.float32 and d.dtype == np.float32
        dev_o, dev_d = np.abs(o.reshape(o64.shape) - o64).max(), np.abs(d.reshape(d64.shape) - d64).max()
        print(f"host float32 numpy vs ndc64: origins {dev_o:.3e} directions {dev_d:.3e} (bound {4 * eo:.3e})")
        assert dev_o <= 4 * eo and dev_d <= 4 * ed
        # torch tensors take the same path
        ot, dt = llff.convert_to_ndc(torch.from_numpy(np.ascontiguousarray(rays.origins)), torch.from_numpy(rays.directions),
                                     float(focal), w, h)
        assert ot.dtype == torch.float32
        assert np.abs(ot.numpy().reshape(o64.shape) - o64).max() <= 4 * eo
        assert np.abs(dt.numpy().reshape(d64.shape) - d64).max() <= 4 * ed
        # in float64 the formula IS the reference's: same values to rounding of the last bits
        r64 = utils.generate_rays(w, h, np.float64(focal), c2w.astype(np.float64))
        o2, d2 = llff.convert_to_ndc(r64.origins, r64.directions, np.float64(focal), w, h)
        np.testing.assert_allclose(o2.reshape(o64.shape), o64, rtol=0, atol=1e-14)
        np.testing.assert_allclose(d2.reshape(d64.shape), d64, rtol=0, atol=1e-14)
        # known answers: origins on the near plane z = -1, every ray ends on the far plane z = +1
        np.testing.assert_allclose(o64[..., 2], -1.0, rtol=0, atol=1e-14)
        np.testing.assert_allclose(o64[..., 2] + d64[..., 2], 1.0, rtol=0, atol=1e-14)


@pytest.mark.parametrize("split,s,f,hold", CASES8)
def test_image_rays_match_the_reference(ref, split, s, f, hold):
    k = _key(split, s, f, hold)
    ds = _dataset(split, s, f, hold)
    e = max(float(ref["e_ref_origins"]), float(ref["e_ref_directions"]))
    plain = datasets.Dataset.feeder_factory(CPU)
    for j, cam in enumerate(ref[k + "ray_cams"]):
        ex = ds.get_image(int(cam))
        assert ex["pixels"].shape == (ds.h, ds.w, 3) and ex["rays"].origins.shape == (ds.h, ds.w, 3)
        np.testing.assert_array_equal(ex["pixels"].numpy(), ref[k + "images"][cam])
        o, d, v = [r.reshape(-1, 3).numpy() for r in ex["rays"]]
        world = plain.generate_rays(torch.from_numpy(ds.camtoworlds[cam]), ds.w, ds.h, ds.focal, torch.arange(ds.h * ds.w))
        np.testing.assert_allclose(np.linalg.norm(v, axis=-1), 1.0, rtol=0, atol=1e-6)
        np.testing.assert_array_equal(v, world[2].numpy())           # NDC or not: the world-space unit direction
        np.testing.assert_allclose(v, ref[k + "rays_viewdirs"][j], rtol=1e-5, atol=1e-6)
        if s:
            # --spherify: no NDC, world-space rays from the camera centres
            np.testing.assert_array_equal(o, np.broadcast_to(ds.camtoworlds[cam][:, 3], o.shape))
            np.testing.assert_allclose(o, ref[k + "rays_origins"][j], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(d, ref[k + "rays_directions"][j], rtol=1e-5, atol=1e-6)
        else:
            assert np.abs(o - ref[k + "ndc64_origins"][j]).max() <= 4 * e
            assert np.abs(d - ref[k + "ndc64_directions"][j]).max() <= 4 * e
            assert np.abs(o - ref[k + "rays_origins"][j]).max() <= 5 * e
            assert np.abs(d - ref[k + "rays_directions"][j]).max() <= 5 * e


@pytest.mark.parametrize("s,f", [(0, 0), (0, 2), (1, 0), (1, 2)])
def test_render_path_iterates_the_camera_path_without_ground_truth(ref, s, f):
    k = _key("test", s, f, 8)
    ds = _dataset("test", s, f, 8, render_path=True)
    assert ds.size == 120
    e = max(float(ref["e_ref_origins"]), float(ref["e_ref_directions"]))
    first = next(ds)
    assert set(first) == {"rays"} and set(ds.peek()) == {"rays"}       # nothing a pixels-based metric could use
    assert first["rays"].origins.shape == (ds.h, ds.w, 3)
    for j, pose in enumerate(ref["render_ray_poses"]):
        o, d, v = [r.reshape(-1, 3).numpy() for r in ds.get_image(int(pose))["rays"]]
        np.testing.assert_allclose(v, ref[k + "render_rays_viewdirs"][j], rtol=1e-5, atol=1e-6)
        if s:
            np.testing.assert_allclose(o, ref[k + "render_rays_origins"][j], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(d, ref[k + "render_rays_directions"][j], rtol=1e-5, atol=1e-6)
        else:
            assert np.abs(o - ref[k + "ndc64_render_origins"][j]).max() <= 4 * e
            assert np.abs(d - ref[k + "ndc64_render_directions"][j]).max() <= 4 * e
            assert np.abs(o - ref[k + "render_rays_origins"][j]).max() <= 5 * e
            assert np.abs(d - ref[k + "render_rays_directions"][j]).max() <= 5 * e
    # the iterator wraps around after the 120 poses
    ds.it = 119
    next(ds)
    assert ds.it == 0


@pytest.mark.parametrize("s", [0, 1])
def test_training_batches_are_rows_of_the_image_rays(s):
    seed, B = 20201473, 37
    ds = _dataset("train", s, 0, 8, batch_size=B, seed=seed)
    rs_img, rs_pix = np.random.RandomState(seed), np.random.RandomState(seed)
    for _ in range(3):
        batch = next(ds)
        cam = int(rs_img.randint(0, ds.size))
        ids = rs_pix.randint(0, ds.h * ds.w, (B,))
        full = ds.get_image(cam)
        assert torch.equal(batch["pixels"], full["pixels"].reshape(-1, 3)[ids])
        for got, want in zip(batch["rays"], full["rays"]):
            assert torch.equal(got, want.reshape(-1, 3)[ids])
        if not s:
            assert torch.all((batch["rays"].origins[:, 2] + 1.0).abs() < 2e-6)


def test_image_batching_draws_ndc_rays_of_all_images():
    seed, B = 7, 64
    ds = _dataset("train", 0, 2, 8, batch_size=B, seed=seed, image_batching=True)
    batch = next(ds)
    hw = ds.h * ds.w
    ids = np.random.RandomState(seed).randint(0, ds.size * hw, (B,))
    assert len(set(ids // hw)) > 1
    for row, i in enumerate(ids):
        full = ds.get_image(int(i // hw))
        assert torch.equal(batch["pixels"][row], full["pixels"].reshape(-1, 3)[i % hw])
        for got, want in zip(batch["rays"], full["rays"]):
            # not bit-equal: the stand-in's torch matmul rounds differently for a different number of rows (the device kernel
            # computes every ray alone; tests/test_gpu_llff.py asks it for equality)
            np.testing.assert_allclose(got[row].numpy(), want.reshape(-1, 3)[i % hw].numpy(), rtol=0, atol=2e-6)


def test_shards_are_contiguous_rows_of_the_unsharded_batch():
    B, world = 16, 4
    whole = _dataset("train", 0, 0, 8, batch_size=B * world, seed=11)
    shards = [_dataset("train", 0, 0, 8, batch_size=B, seed=11, shard=(r, world)) for r in range(world)]
    for _ in range(3):
        want = next(whole)
        for r, d in enumerate(shards):
            got = next(d)
            assert torch.equal(got["pixels"], want["pixels"][r * B:(r + 1) * B])
            for a, b in zip(got["rays"], want["rays"]):
                assert torch.equal(a, b[r * B:(r + 1) * B])


def test_flags():
    a = _args()
    utils.check_flags(a)
    assert (a.dataset, a.white_bkgd, a.near, a.far, a.use_viewdirs, a.sh_deg, a.noise_std, a.lindisp) == \
        ("llff", False, 0.0, 1.0, False, 3, 1.0, False)
    assert _args().factor == 0 and utils.define_flags().parse_args(["--config", "llff"]).factor == 4
    b = utils.define_flags().parse_args(["--config", "llff"]); utils.update_flags(b)
    assert b.factor == 4
    blender = utils.define_flags().parse_args(["--config", "blender"]); utils.update_flags(blender)
    for key in ("num_coarse_samples", "num_fine_samples", "batch_size", "randomized", "max_steps", "image_batching"):
        assert getattr(b, key) == getattr(blender, key), key
    # the LLFF flags take effect with the LLFF dataset ...
    utils.check_flags(_args(render_path=True))
    utils.check_flags(_args(spherify=True))
    # ... and are refused with any other, as before
    for over in (dict(render_path=True), dict(spherify=True)):
        for name in ("blender", "nsvf", "synthetic"):
            with pytest.raises(NotImplementedError, match="LLFF"):
                utils.check_flags(_args(dataset=name, **over))
    # SG models and the view-conditioned head stay refused on LLFF scenes, by name
    sg_args = _args(sg_dim=4, sh_deg=-1)
    assert any("llff" in m for m in utils.unbuilt_flags(sg_args, families.SG.checks["train"][1]))
    with pytest.raises(NotImplementedError, match="LLFF"):
        families.check(sg_args, "train")
    with pytest.raises(NotImplementedError, match="LLFF"):
        families.check(_args(sg_dim=4, sh_deg=-1, dataset="blender", render_path=True), "render")
    vd_args = viewdirs.add_checkpoint_flags(utils.define_flags()).parse_args(["--config", "llff", "--train_dir", "x", "--data_dir", TINY])
    utils.update_flags(vd_args)
    vd_args.use_viewdirs, vd_args.sh_deg = True, -1
    with pytest.raises(NotImplementedError, match="LLFF"):
        families.check(vd_args, "render")
    with pytest.raises(NotImplementedError, match="use_viewdirs"):
        utils.check_flags(_args(use_viewdirs=True))
    # the plain dataset table still refuses llff: the octree entry points, which call it, do not build these scenes
    assert "llff" not in datasets.dataset_dict
    with pytest.raises(NotImplementedError, match="llff"):
        datasets.get_dataset("train", a, CPU)
    # every other dataset goes through llff.get_dataset unchanged
    syn = utils.define_flags().parse_args(["--config", "blender", "--train_dir", "x", "--dataset", "synthetic"])
    utils.update_flags(syn); syn.dataset = "synthetic"; syn.factor = 8
    assert type(llff.get_dataset("test", syn, CPU)) is datasets.Synthetic
