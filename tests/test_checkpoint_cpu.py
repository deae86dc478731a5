"""flax-msgpack checkpoint interop, CPU only.

The files written by plenoctree_amd.nerf_sh.nerf.checkpoints were fed to the REFERENCE's own
consumer, octree/nerf/models.py:restore_model_state_from_jaxnerf, through a stand-in `flax.training.checkpoints`
module that only wraps our msgpack reader; tests/golden/reference_consumers.npz (make_golden_consumers.py) holds
what the torch NerfModel it filled evaluates, and the hash of the file it read.  That twin must reproduce the
oracle's eval_points_raw on the same parameters, and the file written here must be the one it read."""
import hashlib
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from plenoctree_amd import _lib
from plenoctree_amd.nerf_sh.nerf import checkpoints


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "reference_consumers.npz"))


def _twin_state_dict(golden_dir, z):
    """The torch twin's state dict of the fixture: its keys and shapes, the contents make_golden_consumers.py gave it."""
    sys.path.insert(0, golden_dir)
    try:
        from make_golden_consumers import twin_state_dict
    finally:
        sys.path.remove(golden_dir)
    shapes = [tuple(int(n) for n in s[:d]) for s, d in zip(z["twin_shapes"], z["twin_ndim"])]
    return twin_state_dict([str(k) for k in z["twin_keys"]], shapes)


class _State:
    """TrainState stand-in without GPU kernels (repack is a no-op)."""

    def __init__(self, cfg, flat, step=0):
        self.cfg, self.params, self.step = cfg, flat.clone(), step
        self.m = torch.zeros_like(flat); self.v = torch.zeros_like(flat)

    def repack(self):
        pass


def _flat(deg, seed=3):
    ocfg = O.Cfg(sh_deg=deg)
    flat = O.flatten_params(O.init_params(ocfg, seed=seed))
    return ocfg, flat + 0.01 * torch.randn(flat.shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("deg", [3, 4])
def test_roundtrip_and_tree_layout(tmp_path, deg):
    ocfg, flat = _flat(deg)
    cfg = _lib.make_cfg(sh_deg=deg)
    st = _State(cfg, flat, step=1234)
    st.m = torch.rand_like(flat); st.v = torch.rand_like(flat)
    path = checkpoints.save_checkpoint(str(tmp_path), st, 1234)
    assert os.path.basename(path) == "checkpoint_1234"
    raw = checkpoints.restore_checkpoint(str(tmp_path))            # target=None -> raw state dict
    params = raw["optimizer"]["target"]["params"]
    assert sorted(params) == ["MLP_0", "MLP_1"] and sorted(params["MLP_0"]) == [f"Dense_{i}" for i in range(10)]
    shapes = O.layer_shapes(ocfg)
    oparams = O.unflatten_params(flat, ocfg)
    for mi in range(2):
        for li, (fi, fo) in enumerate(shapes):
            k = params[f"MLP_{mi}"][f"Dense_{li}"]["kernel"]
            assert k.shape == (fi, fo) and k.dtype == np.float32
            np.testing.assert_array_equal(k, oparams[mi][li][0].numpy())
            np.testing.assert_array_equal(params[f"MLP_{mi}"][f"Dense_{li}"]["bias"], oparams[mi][li][1].numpy())
    assert int(raw["optimizer"]["state"]["step"]) == 1234
    ps = raw["optimizer"]["state"]["param_states"]["params"]["MLP_1"]["Dense_5"]["kernel"]
    assert sorted(ps) == ["grad_ema", "grad_sq_ema"] and ps["grad_ema"].shape == (319, 256)
    fresh = _State(cfg, torch.zeros_like(flat))
    assert checkpoints.restore_checkpoint(str(tmp_path), fresh) == path
    assert torch.equal(fresh.params, st.params) and torch.equal(fresh.m, st.m) and torch.equal(fresh.v, st.v)
    assert fresh.step == 1234
    # keep=N retention
    for s in (2000, 3000):
        checkpoints.save_checkpoint(str(tmp_path), st, s, keep=2)
    assert sorted(os.listdir(tmp_path)) == ["checkpoint_2000", "checkpoint_3000"]
    bad = _State(_lib.make_cfg(sh_deg=7 - deg), torch.zeros(2 * {3: 512588, 4: 505649}[deg]))
    with pytest.raises(ValueError):
        checkpoints.restore_checkpoint(str(tmp_path), bad)


def test_reference_consumer_reads_our_checkpoint(tmp_path, golden_dir):
    z = _golden(golden_dir)
    ocfg, flat = _flat(3, seed=11)
    st = _State(_lib.make_cfg(sh_deg=3), flat, step=77)
    path = checkpoints.save_checkpoint(str(tmp_path), st, 77)
    # byte for byte the file the reference's restore_model_state_from_jaxnerf (octree/nerf/models.py:66-113) read
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == str(z["ckpt_file_sha256"])
    pts = (torch.rand(50, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 1.5
    rgb, sigma, rgb_c, sigma_c = (torch.from_numpy(z[k]) for k in ("ckpt_rgb", "ckpt_sigma", "ckpt_rgb_c", "ckpt_sigma_c"))
    params = O.unflatten_params(flat, ocfg)
    o_rgb, o_sigma = O.eval_points_raw(params, pts, ocfg)
    o_rgb_c, o_sigma_c = O.eval_points_raw(params, pts, ocfg, coarse=True)
    np.testing.assert_allclose(rgb.numpy(), o_rgb.numpy(), atol=2e-6)
    np.testing.assert_allclose(sigma.numpy(), o_sigma.numpy(), atol=2e-6)
    np.testing.assert_allclose(rgb_c.numpy(), o_rgb_c.numpy(), atol=2e-6)
    np.testing.assert_allclose(sigma_c.numpy(), o_sigma_c.numpy(), atol=2e-6)


def test_torch_state_dict_checkpoint_of_the_reference_twin(tmp_path, golden_dir):
    """The reference's OTHER input format (octree/nerf/models.py:52-63, taken without --is_jaxnerf_ckpt): `*.ckpt` =
    {"model": state_dict of its torch NerfModel}.  The state dict has the twin's keys and shapes, and the twin's
    eval_points_raw on it is in tests/golden/reference_consumers.npz (make_golden_consumers.py); our reader must
    fill the arena so that the oracle reproduces those outputs, and extraction's loader must pick the format the
    way the reference's flag does -- and refuse to go on with random weights when there is nothing to read."""
    z = _golden(golden_dir)
    sd = _twin_state_dict(golden_dir, z)
    torch.save({"model": sd}, str(tmp_path / "000100.ckpt"))
    torch.save({"model": {k: torch.zeros_like(v) for k, v in sd.items()}}, str(tmp_path / "000050.ckpt"))
    ocfg = O.Cfg(sh_deg=3)
    st = _State(_lib.make_cfg(sh_deg=3), torch.zeros(2 * 505649))
    st.m += 1.0
    path = checkpoints.restore_torch_checkpoint(str(tmp_path), st)
    assert os.path.basename(path) == "000100.ckpt" and float(st.m.abs().max()) == 0.0        # sorted()[-1]; no stale moments
    # a file that also holds non-tensor objects (the reference's plain torch.load would unpickle them): refused with a message
    # that names the way out, read with trust_pickle=True
    import argparse
    extra = tmp_path / "extra"; extra.mkdir()
    torch.save({"model": sd, "args": argparse.Namespace(lr=5e-4)}, str(extra / "000200.ckpt"))
    with pytest.raises(ValueError, match="trust_pickle=True"):
        checkpoints.restore_torch_checkpoint(str(extra), st)
    p0 = st.params.clone()
    assert checkpoints.restore_torch_checkpoint(str(extra), st, trust_pickle=True).endswith("000200.ckpt")
    assert torch.equal(st.params, p0)
    pts = (torch.rand(64, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1) * 1.5
    rgb, sigma, rgb_c, sigma_c = (torch.from_numpy(z[k]) for k in ("twin_rgb", "twin_sigma", "twin_rgb_c", "twin_sigma_c"))
    params = O.unflatten_params(st.params, ocfg)
    o_rgb, o_sigma = O.eval_points_raw(params, pts, ocfg)
    o_rgb_c, o_sigma_c = O.eval_points_raw(params, pts, ocfg, coarse=True)
    np.testing.assert_allclose(rgb.numpy(), o_rgb.numpy(), atol=2e-6)
    np.testing.assert_allclose(sigma.numpy(), o_sigma.numpy(), atol=2e-6)
    np.testing.assert_allclose(rgb_c.numpy(), o_rgb_c.numpy(), atol=2e-6)
    np.testing.assert_allclose(sigma_c.numpy(), o_sigma_c.numpy(), atol=2e-6)
    # extraction's loader: format chosen as the reference's flag does
    from plenoctree_amd.octree import extraction
    a = types.SimpleNamespace(train_dir=str(tmp_path), is_jaxnerf_ckpt=False)
    st2 = _State(_lib.make_cfg(sh_deg=3), torch.zeros(2 * 505649))
    assert "torch state dict" in extraction.load_nerf_checkpoint(a, st2) and torch.equal(st2.params, st.params)
    a.is_jaxnerf_ckpt = True
    with pytest.raises(FileNotFoundError):
        extraction.load_nerf_checkpoint(a, st2)                       # the flag asks for flax; only *.ckpt here
    checkpoints.save_checkpoint(str(tmp_path), _State(_lib.make_cfg(sh_deg=3), st.params + 1.0, step=9), 9)
    assert "flax msgpack" in extraction.load_nerf_checkpoint(a, st2) and torch.equal(st2.params, st.params + 1.0)
    empty = tmp_path / "empty"; empty.mkdir()
    a = types.SimpleNamespace(train_dir=str(empty), is_jaxnerf_ckpt=False)
    with pytest.raises(FileNotFoundError):
        extraction.load_nerf_checkpoint(a, st2)
    # a view-conditioned twin is rejected, not half-loaded
    with pytest.raises(ValueError, match="view-conditioned"):
        checkpoints.torch_state_dict_to_tree({"MLP_0.bottleneck_layer.weight": torch.zeros(1)})
