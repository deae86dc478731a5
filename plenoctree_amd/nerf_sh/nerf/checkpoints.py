"""Checkpoint save/restore in the flax msgpack format of the reference.

The reference saves `flax.training.checkpoints.save_checkpoint(train_dir, state, step, keep=200)`
(nerf_sh/train.py:240-242, 306-310) and reads the files back in three places: resume
(nerf_sh/nerf/models.py:46-48), eval (nerf_sh/eval.py:70) and the PlenOctree extraction, whose
consumer fixes the key names: ckpt["optimizer"]["target"]["params"]["MLP_i"]["Dense_j"]{"kernel",
"bias"} with kernels [in,out] (octree/nerf/models.py:75-102).

flax (>=0.3.1, environment.yml:19) is a third-party dependency that is not installed here; its
published serialisation (flax/serialization.py) is restated: the file `checkpoint_<step>` is
msgpack of the nested state dict, every ndarray leaf packed as ExtType(1, msgpack((shape, dtype
name, C-order bytes))).  State dict of TrainState(optimizer=flax.optim.Optimizer):
  {"optimizer": {"target": {"params": ...},
                 "state": {"step": int32 scalar,
                           "param_states": {"params": <same tree>{"grad_ema", "grad_sq_ema"}}}}}
Unverified against a live flax (none available); tests/test_checkpoint_cpu.py drives the
reference's own consumer code with these files instead.

A NeRF-SG (sg_dim > 0) carries two more leaves beside MLP_0 / MLP_1, `sg_lambda` [K] and `sg_mu_spher` [K,2]
(nerf_sh/nerf/models.py:107-117; top-level keys of the torch twin's state dict, octree/nerf/models.py:104-107).  They are
read and written for the states of nerf.sg only; any other model refuses a file that holds them, by the key's name.  In the
flax format their Adam moments travel like the MLPs': param_states/params/sg_lambda|sg_mu_spher/{grad_ema, grad_sq_ema}, the
shape of the leaf (nerf_sh.train optimises them, so a resumed NeRF-SG run continues its trajectory); a file without them --
one written before NeRF-SG training existed, or a foreign one -- loads with zero moments, and a torch state dict carries none.
"""
import glob
import os
import re

import msgpack
import numpy as np
import torch

_EXT_NDARRAY = 1
_EXT_NPSCALAR = 3


def _pack_ndarray(arr):
    arr = np.ascontiguousarray(arr)
    return msgpack.packb((list(arr.shape), arr.dtype.name, arr.tobytes("C")), use_bin_type=True)


def _ext_pack(x):
    if isinstance(x, np.ndarray):
        return msgpack.ExtType(_EXT_NDARRAY, _pack_ndarray(x))
    if isinstance(x, np.generic):
        return msgpack.ExtType(_EXT_NPSCALAR, _pack_ndarray(np.asarray(x)))
    raise TypeError(f"cannot serialise {type(x)}")


def _ext_unpack(code, data):
    if code in (_EXT_NDARRAY, _EXT_NPSCALAR):
        shape, dtype_name, buf = msgpack.unpackb(data, raw=False)
        arr = np.frombuffer(buf, dtype=np.dtype(dtype_name)).reshape(shape).copy()
        return arr[()] if code == _EXT_NPSCALAR else arr
    return msgpack.ExtType(code, data)


def msgpack_serialize(tree):
    return msgpack.packb(tree, default=_ext_pack, strict_types=True)


def msgpack_restore(blob):
    return msgpack.unpackb(blob, ext_hook=_ext_unpack, raw=False)


def _leaves(cfg):
    from ... import ops
    return ops.param_layout(cfg)


def arena_to_tree(flat, cfg):
    """flat 2-MLP arena (numpy) -> {"MLP_0": {"Dense_0": {"kernel": [in,out], "bias": [out]}, ...}, "MLP_1": ...}"""
    leaves, n = _leaves(cfg)
    tree = {}
    for mi in range(2):
        mlp = {}
        for layer, is_bias, off, rows, cols in leaves:
            d = mlp.setdefault(f"Dense_{layer}", {})
            a = flat[mi * n + off: mi * n + off + rows * cols]
            d["bias" if is_bias else "kernel"] = a.copy() if is_bias else a.reshape(rows, cols).copy()
        tree[f"MLP_{mi}"] = mlp
    return tree


def tree_to_arena(tree, cfg, leaf=None):
    """Inverse of arena_to_tree; `leaf` picks a sub-key (e.g. "grad_ema") of every array leaf."""
    leaves, n = _leaves(cfg)
    flat = np.zeros(2 * n, np.float32)
    for mi in range(2):
        for layer, is_bias, off, rows, cols in leaves:
            a = tree[f"MLP_{mi}"][f"Dense_{layer}"]["bias" if is_bias else "kernel"]
            if leaf is not None:
                a = a[leaf]
            a = np.asarray(a, np.float32)
            want = (rows,) if is_bias else (rows, cols)
            if tuple(a.shape) != want:
                raise ValueError(f"checkpoint leaf MLP_{mi}/Dense_{layer} has shape {a.shape}, expected {want}")
            flat[mi * n + off: mi * n + off + rows * cols] = a.reshape(-1)
    return flat


def state_to_tree(state):
    p = state.params.detach().cpu().numpy()
    m = state.m.detach().cpu().numpy()
    v = state.v.detach().cpu().numpy()
    params = arena_to_tree(p, state.cfg)
    mt, vt = arena_to_tree(m, state.cfg), arena_to_tree(v, state.cfg)
    pstates = {mk: {dk: {lk: {"grad_ema": mt[mk][dk][lk], "grad_sq_ema": vt[mk][dk][lk]} for lk in dv}
                    for dk, dv in mv.items()} for mk, mv in params.items()}
    if _is_sg(state):
        # the two model-level parameters of a NeRF-SG (nerf_sh/nerf/models.py:107-117), beside MLP_0 / MLP_1, with their Adam
        # moments in the same tree shape
        ms, vs = state.sg_moments()
        for i, k in enumerate(_SG_KEYS):
            a = getattr(state, k).detach().cpu().numpy().astype(np.float32)
            params[k] = a
            pstates[k] = {"grad_ema": ms[i].numpy().astype(np.float32).reshape(a.shape),
                          "grad_sq_ema": vs[i].numpy().astype(np.float32).reshape(a.shape)}
    return {"optimizer": {"target": {"params": params},
                          "state": {"step": np.asarray(state.step, np.int32), "param_states": {"params": pstates}}}}


_SG_KEYS = ("sg_lambda", "sg_mu_spher")


def _is_sg(state):
    """A state of nerf.sg (sg_dim > 0): it carries sg_lambda / sg_mu_spher and takes them through set_lobe_params."""
    return hasattr(state, "set_lobe_params")


def _load_sg_keys(get, has, state, where, moments=None):
    """The SG keys of a checkpoint into an SG state; a non-SG state refuses them and an SG state requires them, by name.
    `moments`: the param_states tree of a flax checkpoint; SG leaves without moments there load with zeros."""
    present = [k for k in _SG_KEYS if has(k)]
    if not _is_sg(state):
        if present:
            raise ValueError(f"{where}: key {present[0]!r}: a spherical-Gaussian model; this model has sg_dim <= 0 "
                             "(pass --sg_dim K --sh_deg -1)")
        return
    if len(present) != len(_SG_KEYS):
        missing = [k for k in _SG_KEYS if k not in present]
        raise ValueError(f"{where}: no {missing[0]!r}: not a NeRF-SG checkpoint (the model has sg_dim={state.sg_dim})")
    lam, mu = (np.asarray(get(k).detach().cpu() if torch.is_tensor(get(k)) else get(k), np.float32) for k in _SG_KEYS)
    K = state.sg_dim
    if lam.shape != (K,) or mu.shape != (K, 2):
        raise ValueError(f"{where}: sg_lambda {lam.shape} / sg_mu_spher {mu.shape}, the model (sg_dim={K}) needs ({K},) / ({K}, 2)")
    mv = [None, None]
    if moments is not None and all(isinstance(moments.get(k), dict) for k in _SG_KEYS):
        for i, leaf in enumerate(("grad_ema", "grad_sq_ema")):
            parts = [moments[k].get(leaf) for k in _SG_KEYS]
            if all(p is not None for p in parts):
                parts = [np.asarray(p, np.float32) for p in parts]
                if parts[0].shape != (K,) or parts[1].shape != (K, 2):
                    raise ValueError(f"{where}: {leaf} of sg_lambda {parts[0].shape} / sg_mu_spher {parts[1].shape}, the model "
                                     f"(sg_dim={K}) needs ({K},) / ({K}, 2)")
                mv[i] = torch.from_numpy(np.concatenate([parts[0], parts[1].reshape(-1)]))
    state.set_lobe_params(torch.from_numpy(lam), torch.from_numpy(mu), *mv)


def load_tree_into_state(tree, state):
    opt = tree["optimizer"]
    params = opt["target"]["params"]
    dev = state.params.device
    ps = opt.get("state", {}).get("param_states", {}).get("params")
    _load_sg_keys(params.__getitem__, params.__contains__, state, "flax checkpoint", ps)
    state.params.copy_(torch.from_numpy(tree_to_arena(params, state.cfg)).to(dev))
    if ps is not None:
        state.m.copy_(torch.from_numpy(tree_to_arena(ps, state.cfg, "grad_ema")).to(dev))
        state.v.copy_(torch.from_numpy(tree_to_arena(ps, state.cfg, "grad_sq_ema")).to(dev))
    state.step = int(np.asarray(opt.get("state", {}).get("step", 0)).reshape(-1)[0])
    state.repack()


def _step_of(path):
    m = re.search(r"checkpoint_(\d+)$", path)
    return int(m.group(1)) if m else -1


def latest_checkpoint(train_dir):
    paths = [p for p in glob.glob(os.path.join(train_dir, "checkpoint_*")) if _step_of(p) >= 0]
    return max(paths, key=_step_of) if paths else None


def save_checkpoint(train_dir, state, step, keep=200):
    """flax.training.checkpoints.save_checkpoint(train_dir, state, step, keep)."""
    os.makedirs(train_dir, exist_ok=True)
    path = os.path.join(train_dir, f"checkpoint_{int(step)}")
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(msgpack_serialize(state_to_tree(state)))
    os.replace(tmp, path)
    paths = sorted((p for p in glob.glob(os.path.join(train_dir, "checkpoint_*")) if _step_of(p) >= 0), key=_step_of)
    for old in paths[:-keep]:
        os.remove(old)
    return path


def restore_checkpoint(train_dir, state=None):
    """flax.training.checkpoints.restore_checkpoint: newest `checkpoint_<step>` in train_dir (or the
    file itself).  With `state` the arrays are loaded in place and the path is returned (None if
    there is no checkpoint); with state=None the raw state dict is returned (flax's target=None)."""
    path = train_dir if os.path.isfile(train_dir) else latest_checkpoint(train_dir)
    if path is None:
        return None
    with open(path, "rb") as f:
        tree = msgpack_restore(f.read())
    if state is None:
        return tree
    load_tree_into_state(tree, state)
    return path


# ---- the reference's OTHER checkpoint format: a torch state dict of its torch twin ------------------------------------------
def torch_state_dict_to_tree(sd, depth=8, sg=False):
    """`ckpt["model"]` of octree/nerf/models.py:52-63 (restore_model_state: `*.ckpt` files holding the state dict of the torch
    NerfModel, whose Linear weights are [out, in]) as the flax params tree: the inverse of the key map the reference applies to
    a flax checkpoint (octree/nerf/models.py:79-102: Dense_i -> input_layers.i for i < net_depth, then sigma_layer, then --
    without view directions -- rgb_layer; kernel = weight.T)."""
    names = [f"input_layers.{i}" for i in range(depth)] + ["sigma_layer", "rgb_layer"]
    for k in sd:
        if sg and k in _SG_KEYS:           # a NeRF-SG state (octree/nerf/models.py:104-107): read by restore_torch_checkpoint
            continue
        if any(t in k for t in ("bottleneck_layer", "condition_layers", "sg_lambda", "sg_mu_spher")):
            raise ValueError(f"torch checkpoint key {k!r}: the view-conditioned head / SG basis is not built on the MI355X path "
                             "(use_viewdirs=false SH models only)")
    tree = {}
    for mi in range(2):
        mlp = {}
        for li, name in enumerate(names):
            wk, bk = f"MLP_{mi}.{name}.weight", f"MLP_{mi}.{name}.bias"
            if wk not in sd or bk not in sd:
                raise ValueError(f"torch checkpoint has no {wk} / {bk}")
            w = sd[wk].detach().cpu().numpy() if hasattr(sd[wk], "detach") else np.asarray(sd[wk])
            b = sd[bk].detach().cpu().numpy() if hasattr(sd[bk], "detach") else np.asarray(sd[bk])
            mlp[f"Dense_{li}"] = {"kernel": np.ascontiguousarray(w.T.astype(np.float32)), "bias": b.astype(np.float32)}
        tree[f"MLP_{mi}"] = mlp
    return tree


def torch_state_dict_from_state(state):
    """The torch twin's state dict (Linear weights [out,in]; plus sg_lambda / sg_mu_spher for a NeRF-SG, octree/nerf/models.py:
    198-210) of a TrainState: what a `*.ckpt` of the reference holds under "model"."""
    tree = arena_to_tree(state.params.detach().cpu().numpy(), state.cfg)
    depth = len(tree["MLP_0"]) - 2
    names = [f"input_layers.{i}" for i in range(depth)] + ["sigma_layer", "rgb_layer"]
    sd = {}
    for mi in range(2):
        for li, name in enumerate(names):
            d = tree[f"MLP_{mi}"][f"Dense_{li}"]
            sd[f"MLP_{mi}.{name}.weight"] = torch.from_numpy(np.ascontiguousarray(d["kernel"].T))
            sd[f"MLP_{mi}.{name}.bias"] = torch.from_numpy(d["bias"].copy())
    if _is_sg(state):
        for k in _SG_KEYS:
            sd[k] = getattr(state, k).detach().cpu().clone()
    return sd


def latest_torch_checkpoint(train_dir):
    paths = sorted(glob.glob(os.path.join(train_dir, "*.ckpt")))       # octree/nerf/models.py:56-59: sorted, last one
    return paths[-1] if paths else None


def restore_torch_checkpoint(train_dir, state, trust_pickle=False):
    """restore_model_state (octree/nerf/models.py:52-63): the newest `*.ckpt` of train_dir into `state` (parameters only; a
    state dict carries no optimizer moments).  Returns the path, or None when there is no such file.  The file is read with
    weights_only=True; one that also holds non-tensor objects needs trust_pickle=True (the reference's plain torch.load)."""
    path = train_dir if os.path.isfile(train_dir) else latest_torch_checkpoint(train_dir)
    if path is None:
        return None
    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:            # pickle.UnpicklingError and friends: non-tensor extras (argparse.Namespace, numpy scalars)
        if not trust_pickle:
            raise ValueError(
                f"{path}: holds more than tensors ({type(e).__name__}: {str(e).splitlines()[0][:200]}).  The reference loads its "
                "*.ckpt files with a plain torch.load, i.e. it unpickles arbitrary objects; this loader does that only when "
                "asked to: restore_torch_checkpoint(..., trust_pickle=True) / --trust_ckpt_pickle true, for files you trust") from e
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(ckpt, dict) or "model" not in ckpt:
        raise ValueError(f'{path}: not a checkpoint of the reference\'s torch twin (no "model" state dict)')
    from ... import _lib
    params = torch_state_dict_to_tree(ckpt["model"], depth=_lib.NET_DEPTH, sg=_is_sg(state))   # the depth the kernels (and state.cfg's arena) are built for
    if _is_sg(state):
        _load_sg_keys(ckpt["model"].__getitem__, ckpt["model"].__contains__, state, path)
    state.params.copy_(torch.from_numpy(tree_to_arena(params, state.cfg)).to(state.params.device))
    state.m.zero_(); state.v.zero_()
    state.repack()
    return path


# ---- view-conditioned NeRF (use_viewdirs = true), read for extraction by SH projection --------------------------------------
# Both formats the reference reads for such a model (octree/nerf/models.py:52-113): the torch twin's state dict (MLP_i.
# input_layers.j, sigma_layer, bottleneck_layer, condition_layers.0, rgb_layer; Linear weights [out,in]) and the flax / JaxNeRF
# msgpack tree (Dense_0..11, kernels [in,out]).
_VD_TORCH_NAMES = ([f"input_layers.{i}" for i in range(8)] +
                   ["sigma_layer", "bottleneck_layer", "condition_layers.0", "rgb_layer"])


def _vd_leaves():
    from ... import ops
    return ops.vd_param_layout()


def vd_arena_to_tree(flat):
    """flat 2-MLP arena (numpy) of a view-conditioned model -> {"MLP_i": {"Dense_j": {"kernel": [in,out], "bias": [out]}}}."""
    leaves, n = _vd_leaves()
    tree = {}
    for mi in range(2):
        mlp = {}
        for layer, is_bias, off, rows, cols in leaves:
            d = mlp.setdefault(f"Dense_{layer}", {})
            a = flat[mi * n + off: mi * n + off + rows * cols]
            d["bias" if is_bias else "kernel"] = a.copy() if is_bias else a.reshape(rows, cols).copy()
        tree[f"MLP_{mi}"] = mlp
    return tree


def vd_tree_to_arena(tree, where="checkpoint"):
    """Inverse of vd_arena_to_tree.  A tree whose shapes are not those of the view-conditioned model raises a ValueError that names
    the first leaf that does not fit (and says so when the shapes are an SH model's)."""
    leaves, n = _vd_leaves()
    flat = np.zeros(2 * n, np.float32)
    for mi in range(2):
        mlp = tree.get(f"MLP_{mi}")
        if mlp is None:
            raise ValueError(f"{where}: no MLP_{mi} in the parameter tree")
        for layer, is_bias, off, rows, cols in leaves:
            name = f"MLP_{mi}/Dense_{layer}/{'bias' if is_bias else 'kernel'}"
            dense = mlp.get(f"Dense_{layer}")
            if dense is None or ("bias" if is_bias else "kernel") not in dense:
                hint = " (Dense_0..9 only: a use_viewdirs=false SH model; extract it without --use_viewdirs)" if layer >= 10 else ""
                raise ValueError(f"{where}: leaf {name} is missing{hint}")
            a = np.asarray(dense["bias" if is_bias else "kernel"], np.float32)
            want = (rows,) if is_bias else (rows, cols)
            if tuple(a.shape) != want:
                raise ValueError(f"{where}: leaf {name} has shape {tuple(a.shape)}, the view-conditioned model "
                                 f"(use_viewdirs=true, net_width_condition 128, deg_view 4) needs {want}")
            flat[mi * n + off: mi * n + off + rows * cols] = a.reshape(-1)
    return flat


def vd_torch_state_dict_to_tree(sd, where="torch checkpoint"):
    """The torch twin's state dict of a use_viewdirs=True model as the flax tree (the inverse of octree/nerf/models.py:79-102:
    Dense_i -> input_layers.i, sigma_layer, bottleneck_layer, condition_layers.0, rgb_layer; kernel = weight.T)."""
    for k in sd:
        if "sg_lambda" in k or "sg_mu_spher" in k:
            raise ValueError(f"{where}: key {k!r}: the SG basis is not built on the MI355X path")
        if "condition_layers." in k and "condition_layers.0." not in k:
            raise ValueError(f"{where}: key {k!r}: net_depth_condition must be 1")
    tree = {}
    for mi in range(2):
        mlp = {}
        for li, name in enumerate(_VD_TORCH_NAMES):
            wk, bk = f"MLP_{mi}.{name}.weight", f"MLP_{mi}.{name}.bias"
            if wk not in sd or bk not in sd:
                hint = " (no view-conditioned head: a use_viewdirs=false SH model)" if li >= 9 else ""
                raise ValueError(f"{where}: leaf {wk} / {bk} is missing{hint}")
            w = sd[wk].detach().cpu().numpy() if hasattr(sd[wk], "detach") else np.asarray(sd[wk])
            b = sd[bk].detach().cpu().numpy() if hasattr(sd[bk], "detach") else np.asarray(sd[bk])
            mlp[f"Dense_{li}"] = {"kernel": np.ascontiguousarray(w.T.astype(np.float32)), "bias": b.astype(np.float32)}
        tree[f"MLP_{mi}"] = mlp
    return tree


def vd_state_dict_from_arena(flat):
    """The torch twin's state dict (weights [out,in]) of a flat view-conditioned arena: what its `*.ckpt` holds under "model"."""
    tree = vd_arena_to_tree(np.asarray(flat, np.float32))
    sd = {}
    for mi in range(2):
        for li, name in enumerate(_VD_TORCH_NAMES):
            d = tree[f"MLP_{mi}"][f"Dense_{li}"]
            sd[f"MLP_{mi}.{name}.weight"] = torch.from_numpy(np.ascontiguousarray(d["kernel"].T))
            sd[f"MLP_{mi}.{name}.bias"] = torch.from_numpy(d["bias"].copy())
    return sd


def load_viewdirs_arena(train_dir, is_jaxnerf_ckpt=False, trust_pickle=False):
    """(flat arena as numpy, path, format) of the newest checkpoint of a view-conditioned model in train_dir, chosen like
    extraction.load_nerf_checkpoint chooses for SH models: `*.ckpt` torch state dict first unless is_jaxnerf_ckpt, else the flax
    msgpack `checkpoint_<step>`."""
    if not is_jaxnerf_ckpt:
        path = train_dir if os.path.isfile(train_dir) and train_dir.endswith(".ckpt") else latest_torch_checkpoint(train_dir)
        if path is not None:
            try:
                ckpt = torch.load(path, map_location="cpu", weights_only=True)
            except Exception as e:
                if not trust_pickle:
                    raise ValueError(f"{path}: holds more than tensors ({type(e).__name__}); pass --trust_ckpt_pickle true for "
                                     "files you trust") from e
                ckpt = torch.load(path, map_location="cpu", weights_only=False)
            if not isinstance(ckpt, dict) or "model" not in ckpt:
                raise ValueError(f'{path}: not a checkpoint of the reference\'s torch twin (no "model" state dict)')
            return vd_tree_to_arena(vd_torch_state_dict_to_tree(ckpt["model"], path), path), path, "torch state dict"
    path = train_dir if os.path.isfile(train_dir) else latest_checkpoint(train_dir)
    if path is None:
        raise FileNotFoundError(f"no *.ckpt (torch state dict) and no checkpoint_<step> (flax msgpack) in {train_dir}")
    with open(path, "rb") as f:
        tree = msgpack_restore(f.read())
    return vd_tree_to_arena(tree["optimizer"]["target"]["params"], path), path, "flax msgpack"


def restore_viewdirs_checkpoint(train_dir, state, is_jaxnerf_ckpt=False, trust_pickle=False):
    flat, path, fmt = load_viewdirs_arena(train_dir, is_jaxnerf_ckpt, trust_pickle)
    state.params.copy_(torch.from_numpy(flat).to(state.params.device))
    state.repack()
    return f"* restore ckpt from {path} ({fmt}, view-conditioned head)"
