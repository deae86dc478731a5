"""Host-side mirror of the slice of `svox` the reference uses (N3Tree, VolumeRenderer, helpers) on the MI355X path.

svox (pin svox>=0.2.28) is a third-party dependency of the reference and is not part of its tree; the classes
below keep its names, argument meaning, indexing surface and npz format for exactly the calls the reference makes,
so that the reference's own octree/extraction.py (step1, step2), octree/optimization.py and octree/evaluation.py
run UNCHANGED with `sys.modules["svox"]` pointing here (tests/test_reference_drivers_cpu.py does exactly that):

    N3Tree(N, data_dim, init_refine=0, init_reserve, geom_resize_fact, depth_limit, radius, center, data_format,
           extra_data, map_location)                                               octree/extraction.py:489-499
    tree.offset.cpu(), tree.invradius.cpu()                                        octree/extraction.py:291-292
    tree[grid].refine()         (grid: [n,3] world-space points)                   octree/extraction.py:341-350
    tree.max_depth, tree.depths, tree[leaf_inds].sample(S), tree[leaf_inds] = rgba octree/extraction.py:353-394
    tree.data_format.format == tree.data_format.RGBA, tree.data_dim                octree/extraction.py:377-378
    tree[:, -1:].relu_(), tree.shrink_to_fit(), print(tree), tree.save(path, compress=False)   :503-509
    svox.N3Tree.load(path, map_location), t.parameters(), t.data.dtype / .grad / .device, t.clone(device='cpu')
                                                                                   octree/optimization.py:167-240
    svox.VolumeRenderer(t, step_size, ndc).render_persp(c2w, height, width, fx, fast, cuda)
                                                                  octree/nerf/utils.py:456-474, octree/optimization.py:174-216
    svox.NDCConfig(width, height, focal)                          octree/nerf/utils.py:456-459, octree/optimization.py:170-173
                                                                  (LLFF scenes: the tree lives in the NDC cube, see VolumeRenderer)
    svox.helpers._get_c_extension(): RenderOptions(), CameraSpec(), grid_weight_render(...)    octree/extraction.py:181-214
    with tree.accumulate_weights(op) as accum: ...; accum.value      no call site in the reference: svox's published interface
                                                                  (octree/pruning.py here); prune_ / refine_leaves are additions

Two ways to build a tree: the generic `tree[points].refine()` above (leaf lookup in HIP, structure edits as tensor
index operations, as svox itself does them), and `refine_from_mask` -- the whole init_grid_depth refinement of the
masked grid in one pass (Morton pyramid + scans, 0.3 ms at 512^3), which our own extraction driver uses; with whole
levels refined per call both produce the same arrays (tests/test_gpu_octree.py).

Storage and node order are svox's (include/plenoctree_octree.h).  Rendering, sampling, leaf lookup, the weight mask
and the tree build run in libplenoctree_hip.so through plenoctree_amd.octree_ops; torch holds the device arrays.  Only
N = 2 and the SH data formats (`SH1/4/9/16/25`) and the spherical-Gaussian ones (`SG1/4/9/16/25` with `extra_data`, the [K,4]
lobes (lambda, mu) of octree/extraction.py:436-442) are supported -- anything else raises, there is no fallback.

SG rule (restated from the published svox, like the rest of this file; anchored to the reference's own eval_sg by
tests/golden/sg_reference.npz): basis_i(d) = exp(lambda_i (mu_i . d - 1)) / K, colour_c = sigmoid(sum_i data[c*K+i] basis_i).
extra_data is a buffer, not a parameter: it is saved, loaded, cloned and moved with the tree and never optimised.  An SG tree
renders (render_persp, forward) and back-propagates; the extra outputs (render_persp_aux) and the palette form
(keep_quantized) are not built for it.

Level of detail (no svox counterpart; the reduction is this project's definition, include/plenoctree_octree.h "level of
detail"): N3Tree.fill_internal_() writes the density-weighted mean of every subtree into the row of the
cell that holds it -- rows no renderer reads --, N3Tree.lod(L) cuts a standalone tree at depth L from them, and
VolumeRenderer(tree, max_depth=L) renders level L in place through a copy of `child` with the deeper pointers zeroed.
"""
import re
import types

import numpy as np
import torch

from .. import octree_ops as oops
from .._lib import PxoError, TREE_MAX_DEPTH


def _vec3(v, name):
    a = np.asarray(v, np.float32).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError(f"{name} must have 1 or 3 entries")
    return a.astype(np.float32)


class DataFormat:
    """svox.DataFormat: `.format` in {RGBA, SH, SG, ASG}, `.basis_dim`; str() gives the npz spelling ('SH16')."""
    RGBA, SH, SG, ASG = 0, 1, 2, 3

    def __init__(self, txt, data_dim=None):
        m = re.fullmatch(r"(SH|SG)(\d+)", str(txt))
        if not m:
            raise NotImplementedError(f"data_format {txt!r}: only the spherical-harmonics formats SH1/4/9/16/25 and the "
                                      "spherical-Gaussian formats SG1/4/9/16/25 are supported")
        k = int(m.group(2))
        if k not in (1, 4, 9, 16, 25):
            if m.group(1) == "SG":
                raise NotImplementedError(f"data_format {txt}: SG is built for sg_dim 1, 4, 9, 16 and 25 only (the widths of the "
                                          "MLP head and of the renderers)")
            raise ValueError(f"data_format {txt}: basis_dim must be a square <= 25")
        if data_dim is not None and data_dim != 3 * k + 1:
            raise ValueError(f"data_dim {data_dim} does not match data_format {txt} (expected {3 * k + 1})")
        self.format = DataFormat.SH if m.group(1) == "SH" else DataFormat.SG
        self.basis_dim = k
        self.data_dim = 3 * k + 1

    def __repr__(self):
        return f"{'SG' if self.format == DataFormat.SG else 'SH'}{self.basis_dim}"

    __str__ = __repr__

    def __eq__(self, other):
        return str(self) == str(other)

    def __hash__(self):
        return hash(str(self))


def parse_data_format(fmt, data_dim):
    """'SH16' -> basis_dim 16."""
    return DataFormat(fmt, data_dim).basis_dim


class NDCConfig:
    """svox.NDCConfig (forward-facing LLFF scenes): the projection the scene's NeRF was trained with -- image width, height and
    focal length in pixels, near plane at `near` (the reference always uses 1).  A plain record; VolumeRenderer(ndc=...) and
    the weight mask read it."""

    def __init__(self, width, height, focal, near=1.0):
        self.width, self.height, self.focal, self.near = int(width), int(height), float(focal), float(near)
        if self.width < 1 or self.height < 1 or not self.focal > 0.0 or not self.near > 0.0:
            raise ValueError(f"NDCConfig: width {width} / height {height} must be >= 1, focal {focal} and near {near} > 0")

    def __repr__(self):
        return f"svox.NDCConfig(width={self.width}, height={self.height}, focal={self.focal}, near={self.near})"


class N3TreeView:
    """`tree[key]`: a set of leaves (given by packed cell index node*8 + cell) and a channel slice."""

    def __init__(self, tree, packed, channels=slice(None)):
        self.tree, self.packed, self.channels = tree, packed, channels

    def _all(self):
        return self.packed is None

    def _packed(self):
        return self.tree._leaf_packed() if self.packed is None else self.packed

    def refine(self, repeats=1):
        """svox N3TreeView.refine: split every selected leaf (unique) into 2^3 children holding its value.  Returns
        the number of nodes added.  `repeats` > 1 re-selects all leaves each time and is only defined for tree[:]."""
        if repeats != 1 and not self._all():
            raise NotImplementedError("refine(repeats > 1) is only supported on tree[:]")
        return sum(self.tree._refine_packed(self._packed()) for _ in range(repeats))

    def sample(self, n_samples, device=None):
        """[n_leaves, n_samples, 3] uniform world-space points inside each selected leaf (octree/extraction.py:369)."""
        t = self.tree
        t._sample_calls += 1
        return oops.tree_sample_leaves(t.parent_depth, self._packed(), n_samples, t.offset, t.invradius,
                                       seed=t._sample_seed, stream_id=0x51A0 + t._sample_calls)

    @property
    def values(self):
        d = self.tree.data.data.view(-1, self.tree.data_dim)
        return d[:, self.channels] if self._all() else d[self.packed][:, self.channels]

    @property
    def depths(self):
        return self.tree.parent_depth[self._packed() >> 3, 1]

    def relu_(self):
        """`tree[:, -1:].relu_()` (octree/extraction.py:503) runs the HIP kernel; other selections index tensors."""
        t = self.tree
        ch = range(t.data_dim)[self.channels]
        if self._all() and list(ch) == [t.data_dim - 1]:
            t.relu_sigma_()
            return self
        t._lod_filled = False
        d = t.data.data.view(-1, t.data_dim)
        with torch.no_grad():
            if self._all():
                d[:, self.channels] = d[:, self.channels].relu()
            else:
                rows = d[self.packed]
                rows[:, self.channels] = rows[:, self.channels].relu()
                d[self.packed] = rows
        return self

    def set(self, value):
        t = self.tree
        t._lod_filled = False
        d = t.data.data.view(-1, t.data_dim)
        value = torch.as_tensor(value, dtype=d.dtype, device=d.device)
        with torch.no_grad():
            if self._all():
                d[:, self.channels] = value
            elif self.channels == slice(None):
                d[self.packed] = value
            else:
                rows = d[self.packed]
                rows[:, self.channels] = value
                d[self.packed] = rows


class N3Tree:
    def __init__(self, N=2, data_dim=None, depth_limit=10, init_reserve=1, init_refine=0, geom_resize_fact=1.0,
                 radius=0.5, center=(0.5, 0.5, 0.5), data_format="RGBA", extra_data=None, device="cpu",
                 map_location=None):
        if N != 2:
            raise NotImplementedError("only octrees (tree_branch_n = 2) are supported")
        if init_refine != 0:
            raise NotImplementedError("init_refine must be 0 (octree/extraction.py:491)")
        if not 1 <= depth_limit <= TREE_MAX_DEPTH:
            raise ValueError(f"depth_limit must be in [1, {TREE_MAX_DEPTH}]")
        self.N = 2
        self.data_format = DataFormat(data_format, data_dim)
        self.depth_limit = int(depth_limit)
        self.geom_resize_fact = float(geom_resize_fact)
        dev = torch.device(map_location if map_location is not None else device)
        self.extra_data = _checked_extra_data(extra_data, self.data_format, dev)
        radius, center = _vec3(radius, "radius"), _vec3(center, "center")
        self._set_transform((np.float32(0.5) / radius).astype(np.float32),
                            (np.float32(0.5) * (np.float32(1.0) - center / radius)).astype(np.float32))
        self.child = torch.zeros(1, 2, 2, 2, dtype=torch.int32, device=dev)
        self.parent_depth = torch.zeros(1, 2, dtype=torch.int32, device=dev)
        self.data = torch.nn.Parameter(torch.zeros(1, 2, 2, 2, self.data_dim, dtype=torch.float32, device=dev))
        self.level_nodes = [1]
        self._reset_caches()

    def _set_transform(self, invradius, offset):
        # host float32 tensors (svox keeps them as buffers; the reference calls .cpu() on them and hands them back)
        self.invradius = torch.from_numpy(np.ascontiguousarray(invradius, dtype=np.float32))
        self.offset = torch.from_numpy(np.ascontiguousarray(offset, dtype=np.float32))

    def _reset_caches(self):
        self._leaves = None            # packed indices of all leaves, svox order
        self._level_order = True       # nodes stored breadth-first, levels contiguous (fast-path methods need it)
        self._sample_seed, self._sample_calls = 0, 0
        self._weight_accum = None      # the active WeightAccumulator (accumulate_weights), if any
        self._lod_filled = False       # the rows of cells that have a child hold the pyramid of fill_internal_()

    # ---- structure -------------------------------------------------------------------------------
    @property
    def basis_dim(self):
        return self.data_format.basis_dim

    @property
    def data_dim(self):
        return self.data_format.data_dim

    @property
    def device(self):
        return self.data.device

    @property
    def n_internal(self):
        return self.child.shape[0]

    @property
    def capacity(self):
        return self.child.shape[0]

    @property
    def n_leaves(self):
        return 7 * self.n_internal + 1          # every internal node replaces one leaf by eight

    @property
    def max_depth(self):
        return len(self.level_nodes) - 1

    @property
    def depths(self):
        """Depth of every leaf (= depth of the node that holds it), leaves in svox order (octree/extraction.py:358)."""
        return self.parent_depth[self._leaf_packed() >> 3, 1]

    def parameters(self):
        """nn.Module.parameters() of svox's N3Tree: the data array (octree/optimization.py:180-186)."""
        return [self.data]

    def __repr__(self):
        return (f"svox.N3Tree(N={self.N}, data_dim={self.data_dim}, depth_limit={self.depth_limit}, "
                f"capacity:{self.n_internal}/{self.capacity}, data_format:{self.data_format})")

    def _leaf_packed(self):
        """int64 packed index node*8 + cell of every leaf, ascending = svox's leaf order (nonzero of child == 0)."""
        if self._leaves is None:
            self._leaves = torch.nonzero(self.child.view(-1) == 0).reshape(-1)
        return self._leaves

    # ---- indexing (svox N3Tree.__getitem__ / __setitem__ for the reference's uses) ---------------------
    def _view(self, key):
        channels = slice(None)
        if isinstance(key, tuple):
            if len(key) != 2:
                raise NotImplementedError("tree[...] takes a leaf selector and optionally a channel slice")
            key, channels = key
            if isinstance(channels, int):
                channels = slice(channels, channels + 1 if channels != -1 else None)
            if not isinstance(channels, slice):
                raise NotImplementedError("the channel selector must be an int or a slice")
        if isinstance(key, slice):
            if key != slice(None):
                raise NotImplementedError("leaf slices other than ':' are not supported")
            return N3TreeView(self, None, channels)
        key = torch.as_tensor(key, device=self.device)
        if key.is_floating_point():
            if key.shape[-1] != 3:
                raise ValueError("tree[points]: points must be [n, 3] world coordinates")
            return N3TreeView(self, oops.tree_query(self.child, key.to(self.device), self.offset, self.invradius), channels)
        if key.dtype == torch.bool:
            key = torch.nonzero(key.reshape(-1)).reshape(-1)
        return N3TreeView(self, self._leaf_packed()[key.reshape(-1).long()], channels)

    def __getitem__(self, key):
        return self._view(key)

    def __setitem__(self, key, value):
        self._view(key).set(value)

    def _refine_packed(self, packed):
        """Splits the leaves `packed` (any order, duplicates allowed): new nodes are appended in ascending packed
        order of their parent cell (svox N3Tree._refine_at / refine), children inherit the leaf's value."""
        with torch.no_grad():
            packed = torch.unique(packed.reshape(-1))
            node = packed >> 3
            depth = self.parent_depth[node, 1]
            keep = depth < self.depth_limit
            packed, node, depth = packed[keep], node[keep], depth[keep]
            k = int(packed.numel())
            if k == 0:
                return 0
            n0, D, dev = self.n_internal, self.data_dim, self.device
            self._lod_filled = False
            if n0 + k >= 1 << 28:
                raise PxoError(f"{n0 + k} nodes exceed the int32 packed-index range")
            if int(depth.min()) < self.max_depth:
                self._level_order = False          # a shallower leaf split after deeper nodes exist
            child = torch.cat([self.child, torch.zeros(k, 2, 2, 2, dtype=torch.int32, device=dev)])
            new = torch.arange(n0, n0 + k, device=dev)
            child.view(-1)[packed] = (new - node).int()
            old = self.data.data
            data = torch.cat([old, old.view(-1, D)[packed][:, None, :].expand(k, 8, D).reshape(k, 2, 2, 2, D)])
            pd = torch.cat([self.parent_depth, torch.stack([packed.int(), depth + 1], 1)])
            self.child, self.parent_depth = child, pd
            self.data = torch.nn.Parameter(data, requires_grad=self.data.requires_grad)
            self.level_nodes = [int(c) for c in torch.bincount(pd[:, 1].long()).tolist()]
            self._leaves = None
            return k

    def refine_from_mask(self, mask):
        """Replaces `for _ in range(depth): tree[grid].refine()` (octree/extraction.py:337-350), where grid are
        the centres of the masked voxels of the 2^(depth_limit+1) grid: `mask` is that grid's uint8 mask
        (x slowest).  Must be called on a fresh tree (root only)."""
        if self.n_internal != 1:
            raise PxoError("refine_from_mask needs a fresh tree")
        self.child, self.parent_depth, self.level_nodes = oops.tree_from_mask(mask.reshape(-1), self.depth_limit)
        while len(self.level_nodes) > 1 and self.level_nodes[-1] == 0:
            self.level_nodes.pop()
        self.data = torch.nn.Parameter(torch.zeros(self.n_internal, 2, 2, 2, self.data_dim, dtype=torch.float32,
                                                   device=mask.device), requires_grad=self.data.requires_grad)
        self._leaves, self._level_order, self._lod_filled = None, True, False
        return self

    def _need_level_order(self, what):
        if not self._level_order:
            raise PxoError(f"{what} needs breadth-first node storage (levels refined one at a time)")

    def max_depth_nodes(self):
        """(first node, count) of the deepest level: its 8*count cells are the leaves with depth == max_depth,
        in leaf order (`tree.depths == tree.max_depth`, octree/extraction.py:358-360)."""
        self._need_level_order("max_depth_nodes")
        count = self.level_nodes[-1]
        return self.n_internal - count, count

    def sample_max_depth_cells(self, n_samples, first=0, count=None, seed=0, u=None):
        """tree[leaf_ind[...]].sample(n_samples) for the cells of `count` deepest-level nodes starting at the
        `first`-th: [count*8, n_samples, 3] world-space points (octree/extraction.py:369)."""
        node0, total = self.max_depth_nodes()
        count = total - first if count is None else count
        return oops.tree_sample_cells(self.parent_depth, node0 + first, count, n_samples, self.offset, self.invradius,
                                      u=u, seed=seed, stream_id=0x7A3 + first)

    def max_depth_data(self, first=0, count=None):
        """View [count*8, data_dim] of the deepest-level cells: writing it is `tree[chunk_inds] = rgba`
        (octree/extraction.py:394)."""
        node0, total = self.max_depth_nodes()
        count = total - first if count is None else count
        self._lod_filled = False                 # the view is there to be written
        return self.data.data[node0 + first: node0 + first + count].view(count * 8, self.data_dim)

    def relu_sigma_(self):
        """tree[:, -1:].relu_() (octree/extraction.py:503)."""
        oops.tree_relu_sigma(self.data.data)
        self._lod_filled = False
        return self

    def shrink_to_fit(self):
        return self                              # arrays are always exactly n_internal long

    def view(self):
        return oops.tree_view(self.child, self.data.data, self.offset, self.invradius)

    # what VolumeRenderer asks of a tree of any storage form (the read-only forms: _ReadOnlyTree)
    render_view = view
    ndc_refusal = None
    requires_grad = property(lambda self: self.data.requires_grad)

    def basis_kwargs(self):
        """What selects the renderer of this tree's basis in octree_ops: the lobes of an SG tree, nothing for an SH tree."""
        return {} if self.extra_data is None else {"lobes": self.extra_data}

    def to(self, device):
        """The tree on another device (a new object; nn.Module.to of svox's N3Tree)."""
        return self.clone(device=device)

    def clone(self, device=None):
        t = object.__new__(N3Tree)
        t.__dict__.update(self.__dict__)
        dev = torch.device(device) if device is not None else self.device
        t.child, t.parent_depth = (x.detach().clone().to(dev) for x in (self.child, self.parent_depth))
        t.data = torch.nn.Parameter(self.data.data.detach().clone().to(dev), requires_grad=self.data.requires_grad)
        t.invradius, t.offset = self.invradius.clone(), self.offset.clone()
        t.extra_data = None if self.extra_data is None else self.extra_data.detach().clone().to(dev)
        t.level_nodes = list(self.level_nodes)
        t._leaves = None
        t._weight_accum = None                   # an accumulator belongs to the tree it was opened on
        return t

    # ---- leaf weights (svox N3Tree.accumulate_weights; published interface, parity unpinned) -------------------------
    def accumulate_weights(self, op="sum"):
        """Context manager: while it is active every VolumeRenderer.render_persp / forward call on this tree also accumulates,
        per leaf, the compositing weights of its samples (`op`: "sum" or "max" over all rays rendered inside the block).

            with tree.accumulate_weights(op="max") as accum:
                renderer.render_persp(c2w, ...)
            accum.value            # [n_internal, 2, 2, 2]; accum() is the same tensor

        The images rendered inside the block are those rendered outside it.  Blocks do not nest, and the tree's structure must
        not change inside one (refine, prune_, refine_from_mask): the next render then raises."""
        return WeightAccumulator(self, op)

    # ---- additions (no svox counterpart): prune by a mask over cells, split a chosen set of leaves --------------------
    def _cell_mask(self, mask, what):
        mask = torch.as_tensor(mask, device=self.device)
        if mask.dtype != torch.bool or mask.numel() != self.n_internal * 8:
            raise ValueError(f"{what}: the mask must be bool over the tree's {self.n_internal} x 2 x 2 x 2 cells, got "
                             f"{mask.dtype} with {mask.numel()} entries")
        return mask.reshape(-1)

    def prune_(self, keep, collapse=True):
        """Zeroes every leaf whose `keep` (bool over cells, e.g. `accum.value > thresh`) is False and, with `collapse`, removes
        every node left with nothing but dead leaves below it, bottom-up, folding it back into one zero leaf of its parent (the
        root stays).  Entries of `keep` at cells that are not leaves are ignored.  Returns the number of nodes removed."""
        keep = self._cell_mask(keep, "prune_")
        n0 = self.n_internal
        self._lod_filled = False
        with torch.no_grad():
            if not collapse:
                dead = (self.child.view(-1) == 0) & ~keep
                self.data.data.view(-1, self.data_dim)[dead] = 0
                return 0
            child, pd, data, _ = oops.tree_collapse(self.child, self.parent_depth, self.data.data, keep)
            self.child, self.parent_depth = child, pd
            self.data = torch.nn.Parameter(data, requires_grad=self.data.requires_grad)
            self.level_nodes = [int(c) for c in torch.bincount(pd[:, 1].long()).tolist()]
            self._leaves = None                  # survivors keep their order: _level_order stays as it was
        return n0 - self.n_internal

    def refine_leaves(self, mask):
        """Splits every leaf whose `mask` (bool over cells) is True into 2^3 children holding its value; leaves already at
        depth_limit stay.  Entries at cells that are not leaves are ignored.  Returns the number of nodes added."""
        mask = self._cell_mask(mask, "refine_leaves")
        return self._refine_packed(torch.nonzero(mask & (self.child.view(-1) == 0)).reshape(-1))

    # ---- additions (no svox counterpart): level of detail from a mean pyramid in the rows no renderer reads -----------------
    def fill_internal_(self):
        """Writes into the row of every cell that has a child the density-weighted mean of the subtree below it, bottom-up
        (pxo_tree_lod_fill: this project's reduction, not svox's; include/plenoctree_octree.h, "level of detail").  Leaf rows
        and every full-depth render stay as they are.  The tree is then marked filled; every method of this class that changes
        structure or data (refine, refine_from_mask, prune_, tree[...] = value, relu_, relu_sigma_, max_depth_data) clears the
        mark.  Writes that bypass the class -- an optimizer step, a kernel writing through tree.data -- do not: call this again
        after them (torch's version counter is no help, the kernels write through raw pointers)."""
        oops.tree_lod_fill(self.child, self.parent_depth, self.data.data, self.max_depth)
        self._lod_filled = True
        return self

    def _lod_depth(self, L, what):
        if not isinstance(L, (int, np.integer)) or isinstance(L, bool) or not 0 <= L <= self.max_depth:
            raise ValueError(f"{what}: depth {L!r} is outside [0, {self.max_depth}] (the tree's max_depth)")
        return int(L)

    def lod_child(self, L):
        """A copy of `child` with the pointers of every node of depth >= L zeroed: rendered with the tree's own (filled) data,
        it shows the tree at level L (2^(L+1) cells per axis), since a marcher stops wherever child == 0 and reads the row there."""
        L = self._lod_depth(L, "lod_child")
        return self.child * (self.parent_depth[:, 1] < L).to(torch.int32)[:, None, None, None]

    def lod(self, L, fill=True):
        """A new N3Tree holding the nodes of depth <= L in their original order, the cells of its depth-L nodes all leaves: a
        cell that had a child carries the filled row of that child (the mean of its subtree), surviving leaves keep their rows
        bit for bit, and the rows of cells that still have a child are zero, as the extraction leaves them.  Transform, format,
        depth_limit, geom_resize_fact and a copy of extra_data are carried over.  fill=True runs fill_internal_() on THIS tree
        first unless it is marked filled (a side effect on its unused rows only); fill=False takes the rows as they stand and
        runs on a CPU tree."""
        L = self._lod_depth(L, "lod")
        if fill and not self._lod_filled:
            self.fill_internal_()
        with torch.no_grad():
            depth = self.parent_depth[:, 1]
            keep = depth <= L
            new_index = torch.cumsum(keep.long(), 0) - 1                  # of survivors; unused elsewhere
            old = torch.nonzero(keep).reshape(-1)
            skip = self.child.view(-1, 8)[old].long()
            inner = (skip != 0) & (depth[old] < L)[:, None]               # cells that still have a child
            target = old[:, None] + skip                                  # == old where skip == 0: always a valid index
            child = torch.where(inner, new_index[target] - new_index[old][:, None], torch.zeros_like(skip))
            parent = self.parent_depth[old, 0].long()                     # the parent of a survivor survives; root: (0, 0)
            pd = torch.stack([(new_index[parent >> 3] * 8 + (parent & 7)).int(), depth[old]], 1)
            data = self.data.data.view(-1, 8, self.data_dim)[old]
            data = torch.where(inner[:, :, None], torch.zeros_like(data), data)
        t = object.__new__(N3Tree)
        t.__dict__.update(self.__dict__)
        t.child, t.parent_depth = child.int().reshape(-1, 2, 2, 2), pd
        t.data = torch.nn.Parameter(data.reshape(-1, 2, 2, 2, self.data_dim), requires_grad=self.data.requires_grad)
        t.invradius, t.offset = self.invradius.clone(), self.offset.clone()
        t.extra_data = None if self.extra_data is None else self.extra_data.detach().clone()
        t.level_nodes = list(self.level_nodes[:L + 1])
        t._leaves, t._weight_accum, t._lod_filled = None, None, False
        t._level_order = not bool((pd[1:, 1] < pd[:-1, 1]).any())
        return t

    # ---- npz (svox N3Tree.save / load; keys as consumed by octree/compression.py:76-86) ------------------
    def save(self, path, shrink=True, compress=True):
        z = {
            "data_dim": self.data_dim,
            "child": self.child.cpu().numpy(),
            "parent_depth": self.parent_depth.cpu().numpy(),
            "n_internal": self.n_internal,
            "n_free": 0,
            "invradius3": self.invradius.numpy(),
            "offset": self.offset.numpy(),
            "depth_limit": self.depth_limit,
            "geom_resize_fact": self.geom_resize_fact,
            "data": self.data.data.detach().half().cpu().numpy(),       # svox stores float16
            "data_format": str(self.data_format),
        }
        if self.extra_data is not None:
            z["extra_data"] = self.extra_data.detach().cpu().numpy()      # the SG lobes, float32 [K,4]
        (np.savez_compressed if compress else np.savez)(path, **z)

    @classmethod
    def load(cls, path, device="cpu", map_location=None, keep_quantized=False, keep_half=False):
        """svox N3Tree.load.  A compressed file (octree/compression.py) is re-inflated to float32 `data`, unless
        `keep_quantized`: then the palette form is kept as it is and a read-only QuantizedN3Tree comes back.
        `keep_half`: the float16 `data` of an uncompressed file is kept as it is (SH or SG) and a read-only HalfN3Tree comes
        back, which renders exactly what the float tree of the same file renders."""
        dev = torch.device(map_location if map_location is not None else device)
        if keep_half and keep_quantized:
            raise ValueError(f"{path}: keep_half=True together with keep_quantized=True: a file holds either float16 data or the "
                             "palette form; choose one")
        z = np.load(path)
        if keep_half:
            if "data" not in z.files:
                what = "a compressed tree (the palette form): load it with keep_quantized=True" if "quant_colors" in z.files \
                    else "no data array"
                raise ValueError(f"{path}: keep_half=True needs the float16 data of an uncompressed tree; the file has {what}")
            data = z["data"]
            if data.dtype != np.float16:
                raise ValueError(f"{path}: keep_half=True needs float16 data; the file's data is {data.dtype}")
            return HalfN3Tree(z, data, dev)
        if keep_quantized:
            if "quant_colors" not in z.files:
                raise ValueError(f"{path}: keep_quantized=True needs a compressed tree (no quant_colors in the file)")
            if "data_format" in z.files and str(z["data_format"]).startswith("SG"):
                raise NotImplementedError(f"{path}: keep_quantized=True on an SG tree ({z['data_format']}): palette-form rendering "
                                          "is built for SH trees only; load it without keep_quantized")
            return QuantizedN3Tree(z, dev)
        return cls._from_npz(z, dev)

    @classmethod
    def _from_npz(cls, z, dev):
        if "quant_colors" in z.files:
            z = _dequantized(z)
        t = object.__new__(cls)
        n = _load_geometry(t, z, dev)
        t.data = torch.nn.Parameter(torch.from_numpy(z["data"][:n].astype(np.float32)).to(dev))
        return t


class WeightAccumulator:
    """What `with tree.accumulate_weights(op) as accum` yields: `accum.value` (also `accum()`) is the [n_internal, 2, 2, 2]
    float32 tensor of per-leaf weights, zero at cells that are not leaves and at leaves no ray rendered inside the block has
    shaded.  It stays readable after the block."""

    def __init__(self, tree, op):
        if op not in oops.WEIGHT_OPS:
            raise ValueError(f"accumulate_weights(op={op!r}): op must be 'sum' or 'max'")
        self.tree, self.op, self.value = tree, op, None
        self._child = None

    def __enter__(self):
        t = self.tree
        if t._weight_accum is not None:
            raise PxoError("accumulate_weights: this tree already has an active accumulator (the blocks do not nest)")
        self._child = t.child                    # every structure edit replaces tree.child by a new tensor
        self.value = torch.zeros(t.n_internal, 2, 2, 2, dtype=torch.float32, device=t.device)
        t._weight_accum = self
        return self

    def __exit__(self, *exc):
        self.tree._weight_accum = None
        self._child = None
        return False

    def __call__(self):
        return self.value

    def _buffer(self):
        """The flat accumulator for a launch; refuses a tree that was refined / pruned / rebuilt since the block opened."""
        if self.tree.child is not self._child:
            raise PxoError("accumulate_weights: the tree's structure changed inside the block (refine / prune_ / "
                           "refine_from_mask): the accumulated weights no longer address its cells")
        return self.value.view(-1)


def _checked_extra_data(extra_data, data_format, dev):
    """The [K,4] float32 lobes of an SG tree on `dev`, or None for an SH tree; every mismatch with the format is named."""
    if data_format.format != DataFormat.SG:
        if extra_data is not None:
            raise ValueError(f"extra_data given with data_format {data_format}: only the SG formats carry extra_data")
        return None
    if extra_data is None:
        raise NotImplementedError(f"data_format {data_format} without extra_data: an SG tree needs its [{data_format.basis_dim}, 4] "
                                  "lobes (lambda, mu.x, mu.y, mu.z), octree/extraction.py:436-442")
    e = torch.as_tensor(np.asarray(extra_data.detach().cpu() if torch.is_tensor(extra_data) else extra_data), dtype=torch.float32)
    if tuple(e.shape) != (data_format.basis_dim, 4):
        raise ValueError(f"extra_data has shape {tuple(e.shape)}, data_format {data_format} needs ({data_format.basis_dim}, 4)")
    if not bool(torch.isfinite(e).all()) or not bool((e[:, 0] > 0).all()):
        raise ValueError("extra_data: the lobes must be finite with lambda (column 0) > 0")
    return e.contiguous().to(dev)


def _load_geometry(t, z, dev):
    """The part of N3Tree.load that does not touch the leaf values: format, child, parent_depth, transform, levels.
    Returns the node count."""
    t.N = 2
    fmt = str(z["data_format"]) if "data_format" in z.files else "RGBA"
    t.data_format = DataFormat(fmt, int(z["data_dim"]))
    t.extra_data = _checked_extra_data(z["extra_data"] if "extra_data" in z.files else None, t.data_format, dev)
    child = z["child"]
    if child.shape[1:] != (2, 2, 2):
        raise NotImplementedError("only octrees (N = 2) are supported")
    n = int(z["n_internal"]) if "n_internal" in z.files else child.shape[0]
    t.child = torch.from_numpy(child[:n].astype(np.int32)).to(dev)
    if "parent_depth" in z.files:
        pd = z["parent_depth"][:n].astype(np.int32)
    else:
        pd = parent_depth_from_child(child[:n])
    t.parent_depth = torch.from_numpy(pd).to(dev)
    if "invradius3" in z.files:
        invradius = z["invradius3"].astype(np.float32)
    else:
        invradius = np.repeat(np.float32(z["invradius"]), 3)
    N3Tree._set_transform(t, invradius, z["offset"].astype(np.float32))
    t.depth_limit = int(z["depth_limit"]) if "depth_limit" in z.files else int(pd[:, 1].max())
    t.geom_resize_fact = float(z["geom_resize_fact"]) if "geom_resize_fact" in z.files else 1.0
    counts = np.bincount(pd[:, 1])
    N3Tree._reset_caches(t)
    t._level_order = not bool((np.diff(pd[:, 1]) < 0).any())
    t.level_nodes = [int(c) for c in counts]
    if len(t.level_nodes) - 1 > TREE_MAX_DEPTH:
        raise NotImplementedError(f"tree depth {len(t.level_nodes) - 1} exceeds {TREE_MAX_DEPTH}")
    return n


def _dequantized(z):
    """Undoes octree/compression.py:88-136 on a loaded npz: `data` [n,2,2,2,3K+1] from `quant_colors` [K', 2^bits, 3] +
    `quant_map` [K', n,2,2,2] (+ `data_retained` [r, n,2,2,2,3] for the first r basis functions) + `sigma` [n,2,2,2]."""
    out = {k: z[k] for k in z.files}
    colors, qmap, sigma = z["quant_colors"].astype(np.float32), z["quant_map"].astype(np.int64), z["sigma"].astype(np.float32)
    retained = z["data_retained"].astype(np.float32) if "data_retained" in z.files else np.zeros((0,) + sigma.shape + (3,), np.float32)
    K = retained.shape[0] + colors.shape[0]
    rgb = np.empty(sigma.shape + (3, K), np.float32)                      # [..., channel, basis]: the layout of `data`
    for b in range(retained.shape[0]):
        rgb[..., b] = retained[b]
    for b in range(colors.shape[0]):
        rgb[..., retained.shape[0] + b] = colors[b][qmap[b]]
    out["data"] = np.concatenate([rgb.reshape(sigma.shape + (3 * K,)), sigma[..., None]], -1)
    return _NpzDict(out)


class _NpzDict(dict):
    """dict with the `.files` attribute of an NpzFile."""

    @property
    def files(self):
        return list(self.keys())


def _validated_quant(z, n):
    """The palette arrays of a compressed npz (first n nodes), checked on the host before anything reaches the GPU:
    (quant_map uint16 [Kq, n*8], quant_colors float16 [Kq, 2^bits, 3], sigma [n*8], data_retained float16 [r, n*8, 3] or
    None, bits).  Every inconsistency is a ValueError naming the offending array."""
    K = (int(z["data_dim"]) - 1) // 3
    colors, qmap, sigma = np.asarray(z["quant_colors"]), np.asarray(z["quant_map"]), np.asarray(z["sigma"])
    retained = np.asarray(z["data_retained"]) if "data_retained" in z.files else None
    if colors.ndim != 3 or colors.shape[2] != 3:
        raise ValueError(f"quant_colors: shape {colors.shape} is not [K', 2^bits, 3]")
    Kq, P = colors.shape[0], colors.shape[1]
    bits = P.bit_length() - 1
    if P != 1 << bits or not 1 <= bits <= 16:
        raise ValueError(f"quant_colors: {P} palette entries are not 2^bits with bits in 1..16")
    if qmap.shape[0] != Kq:
        raise ValueError(f"quant_map: {qmap.shape[0]} planes but quant_colors has {Kq} palettes")
    r = 0 if retained is None else retained.shape[0]
    if Kq < 1 or r + Kq != K:
        which = "quant_colors" if retained is None else "data_retained"
        raise ValueError(f"{which}: {r} retained + {Kq} quantised planes do not make basis_dim {K} of {z['data_format']}")
    cells = (2, 2, 2)
    if qmap.shape[1] < n or qmap.shape[2:] != cells:
        raise ValueError(f"quant_map: shape {qmap.shape} does not hold [K', {n}, 2, 2, 2] leaves like child")
    if sigma.shape[0] < n or sigma.shape[1:] != cells:
        raise ValueError(f"sigma: shape {sigma.shape} does not hold [{n}, 2, 2, 2] leaves like child")
    if retained is not None and (retained.ndim != 6 or retained.shape[1] < n or retained.shape[2:] != cells + (3,)):
        raise ValueError(f"data_retained: shape {retained.shape} does not hold [r, {n}, 2, 2, 2, 3] leaves like child")
    if not np.issubdtype(qmap.dtype, np.integer):
        raise ValueError(f"quant_map: dtype {qmap.dtype} is not an integer type")
    qmap = qmap[:, :n].reshape(Kq, n * 8)
    if qmap.size and (int(qmap.min()) < 0 or int(qmap.max()) >= P):
        raise ValueError(f"quant_map: index {int(qmap.max()) if int(qmap.min()) >= 0 else int(qmap.min())} is outside its "
                         f"palette of {P} entries")
    if sigma.dtype not in (np.float16, np.float32):
        raise ValueError(f"sigma: dtype {sigma.dtype} is neither float16 nor float32")
    if colors.dtype != np.float16 or (retained is not None and retained.dtype != np.float16):
        raise ValueError("quant_colors / data_retained: expected float16, as octree.compression writes them")
    return (np.ascontiguousarray(qmap.astype(np.uint16, copy=False)), np.ascontiguousarray(colors),
            np.ascontiguousarray(sigma[:n].reshape(n * 8)),
            None if retained is None else np.ascontiguousarray(retained[:, :n].reshape(r, n * 8, 3)), bits)


class _ReadOnlyTree:
    """What QuantizedN3Tree and HalfN3Tree share: the geometry of an N3Tree, no float leaf data, and a refusal by name of
    everything that reads or edits it.  A subclass gives its NOUN, the name of its WAY_OUT to a float N3Tree, and
    render_view()."""

    basis_dim = N3Tree.basis_dim
    data_dim = N3Tree.data_dim
    n_internal = N3Tree.n_internal
    n_leaves = N3Tree.n_leaves
    max_depth = N3Tree.max_depth
    basis_kwargs = N3Tree.basis_kwargs
    # what VolumeRenderer asks of a tree before it renders it
    requires_grad = False                        # never differentiable
    _weight_accum = None                         # no weight accumulation
    ndc_refusal = None                           # why VolumeRenderer(ndc=...) refuses this form, if it does

    @property
    def device(self):
        return self.child.device

    @property
    def float_nbytes(self):
        """Device bytes the float form (what N3Tree.load makes of the same file) takes."""
        return 4 * self.n_internal * 8 * self.data_dim + 4 * (self.child.numel() + self.parent_depth.numel())

    def _device_form(self):
        if self._packed is None:
            raise PxoError(f"a {self.NOUN} renders on a ROCm device only (there is no CPU fallback): load it with map_location='cuda'")
        return self._packed

    def _read_only(self, what):
        raise PxoError(f"{what}: a {self.NOUN} is read-only and has no float leaf data; call {self.WAY_OUT}() for an N3Tree")


def _refused(what):
    def stub(self, *args, **kwargs):
        self._read_only(what)
    return stub


for _name, _what in (("parameters", "tree.parameters()"), ("__getitem__", "tree[...]"), ("__setitem__", "tree[...] = value"),
                     ("refine", "refine"), ("refine_from_mask", "refine_from_mask"), ("relu_sigma_", "relu_sigma_"),
                     ("accumulate_weights", "accumulate_weights"), ("prune_", "prune_"), ("refine_leaves", "refine_leaves"),
                     ("view", "view()"), ("save", "save")):
    setattr(_ReadOnlyTree, _name, _refused(_what))
_ReadOnlyTree.data = property(_refused("tree.data"))
del _name, _what


class QuantizedN3Tree(_ReadOnlyTree):
    """A compressed tree (octree/compression.py) kept in its palette form: `N3Tree.load(path, keep_quantized=True)`.

    Read-only.  It has the geometry of an N3Tree (child, parent_depth, offset, invradius, depth_limit, data_format,
    n_internal, max_depth, device) and is rendered in place by VolumeRenderer; on a GPU device the file's arrays are
    uploaded as they are and packed there (include/plenoctree_octree.h, PxoQuantLayout), with no gather over the leaves
    on the host.  There is no `data`: everything that needs float leaf values goes through `dequantize()`."""

    def __init__(self, z, dev):
        self._z = _NpzDict({k: z[k] for k in z.files})           # the file's arrays, for dequantize()
        n = _load_geometry(self, self._z, dev)
        qmap, colors, sigma, retained, self.bits = _validated_quant(self._z, n)
        self.n_retained = 0 if retained is None else retained.shape[0]
        self._layout = oops.quant_layout(n, self.basis_dim, self.n_retained, self.bits)
        self._packed = None
        if dev.type == "cuda":
            up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
            self._packed, _ = oops.quant_pack(up(qmap.view(np.int16)), up(colors), up(sigma), up(retained), n, self.basis_dim,
                                              self.n_retained, self.bits)

    NOUN, WAY_OUT = "QuantizedN3Tree", "dequantize"
    ndc_refusal = ("VolumeRenderer(ndc=...) on a QuantizedN3Tree: NDC rendering of the palette form is not built; load the tree "
                   "without keep_quantized")

    @property
    def nbytes(self):
        """Device bytes of this form: the packed buffer (indices, palettes, sigma, retained planes) + child + parent_depth."""
        return int(self._layout.total_bytes) + 4 * (self.child.numel() + self.parent_depth.numel())

    def quant_view(self):
        return oops.quant_tree_view(self.child, self._device_form(), self._layout, self.basis_dim, self.n_retained, self.bits,
                                    self.offset, self.invradius)

    render_view = quant_view

    def dequantize(self):
        """The float N3Tree that `N3Tree.load(path)` makes of the same file, on this tree's device."""
        return N3Tree._from_npz(self._z, self.device)

    def __repr__(self):
        return (f"svox.QuantizedN3Tree(N=2, data_format:{self.data_format}, n_internal:{self.n_internal}, bits:{self.bits}, "
                f"retained:{self.n_retained}, {self.nbytes / 2 ** 20:.1f} MB on the device, float form {self.float_nbytes / 2 ** 20:.1f} MB)")


class HalfN3Tree(_ReadOnlyTree):
    """An uncompressed tree kept in the float16 of its file: `N3Tree.load(path, keep_half=True)`.

    Read-only.  It has the geometry of an N3Tree (child, parent_depth, offset, invradius, depth_limit, data_format,
    extra_data for an SG file, n_internal, max_depth, device) and is rendered in place by VolumeRenderer, bit for bit as the
    float tree of the same file: on a GPU device the file's data is uploaded as it is and laid out there at the row stride
    of include/plenoctree_octree.h (PxoHalfTree).  There is no float `data`: everything that needs or edits float leaf values
    goes through `to_float()`."""

    def __init__(self, z, data, dev):
        n = _load_geometry(self, z, dev)
        if data.ndim != 5 or data.shape[0] < n or data.shape[1:] != (2, 2, 2, self.data_dim):
            raise ValueError(f"data: shape {data.shape} does not hold [{n}, 2, 2, 2, {self.data_dim}] leaves like child")
        self.row_stride, self._packed_bytes = oops.half_layout(n, self.data_dim)
        half = torch.from_numpy(np.ascontiguousarray(data[:n]))
        self._half, self._packed = None, None
        if dev.type == "cuda":
            self._packed, _ = oops.half_pack(half.to(dev), n)        # the upload is dropped once it is laid out
        else:
            self._half = half

    NOUN, WAY_OUT = "HalfN3Tree", "to_float"

    @property
    def nbytes(self):
        """Device bytes of this form: the float16 rows at their stride + child + parent_depth."""
        return int(self._packed_bytes) + 4 * (self.child.numel() + self.parent_depth.numel())

    def half_view(self):
        return oops.half_tree_view(self.child, self._device_form(), self.data_dim, self.offset, self.invradius)

    render_view = half_view

    def to_float(self):
        """The float N3Tree that `N3Tree.load(path)` makes of the same file, on this tree's device."""
        n, D = self.n_internal, self.data_dim
        half = self._half if self._packed is None else self._packed[:, :D].reshape(n, 2, 2, 2, D)
        t = object.__new__(N3Tree)
        t.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("row_stride", "_packed_bytes", "_half", "_packed")})
        t.child, t.parent_depth = self.child.clone(), self.parent_depth.clone()
        t.invradius, t.offset = self.invradius.clone(), self.offset.clone()
        t.extra_data = None if self.extra_data is None else self.extra_data.clone()
        t.level_nodes = list(self.level_nodes)
        t.data = torch.nn.Parameter(half.float().contiguous())
        return t

    def __repr__(self):
        return (f"svox.HalfN3Tree(N=2, data_format:{self.data_format}, n_internal:{self.n_internal}, row_stride:{self.row_stride}, "
                f"{self.nbytes / 2 ** 20:.1f} MB on the device, float form {self.float_nbytes / 2 ** 20:.1f} MB)")


def parent_depth_from_child(child):
    """Rebuilds parent_depth [n,2] from the child offsets (compressed npz files drop it, compression.py:77)."""
    n = child.shape[0]
    pd = np.zeros((n, 2), np.int32)
    flat = child.reshape(n, 8)
    src, cell = np.nonzero(flat)
    dst = src + flat[src, cell]
    pd[dst, 0] = src * 8 + cell
    order = np.argsort(dst)                     # parents precede children (nodes are only ever appended)
    for s, d in zip(src[order], dst[order]):
        pd[d, 1] = pd[s, 1] + 1
    return pd


class _RenderPersp(torch.autograd.Function):
    """torch.autograd bridge so `mse.backward()` on a rendered image reaches tree.data as in
    octree/optimization.py:216-224; forward/backward are the HIP kernels."""

    @staticmethod
    def forward(ctx, data, renderer, c2w, width, height, fx, fy, opts):
        tree = renderer.tree
        ctx.args = (renderer, c2w, width, height, fx, fy, opts)
        out = oops.octree_render_persp(oops.tree_view(tree.child, data.detach(), tree.offset, tree.invradius), c2w, width,
                                       height, fx, opts, fy, **renderer._basis_kwargs())
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        renderer, c2w, width, height, fx, fy, opts = ctx.args
        tree = renderer.tree
        grad = torch.zeros_like(tree.data.data)
        out, = ctx.saved_tensors
        oops.octree_render_persp_bwd(tree.view(), c2w, width, height, fx, opts, grad_out.contiguous(), grad, fy, out_rgb=out,
                                     **renderer._basis_kwargs())
        return grad, None, None, None, None, None, None, None


class VolumeRenderer:
    """svox.VolumeRenderer for perspective cameras.

    ndc: None, or the NDCConfig of a forward-facing (LLFF) scene whose tree lives in the NDC cube.  Cameras and rays are still
    given in world space; every ray is converted as include/plenoctree_octree.h ("forward-facing scenes") and DESIGN section 13
    define: the SH basis on the world-space direction, convert_to_ndc, a unit NDC direction, then the unchanged march (step
    lengths are NDC lengths, what the NeRF integrated sigma over).  svox's own NDC kernel could not be compared.  Float SH
    trees only: a QuantizedN3Tree, an SG tree and the alpha / depth / surface outputs are refused by name.

    A HalfN3Tree renders wherever the float tree of the same file does (SH and SG in world space, SH with ndc, the alpha /
    depth / surface outputs on SH in world space), the same values bit for bit, and is refused where that tree is, in the same
    words.  It is never differentiable.

    max_depth (an addition, no svox counterpart): None, or the level L the tree is rendered at, in place: through a copy of
    `child` with the pointers of depth >= L nodes zeroed (N3Tree.lod_child) and the tree's own data, whose unused rows
    N3Tree.fill_internal_() has filled with the mean of the subtree below them.  The images are those of `tree.lod(L)`, bit for
    bit, through the same launches (SH and SG, world space and ndc, the aux outputs).  The first capped render fills the tree
    if it is not marked filled, and every capped render checks the mark and the identity of tree.child, so a change made
    through the class is followed by a refill; a stale pyramid is never rendered.  max_depth >= tree.max_depth renders the
    full tree.  Float N3Tree only; a capped render is refused by name while the tree requires grad with grad mode on
    (fine-tune tree.lod(L) instead) and inside accumulate_weights.

    lod_pixels (an addition, no svox counterpart): None or 0 for the launches above, or P > 0: every sample stops its descent
    at the first cell that is no wider than P pixels where the sample lies, and reads the filled row there (the definition:
    include/plenoctree_octree.h, "footprint"; forward only, hard steps between levels).  render_persp / render_persp_aux take
    the width of a pixel from the camera, cone = P / max(fx, fy); forward / forward_aux need pixel_angle, radians per pixel
    for unit dirs, cone = P * pixel_angle.  lod_min_depth: no sample is folded above this depth.  The tree is filled and
    refilled as for max_depth, with which it composes (the footprint march then runs on the capped child array).  Float
    N3Tree in world space only; refused by name for the other forms, with ndc, while the tree requires grad with grad mode
    on, and inside accumulate_weights."""

    def __init__(self, tree, step_size=1e-3, background_brightness=1.0, ndc=None, max_depth=None, lod_pixels=None,
                 lod_min_depth=0):
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
        if lod_pixels is not None and not (number(lod_pixels) and 0 <= lod_pixels < float("inf")):
            raise ValueError(f"VolumeRenderer(lod_pixels={lod_pixels!r}): must be None or a finite number >= 0")
        if not isinstance(lod_min_depth, (int, np.integer)) or isinstance(lod_min_depth, bool) or \
                not 0 <= lod_min_depth <= TREE_MAX_DEPTH:
            raise ValueError(f"VolumeRenderer(lod_min_depth={lod_min_depth!r}): must be an integer in [0, {TREE_MAX_DEPTH}]")
        self.lod_pixels = float(lod_pixels) if lod_pixels else None          # None and 0: the launches without a footprint
        self.lod_min_depth = int(lod_min_depth)
        if self.lod_pixels is not None:
            if not isinstance(tree, N3Tree):
                raise NotImplementedError(f"VolumeRenderer(lod_pixels=...) on a {type(tree).__name__}: footprint rendering is "
                                          f"built for the float N3Tree only; call {getattr(tree, 'WAY_OUT', 'to_float')}() first")
            if ndc is not None:
                raise NotImplementedError("VolumeRenderer(lod_pixels=...) with ndc: footprint rendering is not built for an NDC "
                                          "scene (a ray parameter there is an NDC length, and a pixel footprint along it has no "
                                          "meaning)")
        if max_depth is not None:
            if not isinstance(tree, N3Tree):
                raise NotImplementedError(f"VolumeRenderer(max_depth=...) on a {type(tree).__name__}: capped rendering is built "
                                          f"for the float N3Tree only; call {getattr(tree, 'WAY_OUT', 'to_float')}() first")
            if not isinstance(max_depth, (int, np.integer)) or isinstance(max_depth, bool) or max_depth < 0:
                raise ValueError(f"VolumeRenderer(max_depth={max_depth!r}): must be None or an integer >= 0")
        self.max_depth = None if max_depth is None else int(max_depth)
        self._lod_child, self._lod_of = None, None       # the capped child array and the tree.child it was made from
        if ndc is not None:
            if not isinstance(ndc, NDCConfig):
                raise NotImplementedError(f"VolumeRenderer(ndc=...): NDC rendering takes an svox.NDCConfig, got {type(ndc).__name__}")
            if tree.ndc_refusal:
                raise NotImplementedError(tree.ndc_refusal)
            if getattr(tree, "extra_data", None) is not None:
                raise NotImplementedError(f"VolumeRenderer(ndc=...) on an SG tree ({tree.data_format}): NDC rendering is built for "
                                          "SH trees only")
        self.ndc = ndc
        self.tree = tree
        self.step_size = float(step_size)
        self.background_brightness = float(background_brightness)

    def _opts(self, fast):
        thr = 1e-2 if fast else 0.0              # svox: fast = early stopping + skip of near-empty cells
        return oops.render_opts(self.step_size, self.background_brightness, thr, thr)

    def _basis_kwargs(self):
        """What selects the launch in octree_ops: the lobes of an SG tree, the projection of an NDC scene, nothing otherwise."""
        kw = dict(self.tree.basis_kwargs())
        if self.ndc is not None:
            kw["ndc"] = self.ndc
        return kw

    def _view(self, what):
        """The view a forward launch of `what` renders: the tree's own, or with an active cap (max_depth below the tree's
        depth) the capped child array over the tree's filled data, refilled / rebuilt if the tree changed since."""
        t = self.tree
        capped = self.max_depth is not None and self.max_depth < t.max_depth
        if not capped and self.lod_pixels is None:
            return t.render_view()
        if capped:
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError(f"{what} with max_depth={self.max_depth} on a tree that requires grad: there is no "
                                          f"gradient through a capped view; fine-tune tree.lod({self.max_depth}) instead, or "
                                          "render under torch.no_grad()")
            if t._weight_accum is not None:
                raise NotImplementedError(f"{what} with max_depth={self.max_depth} inside accumulate_weights: the weights address "
                                          f"the full tree's leaves; accumulate them on tree.lod({self.max_depth})")
        if self.lod_pixels is not None:                  # a footprint render reads the filled rows as well, cap or no cap
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError(f"{what} with lod_pixels={self.lod_pixels:g} on a tree that requires grad: there is no "
                                          "gradient through a footprint render; render under torch.no_grad()")
            if t._weight_accum is not None:
                raise NotImplementedError(f"{what} with lod_pixels={self.lod_pixels:g} inside accumulate_weights: the weights "
                                          "address leaves, a footprint render also reads the rows of cells that have a child")
        if not t._lod_filled:
            t.fill_internal_()
        if not capped:
            return t.render_view()
        if self._lod_of is not t.child:                  # every structure edit replaces tree.child by a new tensor
            self._lod_child, self._lod_of = t.lod_child(self.max_depth).contiguous(), t.child
        return oops.tree_view(self._lod_child, t.data.data, t.offset, t.invradius)

    def _cone(self, what, pixel_angle):
        """The cone of a footprint launch on explicit rays; None without lod_pixels (pixel_angle is then not looked at)."""
        if self.lod_pixels is None:
            return None
        if pixel_angle is None:
            raise ValueError(f"{what} with lod_pixels={self.lod_pixels:g} needs pixel_angle (radians per pixel for unit dirs): "
                             "explicit rays carry no pixel size")
        if isinstance(pixel_angle, bool) or not isinstance(pixel_angle, (int, float, np.integer, np.floating)) or \
                not 0 <= pixel_angle < float("inf"):
            raise ValueError(f"{what}(pixel_angle={pixel_angle!r}): must be a finite number >= 0")
        return self.lod_pixels * float(pixel_angle)

    def _camera_cone(self, fx, fy):
        return None if self.lod_pixels is None else self.lod_pixels / max(float(fx), float(fx if fy is None else fy))

    def _check_ndc_camera(self, width, height, fx, fy):
        """An NDC tree was built for ONE projection: a camera of another size or focal length renders rubbish without a word."""
        n = self.ndc
        if n is None:
            return
        if int(width) != n.width or int(height) != n.height or float(fx) != n.focal or (fy is not None and float(fy) != n.focal):
            raise ValueError(f"render_persp(width={width}, height={height}, fx={fx}, fy={fy}) does not match the renderer's "
                             f"{n!r}: an NDC tree renders only the projection it was extracted for")

    def render_persp(self, c2w, width=800, height=800, fx=1111.111, fy=None, fast=False, cuda=True):
        """[H,W,3] image.  With grad mode on and a tree whose `data` requires grad the exact render (fast=False, as in
        octree/optimization.py:216) is differentiable; the early-stopping preset (fast=True, evaluation) never is."""
        self._check_ndc_camera(width, height, fx, fy)
        c2w = torch.as_tensor(c2w, dtype=torch.float32, device=self.tree.device)
        view = self._view("render_persp")
        # nothing in a read-only tree (the palette form, the file's float16 rows) requires grad or accumulates weights: it is
        # rendered directly, with grad mode on as well, `fast` both ways
        differentiable = torch.is_grad_enabled() and self.tree.requires_grad
        accum = self.tree._weight_accum
        if accum is not None and not (differentiable and fast):
            # one more launch on the same camera and options; the rgb launches and their results are untouched
            oops.octree_weight_accum_cams(self.tree.view(), c2w[None], width, height, fx, self._opts(fast), accum.op,
                                          accum._buffer(), fy, ndc=self.ndc)
        if differentiable:
            if fast:
                # every fast=True call site of the reference sits under torch.no_grad() (octree/nerf/utils.py:276,
                # octree/evaluation.py:73); silently returning a detached image would surface later as an obscure
                # "does not require grad" error in the caller's backward
                raise oops.PxoError("render_persp(fast=True) is not differentiable: call it under torch.no_grad(), "
                                    "or use fast=False to optimise the tree")
            return _RenderPersp.apply(self.tree.data, self, c2w, width, height, fx, fy, self._opts(False))
        if self.lod_pixels is not None:
            return oops.octree_render_foot_persp(view, c2w, width, height, fx, self._opts(fast), self._camera_cone(fx, fy),
                                                 self.lod_min_depth, fy, **self.tree.basis_kwargs())
        return oops.octree_render_persp(view, c2w, width, height, fx, self._opts(fast), fy,
                                        **self._basis_kwargs())

    def forward(self, origins, dirs, viewdirs, fast=False, pixel_angle=None):
        """Colours [B,3] of explicit world-space rays (unit `dirs`); with `ndc` the rays are converted per ray and `viewdirs`
        (world space) shade them.  pixel_angle: with lod_pixels, the angle between neighbouring rays, radians per pixel."""
        cone = self._cone("forward", pixel_angle)
        view = self._view("forward")
        if cone is not None:
            return oops.octree_render_foot_rays(view, origins, dirs, viewdirs, self._opts(fast), cone, self.lod_min_depth,
                                                **self.tree.basis_kwargs())
        accum = self.tree._weight_accum
        if accum is not None:
            oops.octree_weight_accum_rays(self.tree.view(), origins, dirs, self._opts(fast), accum.op, accum._buffer(),
                                          ndc=self.ndc)
        return oops.octree_render_rays(view, origins, dirs, viewdirs, self._opts(fast), **self._basis_kwargs())

    __call__ = forward

    # ---- additions (no svox counterpart): opacity, expected distance and surface distance from the same march ----
    def _aux_view(self, what):
        if self.ndc is not None:
            raise NotImplementedError(f"{what} with NDC: alpha / depth / surface are not built for an NDC scene (the distances "
                                      "would be NDC lengths, not world distances)")
        if getattr(self.tree, "extra_data", None) is not None:
            raise NotImplementedError(f"{what} on an SG tree ({self.tree.data_format}): alpha / depth / surface are built for SH "
                                      "trees only")
        view = self._view(what)                          # a capped view has refusals of its own, by name
        if torch.is_grad_enabled() and self.tree.requires_grad:
            raise oops.PxoError(f"{what} is not differentiable (alpha, depth and surface have no gradient kernel): call it "
                                "under torch.no_grad()")
        return view

    @staticmethod
    def _aux_dict(rgb, aux):
        return {"rgb": rgb, "alpha": aux[..., 0], "depth": aux[..., 1], "surface": aux[..., 2]}

    def render_persp_aux(self, c2w, width=800, height=800, fx=1111.111, fy=None, fast=False, surface_thresh=0.5):
        """dict(rgb [H,W,3], alpha [H,W], depth [H,W], surface [H,W]): render_persp's image with, per pixel, the opacity (sum
        of the compositing weights), the expected termination distance (sum of weight x sample distance, not divided by
        alpha) and the distance at which the transmittance first falls to `surface_thresh` (+inf where it never does).
        Distances are Euclidean, in world units, from the ray origin.  Not differentiable."""
        view = self._aux_view("render_persp_aux")
        c2w = torch.as_tensor(c2w, dtype=torch.float32, device=self.tree.device)
        if self.lod_pixels is not None:
            return self._aux_dict(*oops.octree_render_foot_persp(view, c2w, width, height, fx, self._opts(fast),
                                                                 self._camera_cone(fx, fy), self.lod_min_depth, fy,
                                                                 surface_thresh=surface_thresh))
        return self._aux_dict(*oops.octree_render_aux_persp(view, c2w, width, height, fx, self._opts(fast), fy, surface_thresh))

    def forward_aux(self, origins, dirs, viewdirs, fast=False, surface_thresh=0.5, pixel_angle=None):
        """render_persp_aux for explicit world-space rays (unit `dirs`): rgb [B,3], alpha / depth / surface [B].  pixel_angle:
        as in forward."""
        cone = self._cone("forward_aux", pixel_angle)
        view = self._aux_view("forward_aux")
        if cone is not None:
            return self._aux_dict(*oops.octree_render_foot_rays(view, origins, dirs, viewdirs, self._opts(fast), cone,
                                                                self.lod_min_depth, surface_thresh=surface_thresh))
        return self._aux_dict(*oops.octree_render_aux_rays(view, origins, dirs, viewdirs, self._opts(fast), surface_thresh))


# ---- scenes (an addition, no svox counterpart): several trees in one world, each under its own transform ------------------
class Instance:
    """A tree placed in a scene: x_world = scale * rotation @ x_object + translation.

    rotation: 3x3, orthonormal with det +1 (within 1e-5, checked in float64); translation: 3 finite numbers; scale: finite, > 0.
    matrix=: instead of the three, a 3x3 (scale * rotation) or 4x4 ([scale * rotation | translation; 0 0 0 1]) matrix, from
    which the uniform scale is extracted (cbrt of the determinant); non-uniform scale and shear fail the rotation check.
    Float SH N3Tree only: a QuantizedN3Tree, a HalfN3Tree and an SG tree are refused by name."""

    def __init__(self, tree, rotation=None, translation=None, scale=None, matrix=None):
        if isinstance(tree, _ReadOnlyTree):
            raise NotImplementedError(f"Instance of a {tree.NOUN}: a scene renders float SH trees only; call tree.{tree.WAY_OUT}() "
                                      "for an N3Tree")
        if not isinstance(tree, N3Tree):
            raise TypeError(f"Instance(tree): expected an svox.N3Tree, got {type(tree).__name__}")
        if getattr(tree, "extra_data", None) is not None:
            raise NotImplementedError(f"Instance of an SG tree ({tree.data_format}): a scene renders SH trees only")
        if matrix is not None:
            if rotation is not None or translation is not None or scale is not None:
                raise ValueError("Instance(matrix=...) excludes rotation, translation and scale")
            m = np.asarray(matrix, np.float64)
            if m.shape == (4, 4):
                if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
                    raise ValueError(f"Instance(matrix=...): the last row of a 4x4 matrix must be (0, 0, 0, 1), got {m[3].tolist()}")
                translation, m = m[:3, 3], m[:3, :3]
            elif m.shape != (3, 3):
                raise ValueError(f"Instance(matrix=...): expected a 3x3 or 4x4 matrix, got shape {m.shape}")
            det = np.linalg.det(m) if np.isfinite(m).all() else np.nan
            if not (np.isfinite(det) and det > 0):
                raise ValueError(f"Instance(matrix=...): determinant {det} is not finite and > 0 (no reflection, no collapse)")
            scale = float(np.cbrt(det))
            rotation = m / scale
        self.tree = tree
        self.rotation = np.eye(3) if rotation is None else np.asarray(rotation, np.float64)
        self.translation = np.zeros(3) if translation is None else np.asarray(translation, np.float64)
        self.scale = 1.0 if scale is None else scale
        if isinstance(self.scale, bool) or not isinstance(self.scale, (int, float, np.integer, np.floating)) or \
                not (np.isfinite(self.scale) and self.scale > 0 and np.isfinite(np.float32(self.scale))
                     and np.float32(self.scale) > 0):
            raise ValueError(f"Instance(scale={scale!r}): must be a finite number > 0")
        self.scale = float(self.scale)
        R = self.rotation
        if R.shape != (3, 3) or not np.isfinite(R).all():
            raise ValueError(f"Instance(rotation=...): expected a finite 3x3 matrix, got shape {R.shape}")
        if np.abs(R.T @ R - np.eye(3)).max() > 1e-5 or abs(np.linalg.det(R) - 1.0) > 1e-5:
            raise ValueError("Instance(rotation=...): not a rotation (R^T R = I and det R = +1 within 1e-5); non-uniform scale, "
                             "shear and reflections are not built")
        if self.translation.shape != (3,) or not np.isfinite(self.translation).all():
            raise ValueError(f"Instance(translation=...): expected 3 finite numbers, got {self.translation!r}")

    def __repr__(self):
        return f"svox.Instance({self.tree!r}, scale={self.scale:g}, translation={self.translation.tolist()})"


class SceneRenderer:
    """Renders 1 .. 8 Instances together (the definition: include/plenoctree_octree.h, "scene"): every ray is
    carried into each object's frame, the view direction with it, and the trees are marched in one loop with one compositing
    sample per round, so overlapping objects blend by density and a scaled object keeps its opacity.  Forward only.

    Refused by name: ndc, max_depth / lod_pixels, a tree that requires grad with grad mode on, a render inside
    accumulate_weights, and (by Instance) the read-only and SG forms.  A one-instance scene still runs the scene kernel.
    The device records are rebuilt whenever a tree's `child` or `data` tensor has been replaced since the last render."""

    def __init__(self, instances, step_size=1e-3, background_brightness=1.0, ndc=None, max_depth=None, lod_pixels=None):
        if ndc is not None:
            raise NotImplementedError("SceneRenderer(ndc=...): NDC scenes are not built (an NDC tree lives in one camera's "
                                      "projection, not in a world that objects can share)")
        if max_depth is not None or lod_pixels:
            raise NotImplementedError("SceneRenderer(max_depth=... / lod_pixels=...): level of detail is not built for a scene; "
                                      "place tree.lod(L) as the instance instead")
        instances = list(instances)
        if not 1 <= len(instances) <= oops._lib.SCENE_MAX_INSTANCES:
            raise ValueError(f"SceneRenderer: a scene takes 1 .. {oops._lib.SCENE_MAX_INSTANCES} instances, got {len(instances)}")
        for i in instances:
            if not isinstance(i, Instance):
                raise TypeError(f"SceneRenderer: expected svox.Instance objects, got {type(i).__name__}")
        if len({i.tree.device for i in instances}) != 1:
            raise ValueError("SceneRenderer: the instances' trees must live on one device")
        self.instances = instances
        self.step_size = float(step_size)
        self.background_brightness = float(background_brightness)
        self._scene, self._scene_of = None, None

    @property
    def device(self):
        return self.instances[0].tree.device

    def _opts(self, fast):
        thr = 1e-2 if fast else 0.0
        return oops.render_opts(self.step_size, self.background_brightness, thr, thr)

    def _records(self, what):
        for k, i in enumerate(self.instances):
            t = i.tree
            if torch.is_grad_enabled() and t.requires_grad:
                raise NotImplementedError(f"SceneRenderer.{what}: instance {k}'s tree requires grad and there is no gradient "
                                          "through a scene; render under torch.no_grad()")
            if t._weight_accum is not None:
                raise NotImplementedError(f"SceneRenderer.{what} inside accumulate_weights (instance {k}): the weights of a "
                                          "scene's samples are shared between trees; accumulate them with a VolumeRenderer")
        # a structure edit replaces tree.child, an assignment to tree.data the parameter, one to tree.data.data its storage
        now = tuple((i.tree.child, i.tree.data, i.tree.data.data_ptr()) for i in self.instances)
        if self._scene_of is None or any(a[0] is not b[0] or a[1] is not b[1] or a[2] != b[2]
                                         for a, b in zip(now, self._scene_of)):
            self._scene = oops.scene_instances([(i.tree.view(), i.rotation, i.translation, i.scale) for i in self.instances],
                                               self.device)
            self._scene_of = now                     # also keeps the tensors the records point into alive
        return self._scene

    def render_persp(self, c2w, width=800, height=800, fx=1111.111, fy=None, fast=False):
        """[H,W,3] image of the scene from a world-space pinhole camera."""
        scene = self._records("render_persp")
        c2w = torch.as_tensor(c2w, dtype=torch.float32, device=self.device)
        return oops.scene_render_persp(scene, c2w, width, height, fx, self._opts(fast), fy)

    def forward(self, origins, dirs, viewdirs, fast=False):
        """Colours [B,3] of explicit world-space rays (unit `dirs`); `viewdirs` shade them, rotated into each object's frame."""
        return oops.scene_render_rays(self._records("forward"), origins, dirs, viewdirs, self._opts(fast))

    __call__ = forward


# ---- svox.helpers._get_c_extension(): the slice of svox's native module the reference touches ---------------------------
class _RenderOptions:
    """svox.csrc RenderOptions as filled in by octree/extraction.py:184-195."""

    def __init__(self):
        self.step_size = 1e-3
        self.background_brightness = 1.0
        self.sigma_thresh = 0.0
        self.stop_thresh = 0.0
        self.ndc_width, self.ndc_height, self.ndc_focal = -1, -1, -1.0


class _CameraSpec:
    """svox.csrc CameraSpec (octree/extraction.py:197-203)."""

    def __init__(self):
        self.c2w = None
        self.fx = self.fy = 0.0
        self.width = self.height = 0


def _grid_weight_render(grid_data, cam, opts, offset, invradius):
    """_C.grid_weight_render (octree/extraction.py:205-211): (max compositing weight per voxel, hit mask) of one camera
    through the dense sigma grid [reso, reso, reso]."""
    ndc = None
    if getattr(opts, "ndc_width", -1) > 0:              # octree/extraction.py:190-193: set for LLFF scenes, -1 otherwise
        ndc = NDCConfig(opts.ndc_width, opts.ndc_height, opts.ndc_focal)
    reso = grid_data.shape[0]
    o = oops.render_opts(opts.step_size, opts.background_brightness, opts.sigma_thresh, opts.stop_thresh)
    c2w = torch.as_tensor(cam.c2w, dtype=torch.float32, device=grid_data.device)[None, :3, :4]
    w = oops.grid_weight_render(grid_data.contiguous().reshape(-1), reso, c2w, cam.fx, cam.fy, cam.width, cam.height, o,
                                offset, invradius, **({} if ndc is None else {"ndc": ndc}))
    w = w.reshape(reso, reso, reso)
    return w, w > 0


def _quantize_median_cut(data, weights, order):
    """_C.quantize_median_cut(data [n,3], weights [n] or empty, order) -> (colors [2^order, 3] float32, color_id_map [n]
    int32), as called by octree/compression.py:114-116.

    Median cut (Heckbert): `order` rounds, every box split at its (weighted) median along the axis of its largest extent,
    lower half first, so box b of a round becomes boxes 2b and 2b+1 of the next; a colour is the (weighted) mean of its
    box, a point's id the index of its box.  All boxes of a round are split at once (two stable sorts per round), in
    torch on whatever device `data` lives on.  svox's native implementation is not in the reference tree: this follows
    the published algorithm and the call site's contract (shapes, dtypes, id range), not svox's tie-breaking - parity
    unpinned, like the rest of the svox surface.  Boxes that run empty (n < 2^order) get colour 0."""
    x = torch.as_tensor(data).detach().to(torch.float32)
    if x.dim() != 2:
        raise ValueError("quantize_median_cut: data must be [n, channels]")
    n, dev = x.shape[0], x.device
    nbox = 1 << int(order)
    colors = torch.zeros(nbox, x.shape[1], dtype=torch.float32, device=dev)
    if n == 0:
        return colors, torch.zeros(0, dtype=torch.int32, device=dev)
    w = torch.as_tensor(weights).detach().to(torch.float32).to(dev).reshape(-1)
    weighted = w.numel() == n
    if not weighted:
        w = torch.ones(n, dtype=torch.float32, device=dev)
    box = torch.zeros(n, dtype=torch.int64, device=dev)
    for level in range(int(order)):
        nb = 1 << level
        lo = torch.full((nb, x.shape[1]), float("inf"), device=dev).scatter_reduce_(
            0, box[:, None].expand_as(x), x, "amin", include_self=True)
        hi = torch.full((nb, x.shape[1]), float("-inf"), device=dev).scatter_reduce_(
            0, box[:, None].expand_as(x), x, "amax", include_self=True)
        axis = (hi - lo).argmax(dim=1)                                   # per box; empty boxes give nan -> axis 0, unused
        key = x.gather(1, axis[box][:, None])[:, 0]
        order1 = torch.sort(key, stable=True).indices                    # by value ...
        order2 = torch.sort(box[order1], stable=True).indices            # ... then by box, values staying sorted
        perm = order1[order2]
        pbox = box[perm]
        start = torch.zeros(nb + 1, dtype=torch.int64, device=dev)
        start[1:] = torch.bincount(pbox, minlength=nb).cumsum(0)
        rank = torch.arange(n, device=dev) - start[pbox]
        size = (start[1:] - start[:-1])[pbox]
        if weighted:                                                      # first point at which half of the box's weight is reached
            cw = torch.cumsum(w[perm].double(), 0)
            base = torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), cw])[start[pbox]]
            total = (torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), cw])[start[1:]] - \
                     torch.cat([torch.zeros(1, dtype=torch.float64, device=dev), cw])[start[:-1]])[pbox]
            upper = (cw - base) > 0.5 * total
            upper &= rank > 0                                             # never leave the lower half empty ...
            upper |= (rank == size - 1) & (size > 1)                      # ... nor the upper one
        else:
            upper = rank >= size // 2                                     # nth_element at begin + size / 2
        new_box = torch.empty_like(box)
        new_box[perm] = 2 * pbox + upper.to(torch.int64)
        box = new_box
    wsum = torch.zeros(nbox, dtype=torch.float64, device=dev).index_add_(0, box, w.double())
    acc = torch.zeros(nbox, x.shape[1], dtype=torch.float64, device=dev).index_add_(0, box, x.double() * w.double()[:, None])
    filled = wsum > 0
    colors[filled] = (acc[filled] / wsum[filled][:, None]).float()
    return colors, box.to(torch.int32)


def _get_c_extension():
    return types.SimpleNamespace(RenderOptions=_RenderOptions, CameraSpec=_CameraSpec, grid_weight_render=_grid_weight_render,
                                 quantize_median_cut=_quantize_median_cut)


helpers = types.ModuleType(__name__ + ".helpers")
helpers._get_c_extension = _get_c_extension
helpers.__doc__ = "svox.helpers: `_get_c_extension()` as imported by octree/extraction.py:57 and octree/compression.py:34."


def install_as_svox():
    """Registers this module as `svox` (and `svox.helpers`), so that `import svox` / `from svox import N3Tree` /
    `from svox.helpers import _get_c_extension` in the reference's drivers resolve here."""
    import sys
    me = sys.modules[__name__]
    sys.modules["svox"] = me
    sys.modules["svox.helpers"] = helpers
    return me
