"""The model families of the NeRF side -- the plain NeRF-SH, NeRF-SG (sg_dim > 0) and the view-conditioned "vanilla" head
(use_viewdirs) -- as ONE table: what each rejects, what it is built for, how its model and state are made, which checkpoints
it reads, what octree.extraction needs from it.  nerf_sh.train, nerf_sh.eval, nerf_sh.gen_video, nerf_sh.gen_mesh and
octree.extraction ask select / check / restore and hold no family branch of their own; a new family, or a family built for one
more purpose, is one entry here.
"""
import collections

from . import checkpoints, models, occupancy, sg, utils, viewdirs

PURPOSES = ("train", "render", "extract", "mesh")      # nerf_sh.train | eval, gen_video | octree.extraction | nerf_sh.gen_mesh

Family = collections.namedtuple("Family", (
    "name",
    "selects",       # args -> whether the flags ask for this family; FAMILIES is tried in its order
    "checks",        # purpose the family is built for -> (how its refusal opens, its clauses in the order they are named)
    "instead",       # purpose it is not built for -> the families whose check answers: the first of them that `selects`
    "construct",     # (args, device, purpose) -> (model, state) with fresh parameters
    "loading",       # args -> the line that goes before a checkpoint read that reports itself
    "checkpoint",    # purpose -> Policy
    "n_params",      # (args, state) -> trainable scalars, for the line nerf_sh.train opens with
    "tree",          # (args, state) -> (data_format, basis_dim, extra_data) of the PlenOctree extracted from it
    "projection",    # (args, device) -> the directions step 2 of the extraction projects onto SH with; None: the network's own
))                   # coefficients are averaged

# formats: what is looked for, in this order unless --is_jaxnerf_ckpt says flax; absent: "fresh" goes on, without a word, with
# the freshly initialised network (and then says nothing about what it read either), "raises" is a FileNotFoundError
Policy = collections.namedtuple("Policy", ("formats", "absent", "load"))      # load(args, state) -> what to say, or None


# ---- checkpoints: today's policy, one row per way of reading ---------------------------------------------------------------
def _flax_if_any(args, state):
    """get_model_state (nerf_sh/nerf/models.py:38-49): the newest flax `checkpoint_<step>` of train_dir if there is one --
    parameters, Adam moments and step, so a training run resumes."""
    if args.train_dir:
        checkpoints.restore_checkpoint(args.train_dir, state)


def load_nerf_checkpoint(args, state):
    """get_model_state(args, restore=True) of octree/nerf/models.py:38-49.  The reference reads one of two formats, chosen by
    --is_jaxnerf_ckpt (:45): a flax-msgpack `checkpoint_<step>` of nerf_sh.train (restore_model_state_from_jaxnerf, :66-113) or
    a torch state dict `*.ckpt` of its torch twin (restore_model_state, :52-63).  Both are read here.  Where the reference, with
    no file of the chosen format in train_dir, silently goes on with the freshly initialised network, this raises -- except that
    without the flag a train_dir holding only flax checkpoints (what nerf_sh.train here and the reference's JAX trainer write)
    is read as such, and said so."""
    if args.is_jaxnerf_ckpt:
        path = checkpoints.restore_checkpoint(args.train_dir, state)
        if path is None:
            raise FileNotFoundError(f"--is_jaxnerf_ckpt: no flax checkpoint_<step> in {args.train_dir}")
        return f"* restore ckpt from {path} (flax msgpack)"
    path = checkpoints.restore_torch_checkpoint(args.train_dir, state, trust_pickle=bool(getattr(args, "trust_ckpt_pickle", False)))
    if path is not None:
        return f"* restore ckpt from {path}. (torch state dict)"
    path = checkpoints.restore_checkpoint(args.train_dir, state)
    if path is None:
        raise FileNotFoundError(f"no *.ckpt (torch state dict) and no checkpoint_<step> (flax msgpack) in {args.train_dir}: "
                                "nothing to extract from")
    return f"* no *.ckpt in {args.train_dir}: restore ckpt from {path} (flax msgpack, as with --is_jaxnerf_ckpt)"


def _viewdirs_either(args, state):
    return checkpoints.restore_viewdirs_checkpoint(args.train_dir, state, bool(getattr(args, "is_jaxnerf_ckpt", False)),
                                                   bool(getattr(args, "trust_ckpt_pickle", False)))


RESUME = Policy(("flax",), "fresh", _flax_if_any)
EITHER = Policy(("torch", "flax"), "raises", load_nerf_checkpoint)
EITHER_VIEWDIRS = Policy(("torch", "flax"), "raises", _viewdirs_either)


# ---- the clauses only some families reject (utils.COMMON_CLAUSES holds the rest) ---------------------------------------------
def _no_sg(a):
    return a.sg_dim > 0 and "sg_dim>0 (spherical gaussians)"


def _render_path_off_llff(a):
    """check_supported's wording of the common clause: an SH model on an LLFF scene renders the scene's camera path."""
    words = utils.COMMON_CLAUSES["render_path"](a)
    return words and a.dataset != "llff" and words


def _sg_dim(a):
    if a.sg_dim <= 0:
        return f"sg_dim={a.sg_dim} (an SH model: the plain path)"
    return (a.sg_dim not in sg.SUPPORTED_DIMS
            and f"sg_dim={a.sg_dim} (need one of {sg.SUPPORTED_DIMS}: the widths of the MLP head and the renderers)")


def _occupancy_render(a):
    """--occupancy_reso R (nerf/occupancy.py) in nerf_sh.eval / nerf_sh.gen_video: what of it is not built."""
    return "; ".join(occupancy.clauses(a))


def _occupancy_elsewhere(a):
    return occupancy.wanted(a) and ("occupancy_reso (the grid of --occupancy_reso serves the renders of nerf_sh.eval and "
                                    "nerf_sh.gen_video: culling inside training and its test renders is --cull_reso of nerf_sh.train, "
                                    "culling in the extraction or meshing is not built)")


def _cull_train(a):
    """--cull_reso R (nerf/occupancy.py TrainingGrid) in nerf_sh.train with an SH model: what of it is not built."""
    return "; ".join(occupancy.cull_clauses(a))


def _cull_train_sg(a):
    return occupancy.cull_wanted(a) and "cull_reso with sg_dim>0 (training a NeRF-SG through the occupancy grid is not built)"


def _cull_elsewhere(a):
    return occupancy.cull_wanted(a) and ("cull_reso (the grid that follows a model is nerf_sh.train's: eval and gen_video take "
                                         "--occupancy_reso, culling in the extraction or meshing is not built)")


def _with_occupancy(clauses, purpose, cull_train=_cull_train):
    """`clauses` plus the family's answer to the two grids: --occupancy_reso is the renderers', --cull_reso is nerf_sh.train's."""
    return clauses + ((_occupancy_render if purpose == "render" else _occupancy_elsewhere),
                      (cull_train if purpose == "train" else _cull_elsewhere))


_SH_CLAUSES = (lambda a: a.use_viewdirs and "use_viewdirs=true (vanilla NeRF head)",
               lambda a: (a.sh_deg < 0 or a.sh_deg > 4) and f"sh_deg={a.sh_deg} (need 0..4)",
               _no_sg, "trunk", "posenc", "noise_std", _render_path_off_llff, "legacy_posenc_order", "activations")

_SG_CLAUSES = (_sg_dim,
               lambda a: a.sh_deg != -1 and f"sh_deg={a.sh_deg} (need -1: you can only use up to one of SH or SG)",
               lambda a: a.use_viewdirs and "use_viewdirs=true (an SG model has no view-conditioned head)",
               "trunk", "posenc", "channels", "noise_std", "render_path", utils.llff_clause("an SG model"), "legacy_posenc_order",
               "activations")

_VD_HEAD = (lambda a: not a.use_viewdirs and "use_viewdirs=false (an SH model: the plain path)",
            lambda a: a.net_depth_condition != 1 and f"net_depth_condition={a.net_depth_condition} (need 1)",
            lambda a: a.net_width_condition != 128 and f"net_width_condition={a.net_width_condition} (need 128)",
            lambda a: a.deg_view != 4 and f"deg_view={a.deg_view} (need 4)")
_VD_TRUNK = (_no_sg, "legacy_posenc_order", "trunk", "posenc", "channels",
             lambda a: (getattr(a, "mlp_precision", "f32") != "f32"
                        and f"mlp_precision={a.mlp_precision} (the view-conditioned head is float32 only)"))
_VD_SCENE = ("render_path", utils.llff_clause("the view-conditioned head"),
             lambda a: (a.net_activation.lower(), a.sigma_activation.lower()) != ("relu", "relu") and "activations other than relu")
# the SH projection reads sh_deg and projection_samples and never the rgb activation (it projects the raw rgb); the ray renderer
# takes any sh_deg (the reference's rendering presets say -1) and reads what a renderer reads
_VD_PROJECTION = (_VD_HEAD
                  + (lambda a: (a.sh_deg < 0 or a.sh_deg > 4) and f"sh_deg={a.sh_deg} (the projection needs 0..4)",)
                  + _VD_TRUNK
                  + (lambda a: (getattr(a, "projection_samples", 1) < 1
                                and f"projection_samples={a.projection_samples} (need >= 1)"),)
                  + _VD_SCENE)
_VD_RENDER = (_VD_HEAD + _VD_TRUNK + _VD_SCENE
              + (lambda a: a.rgb_activation.lower() != "sigmoid" and "rgb_activation other than sigmoid", "noise_std"))


# ---- the table ---------------------------------------------------------------------------------------------------------------
def _sh_tree(args, state):
    basis_dim = (args.sh_deg + 1) ** 2
    return f"SH{basis_dim}", basis_dim, None


# A view-dependent ("vanilla") NeRF: eval, gen_video and octree.extraction opt in explicitly; the extraction projects its radiance
# onto SH of degree --sh_deg (octree/extraction.py:362-375).  Training and meshing with this head are not built, and the check
# that says so is the one the flags would get without use_viewdirs -- in nerf_sh.train the SG check when sg_dim > 0 -- whose
# use_viewdirs clause always refuses.
VIEWDIRS = Family(
    name="viewdirs",
    selects=lambda a: a.use_viewdirs,
    checks={"render": ("rendering a view-dependent NeRF, ", _with_occupancy(_VD_RENDER, "render")),
            "extract": ("SH projection of a view-dependent NeRF, ", _with_occupancy(_VD_PROJECTION, "extract"))},
    instead={"train": ("sg", "sh"), "mesh": ("sh",)},
    construct=viewdirs.get_model_state,
    loading=lambda a: "* Loading NeRF (view-conditioned head)",
    checkpoint={"render": EITHER_VIEWDIRS, "extract": EITHER_VIEWDIRS},
    n_params=None,
    tree=_sh_tree,
    projection=lambda a, device: viewdirs.draw_directions(a.seed, a.projection_samples, device))

# A NeRF-SG (--sg_dim K --sh_deg -1; octree/extraction.py:436-442, :481-499): the SH steps with the head width of sg_dim, the
# tree takes the lobes as extra_data.  gen_mesh needs the sigma head and, for --color view, the lobes: the renderer's check.
SG = Family(
    name="sg",
    selects=lambda a: a.sg_dim > 0,
    checks={"train": ("training a NeRF-SG, ", _with_occupancy(_SG_CLAUSES, "train", _cull_train_sg)),
            "render": ("rendering a NeRF-SG, ", _with_occupancy(_SG_CLAUSES, "render")),
            "extract": ("extraction of an SG PlenOctree, ", _with_occupancy(_SG_CLAUSES, "extract")),
            "mesh": ("rendering a NeRF-SG, ", _with_occupancy(_SG_CLAUSES, "mesh"))},
    instead={},
    construct=sg.get_model_state,
    loading=lambda a: f"* Loading NeRF (SG{a.sg_dim})",
    checkpoint={"train": RESUME, "render": EITHER, "extract": EITHER, "mesh": EITHER},
    n_params=lambda a, state: 2 * state.n_mlp + 3 * a.sg_dim,
    tree=lambda a, state: (f"SG{a.sg_dim}", a.sg_dim, state.lobes),                   # :437-442
    projection=None)

SH = Family(
    name="sh",
    selects=lambda a: True,
    checks={purpose: ("", _with_occupancy(_SH_CLAUSES, purpose)) for purpose in PURPOSES},
    instead={},
    construct=lambda a, device, purpose: models.get_model_state(a, device, restore=False, purpose=purpose),
    loading=lambda a: "* Loading NeRF",
    checkpoint={"train": RESUME, "render": RESUME, "extract": EITHER, "mesh": RESUME},
    n_params=lambda a, state: 2 * state.n_mlp,
    tree=_sh_tree,
    projection=None)

FAMILIES = (VIEWDIRS, SG, SH)                 # the order of precedence: use_viewdirs, then sg_dim > 0, else SH
_BY_NAME = {f.name: f for f in FAMILIES}


def select(args):
    return next(f for f in FAMILIES if f.selects(args))


def check_flags(family, args, purpose="render"):
    """What `family` builds for `purpose`; everything else is rejected by name, all of it in one NotImplementedError."""
    opening, clauses = family.checks[purpose]
    bad = utils.unbuilt_flags(args, clauses)
    if bad:
        raise NotImplementedError(opening + "not built on the MI355X path: " + "; ".join(bad))


def check(args, purpose, require_data=True, world_size=1):
    """The flag check of an entry point: the directory (and, for training, batch-size) checks, then the clauses of the family
    the flags select -- or, where that family is not built for `purpose`, of the family its entry names instead."""
    utils.check_dirs(args, require_data, purpose == "train", world_size)
    family = select(args)
    if purpose not in family.checks:
        family = next(f for f in map(_BY_NAME.get, family.instead[purpose]) if f.selects(args))
    check_flags(family, args, purpose)


def load_checkpoint(family, purpose, args, state, say=print):
    """The checkpoint step of `restore`: the family's policy for `purpose`, and what it reports."""
    said = family.checkpoint[purpose].load(args, state)
    if said:
        say(said, flush=True)


def restore(args, device, purpose, say=print, require_data=True):
    """(model, state) of the family the flags select, as `purpose` wants it: flag checks, model + state, checkpoint."""
    check(args, purpose, require_data)
    family = select(args)
    if family.checkpoint[purpose].absent == "raises":
        say(family.loading(args), flush=True)
    model, state = family.construct(args, device, purpose)
    load_checkpoint(family, purpose, args, state, say)
    return model, state
