"""The family table (plenoctree_amd/nerf_sh/nerf/families.py) on the CPU: which family a command line selects and, word for word,
what every (family, purpose) refuses.  The expected messages are literals.  They were recorded once, before the clauses were
moved, by running the functions the table replaced (utils.check_flags, sg.check_dirs, viewdirs.check_render_dirs,
extraction.check_viewdirs_flags, routed as the five entry points routed them) on these same argument sets.  Likewise the call
log of the train step: what sg.train_step and models.train_step asked of `ops` before they became one."""
import argparse
import types

import pytest
import torch

from plenoctree_amd import _lib, ops
from plenoctree_amd.nerf_sh.nerf import families, models, sg, utils
from plenoctree_amd.octree import extraction

PURPOSES = ("train", "render", "extract", "mesh")
BASES = {"sh": dict(use_viewdirs=False, sh_deg=4),
         "sg": dict(use_viewdirs=False, sg_dim=25, sh_deg=-1),
         "vd": dict(use_viewdirs=True, sh_deg=4)}
FAMILY = {"sh": families.SH, "sg": families.SG, "vd": families.VIEWDIRS}
# one flag each, none of which changes the family that is selected; a flag that a combination does not name below passes its check
MUTATIONS = {
    "sh_deg_7": dict(sh_deg=7),
    "sh_deg_-1": dict(sh_deg=-1),
    "trunk": dict(net_width=128),
    "posenc": dict(max_deg_point=8),
    "channels": dict(num_rgb_channels=4),
    "legacy_posenc_order": dict(legacy_posenc_order=True),
    "net_activation": dict(net_activation="tanh"),
    "rgb_activation": dict(rgb_activation="relu"),
    "sigma_activation": dict(sigma_activation="softplus"),
    "noise_std": dict(noise_std=-1.0),
    "render_path": dict(render_path=True),
    "spherify": dict(spherify=True),
    "llff": dict(dataset="llff"),
    "llff_render_path": dict(dataset="llff", render_path=True),
    "net_depth_condition": dict(net_depth_condition=2),
    "net_width_condition": dict(net_width_condition=64),
    "deg_view": dict(deg_view=2),
    "mlp_precision": dict(mlp_precision="bf16x3"),
    "projection_samples": dict(projection_samples=0),
    "sg_dim_7": dict(sg_dim=7),                      # applied to the SG base only: elsewhere it would select another family
    # every offending flag at once: the clauses come in the order the message names them
    "all": dict(sh_deg=7, net_width=128, max_deg_point=8, num_rgb_channels=4, legacy_posenc_order=True, net_activation="tanh",
                rgb_activation="relu", noise_std=-1.0, render_path=True, dataset="llff", net_depth_condition=2,
                net_width_condition=64, deg_view=2, mlp_precision="bf16x3", projection_samples=0),
}

# (family, purpose) -> offending flag -> the text of the NotImplementedError.  The SH text is that of all four purposes; SG's
# `mesh` is its `render` (gen_mesh takes the renderer's check).
REFUSED = {
    ("sh", "train"): {
        "all": "not built on the MI355X path: sh_deg=7 (need 0..4); net_depth/net_width/skip_layer != 8/256/4; "
               "min/max_deg_point != 0/10; noise_std < 0; legacy_posenc_order; activations other than relu/sigmoid/relu",
        "legacy_posenc_order": "not built on the MI355X path: legacy_posenc_order",
        "net_activation": "not built on the MI355X path: activations other than relu/sigmoid/relu",
        "noise_std": "not built on the MI355X path: noise_std < 0",
        "posenc": "not built on the MI355X path: min/max_deg_point != 0/10",
        "render_path": "not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "rgb_activation": "not built on the MI355X path: activations other than relu/sigmoid/relu",
        "sh_deg_-1": "not built on the MI355X path: sh_deg=-1 (need 0..4)",
        "sh_deg_7": "not built on the MI355X path: sh_deg=7 (need 0..4)",
        "sigma_activation": "not built on the MI355X path: activations other than relu/sigmoid/relu",
        "spherify": "not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "trunk": "not built on the MI355X path: net_depth/net_width/skip_layer != 8/256/4",
    },
    ("sg", "train"): {
        "all": "training a NeRF-SG, not built on the MI355X path: sh_deg=7 (need -1: you can only use up to one of SH or SG); "
               "net_depth/net_width/skip_layer != 8/256/4; min/max_deg_point != 0/10; num_rgb_channels/num_sigma_channels != "
               "3/1; noise_std < 0; render_path / spherify (LLFF scenes); dataset=llff (LLFF scenes: an SG model on a "
               "forward-facing scene is not built); legacy_posenc_order; activations other than relu/sigmoid/relu",
        "channels": "training a NeRF-SG, not built on the MI355X path: num_rgb_channels/num_sigma_channels != 3/1",
        "legacy_posenc_order": "training a NeRF-SG, not built on the MI355X path: legacy_posenc_order",
        "llff": "training a NeRF-SG, not built on the MI355X path: dataset=llff (LLFF scenes: an SG model on a forward-facing "
                "scene is not built)",
        "llff_render_path": "training a NeRF-SG, not built on the MI355X path: render_path / spherify (LLFF scenes); "
                            "dataset=llff (LLFF scenes: an SG model on a forward-facing scene is not built)",
        "net_activation": "training a NeRF-SG, not built on the MI355X path: activations other than relu/sigmoid/relu",
        "noise_std": "training a NeRF-SG, not built on the MI355X path: noise_std < 0",
        "posenc": "training a NeRF-SG, not built on the MI355X path: min/max_deg_point != 0/10",
        "render_path": "training a NeRF-SG, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "rgb_activation": "training a NeRF-SG, not built on the MI355X path: activations other than relu/sigmoid/relu",
        "sg_dim_7": "training a NeRF-SG, not built on the MI355X path: sg_dim=7 (need one of (1, 4, 9, 16, 25): the widths of "
                    "the MLP head and the renderers)",
        "sh_deg_7": "training a NeRF-SG, not built on the MI355X path: sh_deg=7 (need -1: you can only use up to one of SH or "
                    "SG)",
        "sigma_activation": "training a NeRF-SG, not built on the MI355X path: activations other than relu/sigmoid/relu",
        "spherify": "training a NeRF-SG, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "trunk": "training a NeRF-SG, not built on the MI355X path: net_depth/net_width/skip_layer != 8/256/4",
    },
    ("sg", "render"): {
        "all": "rendering a NeRF-SG, not built on the MI355X path: sh_deg=7 (need -1: you can only use up to one of SH or "
               "SG); net_depth/net_width/skip_layer != 8/256/4; min/max_deg_point != 0/10; "
               "num_rgb_channels/num_sigma_channels != 3/1; noise_std < 0; render_path / spherify (LLFF scenes); dataset=llff "
               "(LLFF scenes: an SG model on a forward-facing scene is not built); legacy_posenc_order; activations other "
               "than relu/sigmoid/relu",
        "channels": "rendering a NeRF-SG, not built on the MI355X path: num_rgb_channels/num_sigma_channels != 3/1",
        "legacy_posenc_order": "rendering a NeRF-SG, not built on the MI355X path: legacy_posenc_order",
        "llff": "rendering a NeRF-SG, not built on the MI355X path: dataset=llff (LLFF scenes: an SG model on a "
                "forward-facing scene is not built)",
        "llff_render_path": "rendering a NeRF-SG, not built on the MI355X path: render_path / spherify (LLFF scenes); "
                            "dataset=llff (LLFF scenes: an SG model on a forward-facing scene is not built)",
        "net_activation": "rendering a NeRF-SG, not built on the MI355X path: activations other than relu/sigmoid/relu",
        "noise_std": "rendering a NeRF-SG, not built on the MI355X path: noise_std < 0",
        "posenc": "rendering a NeRF-SG, not built on the MI355X path: min/max_deg_point != 0/10",
        "render_path": "rendering a NeRF-SG, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "rgb_activation": "rendering a NeRF-SG, not built on the MI355X path: activations other than relu/sigmoid/relu",
        "sg_dim_7": "rendering a NeRF-SG, not built on the MI355X path: sg_dim=7 (need one of (1, 4, 9, 16, 25): the widths "
                    "of the MLP head and the renderers)",
        "sh_deg_7": "rendering a NeRF-SG, not built on the MI355X path: sh_deg=7 (need -1: you can only use up to one of SH "
                    "or SG)",
        "sigma_activation": "rendering a NeRF-SG, not built on the MI355X path: activations other than relu/sigmoid/relu",
        "spherify": "rendering a NeRF-SG, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "trunk": "rendering a NeRF-SG, not built on the MI355X path: net_depth/net_width/skip_layer != 8/256/4",
    },
    ("sg", "extract"): {
        "all": "extraction of an SG PlenOctree, not built on the MI355X path: sh_deg=7 (need -1: you can only use up to one "
               "of SH or SG); net_depth/net_width/skip_layer != 8/256/4; min/max_deg_point != 0/10; "
               "num_rgb_channels/num_sigma_channels != 3/1; noise_std < 0; render_path / spherify (LLFF scenes); dataset=llff "
               "(LLFF scenes: an SG model on a forward-facing scene is not built); legacy_posenc_order; activations other "
               "than relu/sigmoid/relu",
        "channels": "extraction of an SG PlenOctree, not built on the MI355X path: num_rgb_channels/num_sigma_channels != 3/1",
        "legacy_posenc_order": "extraction of an SG PlenOctree, not built on the MI355X path: legacy_posenc_order",
        "llff": "extraction of an SG PlenOctree, not built on the MI355X path: dataset=llff (LLFF scenes: an SG model on a "
                "forward-facing scene is not built)",
        "llff_render_path": "extraction of an SG PlenOctree, not built on the MI355X path: render_path / spherify (LLFF "
                            "scenes); dataset=llff (LLFF scenes: an SG model on a forward-facing scene is not built)",
        "net_activation": "extraction of an SG PlenOctree, not built on the MI355X path: activations other than "
                          "relu/sigmoid/relu",
        "noise_std": "extraction of an SG PlenOctree, not built on the MI355X path: noise_std < 0",
        "posenc": "extraction of an SG PlenOctree, not built on the MI355X path: min/max_deg_point != 0/10",
        "render_path": "extraction of an SG PlenOctree, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "rgb_activation": "extraction of an SG PlenOctree, not built on the MI355X path: activations other than "
                          "relu/sigmoid/relu",
        "sg_dim_7": "extraction of an SG PlenOctree, not built on the MI355X path: sg_dim=7 (need one of (1, 4, 9, 16, 25): "
                    "the widths of the MLP head and the renderers)",
        "sh_deg_7": "extraction of an SG PlenOctree, not built on the MI355X path: sh_deg=7 (need -1: you can only use up to "
                    "one of SH or SG)",
        "sigma_activation": "extraction of an SG PlenOctree, not built on the MI355X path: activations other than "
                            "relu/sigmoid/relu",
        "spherify": "extraction of an SG PlenOctree, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "trunk": "extraction of an SG PlenOctree, not built on the MI355X path: net_depth/net_width/skip_layer != 8/256/4",
    },
    ("vd", "render"): {
        "all": "rendering a view-dependent NeRF, not built on the MI355X path: net_depth_condition=2 (need 1); "
               "net_width_condition=64 (need 128); deg_view=2 (need 4); legacy_posenc_order; net_depth/net_width/skip_layer "
               "!= 8/256/4; min/max_deg_point != 0/10; num_rgb_channels/num_sigma_channels != 3/1; mlp_precision=bf16x3 (the "
               "view-conditioned head is float32 only); render_path / spherify (LLFF scenes); dataset=llff (LLFF scenes: the "
               "view-conditioned head on a forward-facing scene is not built); activations other than relu; rgb_activation "
               "other than sigmoid; noise_std < 0",
        "channels": "rendering a view-dependent NeRF, not built on the MI355X path: num_rgb_channels/num_sigma_channels != 3/1",
        "deg_view": "rendering a view-dependent NeRF, not built on the MI355X path: deg_view=2 (need 4)",
        "legacy_posenc_order": "rendering a view-dependent NeRF, not built on the MI355X path: legacy_posenc_order",
        "llff": "rendering a view-dependent NeRF, not built on the MI355X path: dataset=llff (LLFF scenes: the "
                "view-conditioned head on a forward-facing scene is not built)",
        "llff_render_path": "rendering a view-dependent NeRF, not built on the MI355X path: render_path / spherify (LLFF "
                            "scenes); dataset=llff (LLFF scenes: the view-conditioned head on a forward-facing scene is not "
                            "built)",
        "mlp_precision": "rendering a view-dependent NeRF, not built on the MI355X path: mlp_precision=bf16x3 (the "
                         "view-conditioned head is float32 only)",
        "net_activation": "rendering a view-dependent NeRF, not built on the MI355X path: activations other than relu",
        "net_depth_condition": "rendering a view-dependent NeRF, not built on the MI355X path: net_depth_condition=2 (need 1)",
        "net_width_condition": "rendering a view-dependent NeRF, not built on the MI355X path: net_width_condition=64 (need "
                               "128)",
        "noise_std": "rendering a view-dependent NeRF, not built on the MI355X path: noise_std < 0",
        "posenc": "rendering a view-dependent NeRF, not built on the MI355X path: min/max_deg_point != 0/10",
        "render_path": "rendering a view-dependent NeRF, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "rgb_activation": "rendering a view-dependent NeRF, not built on the MI355X path: rgb_activation other than sigmoid",
        "sigma_activation": "rendering a view-dependent NeRF, not built on the MI355X path: activations other than relu",
        "spherify": "rendering a view-dependent NeRF, not built on the MI355X path: render_path / spherify (LLFF scenes)",
        "trunk": "rendering a view-dependent NeRF, not built on the MI355X path: net_depth/net_width/skip_layer != 8/256/4",
    },
    ("vd", "extract"): {
        "all": "SH projection of a view-dependent NeRF, not built on the MI355X path: net_depth_condition=2 (need 1); "
               "net_width_condition=64 (need 128); deg_view=2 (need 4); sh_deg=7 (the projection needs 0..4); "
               "legacy_posenc_order; net_depth/net_width/skip_layer != 8/256/4; min/max_deg_point != 0/10; "
               "num_rgb_channels/num_sigma_channels != 3/1; mlp_precision=bf16x3 (the view-conditioned head is float32 only); "
               "projection_samples=0 (need >= 1); render_path / spherify (LLFF scenes); dataset=llff (LLFF scenes: the "
               "view-conditioned head on a forward-facing scene is not built); activations other than relu",
        "channels": "SH projection of a view-dependent NeRF, not built on the MI355X path: "
                    "num_rgb_channels/num_sigma_channels != 3/1",
        "deg_view": "SH projection of a view-dependent NeRF, not built on the MI355X path: deg_view=2 (need 4)",
        "legacy_posenc_order": "SH projection of a view-dependent NeRF, not built on the MI355X path: legacy_posenc_order",
        "llff": "SH projection of a view-dependent NeRF, not built on the MI355X path: dataset=llff (LLFF scenes: the "
                "view-conditioned head on a forward-facing scene is not built)",
        "llff_render_path": "SH projection of a view-dependent NeRF, not built on the MI355X path: render_path / spherify "
                            "(LLFF scenes); dataset=llff (LLFF scenes: the view-conditioned head on a forward-facing scene is "
                            "not built)",
        "mlp_precision": "SH projection of a view-dependent NeRF, not built on the MI355X path: mlp_precision=bf16x3 (the "
                         "view-conditioned head is float32 only)",
        "net_activation": "SH projection of a view-dependent NeRF, not built on the MI355X path: activations other than relu",
        "net_depth_condition": "SH projection of a view-dependent NeRF, not built on the MI355X path: net_depth_condition=2 "
                               "(need 1)",
        "net_width_condition": "SH projection of a view-dependent NeRF, not built on the MI355X path: net_width_condition=64 "
                               "(need 128)",
        "posenc": "SH projection of a view-dependent NeRF, not built on the MI355X path: min/max_deg_point != 0/10",
        "projection_samples": "SH projection of a view-dependent NeRF, not built on the MI355X path: projection_samples=0 "
                              "(need >= 1)",
        "render_path": "SH projection of a view-dependent NeRF, not built on the MI355X path: render_path / spherify (LLFF "
                       "scenes)",
        "sh_deg_-1": "SH projection of a view-dependent NeRF, not built on the MI355X path: sh_deg=-1 (the projection needs "
                     "0..4)",
        "sh_deg_7": "SH projection of a view-dependent NeRF, not built on the MI355X path: sh_deg=7 (the projection needs "
                    "0..4)",
        "sigma_activation": "SH projection of a view-dependent NeRF, not built on the MI355X path: activations other than relu",
        "spherify": "SH projection of a view-dependent NeRF, not built on the MI355X path: render_path / spherify (LLFF "
                    "scenes)",
        "trunk": "SH projection of a view-dependent NeRF, not built on the MI355X path: net_depth/net_width/skip_layer != "
                 "8/256/4",
    },
}
REFUSED.update({("sh", p): REFUSED["sh", "train"] for p in PURPOSES})
REFUSED["sg", "mesh"] = REFUSED["sg", "render"]

VANILLA = "not built on the MI355X path: use_viewdirs=true (vanilla NeRF head)"
# flags that select another family, or a family that is not built for the purpose: (base, flags over it, purpose) -> the text
ROUTED = {
    # the view-conditioned head is not built for training and meshing: the check the flags would get without it answers
    ("vd", "none", "train"): VANILLA,
    ("vd", "none", "mesh"): VANILLA,
    ("vd", "all", "train"): "not built on the MI355X path: use_viewdirs=true (vanilla NeRF head); sh_deg=7 (need 0..4); "
                            "net_depth/net_width/skip_layer != 8/256/4; min/max_deg_point != 0/10; noise_std < 0; "
                            "legacy_posenc_order; activations other than relu/sigmoid/relu",
    ("vd", "all", "mesh"): "not built on the MI355X path: use_viewdirs=true (vanilla NeRF head); sh_deg=7 (need 0..4); "
                           "net_depth/net_width/skip_layer != 8/256/4; min/max_deg_point != 0/10; noise_std < 0; "
                           "legacy_posenc_order; activations other than relu/sigmoid/relu",
    # use_viewdirs together with sg_dim > 0, in the purposes of the five entry points (eval and gen_video both render)
    ("vd", "sg_preset", "train"): "training a NeRF-SG, not built on the MI355X path: use_viewdirs=true (an SG model has no "
                                  "view-conditioned head)",
    ("vd", "sg_preset", "render"): "rendering a view-dependent NeRF, not built on the MI355X path: sg_dim>0 (spherical gaussians)",
    ("vd", "sg_preset", "extract"): "SH projection of a view-dependent NeRF, not built on the MI355X path: sh_deg=-1 (the "
                                    "projection needs 0..4); sg_dim>0 (spherical gaussians)",
    ("vd", "sg_preset", "mesh"): "not built on the MI355X path: use_viewdirs=true (vanilla NeRF head); sh_deg=-1 (need 0..4); "
                                 "sg_dim>0 (spherical gaussians)",
    ("vd", "sg_dim_4", "train"): "training a NeRF-SG, not built on the MI355X path: sh_deg=4 (need -1: you can only use up to "
                                 "one of SH or SG); use_viewdirs=true (an SG model has no view-conditioned head)",
    ("vd", "sg_dim_4", "render"): "rendering a view-dependent NeRF, not built on the MI355X path: sg_dim>0 (spherical gaussians)",
    ("vd", "sg_dim_4", "extract"): "SH projection of a view-dependent NeRF, not built on the MI355X path: sg_dim>0 (spherical "
                                   "gaussians)",
    ("vd", "sg_dim_4", "mesh"): "not built on the MI355X path: use_viewdirs=true (vanilla NeRF head); sg_dim>0 (spherical "
                                "gaussians)",
    # an SH command line that gains --sg_dim is an SG one, with the SH degree it still carries
    ("sh", "sg_dim_25", "train"): "training a NeRF-SG, not built on the MI355X path: sh_deg=4 (need -1: you can only use up to "
                                  "one of SH or SG)",
    ("sh", "sg_dim_25", "render"): "rendering a NeRF-SG, not built on the MI355X path: sh_deg=4 (need -1: you can only use up to "
                                   "one of SH or SG)",
    ("sh", "sg_dim_25", "extract"): "extraction of an SG PlenOctree, not built on the MI355X path: sh_deg=4 (need -1: you can "
                                    "only use up to one of SH or SG)",
    ("sh", "sg_dim_25", "mesh"): "rendering a NeRF-SG, not built on the MI355X path: sh_deg=4 (need -1: you can only use up to "
                                 "one of SH or SG)",
    # and an SG one that loses it is an SH one, with sh_deg -1
    ("sg", "sg_dim_-1", "train"): "not built on the MI355X path: sh_deg=-1 (need 0..4)",
    ("sg", "sg_dim_-1", "render"): "not built on the MI355X path: sh_deg=-1 (need 0..4)",
    ("sg", "sg_dim_-1", "extract"): "not built on the MI355X path: sh_deg=-1 (need 0..4)",
    ("sg", "sg_dim_-1", "mesh"): "not built on the MI355X path: sh_deg=-1 (need 0..4)",
}
ROUTED_FLAGS = {"none": {}, "all": MUTATIONS["all"], "sg_preset": dict(sg_dim=25, sh_deg=-1), "sg_dim_4": dict(sg_dim=4),
                "sg_dim_25": dict(sg_dim=25), "sg_dim_-1": dict(sg_dim=-1)}

# a family's own check on flags that select another family (what sg.get_model_state / viewdirs.get_model_state still run)
OWN = {
    ("sg", "train", "sg_dim_-1"): "training a NeRF-SG, not built on the MI355X path: sg_dim=-1 (an SH model: the plain path)",
    ("sg", "render", "sg_dim_-1"): "rendering a NeRF-SG, not built on the MI355X path: sg_dim=-1 (an SH model: the plain path)",
    ("sg", "extract", "sg_dim_-1"): "extraction of an SG PlenOctree, not built on the MI355X path: sg_dim=-1 (an SH model: the "
                                    "plain path)",
    ("sg", "mesh", "sg_dim_-1"): "rendering a NeRF-SG, not built on the MI355X path: sg_dim=-1 (an SH model: the plain path)",
    ("sg", "train", "use_viewdirs"): "training a NeRF-SG, not built on the MI355X path: use_viewdirs=true (an SG model has no "
                                     "view-conditioned head)",
    ("sg", "render", "use_viewdirs"): "rendering a NeRF-SG, not built on the MI355X path: use_viewdirs=true (an SG model has no "
                                      "view-conditioned head)",
    ("sg", "extract", "use_viewdirs"): "extraction of an SG PlenOctree, not built on the MI355X path: use_viewdirs=true (an SG "
                                       "model has no view-conditioned head)",
    ("vd", "render", "no_viewdirs"): "rendering a view-dependent NeRF, not built on the MI355X path: use_viewdirs=false (an SH "
                                     "model: the plain path)",
    ("vd", "extract", "no_viewdirs"): "SH projection of a view-dependent NeRF, not built on the MI355X path: use_viewdirs=false "
                                      "(an SH model: the plain path)",
    ("sh", "train", "sg_dim_25"): "not built on the MI355X path: sg_dim>0 (spherical gaussians)",
    ("sh", "train", "use_viewdirs"): VANILLA,
}
OWN_FLAGS = {"sg_dim_-1": dict(sg_dim=-1), "use_viewdirs": dict(use_viewdirs=True), "no_viewdirs": dict(use_viewdirs=False),
             "sg_dim_25": dict(sg_dim=25)}


DEFAULTS = vars(extraction.define_flags().parse_args(["--train_dir", "x", "--data_dir", "d"]))     # the superset of the five parsers


def _args(base, **over):
    return argparse.Namespace(**{**DEFAULTS, **BASES[base], **over})


def _outcome(fn, *a, **k):
    try:
        fn(*a, **k)
    except Exception as e:                  # noqa: BLE001 -- the type is part of what is compared
        return type(e).__name__, str(e)
    return None


# ---- selection -------------------------------------------------------------------------------------------------------
def test_select_takes_use_viewdirs_first_then_sg_dim():
    assert families.FAMILIES == (families.VIEWDIRS, families.SG, families.SH)
    for base, fam in FAMILY.items():
        assert families.select(_args(base)) is fam
        for name, flags in MUTATIONS.items():
            if name != "sg_dim_7" or base == "sg":
                assert families.select(_args(base, **flags)) is fam, (base, name)
    assert families.select(_args("vd", sg_dim=25, sh_deg=-1)) is families.VIEWDIRS
    assert families.select(_args("vd", sg_dim=4)) is families.VIEWDIRS
    assert families.select(_args("sh", sg_dim=25)) is families.SG and families.select(_args("sh", sg_dim=7)) is families.SG
    assert families.select(_args("sg", sg_dim=-1)) is families.SH and families.select(_args("sg", sg_dim=0)) is families.SH
    assert families.select(_args("sg", use_viewdirs=True)) is families.VIEWDIRS
    assert families.select(_args("sh", use_viewdirs=True)) is families.VIEWDIRS


def test_every_built_purpose_has_a_checkpoint_policy_and_every_other_an_answer():
    for fam in families.FAMILIES:
        assert set(fam.checks) | set(fam.instead) == set(PURPOSES) and not set(fam.checks) & set(fam.instead), fam.name
        assert set(fam.checkpoint) == set(fam.checks), fam.name
        assert all(isinstance(p, families.Policy) and p.absent in ("fresh", "raises") for p in fam.checkpoint.values())
        for names in fam.instead.values():
            assert names[-1] == "sh" and all(p in families.SH.checks for p in fam.instead)
    assert set(families.VIEWDIRS.checks) == {"render", "extract"}
    assert (families.SH.n_params(_args("sh"), types.SimpleNamespace(n_mlp=10)),
            families.SG.n_params(_args("sg"), types.SimpleNamespace(n_mlp=10)), families.VIEWDIRS.n_params) == (20, 95, None)
    lobes = object()
    assert families.SH.tree(_args("sh"), None) == families.VIEWDIRS.tree(_args("vd"), None) == ("SH25", 25, None)
    assert families.SG.tree(_args("sg"), types.SimpleNamespace(lobes=lobes)) == ("SG25", 25, lobes)
    assert families.SH.projection is families.SG.projection is None and callable(families.VIEWDIRS.projection)


# ---- the flag checks, word for word ------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,purpose", sorted(REFUSED))
def test_each_offending_flag_alone_and_all_at_once(base, purpose):
    table = REFUSED[base, purpose]
    assert set(table) <= set(MUTATIONS)
    assert _outcome(families.check, _args(base), purpose) is None
    assert _outcome(families.check_flags, FAMILY[base], _args(base), purpose) is None
    for name, flags in MUTATIONS.items():
        if name == "sg_dim_7" and base != "sg":
            continue
        want = ("NotImplementedError", table[name]) if name in table else None
        assert _outcome(families.check, _args(base, **flags), purpose) == want, name
        assert _outcome(families.check_flags, FAMILY[base], _args(base, **flags), purpose) == want, name
    if base == "sh":        # the names that stay are the same check
        for name, flags in MUTATIONS.items():
            want = ("NotImplementedError", table[name]) if name in table else None
            if name != "sg_dim_7":
                assert _outcome(utils.check_supported, _args(base, **flags)) == want, name
                assert _outcome(utils.check_flags, _args(base, **flags)) == want, name


@pytest.mark.parametrize("base,flags,purpose", sorted(ROUTED))
def test_flags_that_select_another_family_or_an_unbuilt_purpose(base, flags, purpose):
    for require_data in (True, False):                   # gen_video renders without a data_dir: the same words
        got = _outcome(families.check, _args(base, **ROUTED_FLAGS[flags]), purpose, require_data=require_data)
        assert got == ("NotImplementedError", ROUTED[base, flags, purpose])


@pytest.mark.parametrize("base,purpose,flags", sorted(OWN))
def test_a_familys_own_check_on_flags_of_another(base, purpose, flags):
    got = _outcome(families.check_flags, FAMILY[base], _args(base, **OWN_FLAGS[flags]), purpose)
    assert got == ("NotImplementedError", OWN[base, purpose, flags])


# ---- directories and batch size ------------------------------------------------------------------------------------------
TRAIN_DIR = ("ValueError", "train_dir must be set. None set now.")
DATA_DIR = ("ValueError", "data_dir must be set. None set now.")
BATCH = ("ValueError", "Batch size must be divisible by the number of devices.")


@pytest.mark.parametrize("base", sorted(BASES))
@pytest.mark.parametrize("purpose", PURPOSES)
def test_directory_and_batch_size_errors_come_first(base, purpose):
    built = purpose in FAMILY[base].checks
    after = None if built else ("NotImplementedError", VANILLA)          # what a command line with its directories set gets
    assert _outcome(families.check, _args(base, train_dir=None), purpose) == TRAIN_DIR
    assert _outcome(families.check, _args(base, data_dir=None), purpose) == DATA_DIR
    assert _outcome(families.check, _args(base, data_dir=None), purpose, require_data=False) == after
    assert _outcome(families.check, _args(base, data_dir=None, dataset="synthetic"), purpose) == after
    assert _outcome(families.check, _args(base, batch_size=1023), purpose, world_size=2) == (BATCH if purpose == "train" else after)
    assert _outcome(families.check, _args(base, batch_size=1024), purpose, world_size=2) == after
    # before any flag clause, in this order
    wrong = dict(MUTATIONS["all"], batch_size=1023)
    assert _outcome(families.check, _args(base, train_dir=None, data_dir=None, **wrong), purpose, world_size=2) == TRAIN_DIR
    assert _outcome(families.check, _args(base, data_dir=None, **wrong), purpose, world_size=2) == DATA_DIR
    if purpose == "train":
        assert _outcome(families.check, _args(base, **wrong), purpose, world_size=2) == BATCH
    assert _outcome(utils.check_dirs, _args(base, train_dir=None)) == TRAIN_DIR
    assert _outcome(utils.check_flags, _args(base, train_dir=None)) == TRAIN_DIR


# ---- one train step, the same calls ----------------------------------------------------------------------------------------
SH_CALLS = ["train_workspace_bytes", "train_fwd_bwd", "adam_pack_step"]
SG_CALLS = ["sg_train_workspace_bytes", "sg_train_fwd_bwd", "adam_pack_step", "adam_step", "sg_lobes"]
FWD_KW = {"randomized": "True", "seed": "77", "sp_points": "sp_points", "t_rand": "t_rand", "u": "u"}
SH_LOG = [
    ("train_workspace_bytes", ["cfg", "8"], {}),
    ("train_fwd_bwd", ["cfg", "params", "packed", "origins", "directions", "viewdirs", "pixels", "grads", "stats", "_ws"], FWD_KW),
    ("adam_pack_step", ["cfg", "params", "m", "v", "grads", "0.0005", "5", "packed"], {"grad_scale": "SCALE"}),
]
SG_LOG = [
    ("sg_train_workspace_bytes", ["cfg", "8"], {}),
    ("sg_train_fwd_bwd", ["cfg", "params", "sg_params", "packed", "origins", "directions", "viewdirs", "pixels", "grads", "sg_grads",
                          "stats", "_ws"], FWD_KW),
    ("adam_pack_step", ["cfg", "params", "m", "v", "grads", "0.0005", "5", "packed"], {"grad_scale": "SCALE"}),
    ("adam_step", ["sg_params", "sg_m", "sg_v", "sg_grads", "0.0005", "5"], {"grad_scale": "SCALE"}),
    ("sg_lobes", ["sg_params", "4", "lobes"], {}),
]
STATE_TENSORS = ("params", "m", "v", "grads", "stats", "bucket0", "bucket1", "sg_params", "sg_m", "sg_v", "sg_grads", "lobes", "_ws")


def _logged_step(monkeypatch, kind, world_size, with_reducer):
    """models.train_step on a TrainState / SgState with every `ops` entry it may reach replaced by a recorder: the calls in order,
    each argument named after the state or batch field it is (by storage and shape), scalars by their repr."""
    monkeypatch.setattr(models.TrainState, "repack", lambda self, need_bwd=True: None)      # no GPU: no weight images
    cfg = _lib.make_cfg(sh_deg=1, num_coarse_samples=8, num_fine_samples=8, sparsity_npoints=64)
    params = torch.zeros(64)
    state = sg.SgState(cfg, params, *sg.init_lobe_params(4)) if kind == "sg" else models.TrainState(cfg, params)
    state.step = 5
    rays = utils.Rays(torch.zeros(8, 3), torch.ones(8, 3), torch.full((8, 3), 2.0))
    batch = {"rays": rays, "pixels": torch.zeros(8, 3)}
    extra = {"t_rand": torch.zeros(8, 8), "u": torch.zeros(8, 8), "sp_points": torch.zeros(64, 3)}

    def name(x):
        if not torch.is_tensor(x):
            return "cfg" if x is cfg else "packed" if x is state.packed else repr(x)
        for owner, attrs in ((state, STATE_TENSORS), (rays, rays._fields)):
            for a in attrs:
                t = getattr(owner, a, None)
                if t is not None and t.data_ptr() == x.data_ptr() and t.shape == x.shape:
                    return a
        return next(k for k, t in {**extra, "pixels": batch["pixels"]}.items() if t is x)

    log = []

    def recorder(n, ret=None):
        def f(*a, **k):
            log.append((n, [name(x) for x in a], {kk: name(v) for kk, v in sorted(k.items())}))
            return ret
        return f
    for n in set(SH_CALLS + SG_CALLS):
        monkeypatch.setattr(ops, n, recorder(n, 4096 if n.endswith("workspace_bytes") else None))
    reducer = types.SimpleNamespace(ready_event=lambda: "ev", reduce=recorder("reducer.reduce")) if with_reducer else None
    out = models.train_step(types.SimpleNamespace(cfg=cfg), state, batch, 5e-4, randomized=True, seed=77, world_size=world_size,
                            reducer=reducer, **extra)
    assert out is state.stats and state.step == 6
    return log, state


@pytest.mark.parametrize("kind", ["sh", "sg"])
@pytest.mark.parametrize("world_size,with_reducer", [(1, False), (2, True)])
def test_one_train_step_makes_the_calls_of_the_two_it_replaced(monkeypatch, kind, world_size, with_reducer):
    log, state = _logged_step(monkeypatch, kind, world_size, with_reducer)
    want = [(n, list(a), dict(k)) for n, a, k in (SG_LOG if kind == "sg" else SH_LOG)]
    for n, a, k in want:
        if "grad_scale" in k:
            k["grad_scale"] = repr(1.0 / world_size)
    want[1][2]["grads0_ready"] = "'ev'" if with_reducer else "None"
    if with_reducer:                                     # the exchange sits between the backward pass and the first update
        want.insert(2, ("reducer.reduce", ["bucket0", "bucket1"], {}))
    assert [c[0] for c in log] == [c[0] for c in want]
    assert [c[0] for c in log if c[0] != "reducer.reduce"] == (SG_CALLS if kind == "sg" else SH_CALLS)
    assert log == want
    assert getattr(state, "_sg_stale", None) is (True if kind == "sg" else None)
    assert not hasattr(sg, "train_step")
