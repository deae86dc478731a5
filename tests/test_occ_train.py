"""Training through the occupancy grid on the CPU: the --cull_* flags, what the families table accepts and refuses for them, the
rebuild schedule of occupancy.TrainingGrid with a stand-in builder, and that train_step without a grid makes the call it always
made -- nothing here touches a GPU."""
import types

import pytest

from plenoctree_amd import ops
from plenoctree_amd.nerf_sh.nerf import families, models, occupancy, utils


def _args(*argv):
    return utils.define_flags().parse_args(["--train_dir", "x", "--dataset", "synthetic", "--use_viewdirs", "false", "--sh_deg", "2", *argv])


# ---- flags ------------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_and_parsing():
    a = _args()
    assert (a.cull_reso, a.cull_center, a.cull_radius, a.cull_alpha_thresh, a.cull_dilate, a.cull_warmup_steps,
            a.cull_update_every) == (0, [0.0, 0.0, 0.0], [1.5, 1.5, 1.5], 0.01, 1, 500, 32)
    assert not occupancy.cull_wanted(a) and occupancy.cull_clauses(a) == [] and occupancy.TrainingGrid.from_args(a) is None
    a = _args("--cull_reso", "128", "--cull_center", "0.5 0 -1", "--cull_radius", "2", "--cull_dilate", "0", "--cull_warmup_steps", "4",
              "--cull_update_every", "8", "--cull_alpha_thresh", "0.05")
    assert a.cull_center == [0.5, 0.0, -1.0] and a.cull_radius == [2.0, 2.0, 2.0]
    assert occupancy.cull_wanted(a) and occupancy.cull_clauses(a) == []
    g = occupancy.TrainingGrid.from_args(a)
    assert (g.reso, g.warmup_steps, g.update_every) == (128, 4, 8)
    help_text = utils.define_flags().format_help()
    assert "resumed from a checkpoint whose step is a multiple of" in " ".join(help_text.split())


# ---- the families table -----------------------------------------------------------------------------------------------------------
def test_accepted_for_sh_training_and_off_by_default():
    families.check(_args("--cull_reso", "64"), "train")
    families.check(_args("--cull_reso", "64", "--noise_std", "1.0", "--randomized", "false"), "train")
    families.check(_args("--cull_reso", "64", "--dataset", "llff", "--data_dir", "d", "--spherify", "true"), "train")
    for purpose in families.PURPOSES:
        families.check(_args(), purpose)


@pytest.mark.parametrize("argv, words", [
    (["--sg_dim", "9", "--sh_deg", "-1"], "cull_reso with sg_dim>0"),
    (["--use_viewdirs", "true"], "cull_reso with use_viewdirs=true"),
    (["--dataset", "llff", "--data_dir", "d"], "cull_reso on a forward-facing scene without --spherify (NDC"),
    (["--noise_std", "1.0", "--randomized", "true"], "cull_reso with noise_std and randomized sampling"),
    (["--cull_reso", "2048"], "cull_reso=2048 (need 1..1024"),
    (["--cull_alpha_thresh", "1.0"], "cull_alpha_thresh=1"),
    (["--cull_update_every", "0"], "cull_update_every=0"),
    (["--cull_warmup_steps", "-1"], "cull_warmup_steps=-1"),
])
def test_train_refusals_by_name(argv, words):
    a = _args("--cull_reso", "32", *argv)
    with pytest.raises(NotImplementedError) as e:
        families.check(a, "train")
    assert words in str(e.value), str(e.value)
    a.cull_reso = 0                                               # the same flags without the grid are not refused for it
    try:
        families.check(a, "train")
    except NotImplementedError as e2:
        assert "cull_" not in str(e2)


@pytest.mark.parametrize("purpose", ["render", "extract", "mesh"])
@pytest.mark.parametrize("family", [[], ["--sg_dim", "9", "--sh_deg", "-1"]])
def test_every_other_purpose_refuses_the_training_grid(purpose, family):
    with pytest.raises(NotImplementedError, match="cull_reso \\(the grid that follows a model is nerf_sh.train's"):
        families.check(_args("--cull_reso", "32", *family), purpose)


def test_viewdirs_family_refuses_the_training_grid():
    for purpose in ("render", "extract"):
        with pytest.raises(NotImplementedError, match="cull_reso"):
            families.check(_args("--cull_reso", "32", "--use_viewdirs", "true"), purpose)


def test_the_renderers_flag_in_training_points_to_cull_reso():
    with pytest.raises(NotImplementedError) as e:
        families.check(_args("--occupancy_reso", "32"), "train")
    assert "culling inside training" in str(e.value) and "--cull_reso" in str(e.value)


# ---- the schedule -----------------------------------------------------------------------------------------------------------------
class _Grid:
    def __init__(self, frac, tag):
        self.frac, self.tag = frac, tag

    def fraction_occupied(self):
        return self.frac


def _training_grid(fracs=None, **kw):
    """A TrainingGrid whose builder counts its calls; fracs: occupied fraction of the i-th build (default 0.25)."""
    said, built = [], []

    def build(model, state):
        built.append((model, state))
        return _Grid((fracs or {}).get(len(built), 0.25), len(built))
    g = occupancy.TrainingGrid(16, build=build, say=lambda *a, **k: said.append(a[0]), **kw)
    return g, built, said


def _run(g, first, last):
    """before_step over the steps first..last; the tag of the grid each step got (None = dense)."""
    out = {}
    for step in range(first, last + 1):
        grid = g.before_step(step, "model", f"state{step}")
        out[step] = None if grid is None else grid.tag
    return out


def test_schedule_warmup_then_every_n_steps():
    g, built, _ = _training_grid(warmup_steps=4, update_every=4)
    got = _run(g, 1, 12)
    assert got == {1: None, 2: None, 3: None, 4: None, 5: 1, 6: 1, 7: 1, 8: 1, 9: 2, 10: 2, 11: 2, 12: 2}
    assert g.rebuilds == [5, 9] and [s for _, s in built] == ["state5", "state9"]       # built from the state the step starts from
    assert g.before_step(12, "model", "again") .tag == 2 and len(built) == 2             # asking twice does not rebuild


def test_schedule_with_a_warmup_off_the_grid_of_updates_and_none():
    g, _, _ = _training_grid(warmup_steps=5, update_every=4)
    _run(g, 1, 14)
    assert g.rebuilds == [6, 9, 13]                               # the first culled step has no grid; then (s - 1) % 4 == 0
    g, _, _ = _training_grid(warmup_steps=0, update_every=3)
    _run(g, 1, 8)
    assert g.rebuilds == [1, 4, 7]


def test_schedule_is_a_function_of_the_step_a_resume_rebuilds_where_the_run_would():
    whole, _, _ = _training_grid(warmup_steps=4, update_every=4)
    _run(whole, 1, 12)
    resumed, built, _ = _training_grid(warmup_steps=4, update_every=4)          # a fresh process at the checkpoint of step 8
    got = _run(resumed, 9, 12)
    assert resumed.rebuilds == [9] and [s for s in whole.rebuilds if s > 8] == [9] and set(got.values()) == {1}
    # a checkpoint off the schedule: the resumed run has no grid and builds one at once (from later parameters than the whole run's)
    off, _, _ = _training_grid(warmup_steps=4, update_every=4)
    _run(off, 11, 14)
    assert off.rebuilds == [11, 13]
    # a resume inside the warm-up stays dense
    early, built, _ = _training_grid(warmup_steps=4, update_every=4)
    assert _run(early, 3, 4) == {3: None, 4: None} and built == []


def test_an_empty_rebuild_runs_dense_and_says_so_once():
    g, built, said = _training_grid(fracs={1: 0.0, 2: 0.0, 3: 0.5}, warmup_steps=2, update_every=2)
    got = _run(g, 1, 8)
    assert got == {1: None, 2: None, 3: None, 4: None, 5: None, 6: None, 7: 3, 8: 3}
    assert g.rebuilds == [3, 5, 7] and len(built) == 3            # an empty grid is not rebuilt every step
    assert len(said) == 1 and "no occupied cell" in said[0] and "dense" in said[0]


def test_live_fractions_line():
    g, _, _ = _training_grid(warmup_steps=1, update_every=4)
    cfg = ops.make_cfg(num_coarse_samples=8, num_fine_samples=16)
    assert "dense until step 2" in g.line()
    g.before_step(2, None, None)
    g.count(cfg, [40, 60], 10)                                    # 10 rays: 80 coarse rows, 240 fine rows
    g.count(cfg, [0, 60], 10)
    line = g.line()
    assert "live rows: coarse 25.00 %, fine 25.00 %" in line and "rebuilt before step 2 in" in line and "25.00 % occupied" in line
    assert "dense" in g.line()                                    # the counts start again after every line


def test_bad_schedule_arguments():
    with pytest.raises(ValueError, match="update_every"):
        occupancy.TrainingGrid(16, update_every=0)
    with pytest.raises(ValueError, match="reso"):
        occupancy.TrainingGrid(0)


# ---- train_step ---------------------------------------------------------------------------------------------------------------------
class _State:
    """Records the library calls train_step makes."""

    def __init__(self):
        self.calls, self.step, self.stats = [], 0, "stats"

    def workspace(self, n):
        self.calls.append(("workspace", n))
        return "ws"

    def train_workspace_bytes(self, cfg, B):
        return 100

    def train_culled_workspace_bytes(self, cfg, B):
        return 200

    def fwd_bwd(self, cfg, rays, pixels, ws, **kw):
        self.calls.append(("fwd_bwd", ws, kw))

    def update(self, cfg, lr, scale):
        self.calls.append(("update", lr, scale))


def _batch():
    rays = types.SimpleNamespace(origins=types.SimpleNamespace(shape=(5, 3)))
    return {"rays": rays, "pixels": "px"}


def test_train_step_without_occupancy_makes_todays_call():
    model = types.SimpleNamespace(cfg="cfg")
    for kw in ({}, {"occupancy": None, "live_rows": []}):
        state = _State()
        models.train_step(model, state, _batch(), 1e-3, randomized=True, seed=7, **kw)
        assert state.calls == [("workspace", 100),
                               ("fwd_bwd", "ws", dict(randomized=True, t_rand=None, u=None, sp_points=None, seed=7, grads0_ready=None)),
                               ("update", 1e-3, 1.0)]                  # no occupancy keyword reaches a state that does not know it
        assert state.step == 1


def test_train_step_with_occupancy_takes_the_culled_workspace_and_passes_the_grid():
    model, state, rows = types.SimpleNamespace(cfg="cfg"), _State(), []
    models.train_step(model, state, _batch(), 1e-3, randomized=False, seed=7, occupancy="grid", live_rows=rows)
    assert state.calls[0] == ("workspace", 200)
    assert state.calls[1] == ("fwd_bwd", "ws", dict(randomized=False, t_rand=None, u=None, sp_points=None, seed=7, grads0_ready=None,
                                                    occupancy="grid", live_rows=rows))


def test_fwd_bwd_of_the_sh_state_routes_by_the_argument(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, "train_fwd_bwd", lambda *a, **k: calls.append(("dense", k)))
    monkeypatch.setattr(ops, "train_fwd_bwd_culled", lambda *a, **k: calls.append(("culled", a[1], k)))
    state = types.SimpleNamespace(params="p", packed="pk", grads="g", stats="s")
    rays = types.SimpleNamespace(origins="o", directions="d", viewdirs="v")
    models.TrainState.fwd_bwd(state, "cfg", rays, "px", "ws", seed=3)
    models.TrainState.fwd_bwd(state, "cfg", rays, "px", "ws", seed=3, occupancy="grid", live_rows=[])
    assert calls == [("dense", {"seed": 3}), ("culled", "grid", {"seed": 3, "live_rows": []})]


def test_the_model_constructor_judges_the_flag_by_the_entry_points_purpose():
    """models.construct_nerf runs the SH family's check itself (utils.check_supported): for nerf_sh.train it is the `train` check."""
    a = _args("--cull_reso", "64")
    utils.check_supported(a, "train")
    with pytest.raises(NotImplementedError, match="cull_reso"):
        utils.check_supported(a)                                  # the default purpose is a renderer's
    utils.check_supported(_args())
