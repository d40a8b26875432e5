"""Episodes of an ensemble of actors, the parts that need no device: the reference module on hand-made dense actor tables with one step of
each rule worked out by hand, the new unit in the build lists, the declarations and the binding, the views of an ActorEnsembleTrajectory,
and the refusals of `grlxd -A`, which come before any device is looked for.

One step by hand, lo = -15, hi = 15 (the cart-pole's force), members in ascending order:

  MEAN         a = [3, -6, 7.5]:  m = 3; m = 3 + -6 = -3; m = -3 + 7.5 = 4.5; action = 4.5 / 3 = 1.5
  BINNING      B = 6 (bins of width 5), a = [-14, -13, 1, 2, 12]: bins [0, 0, 3, 3, 5], hist = [2, 0, 0, 2, 0, 1]; the ascending scan stops at
               binmax = 0 (count 2; bin 3's equal count is not strictly greater).  Members with hist[bin] == 2: ALL of -14, -13, 1, 2 -- the
               equal-count second bin joins the sum --: s = -14 - 13 + 1 + 2 = -24, n = 4, action = -6; two bins hold the count: a tie
  DATA_CENTER  K = 2, a = [1, 2, 9]: mean = (1 + 2 + 9) / 3 = 4; d = [9, 4, 25]: member 2 (not the first alive) is removed; mean = (1 + 2) / 2
               = 1.5; two are alive: action = 1.5, no tie.  K = 1 goes on: d = [0.25, 0.25]: two members at the greatest d, the FIRST is
               removed and the step ties; action = 2
  DENSITY      r = 0.1, a = [-15, 0, 0.75, 15]: n = [-1, 0, 0.05, 1]; between members 1 and 2 the kernel is pexp(-(0.05 * 0.05) / 0.01) =
               pexp(-0.25), every other pair is pexp(-100) and below: rho_1 = rho_2 = 1 + pexp(-0.25) + ... are the greatest, in bits equal or
               not; the first of strictly greatest rho is selected.  At r = 1e-6 every off-diagonal term is pexp(< -745.2) = 0.0: every rho is
               exactly 1.0, all four tie and member 0 acts"""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_actor_ensemble_ref as ae
from tests import policy_evaluate_ref as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LO, HI = -15.0, 15.0


class Dense:
    """a hand-made dense actor table: every slot holds the same weight, so the actor's read is that weight at every observation"""
    def __init__(self, w):
        self.w = float(w)

    def __getitem__(self, slot):
        return self.w


# ---- the rules, one step each by hand ------------------------------------------------------------------------------------------------
def test_the_rules_by_hand():
    assert ae.combine([3.0, -6.0, 7.5], ae.MEAN, 10, 0.001, LO, HI) == (1.5, -1, 1, 3, False)
    seen = {}
    assert ae.combine([-14.0, -13.0, 1.0, 2.0, 12.0], ae.BINNING, 6, 0.001, LO, HI, seen) == (-6.0, 0, 2, 4, True)
    assert seen["occupied"] == 3
    assert [ae.bin_of(a, 6, LO, HI) for a in (-15.0, -10.0, 14.999, 15.0)] == [0, 1, 5, 5], "the upper bound falls into the last bin"
    assert ae.combine([-14.0, 1.0, 2.0], ae.BINNING, 6, 0.001, LO, HI) == (1.5, 3, 1, 2, False)
    seen = {}
    assert ae.combine([1.0, 2.0, 9.0], ae.DATA_CENTER, 2, 0.001, LO, HI, seen) == (1.5, -1, 1, 2, False)
    assert seen == {"removals": 1, "not_first": 1}
    assert ae.data_center([1.0, 2.0, 9.0], 1) == (2.0, 2, 1, [(2, 0), (0, 0)])
    assert ae.combine([1.0, 2.0, 9.0], ae.DATA_CENTER, 1, 0.001, LO, HI) == (2.0, -1, 2, 1, True)
    assert ae.combine([1.0, 2.0, 9.0], ae.DATA_CENTER, 5, 0.001, LO, HI) == (ae.mean([1.0, 2.0, 9.0]), -1, 1, 3, False), "K >= G: nobody is removed"
    a = [-15.0, 0.0, 0.75, 15.0]
    action, at, n, rho = ae.density(a, 0.1, LO, HI)
    near = ae.pexp(-0.25)
    assert 0.778 < near < 0.779 and rho[0] == 1.0 + ae.pexp(-100.0) + ae.pexp((-1 * (1.05 * 1.05)) / (0.1 * 0.1)) + ae.pexp(-400.0)
    assert at in (1, 2) and action == a[at] and rho[at] == max(rho) and abs(rho[1] - (1 + near)) < 1e-12
    assert ae.combine(a, ae.DENSITY, 10, 1e-6, LO, HI) == (-15.0, 0, 4, 1, True)
    assert ae.density(a, 1e-6, LO, HI)[3] == [1.0] * 4
    assert ae.combine([2.0, 5.0, 5.0], ae.DENSITY, 10, 1e-6, LO, HI) == (5.0, 1, 2, 1, True), "two members that agree to the last bit have rho 2"
    assert ae.spread_of([3.0, -6.0, 7.5]) == 13.5
    for rule in (ae.MEAN, ae.BINNING, ae.DATA_CENTER, ae.DENSITY):
        assert ae.combine([4.25], rule, 3, 0.05, LO, HI)[0] == 4.25, "a group of one hands its member's action on"


def test_an_episode_on_hand_made_tables(grlx):
    """three members whose actors read 3, -6 and 40 (clipped to 15) everywhere: every step combines [3, -6, 15], and the episode is the
    single-policy reference's on the combined action"""
    from tests import configs
    _, spec = configs.cart_pole_ac(grlx, 3, end_stop_penalty=1)
    spec.math = ob.MATH_PORTABLE
    members = [[None, Dense(w)] for w in (3.0, -6.0, 40.0)]
    state = [0.0, np.pi, 0.0, 0.0, 0.0]
    obs, _ = ev.observe(spec, state)
    assert ae.member_actions(members, spec, obs) == [3.0, -6.0, 15.0]
    for rule, bins, r, action, index, n_max, kept in (("mean", 10, 0.001, 4.0, -1, 1, 3), ("binning", 6, 0.001, 4.0, 1, 3, 3),
                                                      ("data_center", 2, 0.001, -1.5, -1, 1, 2), ("density", 10, 0.05, 3.0, 0, 3, 1)):
        got = ae.episode(members, spec, state, rule, bins, r, max_steps=5)
        want = ev.episode([None, Dense(action)], spec, state, 5)
        assert (got["ret"], got["disc"], got["steps"], got["terminal"]) == want[:4] and (got["final_state"] == want[5]).all(), rule
        assert got["records"].shape == (5, 17) and (got["records"][:, 0] == action).all() and (got["records"][:, 2] == 4.0).all(), rule
        assert (got["records"][:, 3] == index).all() and (got["records"][:, 4] == n_max).all(), rule
        assert got["kept"] == 5 * kept and got["spread"] == 5 * 21.0 and got["ties"] == (5 if n_max > 1 else 0), rule
        assert (got["records"][:, -2] == kept).all() and (got["records"][:, -1] == 21.0).all(), rule
    both = ae.evaluate(members, spec, [state, state], "mean", max_steps=7)
    assert both["records"].shape == (2, 7, 17) and both["kept"].dtype == np.int64 and both["steps"].dtype == np.int32


# ---- the build lists, the declarations and the binding -------------------------------------------------------------------------------
def test_the_unit_is_in_the_build_lists():
    from grl_amd import _build
    assert "grlx_evaluate_actor_ensemble.hip" in _build.SOURCES
    deps = _build.UNIT_DEPS["grlx_evaluate_actor_ensemble.hip"]
    src = open(os.path.join(_build.CSRC, "grlx_evaluate_actor_ensemble.hip")).read()
    for line in src.splitlines():
        if line.startswith('#include "'):
            assert line.split('"')[1] in deps, line
    assert "grlx_evaluate_actor_ensemble.h" in _build.UNIT_DEPS["grlx_api_read.cpp"] and "grlx_evaluate_actor_ensemble.h" in _build.API_DEPS
    for f in deps:
        assert os.path.exists(os.path.join(_build.CSRC, f)), f
    # the siblings and the rollout kernels are not touched by the feature: none of them includes the new unit's header or names its blocks
    for name in ("grlx_evaluate.hip", "grlx_evaluate_sampled.hip", "grlx_evaluate_noisy.hip", "grlx_kernels.hip", "grlx_episode.h", "grlx_evaluate.h",
                 "grlx_internal.h"):
        assert "actor_ensemble" not in open(os.path.join(_build.CSRC, name)).read().lower().replace(" ", "_"), name


def test_the_binding_names_what_the_header_declares():
    import grl_amd
    from grl_amd import capi
    header = open(os.path.join(ROOT, "include", "grlx.h")).read()
    for name in ("grlx_evaluate_actor_ensemble", "grlx_actor_ensemble_trajectory_record_words", "grlx_evaluate_actor_ensemble_trajectory"):
        assert name + "(" in header and name in capi._SIGS and name in capi._NEWER_SIGS
    assert "#define GRLX_ACTOR_ENSEMBLE_MAX 256" in header and capi.ACTOR_ENSEMBLE_MAX == 256
    assert "GRLX_ACTOR_ENSEMBLE_MEAN = 0, GRLX_ACTOR_ENSEMBLE_BINNING = 1, GRLX_ACTOR_ENSEMBLE_DATA_CENTER = 2, GRLX_ACTOR_ENSEMBLE_DENSITY = 3" in header
    assert (capi.ACTOR_ENSEMBLE_MEAN, capi.ACTOR_ENSEMBLE_BINNING, capi.ACTOR_ENSEMBLE_DATA_CENTER, capi.ACTOR_ENSEMBLE_DENSITY) == \
        (ae.MEAN, ae.BINNING, ae.DATA_CENTER, ae.DENSITY) == (0, 1, 2, 3)
    assert len(capi._SIGS["grlx_evaluate_actor_ensemble"][1]) == 18 and len(capi._SIGS["grlx_evaluate_actor_ensemble_trajectory"][1]) == 19
    assert grl_amd.ActorEnsembleEvaluation._fields == ae.FIELDS == ("ret", "disc", "steps", "terminal", "ties", "kept", "spread", "final_state")
    assert grl_amd.ActorEnsembleTrajectory._fields == ("ret", "disc", "steps", "terminal", "ties", "n_kept", "total_spread", "final_state", "records")
    for name in ("ActorEnsembleEvaluation", "ActorEnsembleTrajectory"):
        assert name in grl_amd.__all__
    for name in ("evaluate_actor_ensemble", "evaluate_actor_ensemble_trajectory", "actor_ensemble_trajectory_record_words"):
        assert callable(getattr(grl_amd.Runner, name))
    import inspect
    sig = inspect.signature(grl_amd.Runner.evaluate_actor_ensemble)
    assert [sig.parameters[k].default for k in ("rule", "bins", "r", "replicas", "max_steps")] == ["mean", 10, 0.001, None, 0], "the reference's defaults"
    # the header states the rules in the reference module's words
    for phrase in ("starting from the first one and not from", "Members of ANOTHER bin with the same count are included", "scanning from -inf",
                   "No clip follows the", "the FIRST acts"):
        assert phrase in header, phrase


def test_the_views_of_an_actor_ensemble_trajectory():
    import grl_amd
    rec = np.arange(2 * 3 * 4 * 17, dtype=np.float64).reshape(2, 3, 4, 17)          # the cart-pole's 15 words, the step's kept and its spread
    t = grl_amd.ActorEnsembleTrajectory(None, None, np.full((2, 3), 2, np.int32), None, None, None, None, np.zeros((2, 3, 5)), rec)
    assert t.obs.shape == (2, 3, 4, 4) and t.state.shape == (2, 3, 4, 5) and t.kept.shape == t.spread.shape == (2, 3, 4)
    assert t.obs[0, 1, 2, 0] == rec[0, 1, 2, 6] and t.state[0, 0, 0, 4] == rec[0, 0, 0, 14]
    assert t.kept[1, 2, 3] == rec[1, 2, 3, 15] and t.spread[1, 2, 3] == rec[1, 2, 3, 16]
    assert t.action[1, 0, 0] == rec[1, 0, 0, 0] and t.value[1, 0, 0] == rec[1, 0, 0, 2] and t.episode(1, 2).shape == (2, 17)
    with pytest.raises(ValueError):
        t.spread[0, 0, 0] = 1.0


# ---- grlxd -A: refused before any device is looked for -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def test_grlxd_usage_mentions_both_ensembles(grlxd, tmp_path):
    res = subprocess.run([grlxd], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    said = res.stdout + res.stderr
    assert res.returncode != 0 and "[-V vote|mean]" in said and "[-A mean|binning[:bins]|data_center[:keep]|density[:r]]" in said


@pytest.mark.parametrize("args,yaml,word", [
    (["-r", "4", "-A", "mean"], "cart_pole-ac-tc.yaml", "needs the start states of -E"),
    (["-r", "4", "-E", "states5.txt", "-A", "median"], "cart_pole-ac-tc.yaml", "unknown rule 'median'"),
    (["-r", "4", "-E", "states5.txt", "-A", ""], "cart_pole-ac-tc.yaml", "unknown rule ''"),
    (["-r", "4", "-E", "states5.txt", "-A", "mean:3"], "cart_pole-ac-tc.yaml", "takes no parameter"),
    (["-r", "4", "-E", "states5.txt", "-A", "binning:0"], "cart_pole-ac-tc.yaml", "a number of bins in 1 ... 64"),
    (["-r", "4", "-E", "states5.txt", "-A", "binning:65"], "cart_pole-ac-tc.yaml", "a number of bins in 1 ... 64"),
    (["-r", "4", "-E", "states5.txt", "-A", "binning:"], "cart_pole-ac-tc.yaml", "a number of bins in 1 ... 64"),
    (["-r", "4", "-E", "states5.txt", "-A", "binning:7x"], "cart_pole-ac-tc.yaml", "a number of bins in 1 ... 64"),
    (["-r", "4", "-E", "states5.txt", "-A", "data_center:0"], "cart_pole-ac-tc.yaml", "a number of members kept >= 1"),
    (["-r", "4", "-E", "states5.txt", "-A", "data_center:2.5"], "cart_pole-ac-tc.yaml", "a number of members kept >= 1"),
    (["-r", "4", "-E", "states5.txt", "-A", "density:0"], "cart_pole-ac-tc.yaml", "not a finite radius above 0"),
    (["-r", "4", "-E", "states5.txt", "-A", "density:-1"], "cart_pole-ac-tc.yaml", "not a finite radius above 0"),
    (["-r", "4", "-E", "states5.txt", "-A", "density:nan"], "cart_pole-ac-tc.yaml", "not a finite radius above 0"),
    (["-r", "4", "-E", "states5.txt", "-A", "density:inf"], "cart_pole-ac-tc.yaml", "not a finite radius above 0"),
    (["-r", "4", "-E", "states5.txt", "-A", "density:wide"], "cart_pole-ac-tc.yaml", "not a finite radius above 0"),
    (["-r", "4", "-E", "states.txt", "-A", "mean"], "pendulum-sarsa-tc.yaml", "serves the actor-critic agent only"),
    (["-r", "4", "-g", "2", "-E", "states5.txt", "-A", "mean"], "cart_pole-ac-tc.yaml", "-g 2 is not built"),
    (["-r", "4", "-E", "states.txt", "-A", "density:0.05"], "pendulum-fqi-ann.yaml", "not for experiment/batch_learning"),
    (["-r", "2", "-p", "/experiment/agent/predictor/alpha=0.1,0.2", "-E", "states5.txt", "-A", "mean"], "cart_pole-ac-tc.yaml", "per-replica parameters (-p) are not built"),
])
def test_grlxd_actor_ensemble_refusals_name_their_reason(grlxd, tmp_path, args, yaml, word):
    (tmp_path / "states.txt").write_text("# angle velocity time\n3.14159 0 0\n0 0 0   # upright\n\n1 -2 1.5\n")
    (tmp_path / "states5.txt").write_text("0 3.14159 0 0 0\n0.5 0 0 0 1.0\n")
    res = subprocess.run([grlxd, "-s", "1", "-q", "-t", "12"] + args + [os.path.join(GOLDEN, yaml)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    said = res.stderr + res.stdout
    assert res.returncode != 0 and word in said, said
    assert "-A" in said
    assert "no HIP device" not in said, "refused only after a device was looked for"
    assert not list(tmp_path.glob("*actor-ensemble*"))


def test_grlxd_keeps_refusing_a_vote_of_actors_and_names_the_new_option(grlxd, tmp_path):
    (tmp_path / "states5.txt").write_text("0 3.14159 0 0 0\n0.5 0 0 0 1.0\n")
    res = subprocess.run([grlxd, "-s", "1", "-q", "-t", "12", "-r", "4", "-E", "states5.txt", "-V", "vote", os.path.join(GOLDEN, "cart_pole-ac-tc.yaml")],
                         cwd=tmp_path, capture_output=True, text=True, timeout=120)
    said = res.stderr + res.stdout
    assert res.returncode != 0 and "not built for the actor-critic" in said and "-A" in said, said
