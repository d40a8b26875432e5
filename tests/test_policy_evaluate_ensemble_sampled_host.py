"""Sampled ensemble episodes (grlx_evaluate_ensemble_sampled), the parts that need no device: the reference module's step by hand, the
declarations and the binding's shapes, the views of a SampledEnsembleTrajectory, a null context.  The
refusals that need a context are in test_gpu_policy_evaluate_ensemble_sampled.py.

By hand.  softmax([2, 1, 1], 1): maxp = 2, center = -48; e = pexp(50), pexp(49), pexp(49); every entry is kept.  softmax([200, 1, 1], 1):
minp = 100, the two 1s are dropped: [1, 0, 0].  EPSILON 0.3 on q = [5, 7, 7]: greedy d = [0, .5, .5], no entry is 1, so d = [.1, .6, .6];
on q = [5, 7, 6]: d = [0, 1, 0] -> [.1, (1 - .3) + .1, .1].  e = 1 on an untied q: d = [1/3, (1 - 1) + 1/3, 1/3]: no entry is above the
first, the vote is action 0 and not the maximum.  An all-zero d votes for NA - 1."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import policy_evaluate_ensemble_sampled_ref as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("grlx_evaluate_ensemble_sampled", "grlx_ensemble_sampled_trajectory_record_words", "grlx_evaluate_ensemble_sampled_trajectory")


def test_the_step_by_hand(oracle):
    d = es.softmax([2, 1, 1], 1.0)
    total = es.pexp(50.0) + es.pexp(49.0) + es.pexp(49.0)
    assert d == [es.pexp(50.0) / total, es.pexp(49.0) / total, es.pexp(49.0) / total] and abs(d[0] - np.e / (np.e + 2)) < 1e-12
    assert es.softmax([200, 1, 1], 1.0) == [1.0, 0.0, 0.0] and es.softmax([0, 0, 0], 0.1) == [es.pexp(50.0) / (3 * es.pexp(50.0))] * 3
    assert es.member_distribution([5., 7., 7.], es.GREEDY, 0.) == ([0., .5, .5], 2)
    assert es.member_distribution([5., 7., 7.], es.EPSILON, .3)[0] == [.3 / 3, .5 + .3 / 3, .5 + .3 / 3]
    assert es.member_distribution([5., 7., 6.], es.EPSILON, .3)[0] == [.3 / 3, (1 - .3) + .3 / 3, .3 / 3]
    uniform = es.member_distribution([5., 7., 6.], es.EPSILON, 1.)[0]
    assert uniform == [1 / 3] * 3 and es.vote_of(uniform) == 0, "e = 1: the first entry takes the vote, not the maximum"
    assert es.vote_of([0., 0., 0.]) == 2 and es.vote_of([.2, .5, .5]) == 1
    assert es.ranks_of([.5, .2, .3]) == [3, 1, 2] and es.ranks_of([0., .5, .5]) == [1, 2, 2] and es.ranks_of([1 / 3] * 3) == [1, 1, 1]


def test_the_binding_names_what_the_header_declares():
    import inspect
    import grl_amd
    from grl_amd import capi
    header = open(os.path.join(ROOT, "include", "grlx.h")).read()
    for name in NAMES:
        assert name + "(" in header and name in capi._SIGS and name in capi._NEWER_SIGS
    assert [len(capi._SIGS[n][1]) for n in NAMES] == [22, 1, 23]
    assert "GRLX_ENSEMBLE_MAJORITY = 0, GRLX_ENSEMBLE_RANK = 1" in header and (capi.ENSEMBLE_MAJORITY, capi.ENSEMBLE_RANK) == (es.MAJORITY, es.RANK) == (0, 1)
    assert "GRLX_MEMBER_GREEDY = 0, GRLX_MEMBER_EPSILON = 1, GRLX_MEMBER_SOFTMAX = 2" in header
    assert (capi.MEMBER_GREEDY, capi.MEMBER_EPSILON, capi.MEMBER_SOFTMAX) == (es.GREEDY, es.EPSILON, es.SOFTMAX) == (0, 1, 2)
    assert grl_amd.SampledEnsembleEvaluation._fields == es.FIELDS
    assert grl_amd.SampledEnsembleTrajectory._fields == es.FIELDS[:7] + ("n_explored",) + es.FIELDS[8:] + ("records",)
    sig = inspect.signature(grl_amd.Runner.evaluate_ensemble_sampled)
    assert list(sig.parameters)[1:] == ["states", "group_size", "strategy", "tau", "member", "member_param", "streams", "replicas", "max_steps"]
    assert [sig.parameters[k].default for k in ("strategy", "tau", "member", "member_param", "streams", "replicas", "max_steps")] == \
        ["majority", 0.1, "greedy", None, None, None, 0]
    for phrase in ("those\n * draws are not made", "pow(x, 50)", "grlx_evaluate_actor_ensemble's"):
        assert phrase in header, phrase


def test_the_views_of_a_sampled_ensemble_trajectory():
    import grl_amd
    rec = np.arange(2 * 3 * 4 * 15, dtype=np.float64).reshape(2, 3, 4, 15)          # the pendulum's 13 ensemble words, explored and prob
    t = grl_amd.SampledEnsembleTrajectory(*[None] * 2, np.full((2, 3), 2, np.int32), *[None] * 5, np.zeros((2, 3, 3)), None, rec)
    assert t.obs.shape == (2, 3, 4, 2) and t.state.shape == (2, 3, 4, 3) and t.explored.shape == t.prob.shape == (2, 3, 4)
    assert t.obs[0, 1, 2, 0] == rec[0, 1, 2, 8] and t.state[0, 0, 0, 2] == rec[0, 0, 0, 12] and t.step_agreement[1, 1, 1] == rec[1, 1, 1, 6]
    assert t.explored[1, 2, 3] == rec[1, 2, 3, 13] and t.prob[1, 2, 3] == rec[1, 2, 3, 14] and t.episode(1, 2).shape == (2, 15)
    with pytest.raises(ValueError):
        t.prob[0, 0, 0] = 1.0


def test_a_null_context_is_refused_without_a_device(grlx):
    lib = grlx.capi.load()
    states, out = np.array([[np.pi, 0.0, 0.0]]), np.full(1, 7.0)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = lib.grlx_evaluate_ensemble_sampled(None, 0, 1, 1, 0, 0.1, 0, 0.0, P(states, C.c_double), 1, 4, None, P(out, C.c_double), *[None] * 9)
    assert rc == grlx.capi.ERR_INVALID and out[0] == 7.0
    assert lib.grlx_ensemble_sampled_trajectory_record_words(None) == grlx.capi.ERR_INVALID
