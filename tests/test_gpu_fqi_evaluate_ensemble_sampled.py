"""The batch path's sampled ensemble on the GPU (grlx_fqi_evaluate_ensemble_sampled, grlx_fqi_evaluate_ensemble_sampled_trajectory) against
tests/fqi_evaluate_sampled_ref.py.  Every comparison is on bit patterns.

Members: the initial networks of 37 seeds at hidden = 20 (no batch) for the group sizes, and the trained seeds 3, 4, 5 of
test_gpu_fqi_evaluate.py at hidden = 64 as one group.  The 7 start states leave the last wave with one dead row.  tau starts from 1.0
(majority) and from the group size (rank); on the CPU oracle only the majority vote of 33 near-unanimous networks needed more (8.0) to
explore.  tau_m = 1e-8 makes the initial networks' Q differences of about 1e-5 exceed 100 tau_m: already the single-member group drops
an entry (p_i <= minp), as does every other softmax case (`dropped`, asserted per grouping)."""
import ctypes as C

import numpy as np
import pytest

from tests import fqi_evaluate_sampled_ref as fs
from tests import oracle_binding as ob
from tests import policy_evaluate_ensemble_sampled_ref as esr
from tests import policy_evaluate_sampled_ref as sr
from tests import test_gpu_fqi_evaluate as single
from tests.test_gpu_fqi_evaluate_ensemble import big_states

pytestmark = pytest.mark.gpu

FULL, start_states, same_bits = single.FULL, single.start_states, single.same_bits
SEEDS37 = list(range(1, 38))
STRATEGIES = {"majority": esr.MAJORITY, "rank": esr.RANK}
MEMBERS = {"greedy": (esr.GREEDY, 0.0), "epsilon": (esr.EPSILON, 0.2), "softmax": (esr.SOFTMAX, 1e-8)}
# (replicas, group size, max_steps, compare the records?): a single member; 13 idle lanes per row; one full round; a second round with 15
# idle lanes; a third round; two groups in one call
GROUPINGS = ((1, 1, FULL, False), (3, 3, FULL, True), (16, 16, FULL, False), (17, 17, 12, True), (33, 33, 12, False), (32, 16, FULL, False))

tau_of = lambda strategy, g: (8.0 if g == 33 else 1.0) if strategy == "majority" else float(g)      # noqa: E731
_made = {}


def initial(grlx=None):
    """the 37 initial networks: the oracle's experiments, and with grlx the context that holds the same ones"""
    if "oracles" not in _made:
        _made["oracles"] = [ob.FqiExperiment(ob.pendulum_fqi_spec(hidden=20, **single.SHAPE), seed=s) for s in SEEDS37]
    if grlx is not None and "runner" not in _made:
        _made["runner"] = grlx.FqiRunner(grlx.pendulum_fqi_config(37, max_batches=1, hidden=20, **single.SHAPE), SEEDS37)
    return _made["oracles"], _made.get("runner")


def reference(es, g, states, strategy, tau, member, param, streams, max_steps, seen=None):
    per = [fs.evaluate_ensemble(es[k * g:(k + 1) * g], states, STRATEGIES[strategy], tau, member, param, streams[k], max_steps, seen) for k in range(len(es) // g)]
    return {f: np.stack([p[f] for p in per]) for f in fs.ENS_FIELDS + ("records",)}


def check(r, want, count, g, states, strategy, tau, mname, param, streams, max_steps, records, what):
    got = r.evaluate_ensemble_sampled(states, g, strategy, tau, mname, param, streams, (0, count), max_steps)
    for k, f in enumerate(fs.ENS_FIELDS):
        same_bits(got[k], want[f], f"{what}: {f}")
    if records:
        traj = r.evaluate_ensemble_sampled_trajectory(states, g, max_steps, strategy, tau, mname, param, streams, (0, count))
        assert traj.records.shape[-1] == r.ensemble_sampled_trajectory_record_words() == fs.ENS_WORDS
        for k, f in enumerate(fs.ENS_FIELDS):
            same_bits(traj[k], want[f], f"{what}, trajectory: {f}")
        same_bits(traj.records, want["records"], f"{what}: records, zeros behind the ends included")


def explores(want, what):
    """the reference itself explores and draws at least two indices, in every group"""
    taken = np.arange(want["records"].shape[2]) < want["steps"][..., None]
    for k in range(want["steps"].shape[0]):
        assert want["explored"][k].sum() > 0 and len(set(want["records"][k][..., 3][taken[k]])) >= 2, f"{what}, group {k}"


@pytest.mark.parametrize("mname", sorted(MEMBERS))
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_against_the_reference(grlx, strategy, mname):
    member, param = MEMBERS[mname]
    states = start_states()
    es, _ = initial()
    cases = []
    for count, g, max_steps, records in GROUPINGS:
        streams, seen = sr.episode_streams(9, count // g, 7)[..., 0], {}
        want = reference(es[:count], g, states, strategy, tau_of(strategy, g), member, param, streams, max_steps, seen)
        explores(want, f"{strategy}, {mname}, {count} in groups of {g}")
        assert member != esr.SOFTMAX or seen.get("dropped"), f"{count} in groups of {g}: no softmax member drops an entry"
        cases.append((count, g, max_steps, records, streams, want))
    trained, tstreams = single.oracles(64), sr.episode_streams(9, 1, 7)[..., 0]
    twant = reference(trained, 3, states, strategy, tau_of(strategy, 3), member, param, tstreams, FULL)
    explores(twant, f"{strategy}, {mname}, the trained group")
    assert twant["ties"].sum() > 0 and twant["member_ties"].sum() > 0

    _, r = initial(grlx)
    for count, g, max_steps, records, streams, want in cases:
        check(r, want, count, g, states, strategy, tau_of(strategy, g), mname, param, streams, max_steps, records, f"{strategy}, {mname}, {count} in groups of {g}")
    check(single.runner(grlx, 64), twant, 3, 3, states, strategy, tau_of(strategy, 3), mname, param, tstreams, FULL, False, f"{strategy}, {mname}, trained")


def test_several_blocks(grlx):
    """67 start states x 2 groups of 16: 17 blocks per group, the last with three dead rows; max_steps = 12"""
    states = big_states()
    es, r = initial(grlx)
    streams = sr.episode_streams(4, 2, 67)[..., 1]
    want = reference(es[:32], 16, states, "rank", 16.0, esr.SOFTMAX, 1e-8, streams, 12)
    assert (want["terminal"] == 0).any() and (want["terminal"] == 1).any()
    check(r, want, 32, 16, states, "rank", 16.0, "softmax", 1e-8, streams, 12, True, "67 states, 2 groups of 16")
    own = r.evaluate_ensemble_sampled(states[:7], 16, replicas=(0, 32), max_steps=12)             # streams = None: G of each group's first replica
    first = np.array([[r.info(0)["rng"][0]] * 7, [r.info(16)["rng"][0]] * 7], np.uint64)
    same_bits(own.ret, r.evaluate_ensemble_sampled(states[:7], 16, streams=first, replicas=(0, 32), max_steps=12).ret, "streams = None")


def test_refusals(grlx):
    """the new refusals only, on sentinel-filled outputs"""
    _, r = initial(grlx)
    states, good = start_states(), sr.episode_streams(1, 2, 7)[..., 0].copy()
    bad = good.copy(); bad[1, 2] = 1 << 48
    lib, p = grlx.capi.load(), lambda a, t: a.ctypes.data_as(C.POINTER(t))
    ok = dict(strategy=0, tau=1.0, member=0, param=0.0, streams=good)
    cases = [(dict(strategy=2), "unknown strategy 2"), (dict(tau=0.0), "tau = 0"), (dict(tau=float("inf")), "tau = inf"), (dict(member=3), "unknown member sampler 3"),
             (dict(member=1, param=-1.0), "GRLX_EPSILON_OWN"), (dict(member=1, param=1.5), "outside [0, 1]"), (dict(member=2, param=0.0), "tau_m = 0"),
             (dict(streams=bad), "row 9 (group 1, start state 2)")]
    for over, word in cases:
        a = dict(ok, **over)
        ret, out = np.full((2, 7), 7.0), np.full((2, 7), 7, np.uint64)
        rc = lib.grlx_fqi_evaluate_ensemble_sampled(r._ctx, 0, 6, 3, a["strategy"], a["tau"], a["member"], a["param"], p(states, C.c_double), 7, 5,
                                                    p(a["streams"], C.c_uint64), p(ret, C.c_double), None, None, None, None, None, None, None, None,
                                                    p(out, C.c_uint64))
        assert rc == grlx.capi.ERR_INVALID and word in lib.grlx_last_error().decode(), (word, lib.grlx_last_error().decode())
        assert (ret == 7.0).all() and (out == 7).all(), f"{word}: something was written"
