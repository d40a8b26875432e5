"""The batch path's sampled episodes of one network on the GPU (grlx_fqi_evaluate_sampled, grlx_fqi_evaluate_sampled_trajectory) against
tests/fqi_evaluate_sampled_ref.py, on the trained experiments of test_gpu_fqi_evaluate.py.  Every comparison is on bit patterns."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import fqi_evaluate_sampled_ref as fs
from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev
from tests import policy_evaluate_sampled_ref as sr
from tests import test_gpu_fqi_evaluate as single
from tests.test_gpu_fqi_evaluate_ensemble import big_states

pytestmark = pytest.mark.gpu

FULL, SEEDS, start_states, same_bits, bits = single.FULL, single.SEEDS, single.start_states, single.same_bits, single.bits
SAMPLERS = {"greedy": (sr.GREEDY, 0.0), "epsilon": (sr.EPSILON, 0.3)}


def reference(es, states, sampler, eps, streams, max_steps):
    per = [fs.evaluate(e, states, sampler, eps, streams[k], max_steps) for k, e in enumerate(es)]
    return {f: np.stack([p[f] for p in per]) for f in fs.FIELDS + ("records",)}


def check(r, want, states, name, eps, streams, max_steps, replicas, what):
    """the sums call and the trajectory call against the reference: all eight outputs, the records with the zeros behind every end"""
    got = r.evaluate_sampled(states, name, eps, streams, replicas, max_steps)
    traj = r.evaluate_sampled_trajectory(states, max_steps, name, eps, streams, replicas)
    assert traj.records.shape[-1] == r.sampled_trajectory_record_words() == fs.WORDS
    for k, f in enumerate(fs.FIELDS):
        same_bits(got[k], want[f], f"{what}, evaluate_sampled: {f}")
        same_bits(traj[k], want[f], f"{what}, evaluate_sampled_trajectory: {f}")
    same_bits(traj.records, want["records"], f"{what}: records")
    return got


@pytest.mark.parametrize("name", sorted(SAMPLERS))
@pytest.mark.parametrize("hidden", [20, 64])
def test_against_the_reference(grlx, hidden, name):
    """three replicas x the seven states on the streams of episode_streams, max_steps = 100"""
    sampler, eps = SAMPLERS[name]
    states, streams = start_states(), sr.episode_streams(11, len(SEEDS), 7)
    want = reference(single.oracles(hidden), states, sampler, eps, streams, FULL)
    if sampler == sr.GREEDY:
        assert ((want["ties"] > 0) & (want["streams"][..., 1] != streams[..., 1])).any() and not want["explored"].any()
        same_bits(want["streams"][..., 0], streams[..., 0], "the greedy sampler never draws from the sampler's stream")
    else:
        taken = np.arange(FULL) < want["steps"][..., None]
        assert (want["explored"] > 0).any() and len(set(want["records"][..., fs.fr.ACTION_INDEX][taken])) >= 2
    check(single.runner(grlx, hidden), want, states, name, eps, streams, FULL, None, f"hidden = {hidden}, {name}")


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_more_pairs_than_one_wave_and_the_cut(grlx, name):
    """hidden = 20, 67 start states (a second block with 61 dead lanes), replicas 1 and 2, max_steps = 12: code 0 occurs"""
    sampler, eps = SAMPLERS[name]
    states, streams = big_states(), sr.episode_streams(5, 2, 67)
    want = reference(single.oracles(20)[1:3], states, sampler, eps, streams, 12)
    assert (want["terminal"] == 0).any() and (want["terminal"] == 1).any() and (want["steps"] == 1).any()
    check(single.runner(grlx, 20), want, states, name, eps, streams, 12, range(1, 3), f"67 states, {name}")


def test_epsilon_zero_and_one(grlx):
    """epsilon = 0 never explores and still draws from the sampler's stream at every step; epsilon = 1 explores at every step"""
    states, streams = start_states(), sr.episode_streams(7, len(SEEDS), 7)
    for eps in (0.0, 1.0):
        want = reference(single.oracles(20), states, sr.EPSILON, eps, streams, FULL)
        assert (want["explored"] == (want["steps"] if eps else 0)).all() and (want["streams"][..., 0] != streams[..., 0]).all()
        check(single.runner(grlx, 20), want, states, "epsilon", eps, streams, FULL, None, f"epsilon = {eps}")


def test_greedy_without_a_tie_is_evaluate(grlx):
    """under the greedy sampler an episode without a tie equals grlx_fqi_evaluate's in every output and leaves its streams where they were"""
    r, states, streams = single.runner(grlx, 20), start_states(), sr.episode_streams(3, len(SEEDS), 7)
    got, plain = r.evaluate_sampled(states, "greedy", streams=streams), r.evaluate(states)
    free = plain.ties == 0
    assert free.any() and not free.all() and ((got.ties == 0) == free).all()
    for f in ("ret", "disc", "steps", "terminal", "ties", "final_state"):
        same_bits(getattr(got, f)[free], getattr(plain, f)[free], f)
    same_bits(got.streams[free], streams[free], "streams_out against streams")


def test_an_episode_on_the_stream_before_a_batch_is_the_row(grlx):
    """seeds 4 (tie-heavy) and 3 (tie-free), hidden = 20.  A batch draws from the global stream in its test trial only (oracle/fqi.c,
    fqi_generate_kernel), so the episode from (pi, 0, 0) on the G read BEFORE batch k returns row k bit for bit, ties included.  The trial asks
    its policy once more at the observation the timeout ends on: the G read after the batch is streams_out advanced by that one draw where
    that observation ties (seed 4) and streams_out itself where it does not (seed 3)."""
    r = grlx.FqiRunner(grlx.pendulum_fqi_config(2, max_batches=2, hidden=20, **single.SHAPE), [4, 3])
    spec = ob.pendulum_fqi_spec(hidden=20, **single.SHAPE)
    start, tied, extra = np.array([[math.pi, 0.0, 0.0]]), 0, set()
    for k in range(2):
        before = np.array([[[0, r.info(m)["rng"][0]]] for m in range(2)], np.uint64)
        r.run_batch(); r.sync()
        got = r.evaluate_sampled(start, "greedy", streams=before)
        tied += int(got.ties[0, 0])
        assert got.ties[1, 0] == 0 and not got.streams[..., 0].any()
        for m in range(2):
            same_bits(got.ret[m], r.rows(m, k + 1)[2][k:k + 1], f"batch {k}, replica {m}: ret against the row")
            q = r.query([ev.observe(spec.base, got.final_state[m, 0])[0]], replicas=(m, 1))[0, 0]
            extra.add((m, int((q == q.max()).sum() > 1)))
            assert sr.jumped(got.streams[m, 0, 1], int((q == q.max()).sum() > 1)) == r.info(m)["rng"][0], f"batch {k}, replica {m}: the global stream after"
        now = np.array([[[0, r.info(m)["rng"][0]]] for m in range(2)], np.uint64)
        for a, b in zip(r.evaluate_sampled(start), r.evaluate_sampled(start, streams=now)):
            same_bits(a, b, f"batch {k}: streams = None copies the replica's global stream as it stands")
    assert tied > 0 and extra == {(0, 1), (1, 0)}, (tied, extra)
    r.close()


def test_refusals_and_nothing_changes(grlx):
    """the new refusals, on sentinel-filled outputs; a sampled call before and after a batch leaves the context as a twin's"""
    over = dict(batch_size=300, iterations=2, epochs=20)
    cfg = grlx.pendulum_fqi_config(2, max_batches=1, **over)
    r, twin = grlx.FqiRunner(cfg, [1, 2]), grlx.FqiRunner(cfg, [1, 2])
    states, good = start_states(), sr.episode_streams(1, 2, 7)
    bad = good.copy(); bad[1, 3, 1] = 1 << 48
    lib, p = grlx.capi.load(), lambda a, t: a.ctypes.data_as(C.POINTER(t))
    cases = [((2, 0.1, good), "unknown sampler 2"), ((1, float("nan"), good), "not finite"), ((1, 1.5, good), "outside [0, 1]"),
             ((0, -1.0, good), "GRLX_EPSILON_OWN"), ((1, 0.1, None), "streams is null"), ((0, 0.1, bad), "row 10 (replica 1, start state 3), word 1")]
    for (sampler, eps, streams), word in cases:
        ret, out = np.full((2, 7), 7.0), np.full((2, 7, 2), 7, np.uint64)
        rc = lib.grlx_fqi_evaluate_sampled(r._ctx, 0, 2, p(states, C.c_double), 7, 5, sampler, eps, None if streams is None else p(streams, C.c_uint64),
                                           p(ret, C.c_double), None, None, None, None, None, None, p(out, C.c_uint64))
        assert rc == grlx.capi.ERR_INVALID and word in lib.grlx_last_error().decode(), (word, lib.grlx_last_error().decode())
        assert (ret == 7.0).all() and (out == 7).all(), f"{word}: something was written"

    state_of = lambda x: [(x.params(k), x.rows(k, 1), x.info(k), x.transitions(k, 0, cfg.batch_size)) for k in range(2)]
    for when in ("before", "after"):
        r.evaluate_sampled_trajectory(states, 30, "epsilon", 0.3, good)
        r.evaluate_ensemble_sampled_trajectory(states, 2, 30, "rank", 2.0, "softmax", 0.01)
        for (pa, ra, ia, ta), (pb, rb, ib, tb) in zip(state_of(r), state_of(twin)):
            same_bits(pa, pb, f"{when} the batch: parameters")
            assert all(ia[f] == ib[f] for f in ("rng", "n", "iterations")), f"{when} the batch: {ia} vs {ib}"
            same_bits([ia["maxdelta"], ia["error"]], [ib["maxdelta"], ib["error"]], f"{when} the batch: maxdelta, error")
            for a, b in zip(ra + tuple(ta), rb + tuple(tb)):
                same_bits(a, b, f"{when} the batch: rows and stored transitions")
        if when == "before":
            for x in (r, twin):
                x.run_batch(); x.sync()
    r.close(); twin.close()
