"""Noisy evaluation episodes (grlx_evaluate_noisy / Runner.evaluate_noisy and their trajectory call): grlx_evaluate's episodes of the
actor-critic acted by its exploring policy -- the actor's read plus Gaussian / Ornstein-Uhlenbeck noise by Box-Muller from a rand48 stream
the episode carries, clipped to the action range -- against tests/policy_evaluate_noisy_ref.py: a plain Python loop over the oracle's dense
tables, env_step, Rand48 and portable log / cos.  Every comparison is on the bit patterns; there is no tolerance anywhere.  A noisy
evaluation must change nothing in the context.

Shapes: 5 replicas x the 7 start states of test_gpu_policy_evaluate.py = 35 pairs (never a multiple of 4: dead 16-lane groups in the last
wave, a partial block); one case of 17 start states staged in three chunks; max_steps 40 at most; 6 learning trials.  The oracle's half is
computed once per case (every GPU test runs clean and with poisoned registers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import configs
from tests import oracle_binding as ob
from tests import policy_evaluate_noisy_ref as nref
from tests import policy_evaluate_ref as ev
from tests.test_gpu_policy_evaluate import start_states
from tests.test_gpu_policy_query import SEED0, build, same_bits

pytestmark = pytest.mark.gpu

N, TRIALS, MS = 5, 6, 40
STREAM_SEED = 4          # chosen on the oracle's half: with it sigma 5 clips on both cart-pole graphs (under seed 9 the twin-table case never clipped)
GRAPHS = ["ac_twin", "ac_independent", "pendulum_ac"]
_cache = {}


def make(grlx, graph, n=N):
    """(configuration, oracle spec) of a graph; the pendulum's actor-critic is not among test_gpu_policy_query's graphs"""
    if graph != "pendulum_ac":
        return build(grlx, graph, n)
    cfg, spec = configs.pendulum_ac(grlx, n)
    cfg.max_rows = 64
    spec.math = ob.MATH_PORTABLE
    return cfg, spec


def check(got, want, what, records=False):
    """the eight outputs (and the records) of all replicas at once against want[replica]"""
    names = {"clipped": "n_clipped", "noise": "final_noise"} if records else {}
    for f in nref.FIELDS:
        same_bits(getattr(got, names.get(f, f)), np.stack([w[f] for w in want]), f"{what}: {f}")
    if records:
        same_bits(got.records, np.stack([w["records"] for w in want]), f"{what}: records")


def oracle_stages(key, spec, seeds, states, stages, sg, theta, streams, noise, max_steps=MS):
    """[stage][replica] -> the reference's dict; stage s is taken after sum(stages[:s + 1]) trials (0: before any launch).  sg: a number,
    or a function of (spec, learning trials run)"""
    if key not in _cache:
        exps = [ob.Experiment(spec, seed=int(seed)) for seed in seeds]
        out, done = [], 0
        for trials in stages:
            done += trials
            stage = []
            for k, e in enumerate(exps):
                if trials:
                    e.run(trials)
                s = sg(spec, done) if callable(sg) else sg
                stage.append(nref.evaluate(ev.tables_of(e), spec, states, s, theta, streams[k], noise[k], max_steps))
            out.append(stage)
        for e in exps:
            e.close()
        _cache[key] = out
    return _cache[key]


def stacked(stage, f):
    return np.stack([w[f] for w in stage])


# ---- 1: against the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
def test_against_the_reference(grlx, graph):
    """before any launch and after 6 trials, streams from episode_stream_words, sigma = 5, theta = 1: the eight outputs of the plain call
    and the same with the records of the trajectory call"""
    cfg, spec = make(grlx, graph)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + N)
    streams = nref.episode_stream_words(STREAM_SEED, N, len(states))
    noise = np.zeros((N, len(states)))
    want = oracle_stages(("parity", graph), spec, seeds, states, (0, TRIALS), 5.0, 1.0, streams, noise)
    # asserted on the oracle's half, so that a counter stuck at zero cannot pass
    clipped = np.concatenate([stacked(stage, "clipped") for stage in want])
    if graph == "pendulum_ac":
        assert (clipped > 0).sum() > clipped.size // 2, "torques in [-3, 3] under sigma 5 were meant to clip in most pairs"
    else:
        assert (clipped > 0).any(), "sigma 5 was meant to clip in at least one pair"
    codes = set(int(c) for stage in want for w in stage for c in w["terminal"])
    need = {0, 1} if spec.env == ob.ENV_PENDULUM else {0, 1, 2}
    assert need <= codes, f"{graph}: the start states show the terminal codes {sorted(codes)} only"
    same_bits(grlx.episode_stream_words(STREAM_SEED, N, len(states)), streams, "episode_stream_words")
    same_bits(grlx.episode_streams(STREAM_SEED, N, len(states))[..., 0], streams, "the even streams of episode_streams")
    r = grlx.Runner(cfg, seeds)
    assert r.noisy_trajectory_record_words() == r.trajectory_record_words() + 2 == want[0][0]["records"].shape[-1]
    for s, trials in enumerate((0, TRIALS)):
        if trials:
            r.run(trials); r.sync()
        check(r.evaluate_noisy(states, 5.0, 1.0, streams, noise, max_steps=MS), want[s], f"{graph} after {trials} trials")
        check(r.evaluate_noisy_trajectory(states, MS, 5.0, 1.0, streams, noise), want[s], f"{graph} after {trials} trials, trajectory", records=True)
    # ---- 8: a replica range of its own: the middle replica alone, one output only, the others NULL
    ret = np.full(len(states), 777.0)
    st = np.ascontiguousarray(states, np.float64)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    mid = np.ascontiguousarray(streams[2:3])
    rc = r.lib.grlx_evaluate_noisy(r._ctx, 2, 1, P(st, C.c_double), len(states), MS, 5.0, 1.0, P(mid, C.c_uint64), None, P(ret, C.c_double),
                                   None, None, None, None, None, None, None)
    assert rc == 0, r.lib.grlx_last_error().decode()
    same_bits(ret, want[-1][2]["ret"], "replica range, one output: ret")
    got = r.evaluate_noisy(states, 5.0, 1.0, streams[2:3], None, replicas=range(2, 3), max_steps=MS)
    check(got, want[-1][2:3], f"{graph}: replica range")
    r.close()


# ---- 2: Ornstein-Uhlenbeck -----------------------------------------------------------------------------------------------------------
def test_ornstein_uhlenbeck(grlx):
    """theta = 0.15, sigma = 1, a noise array of non-zero entries: against the reference; for start states whose time is not 0 the entry
    shows in the first action, for the start state at time 0 it is reset; theta = 0: the noise is a running sum of the draws"""
    graph = "ac_twin"
    cfg, spec = make(grlx, graph)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + N)
    streams = nref.episode_stream_words(STREAM_SEED, N, len(states))
    noise = np.array([[(0.5 + 0.25 * k + 0.125 * s) * (-1) ** s for s in range(len(states))] for k in range(N)])
    at_zero = states[:, -1] == 0                         # the test start and the state beyond the end stop; every other has run for a while
    assert (noise != 0).all() and at_zero[0] and 0 < at_zero.sum() < len(states) - 1
    want = oracle_stages(("ou", graph), spec, seeds, states, (TRIALS,), 1.0, 0.15, streams, noise)[0]
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    got = r.evaluate_noisy_trajectory(states, MS, 1.0, 0.15, streams, noise)
    check(got, want, "theta 0.15", records=True)
    check(r.evaluate_noisy(states, 1.0, 0.15, streams, noise, max_steps=MS), want, "theta 0.15, the plain call")
    L = ob.load()
    for k in range(N):
        for s in range(len(states)):
            g = ob.Rand48(int(streams[k, s]))
            U1, U2 = float(L.orc_drand48(C.byref(g))), float(L.orc_drand48(C.byref(g)))
            nrm = np.sqrt(-2 * float(L.orc_plog(U1))) * float(L.orc_pcos(2 * np.pi * U2)) * 1.0 + 0.
            before = 0.0 if at_zero[s] else float(noise[k, s])                   # at time 0 the entry is reset
            first = (1 - 0.15) * before + nrm
            assert float(got.noise[k, s, 0]) == first, f"pair ({k}, {s}): the noise state after the first step"
            out = float(got.value[k, s, 0]) + first
            assert float(got.action[k, s, 0]) == min(max(out, spec.action_min), spec.action_max), f"pair ({k}, {s}): the first action"
            assert (float(got.clipped[k, s, 0]) == 1.0) == (out < spec.action_min or out > spec.action_max)
    # theta = 0: a running sum
    run = r.evaluate_noisy_trajectory(states, MS, 1.0, 0.0, streams, noise)
    ind = r.evaluate_noisy_trajectory(states, MS, 1.0, 1.0, streams, noise)
    for k in range(N):
        for s in range(len(states)):
            g, acc = ob.Rand48(int(streams[k, s])), (0.0 if at_zero[s] else float(noise[k, s]))
            for t in range(int(run.steps[k, s])):
                U1, U2 = float(L.orc_drand48(C.byref(g))), float(L.orc_drand48(C.byref(g)))
                nrm = np.sqrt(-2 * float(L.orc_plog(U1))) * float(L.orc_pcos(2 * np.pi * U2)) * 1.0 + 0.
                acc = (1 - 0.0) * acc + nrm
                assert float(run.noise[k, s, t]) == acc, f"pair ({k}, {s}), step {t}: the running sum"
                if t == 0:
                    assert float(ind.noise[k, s, 0]) == (1 - 1.0) * (0.0 if at_zero[s] else float(noise[k, s])) + nrm
            assert int(run.streams[k, s]) == int(g.x) == nref.jumped(streams[k, s], 2 * int(run.steps[k, s])), "two draws per step"
    r.close()


# ---- 3: sigma = 0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["ac_twin", "pendulum_ac"])
def test_sigma_zero_is_the_noise_free_actor(grlx, graph):
    cfg, spec = make(grlx, graph)
    states = start_states(graph, spec)
    streams = grlx.episode_stream_words(STREAM_SEED, N, len(states))
    noise = np.array([[1.5 - 0.5 * k + 0.25 * s for s in range(len(states))] for k in range(N)])
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    r.run(TRIALS); r.sync()
    plain, plain_t = r.evaluate(states, max_steps=MS), r.evaluate_trajectory(states, MS)
    got, got_t = r.evaluate_noisy(states, 0.0, 0.15, streams, noise, max_steps=MS), r.evaluate_noisy_trajectory(states, MS, 0.0, 0.15, streams, noise)
    for f in ("ret", "disc", "steps", "terminal", "final_state"):
        same_bits(getattr(got, f), getattr(plain, f), f"sigma 0: {f} against Runner.evaluate")
        same_bits(getattr(got_t, f), getattr(plain, f), f"sigma 0, trajectory: {f} against Runner.evaluate")
    assert (got.clipped == 0).all() and (got_t.n_clipped == 0).all() and (plain.ties == 0).all()
    same_bits(got.streams, streams, "sigma 0: streams_out == streams")
    same_bits(got_t.streams, streams, "sigma 0, trajectory: streams_out == streams")
    timed = states[:, -1] != 0
    assert 0 < timed.sum() < len(states)
    same_bits(got.noise[:, timed], noise[:, timed], "sigma 0: noise_out == noise where the start time is not 0")
    same_bits(got_t.final_noise[:, timed], noise[:, timed], "sigma 0, trajectory: noise_out == noise where the start time is not 0")
    assert (got.noise[:, ~timed] == 0).all(), "a start at time 0 resets the noise state"
    R = plain_t.records.shape[-1]
    same_bits(got_t.records[..., :R], plain_t.records, "sigma 0: the shared words of the records")
    r.close()


# ---- 4: sigma and theta of the replica's own -----------------------------------------------------------------------------------------
def decayed(spec, learning_trials):
    """ActionPolicy::decay_ after that many learning episodes: decay = fmax(decay * rate, min) once per episode, at its time 0
    (action.cpp:139; oracle/experiment.c: ac_policy_act)"""
    d = 1.0
    for _ in range(learning_trials):
        d = max(d * float(spec.ac_decay_rate), float(spec.ac_decay_min))
    return d


def test_own_sigma_is_the_decayed_one_and_own_theta_the_configurations(grlx):
    graph = "ac_twin"
    cfg, spec = make(grlx, graph)
    for obj in (cfg, spec):
        obj.ac_decay_rate, obj.ac_decay_min, obj.theta = 0.9, 0.2, 0.15
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + N)
    streams = nref.episode_stream_words(STREAM_SEED, N, len(states))
    noise = np.zeros((N, len(states)))
    own = lambda s, done: decayed(s, done) * float(s.sigma)
    assert own(spec, 0) == 5.0 and 2.6 < own(spec, TRIALS) < 2.7
    want = oracle_stages(("own", graph), spec, seeds, states, (0, TRIALS), own, 0.15, streams, noise)
    r = grlx.Runner(cfg, seeds)
    for s, trials in enumerate((0, TRIALS)):
        if trials:
            r.run(trials); r.sync()
        first = r.evaluate_noisy(states, "own", "own", streams, max_steps=MS)
        check(first, want[s], f"own sigma and theta after {trials} trials")
        again = r.evaluate_noisy(states, "own", "own", streams, max_steps=MS)
        for f in nref.FIELDS:
            same_bits(getattr(again, f), getattr(first, f), f"the decay has not moved: {f} of a second call")
    full = r.evaluate_noisy(states, 5.0, 0.15, streams, max_steps=MS)
    assert (full.noise != first.noise).any(), "the undecayed sigma was meant to give other noise"
    r.close()


# ---- 5: the replica's own stream -----------------------------------------------------------------------------------------------------
def test_without_streams_every_episode_starts_from_the_replicas_thread_local_stream(grlx):
    graph = "ac_twin"
    cfg, spec = make(grlx, graph)
    states = start_states(graph, spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    r.run(TRIALS); r.sync()
    before = [list(r.rng(k)) for k in range(N)]
    own = np.array([[before[k][1]] * len(states) for k in range(N)], np.uint64)
    got = r.evaluate_noisy(states, 5.0, 1.0, None, None, max_steps=MS)
    want = r.evaluate_noisy(states, 5.0, 1.0, own, np.zeros(own.shape), max_steps=MS)
    for f in nref.FIELDS:
        same_bits(getattr(got, f), getattr(want, f), f"streams = None: {f}")
    for k in range(N):
        for s in range(len(states)):
            assert int(got.streams[k, s]) == nref.jumped(before[k][1], 2 * int(got.steps[k, s])), f"pair ({k}, {s}): two draws per step from word 1"
    # the noise alone given: the stream is still the replica's own
    noise = np.full(own.shape, 0.75)
    a = r.evaluate_noisy_trajectory(states, MS, 5.0, 0.5, None, noise)
    b = r.evaluate_noisy_trajectory(states, MS, 5.0, 0.5, own, noise)
    same_bits(a.records, b.records, "noise without streams")
    same_bits(a.streams, b.streams, "noise without streams: streams_out")
    assert [list(r.rng(k)) for k in range(N)] == before, "grlx_get_rng moved"
    r.close()


# ---- 6: a call changes nothing -------------------------------------------------------------------------------------------------------
def test_a_noisy_evaluation_changes_nothing(grlx):
    from tests.test_gpu_sweep import check_replica, oracle_run
    graph, n = "ac_twin", 3
    cfg, spec = make(grlx, graph, n)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    streams = grlx.episode_stream_words(STREAM_SEED, n, len(states))
    r = grlx.Runner(cfg, seeds)

    def look():
        return (r.snapshot(), [[r.table_load(k, t) for t in range(2)] for k in range(n)], [list(r.rng(k)) for k in range(n)],
                [r.env_state(k).tobytes() for k in range(n)], r.step_counts())

    def both_calls():
        r.evaluate_noisy(states, "own", "own", None, None, max_steps=MS)
        r.evaluate_noisy(states, 5.0, 1.0, streams, None, max_steps=MS)
        r.evaluate_noisy_trajectory(states[:3], MS, 2.0, 0.15, None, None, replicas=range(1, 3))

    before = look()
    both_calls()
    assert look() == before, "a noisy evaluation before the first launch changed the context"
    r.run(TRIALS); r.sync()
    before = look()
    both_calls()
    after = look()
    assert after[0] == before[0], "a noisy evaluation changed the context's snapshot"
    assert after[1:] == before[1:], "a noisy evaluation changed table occupancy, a stream, an environment state or a counter"
    r.run(TRIALS); r.sync()
    for k in range(n):
        want = oracle_run(spec, seeds[k], (("run", TRIALS), ("run", TRIALS)), cfg.projector.memory, tables=(0, 1))
        check_replica(r, k, want, f"{graph}: replica {k} after noisy evaluations in between", cfg.projector.memory, n_rng=2)
    r.close()


# ---- 7: chunk invariance -------------------------------------------------------------------------------------------------------------
def test_chunked_staging_gives_the_same_bits(grlx):
    """17 start states under a bound that holds 6 of them: chunks of 6, 6 and 5.  streams and noise are [replica][start], so a chunk's
    rows are strided in the caller's arrays -- in and out"""
    graph, ms, n = "ac_twin", 30, 3
    cfg, spec = make(grlx, graph, n)
    states = np.array([[-2.0 + 0.25 * i, 0.4 * i, 0.5 * i - 4.0, 3.0 - 0.3 * i, 8.0 + 0.1 * i] for i in range(17)], np.float64)
    S = states.shape[1]
    streams = grlx.episode_stream_words(STREAM_SEED, n, 17)
    noise = np.array([[0.25 * k - 0.125 * s for s in range(17)] for k in range(n)])
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(TRIALS); r.sync()
    lib = grlx.capi.load()
    R = r.noisy_trajectory_record_words()
    whole = r.evaluate_noisy(states, 5.0, 0.15, streams, noise, max_steps=ms)
    whole_t = r.evaluate_noisy_trajectory(states, ms, 5.0, 0.15, streams, noise)
    own = r.evaluate_noisy(states, 5.0, 0.15, None, None, max_steps=ms)
    assert len(set(whole.steps.ravel().tolist())) > 1
    try:
        per_start = 8 * S + n * (2 * 8 + 3 * 4 + 8 * S + 4 * 8)
        assert lib.grlx_set_query_chunk_bytes(6 * per_start) == 0
        got = r.evaluate_noisy(states, 5.0, 0.15, streams, noise, max_steps=ms)
        got_own = r.evaluate_noisy(states, 5.0, 0.15, None, None, max_steps=ms)
        assert lib.grlx_set_query_chunk_bytes(6 * (per_start + n * ms * R * 8)) == 0
        got_t = r.evaluate_noisy_trajectory(states, ms, 5.0, 0.15, streams, noise)
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    names = {"clipped": "n_clipped", "noise": "final_noise"}
    for f in nref.FIELDS:
        same_bits(getattr(got, f), getattr(whole, f), f"{f} in three chunks")
        same_bits(getattr(got_own, f), getattr(own, f), f"{f} in three chunks, the replicas' own streams")
        same_bits(getattr(got_t, names.get(f, f)), getattr(whole_t, names.get(f, f)), f"trajectory: {f} in three chunks")
        same_bits(getattr(whole_t, names.get(f, f)), getattr(whole, f), f"trajectory: {f} against the sibling")
    same_bits(got_t.records, whole_t.records, "records in three chunks")
    for k in range(n):
        for s in range(17):
            assert not whole_t.records[k, s, int(whole_t.steps[k, s]):].view(np.uint64).any(), f"pair ({k}, {s}): records behind the episode's end"
    r.close()


# ---- 9: refusals ---------------------------------------------------------------------------------------------------------------------
def raw(grlx, r, states, first=0, count=3, max_steps=0, n_starts=None, null_states=False, sigma=1.0, theta=1.0, streams=None, noise=None, trajectory=False):
    """either entry point on outputs filled with a pattern: (status, message, outputs untouched?)"""
    states = np.ascontiguousarray(states, np.float64)
    n = states.shape[0] if n_starts is None else n_starts
    rows, S = max(count, 1) * max(n, 1), states.shape[1]
    f64 = [np.full(rows, 777.0) for _ in range(2)] + [np.full(rows * S, 777.0), np.full(rows, 777.0)]
    i32 = [np.full(rows, 777, np.int32) for _ in range(3)]
    u64 = [np.full(rows, 777, np.uint64)]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    args = [r._ctx, first, count, None if null_states else P(states, C.c_double), n, max_steps, sigma, theta,
            None if streams is None else P(streams, C.c_uint64), None if noise is None else P(noise, C.c_double),
            P(f64[0], C.c_double), P(f64[1], C.c_double), P(i32[0], C.c_int32), P(i32[1], C.c_int32), P(i32[2], C.c_int32), P(f64[2], C.c_double),
            P(u64[0], C.c_uint64), P(f64[3], C.c_double)]
    if trajectory:
        f64.append(np.full(rows * max(max_steps, 1) * 32, 777.0))
        rc = r.lib.grlx_evaluate_noisy_trajectory(*args, P(f64[4], C.c_double))
    else:
        rc = r.lib.grlx_evaluate_noisy(*args)
    return rc, r.lib.grlx_last_error().decode(), all((a == 777).all() for a in f64 + i32 + u64)


def refused(grlx, r, word, states, **kw):
    for trajectory in (False, True):
        who = "grlx_evaluate_noisy_trajectory" if trajectory else "grlx_evaluate_noisy"
        k = dict(kw)
        if trajectory and "max_steps" not in k:
            k["max_steps"] = 7
        rc, msg, untouched = raw(grlx, r, states, trajectory=trajectory, **k)
        assert rc == grlx.capi.ERR_INVALID and word in msg and who in msg, (rc, msg)
        assert untouched, "a refused call wrote to its outputs"


def test_refusals(grlx):
    cfg, spec = make(grlx, "ac_twin", 3)
    states = start_states("ac_twin", spec)
    r = grlx.Runner(cfg, [1, 2, 3])
    # everything grlx_evaluate refuses
    refused(grlx, r, "states is null", states, null_states=True)
    refused(grlx, r, "n_starts = -1", states, n_starts=-1)
    refused(grlx, r, "replica range", states, first=2, count=2)
    refused(grlx, r, "max_steps = -1", states, max_steps=-1)
    refused(grlx, r, "max_steps = 100001", states, max_steps=100001)
    bad = states.copy(); bad[2, 1] = np.nan
    refused(grlx, r, "row 2, component 1 is not finite", bad)
    bad[2, 1] = 0.0; bad[3, 0] = -2.0 ** 17
    refused(grlx, r, "2^17", bad)
    # sigma, theta, the streams, the noise
    for v in (np.nan, np.inf, -np.inf):
        refused(grlx, r, "sigma is not finite", states, sigma=v)
        refused(grlx, r, "theta is not finite", states, theta=v)
    for v in (-0.5, -1.0000001, -2.0):
        refused(grlx, r, "is negative and is not GRLX_SIGMA_OWN", states, sigma=v)
    for v in (-0.5, 1.0000001, -1.0000001, -2.0):
        refused(grlx, r, "outside [0, 1]", states, theta=v)
    streams = grlx.episode_stream_words(STREAM_SEED, 3, len(states))
    bad = streams.copy(); bad[1, 2] = 1 << 48
    refused(grlx, r, "stream row 9 (replica 1, start state 2)", states, streams=bad)
    bad = streams.copy(); bad[2, 4] = (1 << 64) - 1
    refused(grlx, r, "stream row 18 (replica 2, start state 4)", states, streams=bad)
    noise = np.zeros((3, len(states)))
    for v in (np.nan, np.inf, -np.inf):
        bad = noise.copy(); bad[1, 5] = v
        refused(grlx, r, "noise row 12 (replica 1, start state 5) is not finite", states, noise=bad)
    # the trajectory call's own
    rc, msg, untouched = raw(grlx, r, states, trajectory=True, max_steps=0)
    assert rc == grlx.capi.ERR_INVALID and "max_steps = 0" in msg and "grlx_evaluate_noisy_trajectory" in msg and untouched
    lib = grlx.capi.load()
    try:
        lib.grlx_set_query_chunk_bytes(1000)
        rc, msg, untouched = raw(grlx, r, states, trajectory=True, max_steps=7)
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    assert rc == grlx.capi.ERR_INVALID and "grlx_evaluate_noisy_trajectory" in msg and untouched
    assert "fewer replicas" in msg and "smaller max_steps" in msg and "grlx_set_query_chunk_bytes" in msg
    with pytest.raises(ValueError):
        r.evaluate_noisy(states, streams=streams[:, :3])
    with pytest.raises(ValueError):
        r.evaluate_noisy(states, noise=noise[:2])
    with pytest.raises(ValueError):
        r.evaluate_noisy(states, sigma="decayed")
    # nothing to do is no error, and nothing is written; the ends of the ranges, both OWNs and the largest stream word are accepted
    for trajectory in (False, True):
        assert raw(grlx, r, states, n_starts=0, max_steps=7, trajectory=trajectory)[::2] == (0, True)
        assert raw(grlx, r, states, first=1, count=0, max_steps=7, trajectory=trajectory)[::2] == (0, True)
    ok = streams.copy(); ok[0, 0] = (1 << 48) - 1
    for sigma, theta in ((0.0, 0.0), (1e6, 1.0), (-1.0, -1.0)):
        assert raw(grlx, r, states, sigma=sigma, theta=theta, streams=ok, noise=noise, max_steps=7)[0] == 0
    r.close()

    # (grlx_evaluate's refusal of projector/tile_coding:safe >= 1 cannot be reached: grlx_create admits no actor-critic context with it)
    q, q_spec = build(grlx, "pendulum_sarsa", 3)
    q_states = start_states("pendulum_sarsa", q_spec)
    r = grlx.Runner(q, [1, 2, 3])
    refused(grlx, r, "actor-critic only", q_states)
    refused(grlx, r, "grlx_evaluate_sampled", q_states)
    assert r.lib.grlx_noisy_trajectory_record_words(r._ctx) == grlx.capi.ERR_INVALID
    r.close()

    ext, _ = make(grlx, "ac_twin", 3)
    ext.env = grlx.capi.ENV_EXTERNAL
    ext.control_step, ext.timeout, ext.integration_steps = 0.0, 0.0, 0
    r = grlx.Runner(ext, [1, 2, 3])
    refused(grlx, r, "no environment", states)
    r.close()


# ---- 10: grlxd -E -N -----------------------------------------------------------------------------------------------------------------
def test_grlxd_noisy_evaluation(grlx, tmp_path):
    """golden cart-pole actor-critic yaml, -r 4 -t 12, -E -N 2.5 -T 12: <output>-0-noisy.txt against Runner.evaluate_noisy on an identical
    context with episode_stream_words(seed, ...), the configuration's theta and the host's sums (ascending clones, two passes), number
    for number; the noisy-trajectories file against the records; the returns file byte for byte that of the run without -N"""
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "cart_pole-ac-tc.yaml")
    states = np.array([[0.0, np.pi, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0, 1.0], [-1.5, 0.4, 2.0, -3.0, 2.5], [2.2, 3.0, 4.0, 1.0, 9.9], [0.1, 0.2, -0.3, 0.4, 11.0]])
    (tmp_path / "states.txt").write_text("# x theta xd thetad time\n" + "\n".join(" ".join(repr(float(v)) for v in s) for s in states) + "\n")
    base = [grlxd, "-s", "5", "-r", "4", "-t", "12", "-q", "-E", os.path.join("..", "states.txt")]
    (tmp_path / "plain").mkdir(); (tmp_path / "with_n").mkdir()
    for d, extra in (("plain", []), ("with_n", ["-N", "2.5", "-T", "12"])):
        res = subprocess.run(base + extra + [yaml], cwd=tmp_path / d, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr + res.stdout
    name = "cart_pole-ac-tc-0-"
    assert (tmp_path / "with_n" / (name + "returns.txt")).read_bytes() == (tmp_path / "plain" / (name + "returns.txt")).read_bytes()
    assert not (tmp_path / "plain" / (name + "noisy.txt")).exists()

    cfg = grlx.cart_pole_ac_config(4, max_rows=8)
    r = grlx.Runner(cfg, [5, 6, 7, 8])
    r.run(12); r.sync()
    streams = grlx.episode_stream_words(5, 4, len(states))
    got = r.evaluate_noisy(states, 2.5, "own", streams)
    traj = r.evaluate_noisy_trajectory(states, 12, 2.5, "own", streams)
    r.close()
    lines = [ln.split() for ln in (tmp_path / "with_n" / (name + "noisy.txt")).read_text().split("\n") if ln.strip()]
    assert len(lines) == states.shape[0]
    for s, f in enumerate(lines):
        assert len(f) == 9, f
        total = steps = 0.0
        for k in range(4):
            total += float(got.ret[k, s]); steps += float(got.steps[k, s])
        mean, sq = total / 4, 0.0
        for k in range(4):
            sq += (float(got.ret[k, s]) - mean) * (float(got.ret[k, s]) - mean)
        assert [float(f[0]), float(f[1]), float(f[2])] == [mean, float(np.sqrt(sq / 3)), steps / 4], f"start state {s}: {f}"
        assert [int(x) for x in f[3:7]] == [int((got.terminal[:, s] == c).sum()) for c in range(4)], f"start state {s}: codes"
        assert int(f[7]) == 0 and int(f[8]) == int(got.clipped[:, s].sum()), f"start state {s}"
    assert (got.noise != 0).any()
    R = traj.records.shape[-1]
    tl = [ln.split() for ln in (tmp_path / "with_n" / (name + "noisy-trajectories.txt")).read_text().split("\n") if ln.strip()]
    assert len(tl) == int(traj.steps.sum())
    at = 0
    for k in range(4):
        for s in range(states.shape[0]):
            for t in range(int(traj.steps[k, s])):
                f = tl[at]; at += 1
                assert [int(x) for x in f[:3]] == [k, s, t] and len(f) == 3 + R
                assert [float(x) for x in f[3:]] == [float(v) for v in traj.records[k, s, t]], f"clone {k}, start {s}, step {t}"
