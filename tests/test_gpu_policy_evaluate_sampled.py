"""Sampled evaluation episodes (grlx_evaluate_sampled / Runner.evaluate_sampled and their trajectory call): grlx_evaluate's episodes acted by
the reference's samplers -- the greedy sampler with its DRAWN tie break, the epsilon-greedy one -- on two rand48 streams per episode, against
tests/policy_evaluate_sampled_ref.py: a plain Python loop over the oracle's dense tables, tile_project, env_step and the oracle's Rand48.
Every comparison is on the bit patterns; there is no tolerance anywhere.  A sampled evaluation must change nothing in the context.

Shapes: 3 replicas x 5 start states = 15 pairs (a dead 16-lane group in the last wave, a partial block); one case of 17 start states staged
in three chunks; max_steps 40 at most (acrobot 6, walker 5, as in test_gpu_policy_evaluate.py); 4 learning trials.  The oracle's half is
computed once per case (every GPU test runs clean and with poisoned registers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_sampled_ref as sref
from tests import policy_query_ref as ref
from tests.test_gpu_policy_evaluate import max_steps_of, start_states
from tests.test_gpu_policy_query import SEED0, build, same_bits

pytestmark = pytest.mark.gpu

N, TRIALS, STREAM_SEED = 3, 4, 9
PICK = [0, 1, 3, 4, 6]          # of the 7 start states: the test start, two tapped, one a step short of the timeout, the hand-made one
SAMPLERS = {"greedy": sref.GREEDY, "epsilon": sref.EPSILON}
_cache = {}


def five_states(graph, spec):
    return np.ascontiguousarray(start_states(graph, spec)[PICK])


def check(got, want, what, records=False):
    """the eight outputs (and the records) of all replicas at once against want[replica]"""
    for f in sref.FIELDS:
        name = "n_explored" if f == "explored" and records else f
        same_bits(getattr(got, name), np.stack([w[f] for w in want]), f"{what}: {f}")
    if records:
        same_bits(got.records, np.stack([w["records"] for w in want]), f"{what}: records")


def oracle_case(key, specs, seeds, trials, states, runs, max_steps, epsilon_of=None):
    """runs: [(sampler name, epsilon or None = own)] -> {run: [replica] -> reference dict}; streams from episode_streams(STREAM_SEED)"""
    if key not in _cache:
        streams = sref.episode_streams(STREAM_SEED, len(specs), len(states))
        out = {run: [] for run in runs}
        for k, (spec, seed) in enumerate(zip(specs, seeds)):
            e = ob.Experiment(spec, seed=int(seed))
            if trials:
                e.run(trials)
            w = ref.dense(e, 0)
            for run in runs:
                eps = run[1] if run[1] is not None else epsilon_of(spec)
                out[run].append(sref.evaluate(w, spec, states, SAMPLERS[run[0]], eps, streams[k], max_steps))
            e.close()
        _cache[key] = (streams, out)
    return _cache[key]


def test_episode_streams_against_rand48_at(grlx):
    """the draw that follows stream k is rand48_at's draw number k * 2^20 of the seed's stream"""
    streams = grlx.episode_streams(SEED0, 2, 3).reshape(-1)
    want = grlx.runner.rand48_at(SEED0, [k * sref.TWO20 for k in range(streams.size)])
    got = np.array([sref.drand48(ob.Rand48(int(x))) for x in streams])
    same_bits(got, want, "episode_streams against rand48_at")


# ---- 1: every instantiation against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum_sarsa", "pendulum_q_five_actions", "acrobot_q", "cart_pole_q", "walker_q"])
def test_every_instantiation_against_the_reference(grlx, graph):
    """after 4 trials, both samplers (epsilon 0.3: both branches of the epsilon-greedy sampler occur), the caller's streams: the eight
    outputs of the plain call, and the same with the records of the trajectory call"""
    cfg, spec = build(grlx, graph, N)
    states, ms = five_states(graph, spec), max_steps_of(graph)
    seeds = np.arange(SEED0, SEED0 + N)
    runs = (("greedy", 0.0), ("epsilon", 0.3))
    streams, want = oracle_case(("parity", graph), [spec] * N, seeds, TRIALS, states, runs, ms)
    same_bits(grlx.episode_streams(STREAM_SEED, N, len(states)), streams, "episode_streams")
    explored = np.stack([w["explored"] for w in want[runs[1]]])
    steps = np.stack([w["steps"] for w in want[runs[1]]])
    assert 0 < explored.sum() < steps.sum(), "epsilon 0.3 was meant to show both branches"
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    assert r.sampled_trajectory_record_words() == r.trajectory_record_words() + 1 == want[runs[0]][0]["records"].shape[-1]
    for run in runs:
        check(r.evaluate_sampled(states, run[0], run[1], streams, max_steps=ms), want[run], f"{graph} {run}")
        check(r.evaluate_sampled_trajectory(states, ms, run[0], run[1], streams), want[run], f"{graph} {run} trajectory", records=True)
    # a replica range of its own: the middle replica alone
    got = r.evaluate_sampled(states, "epsilon", 0.3, streams[1:2], replicas=range(1, 2), max_steps=ms)
    check(got, want[runs[1]][1:2], f"{graph}: replica range")
    r.close()


@pytest.mark.parametrize("graph", ["advantage", "qv", "accumulating", "target_network"])
def test_the_other_q_agents_are_accepted_and_equal_the_reference(grlx, graph):
    """everything grlx_evaluate accepts as a Q agent: advantage learning, QV's table 0, an accumulating trace, a context with a target
    network (the MAIN parameters are read) -- the epsilon-greedy sampler after 4 trials, the plain call"""
    cfg, spec = build(grlx, graph, N)
    states = five_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + N)
    run = ("epsilon", 0.3)
    streams, want = oracle_case(("parity", graph), [spec] * N, seeds, TRIALS, states, (run,), 40)
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    check(r.evaluate_sampled(states, run[0], run[1], streams, max_steps=40), want[run], f"{graph} {run}")
    r.close()


# ---- 2: ties that are drawn -----------------------------------------------------------------------------------------------------------
def test_ties_are_broken_by_the_global_streams_draws(grlx):
    """init_min == init_max on a fresh context: every lazy weight is equal, so man == NA at every step and the (jj + 1)-th maximal entry
    is entry jj.  The greedy sampler's action index at step t is lrand48 % NA of the global stream's t-th draw, ties == steps, and the
    sampler's stream has not moved.  (grlx_evaluate takes index 0 there at every step.)"""
    cfg, spec = build(grlx, "ties", N)
    states = five_states("ties", spec)
    seeds = np.arange(SEED0, SEED0 + N)
    streams, want = oracle_case(("ties", "fresh"), [spec] * N, seeds, 0, states, (("greedy", 0.0),), 40)
    want = want[("greedy", 0.0)]
    r = grlx.Runner(cfg, seeds)
    got = r.evaluate_sampled_trajectory(states, 40, "greedy", 0.0, streams)
    check(got, want, "every step a tie", records=True)
    assert (got.ties == got.steps).all() and (got.steps >= 1).all() and (got.n_explored == 0).all()
    same_bits(got.streams[..., 0], streams[..., 0], "the sampler's stream must not move under the greedy sampler")
    NA = int(cfg.action_steps)
    seen = set()
    for k in range(N):
        for s in range(len(states)):
            g = ob.Rand48(int(streams[k, s, 1]))
            drawn = [sref.lrand48(g) % NA for _ in range(int(got.steps[k, s]))]
            assert [int(v) for v in got.action_index[k, s, :len(drawn)]] == drawn, f"pair ({k}, {s}): the indices are not the stream's draws"
            assert (got.n_max[k, s, :len(drawn)] == NA).all()
            assert int(got.streams[k, s, 1]) == int(g.x), f"pair ({k}, {s}): the global stream after the episode"
            seen |= set(drawn)
    assert seen == set(range(NA)), "the draws were meant to reach every action"
    first = r.evaluate(states, max_steps=40)
    assert (first.ties == first.steps).all(), "grlx_evaluate reports these ties and takes the first maximum"
    r.close()


# ---- 3: epsilon at its ends -----------------------------------------------------------------------------------------------------------
def test_epsilon_at_its_ends(grlx):
    graph = "pendulum_sarsa"
    cfg, spec = build(grlx, graph, N)
    states = five_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + N)
    streams = grlx.episode_streams(STREAM_SEED, N, len(states))
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    NA = int(cfg.action_steps)
    # epsilon = 1: every step explores (drand48 < 1 always), the indices are the global stream's lrand48 % NA
    one = r.evaluate_sampled_trajectory(states, 40, "epsilon", 1.0, streams)
    assert (one.n_explored == one.steps).all() and (one.ties == 0).all()
    for k in range(N):
        for s in range(len(states)):
            n = int(one.steps[k, s])
            g = ob.Rand48(int(streams[k, s, 1]))
            assert [int(v) for v in one.action_index[k, s, :n]] == [sref.lrand48(g) % NA for _ in range(n)], f"pair ({k}, {s})"
            assert int(one.streams[k, s, 1]) == int(g.x) and int(one.streams[k, s, 0]) == sref.jumped(streams[k, s, 0], n)
    # epsilon = 0 on a trained table without ties: grlx_evaluate's outputs; S advanced by exactly `steps` draws, G not at all
    plain = r.evaluate(states, max_steps=40)
    assert (plain.ties == 0).all(), "precondition: no tie on these episodes; choose other seeds"
    zero = r.evaluate_sampled(states, "epsilon", 0.0, streams, max_steps=40)
    greedy = r.evaluate_sampled(states, "greedy", 0.0, streams, max_steps=40)
    for got, what in ((zero, "epsilon 0"), (greedy, "greedy sampler")):
        for f in ("ret", "disc", "steps", "terminal", "ties", "final_state"):
            same_bits(getattr(got, f), getattr(plain, f), f"{what}: {f} against grlx_evaluate")
        assert (got.explored == 0).all()
        same_bits(got.streams[..., 1], streams[..., 1], f"{what}: the global stream must not move")
    for k in range(N):
        for s in range(len(states)):
            assert int(zero.streams[k, s, 0]) == sref.jumped(streams[k, s, 0], int(zero.steps[k, s])), f"pair ({k}, {s}): one epsilon draw per step"
    same_bits(greedy.streams, streams, "greedy sampler without ties: streams_out == streams")
    r.close()


# ---- 4: the reference's own test episode, ties included -------------------------------------------------------------------------------
def test_the_next_test_episode_with_its_ties(grlx):
    """The context of test 2 (all weights equal at first) with test_interval 2 and the representation's output bounded below at -10, run
    trial by trial: after two learning trials the next trial is a test trial, and wherever more than one Q-value has sunk to the bound the
    maximum is not unique -- about half the steps of the test episode draw a tie break, the others do not.  evaluate_sampled(greedy,
    streams=None) from the task's test start state, on copies of the replica's own streams, is that trial: its row's return and episode
    steps, and the global stream the replica is left with.  The pendulum's start draws nothing from that stream, but the trial's END can:
    after a step that timed out the reference's loop hands the last observation to Agent::step once more (online_learning.cpp:210-213; only
    an absorbing state gets Agent::end), and the test policy, acting on it, breaks a tie there too.  So the replica's global stream is
    streams_out's, one draw further where the episode timed out on an observation with a tie."""
    cfg, spec = build(grlx, "ties", N)
    for obj in (cfg, spec):
        obj.test_interval = 2
        obj.representation.output_min = -10.0
    start = start_states("ties", spec)[:1]
    seeds = np.arange(SEED0, SEED0 + N)
    key = ("ties", "next test row")
    if key not in _cache:
        out = []
        for seed in seeds:
            e = ob.Experiment(spec, seed=int(seed))
            e.run(1); e.run(1)
            rng = e.rng()
            dense = ref.dense(e, 0)
            w = sref.evaluate(dense, spec, start, sref.GREEDY, 0.0, [(rng[2], rng[0])], sref.ev.MAX_EPISODE_STEPS)
            last_obs = sref.ev.observe(spec, w["final_state"][0])[0]
            last_tie = int(w["terminal"][0]) == 1 and int(ref.query_q(dense, spec, [last_obs])[3][0]) > 1
            rows = e.run(1)[0]
            out.append((w, rows[-1].reward, int(rows[-1].time), int(e.rng()[0]), 1 if last_tie else 0))
            e.close()
        _cache[key] = out
    want = _cache[key]
    for k, (w, reward, steps, G, more) in enumerate(want):
        assert 0 < w["ties"][0] < w["steps"][0], f"seed {seeds[k]}: the episode was meant to have steps with and steps without a tie"
        assert (w["steps"][0], w["ret"][0]) == (steps, reward), "the reference's loop is not the oracle's test trial"
        assert sref.jumped(w["streams"][0][1], more) == G, "the oracle's global stream after the test trial is not the loop's"
    assert any(more for _, _, _, _, more in want) and not all(more for _, _, _, _, more in want), "both endings were meant to occur"
    r = grlx.Runner(cfg, seeds)
    r.run(1); r.sync(); r.run(1); r.sync()
    got = r.evaluate_sampled(start, "greedy", 0.0, None)
    for f in sref.FIELDS:
        same_bits(getattr(got, f), np.stack([w[f] for w, _, _, _, _ in want]), f"from the test start: {f}")
    first = r.evaluate(start)
    assert any(first.ret[k, 0] != got.ret[k, 0] for k in range(N)), "the first maximum was meant to give another episode than the drawn tie break"
    r.run(1); r.sync()
    for k in range(N):
        _, _, reward = r.rows(k)
        assert int(r.row_times(k, 0, len(reward))[-1]) == int(got.steps[k, 0]) == want[k][2], f"replica {k}: episode steps of the test row"
        same_bits(reward[-1:], got.ret[k], f"replica {k}: return of the test row")
        assert int(r.rng(k)[0]) == sref.jumped(got.streams[k, 0, 1], want[k][4]) == want[k][3], f"replica {k}: the global stream after the test trial"
    r.close()


# ---- 5: GRLX_EPSILON_OWN --------------------------------------------------------------------------------------------------------------
def decayed(spec, learning_trials):
    """EpsilonGreedySampler::decay_ after that many learning episodes: decay = fmax(decay * decay_rate, decay_min) once per episode, at
    its time 0 (greedy.cpp:150-151; oracle/experiment.c: sample_epsilon_greedy) -- the oracle keeps it in a field it does not export"""
    d = 1.0
    for _ in range(learning_trials):
        d = max(d * float(spec.decay_rate), float(spec.decay_min))
    return d


def test_own_epsilon_is_the_decayed_one(grlx):
    """decay_rate 0.8, epsilon 0.6: after 4 learning trials e = 0.8^4 * 0.6 (the products formed one by one), against the Python loop on it"""
    graph = "pendulum_sarsa"
    cfg, spec = build(grlx, graph, N)
    for obj in (cfg, spec):
        obj.decay_rate, obj.decay_min, obj.epsilon = 0.8, 0.01, 0.6
    states = five_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + N)
    e_own = lambda s: decayed(s, TRIALS) * float(s.epsilon)
    assert 0.2 < e_own(spec) < 0.3
    streams, want = oracle_case(("own", graph), [spec] * N, seeds, TRIALS, states, (("epsilon", None),), 40, e_own)
    want = want[("epsilon", None)]
    assert sum(int(w["explored"].sum()) for w in want) > 0
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    check(r.evaluate_sampled(states, "epsilon", "own", streams, max_steps=40), want, "own epsilon")
    full = r.evaluate_sampled(states, "epsilon", 0.6, streams, max_steps=40)
    assert (full.explored != np.stack([w["explored"] for w in want])).any(), "the undecayed epsilon was meant to explore differently"
    r.close()


def test_own_epsilon_in_a_sweep_context(grlx):
    """four epsilons, seeds in equal pairs: before any launch (equal tables, decay 1) two replicas of one seed on equal streams differ
    in `explored` by their epsilon alone; after 4 trials each replica equals its own Python loop on its own decayed epsilon"""
    graph, n, epsilons = "pendulum_sarsa", 4, [0.05, 0.6, 0.3, 0.9]
    cfg, spec = build(grlx, graph, n)
    for obj in (cfg, spec):
        obj.decay_rate, obj.decay_min = 0.9, 0.01
    specs = []
    for eps in epsilons:
        s = type(spec).from_buffer_copy(spec)
        s.epsilon = eps
        specs.append(s)
    states = five_states(graph, spec)
    seeds = np.array([SEED0, SEED0, SEED0 + 1, SEED0 + 1])
    streams = sref.episode_streams(STREAM_SEED, n, len(states))
    streams[1], streams[3] = streams[0], streams[2]          # equal seeds act on equal streams
    key = ("own", "sweep")
    if key not in _cache:
        out = []
        for trials in (0, TRIALS):
            stage = []
            for k in range(n):
                e = ob.Experiment(specs[k], seed=int(seeds[k]))
                if trials:
                    e.run(trials)
                stage.append(sref.evaluate(ref.dense(e, 0), specs[k], states, sref.EPSILON, decayed(specs[k], trials) * epsilons[k], streams[k], 40))
                e.close()
            out.append(stage)
        _cache[key] = out
    want = _cache[key]
    r = grlx.Runner(cfg, seeds)
    r.set_replica_params(epsilon=epsilons)
    got = r.evaluate_sampled(states, "epsilon", "own", streams, max_steps=40)
    check(got, want[0], "sweep, before any launch")
    assert (got.explored[0] != got.explored[1]).any() and (got.explored[2] != got.explored[3]).any()
    r.run(TRIALS); r.sync()
    check(r.evaluate_sampled(states, "epsilon", "own", streams, max_steps=40), want[1], "sweep, after 4 trials")
    r.close()


# ---- 6: a sampled evaluation changes nothing ------------------------------------------------------------------------------------------
def test_a_sampled_evaluation_changes_nothing(grlx):
    graph = "pendulum_sarsa"
    cfg, spec = build(grlx, graph, N)
    states = five_states(graph, spec)
    streams = grlx.episode_streams(STREAM_SEED, N, len(states))
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))

    def look():
        return (r.snapshot(), [r.table_load(k) for k in range(N)], [list(r.rng(k)) for k in range(N)], [r.env_state(k).tobytes() for k in range(N)],
                r.step_counts())

    def every_call():
        r.evaluate_sampled(states, "epsilon", "own", None, max_steps=40)
        r.evaluate_sampled(states, "greedy", 0.0, streams, max_steps=40)
        r.evaluate_sampled_trajectory(states[:3], 40, "epsilon", 0.5, None, replicas=range(1, 3))

    before = look()
    every_call()
    assert look() == before, "a sampled evaluation before the first launch changed the context"
    r.set_replica_params(alpha=[cfg.alpha] * N)          # an evaluation is no launch
    r.run(TRIALS); r.sync()
    before = look()
    every_call()
    assert look() == before, "a sampled evaluation changed the snapshot, table occupancy, a stream, an environment state or a counter"
    r.close()


# ---- 7: chunk invariance --------------------------------------------------------------------------------------------------------------
def test_chunked_staging_gives_the_same_bits(grlx):
    """17 start states under a bound that holds 6 of them: chunks of 6, 6 and 5.  The streams' layout is [replica][start][2], so a chunk's
    rows are strided in the caller's arrays -- in and out"""
    graph, ms = "pendulum_q_five_actions", 30
    cfg, spec = build(grlx, graph, N)
    states = np.array([[-3.0 + 0.4 * i, 0.5 * i - 4.0, 2.0 + 0.06 * i] for i in range(17)], np.float64)          # the later ones time out within 30 steps
    S = states.shape[1]
    streams = grlx.episode_streams(STREAM_SEED, N, 17)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    r.run(TRIALS); r.sync()
    lib = grlx.capi.load()
    R = r.sampled_trajectory_record_words()
    whole = r.evaluate_sampled(states, "epsilon", 0.3, streams, max_steps=ms)
    whole_t = r.evaluate_sampled_trajectory(states, ms, "epsilon", 0.3, streams)
    own = r.evaluate_sampled(states, "epsilon", 0.3, None, max_steps=ms)
    assert len(set(whole.steps.ravel().tolist())) > 1 and whole.explored.sum() > 0
    try:
        per_start = 8 * S + N * (2 * 8 + 4 * 4 + 8 * S + 4 * 8)
        assert lib.grlx_set_query_chunk_bytes(6 * per_start) == 0
        got = r.evaluate_sampled(states, "epsilon", 0.3, streams, max_steps=ms)
        got_own = r.evaluate_sampled(states, "epsilon", 0.3, None, max_steps=ms)
        assert lib.grlx_set_query_chunk_bytes(6 * (per_start + N * ms * R * 8)) == 0
        got_t = r.evaluate_sampled_trajectory(states, ms, "epsilon", 0.3, streams)
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    for f in sref.FIELDS:
        same_bits(getattr(got, f), getattr(whole, f), f"{f} in three chunks")
        same_bits(getattr(got_own, f), getattr(own, f), f"{f} in three chunks, the replicas' own streams")
        name = "n_explored" if f == "explored" else f
        same_bits(getattr(got_t, name), getattr(whole_t, name), f"trajectory: {f} in three chunks")
        same_bits(getattr(whole_t, name), getattr(whole, f), f"trajectory: {f} against the sibling")
    same_bits(got_t.records, whole_t.records, "records in three chunks")
    r.close()


# ---- 8: the trajectory ----------------------------------------------------------------------------------------------------------------
def test_the_records_add_up(grlx):
    """on the context of test 4 after two trials (ties and exploration both occur): the sums are the sibling's, the explored word adds up
    to explored, n_max > 1 on steps that did not explore adds up to ties, records behind an episode's end are zeros"""
    cfg, spec = build(grlx, "ties", N)
    states = five_states("ties", spec)
    streams = grlx.episode_streams(STREAM_SEED, N, len(states))
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    r.run(2); r.sync()
    t = r.evaluate_sampled_trajectory(states, 40, "epsilon", 0.3, streams)
    e = r.evaluate_sampled(states, "epsilon", 0.3, streams, max_steps=40)
    for f in sref.FIELDS:
        same_bits(getattr(t, "n_explored" if f == "explored" else f), getattr(e, f), f"{f} against the sibling")
    assert t.ties.sum() > 0 and t.n_explored.sum() > 0 and len(set(t.steps.ravel().tolist())) > 1
    same_bits(t.explored.sum(axis=2).astype(np.int32), t.n_explored, "the explored word summed")
    same_bits(((t.n_max > 1) & (t.explored == 0)).sum(axis=2).astype(np.int32), t.ties, "ties from the records")
    for k in range(N):
        for s in range(len(states)):
            n = int(t.steps[k, s])
            assert not t.records[k, s, n:].view(np.uint64).any(), f"pair ({k}, {s}): records behind the episode's end"
            ret = 0.0
            for v in t.reward[k, s, :n]:
                ret += float(v)
            assert ret == t.ret[k, s] and t.code[k, s, n - 1] == t.terminal[k, s]
            same_bits(t.state[k, s, n - 1], t.final_state[k, s], f"pair ({k}, {s}): the last record's state")
            assert t.obs.shape[-1] == r.obs_dims
    # the staging refusal is the sibling's and names its remedies
    lib = grlx.capi.load()
    try:
        lib.grlx_set_query_chunk_bytes(1000)
        with pytest.raises(grlx.capi.GrlxError) as ei:
            r.evaluate_sampled_trajectory(states, 40, "epsilon", 0.3, streams)
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    msg = str(ei.value)
    assert ei.value.code == grlx.capi.ERR_INVALID and "grlx_evaluate_sampled_trajectory" in msg
    assert "fewer replicas" in msg and "smaller max_steps" in msg and "grlx_set_query_chunk_bytes" in msg
    with pytest.raises(grlx.capi.GrlxError) as ei:
        r.evaluate_sampled_trajectory(states, 0)
    assert "max_steps = 0" in str(ei.value)
    r.close()


# ---- 9: refusals ----------------------------------------------------------------------------------------------------------------------
def raw(grlx, r, states, first=0, count=N, max_steps=0, n_starts=None, null_states=False, sampler=1, epsilon=0.1, streams=None, trajectory=False):
    """either entry point on outputs filled with a pattern: (status, message, outputs untouched?)"""
    states = np.ascontiguousarray(states, np.float64)
    n = states.shape[0] if n_starts is None else n_starts
    rows, S = max(count, 1) * max(n, 1), states.shape[1]
    f64 = [np.full(rows, 777.0) for _ in range(2)] + [np.full(rows * S, 777.0)]
    i32 = [np.full(rows, 777, np.int32) for _ in range(4)]
    u64 = [np.full(rows * 2, 777, np.uint64)]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    args = [r._ctx, first, count, None if null_states else P(states, C.c_double), n, max_steps, sampler, epsilon,
            None if streams is None else P(streams, C.c_uint64), P(f64[0], C.c_double), P(f64[1], C.c_double), P(i32[0], C.c_int32),
            P(i32[1], C.c_int32), P(i32[2], C.c_int32), P(i32[3], C.c_int32), P(f64[2], C.c_double), P(u64[0], C.c_uint64)]
    if trajectory:
        f64.append(np.full(rows * max(max_steps, 1) * 32, 777.0))
        rc = r.lib.grlx_evaluate_sampled_trajectory(*args, P(f64[3], C.c_double))
    else:
        rc = r.lib.grlx_evaluate_sampled(*args)
    return rc, r.lib.grlx_last_error().decode(), all((a == 777).all() for a in f64 + i32 + u64)


def refused(grlx, r, word, states, **kw):
    for trajectory in (False, True):
        who = "grlx_evaluate_sampled_trajectory" if trajectory else "grlx_evaluate_sampled"
        k = dict(kw)
        if trajectory and "max_steps" not in k:
            k["max_steps"] = 7
        rc, msg, untouched = raw(grlx, r, states, trajectory=trajectory, **k)
        assert rc == grlx.capi.ERR_INVALID and word in msg and who in msg, (rc, msg)
        assert untouched, "a refused call wrote to its outputs"


def test_refusals(grlx):
    cfg, spec = build(grlx, "pendulum_sarsa", N)
    states = five_states("pendulum_sarsa", spec)
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
    # the sampler, epsilon, the streams
    refused(grlx, r, "unknown sampler 2", states, sampler=2)
    refused(grlx, r, "unknown sampler -1", states, sampler=-1)
    for eps in (np.nan, np.inf, -np.inf):
        refused(grlx, r, "epsilon is not finite", states, epsilon=eps)
        refused(grlx, r, "epsilon is not finite", states, epsilon=eps, sampler=0)         # ignored by the greedy sampler, still checked
    for eps in (-0.5, 1.0000001, -1.0000001, -2.0):
        refused(grlx, r, "outside [0, 1]", states, epsilon=eps)
    streams = grlx.episode_streams(STREAM_SEED, N, len(states))
    bad = streams.copy(); bad[1, 2, 1] = 1 << 48
    refused(grlx, r, "stream row 7 (replica 1, start state 2), word 1", states, streams=bad)
    bad = streams.copy(); bad[2, 4, 0] = (1 << 64) - 1
    refused(grlx, r, "stream row 14 (replica 2, start state 4), word 0", states, streams=bad)
    rc, msg, untouched = raw(grlx, r, states, trajectory=True, max_steps=0)
    assert rc == grlx.capi.ERR_INVALID and "max_steps = 0" in msg and untouched
    with pytest.raises(ValueError):
        r.evaluate_sampled(states, streams=streams[:, :3])
    # nothing to do is no error, and nothing is written; the ends of epsilon's range, GRLX_EPSILON_OWN and the largest stream word are accepted
    for trajectory in (False, True):
        assert raw(grlx, r, states, n_starts=0, max_steps=7, trajectory=trajectory)[::2] == (0, True)
        assert raw(grlx, r, states, first=1, count=0, max_steps=7, trajectory=trajectory)[::2] == (0, True)
    ok = streams.copy(); ok[0, 0, 0] = (1 << 48) - 1
    for eps in (0.0, 1.0, -1.0):
        assert raw(grlx, r, states, epsilon=eps, streams=ok, max_steps=7)[0] == 0
    r.close()

    safe, _ = build(grlx, "pendulum_sarsa", N)
    safe.projector.safe = 1
    r = grlx.Runner(safe, [1, 2, 3])
    refused(grlx, r, "safe", states)
    refused(grlx, r, "not built", states)
    r.close()

    ext, _ = build(grlx, "pendulum_sarsa", N)
    ext.env = grlx.capi.ENV_EXTERNAL
    ext.control_step, ext.timeout, ext.integration_steps = 0.0, 0.0, 0
    r = grlx.Runner(ext, [1, 2, 3])
    refused(grlx, r, "no environment", states)
    r.close()

    ac, ac_spec = build(grlx, "ac_twin", N)
    ac_states = start_states("ac_twin", ac_spec)[PICK]
    r = grlx.Runner(ac, [1, 2, 3])
    refused(grlx, r, "not built", ac_states)
    refused(grlx, r, "actor-critic", ac_states)
    assert r.lib.grlx_sampled_trajectory_record_words(r._ctx) == grlx.capi.ERR_INVALID
    r.close()


# ---- 10: grlxd -E -e ------------------------------------------------------------------------------------------------------------------
def test_grlxd_sampled_evaluation_of_a_sweep(grlx, tmp_path):
    """golden pendulum yaml, -p over two epsilons x -r 2, -t 220 (a sweep wants 20 test rows), -E -e 0.05 -T 12: <output>-0-sampled.txt against Runner.evaluate_sampled on an
    identical context with episode_streams(seed, ...) and the host's sums (ascending clones, two passes), number for number; the
    sampled-trajectories file against the records; the returns file byte for byte that of the run without -e"""
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")
    states = np.array([[np.pi, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.0, 2.0, 1.5], [7.9, -11.25, 2.9], [0.5, 30.0, 3.5]])
    (tmp_path / "states.txt").write_text("# angle velocity time\n" + "\n".join(" ".join(repr(float(v)) for v in s) for s in states) + "\n")
    epsilons = [0.05, 0.5]
    base = [grlxd, "-s", "5", "-r", "2", "-t", "220", "-q", "-p", "/experiment/agent/policy/sampler/epsilon=0.05,0.5", "-E", "states.txt"]
    (tmp_path / "plain").mkdir(); (tmp_path / "with_e").mkdir()
    for d, extra in (("plain", []), ("with_e", ["-e", "0.05", "-T", "12"])):
        cmd = base[:-1] + [os.path.join("..", "states.txt")] + extra + [yaml]
        res = subprocess.run(cmd, cwd=tmp_path / d, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr + res.stdout
    name = "pendulum-sarsa-tc-0-"
    assert (tmp_path / "with_e" / (name + "returns.txt")).read_bytes() == (tmp_path / "plain" / (name + "returns.txt")).read_bytes()
    assert not (tmp_path / "plain" / (name + "sampled.txt")).exists()

    cfg = grlx.pendulum_sarsa_config(4, max_rows=32)
    r = grlx.Runner(cfg, [5, 6, 7, 8])
    r.set_replica_params(epsilon=[epsilons[0]] * 2 + [epsilons[1]] * 2)
    r.run(220); r.sync()
    streams = grlx.episode_streams(5, 4, len(states))
    got = r.evaluate_sampled(states, "epsilon", 0.05, streams)
    traj = r.evaluate_sampled_trajectory(states, 12, "epsilon", 0.05, streams)
    r.close()
    lines = [ln.split() for ln in (tmp_path / "with_e" / (name + "sampled.txt")).read_text().split("\n") if ln.strip()]
    assert len(lines) == 2 * states.shape[0]
    for g in range(2):
        for s in range(states.shape[0]):
            f = lines[g * states.shape[0] + s]
            assert len(f) == 10 and int(f[0]) == g, f
            ks = (2 * g, 2 * g + 1)
            total = steps = 0.0
            for k in ks:
                total += float(got.ret[k, s]); steps += float(got.steps[k, s])
            mean, sq = total / 2, 0.0
            for k in ks:
                sq += (float(got.ret[k, s]) - mean) * (float(got.ret[k, s]) - mean)
            assert [float(f[1]), float(f[2]), float(f[3])] == [mean, float(np.sqrt(sq / 1)), steps / 2], f"point {g}, start state {s}: {f}"
            assert [int(x) for x in f[4:8]] == [int((got.terminal[list(ks), s] == c).sum()) for c in range(4)], f"point {g}, start state {s}: codes"
            assert int(f[8]) == int(got.ties[list(ks), s].sum()) and int(f[9]) == int(got.explored[list(ks), s].sum()), f"point {g}, start state {s}"
    assert got.explored.sum() > 0
    R = traj.records.shape[-1]
    tl = [ln.split() for ln in (tmp_path / "with_e" / (name + "sampled-trajectories.txt")).read_text().split("\n") if ln.strip()]
    assert len(tl) == int(traj.steps.sum())
    at = 0
    for k in range(4):
        for s in range(states.shape[0]):
            for t in range(int(traj.steps[k, s])):
                f = tl[at]; at += 1
                assert [int(x) for x in f[:3]] == [k, s, t] and len(f) == 3 + R
                assert [float(x) for x in f[3:]] == [float(v) for v in traj.records[k, s, t]], f"clone {k}, start {s}, step {t}"
