"""Per-step trajectories of the greedy evaluation episodes (grlx_evaluate_trajectory, grlx_evaluate_ensemble_trajectory and their Runner
methods) against tests/policy_trajectory_ref.py -- the episode references' loop keeping every step --, against the siblings' sums on the
same context and against the queries.  Every comparison is on the bit patterns.  A trajectory call must change nothing in the context.

Shapes: those of test_gpu_policy_evaluate.py -- 3 replicas (actor-critic 5) x 7 start states, never a multiple of 4 pairs, 6 trials of
training, max_steps 40 at most.  Record widths: pendulum 11, acrobot and cart-pole 15, walker 22 (two stores per step); ensemble 13, 17
(two stores), 24; the ensemble's round loop beyond its first round on 64 replicas in groups of 17, 33, 64 and 32.  The oracle's half is computed once per case (every GPU test runs clean and with poisoned registers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_ensemble_ref as ens
from tests import policy_evaluate_ref as ev
from tests import policy_query_ref as ref
from tests import policy_trajectory_ref as tr
from tests.test_gpu_policy_evaluate import AC_GRAPHS, Q_GRAPHS, domain_exit_states, max_steps_of, start_states
from tests.test_gpu_policy_query import SEED0, build, same_bits

pytestmark = pytest.mark.gpu

RULES = (("vote", ens.VOTE), ("mean", ens.MEAN_Q))
_ref_cache = {}


def oracle_stages(key, specs, seeds, states, stages, max_steps):
    """[stage][replica] -> policy_trajectory_ref.evaluate's dict; stage s is taken after sum(stages[:s + 1]) trials"""
    if key not in _ref_cache:
        exps = [ob.Experiment(s, seed=int(seed)) for s, seed in zip(specs, seeds)]
        out = []
        for trials in stages:
            for e in exps:
                if trials:
                    e.run(trials)
            out.append([tr.evaluate(ev.tables_of(e), s, states, max_steps) for e, s in zip(exps, specs)])
        for e in exps:
            e.close()
        _ref_cache[key] = out
    return _ref_cache[key]


def check_trajectory(got, want, what, fields=tr.FIELDS):
    """every output against want[replica or group], all at once"""
    for f in fields:
        same_bits(getattr(got, f), np.stack([w[f] for w in want]), f"{what}: {f}")


def check_shape_of_the_records(got, what):
    """zeros behind every episode's end, the last record's state is the final state, its code the episode's, the rewards add up to ret"""
    records, steps = got.records, got.steps
    T = records.shape[2]
    behind = np.arange(T)[None, None, :] >= steps[:, :, None]
    assert not records.view(np.uint64)[behind].any(), f"{what}: a record behind an episode's end is not all-zero bits"
    assert (steps >= 1).all()
    k, s = np.indices(steps.shape)
    same_bits(got.state[k, s, steps - 1], got.final_state, f"{what}: the last record's state")
    same_bits(got.code[k, s, steps - 1], got.terminal, f"{what}: the last record's code")
    ret = np.zeros(steps.shape)
    for t in range(T):                                          # in step order; +0.0 behind the end changes nothing
        ret = np.where(t < steps, ret + got.reward[:, :, t], ret)
    same_bits(ret, got.ret, f"{what}: the reward column added up")


def run_against_oracle(grlx, graph, n, stages, specs=None, prepare=None, key=None, **cfg_only):
    cfg, spec = build(grlx, graph, n, **cfg_only)
    seeds = np.arange(SEED0, SEED0 + n)
    specs = [spec] * n if specs is None else specs(spec)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    want = oracle_stages(key or (graph, n, tuple(stages)), specs, seeds, states, stages, ms)
    r = grlx.Runner(cfg, seeds)
    if prepare:
        prepare(r)
    got = None
    for s, trials in enumerate(stages):
        if trials:
            r.run(trials); r.sync()
        what = f"{graph} after {sum(stages[:s + 1])} trials"
        got = r.evaluate_trajectory(states, ms)
        assert got.records.shape == (n, states.shape[0], ms, tr.record_words(spec)) == (n, 7, ms, r.trajectory_record_words())
        check_trajectory(got, want[s], what)
        check_shape_of_the_records(got, what)
        sums = r.evaluate(states, max_steps=ms)
        for f in ev.FIELDS:
            same_bits(getattr(got, f), getattr(sums, f), f"{what}: {f} against Runner.evaluate")
    return r, spec, states, want, got


# ---- 1: every family against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", Q_GRAPHS + AC_GRAPHS)
def test_families_against_the_reference(grlx, graph):
    """before any launch and after 6 trials: records and sums against the reference, the sums against Runner.evaluate.  Some pair must end
    at step 1 or 2 and some must run to max_steps, or the zero fill and the last index go unchecked."""
    n = 5 if graph in AC_GRAPHS else 3
    r, spec, states, want, got = run_against_oracle(grlx, graph, n, (0, 6))
    steps = np.stack([w["steps"] for w in want[-1]])
    assert (steps <= 2).any() and steps.max() == max_steps_of(graph), f"{graph}: steps {sorted(set(steps.ravel().tolist()))}"
    if graph in AC_GRAPHS:
        assert (got.action_index == np.where(np.arange(got.records.shape[2]) < got.steps[:, :, None], -1.0, 0.0)).all()
    # a replica range of its own, the records alone
    rec = np.zeros((1,) + got.records.shape[1:])
    states_c = np.ascontiguousarray(states)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert r.lib.grlx_evaluate_trajectory(r._ctx, 1, 1, P(states_c), states.shape[0], max_steps_of(graph), None, None, None, None, None, None, P(rec)) == 0
    same_bits(rec[0], want[-1][1]["records"], "replica range, every other output null: records")
    r.close()


# ---- 2: the value word is the queries' value -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum_sarsa", "qv", "ac_twin"])
def test_the_value_word_is_the_queries_value(grlx, graph):
    n, k = 3, 1
    cfg, spec = build(grlx, graph, n)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    got = r.evaluate_trajectory(states, ms, replicas=range(k, k + 1))
    rows = [got.episode(0, s) for s in range(states.shape[0])]
    taken = np.concatenate(rows)
    obs = np.concatenate([got.obs[0, s, :got.steps[0, s]] for s in range(states.shape[0])])
    assert taken.shape[0] == int(got.steps.sum()) == obs.shape[0]
    if graph in AC_GRAPHS:
        same_bits(r.query_state(obs, 1, replicas=range(k, k + 1))[0], taken[:, tr.VALUE], "the actor's read at the recorded observations")
        clipped = np.minimum(np.maximum(taken[:, tr.VALUE], spec.action_min), spec.action_max)
        same_bits(clipped, taken[:, tr.ACTION], "the action is the clipped read")
    else:
        _, value, greedy, n_max = r.query_q(obs, replicas=range(k, k + 1))
        same_bits(value[0], taken[:, tr.VALUE], "query_q's value at the recorded observations")
        same_bits(greedy[0], taken[:, tr.ACTION_INDEX].astype(np.int32), "query_q's greedy")
        same_bits(n_max[0], taken[:, tr.N_MAX].astype(np.int32), "query_q's n_max")
        same_bits(np.array(ref.actions_of(spec))[greedy[0]], taken[:, tr.ACTION], "the action is the discretizer's")
    r.close()


# ---- 3: the ensemble -----------------------------------------------------------------------------------------------------------------
def oracle_groups(key, spec, seeds, states, trials, max_steps, groups):
    """[rule name] -> list over groups of policy_trajectory_ref.evaluate_ensemble's dict, after `trials` trials"""
    if key not in _ref_cache:
        exps = [ob.Experiment(spec, seed=int(seed)) for seed in seeds]
        for e in exps:
            e.run(trials)
        tables = [ref.dense(e, 0) for e in exps]
        _ref_cache[key] = {name: [tr.evaluate_ensemble([tables[m] for m in g], spec, states, rule, max_steps) for g in groups] for name, rule in RULES}
        for e in exps:
            e.close()
    return _ref_cache[key]


@pytest.mark.parametrize("graph", ["pendulum_sarsa", "acrobot_q", "walker_q"])
def test_ensemble_against_the_reference(grlx, graph):
    """6 replicas in two groups of 3, both rules, after 6 trials; record widths 13, 17 (the second store) and 24"""
    n, G = 6, 3
    cfg, spec = build(grlx, graph, n)
    seeds = np.arange(SEED0, SEED0 + n)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    want = oracle_groups((graph, n, G), spec, seeds, states, 6, ms, [[0, 1, 2], [3, 4, 5]])
    r = grlx.Runner(cfg, seeds)
    r.run(6); r.sync()
    for name, _ in RULES:
        what = f"{graph}, {name}"
        got = r.evaluate_ensemble_trajectory(states, G, ms, name)
        assert got.records.shape == (2, 7, ms, tr.record_words(spec, True)) == (2, 7, ms, r.trajectory_record_words(True))
        check_trajectory(got, want[name], what, tr.ENSEMBLE_FIELDS)
        check_shape_of_the_records(got, what)
        sums = r.evaluate_ensemble(states, G, name, max_steps=ms)
        for f in ens.FIELDS:
            same_bits(getattr(got, f), getattr(sums, f), f"{what}: {f} against Runner.evaluate_ensemble")
        same_bits(got.step_agreement.sum(axis=2).astype(np.int64), got.agreement, f"{what}: the agreement column summed")
        same_bits(got.step_member_ties.sum(axis=2).astype(np.int64), got.member_ties, f"{what}: the member_ties column summed")
    steps = np.stack([w["steps"] for w in want["vote"]])
    assert (steps <= 2).any() and steps.max() == ms
    r.close()


ROUNDS = [(17, 17), (33, 33), (64, 64), (64, 32)]              # (replicas, group size): 2, 3 and 4 rounds of 16 members, two groups of 2 rounds


def many_members(grlx, graph, n, trials, groups, max_steps):
    """(configuration, seeds, start states, [rule name] -> list over groups of the reference's dict, does a member of a round after the
    first tie?) of one context of n replicas on a 32768-slot memory, which lets the oracle hold a dense vector per member"""
    if ("rounds", graph) not in _ref_cache:
        cfg, spec = build(grlx, graph, n)
        states = start_states(graph, spec)[1:3]
        for obj in (cfg, spec):
            obj.projector.memory = 32768
        seeds = np.arange(SEED0, SEED0 + n)
        exps = [ob.Experiment(spec, seed=int(seed)) for seed in seeds]
        for e in exps:
            if trials:
                e.run(trials)
        tables = [ref.dense(e, 0) for e in exps]
        want = {name: [tr.evaluate_ensemble([tables[m] for m in g], spec, states, rule, max_steps) for g in groups] for name, rule in RULES}
        D = tr.dims(spec)[0]
        later = False                                           # step_member_ties > 0 with a tied member of index >= 16 in its group
        for g, w in zip(groups, want["vote"]):
            for rec in w["records"].reshape(-1, w["records"].shape[-1]):
                if rec[tr.ENS_MEMBER_TIES] > 0 and not later:
                    later = any(int(ref.query_q(tables[m], spec, [rec[tr.ENS_OBS:tr.ENS_OBS + D]])[3][0]) > 1 for m in g[16:])
        for e in exps:
            e.close()
        _ref_cache[("rounds", graph)] = (cfg, seeds, states, want, later)
    return _ref_cache[("rounds", graph)]


@pytest.mark.parametrize("graph,trials", [("pendulum_sarsa", 6), ("pendulum_q_five_actions", 6), ("ties", 0)])
def test_ensemble_of_more_than_one_round(grlx, graph, trials):
    """64 replicas on a 32768-slot memory, 2 start states, 12 steps, both rules: one group each of 17, 33 and 64 members and two groups of
    32 -- the kernel's round loop beyond its first round: the members' double buffer, the partial last round, and the step's member ties
    counted across the rounds.  Asserted on the reference alone: the learned members disagree, their vote ties, the two rules part.  The
    learned tables give no member of a later round that ties (their weights are drawn, no two Q-values agree), so that precondition is
    the `ties` graph's, before any launch: init_min = init_max = 0, every member ties at every step."""
    n, ms = 64, 12
    groups = [list(range(g * G, (g + 1) * G)) for count, G in ROUNDS for g in range(count // G)]
    cfg, seeds, states, want, later = many_members(grlx, graph, n, trials, groups, ms)
    sizes = np.array([len(g) for g in groups], np.float64)[:, None, None]
    agreement = np.stack([w["records"][..., tr.ENS_AGREEMENT] for w in want["vote"]])
    steps = np.stack([w["steps"] for w in want["vote"]])
    live = np.arange(ms)[None, None, :] < steps[:, :, None]
    assert steps.max() == ms
    if graph == "ties":
        member_ties = np.stack([w["records"][..., tr.ENS_MEMBER_TIES] for w in want["vote"]])
        assert later and (member_ties == sizes)[live].all(), "ties: every member was meant to tie at every step"
    else:
        assert (agreement < sizes)[live].any(), f"{graph}: the members never disagree"
        assert any((w["ties"] > 0).any() for w in want["vote"]), f"{graph}: the vote never ties"
        assert any(v["records"].tobytes() != m["records"].tobytes() for v, m in zip(want["vote"], want["mean"])), f"{graph}: the two rules never part"
    r = grlx.Runner(cfg, seeds)
    if trials:
        r.run(trials); r.sync()
    at = 0
    for count, G in ROUNDS:
        for name, _ in RULES:
            what = f"{graph}: {count} replicas in groups of {G}, {name}"
            got = r.evaluate_ensemble_trajectory(states, G, ms, name, replicas=range(count))
            check_trajectory(got, want[name][at:at + count // G], what, tr.ENSEMBLE_FIELDS)
            check_shape_of_the_records(got, what)
            same_bits(got.step_agreement.sum(axis=2).astype(np.int64), got.agreement, f"{what}: the agreement column summed")
            same_bits(got.step_member_ties.sum(axis=2).astype(np.int64), got.member_ties, f"{what}: the member_ties column summed")
        at += count // G
    r.close()


def test_a_group_of_one_is_the_single_policys_trajectory(grlx):
    graph, n = "pendulum_sarsa", 3
    cfg, spec = build(grlx, graph, n)
    states, ms = start_states(graph, spec), 40
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    single = r.evaluate_trajectory(states, ms)
    for name, rule in RULES:
        got = r.evaluate_ensemble_trajectory(states, 1, ms, name)
        for view in ("action", "reward", "action_index", "code", "obs", "state"):
            same_bits(getattr(got, view), getattr(single, view), f"{name}: {view}")
        same_bits(got.step_member_ties, (single.n_max > 1).astype(np.float64), f"{name}: member_ties per step")
        same_bits(got.step_agreement, (np.arange(ms) < single.steps[:, :, None]).astype(np.float64), f"{name}: one member always agrees")
        if rule == ens.MEAN_Q:                                  # 0.0 + q: q but for the sign of a zero
            assert (got.value == single.value).all() and (got.n_max == single.n_max).all()
        else:
            same_bits(got.value, got.step_agreement, "vote: the score is the vote")
    r.close()


# ---- 4: code 3, ties -------------------------------------------------------------------------------------------------------------------
def test_a_domain_exit_is_a_one_step_episode_whose_record_carries_code_3(grlx):
    graph, n = "walker_q", 3
    cfg, spec = build(grlx, graph, n)
    states = domain_exit_states(spec)
    seeds = np.arange(SEED0, SEED0 + n)
    want = oracle_stages(("domain", n), [spec] * n, seeds, states, (0,), 5)[0]
    assert all(list(w["steps"]) == [1, 5, 1] and list(w["records"][:, 0, tr.TERMINAL]) == [3.0, 0.0, 3.0] for w in want)
    r = grlx.Runner(cfg, seeds)
    got = r.evaluate_trajectory(states, 5)
    check_trajectory(got, want, "domain exit")
    check_shape_of_the_records(got, "domain exit")
    assert (got.code[:, 0, 0] == 3).all() and (got.code[:, 2, 0] == 3).all() and not got.records[:, 0, 1:].any()
    r.sync()
    r.close()


def test_ties_record_the_first_action_and_every_maximum(grlx):
    """init_min = init_max = 0 on a fresh context: every step is an NA-way tie, the first action acts, Q = 0; no stream is drawn from"""
    cfg, spec = build(grlx, "ties", 3)
    states = start_states("ties", spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + 3))
    rng_before = [list(r.rng(k)) for k in range(3)]
    got = r.evaluate_trajectory(states, 40)
    ens_got = r.evaluate_ensemble_trajectory(states, 3, 40, "vote")
    taken = np.arange(40)[None, None, :] < got.steps[:, :, None]
    NA = int(spec.action_steps)
    assert (got.n_max[taken] == NA).all() and (got.action_index[taken] == 0).all() and (got.action[taken] == spec.action_min).all()
    assert not got.value[taken].any() and (got.ties == got.steps).all()
    check_shape_of_the_records(got, "ties")
    assert (ens_got.step_member_ties[0][taken[0]] == 3).all() and (ens_got.action[0][taken[0]] == spec.action_min).all()
    assert [list(r.rng(k)) for k in range(3)] == rng_before, "a tie must not draw from any stream"
    r.close()


# ---- 5: a trajectory call changes nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,tables,n_rng", [("pendulum_sarsa", 1, 3), ("ac_twin", 2, 2)])
def test_a_trajectory_call_changes_nothing(grlx, graph, tables, n_rng):
    """snapshot bytes, table_load, streams and environment states before and after both calls; then 6 more trials: rows, streams, environment
    state and sampled weights equal the oracle's uninterrupted run"""
    from tests.test_gpu_sweep import check_replica, oracle_run
    n = 3
    cfg, spec = build(grlx, graph, n)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    seeds = np.arange(SEED0, SEED0 + n)
    r = grlx.Runner(cfg, seeds)
    r.evaluate_trajectory(states, ms)                           # allowed before the first launch, and no launch itself
    if graph == "pendulum_sarsa":
        r.set_replica_params(alpha=[cfg.alpha] * n)
    r.run(6); r.sync()

    def look():
        return (r.snapshot(), [[r.table_load(k, t) for t in range(tables)] for k in range(n)], [list(r.rng(k)) for k in range(n)],
                [r.env_state(k).tobytes() for k in range(n)])

    before = look()
    r.evaluate_trajectory(states, ms)
    r.evaluate_trajectory(states[:3], 7, replicas=range(1, 3))
    if graph == "pendulum_sarsa":
        r.evaluate_ensemble_trajectory(states, 3, ms, "vote")
        r.evaluate_ensemble_trajectory(states, 1, ms, "mean")
    after = look()
    assert after[0] == before[0], "a trajectory call changed the context's snapshot"
    assert after[1:] == before[1:], "a trajectory call changed table occupancy, a stream or an environment state"
    r.run(6); r.sync()
    for k in range(n):
        want = oracle_run(spec, seeds[k], (("run", 6), ("run", 6)), cfg.projector.memory, tables=tuple(range(tables)))
        check_replica(r, k, want, f"{graph}: replica {k} after trajectory calls in between", cfg.projector.memory, n_rng=n_rng)
    r.close()


# ---- 6: layouts and staging ----------------------------------------------------------------------------------------------------------
def test_eight_replicas_per_wave_thirteen_replicas(grlx):
    r = run_against_oracle(grlx, "pendulum_sarsa", 13, (6,), replicas_per_wave=8)[0]
    assert r.replicas_per_wave() == 8
    r.close()


def test_tables_that_have_grown(grlx):
    graph, n = "pendulum_sarsa", 3
    cfg, spec = build(grlx, graph, n, table_log2_capacity=13)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    want = oracle_stages((graph, n, (12,)), [spec] * n, seeds, states, (12,), 40)
    r = grlx.Runner(cfg, seeds)
    assert r.table_capacity() == 13
    for c in (1, 1, 2, 2, 3, 3):
        r.run(c); r.sync()
    assert r.table_capacity() > 13, "the tables were meant to grow"
    check_trajectory(r.evaluate_trajectory(states, 40), want[0], "grown tables after 12 trials")
    r.close()


def test_a_sweep_context_changes_disc_and_nothing_in_the_records(grlx):
    """four gammas on one seed's training would part the tables; before any launch the tables are the same, so: four discounted returns,
    and records that do not know gamma -- equal to those of a context that shares one gamma"""
    n, gammas = 4, [0.8, 0.9, 0.95, 0.97]
    graph = "pendulum_sarsa"
    cfg, spec = build(grlx, graph, n)
    states = start_states(graph, spec)
    seeds = [SEED0] * n
    r = grlx.Runner(cfg, seeds)
    shared = r.evaluate_trajectory(states, 40)
    r.close()
    r = grlx.Runner(cfg, seeds)
    r.set_replica_params(gamma=gammas)
    swept = r.evaluate_trajectory(states, 40)
    r.close()
    same_bits(swept.records, shared.records, "gamma does not enter a record")
    for f in ("ret", "steps", "terminal", "ties", "final_state"):
        same_bits(getattr(swept, f), getattr(shared, f), f)
    assert len(set(swept.disc[:, 0].tolist())) == n, "four gammas were meant to give four discounted returns from one start state"
    want = np.zeros(states.shape[0])                            # disc by hand from the recorded rewards, replica 1's gamma
    g = np.ones(states.shape[0])
    for t in range(40):
        live = t < swept.steps[1]
        want = np.where(live, want + g * swept.reward[1, :, t], want)
        g = g * gammas[1]
    same_bits(swept.disc[1], want, "disc from the recorded rewards and the replica's own gamma")
    same_bits(swept.disc[3], shared.disc[3], "0.97 is the configuration's gamma")


@pytest.mark.parametrize("graph", ["pendulum_q_five_actions", "ac_twin"])
def test_chunked_staging_gives_the_same_bytes(grlx, graph):
    """a bound that holds exactly one start state's column (7 chunks) and one that holds two"""
    n = 5
    cfg, spec = build(grlx, graph, n)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    S, R = states.shape[1], tr.record_words(spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    lib = grlx.capi.load()
    whole = r.evaluate_trajectory(states, ms)
    assert len(set(whole.steps.ravel().tolist())) > 1
    try:
        per_start = 8 * S + n * (2 * 8 + 3 * 4 + 8 * S) + n * ms * R * 8
        for bound in (per_start, 2 * per_start + 7):
            assert lib.grlx_set_query_chunk_bytes(bound) == 0
            got = r.evaluate_trajectory(states, ms)
            for f in tr.FIELDS:
                same_bits(getattr(got, f), getattr(whole, f), f"{f} with staging bounded to {bound} bytes")
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    r.close()


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------
SENTINEL = 777


def raw_call(r, states, first, count, max_steps, ensemble=None, n_starts=None, null_states=False, null_records=False):
    """the C entry point on outputs filled with a pattern: (status, message, outputs untouched?); ensemble = (group_size, rule) or None"""
    states = np.ascontiguousarray(states, np.float64)
    n = states.shape[0] if n_starts is None else n_starts
    rows, S = max(count, 1) * max(n, 1), states.shape[1]
    f64 = [np.full(rows, float(SENTINEL)) for _ in range(2)] + [np.full(rows * S, float(SENTINEL)), np.full(rows * max(min(max_steps, 40), 1) * 24, float(SENTINEL))]       # (a call with more steps than 40 is a refused one here)
    i32 = [np.full(rows, SENTINEL, np.int32) for _ in range(3)]
    i64 = [np.full(rows, SENTINEL, np.int64) for _ in range(2)]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    st = None if null_states else P(states, C.c_double)
    rec = None if null_records else P(f64[3], C.c_double)
    if ensemble is None:
        rc = r.lib.grlx_evaluate_trajectory(r._ctx, first, count, st, n, max_steps, P(f64[0], C.c_double), P(f64[1], C.c_double), P(i32[0], C.c_int32),
                                            P(i32[1], C.c_int32), P(i32[2], C.c_int32), P(f64[2], C.c_double), rec)
    else:
        rc = r.lib.grlx_evaluate_ensemble_trajectory(r._ctx, first, count, ensemble[0], ensemble[1], st, n, max_steps, P(f64[0], C.c_double),
                                                     P(f64[1], C.c_double), P(i32[0], C.c_int32), P(i32[1], C.c_int32), P(i32[2], C.c_int32),
                                                     P(i64[0], C.c_int64), P(i64[1], C.c_int64), P(f64[2], C.c_double), rec)
    return rc, r.lib.grlx_last_error().decode(), all((a == SENTINEL).all() for a in f64 + i32 + i64)


def refused(grlx, r, word, states, first=0, count=3, max_steps=5, **kw):
    rc, msg, untouched = raw_call(r, states, first, count, max_steps, **kw)
    assert rc == grlx.capi.ERR_INVALID and word in msg, (rc, msg)
    assert untouched, "a refused trajectory call wrote to its outputs"


def test_refusals(grlx):
    cfg, spec = build(grlx, "pendulum_sarsa", 3)
    states = start_states("pendulum_sarsa", spec)
    r = grlx.Runner(cfg, [1, 2, 3])
    lib = grlx.capi.load()
    for e in (None, (3, 0)):
        who = "grlx_evaluate_trajectory" if e is None else "grlx_evaluate_ensemble_trajectory"
        sibling = "grlx_evaluate" if e is None else "grlx_evaluate_ensemble"
        # what the sibling refuses
        refused(grlx, r, "states is null", states, null_states=True, ensemble=e)
        refused(grlx, r, "n_starts = -1", states, n_starts=-1, ensemble=e)
        refused(grlx, r, "replica range", states, first=2, count=3, ensemble=e)
        refused(grlx, r, "replica range", states, first=-1, count=3, ensemble=e)
        refused(grlx, r, "max_steps = -1", states, max_steps=-1, ensemble=e)
        refused(grlx, r, "max_steps = 100001", states, max_steps=100001, ensemble=e)
        bad = states.copy(); bad[2, 1] = np.nan
        refused(grlx, r, "row 2, component 1 is not finite", bad, ensemble=e)
        bad[2, 1] = 0.0; bad[6, 2] = 131072.0
        refused(grlx, r, "row 6, component 2", bad, ensemble=e)
        refused(grlx, r, "2^17", bad, ensemble=e)
        # its own
        refused(grlx, r, "records is null", states, null_records=True, ensemble=e)
        refused(grlx, r, f"call {sibling})", states, null_records=True, ensemble=e)
        refused(grlx, r, "max_steps = 0", states, max_steps=0, ensemble=e)
        refused(grlx, r, "no default", states, max_steps=0, ensemble=e)
        refused(grlx, r, who, states, max_steps=0, ensemble=e)
        rows, R = (3, 11) if e is None else (1, 13)
        column = rows * 5 * R * 8
        try:
            assert lib.grlx_set_query_chunk_bytes(column) == 0              # the records alone fit, their sums no more
            for word in (f"{column} bytes", f"bound of {column} bytes", "fewer replicas", "smaller max_steps", "grlx_set_query_chunk_bytes"):
                refused(grlx, r, word, states, ensemble=e)
            assert lib.grlx_set_query_chunk_bytes(column + 8 * 3 + rows * (2 * 8 + 3 * 4 + 2 * 8 + 8 * 3)) == 0
            assert raw_call(r, states, 0, 3, 5, ensemble=e)[0] == 0
        finally:
            lib.grlx_set_query_chunk_bytes(0)
        # nothing to do is no error, and nothing is written
        assert raw_call(r, states, 0, 3, 5, n_starts=0, ensemble=e)[::2] == (0, True)
        assert raw_call(r, states, 1, 0, 5, ensemble=e)[::2] == (0, True)
    refused(grlx, r, "group_size = 0", states, ensemble=(0, 0))
    refused(grlx, r, "does not divide", states, ensemble=(2, 0))
    refused(grlx, r, "unknown rule 2", states, ensemble=(3, 2))
    assert r.trajectory_record_words() == 11 and r.trajectory_record_words(True) == 13
    with pytest.raises(ValueError):
        r.evaluate_trajectory(states[:, :2], 5)
    with pytest.raises(grlx.capi.GrlxError):
        r.evaluate_trajectory(states, 0)
    r.close()

    safe, _ = build(grlx, "pendulum_sarsa", 3)
    safe.projector.safe = 1
    r = grlx.Runner(safe, [1, 2, 3])
    refused(grlx, r, "not built", states)
    refused(grlx, r, "safe", states, ensemble=(3, 0))
    r.close()

    ext, _ = build(grlx, "pendulum_sarsa", 3)
    ext.env = grlx.capi.ENV_EXTERNAL
    ext.control_step, ext.timeout, ext.integration_steps = 0.0, 0.0, 0
    r = grlx.Runner(ext, [1, 2, 3])
    refused(grlx, r, "no environment", states)
    assert lib.grlx_trajectory_record_words(r._ctx, 0) == grlx.capi.ERR_INVALID
    r.close()

    ac, ac_spec = build(grlx, "ac_twin", 3)
    r = grlx.Runner(ac, [1, 2, 3])
    refused(grlx, r, "actor-critic", start_states("ac_twin", ac_spec), ensemble=(3, 0))
    assert r.trajectory_record_words() == 15 and lib.grlx_trajectory_record_words(r._ctx, 1) == grlx.capi.ERR_INVALID
    r.close()


# ---- 8: grlxd -E -T ------------------------------------------------------------------------------------------------------------------
def _record_lines(path):
    return [ln.split() for ln in open(path).read().split("\n") if ln.strip()]


def _check_file(lines, got, what):
    """the file's lines, re-parsed, are the records of the steps taken, ascending; %.17g gives every double back"""
    want = [(k, s, t) for k in range(got.steps.shape[0]) for s in range(got.steps.shape[1]) for t in range(int(got.steps[k, s]))]
    assert [tuple(int(x) for x in f[:3]) for f in lines] == want, f"{what}: the lines' (row, start, step)"
    R = got.records.shape[-1]
    for f, (k, s, t) in zip(lines, want):
        assert len(f) == 3 + R, f
        for w in (tr.ACTION_INDEX, tr.N_MAX, tr.TERMINAL):
            assert "." not in f[3 + w] and "e" not in f[3 + w], f"{what}: word {w} is printed as an integer"
        same_bits(np.array([float(x) for x in f[3:]]), got.records[k, s, t], f"{what}: line {k} {s} {t}")


def test_grlxd_trajectories(grlx, tmp_path):
    """golden pendulum yaml, -r 4 -t 12 -E -T 12 -V vote: both files against the Runner's methods on a context run the same way"""
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")
    states = np.array([[np.pi, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.0, 2.0, 1.5], [7.9, -11.25, 2.9], [0.5, 30.0, 3.5]])
    (tmp_path / "states.txt").write_text("# angle velocity time\n" + "\n".join(" ".join(repr(float(v)) for v in s) for s in states) + "\n")
    res = subprocess.run([grlxd, "-s", "5", "-r", "4", "-t", "12", "-q", "-E", "states.txt", "-T", "12", "-V", "vote", yaml], cwd=tmp_path,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr + res.stdout
    cfg = grlx.pendulum_sarsa_config(4, max_rows=8)
    r = grlx.Runner(cfg, [5, 6, 7, 8])
    r.run(12); r.sync()
    single = r.evaluate_trajectory(states, 12)
    group = r.evaluate_ensemble_trajectory(states, 4, 12, "vote")
    r.close()
    assert (single.steps[:, 4] == 1).all() and single.steps.max() == 12, "a start past the timeout takes one step; the others are cut at -T"
    _check_file(_record_lines(tmp_path / "pendulum-sarsa-tc-0-trajectories.txt"), single, "trajectories")
    _check_file(_record_lines(tmp_path / "pendulum-sarsa-tc-0-ensemble-trajectories.txt"), group, "ensemble trajectories")
    assert (tmp_path / "pendulum-sarsa-tc-0-returns.txt").exists() and (tmp_path / "pendulum-sarsa-tc-0-ensemble.txt").exists()
