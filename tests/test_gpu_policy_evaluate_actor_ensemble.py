"""Episodes of an ensemble of actors (grlx_evaluate_actor_ensemble / Runner.evaluate_actor_ensemble and their trajectory call): one episode
per (group of consecutive actor-critic replicas, start state) on the members' combined action -- mapping/policy/multi's mean, binning,
data_center and density -- against tests/policy_evaluate_actor_ensemble_ref.py: a plain Python loop over the oracle's dense actor tables,
its env_step and its portable exponential.  Every comparison is on the bit patterns; there is no tolerance anywhere.  A call must change
nothing in the context.

Shapes: the siblings' -- 6 replicas in groups of 3, the 7 start states of test_gpu_policy_evaluate.py (5 where a case needs no more),
max_steps 40, 6 learning trials; one group of 17 (two probe rounds, the second partial) and one of 37 on a small memory.  The parameters
of the rules (64 bins, 2 members kept, r = 0.05) were chosen on the oracle's half so that every branch is taken, and the tests assert that
on the REFERENCE's outputs.  The oracle's half is computed once per case (every GPU test runs clean and with poisoned registers)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_actor_ensemble_ref as ae
from tests import policy_evaluate_ref as ev
from tests.test_gpu_policy_evaluate import start_states
from tests.test_gpu_policy_evaluate_noisy import make
from tests.test_gpu_policy_query import SEED0, build, same_bits

pytestmark = pytest.mark.gpu

TRIALS, MS = 6, 40
GRAPHS = ["ac_twin", "ac_independent", "pendulum_ac"]
CASES = (("mean", 10, 0.001), ("binning", 64, 0.001), ("data_center", 2, 0.001), ("density", 10, 0.05))     # (rule, bins, r)
_cache = {}


def small_memory(cfg, spec, memory=32768):
    """both projectors on a small memory: an oracle experiment holds its tables dense"""
    for obj in (cfg, spec):
        obj.projector.memory = memory
        obj.actor_projector.memory = memory


def oracle_groups(key, spec, seeds, states, stages, groups, cases, max_steps=MS):
    """[stage][case][group] -> the reference's dict, and per case what branches the reference took; stage s is taken after
    sum(stages[:s + 1]) trials (0: before any launch); groups: lists of replica indices"""
    if key not in _cache:
        exps = [ob.Experiment(spec, seed=int(seed)) for seed in seeds]
        out, seen = [], [dict() for _ in cases]
        for trials in stages:
            if trials:
                for e in exps:
                    e.run(trials)
            tabs = [ev.tables_of(e) for e in exps]
            out.append([[ae.evaluate([tabs[k] for k in g], spec, states, rule, bins, r, max_steps, seen[c]) for g in groups]
                        for c, (rule, bins, r) in enumerate(cases)])
        for e in exps:
            e.close()
        _cache[key] = (out, seen)
    return _cache[key]


def check(got, want, what, records=False):
    """the eight outputs (and the records) of all groups at once against want[group]"""
    names = {"kept": "n_kept", "spread": "total_spread"} if records else {}
    for f in ae.FIELDS:
        same_bits(getattr(got, names.get(f, f)), np.stack([w[f] for w in want]), f"{what}: {f}")
    if records:
        same_bits(got.records, np.stack([w["records"] for w in want]), f"{what}: records")


def records_add_up(t, what):
    """the records' sums, in step order, are the summary's"""
    for g in range(t.steps.shape[0]):
        for s in range(t.steps.shape[1]):
            n = int(t.steps[g, s])
            ret, spread, kept, ties = 0.0, 0.0, 0, 0
            for k in range(n):
                ret += float(t.reward[g, s, k]); spread += float(t.spread[g, s, k]); kept += int(t.kept[g, s, k]); ties += int(t.n_max[g, s, k] > 1)
            assert (ret, spread, kept, ties) == (float(t.ret[g, s]), float(t.total_spread[g, s]), int(t.n_kept[g, s]), int(t.ties[g, s])), f"{what}: pair ({g}, {s})"
            assert not t.records[g, s, n:].view(np.uint64).any(), f"{what}: pair ({g}, {s}): records behind the episode's end"
            assert n == 0 or (t.state[g, s, n - 1] == t.final_state[g, s]).all()


def branches_taken(want, seen, G, K, what):
    """asserted on the REFERENCE's outputs: a test that never leaves one bin proves nothing"""
    by = {rule: c for c, (rule, _, _) in enumerate(CASES)}
    stages = range(len(want))
    assert seen[by["binning"]]["occupied"] >= 2, f"{what}: binning never left one bin"
    assert any((want[s][by["binning"]][g]["records"][..., 0] != want[s][by["mean"]][g]["records"][..., 0]).any() for s in stages for g in range(len(want[s][0]))), \
        f"{what}: binning's actions never differ from the mean's"
    assert G > K and seen[by["data_center"]]["removals"] > 0 and seen[by["data_center"]]["not_first"] > 0, f"{what}: data_center never removed a member other than the first alive"
    assert seen[by["density"]]["not_first"] > 0, f"{what}: density never selected a member other than the group's first"
    assert any((w["ties"] < w["steps"]).any() for s in stages for w in want[s][by["density"]]), f"{what}: density tied at every step"
    assert any((w["ties"] > 0).any() for s in stages for c in (by["binning"], by["density"]) for w in want[s][c]), f"{what}: no tie anywhere"


# ---- 1, 5: every graph x every rule against the reference; the second group alone ----------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
def test_against_the_reference(grlx, graph):
    n, G = 6, 3
    cfg, spec = make(grlx, graph, n)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    want, seen = oracle_groups(("parity", graph), spec, seeds, states, (0, TRIALS), [[0, 1, 2], [3, 4, 5]], CASES)
    branches_taken(want, seen, G, 2, graph)
    r = grlx.Runner(cfg, seeds)
    assert r.actor_ensemble_trajectory_record_words() == r.trajectory_record_words() + 2 == want[0][0][0]["records"].shape[-1]
    for s, trials in enumerate((0, TRIALS)):
        if trials:
            r.run(trials); r.sync()
        for c, (rule, bins, rad) in enumerate(CASES):
            what = f"{graph} after {trials} trials, {rule}"
            check(r.evaluate_actor_ensemble(states, G, rule, bins, rad, max_steps=MS), want[s][c], what)
            t = r.evaluate_actor_ensemble_trajectory(states, G, MS, rule, bins, rad)
            check(t, want[s][c], what + ", trajectory", records=True)
            records_add_up(t, what)
            if rule == "mean":
                same_bits(t.value, t.action, what + ": the value word is the mean")
                assert (t.ties == 0).all() and (t.n_kept == G * t.steps).all()
            if rule == "density":
                assert (t.n_kept == t.steps).all()
    # the second group alone, through replicas=
    for c, (rule, bins, rad) in enumerate(CASES):
        got = r.evaluate_actor_ensemble(states, G, rule, bins, rad, replicas=range(3, 6), max_steps=MS)
        check(got, want[-1][c][1:], f"{graph}: the second group alone, {rule}")
        t = r.evaluate_actor_ensemble_trajectory(states, G, MS, rule, bins, rad, replicas=range(3, 6))
        check(t, want[-1][c][1:], f"{graph}: the second group alone, {rule}, trajectory", records=True)
    r.close()


# ---- 2: many members: two probe rounds, the second partial; three rounds ----------------------------------------------------------------
def test_many_members(grlx):
    """one context of 37 replicas on a small memory: its first 17 as one group (rounds of 16 + 1), all 37 as one group (16 + 16 + 5)"""
    graph, n = "ac_twin", 37
    cfg, spec = make(grlx, graph, n)
    small_memory(cfg, spec)
    states = start_states(graph, spec)[[0, 1, 3, 4, 6]]
    seeds = np.arange(SEED0, SEED0 + n)
    cases = (CASES[0], CASES[3])
    want, seen = oracle_groups(("many", graph), spec, seeds, states, (TRIALS,), [list(range(17)), list(range(37))], cases)
    assert seen[1]["not_first"] > 0
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    for c, (rule, bins, rad) in enumerate(cases):
        for k, count in enumerate((17, 37)):
            what = f"one group of {count}, {rule}"
            check(r.evaluate_actor_ensemble(states, count, rule, bins, rad, replicas=range(count), max_steps=MS), want[0][c][k:k + 1], what)
            check(r.evaluate_actor_ensemble_trajectory(states, count, MS, rule, bins, rad, replicas=range(count)), want[0][c][k:k + 1], what + ", trajectory",
                  records=True)
    r.close()


# ---- 3: a group of one ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["ac_twin", "pendulum_ac"])
def test_a_group_of_one_is_the_single_policy(grlx, graph):
    n = 5
    cfg, spec = make(grlx, graph, n)
    states = start_states(graph, spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(TRIALS); r.sync()
    plain, plain_t = r.evaluate(states, max_steps=MS), r.evaluate_trajectory(states, MS)
    R = plain_t.records.shape[-1]
    for rule, bins, rad in CASES:
        got, got_t = r.evaluate_actor_ensemble(states, 1, rule, bins, rad, max_steps=MS), r.evaluate_actor_ensemble_trajectory(states, 1, MS, rule, bins, rad)
        for f in ev.FIELDS:
            same_bits(getattr(got, f), getattr(plain, f), f"{graph}, {rule}, groups of one: {f} against Runner.evaluate")
            same_bits(getattr(got_t, f), getattr(plain, f), f"{graph}, {rule}, groups of one, trajectory: {f} against Runner.evaluate")
        assert (got.kept == got.steps).all() and not got.spread.view(np.uint64).any()
        for w in range(R):
            if w not in (grlx.capi.TRAJ_VALUE, grlx.capi.TRAJ_ACTION_INDEX):
                same_bits(got_t.records[..., w], plain_t.records[..., w], f"{graph}, {rule}, groups of one: word {w} of the records")
        same_bits(got_t.value, got_t.action, "the mean of one member is the member")
    r.close()


# ---- 4: a radius at which nothing is near anything ---------------------------------------------------------------------------------------
def test_density_at_a_tiny_radius_acts_as_the_first_member(grlx):
    """r = 1e-6: every rho is exactly 1.0 unless two members agree to the last bit, so every step ties and the group's first member acts.
    Before any launch: the members' initial weights are drawn, no two agree (after the trials most actions sit on the clip)."""
    graph, n, G = "ac_twin", 6, 3
    cfg, spec = make(grlx, graph, n)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    cases = (("density", 10, 1e-6),)
    want, _ = oracle_groups(("tiny", graph), spec, seeds, states, (0,), [[0, 1, 2], [3, 4, 5]], cases)
    for w in want[0][0]:                                  # the precondition, on the reference's actions
        for episode in w["actions"]:
            for a in episode:
                _, at, tied, rho = ae.density(a, 1e-6, float(spec.action_min), float(spec.action_max))
                assert rho == [1.0] * G and (at, tied) == (0, G)
        assert (w["ties"] == w["steps"]).all()
    r = grlx.Runner(cfg, seeds)
    got = r.evaluate_actor_ensemble(states, G, "density", r=1e-6, max_steps=MS)
    check(got, want[0][0], "r = 1e-6")
    assert (got.ties == got.steps).all()
    for g in range(2):
        plain = r.evaluate(states, replicas=range(3 * g, 3 * g + 1), max_steps=MS)
        for f in ("ret", "disc", "steps", "terminal", "final_state"):
            same_bits(getattr(got, f)[g], getattr(plain, f)[0], f"r = 1e-6, group {g}: {f} against Runner.evaluate of its first replica")
    r.close()


# ---- 6: chunk invariance -----------------------------------------------------------------------------------------------------------------
def test_chunked_staging_gives_the_same_bits(grlx):
    """17 start states under a bound that holds 6 of them: chunks of 6, 6 and 5"""
    graph, ms, n, G = "ac_twin", 30, 6, 3
    cfg, spec = make(grlx, graph, n)
    states = np.array([[-2.0 + 0.25 * i, 0.4 * i, 0.5 * i - 4.0, 3.0 - 0.3 * i, 8.0 + 0.1 * i] for i in range(17)], np.float64)
    S = states.shape[1]
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(TRIALS); r.sync()
    lib = grlx.capi.load()
    R = r.actor_ensemble_trajectory_record_words()
    for rule, bins, rad in CASES[1:]:
        whole = r.evaluate_actor_ensemble(states, G, rule, bins, rad, max_steps=ms)
        whole_t = r.evaluate_actor_ensemble_trajectory(states, G, ms, rule, bins, rad)
        assert len(set(whole.steps.ravel().tolist())) > 1
        try:
            per_start = 8 * S + (n // G) * (2 * 8 + 3 * 4 + 8 * S + 2 * 8)
            assert lib.grlx_set_query_chunk_bytes(6 * per_start) == 0
            got = r.evaluate_actor_ensemble(states, G, rule, bins, rad, max_steps=ms)
            assert lib.grlx_set_query_chunk_bytes(6 * (per_start + (n // G) * ms * R * 8)) == 0
            got_t = r.evaluate_actor_ensemble_trajectory(states, G, ms, rule, bins, rad)
        finally:
            lib.grlx_set_query_chunk_bytes(0)
        names = {"kept": "n_kept", "spread": "total_spread"}
        for f in ae.FIELDS:
            same_bits(getattr(got, f), getattr(whole, f), f"{rule}: {f} in three chunks")
            same_bits(getattr(got_t, names.get(f, f)), getattr(whole_t, names.get(f, f)), f"{rule}, trajectory: {f} in three chunks")
            same_bits(getattr(whole_t, names.get(f, f)), getattr(whole, f), f"{rule}, trajectory: {f} against the sibling")
        same_bits(got_t.records, whole_t.records, f"{rule}: records in three chunks")
    r.close()


# ---- 7: eight replicas per wave ------------------------------------------------------------------------------------------------------------
def test_thirteen_replicas_at_eight_per_wave(grlx):
    graph, n = "ac_twin", 13
    cfg, spec = make(grlx, graph, n)
    cfg.replicas_per_wave = 8
    small_memory(cfg, spec)
    states = start_states(graph, spec)[[0, 1, 3, 4, 6]]
    seeds = np.arange(SEED0, SEED0 + n)
    want, _ = oracle_groups(("thirteen", graph), spec, seeds, states, (TRIALS,), [list(range(13))], CASES)
    r = grlx.Runner(cfg, seeds)
    assert r.replicas_per_wave() == 8
    r.run(TRIALS); r.sync()
    for c, (rule, bins, rad) in enumerate(CASES):
        check(r.evaluate_actor_ensemble(states, n, rule, bins, rad, max_steps=MS), want[0][c], f"one group of 13, {rule}")
    r.close()


# ---- 8: tables that have grown -----------------------------------------------------------------------------------------------------------
def test_tables_that_have_grown(grlx):
    """2^13 entries at first, short launches so that the tables grow between them (positions change; the episodes do not)"""
    graph, n, G = "ac_twin", 6, 3
    cfg, spec = make(grlx, graph, n)
    cfg.table_log2_capacity = 13
    states = start_states(graph, spec)[[0, 1, 3, 4, 6]]
    seeds = np.arange(SEED0, SEED0 + n)
    want, _ = oracle_groups(("grown", graph), spec, seeds, states, (6, 6), [[0, 1, 2], [3, 4, 5]], CASES)
    r = grlx.Runner(cfg, seeds)
    assert r.table_capacity() == 13
    for c in (1, 1, 2, 2):
        r.run(c); r.sync()
    for c, (rule, bins, rad) in enumerate(CASES):
        check(r.evaluate_actor_ensemble(states, G, rule, bins, rad, max_steps=MS), want[0][c], f"grown tables after 6 trials, {rule}")
    for c in (3, 3):
        r.run(c); r.sync()
    assert r.table_capacity() > 13, "the tables were meant to grow"
    for c, (rule, bins, rad) in enumerate(CASES):
        check(r.evaluate_actor_ensemble_trajectory(states, G, MS, rule, bins, rad), want[1][c], f"grown tables after 12 trials, {rule}", records=True)
    r.close()


# ---- 9: a call changes nothing -----------------------------------------------------------------------------------------------------------
def test_an_actor_ensemble_evaluation_changes_nothing(grlx):
    from tests.test_gpu_sweep import check_replica, oracle_run
    graph, n = "ac_twin", 3
    cfg, spec = make(grlx, graph, n)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    r = grlx.Runner(cfg, seeds)

    def look():
        return (r.snapshot(), [[r.table_load(k, t) for t in range(2)] for k in range(n)], [list(r.rng(k)) for k in range(n)],
                [r.env_state(k).tobytes() for k in range(n)], r.step_counts())

    def every_call():
        for rule, bins, rad in CASES:
            r.evaluate_actor_ensemble(states, 3, rule, bins, rad, max_steps=MS)
            r.evaluate_actor_ensemble_trajectory(states[:3], 1, MS, rule, bins, rad, replicas=range(1, 3))

    before = look()
    every_call()
    assert look() == before, "an actor ensemble's evaluation before the first launch changed the context"
    r.run(TRIALS); r.sync()
    before = look()
    every_call()
    after = look()
    assert after[0] == before[0], "an actor ensemble's evaluation changed the context's snapshot"
    assert after[1:] == before[1:], "an actor ensemble's evaluation changed table occupancy, a stream, an environment state or a counter"
    r.run(TRIALS); r.sync()
    for k in range(n):
        want = oracle_run(spec, seeds[k], (("run", TRIALS), ("run", TRIALS)), cfg.projector.memory, tables=(0, 1))
        check_replica(r, k, want, f"{graph}: replica {k} after actor ensemble evaluations in between", cfg.projector.memory, n_rng=2)
    r.close()


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------------
def raw(grlx, r, states, first=0, count=4, group_size=2, rule=0, bins=10, rad=0.001, max_steps=0, n_starts=None, null_states=False, trajectory=False):
    """either entry point on outputs filled with a pattern: (status, message, outputs untouched?)"""
    states = np.ascontiguousarray(states, np.float64)
    n = states.shape[0] if n_starts is None else n_starts
    rows, S = max(count, 1) * max(n, 1), states.shape[1]
    f64 = [np.full(rows, 777.0) for _ in range(3)] + [np.full(rows * S, 777.0)]
    i32 = [np.full(rows, 777, np.int32) for _ in range(3)]
    i64 = [np.full(rows, 777, np.int64)]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    args = [r._ctx, first, count, group_size, rule, bins, rad, None if null_states else P(states, C.c_double), n, max_steps,
            P(f64[0], C.c_double), P(f64[1], C.c_double), P(i32[0], C.c_int32), P(i32[1], C.c_int32), P(i32[2], C.c_int32), P(i64[0], C.c_int64),
            P(f64[2], C.c_double), P(f64[3], C.c_double)]
    if trajectory:
        f64.append(np.full(rows * max(max_steps, 1) * 32, 777.0))
        rc = r.lib.grlx_evaluate_actor_ensemble_trajectory(*args, P(f64[4], C.c_double))
    else:
        rc = r.lib.grlx_evaluate_actor_ensemble(*args)
    return rc, r.lib.grlx_last_error().decode(), all((a == 777).all() for a in f64 + i32 + i64)


def refused(grlx, r, word, states, **kw):
    for trajectory in (False, True):
        who = "grlx_evaluate_actor_ensemble_trajectory" if trajectory else "grlx_evaluate_actor_ensemble"
        k = dict(kw)
        if trajectory and "max_steps" not in k:
            k["max_steps"] = 7
        rc, msg, untouched = raw(grlx, r, states, trajectory=trajectory, **k)
        assert rc == grlx.capi.ERR_INVALID and word in msg and who in msg, (rc, msg)
        assert untouched, "a refused call wrote to its outputs"


def test_refusals(grlx):
    E = ae
    cfg, spec = make(grlx, "ac_twin", 4)
    states = start_states("ac_twin", spec)
    r = grlx.Runner(cfg, [1, 2, 3, 4])
    # everything grlx_evaluate refuses
    refused(grlx, r, "states is null", states, null_states=True)
    refused(grlx, r, "n_starts = -1", states, n_starts=-1)
    refused(grlx, r, "replica range", states, first=2, count=4)
    refused(grlx, r, "max_steps = -1", states, max_steps=-1)
    refused(grlx, r, "max_steps = 100001", states, max_steps=100001)
    bad = states.copy(); bad[2, 1] = np.nan
    refused(grlx, r, "row 2, component 1 is not finite", bad)
    bad[2, 1] = 0.0; bad[3, 0] = -2.0 ** 17
    refused(grlx, r, "2^17", bad)
    # the groups, the rule and its parameter
    refused(grlx, r, "group_size = 0 is below 1", states, group_size=0)
    refused(grlx, r, "group_size = -2 is below 1", states, group_size=-2)
    refused(grlx, r, "group_size 3 does not divide the 4 replicas", states, group_size=3)
    for rule in (-1, 4, 99):
        refused(grlx, r, f"unknown rule {rule}", states, rule=rule)
    for bins in (0, -3, 65):
        refused(grlx, r, f"bins = {bins} is outside 1 ... 64", states, rule=E.BINNING, bins=bins)
    for bins in (0, -1):
        refused(grlx, r, f"bins = {bins}, the members kept, is below 1", states, rule=E.DATA_CENTER, bins=bins)
    for rad in (np.nan, np.inf, -np.inf):
        refused(grlx, r, "r is not finite", states, rule=E.DENSITY, rad=rad)
    for rad in (0.0, -0.001):
        refused(grlx, r, "is not above 0", states, rule=E.DENSITY, rad=rad)
    # the trajectory call's own
    rc, msg, untouched = raw(grlx, r, states, trajectory=True, max_steps=0)
    assert rc == grlx.capi.ERR_INVALID and "max_steps = 0" in msg and "grlx_evaluate_actor_ensemble_trajectory" in msg and untouched
    lib = grlx.capi.load()
    try:
        lib.grlx_set_query_chunk_bytes(1000)
        rc, msg, untouched = raw(grlx, r, states, trajectory=True, max_steps=7)
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    assert rc == grlx.capi.ERR_INVALID and "grlx_evaluate_actor_ensemble_trajectory" in msg and untouched
    assert "fewer replicas" in msg and "smaller max_steps" in msg and "grlx_set_query_chunk_bytes" in msg
    with pytest.raises(ValueError):
        r.evaluate_actor_ensemble(states, 2, rule="median")
    # nothing to do is no error, and nothing is written; parameters a rule does not read are not checked; the ends of the ranges are accepted
    for trajectory in (False, True):
        assert raw(grlx, r, states, n_starts=0, max_steps=7, trajectory=trajectory)[::2] == (0, True)
        assert raw(grlx, r, states, first=1, count=0, max_steps=7, trajectory=trajectory)[::2] == (0, True)
    assert raw(grlx, r, states, rule=E.MEAN, bins=0, rad=-1.0, max_steps=7)[0] == 0
    assert raw(grlx, r, states, rule=E.BINNING, bins=1, rad=np.nan, max_steps=7)[0] == 0
    assert raw(grlx, r, states, rule=E.BINNING, bins=64, max_steps=7)[0] == 0
    assert raw(grlx, r, states, rule=E.DATA_CENTER, bins=1000, max_steps=7)[0] == 0
    assert raw(grlx, r, states, rule=E.DENSITY, bins=0, rad=5e-324, max_steps=7)[0] == 0
    r.close()

    # a group above GRLX_ACTOR_ENSEMBLE_MAX is refused; one of exactly that size runs (two steps of one episode, before any launch)
    big, _ = make(grlx, "ac_twin", 257)
    r = grlx.Runner(big, np.arange(1, 258))
    refused(grlx, r, "group_size = 257 exceeds GRLX_ACTOR_ENSEMBLE_MAX (256)", states, count=257, group_size=257)
    for rule in (E.MEAN, E.BINNING, E.DATA_CENTER, E.DENSITY):
        assert raw(grlx, r, states[:1], count=256, group_size=256, rule=rule, bins=3, rad=0.05, max_steps=2)[0] == 0
    r.close()

    q, q_spec = build(grlx, "pendulum_sarsa", 4)
    q_states = start_states("pendulum_sarsa", q_spec)
    r = grlx.Runner(q, [1, 2, 3, 4])
    refused(grlx, r, "actor-critic only", q_states)
    refused(grlx, r, "grlx_evaluate_ensemble", q_states)
    assert r.lib.grlx_actor_ensemble_trajectory_record_words(r._ctx) == grlx.capi.ERR_INVALID
    r.close()

    # the sibling keeps its refusal of the actor-critic, and names this call
    r = grlx.Runner(cfg, [1, 2, 3, 4])
    with pytest.raises(grlx.capi.GrlxError) as ei:
        r.evaluate_ensemble(states, 2)
    assert "actor-critic" in str(ei.value) and "not built" in str(ei.value) and "grlx_evaluate_actor_ensemble" in str(ei.value)
    r.close()

    ext, _ = make(grlx, "ac_twin", 4)
    ext.env = grlx.capi.ENV_EXTERNAL
    ext.control_step, ext.timeout, ext.integration_steps = 0.0, 0.0, 0
    r = grlx.Runner(ext, [1, 2, 3, 4])
    refused(grlx, r, "no environment", states)
    r.close()


# ---- 11: grlxd -E -A -T ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arg,rule,bins,rad", [("binning:64", "binning", 64, 0.001), ("density:0.05", "density", 10, 0.05)])
def test_grlxd_actor_ensemble(grlx, tmp_path, arg, rule, bins, rad):
    """golden cart-pole actor-critic yaml, -r 4 -t 12, -E -A <rule> -T 12: <output>-0-actor-ensemble.txt against Runner.evaluate_actor_ensemble
    on an identical context with all four clones as one group, number for number; the trajectories file against the records; the returns
    file byte for byte that of the run without -A"""
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "cart_pole-ac-tc.yaml")
    states = np.array([[0.0, np.pi, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.0, 1.0], [-1.5, 0.4, 2.0, -3.0, 2.5], [2.2, 3.0, 4.0, 1.0, 9.9], [0.1, 0.2, -0.3, 0.4, 11.0]])
    (tmp_path / "states.txt").write_text("# x theta xd thetad time\n" + "\n".join(" ".join(repr(float(v)) for v in s) for s in states) + "\n")
    base = [grlxd, "-s", "5", "-r", "4", "-t", "12", "-q", "-E", os.path.join("..", "states.txt")]
    (tmp_path / "plain").mkdir(); (tmp_path / "with_a").mkdir()
    for d, extra in (("plain", []), ("with_a", ["-A", arg, "-T", "12"])):
        res = subprocess.run(base + extra + [yaml], cwd=tmp_path / d, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr + res.stdout
    name = "cart_pole-ac-tc-0-"
    assert (tmp_path / "with_a" / (name + "returns.txt")).read_bytes() == (tmp_path / "plain" / (name + "returns.txt")).read_bytes()
    assert not (tmp_path / "plain" / (name + "actor-ensemble.txt")).exists()

    cfg = grlx.cart_pole_ac_config(4, max_rows=8)
    r = grlx.Runner(cfg, [5, 6, 7, 8])
    r.run(12); r.sync()
    got = r.evaluate_actor_ensemble(states, 4, rule, bins, rad)
    traj = r.evaluate_actor_ensemble_trajectory(states, 4, 12, rule, bins, rad)
    r.close()
    lines = [ln.split() for ln in (tmp_path / "with_a" / (name + "actor-ensemble.txt")).read_text().split("\n") if ln.strip()]
    assert len(lines) == states.shape[0]
    for s, f in enumerate(lines):
        assert len(f) == 7, f
        assert [float(f[0]), float(f[1]), float(f[6])] == [float(got.ret[0, s]), float(got.disc[0, s]), float(got.spread[0, s])], f"start state {s}: {f}"
        assert [int(x) for x in f[2:6]] == [int(got.steps[0, s]), int(got.terminal[0, s]), int(got.ties[0, s]), int(got.kept[0, s])], f"start state {s}: {f}"
    assert (got.spread > 0).all()
    R = traj.records.shape[-1]
    tl = [ln.split() for ln in (tmp_path / "with_a" / (name + "actor-ensemble-trajectories.txt")).read_text().split("\n") if ln.strip()]
    assert len(tl) == int(traj.steps.sum())
    at = 0
    for s in range(states.shape[0]):
        for t in range(int(traj.steps[0, s])):
            f = tl[at]; at += 1
            assert [int(x) for x in f[:3]] == [0, s, t] and len(f) == 3 + R
            assert [float(x) for x in f[3:]] == [float(v) for v in traj.records[0, s, t]], f"start {s}, step {t}"
