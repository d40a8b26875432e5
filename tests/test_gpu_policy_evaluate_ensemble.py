"""Ensemble evaluation episodes (grlx_evaluate_ensemble / Runner.evaluate_ensemble): one episode per (group of consecutive replicas, start
state) pair on the group's vote or mean Q, against tests/policy_evaluate_ensemble_ref.py -- a plain Python loop over the oracle's dense
tables -- and against the project's own grlx_evaluate, grlx_query_ensemble and the oracle's environment step.  Every comparison is on the
bit patterns, all eight outputs.  An evaluation must change nothing in the context.

Shapes: 10 replicas in two groups of 5 x 5 start states where nothing else is said; max_steps 40 at most.  One block serves one episode
with 16 members per round: 16 | 17 members are the two sides of the second round, 19 and 13 are no multiple of anything; 33, 48, 49
and 64 members of one 64-replica context are three and four rounds.  The oracle's
half is computed once per case (every GPU test runs clean and with poisoned registers)."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_ensemble_ref as ens
from tests import policy_evaluate_ref as ev
from tests import policy_query_ref as ref
from tests.test_gpu_policy_evaluate import max_steps_of, start_states
from tests.test_gpu_policy_query import SEED0, build, same_bits

pytestmark = pytest.mark.gpu

RULES = (("vote", ens.VOTE), ("mean", ens.MEAN_Q))
GRAPHS = ["pendulum_sarsa", "pendulum_q_five_actions", "acrobot_q", "walker_q", "cart_pole_q", "qv", "target_network"]

_ref_cache = {}


def five_states(graph, spec):
    """the test start, three tapped states, one a step short of the timeout"""
    return start_states(graph, spec)[:5]


def small_memory(cfg, spec, memory=32768):
    """many members: the oracle holds a dense vector per member"""
    for obj in (cfg, spec):
        obj.projector.memory = memory


def oracle_groups(key, specs, seeds, states, stages, max_steps, groups, gammas=None):
    """[stage][rule name] -> dict of the eight outputs stacked over `groups` (lists of member indices, ascending); stage s is taken after
    sum(stages[:s + 1]) trials.  gammas: per group, else the spec's."""
    if key not in _ref_cache:
        exps = [ob.Experiment(s, seed=int(seed)) for s, seed in zip(specs, seeds)]
        out = []
        for trials in stages:
            for e in exps:
                if trials:
                    e.run(trials)
            tables = [ref.dense(e, 0) for e in exps]
            stage = {}
            for name, rule in RULES:
                per = [ens.evaluate([tables[m] for m in g], specs[g[0]], states, rule, max_steps, None if gammas is None else gammas[k])
                       for k, g in enumerate(groups)]
                stage[name] = {f: np.stack([p[f] for p in per]) for f in ens.FIELDS}
            out.append(stage)
        for e in exps:
            e.close()
        _ref_cache[key] = out
    return _ref_cache[key]


def check(got, want, what):
    for f in ens.FIELDS:
        same_bits(getattr(got, f), want[f], f"{what}: {f}")


def consecutive(n, G, first=0):
    return [list(range(first + g * G, first + (g + 1) * G)) for g in range(n // G)]


# ---- 1: every family against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
def test_families_against_the_reference(grlx, graph):
    """10 replicas in two groups of 5, both rules, before any launch and after 6 trials.  The inputs must exercise the combination (asserted
    on the reference alone): members that disagree, a tied vote, and the two rules parting."""
    n, G = 10, 5
    cfg, spec = build(grlx, graph, n)
    seeds = np.arange(SEED0, SEED0 + n)
    states, ms = five_states(graph, spec), max_steps_of(graph)
    want = oracle_groups((graph, n, G), [spec] * n, seeds, states, (0, 6), ms, consecutive(n, G))
    everything = [stage[name] for stage in want for name, _ in RULES]
    assert any((w["agreement"] < w["steps"].astype(np.int64) * G).any() for w in everything), f"{graph}: the members never disagree"
    assert any((stage["vote"]["ties"] > 0).any() for stage in want), f"{graph}: the vote never ties"
    assert any(stage["vote"][f].tobytes() != stage["mean"][f].tobytes() for stage in want for f in ens.FIELDS), f"{graph}: the two rules never part"
    steps = want[-1]["vote"]["steps"]
    assert (steps[:, 4] <= 2).all() and steps.max() == ms, f"{graph}: the pairs were meant to be ragged"
    r = grlx.Runner(cfg, seeds)
    for s, trials in enumerate((0, 6)):
        if trials:
            r.run(trials); r.sync()
        for name, _ in RULES:
            check(r.evaluate_ensemble(states, G, name, max_steps=ms), want[s][name], f"{graph}, {name}, after {trials} trials")
    r.close()


# ---- 2: a group of one is grlx_evaluate --------------------------------------------------------------------------------------------
def test_a_group_of_one_is_the_single_policy(grlx):
    graph, n = "pendulum_sarsa", 3
    cfg, spec = build(grlx, graph, n)
    states = five_states(graph, spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    single = r.evaluate(states, max_steps=40)
    for name, _ in RULES:
        got = r.evaluate_ensemble(states, 1, name, max_steps=40)
        for f in ("ret", "disc", "steps", "terminal", "final_state"):
            same_bits(getattr(got, f), getattr(single, f), f"{name}: {f}")
        same_bits(got.member_ties, single.ties, f"{name}: member_ties")
        same_bits(got.agreement, single.steps, f"{name}: agreement")
    r.close()


# ---- 3: one step is one query ------------------------------------------------------------------------------------------------------
def test_one_step_is_one_query(grlx):
    """max_steps = 1: the state after the step is the oracle's env_step with actions[first maximum] of the columns grlx_query_ensemble
    returns at observe(state); the agreement is that column's vote"""
    graph, n, G = "pendulum_sarsa", 10, 5
    cfg, spec = build(grlx, graph, n)
    states = five_states(graph, spec)
    A, acts = int(spec.action_steps), ref.actions_of(spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    obs = np.array([ev.observe(spec, s)[0] for s in states])
    cols = r.query_ensemble_raw(obs, G)
    assert cols.shape == (n // G, states.shape[0], 2 + 2 * A)
    for name, _ in RULES:
        got = r.evaluate_ensemble(states, G, name, max_steps=1)
        assert (got.steps == 1).all()
        for g in range(n // G):
            for s in range(states.shape[0]):
                votes, sumq = [float(v) for v in cols[g, s, 2 + A:]], [float(v) for v in cols[g, s, 2:2 + A]]
                mai, man = ref.findmax(votes if name == "vote" else sumq)
                x, _, reward, term = ob.env_step(spec, states[s], acts[mai])
                same_bits(got.final_state[g, s], x[0], f"{name}: group {g}, state {s}: final_state")
                same_bits(got.ret[g, s:s + 1], reward[:1], f"{name}: group {g}, state {s}: ret")
                assert int(got.agreement[g, s]) == int(votes[mai]) and int(got.ties[g, s]) == (1 if man > 1 else 0)
                assert int(got.terminal[g, s]) == int(term[0])
    r.close()


# ---- 4: more members than one round, and no power of two ---------------------------------------------------------------------------
def test_many_members(grlx):
    """38 replicas on a 32768-slot memory, 2 start states, 12 steps: two groups of 19, one group of 19, and on the first replicas two
    groups of 4, one group of 16 (exactly one round) and one of 17 (a second round with one member)"""
    graph, n = "pendulum_sarsa", 38
    cfg, spec = build(grlx, graph, n)
    small_memory(cfg, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    states = five_states(graph, spec)[1:3]
    cases = [(38, 19), (19, 19), (8, 4), (16, 16), (17, 17)]
    groups = [g for count, G in cases for g in consecutive(count, G)]
    want = oracle_groups(("many", n), [spec] * n, seeds, states, (6,), 12, groups)[0]
    r = grlx.Runner(cfg, seeds)
    r.run(6); r.sync()
    at = 0
    for count, G in cases:
        for name, _ in RULES:
            got = r.evaluate_ensemble(states, G, name, replicas=range(0, count), max_steps=12)
            check(got, {f: want[name][f][at:at + count // G] for f in ens.FIELDS}, f"{count} replicas in groups of {G}, {name}")
        at += count // G
    r.close()


# ---- 4b: three and four rounds per step ----------------------------------------------------------------------------------------------
LARGE = [(0, 33, 33), (0, 48, 48), (0, 49, 49), (0, 64, 64), (0, 64, 32), (16, 48, 48)]      # (first replica, replicas, group size)


@pytest.mark.parametrize("graph,trials", [("pendulum_sarsa", 6), ("pendulum_q_five_actions", 6), ("ties", 0)])
def test_three_and_four_rounds(grlx, graph, trials):
    """64 replicas on a 32768-slot memory, 2 start states, 12 steps: one group each of 33 (three rounds, one member in the last), 48, 49
    and 64 (four full rounds), two groups of 32, and replicas 16 ... 63 as one group of 48.  An odd number of rounds flips the parity of
    the members' LDS buffer from step to step.  pendulum_q_five_actions: five Q-values per member slot.  The combination must be
    exercised (asserted on the reference alone): members that disagree, a tied vote, and the two rules parting.  The learned members
    never tie among their own Q-values (member_ties is 0 throughout), so the `ties` graph is run before any launch: init_min =
    init_max = 0, every member of every round ties at every step."""
    n = 64
    cfg, spec = build(grlx, graph, n)
    states = five_states(graph, spec)[1:3]
    small_memory(cfg, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    groups = [g for first, count, G in LARGE for g in consecutive(count, G, first)]
    want = oracle_groups(("large", graph, n), [spec] * n, seeds, states, (trials,), 12, groups)[0]
    sizes = np.array([len(g) for g in groups], np.int64)[:, None]
    assert want["vote"]["steps"].max() == 12
    if graph == "ties":
        assert all((want[name]["member_ties"] == want[name]["steps"] * sizes).all() for name, _ in RULES), "ties: every member was meant to tie at every step"
    else:
        assert all((want[name]["agreement"] < want[name]["steps"] * sizes).any() for name, _ in RULES), f"{graph}: the members never disagree"
        assert (want["vote"]["ties"] > 0).any(), f"{graph}: the vote never ties"
        assert any(want["vote"][f].tobytes() != want["mean"][f].tobytes() for f in ens.FIELDS), f"{graph}: the two rules never part"
    r = grlx.Runner(cfg, seeds)
    if trials:
        r.run(trials); r.sync()
    at = 0
    for first, count, G in LARGE:
        for name, _ in RULES:
            got = r.evaluate_ensemble(states, G, name, replicas=range(first, first + count), max_steps=12)
            check(got, {f: want[name][f][at:at + count // G] for f in ens.FIELDS}, f"{graph}: replicas {first} ... {first + count - 1} in groups of {G}, {name}")
        at += count // G
    r.close()


# ---- 5: ranges and layouts ---------------------------------------------------------------------------------------------------------
def test_the_second_group_alone_and_chunked_staging(grlx):
    """first_replica != 0: the second group alone gives its rows of the full call; a staging bound that holds two start states, and one
    below a single start state, give the same outputs"""
    graph, n, G = "pendulum_q_five_actions", 10, 5
    cfg, spec = build(grlx, graph, n)
    states, S = five_states(graph, spec), 3
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    lib = grlx.capi.load()
    for name, _ in RULES:
        whole = r.evaluate_ensemble(states, G, name, max_steps=40)
        assert len(set(whole.steps.ravel().tolist())) > 1
        second = r.evaluate_ensemble(states, G, name, replicas=range(5, 10), max_steps=40)
        for f in ens.FIELDS:
            same_bits(getattr(second, f), getattr(whole, f)[1:], f"{name}: the second group alone: {f}")
        try:
            per_start = 8 * S + (n // G) * (2 * 8 + 3 * 4 + 2 * 8 + 8 * S)
            for bound in (2 * per_start, 1):
                assert lib.grlx_set_query_chunk_bytes(bound) == 0
                got = r.evaluate_ensemble(states, G, name, max_steps=40)
                for f in ens.FIELDS:
                    same_bits(getattr(got, f), getattr(whole, f), f"{name}: {f} with staging bounded to {bound} bytes")
        finally:
            lib.grlx_set_query_chunk_bytes(0)
    r.close()


def test_thirteen_replicas_at_eight_per_wave(grlx):
    graph, n = "pendulum_sarsa", 13
    cfg, spec = build(grlx, graph, n, replicas_per_wave=8)
    small_memory(cfg, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    states = five_states(graph, spec)
    want = oracle_groups(("thirteen", n), [spec] * n, seeds, states, (6,), 40, consecutive(n, n))[0]
    r = grlx.Runner(cfg, seeds)
    assert r.replicas_per_wave() == 8
    r.run(6); r.sync()
    for name, _ in RULES:
        check(r.evaluate_ensemble(states, n, name, max_steps=40), want[name], f"one group of 13, {name}")
    r.close()


def test_a_small_memory(grlx):
    graph, n, G = "memory_2048", 10, 5
    cfg, spec = build(grlx, graph, n)
    seeds = np.arange(SEED0, SEED0 + n)
    states = five_states(graph, spec)
    want = oracle_groups((graph, n, G), [spec] * n, seeds, states, (0, 6), 40, consecutive(n, G))
    r = grlx.Runner(cfg, seeds)
    for s, trials in enumerate((0, 6)):
        if trials:
            r.run(trials); r.sync()
        for name, _ in RULES:
            check(r.evaluate_ensemble(states, G, name, max_steps=40), want[s][name], f"2048 slots, {name}, after {trials} trials")
    r.close()


def test_tables_that_have_grown(grlx):
    """2^13 entries at first, short launches so that the tables grow between them (positions change; the episodes do not)"""
    graph, n, G = "pendulum_sarsa", 10, 5
    cfg, spec = build(grlx, graph, n, table_log2_capacity=13)
    seeds = np.arange(SEED0, SEED0 + n)
    states = five_states(graph, spec)
    want = oracle_groups((graph, n, G, "grown"), [spec] * n, seeds, states, (6, 6), 40, consecutive(n, G))
    r = grlx.Runner(cfg, seeds)
    assert r.table_capacity() == 13
    for c in (1, 1, 2, 2):
        r.run(c); r.sync()
    for name, _ in RULES:
        check(r.evaluate_ensemble(states, G, name, max_steps=40), want[0][name], f"grown tables after 6 trials, {name}")
    for c in (3, 3):
        r.run(c); r.sync()
    assert r.table_capacity() > 13, "the tables were meant to grow"
    for name, _ in RULES:
        check(r.evaluate_ensemble(states, G, name, max_steps=40), want[1][name], f"grown tables after 12 trials, {name}")
    r.close()


# ---- 6: a sweep context ------------------------------------------------------------------------------------------------------------
def test_a_sweep_context_discounts_with_the_first_members_gamma(grlx):
    """two points x 3 repetitions, gamma 0.8 and 0.97"""
    graph, n, G = "pendulum_sarsa", 6, 3
    gammas = [0.8] * 3 + [0.97] * 3
    cfg, spec = build(grlx, graph, n)
    specs = []
    for g in gammas:
        s = type(spec).from_buffer_copy(spec)
        s.gamma = g
        specs.append(s)
    seeds = np.arange(SEED0, SEED0 + n)
    states = five_states(graph, spec)
    want = oracle_groups(("sweep", n), specs, seeds, states, (0, 6), 40, consecutive(n, G), gammas=[0.8, 0.97])
    for stage in want:
        for name, _ in RULES:
            w = stage[name]
            assert (w["disc"][:, 0] != w["ret"][:, 0]).all()
    r = grlx.Runner(cfg, seeds)
    r.set_replica_params(gamma=gammas)
    for s, trials in enumerate((0, 6)):
        if trials:
            r.run(trials); r.sync()
        for name, _ in RULES:
            check(r.evaluate_ensemble(states, G, name, max_steps=40), want[s][name], f"sweep, {name}, after {trials} trials")
    # the same episodes discount differently under the other point's gamma: disc depends on the FIRST member of the group alone
    got = r.evaluate_ensemble(states, G, "vote", replicas=range(3, 6), max_steps=40)
    same_bits(got.disc[0], want[1]["vote"]["disc"][1], "the second point alone")
    r.close()


# ---- 7: an evaluation changes nothing ----------------------------------------------------------------------------------------------
def test_an_ensemble_evaluation_changes_nothing(grlx):
    """snapshot bytes, table_load, streams and environment states before and after; then 6 more trials: rows, streams, environment state
    and sampled weights equal the oracle's uninterrupted run.  On a fresh context set_replica_params stays allowed."""
    from tests.test_gpu_sweep import check_replica, oracle_run
    graph, n = "pendulum_sarsa", 3
    cfg, spec = build(grlx, graph, n)
    states = five_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    r = grlx.Runner(cfg, seeds)
    r.evaluate_ensemble(states, 3, "vote", max_steps=40)
    r.set_replica_params(alpha=[cfg.alpha] * n)              # an evaluation is no launch (the values are the configuration's: same oracle)
    r.run(6); r.sync()

    def look():
        return (r.snapshot(), [r.table_load(k, 0) for k in range(n)], [list(r.rng(k)) for k in range(n)], [r.env_state(k).tobytes() for k in range(n)])

    before = look()
    r.evaluate_ensemble(states, 3, "vote", max_steps=40)
    r.evaluate_ensemble(states[:3], 1, "mean", replicas=range(1, 3))
    after = look()
    assert after[0] == before[0], "an ensemble evaluation changed the context's snapshot"
    assert after[1:] == before[1:], "an ensemble evaluation changed table occupancy, a stream or an environment state"
    r.run(6); r.sync()
    for k in range(n):
        want = oracle_run(spec, seeds[k], (("run", 6), ("run", 6)), cfg.projector.memory, tables=(0,))
        check_replica(r, k, want, f"replica {k} after an ensemble evaluation in between", cfg.projector.memory, n_rng=3)
    r.close()


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------
def raw(grlx, r, states, count=4, group_size=2, rule=0, max_steps=0, null_states=False):
    """grlx_evaluate_ensemble on outputs filled with a pattern: (status, message, outputs untouched?)"""
    import ctypes as C
    states = np.ascontiguousarray(states, np.float64)
    n, S = states.shape
    rows = max(count, 1) * n
    f64 = [np.full(rows, 777.0) for _ in range(2)] + [np.full(rows * S, 777.0)]
    i32 = [np.full(rows, 777, np.int32) for _ in range(3)]
    i64 = [np.full(rows, 777, np.int64) for _ in range(2)]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = r.lib.grlx_evaluate_ensemble(r._ctx, 0, count, group_size, rule, None if null_states else P(states, C.c_double), n, max_steps,
                                      P(f64[0], C.c_double), P(f64[1], C.c_double), P(i32[0], C.c_int32), P(i32[1], C.c_int32), P(i32[2], C.c_int32),
                                      P(i64[0], C.c_int64), P(i64[1], C.c_int64), P(f64[2], C.c_double))
    return rc, r.lib.grlx_last_error().decode(), all((a == 777).all() for a in f64 + i32 + i64)


def refused(grlx, r, word, states, **kw):
    rc, msg, untouched = raw(grlx, r, states, **kw)
    assert rc == grlx.capi.ERR_INVALID and word in msg and "grlx_evaluate_ensemble" in msg, (rc, msg)
    assert untouched, "a refused evaluation wrote to its outputs"


def test_refusals(grlx):
    cfg, spec = build(grlx, "pendulum_sarsa", 4)
    states = five_states("pendulum_sarsa", spec)
    r = grlx.Runner(cfg, [1, 2, 3, 4])
    refused(grlx, r, "group_size = 0", states, group_size=0)
    refused(grlx, r, "group_size = -2", states, group_size=-2)
    refused(grlx, r, "group_size 3 does not divide the 4 replicas", states, group_size=3)
    refused(grlx, r, "unknown rule 2", states, rule=2)
    refused(grlx, r, "unknown rule -1", states, rule=-1)
    refused(grlx, r, "states is null", states, null_states=True)
    refused(grlx, r, "replica range", states, count=5, group_size=5)
    refused(grlx, r, "max_steps = -1", states, max_steps=-1)
    refused(grlx, r, "max_steps = 100001", states, max_steps=100001)
    bad = states.copy(); bad[3, 0] = -2.0 ** 17
    refused(grlx, r, "row 3, component 0", bad)
    refused(grlx, r, "2^17", bad)
    bad[3, 0] = np.nan
    refused(grlx, r, "row 3, component 0 is not finite", bad)
    # nothing to do is no error, and nothing is written
    assert raw(grlx, r, states[:0])[::2] == (0, True)
    assert raw(grlx, r, states, count=0)[::2] == (0, True)
    # the whole context as one group, the largest max_steps: accepted
    assert raw(grlx, r, states[4:], group_size=4, max_steps=100000)[0] == 0
    r.close()

    safe, _ = build(grlx, "pendulum_sarsa", 4)
    safe.projector.safe = 1
    r = grlx.Runner(safe, [1, 2, 3, 4])
    refused(grlx, r, "safe", states)
    refused(grlx, r, "not built", states)
    r.close()

    ac, ac_spec = build(grlx, "ac_twin", 4)
    r = grlx.Runner(ac, [1, 2, 3, 4])
    ac_states = start_states("ac_twin", ac_spec)[:2]
    refused(grlx, r, "actor-critic", ac_states)
    refused(grlx, r, "not built", ac_states)
    r.close()


# ---- 9: grlxd -p ... -E ... -V -----------------------------------------------------------------------------------------------------
def test_grlxd_ensemble_of_a_sweep(grlx, tmp_path):
    """golden pendulum yaml, two points x 3 repetitions, -t 220 (a sweep's regret wants 20 rows): <output>-0-ensemble.txt against Runner.evaluate_ensemble on an identical
    context, number for number (the file prints 17 significant digits); the returns file is the one of a run without -V, byte for byte"""
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")
    states = np.array([[np.pi, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.0, 2.0, 1.5], [7.9, -11.25, 2.9], [0.5, 30.0, 3.5]])
    text = "# angle velocity time\n" + "\n".join(" ".join(repr(float(v)) for v in s) for s in states) + "\n"
    common = [grlxd, "-s", "5", "-r", "3", "-t", "220", "-q", "-p", "/experiment/agent/predictor/alpha=0.1,0.2", "-E", "states.txt"]
    files = {}
    for sub, extra in (("plain", []), ("vote", ["-V", "vote"])):
        (tmp_path / sub).mkdir()
        (tmp_path / sub / "states.txt").write_text(text)
        res = subprocess.run(common + extra + [yaml], cwd=tmp_path / sub, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr + res.stdout
        files[sub] = (tmp_path / sub / "pendulum-sarsa-tc-0-returns.txt").read_bytes()
    assert files["plain"] == files["vote"] and files["plain"], "-V changed the returns file"
    assert not (tmp_path / "plain" / "pendulum-sarsa-tc-0-ensemble.txt").exists()
    cfg = grlx.pendulum_sarsa_config(6, max_rows=32)
    r = grlx.Runner(cfg, [5, 6, 7, 8, 9, 10])
    r.set_replica_params(alpha=[0.1] * 3 + [0.2] * 3)
    r.run(220); r.sync()
    got = r.evaluate_ensemble(states, 3, "vote")
    r.close()
    lines = [ln.split() for ln in (tmp_path / "vote" / "pendulum-sarsa-tc-0-ensemble.txt").read_text().split("\n") if ln.strip()]
    assert len(lines) == 2 * states.shape[0]
    for g in range(2):
        for s in range(states.shape[0]):
            f = lines[g * states.shape[0] + s]
            assert len(f) == 8 and int(f[0]) == g, f
            assert [float(f[1]), float(f[2])] == [float(got.ret[g, s]), float(got.disc[g, s])], f"point {g}, start state {s}: {f}"
            assert [int(x) for x in f[3:7]] == [int(got.steps[g, s]), int(got.terminal[g, s]), int(got.ties[g, s]), int(got.member_ties[g, s])], f
            assert float(f[7]) == float(got.agreement[g, s]) / (float(got.steps[g, s]) * 3.0), f
    assert int(lines[4][3]) == 1 and int(lines[4][4]) == 1, "a start past the timeout takes one step and times out"
