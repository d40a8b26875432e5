"""Greedy evaluation episodes (grlx_evaluate / Runner.evaluate): one episode of the test agent per (replica, start state) pair, on the
device, against tests/policy_evaluate_ref.py -- a plain Python loop over the oracle's dense tables, its environment step and its first
observation.  Every comparison is on the bit patterns.  An evaluation must change nothing in the context.

Shapes: 3 or 5 replicas x 7 start states (21 or 35 pairs, never a multiple of 4: the last wave has dead 16-lane groups; the sweep's four
gammas cannot avoid one), 6 trials of training, max_steps 40 at most.  The oracle's half is computed once per case (every GPU test runs
clean and with poisoned registers)."""
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev
from tests.test_gpu_policy_query import SEED0, build, is_ac, same_bits

pytestmark = pytest.mark.gpu

# steps after which an episode is cut.  40 where the untrained agents' episodes are longer; the balancing acrobot and the walker fall
# within a dozen steps from most states, so their cut comes earlier -- every graph must show the codes 0, 1 and (where it has one) 2
MAX_STEPS = {"acrobot_q": 6, "walker_q": 5}
Q_GRAPHS = ["pendulum_sarsa", "pendulum_q_five_actions", "acrobot_q", "walker_q", "cart_pole_q", "advantage", "qv", "accumulating", "target_network"]
AC_GRAPHS = ["ac_twin", "ac_independent"]

_state_cache, _ref_cache = {}, {}


def max_steps_of(graph):
    return MAX_STEPS.get(graph, 40)


def start_states(graph, spec):
    """The 7 start states of a graph: the oracle's test start, three states its taps recorded, one a step short of the timeout (an episode
    of 1 or 2 steps: a ragged wave), one that is terminal already (absorbing where the task has such states, else past the timeout: it still
    takes one step), and a hand-made one inside the bound."""
    if graph in _state_cache:
        return _state_cache[graph]
    e = ob.Experiment(spec, seed=SEED0)
    e.env_start(1)
    first = e.state()
    e.close()
    e = ob.Experiment(spec, seed=SEED0)
    taps = e.run(3, tap_cap=400)[1]
    e.close()
    S = first.size
    tapped = [np.array(t.state[:S]) for t in taps]
    assert len(tapped) >= 6
    picks = [tapped[1], tapped[len(tapped) // 3], tapped[-2]]
    near, done, hand = first.copy(), first.copy(), first.copy()
    if spec.env == ob.ENV_COMPASS_WALKER:                   # [sla, ha, slar, har, changed, sfx, lasthipx, hipvel, stepdist, time, timeout]
        near[9] = near[10] - spec.control_step
        done[0] = 0.5                                       # the stance leg beyond pi / 8: fallen
        hand[0], hand[1], hand[2], hand[3], hand[9] = 0.12, 0.26, -0.2, 0.05, 3.0
    else:
        timeout = 20.0 if spec.env == ob.ENV_ACROBOT else spec.timeout
        near[S - 1] = timeout - spec.control_step
        if spec.env == ob.ENV_PENDULUM:
            done[S - 1] = timeout + 1.0                     # no absorbing state: past the timeout
            hand[:] = [-7.25, 11.5, 0.37]                   # more than one turn below zero
        elif spec.env == ob.ENV_ACROBOT:
            done[0] = np.pi + 0.5                           # the first link beyond 12 degrees: failed
            hand[:] = [np.pi + 0.01, -0.02, 0.3, -0.4, 1.0]
        else:
            done[0] = 3.0                                   # beyond the end stop (end_stop_penalty = 1: absorbing)
            hand[:] = [-1.5, 0.4, 2.0, -3.0, 2.5]
    states = np.array([first] + picks + [near, done, hand], np.float64)
    assert states.shape == (7, S) and np.isfinite(states).all() and (np.abs(states) < 2.0 ** 17).all()
    _state_cache[graph] = states
    return states


def reference(e, spec, states, max_steps, gamma=None):
    return ev.evaluate(ev.tables_of(e), spec, states, max_steps, gamma)


def oracle_stages(key, specs, seeds, states, stages, max_steps, prepare=None):
    """[stage][replica] -> the reference's dict; stage s is taken after sum(stages[:s + 1]) trials (stages[0] = 0: before any launch)"""
    if key not in _ref_cache:
        exps = [ob.Experiment(s, seed=int(seed)) for s, seed in zip(specs, seeds)]
        out = []
        for e in exps:
            if prepare:
                prepare(e)
        for trials in stages:
            for e in exps:
                if trials:
                    e.run(trials)
            out.append([reference(e, s, states, max_steps) for e, s in zip(exps, specs)])
        for e in exps:
            e.close()
        _ref_cache[key] = out
    return _ref_cache[key]


def check_evaluation(got, want, what):
    """all six outputs of Runner.evaluate, all replicas at once, against want[replica]"""
    for f in ev.FIELDS:
        same_bits(getattr(got, f), np.stack([w[f] for w in want]), f"{what}: {f}")


def run_against_oracle(grlx, graph, n, stages, seeds=None, specs=None, prepare=None, oracle_prepare=None, key=None, **cfg_only):
    cfg, spec = build(grlx, graph, n, **cfg_only)
    seeds = np.arange(SEED0, SEED0 + n) if seeds is None else seeds
    specs = [spec] * n if specs is None else specs(spec)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    want = oracle_stages(key or (graph, n, tuple(stages)), specs, seeds, states, stages, ms, oracle_prepare)
    r = grlx.Runner(cfg, seeds)
    if prepare:
        prepare(r)
    for s, trials in enumerate(stages):
        if trials:
            r.run(trials); r.sync()
        check_evaluation(r.evaluate(states, max_steps=ms), want[s], f"{graph} after {sum(stages[:s + 1])} trials")
    return r, spec, states, want


# ---- 1: every family against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", Q_GRAPHS + AC_GRAPHS)
def test_families_against_the_reference(grlx, graph):
    """evaluated before any launch and after 6 trials; Q agents 3 replicas, the actor-critic 5.  Over the pairs of the case every
    terminal code the task has must occur: 0 (cut), 1 (timed out) and, with absorbing states, 2."""
    n = 5 if graph in AC_GRAPHS else 3
    r, spec, states, want = run_against_oracle(grlx, graph, n, (0, 6))
    codes = set(int(c) for stage in want for w in stage for c in w["terminal"])
    need = {0, 1} if spec.env == ob.ENV_PENDULUM else {0, 1, 2}
    assert need <= codes, f"{graph}: the start states show the terminal codes {sorted(codes)} only"
    steps = np.stack([w["steps"] for w in want[-1]])
    assert (steps[:, 4] <= 2).all() and (steps[:, 5] == 1).all() and steps.max() == max_steps_of(graph)
    # a replica range of its own: the middle replica alone, one output only
    got = r.evaluate(states, replicas=range(1, 2), max_steps=max_steps_of(graph))
    same_bits(got.ret[0], want[-1][1]["ret"], "replica range: ret")
    same_bits(got.final_state[0], want[-1][1]["final_state"], "replica range: final_state")
    r.close()


def domain_exit_states(spec):
    """admitted walker states (every component below 2^17) whose first step ends outside Env::in_domain (|leg angle| >= 8)"""
    first = start_states("walker_q", spec)[0]
    a, b = first.copy(), first.copy()
    a[0] = 1000.0              # the model takes off one turn per sub-step at most: 20 of them leave about 874
    b[1] = -900.0
    return np.array([a, first, b])


def test_a_domain_exit_ends_the_episode_with_code_3(grlx):
    """the step is counted, the episode stops there with code 3 (it outranks the task's code), and no sticky flag is set: sync() after
    it, and a launch after that, raise nothing"""
    graph, n = "walker_q", 3
    cfg, spec = build(grlx, graph, n)
    states = domain_exit_states(spec)
    seeds = np.arange(SEED0, SEED0 + n)
    want = oracle_stages(("domain", n), [spec] * n, seeds, states, (0,), 5)[0]
    assert all(list(w["terminal"]) == [ev.DOMAIN, 0, ev.DOMAIN] and list(w["steps"]) == [1, 5, 1] for w in want)
    r = grlx.Runner(cfg, seeds)
    check_evaluation(r.evaluate(states, max_steps=5), want, "domain exit")
    r.sync()
    r.run(2); r.sync()
    r.close()


# ---- 2: the first maximum acts -----------------------------------------------------------------------------------------------------
def test_ties_take_the_first_action_and_are_counted(grlx):
    """init_min = init_max = 0 on a fresh context: every step ties, so ties == steps and the episode is the one of actions[0] throughout
    (the oracle's environment stepped with it, no table involved); no stream is drawn from"""
    cfg, spec = build(grlx, "ties", 3)
    states = start_states("ties", spec)
    key = ("ties", "first action")
    if key not in _ref_cache:
        want = dict(ret=[], steps=[], final_state=[])
        for s in states:
            x, ret, k = s.copy(), 0.0, 0
            while True:
                nx, _, rew, term = ob.env_step(spec, x, spec.action_min)
                x, ret, k = nx[0], ret + float(rew[0]), k + 1
                if term[0] or k == 40:
                    break
            want["ret"].append(ret); want["steps"].append(k); want["final_state"].append(x)
        _ref_cache[key] = {f: np.array(v) for f, v in want.items()}
    want = _ref_cache[key]
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + 3))
    rng_before = [list(r.rng(k)) for k in range(3)]
    got = r.evaluate(states, max_steps=40)
    assert (got.ties == got.steps).all() and (got.steps >= 1).all()
    for k in range(3):
        same_bits(got.ret[k], want["ret"], f"replica {k}: ret"); same_bits(got.steps[k], want["steps"], f"replica {k}: steps")
        same_bits(got.final_state[k], want["final_state"], f"replica {k}: final_state")
    assert [list(r.rng(k)) for k in range(3)] == rng_before, "a tie must not draw from any stream"
    r.close()


# ---- 3: against the project's own rows ---------------------------------------------------------------------------------------------
def test_an_evaluation_from_the_test_start_is_the_next_test_row(grlx):
    """independent of the Python reference's loop: after 10 trials (test_interval 10: the next trial is a test trial) the evaluation from
    the task's test start state, run to its end, has the return and the episode steps (the row's time column: discrete time) of the row
    that trial then writes, for every replica.
    Precondition (asserted on the reference's side, never skipped): no tie on the way."""
    n, graph = 3, "pendulum_sarsa"
    cfg, spec = build(grlx, graph, n)
    assert spec.test_interval == 10
    seeds = np.arange(SEED0, SEED0 + n)
    start = start_states(graph, spec)[:1]
    key = ("next test row", n)
    if key not in _ref_cache:
        out = []
        for seed in seeds:
            e = ob.Experiment(spec, seed=int(seed))
            e.run(10)
            w = reference(e, spec, start, 0)
            rows = e.run(1)[0]
            out.append((w, rows[-1].reward, int(rows[-1].time)))        # time: the episode's own steps (the steps column counts learning steps)
            e.close()
        _ref_cache[key] = out
    want = _ref_cache[key]
    for k, (w, reward, steps) in enumerate(want):
        assert w["ties"][0] == 0, f"seed {seeds[k]}: the reference's episode has ties; choose another seed"
        assert (w["steps"][0], w["terminal"][0]) == (steps, 1) and w["ret"][0] == reward, "the reference's loop is not the oracle's test trial"
    r = grlx.Runner(cfg, seeds)
    r.run(10); r.sync()
    got = r.evaluate(start)
    check_evaluation(got, [w for w, _, _ in want], "from the test start")
    assert (got.ties == 0).all()
    r.run(1); r.sync()
    for k in range(n):
        _, _, reward = r.rows(k)
        assert int(r.row_times(k, 0, len(reward))[-1]) == int(got.steps[k, 0]) == want[k][2], f"replica {k}: episode steps of the test row"
        same_bits(reward[-1:], got.ret[k], f"replica {k}: return of the test row")
    r.close()


# ---- 4: an evaluation changes nothing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,tables,n_rng", [("pendulum_sarsa", 1, 3), ("qv", 2, 3), ("ac_twin", 2, 2)])
def test_an_evaluation_changes_nothing(grlx, graph, tables, n_rng):
    """snapshot bytes, table_load, streams and environment states before and after; then 6 more trials: rows, streams, environment state
    and 2000 sampled weights equal the oracle's uninterrupted run.  On a fresh context set_replica_params stays allowed."""
    from tests.test_gpu_sweep import check_replica, oracle_run
    n = 3
    cfg, spec = build(grlx, graph, n)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    seeds = np.arange(SEED0, SEED0 + n)
    r = grlx.Runner(cfg, seeds)
    r.evaluate(states, max_steps=ms)
    if graph == "pendulum_sarsa":
        r.set_replica_params(alpha=[cfg.alpha] * n)          # an evaluation is no launch (the values are the configuration's: same oracle)
    r.run(6); r.sync()

    def look():
        return (r.snapshot(), [[r.table_load(k, t) for t in range(tables)] for k in range(n)], [list(r.rng(k)) for k in range(n)],
                [r.env_state(k).tobytes() for k in range(n)])

    before = look()
    r.evaluate(states, max_steps=ms)
    r.evaluate(states[:3], replicas=range(1, 3))
    after = look()
    assert after[0] == before[0], "an evaluation changed the context's snapshot"
    assert after[1:] == before[1:], "an evaluation changed table occupancy, a stream or an environment state"
    r.run(6); r.sync()
    for k in range(n):
        want = oracle_run(spec, seeds[k], (("run", 6), ("run", 6)), cfg.projector.memory, tables=tuple(range(tables)))
        check_replica(r, k, want, f"{graph}: replica {k} after an evaluation in between", cfg.projector.memory, n_rng=n_rng)
    r.close()


# ---- 5: a sweep context ------------------------------------------------------------------------------------------------------------
def test_a_sweep_context_discounts_with_each_replicas_gamma(grlx):
    n, gammas = 4, [0.8, 0.9, 0.95, 0.97]          # gamma * lambda must fit the trace's 10 entries: gamma <= 0.97 at lambda 0.65

    def specs(spec):
        out = []
        for g in gammas:
            s = type(spec).from_buffer_copy(spec)
            s.gamma = g
            out.append(s)
        return out

    r, spec, states, want = run_against_oracle(grlx, "pendulum_sarsa", n, (0, 6), specs=specs, prepare=lambda r: r.set_replica_params(gamma=gammas),
                                               key=("sweep", n))
    disc = np.stack([w["disc"] for w in want[-1]])
    assert len(set(disc[:, 0].tolist())) == n, "four gammas were meant to give four discounted returns from one start state"
    r.close()


# ---- 6: layouts and tables ---------------------------------------------------------------------------------------------------------
def test_a_small_memory(grlx):
    run_against_oracle(grlx, "memory_2048", 3, (0, 6))[0].close()


def test_eight_replicas_per_wave_thirteen_replicas(grlx):
    r = run_against_oracle(grlx, "pendulum_sarsa", 13, (0, 6), replicas_per_wave=8)[0]
    assert r.replicas_per_wave() == 8
    r.close()


def test_tables_that_have_grown(grlx):
    """2^13 entries at first, short launches so that the tables grow between them (positions change; the episodes do not)"""
    graph, n = "pendulum_sarsa", 3
    cfg, spec = build(grlx, graph, n, table_log2_capacity=13)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    want = oracle_stages((graph, n, (0, 6, 6)), [spec] * n, seeds, states, (0, 6, 6), 40)
    r = grlx.Runner(cfg, seeds)
    assert r.table_capacity() == 13
    for c in (1, 1, 2, 2):
        r.run(c); r.sync()
    check_evaluation(r.evaluate(states, max_steps=40), want[1], "grown tables after 6 trials")
    for c in (3, 3):
        r.run(c); r.sync()
    assert r.table_capacity() > 13, "the tables were meant to grow"
    check_evaluation(r.evaluate(states, max_steps=40), want[2], "grown tables after 12 trials")
    r.close()


def test_a_loaded_policy(grlx):
    """load_weights of a random image against the oracle's set_weights, before any launch and after 6 trials"""
    graph, n = "memory_2048", 3
    image = np.random.default_rng(5).uniform(-40.0, 10.0, 2048)
    r = run_against_oracle(grlx, graph, n, (0, 6), prepare=lambda r: r.load_weights(image), oracle_prepare=lambda e: e.set_weights(image),
                           key=("loaded", graph, n))[0]
    r.close()


def test_a_context_driven_step_by_step(grlx):
    """after agent_start and two agent_step calls, in mid-episode, against an oracle driven through the same calls; the episode then
    goes on as the oracle's does"""
    n, graph = 3, "pendulum_sarsa"
    cfg, spec = build(grlx, graph, n)
    states = start_states(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    key = ("stepwise", n)
    if key not in _ref_cache:
        want, nxt = [], []
        for seed in seeds:
            e = ob.Experiment(spec, seed=int(seed))
            a = e.agent_start(0, e.env_start(0))
            for _ in range(2):
                tau, o, rew, term = e.env_step(a)
                a = e.agent_step(0, tau, o, rew)
            want.append(reference(e, spec, states, 40))
            tau, o, rew, term = e.env_step(a)
            nxt.append(e.agent_step(0, tau, o, rew))
            e.close()
        _ref_cache[key] = (want, np.array(nxt))
    want, nxt = _ref_cache[key]
    r = grlx.Runner(cfg, seeds)
    a = r.agent_start(0, r.env_start(0))
    for _ in range(2):
        o, rew, term = r.env_advance(a)
        a = r.agent_step(0, o, rew)
    check_evaluation(r.evaluate(states, max_steps=40), want, "in mid-episode of a context driven step by step")
    o, rew, term = r.env_advance(a)
    same_bits(r.agent_step(0, o, rew), nxt, "the action after the evaluation")
    r.close()


# ---- 7: chunking -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum_q_five_actions", "ac_twin"])
def test_chunked_staging_gives_the_same_outputs(grlx, graph):
    """a bound on the staging that holds two start states (7 of them: four chunks), and one below a single start state (a chunk never has
    less than one)"""
    n = 5
    cfg, spec = build(grlx, graph, n)
    states, ms = start_states(graph, spec), max_steps_of(graph)
    S = states.shape[1]
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    lib = grlx.capi.load()
    whole = r.evaluate(states, max_steps=ms)
    assert len(set(whole.steps.ravel().tolist())) > 1
    try:
        per_start = 8 * S + n * (2 * 8 + 3 * 4 + 8 * S)
        for bound in (2 * per_start, 1):
            assert lib.grlx_set_query_chunk_bytes(bound) == 0
            got = r.evaluate(states, max_steps=ms)
            for f in ev.FIELDS:
                same_bits(getattr(got, f), getattr(whole, f), f"{f} with staging bounded to {bound} bytes")
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    r.close()


# ---- 8: refusals -------------------------------------------------------------------------------------------------------------------
def raw_evaluate(grlx, r, states, first, count, max_steps=0, n_starts=None, null_states=False):
    """grlx_evaluate on outputs filled with a pattern: (status, message, outputs untouched?)"""
    import ctypes as C
    states = np.ascontiguousarray(states, np.float64)
    n = states.shape[0] if n_starts is None else n_starts
    rows, S = max(count, 1) * max(n, 1), states.shape[1]
    f64 = [np.full(rows, 777.0) for _ in range(2)] + [np.full(rows * S, 777.0)]
    i32 = [np.full(rows, 777, np.int32) for _ in range(3)]
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = r.lib.grlx_evaluate(r._ctx, first, count, None if null_states else P(states, C.c_double), n, max_steps, P(f64[0], C.c_double), P(f64[1], C.c_double),
                             P(i32[0], C.c_int32), P(i32[1], C.c_int32), P(i32[2], C.c_int32), P(f64[2], C.c_double))
    return rc, r.lib.grlx_last_error().decode(), all((a == 777).all() for a in f64 + i32)


def refused(grlx, r, word, states, first=0, count=3, **kw):
    rc, msg, untouched = raw_evaluate(grlx, r, states, first, count, **kw)
    assert rc == grlx.capi.ERR_INVALID and word in msg, (rc, msg)
    assert untouched, "a refused evaluation wrote to its outputs"


def test_refusals(grlx):
    cfg, spec = build(grlx, "pendulum_sarsa", 3)
    states = start_states("pendulum_sarsa", spec)
    r = grlx.Runner(cfg, [1, 2, 3])
    refused(grlx, r, "states is null", states, null_states=True)
    refused(grlx, r, "n_starts = -1", states, n_starts=-1)
    refused(grlx, r, "replica range", states, first=2, count=2)
    refused(grlx, r, "replica range", states, first=-1, count=2)
    refused(grlx, r, "max_steps = -1", states, max_steps=-1)
    refused(grlx, r, "max_steps = 100001", states, max_steps=100001)
    bad = states.copy(); bad[2, 1] = np.nan
    refused(grlx, r, "row 2, component 1 is not finite", bad)
    bad[2, 1] = -np.inf
    refused(grlx, r, "row 2, component 1 is not finite", bad)
    bad[2, 1] = 0.0; bad[3, 0] = -2.0 ** 17
    refused(grlx, r, "row 3, component 0", bad)
    refused(grlx, r, "2^17", bad)
    bad[3, 0] = 0.0; bad[6, 2] = 131072.0
    refused(grlx, r, "row 6, component 2", bad)
    # (an (environment, action count) pair without an instantiation cannot be had: grlx_create admits no such context)
    with pytest.raises(ValueError):
        r.evaluate(states[:, :2])
    # nothing to do is no error, and nothing is written
    assert raw_evaluate(grlx, r, states, 0, 3, n_starts=0)[::2] == (0, True)
    assert raw_evaluate(grlx, r, states, 1, 0)[::2] == (0, True)
    # just inside the bound, and the largest max_steps: accepted
    ok = states.copy(); ok[3, 1] = np.nextafter(2.0 ** 17, 0.0)
    assert raw_evaluate(grlx, r, ok, 0, 3, max_steps=100000)[0] == 0
    r.close()

    safe, _ = build(grlx, "pendulum_sarsa", 3)
    safe.projector.safe = 1
    r = grlx.Runner(safe, [1, 2, 3])
    refused(grlx, r, "safe", states)
    refused(grlx, r, "not built", states)
    r.close()

    ext, _ = build(grlx, "pendulum_sarsa", 3)
    ext.env = grlx.capi.ENV_EXTERNAL
    ext.control_step, ext.timeout, ext.integration_steps = 0.0, 0.0, 0
    r = grlx.Runner(ext, [1, 2, 3])
    refused(grlx, r, "no environment", states)
    r.close()


# ---- 9: grlxd -E -------------------------------------------------------------------------------------------------------------------
def test_grlxd_evaluate(grlx, tmp_path):
    """golden pendulum yaml, -r 4 -t 12 -E: <output>-0-returns.txt against Runner.evaluate on an identical context and the host's sums
    (ascending clones, two passes), number for number: the file prints 17 significant digits"""
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")
    states = np.array([[np.pi, 0.0, 0.0], [0.0, 0.0, 0.0], [-1.0, 2.0, 1.5], [7.9, -11.25, 2.9], [0.5, 30.0, 3.5]])
    (tmp_path / "states.txt").write_text("# angle velocity time\n" + "\n".join(" ".join(repr(float(v)) for v in s) for s in states) + "\n")
    res = subprocess.run([grlxd, "-s", "5", "-r", "4", "-t", "12", "-q", "-E", "states.txt", yaml], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr + res.stdout
    cfg = grlx.pendulum_sarsa_config(4, max_rows=8)
    r = grlx.Runner(cfg, [5, 6, 7, 8])
    r.run(12); r.sync()
    got = r.evaluate(states)
    r.close()
    lines = [ln.split() for ln in (tmp_path / "pendulum-sarsa-tc-0-returns.txt").read_text().split("\n") if ln.strip()]
    assert len(lines) == states.shape[0]
    for s, f in enumerate(lines):
        assert len(f) == 8, f
        total = steps = 0.0
        for k in range(4):
            total += float(got.ret[k, s]); steps += float(got.steps[k, s])
        mean, sq = total / 4, 0.0
        for k in range(4):
            sq += (float(got.ret[k, s]) - mean) * (float(got.ret[k, s]) - mean)
        assert [float(f[0]), float(f[1]), float(f[2])] == [mean, float(np.sqrt(sq / 3)), steps / 4], f"start state {s}: {f}"
        assert [int(x) for x in f[3:7]] == [int((got.terminal[:, s] == c).sum()) for c in range(4)], f"start state {s}: terminal codes"
        assert int(f[7]) == int(got.ties[:, s].sum()), f"start state {s}: ties"
    assert int(lines[4][4]) == 4 and float(lines[4][2]) == 1.0, "a start past the timeout takes one step and times out"
