"""Policy queries (grlx_query_q / _state / _ensemble): Q-values, state values and greedy actions of every replica at observations of the
caller's choice, against the oracle's dense tables (tests/policy_query_ref.py: plain float loops in the reference's order).  Every
comparison is on the bit patterns (0 ulp).  A query must change nothing in the context; grlx_read, the path it replaces,
does -- which is pinned here too.

Shapes: 3 / 5 / 13 replicas x 11 observations (never a multiple of 4: the last wave has dead 16-lane groups; the ensemble's 8 replicas
cannot avoid a multiple), 12 trials in two launches.  The oracle's half is computed once per case (every GPU test runs clean and with
poisoned registers)."""
import numpy as np
import pytest

from tests import configs
from tests import oracle_binding as ob
from tests import policy_query_ref as ref
from tests.test_gpu_sweep import check_replica, oracle_run

pytestmark = pytest.mark.gpu

SEED0 = 71


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} vs {want.shape}"
    if got.dtype.kind == "f":
        g, w = got.astype(np.float64).view(np.uint64).ravel(), want.astype(np.float64).view(np.uint64).ravel()
    else:
        g, w = got.astype(np.int64).ravel(), want.astype(np.int64).ravel()
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} differ, first at {bad[:5]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


# ---- the graphs: name -> (builder, builder keywords, fields set on configuration AND oracle spec, tweak) -----------------------------
def _memory(m):
    def tweak(cfg, spec):
        for obj in (cfg, spec):
            obj.projector.memory = m
    return tweak


def _independent(cfg, spec):
    for obj in (cfg, spec):                                  # test_actor_critic_with_different_tile_codings: no twin tables
        obj.projector.memory = 4194304
        obj.projector.resolution[0] = 1.25
        obj.projector.resolution[2] = 5.0


GRAPHS = {
    "pendulum_sarsa": (configs.pendulum, dict(agent=0), {}, None),
    "pendulum_q_five_actions": (configs.pendulum, dict(agent=1), dict(action_steps=5), None),
    "acrobot_q": (configs.acrobot, dict(agent=1), {}, None),
    "walker_q": (configs.compass_walker, dict(agent=1), {}, None),
    "cart_pole_q": (configs.cart_pole_q, dict(agent=1), {}, None),
    "advantage": (configs.pendulum, dict(agent=4, kappa=0.2), dict(kappa=0.2), None),
    "qv": (configs.pendulum_qv, {}, {}, None),
    "accumulating": (configs.pendulum, dict(agent=0), dict(trace=2), None),
    # the oracle's target network is a dense vector blended at every synchronisation: a small memory keeps it quick
    "target_network": (configs.pendulum, dict(agent=0), dict(target_interval=10, target_tau=0.3), _memory(32768)),
    "memory_2048": (configs.pendulum, dict(agent=0), {}, _memory(2048)),
    "memory_2039": (configs.pendulum, dict(agent=1), {}, _memory(2039)),
    "ties": (configs.pendulum, dict(agent=0), {}, None),
    "ac_twin": (configs.cart_pole_ac, dict(end_stop_penalty=1), {}, None),
    "ac_independent": (configs.cart_pole_ac, dict(end_stop_penalty=1), {}, _independent),
}


def build(grlx, graph, n, **cfg_only):
    make, kw, both, tweak = GRAPHS[graph]
    cfg, spec = make(grlx, n, **kw)
    for k, v in both.items():
        setattr(cfg, k, v); setattr(spec, k, v)
    if tweak:
        tweak(cfg, spec)
    if graph == "ties":
        for obj in (cfg, spec):
            obj.representation.init_min = obj.representation.init_max = 0.0
    cfg.max_rows = 64
    for k, v in cfg_only.items():
        setattr(cfg, k, v)
    spec.math = ob.MATH_PORTABLE
    return cfg, spec


def is_ac(spec):
    return spec.agent == ob.AGENT_AC


def obs_dims_of(spec):
    return spec.projector.dims - (0 if is_ac(spec) else 1)


_obs_cache, _ref_cache = {}, {}


def observations(graph, spec):
    if graph not in _obs_cache:
        _obs_cache[graph] = ref.observation_set(spec.projector, obs_dims_of(spec), ref.visited_observations(spec, SEED0))
    return _obs_cache[graph]


def reference(e, spec, obs):
    """everything a replica's queries return, from the oracle experiment e as it stands"""
    out = {}
    if is_ac(spec):
        out["state0"] = ref.query_state(ref.dense(e, 0), spec, 0, obs)
        out["state1"] = ref.query_state(ref.dense(e, 1), spec, 1, obs)
    else:
        out["q"], out["value"], out["greedy"], out["n_max"] = ref.query_q(ref.dense(e, 0), spec, obs)
        if spec.agent == ob.AGENT_QV:
            out["state1"] = ref.query_state(ref.dense(e, 1), spec, 1, obs)
    return out


def oracle_stages(key, specs, seeds, obs, stages):
    """[stage][replica] -> reference(); stage s is taken after sum(stages[:s + 1]) trials (stages[0] = 0: before any launch)"""
    if key not in _ref_cache:
        exps = [ob.Experiment(s, seed=int(seed)) for s, seed in zip(specs, seeds)]
        out = []
        for trials in stages:
            for e in exps:
                if trials:
                    e.run(trials)
            out.append([reference(e, s, obs) for e, s in zip(exps, specs)])
        for e in exps:
            e.close()
        _ref_cache[key] = out
    return _ref_cache[key]


def check_queries(r, spec, obs, want, what):
    """every query the graph has, all replicas at once, against want[replica]"""
    n = len(want)
    if is_ac(spec):
        for t in (0, 1):
            same_bits(r.query_state(obs, t), np.stack([w["state%d" % t] for w in want]), f"{what}: query_state({t})")
        clipped = np.minimum(np.maximum(np.stack([w["state1"] for w in want]), spec.action_min), spec.action_max)
        same_bits(r.policy_action(obs), clipped, f"{what}: policy_action")
        return
    q, value, greedy, n_max = r.query_q(obs)
    assert q.shape == (n, obs.shape[0], spec.action_steps)
    same_bits(q, np.stack([w["q"] for w in want]), f"{what}: q")
    same_bits(value, np.stack([w["value"] for w in want]), f"{what}: value")
    same_bits(greedy, np.stack([w["greedy"] for w in want]), f"{what}: greedy")
    same_bits(n_max, np.stack([w["n_max"] for w in want]), f"{what}: n_max")
    same_bits(r.policy_action(obs), np.array(ref.actions_of(spec))[np.stack([w["greedy"] for w in want])], f"{what}: policy_action")
    if spec.agent == ob.AGENT_QV:
        same_bits(r.query_state(obs, 1), np.stack([w["state1"] for w in want]), f"{what}: query_state(1)")


def run_against_oracle(grlx, graph, n, stages, seeds=None, specs=None, prepare=None, key=None, **cfg_only):
    cfg, spec = build(grlx, graph, n, **cfg_only)
    seeds = np.arange(SEED0, SEED0 + n) if seeds is None else seeds
    specs = [spec] * n if specs is None else specs(spec)
    obs = observations(graph, spec)
    want = oracle_stages(key or (graph, n, tuple(stages)), specs, seeds, obs, stages)
    r = grlx.Runner(cfg, seeds)
    if prepare:
        prepare(r)
    for s, trials in enumerate(stages):
        if trials:
            r.run(trials); r.sync()
        check_queries(r, spec, obs, want[s], f"{graph} after {sum(stages[:s + 1])} trials")
    return r, spec, obs, want


# ---- 1: Q agents against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum_sarsa", "pendulum_q_five_actions", "acrobot_q", "walker_q", "cart_pole_q", "advantage", "qv",
                                   "accumulating", "target_network"])
def test_q_agents_against_the_oracle(grlx, graph):
    """3 replicas x 11 observations; queried before any launch, between two launches of 6 trials and after.  QV: query_q on table 0 and
    query_state on table 1.  The target-network context is served its MAIN values (the oracle's table 0)."""
    r, spec, obs, want = run_against_oracle(grlx, graph, 3, (0, 6, 6))
    # a replica range of its own: the middle replica alone
    if not is_ac(spec):
        q, value, greedy, n_max = r.query_q(obs, replicas=range(1, 2))
        same_bits(q[0], want[-1][1]["q"], "replica range: q")
        same_bits(greedy[0], want[-1][1]["greedy"], "replica range: greedy")
    r.close()


# ---- 2: ties ----------------------------------------------------------------------------------------------------------------------
def test_ties_are_reported_not_broken(grlx):
    """init_min = init_max = 0: on a fresh context every action ties everywhere; after 3 trials the ties remain exactly where the
    oracle has them, among them the observations far from anything visited."""
    cfg, spec = build(grlx, "ties", 3)
    obs = observations("ties", spec)
    seeds = np.arange(SEED0, SEED0 + 3)
    want = oracle_stages(("ties", 3), [spec] * 3, seeds, obs, (0, 3))
    r = grlx.Runner(cfg, seeds)
    rng_before = [list(r.rng(k)) for k in range(3)]
    q, value, greedy, n_max = r.query_q(obs)
    assert (n_max == spec.action_steps).all() and (greedy == 0).all()
    same_bits(value, np.zeros_like(value), "value of an all-zero table")
    same_bits(q, np.zeros_like(q), "q of an all-zero table")
    assert [list(r.rng(k)) for k in range(3)] == rng_before, "a tie must not draw from any stream"
    r.run(3); r.sync()
    check_queries(r, spec, obs, want[1], "ties after 3 trials")
    n_max = r.query_q(obs)[3]
    assert (n_max[:, 3:5] == spec.action_steps).all(), "the far observations still tie"
    assert (n_max[:, 0:3] < spec.action_steps).any(), "somewhere the oracle visited, the tie is gone"
    r.close()


# ---- 3: small memories -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["memory_2048", "memory_2039"])
def test_small_memories(grlx, graph):
    """2048 slots (most are shared between tilings) and 2039 (no power of two: the modulo path of the projector)"""
    run_against_oracle(grlx, graph, 3, (0, 6, 6))[0].close()


# ---- 4: layouts and storage --------------------------------------------------------------------------------------------------------
def test_eight_replicas_per_wave_thirteen_replicas(grlx):
    r = run_against_oracle(grlx, "pendulum_sarsa", 13, (0, 6, 6), replicas_per_wave=8)[0]
    assert r.replicas_per_wave() == 8
    r.close()


def test_tables_that_have_grown(grlx):
    """2^13 entries at first, short launches so that the tables grow between them (positions change; the values read do not)"""
    graph, n = "pendulum_sarsa", 3
    cfg, spec = build(grlx, graph, n, table_log2_capacity=13)
    obs = observations(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    want = oracle_stages((graph, n, (0, 6, 6)), [spec] * n, seeds, obs, (0, 6, 6))
    r = grlx.Runner(cfg, seeds)
    assert r.table_capacity() == 13
    for c in (1, 1, 2, 2):
        r.run(c); r.sync()
    check_queries(r, spec, obs, want[1], "grown tables after 6 trials")
    for c in (3, 3):
        r.run(c); r.sync()
    assert r.table_capacity() > 13, "the tables were meant to grow"
    check_queries(r, spec, obs, want[2], "grown tables after 12 trials")
    r.close()


def test_a_loaded_policy(grlx):
    """load_weights of a random image against the oracle's set_weights: untouched slots read the image, touched ones what was learned"""
    graph, n = "memory_2048", 3
    cfg, spec = build(grlx, graph, n)
    obs = observations(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    image = np.random.default_rng(5).uniform(-40.0, 10.0, cfg.projector.memory)
    key = ("loaded", graph, n)
    if key not in _ref_cache:
        out = []
        exps = [ob.Experiment(spec, seed=int(s)) for s in seeds]
        for e in exps:
            e.set_weights(image)
        out.append([reference(e, spec, obs) for e in exps])
        for e in exps:
            e.run(6)
        out.append([reference(e, spec, obs) for e in exps])
        for e in exps:
            e.close()
        _ref_cache[key] = out
    want = _ref_cache[key]
    r = grlx.Runner(cfg, seeds)
    r.load_weights(image)
    check_queries(r, spec, obs, want[0], "loaded policy, before any launch")
    r.run(6); r.sync()
    check_queries(r, spec, obs, want[1], "loaded policy after 6 trials")
    r.close()


def test_a_sweep_context(grlx):
    """replicas that differ in alpha: each against an oracle of its own alpha; the query before the first launch does not count as a
    launch (set_replica_params is still allowed after it)"""
    n, alphas = 5, [0.05, 0.1, 0.2, 0.3, 0.15]

    def specs(spec):
        out = []
        for a in alphas:
            s = type(spec).from_buffer_copy(spec)
            s.alpha = a
            out.append(s)
        return out

    def prepare(r):
        r.query_q(np.zeros((1, 2)))
        r.set_replica_params(alpha=alphas)

    r = run_against_oracle(grlx, "pendulum_sarsa", n, (0, 6, 6), specs=specs, prepare=prepare, key=("sweep", n))[0]
    r.close()


# ---- 5: actor-critic ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["ac_twin", "ac_independent"])
def test_actor_critic(grlx, graph):
    """cart-pole, twin tables and test_actor_critic_with_different_tile_codings' configuration, 5 replicas, three launches: the critic's
    V(s), ActionPolicy::read and the clipped action against the oracle's dense tables"""
    run_against_oracle(grlx, graph, 5, (0, 4, 4, 4))[0].close()


# ---- 6: a query changes nothing ----------------------------------------------------------------------------------------------------
def every_query(r, spec, obs):
    if is_ac(spec):
        r.query_state(obs, 0); r.query_state(obs, 1); r.policy_action(obs)
        return
    r.query_q(obs); r.policy_action(obs); r.query_ensemble(obs); r.query_ensemble_raw(obs, 1)
    if spec.agent == ob.AGENT_QV:
        r.query_state(obs, 1)


@pytest.mark.parametrize("graph,tables,n_rng", [("pendulum_sarsa", 1, 3), ("qv", 2, 3), ("ac_twin", 2, 2)])
def test_a_query_changes_nothing(grlx, graph, tables, n_rng):
    """snapshot bytes and table_load before and after every kind of query; then 6 more trials: rows, streams, environment state and
    2000 sampled weights equal the oracle's uninterrupted run"""
    n = 3
    cfg, spec = build(grlx, graph, n)
    obs = observations(graph, spec)
    seeds = np.arange(SEED0, SEED0 + n)
    r = grlx.Runner(cfg, seeds)
    r.run(6); r.sync()
    before = r.snapshot()
    load = [[r.table_load(k, t) for t in range(tables)] for k in range(n)]
    every_query(r, spec, obs)
    assert r.snapshot() == before, "a query changed the context's snapshot"
    assert [[r.table_load(k, t) for t in range(tables)] for k in range(n)] == load
    r.run(6); r.sync()
    for k in range(n):
        want = oracle_run(spec, seeds[k], (("run", 6), ("run", 6)), cfg.projector.memory, tables=tuple(range(tables)))
        check_replica(r, k, want, f"{graph}: replica {k} after a query in between", cfg.projector.memory, n_rng=n_rng)
    r.close()


def test_grlx_read_does_create_the_entries_it_reads(grlx):
    """why the new path exists: the same look at the same observations through grlx_project + grlx_read changes table occupancy (and
    with it the next snapshot's bytes and the point at which the tables grow)"""
    graph, n = "pendulum_sarsa", 3
    cfg, spec = build(grlx, graph, n)
    obs = observations(graph, spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    before = r.snapshot()
    load = [r.table_load(k) for k in range(n)]
    rows = np.array([list(o) + [a] for o in obs for a in ref.actions_of(spec)])
    idx = grlx.runner.project(cfg.projector, rows)
    for k in range(n):
        r.read(np.full(rows.shape[0], k, np.int32), idx)
    assert all(r.table_load(k) > load[k] for k in range(n)), "grlx_read was expected to create entries"
    assert r.snapshot() != before
    r.close()


# ---- 7: ensemble -------------------------------------------------------------------------------------------------------------------
def test_ensemble(grlx):
    """8 replicas, groups of 4 and of 8: the raw sums against the helper's ascending-order loops over the ORACLE's values, and one group
    of all against the sums built from query_q's own outputs; a group size that does not divide is refused"""
    graph, n = "pendulum_sarsa", 8
    r, spec, obs, want = run_against_oracle(grlx, graph, n, (6,))
    oq, ov, og = (np.stack([w[k] for w in want[0]]) for k in ("q", "value", "greedy"))
    for gs in (4, 8):
        same_bits(r.query_ensemble_raw(obs, gs), ref.ensemble(oq, ov, og, gs), f"raw sums, groups of {gs}")
    q, value, greedy, _ = r.query_q(obs)
    same_bits(r.query_ensemble_raw(obs), ref.ensemble(q, value, greedy, n), "one group of all, from query_q's outputs")
    same_bits(r.query_ensemble_raw(obs, 2, replicas=range(2, 6)), ref.ensemble(q[2:6], value[2:6], greedy[2:6], 2), "a replica range")
    res = r.query_ensemble(obs, 4)
    raw = ref.ensemble(oq, ov, og, 4)
    same_bits(res.mean_value, raw[..., 0] / 4.0, "mean_value")
    same_bits(res.var_value, (raw[..., 1] - raw[..., 0] * raw[..., 0] / 4.0) / 3.0, "var_value")
    same_bits(res.votes, raw[..., 5:8].astype(np.int64), "votes")
    assert (res.votes.sum(axis=-1) == 4).all()
    for g in range(2):
        for o in range(obs.shape[0]):
            v = list(res.votes[g, o])
            assert res.majority[g, o] == v.index(max(v)), "majority: the lowest index wins a tie"
    with pytest.raises(grlx.capi.GrlxError) as ei:
        r.query_ensemble_raw(obs, 3)
    assert ei.value.code == grlx.capi.ERR_INVALID and "group_size" in str(ei.value)
    r.close()


# ---- 8: chunking -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum_q_five_actions", "qv"])
def test_chunked_staging_gives_the_same_outputs(grlx, graph):
    """a bound on the staging that forces at least 3 chunks at 5 replicas x 11 observations; also a bound below one observation (a chunk
    never has less than one)"""
    n = 5
    cfg, spec = build(grlx, graph, n)
    obs = observations(graph, spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    r.run(6); r.sync()
    lib = grlx.capi.load()

    def all_outputs():
        out = list(r.query_q(obs)) + [r.query_ensemble_raw(obs, 5), r.query_ensemble_raw(obs, 1)]
        if graph == "qv":
            out.append(r.query_state(obs, 1))
        return out

    whole = all_outputs()
    try:
        # one observation of the widest call (query_ensemble with groups of 1): 8 D + 5 (8 A + 16) + 5 (2 + 2 A) 8 bytes; four of them
        per_obs = 8 * 2 + n * (8 * spec.action_steps + 16) + n * (2 + 2 * spec.action_steps) * 8
        for bound in (4 * per_obs, 1):
            assert lib.grlx_set_query_chunk_bytes(bound) == 0
            for got, want, name in zip(all_outputs(), whole, ("q", "value", "greedy", "n_max", "ensemble", "ensemble of one", "state")):
                same_bits(got, want, f"{name} with staging bounded to {bound} bytes")
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    r.close()


# ---- 9: per-step contexts ----------------------------------------------------------------------------------------------------------
def from_own_weights(r, spec, obs, k):
    """the helper's formula on Runner.weights (grlx_get_weights) of the slots involved"""
    rows = [list(o) + [a] for o in obs for a in ref.actions_of(spec)]
    slots = np.unique(ob.tile_project(spec.projector, rows))
    w = dict(zip((int(s) for s in slots), r.weights(k, slots)))
    return ref.query_q(w, spec, obs)


@pytest.mark.parametrize("external", [False, True], ids=["own_environment", "external_environment"])
def test_contexts_driven_step_by_step(grlx, external):
    """after agent_start and two agent_step calls, in mid-episode: the query equals the formula on the context's own weights"""
    n = 3
    cfg, spec = build(grlx, "pendulum_sarsa", n)
    obs = observations("pendulum_sarsa", spec)
    env = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    if external:
        ext, _ = build(grlx, "pendulum_sarsa", n)
        ext.env = grlx.capi.ENV_EXTERNAL
        ext.control_step, ext.timeout, ext.integration_steps = 0.0, 0.0, 0
        agent = grlx.Runner(ext, np.arange(SEED0, SEED0 + n))
        assert agent.obs_dims == 2
    else:
        agent = env
    o = env.env_start(0)
    a = agent.agent_start(0, o)
    visited = [o.copy()]
    for _ in range(2):
        o, rew, term = env.env_advance(a)
        a = agent.agent_step(0, o, rew)
        visited.append(o.copy())
    at = np.concatenate([obs] + [v[:1] for v in visited])           # 14 rows: the set and what replica 0 just saw
    q, value, greedy, n_max = agent.query_q(at)
    for k in range(n):
        wq, wv, wg, wn = from_own_weights(agent, spec, at, k)
        same_bits(q[k], wq, f"replica {k}: q"); same_bits(value[k], wv, f"replica {k}: value")
        same_bits(greedy[k], wg, f"replica {k}: greedy"); same_bits(n_max[k], wn, f"replica {k}: n_max")
    o, rew, term = env.env_advance(a)                                # and the episode goes on
    agent.agent_step(0, o, rew)
    env.close()
    if external:
        agent.close()


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------
def refused(grlx, call, word):
    with pytest.raises(grlx.capi.GrlxError) as ei:
        call()
    assert ei.value.code == grlx.capi.ERR_INVALID and word in str(ei.value), str(ei.value)


def raw_query_q(grlx, r, obs, first, count):
    """grlx_query_q on outputs filled with a pattern: (status, outputs untouched?)"""
    import ctypes as C
    obs = np.ascontiguousarray(obs, np.float64)
    n, A = obs.shape[0], r.cfg.action_steps
    q = np.full((max(count, 1), n, A), 777.0); v = np.full((max(count, 1), n), 777.0)
    g = np.full((max(count, 1), n), 777, np.int32); m = np.full((max(count, 1), n), 777, np.int32)
    P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = r.lib.grlx_query_q(r._ctx, first, count, P(obs, C.c_double), n, P(q, C.c_double), P(v, C.c_double), P(g, C.c_int32), P(m, C.c_int32))
    return rc, bool((q == 777.0).all() and (v == 777.0).all() and (g == 777).all() and (m == 777).all())


def test_refusals(grlx):
    capi = grlx.capi
    cfg, spec = build(grlx, "pendulum_sarsa", 3)
    obs = observations("pendulum_sarsa", spec)
    r = grlx.Runner(cfg, [1, 2, 3])
    refused(grlx, lambda: r.query_state(obs, 0), "grlx_query_q")
    refused(grlx, lambda: r.query_state(obs, 1), "table")
    bad = obs.copy(); bad[4, 1] = np.nan
    refused(grlx, lambda: r.query_q(bad), "row 4, dimension 1")
    refused(grlx, lambda: r.query_q(bad), "not finite")
    bad[4, 1] = 0.0; bad[7, 0] = 1e300
    refused(grlx, lambda: r.query_q(bad), "row 7, dimension 0")
    refused(grlx, lambda: r.query_q(bad), "2^30")
    refused(grlx, lambda: r.query_ensemble_raw(bad), "row 7, dimension 0")
    refused(grlx, lambda: r.query_q(obs, replicas=(2, 2)), "replica range")
    refused(grlx, lambda: r.query_q(obs, replicas=(-1, 2)), "replica range")
    for o, first, count in ((bad, 0, 3), (obs, 2, 2)):
        rc, untouched = raw_query_q(grlx, r, o, first, count)
        assert rc == capi.ERR_INVALID and untouched, "a refused query wrote to its outputs"
    # nothing to do is no error, and nothing is written
    assert raw_query_q(grlx, r, obs[:0], 0, 3) == (0, True)
    assert raw_query_q(grlx, r, obs, 1, 0) == (0, True)
    r.close()

    safe, _ = build(grlx, "pendulum_sarsa", 3)
    safe.projector.safe = 1
    r = grlx.Runner(safe, [1, 2, 3])
    refused(grlx, lambda: r.query_q(obs), "safe")
    refused(grlx, lambda: r.query_q(obs), "not built")
    refused(grlx, lambda: r.query_ensemble_raw(obs), "not built")
    r.close()

    ac, acspec = build(grlx, "ac_twin", 3)
    r = grlx.Runner(ac, [1, 2, 3])
    aobs = np.zeros((3, 4))
    refused(grlx, lambda: r.query_ensemble_raw(aobs), "actor-critic")
    refused(grlx, lambda: r.query_q(aobs), "actor-critic")
    refused(grlx, lambda: r.query_state(aobs, 2), "table")
    r.close()


# ---- 11: the batch path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [8, 20])
def test_batch_path_query(grlx, hidden):
    """FqiRunner.query after 2 batches equals FqiExperiment.q (the oracle's normalisation + forward pass) for 3 replicas x the set x every
    action; chunked staging gives the same; the rows, parameters and streams of a third batch are those of a context never queried"""
    seeds, over = [1, 2, 3], dict(batch_size=300, iterations=2, epochs=6, hidden=hidden)
    _, pspec = build(grlx, "pendulum_sarsa", 1)
    obs = observations("pendulum_sarsa", pspec)
    cfg = grlx.pendulum_fqi_config(len(seeds), max_batches=3, **over)
    acts = [cfg.action_min + (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1) * k for k in range(cfg.action_steps)]
    key = ("fqi", hidden)
    if key not in _ref_cache:
        want = np.zeros((len(seeds), obs.shape[0], len(acts)))
        for k, s in enumerate(seeds):
            e = ob.FqiExperiment(ob.pendulum_fqi_spec(**over), seed=s)
            e.run_batch(); e.run_batch()
            for o in range(obs.shape[0]):
                for a, act in enumerate(acts):
                    want[k, o, a] = e.q(obs[o], act)
            e.close()
        _ref_cache[key] = want
    want = _ref_cache[key]
    r, plain = grlx.FqiRunner(cfg, seeds), grlx.FqiRunner(cfg, seeds)
    for x in (r, plain):
        x.run_batch(); x.run_batch(); x.sync()
    q = r.query(obs)
    same_bits(q, want, f"hidden = {hidden}: Q(s, a)")
    same_bits(r.query(obs, replicas=range(1, 3)), want[1:3], "a replica range")
    lib = grlx.capi.load()
    try:
        lib.grlx_set_query_chunk_bytes(4 * (16 + 8 * len(acts) * len(seeds)))
        same_bits(r.query(obs), want, "chunked staging")
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    bad = obs.copy(); bad[2, 1] = np.inf
    refused(grlx, lambda: r.query(bad), "row 2, dimension 1")
    refused(grlx, lambda: r.query(obs, replicas=(2, 2)), "replica range")
    for x in (r, plain):
        x.run_batch(); x.sync()
    for k in range(len(seeds)):
        same_bits(r.params(k), plain.params(k), f"replica {k}: parameters after a third batch")
        same_bits(r.rows(k, 3)[2], plain.rows(k, 3)[2], f"replica {k}: rows")
        assert r.info(k)["rng"] == plain.info(k)["rng"]
    r.close(); plain.close()


# ---- 12: grlxd -Q ------------------------------------------------------------------------------------------------------------------
def _policy_lines(path):
    return [ln.split() for ln in path.read_text().split("\n") if ln.strip()]


def _check_policy_block(lines, obs, res, g, lead, what):
    """the lines of one group against EnsembleResult res: numbers to a relative 1e-5 (the file prints 6 significant digits: half a unit
    of the sixth is 5e-6), votes and the majority action exactly"""
    actions = [-3.0, 0.0, 3.0]
    for o in range(obs.shape[0]):
        f = lines[o]
        assert len(f) == lead + 2 + 2 + 3 + 1, f"{what}: {f}"
        if lead:
            assert int(f[0]) == g
        np.testing.assert_allclose([float(x) for x in f[lead:lead + 2]], obs[o], rtol=1e-5, atol=0)
        sd = np.sqrt(max(res.var_value[g, o], 0.0))
        np.testing.assert_allclose(float(f[lead + 2]), res.mean_value[g, o], rtol=1e-5, atol=0, err_msg=f"{what}: mean of observation {o}")
        np.testing.assert_allclose(float(f[lead + 3]), sd, rtol=1e-5, atol=0, err_msg=f"{what}: standard deviation of observation {o}")
        assert [int(x) for x in f[lead + 4:lead + 7]] == list(res.votes[g, o]), f"{what}: votes of observation {o}"
        assert float(f[lead + 7]) == actions[res.majority[g, o]], f"{what}: majority action of observation {o}"


def test_grlxd_query(grlx, tmp_path):
    """golden pendulum yaml, -r 4 -t 12 -Q: <output>-0-policy.txt against Runner.query_ensemble on an identical context"""
    import os
    import subprocess
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")
    obs = np.array([[0.0, 0.0], [3.14, 1.5], [-1.0, 2.0], [7.9, -11.25], [0.5, 30.0]])
    (tmp_path / "obs.txt").write_text("# angle velocity\n" + "\n".join("%r %r" % (float(a), float(b)) for a, b in obs) + "\n")
    res = subprocess.run([grlxd, "-s", "5", "-r", "4", "-t", "12", "-q", "-Q", "obs.txt", yaml], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr + res.stdout
    cfg = grlx.pendulum_sarsa_config(4, max_rows=8)
    r = grlx.Runner(cfg, [5, 6, 7, 8])
    r.run(12); r.sync()
    want = r.query_ensemble(obs)
    lines = _policy_lines(tmp_path / "pendulum-sarsa-tc-0-policy.txt")
    assert len(lines) == obs.shape[0]
    _check_policy_block(lines, obs, want, 0, 0, "grlxd -Q")
    r.close()


def test_grlxd_query_of_a_sweep(grlx, tmp_path):
    """-p with two points x 2 repetitions: two blocks, the point's index first, the groups being the repetitions"""
    import os
    import subprocess
    from grl_amd import _build
    grlxd = _build.build_host()
    yaml = os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")
    obs = np.array([[0.0, 0.0], [3.14, 1.5], [-1.0, 2.0]])
    (tmp_path / "obs.txt").write_text("\n".join("%r %r" % (float(a), float(b)) for a, b in obs) + "\n")
    res = subprocess.run([grlxd, "-s", "5", "-r", "2", "-t", "220", "-q", "-p", "/experiment/agent/predictor/alpha=0.1,0.2", "-Q", "obs.txt", yaml],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr + res.stdout
    cfg = grlx.pendulum_sarsa_config(4, max_rows=32)
    r = grlx.Runner(cfg, [5, 6, 7, 8])
    r.set_replica_params(alpha=[0.1, 0.1, 0.2, 0.2])
    r.run(220); r.sync()
    want = r.query_ensemble(obs, 2)
    lines = _policy_lines(tmp_path / "pendulum-sarsa-tc-0-policy.txt")
    assert len(lines) == 2 * obs.shape[0]
    for g in range(2):
        _check_policy_block(lines[g * 3:(g + 1) * 3], obs, want, g, 1, f"point {g}")
    r.close()
