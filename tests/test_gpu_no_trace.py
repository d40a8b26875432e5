"""Plain contexts WITHOUT a trace (trace = GRLX_TRACE_NONE, what a yaml without a `trace:` block gives), in every kernel family that
accepts one, against the oracle: one scalar oracle run per replica, bit for bit -- trial and steps columns, returns and episode times,
the RNG positions, the environment state, 2000 random weight slots (both tables of a two-table agent) and r.sync(), which raises on
any sticky status bit.  grlx_set_replica_params is never called here.

Why a module of its own: without a trace the TD update stores the weight of project(s, a) straight into the table.  In the
deferred-update ordering that store comes after the loads of Q(s', .) were issued, and no trace entry hands the newer value to the
lane; p of consecutive steps is the same slot in a fifth to four fifths of all learning steps
(tests/test_oracle_no_trace.py measures it on these very graphs), so 22 trials meet the hazard hundreds of times per replica.
The contract under test is configuration -> result: no case asserts which instantiation ran, the messages name it.

Every replica is checked; the batches are ragged (a last wave with one live replica, a half-empty sub-batch) and the trials are
launched in two chunks, so that the state crosses a launch boundary.  Tolerance: 0 ulp."""
import os
import subprocess

import numpy as np
import pytest

from tests import configs
from tests import oracle_binding as ob
from tests.test_gpu_generic_paths import assert_bit_equal
from tests.test_gpu_sweep import check_replica, oracle_run

pytestmark = pytest.mark.gpu

MAKE = {"pendulum": configs.pendulum, "acrobot": configs.acrobot, "cart_pole_q": configs.cart_pole_q, "compass_walker": configs.compass_walker,
        "pendulum_qv": lambda g, n, agent=None, **o: configs.pendulum_qv(g, n, **o), "cart_pole_ac": lambda g, n, agent=None, **o: configs.cart_pole_ac(g, n, **o)}
KERNEL = {1: "generic", 2: "specialised", 3: "in place"}


def _set(obj, key, value):
    *path, leaf = key.split(".")
    for p in path:
        obj = getattr(obj, p)
    if isinstance(value, dict):                            # {index: value} of an array field
        for i, v in value.items():
            getattr(obj, leaf)[i] = v
    else:
        setattr(obj, leaf, value)


def build(grlx, graph, n, agent=0, rpw=4, both=None, **cfg_only):
    """(cfg, spec) of `graph` with trace = 0 on both sides; `both`: fields set on the two of them ("a.b" reaches into a member);
    cfg_only: fields of the grlx_config alone (layout, taps, force_generic)"""
    cfg, spec = MAKE[graph](grlx, n, agent=agent)
    cfg.replicas_per_wave = rpw
    for k, v in cfg_only.items():
        setattr(cfg, k, v)
    for k, v in dict(both or {}, trace=0).items():
        if k == "safe":
            cfg.projector.safe, spec.safe = v, v
            continue
        _set(cfg, k, v)
        _set(spec, k, v)
    spec.math = ob.MATH_PORTABLE
    assert cfg.trace == 0 and spec.trace == 0
    return cfg, spec


def plain_vs_oracle(grlx, graph, n, plan, agent=0, rpw=4, both=None, seed0=301, max_rows=None, **cfg_only):
    """A plain context of n replicas driven through `plan` (oracle_run's steps) against one oracle run per replica: every replica."""
    runs = sum(c[1] for c in plan if c[0] == "run")
    cfg, spec = build(grlx, graph, n, agent=agent, rpw=rpw, both=both, max_rows=max_rows or runs + 1, **cfg_only)
    two = graph in ("cart_pole_ac", "pendulum_qv")
    seeds = np.arange(seed0, seed0 + n)
    r = grlx.Runner(cfg, seeds)
    wanted = []
    for i, step in enumerate(plan):
        if step[0] == "run":
            r.run(step[1])
        elif step[0] == "steps":
            r.run_steps(100000, step[1])
        else:
            r.reset_run()
            continue
        if i + 1 < len(plan) and plan[i + 1][0] != "reset":
            continue
        # the end of a run (before a reset, or the end of the plan): everything against the oracle at that point
        r.sync()                                               # raises on any sticky status bit
        what = f"{graph} agent {agent}, asked for {rpw} replicas per wave, runs {r.replicas_per_wave()} ({KERNEL.get(r.last_kernel(), '?')} kernel, " \
               f"environment server {r.env_server_counts()}), plan {plan[:i + 1]}"
        for k in range(n):
            want = oracle_run(spec, seeds[k], tuple(plan[:i + 1]), cfg.projector.memory, tables=(0, 1) if two else (0,))
            check_replica(r, k, want, f"{what}: replica {k} of {n}", cfg.projector.memory, n_rng=2 if graph == "cart_pole_ac" else 3)
            wanted.append(want)
    r.close()
    return wanted


def chunks(trials):
    return (("run", trials // 3), ("run", trials - trials // 3))


# ---- A: the TD agents, four replicas per wave ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("server", ["server", "no_server"])
@pytest.mark.parametrize("agent", [0, 1, 3])
def test_pendulum_four_per_wave(grlx, monkeypatch, agent, server):
    """SARSA, Q, Expected SARSA; 13 replicas (the last wave holds one), 33 trials as 10 + 23; with the environment server allowed
    (the default) and with GRLX_ENV_SERVER=0."""
    if server == "no_server":
        monkeypatch.setenv("GRLX_ENV_SERVER", "0")
    plain_vs_oracle(grlx, "pendulum", 13, (("run", 10), ("run", 23)), agent=agent, rpw=4)


@pytest.mark.parametrize("rpw", [4, 8])
def test_pendulum_five_actions(grlx, rpw):
    plain_vs_oracle(grlx, "pendulum", 11, chunks(22), agent=0, rpw=rpw, both=dict(action_steps=5))


@pytest.mark.parametrize("graph,n,trials", [("acrobot", 13, 44), ("cart_pole_q", 9, 22), ("compass_walker", 11, 22)])
def test_acrobot_cart_pole_walker_four_per_wave(grlx, graph, n, trials):
    plain_vs_oracle(grlx, graph, n, chunks(trials), agent=1, rpw=4)


# ---- B: the TD agents, wide waves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,agent,n,trials,rpw", [("pendulum", 0, 21, 22, 8), ("cart_pole_q", 1, 9, 22, 8), ("compass_walker", 1, 11, 22, 8),
                                                      ("acrobot", 1, 19, 22, 16), ("compass_walker", 1, 21, 22, 16), ("compass_walker", 1, 37, 22, 32)])
def test_wide_layouts(grlx, graph, agent, n, trials, rpw):
    """8, 16 and 32 replicas per wave as asked for; what the context runs instead, if anything, is in the message."""
    plain_vs_oracle(grlx, graph, n, chunks(trials), agent=agent, rpw=rpw)


@pytest.mark.parametrize("server", ["server", "no_server"])
def test_acrobot_eight_per_wave(grlx, monkeypatch, server):
    """the layout the wide kernels' environment server works for, with the server allowed and without"""
    if server == "no_server":
        monkeypatch.setenv("GRLX_ENV_SERVER", "0")
    plain_vs_oracle(grlx, "acrobot", 13, chunks(44), agent=1, rpw=8)


# ---- C: the slow paths of the update ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpw", [4, 8])
def test_tiny_memory(grlx, rpw):
    """2048 slots: nearly every slot is shared between tilings, the write-through and reload branches run on every pass"""
    plain_vs_oracle(grlx, "pendulum", 5, chunks(22), agent=0, rpw=rpw, both={"projector.memory": 2048})


@pytest.mark.parametrize("rpw", [4, 8])
@pytest.mark.parametrize("name,both,n,trials", [
    ("limits", {"representation.output_min": -60.0, "representation.output_max": 0.5}, 5, 22),                       # clamped reads AND weights
    ("limits_reads_only", {"representation.output_min": -60.0, "representation.output_max": 0.5, "representation.limit": 0}, 5, 22),
    ("epsilon_decay", dict(decay_rate=0.99, decay_min=0.1), 5, 22),
    ("row_every_trial", dict(test_interval=-1), 5, 22),
    ("seven_step_episodes", dict(timeout=0.2), 7, 44),       # as test_passes_without_eviction_on_a_ragged_batch
])
def test_generic_parameters(grlx, name, both, n, trials, rpw):
    plain_vs_oracle(grlx, "pendulum", n, chunks(trials), agent=0, rpw=rpw, both=both)


@pytest.mark.parametrize("rpw", [4, 8])
def test_force_generic(grlx, rpw):
    plain_vs_oracle(grlx, "pendulum", 5, chunks(22), agent=1, rpw=rpw, force_generic=1)


# ---- D: actor-critic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rpw,n,method", [(4, 13, 0), (4, 13, 1), (8, 13, 0), (12, 13, 0), (16, 19, 0)])
def test_actor_critic(grlx, rpw, n, method):
    """cfg/cart_pole/ac_tc.yaml without the critic's trace, in every layout a context may ask for; both actor update methods; critic
    and actor table."""
    both = dict(ac_update_method=1, ac_step_limit=0.5, end_stop_penalty=1) if method else {}
    plain_vs_oracle(grlx, "cart_pole_ac", n, (("run", 7), ("run", 15)), rpw=rpw, both=both, seed0=201)


@pytest.mark.parametrize("rpw", [4, 8])
def test_actor_critic_with_different_tile_codings(grlx, rpw):
    """another resolution and memory for the critic: two independent tables (the kernels' non-twin path)"""
    both = {"projector.memory": 4194304, "projector.resolution": {0: 1.25, 2: 5.0}, "end_stop_penalty": 1}
    plain_vs_oracle(grlx, "cart_pole_ac", 13, (("run", 7), ("run", 15)), rpw=rpw, both=both, seed0=3)


# ---- E: the other families ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,graph,agent,both", [
    ("target_hard", "pendulum", 0, {"target_interval": 5, "target_tau": 1.0, "projector.memory": 65536}),
    ("target_polyak", "pendulum", 1, {"target_interval": 5, "target_tau": 0.5, "projector.memory": 65536}),
    ("target_hard_acrobot", "acrobot", 1, {"target_interval": 5, "target_tau": 1.0, "projector.memory": 65536}),
    ("target_polyak_acrobot", "acrobot", 1, {"target_interval": 5, "target_tau": 0.5, "projector.memory": 65536}),
    ("safe_1", "pendulum", 0, dict(safe=1)),
    ("safe_2", "pendulum", 0, dict(safe=2)),
    ("safe_1_target", "pendulum", 1, {"safe": 1, "target_interval": 5, "target_tau": 0.5, "projector.memory": 65536}),
    ("qv", "pendulum_qv", 0, {}),
    ("advantage", "pendulum", 4, dict(kappa=0.2)),
    ("advantage_acrobot", "acrobot", 4, dict(kappa=0.2)),
])
def test_other_families(grlx, name, graph, agent, both):
    """target networks (an interval of 5 update() calls: a synchronisation every fifth step), the claim table, QV (Q and V table),
    advantage learning; 5 replicas, 22 trials.  The target cases use a 65536-slot memory: a synchronisation runs over the whole
    parameter vector (representation.h:284-296), every fifth step, and the oracle does that on the CPU."""
    plain_vs_oracle(grlx, graph, 5, chunks(22), agent=agent, rpw=4, both=both)


# ---- F: step by step ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [1, 0], ids=["production_ordering", "in_place"])
@pytest.mark.parametrize("graph,agent,memory", [("pendulum", 0, 8388608), ("pendulum", 1, 8388608), ("pendulum", 0, 2048), ("acrobot", 1, 8388608)])
def test_step_by_step(grlx, graph, agent, memory, deferred):
    """test_production_ordering_step_by_step's recipe without a trace: every field of every step of replica 4 (tile indices, Q-values,
    action, reward, TD error, a trace length of 0); the first stale step is named.  tap_deferred = 0: the in-place instantiation."""
    from tests.test_gpu_parity import _compare_taps
    seeds, cap = [41, 42, 43, 44, 45, 46], 2600
    cfg, spec = build(grlx, graph, len(seeds), agent=agent, both={"projector.memory": memory}, tap_replica=4, tap_capacity=cap, tap_deferred=deferred)
    r = grlx.Runner(cfg, seeds)
    r.run(12); r.run(11); r.sync()
    what = f"{graph} agent {agent} memory {memory}, {KERNEL.get(r.last_kernel(), '?')} kernel"
    e = ob.Experiment(spec, seed=seeds[4])
    rows, otaps = e.run(23, tap_cap=cap)
    gtaps = r.taps()
    assert len(gtaps) == len(otaps) and len(otaps) > 100, what
    D = 2 if graph == "pendulum" else 4
    for k, (gt, ot) in enumerate(zip(gtaps, otaps)):
        try:
            assert gt.trace_len == 0 and ot.trace_len == 0, f"trace lengths {gt.trace_len}, {ot.trace_len}"
            _compare_taps(gt, ot, A=3, D=D)
        except AssertionError as ex:
            raise AssertionError(f"{what}: step {k}: {ex}")
    want = oracle_run(spec, seeds[4], (("run", 23),), memory)
    check_replica(r, 4, want, what + ": replica 4", memory)
    e.close()
    r.close()


# ---- G: the per-step entries --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum", "cart_pole_ac"])
def test_per_step_entries(grlx, graph):
    """grlx_agent_start / _step / _end of a context without a trace beside the ORACLE's environments on the host, against the oracle's
    own run and against Experiment.agent_start / agent_step / agent_end driven the same way: 3 replicas, 2 episodes."""
    from tests.test_gpu_step_api import GpuAgent, HostLoop, OracleAgent, OracleEnv, assert_rows_equal, touched_slots
    seeds, trials = [3, 4, 5], 2
    n = len(seeds)
    cfg, spec = build(grlx, graph, n)
    tables = (0, 1) if graph == "cart_pole_ac" else (0,)
    stepped = grlx.Runner(cfg, seeds)
    envs = [ob.Experiment(spec, seed=s) for s in seeds]
    loop = HostLoop(n, cfg.test_interval, OracleEnv(envs, stepped.obs_dims), GpuAgent(stepped))
    loop.run(trials)
    envs2 = [ob.Experiment(spec, seed=s) for s in seeds]
    agents2 = [ob.Experiment(spec, seed=s) for s in seeds]
    loop2 = HostLoop(n, cfg.test_interval, OracleEnv(envs2, stepped.obs_dims), OracleAgent(agents2))
    loop2.run(trials)
    for k in range(n):
        fresh = ob.Experiment(spec, seed=seeds[k])
        assert_rows_equal(loop.rows[k], loop2.rows[k], f"{graph} replica {k}")
        g, o = stepped.rng(k), agents2[k].rng()
        assert (g[0], g[2]) == (o[0], o[2]) if graph == "pendulum" else list(g)[:2] == list(o)[:2], f"replica {k}: the agent's streams"
        for t in tables:
            sl = touched_slots(agents2[k], fresh, t)
            assert sl.size > 50
            assert_bit_equal(stepped.weights(k, sl, table=t), agents2[k].weights(sl, table=t), f"{graph} replica {k}: table {t}")
        fresh.close()
    if graph == "pendulum":                                    # agent and environment have streams of their own: the oracle's whole run
        whole = ob.Experiment(spec, seed=seeds[1]); fresh = ob.Experiment(spec, seed=seeds[1])
        want_rows, _ = whole.run(trials)
        assert_rows_equal(loop.rows[1], [(x.trial, x.steps, x.reward, x.time) for x in want_rows], "against the oracle's own run")
        sl = touched_slots(whole, fresh)
        assert_bit_equal(stepped.weights(1, sl), whole.weights(sl), "weights against the oracle's own run")
        whole.close(); fresh.close()
    for e in envs + envs2 + agents2:
        e.close()
    stepped.close()


# ---- H: the edges of the experiment loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph,agent,n,rpw,trials", [("pendulum", 0, 7, 4, 22), ("acrobot", 1, 9, 8, 22)])
def test_reset_run_then_a_second_run(grlx, graph, agent, n, rpw, trials):
    plain_vs_oracle(grlx, graph, n, (("run", trials), ("reset",), ("run", trials)), agent=agent, rpw=rpw, seed0=501)


@pytest.mark.parametrize("graph,agent,n,rpw,budget", [("pendulum", 0, 7, 4, 1500), ("acrobot", 1, 9, 8, 2500)])
def test_steps_budget_with_three_test_episodes(grlx, graph, agent, n, rpw, budget):
    plain_vs_oracle(grlx, graph, n, (("run", 5), ("steps", budget)), agent=agent, rpw=rpw, both=dict(test_trials=3), seed0=601, max_rows=400)


# ---- I: a plain context is a sweep whose records all hold the configuration's values --------------------------------------------------
@pytest.mark.parametrize("rpw", [4, 8])
def test_plain_equals_uniform_sweep(grlx, rpw):
    """test_uniform_sweep_equals_the_generic_kernel without a trace and without force_generic"""
    n, trials = 10, 33
    seeds = np.arange(41, 41 + n)
    got, what = [], []
    slots = np.random.default_rng(3).integers(0, 8388608, 2000).astype(np.uint32)
    for sweep in (True, False):
        cfg = grlx.pendulum_sarsa_config(n, trace=0, replicas_per_wave=rpw, max_rows=trials + 1)
        r = grlx.Runner(cfg, seeds)
        if sweep:
            r.set_replica_params(alpha=[cfg.alpha] * n, gamma=[cfg.gamma] * n, lambda_=[cfg.lambda_] * n, epsilon=[cfg.epsilon] * n)
        else:
            p = r.replica_params()                             # before any set: the configuration's values
            assert (p["alpha"] == 0.2).all() and (p["gamma"] == 0.97).all() and (p["lambda_"] == 0.65).all() and (p["epsilon"] == 0.05).all()
        r.run(10); r.run(trials - 10); r.sync()
        what.append(f"{'sweep' if sweep else 'plain'}: {r.replicas_per_wave()} per wave, {KERNEL.get(r.last_kernel(), '?')} kernel, server {r.env_server_counts()}")
        got.append([(r.rows(k), r.row_times(k), list(r.rng(k)), r.env_state(k), r.weights(k, slots)) for k in range(n)])
        r.close()
    for k in range(n):
        (a_rows, a_t, a_rng, a_x, a_w), (b_rows, b_t, b_rng, b_x, b_w) = got[0][k], got[1][k]
        assert list(a_rows[0]) == list(b_rows[0]) and list(a_rows[1]) == list(b_rows[1]), f"{what}: replica {k}"
        assert_bit_equal(a_rows[2], b_rows[2], f"{what}: returns of replica {k}")
        assert_bit_equal(a_t, b_t, f"{what}: episode times of replica {k}")
        assert a_rng == b_rng, f"{what}: streams of replica {k}"
        assert_bit_equal(a_x, b_x, f"{what}: env state of replica {k}")
        assert_bit_equal(a_w, b_w, f"{what}: weights of replica {k}")


def test_the_layout_reported_is_the_layout_that_runs(grlx):
    """16384 acrobots choose 16 replicas per wave by themselves, 32768 walkers 32, 16384 cart-pole actor-critics 16; without a trace
    the context runs -- and reports -- a layout that is built for it, and a replica of it still equals the oracle (one trial)."""
    for graph, n, with_trace in (("acrobot", 16384, 16), ("compass_walker", 32768, 32), ("cart_pole_ac", 16384, 16)):
        cfg, spec = build(grlx, graph, n, agent=1, rpw=0, table_log2_capacity=16, max_rows=2)
        seeds = np.arange(1, n + 1)
        cfg.trace = 1
        t = grlx.Runner(cfg, seeds); assert t.replicas_per_wave() == with_trace; t.close()
        cfg.trace = 0
        r = grlx.Runner(cfg, seeds)
        rpw = r.replicas_per_wave()
        assert rpw in (4, 8), f"{graph}: {rpw} replicas per wave without a trace"
        r.run(1); r.sync()
        assert r.replicas_per_wave() == rpw
        for k in (0, n - 1):
            want = oracle_run(spec, seeds[k], (("run", 1),), cfg.projector.memory)
            check_replica(r, k, want, f"{graph}, {rpw} per wave: replica {k}", cfg.projector.memory, n_rng=2 if graph == "cart_pole_ac" else 3)
        r.close()


def test_stamps_of_the_production_ordering_are_refused(grlx):
    """grlx_set_diag(2) stamps the deferred-update instantiation as it is, which is not built for a context without a trace: refused
    with the alternative named; the in-place stamps (1) run and equal the oracle."""
    n, trials = 5, 11
    cfg, spec = build(grlx, "pendulum", n, agent=0, max_rows=trials + 1)
    seeds = np.arange(71, 71 + n)
    r = grlx.Runner(cfg, seeds)
    with pytest.raises(grlx.capi.GrlxError) as ei:
        grlx.capi.check(r.lib.grlx_set_diag(r._ctx, 2))
    assert ei.value.code == grlx.capi.ERR_INVALID and "without a trace" in str(ei.value) and "grlx_set_diag 1" in str(ei.value)
    r.set_diag(True)
    r.run(trials); r.sync()
    for k in range(n):
        check_replica(r, k, oracle_run(spec, seeds[k], (("run", trials),), cfg.projector.memory), f"in-place stamps: replica {k}", cfg.projector.memory)
    r.close()


# ---- J: the deployer ----------------------------------------------------------------------------------------------------------------
def test_deployer_yaml_without_a_trace_block(grlx, tmp_path):
    """the reference's golden yaml with the predictor's `trace:` block removed: `grlxd -s 1 -r 5 -t 33` runs five clones without a
    trace; clone 0's file is the oracle's rows (trace = 0, seed 1) as Experiment.format_rows writes them"""
    from grl_amd import _build
    grlxd = _build.build_host()
    text = open(os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")).read()
    block = "      trace:\n        type: trace/enumerated/replacing\n"
    assert text.count(block) == 1
    y = tmp_path / "pendulum-sarsa-tc.yaml"
    y.write_text(text.replace(block, ""))
    res = subprocess.run([grlxd, "-s", "1", "-r", "5", "-t", "33", "-l", "-q", str(y)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr + res.stdout
    e = ob.Experiment(ob.pendulum_sarsa_spec(trace=0), seed=1)
    rows, _ = e.run(33)
    with_trace = ob.Experiment(ob.pendulum_sarsa_spec(), seed=1)
    assert e.format_rows(rows) != with_trace.format_rows(with_trace.run(33)[0])
    assert (tmp_path / "pendulum-sarsa-tc-0@0.txt").read_text() == e.format_rows(rows)
    assert (tmp_path / "pendulum-sarsa-tc-0@4.txt").exists() and not (tmp_path / "pendulum-sarsa-tc-0@5.txt").exists()
    e.close(); with_trace.close()
