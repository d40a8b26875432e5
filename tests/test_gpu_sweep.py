"""Per-replica learning parameters (grlx_set_replica_params): a hyper-parameter sweep as the replicas of ONE context.

The specification is the oracle, unchanged: one orc_create per replica with that replica's alpha / gamma / lambda / epsilon
and seed.  Every comparison is bit for bit, as in test_gpu_generic_paths._run_both: trial and steps columns, returns and
episode times, the first three RNG positions, the environment state and 2000 random weight slots.  The kernels are the
SpecSweep instantiations of rollout_kernel (4 replicas per wave) and rollout_wide_kernel (8): the four values are per-lane
data there, the replicas of a wave differ."""
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import configs
from tests import oracle_binding as ob
from tests.test_gpu_generic_paths import assert_bit_equal

pytestmark = pytest.mark.gpu

ALPHAS = (0.05, 0.1, 0.2, 0.25)
GAMMAS = (0.9, 0.95, 0.97)
LAMBDAS = (0.4, 0.5, 0.65)          # the largest gamma * lambda is 0.97 * 0.65 = 0.6305; 0.6305^10 < 0.01: inside kMaxTrace = 10
EPSILONS = (0.01, 0.05, 0.2)
COMBOS = list(itertools.product(ALPHAS, GAMMAS, LAMBDAS, EPSILONS))       # 108
YAML = os.path.join(os.path.dirname(__file__), "golden", "pendulum-sarsa-tc.yaml")
ALPHA_PATH = "/experiment/agent/predictor/alpha"
EPSILON_PATH = "/experiment/agent/policy/sampler/epsilon"


def combos(n, offset=7):
    """n different (alpha, gamma, lambda, epsilon): a stride coprime with 108 through the product of the four value sets"""
    assert n <= len(COMBOS)
    picked = [COMBOS[(offset + 29 * k) % len(COMBOS)] for k in range(n)]
    assert len(set(picked)) == n
    return dict(alpha=[c[0] for c in picked], gamma=[c[1] for c in picked], lambda_=[c[2] for c in picked], epsilon=[c[3] for c in picked])


def replica_spec(spec, params, k):
    s = type(spec).from_buffer_copy(spec)
    s.alpha, s.gamma, s.lambda_, s.epsilon = (params[name][k] for name in ("alpha", "gamma", "lambda_", "epsilon"))
    s.math = ob.MATH_PORTABLE
    return s


_oracle_cache = {}      # every test runs clean and poisoned: the oracle's half is computed once


def oracle_run(spec, seed, plan, memory, tables=(0,)):
    """plan: a tuple of ("run", trials) | ("steps", budget) | ("reset",) applied in order; returns the rows of every run segment
    (a list per reset-separated run), the RNG positions, the environment state, the weight slots and their values (`w`: table 0;
    `w1`: the second table of a two-table agent, when `tables` names it)"""
    key = (bytes(spec), int(seed), plan, int(memory), tuple(tables))
    if key not in _oracle_cache:
        e = ob.Experiment(spec, seed=int(seed))
        runs = [[]]
        for step in plan:
            if step[0] == "run":
                runs[-1] += e.run(step[1])[0]
            elif step[0] == "steps":
                e.set_steps_budget(step[1])
                runs[-1] += e.run(100000)[0]
            else:
                e.reset_run()
                runs.append([])
        slots = np.random.default_rng(11).integers(0, memory, 2000).astype(np.uint32)
        rows = [[(x.trial, x.steps, x.reward, x.time) for x in run] for run in runs]
        _oracle_cache[key] = dict(rows=rows, rng=list(e.rng())[:3], state=np.array(e.state()), slots=slots, w=np.array(e.weights(slots)))
        for t in tables:
            if t != 0:
                _oracle_cache[key]["w%d" % t] = np.array(e.weights(slots, table=t))
        e.close()
    return _oracle_cache[key]


def check_replica(r, k, want, what, memory, n_rng=3):
    """the last run of `want` against the rows the context holds now; streams, state and weights (of every table `want` holds) against
    the oracle's end.  n_rng: the streams the graph has (the actor-critic graph has no samplers: 2)"""
    rows = want["rows"][-1]
    t, s, rew = r.rows(k)
    assert len(rows) == r.replica_rows(k), f"{what}: row count"
    assert list(t) == [x[0] for x in rows], f"{what}: trial column"
    assert list(s) == [x[1] for x in rows], f"{what}: steps column"
    assert_bit_equal(rew, [x[2] for x in rows], f"{what}: returns")
    assert_bit_equal(r.row_times(k, 0, len(rows)), [x[3] for x in rows], f"{what}: episode times")
    assert list(r.rng(k))[:n_rng] == want["rng"][:n_rng], f"{what}: RNG positions"
    assert_bit_equal(r.env_state(k), want["state"], f"{what}: env state")
    assert_bit_equal(r.weights(k, want["slots"]), want["w"], f"{what}: weights")
    if "w1" in want:
        assert_bit_equal(r.weights(k, want["slots"], 1), want["w1"], f"{what}: weights of the second table")


def sweep_vs_oracle(grlx, make, n, chunks, rpw, seeds=None, params=None, **over):
    """A sweep context of n replicas, each with its own combination, against one oracle per replica."""
    trials = sum(chunks)
    cfg, spec = make(grlx, n, replicas_per_wave=rpw, max_rows=trials + 1, **over)
    for k, v in over.items():
        if k in ("trace", "action_steps", "test_trials", "test_interval"):
            setattr(spec, k, v)
    seeds = np.arange(301, 301 + n) if seeds is None else np.asarray(seeds)
    params = params or combos(n)
    r = grlx.Runner(cfg, seeds)
    r.set_replica_params(**params)
    assert r.replicas_per_wave() == rpw
    got = r.replica_params()
    for name in params:
        assert_bit_equal(got[name], params[name], f"replica_params {name}")
    for c in chunks:
        r.run(c)
    r.sync()                                                   # raises on any sticky status bit
    assert r.last_kernel() == 1                                # GRLX_KERNEL_GENERIC
    assert r.env_server_counts() == (0, 0)
    rows = []
    for k in range(n):
        want = oracle_run(replica_spec(spec, params, k), seeds[k], tuple(("run", c) for c in chunks), cfg.projector.memory)
        check_replica(r, k, want, f"replica {k} {[params[p][k] for p in params]}", cfg.projector.memory)
        rows.append(want["rows"][-1])
    r.close()
    return rows


# ---- 1 .. 4: every environment and both layouts -----------------------------------------------------------------------------------
def test_pendulum_sarsa_ragged_wave_two_launches(grlx):
    """13 replicas, 4 per wave (the last wave holds one replica and three dead groups), 33 trials launched as 10 + 23."""
    sweep_vs_oracle(grlx, lambda g, k, **o: configs.pendulum(g, k, agent=0, **o), 13, [10, 23], 4)


@pytest.mark.parametrize("agent", [1, 3])
def test_pendulum_q_and_expected_sarsa_wide(grlx, agent):
    """21 replicas, 8 per wave, 22 trials.  Expected SARSA: the replica's epsilon is inside the target (the weights 1 - de and de / NA)."""
    sweep_vs_oracle(grlx, lambda g, k, **o: configs.pendulum(g, k, agent=agent, **o), 21, [22], 8)


@pytest.mark.parametrize("rpw", [4, 8])
@pytest.mark.parametrize("over", [dict(action_steps=5), dict(trace=0)], ids=["five_actions", "no_trace"])
def test_pendulum_five_actions_and_no_trace(grlx, rpw, over):
    """The other action count, and a context without a trace.  Without a trace the deferred update stores p's weight straight into
    the table, behind the loads of Q(s', .) that are already in flight, and no trace entry forwards it: the sweep kernels load the
    weights again after such an update (p of consecutive steps is often the same slot on the pendulum)."""
    sweep_vs_oracle(grlx, lambda g, k, **o: configs.pendulum(g, k, agent=0, **o), 11, [22], rpw, **over)


@pytest.mark.parametrize("rpw", [4, 8])
@pytest.mark.parametrize("name,n,trials", [("acrobot", 13, 44), ("cart_pole_q", 9, 22), ("compass_walker", 11, 22)])
def test_acrobot_cart_pole_walker_q(grlx, name, n, trials, rpw):
    """Q-learning with the trial counts of test_wide_waves_bit_exact (acrobot 44, walker 22; the cart-pole, which that test does not
    run, as the walker): episodes end at different steps inside a wave, and the wide kernel's sub-batches take turns with different
    parameters."""
    make = {"acrobot": configs.acrobot, "cart_pole_q": configs.cart_pole_q, "compass_walker": configs.compass_walker}[name]
    sweep_vs_oracle(grlx, lambda g, k, **o: make(g, k, agent=1, **o), n, [trials // 3, trials - trials // 3], rpw)


# ---- 5: the comparison tells a sweep from a shared value --------------------------------------------------------------------------
@pytest.mark.parametrize("rpw", [4, 8])
def test_equal_seeds_different_parameters(grlx, rpw):
    n = 9
    rows = sweep_vs_oracle(grlx, lambda g, k, **o: configs.pendulum(g, k, agent=0, **o), n, [33], rpw, seeds=[77] * n)
    assert sum(rows[k] != rows[0] for k in range(1, n)) >= 1                     # same seed, different parameters: the rows differ


# ---- 6: a uniform sweep is the plain generic context ------------------------------------------------------------------------------
@pytest.mark.parametrize("rpw", [4, 8])
def test_uniform_sweep_equals_the_generic_kernel(grlx, rpw):
    n, trials = 10, 33
    seeds = np.arange(41, 41 + n)
    got = []
    slots = np.random.default_rng(3).integers(0, 8388608, 2000).astype(np.uint32)
    for sweep in (True, False):
        cfg = grlx.pendulum_sarsa_config(n, force_generic=1, replicas_per_wave=rpw, max_rows=trials + 1)
        r = grlx.Runner(cfg, seeds)
        if sweep:
            r.set_replica_params(alpha=[cfg.alpha] * n, gamma=[cfg.gamma] * n, lambda_=[cfg.lambda_] * n, epsilon=[cfg.epsilon] * n)
        else:
            p = r.replica_params()                             # before any set: the configuration's values
            assert (p["alpha"] == 0.2).all() and (p["gamma"] == 0.97).all() and (p["lambda_"] == 0.65).all() and (p["epsilon"] == 0.05).all()
        r.run(trials); r.sync()
        assert r.last_kernel() == 1
        got.append([(r.rows(k), r.row_times(k), list(r.rng(k)), r.env_state(k), r.weights(k, slots)) for k in range(n)])
        r.close()
    for k in range(n):
        (a_rows, a_t, a_rng, a_x, a_w), (b_rows, b_t, b_rng, b_x, b_w) = got[0][k], got[1][k]
        assert list(a_rows[0]) == list(b_rows[0]) and list(a_rows[1]) == list(b_rows[1])
        assert_bit_equal(a_rows[2], b_rows[2], f"returns of replica {k}")
        assert_bit_equal(a_t, b_t, f"episode times of replica {k}")
        assert a_rng == b_rng
        assert_bit_equal(a_x, b_x, f"env state of replica {k}")
        assert_bit_equal(a_w, b_w, f"weights of replica {k}")


# ---- 7: the parameters persist across reset_run -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rpw", [4, 8])
def test_reset_run_keeps_the_parameters(grlx, rpw):
    n, trials = 7, 22
    cfg, spec = configs.pendulum(grlx, n, agent=1, replicas_per_wave=rpw, max_rows=trials + 1)
    seeds = np.arange(501, 501 + n)
    params = combos(n, offset=40)
    r = grlx.Runner(cfg, seeds)
    r.set_replica_params(**params)
    plan = (("run", trials),)
    r.run(trials); r.sync()
    for k in range(n):
        check_replica(r, k, oracle_run(replica_spec(spec, params, k), seeds[k], plan, cfg.projector.memory), f"run 0, replica {k}", cfg.projector.memory)
    r.reset_run()
    got = r.replica_params()
    for name in params:
        assert_bit_equal(got[name], params[name], f"replica_params {name} after reset_run")
    with pytest.raises(grlx.capi.GrlxError) as ei:             # still after the first launch
        r.set_replica_params(alpha=[0.1] * n)
    assert ei.value.code == grlx.capi.ERR_INVALID and "first launch" in str(ei.value)
    plan = (("run", trials), ("reset",), ("run", trials))
    r.run(trials); r.sync()
    for k in range(n):
        check_replica(r, k, oracle_run(replica_spec(spec, params, k), seeds[k], plan, cfg.projector.memory), f"run 1, replica {k}", cfg.projector.memory)
    r.close()


# ---- 8: a steps budget, test trials of three episodes -----------------------------------------------------------------------------
@pytest.mark.parametrize("rpw", [4, 8])
def test_run_steps_with_three_test_episodes(grlx, rpw):
    n = 9
    cfg, spec = configs.acrobot(grlx, n, agent=1, replicas_per_wave=rpw, max_rows=400, test_trials=3)
    spec.test_trials = 3
    seeds = np.arange(601, 601 + n)
    params = combos(n, offset=3)
    r = grlx.Runner(cfg, seeds)
    r.set_replica_params(**params)
    r.run(5)
    r.run_steps(100000, 2500)
    r.sync()
    plan = (("run", 5), ("steps", 2500))
    n_rows = set()
    for k in range(n):
        want = oracle_run(replica_spec(spec, params, k), seeds[k], plan, cfg.projector.memory)
        check_replica(r, k, want, f"replica {k}", cfg.projector.memory)
        n_rows.add(len(want["rows"][-1]))
    assert len(n_rows) > 1                                     # the replicas stopped at trials of their own
    r.close()


# ---- 9: what is refused -----------------------------------------------------------------------------------------------------------
def _refused(grlx, call, word):
    with pytest.raises(grlx.capi.GrlxError) as ei:
        call()
    assert ei.value.code == grlx.capi.ERR_INVALID and word in str(ei.value), str(ei.value)


def test_values_are_validated_and_nothing_is_partly_applied(grlx):
    n = 6
    r = grlx.Runner(grlx.pendulum_sarsa_config(n), np.arange(n))
    _refused(grlx, lambda: r.set_replica_params(alpha=[0.1, 0.2, float("nan"), 0.1, 0.1, 0.1]), "replica 2")
    _refused(grlx, lambda: r.set_replica_params(epsilon=[0.1, float("inf"), 0.1, 0.1, 0.1, 0.1]), "replica 1")
    _refused(grlx, lambda: r.set_replica_params(gamma=[0.9] * 5 + [0.0]), "(0,1)")           # gamma * lambda = 0 with a replacing trace
    _refused(grlx, lambda: r.set_replica_params(gamma=[0.9] * 5 + [0.0]), "replica 5")
    p = r.replica_params()                                     # every refusal left the configuration's values
    assert (p["alpha"] == 0.2).all() and (p["gamma"] == 0.97).all() and (p["lambda_"] == 0.65).all() and (p["epsilon"] == 0.05).all()
    r.run(1); r.sync()                                         # not a sweep context: the usual kernel
    assert r.last_kernel() == 2
    r.close()


def test_trace_rule_per_replica(grlx):
    """gamma = 0.99 with lambda = 0.8: 0.792^10 = 0.097 >= 0.01, the trace would need more than kMaxTrace entries -- refused for the
    one replica that has it, with its index and value, and all four parameters stay as they were before the call."""
    n = 5
    r = grlx.Runner(grlx.pendulum_sarsa_config(n), np.arange(n))
    r.set_replica_params(lambda_=[0.4, 0.5, 0.65, 0.5, 0.4])
    before = r.replica_params()
    with pytest.raises(grlx.capi.GrlxError) as ei:
        r.set_replica_params(alpha=[0.1] * n, gamma=[0.9, 0.95, 0.97, 0.99, 0.9], lambda_=[0.4, 0.5, 0.65, 0.8, 0.4])
    assert ei.value.code == grlx.capi.ERR_INVALID
    assert "replica 3" in str(ei.value) and "0.8" in str(ei.value) and "trace longer" in str(ei.value)
    after = r.replica_params()
    for name in before:                                        # nothing partly applied, the alpha of the same call included
        assert_bit_equal(after[name], before[name], f"{name} after a refused call")
    _refused(grlx, lambda: r.set_replica_params(lambda_=[0.4, 0.5, 0.65, 0.8, 0.4]), "replica 3")     # 0.97 * 0.8 = 0.776: too long as well
    r.close()
    r = grlx.Runner(grlx.pendulum_sarsa_config(n, trace=0), np.arange(n))      # without a trace lambda is not read: no rule
    r.set_replica_params(gamma=[0.99] * n, lambda_=[0.8] * n)
    r.close()


def test_a_valid_grid_is_accepted_whatever_the_way_there(grlx):
    """The C entry validates one parameter against the other three as they stand: gamma = 0.99 beside the configuration's lambda = 0.65
    is refused (0.6435^10 = 0.0122).  The Runner moves lambda to min(current, new) first, then gamma, then lambda, so every grid whose
    final pairs are valid is accepted -- also one where gamma rises for some replicas and lambda for others -- and it runs bit-equal."""
    n, trials = 6, 11
    cfg, spec = configs.pendulum(grlx, n, agent=0, max_rows=trials + 1)
    seeds = np.arange(811, 811 + n)
    r = grlx.Runner(cfg, seeds)
    gamma99 = np.full(n, 0.99)
    _refused(grlx, lambda: grlx.capi.check(r.lib.grlx_set_replica_params(r._ctx, grlx.capi.PARAM_GAMMA, gamma99.ctypes.data_as(r.lib.grlx_set_replica_params.argtypes[2]))),
             "trace longer")
    params = dict(alpha=[0.2] * n, gamma=[0.99, 0.9, 0.99, 0.8, 0.97, 0.99], lambda_=[0.4, 0.7, 0.5, 0.78, 0.65, 0.45], epsilon=[0.05] * n)
    r.set_replica_params(gamma=params["gamma"], lambda_=params["lambda_"])      # 0.9 * 0.7 and 0.8 * 0.78 pass only with THEIR gamma
    got = r.replica_params()
    assert_bit_equal(got["gamma"], params["gamma"], "gamma"); assert_bit_equal(got["lambda_"], params["lambda_"], "lambda")
    r.run(trials); r.sync()
    for k in range(n):
        want = oracle_run(replica_spec(spec, params, k), seeds[k], (("run", trials),), cfg.projector.memory)
        check_replica(r, k, want, f"replica {k}", cfg.projector.memory)
    r.close()


@pytest.mark.parametrize("make,over,word", [
    ("pendulum", dict(agent=4, kappa=0.5), "agent"),                          # advantage learning
    ("pendulum_qv", dict(), "agent"),
    ("cart_pole_ac", dict(), "agent"),
    ("pendulum", dict(trace=2), "accumulating"),
    ("pendulum", dict(target_interval=10, target_tau=1.0), "target network"),
    ("pendulum", dict(safe=1), "safe"),
    ("pendulum", dict(tap_replica=0, tap_capacity=100), "taps"),
    ("acrobot", dict(replicas_per_wave=16), "replicas_per_wave"),
])
def test_unbuilt_contexts_are_refused(grlx, make, over, word):
    n = 4
    over = dict(over)
    safe = over.pop("safe", None)
    if make == "pendulum":
        cfg, _ = configs.pendulum(grlx, n, **over)
    elif make == "pendulum_qv":
        cfg, _ = configs.pendulum_qv(grlx, n)
    elif make == "cart_pole_ac":
        cfg, _ = configs.cart_pole_ac(grlx, n)
    else:
        cfg, _ = configs.acrobot(grlx, n, **over)
    if safe is not None:
        cfg.projector.safe = safe
    r = grlx.Runner(cfg, np.arange(n))
    _refused(grlx, lambda: r.set_replica_params(alpha=[0.1] * n), word)
    assert r._ctx                                              # the context is still a plain one, and runs
    r.run(1); r.sync()
    r.close()


def test_set_after_the_first_run_and_the_per_step_entries(grlx):
    n = 4
    r = grlx.Runner(grlx.pendulum_sarsa_config(n), np.arange(n))
    r.run(1); r.sync()
    _refused(grlx, lambda: r.set_replica_params(alpha=[0.1] * n), "first launch")
    r.close()
    # diagnostics first, then a set
    r = grlx.Runner(grlx.pendulum_sarsa_config(n), np.arange(n))
    r.set_diag(True)
    _refused(grlx, lambda: r.set_replica_params(alpha=[0.1] * n), "diagnostics")
    r.close()
    # a sweep context refuses what would run on the shared values
    r = grlx.Runner(grlx.pendulum_sarsa_config(n), np.arange(n))
    r.set_replica_params(alpha=[0.05, 0.1, 0.2, 0.25])
    obs = np.zeros((n, 2))
    _refused(grlx, lambda: r.env_start(0), "sweep context")
    _refused(grlx, lambda: r.env_advance(np.zeros(n)), "sweep context")
    _refused(grlx, lambda: r.agent_start(0, obs), "sweep context")
    _refused(grlx, lambda: r.agent_step(0, obs, np.zeros(n)), "sweep context")
    _refused(grlx, lambda: r.agent_end(0, obs, np.zeros(n)), "sweep context")
    _refused(grlx, lambda: grlx.capi.check(r.lib.grlx_set_diag(r._ctx, 1)), "sweep context")
    _refused(grlx, lambda: grlx.capi.check(r.lib.grlx_set_diag(r._ctx, 2)), "sweep context")
    grlx.capi.check(r.lib.grlx_set_diag(r._ctx, 0))            # off is not a diagnostic run
    _refused(grlx, lambda: grlx.capi.check(r.lib.grlx_set_replica_params(r._ctx, 4, np.zeros(n).ctypes.data_as(r.lib.grlx_set_replica_params.argtypes[2]))), "GRLX_PARAM")
    r.run(2); r.sync()                                         # ... and still runs
    assert r.last_kernel() == 1 and r.env_server_counts() == (0, 0)
    r.close()
    # an external environment has no fused run to sweep
    cfg = grlx.pendulum_sarsa_config(n)
    cfg.env = grlx.capi.ENV_EXTERNAL
    r = grlx.Runner(cfg, np.arange(n))
    _refused(grlx, lambda: r.set_replica_params(alpha=[0.1] * n), "GRLX_ENV_EXTERNAL")
    r.close()


def test_automatic_layout_of_a_sweep_never_exceeds_eight(grlx):
    """16384 acrobots choose 16 replicas per wave by themselves; the same context as a sweep runs 8 per wave (the wider layouts
    have no SpecSweep instantiation), bit-equal to the oracle on a sample."""
    n, trials = 16384, 3
    cfg, spec = configs.acrobot(grlx, n, agent=1, max_rows=trials + 1)
    seeds = np.arange(1, n + 1)
    r = grlx.Runner(cfg, seeds)
    assert r.replicas_per_wave() == 16
    base = combos(100)
    params = {name: [base[name][k % 100] for k in range(n)] for name in base}
    r.set_replica_params(**params)
    assert r.replicas_per_wave() == 8
    r.run(trials); r.sync()
    assert r.last_kernel() == 1
    for k in (0, 5, 8191, n - 1):
        want = oracle_run(replica_spec(spec, params, k), seeds[k], (("run", trials),), cfg.projector.memory)
        check_replica(r, k, want, f"replica {k}", cfg.projector.memory)
    r.close()


# ---- 10: grouped curve statistics -------------------------------------------------------------------------------------------------
def _tree(per_thread):
    s = np.array(per_thread, dtype=np.float64)
    off = 128
    while off > 0:
        s[:off] = s[:off] + s[off:2 * off]
        off //= 2
    return s[0]


def grouped_reference(rew, rows_of, first, count, group_size):
    """curve_stats_grouped_kernel restated: thread t of block (row, group) adds the group's members t, t + 256, ... in that order,
    then the fixed tree over the 256 partial sums.  rew[row][replica]; rows_of[replica] = rows that replica wrote."""
    n = rew.shape[1]
    out = np.zeros((count, n // group_size, 3))
    for i in range(count):
        row = first + i
        for q in range(n // group_size):
            a, b, c = np.zeros(256), np.zeros(256), np.zeros(256)
            for k in range(group_size):
                rep = q * group_size + k
                if row < rows_of[rep]:
                    v = rew[row, rep]
                    a[k % 256] = a[k % 256] + v
                    b[k % 256] = b[k % 256] + v * v
                    c[k % 256] = c[k % 256] + 1
            out[i, q] = (_tree(a), _tree(b), _tree(c))
    return out


def _device_stats(r, first, count, group_size=None):
    import torch
    groups = 1 if group_size is None else r.cfg.n_replicas // group_size
    out = torch.zeros((count, groups, 3), dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    if group_size is None:
        r.curve_stats(out.data_ptr(), first, count, stream)
    else:
        r.curve_stats_grouped(out.data_ptr(), first, count, group_size, stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _all_rewards(r, max_rows):
    n = r.cfg.n_replicas
    rows_of = [r.replica_rows(k) for k in range(n)]
    rew = np.zeros((max_rows, n))
    for k in range(n):
        rew[:rows_of[k], k] = r.rows(k)[2]
    return rew, rows_of


def test_curve_stats_grouped(grlx):
    n, R = 21, 7
    g = grlx.sweep_grid(R, alpha=[0.05, 0.1, 0.25])
    cfg = grlx.pendulum_sarsa_config(n, max_rows=8)
    r = grlx.Runner(cfg, np.arange(700, 700 + n))
    r.set_replica_params(alpha=g["alpha"])
    r.run(33); r.sync()
    assert r.n_rows() == 3
    rew, rows_of = _all_rewards(r, 3)
    assert rows_of == [3] * n
    got = _device_stats(r, 0, 3, R)
    assert got.shape == (3, 3, 3)
    assert_bit_equal(got.ravel(), grouped_reference(rew, rows_of, 0, 3, R).ravel(), "groups of 7")
    assert (got[:, :, 2] == R).all()
    assert_bit_equal(_device_stats(r, 1, 2, 3).ravel(), grouped_reference(rew, rows_of, 1, 2, 3).ravel(), "groups of 3, from row 1")
    # one group of all replicas is grlx_curve_stats, bit for bit
    whole = _device_stats(r, 0, 3, n)
    assert_bit_equal(whole.ravel(), _device_stats(r, 0, 3).ravel(), "group_size = n against curve_stats")
    assert_bit_equal(whole.ravel(), grouped_reference(rew, rows_of, 0, 3, n).ravel(), "group_size = n")
    import torch
    buf = torch.zeros((3, n, 3), dtype=torch.float64, device="cuda")
    for bad in (4, 0, -7, 22):                                 # not whole groups
        _refused(grlx, lambda: r.curve_stats_grouped(buf.data_ptr(), 0, 3, bad), "group_size")
    r.close()


def test_curve_stats_grouped_beyond_one_stride_and_ragged(grlx):
    """600 replicas in groups of 300: threads 0..43 of a block add two members each (the strided part of the order).  Then a steps
    budget on acrobots: the replicas stop at trials of their own and every row counts the replicas that wrote it."""
    n, R = 600, 300
    cfg = grlx.pendulum_sarsa_config(n, max_rows=4, table_log2_capacity=14)
    r = grlx.Runner(cfg, np.arange(1, n + 1))
    r.set_replica_params(epsilon=grlx.sweep_grid(R, epsilon=[0.01, 0.2])["epsilon"])
    r.run(22); r.sync()
    rew, rows_of = _all_rewards(r, 2)
    assert_bit_equal(_device_stats(r, 0, 2, R).ravel(), grouped_reference(rew, rows_of, 0, 2, R).ravel(), "groups of 300")
    assert_bit_equal(_device_stats(r, 0, 2, n).ravel(), _device_stats(r, 0, 2).ravel(), "group_size = n against curve_stats")
    r.close()
    n, R = 24, 6
    cfg, _ = configs.acrobot(grlx, n, agent=1, max_rows=400)
    r = grlx.Runner(cfg, np.arange(900, 900 + n))
    params = combos(n, offset=11)
    r.set_replica_params(**params)
    r.run_steps(100000, 1500); r.sync()
    rows = max(r.replica_rows(k) for k in range(n))
    rew, rows_of = _all_rewards(r, rows)
    assert len(set(rows_of)) > 1                               # ragged
    got = _device_stats(r, 0, rows, R)
    assert_bit_equal(got.ravel(), grouped_reference(rew, rows_of, 0, rows, R).ravel(), "ragged rows")
    assert (got[rows - 1, :, 2] < R).any() and got[:, :, 2].sum() == sum(rows_of)
    assert_bit_equal(_device_stats(r, 0, rows, n).ravel(), _device_stats(r, 0, rows).ravel(), "ragged: group_size = n against curve_stats")
    r.close()


# ---- 11: the deployer -------------------------------------------------------------------------------------------------------------
def test_grlxd_sweep(grlx, tmp_path):
    """`grlxd -s 5 -r 3 -t 220 -l -q -p alpha=0.1,0.2 -p epsilon=0.05,0.1`: 12 clones, clone i = point * 3 + k seeded 5 + i.  Every
    <output>-0@i.txt is the oracle's rows of that clone (-l: the layout Experiment.format_rows restates; without it the rows carry
    the wall time), and <output>-0-sweep.txt is grlo's statistics (bin/grlo:46-48) over the simple regret (bin/grllib.py:71-75)
    of those files, recomputed here from their text: == on the parsed doubles."""
    from grl_amd import _build
    grlxd = _build.build_host()
    res = subprocess.run([grlxd, "-s", "5", "-r", "3", "-t", "220", "-l", "-q", "-p", ALPHA_PATH + "=0.1,0.2", "-p", EPSILON_PATH + "=0.05,0.1", YAML],
                         cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr + res.stdout
    g = grlx.sweep_grid(3, alpha=[0.1, 0.2], epsilon=[0.05, 0.1])
    regrets = []
    for i in range(12):
        spec = ob.pendulum_sarsa_spec()
        spec.alpha, spec.epsilon = g["alpha"][i], g["epsilon"][i]
        e = ob.Experiment(spec, seed=5 + i)
        rows, _ = e.run(220)
        text = (tmp_path / f"pendulum-sarsa-tc-0@{i}.txt").read_text()
        assert text == e.format_rows(rows), f"clone {i}"
        e.close()
        data = [float(line.split()[2]) for line in text.split("\n")[:-1]]
        assert len(data) == 20
        sample = len(data) // 20
        total = 0.0
        for v in data[-sample:]:
            total += v
        regrets.append(total / sample)
    assert not (tmp_path / "pendulum-sarsa-tc-0@12.txt").exists()
    lines = (tmp_path / "pendulum-sarsa-tc-0-sweep.txt").read_text().split("\n")
    assert len(lines) == 5 and lines[4] == ""
    for pt in range(4):
        f = lines[pt].split()
        assert len(f) == 9 and int(f[0]) == pt and int(f[5]) == 3
        assert [float(x) for x in f[1:5]] == [g["alpha"][3 * pt], 0.97, 0.65, g["epsilon"][3 * pt]]
        res_pt = regrets[3 * pt:3 * pt + 3]
        total = 0.0
        for v in res_pt:
            total += v
        avg = total / 3
        sq = 0.0
        for v in res_pt:
            sq += (v - avg) * (v - avg)
        stddev = np.sqrt(sq / 2)
        assert float(f[6]) == avg and float(f[7]) == stddev and float(f[8]) == stddev / np.sqrt(3.0)
        assert f[6] == "%.17g" % avg
    assert len({ln.split()[6] for ln in lines[:4]}) > 1           # the points differ
    # fewer than 20 rows: the reference's "Worker did not return enough data"
    res = subprocess.run([grlxd, "-s", "5", "-r", "2", "-t", "110", "-l", "-q", "-p", ALPHA_PATH + "=0.1,0.2", YAML],
                         cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert res.returncode != 0 and "20 rows" in res.stderr, res.stderr


def _sweep_stats(regrets, R):
    """bin/grlo:46-48 over the R regrets of a point, every sum left to right"""
    total = 0.0
    for v in regrets:
        total += v
    avg = total / R
    sq = 0.0
    for v in regrets:
        sq += (v - avg) * (v - avg)
    stddev = np.sqrt(sq / (R - 1))
    return avg, stddev, stddev / np.sqrt(float(R))


def test_grlxd_sweep_default_row_layout(grlx, tmp_path):
    """Without -l the rows are the reference's six columns (online_learning.cpp:243), the reward printed with three decimals: the
    simple regret is over the reward column AS WRITTEN, so -sweep.txt equals a recomputation from the text of the files."""
    from grl_amd import _build
    grlxd = _build.build_host()
    res = subprocess.run([grlxd, "-s", "5", "-r", "3", "-t", "220", "-q", "-p", ALPHA_PATH + "=0.1,0.2", "-p", EPSILON_PATH + "=0.05,0.1", YAML],
                         cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr + res.stdout
    regrets = []
    for i in range(12):
        rows = [line.split() for line in (tmp_path / f"pendulum-sarsa-tc-0@{i}.txt").read_text().split("\n")[:-1]]
        assert len(rows) == 20 and all(len(f) == 6 for f in rows)
        assert all(len(f[2].split(".")[1]) == 3 for f in rows)                 # three decimals
        regrets.append(float(rows[-1][2]) / 1)                                  # 20 // 20 = one row
    lines = (tmp_path / "pendulum-sarsa-tc-0-sweep.txt").read_text().split("\n")
    assert len(lines) == 5 and lines[4] == ""
    for pt in range(4):
        f = lines[pt].split()
        avg, stddev, stderr = _sweep_stats(regrets[3 * pt:3 * pt + 3], 3)
        assert int(f[0]) == pt and int(f[5]) == 3
        assert float(f[6]) == avg and float(f[7]) == stddev and float(f[8]) == stderr


def _readme_sweep_command():
    """the `grlxd ... -p ...` line of README.md, its continuation joined and its comment dropped"""
    root = os.path.dirname(os.path.dirname(__file__))
    text = open(os.path.join(root, "README.md")).read().replace("\\\n", " ")
    line = next(ln for ln in text.split("\n") if ln.startswith("grl_amd/bin/grlxd") and " -p " in ln)
    return line.split("#")[0].split()


def test_the_documented_sweeps_run(grlx, tmp_path):
    """README.md's grlxd line as it stands (64 points x 64 repetitions, 2000 trials) and the grid of INTEGRATION.md's Python
    example: both are accepted -- every documented value passes the trace rule beside the golden yaml's lambda -- and the
    deployer writes one line of statistics per point."""
    from grl_amd import _build
    grlxd = _build.build_host()
    argv = _readme_sweep_command()
    assert argv[0] == "grl_amd/bin/grlxd" and argv[-1] == "tests/golden/pendulum-sarsa-tc.yaml" and argv.count("-p") == 3
    res = subprocess.run([grlxd] + argv[1:-1] + [YAML], cwd=tmp_path, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr + res.stdout
    lines = (tmp_path / "pendulum-sarsa-tc-0-sweep.txt").read_text().split("\n")
    assert len(lines) == 65 and lines[64] == ""
    assert all(len(ln.split()) == 9 and ln.split()[5] == "64" and np.isfinite([float(x) for x in ln.split()[6:]]).all() for ln in lines[:64])
    assert (tmp_path / "pendulum-sarsa-tc-0@4095.txt").exists() and not (tmp_path / "pendulum-sarsa-tc-0@4096.txt").exists()
    # INTEGRATION.md section 3
    root = os.path.dirname(os.path.dirname(__file__))
    call = next(ln for ln in open(os.path.join(root, "INTEGRATION.md")).read().split("\n") if ln.startswith("g = grl_amd.sweep_grid("))
    g = eval(call.split("#")[0][len("g = "):], {"grl_amd": grlx})
    assert all(len(v) == 4096 for v in g.values())
    r = grlx.Runner(grlx.pendulum_sarsa_config(4096), np.arange(1, 4097))
    r.set_replica_params(**g)
    r.run(1); r.sync()
    assert r.last_kernel() == 1
    r.close()
