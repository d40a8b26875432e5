"""Sampled ensemble episodes (grlx_evaluate_ensemble_sampled / Runner.evaluate_ensemble_sampled) against
tests/policy_evaluate_ensemble_sampled_ref.py, the serial loop of include/grlx.h over the oracle's dense tables, its portable exponential
and its Rand48.  Every output and the streams are compared on the bit patterns.

Shapes: test_gpu_policy_evaluate_ensemble.py's -- 33 replicas on a 32768-slot memory after six trials, 2 start states, 12 steps, streams
from episode_stream_words.  One block serves one episode with 16 members per round: groups of 1, 3, 16 (one full round), 17 (a second
round with one member), 33 (three rounds: the accumulator's buffer of a step differs from step to step) and two groups of 16 in one call.

Temperatures, picked on the CPU with the oracle so that the reference alone shows the draw at work (at the default tau = 0.1 one vote of
difference is a factor e^10 and explored is almost always 0): majority tau = 1.0, rank tau = 2.0, softmax members tau_m = 1.0.  The
reference's explored per (start state) at 12 steps each, three actions, greedy members, streams of seed 5: majority, group of 3: [6 7],
17: [2 3], 33: [3 1]; rank, group of 3: [6 7], 17: [2 3], 33: [3 1].  With softmax members under rank the members' ranks are all six
permutations of (1, 2, 3)."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_ensemble_sampled_ref as es
from tests import policy_query_ref as ref
from tests.test_gpu_policy_evaluate import start_states
from tests.test_gpu_policy_evaluate_ensemble import consecutive, small_memory
from tests.test_gpu_policy_evaluate_sampled import decayed
from tests.test_gpu_policy_query import SEED0, build, same_bits

pytestmark = pytest.mark.gpu

N, STEPS, STREAM_SEED = 33, 12, 5
TAU = {"majority": 1.0, "rank": 2.0}
STRATEGY = {"majority": es.MAJORITY, "rank": es.RANK}
MEMBERS = {"greedy": (es.GREEDY, None), "epsilon": (es.EPSILON, 0.3), "softmax": (es.SOFTMAX, 1.0)}
SHAPES = [(0, 1, 1), (0, 3, 3), (0, 16, 16), (0, 17, 17), (0, 33, 33), (0, 32, 16)]      # (first replica, replicas, group size)

_tables, _want = {}, {}


def setup(grlx, graph, n=N, **both):
    cfg, spec = build(grlx, graph, n)
    small_memory(cfg, spec)
    for k, v in both.items():
        setattr(cfg, k, v); setattr(spec, k, v)
    return cfg, spec, start_states(graph, spec)[1:3]


def tables(key, spec, n, trials):
    """the members' dense tables 0 after `trials` trials; the oracle's experiments stay open: the vectors are theirs"""
    if key not in _tables:
        exps = [ob.Experiment(spec, seed=SEED0 + k) for k in range(n)]
        for e in exps:
            if trials:
                e.run(trials)
        _tables[key] = ([ref.dense(e, 0) for e in exps], exps)
    return _tables[key][0]


def reference(key, w, spec, states, strategy, member, param, shapes, grlx, seen=None):
    """[shape] -> (streams, dict of the ten outputs and the records stacked over the shape's groups)"""
    if key not in _want:
        out = []
        for first, count, G in shapes:
            groups = consecutive(count, G, first)
            streams = grlx.episode_stream_words(STREAM_SEED, len(groups), len(states))
            per = [es.evaluate([w[m] for m in g], spec, states, STRATEGY[strategy], TAU[strategy], MEMBERS[member][0], [param] * G, streams[k], STEPS, seen=seen)
                   for k, g in enumerate(groups)]
            out.append((streams, {f: np.stack([p[f] for p in per]) for f in es.FIELDS + ("records",)}))
        _want[key] = out
    return _want[key]


def check(got, want, what, fields=es.FIELDS):
    for f in fields:
        same_bits(getattr(got, "n_explored" if f == "explored" and hasattr(got, "n_explored") else f), want[f], f"{what}: {f}")


@pytest.mark.parametrize("member", list(MEMBERS))
@pytest.mark.parametrize("strategy", list(TAU))
@pytest.mark.parametrize("graph", ["pendulum_sarsa", "pendulum_q_five_actions"])
def test_against_the_reference(grlx, graph, strategy, member):
    cfg, spec, states = setup(grlx, graph)
    param, seen = MEMBERS[member][1], {}
    want = reference((graph, strategy, member), tables(graph, spec, N, 6), spec, states, strategy, member, param or 0.0, SHAPES, grlx, seen)
    if member == "greedy":       # the draw must matter: asserted on the reference alone
        assert any(((0 < w["explored"]) & (w["explored"] < w["steps"])).any() for _, w in want), f"{graph}, {strategy}: the draw never leaves the maximum"
    if (strategy, member) == ("rank", "softmax") and seen:
        top = int(spec.action_steps)
        assert any(sorted(rk) != [1] * (top - 1) + [top] for rk in seen["ranks"]), "every member ranks its maximum first and the rest equal"
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    r.run(6); r.sync()
    for (first, count, G), (streams, w) in zip(SHAPES, want):
        got = r.evaluate_ensemble_sampled(states, G, strategy, TAU[strategy], member, param, streams, range(first, first + count), STEPS)
        check(got, w, f"{graph}, {strategy}, {member}: replicas {first} ... {first + count - 1} in groups of {G}")
    r.close()


@pytest.mark.parametrize("strategy", list(TAU))
def test_all_weights_zero(grlx, strategy):
    """before any launch on init_min = init_max = 0: every member ties, d_m is uniform, the score has one nonzero entry (majority: every
    vote goes to the first action) or is uniform (rank: every rank is 1), and under rank the cumulative walk alone decides"""
    cfg, spec, states = setup(grlx, "ties", 17)
    (streams, want), = reference(("ties", strategy), tables("ties", spec, 17, 0), spec, states, strategy, "greedy", 0.0, [(0, 17, 17)], grlx)
    assert (want["member_ties"] == want["steps"] * 17).all()
    if strategy == "rank":
        assert (want["ties"] == want["steps"]).all() and (want["records"][..., :2, -1] == es.softmax([17, 17, 17], TAU["rank"])[0]).all()
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + 17))
    check(r.evaluate_ensemble_sampled(states, 17, strategy, TAU[strategy], streams=streams, max_steps=STEPS), want, f"all weights 0, {strategy}")
    r.close()


def test_the_members_own_epsilon(grlx):
    """decay_rate 0.8, epsilon 0.6: after six trials every member's e is 0.8^6 * 0.6, the products formed one by one"""
    cfg, spec, states = setup(grlx, "pendulum_sarsa", 17, decay_rate=0.8, decay_min=0.01, epsilon=0.6)
    e_own = decayed(spec, 6) * float(spec.epsilon)
    assert 0.1 < e_own < 0.2
    (streams, want), = reference("own", tables("own", spec, 17, 6), spec, states, "rank", "epsilon", e_own, [(0, 17, 17)], grlx)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + 17))
    r.run(6); r.sync()
    check(r.evaluate_ensemble_sampled(states, 17, "rank", TAU["rank"], "epsilon", "own", streams, max_steps=STEPS), want, "own epsilon")
    r.close()


def test_a_second_environment(grlx):
    cfg, spec, states = setup(grlx, "cart_pole_q", 17)
    (streams, want), = reference("cart_pole", tables("cart_pole", spec, 17, 6), spec, states, "rank", "softmax", 1.0, [(0, 17, 17)], grlx)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + 17))
    r.run(6); r.sync()
    check(r.evaluate_ensemble_sampled(states, 17, "rank", TAU["rank"], "softmax", 1.0, streams, max_steps=STEPS), want, "cart-pole, group of 17")
    r.close()


@pytest.mark.parametrize("G", [3, 17])
def test_the_trajectory(grlx, G):
    """the sums are the plain call's; the records, .explored and .prob among them, are the reference's; zeros behind an episode's end"""
    graph, strategy, member = "pendulum_sarsa", "rank", "softmax"
    cfg, spec, states = setup(grlx, graph)
    states = np.concatenate([states, start_states(graph, spec)[4:5]])      # a step short of the timeout: an episode that ends early
    (streams, want), = reference(("trajectory", G), tables(graph, spec, N, 6), spec, states, strategy, member, 1.0, [(0, G, G)], grlx)
    assert want["steps"].min() < STEPS == want["steps"].max() and (want["records"][..., -2] == 1).any() and (want["records"][..., -1] > 0).any()
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    r.run(6); r.sync()
    assert r.ensemble_sampled_trajectory_record_words() == r.trajectory_record_words(True) + 2 == want["records"].shape[-1]
    args = (strategy, TAU[strategy], member, 1.0, streams, range(0, G))
    got = r.evaluate_ensemble_sampled_trajectory(states, G, STEPS, *args)
    check(got, want, f"trajectory, group of {G}", es.FIELDS + ("records",))
    check(r.evaluate_ensemble_sampled(states, G, *args, STEPS), want, f"the plain call, group of {G}")
    same_bits(got.explored, want["records"][..., -2], "explored"); same_bits(got.prob, want["records"][..., -1], "prob")
    short = int(np.argmin(want["steps"][0]))
    assert not got.records[0, short, int(want["steps"][0, short]):].view(np.uint64).any(), "records behind an episode's end"
    r.close()


def test_the_call_changes_nothing(grlx):
    cfg, spec, states = setup(grlx, "pendulum_sarsa", 3)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + 3))
    r.run(6); r.sync()
    look = lambda: (r.snapshot(), [list(r.rng(k)) for k in range(3)], [r.env_state(k).tobytes() for k in range(3)])
    before = look()
    own = r.evaluate_ensemble_sampled(states, 3, "rank", 2.0, "epsilon", "own", max_steps=STEPS)       # streams=None: a copy of replica 0's global stream
    r.evaluate_ensemble_sampled_trajectory(states, 3, STEPS, "majority", 1.0, "softmax", 1.0)
    assert look() == before, "a sampled ensemble evaluation changed the context"
    again = r.evaluate_ensemble_sampled(states, 3, "rank", 2.0, "epsilon", "own", np.full((1, 2), r.rng(0)[0], np.uint64), max_steps=STEPS)
    check(again, own._asdict(), "streams = None against the first replica's global stream handed in")
    r.close()


def test_refusals(grlx):
    """each with its reason and the function named, before anything is launched and with nothing written"""
    import ctypes as C
    cfg, spec, states = setup(grlx, "pendulum_sarsa", 4)
    P = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))

    def refused(r, word, states=states, count=4, G=2, strategy=0, tau=1.0, member=0, param=0.0, streams=None):
        ret = np.full(max(count, 1) * len(states), 777.0)
        rc = r.lib.grlx_evaluate_ensemble_sampled(r._ctx, 0, count, G, strategy, tau, member, param, P(states, C.c_double), len(states), STEPS,
                                                  P(streams, C.c_uint64), P(ret, C.c_double), *[None] * 9)
        msg = r.lib.grlx_last_error().decode()
        assert rc == grlx.capi.ERR_INVALID and word in msg and "grlx_evaluate_ensemble_sampled" in msg and (ret == 777).all(), (rc, msg)

    r = grlx.Runner(cfg, [1, 2, 3, 4])
    for kw, word in ((dict(G=0), "group_size = 0"), (dict(G=3), "group_size 3 does not divide the 4 replicas"), (dict(strategy=2), "unknown strategy 2"),
                     (dict(member=3), "unknown member sampler 3"), (dict(tau=0.0), "tau = 0"), (dict(tau=-1.0), "tau = -1"), (dict(tau=np.inf), "tau = inf"),
                     (dict(tau=np.nan), "tau = nan"), (dict(member=2, param=0.0), "tau_m = 0"), (dict(member=2, param=np.nan), "tau_m = nan"),
                     (dict(member=1, param=1.5), "epsilon = 1.5 is outside [0, 1]"), (dict(member=1, param=-0.5), "epsilon = -0.5 is outside [0, 1]"),
                     (dict(member=1, param=np.nan), "epsilon is not finite"), (dict(streams=np.full((2, 2), 1 << 48, np.uint64)), "stream row 0"),
                     (dict(count=5, G=5), "replica range")):
        refused(r, word, **kw)
    r.close()
    ac, ac_spec = build(grlx, "ac_twin", 4)
    r = grlx.Runner(ac, [1, 2, 3, 4])
    for word in ("not built", "grlx_evaluate_actor_ensemble", "no epsilon-greedy exploration for GRLX_EPSILON_OWN"):
        refused(r, word, states=start_states("ac_twin", ac_spec)[:2], member=1, param=-1.0)
    r.close()
