"""Streamed trajectories (grlx_evaluate_trajectory_stream, Runner.evaluate_trajectory_stream): the chunks a sink is handed, assembled,
against Runner.evaluate_trajectory on the same context at the default staging bound -- and, for the pendulum's SARSA and the cart-pole's
actor-critic, against tests/policy_trajectory_ref.py's oracle loop directly.  Every comparison is on the bit patterns (-0.0 is not +0.0).

Shapes: 5 replicas x 7 start states (35 pairs, no multiple of 4: the last wave has dead 16-lane groups), max_steps 40, 6 trials of
training, and a staging bound under which the chunk rule gives 2 start states per chunk: chunks [2, 2, 2, 1], so both slots are
used again within a call (slot 0 by chunks 0 and 2, slot 1 by chunks 1 and 3, and slot 0 a third time by the next call's first chunk),
and the last chunk is partial.

Ragged ends, long first: four starts at model time 0 (some replica runs all 40 steps: no tail), then three whose time component is
8, 3 and 1 control steps short of the timeout (tails of 32, 37 and 39 records) -- so the slot a short episode is staged in held full-length
records before, and a kernel that left the tail to a zero fill nobody does any more would hand those back.  The condition on the inputs
is asserted on the sibling's steps in every case: at least three distinct lengths, one of max_steps, one of at most 2."""
import ctypes as C

import numpy as np
import pytest

from tests import configs
from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev
from tests import policy_trajectory_ref as tr
from tests.test_gpu_policy_query import SEED0, build, same_bits

pytestmark = pytest.mark.gpu

# the seven instantiations: Q agents on pendulum x {3, 5}, acrobot, cart-pole, walker x 3; the actor-critic on cart-pole and pendulum
GRAPHS = ["pendulum_sarsa", "pendulum_q_five_actions", "acrobot_q", "cart_pole_q", "walker_q", "ac_twin", "pendulum_ac"]
N, NS, MS, TRIALS = 5, 7, 40, 6
FIELDS = ("ret", "disc", "steps", "terminal", "ties", "final_state", "records")
_cache = {}


def make(grlx, graph, n=N, **cfg_only):
    """(configuration, oracle spec); the pendulum's actor-critic is not among test_gpu_policy_query's graphs"""
    if graph != "pendulum_ac":
        return build(grlx, graph, n, **cfg_only)
    cfg, spec = configs.pendulum_ac(grlx, n)
    cfg.max_rows = 64
    spec.math = ob.MATH_PORTABLE
    return cfg, spec


def time_of(spec, first):
    """(index of the model state's time component, the timeout it runs against)"""
    if spec.env == ob.ENV_COMPASS_WALKER:                    # [..., time, timeout]: the state carries its own timeout
        return 9, float(first[10])
    return first.size - 1, 20.0 if spec.env == ob.ENV_ACROBOT else float(spec.timeout)


def start_of(graph, spec):
    key = ("first", graph)
    if key not in _cache:
        e = ob.Experiment(spec, seed=SEED0)
        e.env_start(1)
        _cache[key] = e.state()
        e.close()
    return _cache[key].copy()


def ragged_states(graph, spec, which="ragged"):
    """7 start states: the oracle's test start (the pendulum: (pi, 0, t)) with its first component nudged, at the times of `which` --
    "ragged": four at time 0, then 8, 3 and 1 steps before the timeout; "long": all at time 0; "short": all within 8 steps of the timeout"""
    first = start_of(graph, spec)
    ti, timeout = time_of(spec, first)
    dt = float(spec.control_step)
    if spec.env == ob.ENV_PENDULUM:                          # the issue's table: timeout 2.99, steps 8, 3, 1
        short = [2.78, 2.93, 2.97]
    else:
        short = [timeout - 7.2 * dt, timeout - 2.2 * dt, timeout - 0.6 * dt]
    times = {"ragged": [0.0] * 4 + short, "long": [0.0] * NS, "short": (short * 3)[:NS]}[which]
    states = np.tile(first, (NS, 1))
    states[:, 0] += 0.001 * np.array([0, 1, -1, 2, 0, 1, -1])
    states[:, ti] = times
    assert np.isfinite(states).all() and (np.abs(states) < 2.0 ** 17).all()
    return states


def start_bytes(r, n=N, ms=MS):
    """what one start state stages (grlx_host_rules.h: stream_start_bytes), written out here a second time"""
    S, R = r.state_dims, r.trajectory_record_words()
    return 8 * S + n * (ms * R * 8 + 2 * 8 + 8 * S + 3 * 4)


def collect(r, states, ms=MS, replicas=None, sink=None):
    """(the chunks assembled into a Trajectory, [(first_start, n_starts)], chunks delivered); sink(chunk): called after the copy"""
    first, count = r._replica_range(replicas)
    n, S, R = states.shape[0], r.state_dims, r.trajectory_record_words()
    out = dict(ret=np.full((count, n), np.nan), disc=np.full((count, n), np.nan), steps=np.full((count, n), -7, np.int32),
               terminal=np.full((count, n), -7, np.int32), ties=np.full((count, n), -7, np.int32), final_state=np.full((count, n, S), np.nan),
               records=np.full((count, n, ms, R), np.nan))
    seen = []

    def on_chunk(c):
        k = c.ret.shape[1]
        seen.append((c.first_start, k))
        assert c.records.shape == (count, k, ms, R) and c.final_state.shape == (count, k, S) and c.steps.shape == (count, k)
        assert not c.records.flags.writeable and not c.ret.flags.writeable
        for f in FIELDS:
            out[f][:, c.first_start:c.first_start + k] = getattr(c, f)
        return sink(c) if sink else None

    delivered = r.evaluate_trajectory_stream(states, ms, on_chunk, replicas=replicas)
    from grl_amd import runner
    return runner.Trajectory(**out), seen, delivered


def check_same(got, want, what):
    for f in FIELDS:
        same_bits(getattr(got, f), getattr(want, f), f"{what}: {f}")


def check_ragged(steps, what):
    lengths = sorted(set(steps.ravel().tolist()))
    assert len(lengths) >= 3 and lengths[-1] == MS and lengths[0] <= 2, f"{what}: the start states give the lengths {lengths}: a test error"


def check_tails_are_zero_words(got, what):
    behind = np.arange(got.records.shape[2])[None, None, :] >= got.steps[:, :, None]
    assert not got.records.view(np.uint64)[behind].any(), f"{what}: a record behind an episode's end is not all-zero bits"


class bounded:
    """the staging bound under which the rule gives `per_chunk` start states per chunk; the default bound again on the way out"""

    def __init__(self, grlx, r, per_chunk=2, **shape):
        self.lib, self.bound = grlx.capi.load(), 2 * per_chunk * start_bytes(r, **shape) + 3

    def __enter__(self):
        assert self.lib.grlx_set_query_chunk_bytes(self.bound) == 0
        return self.bound

    def __exit__(self, *exc):
        self.lib.grlx_set_query_chunk_bytes(0)


def trained(grlx, graph, n=N, **cfg_only):
    cfg, spec = make(grlx, graph, n, **cfg_only)
    seeds = np.arange(SEED0, SEED0 + n)
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    return r, cfg, spec, seeds


def oracle(graph, spec, seeds, states):
    """[replica] -> policy_trajectory_ref.evaluate's dict after TRIALS trials, computed once (every GPU test runs clean and poisoned)"""
    key = ("oracle", graph)
    if key not in _cache:
        exps = [ob.Experiment(spec, seed=int(s)) for s in seeds]
        for e in exps:
            e.run(TRIALS)
        _cache[key] = [tr.evaluate(ev.tables_of(e), spec, states, MS) for e in exps]
        for e in exps:
            e.close()
    return _cache[key]


# ---- 1: the bits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", GRAPHS)
def test_the_chunks_are_the_siblings_bits(grlx, graph):
    r, cfg, spec, seeds = trained(grlx, graph)
    states = ragged_states(graph, spec)
    whole = r.evaluate_trajectory(states, MS)                   # the default bound: one chunk of the sibling
    check_ragged(whole.steps, graph)
    with bounded(grlx, r):
        got, seen, delivered = collect(r, states)
    assert seen == [(0, 2), (2, 2), (4, 2), (6, 1)] and delivered == 4, seen
    check_same(got, whole, f"{graph}: streamed in [2, 2, 2, 1] against evaluate_trajectory")
    check_tails_are_zero_words(got, graph)
    if graph in ("pendulum_sarsa", "ac_twin"):                  # not only a sibling in the same library
        want = oracle(graph, spec, seeds, states)
        for f in tr.FIELDS:
            same_bits(getattr(got, f), np.stack([w[f] for w in want]), f"{graph}: {f} against the oracle's loop")
    # a replica range of its own: rows are the range's
    with bounded(grlx, r, n=2):
        part, seen, _ = collect(r, states, replicas=range(2, 4))
    assert seen == [(0, 2), (2, 2), (4, 2), (6, 1)]
    for f in FIELDS:
        same_bits(getattr(part, f), getattr(whole, f)[2:4], f"{graph}: replicas 2 and 3 alone: {f}")
    r.close()


# ---- 2: what the staging held before ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum_sarsa", "walker_q", "ac_twin"])
def test_stale_staging_does_not_show_behind_an_episodes_end(grlx, graph):
    """two calls on one context through the same two slots: every episode full length, then every episode short.  Nobody clears the
    slots in between, so the second call's tails are zero only if its kernel wrote them."""
    r, cfg, spec, seeds = trained(grlx, graph)
    long, short = ragged_states(graph, spec, "long"), ragged_states(graph, spec, "short")
    with bounded(grlx, r):
        first, seen1, _ = collect(r, long)
        second, seen2, _ = collect(r, short)
    assert seen1 == seen2 == [(0, 2), (2, 2), (4, 2), (6, 1)]
    assert first.steps.max() == MS and second.steps.min() == 1 and (first.steps > second.steps).all(), \
        f"{graph}: every pair's first episode was meant to be longer than its second, and one of them full length: a test error"
    check_tails_are_zero_words(second, f"{graph}: the second call")
    check_same(second, r.evaluate_trajectory(short, MS), f"{graph}: the second call against evaluate_trajectory")
    check_same(first, r.evaluate_trajectory(long, MS), f"{graph}: the first call against evaluate_trajectory")
    r.close()


# ---- 3: one chunk, nothing to do -------------------------------------------------------------------------------------------------------
def test_one_chunk_under_the_default_bound_and_no_call_for_nothing(grlx):
    r, cfg, spec, seeds = trained(grlx, "pendulum_sarsa")
    states = ragged_states("pendulum_sarsa", spec)
    got, seen, delivered = collect(r, states)
    assert seen == [(0, NS)] and delivered == 1
    check_same(got, r.evaluate_trajectory(states, MS), "one chunk")
    calls = []
    assert r.evaluate_trajectory_stream(states[:0], MS, calls.append) == 0 and calls == []
    assert r.evaluate_trajectory_stream(states, MS, calls.append, replicas=(1, 0)) == 0 and calls == []
    r.close()


# ---- 4: stopping ---------------------------------------------------------------------------------------------------------------------
def test_a_sink_that_stops_the_stream(grlx):
    capi = grlx.capi
    r, cfg, spec, seeds = trained(grlx, "pendulum_sarsa")
    states = ragged_states("pendulum_sarsa", spec)
    whole = r.evaluate_trajectory(states, MS)
    with bounded(grlx, r):
        calls = []
        with pytest.raises(capi.GrlxError) as ei:
            r.evaluate_trajectory_stream(states, MS, lambda c: calls.append(c.first_start) or (5 if len(calls) == 2 else 0))
        assert calls == [0, 2], calls
        assert ei.value.code == capi.ERR_STOPPED and "5" in str(ei.value) and "grlx_evaluate_trajectory_stream" in str(ei.value), str(ei.value)

        class Boom(Exception):
            pass

        def raising(c):
            calls.append(c.first_start)
            raise Boom("from the sink")

        calls = []
        with pytest.raises(Boom):
            r.evaluate_trajectory_stream(states, MS, raising)
        assert calls == [0], "an exception in the sink stops the stream at that chunk"
        # the same context streams again, and then runs on as one that never streamed
        got, seen, _ = collect(r, states)
        assert seen == [(0, 2), (2, 2), (4, 2), (6, 1)]
        check_same(got, whole, "after a stopped stream")
    r.run(1); r.sync()
    plain = grlx.Runner(cfg, seeds)
    plain.run(TRIALS); plain.sync()
    plain.run(1); plain.sync()
    for k in range(N):
        for a, b, name in zip(r.rows(k), plain.rows(k), ("trial", "steps", "reward")):
            same_bits(a, b, f"replica {k}: {name} of the rows after a stopped stream and one more trial")
    assert r.snapshot() == plain.snapshot(), "a context that streamed and was stopped differs from one that never streamed"
    plain.close()
    r.close()


# ---- 5: a streamed call changes nothing ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["pendulum_sarsa", "ac_twin"])
def test_a_streamed_call_changes_nothing(grlx, graph):
    capi = grlx.capi
    r, cfg, spec, seeds = trained(grlx, graph)
    states = ragged_states(graph, spec)

    def look():
        return r.snapshot(), [list(r.rng(k)) for k in range(N)], [r.env_state(k).tobytes() for k in range(N)]

    before = look()
    with bounded(grlx, r):
        collect(r, states)
        with pytest.raises(capi.GrlxError) as ei:
            r.evaluate_trajectory_stream(states, MS, lambda c: 1)
        assert ei.value.code == capi.ERR_STOPPED
    collect(r, states[:3], ms=7, replicas=range(1, 3))
    after = look()
    assert after[0] == before[0], "a streamed call changed the context's snapshot"
    assert after[1:] == before[1:], "a streamed call changed a stream or an environment state"
    r.close()


# ---- 6: calls from inside the sink -----------------------------------------------------------------------------------------------------
def test_the_context_refuses_calls_from_inside_the_sink(grlx):
    capi = grlx.capi
    r, cfg, spec, seeds = trained(grlx, "pendulum_sarsa")
    states = ragged_states("pendulum_sarsa", spec)
    whole = r.evaluate_trajectory(states, MS)
    refusals = []

    def attempt(call):
        with pytest.raises(capi.GrlxError) as ei:
            call()
        refusals.append((ei.value.code, str(ei.value)))

    def sink(c):
        if c.first_start == 2:                                  # with chunk 2 in flight
            attempt(lambda: r.run(1))
            attempt(lambda: r.run_steps(1, 10))
            attempt(r.reset_run)
            attempt(lambda: r.load_snapshot(b"x" * 64))
            attempt(lambda: r.evaluate_trajectory_stream(states, MS, lambda c: 0))
            attempt(lambda: r.evaluate(states))                 # reads on the same context are not served either
            attempt(lambda: r.rng(0))
            assert r.lib.grlx_destroy(r._ctx) == capi.ERR_INVALID and "a streamed call is in progress" in r.lib.grlx_last_error().decode()

    with bounded(grlx, r):
        got, seen, _ = collect(r, states, sink=sink)
    assert len(refusals) == 7
    for code, msg in refusals:
        assert code == capi.ERR_INVALID and "a streamed call is in progress" in msg, msg
    assert seen == [(0, 2), (2, 2), (4, 2), (6, 1)]
    check_same(got, whole, "a stream whose sink tried to change the context")
    r.run(1); r.sync()                                          # and afterwards the context takes calls again
    r.close()


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------
def raw_call(r, states, first=0, count=N, max_steps=MS, null_sink=False, n_starts=None):
    """the C entry point with a counting sink: (status, message, sink calls)"""
    from grl_amd import capi
    states = np.ascontiguousarray(states, np.float64)
    calls = []
    cb = capi.TRAJECTORY_SINK() if null_sink else capi.TRAJECTORY_SINK(lambda user, chunk: calls.append(1) or 0)
    rc = r.lib.grlx_evaluate_trajectory_stream(r._ctx, first, count, states.ctypes.data_as(C.POINTER(C.c_double)),
                                               states.shape[0] if n_starts is None else n_starts, max_steps, cb, None)
    return rc, r.lib.grlx_last_error().decode(), len(calls)


def refused(grlx, r, words, states, **kw):
    rc, msg, calls = raw_call(r, states, **kw)
    assert rc == grlx.capi.ERR_INVALID and calls == 0, (rc, msg, calls)
    for w in [words] if isinstance(words, str) else words:
        assert w in msg, (w, msg)
    assert "grlx_evaluate_trajectory_stream" in msg, msg


def test_refusals(grlx):
    cfg, spec = make(grlx, "pendulum_sarsa")
    states = ragged_states("pendulum_sarsa", spec)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    lib = grlx.capi.load()
    refused(grlx, r, "sink is null", states, null_sink=True)
    refused(grlx, r, ("max_steps = 0", "no default"), states, max_steps=0)
    refused(grlx, r, "max_steps = 100001", states, max_steps=100001)
    refused(grlx, r, "max_steps = -1", states, max_steps=-1)
    refused(grlx, r, "replica range", states, first=3, count=3)
    refused(grlx, r, "replica range", states, first=-1, count=2)
    refused(grlx, r, "n_starts = -1", states, n_starts=-1)
    bad = states.copy(); bad[2, 1] = np.nan
    refused(grlx, r, "row 2, component 1 is not finite", bad)
    # a column over half the bound, under a bound the sibling accepts the same column with
    one = start_bytes(r)
    column = N * MS * 11 * 8
    try:
        assert lib.grlx_set_query_chunk_bytes(2 * one - 1) == 0
        refused(grlx, r, (f"{column} bytes", f"{one} with its sums", f"{one - 1} of {2 * one - 1} bytes", "half the staging bound", "fewer replicas",
                          "smaller max_steps", "grlx_set_query_chunk_bytes"), states)
        r.evaluate_trajectory(states, MS)                       # the sibling stages one chunk at a time: the same column fits its bound
        assert lib.grlx_set_query_chunk_bytes(2 * one) == 0     # the column equal to half the bound: 7 chunks of one
        rc, msg, calls = raw_call(r, states)
        assert (rc, calls) == (0, NS), (rc, msg, calls)
    finally:
        lib.grlx_set_query_chunk_bytes(0)
    # nothing to do is no error
    assert raw_call(r, states, n_starts=0)[::2] == (0, 0) and raw_call(r, states, first=1, count=0)[::2] == (0, 0)
    with pytest.raises(ValueError):
        r.evaluate_trajectory_stream(states[:, :2], MS, lambda c: 0)
    with pytest.raises(grlx.capi.GrlxError) as ei:
        r.evaluate_trajectory_stream(states, MS, None)
    assert ei.value.code == grlx.capi.ERR_INVALID and "sink is null" in str(ei.value)
    r.close()

    safe, _ = make(grlx, "pendulum_sarsa")
    safe.projector.safe = 1
    r = grlx.Runner(safe, np.arange(SEED0, SEED0 + N))
    refused(grlx, r, ("not built", "safe"), states)
    r.close()
