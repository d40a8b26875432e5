"""The batch path's greedy evaluation episodes and their trajectories on the GPU (grlx_fqi_evaluate, grlx_fqi_evaluate_trajectory) against
tests/fqi_evaluate_ref.py, a plain loop over the oracle's observation, Q and environment step.  Every comparison is on bit patterns.

The training shape.  With the small shapes of test_gpu_fqi.py every greedy episode takes action index 0 at every step and most steps are
three-way ties: a kernel that ignored its Q-values would pass.  One batch of batch_size=2000, iterations=10, epochs=100 gives, on the
oracle, for the seeds 3, 4, 5: hidden = 20, 32, 64 a seed-3 policy that uses all three actions without a tie and a tie-heavy seed-4
policy; hidden = 16 two actions and a few tied steps (seed 3) beside tie-heavy ones.  hidden = 8 saturates under RPROP at every shape
tried on the CPU (iterations 1 ... 20, epochs 2 ... 500, batches 1 ... 3, batch sizes up to 6000, seeds 3 ... 10: action 0 throughout),
so its network is fitted by gradient descent, eta = 0.4, at the same shape: two actions, a tie-free full-length episode from the task's
start and 10 ... 38 tied steps in four others, for each of the three seeds.  The condition -- two action indices, a full-length
episode without a tie, an episode with ties -- is asserted on the reference's output per width.

No domain-exit case: the pendulum's damping keeps the angle inside Env::in_domain from every admitted state."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import fqi_evaluate_ref as fr
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

SEEDS = [3, 4, 5]
SHAPE = dict(batch_size=2000, iterations=10, epochs=100)
WIDTHS = {8: dict(SHAPE, eta=0.4), 16: SHAPE, 20: SHAPE, 32: SHAPE, 64: SHAPE}
TIMEOUT, CONTROL_STEP = 2.99, 0.03          # tests/golden/pendulum-fqi-ann.yaml
FULL = 100                                  # steps of an episode from time 0 to the timeout


def start_states():
    return np.array([[math.pi, 0.0, 0.0],                       # the task's test start
                     [-7.25, 11.5, 0.37],                       # more than one turn below zero
                     [math.pi, 0.0, TIMEOUT - CONTROL_STEP],    # 1-2 steps: a ragged wave
                     [1.0, -2.0, TIMEOUT + 1.0],                # past the timeout: exactly one step, code 1
                     [0.5, 1.0, 1.0], [2.0, -6.0, 0.0],         # general states
                     [0.1, 0.0, 0.0]])                          # near upright


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} vs {b.shape}"
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        bad = np.nonzero(bits(a).ravel() != bits(b).ravel())[0]
    else:
        bad = np.nonzero(a.ravel() != b.ravel())[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a.ravel()[bad[0]]!r} vs {b.ravel()[bad[0]]!r}"


_oracles = {}


def oracles(hidden):
    """the three oracle experiments of a width after ONE batch, made once and never advanced again"""
    if hidden not in _oracles:
        made = []
        for s in SEEDS:
            e = ob.FqiExperiment(ob.pendulum_fqi_spec(hidden=hidden, **WIDTHS[hidden]), seed=s)
            e.run_batch()
            made.append(e)
        _oracles[hidden] = made
    return _oracles[hidden]


_runners = {}


def runner(grlx, hidden):
    """the context of a width after ONE batch; the tests only evaluate it, which changes nothing"""
    if hidden not in _runners:
        r = grlx.FqiRunner(grlx.pendulum_fqi_config(len(SEEDS), max_batches=1, hidden=hidden, **WIDTHS[hidden]), SEEDS)
        r.run_batch(); r.sync()
        _runners[hidden] = r
    return _runners[hidden]


def reference(es, states, max_steps):
    """(dict of [replica][start] arrays, records[replica][start][max_steps or steps]) over the oracle experiments es"""
    outs, recs = zip(*[fr.evaluate(e, states, max_steps) for e in es])
    return {k: np.stack([o[k] for o in outs]) for k in fr.FIELDS}, recs


def compare(got, want, what):
    for k in fr.FIELDS:
        same_bits(getattr(got, k), want[k], f"{what}: {k}")


# ---- 1: every width against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", sorted(WIDTHS))
def test_every_width_against_the_reference(grlx, hidden):
    """three replicas x the seven states, max_steps = 0: all six outputs; the trajectory with max_steps = 100: its records, and its six sums
    equal to evaluate's bit for bit"""
    states = start_states()
    want, recs = reference(oracles(hidden), states, 0)
    idx = set(int(v) for per in recs for r in per for v in r[:, fr.ACTION_INDEX])
    assert len(idx) >= 2, f"hidden = {hidden}: the reference policy takes one action only: {idx}"
    assert ((want["steps"] == FULL) & (want["ties"] == 0)).any(), f"hidden = {hidden}: no full-length episode without a tie"
    assert (want["ties"] > 0).any(), f"hidden = {hidden}: no episode with a tie"
    assert want["steps"].max() == FULL and list(want["steps"][0, 2:4]) in ([1, 1], [2, 1]) and (want["terminal"] == 1).all()

    r = runner(grlx, hidden)
    for k, e in enumerate(oracles(hidden)):
        same_bits(r.params(k), e.params(), f"replica {k}: the parameters the episodes run on")
    got = r.evaluate(states)
    compare(got, want, f"hidden = {hidden}, evaluate")
    traj = r.evaluate_trajectory(states, FULL)
    compare(traj, want, f"hidden = {hidden}, evaluate_trajectory")
    for k in fr.FIELDS:
        same_bits(getattr(traj, k), getattr(got, k), f"hidden = {hidden}: {k} of the trajectory call against evaluate's")
    assert traj.records.shape == (len(SEEDS), states.shape[0], FULL, fr.WORDS) and r.trajectory_record_words() == fr.WORDS
    for k in range(len(SEEDS)):
        for s in range(states.shape[0]):
            n = int(want["steps"][k, s])
            same_bits(traj.episode(k, s), recs[k][s], f"hidden = {hidden}, replica {k}, state {s}: records")
            assert not bits(traj.records[k, s, n:]).any(), f"hidden = {hidden}, replica {k}, state {s}: records behind the end are not zero bits"
    same_bits(traj.state[0, 0, FULL - 1], got.final_state[0, 0], "the last record's state is the final state")


# ---- 2: more pairs than one wave, and the cut --------------------------------------------------------------------------------------------
def test_more_pairs_than_one_wave_and_the_cut(grlx):
    """hidden = 20, 67 start states (a second block of start states with 61 dead lanes), replicas 1 and 2, max_steps = 12: code 0 occurs"""
    base = start_states()
    states = np.array([base[i % 7] + [0.01 * (i // 7), 0.0, 0.0] for i in range(67)])
    es = oracles(20)[1:3]
    want, recs = reference(es, states, 12)
    assert (want["terminal"] == 0).any() and (want["terminal"] == 1).any() and (want["steps"] == 12).any() and (want["steps"] == 1).any()
    r = runner(grlx, 20)
    got = r.evaluate(states, replicas=range(1, 3), max_steps=12)
    compare(got, want, "67 states, evaluate")
    traj = r.evaluate_trajectory(states, 12, replicas=range(1, 3))
    compare(traj, want, "67 states, evaluate_trajectory")
    same_bits(traj.records, np.stack([np.stack(per) for per in recs]), "67 states: records, zeros behind the ends included")
    same_bits(r.evaluate(states, replicas=(1, 2), max_steps=12).ret, want["ret"], "a (first, count) pair")


# ---- 3: an evaluation from the test start is the row ------------------------------------------------------------------------------------
def test_an_evaluation_from_the_test_start_is_the_row(grlx):
    """seed 3, hidden = 20: after batch k the tie-free episode from (pi, 0, 0) returns the reward of row k bit for bit -- the oracle's
    -4934.802200544619 and -3572.409078560829"""
    r = grlx.FqiRunner(grlx.pendulum_fqi_config(1, max_batches=2, hidden=20, **SHAPE), [3])
    start = np.array([[math.pi, 0.0, 0.0]])
    for k, row in enumerate((-4934.802200544619, -3572.409078560829)):
        r.run_batch(); r.sync()
        got = r.evaluate(start)
        assert got.ties[0, 0] == 0 and got.steps[0, 0] == FULL and got.terminal[0, 0] == 1
        same_bits(got.ret[0], r.rows(0, k + 1)[2][k:k + 1], f"batch {k}: ret against the row")
        same_bits(got.ret[0], [row], f"batch {k}: ret against the oracle's row")
    r.close()


# ---- 4: an evaluation changes nothing ---------------------------------------------------------------------------------------------------
def test_an_evaluation_changes_nothing(grlx):
    """two contexts on the same seeds; one evaluates and records before the first batch and after it; then both run another batch"""
    over = dict(batch_size=700, iterations=3, epochs=40)
    seeds = [1, 2, 3]
    cfg = grlx.pendulum_fqi_config(len(seeds), max_batches=2, **over)
    r, plain = grlx.FqiRunner(cfg, seeds), grlx.FqiRunner(cfg, seeds)
    states = start_states()

    def state_of(x):
        return [(x.params(k), x.rows(k, 2), x.info(k), x.transitions(k, 0, 2 * cfg.batch_size)) for k in range(len(seeds))]

    def same_state(a, b, when):
        for k, ((pa, ra, ia, ta), (pb, rb, ib, tb)) in enumerate(zip(a, b)):
            same_bits(pa, pb, f"{when}, replica {k}: parameters")
            for x, y, name in zip(ra, rb, ("batch", "transitions", "reward")):
                same_bits(x, y, f"{when}, replica {k}: rows, {name}")
            assert ia["rng"] == ib["rng"] and ia["n"] == ib["n"] and ia["iterations"] == ib["iterations"], f"{when}, replica {k}: {ia} vs {ib}"
            same_bits([ia["maxdelta"], ia["error"]], [ib["maxdelta"], ib["error"]], f"{when}, replica {k}: maxdelta, error")
            for x, y, name in zip(ta, tb, ("inputs", "next observations", "rewards", "targets")):
                same_bits(x, y, f"{when}, replica {k}: stored {name}")

    first = r.evaluate(states)                      # allowed before the first batch: the initial network
    assert (first.steps[:, 0] == FULL).all()
    r.evaluate_trajectory(states, 30)
    same_state(state_of(r), state_of(plain), "before the first batch")
    for x in (r, plain):
        x.run_batch(); x.sync()
    e = r.evaluate(states)
    t = r.evaluate_trajectory(states, FULL, replicas=range(1, 3))
    same_bits(t.ret, e.ret[1:3], "the trajectory call's ret")
    same_state(state_of(r), state_of(plain), "after the first batch")
    for x in (r, plain):
        x.run_batch(); x.sync()
    same_state(state_of(r), state_of(plain), "after the second batch")
    r.close(); plain.close()


# ---- 5: chunked staging ------------------------------------------------------------------------------------------------------------------
def test_chunked_staging(grlx):
    """the 7 states two at a time, sums and records; a bound below one column of records is refused with the remedies named"""
    r, states, n = runner(grlx, 20), start_states(), len(SEEDS)
    whole, whole_t = r.evaluate(states), r.evaluate_trajectory(states, FULL)
    sums = 8 * 3 + (2 * 8 + 3 * 4 + 8 * 3) * n              # a start state's staged bytes without records
    column = n * FULL * fr.WORDS * 8
    lib = grlx.capi.load()
    try:
        lib.grlx_set_query_chunk_bytes(2 * sums + sums // 2)
        got = r.evaluate(states)
        for k in fr.FIELDS:
            same_bits(getattr(got, k), getattr(whole, k), f"chunked evaluate: {k}")
        lib.grlx_set_query_chunk_bytes(2 * (column + sums) + sums)
        got = r.evaluate_trajectory(states, FULL)
        for k in fr.FIELDS + ("records",):
            same_bits(getattr(got, k), getattr(whole_t, k), f"chunked evaluate_trajectory: {k}")
        lib.grlx_set_query_chunk_bytes(column + sums - 1)
        with pytest.raises(grlx.capi.GrlxError) as ei:
            r.evaluate_trajectory(states, FULL)
        said = str(ei.value)
        assert ei.value.code == grlx.capi.ERR_INVALID
        assert "fewer replicas" in said and "smaller max_steps" in said and "grlx_set_query_chunk_bytes" in said, said
        same_bits(r.evaluate_trajectory(states, FULL, replicas=range(0, 1)).records, whole_t.records[:1], "the first remedy")
    finally:
        lib.grlx_set_query_chunk_bytes(0)


# ---- 7: refusals -------------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.0


def raw_call(grlx, r, first, count, states, n_starts, max_steps, trajectory=False, records=True):
    """the entry point itself on sentinel-filled outputs: (status, message, were the outputs left alone?)"""
    lib = grlx.capi.load()
    rows, n = max(count, 1), max(n_starts, 1)
    f64 = [np.full((rows, n), SENTINEL) for _ in range(2)] + [np.full((rows, n, 3), SENTINEL)]
    i32 = [np.full((rows, n), 7, np.int32) for _ in range(3)]
    rec = np.full((rows, n, max_steps if 1 <= max_steps <= 64 else 1, fr.WORDS), SENTINEL)      # (a max_steps beyond is one this test expects refused)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    sp = None if states is None else p(states, C.c_double)
    args = [r._ctx, first, count, sp, n_starts, max_steps, p(f64[0], C.c_double), p(f64[1], C.c_double), p(i32[0], C.c_int32), p(i32[1], C.c_int32),
            p(i32[2], C.c_int32), p(f64[2], C.c_double)]
    if trajectory:
        rc = lib.grlx_fqi_evaluate_trajectory(*args, p(rec, C.c_double) if records else None)
    else:
        rc = lib.grlx_fqi_evaluate(*args)
    untouched = all((a == SENTINEL).all() for a in f64 + [rec]) and all((a == 7).all() for a in i32)
    return rc, lib.grlx_last_error().decode(), untouched


def test_refusals(grlx):
    r = runner(grlx, 20)
    states = start_states()
    nan = states.copy(); nan[4, 1] = float("nan")
    big = states.copy(); big[5, 0] = -2.0 ** 17
    cap = 100000                                # include/grlx.h: GRLX_MAX_EPISODE_STEPS
    cases = [
        (dict(states=None), "states is null"),
        (dict(n_starts=-1), "n_starts = -1"),
        (dict(first=1, count=3), "replica range"),
        (dict(first=-1, count=1), "replica range"),
        (dict(max_steps=-1), "max_steps = -1"),
        (dict(max_steps=cap + 1), "max_steps = %d" % (cap + 1)),
        (dict(states=nan), "row 4, component 1 is not finite"),
        (dict(states=big), "row 5, component 0"),
    ]
    for trajectory in (False, True):
        for over, word in cases:
            a = dict(first=0, count=3, states=states, n_starts=7, max_steps=5)
            a.update(over)
            rc, said, untouched = raw_call(grlx, r, a["first"], a["count"], a["states"], a["n_starts"], a["max_steps"], trajectory)
            assert rc == grlx.capi.ERR_INVALID and word in said, (over.keys(), said)
            assert untouched, f"{word}: something was written"
    rc, said, untouched = raw_call(grlx, r, 0, 3, big, 7, 5)
    assert "2^17" in said
    rc, said, untouched = raw_call(grlx, r, 0, 3, states, 7, 0, trajectory=True)
    assert rc == grlx.capi.ERR_INVALID and "max_steps = 0" in said and untouched
    rc, said, untouched = raw_call(grlx, r, 0, 3, states, 7, 5, trajectory=True, records=False)
    assert rc == grlx.capi.ERR_INVALID and "records is null" in said and untouched
    # nothing to do is not an error, and writes nothing
    for first, count, n in ((0, 0, 7), (0, 3, 0)):
        for trajectory in (False, True):
            rc, said, untouched = raw_call(grlx, r, first, count, states, n, 5, trajectory)
            assert rc == grlx.capi.OK and untouched
    # any output other than the records may be NULL
    lib = grlx.capi.load()
    ret = np.zeros((3, 7))
    assert lib.grlx_fqi_evaluate(r._ctx, 0, 3, states.ctypes.data_as(C.POINTER(C.c_double)), 7, 0, ret.ctypes.data_as(C.POINTER(C.c_double)), None, None, None,
                                 None, None) == grlx.capi.OK
    same_bits(ret, r.evaluate(states).ret, "ret alone")
