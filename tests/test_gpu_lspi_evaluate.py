"""The LSPI context's evaluation episodes, trajectories and ensembles (grlx_lspi_evaluate*, grlx_lspi_query_ensemble) against one plain
Python loop: tests/test_gpu_lspi.py's Ref.q on the replica's weights, the first maximum, the oracle's pendulum step, the sums in
episode_account's order.  Everything is integer or S5 arithmetic, so every comparison is on bit patterns.

Contexts: six replicas each, evaluated before any batch (random weights) and after two batches.  Start states: both ends of each range,
angles and velocities outside them, a cell boundary, times close to the timeout (ragged ends inside a wave) and, for Gauss, a velocity
further outside the grid than the cutoff radius: its projection is empty, every read is 0 and step 0 has n_max == action_steps."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests.test_gpu_lspi import GRID, Ref, bits

pytestmark = pytest.mark.gpu

SEEDS = [3, 4, 5, 6, 7, 8]
CASES = {"tri-f27-n5": dict(steps=[3, 3, 3], projector="triangle", batch_size=5, iterations=1),
         "tri-f60": dict(steps=[5, 4, 3], projector="triangle", batch_size=64, iterations=3),
         "gauss-f60": dict(steps=[5, 4, 3], projector="gauss", batch_size=64, iterations=3),            # the box is clipped on every side
         "gauss-f363": dict(steps=[11, 11, 3], projector="gauss", batch_size=64, iterations=1),         # an interior box
         "gauss-f363-s05": dict(steps=[11, 11, 3], projector="gauss", batch_size=64, iterations=1, sigma=0.5),      # a box of about one cell
         "tri-f60-a5": dict(steps=[5, 4, 3], projector="triangle", batch_size=64, iterations=3, action_steps=5),   # lane 0 owns two actions
         "gauss-f60-s2": dict(steps=[5, 4, 3], projector="gauss", batch_size=64, iterations=3, sigma=2.0),          # the box is wider than the grid on every axis
         "gauss-f363-c1e8": dict(steps=[11, 11, 3], projector="gauss", batch_size=64, iterations=1, cutoff=1e-8)}   # a radius of 4.3 cells, twice the default's
PI = math.pi
# index of the start whose velocity lies beyond the cutoff radius of every Gauss case: 200 > 12 pi + radius * delta, radius =
# sigma sqrt(-log cutoff) cells of delta = 24 pi / (steps[1] - 1).  The defaults at steps[1] = 4: 37.7 + 2.15 * 25.1 = 91.6; gauss-f60-s2:
# 37.7 + 4.29 * 25.1 = 145.6; gauss-f363-c1e8: 37.7 + 4.29 * 7.54 = 70.1; tests/test_gpu_lspi_evaluate_sampled.py's gauss-f512-s3:
# 37.7 + 6.44 * 10.8 = 107.0
FAR = 7
# model states (angle, velocity, time); the observation's angle is (angle + pi) mod 2 pi
STARTS = np.array([[PI, 0.0, 0.0], [-PI, -12 * PI, 2.8], [PI - 1e-9, 12 * PI, 2.9], [7.0, -40.0, 2.95], [-0.5 * PI, 50.0, 2.97], [-4.0, 3.3, 3.0],
                   [0.3, -2.0, 2.7], [1.0, 200.0, 2.9], [2.0, 8 * PI, 2.93]])
SHORT = np.array([s + [0.001 * (i // 8), 0.0, 0.0] for i, s in enumerate(np.tile(STARTS[1:], (9, 1))[:65])])      # 65 starts of at most 11 steps
VOTE, MEAN_Q = 0, 1
GROUPINGS = ((0, 6, 1), (0, 6, 2), (3, 3, 3), (0, 6, 6), (0, 6, 3))      # (first replica, replicas, group size)
FIELDS = ("ret", "disc", "steps", "terminal", "ties", "final_state")


def findmax(v):
    mai, man = 0, 1
    for a in range(1, len(v)):
        if v[a] > v[mai]:
            mai, man = a, 1
        elif v[a] == v[mai]:
            man += 1
    return mai, man


def episode(ref, members, rule, state, max_steps, spec):
    """the specification: (records [steps][11 or 13], ret, disc, steps, code, ties, member_ties, agreement, final state); rule None: one policy"""
    x = np.array(state, dtype=np.float64)
    o = (C.c_double * 2)()
    ob.load().orc_env_observe(C.byref(spec), (C.c_double * 3)(*x), o)
    obs, recs, ret, disc, g, steps, code, ties, member_ties, agreement = list(o), [], 0.0, 0.0, 1.0, 0, 0, 0, 0, 0
    while steps < max_steps and code == 0:
        votes, sumq, mties = [0.0] * len(ref.actions), [0.0] * len(ref.actions), 0
        for w in members:
            q = ref.q(w, obs)
            mai, man = findmax(q)
            votes[mai] += 1
            mties += man > 1
            sumq = [s + v for s, v in zip(sumq, q)]
        score = q if rule is None else votes if rule == VOTE else sumq
        mai, man = findmax(score)
        nx, nobs, rew, term = ob.env_step(spec, x, ref.actions[mai])
        reward = float(rew[0])
        ret, disc, g, steps, ties, code = ret + reward, disc + g * reward, g * ref.gamma_tau, steps + 1, ties + (man > 1), int(term[0])
        member_ties, agreement = member_ties + mties, agreement + int(votes[mai])
        head = [ref.actions[mai], reward, score[mai], mai, man, code] + ([] if rule is None else [votes[mai], mties])
        recs.append(head + obs + list(nx[0]))
        x, obs = nx[0], list(nobs[0])
    return np.array(recs), ret, disc, steps, code, ties, member_ties, agreement, x


_made, _wanted = {}, {}


def context(grlx, name, when):
    """(reference, runner, weights per replica, what must not change); made once: `before` never runs a batch, `after` has run two"""
    if (name, when) not in _made:
        cfg = grlx.pendulum_lspi_config(len(SEEDS), max_batches=2, **CASES[name])
        r = grlx.LspiRunner(cfg, SEEDS)
        for _ in range({"before": 0, "one": 1, "after": 2}[when]):
            r.run_batch(); r.sync()
        _made[name, when] = (Ref(cfg), r, [r.params(k) for k in range(len(SEEDS))], frozen(r))
    return _made[name, when]


def frozen(r):
    return b"".join(r.params(k, w).tobytes() for k in range(len(SEEDS)) for w in (0, 1)) + b"".join(a.tobytes() for k in range(len(SEEDS)) for a in r.rows(k, 2)) + \
        repr([r.info(k) for k in range(len(SEEDS))]).encode()


def wanted(name, when, ref, ws, first, count, group, rule, states, max_steps):
    """the reference over the replicas [first, first + count) in groups (group None: one policy each), computed once per argument list"""
    key = (name, when, first, count, group, rule, states.tobytes(), max_steps)
    if key not in _wanted:
        spec = ob.pendulum_sarsa_spec()
        g = group or 1
        _wanted[key] = [[episode(ref, ws[first + k * g:first + (k + 1) * g], rule if group else None, s, max_steps or 100000, spec) for s in states]
                        for k in range(count // g)]
    return _wanted[key]


def compare(got, want, max_steps, what, extra=()):
    for j, f in enumerate(("ret", "disc", "steps", "terminal", "ties") + extra):
        w = np.array([[e[1 + j] for e in row] for row in want])
        assert (bits(getattr(got, f).astype(np.float64)) == bits(w.astype(np.float64))).all(), f"{what}: {f}\n{getattr(got, f)}\nvs\n{w}"
    assert (bits(got.final_state) == bits(np.array([[e[8] for e in row] for row in want]))).all(), f"{what}: final_state"
    if hasattr(got, "records"):
        for k, row in enumerate(want):
            for s, e in enumerate(row):
                assert (bits(got.records[k, s, :e[3]]) == bits(e[0])).all(), f"{what}: records of row {k}, start {s}"
                assert got.records.shape[2] == max_steps and not bits(got.records[k, s, e[3]:]).any(), f"{what}: words behind the end of row {k}, start {s}"


@pytest.mark.parametrize("when", ["before", "after"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_episodes_and_trajectories(grlx, name, when):
    ref, r, ws, was = context(grlx, name, when)
    n_rep = len(SEEDS)
    # all nine starts to their ends, every replica: sums, then every record word
    want = wanted(name, when, ref, ws, 0, n_rep, None, None, STARTS, 0)
    compare(r.evaluate(STARTS), want, 0, f"{name} {when}: evaluate")
    compare(r.evaluate_trajectory(STARTS, 100), want, 100, f"{name} {when}: evaluate_trajectory")
    assert {e[4] for row in want for e in row} == {1} and want[0][0][3] == 100 and len({e[3] for e in want[0]}) > 4, "ragged ends, all timed out"
    if ref.gauss:
        assert all(row[FAR][0][0, 4] == len(ref.actions) and row[FAR][0][0, 2] == 0.0 for row in want), "the far start's first step reads zeros"
    # a lone quad from the task's start: the batch's row where nothing tied
    if when == "after":
        one = r.evaluate(STARTS[:1])
        rows = np.array([r.rows(k, 2)[2][1] for k in range(n_rep)])
        clean = one.ties[:, 0] == 0
        assert clean.any() and (bits(one.ret[clean, 0]) == bits(rows[clean])).all(), f"{name}: ret from (pi, 0, 0) against the row: {one.ret[:, 0]} vs {rows}"
    # a replica sub-range, a ragged wave, max_steps 7: terminal 0 with records sized by it
    cut = wanted(name, when, ref, ws, 1, 4, None, None, STARTS[:5], 7)
    assert {e[4] for row in cut for e in row} == {0, 1}
    compare(r.evaluate_trajectory(STARTS[:5], 7, replicas=(1, 4)), cut, 7, f"{name} {when}: replicas 1 ... 4, max_steps 7")
    # a second block: 65 starts
    compare(r.evaluate(SHORT, replicas=(4, 2)), wanted(name, when, ref, ws, 4, 2, None, None, SHORT, 0), 0, f"{name} {when}: 65 starts")
    assert frozen(r) == was, "an evaluation changed the context"


def test_a_trained_tie(grlx):
    """seed 4 at [3, 3, 3] after ONE batch of 5 (tests/test_gpu_lspi.py, above SEEDS): no stored transition touches the nodes the start
    observation reads, their weights are exactly 0 and step 0 from (pi, 0, 0) is a tie -- seen by the reference loop itself"""
    ref, r, ws, was = context(grlx, "tri-f27-n5", "one")
    k = SEEDS.index(4)
    want = wanted("tri-f27-n5", "one", ref, ws, k, 1, None, None, STARTS[:1], 0)
    assert want[0][0][5] > 0 and want[0][0][0][0, 4] > 1, "the reference does not tie at step 0"
    compare(r.evaluate_trajectory(STARTS[:1], 100, replicas=(k, 1)), want, 100, "seed 4 after one batch")
    assert frozen(r) == was


@pytest.mark.parametrize("rule", [VOTE, MEAN_Q])
@pytest.mark.parametrize("name", sorted(CASES))
def test_ensembles(grlx, name, rule):
    ref, r, ws, was = context(grlx, name, "after")
    states, rname = STARTS[1:6], ("vote", "mean")[rule]
    extra = ("member_ties", "agreement")
    for first, count, g in GROUPINGS:
        want = wanted(name, "after", ref, ws, first, count, g, rule, states, 7)
        what = f"{name}: {count} replicas from {first} in groups of {g}, {rname}"
        got = r.evaluate_ensemble(states, g, rule=rname, replicas=(first, count), max_steps=7)
        compare(got, want, 7, what, extra)
        compare(r.evaluate_ensemble_trajectory(states, g, 7, rule=rname, replicas=(first, count)), want, 7, what + ", trajectory", extra)
        if g == 1:
            single = r.evaluate(states, replicas=(first, count), max_steps=7)
            for f in ("ret", "disc", "steps", "terminal", "final_state"):
                assert (bits(getattr(got, f).astype(np.float64)) == bits(getattr(single, f).astype(np.float64))).all(), f"{what}: {f} against evaluate's"
            assert (got.member_ties == single.ties).all()
    # 65 starts in two groups of three: a second block of the ensemble's grid
    compare(r.evaluate_ensemble(SHORT, 3, rule=rname), wanted(name, "after", ref, ws, 0, 6, 3, rule, SHORT, 0), 0, f"{name}: 65 starts, {rname}", extra)
    assert frozen(r) == was, "an ensemble evaluation changed the context"


@pytest.mark.parametrize("name", sorted(CASES))
def test_query_ensemble(grlx, name):
    """every column on GRID against serial sums over LspiRunner.query's values, groups of 1, 2, 3 and 6"""
    _, r, _, was = context(grlx, name, "after")
    q = r.query(GRID)
    A = q.shape[2]
    for g in (1, 2, 3, 6):
        want = np.zeros((6 // g, len(GRID), 2 + 2 * A))
        for k in range(6 // g):
            for o in range(len(GRID)):
                sv, svv, sq, votes = 0.0, 0.0, [0.0] * A, [0.0] * A
                for m in range(k * g, (k + 1) * g):
                    qm = [float(v) for v in q[m, o]]
                    mai, man = findmax(qm)
                    v = 0.0
                    for a in range(A):
                        v += qm[a] * (1. / man if qm[a] == qm[mai] else 0.)
                    sv, svv, sq = sv + v, svv + v * v, [s + x for s, x in zip(sq, qm)]
                    votes[mai] += 1.0
                want[k, o] = [sv, svv] + sq + votes
        assert (bits(r.query_ensemble_raw(GRID, g)) == bits(want)).all(), f"{name}: groups of {g}"
    assert (bits(r.query_ensemble_raw(GRID, 3, replicas=(3, 3))) == bits(r.query_ensemble_raw(GRID, 3)[1:])).all(), f"{name}: replicas 3 ... 5"
    assert frozen(r) == was


REFUSALS = [(dict(states=None), "states is null"), (dict(n_starts=-1), "n_starts = -1"), (dict(first=4, count=3), "replica range"),
            (dict(max_steps=-1), "max_steps = -1"), (dict(max_steps=100001), "max_steps = 100001"), (dict(nan=(4, 1)), "row 4, component 1 is not finite"),
            (dict(big=(5, 0)), "2^17"), (dict(group=0), "group_size = 0"), (dict(count=5, group=3), "n_replicas = 5 is not a multiple of group_size = 3"),
            (dict(rule=2), "rule = 2"), (dict(max_steps=0, trajectory_only=True), "max_steps = 0"), (dict(records=False, trajectory_only=True), "records is null")]


@pytest.mark.parametrize("over,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals_name_the_call_and_the_reason(grlx, over, word):
    """the four episode calls on sentinel-filled outputs: GRLX_ERR_INVALID, the entry point and the reason named, nothing written"""
    _, r, _, _ = context(grlx, "tri-f27-n5", "after")
    lib, a = grlx.capi.load(), dict(first=0, count=3, group=3, rule=0, states=STARTS.copy(), n_starts=9, max_steps=5, records=True)
    a.update({k: v for k, v in over.items() if k in a})
    if "nan" in over:
        a["states"][over["nan"]] = math.nan
    if "big" in over:
        a["states"][over["big"]] = -2.0 ** 17
    p = lambda x, t=C.c_double: x.ctypes.data_as(C.POINTER(t))
    for ensemble in (False, True):
        if not ensemble and ("group" in over or "rule" in over):
            continue
        for trajectory in (False, True):
            if over.get("trajectory_only") and not trajectory:
                continue
            f64, i32, i64 = [np.full((3, 9, 3), 7.0) for _ in range(3)], [np.full((3, 9), 7, np.int32) for _ in range(3)], [np.full((3, 9), 7, np.int64) for _ in range(2)]
            rec = np.full((3, 9, 5, 13), 7.0)
            name = "grlx_lspi_evaluate" + ("_ensemble" if ensemble else "") + ("_trajectory" if trajectory else "")
            args = [r._ctx, a["first"], a["count"]] + ([a["group"], a["rule"]] if ensemble else []) + \
                [None if a["states"] is None else p(a["states"]), a["n_starts"], a["max_steps"], p(f64[0]), p(f64[1])] + [p(x, C.c_int32) for x in i32] + \
                ([p(x, C.c_int64) for x in i64] if ensemble else []) + [p(f64[2])] + ([p(rec) if a["records"] else None] if trajectory else [])
            rc, said = getattr(lib, name)(*args), lib.grlx_last_error().decode()
            assert rc == grlx.capi.ERR_INVALID and said.startswith(name + ": ") and word in said, (name, said)
            assert all((x == 7).all() for x in f64 + i32 + i64 + [rec]), f"{name}, {word}: something was written"


@pytest.mark.parametrize("over,word", [(dict(obs=None), "obs is null"), (dict(out=None), "out is null"), (dict(n_obs=-1), "n_obs = -1"),
                                       (dict(first=4, count=3), "replica range"), (dict(inf=(2, 1)), "observation row 2, dimension 1 is not finite"),
                                       (dict(group=0), "group_size = 0"), (dict(count=5, group=3), "n_replicas = 5 is not a multiple of group_size = 3")])
def test_query_ensemble_refusals(grlx, over, word):
    _, r, _, _ = context(grlx, "tri-f27-n5", "after")
    lib, a = grlx.capi.load(), dict(first=0, count=3, group=3, obs=GRID[:4].copy(), n_obs=4, out=np.full((3, 4, 8), 7.0))
    a.update({k: v for k, v in over.items() if k in a})
    if "inf" in over:
        a["obs"][over["inf"]] = math.inf
    cols = np.full((3, 4, 8), 7.0) if a["out"] is None else a["out"]
    p = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_double))
    rc, said = lib.grlx_lspi_query_ensemble(r._ctx, a["first"], a["count"], a["group"], p(a["obs"]), a["n_obs"], p(a["out"])), lib.grlx_last_error().decode()
    assert rc == grlx.capi.ERR_INVALID and said.startswith("grlx_lspi_query_ensemble: ") and word in said and (cols == 7.0).all(), said


def test_nothing_to_do_and_the_staging_bound(grlx):
    """n_starts == 0 or n_replicas == 0 is GRLX_OK; the starts two at a time give the same bytes; a column of records beyond the bound is refused"""
    _, r, _, _ = context(grlx, "tri-f27-n5", "after")
    assert r.evaluate(STARTS[:0]).ret.shape == (6, 0) and r.evaluate_ensemble(STARTS, 3, replicas=(0, 0)).ret.shape == (0, 9)
    assert r.query_ensemble_raw(GRID[:0], 2).shape == (3, 0, 8)
    whole, lib = r.evaluate_trajectory(STARTS, 100), grlx.capi.load()
    sums, column = 8 * 3 + (2 * 8 + 3 * 4 + 8 * 3) * 6, 6 * 100 * 11 * 8
    try:
        lib.grlx_set_query_chunk_bytes(2 * (column + sums) + sums)
        assert r.evaluate_trajectory(STARTS, 100).records.tobytes() == whole.records.tobytes()
        lib.grlx_set_query_chunk_bytes(column + sums - 1)
        with pytest.raises(grlx.capi.GrlxError) as ei:
            r.evaluate_trajectory(STARTS, 100)
        assert "grlx_lspi_evaluate_trajectory" in str(ei.value) and "smaller max_steps" in str(ei.value) and "grlx_set_query_chunk_bytes" in str(ei.value)
    finally:
        lib.grlx_set_query_chunk_bytes(0)
