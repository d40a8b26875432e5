"""The batch path's ensemble on the GPU (grlx_fqi_query_ensemble, grlx_fqi_evaluate_ensemble, grlx_fqi_evaluate_ensemble_trajectory) against
tests/fqi_evaluate_ensemble_ref.py, a plain loop over the oracle's observation, the members' Q and the environment step.  Every comparison
is on bit patterns.

The contexts are trained once per module by ONE batch, as tests/test_gpu_fqi_evaluate.py trains its own (whose oracle experiments of the
seeds 3, 4, 5 are shared, never advanced).  What the fitted members do -- which actions the groups take, where their scores tie, how far
the members agree -- is asserted on the REFERENCE's output first (reference_conditions), so that a kernel that ignored its Q-values or
its members could not pass; the figures were worked out on the CPU oracle.

No domain-exit case: the pendulum's damping keeps the angle inside Env::in_domain from every admitted state."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import fqi_evaluate_ensemble_ref as er
from tests import oracle_binding as ob
from tests import test_gpu_fqi_evaluate as single

pytestmark = pytest.mark.gpu

SHAPE = single.SHAPE                         # batch_size=2000, iterations=10, epochs=100
SIX = [3, 4, 5, 6, 7, 8]
BIG_SEEDS = list(range(1, 38))               # 37 members
BIG_SHAPE = dict(batch_size=700, iterations=3, epochs=40)
FULL = single.FULL
RULES = (("vote", er.VOTE), ("mean", er.MEAN_Q))
# (first replica, replicas, group size): sizes 1, 2, 3 and 6 over the replicas 0 ... 5, and 5 over 0 ... 4
GROUPINGS = ((0, 6, 1), (0, 6, 2), (0, 6, 3), (0, 6, 6), (0, 5, 5))

start_states, bits, same_bits = single.start_states, single.bits, single.same_bits


def shape_of(hidden):
    return single.WIDTHS[hidden]


_oracles = {}


def oracle(hidden, seed, shape=None):
    """the oracle experiment of (width, seed) after ONE batch, made once and never advanced again"""
    key = (hidden, seed, shape is not None)
    if key not in _oracles:
        if shape is None and seed in single.SEEDS:
            _oracles[key] = single.oracles(hidden)[single.SEEDS.index(seed)]
        else:
            e = ob.FqiExperiment(ob.pendulum_fqi_spec(hidden=hidden, **(shape or shape_of(hidden))), seed=seed)
            e.run_batch()
            _oracles[key] = e
    return _oracles[key]


def oracles(hidden, seeds, shape=None):
    return [oracle(hidden, s, shape) for s in seeds]


_runners = {}


def runner(grlx, hidden, seeds, shape=None):
    """the context of (width, seeds) after ONE batch, its parameters checked against the oracle's; the tests only query and evaluate it"""
    key = (hidden, tuple(seeds), shape is not None)
    if key not in _runners:
        r = grlx.FqiRunner(grlx.pendulum_fqi_config(len(seeds), max_batches=1, hidden=hidden, **(shape or shape_of(hidden))), list(seeds))
        r.run_batch(); r.sync()
        for k, e in enumerate(oracles(hidden, seeds, shape)):
            same_bits(r.params(k), e.params(), f"hidden = {hidden}, replica {k}: the parameters the episodes run on")
        _runners[key] = r
    return _runners[key]


_references = {}


def reference(hidden, seeds, first, count, group_size, rule, states, max_steps, shape=None):
    """er.evaluate_groups over the replicas [first, first + count) of (width, seeds), computed once per argument list"""
    key = (hidden, tuple(seeds), first, count, group_size, rule, states.tobytes(), max_steps, shape is not None)
    if key not in _references:
        _references[key] = er.evaluate_groups(oracles(hidden, seeds, shape)[first:first + count], group_size, states, rule, max_steps)
    return _references[key]


def indices(recs):
    return set(int(v) for per in recs for r in per for v in r[:, er.ACTION_INDEX])


def compare(got, want, what):
    for k in er.FIELDS:
        same_bits(getattr(got, k), want[k], f"{what}: {k}")


def check_against(r, want, recs, states, first, count, group_size, rule_name, what):
    """evaluate_ensemble (max_steps = 0) and evaluate_ensemble_trajectory (max_steps = 100) of one grouping against the reference"""
    got = r.evaluate_ensemble(states, group_size, rule=rule_name, replicas=(first, count))
    compare(got, want, f"{what}, evaluate_ensemble")
    traj = r.evaluate_ensemble_trajectory(states, group_size, FULL, rule=rule_name, replicas=(first, count))
    compare(traj, want, f"{what}, evaluate_ensemble_trajectory")
    for k in er.FIELDS:
        same_bits(getattr(traj, k), getattr(got, k), f"{what}: {k} of the trajectory call against the sums call's")
    groups = count // group_size
    assert traj.records.shape == (groups, states.shape[0], FULL, er.WORDS) and r.ensemble_trajectory_record_words() == er.WORDS
    for g in range(groups):
        for s in range(states.shape[0]):
            n = int(want["steps"][g, s])
            same_bits(traj.episode(g, s), recs[g][s], f"{what}, group {g}, state {s}: records")
            assert not bits(traj.records[g, s, n:]).any(), f"{what}, group {g}, state {s}: records behind the end are not zero bits"
    assert (traj.step_agreement.sum(axis=2).astype(np.int64) == got.agreement).all(), f"{what}: the records' agreement words against agreement"
    assert (traj.step_member_ties.sum(axis=2).astype(np.int64) == got.member_ties).all(), f"{what}: the records' member ties against member_ties"
    return got, traj


def reference_conditions(hidden):
    """what the issue's table asks of the reference for the six seeds of a width; returns nothing, asserts"""
    states = start_states()
    ref = lambda first, count, g, rule: reference(hidden, SIX, first, count, g, rule, states, 0)
    some_member_tie = False
    for first, count, g in GROUPINGS:
        for _, rule in RULES:
            want, _ = ref(first, count, g, rule)
            some_member_tie |= bool((want["member_ties"] > 0).any())
            if g > 1:
                assert (want["agreement"] < want["steps"].astype(np.int64) * g).any(), f"hidden = {hidden}, {count} in groups of {g}: the members never disagree"
            else:
                assert (want["agreement"] == want["steps"]).all()
    assert some_member_tie, f"hidden = {hidden}: no member ever ties"
    if hidden == 64:
        for count, g in ((6, 3), (5, 5)):                      # the groups {3, 4, 5} and {3, ..., 7}
            want, recs = ref(0, count, g, er.VOTE)
            assert indices(recs[:1]) == {0, 1, 2}, f"VOTE, group of {g}: {indices(recs[:1])}"
            t = want["ties"][0]
            assert ((t >= 7) & (t <= 19)).sum() >= 3, f"VOTE, group of {g}: ties {t}"
        want, _ = ref(0, 6, 2, er.VOTE)                        # the group {3, 4}
        assert (2 * want["ties"][0] > want["steps"][0]).sum() >= 3, f"VOTE, group {{3, 4}}: ties {want['ties'][0]} of {want['steps'][0]} steps"
        want, recs = ref(0, 6, 3, er.MEAN_Q)                   # the group {3, 4, 5}
        assert indices(recs[:1]) == {0, 1, 2} and not want["ties"][0].any()
    if hidden == 8:
        for _, rule in RULES:                                  # the group {3, ..., 8}
            want, recs = ref(0, 6, 6, rule)
            assert len(indices(recs)) == 2 and (want["ties"] > 0).any(), f"hidden = 8, rule {rule}: {indices(recs)}, ties {want['ties']}"


# ---- 1: decisions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [64, 8])
def test_decisions_against_the_reference(grlx, hidden):
    """six replicas (seeds 3 ... 8) in groups of 1, 2, 3, 6 and five of them in one group of 5, both rules, the seven states: all eight
    outputs with max_steps = 0; the trajectory with max_steps = 100: its records, the zero bits behind every end, its sums equal to the
    sums call's, and the per-episode sums of its agreement and member-tie words"""
    reference_conditions(hidden)
    states = start_states()
    r = runner(grlx, hidden, SIX)
    single_policy = r.evaluate(states)
    for first, count, g in GROUPINGS:
        for name, rule in RULES:
            want, recs = reference(hidden, SIX, first, count, g, rule, states, 0)
            got, _ = check_against(r, want, recs, states, first, count, g, name, f"hidden = {hidden}, {count} replicas in groups of {g}, {name}")
            if g == 1:                                         # a group of one is grlx_fqi_evaluate's episode
                for k in ("ret", "disc", "steps", "terminal", "final_state"):
                    same_bits(getattr(got, k), getattr(single_policy, k), f"hidden = {hidden}, groups of one, {name}: {k} against evaluate's")
                assert (got.member_ties == single_policy.ties).all() and (got.agreement == got.steps).all()
                assert (got.ties == (single_policy.ties if rule == er.MEAN_Q else 0)).all()


@pytest.mark.parametrize("hidden", [16, 20, 32])
def test_the_other_widths(grlx, hidden):
    """seeds 3, 4, 5 as one group under MEAN_Q; hidden = 20: the reference takes all three action indices"""
    states = start_states()
    want, recs = reference(hidden, single.SEEDS, 0, 3, 3, er.MEAN_Q, states, 0)
    if hidden == 20:
        assert indices(recs) == {0, 1, 2}
    check_against(runner(grlx, hidden, single.SEEDS), want, recs, states, 0, 3, 3, "mean", f"hidden = {hidden}, one group of three, mean")


# ---- 2: a large group, many groups, and ragged blocks ---------------------------------------------------------------------------------
def big_states():
    base = start_states()
    return np.array([base[i % 7] + [0.01 * (i // 7), 0.0, 0.0] for i in range(67)])


def test_a_large_group_many_groups_and_ragged_blocks(grlx):
    """hidden = 64, 37 members (seeds 1 ... 37), 67 start states (a second block with 61 dead lanes), max_steps = 12 so that code 0 occurs.
    The kernel does not stage its members (it reads each through its block-uniform address), so no group size is a threshold of its
    code: one group of 37 is a long member loop whose 95 KB of parameters no lane could hold, 37 groups of one are blockIdx.y up to 36.
    On the reference: the group of 37 never agrees fully at some episode, and the combined score of the action taken takes more than one
    value under either rule.  Under MEAN_Q the ONE group of 37 takes action index 0 at every one of these steps (worked out on the CPU
    oracle); two indices occur among the 37 groups of one, which is what is asserted, and the group's VALUE words -- sumq[mai], compared
    bit for bit -- are what pins its Q-values."""
    states = big_states()
    r = None
    mean_indices = set()
    for count, g in ((37, 37), (37, 1)):
        for name, rule in RULES:
            want, recs = reference(64, BIG_SEEDS, 0, count, g, rule, states, 12, BIG_SHAPE)
            assert (want["terminal"] == 0).any() and (want["terminal"] == 1).any() and (want["steps"] == 12).any() and (want["steps"] == 1).any()
            if rule == er.MEAN_Q:
                mean_indices |= indices(recs)
            if g == 37:
                assert (want["agreement"] < want["steps"].astype(np.int64) * 37).any()
                values = set(float(v) for per in recs for rec in per for v in rec[rec[:, er.ENS_AGREEMENT] > 0, er.VALUE])
                assert len(values) > 1, "the combined score of the action taken is the same at every step"
            r = r or runner(grlx, 64, BIG_SEEDS, BIG_SHAPE)
            what = f"{count // g} group(s) of {g}, {name}"
            got = r.evaluate_ensemble(states, g, rule=name, max_steps=12)
            compare(got, want, what + ", evaluate_ensemble")
            traj = r.evaluate_ensemble_trajectory(states, g, 12, rule=name)
            compare(traj, want, what + ", evaluate_ensemble_trajectory")
            same_bits(traj.records, np.stack([np.stack(per) for per in recs]), what + ": records, zeros behind the ends included")
    assert len(mean_indices) >= 2, f"MEAN_Q takes one action only: {mean_indices}"


# ---- 3: query_ensemble --------------------------------------------------------------------------------------------------------------------
def serial_columns(q, group_size):
    """out[group][obs][2 + 2A] from q[replica][obs][A] (FqiRunner.query): every sum in ascending replica order into one accumulator"""
    n_rep, n_obs, A = q.shape
    out = np.zeros((n_rep // group_size, n_obs, 2 + 2 * A))
    for g in range(n_rep // group_size):
        for o in range(n_obs):
            sv, svv, sq, votes = 0.0, 0.0, [0.0] * A, [0.0] * A
            for m in range(g * group_size, (g + 1) * group_size):
                qm = [float(x) for x in q[m, o]]
                mai, man = er.findmax(qm)
                v = 0.0
                for a in range(A):
                    v += qm[a] * (1. / man if qm[a] == qm[mai] else 0.)
                sv += v
                svv += v * v
                for a in range(A):
                    sq[a] += qm[a]
                votes[mai] += 1.0
            out[g, o] = [sv, svv] + sq + votes
    return out


def test_query_ensemble(grlx):
    """every column against the serial sums formed from FqiRunner.query, group sizes 1, 3, 6 (hidden = 64, six replicas) and 37 (the 37
    members), on a 5 x 5 grid; the votes at the observations the episodes start from are those of the evaluation's first step"""
    grid = grlx.observation_grid([0.0, -12 * math.pi], [2 * math.pi, 12 * math.pi], [5, 5])
    r6, r37 = runner(grlx, 64, SIX), runner(grlx, 64, BIG_SEEDS, BIG_SHAPE)
    for r, sizes in ((r6, (1, 3, 6)), (r37, (37,))):
        q = r.query(grid)
        for g in sizes:
            raw = r.query_ensemble_raw(grid, g)
            same_bits(raw, serial_columns(q, g), f"groups of {g}: the columns")
            res = r.query_ensemble(grid, g)
            assert (res.votes.sum(axis=-1) == g).all() and res.raw is not None
    same_bits(r6.query_ensemble_raw(grid, 3, replicas=range(3, 6)), serial_columns(r6.query(grid, replicas=range(3, 6)), 3), "replicas 3 ... 5")
    # the first step of the episodes: the observation acted on is the record's, the votes and the summed Q are the query's there
    states = start_states()
    for r, g in ((r6, 3), (r6, 6), (r37, 37)):
        traj = r.evaluate_ensemble_trajectory(states, g, 1, rule="vote")
        mean = r.evaluate_ensemble_trajectory(states, g, 1, rule="mean")
        for k in range(traj.records.shape[0]):
            cols = r.query_ensemble_raw(traj.obs[k, :, 0], g, replicas=(k * g, g))[0]
            sumq, votes = cols[:, 2:2 + 3], cols[:, 2 + 3:]
            for s in range(states.shape[0]):
                mai, man = er.findmax([float(v) for v in votes[s]])
                assert (mai, man) == (int(traj.action_index[k, s, 0]), int(traj.n_max[k, s, 0])), (g, k, s, votes[s])
                assert votes[s, mai] == traj.step_agreement[k, s, 0] == traj.value[k, s, 0]
                mai, man = er.findmax([float(v) for v in sumq[s]])
                assert (mai, man) == (int(mean.action_index[k, s, 0]), int(mean.n_max[k, s, 0])), (g, k, s, sumq[s])
                same_bits(mean.value[k, s, 0:1], sumq[s, mai:mai + 1], f"group of {g}, group {k}, state {s}: sumq[mai] of the first step")
                assert votes[s, mai] == mean.step_agreement[k, s, 0]


# ---- 4: an ensemble evaluation changes nothing ------------------------------------------------------------------------------------------
def test_an_ensemble_evaluation_changes_nothing(grlx):
    """two contexts on the same seeds; one queries, evaluates and records before the first batch and between the batches"""
    over = dict(batch_size=700, iterations=3, epochs=40)
    seeds = [1, 2, 3, 4]
    cfg = grlx.pendulum_fqi_config(len(seeds), max_batches=2, **over)
    r, plain = grlx.FqiRunner(cfg, seeds), grlx.FqiRunner(cfg, seeds)
    states = start_states()
    grid = grlx.observation_grid([0.0, -12 * math.pi], [2 * math.pi, 12 * math.pi], [3, 3])

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

    def use(x):
        x.query_ensemble_raw(grid, 2)
        e = x.evaluate_ensemble(states, 4, rule="vote")
        t = x.evaluate_ensemble_trajectory(states, 2, FULL, rule="mean", replicas=range(2, 4))
        same_bits(t.ret, x.evaluate_ensemble(states, 2, rule="mean", replicas=range(2, 4)).ret, "the trajectory call's ret")
        return e

    first = use(r)                                  # allowed before the first batch: the initial networks
    assert (first.steps[:, 0] == FULL).all()
    same_state(state_of(r), state_of(plain), "before the first batch")
    for x in (r, plain):
        x.run_batch(); x.sync()
    use(r)
    same_state(state_of(r), state_of(plain), "after the first batch")
    for x in (r, plain):
        x.run_batch(); x.sync()
    same_state(state_of(r), state_of(plain), "after the second batch")
    r.close(); plain.close()


# ---- 5: chunked staging -----------------------------------------------------------------------------------------------------------------
def test_chunked_staging(grlx):
    """the 7 states two at a time, sums and records; a bound one byte below a column of records is refused with the remedies named"""
    r, states, g = runner(grlx, 64, SIX), start_states(), 2
    groups = len(SIX) // g
    whole, whole_t = r.evaluate_ensemble(states, g, rule="mean"), r.evaluate_ensemble_trajectory(states, g, FULL, rule="mean")
    sums = 8 * 3 + (2 * 8 + 3 * 4 + 2 * 8 + 8 * 3) * groups      # a start state's staged bytes without records
    column = groups * FULL * er.WORDS * 8
    fields = er.FIELDS
    lib = grlx.capi.load()
    try:
        lib.grlx_set_query_chunk_bytes(2 * sums + sums // 2)
        got = r.evaluate_ensemble(states, g, rule="mean")
        for k in fields:
            same_bits(getattr(got, k), getattr(whole, k), f"chunked evaluate_ensemble: {k}")
        lib.grlx_set_query_chunk_bytes(2 * (column + sums) + sums)
        got = r.evaluate_ensemble_trajectory(states, g, FULL, rule="mean")
        for k in fields + ("records",):
            same_bits(getattr(got, k), getattr(whole_t, k), f"chunked evaluate_ensemble_trajectory: {k}")
        grid = grlx.observation_grid([0.0, -12 * math.pi], [2 * math.pi, 12 * math.pi], [5, 5])
        whole_q = r.query_ensemble_raw(grid, g)
        lib.grlx_set_query_chunk_bytes(0)
        same_bits(whole_q, r.query_ensemble_raw(grid, g), "query_ensemble under the default bound")
        lib.grlx_set_query_chunk_bytes(2 * (8 * 2 + 8 * 8 * groups))
        same_bits(r.query_ensemble_raw(grid, g), whole_q, "query_ensemble two observations at a time")
        lib.grlx_set_query_chunk_bytes(column + sums - 1)
        with pytest.raises(grlx.capi.GrlxError) as ei:
            r.evaluate_ensemble_trajectory(states, g, FULL, rule="mean")
        said = str(ei.value)
        assert ei.value.code == grlx.capi.ERR_INVALID and "grlx_fqi_evaluate_ensemble_trajectory" in said
        assert "fewer replicas" in said and "smaller max_steps" in said and "grlx_set_query_chunk_bytes" in said, said
        same_bits(r.evaluate_ensemble_trajectory(states, g, FULL, rule="mean", replicas=range(0, 2)).records, whole_t.records[:1], "the first remedy")
    finally:
        lib.grlx_set_query_chunk_bytes(0)


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------
SENTINEL = 7.0


def raw_call(grlx, r, first, count, group_size, rule, states, n_starts, max_steps, trajectory=False, records=True):
    """the entry point itself on sentinel-filled outputs: (status, message, were the outputs left alone?)"""
    lib = grlx.capi.load()
    rows, n = max(count, 1), max(n_starts, 1)
    f64 = [np.full((rows, n), SENTINEL) for _ in range(2)] + [np.full((rows, n, 3), SENTINEL)]
    i32 = [np.full((rows, n), 7, np.int32) for _ in range(3)]
    i64 = [np.full((rows, n), 7, np.int64) for _ in range(2)]
    rec = np.full((rows, n, max_steps if 1 <= max_steps <= 64 else 1, er.WORDS), SENTINEL)      # (a max_steps beyond is one this test expects refused)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    sp = None if states is None else p(states, C.c_double)
    args = [r._ctx, first, count, group_size, rule, sp, n_starts, max_steps, p(f64[0], C.c_double), p(f64[1], C.c_double), p(i32[0], C.c_int32),
            p(i32[1], C.c_int32), p(i32[2], C.c_int32), p(i64[0], C.c_int64), p(i64[1], C.c_int64), p(f64[2], C.c_double)]
    if trajectory:
        rc = lib.grlx_fqi_evaluate_ensemble_trajectory(*args, p(rec, C.c_double) if records else None)
    else:
        rc = lib.grlx_fqi_evaluate_ensemble(*args)
    untouched = all((a == SENTINEL).all() for a in f64 + [rec]) and all((a == 7).all() for a in i32 + i64)
    return rc, lib.grlx_last_error().decode(), untouched


def raw_query(grlx, r, first, count, group_size, obs, n_obs):
    lib = grlx.capi.load()
    out = np.full((max(count, 1), max(n_obs, 1), 8), SENTINEL)
    op = None if obs is None else obs.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.grlx_fqi_query_ensemble(r._ctx, first, count, group_size, op, n_obs, out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, lib.grlx_last_error().decode(), bool((out == SENTINEL).all())


def test_refusals(grlx):
    r = runner(grlx, 64, SIX)
    states = start_states()
    nan = states.copy(); nan[4, 1] = float("nan")
    big = states.copy(); big[5, 0] = -2.0 ** 17
    cap = 100000                                # include/grlx.h: GRLX_MAX_EPISODE_STEPS
    cases = [
        (dict(states=None), "states is null"),
        (dict(n_starts=-1), "n_starts = -1"),
        (dict(first=4, count=3), "replica range"),
        (dict(first=-1, count=1, group=1), "replica range"),
        (dict(max_steps=-1), "max_steps = -1"),
        (dict(max_steps=cap + 1), "max_steps = %d" % (cap + 1)),
        (dict(states=nan), "row 4, component 1 is not finite"),
        (dict(states=big), "row 5, component 0"),
        (dict(group=0), "group_size = 0"),
        (dict(group=-2), "group_size = -2"),
        (dict(count=5, group=3), "n_replicas = 5 is not a multiple of group_size = 3"),
        (dict(rule=2), "rule = 2"),
        (dict(rule=-1), "rule = -1"),
    ]
    for trajectory in (False, True):
        who = "grlx_fqi_evaluate_ensemble_trajectory: " if trajectory else "grlx_fqi_evaluate_ensemble: "
        for over, word in cases:
            a = dict(first=0, count=3, group=3, rule=0, states=states, n_starts=7, max_steps=5)
            a.update(over)
            rc, said, untouched = raw_call(grlx, r, a["first"], a["count"], a["group"], a["rule"], a["states"], a["n_starts"], a["max_steps"], trajectory)
            assert rc == grlx.capi.ERR_INVALID and word in said and said.startswith(who), (sorted(over), said)
            assert untouched, f"{word}: something was written"
    rc, said, untouched = raw_call(grlx, r, 0, 3, 3, 0, big, 7, 5)
    assert "2^17" in said
    rc, said, untouched = raw_call(grlx, r, 0, 3, 3, 0, states, 7, 0, trajectory=True)
    assert rc == grlx.capi.ERR_INVALID and "max_steps = 0" in said and untouched
    rc, said, untouched = raw_call(grlx, r, 0, 3, 3, 1, states, 7, 5, trajectory=True, records=False)
    assert rc == grlx.capi.ERR_INVALID and "records is null" in said and untouched
    # the query's
    grid = grlx.observation_grid([0.0, -1.0], [1.0, 1.0], [2, 2])
    inf = grid.copy(); inf[2, 1] = float("inf")
    for a, word in ((dict(obs=None), "obs is null"), (dict(n_obs=-1), "n_obs = -1"), (dict(first=4, count=3), "replica range"),
                    (dict(obs=inf), "observation row 2, dimension 1 is not finite"), (dict(group=0), "group_size = 0"),
                    (dict(count=5, group=3), "n_replicas = 5 is not a multiple of group_size = 3")):
        b = dict(first=0, count=3, group=3, obs=grid, n_obs=4)
        b.update(a)
        rc, said, untouched = raw_query(grlx, r, b["first"], b["count"], b["group"], b["obs"], b["n_obs"])
        assert rc == grlx.capi.ERR_INVALID and word in said and said.startswith("grlx_fqi_query_ensemble: ") and untouched, (sorted(a), said)
    # an empty replica range through the Python layer: the default group size must not turn it into a refusal
    assert r.query_ensemble_raw(grid, replicas=(0, 0)).shape == (0, 4, 8) and r.evaluate_ensemble(states, 3, replicas=(0, 0)).ret.shape == (0, 7)
    # nothing to do is not an error, and writes nothing
    for first, count, n in ((0, 0, 7), (0, 3, 0)):
        for trajectory in (False, True):
            rc, said, untouched = raw_call(grlx, r, first, count, 3, 0, states, n, 5, trajectory)
            assert rc == grlx.capi.OK and untouched
        rc, said, untouched = raw_query(grlx, r, first, count, 3, grid, min(n, 4))
        assert rc == grlx.capi.OK and untouched
    # any output other than the records may be NULL
    lib = grlx.capi.load()
    ret = np.zeros((2, 7))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.grlx_fqi_evaluate_ensemble(r._ctx, 0, 6, 3, 1, dp(states), 7, 0, dp(ret), None, None, None, None, None, None, None) == grlx.capi.OK
    same_bits(ret, r.evaluate_ensemble(states, 3, rule="mean").ret, "ret alone")
    rec = np.zeros((2, 7, 3, er.WORDS))
    assert lib.grlx_fqi_evaluate_ensemble_trajectory(r._ctx, 0, 6, 3, 1, dp(states), 7, 3, None, None, None, None, None, None, None, None,
                                                     dp(rec)) == grlx.capi.OK
    same_bits(rec, r.evaluate_ensemble_trajectory(states, 3, 3, rule="mean").records, "records alone")
