"""The oracle's acrobot, cart-pole (swing-up and balancing tasks), pendulum and compass walker against the reference's OWN sources,
bit for bit.

oracle/_ref/ref_envs is the reference's acrobot.cpp, cart_pole.cpp, pendulum.cpp, SWModel.cpp and compass_walker.cpp, compiled
unmodified against a stand-in framework header (oracle/ref) with -fno-builtin, i.e. evaluated call by call.  In libm arithmetic the
oracle must give that binary's bits on every case of tests/ref_env_cases.py and every command: derivatives (the cart-pole's end-stop
overrides included), RK4 steps, model steps through heel strikes and refused strikes, observations and their wraps, rewards under
every penalty setting, terminal codes, the strike flag, start states under every randomization and the draws a start consumes.

The fixtures under tests/golden/ (what the GPU test reads) must equal a fresh run of the binary, and the portable-mode oracle
(what the kernels reproduce) must stay inside the bounds recorded with them: tools/record_ref_envs.py rewrites all three.

Skipped only where there is neither a checkout of the reference nor a binary; with the sources and no binary the tests fail.
"""
import json
import os

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import ref_env_cases as rc

ENVS = ("acrobot", "walker", "cart_pole", "pendulum")


@pytest.fixture(scope="module")
def binary():
    ob.load()                                                             # make -C oracle: builds the binary where the sources are
    if not os.path.exists(rc.REF_BIN):
        if rc.reference_sources_present():
            pytest.fail(f"the reference's sources are at {rc.REFERENCE} but make -C oracle left no {rc.REF_BIN}")
        pytest.skip("neither the reference's sources nor oracle/_ref/ref_envs on this machine")
    return rc.REF_BIN


_cache = {}


def cached(what, env, make):
    if (what, env) not in _cache:
        _cache[(what, env)] = make()
    return _cache[(what, env)]


def cases_of(env):
    return cached("cases", env, rc.CASES[env])


def reference_of(env):
    return cached("reference", env, lambda: rc.reference_answers(env, cases_of(env)))


def context_starts_of(env):
    return cached("context_starts", env, lambda: rc.context_starts(env))


def assert_same_bits(want, got, keys, what, rows=None):
    for k in keys:
        a, b = np.ascontiguousarray(want[k]), np.ascontiguousarray(got[k])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what} {k}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
        if a.dtype == np.float64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        tags = "" if rows is None else f", tags {sorted({rc.TAGS[t] for t in rows[bad]})}"
        assert bad.size == 0, f"{what} {k}: {bad.size} of {len(a)} rows differ, first {bad[:8]}{tags}: {want[k][bad[0]]!r} vs {got[k][bad[0]]!r}"


@pytest.mark.parametrize("env", ENVS)
def test_libm_oracle_gives_the_reference_binarys_bits_on_every_case(binary, env):
    cases = cases_of(env)
    assert 300 <= len(cases["action"]) <= rc.MAX_ROWS
    got = rc.oracle_answers(env, cases, ob.MATH_LIBM)
    ref = reference_of(env)
    if env == "walker":                                                   # walker_step (the bare model) and walker_model_step agree in the binary itself
        assert_same_bits({"model": ref["model"], "changed": ref["changed"]},
                         {"model": ref["next"][:, [rc.SLA, rc.HA, rc.SLAR, rc.HAR, rc.SFX]], "changed": ref["next"][:, rc.CHANGED].astype(np.int32)},
                         ("model", "changed"), "reference model against its CompassWalkerModel::step")
        ref, got = dict(ref), dict(got)
        ref["next"], got["next"] = ref["next"][:, rc.WALKER_COMPARED], got["next"][:, rc.WALKER_COMPARED]
    assert_same_bits(ref, got, rc.ANSWER_KEYS[env], env, rows=cases["tag"])


@pytest.mark.parametrize("env", ENVS)
def test_libm_oracle_starts_equal_the_reference_binarys(binary, env):
    """64 seeds x {learn, test} from srand48(seed): start states, first observations and the stream position after the start
    (the draws the walker's rejection sampling consumed).  The walker's go through `walker_start seed test` (srand48 inside the
    binary) as well as through the position."""
    starts = rc.seeded_starts_of(env)
    ref = rc.reference_starts(env, starts)
    got = rc.oracle_starts(env, starts, ob.MATH_LIBM)
    assert_same_bits(ref, got, ("x", "obs", "position_after"), f"{env} starts")
    if env == "walker":
        for test in (0, 1):
            x, after = rc.reference_seeded_walker_starts(rc.START_SEEDS, test)
            rows = slice(test * rc.N_STARTS, (test + 1) * rc.N_STARTS)
            assert_same_bits({"x": x, "position_after": after}, {"x": got["x"][rows], "position_after": got["position_after"][rows]},
                             ("x", "position_after"), f"walker_start seed {test}")
        draws = []
        L = ob.load()
        for before, after in zip(starts["position"][: rc.N_STARTS], got["position_after"][: rc.N_STARTS]):
            g, n = ob.Rand48(int(before)), 0
            while g.x != int(after) and n < 400:
                L.orc_drand48(g); n += 1
            draws.append(n)
        assert set(draws) <= set(range(4, 400, 4)) and max(draws) > 4, "learning starts: whole rounds of four draws, some rejected"
        assert (got["x"][rc.N_STARTS:] == got["x"][rc.N_STARTS]).all(), "test starts do not vary"


@pytest.mark.parametrize("env", ENVS)
def test_context_starts_equal_the_reference_binarys(binary, env):
    """the stream positions at which a 64-replica context starts its first learning and its first test episode (the GPU test's)"""
    starts = context_starts_of(env)
    assert_same_bits(rc.reference_starts(env, starts), rc.oracle_starts(env, starts, ob.MATH_LIBM), ("x", "obs", "position_after"), f"{env} context starts")


@pytest.mark.parametrize("env", ENVS)
def test_fixtures_equal_a_fresh_run_and_the_portable_oracle_stays_inside_the_recorded_bounds(binary, env):
    fx = np.load(rc.FIXTURE[env])
    with open(rc.BOUNDS) as f:
        recorded = json.load(f)[env]
    cases, ref = cases_of(env), reference_of(env)
    assert_same_bits(cases, fx, tuple(cases), f"{env} fixture inputs")
    assert_same_bits(ref, fx, ("next", "obs", "reward", "term"), f"{env} fixture outputs")
    starts = context_starts_of(env)
    sref = rc.reference_starts(env, starts)
    assert_same_bits(dict(starts, **sref), {k[6:]: fx[k] for k in fx.files if k.startswith("start_")}, tuple(starts) + ("x", "obs", "position_after"), f"{env} fixture starts")
    # the portable oracle: discrete outcomes equal on all but 1 % of the rows, by the oracle alone, and the rest inside the bounds
    portable = rc.oracle_answers(env, cases, ob.MATH_PORTABLE)
    excluded = rc.discrete_mismatch(env, ref, portable)
    assert excluded.sum() <= len(excluded) // 100, f"{excluded.sum()} rows differ in a discrete outcome: {np.nonzero(excluded)[0]}"
    assert (excluded == fx["excluded"]).all() and excluded.sum() == recorded["excluded_rows"]
    assert rc.within(env, ref, portable, excluded, recorded["bounds"], 1.0) == []
    sportable = rc.oracle_starts(env, starts, ob.MATH_PORTABLE)
    sexcluded = sref["position_after"] != sportable["position_after"]
    assert sexcluded.sum() <= len(sexcluded) // 100 and (sexcluded == fx["start_excluded"]).all()
    assert rc.starts_within(env, sref, sportable, sexcluded, recorded["start_bounds"], 1.0) == []
    for path in (rc.FIXTURE[env], rc.BOUNDS):
        assert os.path.getsize(path) < 100 * 1024


def test_randomized_starts_vary_and_plain_ones_do_not(binary):
    """the cases of the start tests are what they are there for: the cart-pole's and the pendulum's starts under randomization 1 differ
    from seed to seed (the pendulum's test starts do not), and under randomization 0 the draw is consumed all the same"""
    for env in ("cart_pole", "pendulum"):
        starts = rc.seeded_starts_of(env)
        ref = rc.reference_starts(env, starts)
        angle = ref["x"][:, 1 if env == "cart_pole" else 0]
        plain, learn = starts["randomization"] == 0, starts["test"] == 0
        assert (angle[plain] == np.pi).all() and (ref["position_after"] != starts["position"]).all()
        varies = ~plain & (learn | (env == "cart_pole"))
        assert len(set(angle[varies])) == len(set(starts["position"][varies])) == rc.N_STARTS and (angle[~plain & ~varies] == np.pi).all()


def test_cart_pole_balancing_task_equals_the_reference_binarys(binary):
    """task/cart_pole/balancing's source is in the binary too: observe, evaluate and start on the cart-pole's cases, whose positions
    and angles lie on both sides of its two failure thresholds"""
    import ctypes as C
    L = ob.load()
    spec = ob.cart_pole_balancing_pid_spec(math=ob.MATH_LIBM)
    cases, ref = cases_of("cart_pole"), reference_of("cart_pole")
    state = np.concatenate([cases["state"], cases["state"] * [1, 0.01, 1, 1, 1]])          # the second half: angles about the 12 degrees
    nxt = np.concatenate([ref["next"], ref["next"] * [1, 0.01, 1, 1, 1]])
    action = np.concatenate([cases["action"], cases["action"]])
    lines = [f"balancing_task {rc.hexes(spec.timeout)}"]
    for x, u, y in zip(state, action, nxt):
        lines += [f"balancing_observe {rc.hexes(y)}", f"balancing_evaluate {rc.hexes(x)} {rc.hexes(u)} {rc.hexes(y)}"]
    answers = rc.ask(lines)[1:]
    want = dict(obs=np.array([rc.floats(a[:4]) for a in answers[0::2]]), term=np.array([int(a[4]) for a in answers[0::2]], np.int32),
                reward=np.array([rc.floats(a)[0] for a in answers[1::2]]))
    got = dict(obs=np.zeros((len(state), 4)), term=np.zeros(len(state), np.int32), reward=np.zeros(len(state)))
    for i, (x, u, y) in enumerate(zip(state, action, nxt)):
        o = (C.c_double * 4)()
        got["term"][i] = L.orc_env_observe(C.byref(spec), (C.c_double * 5)(*y), o); got["obs"][i] = o[:]
        got["reward"][i] = L.orc_env_evaluate(C.byref(spec), (C.c_double * 5)(*x), float(u), (C.c_double * 5)(*y))
    assert_same_bits(want, got, ("obs", "term", "reward"), "balancing task")
    assert {0, 1, 2} <= set(want["term"]) and (want["reward"] == 0).any() and ((want["reward"] > 0) & (want["reward"] < 1)).any()
    fallen = np.abs(nxt[:, 1]) > 12 * np.pi / 180
    assert (fallen & (np.abs(nxt[:, 0]) <= 2.4)).any() and (~fallen & (np.abs(nxt[:, 0]) > 2.4)).any() and (~fallen & (np.abs(nxt[:, 0]) <= 2.4)).any()
    starts = rc.seeded_starts()
    draws, after = [], []
    for pos in starts["position"][: rc.N_STARTS]:
        g = ob.Rand48(int(pos))
        draws.append(L.orc_drand48(C.byref(g))); after.append(g.x)
    x = np.array([rc.floats(a) for a in rc.ask([f"balancing_start {rc.hexes(d)}" for d in draws])])
    mine = np.zeros((rc.N_STARTS, 5)); mine_after = []
    for i, pos in enumerate(starts["position"][: rc.N_STARTS]):
        g, tl, xs = C.c_uint64(0), C.c_uint64(int(pos)), (C.c_double * 5)()
        L.orc_env_start_at(C.byref(spec), C.byref(g), C.byref(tl), 0, xs)
        mine[i] = xs[:]; mine_after.append(tl.value)
    assert_same_bits({"x": x}, {"x": mine}, ("x",), "balancing starts")
    assert mine_after == after and len(set(x[:, 1])) == rc.N_STARTS and (np.abs(x[:, 1]) <= 0.05).all()
