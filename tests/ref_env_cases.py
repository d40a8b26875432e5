"""Case sets that hold the acrobot, the cart-pole swing-up, the pendulum and the compass walker against the reference's OWN sources
(oracle/_ref/ref_envs, built by oracle/Makefile from the unmodified reference files), shared by tests/test_oracle_ref_envs.py (CPU: oracle against the binary),
tools/record_ref_envs.py (writes the fixtures under tests/golden/) and tests/test_gpu_ref_envs.py (GPU: kernels against the
fixtures).  Fixed seeds, no clock; the configurations are those of tests/configs.py.

A case set is a dict: state [n, S], action [n], tag [n] (index into TAGS: what the row is there for) and, for the cart-pole, variant [n]
(bit 0: end_stop_penalty, bit 1: action_penalty: the task a row runs under).  The reference's answers
and the oracle's answers to a case set are dicts with the same keys (ANSWER_KEYS), so that every comparison is one loop.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import configs
from tests import oracle_binding as ob

ROOT = ob.ROOT
REF_BIN = os.path.join(ob.ORACLE_DIR, "_ref", "ref_envs")
REF_BIN_FUSED = os.path.join(ob.ORACLE_DIR, "_ref", "ref_envs_fused")        # the same sources at plain -O2 (sin/cos fused into sincos)
REFERENCE = os.environ.get("REFERENCE", "/root/reference")                   # oracle/Makefile's default
REF_SOURCES = [os.path.join(REFERENCE, "base", "src", "environments", f) for f in
               ("acrobot.cpp", "cart_pole.cpp", "pendulum.cpp", os.path.join("compass_walker", "SWModel.cpp"),
                os.path.join("compass_walker", "compass_walker.cpp"))]
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = {env: os.path.join(GOLDEN, f"ref_envs_{env}.npz") for env in ("acrobot", "walker", "cart_pole", "pendulum")}
BOUNDS = os.path.join(GOLDEN, "ref_envs_bounds.json")

MAX_ROWS = 512
N_STARTS = 64
START_SEEDS = np.arange(1, N_STARTS + 1)
START_MEMORY = 32768            # table size of the 64-replica start contexts: the oracle draws `memory` initial weights per replica

# compass walker state (compass_walker.h:40-42)
SLA, HA, SLAR, HAR, CHANGED, SFX, LASTHIPX, HIPVEL, STEPDIST, TIME, TIMEOUT = range(11)
# CompassWalkerModel::step never writes the step distance (uninitialised in the reference, kept by the oracle): not compared
WALKER_COMPARED = [i for i in range(11) if i != STEPDIST]

TAGS = ["balancing", "angle1_threshold", "angle2_threshold", "rate1_limit", "rate2_limit", "timeout", "swinging",
        "walking", "strike", "refused_hip_sign", "refused_stance_rate", "refused_hip_angle", "wrap", "fallen_stance", "fallen_hip",
        "search_exhausted",
        "episode", "end_stop", "end_stop_edge", "failed_threshold", "observe_wrap", "potential_wrap", "action_penalty", "far",
        "rate_range", "turns", "observe_wrap_step", "clamped"]
TAG = {t: i for i, t in enumerate(TAGS)}

DYNAMICAL = {"acrobot": dict(S=5, D=4, prefix="acrobot"), "cart_pole": dict(S=5, D=4, prefix="cartpole"), "pendulum": dict(S=3, D=2, prefix="pendulum")}
THREAD_LOCAL_STARTS = ("acrobot", "cart_pole", "pendulum")                   # environments whose start draws from RandGen, not from drand48
ANSWER_KEYS = {"acrobot": ("xd", "obs0", "term0", "next", "obs", "term", "reward"),
               "cart_pole": ("xd", "obs0", "term0", "next", "obs", "term", "reward"),
               "pendulum": ("xd", "obs0", "term0", "next", "obs", "term", "reward"),
               "walker": ("model", "changed", "obs0", "term0", "next", "obs", "term", "reward")}


CONFIGS = {"acrobot": configs.acrobot, "walker": configs.compass_walker, "cart_pole": configs.cart_pole_ac, "pendulum": configs.pendulum}


def spec_of(env, math, variant=0, randomization=None):
    spec = CONFIGS[env](None, 1)[1]
    spec.math = math
    if env == "cart_pole":
        spec.end_stop_penalty, spec.action_penalty = int(variant) & 1, (int(variant) >> 1) & 1
    if randomization is not None:
        spec.randomization = float(randomization)
    return spec


def _per_variant(answer, cases):
    """answer(rows of one variant, variant) for every variant of the case set, put back in the rows' order"""
    variant = cases.get("variant")
    if variant is None:
        return answer(cases, 0)
    out = {}
    for v in np.unique(variant):
        rows = np.nonzero(variant == v)[0]
        part = answer({k: a[rows] for k, a in cases.items()}, int(v))
        for k, a in part.items():
            out.setdefault(k, np.zeros((len(variant),) + a.shape[1:], a.dtype))[rows] = a
    return out


def reference_sources_present():
    return all(os.path.exists(p) for p in REF_SOURCES)


# ------------------------------------------------------------------------------------------------ the reference ---
def hexes(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel())


def ask(lines, binary=REF_BIN):
    """One answer (a list of words) per command line."""
    out = subprocess.run([binary], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines), f"{binary}: {len(out)} answers to {len(lines)} commands"
    for line, answer in zip(lines, out):
        assert not answer.startswith("error"), f"{line.split()[0]}: {answer}"
    return [answer.split() for answer in out]


def floats(words):
    return [float.fromhex(w) for w in words]


def task_lines(env, spec):
    """the commands that configure the reference's task as the spec says"""
    if env == "cart_pole":
        return [f"cartpole_task {hexes(spec.timeout)} {int(spec.randomization)} {spec.end_stop_penalty} {spec.action_penalty}"]
    if env == "pendulum":
        return [f"pendulum_task {hexes(spec.timeout)} {hexes(spec.randomization)}"]
    return []


def _reference_dynamical(env, cases, variant, binary):
    """eom, the task's observation of the state, control_step / integration_steps RK4 sub-steps around the reference's eom (under
    the task's actuation), the observation of the result and the reward of the transition"""
    state, action = cases["state"], cases["action"]
    spec = spec_of(env, ob.MATH_LIBM, variant)
    p, D = DYNAMICAL[env]["prefix"], DYNAMICAL[env]["D"]
    h, steps = spec.control_step / spec.integration_steps, spec.integration_steps
    setup = task_lines(env, spec)
    actuation = action
    if env == "pendulum":                                                 # Task::actuate: the others pass the action through (environment.h:94)
        actuation = np.array([floats(a)[0] for a in ask([f"pendulum_actuate {hexes(u)}" for u in action], binary)])
    first = ask(setup + [c for x, u in zip(state, actuation) for c in
                         (f"{p}_eom {hexes(x)} {hexes(u)}", f"{p}_observe {hexes(x)}", f"{p}_step {hexes(x)} {hexes(u)} {hexes(h)} {steps}")], binary)[len(setup):]
    xd = np.array([floats(a) for a in first[0::3]])
    obs0 = np.array([floats(a[:D]) for a in first[1::3]]); term0 = np.array([int(a[D]) for a in first[1::3]], np.int32)
    nxt = np.array([floats(a) for a in first[2::3]])
    second = ask(setup + [c for x, u, y in zip(state, action, nxt) for c in
                          (f"{p}_observe {hexes(y)}", f"{p}_evaluate {hexes(x)} {hexes(u)} {hexes(y)}")], binary)[len(setup):]
    obs = np.array([floats(a[:D]) for a in second[0::2]]); term = np.array([int(a[D]) for a in second[0::2]], np.int32)
    reward = np.array([floats(a)[0] for a in second[1::2]])
    return dict(xd=xd, obs0=obs0, term0=term0, next=nxt, obs=obs, term=term, reward=reward)


def reference_answers(env, cases, binary=REF_BIN):
    state, action = cases["state"], cases["action"]
    n = len(action)
    if env in DYNAMICAL:
        return _per_variant(lambda part, variant: _reference_dynamical(env, part, variant, binary), cases)
    spec = spec_of("walker", ob.MATH_LIBM)
    setup = [f"walker_model {hexes(spec.slope_angle)} {hexes(spec.control_step)} {spec.integration_steps}",
             f"walker_task {hexes(spec.timeout)} {hexes(spec.initial_state_variation)} {hexes(spec.slope_angle)} {hexes(spec.negative_reward)}"]
    first = ask(setup + [c for x, u in zip(state, action) for c in
                         (f"walker_step {hexes(spec.slope_angle)} {hexes(spec.control_step)} {spec.integration_steps} {hexes(x[[SLA, HA, SLAR, HAR, SFX]])} {hexes(u)}",
                          f"walker_model_step {hexes(x)} {hexes(u)}", f"walker_observe {hexes(x)}")], binary)[2:]
    model = np.array([floats(a[:5]) for a in first[0::3]]); changed = np.array([int(a[5]) for a in first[0::3]], np.int32)
    nxt = np.array([floats(a) for a in first[1::3]])
    nxt[:, STEPDIST] = state[:, STEPDIST]
    obs0 = np.array([floats(a[:5]) for a in first[2::3]]); term0 = np.array([int(a[5]) for a in first[2::3]], np.int32)
    second = ask(setup + [c for x, u, y in zip(state, action, nxt) for c in
                          (f"walker_observe {hexes(y)}", f"walker_evaluate {hexes(x)} {hexes(u)} {hexes(y)}")], binary)[2:]
    obs = np.array([floats(a[:5]) for a in second[0::2]]); term = np.array([int(a[5]) for a in second[0::2]], np.int32)
    reward = np.array([floats(a)[0] for a in second[1::2]])
    assert n == len(reward)
    return dict(model=model, changed=changed, obs0=obs0, term0=term0, next=nxt, obs=obs, term=term, reward=reward)


def reference_starts(env, starts, binary=REF_BIN):
    """starts: position [n] (48-bit generator state: the thread-local one for the acrobot, drand48's for the walker), test [n].
    -> x [n, S], obs [n, D], position_after [n]"""
    L = ob.load()
    if env == "acrobot":
        lines, after = [], []
        for pos in starts["position"]:
            g = ob.Rand48(int(pos))
            lines.append(f"acrobot_start {hexes([L.orc_drand48(C.byref(g)), L.orc_drand48(C.byref(g))])}")
            after.append(g.x)
        x = np.array([floats(a) for a in ask(lines, binary)])
        obs = np.array([floats(a[:4]) for a in ask([f"acrobot_observe {hexes(r)}" for r in x], binary)])
        return dict(x=x, obs=obs, position_after=np.array(after, np.uint64))
    if env in DYNAMICAL:                                                  # one RandGen draw; the task re-configured where the randomization changes
        p, D = DYNAMICAL[env]["prefix"], DYNAMICAL[env]["D"]
        lines, after, answers_at = [], [], []
        for pos, test, rand in zip(starts["position"], starts["test"], starts["randomization"]):
            g = ob.Rand48(int(pos))
            d = L.orc_drand48(C.byref(g))
            lines += task_lines(env, spec_of(env, ob.MATH_LIBM, randomization=rand))
            answers_at.append(len(lines))
            lines.append(f"{p}_start {hexes(d)}" + (f" {int(test)}" if env == "pendulum" else ""))
            after.append(g.x)
        answers = ask(lines, binary)
        x = np.array([floats(answers[i]) for i in answers_at])
        obs = np.array([floats(a[:D]) for a in ask(task_lines(env, spec_of(env, ob.MATH_LIBM)) + [f"{p}_observe {hexes(r)}" for r in x], binary)[1:]])
        return dict(x=x, obs=obs, position_after=np.array(after, np.uint64))
    spec = spec_of("walker", ob.MATH_LIBM)
    setup = [f"walker_task {hexes(spec.timeout)} {hexes(spec.initial_state_variation)} {hexes(spec.slope_angle)} {hexes(spec.negative_reward)}"]
    answers = ask(setup + [f"walker_start_at {int(p)} {int(t)}" for p, t in zip(starts["position"], starts["test"])], binary)[1:]
    x = np.array([floats(a[:11]) for a in answers])
    obs = np.array([floats(a[:5]) for a in ask(setup + [f"walker_observe {hexes(r)}" for r in x], binary)[1:]])
    return dict(x=x, obs=obs, position_after=np.array([int(a[11]) for a in answers], np.uint64))


def reference_seeded_walker_starts(seeds, test, binary=REF_BIN):
    """srand48(seed), then the task's start: x [n, 11], position_after [n]"""
    answers = ask([f"walker_start {int(s)} {int(test)}" for s in seeds], binary)
    return np.array([floats(a[:11]) for a in answers]), np.array([int(a[11]) for a in answers], np.uint64)


# --------------------------------------------------------------------------------------------------- the oracle ---
def _arr(n):
    return (C.c_double * n)()


def oracle_answers(env, cases, math):
    return _per_variant(lambda part, variant: _oracle_answers(env, part, math, variant), cases)


def _oracle_answers(env, cases, math, variant):
    L = ob.load()
    spec = spec_of(env, math, variant)
    state, action = cases["state"], cases["action"]
    n, S, D = len(action), state.shape[1], L.orc_env_obs_dims(spec.env)
    obs0 = np.zeros((n, D)); term0 = np.zeros(n, np.int32)
    for i in range(n):
        o = _arr(D)
        term0[i] = L.orc_env_observe(C.byref(spec), (C.c_double * S)(*state[i]), o); obs0[i] = o[:]
    nxt, obs, reward, term = ob.env_step(spec, state, action)             # the composed step, as the kernels restate it
    out = dict(obs0=obs0, term0=term0, next=nxt, obs=obs, term=term, reward=reward)
    if env in DYNAMICAL:
        xd = np.zeros((n, S)); integrated = np.zeros((n, S)); evaluated = np.zeros(n)
        h, steps = spec.control_step / spec.integration_steps, spec.integration_steps
        for i in range(n):
            x = (C.c_double * S)(*state[i]); d = _arr(S); y = _arr(S)
            u = min(max(float(action[i]), -3.0), 3.0) if env == "pendulum" else float(action[i])    # the step's own actuation is inside orc_env_step
            L.orc_env_eom(C.byref(spec), x, u, d); xd[i] = d[:]
            L.orc_env_integrate(C.byref(spec), x, u, h, steps, y); integrated[i] = y[:]
            evaluated[i] = L.orc_env_evaluate(C.byref(spec), x, float(action[i]), y)
        assert (integrated.view(np.uint64) == nxt.view(np.uint64)).all() and (evaluated == reward).all(), "orc_env_step is not its pieces"
        out["xd"] = xd
    else:
        out["model"] = nxt[:, [SLA, HA, SLAR, HAR, SFX]].copy()
        out["changed"] = nxt[:, CHANGED].astype(np.int32)
    return out


def oracle_starts(env, starts, math):
    L = ob.load()
    spec = spec_of(env, math)
    S, D = L.orc_env_state_dims(spec.env), L.orc_env_obs_dims(spec.env)
    n = len(starts["position"])
    x = np.zeros((n, S)); obs = np.zeros((n, D)); after = np.zeros(n, np.uint64)
    thread_local = env in THREAD_LOCAL_STARTS
    for i, (pos, test) in enumerate(zip(starts["position"], starts["test"])):
        if "randomization" in starts:
            spec.randomization = float(starts["randomization"][i])
        g, tl = C.c_uint64(0), C.c_uint64(0)
        (tl if thread_local else g).value = int(pos)
        xs, o = _arr(S), _arr(D)
        L.orc_env_start_at(C.byref(spec), C.byref(g), C.byref(tl), int(test), xs)
        L.orc_env_observe(C.byref(spec), xs, o)
        x[i] = xs[:]; obs[i] = o[:]; after[i] = (tl if thread_local else g).value
    return dict(x=x, obs=obs, position_after=after)


def seeded_position(seed):
    """the generator state srand48(seed) leaves"""
    g = ob.Rand48()
    ob.load().orc_srand48(C.byref(g), int(seed))
    return g.x


def seeded_starts():
    """Starts: 64 seeds x {learn, test}, each from srand48(seed)."""
    pos = np.array([seeded_position(s) for s in START_SEEDS], np.uint64)
    return dict(position=np.concatenate([pos, pos]), test=np.repeat([0, 1], N_STARTS).astype(np.int32))


START_RANDOMIZATION = {"cart_pole": (0.0, 1.0), "pendulum": (0.0, 1.0)}     # the tasks that have one: a context per value


def seeded_starts_of(env):
    """seeded_starts, once per randomization where the task has one"""
    starts = seeded_starts()
    if env not in START_RANDOMIZATION:
        return starts
    rands = START_RANDOMIZATION[env]
    return dict(position=np.tile(starts["position"], len(rands)), test=np.tile(starts["test"], len(rands)),
                randomization=np.repeat(rands, len(starts["test"])))


def context_starts(env):
    """The first learning start and the test start after it of a 64-replica context (seeds START_SEEDS, tables of START_MEMORY
    slots): the stream positions at which grlx_env_start draws, which are the oracle experiment's after its construction.  Where the
    task has a randomization, one context per value of START_RANDOMIZATION, one after the other."""
    out = dict(position=[], test=[])
    for rand in START_RANDOMIZATION.get(env, (None,)):
        spec = spec_of(env, ob.MATH_LIBM, randomization=rand)
        spec.projector.memory = spec.actor_projector.memory = START_MEMORY
        which = 1 if env in THREAD_LOCAL_STARTS else 0                    # thread-local / global stream (orc_rng_states)
        pos = {0: [], 1: []}
        for seed in START_SEEDS:
            e = ob.Experiment(spec, seed=int(seed))
            for test in (0, 1):
                pos[test].append(e.rng()[which])
                e.env_start(test)
            e.close()
        out["position"] += pos[0] + pos[1]; out["test"] += [0] * N_STARTS + [1] * N_STARTS
        if rand is not None:
            out.setdefault("randomization", []).extend([rand] * (2 * N_STARTS))
    starts = dict(position=np.array(out["position"], np.uint64), test=np.array(out["test"], np.int32))
    if "randomization" in out:
        starts["randomization"] = np.array(out["randomization"], np.float64)
    return starts


# ------------------------------------------------------------------------------------------- groups and bounds ---
def groups(env, answers, rows=None):
    """{group: flat array} of the continuous outputs that the oracle, the fixtures and the kernels have in common (next, obs,
    reward), over `rows` (a mask).  The walker's groups come apart for rows whose step heel-strikes (reference's flag in `rows`)."""
    nxt, obs, reward = answers["next"], answers["obs"], answers["reward"]
    if rows is not None:
        nxt, obs, reward = nxt[rows], obs[rows], reward[rows]
    if env == "acrobot":
        return {"angles": np.concatenate([nxt[:, 0:2].ravel(), obs[:, 0:2].ravel()]),
                "rates": np.concatenate([nxt[:, 2:4].ravel(), obs[:, 2:4].ravel()]),
                "time": nxt[:, 4].ravel(), "reward": reward.ravel()}
    if env == "cart_pole":
        return {"positions": np.concatenate([nxt[:, 0].ravel(), obs[:, 0].ravel()]), "angles": np.concatenate([nxt[:, 1].ravel(), obs[:, 1].ravel()]),
                "rates": np.concatenate([nxt[:, 2:4].ravel(), obs[:, 2:4].ravel()]), "time": nxt[:, 4].ravel(), "reward": reward.ravel()}
    if env == "pendulum":
        return {"angles": np.concatenate([nxt[:, 0].ravel(), obs[:, 0].ravel()]), "rates": np.concatenate([nxt[:, 1].ravel(), obs[:, 1].ravel()]),
                "time": nxt[:, 2].ravel(), "reward": reward.ravel()}
    return {"angles": np.concatenate([nxt[:, [SLA, HA]].ravel(), obs[:, [0, 1]].ravel()]),
            "rates": np.concatenate([nxt[:, [SLAR, HAR, HIPVEL]].ravel(), obs[:, [2, 3]].ravel()]),
            "positions": nxt[:, [SFX, LASTHIPX]].ravel(), "time": nxt[:, [TIME, TIMEOUT]].ravel(), "reward": reward.ravel()}


def start_groups(env, answers, rows=None):
    x, obs = answers["x"], answers["obs"]
    if rows is not None:
        x, obs = x[rows], obs[rows]
    fake = dict(next=x, obs=obs, reward=np.zeros(len(x)))
    g = groups(env, fake)
    del g["reward"]
    return g


WRAPPED_OBS = {"cart_pole": 1, "pendulum": 0}


def discrete_mismatch(env, ref, got):
    """rows on which two answers differ in a discrete outcome: a terminal code, the strike flag, or the turn the wrapped angle of the
    cart-pole's and the pendulum's observation was taken on (the two sides of the wrap are 2 pi apart)"""
    bad = ref["term"] != got["term"]
    if env in WRAPPED_OBS:
        bad |= np.abs(ref["obs"][:, WRAPPED_OBS[env]] - got["obs"][:, WRAPPED_OBS[env]]) > np.pi
    if env == "walker":
        bad |= (ref["next"][:, CHANGED] != got["next"][:, CHANGED]) | (ref["obs"][:, 4] != got["obs"][:, 4])
    return bad


def deviations(env, ref, got, excluded):
    """largest absolute deviation per group (the walker: per strike / no_strike and group) over the rows that are not excluded"""
    def dev(rows):
        a, b = groups(env, ref, rows), groups(env, got, rows)
        return {k: float(np.max(np.abs(a[k] - b[k]))) if a[k].size else 0.0 for k in a}
    if env != "walker":
        return dev(~excluded)
    strike = ref["next"][:, CHANGED] > 0.5
    return {"strike": dev(strike & ~excluded), "no_strike": dev(~strike & ~excluded)}


def start_deviations(env, ref, got, excluded):
    a, b = start_groups(env, ref, ~excluded), start_groups(env, got, ~excluded)
    return {k: float(np.max(np.abs(a[k] - b[k]))) if a[k].size else 0.0 for k in a}


def within(env, ref, got, excluded, bounds, factor):
    """[(what, deviation, allowed)] for every group that exceeds factor * its recorded bound"""
    found = deviations(env, ref, got, excluded)
    pairs = [(k, found[k], bounds[k]) for k in found] if env != "walker" else \
            [(f"{s}/{k}", found[s][k], bounds[s][k]) for s in found for k in found[s]]
    return [(k, d, factor * b) for k, d, b in pairs if not d <= factor * b]


def starts_within(env, ref, got, excluded, bounds, factor):
    found = start_deviations(env, ref, got, excluded)
    return [(k, d, factor * bounds[k]) for k, d in found.items() if not d <= factor * bounds[k]]


# ------------------------------------------------------------------------------------------------ acrobot cases ---
ACROBOT_TORQUES = [-1.0, 0.0, 1.0, 0.37, -0.731, 0.0521]                 # the grid of configs.acrobot and three off-grid torques
FAIL_ANGLE = 12 * np.pi / 180


def _bisect(margin_of, lo, hi, gap=1e-9):
    """two parameters, `gap` apart at most, at which margin_of has different signs"""
    flo, fhi = margin_of(lo), margin_of(hi)
    assert (flo < 0) != (fhi < 0), "the bracket does not straddle the threshold"
    while abs(hi - lo) > gap:
        mid = 0.5 * (lo + hi)
        if (margin_of(mid) < 0) == (flo < 0):
            lo = mid
        else:
            hi = mid
    return lo, hi


def acrobot_cases():
    rng = np.random.default_rng(20150818)
    L = ob.load()
    spec = spec_of("acrobot", ob.MATH_LIBM)
    rows, tags = [], []

    def add(tag, x, u):
        rows.append(list(x) + [u]); tags.append(TAG[tag])

    def step(x, u):
        return ob.env_step(spec, [x], [u])[0][0]

    for i in range(96):                                                   # the balancing region, every torque
        add("balancing", [np.pi + rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), rng.uniform(-0.6, 0.6), rng.uniform(-1.1, 1.1),
                          rng.uniform(0, 19)], ACROBOT_TORQUES[i % 6])
    for c, tag in ((0, "angle1_threshold"), (1, "angle2_threshold")):     # next step lands just inside / just outside 12 degrees
        for sign in (1.0, -1.0):
            for k in range(4):
                base = np.array([np.pi + rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), rng.uniform(-0.6, 0.6), rng.uniform(-1.1, 1.1), rng.uniform(0, 19)])
                u = ACROBOT_TORQUES[(2 * k + c) % 6]
                centre = np.pi if c == 0 else 0.0

                def at(p):
                    x = base.copy(); x[c] = centre + sign * p
                    return x
                lo, hi = _bisect(lambda p: abs(step(at(p), u)[c] - centre) - FAIL_ANGLE, 0.0, 0.35)
                add(tag, at(lo), u); add(tag, at(hi), u)
    for c, limit, tag in ((2, 4 * np.pi, "rate1_limit"), (3, 9 * np.pi, "rate2_limit")):   # at, just below and just above +-limit
        for sign in (1.0, -1.0):
            for value in (limit, np.nextafter(limit, 0), np.nextafter(limit, np.inf)):
                for k in range(8):
                    x = np.array([rng.uniform(-np.pi, np.pi), rng.uniform(-np.pi, np.pi), rng.uniform(-12, 12), rng.uniform(-28, 28), rng.uniform(0, 19)])
                    x[c] = sign * value
                    add(tag, x, ACROBOT_TORQUES[k % 6])
    for t in (19.9, 19.94, np.nextafter(19.95, 0), 19.95, np.nextafter(19.95, 20), 19.96, 20.0, np.nextafter(20.0, 21), 20.01):   # time: 20
        for k in range(3):
            add("timeout", [np.pi + rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1), rng.uniform(-0.6, 0.6), rng.uniform(-1.1, 1.1), t], ACROBOT_TORQUES[k])
    for i in range(128):                                                  # swinging, angles to +-40
        add("swinging", [rng.uniform(-40, 40), rng.uniform(-40, 40), rng.uniform(-15, 15), rng.uniform(-30, 30), rng.uniform(0, 19.8)], ACROBOT_TORQUES[i % 6])
    a = np.array(rows)
    cases = dict(state=np.ascontiguousarray(a[:, :5]), action=np.ascontiguousarray(a[:, 5]), tag=np.array(tags, np.int32))
    assert len(tags) <= MAX_ROWS
    _check_acrobot_coverage(cases, spec, L)
    return cases


def _check_acrobot_coverage(cases, spec, L):
    """the properties the rows are there for, by the oracle alone"""
    got = oracle_answers("acrobot", cases, ob.MATH_LIBM)
    tag = cases["tag"]
    for c, name in ((0, "angle1_threshold"), (1, "angle2_threshold")):
        rows = tag == TAG[name]
        centre = np.pi if c == 0 else 0.0
        margin = np.abs(got["next"][rows, c] - centre) - FAIL_ANGLE
        assert (np.abs(margin) < 1e-8).all() and (margin > 0).sum() == (margin < 0).sum() == rows.sum() // 2
        assert ((got["term"][rows] == 2) == (margin > 0)).all()
        for centre_side in (1, -1):
            assert ((got["next"][rows, c] - centre) * centre_side > 0).sum() == rows.sum() // 2
    for c, limit, name in ((2, 4 * np.pi, "rate1_limit"), (3, 9 * np.pi, "rate2_limit")):
        rows = tag == TAG[name]
        rate, acc = cases["state"][rows, c], got["xd"][rows, c]
        for sign in (1, -1):
            beyond = sign * rate > limit
            assert beyond.sum() == 8 and (sign * rate == limit).sum() == 8 and ((sign * rate < limit) & (sign * rate > limit - 1e-9)).sum() == 8
            assert (acc[beyond] == 0).any() and (sign * acc[beyond] < 0).any(), "a limiter that fires and one that lets the acceleration through"
            assert (sign * acc[(sign * rate <= limit) & (sign * rate > 0)] > 0).any(), "an acceleration the limiter would have clipped"
    rows = tag == TAG["timeout"]
    assert (got["term"][rows] == 1).any() and (got["term"][rows] == 0).any() and (got["term0"][rows] == 1).any()
    assert np.abs(cases["state"][tag == TAG["swinging"], :2]).max() > 39


# ------------------------------------------------------------------------------------------------- walker cases ---
WALKER_TORQUES = [-1.2, 0.0, 1.2, 0.413, -0.77, 0.0625]
FALL_STANCE, FALL_HIP = np.pi / 8, np.pi / 4


def walker_diag(spec, x, u):
    L = ob.load()
    nxt, d = _arr(11), (C.c_int * 7)()
    L.orc_walker_step_diag(C.byref(spec), (C.c_double * 11)(*x), float(u), nxt, d)
    return np.array(nxt[:]), list(d)


def _walk(spec, rng, episodes, steps):
    """(state, torque, diag, next) of every step of `episodes` walks from the start distribution: mostly passive (torque 0 keeps
    the walker on its gait, so that strides end in heel strikes), one step in four under another torque"""
    L = ob.load()
    out = []
    for ep in range(episodes):
        g, tl, x = C.c_uint64(seeded_position(5000 + ep)), C.c_uint64(0), _arr(11)
        L.orc_env_start_at(C.byref(spec), C.byref(g), C.byref(tl), 0, x)
        x = np.array(x[:])
        for _ in range(steps):
            u = 0.0 if rng.random() < 0.75 else (WALKER_TORQUES[rng.integers(6)] if rng.random() < 0.7 else rng.uniform(-1.2, 1.2))
            nxt, d = walker_diag(spec, x, u)
            out.append((x, u, d, nxt))
            if abs(nxt[SLA]) > FALL_STANCE or abs(nxt[HA] - 2 * nxt[SLA]) > FALL_HIP:
                break
            x = nxt
    return out


def _synthetic(spec, rng, n):
    """states near a foot-on-the-floor configuration (hip angle about twice the stance angle) moving either way"""
    out = []
    for _ in range(n):
        sla = rng.uniform(-0.3, 0.3)
        x = np.zeros(11)
        x[[SLA, HA, SLAR, HAR]] = sla, 2 * sla + rng.uniform(-0.03, 0.03), rng.uniform(-0.4, 0.4), rng.uniform(-0.8, 0.8)
        x[LASTHIPX], x[TIMEOUT] = -np.sin(sla), 100.0
        u = WALKER_TORQUES[rng.integers(6)]
        nxt, d = walker_diag(spec, x, u)
        out.append((x, u, d, nxt))
    return out


def walker_pool():
    """every step the walker's rows are chosen from, as a case set (tools/record_ref_envs.py counts on it how often a binary
    with fused sin/cos differs: the committed 512 rows are too few to meet a step that does)"""
    rng = np.random.default_rng(20110401)
    spec = spec_of("walker", ob.MATH_LIBM)
    pool = _walk(spec, rng, 300, 60) + _synthetic(spec, rng, 4000)
    return dict(state=np.array([r[0] for r in pool]), action=np.array([r[1] for r in pool]), tag=np.zeros(len(pool), np.int32))


def walker_cases():
    rng = np.random.default_rng(20110401)
    spec = spec_of("walker", ob.MATH_LIBM)
    rows, tags = [], []

    def add(tag, x, u):
        rows.append(list(x) + [u]); tags.append(TAG[tag])

    def step(x, u):
        return ob.env_step(spec, [x], [u])[0][0]

    walked = _walk(spec, rng, 300, 60)
    made = _synthetic(spec, rng, 4000)
    pool = walked + made
    # heel strikes: from the walks, half of them with 200 sin(sla) above 30 where the walks offer that many
    strikes = [r for r in walked if r[2][1] > 0]
    rich = [r for r in strikes if 200 * np.sin(r[3][SLA]) > 30]
    poor = [r for r in strikes if not 200 * np.sin(r[3][SLA]) > 30]
    for r in rich[:48] + poor[:96 - min(48, len(rich))]:
        add("strike", r[0], r[1])
    # the swing foot crosses the floor and a clause of detectEvents refuses the strike
    for at, tag in ((2, "refused_hip_sign"), (3, "refused_stance_rate"), (4, "refused_hip_angle")):
        for r in [r for r in pool if r[2][at] > 0 and r[2][1] == 0][:16]:
            add(tag, r[0], r[1])
    for r in [r for r in pool if r[2][6] >= 10][:8]:                      # the secant search spends all 10 iterations (if any)
        add("search_exhausted", r[0], r[1])
    # angle wraps at +-pi: each of the four wraps, the angle on either side of the edge after the sub-step
    for c, rate in ((SLA, SLAR), (HA, HAR)):
        for sign in (1.0, -1.0):
            for k in range(8):
                x = np.zeros(11)
                x[[SLA, HA, SLAR, HAR]] = rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)
                x[c], x[rate] = sign * (np.pi - rng.uniform(0.0, 0.3)), sign * rng.uniform(0.5, 3.0)
                x[TIMEOUT] = 100.0
                add("wrap", x, WALKER_TORQUES[k % 6])
    # fallen: the next step lands just inside / just outside |sla| = pi/8 and |ha - 2 sla| = pi/4
    for tag, c, limit in (("fallen_stance", SLA, FALL_STANCE), ("fallen_hip", HA, FALL_HIP)):
        for sign in (1.0, -1.0):
            for k in range(4):
                base = np.zeros(11)
                base[[SLA, HA, SLAR, HAR]] = rng.uniform(-0.05, 0.05), 0.0, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
                base[HA] = 2 * base[SLA] + (rng.uniform(0.02, 0.1) if c == SLA else 0.0)      # swing foot above the floor side: no strike on the way
                base[TIMEOUT] = 100.0
                u = WALKER_TORQUES[(k + (c == HA)) % 6] * 0.25

                def at(p):
                    x = base.copy()
                    if c == SLA:
                        x[SLA] += sign * p; x[HA] += 2 * sign * p
                    else:
                        x[HA] += sign * p
                    return x

                def margin(p):
                    y = step(at(p), u)
                    return abs(y[SLA]) - limit if c == SLA else abs(y[HA] - 2 * y[SLA]) - limit
                lo, hi = _bisect(margin, 0.0, 0.6 if c == SLA else 1.2)
                add(tag, at(lo), u); add(tag, at(hi), u)
    # time on both sides of the timeout: learning episodes (100) and test episodes (200)
    gait = [r for r in walked if r[2][0] == 0][:: max(1, len(walked) // 40)]
    k = 0
    for timeout in (100.0, 200.0):
        for t in (timeout - 0.5, timeout - 0.2, np.nextafter(timeout - 0.2, timeout), timeout - 0.1, timeout, np.nextafter(timeout, np.inf), timeout + 0.3):
            for _ in range(2):
                x = gait[k % len(gait)][0].copy(); k += 1
                x[TIME], x[TIMEOUT] = t, timeout
                add("timeout", x, WALKER_TORQUES[k % 6])
    # plain walking under every torque, as many rows as are left
    plain = [r for r in walked if r[2][0] == 0]
    for r in plain[:: max(1, len(plain) // (MAX_ROWS - len(tags)) + 1)][: MAX_ROWS - len(tags)]:
        add("walking", r[0], r[1])
    a = np.array(rows)
    cases = dict(state=np.ascontiguousarray(a[:, :11]), action=np.ascontiguousarray(a[:, 11]), tag=np.array(tags, np.int32))
    assert len(tags) <= MAX_ROWS
    _check_walker_coverage(cases, spec)
    return cases


def _check_walker_coverage(cases, spec):
    got = oracle_answers("walker", cases, ob.MATH_LIBM)
    tag, state, action = cases["tag"], cases["state"], cases["action"]
    diag = np.array([walker_diag(spec, x, u)[1] for x, u in zip(state, action)])
    strike = tag == TAG["strike"]
    assert strike.sum() >= 64 and (got["changed"][strike] == 1).all() and (diag[strike, 1] > 0).all()
    raw, up = 200 * np.sin(got["next"][strike, SLA]), got["term"][strike] != 2
    assert ((raw > 30) & up).sum() >= 8 and ((raw < 30) & up).sum() >= 8 and (got["reward"][strike][(raw > 30) & up] == 30).all()
    assert np.allclose(got["reward"][strike][(raw < 30) & up], raw[(raw < 30) & up], rtol=1e-12, atol=0)
    for at, name in ((2, "refused_hip_sign"), (3, "refused_stance_rate"), (4, "refused_hip_angle")):
        rows = tag == TAG[name]
        assert rows.sum() >= 8 and (diag[rows, at] > 0).all() and (got["changed"][rows] == 0).all(), name
    wraps = diag[tag == TAG["wrap"], 5]
    assert all((wraps & bit).astype(bool).sum() >= 4 for bit in (1, 2, 4, 8)), "each of the four wraps"
    for name, limit in (("fallen_stance", FALL_STANCE), ("fallen_hip", FALL_HIP)):
        rows = tag == TAG[name]
        y = got["next"][rows]
        margin = (np.abs(y[:, SLA]) if name == "fallen_stance" else np.abs(y[:, HA] - 2 * y[:, SLA])) - limit
        assert (np.abs(margin) < 1e-8).all() and (margin > 0).sum() == (margin < 0).sum() == 8, name
        assert ((got["term"][rows] == 2) == (margin > 0)).all() and ((got["reward"][rows] == -100) == (margin > 0)).all()
        signed = y[:, SLA] if name == "fallen_stance" else y[:, HA] - 2 * y[:, SLA]
        assert (signed > 0).sum() == (signed < 0).sum() == 8
    rows = tag == TAG["timeout"]
    for timeout in (100.0, 200.0):
        r = rows & (state[:, TIMEOUT] == timeout)
        assert (got["term"][r] == 1).any() and (got["term"][r] == 0).any() and (got["term0"][r] == 1).any()
    assert set(np.round(action[np.isin(action, WALKER_TORQUES[:3])], 1)) == {-1.2, 0.0, 1.2} and (~np.isin(action, WALKER_TORQUES[:3])).sum() > 20


# ---------------------------------------------------------------------------------------------- cart-pole cases ---
CART_FORCES = [-15.0, 0.0, 15.0, 6.31, -11.7, 0.875]                     # the actor-critic's range: its ends, its middle and three off-grid forces
END_STOP = 2.4


def _finish(rows, tags, S, variants=None):
    a = np.array(rows)
    cases = dict(state=np.ascontiguousarray(a[:, :S]), action=np.ascontiguousarray(a[:, S]), tag=np.array(tags, np.int32))
    if variants is not None:
        cases["variant"] = np.array(variants, np.int32)
    assert len(tags) <= MAX_ROWS
    return cases


def cart_pole_cases():
    rng = np.random.default_rng(19830913)
    spec = spec_of("cart_pole", ob.MATH_LIBM)
    timeout = spec.timeout
    rows, tags, variants = [], [], []

    def add(tag, x, u, variant=None):
        rows.append(list(x) + [u]); tags.append(TAG[tag]); variants.append(len(tags) % 4 if variant is None else variant)

    def step(x, u):
        return ob.env_step(spec, [x], [u])[0][0]

    def force(i):
        return CART_FORCES[i % 6] if i % 4 else float(rng.uniform(-15, 15))

    # swing-up episodes from the task's start under forces from the whole range (no penalty: they run on through the end stops)
    for ep in range(8):
        x = np.array([0.0, np.pi + rng.uniform(-0.05, 0.05), 0.0, 0.0, 0.0])
        for k in range(190):
            u = force(int(rng.integers(1000)))
            if k % 9 == ep % 9:
                add("episode", x, u)
            x = step(x, u)
    # the end stops: position excess on either side x velocity into / out of the stop x acceleration of either sign
    for side in (1.0, -1.0):
        for vsign in (1.0, -1.0):
            for asign in (1.0, -1.0):
                found = 0
                while found < 4:
                    x = np.array([side * (END_STOP + rng.uniform(1e-6, 0.4)), rng.uniform(-8, 8), vsign * rng.uniform(0.01, 6), rng.uniform(-8, 8), rng.uniform(0, 9)])
                    u = float(rng.uniform(-15, 15))
                    if _cart_acc(spec, x, u) * asign > 0:
                        add("end_stop", x, u); found += 1
        for value in (END_STOP, np.nextafter(END_STOP, 0), np.nextafter(END_STOP, 3)):      # at, just inside and just beyond the stop, moving into it
            for asign in (1.0, -1.0):
                x = np.array([side * value, rng.uniform(-3, 3), side * rng.uniform(0.5, 3), rng.uniform(-3, 3), rng.uniform(0, 9)])
                add("end_stop_edge", x, side * asign * 15.0)
    # failed(): the next position lands just inside / just outside |x| = 2.4, under every task variant
    for side in (1.0, -1.0):
        for k in range(4):
            base = np.array([0.0, rng.uniform(-3, 3), side * rng.uniform(0.8, 1.5), rng.uniform(-2, 2), rng.uniform(0, 9)])
            u = CART_FORCES[k]

            def at(p):
                x = base.copy(); x[0] = side * p
                return x
            lo, hi = _bisect(lambda p: abs(step(at(p), u)[0]) - END_STOP, 2.0, END_STOP)
            add("failed_threshold", at(lo), u, k); add("failed_threshold", at(hi), u, k)
    # time on both sides of the timeout, stepped there and given
    for k in range(4):
        base = np.array([rng.uniform(-1, 1), rng.uniform(-3, 3), rng.uniform(-1, 1), rng.uniform(-2, 2), 0.0])

        def at(p):
            x = base.copy(); x[4] = p
            return x
        lo, hi = _bisect(lambda p: step(at(p), CART_FORCES[k])[4] - timeout, timeout - 0.09, timeout)
        add("timeout", at(lo), CART_FORCES[k], k); add("timeout", at(hi), CART_FORCES[k], k)
    for t in (timeout - 0.06, np.nextafter(timeout - 0.05, 0), timeout - 0.05, np.nextafter(timeout - 0.05, 10), np.nextafter(timeout, 0), timeout, np.nextafter(timeout, 10), timeout + 0.01):
        add("timeout", [rng.uniform(-1, 1), rng.uniform(-3, 3), rng.uniform(-1, 1), rng.uniform(-2, 2), t], force(len(tags)))
    # observe: state[1] + pi on either side of multiples of 2 pi, the negative ones (the `a < 0` branch) included
    for turn in range(-3, 4):
        edge = 2 * np.pi * turn - np.pi
        for value in (edge, np.nextafter(edge, -np.inf), np.nextafter(edge, np.inf), edge - 1e-9, edge + 1e-9):
            add("observe_wrap", [rng.uniform(-2, 2), value, rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), rng.uniform(0, 9)], force(len(tags)))
    # potential: |theta| mod 2 pi of the next state lands on either side of pi
    for centre in (np.pi, -np.pi, 3 * np.pi, -3 * np.pi, 5 * np.pi, -7 * np.pi):
        base = np.array([rng.uniform(-1, 1), 0.0, rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0, 9)])
        u = force(len(tags))

        def at(p):
            x = base.copy(); x[1] = centre + p
            return x
        lo, hi = _bisect(lambda p: np.fmod(abs(step(at(p), u)[1]), 2 * np.pi) - np.pi, -0.3, 0.3)
        add("potential_wrap", at(lo), u); add("potential_wrap", at(hi), u)
    for i in range(24):                                                   # the action penalty at forces up to the range's ends, with and without it
        add("action_penalty", [rng.uniform(-2, 2), rng.uniform(-7, 7), rng.uniform(-3, 3), rng.uniform(-5, 5), rng.uniform(0, 9)], force(i), 2 * (i % 2) + (i // 2) % 2)
    for i in range(64):                                                   # far from any episode: many turns, rates beyond the observation's range
        add("far", [rng.uniform(-3.5, 3.5), rng.uniform(-40, 40), rng.uniform(-12, 12), rng.uniform(-20, 20), rng.uniform(0, 9.9)], force(i))
    cases = _finish(rows, tags, 5, variants)
    _check_cart_pole_coverage(cases)
    return cases


def _cart_acc(spec, x, u):
    """the cart's acceleration before the end stops override it: it does not depend on the cart's position or velocity"""
    free = np.array(x, np.float64); free[0] = 0.0; free[2] = 0.0
    d = _arr(5)
    ob.load().orc_env_eom(C.byref(spec), (C.c_double * 5)(*free), float(u), d)
    return d[2]


def _check_cart_pole_coverage(cases):
    got = oracle_answers("cart_pole", cases, ob.MATH_LIBM)
    spec = spec_of("cart_pole", ob.MATH_LIBM)
    tag, state, action, variant = cases["tag"], cases["state"], cases["action"], cases["variant"]
    esp, ap = (variant & 1).astype(bool), (variant & 2).astype(bool)
    assert set(variant) == {0, 1, 2, 3}
    rows = tag == TAG["episode"]
    assert rows.sum() >= 120 and (np.abs(state[rows, 0]) > END_STOP).any() and np.isin(action[rows], CART_FORCES[:3]).any() and (~np.isin(action[rows], CART_FORCES)).any()
    # the four overrides of eom: xd[0] = 0 on either side, xd[2] = 0 with it where the acceleration pushes further in, and neither where the cart moves out
    rows = np.nonzero(tag == TAG["end_stop"])[0]
    seen = set()
    for i in rows:
        side, v, acc = np.sign(state[i, 0]), np.sign(state[i, 2]), np.sign(_cart_acc(spec, state[i], action[i]))
        seen.add((side, v, acc))
        into = side == v
        assert (got["xd"][i, 0] == 0) == into and (got["xd"][i, 2] == 0) == (into and acc == side)
        assert into or got["xd"][i, 0] == state[i, 2]
    assert len(seen) == 8
    rows = tag == TAG["end_stop_edge"]
    beyond = np.abs(state[rows, 0]) > END_STOP
    assert beyond.sum() == 4 and (np.abs(state[rows, 0]) == END_STOP).sum() == 4 and ((got["xd"][rows, 0] == 0) == beyond).all()
    rows = tag == TAG["failed_threshold"]
    margin = np.abs(got["next"][rows, 0]) - END_STOP
    assert (np.abs(margin) < 1e-8).all() and (margin > 0).sum() == (margin < 0).sum() == 8
    assert (got["next"][rows, 0] > 0).sum() == (got["next"][rows, 0] < 0).sum() == 8
    assert ((got["term"][rows] == 2) == ((margin > 0) & esp[rows])).all() and (got["term"][rows] == 2).sum() == 4
    assert ((got["reward"][rows] < -9000) == ((margin > 0) & esp[rows])).all()
    rows = tag == TAG["timeout"]
    assert (got["term"][rows] == 1).sum() >= 6 and (got["term"][rows] == 0).sum() >= 6 and (got["term0"][rows] == 1).any() and (got["term0"][rows] == 0).any()
    assert (np.abs(got["next"][rows, 4] - spec.timeout) < 1e-8).sum() >= 8
    rows = tag == TAG["observe_wrap"]
    z = state[rows, 1] + np.pi
    assert (z < 0).sum() >= 10 and (z > 0).sum() >= 10 and (got["obs0"][rows, 1] < 1e-6).any() and (got["obs0"][rows, 1] > 2 * np.pi - 1e-6).any()
    assert ((got["obs0"][rows, 1] >= 0) & (got["obs0"][rows, 1] <= 2 * np.pi)).all()
    rows = tag == TAG["potential_wrap"]
    m = np.fmod(np.abs(got["next"][rows, 1]), 2 * np.pi) - np.pi
    assert (np.abs(m) < 1e-8).all() and (m > 0).sum() == (m < 0).sum() == 6 and (got["next"][rows, 1] < 0).any() and (got["next"][rows, 1] > 0).any()
    rows = tag == TAG["action_penalty"]
    assert set(variant[rows]) == {0, 1, 2, 3} and (np.abs(action[rows]) == 15).any()
    assert np.abs(state[tag == TAG["far"], 1]).max() > 39


# ----------------------------------------------------------------------------------------------- pendulum cases ---
PENDULUM_TORQUES = [-3.0, 0.0, 3.0, 1.37, -2.231, 0.0521]                 # the grid of the yaml and three off-grid torques
RATE_RANGE = 12 * np.pi


def pendulum_cases():
    rng = np.random.default_rng(20150122)
    spec = spec_of("pendulum", ob.MATH_LIBM)
    timeout = spec.timeout
    rows, tags = [], []

    def add(tag, x, u):
        rows.append(list(x) + [u]); tags.append(TAG[tag])

    def step(x, u):
        return ob.env_step(spec, [x], [u])[0][0]

    def torque(i):
        return PENDULUM_TORQUES[i % 6] if i % 4 else float(rng.uniform(-3, 3))

    for ep in range(8):                                                   # episodes from learning starts (any angle) and the test start
        x = np.array([np.pi + (ep % 4 != 0) * rng.uniform(0, 2 * np.pi), 0.0, 0.0])
        for k in range(99):
            u = torque(int(rng.integers(1000)))
            if k % 5 == ep % 5:
                add("episode", x, u)
            x = step(x, u)
    for sign in (1.0, -1.0):                                              # rates to and beyond +-12 pi
        for value in (RATE_RANGE, np.nextafter(RATE_RANGE, 0), np.nextafter(RATE_RANGE, 100), 30.0, 45.0, 60.0, 90.0):
            for k in range(3):
                add("rate_range", [rng.uniform(-7, 7), sign * value, rng.uniform(0, 2.9)], torque(len(tags)))
    for i in range(64):                                                   # angles many turns either way
        add("turns", [rng.uniform(-300, 300), rng.uniform(-40, 40), rng.uniform(0, 2.9)], torque(i))
    for u in (-4.5, 4.5, np.nextafter(3.0, 4), np.nextafter(-3.0, -4), 100.0, -100.0):        # actuate clamps what moves the pendulum, the reward sees the action
        for k in range(2):
            add("clamped", [rng.uniform(-7, 7), rng.uniform(-10, 10), rng.uniform(0, 2.9)], u)
    for turn in range(-3, 4):                                             # observe: state[0] + pi on either side of multiples of 2 pi, given ...
        edge = 2 * np.pi * turn - np.pi
        for value in (edge, np.nextafter(edge, -np.inf), np.nextafter(edge, np.inf), edge - 1e-9, edge + 1e-9):
            add("observe_wrap", [value, rng.uniform(-5, 5), rng.uniform(0, 2.9)], torque(len(tags)))
    for turn in (-2, -1, 0, 1, 2, 3):                                     # ... and stepped to
        edge = 2 * np.pi * turn - np.pi
        base = np.array([0.0, rng.uniform(-5, 5), rng.uniform(0, 2.9)])
        u = torque(len(tags))

        def at(p):
            x = base.copy(); x[0] = edge + p
            return x
        lo, hi = _bisect(lambda p: step(at(p), u)[0] - edge, -0.6, 0.6)
        add("observe_wrap_step", at(lo), u); add("observe_wrap_step", at(hi), u)
    for centre in (np.pi, -np.pi, 3 * np.pi, -5 * np.pi):                # evaluate: |angle| mod 2 pi of the next state on either side of pi
        base = np.array([0.0, rng.uniform(-5, 5), rng.uniform(0, 2.9)])
        u = torque(len(tags))

        def at(p):
            x = base.copy(); x[0] = centre + p + 1e-4                     # off observe's wrap, which sits at the same angles
            return x
        lo, hi = _bisect(lambda p: np.fmod(abs(step(at(p), u)[0]), 2 * np.pi) - np.pi, -0.6, 0.6)
        add("potential_wrap", at(lo), u); add("potential_wrap", at(hi), u)
    for k in range(4):                                                    # time on both sides of the timeout, stepped there and given
        base = np.array([rng.uniform(-7, 7), rng.uniform(-10, 10), 0.0])

        def at(p):
            x = base.copy(); x[2] = p
            return x
        lo, hi = _bisect(lambda p: step(at(p), PENDULUM_TORQUES[k])[2] - timeout, timeout - 0.05, timeout)
        add("timeout", at(lo), PENDULUM_TORQUES[k]); add("timeout", at(hi), PENDULUM_TORQUES[k])
    for t in (timeout - 0.04, np.nextafter(timeout - 0.03, 0), timeout - 0.03, np.nextafter(timeout - 0.03, 10), np.nextafter(timeout, 0), timeout, np.nextafter(timeout, 10), timeout + 0.01):
        add("timeout", [rng.uniform(-7, 7), rng.uniform(-10, 10), t], torque(len(tags)))
    cases = _finish(rows, tags, 3)
    _check_pendulum_coverage(cases)
    return cases


def _check_pendulum_coverage(cases):
    got = oracle_answers("pendulum", cases, ob.MATH_LIBM)
    spec = spec_of("pendulum", ob.MATH_LIBM)
    tag, state, action = cases["tag"], cases["state"], cases["action"]
    rows = tag == TAG["episode"]
    assert rows.sum() >= 120 and set(action[rows][np.isin(action[rows], PENDULUM_TORQUES[:3])]) == {-3.0, 0.0, 3.0} and (~np.isin(action[rows], PENDULUM_TORQUES)).sum() > 20
    rows = tag == TAG["rate_range"]
    assert (np.abs(state[rows, 1]) == RATE_RANGE).sum() == 6 and (np.abs(state[rows, 1]) > 2 * RATE_RANGE).any() and (state[rows, 1] < 0).any()
    assert np.abs(state[tag == TAG["turns"], 0]).max() > 250 and (state[tag == TAG["turns"], 0] < -100).any()
    rows = tag == TAG["clamped"]
    assert (np.abs(action[rows]) > 3).all() and (got["reward"][rows] < -9).all() and (got["reward"][rows] < -9000).any()
    rows = tag == TAG["observe_wrap"]
    z = state[rows, 0] + np.pi
    assert (z < 0).sum() >= 10 and (z > 0).sum() >= 10 and (got["obs0"][rows, 0] < 1e-6).any() and (got["obs0"][rows, 0] > 2 * np.pi - 1e-6).any()
    rows = tag == TAG["observe_wrap_step"]
    assert ((got["obs"][rows, 0] < 1e-8) | (got["obs"][rows, 0] > 2 * np.pi - 1e-8)).all()
    assert (got["obs"][rows, 0] < 1e-8).sum() == (got["obs"][rows, 0] > 1).sum() == 6 and (got["next"][rows, 0] < -np.pi).any()
    rows = tag == TAG["potential_wrap"]
    m = np.fmod(np.abs(got["next"][rows, 0]), 2 * np.pi) - np.pi
    assert (np.abs(m) < 1e-8).all() and (m > 0).sum() == (m < 0).sum() == 4
    rows = tag == TAG["timeout"]
    assert (got["term"][rows] == 1).sum() >= 6 and (got["term"][rows] == 0).sum() >= 6 and (got["term0"][rows] == 1).any() and (got["term0"][rows] == 0).any()
    assert (np.abs(got["next"][rows, 2] - spec.timeout) < 1e-8).sum() >= 8
    assert ((got["obs"][:, 0] >= 0) & (got["obs"][:, 0] <= 2 * np.pi)).all() and ((got["term"] == 0) | (got["term"] == 1)).all()


CASES = {"acrobot": acrobot_cases, "walker": walker_cases, "cart_pole": cart_pole_cases, "pendulum": pendulum_cases}
