"""Reference of the greedy evaluation episodes (grlx_evaluate): a plain Python loop over policy_query_ref.query_q / query_state on the
oracle's DENSE parameter vectors, the oracle's environment step (oracle_binding.env_step) and its first observation (orc_env_observe).

  obs = observe(state)                       the start state's terminal code is ignored: an episode has at least one step
  repeat: action = actions[first maximum of Q(obs, .)]          (Q agents; ties += 1 where the maximum is not unique)
                   clip(read(actor table, obs), action_min, action_max)      (actor-critic)
          state, obs, reward, terminal = step(state, action)
          ret += reward; disc += g * reward; g = g * gamma; steps += 1
  until terminal != 0, the step ended outside the portable math's domain (code 3), or steps == max_steps (code 0)
"""
import ctypes as C

import numpy as np

from tests import oracle_binding as ob
from tests import policy_query_ref as ref

MAX_EPISODE_STEPS = 100000          # include/grlx.h: GRLX_MAX_EPISODE_STEPS
DOMAIN = 3                          # the terminal code of an episode that left the math domain

_observe = None


def observe(spec, state):
    """(obs, terminal code) of a model state: orc_env_observe (oracle/oracle_internal.h), a global symbol of liboracle.so"""
    global _observe
    L = ob.load()
    if _observe is None:
        _observe = L.orc_env_observe
        _observe.argtypes = [C.POINTER(ob.Spec), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        _observe.restype = C.c_int
    S, D = L.orc_env_state_dims(spec.env), L.orc_env_obs_dims(spec.env)
    st = (C.c_double * S)(*[float(v) for v in state])
    obs = (C.c_double * ob.MAX_DIMS)()
    code = _observe(C.byref(spec), st, obs)
    return np.array(obs[:D]), int(code)


def in_domain(spec, x):
    """Env::in_domain (grl_amd/csrc/grlx_envs.h): the condition the rollout kernels flag as ST_DOMAIN at a step end"""
    if spec.env == ob.ENV_PENDULUM:
        return abs(x[0]) < 2.0 ** 19
    if spec.env == ob.ENV_ACROBOT:
        return abs(x[0]) < 2.0 ** 18 and abs(x[1]) < 2.0 ** 18
    if spec.env in (ob.ENV_CART_POLE, ob.ENV_CART_POLE_BALANCING):
        return abs(x[1]) < 2.0 ** 19
    if spec.env == ob.ENV_COMPASS_WALKER:
        return abs(x[0]) < 8.0 and abs(x[1]) < 8.0 and abs(x[2]) < 1e6
    raise ValueError("unknown environment")


def greedy_action(tables, spec, obs):
    """(action, tie?) of the test agent at obs; tables[t] = the dense vector of table t (anything indexable by slot)"""
    if spec.agent == ob.AGENT_AC:
        a = float(ref.query_state(tables[1], spec, 1, [obs])[0])
        return min(max(a, spec.action_min), spec.action_max), False
    _, _, greedy, n_max = ref.query_q(tables[0], spec, [obs])
    return ref.actions_of(spec)[int(greedy[0])], int(n_max[0]) > 1


def episode(tables, spec, state, max_steps=0, gamma=None, actions_out=None):
    """(ret, disc, steps, terminal, ties, final_state) of one episode from `state`"""
    max_steps = max_steps if max_steps else MAX_EPISODE_STEPS
    gamma = float(spec.gamma) if gamma is None else float(gamma)
    x = np.array(state, np.float64)
    obs, _ = observe(spec, x)
    ret, disc, g, steps, ties, code = 0.0, 0.0, 1.0, 0, 0, 0
    while True:
        action, tie = greedy_action(tables, spec, obs)
        if actions_out is not None:
            actions_out.append(action)
        nx, nobs, reward, term = ob.env_step(spec, x, action)
        x, obs, reward = nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * gamma
        steps += 1
        ties += 1 if tie else 0
        code = DOMAIN if not in_domain(spec, x) else int(term[0])
        if code != 0 or steps >= max_steps:
            break
    return ret, disc, steps, code, ties, x


def evaluate(tables, spec, states, max_steps=0, gamma=None):
    """one replica: dict of ret / disc / steps / terminal / ties [n] and final_state [n][S]"""
    states = np.asarray(states, np.float64)
    n = states.shape[0]
    out = dict(ret=np.zeros(n), disc=np.zeros(n), steps=np.zeros(n, np.int32), terminal=np.zeros(n, np.int32), ties=np.zeros(n, np.int32),
               final_state=np.zeros_like(states))
    for s in range(n):
        r, d, k, c, t, x = episode(tables, spec, states[s], max_steps, gamma)
        out["ret"][s], out["disc"][s], out["steps"][s], out["terminal"][s], out["ties"][s] = r, d, k, c, t
        out["final_state"][s] = x
    return out


def tables_of(e):
    """the dense vectors of an oracle experiment as they stand (views, not copies)"""
    n = 2 if e.spec.agent in (ob.AGENT_AC, ob.AGENT_QV) else 1
    return [ref.dense(e, t) for t in range(n)]


FIELDS = ("ret", "disc", "steps", "terminal", "ties", "final_state")
