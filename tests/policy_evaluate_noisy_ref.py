"""Reference of the noisy evaluation episodes (grlx_evaluate_noisy): policy_evaluate_ref's loop of the actor-critic with the exploring
policy in place of the noise-free actor, over the oracle's dense tables, its env_step, its Rand48 (orc_drand48 on a state of the loop's own)
and its portable log and cos.  The step, written out once more (ActionPolicy::act(time, in, out), action.cpp:127-158; Rand::getNormal,
utils.h:120-125; oracle/experiment.c: ac_policy_act):

  u = read(actor table, obs), clamped to the actor representation's output range
  if the model time of the state acted on is 0: noise = 0
  if sg != 0: U1 = drand48; U2 = drand48; nrm = sqrt(-2 * plog(U1)) * pcos(2 * pi * U2) * sg + 0
              noise = (1 - theta) * noise + nrm; out = u + noise
  else:       out = u
  action = fmin(fmax(out, action_min), action_max); clipped += out lay outside
"""
import ctypes as C
import math

import numpy as np

from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev
from tests import policy_query_ref as ref

TWO20 = 1 << 20


def jumped(x, n):
    """the rand48 state x after n further draws"""
    g = ob.Rand48(int(x))
    ob.load().orc_rand48_jump(C.byref(g), int(n))
    return int(g.x)


def seeded(seed):
    g = ob.Rand48(0)
    ob.load().orc_srand48(C.byref(g), int(seed))
    return int(g.x)


def episode_stream_words(seed, n_replicas, n_starts, first_pair=0):
    """grlx_episode_stream_words restated on the oracle's generator: the stream of pair p is srand48(seed) after 2 * p * 2^20 draws"""
    out = np.zeros((n_replicas, n_starts), np.uint64)
    x0 = seeded(seed)
    for r in range(n_replicas):
        for s in range(n_starts):
            out[r, s] = jumped(x0, 2 * (first_pair + r * n_starts + s) * TWO20)
    return out


def act(spec, u, time, sg, theta, TL, noise):
    """(action, noise state after, clipped?) -- TL (oracle Rand48) advances by two draws where sg != 0"""
    L = ob.load()
    if time == 0:
        noise = 0.0
    out = u
    if sg != 0:
        U1 = float(L.orc_drand48(C.byref(TL)))
        U2 = float(L.orc_drand48(C.byref(TL)))
        nrm = math.sqrt(-2 * float(L.orc_plog(U1))) * float(L.orc_pcos(2 * math.pi * U2)) * sg + 0.
        noise = (1 - theta) * noise + nrm
        out = u + noise
    clip = out < spec.action_min or out > spec.action_max
    return min(max(out, spec.action_min), spec.action_max), noise, clip


def episode(tables, spec, state, sg, theta, stream, noise, max_steps=0, gamma=None):
    """dict of one episode's outputs; records: [steps][R] with R = 6 + D + S + 2"""
    max_steps = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    gamma = float(spec.gamma) if gamma is None else float(gamma)
    ar = spec.actor_representation
    TL, noise = ob.Rand48(int(stream)), float(noise)
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec, x)
    ret, disc, g, steps, clipped, code = 0.0, 0.0, 1.0, 0, 0, 0
    records = []
    while True:
        u = float(ref.query_state(tables[1], spec, 1, [obs])[0])
        u = min(max(u, ar.output_min), ar.output_max)
        action, noise, clip = act(spec, u, float(x[-1]), sg, theta, TL, noise)
        nx, nobs, reward, term = ob.env_step(spec, x, action)
        before, x, obs, reward = obs, nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * gamma
        steps += 1
        clipped += 1 if clip else 0
        code = ev.DOMAIN if not ev.in_domain(spec, x) else int(term[0])
        records.append([action, reward, u, -1.0, 1.0, float(code)] + list(before) + list(x) + [noise, 1.0 if clip else 0.0])
        if code != 0 or steps >= max_steps:
            break
    return dict(ret=ret, disc=disc, steps=steps, terminal=code, clipped=clipped, final_state=x, streams=np.uint64(TL.x), noise=noise,
                records=np.array(records, np.float64))


FIELDS = ("ret", "disc", "steps", "terminal", "clipped", "final_state", "streams", "noise")


def evaluate(tables, spec, states, sg, theta, streams, noise, max_steps, gamma=None):
    """one replica: dict of the eight outputs [n] and records [n][max_steps][R] (zeros behind an episode's end); streams, noise [n]"""
    eps = [episode(tables, spec, states[s], sg, theta, streams[s], noise[s], max_steps, gamma) for s in range(len(states))]
    out = {f: np.array([ep[f] for ep in eps]) for f in FIELDS}
    R = eps[0]["records"].shape[1]
    out["records"] = np.zeros((len(states), max_steps, R), np.float64)
    for s, ep in enumerate(eps):
        out["records"][s, :ep["steps"]] = ep["records"]
    return out
