"""Reference of the sampled evaluation episodes (grlx_evaluate_sampled): policy_evaluate_ref's loop with the reference's samplers in place
of the first maximum, over the oracle's dense tables, its tile_project and env_step, and the oracle's own Rand48 (orc_drand48 / orc_lrand48).

  (mai, man) = findmax(Q(obs, .))
  epsilon-greedy: rnd = drand48(S); rnd < e: lrand48(G) % NA acts, explored            (greedy.cpp:144-218)
  otherwise, and the greedy sampler: man > 1: jj = lrand48(G) % man, the (jj + 1)-th maximal entry acts, a tie; else mai   (greedy.cpp:63-86)
"""
import ctypes as C

import numpy as np

from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev
from tests import policy_query_ref as ref

GREEDY, EPSILON = 0, 1
TWO20 = 1 << 20


def drand48(g):
    return float(ob.load().orc_drand48(C.byref(g)))


def lrand48(g):
    return int(ob.load().orc_lrand48(C.byref(g)))


def jumped(x, n):
    """the rand48 state x after n further draws"""
    g = ob.Rand48(int(x))
    ob.load().orc_rand48_jump(C.byref(g), int(n))
    return int(g.x)


def seeded(seed):
    g = ob.Rand48(0)
    ob.load().orc_srand48(C.byref(g), int(seed))
    return int(g.x)


def episode_streams(seed, n_replicas, n_starts, first_pair=0):
    """grlx_episode_streams restated on the oracle's generator: stream k = 2 * pair + which is srand48(seed) after k * 2^20 draws"""
    out = np.zeros((n_replicas, n_starts, 2), np.uint64)
    x0 = seeded(seed)
    for r in range(n_replicas):
        for s in range(n_starts):
            for w in range(2):
                out[r, s, w] = jumped(x0, (2 * (first_pair + r * n_starts + s) + w) * TWO20)
    return out


def sample(q, sampler, e, S, G):
    """(index that acts, man, tie drawn?, explored?) -- S and G (oracle Rand48) advance as the reference's samplers advance them"""
    mai, man = ref.findmax(q)
    if sampler == EPSILON:
        if drand48(S) < e:
            return lrand48(G) % len(q), man, False, True
    if man > 1:
        jj = lrand48(G) % man
        for ii in range(len(q)):
            if q[ii] == q[mai]:
                if jj == 0:
                    return ii, man, True, False
                jj -= 1
    return mai, man, False, False


def episode(w, spec, state, sampler, e, streams, max_steps=0, gamma=None):
    """dict of one episode's outputs; records: [steps][R] with R = 6 + D + S + 1"""
    max_steps = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    gamma = float(spec.gamma) if gamma is None else float(gamma)
    acts = ref.actions_of(spec)
    S, G = ob.Rand48(int(streams[0])), ob.Rand48(int(streams[1]))
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec, x)
    ret, disc, g, steps, ties, explored, code = 0.0, 0.0, 1.0, 0, 0, 0, 0
    records = []
    while True:
        q = [float(v) for v in ref.query_q(w, spec, [obs])[0][0]]
        idx, man, tie, expl = sample(q, sampler, e, S, G)
        action = acts[idx]
        nx, nobs, reward, term = ob.env_step(spec, x, action)
        before, x, obs, reward = obs, nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * gamma
        steps += 1
        ties += 1 if tie else 0
        explored += 1 if expl else 0
        code = ev.DOMAIN if not ev.in_domain(spec, x) else int(term[0])
        records.append([action, reward, q[idx], float(idx), float(man), float(code)] + list(before) + list(x) + [1.0 if expl else 0.0])
        if code != 0 or steps >= max_steps:
            break
    return dict(ret=ret, disc=disc, steps=steps, terminal=code, ties=ties, explored=explored, final_state=x,
                streams=np.array([S.x, G.x], np.uint64), records=np.array(records, np.float64))


FIELDS = ("ret", "disc", "steps", "terminal", "ties", "explored", "final_state", "streams")


def evaluate(w, spec, states, sampler, e, streams, max_steps, gamma=None):
    """one replica: dict of the eight outputs [n] and records [n][max_steps][R] (zeros behind an episode's end); streams [n][2]"""
    eps = [episode(w, spec, states[s], sampler, e, streams[s], max_steps, gamma) for s in range(len(states))]
    out = {f: np.array([ep[f] for ep in eps]) for f in FIELDS}
    R = eps[0]["records"].shape[1]
    out["records"] = np.zeros((len(states), max_steps, R), np.float64)
    for s, ep in enumerate(eps):
        out["records"][s, :ep["steps"]] = ep["records"]
    return out
