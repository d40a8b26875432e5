"""Reference of the sampled ensemble episodes (grlx_evaluate_ensemble_sampled): the serial loop of include/grlx.h over policy_query_ref.query_q
on the members' DENSE parameter vectors, policy_evaluate_ref's environment helpers, the oracle's portable exponential (orc_pexp) and its
Rand48 (orc_drand48).

  d_m      GREEDY: 1 / man on the maximal entries;  EPSILON e: that, 1 replaced by 1 - e, plus e / NA;  SOFTMAX t: softmax(q_m, t)
  vote_m   best = 0.0, idx = NA - 1; for j ascending: d_m[j] > best takes j
  score    MAJORITY: score[vote_m] += 1;  RANK: score[i] += 1 + #{k : d_m[i] > d_m[k]}
  action   grl::sample(softmax(score, tau)) on one drand48 of the episode's stream
"""
import ctypes as C

import numpy as np

from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev
from tests import policy_query_ref as ref

MAJORITY, RANK = 0, 1                   # include/grlx.h: GRLX_ENSEMBLE_MAJORITY, GRLX_ENSEMBLE_RANK
GREEDY, EPSILON, SOFTMAX = 0, 1, 2      # GRLX_MEMBER_*
DBL_MAX = float(np.finfo(np.float64).max)
FIELDS = ("ret", "disc", "steps", "terminal", "ties", "member_ties", "agreement", "explored", "final_state", "streams")


def pexp(x):
    return float(ob.load().orc_pexp(float(x)))


def softmax(v, t):
    """SoftmaxSampler::distribution (softmax.cpp:65-110)"""
    p = [float(x) / t for x in v]
    maxp = -DBL_MAX
    for x in p:
        maxp = x if maxp < x else maxp
    minp = maxp + (-100)
    center = (maxp + minp) / 2.0
    e, total = [None] * len(p), 0.0
    for i, x in enumerate(p):
        if x > minp:
            e[i] = pexp(x - center)
            total += e[i]
    return [0.0 if x is None else x / total for x in e]


def member_distribution(q, member, param):
    """(d_m, man_m)"""
    mai, man = ref.findmax(q)
    if member == SOFTMAX:
        return softmax(q, param), man
    d = [1. / man if x == q[mai] else 0. for x in q]
    if member == EPSILON:
        for i in range(len(d)):
            if d[i] == 1:
                d[i] = 1 - param
            d[i] += param / len(d)
    return d, man


def vote_of(d):
    best, idx = 0.0, len(d) - 1
    for j, x in enumerate(d):
        if x > best:
            best, idx = x, j
    return idx


def ranks_of(d):
    return [1 + sum(1 for y in d if x > y) for x in d]


def combine(members, spec, obs, strategy, member, params, seen=None):
    """(score, votes, members with a tie) at one observation; params: per member (e or tau_m).  seen["ranks"] collects every member's ranks."""
    A = int(spec.action_steps)
    score, votes, mties = [0] * A, [0] * A, 0
    for w, param in zip(members, params):
        q = [float(v) for v in ref.query_q(w, spec, [obs])[0][0]]
        d, man = member_distribution(q, member, param)
        votes[vote_of(d)] += 1
        mties += 1 if man > 1 else 0
        if strategy == RANK:
            rk = ranks_of(d)
            if seen is not None:
                seen.setdefault("ranks", []).append(tuple(rk))
            for a in range(A):
                score[a] += rk[a]
    return (score if strategy == RANK else list(votes)), votes, mties


def draw(dist, g):
    """grl::sample (utils.h:227-250)"""
    s = 0.0
    for x in dist:
        s += x
    r = float(ob.load().orc_drand48(C.byref(g))) * s
    acc = 0.0
    for i, x in enumerate(dist):
        acc += x
        if r < acc:
            return i
    return len(dist) - 1


def episode(members, spec, state, strategy, tau, member, params, stream, max_steps=0, gamma=None, seen=None):
    """dict of one episode's outputs; records: [steps][R] with R = 8 + D + S + 2"""
    max_steps = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    gamma = float(spec.gamma) if gamma is None else float(gamma)
    acts = ref.actions_of(spec)
    g = ob.Rand48(int(stream))
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec, x)
    ret, disc, gg, steps, ties, mties, agree, explored, code = 0.0, 0.0, 1.0, 0, 0, 0, 0, 0, 0
    records = []
    while True:
        score, votes, mt = combine(members, spec, obs, strategy, member, params, seen)
        dist = softmax(score, tau)
        idx = draw(dist, g)
        mai, man = ref.findmax(score)
        action = acts[idx]
        nx, nobs, reward, term = ob.env_step(spec, x, action)
        before, x, obs, reward = obs, nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += gg * reward
        gg = gg * gamma
        steps += 1
        ties += 1 if man > 1 else 0
        mties += mt
        agree += votes[idx]
        explored += 1 if idx != mai else 0
        code = ev.DOMAIN if not ev.in_domain(spec, x) else int(term[0])
        records.append([action, reward, float(score[idx]), float(idx), float(man), float(code), float(votes[idx]), float(mt)] + list(before) + list(x) +
                       [1.0 if idx != mai else 0.0, dist[idx]])
        if code != 0 or steps >= max_steps:
            break
    return dict(ret=ret, disc=disc, steps=steps, terminal=code, ties=ties, member_ties=mties, agreement=agree, explored=explored, final_state=x,
                streams=np.uint64(g.x), records=np.array(records, np.float64))


def evaluate(members, spec, states, strategy, tau, member, params, streams, max_steps, gamma=None, seen=None):
    """one group: dict of the ten outputs [n] and records [n][max_steps][R] (zeros behind an episode's end); streams [n]"""
    eps = [episode(members, spec, states[s], strategy, tau, member, params, streams[s], max_steps, gamma, seen) for s in range(len(states))]
    out = {f: np.array([ep[f] for ep in eps]) for f in FIELDS}
    R = eps[0]["records"].shape[1]
    out["records"] = np.zeros((len(states), max_steps, R), np.float64)
    for s, ep in enumerate(eps):
        out["records"][s, :ep["steps"]] = ep["records"]
    return out
