"""Reference of the actor ensemble's episodes (grlx_evaluate_actor_ensemble): a plain Python loop over policy_query_ref.query_state on the
members' DENSE actor tables, policy_evaluate_ref.greedy_action's clip, the oracle's environment step and its portable exponential
(orc_pexp).  The step, the serial loops of include/grlx.h written out once more (mapping/policy/multi, base/src/policies/multi.cpp):

  a_m = clip(read(actor table of member m, obs), lo, hi) for the members m in ASCENDING order; no noise, no draw anywhere
  MEAN         m = a_0; m = m + a_i (i = 1 ... G-1); action = m / (double)G
  BINNING      bin(a) = min((int)floor(((double)B * (a - lo)) / (hi - lo)), B - 1); hist = the members' bins counted; binmax = the first
               bin of strictly greatest count (ascending scan, cnt < hist[b] from cnt = 0); s = 0.0, n = 0; for i ascending, if
               hist[bin(a_i)] == hist[binmax]: s += a_i, ++n -- members of ANOTHER bin with the same count included --; action = s / n;
               tie: more than one bin holds that count
  DATA_CENTER  all alive; mean = the serial sum of the alive members, starting from the first one and not from 0.0, over their count;
               while more than K are alive: d_i = (a_i - mean) * (a_i - mean), the first alive member with the greatest d is removed, mean is
               recomputed; action = mean; tie: some removal of the step had more than one member at the greatest d (once per step)
  DENSITY      n_i = -1 + 2 * ((a_i - lo) / (hi - lo)); rho_i = sum over j ascending from 0.0 of pexp((-1 * ((n_i - n_j) * (n_i - n_j))) /
               (r * r)); the first i of strictly greatest rho, scanning from -inf; action = a_i; tie: more than one member has that rho
  kept += G / n / min(G, K) / 1; spread += max_m a_m - min_m a_m; then the bookkeeping of policy_evaluate_ref.episode
"""
import math

import numpy as np

from tests import oracle_binding as ob
from tests import policy_evaluate_ref as ev

MEAN, BINNING, DATA_CENTER, DENSITY = 0, 1, 2, 3          # include/grlx.h: GRLX_ACTOR_ENSEMBLE_*
RULES = {"mean": MEAN, "binning": BINNING, "data_center": DATA_CENTER, "density": DENSITY}
FIELDS = ("ret", "disc", "steps", "terminal", "ties", "kept", "spread", "final_state")


def pexp(x):
    return float(ob.load().orc_pexp(float(x)))


def mean(a):
    m = a[0]
    for v in a[1:]:
        m = m + v
    return m / float(len(a))


def bin_of(a, B, lo, hi):
    return min(int(math.floor((float(B) * (a - lo)) / (hi - lo))), B - 1)


def binning(a, B, lo, hi):
    """(action, binmax, the bins of greatest count, members summed, the occupied bins)"""
    hist = [0] * B
    for v in a:
        hist[bin_of(v, B, lo, hi)] += 1
    cnt, binmax = 0, 0
    for b in range(B):
        if cnt < hist[b]:
            cnt, binmax = hist[b], b
    s, n = 0.0, 0
    for v in a:
        if hist[bin_of(v, B, lo, hi)] == hist[binmax]:
            s += v
            n += 1
    return s / n, binmax, sum(1 for h in hist if h == hist[binmax]), n, sum(1 for h in hist if h)


def alive_mean(a, alive):
    s, n = None, 0
    for i in alive:
        s = a[i] if s is None else s + a[i]
        n += 1
    return s / n


def data_center(a, K):
    """(action, the greatest number of members tied at one removal (1: none), the members kept, the removed members in order)"""
    alive = list(range(len(a)))
    m = alive_mean(a, alive)
    most, removed = 1, []
    while len(alive) > K:
        far, at, n = None, -1, 0
        for i in alive:
            d = (a[i] - m) * (a[i] - m)
            if far is None or d > far:
                far, at, n = d, i, 1
            elif d == far:
                n += 1
        most = max(most, n)
        removed.append((at, alive[0]))                  # (the member removed, the first alive member at that removal)
        alive.remove(at)
        m = alive_mean(a, alive)
    return m, most, len(alive), removed


def density(a, r, lo, hi):
    """(action, the member selected, the members of greatest rho, every rho)"""
    nrm = [-1 + 2 * ((v - lo) / (hi - lo)) for v in a]
    rho = []
    for i in range(len(a)):
        s = 0.0
        for j in range(len(a)):
            s += pexp((-1 * ((nrm[i] - nrm[j]) * (nrm[i] - nrm[j]))) / (r * r))
        rho.append(s)
    best, at, n = -math.inf, 0, 0
    for i, v in enumerate(rho):
        if v > best:
            best, at, n = v, i, 1
        elif v == best:
            n += 1
    return a[at], at, n, rho


def spread_of(a):
    top = bottom = a[0]
    for v in a[1:]:
        top = v if v > top else top
        bottom = v if v < bottom else bottom
    return top - bottom


def combine(a, rule, bins, r, lo, hi, seen=None):
    """(action, GRLX_TRAJ_ACTION_INDEX, GRLX_TRAJ_N_MAX, kept, tie?) of the members' actions a; seen: a dict that collects which branches
    were taken (occupied bins, removals of a member other than the first alive, selections other than member 0)"""
    seen = {} if seen is None else seen
    if rule == MEAN:
        return mean(a), -1, 1, len(a), False
    if rule == BINNING:
        action, binmax, n_bins, n, occupied = binning(a, bins, lo, hi)
        seen["occupied"] = max(seen.get("occupied", 0), occupied)
        return action, binmax, n_bins, n, n_bins > 1
    if rule == DATA_CENTER:
        action, most, kept, removed = data_center(a, bins)
        seen["removals"] = seen.get("removals", 0) + len(removed)
        seen["not_first"] = seen.get("not_first", 0) + sum(1 for at, first in removed if at != first)
        return action, -1, most, kept, most > 1
    assert rule == DENSITY
    action, at, n, _ = density(a, r, lo, hi)
    seen["not_first"] = seen.get("not_first", 0) + (1 if at != 0 else 0)
    return action, at, n, 1, n > 1


def member_actions(members, spec, obs):
    """a_m: the action policy_evaluate_ref.greedy_action hands the environment for member m, whose tables are members[m]"""
    return [float(ev.greedy_action(tables, spec, obs)[0]) for tables in members]


def episode(members, spec, state, rule, bins=10, r=0.001, max_steps=0, seen=None):
    """dict of one episode's outputs; members[m] = the tables of member m (policy_evaluate_ref.tables_of); records: [steps][R] with
    R = 6 + D + S + 2; actions: the members' actions of every step"""
    rule = RULES.get(rule, rule)
    max_steps = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    gamma, lo, hi = float(spec.gamma), float(spec.action_min), float(spec.action_max)
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec, x)
    ret, disc, g, steps, ties, kept, spread, code = 0.0, 0.0, 1.0, 0, 0, 0, 0.0, 0
    records, actions = [], []
    while True:
        a = member_actions(members, spec, obs)
        action, index, n_max, k, tie = combine(a, rule, bins, r, lo, hi, seen)
        wide = spread_of(a)
        nx, nobs, reward, term = ob.env_step(spec, x, action)
        before, x, obs, reward = obs, nx[0], nobs[0], float(reward[0])
        ret += reward
        disc += g * reward
        g = g * gamma
        steps += 1
        ties += 1 if tie else 0
        kept += k
        spread += wide
        code = ev.DOMAIN if not ev.in_domain(spec, x) else int(term[0])
        records.append([action, reward, mean(a), float(index), float(n_max), float(code)] + list(before) + list(x) + [float(k), wide])
        actions.append(a)
        if code != 0 or steps >= max_steps:
            break
    return dict(ret=ret, disc=disc, steps=steps, terminal=code, ties=ties, kept=kept, spread=spread, final_state=x,
                records=np.array(records, np.float64), actions=actions)


def evaluate(members, spec, states, rule, bins=10, r=0.001, max_steps=40, seen=None):
    """one group: dict of the eight outputs [n], records [n][max_steps][R] (zeros behind an episode's end) and actions [n][step][member]"""
    eps = [episode(members, spec, s, rule, bins, r, max_steps, seen) for s in states]
    out = {f: np.array([ep[f] for ep in eps]) for f in FIELDS}
    out["steps"], out["terminal"], out["ties"] = (out[f].astype(np.int32) for f in ("steps", "terminal", "ties"))
    out["kept"] = out["kept"].astype(np.int64)
    R = eps[0]["records"].shape[1]
    out["records"] = np.zeros((len(states), max_steps, R), np.float64)
    for s, ep in enumerate(eps):
        out["records"][s, :ep["steps"]] = ep["records"]
    out["actions"] = [ep["actions"] for ep in eps]
    return out
