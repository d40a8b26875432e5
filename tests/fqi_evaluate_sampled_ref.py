"""Reference of the batch path's sampled episodes (grlx_fqi_evaluate_sampled, grlx_fqi_evaluate_ensemble_sampled): plain Python loops over the
oracle's pieces.  The single network's loop is fqi_evaluate_ref.episode with the sampler of policy_evaluate_sampled_ref; the ensemble's is
policy_evaluate_ensemble_sampled_ref.episode with the members' q = [e.q(obs, a) ...] in place of the table read."""
import numpy as np

from tests import fqi_evaluate_ref as fr
from tests import oracle_binding as ob
from tests import policy_evaluate_ensemble_sampled_ref as esr
from tests import policy_evaluate_ref as ev
from tests import policy_evaluate_sampled_ref as sr
from tests.policy_evaluate_ensemble_sampled_ref import draw, member_distribution, ranks_of, softmax, vote_of
from tests.policy_query_ref import findmax

FIELDS, ENS_FIELDS = sr.FIELDS, esr.FIELDS
WORDS, ENS_WORDS = fr.WORDS + 1, 8 + fr.D + fr.S + 2


def _step(e, x, action):
    nx, nobs, reward, term = ob.env_step(e.spec.base, x, action)
    x = nx[0]
    return x, nobs[0], float(reward[0]), (ev.DOMAIN if not ev.in_domain(e.spec.base, x) else int(term[0]))


def _gather(eps, fields, n, max_steps, words):
    out = {f: np.array([ep[f] for ep in eps]) for f in fields}
    out["records"] = np.zeros((n, max_steps, words))
    for s, ep in enumerate(eps):
        out["records"][s, :ep["steps"]] = ep["records"]
    return out


def episode(e, state, sampler, eps, streams, max_steps=0):
    """one episode of FqiExperiment e under `sampler` (sr.GREEDY / sr.EPSILON) on streams = (sampler's word, global word)"""
    cap = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    actions = fr.actions_of(e.spec)
    S, G = ob.Rand48(int(streams[0])), ob.Rand48(int(streams[1]))
    x = np.array(state, np.float64)
    obs, _ = ev.observe(e.spec.base, x)
    ret, disc, g, steps, ties, explored, code, rows = 0.0, 0.0, 1.0, 0, 0, 0, 0, []
    while code == 0 and steps < cap:
        q = [e.q(obs, a) for a in actions]
        idx, man, tie, expl = sr.sample(q, sampler, eps, S, G)
        before = obs
        x, obs, reward, code = _step(e, x, actions[idx])
        ret, disc, g, steps = ret + reward, disc + g * reward, g * float(e.spec.gamma_tau), steps + 1
        ties, explored = ties + tie, explored + expl
        rows.append([actions[idx], reward, q[idx], float(idx), float(man), float(code)] + list(before) + list(x) + [float(expl)])
    return dict(ret=ret, disc=disc, steps=steps, terminal=code, ties=ties, explored=explored, final_state=x,
                streams=np.array([S.x, G.x], np.uint64), records=np.array(rows))


def evaluate(e, states, sampler, eps, streams, max_steps):
    return _gather([episode(e, states[s], sampler, eps, streams[s], max_steps) for s in range(len(states))], FIELDS, len(states), max_steps, WORDS)


def ensemble_episode(members, state, strategy, tau, member, param, stream, max_steps=0, seen=None):
    """one episode of the group `members` (FqiExperiments); seen: a dict that collects "dropped" (a softmax member dropped an entry)"""
    cap = max_steps if max_steps else ev.MAX_EPISODE_STEPS
    spec = members[0].spec
    actions = fr.actions_of(spec)
    g = ob.Rand48(int(stream))
    x = np.array(state, np.float64)
    obs, _ = ev.observe(spec.base, x)
    ret, disc, gg, steps, ties, mties, agree, explored, code, rows = 0.0, 0.0, 1.0, 0, 0, 0, 0, 0, 0, []
    while code == 0 and steps < cap:
        score, votes, mt = [0] * len(actions), [0] * len(actions), 0
        for e in members:
            d, man = member_distribution([e.q(obs, a) for a in actions], member, param)
            votes[vote_of(d)] += 1
            mt += man > 1
            if member == esr.SOFTMAX and seen is not None and 0.0 in d:
                seen["dropped"] = True
            if strategy == esr.RANK:
                score = [a + b for a, b in zip(score, ranks_of(d))]
        score = score if strategy == esr.RANK else list(votes)
        dist = softmax(score, tau)
        idx = draw(dist, g)
        mai, man = findmax(score)
        before = obs
        x, obs, reward, code = _step(members[0], x, actions[idx])
        ret, disc, gg, steps = ret + reward, disc + gg * reward, gg * float(spec.gamma_tau), steps + 1
        ties, mties, agree, explored = ties + (man > 1), mties + mt, agree + votes[idx], explored + (idx != mai)
        rows.append([actions[idx], reward, float(score[idx]), float(idx), float(man), float(code), float(votes[idx]), float(mt)] + list(before) + list(x) +
                    [float(idx != mai), dist[idx]])
    return dict(ret=ret, disc=disc, steps=steps, terminal=code, ties=ties, member_ties=mties, agreement=agree, explored=explored, final_state=x,
                streams=np.uint64(g.x), records=np.array(rows))


def evaluate_ensemble(members, states, strategy, tau, member, param, streams, max_steps, seen=None):
    eps = [ensemble_episode(members, states[s], strategy, tau, member, param, streams[s], max_steps, seen) for s in range(len(states))]
    return _gather(eps, ENS_FIELDS, len(states), max_steps, ENS_WORDS)
