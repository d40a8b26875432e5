#!/usr/bin/env python3
"""evaluate_ensemble_sampled_throughput.py [replicas [starts-per-side [trials [group-size [composed-groups]]]]] -- what a sampled ensemble
evaluation costs: seconds per call, episode-steps/s (one environment step of one (group, start state) episode) and member-steps/s
(episode-steps x group size) of
(a) grlx_evaluate_ensemble_sampled, majority voting over greedy members (tau 1.0),
(b) the same call, rank voting over softmax members (tau 2.0, tau_m 1.0): against (a), the price of the members' exponentials placed
    once per (member, action),
(c) grlx_evaluate_ensemble under `vote`: the greedy ensemble kernel, the yardstick of (a),
(d) the path (a) and (b) replace, composed from the entry points there were: per control step one grlx_query_q per group (a query takes
    the cross product members x observations, and every episode is at an observation of its own), the members' distributions, the
    score, the combined softmax and the draw in numpy -- vectorised over the episodes, the exponentials through grlx_math, rand48 in
    64-bit integers --, and one grlx_env_step over all episodes; on the first `composed-groups` groups only (2 by default), under both
    settings, compared with (a) and (b) bit for bit on those groups,
on 4096 pendulum SARSA replicas after 100 trials in groups of 64, from a 16 x 16 grid of start states at time 0, by default.  Three runs
of each leg (a run: ten calls; a composed leg: one), alternated in one process on one context after a warm-up call of each; the clock
stops after the device-to-host copy.  Also printed per fused leg: the device time of its launches (grlx_read_kernel_timing, in a pass
of its own after the timed runs).  Run it under a time limit of its own."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner

LCG_A, LCG_C, MASK48 = np.uint64(0x5DEECE66D), np.uint64(0xB), np.uint64((1 << 48) - 1)


def pexp(x):
    return runner.device_math(runner.MATH_EXP, np.ascontiguousarray(x).reshape(-1)).reshape(x.shape)


def softmax(v, t):
    """include/grlx.h's softmax(v, t) over the last axis"""
    p = v / t
    maxp = p.max(axis=-1, keepdims=True)
    minp = maxp + (-100)
    center = (maxp + minp) / 2.0
    kept = p > minp
    e = np.where(kept, pexp(np.where(kept, p - center, 0.0)), 0.0)
    total = np.zeros(p.shape[:-1])
    for i in range(p.shape[-1]):
        total = np.where(kept[..., i], total + e[..., i], total)
    return np.where(kept, e / total[..., None], 0.0)


def act(q, rank, tau, tau_m, rng, active):
    """q[episode][member][action] -> (index drawn, score ties?, explored?, votes for it, members with a tie); rng advances where active"""
    eps, G, A = q.shape
    best = q.max(axis=2, keepdims=True)
    man = (q == best).sum(axis=2)
    d = softmax(q, tau_m) if tau_m else np.where(q == best, 1. / man[:, :, None], 0.)
    top, vote = np.zeros((eps, G)), np.full((eps, G), A - 1)
    for j in range(A):
        up = d[:, :, j] > top
        vote, top = np.where(up, j, vote), np.where(up, d[:, :, j], top)
    votes = (vote[:, :, None] == np.arange(A)).sum(axis=1)
    score = (1 + (d[:, :, :, None] > d[:, :, None, :]).sum(axis=3)).sum(axis=1) if rank else votes
    dist = softmax(score.astype(np.float64), tau)
    s = np.zeros(eps)
    for i in range(A):
        s = s + dist[:, i]
    rng[:] = np.where(active, (LCG_A * rng + LCG_C) & MASK48, rng)
    u = rng.astype(np.float64) * 2.0 ** -48 * s
    acc, idx, found = np.zeros(eps), np.full(eps, A - 1), np.zeros(eps, bool)
    for i in range(A):
        acc = acc + dist[:, i]
        here = ~found & (u < acc)
        idx, found = np.where(here, i, idx), found | here
    peak = score.max(axis=1)
    return idx, (score == peak[:, None]).sum(axis=1) > 1, idx != score.argmax(axis=1), votes[np.arange(eps), idx], (man > 1).sum(axis=1)


def composed(r, cfg, states, actions, G, n_groups, rank, tau, tau_m, streams):
    n = states.shape[0]
    x = np.tile(states, (n_groups, 1))
    a = runner.device_math(runner.MATH_FMOD, x[:, 0] + np.pi, np.full(x.shape[0], 2 * np.pi))     # task/pendulum/swingup: observe
    a = np.where(a < 0, a + 2 * np.pi, a)
    obs = np.stack([a, x[:, 1]], axis=1)
    eps = x.shape[0]
    rng = streams[:n_groups].reshape(-1).copy()
    ret, disc, g = np.zeros(eps), np.zeros(eps), np.ones(eps)
    steps, terminal, ties, explored = (np.zeros(eps, np.int32) for _ in range(4))
    member_ties, agreement = np.zeros(eps, np.int64), np.zeros(eps, np.int64)
    active = np.ones(eps, bool)
    while active.any():
        q = np.zeros((eps, G, len(actions)))
        for k in range(n_groups):
            # the query is the cross product: column s of group k's answer is episode (k, s)
            q[k * n:(k + 1) * n] = r.query_q(obs[k * n:(k + 1) * n], replicas=(k * G, G))[0].transpose(1, 0, 2)
        idx, tie, off, agree, mties = act(q, rank, tau, tau_m, rng, active)
        nx, nobs, rew, term = runner.env_step(cfg, x, actions[idx])
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * cfg.gamma, g)
        steps += active
        ties += active & tie
        explored += active & off
        member_ties += np.where(active, mties, 0)
        agreement += np.where(active, agree, 0)
        terminal = np.where(active, term, terminal)
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    shape = (n_groups, n)
    return grl_amd.SampledEnsembleEvaluation(*(v.reshape(shape) for v in (ret, disc, steps, terminal, ties, member_ties, agreement, explored)),
                                             x.reshape(shape + (states.shape[1],)), rng.reshape(shape))


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 4096
    side = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 100
    G = args[3] if len(args) > 3 else 64
    n_groups = n // G
    n_comp = min(args[4] if len(args) > 4 else 2, n_groups)
    cfg = grl_amd.pendulum_sarsa_config(n, max_rows=trials // 10 + 2)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    r.run(trials); r.sync()
    grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    states = np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1)    # time 0: full episodes
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    streams = grl_amd.episode_stream_words(5, n_groups, states.shape[0])
    settings = {"majority/greedy": ("majority", 1.0, "greedy", None), "rank/softmax": ("rank", 2.0, "softmax", 1.0)}
    calls = {"greedy vote": lambda: r.evaluate_ensemble(states, G, "vote")}
    for name, (strategy, tau, member, param) in settings.items():
        calls["fused " + name] = lambda s=strategy, t=tau, m=member, p=param: r.evaluate_ensemble_sampled(states, G, s, t, m, p, streams)
        if n_comp > 0:
            calls["composed " + name] = lambda s=strategy, t=tau, p=param: composed(r, cfg, states, actions, G, n_comp, s == "rank", t, p, streams)
    out, ep_steps, res = {}, {}, {leg: [] for leg in calls}
    for leg in calls:                                                        # warm-up at the timed shape: code object load, first-touch pages
        t0 = time.perf_counter()
        out[leg] = calls[leg]()
        ep_steps[leg] = int(np.asarray(out[leg].steps).sum())
        print(f"warm-up {leg:26s} {time.perf_counter() - t0:9.4f} s", flush=True)
    for i in range(3):
        for leg in calls:
            reps = 1 if leg.startswith("composed") else 10
            t0 = time.perf_counter()
            for _ in range(reps):                                            # every call ends in a device-to-host copy: synchronised
                out[leg] = calls[leg]()
            dt = (time.perf_counter() - t0) / reps
            res[leg].append(dt)
            print(f"run {i}  {leg:26s} {out[leg].steps.size:8d} episodes {dt:9.4f} s/call  {ep_steps[leg] / dt / 1e6:9.3f} M episode-steps/s", flush=True)
    for name in settings:
        if n_comp > 0:
            for field, a, b in zip(grl_amd.SampledEnsembleEvaluation._fields, out["fused " + name], out["composed " + name]):
                assert np.ascontiguousarray(a[:n_comp]).tobytes() == np.ascontiguousarray(b.astype(a.dtype)).tobytes(), f"{name}: the two legs differ in {field}"
    if n_comp > 0:
        print(f"the fused and the composed legs agree bit for bit under both settings on the {n_comp} groups both ran")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    for leg, v in res.items():
        print(f"{leg:26s} median {med[leg]:.4f} s/call  min {min(v):.4f}  max {max(v):.4f}  {ep_steps[leg] / med[leg] / 1e6:10.3f} M episode-steps/s"
              f"  {ep_steps[leg] * G / med[leg] / 1e6:10.3f} M member-steps/s")
    rate = lambda leg: ep_steps[leg] / med[leg]
    print(f"(a) / (c), majority over greedy members against the greedy vote (episode-steps/s at the medians): {rate('fused majority/greedy') / rate('greedy vote'):.2f}x")
    print(f"(b) / (a), rank over softmax members against majority over greedy members: {rate('fused rank/softmax') / rate('fused majority/greedy'):.2f}x")
    for name in settings:
        v = out["fused " + name]
        line = f"{name}: explored at {100.0 * v.explored.sum() / v.steps.sum():.2f} % of the steps, the score tied at {100.0 * v.ties.sum() / v.steps.sum():.2f} %"
        if n_comp > 0:
            line += f";  fused / composed: {rate('fused ' + name) / rate('composed ' + name):.1f}x"
        print(line)
    ms, chunks = C.c_double(0), C.c_int(0)
    for leg in calls:
        if leg.startswith("composed"):
            continue
        r.lib.grlx_read_kernel_timing(1, None, None)
        for _ in range(3):
            calls[leg]()
        r.lib.grlx_read_kernel_timing(0, C.byref(ms), C.byref(chunks))
        print(f"{leg:26s} device time of the launches: {ms.value / 3:.3f} ms per call ({chunks.value // 3} chunk(s)); {ep_steps[leg] / (ms.value / 3) / 1e3:.3f} M episode-steps/s")
    r.close()


if __name__ == "__main__":
    main()
