#!/usr/bin/env python3
"""evaluate_sampled_throughput.py [replicas [starts-per-side [trials [composed-replicas]]]] -- what a sampled evaluation costs: seconds per
call, episodes/s and pair-steps/s (one pair-step = one environment step of one (replica, start state) pair) of
(a) grlx_evaluate_sampled with the epsilon-greedy sampler at epsilon 0.05 and (b) with the greedy sampler, both on the streams of
    grlx_episode_streams, all replicas x all start states, whole episodes, one call each (evaluate_sampled_kernel<pendulum, 3>),
(c) grlx_evaluate at the same shape (with GRLX_LIB naming the parent commit's library and the fourth argument 0 this leg alone runs: the
    parent's figure, taken in a process of its own on the same box), and
(d) the path (a) replaces, composed from the entry points there were: per control step one grlx_query_q per replica, the sampler's draws in
    Python (the 48-bit generator in numpy's uint64), one grlx_env_step over all pairs, the sums in numpy -- on the first
    `composed-replicas` replicas only (8 by default), compared with (a) bit for bit on those replicas, streams and explored included,
on 4096 pendulum SARSA replicas after 100 trials from a 16 x 16 grid of start states at time 0 (1 M episodes of 100 steps) by default.
Three runs of each leg (a run: ten calls; the composed leg: one), alternated in one process on one context after a warm-up call of each;
the clock stops after the device-to-host copy.  Also printed per fused leg: the device time of its launches (grlx_read_kernel_timing, in
a pass of its own after the timed runs).  Run it under a time limit of its own."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner

A48, C48, MASK = np.uint64(0x5DEECE66D), np.uint64(0xB), np.uint64((1 << 48) - 1)


def lcg(x):
    return (A48 * x + C48) & MASK          # uint64 arithmetic wraps modulo 2^64: the low 48 bits are exact


def composed(r, cfg, states, actions, n_rep, epsilon, streams):
    n, na = states.shape[0], len(actions)
    x = np.tile(states, (n_rep, 1))
    a = runner.device_math(runner.MATH_FMOD, x[:, 0] + np.pi, np.full(x.shape[0], 2 * np.pi))     # task/pendulum/swingup: observe
    a = np.where(a < 0, a + 2 * np.pi, a)
    obs = np.stack([a, x[:, 1]], axis=1)
    pairs = x.shape[0]
    S, G = streams[:n_rep, :, 0].reshape(-1).copy(), streams[:n_rep, :, 1].reshape(-1).copy()
    ret, disc, g = np.zeros(pairs), np.zeros(pairs), np.ones(pairs)
    steps, terminal, ties, explored = (np.zeros(pairs, np.int32) for _ in range(4))
    active = np.ones(pairs, bool)
    while active.any():
        q = np.zeros((pairs, na))
        for k in range(n_rep):
            q[k * n:(k + 1) * n] = r.query_q(obs[k * n:(k + 1) * n], replicas=(k, 1))[0][0]
        best = q.max(axis=1)
        is_max = q == best[:, None]
        man = is_max.sum(axis=1)
        S1 = lcg(S)
        explore = active & (S1.astype(np.float64) * 2.0 ** -48 < epsilon)
        tie = active & ~explore & (man > 1)
        draw = explore | tie
        G1 = lcg(G)
        lrand = (G1 >> np.uint64(17)).astype(np.int64)
        jj = lrand % np.maximum(man, 1)
        nth = np.cumsum(is_max, axis=1) - 1                                    # rank of every maximal entry among the maxima
        tie_idx = np.argmax(is_max & (nth == jj[:, None]), axis=1)
        idx = np.where(explore, lrand % na, np.where(tie, tie_idx, np.argmax(is_max, axis=1)))
        S = np.where(active, S1, S)
        G = np.where(draw, G1, G)
        nx, nobs, rew, term = runner.env_step(cfg, x, actions[idx])
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * cfg.gamma, g)
        steps += active
        ties += tie
        explored += explore
        terminal = np.where(active, term, terminal)
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    shape = (n_rep, n)
    return grl_amd.SampledEvaluation(ret.reshape(shape), disc.reshape(shape), steps.reshape(shape), terminal.reshape(shape), ties.reshape(shape),
                                     explored.reshape(shape), x.reshape(shape + (3,)), np.stack([S, G], axis=1).reshape(shape + (2,)))


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 4096
    side = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 100
    n_rep = min(args[3] if len(args) > 3 else 8, n)
    cfg = grl_amd.pendulum_sarsa_config(n, max_rows=trials // 10 + 2)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    r.run(trials); r.sync()
    grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    states = np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1)    # time 0: full episodes
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    sampled = hasattr(r.lib, "grlx_evaluate_sampled")                        # GRLX_LIB may name the parent's library: leg (c) alone
    streams = grl_amd.episode_streams(7, n, states.shape[0]) if sampled else None
    calls = {"evaluate": lambda: r.evaluate(states)}
    if sampled:
        calls["eps 0.05"] = lambda: r.evaluate_sampled(states, "epsilon", 0.05, streams)
        calls["greedy"] = lambda: r.evaluate_sampled(states, "greedy", 0.0, streams)
        if n_rep > 0:
            calls["composed"] = lambda: composed(r, cfg, states, actions, n_rep, 0.05, streams)
    out, pair_steps, res = {}, {}, {leg: [] for leg in calls}
    for leg in calls:                                                        # warm-up at the timed shape: code object load, first-touch pages
        out[leg] = calls[leg]()
        pair_steps[leg] = int(np.asarray(out[leg].steps).sum())
    for i in range(3):
        for leg in calls:
            reps = 1 if leg == "composed" else 10
            t0 = time.perf_counter()
            for _ in range(reps):                                            # every call ends in a device-to-host copy: synchronised
                out[leg] = calls[leg]()
            dt = (time.perf_counter() - t0) / reps
            res[leg].append(dt)
            nr = n_rep if leg == "composed" else n
            print(f"{nr} replicas x {states.shape[0]} starts  run {i}  {leg:9s} {dt:9.4f} s/call  {nr * states.shape[0] / dt / 1e3:11.3f} k episodes/s"
                  f"  {pair_steps[leg] / dt / 1e6:9.3f} M pair-steps/s", flush=True)
    if "composed" in calls:
        for name, a, b in zip(grl_amd.SampledEvaluation._fields, out["eps 0.05"], out["composed"]):
            assert np.ascontiguousarray(a[:n_rep]).tobytes() == np.ascontiguousarray(b.astype(a.dtype)).tobytes(), f"the composed leg differs in {name}"
        print(f"eps 0.05 and the composed leg agree bit for bit on the {n_rep} replicas both ran (explored there: {int(out['composed'].explored.sum())} steps)")
    if sampled:
        e, g = out["evaluate"], out["greedy"]
        print(f"greedy sampler: {int(g.ties.sum())} tie breaks drawn; equal to grlx_evaluate where it reports no tie: "
              f"{bool((g.ret[e.ties == 0] == e.ret[e.ties == 0]).all())}; explored at eps 0.05: {int(out['eps 0.05'].explored.sum())} of {pair_steps['eps 0.05']} steps")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    for leg, v in res.items():
        print(f"{leg:9s} median {med[leg]:.4f} s/call  {pair_steps[leg] / med[leg] / 1e6:.3f} M pair-steps/s  min {min(v):.4f} s  max {max(v):.4f} s")
    if sampled:
        for leg in ("eps 0.05", "greedy"):
            print(f"{leg} / evaluate (s/call at the medians): {med[leg] / med['evaluate']:.3f}")
        if "composed" in calls:
            print(f"eps 0.05 / composed (pair-steps/s at the medians): {pair_steps['eps 0.05'] / med['eps 0.05'] / (pair_steps['composed'] / med['composed']):.1f}x")
    ms, chunks = C.c_double(0), C.c_int(0)
    for leg in calls:
        if leg == "composed":
            continue
        r.lib.grlx_read_kernel_timing(1, None, None)
        for _ in range(3):
            calls[leg]()
        r.lib.grlx_read_kernel_timing(0, C.byref(ms), C.byref(chunks))
        print(f"{leg:9s} device time of the launches: {ms.value / 3:.3f} ms per call ({chunks.value // 3} chunk(s))")
    r.close()


if __name__ == "__main__":
    main()
