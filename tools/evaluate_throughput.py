#!/usr/bin/env python3
"""evaluate_throughput.py [replicas [starts-per-side [trials [composed-replicas]]]] -- what a greedy evaluation costs: seconds per call,
episodes/s and pair-steps/s (one pair-step = one environment step of one (replica, start state) pair = one env-step) of
(a) grlx_evaluate: all replicas x all start states, whole episodes, in one call (evaluate_q_kernel<pendulum, 3>), host arrays in and out, and
(b) the path it replaces, composed from the entry points there were: per control step one grlx_query_q per replica (a query takes the
    cross product replicas x observations, and every pair is at an observation of its own) and one grlx_env_step over all pairs, the
    sums in numpy.  At 4096 replicas that is 4096 calls per step, so this leg runs on the first `composed-replicas` replicas only
    (8 by default) and is compared per pair-step; its first observation comes from the device's own fmod (grlx_math).
on 4096 pendulum SARSA replicas after 100 trials from a 16 x 16 grid of start states at time 0 (1 M episodes of 100 steps) by default.
Three runs of each (a run: ten calls), alternated in one process on one context after a warm-up call of each; the two legs' outputs are compared bit for bit
on the replicas both ran.  Also printed: the share of the waves' step slots lost to ragged episode ends, from `steps` (a wave holds four
consecutive pairs and runs as long as its longest episode).  Run it under a time limit of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner


def composed(r, cfg, states, actions, n_rep):
    n = states.shape[0]
    x = np.tile(states, (n_rep, 1))
    a = runner.device_math(runner.MATH_FMOD, x[:, 0] + np.pi, np.full(x.shape[0], 2 * np.pi))     # task/pendulum/swingup: observe
    a = np.where(a < 0, a + 2 * np.pi, a)
    obs = np.stack([a, x[:, 1]], axis=1)
    pairs = x.shape[0]
    ret, disc, g = np.zeros(pairs), np.zeros(pairs), np.ones(pairs)
    steps, terminal, ties = np.zeros(pairs, np.int32), np.zeros(pairs, np.int32), np.zeros(pairs, np.int32)
    active = np.ones(pairs, bool)
    while active.any():
        greedy, n_max = np.zeros(pairs, np.int64), np.zeros(pairs, np.int64)
        for k in range(n_rep):
            _, _, gk, mk = r.query_q(obs[k * n:(k + 1) * n], replicas=(k, 1))
            # the query is the cross product: row s of replica k's answer is pair (k, s)
            greedy[k * n:(k + 1) * n], n_max[k * n:(k + 1) * n] = gk[0], mk[0]
        nx, nobs, rew, term = runner.env_step(cfg, x, actions[greedy])
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * cfg.gamma, g)
        steps += active
        ties += active & (n_max > 1)
        terminal = np.where(active, term, terminal)
        x = np.where(active[:, None], nx, x)
        obs = np.where(active[:, None], nobs, obs)
        active = active & (term == 0)
    shape = (n_rep, n)
    return ret.reshape(shape), disc.reshape(shape), steps.reshape(shape), terminal.reshape(shape), ties.reshape(shape), x.reshape(shape + (3,))


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
    res = {"fused": [], "composed": []}
    out, pair_steps = {}, {}

    def call(leg):
        return r.evaluate(states) if leg == "fused" else composed(r, cfg, states, actions, n_rep)

    for leg in res:                                                          # warm-up at the timed shape: code object load, first-touch pages
        out[leg] = call(leg)
        pair_steps[leg] = int(np.asarray(out[leg][2]).sum())
    reps = {"fused": 10, "composed": 10}                                     # calls per timed window: about a second of work each
    for i in range(3):
        for leg in res:
            t0 = time.perf_counter()
            for _ in range(reps[leg]):                                       # every call ends in a device-to-host copy: synchronised
                out[leg] = call(leg)
            dt = (time.perf_counter() - t0) / reps[leg]
            res[leg].append(dt)
            nr = n if leg == "fused" else n_rep
            print(f"{nr} replicas x {states.shape[0]} starts  run {i}  {leg:9s} {dt:9.4f} s/call  {nr * states.shape[0] / dt / 1e3:11.3f} k episodes/s"
                  f"  {pair_steps[leg] / dt / 1e6:9.3f} M pair-steps/s (= env-steps/s)", flush=True)
    for name, a, b in zip(grl_amd.Evaluation._fields, out["fused"], out["composed"]):
        assert np.ascontiguousarray(a[:n_rep]).tobytes() == np.ascontiguousarray(b.astype(a.dtype)).tobytes(), f"the two legs differ in {name}"
    print(f"the two legs agree bit for bit on the {n_rep} replicas both ran")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    rate = {leg: pair_steps[leg] / med[leg] for leg in res}
    for leg, v in res.items():
        print(f"{leg:9s} median {med[leg]:.4f} s/call  {rate[leg] / 1e6:.3f} M pair-steps/s  min {min(v):.4f} s  max {max(v):.4f} s")
    print(f"fused / composed (pair-steps/s at the medians): {rate['fused'] / rate['composed']:.1f}x")
    steps = out["fused"].steps.reshape(-1).astype(np.int64)
    steps = np.concatenate([steps, np.zeros(-steps.size % 4, np.int64)]).reshape(-1, 4)
    slots = 4 * steps.max(axis=1).sum()
    print(f"ragged episode ends: {100.0 * (1.0 - steps.sum() / slots):.2f} % of the waves' step slots idle ({steps.sum()} pair-steps in {slots} slots)")
    r.close()


if __name__ == "__main__":
    main()
