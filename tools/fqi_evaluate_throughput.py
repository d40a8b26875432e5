#!/usr/bin/env python3
"""fqi_evaluate_throughput.py [replicas [starts-per-side [batches]]] -- what a greedy evaluation of the batch path costs: seconds per
call, episodes/s and pair-steps/s (one pair-step = one environment step of one (replica, start state) pair) of
(a) grlx_fqi_evaluate: all replicas x all start states, whole episodes, in one call (fqi_evaluate_kernel<20, false>), host arrays in and out,
(b) grlx_fqi_evaluate_trajectory over the same pairs with max_steps = 100 (fqi_evaluate_kernel<20, true>: 11 doubles per step and pair more
    to write, stage and copy), and
(c) the path there was before: per control step one grlx_fqi_query per replica (a query takes the cross product replicas x observations,
    and every pair is at an observation of its own) and one grlx_env_step over all pairs, findmax and the sums in numpy; its first
    observation comes from the device's own fmod (grlx_math),
on 16 replicas of the reference's pendulum-fqi-ann.yaml after two batches, from a 16 x 16 grid of start states at time 0 (4096 episodes
of 100 steps) by default.  Three runs of each, alternated in one process on one context after a warm-up call of each; the legs' outputs are
compared bit for bit.  Also printed: the share of the waves' step slots lost to ragged episode ends, from `steps` (a wave holds 64
consecutive start states of one replica and runs as long as its longest episode).  Run it under a time limit of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import runner


def composed(r, ecfg, gamma_tau, states, actions, n_rep):
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
        q = np.concatenate([r.query(obs[k * n:(k + 1) * n], replicas=(k, 1))[0] for k in range(n_rep)])     # [pair][action]
        greedy = np.argmax(q, axis=1)                                        # the first maximum
        n_max = (q == q.max(axis=1, keepdims=True)).sum(axis=1)
        nx, nobs, rew, term = runner.env_step(ecfg, x, actions[greedy])
        ret = np.where(active, ret + rew, ret)
        disc = np.where(active, disc + g * rew, disc)
        g = np.where(active, g * gamma_tau, g)
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
    n = args[0] if len(args) > 0 else 16
    side = args[1] if len(args) > 1 else 16
    batches = args[2] if len(args) > 2 else 2
    cfg = grl_amd.pendulum_fqi_config(n, max_batches=batches)
    r = grl_amd.FqiRunner(cfg, np.arange(1, n + 1))
    for _ in range(batches):
        r.run_batch()
    r.sync()
    ecfg = grl_amd.pendulum_sarsa_config(1, control_step=cfg.control_step, integration_steps=cfg.integration_steps, timeout=cfg.timeout)
    gamma_tau = float(cfg.gamma) ** float(cfg.control_step)
    grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    states = np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1)    # time 0: full episodes
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    max_steps = int(np.ceil(cfg.timeout / cfg.control_step)) + 1
    res = {"fused": [], "trajectory": [], "composed": []}
    out, pair_steps = {}, {}

    def call(leg):
        if leg == "fused":
            return r.evaluate(states)
        if leg == "trajectory":
            return r.evaluate_trajectory(states, max_steps)
        return composed(r, ecfg, gamma_tau, states, actions, n)

    for leg in res:                                                          # warm-up at the timed shape: code object load, first-touch pages
        out[leg] = call(leg)
        pair_steps[leg] = int(np.asarray(out[leg][2]).sum())
    reps = {"fused": 300, "trajectory": 60, "composed": 3}                   # calls per timed window: about a third of a second each
    for i in range(3):
        for leg in res:
            t0 = time.perf_counter()
            for _ in range(reps[leg]):                                       # every call ends in a device-to-host copy: synchronised
                out[leg] = call(leg)
            dt = (time.perf_counter() - t0) / reps[leg]
            res[leg].append(dt)
            print(f"{n} replicas x {states.shape[0]} starts  run {i}  {leg:10s} {dt:9.4f} s/call  {n * states.shape[0] / dt / 1e3:11.3f} k episodes/s"
                  f"  {pair_steps[leg] / dt / 1e6:9.3f} M pair-steps/s", flush=True)
    for name, a, b, c in zip(grl_amd.Evaluation._fields, out["fused"], out["composed"], out["trajectory"]):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b.astype(a.dtype)).tobytes(), f"fused and composed differ in {name}"
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(c).tobytes(), f"fused and trajectory differ in {name}"
    print(f"the three legs agree bit for bit on all {n} replicas; ties in {int((out['fused'].ties > 0).sum())} of {out['fused'].ties.size} episodes,"
          f" action indices used: {sorted(set(int(v) for v in np.unique(out['trajectory'].action_index[out['trajectory'].n_max > 0])))}")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    rate = {leg: pair_steps[leg] / med[leg] for leg in res}
    for leg, v in res.items():
        print(f"{leg:10s} median {med[leg]:.4f} s/call  {rate[leg] / 1e6:.3f} M pair-steps/s  min {min(v):.4f} s  max {max(v):.4f} s")
    print(f"fused / composed (pair-steps/s at the medians): {rate['fused'] / rate['composed']:.1f}x")
    print(f"trajectory / fused (s/call at the medians): {med['trajectory'] / med['fused']:.2f}x")
    steps = out["fused"].steps.astype(np.int64)
    pad = -steps.shape[1] % 64
    waves = np.concatenate([steps, np.zeros((steps.shape[0], pad), np.int64)], axis=1).reshape(steps.shape[0], -1, 64)
    slots = 64 * waves.max(axis=2).sum()
    print(f"ragged episode ends: {100.0 * (1.0 - steps.sum() / slots):.2f} % of the waves' step slots idle ({steps.sum()} pair-steps in {slots} slots)")
    r.close()


if __name__ == "__main__":
    main()
