#!/usr/bin/env python3
"""query_throughput.py [replicas [observations-per-side [trials]]] -- what a policy query costs: seconds per call and
(replica, observation) pairs/s of
(a) grlx_query_q: all replicas x all observations in one call (query_q_kernel<3>), host arrays in and out, and
(b) the path it replaces, composed from the entry points there were: one grlx_project over observations x actions, one
    grlx_get_weights per replica over the slots involved, the serial-order sums, the clip and findmax in numpy.  (grlx_get_weights, not
    grlx_read: like the query it creates no entries, so both legs can be alternated on one context.)
on 4096 pendulum SARSA replicas after 100 trials at a 16 x 16 grid of observations (1 M pairs) by default.  Three runs of each (a run:
ten calls of (a), one of (b)), alternated in one process on one context after a warm-up call of each; the two legs' outputs are compared bit for bit once.  Run it under a time limit of its own."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd


def composed(r, cfg, obs, actions):
    n, A = obs.shape[0], len(actions)
    rows = np.concatenate([np.repeat(obs, A, axis=0), np.tile(actions, n)[:, None]], axis=1)
    idx = grl_amd.runner.project(cfg.projector, rows)                      # [n * A][16]
    slots, inverse = np.unique(idx, return_inverse=True)
    inverse = inverse.reshape(idx.shape)
    lo, hi = cfg.representation.output_min, cfg.representation.output_max
    q = np.zeros((cfg.n_replicas, n, A))
    for k in range(cfg.n_replicas):
        w = r.weights(k, slots)[inverse]
        s = w[:, 0].copy()
        for j in range(1, 16):                                               # linear.cpp:147-151: the serial order
            s += w[:, j]
        q[k] = np.minimum(np.maximum(s / 16, lo), hi).reshape(n, A)
    best = q.max(axis=2, keepdims=True)
    n_max = (q == best).sum(axis=2)
    greedy = (q == best).argmax(axis=2)
    value = np.zeros(q.shape[:2])
    for a in range(A):
        value += q[:, :, a] * np.where(q[:, :, a] == best[:, :, 0], 1.0 / n_max, 0.0)
    return q, value, greedy.astype(np.int32), n_max.astype(np.int32)


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 4096
    side = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 100
    cfg = grl_amd.pendulum_sarsa_config(n, max_rows=trials // 10 + 2)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    r.run(trials); r.sync()
    obs = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    delta = (cfg.action_max - cfg.action_min) / (cfg.action_steps - 1)
    actions = np.array([cfg.action_min + delta * k for k in range(cfg.action_steps)])
    pairs = n * obs.shape[0]
    res = {"fused": [], "composed": []}
    out = {}
    reps = {"fused": 10, "composed": 1}                                      # calls per timed window: a window of milliseconds measures the clock
    for leg in res:                                                          # warm-up at the timed shape: code object load, first-touch pages
        out[leg] = r.query_q(obs) if leg == "fused" else composed(r, cfg, obs, actions)
    for i in range(3):
        for leg in res:
            t0 = time.perf_counter()
            for _ in range(reps[leg]):                                       # every call ends in a device-to-host copy: synchronised
                out[leg] = r.query_q(obs) if leg == "fused" else composed(r, cfg, obs, actions)
            dt = (time.perf_counter() - t0) / reps[leg]
            res[leg].append(dt)
            print(f"{n} replicas x {obs.shape[0]} observations  run {i}  {leg:9s} {dt:9.4f} s/call  {pairs / dt / 1e6:9.3f} M pairs/s", flush=True)
    for name, a, b in zip(("q", "value", "greedy", "n_max"), out["fused"], out["composed"]):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b.astype(a.dtype)).tobytes(), f"the two legs differ in {name}"
    print("the two legs agree bit for bit")
    med = {leg: sorted(v)[1] for leg, v in res.items()}
    for leg, v in res.items():
        print(f"{leg:9s} median {med[leg]:.4f} s/call  {pairs / med[leg] / 1e6:.3f} M pairs/s  min {min(v):.4f}  max {max(v):.4f}")
    print(f"composed / fused (medians): {med['composed'] / med['fused']:.1f}x")
    r.close()


if __name__ == "__main__":
    main()
