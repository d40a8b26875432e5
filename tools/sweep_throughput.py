#!/usr/bin/env python3
"""sweep_throughput.py [replicas ...] -- what per-lane learning parameters cost: env-steps/s of pendulum SARSA as
(a) a uniform sweep context (every replica given the configuration's own alpha / gamma / lambda / epsilon: the SpecSweep
    instantiation, same arithmetic) and
(b) the same configuration with force_generic = 1 and the environment server off (run with GRLX_ENV_SERVER=0): the SpecNone
    instantiation, whose instruction stream the sweep did not change.
(c) a real sweep: the 64 points alpha x gamma x epsilon of the README's grid, lambda alternating 0.5 / 0.65 between neighbouring
    replicas.  Not the same arithmetic as (a) and (b) -- the pendulum's episodes have a fixed length, so the env-steps are the same --
    but the replicas of a wave now keep traces of different lengths, which takes td_update_lane off its steady-state write-back path.
Three runs of each, alternated in one process, each timed after the table-creation phase (11 trials) of its own context.
Replica counts default to 4096 (4 per wave) and 16384 (8 per wave)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd

TRIALS = 1100          # 450 M (4096 replicas) to 1.8 G (16384) env-steps in the timed window: about a second and more


def one(n, sweep):
    cfg = grl_amd.pendulum_sarsa_config(n, force_generic=1, max_rows=256)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    if sweep == "varied":
        g = grl_amd.sweep_grid(n // 64, alpha=[0.05, 0.1, 0.2, 0.25], gamma=[0.9, 0.93, 0.95, 0.97], epsilon=[0.01, 0.02, 0.05, 0.1])
        r.set_replica_params(lambda_=[0.5, 0.65] * (n // 2), **g)
    elif sweep:
        r.set_replica_params(alpha=[cfg.alpha] * n, gamma=[cfg.gamma] * n, lambda_=[cfg.lambda_] * n, epsilon=[cfg.epsilon] * n)
    r.run(11); r.sync()
    l0, t0s = r.step_counts()
    t0 = time.perf_counter(); r.run(TRIALS); r.sync(); dt = time.perf_counter() - t0
    l1, t1s = r.step_counts()
    assert r.last_kernel() == 1 and r.env_server_counts() == (0, 0), "not the generic kernel without the environment server: set GRLX_ENV_SERVER=0"
    rpw = r.replicas_per_wave()
    r.close()
    return ((l1 - l0) + (t1s - t0s)) / dt / 1e6, rpw


def main():
    if os.environ.get("GRLX_ENV_SERVER", "1") != "0":
        sys.exit("run with GRLX_ENV_SERVER=0: leg (b) is the generic kernel that integrates itself")
    for n in [int(a) for a in sys.argv[1:]] or [4096, 16384]:
        legs = {True: "(a) uniform sweep", False: "(b) force_generic", "varied": "(c) varied sweep "}
        res = {leg: [] for leg in legs}
        for i in range(3):
            for leg in legs:
                v, rpw = one(n, leg)
                res[leg].append(v)
                print(f"{n:6d} replicas ({rpw} per wave)  run {i}  {legs[leg]}  {v:8.1f} M env-steps/s", flush=True)
        for leg in legs:
            v = res[leg]
            print(f"{n:6d} replicas  {legs[leg]}  median {sorted(v)[1]:8.1f}  min {min(v):8.1f}  max {max(v):8.1f}  "
                  f"spread {(max(v) - min(v)) / sorted(v)[1] * 100:5.2f} %", flush=True)
        print(f"{n:6d} replicas  (a) / (b) medians: {sorted(res[True])[1] / sorted(res[False])[1]:.4f}   (c) / (b): {sorted(res['varied'])[1] / sorted(res[False])[1]:.4f}", flush=True)


if __name__ == "__main__":
    main()
