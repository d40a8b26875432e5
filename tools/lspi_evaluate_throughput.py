#!/usr/bin/env python3
"""lspi_evaluate_throughput.py [--json] | --ab LIB [rounds] | --profile DIR -- what the LSPI context's evaluation calls cost on the GPU
(profiles/lspi_evaluate.md).

Shape: 16 replicas of the reference's cfg/pendulum/lspi_triangle.yaml and lspi_gauss.yaml after one batch, 256 start states (a 16 x 16
grid of angles and velocities at time 0), episodes of 100 steps.  Per projector, seconds per call by a host clock around the call (every
call ends in a device synchronise and the copy back): evaluate, evaluate_trajectory (max_steps 100), evaluate_ensemble (4 groups of 4)
under both rules.  The calls are warmed up once, then timed in rounds that alternate between them; the figure is the median round.

The composed path -- one grlx_lspi_query per replica and one grlx_env_step per control step from the host, what a caller had before
these calls -- runs on 2 replicas and is ASSERTED bit for bit equal to evaluate (ret, disc, steps, terminal, ties, final_state); its
time is for those 2 replicas, beside evaluate's for the same 2.  The observation of step 0 is taken from a one-step trajectory.

--ab LIB: the same figures from this tree's library and from LIB (GRLX_LIB) in alternating fresh child processes: the measurement builds
of grlx_lspi_evaluate.hip (-DGRLX_LSPI_EVAL_FULL_WALK: lspi_read's walk of the whole grid inside the same kernel;
-DGRLX_LSPI_ENS_LDS: the ensemble with its group's weights staged in LDS), each built with GRLX_EXTRA_FLAGS and copied aside.
--profile DIR: one pass under `rocprofv3 --kernel-trace --stats` as a child process of its own, and the kernels' times from its statistics."""
import csv, glob, json, math, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_REPLICAS, GROUP, STEPS, ROUNDS, REPS = 16, 4, 100, 5, 5


def start_states():
    import numpy as np
    return np.array([[a, v, 0.0] for a in np.linspace(-math.pi, math.pi, 16) for v in np.linspace(-30.0, 30.0, 16)])


def composed(grlx, r, states, n_replicas):
    """the host-composed episodes of the replicas [0, n_replicas): (ret, disc, steps, terminal, ties, final_state), seconds"""
    import numpy as np
    online = grlx.pendulum_sarsa_config(1)
    actions = np.array([r.cfg.action_min + (r.cfg.action_max - r.cfg.action_min) / (float(r.cfg.action_steps) - 1) * k for k in range(r.cfg.action_steps)])
    gamma_tau = math.pow(r.cfg.gamma, r.cfg.control_step)
    first_obs = r.evaluate_trajectory(states, 1, replicas=(0, 1)).obs[0, :, 0]
    n = len(states)
    out = [np.zeros((n_replicas, n)), np.zeros((n_replicas, n)), np.zeros((n_replicas, n), np.int32), np.zeros((n_replicas, n), np.int32),
           np.zeros((n_replicas, n), np.int32), np.zeros((n_replicas, n, 3))]
    t0 = time.perf_counter()
    for k in range(n_replicas):
        x, obs, g, live = states.copy(), first_obs.copy(), np.ones(n), np.ones(n, bool)
        ret, disc, steps, code, ties, final = (o[k] for o in out)
        while live.any():
            q = r.query(obs, replicas=(k, 1))[0]
            mai = q.argmax(axis=1)                                  # the first maximum
            man = (q == q.max(axis=1, keepdims=True)).sum(axis=1)
            nx, nobs, rew, term = grlx.runner.env_step(online, x, actions[mai])
            ret[live] += rew[live]
            disc[live] += g[live] * rew[live]
            g = g * gamma_tau
            steps[live] += 1
            ties[live] += man[live] > 1
            code[live] = term[live]
            x[live], obs[live] = nx[live], nobs[live]
            live &= term == 0
        final[:] = x
    return out, time.perf_counter() - t0


def measure():
    import numpy as np
    import grl_amd as grlx
    states, result = start_states(), {}
    for projector in ("triangle", "gauss"):
        r = grlx.LspiRunner(grlx.pendulum_lspi_config(N_REPLICAS, projector, max_batches=1), np.arange(1, N_REPLICAS + 1))
        r.run_batch(); r.sync()
        calls = {"evaluate": lambda: r.evaluate(states), "evaluate_trajectory": lambda: r.evaluate_trajectory(states, STEPS),
                 "evaluate_ensemble vote": lambda: r.evaluate_ensemble(states, GROUP, rule="vote"),
                 "evaluate_ensemble mean": lambda: r.evaluate_ensemble(states, GROUP, rule="mean"),
                 "evaluate, 2 replicas": lambda: r.evaluate(states, replicas=(0, 2))}
        for f in calls.values():
            f()
        rounds = {name: [] for name in calls}
        for _ in range(ROUNDS):
            for name, f in calls.items():
                t0 = time.perf_counter()
                for _ in range(REPS):
                    f()
                rounds[name].append((time.perf_counter() - t0) / REPS)
        for name, t in rounds.items():
            result[f"{projector}: {name}"] = dict(ms=statistics.median(t) * 1e3, lo=min(t) * 1e3, hi=max(t) * 1e3)
        if "--no-composed" not in sys.argv:
            want = r.evaluate(states, replicas=(0, 2))
            assert (want.steps == STEPS).all(), "the shape is episodes of 100 steps"
            got, seconds = composed(grlx, r, states, 2)
            for a, b, name in zip(got, want, "ret disc steps terminal ties final_state".split()):
                assert a.tobytes() == np.ascontiguousarray(b).tobytes(), f"{projector}: the composed path's {name} differs from evaluate's"
            result[f"{projector}: composed path, 2 replicas (bit for bit equal)"] = dict(ms=seconds * 1e3, lo=seconds * 1e3, hi=seconds * 1e3)
        r.close()
    return result


def show(result, title=""):
    print(title or f"{N_REPLICAS} replicas x 256 start states x {STEPS} steps; ms per call, median of {ROUNDS} alternating rounds of {REPS} calls (min ... max)")
    for name, v in result.items():
        print(f"  {name:62s} {v['ms']:10.3f}   ({v['lo']:.3f} ... {v['hi']:.3f})")


def ab(lib, rounds):
    runs = {"this tree": [], lib: []}
    for _ in range(rounds):
        for which in runs:
            env = dict(os.environ)
            if which != "this tree":
                env["GRLX_LIB"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--json", "--no-composed"], env=env, check=True, capture_output=True, text=True).stdout
            runs[which].append(json.loads(out.strip().split("\n")[-1]))
    for which, rs in runs.items():
        show({k: dict(ms=statistics.median(x[k]["ms"] for x in rs), lo=min(x[k]["lo"] for x in rs), hi=max(x[k]["hi"] for x in rs)) for k in rs[0]},
             f"{which}: median of {rounds} alternating processes")


def profile(out):
    os.makedirs(out, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "lspi_evaluate", "--", sys.executable,
                    os.path.abspath(__file__), "--json", "--no-composed"], check=True)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel statistics under {out}")
    print(f"{'kernel':110s} {'calls':>6s} {'mean us':>10s}")
    for x in csv.DictReader(open(files[0])):
        if "lspi_evaluate" in x["Name"] or "lspi_query" in x["Name"]:
            print(f"{x['Name'][:110]:110s} {int(x['Calls']):6d} {float(x['TotalDurationNs']) / 1e3 / int(x['Calls']):10.1f}")


if __name__ == "__main__":
    if "--ab" in sys.argv:
        i = sys.argv.index("--ab")
        ab(sys.argv[i + 1], int(sys.argv[i + 2]) if len(sys.argv) > i + 2 else 3)
    elif "--profile" in sys.argv:
        profile(sys.argv[sys.argv.index("--profile") + 1])
    else:
        res = measure()
        if "--json" in sys.argv:
            print(json.dumps(res))
        else:
            show(res)
