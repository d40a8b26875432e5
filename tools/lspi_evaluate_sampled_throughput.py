#!/usr/bin/env python3
"""lspi_evaluate_sampled_throughput.py [--json] | --profile DIR -- what the LSPI context's sampled episodes cost on the GPU beside their
greedy siblings (profiles/lspi_evaluate_sampled.md).

Shape, as tools/lspi_evaluate_throughput.py: 16 replicas of the reference's cfg/pendulum/lspi_triangle.yaml and lspi_gauss.yaml after one
batch, 256 start states (a 16 x 16 grid of angles and velocities at time 0), episodes of 100 steps.  Per projector, ms per call by a host
clock around the call (every call ends in a device synchronise and the copy back): evaluate beside evaluate_sampled (greedy sampler, and
epsilon = 0.1); evaluate_ensemble (vote) beside evaluate_ensemble_sampled (majority over greedy members, rank over softmax members) in
4 groups of 4 and in 1 group of 16.  The calls are warmed up once, then timed in rounds that alternate between them in one process; the
figure is the median round, with the smallest and the largest beside it.

The composed path -- one grlx_lspi_query for the group and one grlx_env_step per control step from the host, the members' distributions,
votes and ranks, the combined softmax and the draw in numpy (the exponential: grlx_math's pexp; the stream: rand48 on uint64), what a
caller had before these calls -- runs on ONE group of 4 under both (strategy, member) pairs and is ASSERTED byte for byte equal to
evaluate_ensemble_sampled in every output (ret, disc, steps, terminal, ties, member_ties, agreement, explored, final_state, streams)
before any time is reported; its time stands beside the call's for the same group.  --no-composed leaves it out (the profile pass).

--profile DIR: one pass under `rocprofv3 --kernel-trace --stats` as a child process of its own, and the kernels' times from its statistics."""
import csv, glob, json, math, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_REPLICAS, STEPS, ROUNDS, REPS, GROUP = 16, 100, 5, 5, 4
PAIRS = (("majority", 1.0, "greedy", None), ("rank", 2.0, "softmax", 1.0))      # (strategy, tau, member sampler, its parameter)


def softmax(v, t, pexp):
    """SoftmaxSampler::distribution (softmax.cpp:65-110) per row of v[n][A], as include/grlx.h restates it: the sum in index order"""
    import numpy as np
    p = v / t
    maxp = p.max(axis=1, keepdims=True)
    minp = maxp + (-100)
    center = (maxp + minp) / 2.0
    kept = p > minp
    e = np.where(kept, pexp(np.where(kept, p - center, 0.0)), 0.0)
    total = np.zeros(len(v))
    for a in range(v.shape[1]):
        total = np.where(kept[:, a], total + e[:, a], total)
    return np.where(kept, e / total[:, None], 0.0)


def composed(grlx, r, states, strategy, tau, member, param, streams):
    """the host-composed episodes of the group of replicas [0, GROUP): evaluate_ensemble_sampled's ten outputs [1][n], seconds"""
    import numpy as np
    online = grlx.pendulum_sarsa_config(1)
    A, n = int(r.cfg.action_steps), len(states)
    actions = np.array([r.cfg.action_min + (r.cfg.action_max - r.cfg.action_min) / (float(A) - 1) * k for k in range(A)])
    gamma_tau = math.pow(r.cfg.gamma, r.cfg.control_step)
    pexp = lambda x: grlx.runner.device_math(grlx.runner.MATH_EXP, x).reshape(x.shape)
    obs = r.evaluate_trajectory(states, 1, replicas=(0, 1)).obs[0, :, 0].copy()
    x, g, live, rng = states.copy(), np.ones(n), np.ones(n, bool), streams.astype(np.uint64).copy()
    ret, disc, final = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    steps, code, ties, explored = (np.zeros(n, np.int32) for _ in range(4))
    mties, agreement = np.zeros(n, np.int64), np.zeros(n, np.int64)
    rows = np.arange(n)
    t0 = time.perf_counter()
    while live.any():
        votes, ranks, tied = np.zeros((n, A), np.int64), np.zeros((n, A), np.int64), np.zeros(n, np.int64)
        for q in r.query(obs, replicas=(0, GROUP)):                # q[n][A] of one member
            best = q.max(axis=1, keepdims=True)
            man = (q == best).sum(axis=1)
            d = softmax(q, param, pexp) if member == "softmax" else np.where(q == best, 1. / man[:, None], 0.)
            top, vote = np.zeros(n), np.full(n, A - 1)             # multi_discrete.cpp:218-229
            for a in range(A):
                up = d[:, a] > top
                vote, top = np.where(up, a, vote), np.where(up, d[:, a], top)
            votes[rows, vote] += 1
            ranks += 1 + (d[:, :, None] > d[:, None, :]).sum(axis=2)
            tied += man > 1
        score = ranks if strategy == "rank" else votes
        dist = softmax(score.astype(np.float64), tau, pexp)
        total = np.zeros(n)
        for a in range(A):
            total = total + dist[:, a]
        drawn = (rng * np.uint64(0x5DEECE66D) + np.uint64(0xB)) & np.uint64((1 << 48) - 1)      # one drand48 of the episode's word
        u, acc, idx, found = drawn.astype(np.float64) * 2.0 ** -48 * total, np.zeros(n), np.full(n, A - 1), np.zeros(n, bool)
        for a in range(A):                                         # grl::sample (utils.h:227-250)
            acc = acc + dist[:, a]
            here = ~found & (u < acc)
            idx, found = np.where(here, a, idx), found | here
        mai, top_n = score.argmax(axis=1), (score == score.max(axis=1, keepdims=True)).sum(axis=1)
        nx, nobs, rew, term = grlx.runner.env_step(online, x, actions[idx])
        ret[live] += rew[live]
        disc[live] += g[live] * rew[live]
        g = g * gamma_tau
        steps[live] += 1
        ties[live] += top_n[live] > 1
        mties[live] += tied[live]
        agreement[live] += votes[rows, idx][live]
        explored[live] += (idx != mai)[live]
        code[live] = term[live]
        rng[live] = drawn[live]
        x[live], obs[live] = nx[live], nobs[live]
        live &= term == 0
    final[:] = x
    return [o[None] for o in (ret, disc, steps, code, ties, mties, agreement, explored, final, rng)], time.perf_counter() - t0


def measure():
    import numpy as np
    import grl_amd as grlx
    states, result = np.array([[a, v, 0.0] for a in np.linspace(-math.pi, math.pi, 16) for v in np.linspace(-30.0, 30.0, 16)]), {}
    one = grlx.episode_streams(1, N_REPLICAS, len(states))
    for projector in ("triangle", "gauss"):
        r = grlx.LspiRunner(grlx.pendulum_lspi_config(N_REPLICAS, projector, max_batches=1), np.arange(1, N_REPLICAS + 1))
        r.run_batch(); r.sync()
        calls = {"evaluate": lambda: r.evaluate(states), "evaluate_sampled greedy": lambda: r.evaluate_sampled(states, "greedy", None, one),
                 "evaluate_sampled epsilon 0.1": lambda: r.evaluate_sampled(states, "epsilon", 0.1, one)}
        for g in (4, 16):
            words = np.ascontiguousarray(one[:N_REPLICAS // g, :, 1])
            calls[f"evaluate_ensemble vote, groups of {g}"] = lambda g=g: r.evaluate_ensemble(states, g, rule="vote")
            calls[f"evaluate_ensemble_sampled majority / greedy, groups of {g}"] = lambda g=g, w=words: r.evaluate_ensemble_sampled(states, g, "majority", 1.0, "greedy", None, w)
            calls[f"evaluate_ensemble_sampled rank / softmax, groups of {g}"] = lambda g=g, w=words: r.evaluate_ensemble_sampled(states, g, "rank", 2.0, "softmax", 1.0, w)
        for f in calls.values():
            f()
        rounds = {name: [] for name in calls}
        for _ in range(ROUNDS):
            for name, f in calls.items():
                t0 = time.perf_counter()
                for _ in range(REPS):
                    f()
                rounds[name].append((time.perf_counter() - t0) / REPS)
        assert (r.evaluate(states).steps == STEPS).all(), "the shape is episodes of 100 steps"
        for name, t in rounds.items():
            result[f"{projector}: {name}"] = dict(ms=statistics.median(t) * 1e3, lo=min(t) * 1e3, hi=max(t) * 1e3)
        if "--no-composed" not in sys.argv:
            words = np.ascontiguousarray(one[:1, :, 1])
            for strategy, tau, member, param in PAIRS:
                call = lambda: r.evaluate_ensemble_sampled(states, GROUP, strategy, tau, member, param, words, replicas=(0, GROUP))
                want = call()
                assert (want.steps == STEPS).all()
                got, seconds = composed(grlx, r, states, strategy, tau, member, param, words[0])
                for a, b, name in zip(got, want, want._fields):
                    assert a.tobytes() == np.ascontiguousarray(b).tobytes(), f"{projector} {strategy} / {member}: the composed path's {name} differs from the call's"
                t0 = time.perf_counter()
                for _ in range(REPS):
                    call()
                ms = (time.perf_counter() - t0) / REPS * 1e3
                result[f"{projector}: evaluate_ensemble_sampled {strategy} / {member}, one group of {GROUP}"] = dict(ms=ms, lo=ms, hi=ms)
                result[f"{projector}: composed path {strategy} / {member}, one group of {GROUP} (byte for byte equal)"] = dict(ms=seconds * 1e3, lo=seconds * 1e3, hi=seconds * 1e3)
        r.close()
    return result


def show(result):
    print(f"{N_REPLICAS} replicas x 256 start states x {STEPS} steps; ms per call, median of {ROUNDS} alternating rounds of {REPS} calls (min ... max)")
    for name, v in result.items():
        print(f"  {name:75s} {v['ms']:10.3f}   ({v['lo']:.3f} ... {v['hi']:.3f})")


def profile(out):
    os.makedirs(out, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "lspi_evaluate_sampled", "--", sys.executable,
                    os.path.abspath(__file__), "--json", "--no-composed"], check=True)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel statistics under {out}")
    print(f"{'kernel':110s} {'calls':>6s} {'mean us':>10s}")
    for x in csv.DictReader(open(files[0])):
        if "lspi_e" in x["Name"]:
            print(f"{x['Name'][:110]:110s} {int(x['Calls']):6d} {float(x['TotalDurationNs']) / 1e3 / int(x['Calls']):10.1f}")


if __name__ == "__main__":
    if "--profile" in sys.argv:
        profile(sys.argv[sys.argv.index("--profile") + 1])
    else:
        res = measure()
        print(json.dumps(res)) if "--json" in sys.argv else show(res)
