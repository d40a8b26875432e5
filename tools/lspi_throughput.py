#!/usr/bin/env python3
"""lspi_throughput.py [--profile DIR] [replicas [batch_size [batches [projector]]]] -- what a batch of least-squares policy iteration costs
on the GPU: 16 replicas of the reference's cfg/pendulum/lspi_triangle.yaml (batch_size 10,000, 10 batches, 10 iterations, F = 363) by
default.

Without --profile: seconds per batch (a host clock around grlx_lspi_run_batch + grlx_lspi_sync, after a warm-up context of one small
batch), the transitions each rebuild ran over, and the f64 rate of the two products from the operations the algorithm needs
(2 n Fp^2 per product and replica over the tiles computed) -- an end-to-end figure of the batch, not a kernel's.

With --profile DIR: the same run as a fresh child process under `rocprofv3 --kernel-trace --stats` (a run of its own: tracing slows the
host), and the kernels' total and mean times per phase from its statistics.  Run it under a time limit of its own."""
import csv, glob, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PHASES = [("sampling", "lspi_generate_kernel"), ("A_s and b: accumulate", "lspi_accumulate_kernel<0>"), ("A_s and b: reduce", "lspi_reduce_kernel<0>"),
          ("greedy choice", "lspi_greedy_kernel"), ("Phi^T Psi: accumulate", "lspi_accumulate_kernel<1>"), ("Phi^T Psi: reduce", "lspi_reduce_kernel<1>"),
          ("solve", "lspi_solve_kernel"), ("test trial", "lspi_test_kernel")]


def run(n, batch_size, batches, projector):
    import numpy as np
    import grl_amd
    warm = grl_amd.LspiRunner(grl_amd.pendulum_lspi_config(n, projector, batch_size=512, max_batches=1, iterations=1), np.arange(1, n + 1))
    warm.run_batch(); warm.sync(); warm.close()
    cfg = grl_amd.pendulum_lspi_config(n, projector, batch_size=batch_size, max_batches=batches)
    r = grl_amd.LspiRunner(cfg, np.arange(1, n + 1))
    fp = (r.n_params + 15) // 16 * 16
    total = 0.0
    for b in range(batches):
        t0 = time.perf_counter()
        r.run_batch(); r.sync()
        dt = time.perf_counter() - t0
        total += dt
        stored = (b + 1) * batch_size
        flop = 2.0 * stored * fp * fp * n * (0.5 + cfg.iterations)       # the triangle of Phi^T Phi once, Phi^T Psi per iteration
        print(f"batch {b}: {stored:7d} transitions  {dt * 1e3:9.2f} ms  products {flop / dt / 1e12:6.2f} TFLOP/s (f64, over the batch's whole time)")
    print(f"{n} replicas x {batches} batches of {batch_size}: {total:.3f} s; last returns {[float(r.rows(k, batches)[2][-1]) for k in range(min(n, 4))]}")


def profile(out, args):
    os.makedirs(out, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "lspi", "--", sys.executable, os.path.abspath(__file__)] + args
    subprocess.run(cmd, check=True)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel statistics under {out}")
    rows = list(csv.DictReader(open(files[0])))
    print(f"{'phase':26s} {'calls':>7s} {'total ms':>10s} {'mean us':>10s} {'share':>7s}")
    for phase, kernel in PHASES:
        hit = [x for x in rows if kernel.replace("<", "<(int)") in x["Name"] or kernel in x["Name"]]
        calls = sum(int(x["Calls"]) for x in hit)
        ns = sum(float(x["TotalDurationNs"]) for x in hit)
        pct = sum(float(x["Percentage"]) for x in hit)
        print(f"{phase:26s} {calls:7d} {ns / 1e6:10.2f} {ns / 1e3 / max(calls, 1):10.1f} {pct:6.1f}%")


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == "--profile":
        return profile(argv[1], argv[2:])
    nums = [int(a) for a in argv[:3]]
    n = nums[0] if len(nums) > 0 else 16
    batch_size = nums[1] if len(nums) > 1 else 10000
    batches = nums[2] if len(nums) > 2 else 10
    run(n, batch_size, batches, argv[3] if len(argv) > 3 else "triangle")


if __name__ == "__main__":
    main()
