#!/usr/bin/env python3
"""snapshot_throughput.py [--quick] -- what a snapshot costs: save time, load time and bytes of grlx_snapshot_save / _load for
  the headline batch (4096 pendulum SARSA replicas) after 100 and after 1000 trials, and
  16384 cart-pole actor-critic replicas after 32 trials,
against the naive snapshot timed in the same process on the same context: hipMemcpy of the context's own raw arrays (tables, target
values, states, rows, trace) to one fresh pageable host buffer and back (grlx_snapshot_naive_copy, include/grlx_diag.h).  Prints the
occupied fraction of the tables, on which the gain depends, and the device time of snapshot_pack_kernel / snapshot_unpack_kernel
(events around the launch: grlx_snapshot_timing) with the rate at which pack swept the tables' bucket lines.
Every workload runs in a child process of its own under a time limit (LIMIT seconds); the first one that fails or runs into it ends
the script: nothing more is started on a device that may be in trouble.  --quick: 256 / 1024 replicas."""
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMIT = 420


def measure(kind, n, trials):
    import numpy as np
    import grl_amd
    check = grl_amd.capi.check
    cfg = grl_amd.pendulum_sarsa_config(n, max_rows=256) if kind == "pendulum" else grl_amd.cart_pole_ac_config(n, max_rows=64)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    done = 0
    while done < trials:                     # launches of at most 32 trials with a sync between: the tables may grow
        c = min(32, trials - done)
        r.run(c); r.sync()
        done += c
    t0 = time.perf_counter(); size = r.snapshot_size(); t_size = time.perf_counter() - t0
    buf = (C.c_ubyte * size)()
    written = C.c_uint64(0)
    t0 = time.perf_counter()
    check(r.lib.grlx_snapshot_save(r._ctx, buf, size, C.byref(written)))
    t_save = time.perf_counter() - t0
    pack, unpack = C.c_double(-1), C.c_double(-1)
    check(r.lib.grlx_snapshot_timing(r._ctx, C.byref(pack), None))
    raw, out_ms, back_ms = C.c_uint64(0), C.c_double(0), C.c_double(0)
    rc = r.lib.grlx_snapshot_naive_copy(r._ctx, C.byref(raw), C.byref(out_ms), C.byref(back_ms))
    info = grl_amd.snapshot_info(bytes(memoryview(buf)[:4096]))
    logc, tables = info.table_log2, info.n_tables
    table_bytes = (n * tables * 16) << logc
    r.close()
    r2 = grl_amd.Runner(cfg, np.zeros(n, np.int64))
    t0 = time.perf_counter()
    check(r2.lib.grlx_snapshot_load(r2._ctx, buf, size))
    t_load = time.perf_counter() - t0
    check(r2.lib.grlx_snapshot_timing(r2._ctx, None, C.byref(unpack)))
    r2.close()
    occupied = info.n_records / float((n * tables) << logc)
    print(f"{kind}: {n} replicas, {trials} trials, tables 2^{logc} x {tables}, occupied {occupied * 100:.2f} %", flush=True)
    print(f"  snapshot {size / 2**20:10.1f} MiB   size query {t_size * 1e3:8.1f} ms   save {t_save * 1e3:9.1f} ms   load {t_load * 1e3:9.1f} ms", flush=True)
    if rc == 0:
        print(f"  raw      {raw.value / 2**20:10.1f} MiB   device->host {out_ms.value:9.1f} ms   host->device {back_ms.value:9.1f} ms   "
              f"(save / raw out = {t_save * 1e3 / out_ms.value:.3f}, load / raw back = {t_load * 1e3 / back_ms.value:.3f}, bytes {size / raw.value:.4f})", flush=True)
    else:
        print(f"  raw      baseline not taken: {r.lib.grlx_last_error().decode()}", flush=True)
    print(f"  pack kernel {pack.value:8.3f} ms: {table_bytes / 2**30:.2f} GiB of bucket lines swept = {table_bytes / (pack.value * 1e-3) / 1e12:.3f} TB/s "
          f"({table_bytes / 4 / (pack.value * 1e-3) / 1e12:.3f} TB/s of key quads asked for)   unpack kernel {unpack.value:8.3f} ms", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        measure(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
        return
    np_, nc = (256, 1024) if "--quick" in sys.argv else (4096, 16384)
    for kind, n, trials in (("pendulum", np_, 100), ("pendulum", np_, 1000), ("cart_pole_ac", nc, 32)):
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, str(n), str(trials)], timeout=LIMIT)
        except subprocess.TimeoutExpired:
            sys.exit(f"{kind} {n} x {trials}: no result within {LIMIT} s; nothing more is started")
        if res.returncode != 0:
            sys.exit(f"{kind} {n} x {trials}: exit status {res.returncode}; nothing more is started")


if __name__ == "__main__":
    main()
