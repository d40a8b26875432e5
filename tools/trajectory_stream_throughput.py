#!/usr/bin/env python3
"""trajectory_stream_throughput.py [replicas [starts-per-side [trials [max-steps [ragged-replicas]]]]] -- grlx_evaluate_trajectory_stream
against grlx_evaluate_trajectory, its baseline, on pendulum SARSA replicas after `trials` trials from a grid of start states at time 0
(4096 replicas x 16 x 16 starts, 100 trials, max_steps 100 by default: 1 M episodes, about 9.2 GB of records), in one process on one
context, the legs alternated, each warmed up once, medians of five with min - max:
(a) grlx_evaluate_trajectory into arrays allocated once: seconds per call (call time);
(b) the stream with an empty sink: call time -- the library's whole work, nothing kept;
(c) the stream with a sink that copies every chunk into a preallocated [replica][start] array, which is (a)'s product: call time, and
    the array against (a)'s word for word;
(d) the kernels alone, by events around every chunk's launches (grlx_read_kernel_timing; (a)'s chunk is the zero fill of its records and
    its kernel, the stream's chunk is its kernel), under the default staging bound and under a bound that makes one chunk of the call;
(e) the ragged case: max_steps 400 on the same episodes of 100 steps, (a) against (b), on `ragged-replicas` replicas (a quarter of the
    replicas by default, so that (a)'s host array stays the size of the main legs').
The first streamed call is timed on its own: it allocates and page-locks the staging.  Where the host has less free memory than two
result arrays and the staging need, the replicas are halved until they fit, and the line that reports the shape says so.
Run it under a time limit of its own."""
import ctypes as C
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import grl_amd
from grl_amd import capi

RUNS = 5


def median(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return f"median {median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}"


def mem_available():
    try:
        for ln in open("/proc/meminfo"):
            if ln.startswith("MemAvailable:"):
                return int(ln.split()[1]) * 1024
    except OSError:
        pass
    return None


def kernel_ms(lib, call):
    ms, chunks = C.c_double(0), C.c_int(0)
    capi.check(lib.grlx_read_kernel_timing(1, None, None))
    call()
    capi.check(lib.grlx_read_kernel_timing(0, C.byref(ms), C.byref(chunks)))
    return ms.value, chunks.value


class Outputs:
    """the arrays of one call's result, allocated (and touched) once"""

    def __init__(self, n, ns, max_steps, words, S):
        self.ret, self.disc, self.fin = np.zeros((n, ns)), np.zeros((n, ns)), np.zeros((n, ns, S))
        self.steps, self.term, self.ties = np.zeros((n, ns), np.int32), np.zeros((n, ns), np.int32), np.zeros((n, ns), np.int32)
        self.records = np.zeros((n, ns, max_steps, words))

    def pointers(self):
        P = lambda a, t=C.c_double: a.ctypes.data_as(C.POINTER(t))
        return (P(self.ret), P(self.disc), P(self.steps, C.c_int32), P(self.term, C.c_int32), P(self.ties, C.c_int32), P(self.fin), P(self.records))

    def take(self, c):
        k, s0 = c.ret.shape[1], c.first_start
        self.ret[:, s0:s0 + k], self.disc[:, s0:s0 + k], self.fin[:, s0:s0 + k] = c.ret, c.disc, c.final_state
        self.steps[:, s0:s0 + k], self.term[:, s0:s0 + k], self.ties[:, s0:s0 + k] = c.steps, c.terminal, c.ties
        self.records[:, s0:s0 + k] = c.records

    def same(self, o):
        return all(a.tobytes() == b.tobytes() for a, b in ((self.ret, o.ret), (self.disc, o.disc), (self.fin, o.fin), (self.steps, o.steps),
                                                           (self.term, o.term), (self.ties, o.ties))) and np.array_equal(self.records.view(np.uint64), o.records.view(np.uint64))


def timed(legs, label, note=lambda leg, m: ""):
    wall = {leg: [] for leg in legs}
    for i in range(RUNS):
        for leg in legs:
            t0 = time.perf_counter()
            legs[leg]()
            wall[leg].append(time.perf_counter() - t0)
            print(f"{label} run {i}  {leg:12s} {wall[leg][-1]:9.4f} s/call", flush=True)
    for leg in legs:
        print(f"{label} {leg:12s} call time {spread(wall[leg])} s/call{note(leg, median(wall[leg]))}", flush=True)
    return wall


def main():
    args = [int(a) for a in sys.argv[1:]]
    n = args[0] if len(args) > 0 else 4096
    side = args[1] if len(args) > 1 else 16
    trials = args[2] if len(args) > 2 else 100
    max_steps = args[3] if len(args) > 3 else 100
    words, S, ns = 11, 3, side * side
    avail = mem_available()
    asked = n
    while avail is not None and n > 64 and 3.5 * n * ns * max_steps * words * 8 > avail:
        n //= 2
    n_ragged = args[4] if len(args) > 4 else max(n // 4, 1)
    cfg = grl_amd.pendulum_sarsa_config(n, max_rows=trials // 10 + 2)
    r = grl_amd.Runner(cfg, np.arange(1, n + 1))
    lib = r.lib
    r.run(trials); r.sync()
    grid = grl_amd.observation_grid([-np.pi, -12 * np.pi], [np.pi, 12 * np.pi], [side, side])
    states = np.ascontiguousarray(np.concatenate([grid, np.zeros((grid.shape[0], 1))], axis=1))    # time 0: full episodes
    assert r.trajectory_record_words() == words and r.state_dims == S
    PS = states.ctypes.data_as(C.POINTER(C.c_double))
    whole, streamed = Outputs(n, ns, max_steps, words, S), Outputs(n, ns, max_steps, words, S)
    print(f"{n} replicas{'' if n == asked else f' ({asked} asked for; host memory available: {avail / 1e9:.1f} GB)'} x {ns} starts, max_steps {max_steps}, "
          f"record of {words} doubles: {whole.records.nbytes / 1e9:.3f} GB of records per call", flush=True)

    empty = capi.TRAJECTORY_SINK(lambda user, chunk: 0)
    chunks_seen = []

    def stream_empty(ms=max_steps, count=n):
        capi.check(lib.grlx_evaluate_trajectory_stream(r._ctx, 0, count, PS, ns, ms, empty, None))

    def keep(c):
        chunks_seen.append(c.ret.shape[1])
        streamed.take(c)

    def stream_copy():
        chunks_seen.clear()
        r.evaluate_trajectory_stream(states, max_steps, keep)

    def parent(ms=max_steps, count=n, out=whole):
        capi.check(lib.grlx_evaluate_trajectory(r._ctx, 0, count, PS, ns, ms, *out.pointers()))

    t0 = time.perf_counter()
    stream_empty()
    print(f"the first streamed call, which allocates and page-locks the staging: {time.perf_counter() - t0:.4f} s (call time)", flush=True)
    legs = {"(a) parent": parent, "(b) empty": stream_empty, "(c) copy": stream_copy}
    for leg in legs:                                                         # warm-up at the timed shape
        legs[leg]()
    pair_steps = int(whole.steps.sum())
    assert 1 <= whole.steps.min() and whole.steps.max() <= max_steps
    nbytes = whole.records.nbytes + sum(a.nbytes for a in (whole.ret, whole.disc, whole.fin, whole.steps, whole.term, whole.ties))
    print(f"{pair_steps} pair-steps; {len(chunks_seen)} streamed chunks of {max(chunks_seen)} start states ({nbytes / 1e9:.3f} GB over the host link per call)", flush=True)
    wall = timed(legs, "(a-c)", lambda leg, m: f"  {nbytes / m / 1e9:.2f} GB/s (bytes over the host link over call time)")
    a, b, c = (wall[k] for k in legs)
    print(f"(b) - (a) at the medians: {median(b) - median(a):+.4f} s; (a)'s own min - max spread: {max(a) - min(a):.4f} s; (b) / (a) = {median(b) / median(a):.3f}; "
          f"(c) / (a) = {median(c) / median(a):.3f}", flush=True)
    assert streamed.same(whole), "the streamed chunks, assembled, differ from grlx_evaluate_trajectory's arrays"
    print(f"(c) the assembled chunks equal (a)'s arrays word for word ({whole.records.size} record words, the sums and the final states)", flush=True)

    # (d) the kernels alone
    for bound, name in ((0, "default staging bound"), (2 * nbytes + 2 * states.nbytes + (1 << 20), "one chunk")):
        capi.check(lib.grlx_set_query_chunk_bytes(bound))
        try:
            dev = {"(a) parent": [], "(b) empty": []}
            n_chunks = {}
            for leg in dev:                                                  # warm-up under this bound (the one-chunk bound grows the staging)
                legs[leg]()
            for i in range(RUNS):
                for leg in dev:
                    ms, n_chunks[leg] = kernel_ms(lib, legs[leg])
                    dev[leg].append(ms)
        finally:
            capi.check(lib.grlx_set_query_chunk_bytes(0))
        for leg in dev:
            print(f"(d) {name}: {leg:12s} kernel time {spread(dev[leg])} ms in {n_chunks[leg]} chunk(s)  {pair_steps / median(dev[leg]) / 1e6:9.3f} G pair-steps/s", flush=True)
        print(f"(d) {name}: stream / parent kernel time at the medians: {median(dev['(b) empty']) / median(dev['(a) parent']):.3f}", flush=True)

    # (e) the ragged case: four times the records, the same steps
    del streamed
    ragged_steps = 4 * max_steps
    out_r = whole if n_ragged * ragged_steps <= n * max_steps else Outputs(n_ragged, ns, ragged_steps, words, S)
    view = Outputs.__new__(Outputs)                                          # (a)'s arrays cut for n_ragged replicas x ragged_steps records
    for name in ("ret", "disc", "fin", "steps", "term", "ties"):
        setattr(view, name, np.ascontiguousarray(getattr(out_r, name)[:n_ragged]))
    view.records = out_r.records.reshape(-1)[:n_ragged * ns * ragged_steps * words].reshape(n_ragged, ns, ragged_steps, words)
    legs_e = {"(a) parent": lambda: parent(ragged_steps, n_ragged, view), "(b) empty": lambda: stream_empty(ragged_steps, n_ragged)}
    for leg in legs_e:
        legs_e[leg]()
    taken = int(view.steps.sum())
    print(f"(e) {n_ragged} replicas x {ns} starts, max_steps {ragged_steps}: {view.records.nbytes / 1e9:.3f} GB of records per call, {taken} pair-steps "
          f"({100.0 * taken / (n_ragged * ns * ragged_steps):.1f} % of the records are steps taken)", flush=True)
    wall = timed(legs_e, "(e)", lambda leg, m: f"  {view.records.nbytes / m / 1e9:.2f} GB/s (record bytes over call time)")
    print(f"(e) (b) / (a) at the medians = {median(wall['(b) empty']) / median(wall['(a) parent']):.3f}", flush=True)
    dev = {leg: [kernel_ms(lib, legs_e[leg])[0] for _ in range(3)] for leg in legs_e}
    for leg in dev:
        print(f"(e) {leg:12s} kernel time {spread(dev[leg])} ms (three runs)", flush=True)
    behind = view.records[:, :, max_steps:]
    assert not behind.view(np.uint64).any(), "(e): a record behind an episode's end is not all-zero bits"
    r.close()


if __name__ == "__main__":
    main()
