"""Least-squares policy iteration on the GPU (grlx_lspi_*) against plain numpy on the device's own stored transitions: the projection and
the read written as grl_amd/csrc/grlx_lspi.h specifies them (S3-S6, D2-D5), the oracle's pendulum step and orc_pexp.

Shapes: F = 27 (one full and one ragged 16-tile), 60, 108 and the reference's 363; batch sizes 5 (one full K-step of 4 and a ragged one),
64, and 257 = kLspiChunkMin + 1 (two blocks' partial tiles meet; three after the second batch); and the bounds: F = 64 (nothing padded),
F = 512 = kLspiMaxF, 4097 transitions (kLspiMaxSplits chunks, a ragged last one), Gauss weights between the cutoff and the prune of S6,
a Gauss box wider than the grid, five actions.  Every case runs two batches of two replicas with different seeds, so the second rebuild
runs over 2 x batch_size transitions from non-initial weights."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import lspi_solve_ref
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

# Seeds for which no step of test_the_row's loop ties in any case, found on the CPU with a numpy LSPI on transitions drawn as the device
# draws them (rand48 replay, the oracle's pendulum step): 1, 2, 3, 5 ... 9 all do.  Seed 4 does not: a basis function that no stored
# transition touches keeps A = 1e-5 I and b = 0, so its weight is exactly 0, and none of seed 4's first five transitions has an angle below
# pi -- at steps [3, 3, 3] the three nodes that the start observation (0, 0) reads stay untouched and step 0 is a tie of zeros.
# A row with a `seeds` entry runs on those instead: at F = 512 seed 3's first 64 transitions leave the start observation's nodes untouched
# under the first and the last action (step 0 reads 0, -22.8, 0); 1, 2, 5 ... 9 do not tie there.
SEEDS = [3, 5]
CASES = {"f27-tri-n5-it1": dict(steps=[3, 3, 3], projector="triangle", batch_size=5, iterations=1),
         "f60-tri-n64-it3": dict(steps=[5, 4, 3], projector="triangle", batch_size=64, iterations=3),
         "f60-gauss-n64-it3": dict(steps=[5, 4, 3], projector="gauss", batch_size=64, iterations=3),
         "f108-tri-n257-it1": dict(steps=[6, 6, 3], projector="triangle", batch_size=257, iterations=1),
         "f363-tri-n300-it3": dict(steps=[11, 11, 3], projector="triangle", batch_size=300, iterations=3),
         # the bounds of the accumulation and of the greedy choice
         "f64-tri-n64-it2": dict(steps=[4, 4, 4], projector="triangle", batch_size=64, iterations=2),                # F = Fp: no padding anywhere
         "f512-tri-n64-it1": dict(steps=[8, 8, 8], projector="triangle", batch_size=64, iterations=1, seeds=[5, 6]),             # kLspiMaxF: both LDS maxima, 1024 tiles, 32 panels
         "f27-tri-n4097-it1": dict(steps=[3, 3, 3], projector="triangle", batch_size=4097, iterations=1),            # kLspiMaxSplits chunks of 272, the last of 17 rows; then 16 of 528
         "f64-gauss-n64-it2-c1e8": dict(steps=[4, 4, 4], projector="gauss", batch_size=64, iterations=2, cutoff=1e-8),      # kept weights in (1e-8, 1e-5]: read, pruned from Phi and Psi
         "f27-gauss-n5-s2": dict(steps=[3, 3, 3], projector="gauss", batch_size=5, iterations=1, sigma=2.0),         # every function kept; the ragged tail of the f += 16 loop
         "f60-tri-n64-it3-a5": dict(steps=[5, 4, 3], projector="triangle", batch_size=64, iterations=3, action_steps=5)}    # a five-way greedy choice and action select
EPS = 2.0 ** -52
# both ends of each range, points outside them, a cell boundary and general points
GRID = np.array([[a, v] for a in (-0.5, 0.0, 1.0, math.pi, 2 * math.pi, 7.0) for v in (-40.0, -12 * math.pi, -3.3, 0.0, 12 * math.pi, 50.0)])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Ref:
    """the specification in numpy for one configuration"""

    def __init__(self, cfg):
        self.steps = [int(s) for s in cfg.steps]
        self.F = int(np.prod(self.steps))
        self.mn = [0.0, -12 * math.pi, cfg.action_min]
        mx = [2 * math.pi, 12 * math.pi, cfg.action_max]
        self.delta = [(mx[d] - self.mn[d]) / (float(self.steps[d]) - 1) for d in range(3)]
        self.stride = [1, self.steps[0], self.steps[0] * self.steps[1]]
        self.gauss = cfg.projector == 1
        self.sigmasq = cfg.sigma * cfg.sigma
        self.cut = -self.sigmasq * math.log(cfg.cutoff)
        self.actions = [cfg.action_min + (cfg.action_max - cfg.action_min) / (float(cfg.action_steps) - 1) * k for k in range(cfg.action_steps)]
        self.gamma_tau = math.pow(cfg.gamma, cfg.control_step)
        self.pexp = ob.load().orc_pexp

    def project(self, x):
        """the unpruned (index, weight) pairs in the projection's order"""
        if self.gauss:
            base = [(self.mn[d] - x[d]) / self.delta[d] for d in range(3)]
            out = []
            for f in range(self.F):
                k = [f % self.steps[0], f // self.steps[0] % self.steps[1], f // self.stride[2]]
                d = [base[i] + k[i] for i in range(3)]
                distsq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if distsq < self.cut:
                    out.append((f, self.pexp(-distsq / self.sigmasq)))
            return out
        index, dist = 0, []
        for d in range(3):
            gridpos = min(max((x[d] - self.mn[d]) / self.delta[d], 0.0), self.steps[d] - 1 - 1e-10)
            v = int(gridpos)
            index += v * self.stride[d]
            dist.append(gridpos - v)
        out = []
        for ii in range(8):
            w, diff = 1.0, 0
            for d in range(3):
                edge = (ii >> d) & 1
                diff += edge * self.stride[d]
                w *= dist[d] if edge else (1 - dist[d])
            out.append((index + diff, w))
        return out

    def read(self, w, x):
        q = 0.0
        for i, wt in self.project(x):
            q += float(w[i]) * wt
        return q

    def q(self, w, obs):
        return [self.read(w, [obs[0], obs[1], a]) for a in self.actions]

    def phi(self, x):
        v = np.zeros(self.F)
        for i, wt in self.project(x):
            if abs(wt) > 0.00001:
                v[i] = wt
        return v


_made = {}


def seeds_of(name):
    return CASES[name].get("seeds", SEEDS)


def case(grlx, name):
    """(reference, runner, snapshots after each of the two batches per replica); made once, never advanced again"""
    if name not in _made:
        cfg = grlx.pendulum_lspi_config(len(SEEDS), max_batches=2, **{k: v for k, v in CASES[name].items() if k != "seeds"})
        r = grlx.LspiRunner(cfg, seeds_of(name))
        ref = Ref(cfg)
        snaps = [[dict(w=r.params(k), q=r.query(GRID)[k]) for k in range(len(SEEDS))]]
        for _ in range(2):
            r.run_batch(); r.sync()
            snaps.append([dict(w=r.params(k), w_prev=r.params(k, 1), q=r.query(GRID)[k], tr=r.transitions(k), sys=r.system(k), info=r.info(k))
                          for k in range(len(SEEDS))])
        _made[name] = (ref, r, snaps)
    return _made[name]


def each(snaps, first=1):
    return [(b, k, s) for b in range(first, len(snaps)) for k, s in enumerate(snaps[b])]


@pytest.mark.parametrize("name", sorted(CASES))
def test_projection_and_read_bit_for_bit(grlx, name):
    ref, _, snaps = case(grlx, name)
    for b, k, s in each(snaps[:2], first=0):
        want = np.array([ref.q(s["w"], o) for o in GRID])
        bad = np.nonzero(bits(s["q"]) != bits(want))
        assert bad[0].size == 0, f"after {b} batches, replica {k}: {bad[0].size} reads differ, first at {GRID[bad[0][0]]}: {s['q'][bad][0]!r} vs {want[bad][0]!r}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_greedy_choice(grlx, name):
    ref, _, snaps = case(grlx, name)
    for b, k, s in each(snaps):
        _, nobs, _, best = s["tr"]
        assert len(best) == b * CASES[name]["batch_size"] == s["info"]["n"]
        for j, o in enumerate(nobs):
            q = ref.q(s["w_prev"], o)
            assert q[best[j]] == max(q), f"batch {b}, replica {k}, transition {j}: best = {best[j]}, reads {q}"
            if q.count(max(q)) == 1:
                assert best[j] == q.index(max(q))


_systems, _solves = {}, {}


def system_reference(ref, tr, key):
    """(A, b, their elementwise bounds) in longdouble from the transitions and `best`; made once per snapshot"""
    if key in _systems:
        return _systems[key]
    oa, nobs, rew, best = tr
    L = np.longdouble
    Phi = np.array([ref.phi(x) for x in oa])
    Psi = np.array([ref.gamma_tau * ref.phi([o[0], o[1], ref.actions[a]]) for o, a in zip(nobs, best)])
    I = 0.00001 * np.eye(ref.F)
    A = I.astype(L) + Phi.T.astype(L) @ Phi.astype(L) - Phi.T.astype(L) @ Psi.astype(L)
    b = Phi.T.astype(L) @ rew.astype(L)
    n = len(rew)
    tolA = (n + 2) * EPS * (np.abs(Phi).T @ np.abs(Phi) + np.abs(Phi).T @ np.abs(Psi) + I)
    tolb = (n + 2) * EPS * (np.abs(Phi).T @ np.abs(rew))
    _systems[key] = (A, b, tolA, tolb)
    return _systems[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_system(grlx, name):
    """A and b against longdouble sums within the bound of an n-term sum in any order; A bit-identical between two runs of one seed"""
    ref, r, snaps = case(grlx, name)
    for b_, k, s in each(snaps):
        A, b, tolA, tolb = system_reference(ref, s["tr"], (name, b_, k))
        gotA, gotb = s["sys"]
        errA, errb = np.abs(gotA.astype(np.longdouble) - A), np.abs(gotb.astype(np.longdouble) - b)
        print(f"{name} batch {b_} replica {k}: max |dA| / bound = {float(np.max(errA / np.maximum(tolA, 1e-300))):.3g}, max |db| / bound = {float(np.max(errb / np.maximum(tolb, 1e-300))):.3g}")
        assert (errA <= tolA).all(), f"batch {b_}, replica {k}: A misses its bound at {np.argwhere(errA > tolA)[:5].tolist()}"
        assert (errb <= tolb).all(), f"batch {b_}, replica {k}: b misses its bound at {np.argwhere(errb > tolb)[:5].tolist()}"
    again = grlx.LspiRunner(r.cfg, seeds_of(name))
    for b_ in (1, 2):
        again.run_batch(); again.sync()
        for k in range(len(SEEDS)):
            assert (bits(again.system(k)[0]) == bits(snaps[b_][k]["sys"][0])).all(), f"batch {b_}, replica {k}: A differs between two runs"
    again.close()


def test_the_small_cutoff_keeps_weights_that_s6_prunes(grlx):
    """what the c1e8 row is for: among each replica's stored transitions some unpruned projection weight lies in (cutoff, 1e-5] -- read
    by the greedy choice, dropped from Phi or Psi.  (Ref.project keeps distsq < -sigma^2 log(cutoff), i.e. weights above the cutoff.)"""
    name = "f64-gauss-n64-it2-c1e8"
    ref, r, snaps = case(grlx, name)
    for k, s in enumerate(snaps[2]):
        oa, nobs, _, best = s["tr"]
        for side, inputs in (("Phi", [list(x) for x in oa]), ("Psi", [[o[0], o[1], ref.actions[a]] for o, a in zip(nobs, best)])):
            small = sum(1 for x in inputs for _, wt in ref.project(x) if r.cfg.cutoff < wt <= 0.00001)
            assert small > 0, f"replica {k}: no weight of {side} in (cutoff, 1e-5]"


def backward_error(A, b, w):
    L = np.longdouble
    A, b, w = A.astype(L), b.astype(L), w.astype(L)
    return float(np.max(np.abs(b - A @ w)) / (np.max(np.sum(np.abs(A), axis=1)) * np.max(np.abs(w)) + np.max(np.abs(b))))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_solve(grlx, name):
    """normwise backward error of the device's weights on the device's own system: within 4 x numpy.linalg.solve's or F 2^-52"""
    ref, _, snaps = case(grlx, name)
    for b_, k, s in each(snaps):
        A, b = s["sys"]
        eta, eta_np = backward_error(A, b, s["w"]), backward_error(A, b, np.linalg.solve(A, b))
        print(f"{name} batch {b_} replica {k}: eta = {eta:.3e}, numpy's = {eta_np:.3e}")
        assert s["info"]["status"] == 0
        assert eta <= max(4 * eta_np, ref.F * EPS), f"batch {b_}, replica {k}: eta = {eta:.3e}, numpy's = {eta_np:.3e}"
        # and the elimination order restated (tests/lspi_solve_ref.py): the weights bit for bit
        if (name, b_, k) not in _solves:
            _solves[name, b_, k] = lspi_solve_ref.solve(A, b)
        want, _, flagged = _solves[name, b_, k]
        bad = np.nonzero(bits(s["w"]) != bits(want))[0]
        assert not flagged and bad.size == 0, f"batch {b_}, replica {k}: {bad.size} of {ref.F} weights differ from the restated order, first at {bad[:1]}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_row(grlx, name):
    """the return of each batch's row: a Python loop from (pi, 0, 0) on that batch's weights -- numpy reads, first maximum, the oracle's
    pendulum step.  Meaningful only if no step of the loop ties: asserted (see SEEDS)."""
    ref, r, snaps = case(grlx, name)
    lib, spec = ob.load(), ob.pendulum_sarsa_spec()
    for k in range(len(SEEDS)):
        batch, transitions, ret = r.rows(k, 2)
        assert list(batch) == [0, 1] and list(transitions) == [0, CASES[name]["batch_size"]]
        for b_ in (1, 2):
            x = np.array([math.pi, 0.0, 0.0])
            obs = (C.c_double * 2)()
            lib.orc_env_observe(C.byref(spec), (C.c_double * 3)(*x), obs)
            obs, total, term, steps = list(obs), 0.0, 0, 0
            while not term:
                q = ref.q(snaps[b_][k]["w"], obs)
                assert q.count(max(q)) == 1, f"batch {b_}, replica {k}, step {steps}: a tie {q}"
                x, o, rew, t = ob.env_step(spec, x, ref.actions[q.index(max(q))])
                obs, term, total, steps = list(o[0]), int(t[0]), total + float(rew[0]), steps + 1
            assert steps == 100 and bits(total) == bits(ret[b_ - 1]), f"batch {b_}, replica {k}: {total!r} vs {ret[b_ - 1]!r}"
        assert snaps[2][k]["info"]["ties"] == 0


@pytest.mark.parametrize("call,word", [
    (lambda r, c: r.params(2), "replica 2"), (lambda r, c: r.params(-1), "replica -1"), (lambda r, c: r.params(0, which=2), "which = 2"),
    (lambda r, c: c.check(r.lib.grlx_lspi_get_params(r._ctx, 0, 0, (C.c_double * 26)(), 26)), "n = 26"),
    (lambda r, c: r.rows(2, 1), "replica 2"), (lambda r, c: r.rows(0, 3), "rows [0, 3)"),
    (lambda r, c: r.transitions(2, 0, 1), "replica 2"), (lambda r, c: r.transitions(0, 8, 3), "transitions [8, 11)"),
    (lambda r, c: r.system(2), "replica 2"), (lambda r, c: r.info(-1), "replica -1"),
    (lambda r, c: r.query(GRID, replicas=(1, 2)), "replica range [1, 3)"), (lambda r, c: r.query([[math.nan, 0.0]]), "row 0, dimension 0")])
def test_replica_and_range_refusals(grlx, call, word):
    """the replica and range checks of the getters and the query, on a context of 2 replicas, 2 rows and a store of 10"""
    _, r, _ = case(grlx, "f27-tri-n5-it1")
    with pytest.raises(grlx.capi.GrlxError) as ei:
        call(r, grlx.capi)
    assert ei.value.code == grlx.capi.ERR_INVALID and word in str(ei.value), str(ei.value)
