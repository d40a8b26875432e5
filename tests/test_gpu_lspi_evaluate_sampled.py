"""The LSPI context's sampled episodes (grlx_lspi_evaluate_sampled*, grlx_lspi_evaluate_ensemble_sampled*) against the plain Python loops of
tests/fqi_evaluate_sampled_ref.py over tests/test_gpu_lspi.py's Ref on the replicas' weights.  Everything is integer or S5 arithmetic or the
oracle's portable exponential, so every comparison is on bit patterns.

Contexts (tests/test_gpu_lspi_evaluate.py says why these): [3, 3, 3] after one batch of 5 with 65 replicas -- untouched features solve to
exact zeros, seed 4 ties at step 0 from (pi, 0, 0), and groups reach 65; [5, 4, 3] with five actions; Gauss with a box clipped on every
side, with more than 64 candidates per action (two rounds of compaction) and with a box of about one cell; and all-zero weights before any
batch, where every step ties over all actions and the draw decides every action."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import fqi_evaluate_sampled_ref as fsr
from tests import oracle_binding as ob
from tests.test_gpu_lspi import Ref, bits
from tests.test_gpu_lspi_evaluate import SHORT, STARTS

pytestmark = pytest.mark.gpu

CASES = {"tri27": dict(n=65, batches=1, steps=[3, 3, 3], projector="triangle", batch_size=5, iterations=1),
         "tri60-a5": dict(n=6, batches=1, steps=[5, 4, 3], projector="triangle", batch_size=64, iterations=3, action_steps=5),
         "gauss60": dict(n=6, batches=1, steps=[5, 4, 3], projector="gauss", batch_size=64, iterations=3),
         "gauss363": dict(n=6, batches=1, steps=[11, 11, 3], projector="gauss", batch_size=64, iterations=1),
         "gauss363-s05": dict(n=6, batches=1, steps=[11, 11, 3], projector="gauss", batch_size=64, iterations=1, sigma=0.5),
         "zero": dict(n=6, batches=0, steps=[3, 3, 3], projector="triangle", init_min=0.0, init_max=0.0),
         "gauss-f60-s2": dict(n=6, batches=1, steps=[5, 4, 3], projector="gauss", batch_size=64, iterations=3, sigma=2.0),       # a box wider than the grid
         "gauss-f363-c1e8": dict(n=6, batches=1, steps=[11, 11, 3], projector="gauss", batch_size=64, iterations=1, cutoff=1e-8),      # a radius of 4.3 cells
         # the capacity of the ensemble kernel's pair list at its bound.  lspi_ens_cap (grlx_lspi_evaluate_sampled.hip) by hand: the radius is
         # 3 sqrt(log 100) = 6.44 cells, ceil(2 * 6.44) + 3 = 16 candidates per dimension, more than the 8 the grid has, so cap = 8 * 8 * 8 = 512
         # = kLspiMaxF slots per action -- and a state whose position on each axis lies in [0.56, 6.44] cells, the middle action among them,
         # fills all 512
         "gauss-f512-s3": dict(n=6, batches=1, steps=[8, 8, 8], projector="gauss", batch_size=64, iterations=1, sigma=3.0)}
# seed 4's zeros; the far start's empty Gauss projection; all-zero weights
TIED = {"tri27", "gauss60", "gauss363", "gauss363-s05", "zero", "gauss-f60-s2", "gauss-f363-c1e8", "gauss-f512-s3"}
SAMPLERS = [("greedy", None), ("epsilon", 0.0), ("epsilon", 0.3), ("epsilon", 1.0)]
MAX_STEPS = 12
TAU = {"majority": 1.0, "rank": 2.0}                                 # draws leave the first maximum
MEMBERS = [("greedy", None), ("epsilon", 0.3), ("softmax", 1.0)]
LARGE = ((0, 65, 65), (0, 64, 64), (0, 17, 17), (0, 32, 16), (1, 3, 3), (3, 1, 1))      # (first replica, replicas, group size)


class Member:
    """what the reference loops ask of an experiment: .spec and .q(obs, a) -- Ref.read on one replica's weights, the projection of an
    (observation, action) pair formed once for all members"""

    def __init__(self, ref, w, spec, pairs):
        self.ref, self.w, self.spec, self.pairs = ref, w, spec, pairs

    def q(self, obs, a):
        key = (float(obs[0]), float(obs[1]), a)
        if key not in self.pairs:
            self.pairs[key] = self.ref.project(list(key))
        q = 0.0
        for i, wt in self.pairs[key]:
            q += float(self.w[i]) * wt
        return q


_made = {}


def context(grlx, name):
    """(runner, members per replica, what must not change); made once"""
    if name not in _made:
        case = dict(CASES[name])
        n, batches = case.pop("n"), case.pop("batches")
        cfg = grlx.pendulum_lspi_config(n, max_batches=1, **case)
        r = grlx.LspiRunner(cfg, list(range(1, n + 1)))
        for _ in range(batches):
            r.run_batch(); r.sync()
        base = ob.pendulum_sarsa_spec()
        base.action_steps = cfg.action_steps
        ref, pairs = Ref(cfg), {}
        spec = types.SimpleNamespace(base=base, gamma_tau=ref.gamma_tau)
        _made[name] = (r, [Member(ref, r.params(k), spec, pairs) for k in range(n)], frozen(r))
    return _made[name]


def frozen(r):
    n = r.cfg.n_replicas
    return b"".join(r.params(k, w).tobytes() for k in range(n) for w in (0, 1)) + b"".join(a.tobytes() for k in range(n) for a in r.rows(k, 1)) + \
        repr([r.info(k) for k in range(n)]).encode()


def compare(got, want, what):
    """got: a result of the runner; want: one reference dict per row (replica or group)"""
    fields = dict(zip(got._fields, got))               # a trajectory calls the episode's count n_explored: explored is its per-step view
    for f in want[0]:
        w = np.array([row[f] for row in want])
        if f == "records" and f not in fields:
            continue                                   # the sums alone: no records
        g = fields[f] if f in fields else fields["n_" + f]
        if w.dtype == np.uint64:
            assert (np.asarray(g) == w).all(), f"{what}: {f}"
        else:
            assert (bits(np.asarray(g, np.float64)) == bits(w.astype(np.float64))).all(), f"{what}: {f}\n{g}\nvs\n{w}"


@pytest.mark.parametrize("sampler,eps", SAMPLERS, ids=[f"{s}-{e}" for s, e in SAMPLERS])
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_policy(grlx, name, sampler, eps):
    r, members, was = context(grlx, name)
    code = fsr.sr.GREEDY if sampler == "greedy" else fsr.sr.EPSILON
    ties = explored = 0
    # nine starts with every record word, replicas 2 ... 4 (seed 4 is replica 3); 65 starts (a partial second block); one start
    for states, (first, count), traj in ((STARTS, (2, 3), True), (SHORT, (0, 1), False), (STARTS[:1], (3, 1), False)):
        streams = grlx.episode_streams(11 + len(states), count, len(states))
        want = [fsr.evaluate(members[first + k], states, code, eps or 0.0, streams[k], MAX_STEPS) for k in range(count)]
        what = f"{name} {sampler} {eps}: {len(states)} starts"
        if traj:
            got = r.evaluate_sampled_trajectory(states, MAX_STEPS, sampler, eps, streams, replicas=(first, count))
            assert got.records.shape[2:] == (MAX_STEPS, 12) == want[0]["records"].shape[1:]
        else:
            got = r.evaluate_sampled(states, sampler, eps, streams, replicas=(first, count), max_steps=MAX_STEPS)
        compare(got, want, what)
        ties, explored = ties + sum(w["ties"].sum() for w in want), explored + sum(w["explored"].sum() for w in want)
        if sampler == "greedy":
            # where nothing tied the call is the greedy one, and no stream moved
            clean = np.array([w["ties"] for w in want]) == 0
            plain = r.evaluate(states, replicas=(first, count), max_steps=MAX_STEPS)
            for f in ("ret", "disc", "steps", "terminal", "final_state"):
                assert (bits(getattr(got, f).astype(np.float64))[clean] == bits(getattr(plain, f).astype(np.float64))[clean]).all(), f"{what}: {f} against evaluate's"
            assert (got.streams[clean] == streams[clean]).all(), f"{what}: a stream moved without a tie"
    if sampler == "greedy":
        # no streams: a copy of the replica's global stream, which does not move
        word = np.array([[[0, r.info(3)["rng"][0]]] * 5], np.uint64)
        compare(r.evaluate_sampled(STARTS[:5], replicas=(3, 1), max_steps=MAX_STEPS), [fsr.evaluate(members[3], STARTS[:5], code, 0.0, word[0], MAX_STEPS)],
                f"{name}: streams=None")
        assert ties > 0 or name not in TIED, f"{name}: the reference never ties"
    assert explored > 0 or eps in (None, 0.0), f"{name}: the reference never explores at epsilon {eps}"
    assert eps != 1.0 or ties == 0
    assert frozen(r) == was, "a sampled evaluation changed the context"


@pytest.mark.parametrize("member,param", MEMBERS, ids=[m for m, _ in MEMBERS])
@pytest.mark.parametrize("strategy", sorted(TAU))
@pytest.mark.parametrize("name", sorted(CASES))
def test_ensembles(grlx, name, strategy, member, param):
    r, members, was = context(grlx, name)
    s_code, m_code = getattr(fsr.esr, strategy.upper()), getattr(fsr.esr, member.upper())
    states, explored = STARTS[:5], 0                   # five starts: a second, partial block of four waves
    for first, count, g in (LARGE if name == "tri27" else ((0, 6, 3), (0, 6, 6), (2, 2, 1))):
        groups = count // g
        streams = np.ascontiguousarray(grlx.episode_streams(5 + g, groups, len(states))[:, :, 1])
        want = [fsr.evaluate_ensemble(members[first + k * g:first + (k + 1) * g], states, s_code, TAU[strategy], m_code, param or 0.0, streams[k], MAX_STEPS)
                for k in range(groups)]
        what = f"{name} {strategy} {member}: {count} replicas from {first} in groups of {g}"
        got = r.evaluate_ensemble_sampled_trajectory(states, g, MAX_STEPS, strategy, TAU[strategy], member, param, streams, replicas=(first, count))
        assert got.records.shape[2:] == (MAX_STEPS, 15)
        compare(got, want, what)
        compare(r.evaluate_ensemble_sampled(states, g, strategy, TAU[strategy], member, param, streams, replicas=(first, count), max_steps=MAX_STEPS), want,
                what + ", the sums alone")
        explored += sum(w["explored"].sum() for w in want)
    # no streams: a copy of the global stream of the group's first replica
    word = np.array([[r.info(k)["rng"][0]] * len(states) for k in (0, 3)], np.uint64)
    compare(r.evaluate_ensemble_sampled(states, 3, strategy, TAU[strategy], member, param, replicas=(0, 6), max_steps=MAX_STEPS),
            [fsr.evaluate_ensemble(members[k:k + 3], states, s_code, TAU[strategy], m_code, param or 0.0, word[k // 3], MAX_STEPS) for k in (0, 3)],
            f"{name} {strategy} {member}: streams=None")
    assert explored > 0, f"{name} {strategy} {member}: the reference's draws never leave the first maximum"
    assert frozen(r) == was, "a sampled ensemble evaluation changed the context"


@pytest.mark.parametrize("name", ["tri60-a5", "gauss60"])
def test_a_softmax_member_drops_entries(grlx, name):
    """tau_m = 1e-6: an entry more than 1e-4 below the member's maximum is dropped from its distribution -- seen by the reference itself"""
    r, members, _ = context(grlx, name)
    streams = np.ascontiguousarray(grlx.episode_streams(3, 2, 5)[:, :, 1])
    for strategy in sorted(TAU):
        seen = {}
        want = [fsr.evaluate_ensemble(members[3 * k:3 * k + 3], STARTS[:5], getattr(fsr.esr, strategy.upper()), TAU[strategy], fsr.esr.SOFTMAX, 1e-6, streams[k],
                                      MAX_STEPS, seen) for k in range(2)]
        assert seen.get("dropped"), "the reference drops nothing"
        compare(r.evaluate_ensemble_sampled_trajectory(STARTS[:5], 3, MAX_STEPS, strategy, TAU[strategy], "softmax", 1e-6, streams), want, f"{name} {strategy}")


REFUSALS = [(dict(epsilon=-1.0), "GRLX_EPSILON_OWN"), (dict(sampler=1, streams=None), "streams is null under GRLX_SAMPLER_EPSILON_GREEDY"),
            (dict(word=1 << 48), "a rand48 state is below 2^48"), (dict(sampler=2), "unknown sampler 2"), (dict(strategy=2), "unknown strategy 2"),
            (dict(member=3), "unknown member sampler 3"), (dict(tau=0.0), "tau = 0"), (dict(member=2, param=-1.0), "tau_m = -1"),
            (dict(member=1, param=-1.0), "GRLX_EPSILON_OWN"), (dict(count=5), "n_replicas = 5 is not a multiple of group_size = 3")]


@pytest.mark.parametrize("over,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals_name_the_call_and_the_reason(grlx, over, word):
    """the four calls on sentinel-filled outputs: GRLX_ERR_INVALID, the entry point and the reason named, nothing written"""
    r, _, was = context(grlx, "zero")
    lib, a = grlx.capi.load(), dict(count=6, sampler=1, epsilon=0.1, strategy=0, tau=1.0, member=0, param=0.0, streams=True)
    a.update({k: v for k, v in over.items() if k in a})
    p = lambda x, t=C.c_double: x.ctypes.data_as(C.POINTER(t))
    for ensemble in (False, True):
        if not ensemble and not set(over) & {"epsilon", "sampler", "streams", "word"} or ensemble and not set(over) & {"strategy", "tau", "member", "count", "word"}:
            continue
        for trajectory in (False, True):
            streams = np.zeros((6, 9, 2), np.uint64)
            streams[0, 1, 1] = over.get("word", 0)         # row 1, word 1 of a policy's streams; row 3 of a group's
            f64, i32, i64 = [np.full((6, 9, 3), 7.0) for _ in range(3)], [np.full((6, 9), 7, np.int32) for _ in range(4)], [np.full((6, 9), 7, np.int64) for _ in range(2)]
            out, rec = np.full((6, 9, 2), 7, np.uint64), np.full((6, 9, 5, 15), 7.0)
            name = "grlx_lspi_evaluate" + ("_ensemble" if ensemble else "") + "_sampled" + ("_trajectory" if trajectory else "")
            args = [r._ctx, 0, a["count"]] + ([3, a["strategy"], a["tau"], a["member"], a["param"]] if ensemble else []) + [p(STARTS), 9, 5] + \
                ([] if ensemble else [a["sampler"], a["epsilon"]]) + [p(streams, C.c_uint64) if a["streams"] else None, p(f64[0]), p(f64[1])] + \
                [p(x, C.c_int32) for x in i32[:3]] + ([p(x, C.c_int64) for x in i64] if ensemble else []) + [p(i32[3], C.c_int32), p(f64[2]), p(out, C.c_uint64)] + \
                ([p(rec)] if trajectory else [])
            rc, said = getattr(lib, name)(*args), lib.grlx_last_error().decode()
            assert rc == grlx.capi.ERR_INVALID and said.startswith(name + ": ") and word in said, (name, said)
            assert all((x == 7).all() for x in f64 + i32 + i64 + [out, rec]), f"{name}, {word}: something was written"
    assert frozen(r) == was
