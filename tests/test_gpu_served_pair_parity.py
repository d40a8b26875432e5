"""The served pendulum pair (rollout_served_kernel + env_server_kernel) against the oracle, bit for bit, on a batch small enough to check
whole: 7 replicas -- a ragged second wave with one dead 16-lane group --, 12 trials in one launch (trial 11 is a test trial; every
learning trial ends with a flush of the register trace).  For every replica: the rows, the RNG positions, the environment state and
the weight of EVERY slot the oracle's run changed (not a sample of the table).

Why a module of its own.  The server's instruction stream is written for its length (grlx_env_server.h: constants made once, the
sine's sign set by an integer add, a flat command loop) and td_update_lane takes the forwarded weight of project(s, a) as the aliased
trace entry's (FORWARDED, grlx_update.h).  Both are claims that the bits do not change; these are the cases that would show it:
  * the specialised kernels with the server (the pair the benchmark runs),
  * the generic kernels with a 2048-slot memory, where most slots are shared between tilings: the cross-lane path of the update, and
    beside it the common path with aliases in nearly every step,
  * both again with GRLX_ENV_SERVER=0: the rollout wave integrates itself, with the code every other kernel shares.
Tolerance: 0 ulp.  The oracle's half is computed once per configuration and shared by all cases (clean and poisoned included)."""
import numpy as np
import pytest

from tests import configs
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

N, TRIALS, SEED0 = 7, 12, 701
MEMORY = {"specialised": 8388608, "generic_2048": 2048}
_oracle = {}


def assert_bit_equal(a, b, what):
    a = np.asarray(a, dtype=np.float64).view(np.uint64).ravel(); b = np.asarray(b, dtype=np.float64).view(np.uint64).ravel()
    assert a.shape == b.shape, f"{what}: {a.size} values against {b.size}"
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a[bad[0]]:#018x} vs {b[bad[0]]:#018x}"


def _pair(grlx, which):
    cfg, spec = configs.pendulum(grlx, N, agent=0, max_rows=TRIALS + 1)
    cfg.projector.memory = MEMORY[which]
    spec.projector.memory = MEMORY[which]
    spec.math = ob.MATH_PORTABLE
    return cfg, spec


def _want(spec, which, k):
    """the oracle's run of replica k: rows, streams, state, and (slot, weight) of every slot whose weight the run changed"""
    if (which, k) not in _oracle:
        e = ob.Experiment(spec, seed=SEED0 + k)
        before = e.all_weights()
        rows, _ = e.run(TRIALS)
        after = e.all_weights()
        slots = np.nonzero(before.view(np.uint64) != after.view(np.uint64))[0].astype(np.uint32)
        _oracle[(which, k)] = dict(rows=[(x.trial, x.steps, x.reward, x.time) for x in rows], rng=list(e.rng())[:3], state=np.array(e.state()),
                                   slots=slots, w=after[slots])
        e.close()
    return _oracle[(which, k)]


@pytest.mark.parametrize("server", ["server", "no_server"])
@pytest.mark.parametrize("which", ["specialised", "generic_2048"])
def test_every_touched_weight_equals_the_oracle(grlx, monkeypatch, which, server):
    if server == "no_server":
        monkeypatch.setenv("GRLX_ENV_SERVER", "0")
    cfg, spec = _pair(grlx, which)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + N))
    r.run(TRIALS)
    r.sync()                                                   # raises on any sticky status bit
    kernel, counts = r.last_kernel(), r.env_server_counts()
    what = f"{which}, {server}: kernel {kernel}, environment server {counts}"
    assert kernel == (2 if which == "specialised" else 1), what
    if server == "no_server":
        assert counts == (0, 0), what
    elif which == "specialised":
        assert counts == (N, 0), what                          # every replica served to the end of the launch, none fell back
    else:
        assert counts[0] + counts[1] == N and counts[0] > 0, what
    for k in range(N):
        want = _want(spec, which, k)
        t, s, rew = r.rows(k)
        assert len(want["rows"]) == r.replica_rows(k) and len(want["rows"]) >= 1, f"{what}: replica {k}: row count"
        assert list(t) == [x[0] for x in want["rows"]], f"{what}: replica {k}: trial column"
        assert list(s) == [x[1] for x in want["rows"]], f"{what}: replica {k}: steps column"
        assert_bit_equal(rew, [x[2] for x in want["rows"]], f"{what}: replica {k}: returns")
        assert_bit_equal(r.row_times(k, 0, len(want["rows"])), [x[3] for x in want["rows"]], f"{what}: replica {k}: episode times")
        assert list(r.rng(k))[:3] == want["rng"], f"{what}: replica {k}: RNG positions"
        assert_bit_equal(r.env_state(k), want["state"], f"{what}: replica {k}: environment state")
        assert want["slots"].size > (1000 if which == "specialised" else 500), f"{what}: replica {k}: the oracle touched {want['slots'].size} slots"
        assert_bit_equal(r.weights(k, want["slots"]), want["w"], f"{what}: replica {k}: weights of the {want['slots'].size} slots the oracle touched")
    r.close()
