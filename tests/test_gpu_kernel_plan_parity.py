"""What every launchable row of the kernel table computes: the cases of tests/kernel_plan_cases.py that a device launches (the cases of
tests/test_gpu_kernel_plan.py), each against one scalar oracle experiment per replica built from the same case (kernel_plan_cases.build_pair),
bit for bit.  Twelve trials in two launches, run(5) and run(7): one greedy test trial (test_interval = 10), the episode ends of the absorbing
tasks, and a launch boundary in the middle of learning (the persisted trace, the deferred update).  One full wave plus one replica: the ragged
last wave and the masked lanes of the wide layouts.  Tables start at the configuration's own capacity; an overflow fails the case.

Compared for every replica: rows (trial, steps, mean return, mean episode time), the four random streams, the environment state, 600 fixed
slots of every table (and of the target network, with its synchronisation count); for the last replica -- alone in the ragged wave -- every
table whole; over all replicas the step counts; for a tapped case the records of the tapped replica as far as tap_capacity reaches.  Before
any of it: the launch ran the row the case names, so these are the bits of that row.

The oracle's replicas of a case run in a thread pool; a case takes 0.1-0.4 s, except the five with a target network (target_interval = 5:
the oracle blends all 8 388 608 weights every five updates, as representation.h:284-296 does), which take 3-11 s in the pass that computes them.

The invariant (tests/test_kernel_plan_oracle.py holds its other half): a row of the kernel table has a launched case here, or a named reason."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import kernel_plan_cases as kc
from tests import oracle_binding as ob
from tests.test_gpu_generic_paths import assert_bit_equal
from tests.test_gpu_parity import _compare_taps

LAUNCHES = (5, 7)
TRIALS = sum(LAUNCHES)
SLOTS = np.random.default_rng(20).integers(0, 8388608, 600).astype(np.uint32)
TABLES = {"cart_pole_ac": 2, "pendulum_ac": 2, "pendulum_qv": 2, "acrobot_qv": 2}       # every other builder: 1


def _oracle_replica(spec, seed, n_tables, target, tap_cap, whole):
    """One replica of the oracle (its C calls release the GIL): everything the test compares, as plain values."""
    e = ob.Experiment(spec, seed=seed)
    try:
        rows, taps = e.run(TRIALS, tap_cap=tap_cap)
        st = e.stats()
        out = dict(trial=[x.trial for x in rows], steps=[x.steps for x in rows], reward=[x.reward for x in rows], time=[x.time for x in rows],
                   rng=[int(v) for v in e.rng()[:4]], state=e.state(), w=[e.weights(SLOTS, t) for t in range(n_tables)],
                   learn=int(st.learn_steps), test=int(st.test_steps), taps=taps)
        if target:
            out["target"] = e.weights(SLOTS, table=2)
            out["syncs"] = int(e.L.orc_target_syncs(e.h))
        if whole:
            out["whole"] = [e.all_weights(t) for t in range(n_tables)]
        return out
    finally:
        e.close()


_REFERENCE = {}     # case id -> the oracle's replicas: computed once, shared by the clean and the poisoned pass, never changed


def _specs(grlx, case, alphas):
    name, builder, n, over, flags = case[:5]
    spec = kc.build_pair(grlx, builder, n, over)[1]        # (with the library: a spec half may take the task's switches from its config half)
    spec.math = ob.MATH_PORTABLE
    specs = []
    for k in range(n):
        s = ob.Spec.from_buffer_copy(spec)
        if flags & kc.SWEEP:
            s.alpha = 0.1 + 0.01 * k
            assert s.alpha == alphas[k]
        specs.append(s)
    return specs


def _reference(grlx, case, alphas):
    """The oracle half of a case.  The dense tables of the last replica (64 MiB each) are not kept: a pass that finds them gone runs
    that one replica again -- except with a target network, whose oracle blends 8 388 608 weights at every synchronisation and takes
    seconds per replica: those five cases keep theirs."""
    name, builder, n, over = case[:4]
    n_tables, target, tap_cap = TABLES.get(builder, 1), over.get("target_interval", 0) > 0, over.get("tap_capacity", 0)
    specs = _specs(grlx, case, alphas)

    def one(k, whole=False):
        return _oracle_replica(specs[k], k + 1, n_tables, target, tap_cap if k == over.get("tap_replica", -1) else 0, whole)

    if name not in _REFERENCE:
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            ref = list(pool.map(lambda k: one(k, whole=(k == n - 1)), range(n)))
        whole = ref[-1]["whole"] if target else ref[-1].pop("whole")
        _REFERENCE[name] = ref
    else:
        ref = _REFERENCE[name]
        whole = ref[-1]["whole"] if target else one(n - 1, whole=True)["whole"]
    return ref, whole


@pytest.mark.gpu
@pytest.mark.parametrize("case", kc.LAUNCHED, ids=[c[0] for c in kc.LAUNCHED])
def test_launch_equals_the_oracle(grlx, oracle, monkeypatch, case):
    name, builder, n, over, flags, _, _, (rpw, rollout, server, variant) = case
    n_tables, target = TABLES.get(builder, 1), over.get("target_interval", 0) > 0
    cfg = kc.build(grlx, builder, n, over)
    cfg.max_rows = TRIALS + 1
    r, alphas = kc.open_runner(grlx, monkeypatch, case, cfg)
    try:
        for trials in LAUNCHES:
            r.run(trials)
        r.sync()                                                   # raises on any sticky status bit: a full table is a failure
        assert (r.replicas_per_wave(), r.last_kernel_name(), r.last_kernel()) == (rpw, rollout, variant)
        served, fell_back = r.env_server_counts()
        assert (served + fell_back > 0) == (server != "")
        if server != "":
            assert served > 0
        ref, whole = _reference(grlx, case, alphas)
        for t in range(n_tables):
            r.table_load(0, t)
        with pytest.raises(grlx.capi.GrlxError):                    # ... and no table beyond them
            r.table_load(0, n_tables)
        learn = test = 0
        for k, o in enumerate(ref):
            who = f"{name}: replica {k}"
            t, s, rew = r.rows(k)
            assert list(t) == o["trial"] and list(s) == o["steps"] and len(o["trial"]) > 0, f"{who}: trial and steps columns"
            assert_bit_equal(rew, o["reward"], f"{who}: returns")
            assert_bit_equal(r.row_times(k, 0, len(t)), o["time"], f"{who}: episode times")
            assert [int(v) for v in r.rng(k)[:4]] == o["rng"], f"{who}: random streams"
            assert_bit_equal(r.env_state(k), o["state"], f"{who}: environment state")
            for tb in range(n_tables):
                assert_bit_equal(r.weights(k, SLOTS, tb), o["w"][tb], f"{who}: table {tb}")
            if target:
                tw, syncs = r.target_weights(k, SLOTS)
                assert syncs == o["syncs"] and syncs > 0, f"{who}: synchronisations {syncs} vs {o['syncs']}"
                assert_bit_equal(tw, o["target"], f"{who}: target network")
            learn += o["learn"]
            test += o["test"]
        for tb in range(n_tables):
            assert_bit_equal(r.export_weights(n - 1, tb), whole[tb], f"{name}: the whole table {tb} of replica {n - 1}")
        assert r.step_counts() == (learn, test)
        if over.get("tap_capacity", 0) > 0:
            otaps, gtaps = ref[over["tap_replica"]]["taps"], r.taps()
            assert len(gtaps) == len(otaps) == over["tap_capacity"]
            A = 1 if cfg.agent == grlx.capi.AGENT_AC else cfg.action_steps
            for i, (gt, ot) in enumerate(zip(gtaps, otaps)):
                try:
                    if cfg.agent == grlx.capi.AGENT_QV:
                        assert list(gt.p_idx[16:32]) == list(ot.p_idx[16:32])
                    _compare_taps(gt, ot, A=A, D=r.obs_dims)
                except AssertionError as ex:
                    raise AssertionError(f"{name}: record {i}: {ex}")
    finally:
        r.close()
