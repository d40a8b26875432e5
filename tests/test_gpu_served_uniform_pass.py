"""The wave-uniform pass of rollout_served_kernel (grl_amd/csrc/grlx_rollout.h) against the oracle, bit for bit, and the count of the
passes taken in it (Runner.uniform_pass_counts: per replica, what its wave counted in the last launch).

The loop restates the pass of a learning episode for a full wave whose four replicas are all served, from the episode's third pass on;
everything else runs the general pass.  Without the count no test could tell that the loop ran at all, so every case asserts it in
closed form:
  * the first pass of an episode only acts, the second has no update pending, every later one -- one per environment step, the
    terminal one included -- qualifies: an episode of S steps counts S - 1 (99 for the pendulum's 100 steps, 6 for 7, 1 for 2, 0 for 1);
  * a test episode, a ragged wave (a dead 16-lane group), a wave that lost its server, a launch without the server count nothing.
Every run is compared with the oracle as tests/test_gpu_served_pair_parity.py does: rows, RNG positions, environment state and the weight
of EVERY slot the oracle's run changed.  Tolerance: 0 ulp.  The oracle's half is computed once per configuration and replica and shared by
all cases (clean and poisoned included).

A MIXED wave (the second half of this file).  GRLX_ENV_SERVER_TUNE bits 24-31 restrict the "server leaves" hook of bits 8-23 to some
replicas of every server block (bit 24 + q: replica q of the block), so that ONE 16-lane group of a rollout wave loses its server while
its neighbours stay served -- what a server that is alive but late does, made deterministic from the server's side alone.  Three layers
of grlx_rollout.h then run in a state the suite otherwise reaches only by accident of timing: mail_take_wave gives up and changes nothing;
the general pass takes the same step again with mail_take, which succeeds for the served groups and runs into its bound for one; env_step
integrates for that one group under a partial exec mask, and the wave stays mixed (`srv` true in some groups, false in others) for the
rest of the launch -- deferred update, sharing events and `risky` reloads included.  Every such case asserts oracle parity as above, the
per-replica flags (Runner.env_server_flags: 2 exactly for the replicas the mask names, 1 for the others) and the count in closed form:
the vote of mail_take_wave is the whole wave's, so ALL FOUR replicas of a wave stop counting where a whole-block quit would stop them.
Cases: masks x positions (only the reset answered / mid-episode / exactly a trial boundary / the third episode), each specialised
instantiation, the generic instantiation with a 2048-slot memory, a fallback inside a test episode, two launches, a ragged wave."""
import numpy as np
import pytest

from tests import configs
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

N, TRIALS, SEED0 = 8, 12, 701
TEST_INTERVAL = 10
_oracle = {}


def assert_bit_equal(a, b, what):
    a = np.asarray(a, dtype=np.float64).view(np.uint64).ravel(); b = np.asarray(b, dtype=np.float64).view(np.uint64).ravel()
    assert a.shape == b.shape, f"{what}: {a.size} values against {b.size}"
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a[bad[0]]:#018x} vs {b[bad[0]]:#018x}"


def _pair(grlx, n, memory=8388608, timeout=2.99, agent=0):
    cfg, spec = configs.pendulum(grlx, n, agent=agent, max_rows=TRIALS + 1, timeout=timeout)
    cfg.projector.memory = memory
    spec.projector.memory = memory
    spec.timeout = timeout
    spec.math = ob.MATH_PORTABLE
    return cfg, spec


def _want(spec, key, k):
    """the oracle's run of replica k: rows, streams, state, and (slot, weight) of every slot whose weight the run changed"""
    if (key, k) not in _oracle:
        e = ob.Experiment(spec, seed=SEED0 + k)
        before = e.all_weights()
        rows, _ = e.run(TRIALS)
        after = e.all_weights()
        slots = np.nonzero(before.view(np.uint64) != after.view(np.uint64))[0].astype(np.uint32)
        _oracle[(key, k)] = dict(rows=[(x.trial, x.steps, x.reward, x.time) for x in rows], rng=list(e.rng())[:3], state=np.array(e.state()),
                                 slots=slots, w=after[slots])
        e.close()
    return _oracle[(key, k)]


def _learning_trials(first, count):
    """of the trials first .. first + count - 1 of a run, those that are learning trials (online_learning.cpp:160)"""
    return sum(1 for tt in range(first, first + count) if tt % (TEST_INTERVAL + 1) != TEST_INTERVAL)


def _run_and_compare(grlx, n, memory=8388608, timeout=2.99, chunks=(TRIALS,), min_slots=1000, agent=0, with_flags=False):
    """run n replicas in launches of `chunks` trials, hold every replica to the oracle, return (runner's last kernel, server counts,
    uniform-pass counts of the last launch, steps of a learning episode as the oracle's rows give them, a description of the run) and,
    with_flags, the per-replica flags of the last launch (Runner.env_server_flags: 1 served to the end, 2 fell back)"""
    cfg, spec = _pair(grlx, n, memory, timeout, agent)
    r = grlx.Runner(cfg, np.arange(SEED0, SEED0 + n))
    for c in chunks:
        r.run(c)
    r.sync()                                                   # raises on any sticky status bit
    kernel, counts, uniform, flags = r.last_kernel(), r.env_server_counts(), r.uniform_pass_counts(), [int(f) for f in r.env_server_flags()]
    what = (f"{n} replicas, agent {agent}, memory {memory}, timeout {timeout}, launches {chunks}: kernel {kernel}, environment server {counts}, "
            f"flags {flags}, uniform passes {list(uniform)}")
    print(what)
    steps = None
    for k in range(n):
        want = _want(spec, (memory, timeout, agent), k)
        t, s, rew = r.rows(k)
        assert len(want["rows"]) == r.replica_rows(k) and len(want["rows"]) >= 1, f"{what}: replica {k}: row count"
        assert list(t) == [x[0] for x in want["rows"]], f"{what}: replica {k}: trial column"
        assert list(s) == [x[1] for x in want["rows"]], f"{what}: replica {k}: steps column"
        assert_bit_equal(rew, [x[2] for x in want["rows"]], f"{what}: replica {k}: returns")
        assert_bit_equal(r.row_times(k, 0, len(want["rows"])), [x[3] for x in want["rows"]], f"{what}: replica {k}: episode times")
        assert list(r.rng(k))[:3] == want["rng"], f"{what}: replica {k}: RNG positions"
        assert_bit_equal(r.env_state(k), want["state"], f"{what}: replica {k}: environment state")
        assert want["slots"].size > min_slots, f"{what}: replica {k}: the oracle touched {want['slots'].size} slots"
        assert_bit_equal(r.weights(k, want["slots"]), want["w"], f"{what}: replica {k}: weights of the {want['slots'].size} slots the oracle touched")
        # the row of the test trial (trial 11 of 12) reports the learning steps so far: 10 learning episodes of equal length
        per_episode = want["rows"][0][1] / TEST_INTERVAL
        assert per_episode == int(per_episode) and (steps is None or steps == per_episode), f"{what}: replica {k}: {want['rows'][0][1]} learning steps in {TEST_INTERVAL} episodes"
        steps = int(per_episode)
    r.close()
    return (kernel, counts, uniform, steps, what, flags) if with_flags else (kernel, counts, uniform, steps, what)


@pytest.mark.parametrize("which", ["specialised", "generic_2048"])
def test_two_full_waves_count_every_qualifying_pass(grlx, which):
    """8 replicas = two full waves, 12 trials in one launch: trial 11 is a test trial, so the loop is left and entered again.  The generic
    kernel with a 2048-slot memory shares nearly every slot between tilings: the update's general case, the sharing events and the
    `risky` reload run inside the loop."""
    memory = 8388608 if which == "specialised" else 2048
    kernel, counts, uniform, steps, what = _run_and_compare(grlx, N, memory=memory, min_slots=1000 if which == "specialised" else 500)
    assert kernel == (2 if which == "specialised" else 1), what
    assert steps == 100, what
    if which == "specialised":
        assert counts == (N, 0), what
    if counts == (N, 0):
        assert list(uniform) == [_learning_trials(0, TRIALS) * (steps - 1)] * N, what        # 11 learning episodes x 99
    else:   # (the small memory may make a wave late once; a wave that fell back stops counting, the other is unaffected)
        assert counts[0] + counts[1] == N and all(0 < u <= _learning_trials(0, TRIALS) * (steps - 1) for u in uniform), what


def test_a_ragged_wave_runs_the_general_pass(grlx):
    """7 replicas: the full wave counts the closed form, the ragged wave (one dead 16-lane group) nothing; same bits."""
    kernel, counts, uniform, steps, what = _run_and_compare(grlx, 7)
    assert kernel == 2 and counts == (7, 0), what
    assert list(uniform) == [_learning_trials(0, TRIALS) * (steps - 1)] * 4 + [0] * 3, what


def test_two_launches_equal_one(grlx):
    """the same 8 replicas as two launches of 6 trials: same bits as the single launch (the oracle's); the count is the last launch's."""
    kernel, counts, uniform, steps, what = _run_and_compare(grlx, N, chunks=(6, 6))
    assert kernel == 2 and counts == (N, 0), what
    assert list(uniform) == [_learning_trials(6, 6) * (steps - 1)] * N, what                # trials 7 .. 12: five learning episodes


@pytest.mark.parametrize("timeout,steps_want", [(0.2, 7), (0.05, 2), (0.02, 1)])
def test_short_episodes(grlx, timeout, steps_want):
    """Episodes of 7 steps: no pass ever evicts (the trace is cleared before it fills), the loop runs 6 passes per episode.  Episodes
    of 2 steps: exactly the terminal pass.  Episodes of 1 step: the loop never runs."""
    kernel, counts, uniform, steps, what = _run_and_compare(grlx, N, timeout=timeout, min_slots=15)      # (one step updates 16 slots)
    assert kernel == 1 and counts == (N, 0) and steps == steps_want, what
    assert list(uniform) == [_learning_trials(0, TRIALS) * (steps_want - 1)] * N, what


@pytest.mark.parametrize("quit_after", [37, 101, 250])
def test_a_server_that_leaves_in_mid_episode(grlx, monkeypatch, quit_after):
    """GRLX_ENV_SERVER_TUNE bits 8-23: the server leaves, unannounced, once it has answered that many commands of a replica.  The take
    runs into its bound INSIDE the loop, which is left with nothing changed; the general pass polls again and falls back.  Same bits as
    the oracle (so as GRLX_ENV_SERVER=0), and the count stops growing.  An episode of S steps sends S + 1 commands (its reset, then
    the action chosen in each of the passes 1 .. S; the terminal pass S + 1 sends none); its pass p takes the answer to the episode's
    command p - 1, and the passes 3 .. S + 1 count.  With Q commands answered, Q = whole * (S + 1) + rest, the whole episodes count
    S - 1 each and the broken one the passes 3 .. rest + 1."""
    monkeypatch.setenv("GRLX_ENV_SERVER_TUNE", str((quit_after << 8) | 3))
    kernel, counts, uniform, steps, what = _run_and_compare(grlx, N)
    assert kernel == 2 and counts == (0, N), what
    whole, rest = divmod(quit_after, steps + 1)
    assert list(uniform) == [whole * (steps - 1) + min(max(rest - 1, 0), steps - 1)] * N, what


def test_without_a_server(grlx, monkeypatch):
    """GRLX_ENV_SERVER_TUNE=64: the server's kernel is launched and leaves at once; every replica falls back at its first take (in the
    general pass: the second pass of the first episode) and the loop never runs."""
    monkeypatch.setenv("GRLX_ENV_SERVER_TUNE", "64")
    kernel, counts, uniform, steps, what = _run_and_compare(grlx, N)
    assert kernel == 2 and counts == (0, N), what
    assert list(uniform) == [0] * N, what


# ------------------------------------------------------------------------------------------------------------------------------------
# A mixed wave: the server leaves SOME replicas of every block (GRLX_ENV_SERVER_TUNE bits 24-31), the others are served to the end.

def _tune(mask, quit_after):
    return str((mask << 24) | (quit_after << 8) | 3)


def _flags_want(mask, n):
    """replica r is replica r % 4 of its server block: 2 (fell back) where the mask names it, 1 (served to the end) elsewhere"""
    return [2 if (mask >> (r % 4)) & 1 else 1 for r in range(n)]


def _count_want(quit_after, steps):
    """the passes a wave counts before the first take that the server does not answer (test_a_server_that_leaves_in_mid_episode): an
    episode of S steps sends S + 1 commands and counts its passes 3 .. S + 1; of a broken episode with `rest` commands answered, the
    passes 3 .. rest + 1.  Holds while all the commands answered belong to learning episodes."""
    whole, rest = divmod(quit_after, steps + 1)
    return whole * (steps - 1) + min(max(rest - 1, 0), steps - 1)


def _mixed(grlx, monkeypatch, mask, quit_after, n=N, **kw):
    monkeypatch.setenv("GRLX_ENV_SERVER_TUNE", _tune(mask, quit_after))
    kernel, counts, uniform, steps, what, flags = _run_and_compare(grlx, n, with_flags=True, **kw)
    what = f"mask {mask:#06b}, quit_after {quit_after}: {what}"
    assert steps == 100, what
    return kernel, counts, [int(u) for u in uniform], steps, what, flags


@pytest.mark.parametrize("mask,quit_after", [(0b0001, 1), (0b0001, 37), (0b0001, 101), (0b0001, 250),
                                             (0b1010, 1), (0b1010, 37), (0b1010, 101), (0b1010, 250),
                                             (0b0100, 37), (0b0100, 101), (0b0111, 1), (0b0111, 250)])
def test_some_replicas_of_a_wave_lose_their_server(grlx, monkeypatch, mask, quit_after):
    """One, two or three of the four 16-lane groups of each wave fall back -- at the first pass that would qualify for the loop (1: only
    the reset is answered), in mid-episode (37), exactly at a trial boundary (101: the second episode's reset is not answered; its second
    pass, a general one, falls back), in the third episode (250).  The served neighbours stay served to the end of the launch, through
    every later pass of the mixed wave, and the whole wave stops counting where the first group fell back."""
    kernel, counts, uniform, steps, what, flags = _mixed(grlx, monkeypatch, mask, quit_after)
    assert kernel == 2 and counts[0] > 0, what
    assert flags == _flags_want(mask, N), what
    assert counts == (flags.count(1), flags.count(2)), what
    assert uniform == [_count_want(quit_after, steps)] * N, what


@pytest.mark.parametrize("agent", [0, 1, 3])          # SARSA, Q, Expected SARSA: the three specialised instantiations
def test_a_mixed_wave_in_each_specialised_instantiation(grlx, monkeypatch, agent):
    kernel, counts, uniform, steps, what, flags = _mixed(grlx, monkeypatch, 0b0010, 37, agent=agent)
    assert kernel == 2 and counts[0] > 0, what
    assert flags == _flags_want(0b0010, N), what
    assert uniform == [_count_want(37, steps)] * N, what


def test_a_mixed_wave_in_the_generic_instantiation(grlx, monkeypatch):
    """The generic kernel with a 2048-slot memory (test_two_full_waves_count_every_qualifying_pass): sharing events, the update's general
    case and the `risky` reload run in a mixed wave.  That configuration tolerates a wave that is late on its own, so a replica the mask
    does not name may have fallen back too: the masked ones must have."""
    mask = 0b0101
    kernel, counts, uniform, steps, what, flags = _mixed(grlx, monkeypatch, mask, 37, memory=2048, min_slots=500)
    assert kernel == 1 and counts[0] > 0, what
    assert counts[0] + counts[1] == N and all(f in (1, 2) for f in flags), what
    assert all(flags[r] == 2 for r in range(N) if (mask >> (r % 4)) & 1), what


def test_a_fallback_inside_a_test_episode(grlx, monkeypatch):
    """Every episode, greedy ones included, sends S + 1 = 101 commands: the ten learning episodes before the test trial (trial index 10)
    send 1010, so command 1050 is the test episode's 40th and the general pass falls back with `test` set.  Test passes never count, and
    trial index 11 -- a learning trial again -- runs in a wave that is mixed by then: 10 x (S - 1) = 990 for every replica."""
    quit_after = TEST_INTERVAL * (100 + 1) + 40
    kernel, counts, uniform, steps, what, flags = _mixed(grlx, monkeypatch, 0b0001, quit_after)
    assert kernel == 2 and counts[0] > 0, what
    assert flags == _flags_want(0b0001, N), what
    assert uniform == [TEST_INTERVAL * (steps - 1)] * N, what


def test_a_mixed_wave_in_two_launches(grlx, monkeypatch):
    """Every launch counts its commands from 1 and clears the mailboxes: the second launch of 6 trials starts fully served and loses the
    same replicas again, in its first episode (trial index 6, a learning trial).  Flags and count are the last launch's; parity covers
    the whole run."""
    kernel, counts, uniform, steps, what, flags = _mixed(grlx, monkeypatch, 0b1000, 37, chunks=(6, 6))
    assert kernel == 2 and counts[0] > 0, what
    assert flags == _flags_want(0b1000, N), what
    assert uniform == [_count_want(37, steps)] * N, what


@pytest.mark.parametrize("mask,uniform_want", [(0b1000, [36] * 4 + [0] * 3), (0b0001, [36] * 4 + [0] * 3)])
def test_a_mixed_ragged_wave(grlx, monkeypatch, mask, uniform_want):
    """7 replicas.  0b1000: replica 3 falls back in the full wave; in the ragged wave the mask names only the dead group, which changes
    nothing -- its three replicas are served to the end (and a ragged wave never counts).  0b0001: replica 4 falls back in a wave that
    never enters the loop, so straight from the general pass."""
    kernel, counts, uniform, steps, what, flags = _mixed(grlx, monkeypatch, mask, 37, n=7)
    assert kernel == 2 and counts[0] > 0, what
    assert flags == _flags_want(mask, 7), what
    assert _count_want(37, steps) == 36 and uniform == uniform_want, what
