"""The oracle's branches without a trace (oracle/experiment.c: `if (s->trace != ORC_TRACE_NONE)` in the SARSA, Expected SARSA, Q,
advantage, TD-critic and QV predictors, each beside the reference lines it restates) are what tests/test_gpu_no_trace.py measures
every kernel family against; no golden file of the reference pins them.  Here, on the CPU:

  * without a trace the predictor's whole update is the one write of project(s, a): a closed-form count of weight updates with no
    trace term, and no trace entry ever;
  * the field reaches the predictor: the rows differ from those of the same seed with a trace;
  * the inputs of the GPU tests meet the hazard they are there for.  In the deferred-update ordering a lane holds the weights of
    Q(s', .) before the previous step's update stores the weight of project(s, a); the slot just stored is among those already loaded
    when consecutive steps update the same slot of a tiling.  The share of such learning steps is measured on the graphs the GPU tests
    run, so that a later change of a config builder cannot quietly make them miss it."""
import pytest

from tests import configs
from tests import oracle_binding as ob


def _no_trace(spec):
    spec.trace = 0
    spec.math = ob.MATH_PORTABLE
    return spec


def test_update_count_has_no_trace_term():
    """12 trials of pendulum SARSA: 11 learning trials of 100 steps and one test trial.  lin_write -> lin_update counts one
    read-modify-write per valid index of project(s, a): 16 tilings, once per learning step; with a trace lin_update_trace would add
    one per live trace slot on top of that."""
    e = ob.Experiment(_no_trace(ob.pendulum_sarsa_spec()), seed=7)
    e.run(12)
    st = e.stats()
    assert st.learn_steps == 1100 and st.test_steps == 100
    assert st.trace_entries_sum == 0
    assert st.weight_rmws == 16 * st.learn_steps
    e.close()
    t = ob.Experiment(ob.pendulum_sarsa_spec(), seed=7)
    t.run(12)
    assert t.stats().trace_entries_sum > 0 and t.stats().weight_rmws > 16 * t.stats().learn_steps
    t.close()


def test_the_field_reaches_the_predictor():
    rows = []
    for trace in (0, 1):
        e = ob.Experiment(ob.pendulum_sarsa_spec(trace=trace), seed=7)
        rows.append([(x.trial, x.steps, x.reward) for x in e.run(12)[0]])
        e.close()
    assert len(rows[0]) == len(rows[1]) == 1
    assert rows[0] != rows[1]


GRAPHS = {
    "pendulum_sarsa": lambda: configs.pendulum(None, 1, agent=0)[1],
    "pendulum_q": lambda: configs.pendulum(None, 1, agent=1)[1],
    "pendulum_qv": lambda: configs.pendulum_qv(None, 1)[1],
    "acrobot_q": lambda: configs.acrobot(None, 1, agent=1)[1],
    "walker_q": lambda: configs.compass_walker(None, 1, agent=1)[1],
    "cart_pole_q": lambda: configs.cart_pole_q(None, 1, agent=1)[1],
    "cart_pole_ac": lambda: configs.cart_pole_ac(None, 1)[1],
}


def hazard_share(spec, seed, trials, cap=12000):
    """(learning steps with an update, those of them in which at least one tiling updates the slot it updated in the step before) over
    the oracle's per-step records: p_idx[:16] is project(s, a) of the update made at that step (the critic's projection for the
    actor-critic, the Q table's for QV)"""
    e = ob.Experiment(spec, seed=seed)
    _, taps = e.run(trials, tap_cap=cap)
    e.close()
    assert 0 < len(taps) < cap
    steps = repeated = 0
    prev = None
    for t in taps:
        if t.test:
            prev = None
            continue
        p = list(t.p_idx[:16])
        steps += 1
        if prev is not None and any(a == b for a, b in zip(p, prev)):
            repeated += 1
        prev = None if t.terminal else p                      # the next record starts another episode
    return steps, repeated


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_the_gpu_tests_inputs_meet_the_hazard(graph):
    """22 trials from seed 301 (the first replica of most GPU cases).  Measured when this test was written: pendulum 24-25 %, acrobot
    86 %, walker 18 %, cart-pole Q 19 %, cart-pole actor-critic 71 %; the bar is 10 %: hundreds of occurrences per replica."""
    steps, repeated = hazard_share(_no_trace(GRAPHS[graph]()), 301, 22)
    print(f"{graph}: {steps} learning steps, {repeated} repeat a slot of the step before ({100.0 * repeated / steps:.1f} %)")
    assert steps >= 400
    assert repeated >= 0.10 * steps, (graph, steps, repeated)
