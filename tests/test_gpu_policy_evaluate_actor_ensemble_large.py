"""The actor ensemble's episodes (grlx_evaluate_actor_ensemble and its trajectory call) at the workload's group sizes: one context of 256
actor-critic replicas per graph, groups of 63 ... 256 members, against tests/policy_evaluate_actor_ensemble_ref.py on the bit patterns of
all eight outputs and of every record.  No tolerance anywhere.  What the sibling's groups of 1 ... 37 members leave unreached:

  data_center's alive mask of four 64-bit words: its initialisation at 63, 64 and 65 members (and one word later), members of the words
      1 ... 3, removals there, a word that empties while later words stay populated
  the shared-out part of binning and density: thread t serves member t, so above 64 members more than one wave writes sh_r
  four and more probe rounds per step (16 members a round): 64 is four full rounds, 65 a fifth with one member, 256 sixteen
  more than one group in a launch at a group size above 16, and first_replica != 0 there

Shapes: both projectors at 8192 slots, so the oracle can hold 256 dense tables; seeds SEED0 ...; max_steps 8; 6 learning trials; the 3
start states [0, 1, 6] of test_gpu_policy_evaluate.py for the sweep over the sizes, all 7 for the group of 256, which is also compared
before any launch.  Rules per size G: mean, binning with 64 bins, data_center keeping 2, G // 2 and G - 1, density with r = 0.05.  The
oracle's experiments are run once per graph and their tables kept; a group's reference is computed once (every GPU test runs clean and
with poisoned registers).  Every precondition is asserted on the REFERENCE's outputs before the Runner is created."""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_actor_ensemble_ref as ae
from tests import policy_evaluate_ref as ev
from tests import policy_trajectory_ref as tr
from tests.test_gpu_policy_evaluate import start_states
from tests.test_gpu_policy_evaluate_actor_ensemble import check, records_add_up, small_memory
from tests.test_gpu_policy_evaluate_noisy import make
from tests.test_gpu_policy_query import SEED0, same_bits

pytestmark = pytest.mark.gpu

N, TRIALS, MS, MEMORY = 256, 6, 8, 8192
GRAPHS = ["pendulum_ac", "ac_twin"]
SIZES = (63, 64, 65, 127, 128, 129, 192, 193, 255)          # and 256, a test of its own
THREE = (0, 1, 6)                                           # the start states of the sweep over the sizes
SEVEN = tuple(range(7))
_contexts, _wants = {}, {}


def rules(G):
    """(rule, bins or the members kept, r) of a group of G"""
    return (("mean", 10, 0.001), ("binning", 64, 0.001), ("data_center", 2, 0.001), ("data_center", G // 2, 0.001), ("data_center", G - 1, 0.001),
            ("density", 10, 0.05))


def context(grlx, graph):
    """(configuration, spec, seeds, the 7 start states, {trials: the 256 members' tables after that many trials}): the oracle's
    experiments are built and run once per graph, their dense tables copied"""
    if graph not in _contexts:
        cfg, spec = make(grlx, graph, N)
        states = start_states(graph, spec)
        small_memory(cfg, spec, MEMORY)
        seeds = np.arange(SEED0, SEED0 + N)
        exps = [ob.Experiment(spec, seed=int(seed)) for seed in seeds]
        tables = {0: [[t.copy() for t in ev.tables_of(e)] for e in exps]}
        for e in exps:
            e.run(TRIALS)
        tables[TRIALS] = [[t.copy() for t in ev.tables_of(e)] for e in exps]
        for e in exps:
            e.close()
        _contexts[graph] = (cfg, spec, seeds, states, tables)
    return _contexts[graph]


def reference(grlx, graph, members, case, which=THREE, trials=TRIALS):
    """the reference's dict of one group (members: a range of replica indices) under one case, computed once"""
    key = (graph, trials, members.start, members.stop, which, case)
    if key not in _wants:
        _, spec, _, states, tables = context(grlx, graph)
        rule, bins, r = case
        seen = {}
        _wants[key] = ae.evaluate([tables[trials][k] for k in members], spec, states[list(which)], rule, bins, r, MS, seen)
        _wants[key]["seen"] = seen
    return _wants[key]


def trained(grlx, graph):
    cfg, _, seeds, _, _ = context(grlx, graph)
    r = grlx.Runner(cfg, seeds)
    r.run(TRIALS); r.sync()
    return r


def both_calls(r, states, G, case, want, what, **kw):
    """the plain call and the trajectory call of one case against want[group]; the records' sums are the summary's"""
    rule, bins, rad = case
    check(r.evaluate_actor_ensemble(states, G, rule, bins, rad, max_steps=MS, **kw), want, what)
    t = r.evaluate_actor_ensemble_trajectory(states, G, MS, rule, bins, rad, **kw)
    check(t, want, what + ", trajectory", records=True)
    records_add_up(t, what)
    return t


def taken(w):
    """[start][step]: the steps of the reference's records that were taken"""
    return np.arange(w["records"].shape[1])[None, :] < w["steps"][:, None]


def differ(a, b):
    return any(a[f].tobytes() != b[f].tobytes() for f in ae.FIELDS + ("records",))


# ---- 1: one group of every size -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", SIZES)
@pytest.mark.parametrize("graph", GRAPHS)
def test_one_large_group(grlx, graph, G):
    """replicas 0 ... G - 1 as one group under the six cases, both calls; then what needs no further reference: data_center keeping G and
    G + 7 members is mean word for word (the serial alive-mean starts from the first member as mean does, nothing is removed: kept = G per
    step, index -1, n_max 1), and binning with one bin keeps every member"""
    _, spec, _, states, _ = context(grlx, graph)
    states = states[list(THREE)]
    members = range(G)
    want = [reference(grlx, graph, members, case) for case in rules(G)]
    one_bin = reference(grlx, graph, members, ("binning", 1, 0.001))
    mean = want[0]
    assert (one_bin["kept"] == G * one_bin["steps"].astype(np.int64)).all() and (mean["kept"] == one_bin["kept"]).all()
    assert any(differ(w, mean) for w in want[1:]), f"{graph}, {G} members: no rule parts from the mean"
    if G in (64, 65):                                           # the sizes are not interchangeable: one member more changes the episodes
        a, b = (reference(grlx, graph, range(g), rules(g)[0]) for g in (64, 65))
        assert differ(a, b), f"{graph}: the group of 65 gives the episodes of its first 64 members"
    r = trained(grlx, graph)
    for case, w in zip(rules(G), want):
        both_calls(r, states, G, case, [w], f"{graph}, one group of {G}, {case[0]}:{case[1]}", replicas=members)
    for K in (G, G + 7):
        t = both_calls(r, states, G, ("data_center", K, 0.001), [mean], f"{graph}, one group of {G}, data_center keeping {K} is the mean", replicas=members)
        live = np.arange(MS)[None, None, :] < t.steps[:, :, None]
        assert (t.kept[live] == G).all() and (t.action_index[live] == -1).all() and (t.n_max[live] == 1).all() and (t.ties == 0).all()
    t = both_calls(r, states, G, ("binning", 1, 0.001), [one_bin], f"{graph}, one group of {G}, one bin", replicas=members)
    assert (t.n_kept == G * t.steps).all()
    r.close()


# ---- 2: the largest group, all seven start states, before any launch and after the trials --------------------------------------------------
def removals(w, K):
    """data_center's removals of every step the reference took: lists of (the member removed, the first alive member then)"""
    return [ae.data_center(a, K)[3] for episode in w["actions"] for a in episode]


def large_group_branches(grlx, graph):
    """asserted on the REFERENCE's outputs after the trials, 256 members x 7 start states x 8 steps.  What holds for one graph alone says so:
    ac_twin has no member on the clip after 6 trials, the pendulum has members on both ends; ac_twin's data_center keeping 2 ties at no
    removal after the trials (the pendulum's does, up to 4 members at one removal), it ties before any launch, which is compared too."""
    _, spec, _, _, _ = context(grlx, graph)
    lo, hi = float(spec.action_min), float(spec.action_max)
    mean, binning, center, _, _, density = (reference(grlx, graph, range(N), case, SEVEN) for case in rules(N))
    quarters = {int(i) >> 6 for i in density["records"][..., tr.ACTION_INDEX][taken(density)]}
    assert quarters == {0, 1, 2, 3}, f"{graph}: density selects members of the index quarters {sorted(quarters)} alone"
    steps = removals(center, 2)
    assert {at >> 6 for step in steps for at, _ in step} == {0, 1, 2, 3}, f"{graph}: data_center never removes from some word of the mask"
    assert any(at != first for step in steps for at, first in step), f"{graph}: data_center removes the first alive member alone"
    tying = center if graph == "pendulum_ac" else reference(grlx, graph, range(N), rules(N)[2], SEVEN, 0)
    assert tying["records"][..., tr.N_MAX].max() > 1 and (tying["ties"] > 0).any(), f"{graph}: data_center never ties at a removal"
    emptied = 0
    for step in steps:
        left = [64] * 4
        for at, _ in step:
            left[at >> 6] -= 1
            emptied += 1 if left[at >> 6] == 0 and any(left[(at >> 6) + 1:]) else 0
    assert emptied > 0, f"{graph}: no word of the mask empties while a later word stays populated"
    assert binning["seen"]["occupied"] > 8 and (binning["ties"] > 0).any(), f"{graph}: binning occupies {binning['seen']['occupied']} bins, ties {binning['ties']}"
    for w, name in ((binning, "binning"), (center, "data_center")):
        assert (w["records"][..., tr.ACTION] != mean["records"][..., tr.ACTION])[taken(w) & taken(mean)].any(), f"{graph}: {name}'s actions are the mean's"
    if graph == "pendulum_ac":
        actions = np.array([a for episode in mean["actions"] for step in episode for a in step])
        assert (actions == hi).any() and (actions == lo).any(), f"{graph}: {(actions == hi).sum()} member-steps on action_max, {(actions == lo).sum()} on action_min"


@pytest.mark.parametrize("trials", (0, TRIALS))
@pytest.mark.parametrize("graph", GRAPHS)
def test_a_group_of_256(grlx, graph, trials):
    """all 256 replicas as one group from all 7 start states, before any launch (the drawn initial weights) and after the trials"""
    cfg, _, seeds, states, _ = context(grlx, graph)
    want = [reference(grlx, graph, range(N), case, SEVEN, trials) for case in rules(N)]
    if trials:
        large_group_branches(grlx, graph)
    r = grlx.Runner(cfg, seeds)
    if trials:
        r.run(trials); r.sync()
    for case, w in zip(rules(N), want):
        both_calls(r, states, N, case, [w], f"{graph}, one group of 256 after {trials} trials, {case[0]}:{case[1]}")
    r.close()


# ---- 3: several large groups in one launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first,count,G", [(0, 256, 128), (0, 256, 64), (64, 128, 64)])
@pytest.mark.parametrize("graph", GRAPHS)
def test_several_large_groups_in_one_launch(grlx, graph, first, count, G):
    """2 groups of 128 and 4 groups of 64 on all replicas; replicas 64 ... 191 as 2 groups of 64 (first_replica != 0 at a large group):
    every row is the reference's for that member list"""
    _, _, _, states, _ = context(grlx, graph)
    states = states[list(THREE)]
    groups = [range(first + g * G, first + (g + 1) * G) for g in range(count // G)]
    want = [[reference(grlx, graph, members, case) for members in groups] for case in rules(G)]
    assert all(differ(w[0], w[1]) for w in want), f"{graph}: two groups give the same episodes"
    r = trained(grlx, graph)
    for case, w in zip(rules(G), want):
        both_calls(r, states, G, case, w, f"{graph}, replicas {first} ... {first + count - 1} in groups of {G}, {case[0]}:{case[1]}", replicas=range(first, first + count))
    r.close()
