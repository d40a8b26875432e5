"""Sampled evaluation episodes, the parts that need no device: grlx_episode_streams against the oracle's generator (rand48_at runs on the
device: test_gpu_policy_evaluate_sampled.py holds that comparison), the new unit in the build lists, the binding's shapes, and the refusals of `grlxd -e`, which come before any device is looked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import policy_evaluate_sampled_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- grlx_episode_streams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 5, 71, 2 ** 31 + 3, -4])
def test_episode_streams_are_the_seeds_stream_at_multiples_of_two_to_the_twenty(grlx, seed):
    """stream k = 2 * pair + which is srand48(seed) after k * 2^20 draws: against orc_srand48 / orc_rand48_jump, and against the stream walked
    draw by draw for the first jump"""
    got = grlx.episode_streams(seed, 3, 5)
    assert got.shape == (3, 5, 2) and got.dtype == np.uint64 and (got < (1 << 48)).all()
    x0 = sref.seeded(seed)
    flat = got.reshape(-1)
    assert int(flat[0]) == x0
    for k in range(flat.size):
        assert int(flat[k]) == sref.jumped(x0, k * sref.TWO20), f"stream {k}"
    g = ob.Rand48(x0)
    for _ in range(sref.TWO20):
        ob.load().orc_lrand48(C.byref(g))
    assert int(flat[1]) == int(g.x), "2^20 draws, one by one"
    assert len(set(flat.tolist())) == flat.size
    # first_pair: the same streams from any offset, the 2^31-th pair included (k * 2^20 passes 2^51: the jump is taken modulo the period)
    same = grlx.episode_streams(seed, 2, 5, first_pair=5)
    assert (same == got[1:]).all()
    far = grlx.episode_streams(seed, 1, 2, first_pair=2 ** 31)
    assert int(far[0, 0, 0]) == sref.jumped(x0, (2 * 2 ** 31) * sref.TWO20) and int(far[0, 1, 1]) == sref.jumped(x0, (2 * (2 ** 31 + 1) + 1) * sref.TWO20)


def test_nothing_is_written_for_nothing_asked(grlx):
    lib = grlx.capi.load()
    out = np.full(8, 777, np.uint64)
    lib.grlx_episode_streams(3, 0, 0, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    lib.grlx_episode_streams(3, -1, 2, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    lib.grlx_episode_streams(3, 0, 2, None)
    assert (out == 777).all()


# ---- the build lists and the binding -------------------------------------------------------------------------------------------------
def test_the_unit_is_in_the_build_lists():
    from grl_amd import _build
    assert "grlx_evaluate_sampled.hip" in _build.SOURCES
    deps = _build.UNIT_DEPS["grlx_evaluate_sampled.hip"]
    src = open(os.path.join(_build.CSRC, "grlx_evaluate_sampled.hip")).read()
    for line in src.splitlines():
        if line.startswith('#include "'):
            assert line.split('"')[1] in deps, line
    assert "grlx_evaluate_sampled.h" in _build.UNIT_DEPS["grlx_api_read.cpp"]
    for f in deps:
        assert os.path.exists(os.path.join(_build.CSRC, f)), f
    # grlx_evaluate.hip is not touched by the feature: it neither includes nor is included by the new unit
    assert "sampled" not in open(os.path.join(_build.CSRC, "grlx_evaluate.hip")).read()


def test_the_binding_names_what_the_header_declares():
    import grl_amd
    from grl_amd import capi
    header = open(os.path.join(ROOT, "include", "grlx.h")).read()
    for name in ("grlx_evaluate_sampled", "grlx_sampled_trajectory_record_words", "grlx_evaluate_sampled_trajectory", "grlx_episode_streams"):
        assert name + "(" in header and name in capi._SIGS
    assert "GRLX_SAMPLER_GREEDY = 0, GRLX_SAMPLER_EPSILON_GREEDY = 1" in header and (capi.SAMPLER_GREEDY, capi.SAMPLER_EPSILON_GREEDY) == (0, 1)
    assert "#define GRLX_EPSILON_OWN (-1.0)" in header and capi.EPSILON_OWN == -1.0
    assert grl_amd.SampledEvaluation._fields == ("ret", "disc", "steps", "terminal", "ties", "explored", "final_state", "streams")
    assert grl_amd.SampledTrajectory._fields == ("ret", "disc", "steps", "terminal", "ties", "n_explored", "final_state", "streams", "records")
    for name in ("SampledEvaluation", "SampledTrajectory", "episode_streams"):
        assert name in grl_amd.__all__
    for name in ("evaluate_sampled", "evaluate_sampled_trajectory", "sampled_trajectory_record_words"):
        assert callable(getattr(grl_amd.Runner, name))


def test_the_views_of_a_sampled_trajectory():
    import grl_amd
    rec = np.arange(2 * 3 * 4 * 12, dtype=np.float64).reshape(2, 3, 4, 12)          # the pendulum's 11 words and the explored word
    t = grl_amd.SampledTrajectory(None, None, np.full((2, 3), 2, np.int32), None, None, None, np.zeros((2, 3, 3)), None, rec)
    assert t.obs.shape == (2, 3, 4, 2) and t.state.shape == (2, 3, 4, 3) and t.explored.shape == (2, 3, 4)
    assert t.obs[0, 1, 2, 0] == rec[0, 1, 2, 6] and t.state[0, 0, 0, 2] == rec[0, 0, 0, 10] and t.explored[1, 2, 3] == rec[1, 2, 3, 11]
    assert t.action_index[1, 0, 0] == rec[1, 0, 0, 3] and t.episode(1, 2).shape == (2, 12)
    with pytest.raises(ValueError):
        t.explored[0, 0, 0] = 1.0


# ---- grlxd -e: refused before any device is looked for -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def test_grlxd_usage_mentions_the_sampler(grlxd, tmp_path):
    res = subprocess.run([grlxd], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "[-e epsilon|own|greedy]" in res.stdout + res.stderr


@pytest.mark.parametrize("args,yaml,word", [
    (["-r", "4", "-e", "0.05"], "pendulum-sarsa-tc.yaml", "needs the start states of -E"),
    (["-r", "4", "-E", "states.txt", "-e", "1.5"], "pendulum-sarsa-tc.yaml", "neither a number in [0, 1] nor 'own'"),
    (["-r", "4", "-E", "states.txt", "-e", "-0.1"], "pendulum-sarsa-tc.yaml", "neither a number in [0, 1] nor 'own'"),
    (["-r", "4", "-E", "states.txt", "-e", "nan"], "pendulum-sarsa-tc.yaml", "neither a number in [0, 1] nor 'own'"),
    (["-r", "4", "-E", "states.txt", "-e", "softmax"], "pendulum-sarsa-tc.yaml", "neither a number in [0, 1] nor 'own'"),
    (["-r", "4", "-g", "2", "-E", "states.txt", "-e", "0.05"], "pendulum-sarsa-tc.yaml", "-g 2 is not built"),
    (["-r", "1", "-E", "states.txt", "-e", "own"], "pendulum-sarsa-tc.yaml", "divides by n - 1"),
    (["-r", "4", "-E", "states.txt", "-e", "greedy"], "pendulum-fqi-ann.yaml", "not for experiment/batch_learning"),
    (["-r", "4", "-E", "states5.txt", "-e", "0.05"], "cart_pole-ac-tc.yaml", "not built for the actor-critic agent"),
])
def test_grlxd_sampled_refusals_name_their_reason(grlxd, tmp_path, args, yaml, word):
    (tmp_path / "states.txt").write_text("# angle velocity time\n3.14159 0 0\n0 0 0   # upright\n\n1 -2 1.5\n")
    (tmp_path / "states5.txt").write_text("0 3.14159 0 0 0\n0.5 0 0 0 1.0\n")
    res = subprocess.run([grlxd, "-s", "1", "-q", "-t", "12"] + args + [os.path.join(GOLDEN, yaml)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    said = res.stderr + res.stdout
    assert res.returncode != 0 and word in said, said
    assert "-e" in said
    assert "no HIP device" not in said, "refused only after a device was looked for"
    assert not list(tmp_path.glob("*sampled*"))
