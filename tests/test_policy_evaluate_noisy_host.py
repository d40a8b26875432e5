"""Noisy evaluation episodes of the actor-critic, the parts that need no device: grlx_episode_stream_words against the oracle's generator,
the new unit in the build lists, the binding's shapes, the views of a NoisyTrajectory, and the refusals of `grlxd -N`, which come before any
device is looked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import policy_evaluate_noisy_ref as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- grlx_episode_stream_words -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 5, 71, 2 ** 31 + 3, -4])
def test_episode_stream_words_are_the_even_streams(grlx, seed):
    """the stream of pair p is srand48(seed) after 2 * p * 2^20 draws (orc_srand48 / orc_rand48_jump): the even streams of episode_streams"""
    got = grlx.episode_stream_words(seed, 3, 5)
    assert got.shape == (3, 5) and got.dtype == np.uint64 and (got < (1 << 48)).all()
    x0 = nref.seeded(seed)
    flat = got.reshape(-1)
    assert int(flat[0]) == x0
    for p in range(flat.size):
        assert int(flat[p]) == nref.jumped(x0, 2 * p * nref.TWO20), f"pair {p}"
    assert (got == grlx.episode_streams(seed, 3, 5)[..., 0]).all()
    assert (got == nref.episode_stream_words(seed, 3, 5)).all()
    assert len(set(flat.tolist())) == flat.size
    same = grlx.episode_stream_words(seed, 2, 5, first_pair=5)
    assert (same == got[1:]).all()
    far = grlx.episode_stream_words(seed, 1, 2, first_pair=2 ** 31)
    assert int(far[0, 1]) == nref.jumped(x0, 2 * (2 ** 31 + 1) * nref.TWO20)


def test_nothing_is_written_for_nothing_asked(grlx):
    lib = grlx.capi.load()
    out = np.full(8, 777, np.uint64)
    lib.grlx_episode_stream_words(3, 0, 0, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    lib.grlx_episode_stream_words(3, -1, 2, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    lib.grlx_episode_stream_words(3, 0, 2, None)
    assert (out == 777).all()


# ---- the build lists and the binding -------------------------------------------------------------------------------------------------
def test_the_unit_is_in_the_build_lists():
    from grl_amd import _build
    assert "grlx_evaluate_noisy.hip" in _build.SOURCES
    deps = _build.UNIT_DEPS["grlx_evaluate_noisy.hip"]
    src = open(os.path.join(_build.CSRC, "grlx_evaluate_noisy.hip")).read()
    for line in src.splitlines():
        if line.startswith('#include "'):
            assert line.split('"')[1] in deps, line
    assert "grlx_evaluate_noisy.h" in _build.UNIT_DEPS["grlx_api_read.cpp"] and "grlx_evaluate_noisy.h" in _build.API_DEPS
    for f in deps:
        assert os.path.exists(os.path.join(_build.CSRC, f)), f
    # the siblings and the rollout kernels are not touched by the feature: none of them includes the new unit's header
    for name in ("grlx_evaluate.hip", "grlx_evaluate_sampled.hip", "grlx_kernels.hip", "grlx_rollout_ac.h", "grlx_step.h"):
        assert "noisy" not in open(os.path.join(_build.CSRC, name)).read(), name


def test_the_binding_names_what_the_header_declares():
    import grl_amd
    from grl_amd import capi
    header = open(os.path.join(ROOT, "include", "grlx.h")).read()
    for name in ("grlx_evaluate_noisy", "grlx_noisy_trajectory_record_words", "grlx_evaluate_noisy_trajectory", "grlx_episode_stream_words"):
        assert name + "(" in header and name in capi._SIGS and name in capi._NEWER_SIGS
    assert "#define GRLX_SIGMA_OWN (-1.0)" in header and capi.SIGMA_OWN == -1.0
    assert "#define GRLX_THETA_OWN (-1.0)" in header and capi.THETA_OWN == -1.0
    assert len(capi._SIGS["grlx_evaluate_noisy"][1]) == 18 and len(capi._SIGS["grlx_evaluate_noisy_trajectory"][1]) == 19
    assert grl_amd.NoisyEvaluation._fields == ("ret", "disc", "steps", "terminal", "clipped", "final_state", "streams", "noise")
    assert grl_amd.NoisyTrajectory._fields == ("ret", "disc", "steps", "terminal", "n_clipped", "final_state", "streams", "final_noise", "records")
    for name in ("NoisyEvaluation", "NoisyTrajectory", "episode_stream_words"):
        assert name in grl_amd.__all__
    for name in ("evaluate_noisy", "evaluate_noisy_trajectory", "noisy_trajectory_record_words"):
        assert callable(getattr(grl_amd.Runner, name))


def test_the_views_of_a_noisy_trajectory():
    import grl_amd
    rec = np.arange(2 * 3 * 4 * 17, dtype=np.float64).reshape(2, 3, 4, 17)          # the cart-pole's 15 words, the noise state and the clip flag
    t = grl_amd.NoisyTrajectory(None, None, np.full((2, 3), 2, np.int32), None, None, np.zeros((2, 3, 5)), None, None, rec)
    assert t.obs.shape == (2, 3, 4, 4) and t.state.shape == (2, 3, 4, 5) and t.noise.shape == t.clipped.shape == (2, 3, 4)
    assert t.obs[0, 1, 2, 0] == rec[0, 1, 2, 6] and t.state[0, 0, 0, 4] == rec[0, 0, 0, 14]
    assert t.noise[1, 2, 3] == rec[1, 2, 3, 15] and t.clipped[1, 2, 3] == rec[1, 2, 3, 16]
    assert t.action[1, 0, 0] == rec[1, 0, 0, 0] and t.value[1, 0, 0] == rec[1, 0, 0, 2] and t.episode(1, 2).shape == (2, 17)
    with pytest.raises(ValueError):
        t.clipped[0, 0, 0] = 1.0


# ---- grlxd -N: refused before any device is looked for -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def test_grlxd_usage_mentions_the_noise(grlxd, tmp_path):
    res = subprocess.run([grlxd], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "[-N sigma|own]" in res.stdout + res.stderr


@pytest.mark.parametrize("args,yaml,word", [
    (["-r", "4", "-N", "2.5"], "cart_pole-ac-tc.yaml", "needs the start states of -E"),
    (["-r", "4", "-E", "states5.txt", "-N", "-0.1"], "cart_pole-ac-tc.yaml", "neither a finite number >= 0 nor 'own'"),
    (["-r", "4", "-E", "states5.txt", "-N", "nan"], "cart_pole-ac-tc.yaml", "neither a finite number >= 0 nor 'own'"),
    (["-r", "4", "-E", "states5.txt", "-N", "inf"], "cart_pole-ac-tc.yaml", "neither a finite number >= 0 nor 'own'"),
    (["-r", "4", "-E", "states5.txt", "-N", "gaussian"], "cart_pole-ac-tc.yaml", "neither a finite number >= 0 nor 'own'"),
    (["-r", "4", "-E", "states.txt", "-N", "0.5"], "pendulum-sarsa-tc.yaml", "serves the actor-critic agent only"),
    (["-r", "4", "-g", "2", "-E", "states5.txt", "-N", "own"], "cart_pole-ac-tc.yaml", "-g 2 is not built"),
    (["-r", "1", "-E", "states5.txt", "-N", "own"], "cart_pole-ac-tc.yaml", "divides by n - 1"),
    (["-r", "4", "-E", "states.txt", "-N", "1"], "pendulum-fqi-ann.yaml", "not for experiment/batch_learning"),
    (["-r", "2", "-p", "/experiment/agent/predictor/alpha=0.1,0.2", "-E", "states5.txt", "-N", "1"], "cart_pole-ac-tc.yaml", "per-replica parameters (-p) are not built"),
])
def test_grlxd_noisy_refusals_name_their_reason(grlxd, tmp_path, args, yaml, word):
    (tmp_path / "states.txt").write_text("# angle velocity time\n3.14159 0 0\n0 0 0   # upright\n\n1 -2 1.5\n")
    (tmp_path / "states5.txt").write_text("0 3.14159 0 0 0\n0.5 0 0 0 1.0\n")
    res = subprocess.run([grlxd, "-s", "1", "-q", "-t", "12"] + args + [os.path.join(GOLDEN, yaml)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    said = res.stderr + res.stdout
    assert res.returncode != 0 and word in said, said
    assert "-N" in said
    assert "no HIP device" not in said, "refused only after a device was looked for"
    assert not list(tmp_path.glob("*noisy*"))
