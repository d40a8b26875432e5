"""The host-side pieces of the policy queries that need no device: grl_amd.observation_grid, the statistics Runner.query_ensemble forms
from the library's raw sums, the declarations of the new entry points, and what `grlxd -Q` refuses before it looks for a device."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_observation_grid_is_numpy_meshgrid_row_major():
    import grl_amd
    lo, hi, points = [-3.0, 0.5, 10.0], [3.0, 0.5, 14.0], [5, 1, 3]
    g = grl_amd.observation_grid(lo, hi, points)
    assert g.shape == (15, 3) and g.dtype == np.float64 and g.flags["C_CONTIGUOUS"]
    mesh = np.meshgrid(*[np.linspace(a, b, n) for a, b, n in zip(lo, hi, points)], indexing="ij")
    want = np.stack([m.ravel() for m in mesh], axis=1)
    assert g.tobytes() == want.tobytes()
    # row-major: the last dimension fastest; end points included
    assert list(g[0]) == [-3.0, 0.5, 10.0] and list(g[1]) == [-3.0, 0.5, 12.0] and list(g[-1]) == [3.0, 0.5, 14.0]
    row = 0
    for a in np.linspace(-3.0, 3.0, 5):
        for c in np.linspace(10.0, 14.0, 3):
            assert list(g[row]) == [a, 0.5, c]
            row += 1


def test_observation_grid_of_one_dimension_and_its_refusals():
    import grl_amd
    g = grl_amd.observation_grid(0.0, 1.0, 3)
    assert g.shape == (3, 1) and list(g[:, 0]) == [0.0, 0.5, 1.0]
    with pytest.raises(ValueError):
        grl_amd.observation_grid([0, 0], [1, 1], [3])
    with pytest.raises(ValueError):
        grl_amd.observation_grid([0, 0], [1, 1], [3, 0])


def test_ensemble_result_from_raw_sums():
    """mean, variance (n - 1), votes and the majority with the lowest index winning a tie, from the raw sums of two groups of four"""
    from grl_amd import EnsembleResult
    values = np.array([[1.0, 2.0, 4.0, 9.0], [-1.0, -1.0, -1.0, -1.0]])
    raw = np.zeros((2, 1, 8))
    for g in range(2):
        raw[g, 0, 0] = values[g].sum()
        raw[g, 0, 1] = (values[g] * values[g]).sum()
    raw[0, 0, 2:5] = [4.0, 8.0, 12.0]
    raw[0, 0, 5:8] = [1, 1, 2]
    raw[1, 0, 5:8] = [2, 2, 0]
    res = EnsembleResult(raw, 4, 3)
    assert res.mean_value[0, 0] == 4.0 and res.mean_value[1, 0] == -1.0
    assert abs(res.var_value[0, 0] - np.var(values[0], ddof=1)) < 1e-12 and res.var_value[1, 0] == 0.0
    assert list(res.mean_q[0, 0]) == [1.0, 2.0, 3.0]
    assert res.votes.dtype == np.int64 and list(res.votes[0, 0]) == [1, 1, 2]
    assert res.majority[0, 0] == 2 and res.majority[1, 0] == 0
    assert np.isnan(EnsembleResult(raw, 1, 3).var_value).all()


def test_reference_helper_on_a_hand_made_table():
    """tests/policy_query_ref.py itself: findmax, value and the ensemble's sums on values small enough to check by hand"""
    from tests import policy_query_ref as ref
    assert ref.findmax([1.0, 3.0, 3.0]) == (1, 2) and ref.findmax([0.0, 0.0, 0.0]) == (0, 3) and ref.findmax([2.0, 1.0, 2.0, 0.0, 2.0]) == (0, 3)
    assert ref.value_of([1.0, 3.0, 3.0]) == 3.0 and ref.value_of([0.0, 0.0, 0.0]) == 0.0
    assert ref.value_of([0.1, 0.1, 0.1]) == (0.0 + 0.1 * (1.0 / 3)) + 0.1 * (1.0 / 3) + 0.1 * (1.0 / 3)
    q = np.array([[[1.0, 2.0, 0.0]], [[5.0, 2.0, 5.0]]])
    value, greedy = np.array([[2.0], [5.0]]), np.array([[1], [0]])
    assert list(ref.ensemble(q, value, greedy, 2)[0, 0]) == [7.0, 29.0, 6.0, 4.0, 5.0, 1.0, 1.0, 0.0]


def test_the_query_entry_points_are_declared_and_bound():
    """include/grlx.h declares the three queries with the reference lines they replace, grlx_diag.h the staging bound, and the binding
    has a signature for each (tests/test_capi_symbols.py holds header, exports and binding to each other once the library is built)"""
    from grl_amd import capi
    with open(os.path.join(ROOT, "include", "grlx.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "include", "grlx_diag.h")) as f:
        diag = f.read()
    for name in ("grlx_query_q", "grlx_query_state", "grlx_query_ensemble", "grlx_fqi_query"):
        assert re.search(r"\bint\s+" + name + r"\(grlx_(fqi_)?ctx \*ctx", header), name
        assert name in capi._SIGS
    for cite in ("q.cpp:94-107", "q.cpp:56-68", "greedy.cpp:47-61", "action.cpp:99-112"):
        assert cite in header, cite
    assert "grlx_set_query_chunk_bytes" in diag and "grlx_set_query_chunk_bytes" in capi._DIAG_SIGS
    assert "#define GRLX_ABI_VERSION 2" in header


# ---- grlxd -Q: refused before any device is looked for (without a GPU, a run that got as far as the device would say "no HIP device") ----
GOLDEN = os.path.join(ROOT, "tests", "golden")
YAML = os.path.join(GOLDEN, "pendulum-sarsa-tc.yaml")


@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def run(grlxd, args, cwd):
    return subprocess.run([grlxd, "-s", "1", "-q"] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.fixture()
def obs_file(tmp_path):
    (tmp_path / "obs.txt").write_text("# angle velocity\n0 0\n3.14 1.5   # hanging\n\n-1 2\n")
    return "obs.txt"


def test_grlxd_usage_mentions_the_query(grlxd, tmp_path):
    res = subprocess.run([grlxd], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert res.returncode != 0 and "[-Q observations]" in res.stdout + res.stderr


@pytest.mark.parametrize("content,word", [(None, "could not open"), ("0 0\n1\n", "line 2 has 1 columns"), ("0 x\n", "'x' is not a finite number"),
                                          ("0 nan\n", "not a finite number"), ("# nothing\n\n", "no observations"),
                                          ("0 0 0\n", "3 columns, the agent's observation has 2")])
def test_grlxd_query_refuses_a_missing_or_malformed_file(grlxd, tmp_path, content, word):
    if content is not None:
        (tmp_path / "q.txt").write_text(content)
    res = run(grlxd, ["-r", "4", "-t", "12", "-Q", "q.txt", YAML], tmp_path)
    assert res.returncode != 0 and word in res.stderr + res.stdout, res.stderr + res.stdout
    assert "no HIP device" not in res.stderr + res.stdout, "refused only after a device was looked for"
    assert not list(tmp_path.glob("*policy*"))


@pytest.mark.parametrize("args,yaml,word", [
    (["-r", "4", "-g", "2"], "pendulum-sarsa-tc.yaml", "-g 2 is not built"),
    (["-r", "1"], "pendulum-sarsa-tc.yaml", "divides by n - 1"),
    (["-r", "4"], "pendulum-fqi-ann.yaml", "not for experiment/batch_learning"),
    (["-r", "4"], "cart_pole-ac-tc.yaml", "actor-critic"),
])
def test_grlxd_query_refusals_name_their_reason(grlxd, tmp_path, obs_file, args, yaml, word):
    if "cart_pole" in yaml:
        (tmp_path / obs_file).write_text("0 0 0 0\n")
    res = run(grlxd, args + ["-t", "12", "-Q", obs_file, os.path.join(GOLDEN, yaml)], tmp_path)
    assert res.returncode != 0 and word in res.stderr + res.stdout, res.stderr + res.stdout
    assert "no HIP device" not in res.stderr + res.stdout, "refused only after a device was looked for"
