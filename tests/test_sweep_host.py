"""Hyper-parameter sweeps without a GPU: the layout of the grid (grl_amd.sweep_grid and `grlxd -p ... -n` must agree clone
by clone), what `grlxd -p` refuses, and the three entry points of include/grlx.h -- declared, exported, bound."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "tests", "golden", "pendulum-sarsa-tc.yaml")
ALPHA = "/experiment/agent/predictor/alpha"
GAMMA = "/experiment/agent/predictor/gamma"
LAMBDA = "/experiment/agent/predictor/lambda"
EPSILON = "/experiment/agent/policy/sampler/epsilon"
NEW = ("grlx_set_replica_params", "grlx_get_replica_params", "grlx_curve_stats_grouped")


@pytest.fixture(scope="module")
def grlxd():
    from grl_amd import _build
    return _build.build_host()


def run(grlxd, args, cwd):
    return subprocess.run([grlxd] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def test_sweep_grid_order_and_sizes():
    import grl_amd
    g = grl_amd.sweep_grid(3, alpha=[0.1, 0.2], epsilon=[0.05, 0.1])
    assert list(g) == ["alpha", "epsilon"]                       # the axes in the order given
    assert all(len(v) == 2 * 2 * 3 for v in g.values())          # points x repetitions
    # point-major, the last axis fastest, every point three times in a row: replica i = point * repetitions + k
    assert g["alpha"] == [0.1] * 6 + [0.2] * 6
    assert g["epsilon"] == ([0.05] * 3 + [0.1] * 3) * 2
    g = grl_amd.sweep_grid(1, gamma=[0.9, 0.95, 0.97], lambda_=[0.4, 0.65], alpha=[0.2])
    assert g["gamma"] == [0.9, 0.9, 0.95, 0.95, 0.97, 0.97]
    assert g["lambda_"] == [0.4, 0.65] * 3
    assert g["alpha"] == [0.2] * 6
    for i in range(6):                                           # the general rule, digit by digit
        assert (g["gamma"][i], g["lambda_"][i]) == ([0.9, 0.95, 0.97][i // 2], [0.4, 0.65][i % 2])
    assert grl_amd.sweep_grid(4, epsilon=[0.01]) == {"epsilon": [0.01] * 4}
    for bad in (dict(repetitions=0, alpha=[0.1]), dict(repetitions=2), dict(repetitions=2, alpha=[])):
        with pytest.raises(ValueError):
            grl_amd.sweep_grid(**bad)


def test_grlxd_plan_equals_sweep_grid(grlxd, tmp_path):
    """`grlxd -n`: one line per clone (i seed alpha gamma lambda epsilon, %.17g), printed before anything touches the device --
    so it works on a box without one -- in the order of sweep_grid; the parameters not swept are the yaml's."""
    import grl_amd
    res = run(grlxd, ["-n", "-s", "5", "-r", "3", "-p", ALPHA + "=0.1,0.2", "-p", EPSILON + "=0.05,0.1", YAML], tmp_path)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.strip().split("\n")
    assert len(lines) == 12
    g = grl_amd.sweep_grid(3, alpha=[0.1, 0.2], epsilon=[0.05, 0.1])
    for i, line in enumerate(lines):
        f = line.split()
        assert len(f) == 6
        assert int(f[0]) == i and int(f[1]) == 5 + i
        assert [float(x) for x in f[2:]] == [g["alpha"][i], 0.97, 0.65, g["epsilon"][i]]
        assert f[2] == "%.17g" % g["alpha"][i] and f[5] == "%.17g" % g["epsilon"][i]
    assert not list(tmp_path.iterdir())                           # a plan writes nothing
    # the order of the -p options is the order of the axes
    res = run(grlxd, ["-n", "-s", "1", "-r", "2", "-p", LAMBDA + "=0.4,0.5", "-p", GAMMA + "=0.9,0.95,0.97", YAML], tmp_path)
    assert res.returncode == 0, res.stderr
    g = grl_amd.sweep_grid(2, lambda_=[0.4, 0.5], gamma=[0.9, 0.95, 0.97])
    got = [[float(x) for x in line.split()[2:]] for line in res.stdout.strip().split("\n")]
    assert got == [[0.2, g["gamma"][i], g["lambda_"][i], 0.05] for i in range(12)]
    # without -p: the clones of -r with the yaml's values
    res = run(grlxd, ["-n", "-s", "7", "-r", "2", YAML], tmp_path)
    assert res.returncode == 0 and res.stdout.strip().split("\n") == ["0 7 0.20000000000000001 0.96999999999999997 0.65000000000000002 0.050000000000000003",
                                                                       "1 8 0.20000000000000001 0.96999999999999997 0.65000000000000002 0.050000000000000003"]


@pytest.mark.parametrize("args,words", [
    (["-p", "/experiment/agent/policy/projector/sres=0.5,1"], ["unknown path", "/experiment/agent/policy/projector/sres"]),
    (["-p", "/experiment/agent/predictor/alfa=0.1"], ["unknown path", "alfa"]),
    (["-p", ALPHA + "="], ["empty value list", ALPHA]),
    (["-p", ALPHA], ["empty value list", ALPHA]),
    (["-p", ALPHA + "=0.1,"], ["empty value list"]),
    (["-p", ALPHA + "=0.1,x"], ["not a number", "'x'"]),
    (["-p", ALPHA + "=0.1", "-p", ALPHA + "=0.2"], ["given twice"]),
    (["-g", "2", "-p", ALPHA + "=0.1,0.2"], ["-g 2", "one GPU"]),
    (["-r", "1", "-p", ALPHA + "=0.1,0.2"], ["repetitions per point", ">= 2"]),        # one repetition has no standard deviation (n - 1 = 0)
])
def test_grlxd_sweep_refusals(grlxd, tmp_path, args, words):
    res = run(grlxd, ["-n", "-s", "5", "-r", "3"] + args + [YAML], tmp_path)
    assert res.returncode != 0
    for w in words:
        assert w in res.stderr, res.stderr
    assert res.stdout == ""


def test_grlxd_sweep_with_a_steps_budget_or_multi_is_refused(grlxd, tmp_path):
    text = open(YAML).read()
    assert text.startswith("experiment:\n") and "steps: 0" in text
    y = tmp_path / "budget.yaml"
    y.write_text(text.replace("steps: 0", "steps: 5000"))
    res = run(grlxd, ["-n", "-s", "5", "-r", "3", "-p", ALPHA + "=0.1,0.2", str(y)], tmp_path)
    assert res.returncode != 0 and "steps budget" in res.stderr and res.stdout == "", res.stderr + res.stdout
    # experiment/multi around the same experiment (absolute references move one level down)
    inner = "".join("  " + line + "\n" for line in text.splitlines()[1:])
    for sub in ("environment", "agent"):
        inner = inner.replace(f": experiment/{sub}", f": experiment/experiment/{sub}")
    y = tmp_path / "multi.yaml"
    y.write_text("experiment:\n  type: experiment/multi\n  instances: 2\n  experiment:\n" + inner)
    res = run(grlxd, ["-n", "-s", "5", "-r", "3", "-p", ALPHA + "=0.1,0.2", str(y)], tmp_path)
    assert res.returncode != 0 and "experiment/multi" in res.stderr and res.stdout == "", res.stderr + res.stdout


def test_grlxd_sweep_of_a_batch_experiment_is_refused(grlxd, tmp_path):
    res = run(grlxd, ["-n", "-s", "5", "-r", "3", "-p", ALPHA + "=0.1,0.2", os.path.join(ROOT, "tests", "golden", "pendulum-fqi-ann.yaml")], tmp_path)
    assert res.returncode != 0 and "experiment/batch_learning" in res.stderr, res.stderr


def test_new_symbols_declared_exported_and_bound(grlx):
    from tests.test_capi_symbols import declared_functions, exported_functions
    declared, exported = declared_functions(), exported_functions(grlx.capi.lib_path())
    lib = grlx.capi.load()
    for name in NEW:
        assert name in declared and name in exported and name in grlx.capi._SIGS
        assert getattr(lib, name).argtypes == grlx.capi._SIGS[name][1]
    assert lib.grlx_abi_version() == 2                           # pure additions: the version stays
    assert (grlx.capi.PARAM_ALPHA, grlx.capi.PARAM_GAMMA, grlx.capi.PARAM_LAMBDA, grlx.capi.PARAM_EPSILON) == (0, 1, 2, 3)
    for method in ("set_replica_params", "replica_params", "curve_stats_grouped"):
        assert callable(getattr(grlx.Runner, method))


def test_null_context_is_invalid(grlx):
    lib = grlx.capi.load()
    v = (C.c_double * 4)(0.1, 0.1, 0.1, 0.1)
    assert lib.grlx_set_replica_params(None, 0, v) == grlx.capi.ERR_INVALID
    assert b"null" in lib.grlx_last_error()
    assert lib.grlx_get_replica_params(None, 0, v) == grlx.capi.ERR_INVALID
    assert lib.grlx_curve_stats_grouped(None, 0, 1, 1, None, None) == grlx.capi.ERR_INVALID
