"""grlx_lspi_evaluate*, grlx_lspi_query_ensemble: what needs no device -- the bindings and the refusal of a null context by name, before
any device work (the refusals that need a context: tests/test_gpu_lspi_evaluate.py)."""
import ctypes as C

import numpy as np
import pytest

# entry point -> (arguments after the context, arguments of its ctypes signature)
CALLS = {"grlx_lspi_evaluate": ("pairs", 12), "grlx_lspi_trajectory_record_words": ("none", 1), "grlx_lspi_evaluate_trajectory": ("pairs", 13),
         "grlx_lspi_query_ensemble": ("query", 7), "grlx_lspi_evaluate_ensemble": ("groups", 16),
         "grlx_lspi_ensemble_trajectory_record_words": ("none", 1), "grlx_lspi_evaluate_ensemble_trajectory": ("groups", 17)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_null_context_is_refused_by_name(grlx, name):
    capi = grlx.capi
    lib = capi.load()
    kind, n_args = CALLS[name]
    assert len(capi._SIGS[name][1]) == n_args and capi._SIGS[name] == capi._SIGS[name.replace("grlx_lspi_", "grlx_fqi_")]
    states, out = np.array([[np.pi, 0.0, 0.0]]), np.full(13, 7.0)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    args = {"none": [], "query": [0, 1, 1, p(states), 1, p(out)], "pairs": [0, 1, p(states), 1, 1, p(out)], "groups": [0, 1, 1, 0, p(states), 1, 1, p(out)]}[kind]
    args += [None] * (n_args - 1 - len(args) - name.endswith("_trajectory")) + ([p(out)] if name.endswith("_trajectory") else [])
    assert getattr(lib, name)(None, *args) == capi.ERR_INVALID
    assert (name + ": ctx is null") in lib.grlx_last_error().decode() and (out == 7.0).all()


def test_the_runner_has_fqi_runners_calls(grlx):
    import inspect
    for m in ("evaluate", "trajectory_record_words", "evaluate_trajectory", "query_ensemble_raw", "query_ensemble", "evaluate_ensemble",
              "ensemble_trajectory_record_words", "evaluate_ensemble_trajectory"):
        assert inspect.signature(getattr(grlx.LspiRunner, m)) == inspect.signature(getattr(grlx.FqiRunner, m)), m
