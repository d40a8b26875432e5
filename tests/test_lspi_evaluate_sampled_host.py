"""grlx_lspi_evaluate_sampled*, grlx_lspi_evaluate_ensemble_sampled*: what needs no device -- the bindings, the refusal of a null context
by name before any device work, and the runner's methods (the refusals that need a context: tests/test_gpu_lspi_evaluate_sampled.py)."""
import ctypes as C
import inspect

import numpy as np
import pytest

# entry point -> (arguments after the context and before the outputs, arguments of its ctypes signature)
CALLS = {"grlx_lspi_evaluate_sampled": ("policy", 17), "grlx_lspi_sampled_trajectory_record_words": ("none", 1),
         "grlx_lspi_evaluate_sampled_trajectory": ("policy", 18), "grlx_lspi_evaluate_ensemble_sampled": ("group", 22),
         "grlx_lspi_ensemble_sampled_trajectory_record_words": ("none", 1), "grlx_lspi_evaluate_ensemble_sampled_trajectory": ("group", 23)}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_null_context_is_refused_by_name(grlx, name):
    capi = grlx.capi
    lib = capi.load()
    kind, n_args = CALLS[name]
    assert len(capi._SIGS[name][1]) == n_args and capi._SIGS[name] == capi._SIGS[name.replace("grlx_lspi_", "grlx_fqi_")]
    states, out = np.array([[np.pi, 0.0, 0.0]]), np.full(15, 7.0)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    args = {"none": [], "policy": [0, 1, p(states), 1, 1, 0, 0.0, None, p(out)], "group": [0, 1, 1, 0, 1.0, 0, 0.0, p(states), 1, 1, None, p(out)]}[kind]
    args += [None] * (n_args - 1 - len(args) - name.endswith("_trajectory")) + ([p(out)] if name.endswith("_trajectory") else [])
    assert getattr(lib, name)(None, *args) == capi.ERR_INVALID
    assert (name + ": ctx is null") in lib.grlx_last_error().decode() and (out == 7.0).all()


# FqiRunner's signatures as they stood before both runners took these methods from one place: names, order and defaults, written out
SIGNATURES = {"evaluate_sampled": "(self, states, sampler='greedy', epsilon=None, streams=None, replicas=None, max_steps=0)",
              "sampled_trajectory_record_words": "(self)",
              "evaluate_sampled_trajectory": "(self, states, max_steps, sampler='greedy', epsilon=None, streams=None, replicas=None)",
              "evaluate_ensemble_sampled": "(self, states, group_size, strategy='majority', tau=0.1, member='greedy', member_param=None, streams=None, "
                                           "replicas=None, max_steps=0)",
              "ensemble_sampled_trajectory_record_words": "(self)",
              "evaluate_ensemble_sampled_trajectory": "(self, states, group_size, max_steps, strategy='majority', tau=0.1, member='greedy', member_param=None, "
                                                      "streams=None, replicas=None)"}


@pytest.mark.parametrize("m", sorted(SIGNATURES))
def test_both_runners_have_fqi_runners_signatures(grlx, m):
    for runner in (grlx.LspiRunner, grlx.FqiRunner):
        assert str(inspect.signature(getattr(runner, m))) == SIGNATURES[m], (runner.__name__, m)
