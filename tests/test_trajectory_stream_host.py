"""Streamed trajectories (grlx_evaluate_trajectory_stream), the part that needs no device: the chunk rule of grlx_host_rules.h against a
table of hand-computed cases and its stated properties, as a stand-alone program under the host sanitizers (tools/stream_rules_check.cpp,
built as tests/test_host_rules.py builds its checkers); and the binding's half -- the struct's layout, the callback type, the constants.
The symbols themselves are tests/test_capi_symbols.py's."""
import ctypes as C
import os
import re

from tests.test_host_rules import ROOT, _build_and_run

CHECK = os.path.join(ROOT, "tools", "stream_rules_check.cpp")


def test_the_chunk_rule_gives_its_hand_computed_values_under_the_host_sanitizers(tmp_path):
    _build_and_run(CHECK, tmp_path, "stream rules ok")


def test_the_binding_matches_the_header(grlx):
    capi = grlx.capi
    header = open(os.path.join(ROOT, "include", "grlx.h")).read()
    assert re.search(r"GRLX_ERR_STOPPED\s*=\s*-8\b", header) and capi.ERR_STOPPED == -8
    assert re.search(r"#define GRLX_ABI_VERSION 2\b", header), "the additions are pure: the ABI version stays"
    body = re.search(r"typedef struct grlx_trajectory_chunk \{(.*?)\} grlx_trajectory_chunk;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if stmt:
            kind = "ptr" if "*" in stmt else "i32"
            assert stmt.startswith(("int32_t", "const double", "const int32_t")), stmt
            declared += [(name.strip(" *"), kind) for name in stmt.split(None, 2 if kind == "ptr" else 1)[-1].split(",")]
    fields = [(name, "ptr" if isinstance(t, type(C.POINTER(C.c_double))) else "i32") for name, t in capi.TrajectoryChunkC._fields_]
    assert fields == declared, (fields, declared)
    assert declared[0] == ("struct_size", "i32") and [n for n, k in declared if k == "ptr"] == ["ret", "disc", "steps", "terminal", "ties", "final_state", "records"]
    assert C.sizeof(capi.TrajectoryChunkC) == 7 * 4 + 4 + 7 * 8, "seven int32, padding to the pointers, seven pointers"
    res, args = capi._SIGS["grlx_evaluate_trajectory_stream"]
    assert res is C.c_int and args[-2] is capi.TRAJECTORY_SINK and len(args) == 8
    assert not capi.TRAJECTORY_SINK(), "a sink made of nothing is the null pointer the library refuses"


def test_a_chunk_carries_the_views_of_a_trajectory(grlx):
    import numpy as np
    rec = np.arange(2 * 3 * 4 * 11, dtype=np.float64).reshape(2, 3, 4, 11)
    fin = np.zeros((2, 3, 3))
    z = np.zeros((2, 3))
    chunk = grlx.runner.TrajectoryChunk(5, z, z, np.full((2, 3), 2, np.int32), z, z, fin, rec)
    assert chunk.first_start == 5 and chunk.reward.shape == (2, 3, 4) and chunk.obs.shape == (2, 3, 4, 2) and chunk.state.shape == (2, 3, 4, 3)
    assert chunk.episode(1, 2).shape == (2, 11) and not chunk.action.flags.writeable
