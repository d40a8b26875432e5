"""grlx_project against the reference's OWN tile coding, through a recorded fixture.

tests/golden/ref_tiles.npz holds the specs and inputs of tests/ref_tile_cases.py and the indices that oracle/_ref/ref_tiles -- the
reference's tile_coding.cpp and its header compiled unmodified -- answered on them (tools/record_ref_envs.py;
tests/test_oracle_ref_tiles.py keeps the file fresh).  Nothing here reads the reference or the oracle: every number compared is the
reference binary's.  One grlx_project launch per spec on all its rows; the indices are integers and must be EQUAL on every row of
every spec, with no tolerance and no exclusions: inputs on and beside tile edges (where a kernel that multiplied by a reciprocal,
divided or fused would land in the neighbouring tile), the wrap, zero, negative coordinates and the last coordinates inside the
|x * scaling| < 2^30 bound.  The specs configure() refuses answer GRLX_ERR_INVALID, and so do the first value outside the bound, NaN
and the infinities, with nothing written.

The claim table of safe = 1 / 2 has no stateless entry point on the device: its kernels stay compared with the oracle
(tests/test_gpu_target_network.py), whose claim walk tests/test_oracle_ref_tiles.py now holds to the same binary.
"""
import ctypes as C

import numpy as np
import pytest

from tests import ref_tile_cases as tc

pytestmark = pytest.mark.gpu

FX = np.load(tc.FIXTURE)
NAMES = [str(n) for n in FX["names"]]
SENTINEL = 0xDEADBEEF


def spec_of(capi, k, prefix=""):
    D = int(FX[prefix + "dims"][k])
    return tc.tile_spec(dict(tilings=int(FX[prefix + "tilings"][k]), memory=int(FX[prefix + "memory"][k]),
                             res=list(FX[prefix + "res"][k, :D]), wrap=list(FX[prefix + "wrap"][k, :D])), capi.TileSpec)


@pytest.mark.parametrize("k", range(len(NAMES)), ids=NAMES)
def test_project_equals_the_reference_binarys_indices_on_every_row(grlx, k):
    x, want, tag = FX[f"x{k}"], FX[f"idx{k}"], FX[f"tag{k}"]
    assert 50 <= len(x) <= 512 and want.dtype == np.uint32
    got = grlx.runner.project(spec_of(grlx.capi, k), x)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert got.shape == want.shape and bad.size == 0, (f"{NAMES[k]}: {bad.size} of {len(x)} rows differ, tags {sorted({tc.TAGS[t] for t in tag[bad]})}, "
                                                        f"first {bad[0]}: x = {x[bad[0]]!r}, {want[bad[0]]} vs {got[bad[0]]}")
    inside = tag == tc.TAG["bound"]                                       # the rows just inside the bound are there, and passed
    q = np.abs(x[inside] * (FX["tilings"][k] / FX["res"][k, :x.shape[1]]))
    assert inside.sum() == 8 and ((q >= tc.BOUND - 2) & (q < tc.BOUND)).any(axis=1).all()


def test_refused_specs_answer_invalid(grlx):
    capi = grlx.capi
    sayable = [k for k in range(len(FX["refused_names"])) if FX["refused_wrap_len"][k] == FX["refused_dims"][k]]
    assert len(sayable) >= 2                                              # a wrapping vector of another length has no grlx_tile_spec
    for k in sayable:
        with pytest.raises(capi.GrlxError) as ei:
            grlx.runner.project(spec_of(capi, k, "refused_"), np.zeros((1, int(FX["refused_dims"][k]))))
        assert ei.value.code == capi.ERR_INVALID, str(FX["refused_names"][k])


@pytest.mark.parametrize("k", [0, 2, len(NAMES) - 5], ids=lambda k: NAMES[k])
def test_project_refuses_what_the_queries_refuse_and_writes_nothing(grlx, k):
    capi, lib = grlx.capi, grlx.capi.load()
    spec = spec_of(capi, k)
    s = dict(tilings=int(FX["tilings"][k]), res=list(FX["res"][k, :spec.dims]))
    plain = FX[f"x{k}"][:3]
    for bad, dim in tc.beyond_bound(s):
        x = np.ascontiguousarray(np.vstack([plain[:2], bad[None], plain[2:]]))
        out = np.full((4, spec.tilings), SENTINEL, np.uint32)
        rc = lib.grlx_project(C.byref(spec), x.ctypes.data_as(C.POINTER(C.c_double)), 4, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        msg = lib.grlx_last_error().decode()
        assert rc == capi.ERR_INVALID, f"{bad!r}: {rc} {msg}"
        assert f"row 2, dimension {dim}" in msg, msg
        assert (out == SENTINEL).all(), "a refused call wrote indices"
    # the same rows without the offender pass
    assert (grlx.runner.project(spec, plain) == FX[f"idx{k}"][:3]).all()
