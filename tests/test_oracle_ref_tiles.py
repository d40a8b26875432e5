"""The oracle's tile coding against the reference's OWN source, index by index.

oracle/_ref/ref_tiles is the reference's base/src/projectors/tile_coding.cpp with its header (the hash, the claim table), compiled
unmodified against stand-in framework headers (oracle/ref).  On every row of every spec of tests/ref_tile_cases.py -- the projectors
of all four environments, 1 to 32 tilings, 1 to 8 dimensions, wrapping on any dimension, memories that are no power of two, inputs on
and beside tile edges, the wrap, zero and the +-2^30 bound -- orc_tile_project must give the binary's indices and
orc_tile_project_hash its hash sums, with no exclusions.  orc_tile_claim, the function the oracle's experiments walk their claim
table with, must give the binary's index through interleaved single and variant projections under safe = 1 and 2 on tables of 61,
64 and 257 slots, and leave the binary's claim table.  The oracle refuses the specs configure() throws on.

tests/golden/ref_tiles.npz (what the GPU test reads) must equal a fresh run: tools/record_ref_envs.py rewrites it.

Skipped only where there is neither a checkout of the reference nor a binary; with the sources and no binary the tests fail.
"""
import os

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import ref_tile_cases as tc


@pytest.fixture(scope="module")
def binary():
    ob.load()                                                             # make -C oracle: builds the binary where the sources are
    if not os.path.exists(tc.REF_BIN):
        if tc.reference_sources_present():
            pytest.fail(f"the reference's sources are at {tc.REFERENCE} but make -C oracle left no {tc.REF_BIN}")
        pytest.skip("neither the reference's sources nor oracle/_ref/ref_tiles on this machine")
    return tc.REF_BIN


SPECS = tc.specs()
_cache = {}


def cases_of(k):
    if k not in _cache:
        _cache[k] = tc.inputs(SPECS[k], seed=7000 + k)
    return _cache[k]


def test_the_specs_cover_what_the_kernels_are_built_for():
    dims = {len(s["res"]) for s in SPECS}
    assert {1, 2, 3, 4, 5, 6, 8} <= dims and max(dims) == tc.MAX_DIMS
    assert {1, 8, 16, 32} <= {s["tilings"] for s in SPECS}
    assert any(s["memory"] & (s["memory"] - 1) for s in SPECS), "a memory that is no power of two"
    wrapped = [tuple(np.nonzero(s["wrap"])[0]) for s in SPECS]
    assert (0,) in wrapped and (1,) in wrapped and any(len(w) >= 3 for w in wrapped)
    assert any(w and w[-1] == len(s["res"]) - 1 for w, s in zip(wrapped, SPECS)), "wrapping on the last dimension"
    assert len({s["name"] for s in SPECS}) == len(SPECS)


@pytest.mark.parametrize("k", range(len(SPECS)), ids=[s["name"] for s in SPECS])
def test_oracle_indices_and_hash_sums_equal_the_reference_binarys(binary, k):
    s, cases = SPECS[k], cases_of(k)
    x = cases["x"]
    assert 50 <= len(x) <= tc.MAX_ROWS
    for what, ref, got in (("index", tc.reference_indices(s, x), tc.oracle_indices(s, x)),
                           ("hash sum", tc.reference_hashes(s, x), tc.oracle_indices(s, x, full_hash=True))):
        bad = np.nonzero((ref != got).any(axis=1))[0]
        assert bad.size == 0, (f"{s['name']} {what}: {bad.size} of {len(x)} rows differ, tags {sorted({tc.TAGS[t] for t in cases['tag'][bad]})}, "
                               f"first {bad[0]}: x = {x[bad[0]]!r}, {ref[bad[0]]} vs {got[bad[0]]}")
    assert (tc.reference_indices(s, x) < s["memory"]).all()


@pytest.mark.parametrize("safe", [1, 2])
@pytest.mark.parametrize("memory", tc.CLAIM_MEMORIES)
def test_claim_function_equals_the_reference_binarys_through_a_sequence(binary, memory, safe):
    seq = tc.claim_sequence(memory, safe)
    assert (seq["kind"] == tc.RESET).sum() == 1 and (seq["kind"] == tc.SINGLE).sum() > 100 and (seq["kind"] == tc.VARIANTS).sum() > 60
    ref, ref_table = tc.reference_claims(seq)
    got, got_table = tc.oracle_claims(seq)
    for n, (kind, a, b) in enumerate(zip(seq["kind"], ref, got)):
        assert a == b, f"memory {memory}, safe {safe}, operation {n} (kind {kind}): {a} vs {b}"
    assert ref_table == got_table
    taken = sum(v != -1 for v in ref_table)
    assert 0 < taken <= tc.MAX_OCCUPANCY * memory
    before_reset = ref[int(np.nonzero(seq["kind"] == tc.RESET)[0][0])]
    assert 0.5 * memory < sum(v != -1 for v in before_reset) <= tc.MAX_OCCUPANCY * memory


def test_variant_projections_claim_under_safe_2_only(binary):
    """the variant projections of a sequence alone leave no claim under safe = 1: they find their way without taking slots"""
    tables = {}
    for safe in (1, 2):
        seq = tc.claim_sequence(257, safe)
        keep = seq["kind"] != tc.SINGLE                                   # a part of the sequence: it claims no more than the whole
        only_variants = dict(seq, kind=seq["kind"][keep], x=seq["x"][keep])
        tables[safe] = tc.reference_claims(only_variants)[1]
        assert tables[safe] == tc.oracle_claims(only_variants)[1]
    assert all(v == -1 for v in tables[1]) and any(v != -1 for v in tables[2])


def test_oracle_refuses_the_specs_the_reference_refuses(binary):
    refused = tc.refused_specs()
    assert len(refused) >= 2
    for s in refused:
        assert tc.reference_refuses(s), s["name"]
        if tc.tile_spec(s) is not None:                                   # a wrapping vector of another length has no orc_tile_spec
            assert tc.oracle_refuses(s), s["name"]
    assert sum(tc.tile_spec(s) is not None for s in refused) >= 2
    for s in SPECS:
        assert not tc.reference_refuses(s) and not tc.oracle_refuses(s), s["name"]


def test_fixture_equals_a_fresh_run(binary):
    fx = np.load(tc.FIXTURE)
    assert os.path.getsize(tc.FIXTURE) < 256 * 1024
    assert list(fx["names"]) == [s["name"] for s in SPECS] and list(fx["refused_names"]) == [s["name"] for s in tc.refused_specs()]
    for k, s in enumerate(SPECS):
        cases = cases_of(k)
        D = len(s["res"])
        assert (fx["tilings"][k], fx["memory"][k], fx["dims"][k]) == (s["tilings"], s["memory"], D)
        assert (fx["res"][k, :D] == s["res"]).all() and (fx["wrap"][k, :D] == s["wrap"]).all()
        assert (fx[f"x{k}"].view(np.uint64) == cases["x"].view(np.uint64)).all() and (fx[f"tag{k}"] == cases["tag"]).all()
        assert (fx[f"idx{k}"] == tc.reference_indices(s, cases["x"])).all(), s["name"]
