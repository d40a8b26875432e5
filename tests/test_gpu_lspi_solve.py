"""lspi_solve_kernel on systems of the caller's choice (grlx_lspi_solve_systems, include/grlx_diag.h) against tests/lspi_solve_ref.py, bit
for bit: the library is built without contraction and every element of the work copy takes its updates in ascending k, so the blocked LU
has the bits of the plain one, and the back substitution's order is restated (tests/test_lspi_solve_host.py holds the reference to an
emulation of the blocked order and shows that it tells the tie rules apart on the tie fixtures).

The systems LSPI makes for itself, 1e-5 I + Phi^T (Phi - gamma Psi), hardly ever pivot off the diagonal.  These do: dense Gaussian matrices
(a swap at nearly every step, mostly with a row outside the panel), row permutations of a diagonal (exact arithmetic, a closed form),
small-integer matrices and constructed columns whose largest magnitude sits in several rows -- in different waves of the arg-max, inside
and far beyond the panel --, rows scaled over 2^+-200, and singular or non-finite systems for the flag of S9.

Shapes: F = 8 (one short panel), 16 (exactly one), 18 (one and two rows), 64 (four full panels, nothing padded), 363 (a ragged last
panel of 11) and 512 = kLspiMaxF.  Two replicas with different systems per context: the per-replica offsets of Asys, b, lu and w."""
import ctypes as C

import numpy as np
import pytest

from tests import lspi_solve_ref as ref
from tests.test_gpu_lspi import bits

pytestmark = pytest.mark.gpu

_runners = {}


def runner(grlx, F, fresh=False):
    """a context of two replicas and F features that never runs a batch: one per F, or a fresh one that the caller closes"""
    if fresh or F not in _runners:
        r = grlx.LspiRunner(grlx.pendulum_lspi_config(2, steps=ref.SHAPES[F], batch_size=1, max_batches=1), [1, 2])
        if fresh:
            return r
        _runners[F] = r
    return _runners[F]


@pytest.mark.parametrize("kind,F", ref.FIXTURES, ids=[f"{k}-f{F}" for k, F in ref.FIXTURES])
def test_the_kernel_has_the_references_bits(grlx, kind, F):
    r = runner(grlx, F)
    A, b = ref.fixture(kind, F)
    former = [r.params(k) for k in range(2)]
    x = r.solve_systems(A, b)
    for k, (want, pivots, flagged) in enumerate(ref.solved(kind, F)):
        bad = np.nonzero(bits(x[k]) != bits(want))[0]
        assert bad.size == 0, f"replica {k}: {bad.size} of {F} weights differ, first at {bad[0]}: {x[k][bad[0]]!r} vs {want[bad[0]]!r}"
        assert not flagged and r.info(k)["status"] == 0
        # the context as the kernel leaves it: w[0] = x, w[1] = the former w[0]
        assert (bits(r.params(k)) == bits(x[k])).all() and (bits(r.params(k, 1)) == bits(former[k])).all()
        j = np.arange(F)
        if kind == "dense":
            assert (pivots != j).sum() * 2 >= F, f"replica {k}: {(pivots != j).sum()} swaps in {F} steps"
            assert F < 18 or (pivots >= (j // ref.PANEL + 1) * ref.PANEL).any(), f"replica {k}: no swap crosses a panel"
        if kind == "permutation":
            assert (bits(x[k]) == bits(ref.permutation_closed_form(A[k], b[k]))).all(), f"replica {k}: the closed form"
    assert (bits(x[0]) != bits(x[1])).any()
    r.sync()


@pytest.mark.parametrize("kind", ref.S9)
def test_a_zero_or_non_finite_pivot_is_flagged(grlx, kind):
    """S9: the call returns 0, replica 1 carries status bit 64 and replica 0 does not, replica 0's x is untouched by its neighbour, and
    the context's sync fails from then on"""
    r, capi = runner(grlx, 18, fresh=True), grlx.capi            # a context of its own: the flag stays
    A, b = ref.fixture(kind, 18)
    (want, _, sound), (_, _, flagged) = ref.solved(kind, 18)
    assert not sound and flagged
    r.sync()
    x = r.solve_systems(A, b)                                   # (raises on any code but 0)
    assert r.info(1)["status"] & 64 and not r.info(0)["status"] & 64
    assert (bits(x[0]) == bits(want)).all()
    for _ in range(2):                                          # nothing clears the flag
        with pytest.raises(capi.GrlxError) as ei:
            r.sync()
        assert ei.value.code == capi.ERR_DOMAIN and "pivot" in str(ei.value)
    r.close()


@pytest.mark.parametrize("null", ["ctx", "A", "b", "x"])
def test_refusals_name_the_call(grlx, null):
    r, capi = runner(grlx, 8), grlx.capi
    A, b = ref.fixture("dense", 8)
    x, was = np.full((2, 8), 7.0), [r.params(k).tobytes() for k in range(2)]
    p = lambda name, a: None if null == name else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = r.lib.grlx_lspi_solve_systems(None if null == "ctx" else r._ctx, p("A", A), p("b", b), p("x", x))
    said = r.lib.grlx_last_error().decode()
    assert rc == capi.ERR_INVALID and said.startswith("grlx_lspi_solve_systems: ") and null + " is null" in said, said
    assert (x == 7.0).all() and [r.params(k).tobytes() for k in range(2)] == was, "a refused call wrote something"
    with pytest.raises(ValueError):
        r.solve_systems(A[:1], b)
