"""tests/lspi_solve_ref.py on its own (runs without a GPU): the reference that tests/test_gpu_lspi_solve.py holds lspi_solve_kernel to is a
sound solve, is exact where the arithmetic is, tells the two tie rules apart on every tie fixture, and has the bits of the kernel's
blocked elimination order restated step for step."""
import numpy as np
import pytest

from tests import lspi_solve_ref as ref
from tests.test_gpu_lspi import backward_error, bits

RANDOM = [(kind, F) for kind, F in ref.FIXTURES if kind != "permutation"]
TIES = [(kind, F) for kind, F in ref.FIXTURES if kind.startswith("tie")]

solved = ref.solved


@pytest.mark.parametrize("kind,F", RANDOM)
def test_backward_error_within_four_times_numpys(kind, F):
    A, b = ref.fixture(kind, F)
    for k, (x, _, flagged) in enumerate(solved(kind, F)):
        eta, eta_np = backward_error(A[k], b[k], x), backward_error(A[k], b[k], np.linalg.solve(A[k], b[k]))
        print(f"{kind} F = {F} replica {k}: eta = {eta:.3e}, numpy's = {eta_np:.3e}")
        assert not flagged
        assert eta <= 4 * eta_np, f"replica {k}: eta = {eta:.3e}, numpy's = {eta_np:.3e}"


@pytest.mark.parametrize("F", sorted(ref.SHAPES))
def test_permutations_give_the_closed_form_bit_for_bit(F):
    A, b = ref.fixture("permutation", F)
    for k, (x, pivots, flagged) in enumerate(solved("permutation", F)):
        assert not flagged and (bits(x) == bits(ref.permutation_closed_form(A[k], b[k]))).all(), f"replica {k}"
        assert (pivots != np.arange(F)).any(), f"replica {k}: the permutation is the identity"


@pytest.mark.parametrize("kind,F", TIES)
def test_the_tie_rule_shows_in_the_bits(kind, F):
    """a condition on the fixtures: taking the highest of the tied rows gives other bits of x, in both replicas"""
    for k in range(2):
        (x, piv, _), (xh, pivh, _) = solved(kind, F)[k], solved(kind, F, "highest")[k]
        assert (piv != pivh).any() and (bits(x) != bits(xh)).any(), f"replica {k}: the fixture does not tell the tie rules apart"


def test_the_constructed_ties_are_where_they_claim():
    for k, (r1, r2) in enumerate(ref.TIE_WAVES):
        assert r1 // 64 != r2 // 64
        assert solved("tie-waves", 363)[k][1][0] == min(r1, r2) and solved("tie-waves", 363, "highest")[k][1][0] == max(r1, r2)
    for k, (c, r1, r2) in enumerate(ref.TIE_PANEL):
        p0 = c // ref.PANEL * ref.PANEL
        assert p0 <= r1 < p0 + ref.PANEL and (r2 - p0) // 64 > 0 and (r1 - p0) // 64 == 0
        assert solved("tie-panel", 363)[k][1][c] == r1 and solved("tie-panel", 363, "highest")[k][1][c] == r2


@pytest.mark.parametrize("F", sorted(ref.SHAPES))
def test_dense_systems_swap_and_cross_panels(F):
    """what the dense fixtures claim: at least half the steps swap, and from F = 18 on some swap takes a row from beyond its panel"""
    for k, (_, pivots, _) in enumerate(solved("dense", F)):
        j = np.arange(F)
        assert (pivots != j).sum() * 2 >= F, f"replica {k}: {(pivots != j).sum()} swaps in {F} steps"
        if F >= 18:
            assert (pivots >= (j // ref.PANEL + 1) * ref.PANEL).any(), f"replica {k}: no swap crosses a panel"


@pytest.mark.parametrize("kind", ref.S9)
def test_the_flag(kind):
    (_, _, sound), (_, _, bad) = solved(kind, 18)
    assert not sound and bad


def blocked(A, b):
    """lspi_solve_kernel's factorisation as the kernel reads: per panel the pivot steps on the panel's columns alone, the panel's swaps
    on the other columns afterwards, U12 by forward substitution, A22 -= L21 U12 in ascending k.  Returns the work copy [LU | y]."""
    F = len(b)
    a, P = np.concatenate([A, b[:, None]], axis=1), ref.PANEL
    for p0 in range(0, F, P):
        pw = min(P, F - p0)
        sp, piv = a[p0:, p0:p0 + pw].copy(), []
        for j in range(pw):
            mag = np.abs(sp[j:, j])
            bi = j + int(np.argmax(np.where(mag >= 0, mag, -1.0)))
            piv.append(bi)
            sp[[j, bi]] = sp[[bi, j]]
            sp[j + 1:, j] = sp[j + 1:, j] / sp[j, j]
            sp[j + 1:, j + 1:] = sp[j + 1:, j + 1:] - sp[j + 1:, j][:, None] * sp[j, j + 1:][None, :]
        a[p0:, p0:p0 + pw] = sp
        other = np.r_[0:p0, p0 + pw:F + 1]
        for j, bi in enumerate(piv):
            if bi != j:
                a[np.ix_([p0 + j, p0 + bi], other)] = a[np.ix_([p0 + bi, p0 + j], other)]
        for k in range(pw):
            for q in range(k):
                a[p0 + k, p0 + pw:] = a[p0 + k, p0 + pw:] - sp[k, q] * a[p0 + q, p0 + pw:]
        for k in range(pw):
            a[p0 + pw:, p0 + pw:] = a[p0 + pw:, p0 + pw:] - sp[pw:, k][:, None] * a[p0 + k, p0 + pw:][None, :]
    return a


@pytest.mark.parametrize("F", [18, 60])
def test_the_blocked_order_gives_the_same_bits(F):
    """the premise of the kernel's test: blocked right-looking with panels of 16 and b as column F = plain row-swap LU, bit for bit"""
    rng = np.random.default_rng((808, F))
    for A, b in ((rng.standard_normal((F, F)), rng.standard_normal(F)), (rng.integers(-2, 3, (F, F)).astype(np.float64), rng.standard_normal(F))):
        x, _, flagged = ref.solve(A, b)
        assert not flagged and (bits(ref.back_substitute(blocked(A, b))) == bits(x)).all()
