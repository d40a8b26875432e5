"""lspi_solve_kernel (grl_amd/csrc/grlx_lspi.hip) restated in plain numpy, operation for operation: what the kernel's x is held to bit for bit.

The factorisation here is the UNBLOCKED one.  The kernel's is blocked (panels of PANEL columns, U12, A22), but every element of its work
copy [A | b] receives its updates a -= l * u in ascending k wherever they happen, products and differences rounded separately
(-ffp-contract=off), and the pivot of a column is searched after all updates of that column: the bits are those of the plain loop below
(tests/test_lspi_solve_host.py holds an emulation of the blocked order to this).  Only the back substitution has an order of its own.

Also the systems the solve is tested on (fixture, FIXTURES): the kernel's test and the reference's own share them."""
import numpy as np

PANEL = 16      # kPanel: the back substitution runs in blocks of this many rows

SHAPES = {8: [2, 2, 2], 16: [2, 2, 4], 18: [2, 3, 3], 64: [4, 4, 4], 363: [11, 11, 3], 512: [8, 8, 8]}      # F: the steps that give it


def back_substitute(a):
    """x from the factorised work copy [U | y] in the kernel's order: blocks of PANEL rows from the bottom; inside the diagonal block
    ascending k from i + 1; a row above a block subtracts that block's terms in ascending k, blocks in descending order"""
    F = a.shape[0]
    x = a[:, F].copy()
    for p0 in range((F - 1) // PANEL * PANEL, -1, -PANEL):
        pw = min(PANEL, F - p0)
        for i in range(pw - 1, -1, -1):
            s = x[p0 + i]
            for k in range(i + 1, pw):
                s = s - a[p0 + i, p0 + k] * x[p0 + k]
            x[p0 + i] = s / a[p0 + i, p0 + i]
        s = x[:p0].copy()
        for k in range(pw):
            s = s - a[:p0, p0 + k] * x[p0 + k]
        x[:p0] = s
    return x


def solve(A, b, tie="lowest"):
    """(x, pivots, flagged) of A x = b: pivots[j] = the row that step j took its pivot from, flagged = a pivot was 0, NaN or infinite (S9).
    tie: which of several rows of equal largest magnitude is the pivot -- "lowest" is the kernel's rule (S8)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    F = A.shape[0]
    assert A.shape == (F, F) and b.shape == (F,) and tie in ("lowest", "highest")
    a = np.concatenate([A, b[:, None]], axis=1)             # b rides along as column F
    pivots, flagged = np.zeros(F, np.int64), False
    with np.errstate(all="ignore"):
        for j in range(F):
            mag = np.abs(a[j:, j])
            mag = np.where(mag >= 0, mag, -1.0)             # a NaN is never larger
            at = np.nonzero(mag == mag.max())[0]
            p = j + int(at[0] if tie == "lowest" else at[-1])
            pivots[j] = p
            if p != j:
                a[[j, p]] = a[[p, j]]
            pv = a[j, j]
            if not (abs(pv) > 0 and abs(pv) < np.inf):
                flagged = True
            l = a[j + 1:, j] / pv
            prod = l[:, None] * a[j, j + 1:][None, :]       # a product, then a difference: numpy fuses nothing
            a[j + 1:, j + 1:] = a[j + 1:, j + 1:] - prod
        x = back_substitute(a)
    return x, pivots, flagged


# ------------------------------------------------------------------------------------------ the systems ---
# fixture(kind, F) -> (A[2][F][F], b[2][F]): one system per replica of a two-replica context, never the same two.  Every draw comes from
# default_rng((seed of the kind, F)); the seeds are written out here.
SEEDS = {"dense": 101, "permutation": 202, "tie-int": 303, "tie-waves": 404, "tie-panel": 505, "range": 606,
         "zero-column": 701, "same-rows": 702, "inf": 703, "nan": 704}
S9 = ("zero-column", "same-rows", "inf", "nan")                # replica 0 sound, replica 1 singular or not finite
# which F each kind is made at
FIXTURES = ([("dense", F) for F in SHAPES] + [("permutation", F) for F in SHAPES] + [("tie-int", F) for F in (18, 64, 363)] +
            [("tie-waves", 363), ("tie-panel", 363), ("range", 64)])
# tie-waves: column 0 of replica k has +v in row TIE_WAVES[k][0] and -v in row TIE_WAVES[k][1], v above every other magnitude: the tied
# rows sit in different waves of the block-wide arg-max (row = thread, 64 to a wave)
TIE_WAVES = [(3, 70), (130, 65)]
# tie-panel: (column c, row inside c's panel, row beyond it by more than 64 k) -- both rows are zero left of c, so that no earlier step
# touches or moves them, and carry -v / +v in column c, v = 2^40 far above what the elimination makes of the Gaussian entries
TIE_PANEL = [(17, 20, 16 + 64 * 2 + 5), (35, 47, 32 + 64 * 4 + 9)]


def fixture(kind, F):
    rng = np.random.default_rng((SEEDS[kind], F))
    A, b = rng.standard_normal((2, F, F)), rng.standard_normal((2, F))
    if kind == "permutation":
        for k in range(2):
            p, d = rng.permutation(F), 2.0 ** rng.integers(-20, 20, F)
            A[k] = 0
            A[k, np.arange(F), p] = d                       # row i: d[i] x[p[i]] = b[i]
    elif kind == "tie-int":
        A = rng.integers(-2, 3, (2, F, F)).astype(np.float64)
    elif kind == "tie-waves":
        for k, (r1, r2) in enumerate(TIE_WAVES):
            A[k, r1, 0], A[k, r2, 0] = 8.0, -8.0
    elif kind == "tie-panel":
        for k, (c, r1, r2) in enumerate(TIE_PANEL):
            A[k, [r1, r2], :c] = 0
            A[k, r1, c], A[k, r2, c] = -2.0 ** 40, 2.0 ** 40
    elif kind == "range":
        scale = 2.0 ** rng.integers(-200, 201, (2, F))
        A, b = A * scale[:, :, None], b * scale
    elif kind == "zero-column":
        A[1, :, 7] = 0
    elif kind == "same-rows":
        A[1, 11], b[1, 11] = A[1, 4], b[1, 4]
    elif kind == "inf":
        A[1, 5, 9] = np.inf
    elif kind == "nan":
        A[1, 5, 9] = np.nan
    else:
        assert kind == "dense"
    return A, b


_solved = {}


def solved(kind, F, tie="lowest"):
    """solve()'s (x, pivots, flagged) per replica of a fixture; made once for every test that asks"""
    if (kind, F, tie) not in _solved:
        A, b = fixture(kind, F)
        _solved[kind, F, tie] = [solve(A[k], b[k], tie) for k in range(2)]
    return _solved[kind, F, tie]


def permutation_closed_form(A, b):
    """x of one permutation system without any elimination: x[p[i]] = b[i] / d[i], exact"""
    i, p = np.nonzero(A)
    x = np.zeros_like(b)
    x[p] = b[i] / A[i, p]
    return x
