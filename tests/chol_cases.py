"""Systems for the reduced-system Cholesky kernels (mcptam_amd/csrc/ba_chol.h, ba_chol2.h) whose right answer is known without trusting
a float64 library: tests/test_chol_cases_cpu.py checks the builders, tests/test_chol_seams_gpu.py runs the kernels on them.

EXACT INTEGER SYSTEMS.  L is unit lower triangular; inside a diagonal 32 x 32 tile only its first sub-diagonal is non-zero (+-1), so the
tile's inverse is all 0 / +-1; the off-diagonal tiles are drawn from {-1, 0, 1} and are non-zero only on the textbook symbolic fill of the
tile pattern the plan is handed.  A = L L^T, x0 an integer vector in [-3, 3], b = A x0.  Every intermediate of the factorisation, of
L_kk^-1, of y = L^-1 b = L^T x0 and of x is then an integer far below 2^53 (|A| <= n, |b| <= 3 n^2), every sum of them is exact in
whatever order it is taken, and a correct kernel returns x0 BIT FOR BIT: a tile update that is dropped, doubled or taken from the wrong
slot shows at full size, whatever the conditioning.  (The kernels take 1/sqrt(pivot) from v_rsq_f64 plus a third-order correction; at a
pivot of exactly 1 the corrected value is 1 unless the raw instruction were off by more than about 2^-18.)

BROKEN PIVOTS.  From an exact system, A[p, p] -= 1 makes pivot p exactly 0 and A[p, p] -= 2 makes it exactly -1; the pivots before p
are untouched.  Two more carry a NaN: A[p, p] = NaN, and a NaN inside tile (ntc - 1, 0), which reaches a pivot only in the last
diagonal tile, after a trip through the far tiles.

GRADED SYSTEMS.  A = Q diag(logspace(0, -e, n)) Q^T, symmetrised, cond_2(A) = 10^e.  Their reference is a column Cholesky and two
triangular solves written out in np.longdouble (reference_solve): with the 64-bit mantissa of x87 extended precision that is 2^11 =
about 2000 times finer than float64, which is fine enough to measure a float64 solver's error only while that error stays well above
cond * 2^-64 -- up to e = 9, not beyond (at e = 12 the reference's own error would be a percent of what it is to judge)."""
import functools

import numpy as np

NB = 32


def ntiles(n):
    return (n + NB - 1) // NB


def dissect_orig(ntc, b):
    """Position -> original block of a band of b tiles ordered [left half | right half reversed | the b blocks between them]."""
    h = (ntc - b) // 2
    return [i if i < h else ((ntc - 1) - (i - h) if i < ntc - b else h + (i - (ntc - b))) for i in range(ntc)]


def tile_pattern(n, band):
    """The lower-triangular tile pattern mcp_chol_debug_runs hands the plan: 0 dense, > 0 band + border, < 0 dissected band."""
    ntc = ntiles(n)
    P = np.zeros((ntc, ntc), dtype=bool)
    orig = dissect_orig(ntc, -band) if band < 0 else None
    for i in range(ntc):
        for j in range(i + 1):
            if band == 0:
                P[i, j] = True
            elif band > 0:
                P[i, j] = i - j <= band or i >= ntc - band
            else:
                P[i, j] = abs(orig[i] - orig[j]) <= -band
    return P


def symbolic_fill(n, pattern):
    """Textbook symbolic Cholesky on the tile graph; the right-hand side is row n of the system, so its tile row (n // 32) is dense.
    Returns (ntr, ntc): ntr = ntc + 1 when the right-hand side has a block row of its own."""
    ntc = ntiles(n)
    ntr = (n + 1 + NB - 1) // NB
    P = np.zeros((ntr, ntc), dtype=bool)
    P[:ntc, :ntc] = np.tril(pattern.astype(bool))
    P[np.arange(ntc), np.arange(ntc)] = True
    P[n // NB, :] = True
    for k in range(ntc):
        below = [i for i in range(k + 1, ntr) if P[i, k]]
        for a in below:
            for b in below:
                if b <= a and b < ntc:
                    P[a, b] = True
    return P


@functools.lru_cache(maxsize=None)
def exact_system(n, band=0, seed=0):
    """dict(L, A, x0, b, fill, pattern) of an exact integer system (module docstring).  Cached: treat the arrays as read-only."""
    rng = np.random.default_rng([n, band + 64, seed])
    ntc = ntiles(n)
    pattern = tile_pattern(n, band)
    fill = symbolic_fill(n, pattern)
    L = np.eye(n)
    for i in range(ntc):
        r0, r1 = NB * i, min(NB * i + NB, n)
        for r in range(r0 + 1, r1):
            L[r, r - 1] = rng.choice([-1.0, 1.0])
        for j in range(i):
            if fill[i, j]:
                L[r0:r1, NB * j:NB * j + NB] = rng.integers(-1, 2, size=(r1 - r0, NB))
    A = L @ L.T
    x0 = rng.integers(-3, 4, size=n).astype(np.float64)
    out = dict(L=L, A=A, x0=x0, b=A @ x0, fill=fill, pattern=pattern)
    for v in out.values():
        v.setflags(write=False)
    return out


def broken(sysm, kind, p=None):
    """(A, b) of the exact system `sysm` with one pivot broken.  kind: "zero" (pivot p = 0), "neg" (pivot p = -1), "nan_diag"
    (A[p, p] = NaN), "nan_far" (a NaN inside tile (ntc - 1, 0): first bad pivot = first row of the last diagonal tile)."""
    A = sysm["A"].copy()
    n = A.shape[0]
    if kind == "zero":
        A[p, p] -= 1.0
    elif kind == "neg":
        A[p, p] -= 2.0
    elif kind == "nan_diag":
        A[p, p] = np.nan
    elif kind == "nan_far":
        A[NB * (ntiles(n) - 1), 5] = np.nan
        A[5, NB * (ntiles(n) - 1)] = np.nan
    else:
        raise ValueError(kind)
    return A, sysm["b"].copy()


def first_bad_pivot(A):
    """Index of the first pivot of a plain float64 column Cholesky that is not > 0 (NaN included), -1 if there is none."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0.0:
            return j
        L[j:, j] = v / np.sqrt(v[0])
    return -1


GRADED_N = (97, 129, 225)
GRADED_E = (3, 6, 9)


@functools.lru_cache(maxsize=None)
def graded_system(n, e):
    """dict(A, b, cond, x_ld, x_np, err_np, bound) -- the reference solutions are computed once here and shared (read-only)."""
    rng = np.random.default_rng([n, e, 7])
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * np.logspace(0, -e, n)) @ Q.T
    A = 0.5 * (A + A.T)
    b = rng.normal(size=n)
    x_ld = reference_solve(A, b)
    x_np = np.linalg.solve(A, b)
    out = dict(A=A, b=b, x_ld=x_ld, x_np=x_np)
    for v in out.values():
        v.setflags(write=False)
    out["cond"] = 10.0 ** e
    out["err_np"] = solve_error(x_np, x_ld)
    out["bound"] = n * 2.0 ** -53 * out["cond"]
    return out


def reference_solve(A, b):
    """A x = b by a column Cholesky and two triangular solves, every operation in np.longdouble; returns x as longdouble."""
    n = A.shape[0]
    A = A.astype(np.longdouble)
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = v / np.sqrt(v[0])
    y = np.zeros(n, dtype=np.longdouble)
    for i in range(n):
        y[i] = (np.longdouble(b[i]) - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve_error(x, x_ld):
    """max |x - x_ld| / max |x_ld|, the difference taken in longdouble."""
    return float(np.abs(np.asarray(x, dtype=np.longdouble) - x_ld).max() / np.abs(x_ld).max())
