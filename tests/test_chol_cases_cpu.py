"""The case builders of tests/chol_cases.py checked on the CPU, for every case tests/test_chol_seams_gpu.py runs: what the GPU tests take
for granted about their inputs -- exact factors, the tile structure the plan is promised, where a broken pivot sits, how good the
long-double reference is -- is asserted here with numpy alone."""
import numpy as np
import pytest

import chol_cases as cc
from chol_cases import NB

# (n, band) of every exact system of the GPU tests
DENSE_N = (2, 30, 31, 32, 33, 64, 65, 95, 96, 97, 128, 129, 160, 161, 193, 225, 256)
BANDED = ((161, 1), (161, 2), (225, 2), (256, 3), (225, 4))
CHAINS = ((288, -3), (320, -3))
PIVOT_SYSTEMS = ((161, 0), (161, 2))
PIVOTS = (0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 144, 159, 160)
LAST_PIVOT = ((32, 0, 31), (64, 0, 63), (160, 0, 159))        # (n, band, p): the matrix ends with the broken pivot
NSEEDS = 8                                                   # two runs of four systems
EXACT = [(n, 0) for n in DENSE_N] + list(BANDED) + list(CHAINS)


@pytest.mark.parametrize("n,band", EXACT)
def test_exact_systems_are_exact_and_keep_to_the_fill(n, band):
    ntc = cc.ntiles(n)
    for seed in range(NSEEDS if (n, band) in PIVOT_SYSTEMS or n in (32, 64, 160) else 4):
        s = cc.exact_system(n, band, seed)
        L, A, fill = s["L"], s["A"], s["fill"]
        assert np.array_equal(A, A.T) and np.array_equal(A, np.round(A)) and np.abs(A).max() <= n
        assert np.array_equal(np.linalg.cholesky(A), L), "numpy's float64 factor is not L itself"
        assert np.abs(s["x0"]).max() <= 3 and np.array_equal(s["b"], A @ s["x0"])
        # unit diagonal, a +-1 first sub-diagonal and nothing else inside a diagonal tile: its inverse is all 0 / +-1
        for i in range(ntc):
            D = L[NB * i:NB * i + NB, NB * i:NB * i + NB]
            m = D.shape[0]
            assert np.array_equal(np.diag(D), np.ones(m)) and np.all(np.abs(np.diag(D, -1)) == 1) and not np.tril(D, -2).any()
            Di = np.linalg.inv(D)
            assert np.array_equal(Di, np.round(Di)) and np.abs(Di).max() == 1
        # A's (and L's) non-zero tiles lie inside the fill; what the plan starts from zero -- every tile outside the fill, the band
        # tiles the one-launch plan adds for its critical workgroup among them -- is zero in A
        for i in range(ntc):
            for j in range(i + 1):
                if not fill[i, j]:
                    assert not A[NB * i:NB * i + NB, NB * j:NB * j + NB].any() and not L[NB * i:NB * i + NB, NB * j:NB * j + NB].any(), (i, j)
                elif i > j:
                    assert L[NB * i:NB * i + NB, NB * j:NB * j + NB].any(), (i, j)       # every tile of the fill carries numbers
        # the intermediates of the two substitutions are small integers as well
        y = L.T @ s["x0"]
        assert np.array_equal(np.linalg.solve(L, s["b"]), y) and np.abs(y).max() <= 3 * n and np.abs(s["b"]).max() <= 3 * n * n


def test_band_cases_hit_the_seams_they_are_named_for():
    """band 1 leaves tiles of the critical workgroup's band (i - j < 3) outside the pattern's fill, band 2 is that band exactly (no far
    tile above the border rows); band 3 and band 4 have far tiles (i - j >= 3) in the fill, band 3 tiles outside it as well; at (225, 4)
    the dense border covers half the block rows and the band the rest; the dissected bands do not couple their first two chains."""
    fill = cc.exact_system(161, 1)["fill"]
    assert any(not fill[i, i - 2] for i in range(2, cc.ntiles(161)))
    for n, band in ((161, 2), (225, 2)):
        fill = cc.exact_system(n, band)["fill"]
        ntc = cc.ntiles(n)
        assert all(fill[i, i - 2] for i in range(2, ntc)) and not any(fill[i, j] for i in range(ntc - band) for j in range(i - 2))
        assert fill[ntc - 1, 0]
    for n, band in ((256, 3), (225, 4)):
        fill = cc.exact_system(n, band)["fill"]
        ntc = cc.ntiles(n)
        assert any(fill[i, i - 3] for i in range(3, ntc)), (n, band)
    assert not np.tril(cc.exact_system(256, 3)["fill"][:8, :8]).all()
    # (225, 4): eight block rows, the last four dense and the first four inside the band -- every tile is there, but named one by one
    # (the plan is handed a pattern and a tile list, not the empty pattern of a dense system)
    assert np.array_equal(cc.tile_pattern(225, 4), np.tril(np.ones((8, 8), dtype=bool)))
    for n, band in CHAINS:
        ntc, b = cc.ntiles(n), -band
        h = (ntc - b) // 2
        assert n % NB == 0 and h >= 3 and ntc - b - h >= 3
        fill = cc.exact_system(n, band)["fill"]
        assert not fill[h:ntc - b, :h].any() and fill[ntc - b:ntc, :ntc - b].any()
    assert (cc.ntiles(320) - 3) // 2 != cc.ntiles(320) - 3 - (cc.ntiles(320) - 3) // 2        # unequal halves


def _pivot_cases():
    for n, band in PIVOT_SYSTEMS:
        for p in PIVOTS:
            yield n, band, p
    yield from LAST_PIVOT


@pytest.mark.parametrize("n,band,p", list(_pivot_cases()))
def test_broken_pivots_break_exactly_there(n, band, p):
    for seed in range(4):                        # (the GPU test breaks system q of a batch: seed q)
        s = cc.exact_system(n, band, seed)
        for kind, want in (("zero", 0.0), ("neg", -1.0)):
            A, _ = cc.broken(s, kind, p)
            if p:
                assert np.array_equal(np.linalg.cholesky(A[:p, :p]), s["L"][:p, :p])
            # pivot p itself, from the untouched factor: A[p, p] - |L[p, :p]|^2
            assert A[p, p] - s["L"][p, :p] @ s["L"][p, :p] == want
            assert cc.first_bad_pivot(A) == p
            with pytest.raises(np.linalg.LinAlgError):
                np.linalg.cholesky(A)
        A, _ = cc.broken(s, "nan_diag", p)
        assert cc.first_bad_pivot(A) == p and np.isnan(A).sum() == 1
        if p:
            assert np.array_equal(np.linalg.cholesky(A[:p, :p]), s["L"][:p, :p])


@pytest.mark.parametrize("n,band", PIVOT_SYSTEMS)
def test_a_nan_in_the_last_far_tile_reaches_a_pivot_in_the_last_diagonal_tile_only(n, band):
    for seed in range(4):
        s = cc.exact_system(n, band, seed)
        A, _ = cc.broken(s, "nan_far")
        ntc = cc.ntiles(n)
        r = NB * (ntc - 1)
        assert s["pattern"][ntc - 1, 0] and np.isnan(A[r, 5]) and np.isnan(np.tril(A)).sum() == 1
        assert cc.first_bad_pivot(A) == r
        assert np.array_equal(np.linalg.cholesky(A[:r, :r]), s["L"][:r, :r])


@pytest.mark.parametrize("n", cc.GRADED_N)
@pytest.mark.parametrize("e", cc.GRADED_E)
def test_graded_systems_and_their_long_double_reference(n, e):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble is no finer than float64 here: the reference would judge nothing"
    g = cc.graded_system(n, e)
    A = g["A"]
    assert np.array_equal(A, A.T)
    w = np.linalg.eigvalsh(A)
    assert abs(w[-1] / w[0] / g["cond"] - 1) < 1e-3          # (cond_2 is what the builder says, to what eigvalsh resolves at 1e9)
    # the reference solves the system 2^11 times finer than float64 could: its residual, taken in long double
    x = g["x_ld"]
    Ald = A.astype(np.longdouble)
    res = np.abs(Ald @ x - g["b"]).max() / (np.abs(Ald).sum(axis=1).max() * np.abs(x).max())
    assert res <= n * 2.0 ** -63
    # numpy's own float64 solve keeps below the condition the GPU test states (n 2^-53 cond_2)
    print("n %d e %d: numpy float64 error %.3g = %.2g of the bound %.3g" % (n, e, g["err_np"], g["err_np"] / g["bound"], g["bound"]))
    assert 0 < g["err_np"] <= g["bound"]
    # ... and the back-substituted solution of the exact-arithmetic identity x = L^-T L^-1 b agrees with float64 numpy to that error,
    # not to the reference's own (which would mean the "reference" is numpy's answer in disguise)
    assert g["err_np"] >= 2.0 ** -60
