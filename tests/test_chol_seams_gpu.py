"""The reduced-system Cholesky kernels at their tile, chain and pivot seams: k_chol_step / k_chol_back (ba_chol.h, "step") and
k_chol_persist / k_chol_persist_seg / k_chol_back2 (ba_chol2.h, "one-launch"), through mcp_chol_debug_runs, which hands every system a
matrix of its own and RETURNS the failure flags and the one-launch error words instead of aborting on them.

The inputs come from tests/chol_cases.py (checked on the CPU by tests/test_chol_cases_cpu.py):
  * exact integer systems, whose solution a correct kernel returns bit for bit on both routes -- tile counts 1 .. 8 with the right-hand
    side inside the last tile and in a block row of its own, band + border plans, the smallest plans of three chains;
  * the same systems with ONE pivot made 0, -1 or NaN, at every position where another piece of code raises the flag, in every system
    of a batch of four in turn: the broken system is flagged "not positive definite" and nothing else, its three neighbours come back
    exact, and a second batch of four good systems on the same plan comes back exact with the one-launch plan still in use -- a
    rejected trial must not be taken for a hand-off time-out;
  * graded systems of condition 1e3, 1e6, 1e9 against a long-double reference.

(The exact systems suppose that v_rsq_f64 plus the kernels' third-order correction gives exactly 1 at a pivot of exactly 1.  It does on
the MI355X: every exact case came back at 0 ulp on both routes at its first run, so they are compared with array_equal, not at 4 ulp.)

Each test runs on both routes, chosen as the solver chooses them: MCP_BA_CHOL_PERSIST in the environment when the plan is built.

Conditioning, measured on the MI355X: err(x) = max |x - x_ld| / max |x_ld|, as a multiple of numpy's float64 error on the same system
("step", "one": the two routes against the reference; "s-o": the two routes against each other, same unit).  The kernels multiply by
explicit inverses of the diagonal tiles and sum in MFMA order, so a factor over LAPACK was expected; there is next to none, and none
that grows with the condition number:

     n  e   err(numpy)   step    one    s-o
    97  3    1.38e-14    1.10   0.91   0.56
    97  6    8.56e-12    0.50   1.34   1.56
    97  9    6.81e-09    0.24   0.53   0.56
   129  3    9.70e-15    1.46   1.23   1.32
   129  6    8.69e-12    0.56   0.76   0.90
   129  9    5.90e-09    0.36   0.79   0.45
   225  3    1.69e-14    1.02   1.01   1.12
   225  6    9.57e-12    1.28   1.05   0.76
   225  9    5.65e-09    0.81   0.54   0.51

The largest figure is 1.56; M_RATIO = 4 is the next power of two above twice that."""
import numpy as np
import pytest

import chol_cases as cc

pytestmark = pytest.mark.gpu

M_RATIO = 4.0

DENSE_N = (2, 30, 31, 32, 33, 64, 65, 95, 96, 97, 128, 129, 160, 161, 193, 225, 256)
BANDED = ((161, 1), (161, 2), (225, 2), (256, 3), (225, 4))
CHAINS = (288, 320)
PIVOTS = (0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 144, 159, 160)
# the matrix ENDS with the broken pivot: no later pivot turns NaN and raises the flag in its place, so this is the one position at which
# the check of pivots 17 .. 31 (the follower's on the one-launch route) is the only one that can notice
LAST_PIVOT = ((32, 31), (64, 63), (160, 159))
# route -> (MCP_BA_CHOL_PERSIST, min_ntc of the one-launch plan)
ROUTES = {"step": ("0", 3), "one1": ("1", 1), "one3": ("1", 3)}


def _run(monkeypatch, route, A, b, band=0):
    """A (runs, nsys, n, n), b (runs, nsys, n) through the hook on `route`; on a one-launch route the plan must have been built, must
    still be in use after the last run and no hand-off may have timed out."""
    from mcptam_amd.chain_bundle import chol_debug_runs
    persist, min_ntc = ROUTES[route]
    monkeypatch.setenv("MCP_BA_CHOL_PERSIST", persist)
    x, fail, err, info = chol_debug_runs(np.tril(A), b, band=band, min_ntc=min_ntc)
    assert info[3] == cc.ntiles(A.shape[-1])
    if route == "step":
        assert info[0] == 0 and not err.any()
    else:
        assert info[0] == 1, "the one-launch plan was not built, or was given up"
        assert not err.any(), "a hand-off of the one-launch factorisation timed out: error words %s" % err
    return x, fail, err, info


def _batch(n, band, nsys, first_seed=0):
    s = [cc.exact_system(n, band, first_seed + q) for q in range(nsys)]
    return np.stack([v["A"] for v in s])[None], np.stack([v["b"] for v in s])[None], np.stack([v["x0"] for v in s])[None]


def _routes_for(n):
    return ("step", "one1", "one3") if cc.ntiles(n) >= 3 else ("step", "one1")


# ---- 1. tile counts 1 .. 8, dense ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", [1, 4])
@pytest.mark.parametrize("n", DENSE_N)
def test_dense_exact_systems_at_every_tile_count(gpu_required, monkeypatch, n, nsys):
    """ntc = 1 .. 8, each with the right-hand side inside the last tile and (n % 32 == 0) in a block row of its own; the one-launch plan
    built from one tile on, and from the solver's own threshold of three tiles on."""
    A, b, x0 = _batch(n, 0, nsys)
    for route in _routes_for(n):
        x, fail, _, _ = _run(monkeypatch, route, A, b)
        assert not fail.any(), (route, fail)
        assert np.array_equal(x, x0), (route, np.argwhere(x != x0)[:8])


# ---- 2. band + border ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsys", [1, 3])
@pytest.mark.parametrize("n,band", BANDED)
def test_banded_exact_systems(gpu_required, monkeypatch, n, band, nsys):
    """band 1: tiles of the critical workgroup's band that are not in S (they start from zero); band 2: that band exactly; band 3 and 4:
    the first far tiles, with and without a "pre" partner; (225, 4): every tile there, but handed over as a pattern."""
    A, b, x0 = _batch(n, band, nsys)
    for route in ("step", "one3"):
        x, fail, _, _ = _run(monkeypatch, route, A, b, band=band)
        assert not fail.any(), (route, fail)
        assert np.array_equal(x, x0), (route, np.argwhere(x != x0)[:8])


# ---- 3. chains -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("back_chains", ["1", "0"])
@pytest.mark.parametrize("nsys", [1, 4])
@pytest.mark.parametrize("n", CHAINS)
def test_smallest_chain_plans_exact(gpu_required, monkeypatch, n, nsys, back_chains):
    """k_chol_persist_seg on three chains of three tiles (n = 288: the smallest plan CholPersist::build accepts) and on unequal halves
    (n = 320); the back-substitution with a workgroup per chain and (MCP_BA_CHOL_BACK_CHAINS=0) on one workgroup; two calls, same bytes."""
    A, b, x0 = _batch(n, -3, nsys)
    monkeypatch.setenv("MCP_BA_CHOL_BACK_CHAINS", back_chains)
    x, fail, _, info = _run(monkeypatch, "one3", A, b, band=-3)
    assert info[1] == 3, "the plan was not built as three chains"
    assert not fail.any() and np.array_equal(x, x0), np.argwhere(x != x0)[:8]
    x2, fail2, _, _ = _run(monkeypatch, "one3", A, b, band=-3)
    assert x.tobytes() == x2.tobytes() and not fail2.any()
    xs, fails, _, _ = _run(monkeypatch, "step", A, b, band=-3)
    assert not fails.any() and np.array_equal(xs, x0)


# ---- 4. pivot positions --------------------------------------------------------------------------------------------------------------------
def _pivot_params():
    for n, band in ((161, 0), (161, 2)):
        for p in PIVOTS:
            for kind in ("zero", "neg"):
                yield n, band, p, kind, p % 4
        for p in (16, 160):                     # the broken system at every place of the batch
            for q in range(4):
                if q != p % 4:
                    yield n, band, p, "zero", q
                    yield n, band, p, "neg", q
        for p in (17, 160):
            yield n, band, p, "nan_diag", (p + 1) % 4
        yield n, band, None, "nan_far", 2
    for n, p in LAST_PIVOT:
        for kind in ("zero", "neg", "nan_diag"):
            yield n, 0, p, kind, (p + 2) % 4


@pytest.mark.parametrize("route", ["step", "one"])
@pytest.mark.parametrize("n,band,p,kind,q", list(_pivot_params()))
def test_a_broken_pivot_is_flagged_where_it_is_and_nowhere_else(gpu_required, monkeypatch, route, n, band, p, kind, q):
    """Pivot p of system q of a batch of four is 0, -1 or NaN (nan_far: a NaN in tile (ntc - 1, 0), which reaches a pivot in the last
    diagonal tile).  fail[q] says "not positive definite" (2) and not "hand-off timed out" (4), no error word is raised, the other three
    systems are untouched by it; then four good systems on the SAME plan come back exact and the one-launch plan is still in use."""
    A, b, x0 = _batch(n, band, 4)
    A2, b2, x02 = _batch(n, band, 4, first_seed=4)
    A, b = A.copy(), b.copy()
    A[0, q], b[0, q] = cc.broken(cc.exact_system(n, band, q), kind, p)
    A, b, x0 = np.concatenate([A, A2]), np.concatenate([b, b2]), np.concatenate([x0, x02])
    x, fail, err, info = _run(monkeypatch, "step" if route == "step" else ("one3" if cc.ntiles(n) >= 3 else "one1"), A, b, band=band)
    assert fail[0, q] & 2, "the broken pivot was not flagged: fail %s" % fail[0]
    assert not fail[0, q] & 4 and err[0, q] == 0, "a rejected system taken for a hand-off time-out: fail %s err %s" % (fail[0], err[0])
    others = [r for r in range(4) if r != q]
    assert not fail[0, others].any(), "the flag of system %d leaked: fail %s" % (q, fail[0])
    assert np.array_equal(x[0, others], x0[0, others])
    assert not fail[1].any() and not err[1].any()
    assert np.array_equal(x[1], x0[1]), "the plan does not recover after a rejected system"


# ---- 5. conditioning -----------------------------------------------------------------------------------------------------------------------
def graded_figures(monkeypatch, n, e):
    """(err_step, err_one, |x_step - x_one| / max |x_ld|) of the graded system (n, e), and the system itself."""
    g = cc.graded_system(n, e)
    x = {}
    for route in ("step", "one3"):
        xr, fail, _, _ = _run(monkeypatch, route, g["A"][None, None], g["b"][None, None])
        assert not fail.any(), (route, fail)
        x[route] = xr[0, 0]
    between = float(np.abs(x["step"] - x["one3"]).max() / np.abs(g["x_ld"]).max())
    return cc.solve_error(x["step"], g["x_ld"]), cc.solve_error(x["one3"], g["x_ld"]), between, g


@pytest.mark.parametrize("e", cc.GRADED_E)
@pytest.mark.parametrize("n", cc.GRADED_N)
def test_graded_systems_against_the_long_double_reference(gpu_required, monkeypatch, n, e):
    """Both routes keep the CONDITION err <= n 2^-53 cond_2(A) (numpy's own float64 solve sits at 2e-4 .. 2e-3 of it), and the tight
    assertion: within M_RATIO of numpy's float64 error on the same system, each route against the reference and the two against each
    other (the module docstring has the measured table M_RATIO comes from)."""
    es, eo, between, g = graded_figures(monkeypatch, n, e)
    print("n %d e %d: numpy %.3g  step %.3g (%.2f x)  one-launch %.3g (%.2f x)  step - one-launch %.3g (%.2f x)  bound %.3g"
          % (n, e, g["err_np"], es, es / g["err_np"], eo, eo / g["err_np"], between, between / g["err_np"], g["bound"]))
    assert es <= g["bound"] and eo <= g["bound"]
    assert es <= M_RATIO * g["err_np"] and eo <= M_RATIO * g["err_np"]
    assert between <= M_RATIO * g["err_np"]
