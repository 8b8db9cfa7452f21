"""The references of the trial-step tests, held against themselves and against the oracle (no GPU here).

  - the float64 run of ba_trial_cases.oplus_reference against its longdouble run, on every case of test_ba_trial_gpu.py (the
    solver's step, for which the oracle's solution of the same system stands in here, and the value-edge step): the floor F per
    quantity, from which the state tolerance of test_ba_trial_gpu.py is taken -- printed, and the constants there asserted;
  - the branch every entry of the value-edge step takes, on the reference alone;
  - OracleBundle.DebugRhs() against the two solutions of DebugSolve();
  - the oracle's own accepted step against the reference: the reference's oplus is the solver's oplus on an ordinary map."""
import numpy as np
import pytest

import ba_trial_cases as tc
from ba_shapes import get_map, rel_err_2

_CASES = {}


def _orc(p):
    from oracle import OracleBundle
    o = OracleBundle(p.cams, True, True, False)
    ids = p.populate(o)
    return o, tc.layout(p, ids)


def _case(name):
    """(map, layout, current poses, current points, the oracle's x at LAMBDA), once per map."""
    if name not in _CASES:
        p = get_map(name)
        o, lay = _orc(p)
        poses, points = tc.current_state(o, lay)
        rc, xs, xd = o.DebugSolve(tc.LAMBDA)
        assert rc == 0
        _CASES[name] = (p, lay, poses, points, xs, xd, o.DebugRhs())
    return _CASES[name]


def _floors(poses, points, lay, x):
    """(pose floor, point floor per free point) of the float64 run against the longdouble run."""
    P64, X64 = tc.oplus_reference(poses[lay.free_pose], points[lay.free_point], x, np.float64)
    PL, XL = tc.oplus_reference(poses[lay.free_pose], points[lay.free_point], x, tc.LD)
    fx = np.array([tc.state_error(X64[j:j + 1], XL[j:j + 1]) for j in range(len(lay.free_point))])
    return tc.pose_error(P64, PL), fx


def test_longdouble_is_an_extended_format():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_float64_floor_of_the_reference_and_the_tolerances_taken_from_it():
    """F = state_error(oplus_reference in float64, in longdouble), the maximum over all cases, for the poses, for the points, and
    for the points whose new inverse depth is a difference of two numbers of the old one's size (value-edge step only: the point
    is sent to a distance of 1e-8 ... 1e7 or through infinity; the difference loses up to five digits in ANY float64 evaluation,
    which is why those points are judged on their own).  The constants of test_ba_trial_gpu.py must be max(16 F, 64 ulp)."""
    import test_ba_trial_gpu as tg
    F_pose, F_point, F_depth = 0.0, 0.0, 0.0
    for name in tc.SOLVER_STEP_MAPS:
        p, lay, poses, points, xs, _, _ = _case(name)
        fp, fx = _floors(poses, points, lay, xs)
        F_pose, F_point = max(F_pose, fp), max(F_point, fx.max() if fx.size else 0.0)
    for name in tc.EDGE_MAPS:
        p, lay, poses, points = _case(name)[:4]
        x, th2s, kinds = tc.edge_step(p, lay, points)
        fp, fx = _floors(poses, points, lay, x)
        depth = np.array([k in tc.DEPTH_KINDS for k in kinds])
        F_pose = max(F_pose, fp)
        F_point, F_depth = max(F_point, fx[~depth].max()), max(F_depth, fx[depth].max())
    print("float64 floor of the reference: poses %.3e  points %.3e  depth-edge points %.3e" % (F_pose, F_point, F_depth))
    print("state tolerances: poses %.3e  points %.3e  depth-edge points %.3e" % tuple(tc.state_tolerance(F) for F in (F_pose, F_point, F_depth)))
    for F, tol in ((F_pose, tg.TOL_POSE), (F_point, tg.TOL_POINT), (F_depth, tg.TOL_POINT_DEPTH)):
        need = tc.state_tolerance(F)
        assert need <= tol <= 1.5 * need, (F, need, tol)      # (the constant is the measured one, rounded up in its third digit)


@pytest.mark.parametrize("name", tc.EDGE_MAPS)
def test_value_edge_step_takes_the_branches_it_is_named_for(name):
    p, lay, poses, points = _case(name)[:4]
    x, th2s, kinds = tc.edge_step(p, lay, points)
    by_kind = tc.assert_edge_branches(poses, points, lay, x, th2s, kinds)
    assert set(by_kind) == set(tc.POINT_KINDS[:min(len(kinds), 12)]) and len(kinds) >= 10
    if name == "shared13_66":
        assert set(th2s.tolist()) == set(tc.POSE_TH2)          # every pose branch, |w| = 3 included
    # the allowance for the truncated series is confined to the poses below 1e-8, and is at most what the dropped term can be
    al = tc.series_allowance(poses[lay.free_pose], x)
    assert ((al[:, 9:].max(axis=1) > 0) == ((th2s > 0) & (th2s < tc.TH_SMALL))).all() and (al[:, :9] == 0).all()
    assert al.max() <= (1e-8 / 6 + 1e-12 / 24) * 0.05


@pytest.mark.parametrize("name", ["pts65", "meas", "calib17", "big_one", "chains65", "poses256"])
def test_oracle_rhs_is_the_right_hand_side_of_its_two_solutions(name):
    """(H + lambda I) x = b for DebugSolve()'s two solutions and DebugRhs()'s b, to 1e-9 in the 2-norm.  The oracle does not hand out
    H, and a central difference of DebugRhs() gives the derivative of J^T r, which is H only up to the second-order terms the
    Gauss-Newton matrix leaves out -- not to 1e-9.  What is at hand without either:
      - at lambda = 1e20, H x is below 1e-12 of b (|H| < 1e8 on these maps, asserted on S): lambda x = b, all of b, point part
        included, for both solutions;
      - at lambda = 1 the pose part of either solution solves the reduced system DebugSystem() reports, S x_p = rhs, and b's pose
        part is DebugSystem()'s J^T r bit for bit;
      - H is symmetric: with (H + l1 I) x1 = (H + l2 I) x2 = b, x1 . H x2 = x1 . (b - l2 x2) equals x2 . H x1 = x2 . (b - l1 x1)."""
    p = get_map(name)
    o, lay = _orc(p)
    b = o.DebugRhs()
    assert b.shape == (o.Prepare(),) and np.isfinite(b).all() and np.abs(b).max() > 0
    S, rhs, bp = o.DebugSystem(tc.LAMBDA)
    n_p = len(bp)
    assert np.array_equal(b[:n_p], bp)
    assert np.abs(S).max() < 1e8
    rc, xs, xd = o.DebugSolve(1e20)
    assert rc == 0
    for x in (xs, xd):
        assert rel_err_2(1e20 * x, b) < 1e-9, (name, rel_err_2(1e20 * x, b))
    sols = {}
    Sf = np.tril(S) + np.tril(S, -1).T
    for lam in (tc.LAMBDA, 10.0):
        rc, xs, xd = o.DebugSolve(lam)
        assert rc == 0
        if lam == tc.LAMBDA:
            for x in (xs, xd):
                assert rel_err_2(Sf @ x[:n_p], rhs) < 1e-9, (name, rel_err_2(Sf @ x[:n_p], rhs))
        sols[lam] = xd
    (l1, x1), (l2, x2) = sols.items()
    s12, s21 = float(x1 @ (b - l2 * x2)), float(x2 @ (b - l1 * x1))
    assert abs(s12 - s21) <= 1e-9 * max(abs(s12), abs(s21)), (name, s12, s21)
    assert float(x1 @ (b - l1 * x1)) > 0


@pytest.mark.parametrize("name", ["pts65", "meas", "calib17"])
def test_oracle_accepted_iteration_is_the_reference_applied_to_its_own_step(name):
    """Compute(1) of the oracle with a given lambda, accepted at its first trial, leaves oplus_reference(start state, DebugSolve's x
    at that lambda): the reference's oplus is the solver's oplus."""
    p = get_map(name)
    lam = 1.0
    o, lay = _orc(p)
    poses, points = tc.current_state(o, lay)
    rc, xs, _ = o.DebugSolve(lam)
    assert rc == 0
    o2, _ = _orc(p)
    assert o2.Compute(1, lam) == 1
    lg = o2.IterLogs()
    assert len(lg) == 1 and lg[0]["trials"] == 1 and lg[0]["accepted"] == 1, lg
    after_poses, after_points = tc.current_state(o2, lay)
    PL, XL = tc.oplus_reference(poses[lay.free_pose], points[lay.free_point], xs, tc.LD)
    al = tc.series_allowance(poses[lay.free_pose], xs)
    ep, ex = tc.pose_error(after_poses[lay.free_pose], PL, al), tc.state_error(after_points[lay.free_point], XL)
    print("%s: oracle's accepted state against the reference: poses %.2e points %.2e" % (name, ep, ex))
    import test_ba_trial_gpu as tg
    assert ep <= tg.TOL_POSE and ex <= tg.TOL_POINT, (name, ep, ex)
    assert np.array_equal(after_poses[lay.fixed_pose], poses[lay.fixed_pose]) and np.array_equal(after_points[lay.fixed_point], points[lay.fixed_point])
