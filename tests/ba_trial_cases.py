"""References and cases for the tests of one LM trial step (test_ba_trial_cpu.py, test_ba_trial_gpu.py): pure numpy.

`oplus_reference` is the state after a step, written from the mathematics and not from csrc/ba_device.h or the oracle: closed
forms, no series, no switch between them.  Run in np.longdouble it is the reference; run in float64 it measures the floor a
float64 implementation of the same mathematics cannot go below (`state_error` between the two).

The solver (and TooN, which the reference implementation uses, and the oracle) evaluates the exponential of a small rotation
by truncated series.  Where such a series is truncated ABOVE the float64 rounding level the difference to the closed form is no
rounding error and no tolerance should hide it: `series_allowance` states it, per pose, from the step alone.  Only one
truncation is that large: SE3::exp below theta^2 = 1e-8 takes t + (w x t) / 2 for the translation and drops C w x (w x t),
C = 1/6, which is up to theta^2 / 6 = 1.7e-9 of the step's translation part.  All others stay below 1e-17 (listed there).
"""
import dataclasses
import math

import numpy as np

LD = np.longdouble
TH_SMALL, TH_MID = 1e-8, 1e-6            # theta^2 at which the exponential's implementations switch series (TooN so3.h, se3.h)
DIST_MAX, DIST_MIN = 1e5, 1e-5           # VertexRelPoint::oplusImpl keeps a point's distance inside [1e-5, 1e5]
MARGIN = 1.5                             # every edge case lies at least this factor away from the threshold it straddles

SHAPE_MAPS = ("pts1", "pts63", "pts64", "pts65", "pts129", "shared1_66", "shared2_66", "shared13_66", "roll5", "big_all", "big_one",
              "meas", "calib17")
CHAIN_MAPS = ("chains64", "chains65", "chains128", "chains129")
POSE_MAPS = ("poses255", "poses256", "poses257")
SOLVER_STEP_MAPS = SHAPE_MAPS + CHAIN_MAPS + POSE_MAPS
EDGE_MAPS = ("meas", "shared2_66", "calib17", "shared13_66")          # (shared13_66: 13 free poses, every pose branch)
LAMBDA = 1.0


# ---------------------------------------------------------------------------------------------------------------------
# the reference

def _hat(w, dt):
    z = dt(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=dt)


def exp_coefficients(th2, dt):
    """A = sin t / t, B = 2 sin^2(t / 2) / t^2, C = (1 - A) / t^2 (t = theta); their limits 1, 1/2, 1/6 at theta = 0."""
    if th2 == 0:
        return dt(1), dt(1) / dt(2), dt(1) / dt(6)
    th = np.sqrt(th2)
    A = np.sin(th) / th
    s = np.sin(th / dt(2))
    return A, dt(2) * s * s / th2, (dt(1) - A) / th2


def so3_exp(w, dt):
    """exp of the rotation vector w: I + A [w]x + B [w]x^2."""
    w = np.asarray(w, dtype=dt)
    A, B, _ = exp_coefficients(w @ w, dt)
    K = _hat(w, dt)
    return np.eye(3, dtype=dt) + A * K + B * (K @ K)


def se3_exp(mu, dt):
    """exp of mu = (t, w): rotation exp(w), translation (I + B [w]x + C [w]x^2) t."""
    mu = np.asarray(mu, dtype=dt)
    t, w = mu[:3], mu[3:]
    A, B, C = exp_coefficients(w @ w, dt)
    K = _hat(w, dt)
    K2 = K @ K
    return np.eye(3, dtype=dt) + A * K + B * K2, t + B * (K @ t) + C * (K2 @ t)


def pose_oplus(T12, mu, dt):
    """exp(mu) . T for a pose given as 12 numbers (R row-major, t)."""
    T12 = np.asarray(T12, dtype=dt)
    R, t = T12[:9].reshape(3, 3), T12[9:]
    Re, te = se3_exp(mu, dt)
    return np.concatenate([(Re @ R).reshape(9), Re @ t + te])


def point_oplus_parts(x, u, dt):
    """VertexRelPoint::oplusImpl: the point as bearing and inverse depth.  Rp is the rotation about dir x e_z by asin|dir x e_z|
    (it takes the direction of a point in front of the camera to +z); the bearing is turned by exp(u0, u1, 0) in that frame, the
    inverse depth becomes rho + u2; then the distance is kept inside [1e-5, 1e5].  Returns (new point, distance before the clamps,
    new inverse depth).  A point exactly on its frame's z axis has no such axis (0 / 0): not a case here."""
    x = np.asarray(x, dtype=dt)
    u = np.asarray(u, dtype=dt)
    rho = dt(1) / np.sqrt(x @ x)
    d = x * rho
    ax = np.array([d[1], -d[0], dt(0)], dtype=dt)
    nrm = np.sqrt(ax @ ax)
    ax = ax / nrm * np.arcsin(nrm)
    Rp = so3_exp(ax, dt)
    E = so3_exp(np.array([u[0], u[1], dt(0)], dtype=dt), dt)
    s = rho + u[2]
    o = (Rp.T @ (E @ (Rp @ d))) / s
    dist = np.sqrt(o @ o)
    out = o
    if dist > dt(DIST_MAX):
        out = o * (dt(DIST_MAX) / dist)
    if dist < dt(DIST_MIN):
        out = o * (dt(DIST_MIN) / dist)
    return out, dist, s


def oplus_reference(poses, points, x, dtype=LD):
    """The state after the step x: `poses` (n, 12) are the FREE poses in the order of their unknowns, `points` (m, 3) the free
    points likewise, x = (6 n pose part, 3 m point part).  Returns (poses, points) in `dtype`."""
    poses, points, x = np.asarray(poses), np.asarray(points), np.asarray(x)
    n, m = poses.shape[0], points.shape[0]
    assert x.shape == (6 * n + 3 * m,)
    P = np.array([pose_oplus(poses[i], x[6 * i:6 * i + 6], dtype) for i in range(n)], dtype=dtype).reshape(n, 12)
    X = np.array([point_oplus_parts(points[j], x[6 * n + 3 * j:6 * n + 3 * j + 3], dtype)[0] for j in range(m)], dtype=dtype).reshape(m, 3)
    return P, X


def series_allowance(poses, x):
    """(n, 12) absolute differences between the closed form and the series every implementation of SE3::exp in use here (TooN, the
    oracle, the solver) takes, for the poses of `oplus_reference` -- from the step alone, no implementation consulted.
      theta^2 < 1e-8:  translation t + (w x t) / 2: the term C w x (w x t) is dropped (at most theta^2 / 6 |t|) and B = 1/2
                       is off by theta^2 / 24 (times |w x t|: theta^3 / 24 |t|).  Rotation: A off by theta^4 / 120, B by theta^2 / 24,
                       i.e. theta^5 / 120 + theta^4 / 24 < 5e-18: not allowed for.
      theta^2 < 1e-6:  A, B and C are cut two terms further on: below 1e-18 everywhere.  Not allowed for.
    The allowance is the translation's, on the three translation entries of the pose (exp(mu) T has translation R_e t_T + t_e: the
    rotation of the step is exact to 5e-18, so the difference is that of t_e)."""
    n = np.asarray(poses).shape[0]
    out = np.zeros((n, 12), dtype=LD)
    for i in range(n):
        mu = np.asarray(x[6 * i:6 * i + 6], dtype=LD)
        th2 = mu[3:] @ mu[3:]
        if th2 < LD(TH_SMALL) * (1 + LD(1e-9)):
            th, tn = np.sqrt(th2), np.sqrt(mu[:3] @ mu[:3])
            out[i, 9:] = (th2 / 6 + th * th2 / 24) * tn
    return out


def state_error(a, b, allowance=None):
    """max over the rows (a rotation, a translation, a point) of max_i (|a_i - b_i| - allowance_i) / max(|b_i|, 1e-3 max_row |b|),
    in longdouble: helpers.rel_err_elem applied row by row, so that a point 1e5 away does not set the floor of the others."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    assert a.shape == b.shape and a.ndim == 2
    if a.size == 0:
        return 0.0
    diff = np.abs(a - b)
    if allowance is not None:
        diff = np.maximum(diff - allowance, 0)
    floor = np.maximum(LD(1e-3) * np.abs(b).max(axis=1, keepdims=True), LD(1e-300))
    return float((diff / np.maximum(np.abs(b), floor)).max())


def pose_rows(P):
    """(n, 12) poses -> (2 n, .) rows: the rotations and the translations are judged each on their own scale."""
    P = np.asarray(P)
    return P[:, :9], P[:, 9:]


def pose_error(a, b, allowance=None):
    (Ra, ta), (Rb, tb) = pose_rows(a), pose_rows(b)
    return max(state_error(Ra, Rb), state_error(ta, tb, None if allowance is None else allowance[:, 9:]))


def state_tolerance(F):
    """The one tolerance that is not the project's: 16 times the float64 floor of the reference itself (a few ulps each for the
    device's sin, cos, asin, sqrt and another order of the operations, on values the float64 run rounds as well), at least 64 ulps."""
    return max(16.0 * F, 64.0 * 2.0 ** -53)


# ---------------------------------------------------------------------------------------------------------------------
# where the state of a Problem lies in a bundle

@dataclasses.dataclass
class Layout:
    pose_ids: np.ndarray          # ids of ALL poses in add order (pose k of DebugTrial's `poses` is pose_ids[k])
    free_pose: np.ndarray         # add-order indices of the free poses, in the order of their unknowns (id order)
    fixed_pose: np.ndarray
    free_point: np.ndarray        # indices of the free points (id order = add order)
    fixed_point: np.ndarray
    point_ids: np.ndarray


def layout(p, ids):
    """`ids`: what p.populate(bundle) returned.  Poses and points share one id counter and all poses are added first."""
    fixed = {}
    for k in range(p.n_mkf):
        fixed[int(ids["mkf"][k])] = bool(p.base_fixed[k])
    for c in range(len(p.cams)):
        if int(ids["cam"][c]) > 0:
            fixed[int(ids["cam"][c])] = p.mode != "calib"
    if int(ids["world"]) > 0:
        fixed[int(ids["world"])] = True
    pose_ids = np.array(sorted(fixed), dtype=np.int32)
    assert pose_ids.tolist() == list(range(1, len(pose_ids) + 1))
    free = np.array([i for i, q in enumerate(pose_ids) if not fixed[int(q)]], dtype=np.int64)
    fx = np.array([i for i, q in enumerate(pose_ids) if fixed[int(q)]], dtype=np.int64)
    pf = np.asarray(p.pt_fixed, dtype=bool)
    return Layout(pose_ids, free, fx, np.flatnonzero(~pf), np.flatnonzero(pf), np.asarray(ids["point"], dtype=np.int32))


def current_state(bundle, lay):
    """((npose, 12), (npoint, 3)) of the state the bundle holds (before any Compute(): exactly what was added)."""
    R, t = bundle.GetPoses(lay.pose_ids) if hasattr(bundle, "GetPoses") else _get_poses(bundle, lay.pose_ids)
    X = bundle.GetPoints(lay.point_ids) if hasattr(bundle, "GetPoints") else np.array([bundle.GetPoint(int(i)) for i in lay.point_ids]).reshape(-1, 3)
    return np.concatenate([np.asarray(R).reshape(-1, 9), np.asarray(t).reshape(-1, 3)], axis=1), np.asarray(X).reshape(-1, 3)


def _get_poses(bundle, ids):
    Rt = [bundle.GetPose(int(i)) for i in ids]
    return np.array([a for a, _ in Rt]), np.array([b for _, b in Rt])


def replaced_problem(p, lay, poses, points):
    """The Problem with its state replaced by (poses (npose, 12) in add order, points (npoint, 3)): what populates a second
    bundle with a trial state.  Fixed poses and points keep the Problem's own numbers."""
    ids = p.ids
    where = {int(q): k for k, q in enumerate(lay.pose_ids)}
    poses = np.asarray(poses, dtype=np.float64)
    kw = dict(pt_x=np.where(np.asarray(p.pt_fixed, dtype=bool)[:, None], p.pt_x, np.asarray(points, dtype=np.float64)), ids={})
    if p.mode == "multi":
        bR, bt = p.base_R.copy(), p.base_t.copy()
        for k in range(p.n_mkf):
            if not p.base_fixed[k]:
                T = poses[where[int(ids["mkf"][k])]]
                bR[k], bt[k] = T[:9].reshape(3, 3), T[9:]
        kw.update(base_R=bR, base_t=bt)
    else:
        # calib: a keyframe's pose is cam_R[0] base + cam_t[0] (synth.Problem.populate): give populate a base that reproduces
        # the trial pose bit for bit -- cam 0 as the identity -- and the relative camera poses as they are
        assert p.mode == "calib"
        bR, bt = np.zeros_like(p.base_R), np.zeros_like(p.base_t)
        for k in range(p.n_mkf):
            T = poses[where[int(ids["mkf"][k])]]
            bR[k], bt[k] = T[:9].reshape(3, 3), T[9:]
        cR, ct = p.cam_R.copy(), p.cam_t.copy()
        cR[0], ct[0] = np.eye(3), np.zeros(3)
        rR, rt = p.rel_R.copy(), p.rel_t.copy()
        for c in range(1, len(p.cams)):
            T = poses[where[int(ids["cam"][c])]]
            rR[c], rt[c] = T[:9].reshape(3, 3), T[9:]
        kw.update(base_R=bR, base_t=bt, cam_R=cR, cam_t=ct, rel_R=rR, rel_t=rt)
    q = dataclasses.replace(p, **kw)
    return q


# ---------------------------------------------------------------------------------------------------------------------
# the step at the value edges

POSE_TH2 = (0.0, 0.5e-8, 2e-8, 0.5e-6, 2e-6, 1e-4, 9.0)          # |w|^2 of the pose steps (9.0: |w| = 3)
# (in this order, so that a map with ten free points -- calib17 -- still meets both clamps, the flip and both ends of the series)
POINT_KINDS = ("far_clamped", "near_clamped", "flipped", "far_inside", "near_inside", "zero", "rot<1e-8", "rot>1e-6", "very_far_clamped",
               "very_near_clamped", "rot>1e-8", "rot<1e-6")
_POINT_ROT_TH2 = {"rot<1e-8": 0.5e-8, "rot>1e-8": 2e-8, "rot<1e-6": 0.5e-6, "rot>1e-6": 2e-6}
_POINT_DIST = {"far_inside": 0.5e5, "far_clamped": 2e5, "very_far_clamped": 1e7, "near_inside": 2e-5, "near_clamped": 0.5e-5,
               "very_near_clamped": 1e-8}
DEPTH_KINDS = tuple(_POINT_DIST) + ("flipped",)          # the new inverse depth is a difference of two numbers of the old one's size


def _unit(rng, n):
    v = rng.normal(size=n)
    return v / np.linalg.norm(v)


def edge_step(p, lay, points):
    """A step that walks the value branches of the state update through the free poses and free points of map p (`points`:
    its current points, (npoint, 3)).  Returns (x, pose_th2 per free pose, kind per free point).
    Pose j: rotation part of squared length POSE_TH2[j % 7] (0; either side of 1e-8 and of 1e-6; 1e-4; |w| = 3), translation
    part of length 0.02 to 0.05.  Point j: POINT_KINDS[j % 12] -- no step; a bearing step of squared length either side of both
    thresholds; an inverse-depth step that takes the distance to 0.5e5 (kept), 2e5 and 1e7 (clamped to 1e5), 2e-5 (kept), 0.5e-5 and
    1e-8 (clamped to 1e-5), each with a bearing step of 0.01; and rho + u2 = -rho: the point flips through infinity to the other
    side of its frame.  No point of these maps lies on its frame's z axis (asserted): the update is 0 / 0 there, as in the
    reference's live code (ChainBundle.cc:258-262)."""
    rng = np.random.default_rng([20261020, len(lay.free_pose), len(lay.free_point)])
    nfp, nfl = len(lay.free_pose), len(lay.free_point)
    x = np.zeros(6 * nfp + 3 * nfl)
    th2s, kinds = [], []
    for j in range(nfp):
        th2 = POSE_TH2[j % len(POSE_TH2)]
        x[6 * j:6 * j + 3] = _unit(rng, 3) * rng.uniform(0.02, 0.05)
        x[6 * j + 3:6 * j + 6] = _unit(rng, 3) * math.sqrt(th2)
        th2s.append(th2)
    for j in range(nfl):
        kind = POINT_KINDS[j % len(POINT_KINDS)]
        X = points[lay.free_point[j]]
        assert math.hypot(X[0], X[1]) > 1e-3 * np.linalg.norm(X), "a point on its frame's z axis"
        rho = 1.0 / np.linalg.norm(X)
        u = np.zeros(3)
        if kind in _POINT_ROT_TH2:
            u[:2] = _unit(rng, 2) * math.sqrt(_POINT_ROT_TH2[kind])
            u[2] = 0.01 * rho
        elif kind in _POINT_DIST:
            u[:2] = _unit(rng, 2) * 0.01
            u[2] = 1.0 / _POINT_DIST[kind] - rho
        elif kind == "flipped":
            u[:2] = _unit(rng, 2) * 0.01
            u[2] = -2.0 * rho
        x[6 * nfp + 3 * j:6 * nfp + 3 * j + 3] = u
        kinds.append(kind)
    return x, np.array(th2s), kinds


def assert_edge_branches(poses, points, lay, x, th2s, kinds):
    """On the reference alone: every entry of an edge step takes the branch it is named for, at least a factor 1.5 away from the
    threshold it straddles.  Returns {kind: indices into the free points}."""
    nfp = len(lay.free_pose)
    seen = set()
    for j in range(nfp):
        w = np.asarray(x[6 * j + 3:6 * j + 6], dtype=LD)
        th2 = float(w @ w)
        assert np.linalg.norm(x[6 * j:6 * j + 3]) >= 0.02 * (1 - 1e-12)
        lo = max([t for t in (0.0, TH_SMALL, TH_MID) if t <= th2s[j]])
        hi = min([t for t in (TH_SMALL, TH_MID, math.inf) if t > th2s[j]])
        assert (th2 == 0.0 if th2s[j] == 0.0 else th2 >= MARGIN * lo) and th2 * MARGIN <= hi, (j, th2)
        seen.add((lo, hi))
    assert nfp < 7 or seen == {(0.0, TH_SMALL), (TH_SMALL, TH_MID), (TH_MID, math.inf)}
    by_kind = {}
    for j, kind in enumerate(kinds):
        u = x[6 * nfp + 3 * j:6 * nfp + 3 * j + 3]
        X = points[lay.free_point[j]]
        new, dist, s = point_oplus_parts(X, u, LD)
        dist, s, r2 = float(dist), float(s), float(LD(u[0]) ** 2 + LD(u[1]) ** 2)
        d_new = float(np.sqrt(new @ new))
        if kind == "zero":
            assert r2 == 0.0 and u[2] == 0.0
        elif kind in _POINT_ROT_TH2:
            t = TH_SMALL if "1e-8" in kind else TH_MID
            assert (r2 * MARGIN <= t) if "<" in kind else (r2 >= MARGIN * t), (kind, r2)
        if kind in ("far_clamped", "very_far_clamped"):
            assert dist >= MARGIN * DIST_MAX and abs(d_new - DIST_MAX) <= 1e-15 * DIST_MAX, (kind, dist)
        elif kind in ("near_clamped", "very_near_clamped"):
            assert dist * MARGIN <= DIST_MIN and abs(d_new - DIST_MIN) <= 1e-15 * DIST_MIN, (kind, dist)
        else:
            assert MARGIN * DIST_MIN <= dist and dist * MARGIN <= DIST_MAX and d_new == dist, (kind, dist)      # no clamp
        if kind == "flipped":
            assert s < 0 and float(np.asarray(new, dtype=LD) @ np.asarray(X, dtype=LD)) < 0, kind
        else:
            assert s > 0, (kind, s)
        by_kind.setdefault(kind, []).append(j)
    assert len(kinds) < len(POINT_KINDS) or set(by_kind) == set(POINT_KINDS)
    return by_kind
