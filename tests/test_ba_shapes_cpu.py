"""The shaped maps of ba_shapes.py are what their designs say, the oracle takes them, and the oracle's own rounding floor on
them lies far below the tolerances test_ba_shapes_gpu.py holds the kernels to (no GPU here)."""
import numpy as np
import pytest

import ba_shapes
from ba_shapes import MAP_NAMES, MEAS_COUNTS, block_scaled_error, get_map, rel_err_2

DESIGNED = [n for n in MAP_NAMES if not n.startswith("calib")]


def _orc(p, robust=True):
    from oracle import OracleBundle
    o = OracleBundle(p.cams, robust, True, False)
    p.populate(o)
    return o


@pytest.mark.parametrize("name", DESIGNED)
def test_map_is_what_its_design_says(name):
    p = get_map(name)
    d = p.design
    assert p.n_points == len(d.points) and p.n_mkf == d.n_mkf and len(p.cams) == d.n_cams
    assert p.base_fixed[0] and not p.base_fixed[1:].any()
    assert p.n_meas == sum(len(pt.obs) for pt in d.points)
    for i, pt in enumerate(d.points):
        ms = np.flatnonzero(p.ms_pt == i)
        assert sorted(zip(p.ms_mkf[ms].tolist(), p.ms_cam[ms].tolist())) == sorted(pt.obs), (name, i)
        assert bool(p.pt_fixed[i]) == pt.fixed and tuple(p.pt_src[i]) == tuple(pt.src)
        assert ba_shapes.problem_poses(p, i) == ba_shapes.design_poses(d, pt), (name, i)


def _pose_counts(p):
    return [len(ba_shapes.problem_poses(p, i)) for i in range(p.n_points)]


@pytest.mark.parametrize("n", ba_shapes.POINT_SEAMS)
def test_point_count_seams(n):
    p = get_map("pts%d" % n)
    assert p.n_points == n and all(ba_shapes.problem_poses(p, i) == set(range(1, 7)) for i in range(n))


@pytest.mark.parametrize("k", ba_shapes.POSE_SEAMS)
@pytest.mark.parametrize("n", [66, 130])
def test_shared_pose_sets(k, n):
    p = get_map("shared%d_%d" % (k, n))
    assert p.n_points == n and all(ba_shapes.problem_poses(p, i) == set(range(1, k + 1)) for i in range(n))
    if k >= 2:      # both kinds of source: the fixed keyframe and a free one (whose own measurement has no free slot)
        assert (p.pt_src[:, 0] == 0).any() and (p.pt_src[:, 0] > 0).any()
    assert ((p.ms_mkf == 0)).any()


@pytest.mark.parametrize("k", [5, 13])
def test_rolling_pose_sets(k):
    p = get_map("roll%d" % k)
    assert p.n_points == 66 and p.n_mkf == 67
    for i in range(66):
        assert ba_shapes.problem_poses(p, i) == {1 + (i + j) % 66 for j in range(k)}


def test_big_point_maps():
    assert _pose_counts(get_map("big_all")) == [17] * 20
    assert _pose_counts(get_map("big_mixed")) == [17 if i % 2 else 6 for i in range(40)]
    assert _pose_counts(get_map("big_one")) == [17 if i == 10 else 6 for i in range(33)]


def test_measurement_count_map_holds_every_count_of_every_kind():
    p = get_map("meas")
    per = np.bincount(p.ms_pt, minlength=p.n_points)
    free = ~p.base_fixed
    seen = set()
    for i in range(p.n_points):
        kind = ba_shapes.MEAS_KINDS[(i // 8) % 6]
        assert per[i] == MEAS_COUNTS[i % 8]
        ms = np.flatnonzero(p.ms_pt == i)
        obs_free = free[p.ms_mkf[ms]]
        npose = len(ba_shapes.problem_poses(p, i))
        if kind == "own_source_only":
            assert not p.pt_fixed[i] and free[p.pt_src[i, 0]] and (p.ms_mkf[ms] == p.pt_src[i, 0]).all() and npose == 0
        elif kind == "fixed_keyframe_only":
            assert not p.pt_fixed[i] and not obs_free.any() and npose == 0
        elif kind == "fixed_point":
            assert p.pt_fixed[i] and obs_free.all() and npose == len(set(p.ms_mkf[ms].tolist()))
        elif kind == "fixed_point_fixed_only":
            assert p.pt_fixed[i] and not obs_free.any() and npose == 0
        elif kind == "regular_free_src":
            assert not p.pt_fixed[i] and free[p.pt_src[i, 0]] and (p.ms_mkf[ms] == p.pt_src[i, 0]).any()
        else:
            assert not p.pt_fixed[i] and p.pt_src[i, 0] == 0 and obs_free.all() and npose == min(per[i], 6)
        seen.add((kind, int(per[i])))
    assert seen == {(k, n) for k in ba_shapes.MEAS_KINDS for n in MEAS_COUNTS}


def test_ten_camera_rig_uses_the_cameras_beyond_the_eighth():
    p = get_map("tencam")
    assert len(p.cams) == 10
    used = np.bincount(p.ms_cam, minlength=10)
    assert (used > 0).all() and used[8] >= 1 and used[9] >= 1
    assert set(p.pt_src[:, 1].tolist()) >= {8, 9}          # ... also as the camera a point is expressed in


@pytest.mark.parametrize("n", [17, 65])
def test_calibration_map_cut_to_a_seam(n):
    p = get_map("calib%d" % n)
    assert p.mode == "calib" and p.n_points == n
    assert set(p.ms_mkf.tolist()) == set(range(p.n_mkf)) and set(p.ms_cam.tolist()) == set(range(len(p.cams)))
    assert p.pt_fixed.any() and not p.pt_fixed.all()
    assert (p.ms_cam > 0).any()          # the relative pose as second link of the observer chain


@pytest.mark.parametrize("name", MAP_NAMES)
def test_oracle_takes_the_map_and_its_rounding_floor_is_far_below_the_tolerances(name):
    """The GPU tests ask 1e-10 (S, scaled per block) and 1e-9 (rhs, J^T r) against the oracle.  The oracle built twice, the second
    time with the measurements in another order, differs from itself by less than 1e-12: the tolerances sit a hundred times above
    what the reference does to itself."""
    p = get_map(name)
    for robust in ((True, False) if name == "meas" else (True,)):
        a, b = _orc(p, robust), _orc(ba_shapes.permuted(p), robust)
        assert a.Prepare() == b.Prepare() > 0
        for lam in (1e-6, 1e-2, 10.0):
            Sa, ra, ba = a.DebugSystem(lam)
            Sb, rb, bb = b.DebugSystem(lam)
            assert np.isfinite(Sa).all() and np.isfinite(ra).all()
            assert block_scaled_error(Sb, Sa) < 1e-12, (name, lam, block_scaled_error(Sb, Sa))
            assert rel_err_2(rb, ra) < 1e-12 and rel_err_2(bb, ba) < 1e-12, (name, lam, rel_err_2(rb, ra), rel_err_2(bb, ba))
        S = np.tril(Sa) + np.tril(Sa, -1).T          # (the last one, lambda = 10)
        assert np.linalg.eigvalsh(S).min() > 0, name
        rc, xs, xd = a.DebugSolve(1.0)
        assert rc == 0 and np.isfinite(xs).all()
