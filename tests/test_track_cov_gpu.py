"""The tracker's pose covariance on the GPU (include/mcp_img.h: mcp_track_pose_cov, mcp_track_pose_cov_enable, mcp_track_pose_cov_last).
The standalone entry against the host entry (the same source under the host compiler, in the same order) at the seams of the wavefront
(64) and of the tile (256), bit-identical over runs and grids; the one-call frames with the switch on against twin tables with it off
(every existing output bit-identical), their record against the standalone entry fed the call's own fine records (bit for bit) and against
the numpy restatement built from the call's items, the table's positions and the CPU oracle's camera derivatives.

Bounds: those of tests/test_track_cov_cpu.py -- info 1e-9 norm-wise, cov 64 kappa 2^-52 against numpy's truncated pseudo-inverse of the
returned info.

Measured on an MI355X: device info and cov equal the host entry's bit for bit at every n (largest difference 0); the one-call record against
the restatement max|info - restatement| / max|info| = 1.2e-16; |cov - numpy pinv|_F / |cov|_F at most 0.85 kappa 2^-52."""
import numpy as np
import pytest

from track_cov_cases import check_against_numpy, check_nan, check_rank2, make_records, nan_case, rank2_case

pytestmark = pytest.mark.gpu

QUALITY = dict(min_patches=10, quality_coarse_min=20, quality_good=0.3, quality_bad=0.13)
PRM = dict(try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=10, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=12345)
V0 = np.array([0.05, -0.03, 0.02, 0.004, -0.003, 0.002])
DT = 0.04


def _info_diff(a, b):
    from mcptam_amd.pvs import pose_cov_arrays
    ia, ib = pose_cov_arrays(a)[0], pose_cov_arrays(b)[0]
    return np.abs(ia - ib).max() / np.abs(ia).max()


# ---- the standalone entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_device_is_the_host_entry(gpu_required, n):
    from mcptam_amd.pvs import pose_cov, pose_cov_arrays, pose_cov_host
    pts, w, cfbs, refined, mu = make_records(n, 4, 40 + n)
    dev = pose_cov(pts, w, cfbs, refined, mu)
    host = pose_cov_host(pts, w, cfbs, refined, mu)
    d = _info_diff(dev, host)
    dc = np.linalg.norm(pose_cov_arrays(dev)[1] - pose_cov_arrays(host)[1]) / np.linalg.norm(pose_cov_arrays(host)[1])
    print("n %d: n_used %d  max|info_dev - info_host| / max|info| = %.3g  |cov_dev - cov_host|_F / |cov|_F = %.3g  sweeps %d / %d" %
          (n, dev.n_used, d, dc, dev.sweeps, host.sweeps))
    assert dev.valid == 1 and dev.n_used == host.n_used == int(((pts["found"] != 0) & (w != 0)).sum())
    assert d <= 1e-9
    check_against_numpy(dev, "n %d device:" % n)
    again = pose_cov(pts, w, cfbs, refined, mu)
    assert bytes(again) == bytes(dev)
    if n == 0:
        assert np.array_equal(pose_cov_arrays(dev)[1], 0.01 * np.eye(6)) and dev.sweeps == 0 and dev.rank == 6
    if n == 1000:
        for wg in (1, 2, 3, 0):
            assert bytes(pose_cov(pts, w, cfbs, refined, mu, max_workgroups=wg)) == bytes(dev), wg


def test_device_edge_cases_end_with_the_documented_records(gpu_required):
    from mcptam_amd.pvs import pose_cov
    check_nan(pose_cov(*nan_case()))
    check_rank2(pose_cov(*rank2_case()))


# ---- the one-call frames -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(gpu_required):
    """The scene of tests/test_track_record_gpu.py: four cameras, one looking away, about 4 % unusable and 2 % fixed rows, counts 1-30 / 0-30."""
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame, make_lite_batch
    from mcptam_amd.synth import so3_exp
    from mcptam_amd.taylor_camera import TaylorCamera
    sc = synth_img.make_tracking_scene()
    src = KeyFrame(640, 480)
    src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
    pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"])
    wp, pr, pd = synth_img.points_soa(pts)
    n = len(pts)
    rng = np.random.default_rng(5)
    cfbs = [(np.eye(3), np.zeros(3)), (so3_exp(np.array([0.0, 0.12, 0.0])), np.array([0.05, 0.0, 0.0])),
            (so3_exp(np.array([0.0, np.pi, 0.0])), np.zeros(3)),                # looks away: an empty PVS
            (so3_exp(np.array([0.08, 0.0, 0.0])), np.array([0.0, 0.03, 0.01]))]
    targets = [KeyFrame(640, 480) for _ in range(4)]
    make_lite_batch(targets, [sc["imgB"]] * 4)
    cols = dict(wp=wp, pr=pr, pd=pd, usable=(rng.random(n) >= 0.04).astype(np.uint8), keys=np.arange(n, dtype=np.int32) * 3 + 7,
                src=[src] * n, level=np.array([p["source_level"] for p in pts], dtype=np.int32),
                center=np.array([p["center"] for p in pts], dtype=np.int32), fixed=(rng.random(n) < 0.02).astype(np.uint8))
    crng = np.random.default_rng(77)
    cols["inl"] = crng.integers(1, 31, n).astype(np.int32)
    cols["outl"] = crng.integers(0, 31, n).astype(np.int32)
    R, t = sc["poseB"]
    prior = (so3_exp(np.array([0.012, -0.006, 0.009])) @ R, t + np.array([0.01, -0.006, 0.004]))
    return dict(sc=sc, cam=sc["cam"], cam_sbi=TaylorCamera(sc["cam"].params, (640, 480), (640, 480), (40, 30)), src=src, cols=cols, cfbs=cfbs, targets=targets,
                prior=prior, n=n)


def _table(cols, on):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    if cols is not None:
        t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
        t.set_source(cols["keys"], cols["src"], cols["level"], cols["center"], cols["fixed"])
        t.set_counts(cols["inl"], cols["outl"])
    if on:
        t.pose_cov_enable(True)
    return t


def _record(t, w):
    return t.track_map_record(w["targets"], [w["cam"]] * 4, w["prior"], w["cfbs"], **QUALITY, **PRM)


def _motion(t, w, start):
    return t.track_frame_motion(w["targets"], [w["cam"]] * 4, [w["cam_sbi"]] * 4, start, w["cfbs"], velocity=V0, dt=DT, apply=True, **QUALITY, **PRM)


def _same_items(a, b):
    if len(a) != len(b):
        return False
    for f in ("point", "stage", "weight_last"):
        if not np.array_equal(a[f], b[f]):
            return False
    return all(np.array_equal(a["out"][f], b["out"][f], equal_nan=a["out"][f].dtype.kind == "f") for f in a["out"].dtype.names)


def _assert_same_outputs(off, on, T_off, T_on, ncam=4):
    """items, pose, res, notes, measurements, record (and the motion report) of the two calls, the count columns and the finders' states."""
    assert np.array_equal(off[1][0], on[1][0]) and np.array_equal(off[1][1], on[1][1])
    assert bytes(off[2]) == bytes(on[2]) and bytes(off[5]) == bytes(on[5])
    for c in range(ncam):
        assert _same_items(off[0][c], on[0][c]), c
        assert off[3][c].tobytes() == on[3][c].tobytes() and off[4][c].tobytes() == on[4][c].tobytes(), c
        assert T_off.get_states(c).tobytes() == T_on.get_states(c).tobytes(), c
    for extra in range(6, len(off)):
        if hasattr(off[extra], "_fields_"):
            assert bytes(off[extra]) == bytes(on[extra]), extra
    if T_off.rows:
        a, b = T_off.get_counts(), T_on.get_counts()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _assert_cov_of_call(w, T, out, tag):
    """The record of the call on T: the standalone entry's bits on the call's own fine records; the numpy restatement from the items, the
    table's positions and the oracle's camera derivatives at the rebuilt pose; n_used == n_inliers."""
    from mcptam_amd.keyframe import POSE_POINT_DTYPE
    from mcptam_amd.pvs import pose_cov, pose_cov_arrays, pose_covariance_restate, se3_exp
    from oracle import cam_project
    items, pose, res, rec = out[0], out[1], out[2], out[5]
    last = T.pose_cov_last()
    recs, wts, mu = T.debug_fine_records()
    assert np.array_equal(mu, np.array(res.mu_last)) and len(recs) == sum(len(i) for i in items)
    again = pose_cov(recs, wts, w["cfbs"], pose, mu)
    assert bytes(again) == bytes(last)
    assert last.valid == 1 and last.n_used == rec.n_inliers and last.n_used > 100
    # the restatement: one record per item, derivatives from the oracle at the pose the last iteration linearised at
    Re, te = se3_exp(-mu)
    before = (Re @ pose[0], Re @ pose[1] + te)
    parts = []
    for c in range(4):
        it = items[c]
        p = np.zeros(len(it), dtype=POSE_POINT_DTYPE)
        p["world_pos"] = w["cols"]["wp"][it["point"]]
        p["sqrt_inv_noise"], p["found"], p["cam"] = it["out"]["sqrt_inv_noise"], it["out"]["found"], c
        Rc, tc = w["cfbs"][c]
        for k in np.nonzero((it["out"]["found"] != 0) & (it["weight_last"] != 0))[0]:
            p["cam_derivs"][k] = cam_project(w["cam"], Rc @ (before[0] @ p["world_pos"][k] + before[1]) + tc)[1].reshape(4)
        parts.append(p)
    ref = pose_covariance_restate(np.concatenate(parts), np.concatenate([i["weight_last"] for i in items]), w["cfbs"], pose, mu, pose_before=before)
    d = np.abs(pose_cov_arrays(last)[0] - ref["info"]).max() / np.abs(ref["info"]).max()
    print(tag, "n_used %d  max|info - restatement| / max|info| = %.3g  norm_fro %.3g  sweeps %d" % (last.n_used, d, last.norm_fro, last.sweeps))
    assert ref["n_used"] == last.n_used
    assert d <= 1e-9
    check_against_numpy(last, tag)
    return last


@pytest.fixture(scope="module")
def runs(world):
    w = world
    off, on = _table(w["cols"], False), _table(w["cols"], True)
    return dict(off=off, on=on, a=_record(off, w), b=_record(on, w))


def test_switch_on_changes_no_existing_output(world, runs):
    _assert_same_outputs(runs["a"], runs["b"], runs["off"], runs["on"])
    assert sum(len(i) for i in runs["b"][0]) > 500


def test_one_call_record_is_the_standalone_entry_and_the_restatement(world, runs):
    _assert_cov_of_call(world, runs["on"], runs["b"], "track_map_record:")


def test_last_is_refused_with_the_switch_off(world, runs):
    from mcptam_amd import chain_bundle
    with pytest.raises(RuntimeError):
        runs["off"].pose_cov_last()
    assert "mcp_track_pose_cov_enable" in chain_bundle.last_error()
    # ... and on a table that had it on, after a call with it off
    w = world
    T = _table(w["cols"], True)
    _record(T, w)
    assert T.pose_cov_last().valid == 1
    T.pose_cov_enable(False)
    _record(T, w)
    with pytest.raises(RuntimeError):
        T.pose_cov_last()


def test_through_the_motion_frame(world, runs):
    w = world
    off, on = _table(w["cols"], False), _table(w["cols"], True)
    a, b = _motion(off, w, w["prior"]), _motion(on, w, w["prior"])
    _assert_same_outputs(a, b, off, on)
    assert np.array(b[6].v_new).any()
    _assert_cov_of_call(w, on, b, "track_frame_motion:")


def test_nobody_recovers_leaves_valid_zero(world):
    from mcptam_amd.synth import so3_exp
    w = world
    lost = (so3_exp(np.array([0.5, -0.4, 0.3])) @ w["sc"]["poseA"][0], w["sc"]["poseA"][1] + np.array([0.7, -0.5, 0.9]))
    outs = []
    for on in (False, True):
        T = _table(w["cols"], on)
        out = T.track_frame_recover(w["targets"], [w["cam"]] * 4, [w["cam_sbi"]] * 4, lost, w["cfbs"], [], [], np.zeros((0, 12)), velocity=V0, lost=True,
                                    **QUALITY, **PRM)
        outs.append((T, out))
    (T_off, a), (T_on, b) = outs
    assert b[7].recovered == 0 and b[7].cam == -1
    _assert_same_outputs(a, b, T_off, T_on)
    last = T_on.pose_cov_last()
    assert last.valid == 0 and not any(bytes(last))
    recs, wts, mu = T_on.debug_fine_records()
    assert len(recs) == 0 and not mu.any()


def test_empty_table(world):
    from mcptam_amd.pvs import pose_cov_arrays
    w = world
    off, on = _table(None, False), _table(None, True)
    a, b = _record(off, w), _record(on, w)
    _assert_same_outputs(a, b, off, on)
    last = on.pose_cov_last()
    info, cov, eig = pose_cov_arrays(last)
    assert last.valid == 1 and last.n_used == 0 == b[5].n_inliers and last.rank == 6 and last.sweeps == 0
    assert np.array_equal(info, 100.0 * np.eye(6)) and np.array_equal(cov, 0.01 * np.eye(6))
    recs, wts, mu = on.debug_fine_records()
    assert len(recs) == 0
