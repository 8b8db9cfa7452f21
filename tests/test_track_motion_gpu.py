"""mcp_track_frame_motion (include/mcp_img.h): TrackFrame's tracking branch in one submission -- the tracker's SmallBlurryImages, the SBI
rotation estimate and ApplyMotionModel on the device, mcp_track_map_record from the prior they give, UpdateMotionModel behind it.  The scene is
tests/test_track_record_gpu.py's (four 640x480 cameras, imgA then imgB as two consecutive frames).  Table B runs the new call; its SBIs and
alignments must carry the bits of mcp_kf_make_sbi / mcp_sbi_iterate on twin keyframes, its prior and velocity must be the host entries' (the
same source under the host compiler) to 1e-9, and everything downstream must equal, bit for bit, what table A gets from
mcp_kf_make_lite_batch + mcp_track_map_record started at B's prior.

Measured on an MI355X: largest |prior - mcp_track_motion_prior_host| = 0 and largest |velocity - mcp_track_motion_update_host| = 0 over every frame of
this file (the bound is 1e-9: host and device differ only in their math libraries, which agreed on these inputs)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = 4
QUALITY = dict(min_patches=10, quality_coarse_min=20, quality_good=0.3, quality_bad=0.13)
PRM = dict(try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=10, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=12345)
DT = 0.04
V0 = np.array([0.05, -0.03, 0.02, 0.004, -0.003, 0.002])          # mv6BaseVelocity before the first frame
GOOD = [1, 1, 0, 1]                                                # camera 2 looks away: never GOOD


@pytest.fixture(scope="module")
def world(gpu_required):
    """The scene and columns of tests/test_track_record_gpu.py, plus the 40x30 camera and twin keyframes that hold imgA / imgB with the
    tracker's SBI (blur 0.75) made by mcp_kf_make_sbi."""
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame, sbi_iterate
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
    cols = dict(wp=wp, pr=pr, pd=pd, usable=(rng.random(n) >= 0.04).astype(np.uint8), keys=np.arange(n, dtype=np.int32) * 3 + 7,
                src=[src] * n, level=np.array([p["source_level"] for p in pts], dtype=np.int32),
                center=np.array([p["center"] for p in pts], dtype=np.int32), fixed=(rng.random(n) < 0.02).astype(np.uint8))
    crng = np.random.default_rng(77)
    cols["inl"] = crng.integers(1, 31, n).astype(np.int32)
    cols["outl"] = crng.integers(0, 31, n).astype(np.int32)
    R, t = sc["poseA"]
    start = (so3_exp(np.array([0.002, -0.001, 0.0015])) @ R, t + np.array([0.004, -0.002, 0.003]))      # last frame's pose, near poseA
    twin = {}
    for name in ("imgA", "imgB"):
        k = KeyFrame(640, 480)
        k.MakeKeyFrame_Lite(sc[name]); k.MakeSBI(0.75)
        twin[name] = k
    align = {}
    for cur, last in (("imgB", "imgA"), ("imgA", "imgB")):
        R2, t2, score = sbi_iterate(twin[cur], twin[last], 6)
        align[cur] = (np.concatenate([R2.ravel(), t2]), score)
    return dict(sc=sc, cam=sc["cam"], cam_sbi=TaylorCamera(sc["cam"].params, (640, 480), (640, 480), (40, 30)), src=src, cols=cols, cfbs=cfbs, start=start, n=n,
                twin=twin, sbi={k: [a.tobytes() for a in v.SBI()] for k, v in twin.items()}, align=align)


def _table(cols):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], cols["src"], cols["level"], cols["center"], cols["fixed"])
    t.set_counts(cols["inl"], cols["outl"])
    return t


def _targets(n=4):
    from mcptam_amd.keyframe import KeyFrame
    return [KeyFrame(640, 480) for _ in range(n)]


def _same_items(a, b):
    """Field by field (numpy copies of structured arrays leave their padding bytes undefined)."""
    if len(a) != len(b):
        return False
    for f in ("point", "stage", "weight_last"):
        if not np.array_equal(a[f], b[f]):
            return False
    return all(np.array_equal(a["out"][f], b["out"][f], equal_nan=a["out"][f].dtype.kind == "f") for f in a["out"].dtype.names)


def _same_result(ra, rb, ncam):
    assert ra.did_coarse == rb.did_coarse and ra.coarse_found == rb.coarse_found
    assert np.array_equal(np.array(ra.mu_last), np.array(rb.mu_last))
    for c in range(ncam):
        assert list(ra.pvs_counts[c]) == list(rb.pvs_counts[c]) and list(ra.set_sizes[c]) == list(rb.set_sizes[c]) and ra.stale[c] == rb.stale[c], c


def _pvs_views(t, ncam):
    from mcptam_amd.pvs import PVS_ENTRY_DTYPE
    out = []
    for c in range(ncam):
        for l in range(LEVELS):
            cnt = ctypes.c_int(0)
            ptr = t._L.mcp_track_find_pvs_view(t._h, c, l, ctypes.byref(cnt))
            out.append(np.frombuffer((ctypes.c_char * (cnt.value * PVS_ENTRY_DTYPE.itemsize)).from_address(ptr), dtype=PVS_ENTRY_DTYPE).tobytes() if cnt.value else b"")
    return out


def _sbis(t, ncam):
    return [[[a.tobytes() for a in t.motion_sbi(c, which)] for which in (0, 1)] for c in range(ncam)]


def _snapshot(t, out, ncam, rows=True):
    """Everything a frame call leaves behind, as comparable values."""
    items, pose, res, notes, meas, rec = out[:6]
    return dict(items=items, pose=pose, res=res, notes=[x.tobytes() for x in notes], meas=[x.tobytes() for x in meas], rec=bytes(rec),
                states=[t.get_states(c).tobytes() for c in range(ncam)] if rows else [], pvs=_pvs_views(t, ncam), counts=[a.tobytes() for a in t.get_counts()],
                motion=bytes(out[6]) if len(out) > 6 else None, mo=out[6] if len(out) > 6 else None, sbis=_sbis(t, ncam) if len(out) > 6 else None)


def _assert_same_downstream(a, b, ncam):
    """Table A (mcp_kf_make_lite_batch + mcp_track_map_record at B's prior) against table B (the one call): bit for bit."""
    assert np.array_equal(a["pose"][0], b["pose"][0]) and np.array_equal(a["pose"][1], b["pose"][1])
    _same_result(a["res"], b["res"], ncam)
    for c in range(ncam):
        assert _same_items(a["items"][c], b["items"][c]), c
        assert a["states"][c] == b["states"][c], c
        assert a["notes"][c] == b["notes"][c] and a["meas"][c] == b["meas"][c], c
    assert a["pvs"] == b["pvs"] and a["rec"] == b["rec"] and a["counts"] == b["counts"]


def _motion_frame(t, w, targets, img, start, velocity, cfbs=None, good=None, **kw):
    n = len(targets)
    cfbs = (cfbs or w["cfbs"])[:n]
    return t.track_frame_motion(targets, [w["cam"]] * n, [w["cam_sbi"]] * n, start, cfbs, velocity=velocity, dt=DT, cam_good=(GOOD if good is None else good)[:n],
                                imgs=[img] * n, **dict(QUALITY, **kw), **PRM)


def _record_frame(t, w, targets, img, prior, cfbs=None):
    """The split sequence's tail: the pyramids, then mcp_track_map_record with imgs = NULL from the given prior."""
    from mcptam_amd.keyframe import make_lite_batch
    cfbs = (cfbs or w["cfbs"])[:len(targets)]
    make_lite_batch(targets, [img] * len(targets))
    return t.track_map_record(targets, [w["cam"]] * len(targets), prior, cfbs, **QUALITY, **PRM)


def _pose_of(v12):
    v = np.array(v12)
    return v[:9].reshape(3, 3).copy(), v[9:].copy()


def _two_frames(w, ncam=4, cfbs=None, good=None, cols=None, twin_table=True):
    """imgA then imgB through the new call on table B with fresh targets; table A follows with the split sequence from B's priors.  Returns
    the snapshots [(a1, b1), (a2, b2)] and the tables / targets."""
    cols = w["cols"] if cols is None else cols
    B, tb = _table(cols) if cols else _empty_table(), _targets(ncam)
    A, ta = (_table(cols) if cols else _empty_table(), _targets(ncam)) if twin_table else (None, None)
    out, start, vel = [], w["start"], V0
    for img in ("imgA", "imgB"):
        b = _motion_frame(B, w, tb, w["sc"][img], start, vel, cfbs, good)
        sb = _snapshot(B, b, ncam, rows=bool(cols))
        sa = None
        if twin_table:
            sa = _snapshot(A, _record_frame(A, w, ta, w["sc"][img], _pose_of(b[6].prior), cfbs), ncam, rows=bool(cols))
        out.append((sa, sb, start, vel))
        start, vel = b[1], np.array(b[6].velocity)
    return dict(frames=out, A=A, B=B, ta=ta, tb=tb, start=start, vel=vel)


def _empty_table():
    from mcptam_amd.pvs import MapPointTable
    return MapPointTable()


def _assert_motion_is_host(w, mo, start, vel, refined, ncam, cfbs=None, good=None, apply=True, worst=None):
    """prior / cam_rot / sbi_rot against mcp_track_motion_prior_host fed the returned se2, velocity against mcp_track_motion_update_host: 1e-9."""
    from mcptam_amd.keyframe import _pose12
    from mcptam_amd.pvs import motion_params, motion_prior_host, motion_update_host
    cfbs = cfbs or w["cfbs"]
    mp = motion_params(vel, DT, (GOOD if good is None else good)[:ncam], apply=apply, ncam=ncam)
    se2 = np.array([list(mo.se2[c]) for c in range(ncam)])
    host = motion_prior_host(se2, [w["cam_sbi"]] * ncam, np.array([_pose12(*c) for c in cfbs[:ncam]]), _pose12(*start), mp)
    assert np.array_equal(np.array(mo.start), _pose12(*start))
    dp = max(np.abs(np.array(mo.prior) - np.array(host.prior)).max(), np.abs(np.array(mo.sbi_rot) - np.array(host.sbi_rot)).max(),
             max(np.abs(np.array(mo.cam_rot[c]) - np.array(host.cam_rot[c])).max() for c in range(8)))
    v_new, v_out = motion_update_host(_pose12(*start), _pose12(*refined), mp)
    dv = max(np.abs(np.array(mo.v_new) - v_new).max(), np.abs(np.array(mo.velocity) - v_out).max())
    print("largest |prior - host| %.3g, largest |velocity - host| %.3g, n_used %d, rounds %d" % (dp, dv, mo.n_used, mo.avg_rounds))
    if worst is not None:
        worst[0], worst[1] = max(worst[0], dp), max(worst[1], dv)
    assert dp <= 1e-9 and dv <= 1e-9
    assert mo.n_used == host.n_used and 0 <= mo.avg_rounds <= 32 and (mo.avg_rounds > 0) == (mo.n_used > 0)


@pytest.fixture(scope="module")
def baseline(world):
    """mcp_track_map_record on a fresh table before mcp_track_frame_motion has ever run in this module."""
    w = world
    return _snapshot(*_baseline_run(w), 4)


def _baseline_run(w):
    T, tg = _table(w["cols"]), _targets()
    return T, _record_frame(T, w, tg, w["sc"]["imgB"], w["start"])


@pytest.fixture(scope="module")
def runs(world, baseline):
    return _two_frames(world)


def test_sbi_bits_are_make_sbis(world, runs):
    """this / last of every camera index against mcp_kf_make_sbi(0.75) + mcp_kf_get_sbi on twin keyframes, byte for byte."""
    w = world
    (_, b1, _, _), (_, b2, _, _) = runs["frames"]
    for c in range(4):
        assert b1["sbis"][c][0] == w["sbi"]["imgA"] and b1["sbis"][c][1] == w["sbi"]["imgA"], c       # first frame: last equals this
        assert b1["mo"].first_frame[c] == 1 and b2["mo"].first_frame[c] == 0
        assert b2["sbis"][c][0] == w["sbi"]["imgB"] and b2["sbis"][c][1] == w["sbi"]["imgA"], c
    assert w["sbi"]["imgA"] != w["sbi"]["imgB"]
    assert not any(b1["mo"].first_frame[4:]) and not any(b2["mo"].first_frame[4:])


def test_alignment_bits_are_sbi_iterates(world, runs):
    w = world
    (_, b1, _, _), (_, b2, _, _) = runs["frames"]
    se2, score = w["align"]["imgB"]
    assert abs(np.degrees(np.arctan2(se2[2], se2[0]))) > 0.1 or np.abs(se2[4:]).max() > 0.05          # the twin's alignment is no identity
    for c in range(4):
        got, sc1 = np.array(b2["mo"].se2[c]), b2["mo"].sbi_score[c]
        first = np.array(b1["mo"].se2[c])
        if GOOD[c]:
            assert got.tobytes() == se2.tobytes() and sc1 == score, c
            assert first.tolist() == [1, 0, 0, 1, 0, 0] and b1["mo"].sbi_score[c] == 0.0                 # an SBI against itself
            assert not np.array(b1["mo"].cam_rot[c]).any()
        else:
            assert not got.any() and sc1 == 0.0 and not first.any()
    assert b1["mo"].n_used == 3 and b2["mo"].n_used == 3
    assert not np.array(b1["mo"].sbi_rot).any()                        # zeros overwrite the velocity's rotation on the first frame
    assert np.linalg.norm(np.array(b2["mo"].sbi_rot)) > 1e-3


def test_prior_and_velocity_are_the_host_entries(world, runs):
    """With a non-zero velocity_in on both frames.  The largest differences seen are recorded in this file's docstring and DESIGN.md 5."""
    worst = [0.0, 0.0]
    for _, b, start, vel in runs["frames"]:
        assert np.abs(vel).min() > 0
        _assert_motion_is_host(world, b["mo"], start, vel, b["pose"], 4, worst=worst)
    print("largest over both frames: prior %.3g, velocity %.3g" % tuple(worst))
    # the first frame's rotation part is zero (three used cameras, each exactly zero), its translation part the velocity's
    mo = runs["frames"][0][1]["mo"]
    from mcptam_amd.pvs import se3_exp
    Rs, ts = world["start"]
    Re, te = se3_exp(np.concatenate([V0[:3] * DT, np.zeros(3)]))
    assert np.abs(np.array(mo.prior) - np.concatenate([(Re @ Rs).ravel(), Re @ ts + te])).max() <= 1e-12
    assert np.array(mo.prior).tobytes() != np.array(mo.start).tobytes()


def test_everything_downstream_is_track_map_records(world, runs):
    for a, b, _, _ in runs["frames"]:
        _assert_same_downstream(a, b, 4)
    b2 = runs["frames"][1][1]
    assert sum(len(i) for i in b2["items"]) > 500
    assert sum(len(m_) for m_ in b2["meas"]) > 32 * 10                 # (32 bytes per measurement: more than ten found)
    assert b2["counts"] != [world["cols"]["inl"].tobytes(), world["cols"]["outl"].tobytes()]
    # (for the record: where frame 2 ended up against poseB; the four cameras were all given one image, so this is no accuracy test)
    R, t = b2["pose"]
    RB, tB = world["sc"]["poseB"]
    print("frame 2: |R - RB| %.3g, |t - tB| %.3g" % (np.abs(R - RB).max(), np.abs(t - tB).max()))


def test_two_runs_from_one_state_give_the_same_bytes(world, runs):
    again = _two_frames(world, twin_table=False)
    for (_, b, _, _), (_, g, _, _) in zip(runs["frames"], again["frames"]):
        assert g["motion"] == b["motion"] and g["rec"] == b["rec"] and g["notes"] == b["notes"] and g["meas"] == b["meas"]
        assert g["states"] == b["states"] and g["pvs"] == b["pvs"] and g["counts"] == b["counts"] and g["sbis"] == b["sbis"]
        assert np.array_equal(g["pose"][0], b["pose"][0]) and np.array_equal(g["pose"][1], b["pose"][1])
        for c in range(4):
            assert _same_items(g["items"][c], b["items"][c])


def test_one_camera(world):
    r = _two_frames(world, ncam=1)
    for a, b, start, vel in r["frames"]:
        _assert_same_downstream(a, b, 1)
        _assert_motion_is_host(world, b["mo"], start, vel, b["pose"], 1)
    b2 = r["frames"][1][1]
    assert b2["mo"].n_used == 1 and np.array(b2["mo"].se2[0]).tobytes() == world["align"]["imgB"][0].tobytes()
    assert np.abs(np.array(b2["mo"].sbi_rot) - np.array(b2["mo"].cam_rot[0])).max() <= 1e-12 and b2["mo"].avg_rounds == 1


def test_eight_cameras_one_image_distinct_cam_from_base(world):
    from mcptam_amd.synth import so3_exp
    w = world
    cfbs = [(so3_exp(np.array([0.02 * c, -0.015 * c, 0.01 * (c % 3)])), np.array([0.01 * c, 0.0, -0.005 * c])) for c in range(8)]
    r = _two_frames(w, ncam=8, cfbs=cfbs, good=[1] * 8)
    for a, b, start, vel in r["frames"]:
        _assert_same_downstream(a, b, 8)
        _assert_motion_is_host(w, b["mo"], start, vel, b["pose"], 8, cfbs=cfbs, good=[1] * 8)
    b2 = r["frames"][1][1]
    assert b2["mo"].n_used == 8
    rots = np.array([list(b2["mo"].cam_rot[c]) for c in range(8)])
    for c in range(8):
        assert np.array(b2["mo"].se2[c]).tobytes() == w["align"]["imgB"][0].tobytes() and b2["sbis"][c][0] == w["sbi"]["imgB"], c
        assert np.abs(rots[c] - cfbs[c][0].T @ rots[0]).max() <= 1e-12      # one rotation, carried into the base frame by each CamFromBase
    assert len({rots[c].tobytes() for c in range(8)}) == 8


def test_a_table_without_rows(world):
    r = _two_frames(world, cols={})
    for a, b, start, vel in r["frames"]:
        assert sum(len(i) for i in b["items"]) == 0 and a["rec"] == b["rec"]
        assert np.array_equal(a["pose"][0], b["pose"][0]) and np.array_equal(a["pose"][1], b["pose"][1])
        _assert_motion_is_host(world, b["mo"], start, vel, b["pose"], 4)
    b2 = r["frames"][1][1]
    assert b2["mo"].n_used == 3 and np.array(b2["mo"].se2[0]).tobytes() == world["align"]["imgB"][0].tobytes()
    assert np.abs(np.array(b2["mo"].velocity)).max() > 0


def test_later_frames_fresh_handles_no_apply_and_reset(world):
    """Frame 3 on fresh keyframe handles (as after AddNewKeyFrame): the SBIs live in the table, the alignment still runs against frame 2's.
    Frame 4 with apply = 0 (after AttemptRecovery): the SBIs roll, prior == start bit for bit, the velocity comes back as given.  Then
    motion_reset: the next frame is a first frame again."""
    w = world
    r = _two_frames(w, twin_table=False)
    B, start, vel = r["B"], r["start"], r["vel"]
    fresh = _targets()
    A, ta = _table(w["cols"]), _targets()
    # (table A follows B through the split sequence so that its finders and counts are B's)
    for (_, b, _, _), img in zip(r["frames"], ("imgA", "imgB")):
        _record_frame(A, w, ta, w["sc"][img], _pose_of(b["mo"].prior))
    out = _motion_frame(B, w, fresh, w["sc"]["imgA"], start, vel)
    b3 = _snapshot(B, out, 4)
    a3 = _snapshot(A, _record_frame(A, w, ta, w["sc"]["imgA"], _pose_of(out[6].prior)), 4)
    _assert_same_downstream(a3, b3, 4)
    _assert_motion_is_host(w, out[6], start, vel, out[1], 4)
    se2, score = w["align"]["imgA"]                                    # imgA against imgB
    for c in range(4):
        assert out[6].first_frame[c] == 0
        assert b3["sbis"][c][0] == w["sbi"]["imgA"] and b3["sbis"][c][1] == w["sbi"]["imgB"], c
        if GOOD[c]:
            assert np.array(out[6].se2[c]).tobytes() == se2.tobytes() and out[6].sbi_score[c] == score
    # frame 4: no motion model
    from mcptam_amd.keyframe import _pose12
    start4, vel4 = out[1], np.array(out[6].velocity)
    out4 = _motion_frame(B, w, fresh, w["sc"]["imgB"], start4, vel4, apply=False)
    mo = out4[6]
    assert np.array(mo.prior).tobytes() == _pose12(*start4).tobytes() == np.array(mo.start).tobytes()
    assert np.array(mo.velocity).tobytes() == vel4.tobytes() and not np.array(mo.v_new).any()
    assert mo.n_used == 0 and mo.avg_rounds == 0 and not np.array(mo.se2[0]).any() and not np.array(mo.sbi_rot).any()
    a4 = _snapshot(A, _record_frame(A, w, ta, w["sc"]["imgB"], start4), 4)
    _assert_same_downstream(a4, _snapshot(B, out4, 4), 4)
    for c in range(4):
        s = [[a.tobytes() for a in B.motion_sbi(c, which)] for which in (0, 1)]
        assert s[0] == w["sbi"]["imgB"] and s[1] == w["sbi"]["imgA"] and mo.first_frame[c] == 0, c
    # reset, then a frame
    B.motion_reset()
    with pytest.raises(RuntimeError):
        B.motion_sbi(0, 0)
    out5 = _motion_frame(B, w, fresh, w["sc"]["imgB"], out4[1], vel4)
    for c in range(4):
        assert out5[6].first_frame[c] == 1
        s = [[a.tobytes() for a in B.motion_sbi(c, which)] for which in (0, 1)]
        assert s[0] == w["sbi"]["imgB"] and s[1] == w["sbi"]["imgB"], c
    assert not np.array(out5[6].sbi_rot).any() and out5[6].n_used == 3
    # imgs = NULL: the targets already hold the frame; the SBIs are made from their level 0 as held
    out6 = B.track_frame_motion(fresh, [w["cam"]] * 4, [w["cam_sbi"]] * 4, out5[1], w["cfbs"], velocity=vel4, dt=DT, cam_good=GOOD, **QUALITY, **PRM)
    assert list(out6[6].first_frame[:4]) == [0] * 4 and np.array(out6[6].se2[0]).tolist() == [1, 0, 0, 1, 0, 0]      # imgB against imgB


def test_refusals_enqueue_nothing_and_roll_no_sbi(world):
    from mcptam_amd import chain_bundle
    from mcptam_amd.keyframe import KeyFrame, _pose12
    from mcptam_amd.pvs import (TrackMapParams, TrackMapResult, TrackMotion, TrackRecord, TrackRecordParams, _bind_track_motion, motion_params)
    from mcptam_amd.taylor_camera import camera_array
    w = world
    r = _two_frames(w, twin_table=False)
    T, tg = r["B"], r["tb"]
    sbis, counts = _sbis(T, 4), [a.copy() for a in T.get_counts()]
    L = _bind_track_motion(T._L)
    hs = (ctypes.c_void_p * 4)(*[k._h for k in tg])
    cs, css = camera_array([w["cam"]] * 4), camera_array([w["cam_sbi"]] * 4)
    bad = camera_array([w["cam_sbi"]] * 4)
    bad[2].n_inv = -1
    b = _pose12(*r["start"]); b0 = b.copy()
    cfb = np.ascontiguousarray(np.concatenate([_pose12(*c) for c in w["cfbs"]]))
    prm = TrackMapParams(PRM["try_coarse"], PRM["coarse_max"], PRM["coarse_range"], PRM["coarse_min"], PRM["coarse_subpix_its"], PRM["max_patches"], 0, PRM["seed"])
    res, rec, mo = TrackMapResult(), TrackRecord(), TrackMotion()
    ctypes.memset(ctypes.byref(mo), 0x5A, ctypes.sizeof(mo))
    mo0 = bytes(mo)
    rp = TrackRecordParams(0, 1, 10, 20, 0.3, 0.13)
    ok = motion_params(r["vel"], DT, GOOD, ncam=4)
    nan_v = r["vel"].copy(); nan_v[1] = np.nan
    empty = KeyFrame(640, 480)                                         # holds no frame
    hs_empty = (ctypes.c_void_p * 4)(tg[0]._h, tg[1]._h, empty._h, tg[3]._h)

    def call(table=T._h, ncam=4, handles=hs, sbi_cams=ctypes.cast(css, ctypes.c_void_p), rp_=ctypes.byref(rp), rec_=ctypes.byref(rec), mp=ok, out=ctypes.byref(mo)):
        return L.mcp_track_frame_motion(table, ncam, handles, None, None, 0, None, ctypes.cast(cs, ctypes.c_void_p), sbi_cams, b.ctypes.data, cfb.ctypes.data,
                                        ctypes.byref(prm), ctypes.byref(res), rp_, rec_, ctypes.byref(mp) if mp is not None else None, out)
    cases = [dict(table=None), dict(ncam=0), dict(ncam=9), dict(rp_=None), dict(rec_=None), dict(mp=None), dict(out=None), dict(sbi_cams=None),
             dict(sbi_cams=ctypes.cast(bad, ctypes.c_void_p)), dict(mp=motion_params(r["vel"], DT, GOOD, blur=0.0, ncam=4)),
             dict(mp=motion_params(r["vel"], DT, GOOD, sbi_iterations=-1, ncam=4)), dict(mp=motion_params(r["vel"], 0.0, GOOD, ncam=4)),
             dict(mp=motion_params(r["vel"], float("nan"), GOOD, ncam=4)), dict(mp=motion_params(r["vel"], float("inf"), GOOD, ncam=4)),
             dict(mp=motion_params(nan_v, DT, GOOD, ncam=4)), dict(handles=hs_empty)]
    for kw in cases:
        assert call(**kw) == -1, kw
        assert chain_bundle.last_error()
    assert np.array_equal(b, b0) and bytes(mo) == mo0
    after = T.get_counts()
    assert np.array_equal(after[0], counts[0]) and np.array_equal(after[1], counts[1])
    assert _sbis(T, 4) == sbis
    # ... and the next good frame still aligns against frame 2's SBI: nothing was rolled
    assert call() == 0
    assert list(mo.first_frame[:4]) == [0] * 4 and np.array(mo.se2[0]).tolist() == [1, 0, 0, 1, 0, 0]      # the targets still hold imgB: imgB against imgB
    assert _sbis(T, 4)[0] == [w["sbi"]["imgB"], w["sbi"]["imgB"]]


def test_track_map_record_is_untouched_by_the_new_path(world, baseline, runs):
    """Last in the file: mcp_track_map_record on a fresh table gives the bytes it gave before mcp_track_frame_motion had run here."""
    now = _snapshot(*_baseline_run(world), 4)
    _assert_same_downstream(baseline, now, 4)
    # ... and on a table the new call has used (the shared parameter block and the PVS camera table carry nothing over): table B against a
    # fresh table brought to the same finders and counts through the split sequence
    w = world
    r = _two_frames(w)
    a = _snapshot(r["A"], _record_frame(r["A"], w, r["ta"], w["sc"]["imgA"], r["start"]), 4)
    b = _snapshot(r["B"], _record_frame(r["B"], w, r["tb"], w["sc"]["imgA"], r["start"]), 4)
    _assert_same_downstream(a, b, 4)
