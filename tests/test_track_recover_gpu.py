"""mcp_track_frame_recover (include/mcp_img.h): TrackFrame's lost branch in one submission -- the relocaliser's SmallBlurryImages, the
candidates' scores, the winner's alignment and the recovered pose on the device, then mcp_track_frame_motion with apply = 0 from that pose.
The scene is tests/test_track_motion_gpu.py's (640x480 cameras, a map of a few hundred rows).  The twin is the split sequence on fresh
handles with the same bytes: mcp_kf_make_sbi(2.5), mcp_sbi_score per camera, mcp_sbi_iterate against the winner -- all compared bit for bit
-- mcp_track_recover_pose_host for the two poses (1e-9: host and device differ only in their math libraries), and
mcp_track_frame_motion(apply = 0) on a second table started at the returned pose for everything downstream, bit for bit.

Candidates come from a pool of eight keyframes with distinct images, listed over and over in a scrambled order, so a list of 130 needs
no 130 pyramids; neighbours in the list differ, and every entry's score is compared with mcp_sbi_score's."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = 4
QUALITY = dict(min_patches=10, quality_coarse_min=20, quality_good=0.3, quality_bad=0.13)
PRM = dict(try_coarse=1, coarse_max=120, coarse_range=60, coarse_min=10, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=4321)   # the doubled coarse caps
DT = 0.04
V0 = np.array([0.05, -0.03, 0.02, 0.004, -0.003, 0.002])
POOL = ["imgA", "imgB", "rollA16", "rollA48", "rollB32", "flipA", "downA12", "rollB40"]
WORST = [0.0]      # largest |device - mcp_track_recover_pose_host| seen in this file


def _pool_images(sc):
    a, b = sc["imgA"], sc["imgB"]
    return dict(imgA=a, imgB=b, rollA16=np.roll(a, 16, axis=1), rollA48=np.roll(a, 48, axis=1), rollB32=np.roll(b, -32, axis=1),
                flipA=np.ascontiguousarray(a[:, ::-1]), downA12=np.roll(a, 12, axis=0), rollB40=np.roll(b, 40, axis=1))


@pytest.fixture(scope="module")
def world(gpu_required):
    """The scene and columns of tests/test_track_motion_gpu.py; the pool: one keyframe per image with the relocaliser's SBI (blur 2.5) made
    by mcp_kf_make_sbi; twins with the tracker's SBI (blur 0.75) of imgA and imgB."""
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame
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
    imgs = _pool_images(sc)
    pool, sbi25, sbi075 = {}, {}, {}
    for name in POOL:
        k = KeyFrame(640, 480)
        k.MakeKeyFrame_Lite(imgs[name]); k.MakeSBI(2.5)
        pool[name] = k
        sbi25[name] = [a.tobytes() for a in k.SBI()]
    for name in ("imgA", "imgB"):
        k = KeyFrame(640, 480)
        k.MakeKeyFrame_Lite(imgs[name]); k.MakeSBI(0.75)
        sbi075[name] = [a.tobytes() for a in k.SBI()]
    assert len({s[1] for s in sbi25.values()}) == len(POOL)            # eight distinct templates
    # a pose far from the map: where a lost tracker believes it is
    lost_pose = (so3_exp(np.array([0.5, -0.4, 0.3])) @ sc["poseA"][0], sc["poseA"][1] + np.array([0.7, -0.5, 0.9]))
    return dict(sc=sc, imgs=imgs, cam=sc["cam"], cam_sbi=TaylorCamera(sc["cam"].params, (640, 480), (640, 480), (40, 30)), src=src, cols=cols, cfbs=cfbs, n=n,
                pool=pool, sbi25=sbi25, sbi075=sbi075, lost_pose=lost_pose)


def _p12(R, t):
    return np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)])


def _pose_of(v12):
    v = np.array(v12)
    return v[:9].reshape(3, 3).copy(), v[9:].copy()


def _table(cols):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], cols["src"], cols["level"], cols["center"], cols["fixed"])
    t.set_counts(cols["inl"], cols["outl"])
    return t


def _targets(n):
    from mcptam_amd.keyframe import KeyFrame
    return [KeyFrame(640, 480) for _ in range(n)]


def _cand_pose(w, j, c):
    """The pose of a keyframe of camera c that holds pool image j: CamFromBase[c] * (a small turn that depends on j) * poseA."""
    from mcptam_amd.synth import so3_exp
    RA, tA = w["sc"]["poseA"]
    Rp, dp = so3_exp(0.002 * j * np.array([1.0, -1.0, 0.5])), 0.001 * j * np.array([1.0, 2.0, -1.0])
    Rc, tc = w["cfbs"][c]
    return Rc @ Rp @ RA, Rc @ (Rp @ tA + dp) + tc


def _candidates(w, ncand, ncam, specials=None, only_cams=None):
    """ncand entries, the cameras interleaved (only_cams: the cameras that get any): the k-th entry of camera c holds pool image
    (5 k + 3 c + 3) % 8 -- every image once in eight entries of a camera, neighbours in the list differ, and a keyframe comes up again every
    eighth entry of its camera; specials: {index: None | raw handle | KeyFrame without SBI}."""
    kfs, cams, poses, names = [], [], [], []
    pick = list(range(ncam)) if only_cams is None else list(only_cams)
    for i in range(ncand):
        c = pick[i % len(pick)]
        j = (5 * (i // len(pick)) + 3 * c + 3) % len(POOL)
        cams.append(c); names.append(POOL[j]); poses.append(_cand_pose(w, j, c))
        kfs.append(w["pool"][POOL[j]])
    for i, v in (specials or {}).items():
        kfs[i], names[i] = v, None
    return dict(kfs=kfs, cams=cams, poses=poses, names=names)


def _recover(t, w, targets, names, start, cd, max_score=1e5, vel=V0, **kw):
    n = len(targets)
    return t.track_frame_recover(targets, [w["cam"]] * n, [w["cam_sbi"]] * n, start, w["cfbs"][:n], cd["kfs"], cd["cams"], cd["poses"], max_score=max_score,
                                 velocity=vel, imgs=[w["imgs"][x] for x in names], lost=True, **dict(QUALITY, **kw), **PRM)


def _motion(t, w, targets, names, start, vel=V0, apply=False):
    n = len(targets)
    return t.track_frame_motion(targets, [w["cam"]] * n, [w["cam_sbi"]] * n, start, w["cfbs"][:n], velocity=vel, dt=DT, apply=apply, imgs=[w["imgs"][x] for x in names],
                                lost=True, **QUALITY, **PRM)


def _same_items(a, b):
    if len(a) != len(b):
        return False
    for f in ("point", "stage", "weight_last"):
        if not np.array_equal(a[f], b[f]):
            return False
    return all(np.array_equal(a["out"][f], b["out"][f], equal_nan=a["out"][f].dtype.kind == "f") for f in a["out"].dtype.names)


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


def _snapshot(t, out, ncam):
    items, pose, res, notes, meas, rec = out[:6]
    return dict(items=items, pose=pose, res=res, notes=[x.tobytes() for x in notes], meas=[x.tobytes() for x in meas], rec=bytes(rec),
                states=[t.get_states(c).tobytes() for c in range(ncam)], pvs=_pvs_views(t, ncam), counts=[a.tobytes() for a in t.get_counts()], sbis=_sbis(t, ncam))


def _assert_same_downstream(a, b, ncam):
    assert np.array_equal(a["pose"][0], b["pose"][0]) and np.array_equal(a["pose"][1], b["pose"][1])
    ra, rb = a["res"], b["res"]
    assert ra.did_coarse == rb.did_coarse and ra.coarse_found == rb.coarse_found and np.array_equal(np.array(ra.mu_last), np.array(rb.mu_last))
    for c in range(ncam):
        assert list(ra.pvs_counts[c]) == list(rb.pvs_counts[c]) and list(ra.set_sizes[c]) == list(rb.set_sizes[c]) and ra.stale[c] == rb.stale[c], c
        assert _same_items(a["items"][c], b["items"][c]), c
        assert a["states"][c] == b["states"][c], c
        assert a["notes"][c] == b["notes"][c] and a["meas"][c] == b["meas"][c], c
    assert a["pvs"] == b["pvs"] and a["rec"] == b["rec"] and a["counts"] == b["counts"] and a["sbis"] == b["sbis"]


def _bits(x):
    return np.asarray(x, dtype=np.float64).tobytes()


def _assert_relocaliser(w, out, targets, names, cd, ncam, max_score=1e5, given=None):
    """The relocaliser's part of a call against the split sequence on the pool's handles: mcp_kf_make_sbi's bytes in the target handles,
    mcp_sbi_score's bits per camera, its winner, mcp_sbi_iterate's bits, the host entry's poses to 1e-9, the first recovering camera."""
    from mcptam_amd.keyframe import KeyFrame, sbi_iterate, sbi_score
    from mcptam_amd.pvs import SCORE_SKIPPED, recover_pose_host
    rv, scores = out[7], out[8]
    ncand = len(cd["kfs"])
    assert len(scores) == ncand
    want_cam, want_bfw = -1, None
    for c in range(ncam):
        assert [a.tobytes() for a in targets[c].SBI()] == w["sbi25"][names[c]], c
        twin = w["pool"][names[c]]
        lst = [k if (cd["cams"][i] == c and isinstance(k, KeyFrame)) else None for i, k in enumerate(cd["kfs"])]
        best, sc = sbi_score(twin, lst)
        for i in range(ncand):
            if cd["cams"][i] == c:
                assert _bits(scores[i]) == _bits(sc[i]), (c, i, scores[i], sc[i])
                if cd["names"][i] is None:
                    assert scores[i] == SCORE_SKIPPED, i
        assert rv.best[c] == best, (c, rv.best[c], best)
        if best < 0:
            assert not np.array(rv.se2[c]).any() and rv.align_score[c] == 0.0 and rv.best_zmssd[c] == 0.0 and not np.array(rv.cam_pose[c]).any()
            continue
        assert cd["names"][best] is not None and cd["cams"][best] == c
        # the first smallest: no earlier entry of this camera has a score as small
        assert all(not (cd["cams"][i] == c and sc[i] <= sc[best]) for i in range(best))
        assert _bits(rv.best_zmssd[c]) == _bits(sc[best])
        R2, t2, score = sbi_iterate(twin, cd["kfs"][best], 6)
        se2 = np.concatenate([R2.ravel(), t2])
        assert _bits(np.array(rv.se2[c])) == _bits(se2) and _bits(rv.align_score[c]) == _bits(score), (c, list(rv.se2[c]), se2)
        pose_h, bfw_h = recover_pose_host(se2, w["cam_sbi"], _p12(*cd["poses"][best]), _p12(*w["cfbs"][c]))
        d = np.abs(np.array(rv.cam_pose[c]) - pose_h).max()
        if want_cam < 0 and score < max_score:
            want_cam, want_bfw = c, bfw_h
            d = max(d, np.abs(np.array(rv.base_from_world) - bfw_h).max())
        WORST[0] = max(WORST[0], d)
        print("camera %d: best %d (%s), zmssd %.6g, align score %.6g, |pose - host| %.3g" % (c, best, cd["names"][best], sc[best], score, d))
        assert d <= 1e-9
    for c in range(ncam, 8):
        assert rv.best[c] == -1 and not np.array(rv.se2[c]).any() and not np.array(rv.cam_pose[c]).any()
    assert rv.cam == want_cam and rv.recovered == (1 if want_cam >= 0 else 0)
    if want_cam < 0:
        assert _bits(np.array(rv.base_from_world)) == _bits(_p12(*given))
    return want_cam


def _lost_frame(w, ncam, names, cd, max_score=1e5, twin=True):
    """One recovery frame on table B with fresh targets, after one ordinary frame (imgA) that leaves finder states, counts and the tracker's
    SBIs behind; table A follows with the split sequence's tail from the returned pose."""
    B, tb = _table(w["cols"]), _targets(ncam)
    first = _motion(B, w, tb, ["imgA"] * ncam, w["sc"]["poseA"], apply=True)
    before = _snapshot(B, first, ncam)
    out = _recover(B, w, tb, names, w["lost_pose"], cd, max_score=max_score)
    sb = _snapshot(B, out, ncam)
    sa = None
    if twin and out[7].recovered:
        A, ta = _table(w["cols"]), _targets(ncam)
        _motion(A, w, ta, ["imgA"] * ncam, w["sc"]["poseA"], apply=True)
        sa = _snapshot(A, _motion(A, w, ta, names, _pose_of(out[7].base_from_world)), ncam)
    return dict(B=B, tb=tb, out=out, before=before, sb=sb, sa=sa)


@pytest.fixture(scope="module")
def four(world):
    """Four cameras, 32 candidates over all of them (each pool image once per camera), every camera sees imgB."""
    cd = _candidates(world, 32, 4)
    return dict(cd=cd, names=["imgB"] * 4, run=_lost_frame(world, 4, ["imgB"] * 4, cd))


def test_relocaliser_bits_and_poses_four_cameras(world, four):
    r = four["run"]
    cam = _assert_relocaliser(world, r["out"], r["tb"], four["names"], four["cd"], 4)
    assert cam == 0 and r["out"][7].recovered == 1
    # a candidate holds imgB itself: its score is exactly zero and it wins
    assert all(r["out"][7].best_zmssd[c] == 0.0 and four["cd"]["names"][r["out"][7].best[c]] == "imgB" for c in range(4))
    print("largest |device - host| so far %.3g" % WORST[0])


def test_everything_downstream_is_track_frame_motions(world, four):
    r = four["run"]
    out, mo, rv = r["out"], r["out"][6], r["out"][7]
    assert r["sa"] is not None
    _assert_same_downstream(r["sa"], r["sb"], 4)
    # the pose TrackMap started from is the recovered one; the velocity comes back zero; the tracker's SBIs have rolled
    assert _bits(np.array(mo.start)) == _bits(np.array(rv.base_from_world)) == _bits(np.array(mo.prior))
    assert not np.array(mo.velocity).any() and not np.array(mo.v_new).any()
    for c in range(4):
        assert r["sb"]["sbis"][c] == [world["sbi075"]["imgB"], world["sbi075"]["imgA"]], c
    n_items = sum(len(i) for i in r["sb"]["items"])
    print("items %d, measurements %d, did_coarse %d" % (n_items, sum(len(m_) for m_ in r["sb"]["meas"]) // 32, out[2].did_coarse))
    assert n_items > 0 and r["sb"]["states"] != r["before"]["states"]
    assert _bits(_p12(*out[1])) != _bits(np.array(rv.base_from_world))      # TrackMap refined the pose


def test_an_alignment_that_is_no_identity(world):
    """Camera 0 sees imgB, and no candidate holds imgB: the winner is another image, the alignment a real one."""
    w = world
    cd = _candidates(w, 16, 2)
    for i, nm in enumerate(cd["names"]):
        if nm == "imgB":
            cd["kfs"][i], cd["names"][i] = w["pool"]["rollB32"], "rollB32"
    r = _lost_frame(w, 2, ["imgB", "imgB"], cd)
    _assert_relocaliser(w, r["out"], r["tb"], ["imgB", "imgB"], cd, 2)
    rv = r["out"][7]
    assert rv.best_zmssd[0] > 0 and np.array(rv.se2[0]).tolist() != [1, 0, 0, 1, 0, 0]
    assert rv.recovered == 1 and r["sa"] is not None
    _assert_same_downstream(r["sa"], r["sb"], 2)


@pytest.mark.parametrize("ncand", [0, 1, 63, 64, 65, 130])
def test_candidate_seams_of_the_scoring_tile(world, ncand):
    """Two cameras interleaved; from three entries on, a NULL entry, a destroyed handle and a handle without SBI sit in the list (DBL_MAX,
    never winning); keyframes repeat, and the lower index wins."""
    from mcptam_amd.keyframe import KeyFrame
    w = world
    T, tg = _table(w["cols"]), _targets(2)
    specials = {}
    if ncand >= 3:
        bare, gone = KeyFrame(640, 480), KeyFrame(640, 480)
        bare.MakeKeyFrame_Lite(w["imgs"]["imgB"])                      # a frame, but no SBI
        gone.MakeKeyFrame_Lite(w["imgs"]["imgB"]); gone.MakeSBI(2.5)
        dead = gone._h
        gone.close()                                                   # (no keyframe is created after this one is destroyed)
        specials = {0: None, 1: dead, 2: bare, ncand - 1: None}
        if ncand > 66:
            specials.update({63: dead, 64: None, 65: bare})
    cd = _candidates(w, ncand, 2, specials)
    names = ["rollA16", "flipA"]
    out = _recover(T, w, tg, names, w["lost_pose"], cd)
    cam = _assert_relocaliser(w, out, tg, names, cd, 2, given=w["lost_pose"])
    rv = out[7]
    if ncand == 0:
        assert cam == -1 and list(rv.best[:2]) == [-1, -1]
    elif ncand == 1:
        assert list(rv.best[:2]) == [0, -1]
    else:
        for c in range(2):
            b = rv.best[c]
            assert b >= 0 and cd["names"][b] == names[c] and rv.best_zmssd[c] == 0.0
            dup = [i for i in range(ncand) if cd["cams"][i] == c and cd["names"][i] == names[c]]
            assert b == dup[0] and (ncand < 63 or len(dup) > 1), (c, b, dup)      # listed more than once: the lower index


def test_camera_order(world):
    w = world
    # camera 0 has no candidate, camera 1 recovers
    cd = _candidates(w, 9, 2, only_cams=[1])
    T, tg = _table(w["cols"]), _targets(2)
    out = _recover(T, w, tg, ["imgB", "imgA"], w["lost_pose"], cd)
    assert _assert_relocaliser(w, out, tg, ["imgB", "imgA"], cd, 2) == 1
    assert out[7].best[0] == -1 and out[7].cam == 1 and out[7].recovered == 1
    # max_score equal to camera 0's align_score: strictly not below, so camera 1 is used (its own score is lower)
    cd = _candidates(w, 16, 2)
    for i, nm in enumerate(cd["names"]):
        if nm == "imgB":
            cd["kfs"][i], cd["names"][i] = w["pool"]["rollB40"], "rollB40"
    out = _recover(T, w, tg, ["imgB", "imgA"], w["lost_pose"], cd)
    assert _assert_relocaliser(w, out, tg, ["imgB", "imgA"], cd, 2) == 0
    s0, s1 = out[7].align_score[0], out[7].align_score[1]
    print("align scores %.9g, %.9g" % (s0, s1))
    assert s1 < s0
    out = _recover(T, w, tg, ["imgB", "imgA"], w["lost_pose"], cd, max_score=s0)
    assert _assert_relocaliser(w, out, tg, ["imgB", "imgA"], cd, 2, max_score=s0) == 1
    out = _recover(T, w, tg, ["imgB", "imgA"], w["lost_pose"], cd, max_score=float(np.nextafter(s0, np.inf)))
    assert _assert_relocaliser(w, out, tg, ["imgB", "imgA"], cd, 2, max_score=float(np.nextafter(s0, np.inf))) == 0


def test_one_camera(world):
    cd = _candidates(world, 7, 1)
    r = _lost_frame(world, 1, ["imgB"], cd)
    assert _assert_relocaliser(world, r["out"], r["tb"], ["imgB"], cd, 1) == 0
    _assert_same_downstream(r["sa"], r["sb"], 1)


@pytest.mark.parametrize("kind", ["no_candidates", "max_score_zero"])
def test_nobody_recovers(world, kind):
    w = world
    cd = _candidates(w, 0 if kind == "no_candidates" else 12, 4)
    r = _lost_frame(w, 4, ["imgB"] * 4, cd, max_score=1e5 if kind == "no_candidates" else 0.0, twin=False)
    items, pose, res, notes, meas, rec, mo, rv, scores = r["out"]
    _assert_relocaliser(w, r["out"], r["tb"], ["imgB"] * 4, cd, 4, max_score=1e5 if kind == "no_candidates" else 0.0, given=w["lost_pose"])
    assert rv.recovered == 0 and rv.cam == -1
    assert _bits(_p12(*pose)) == _bits(_p12(*w["lost_pose"])) == _bits(np.array(rv.base_from_world))
    assert r["sb"]["states"] == r["before"]["states"] and r["sb"]["counts"] == r["before"]["counts"]
    assert not any(bytes(rec)) and sum(len(i) for i in items) == 0 and sum(len(x) for x in notes) == 0 and sum(len(x) for x in meas) == 0
    assert not any(any(res.pvs_counts[c]) for c in range(4)) and not any(any(res.set_sizes[c]) for c in range(4))
    assert _bits(np.array(mo.velocity)) == _bits(V0) and not np.array(mo.v_new).any()
    for c in range(4):
        assert r["sb"]["sbis"][c] == [w["sbi075"]["imgB"], w["sbi075"]["imgA"]], c      # the tracker's SBIs have rolled
        assert [a.tobytes() for a in r["tb"][c].SBI()] == w["sbi25"]["imgB"], c            # the relocaliser's are made
    if kind == "max_score_zero":
        assert all(rv.best[c] >= 0 for c in range(4)) and (scores < 1e300).all()
    # the table tracks again afterwards
    out = _motion(r["B"], w, r["tb"], ["imgA"] * 4, w["sc"]["poseA"], apply=True)
    assert sum(len(i) for i in out[0]) > 0


def test_two_runs_from_one_state_give_the_same_bytes(world, four):
    again = _lost_frame(world, 4, four["names"], four["cd"], twin=False)
    a, b = four["run"], again
    assert bytes(a["out"][7]) == bytes(b["out"][7]) and _bits(a["out"][8]) == _bits(b["out"][8]) and bytes(a["out"][6]) == bytes(b["out"][6])
    _assert_same_downstream(a["sb"], b["sb"], 4)


def test_sbi_score_bits_are_the_raster_order_double_sum(world):
    """mcp_sbi_score, whose kernel now adds with the function it shares with k_reloc_score, still gives the plain scalar loop's bits: the float
    difference, squared and added in double, element by element."""
    from mcptam_amd.keyframe import sbi_score
    from mcptam_amd.pvs import zmssd
    w = world
    cur = w["pool"]["imgB"]
    t_cur = cur.SBI()[1]
    cands = [w["pool"][nm] for nm in ("imgA", "rollB32", "flipA", "imgB")]
    best, sc = sbi_score(cur, cands)
    want = [zmssd(t_cur, k.SBI()[1]) for k in cands]
    assert _bits(sc) == _bits(want) and best == 3 and sc[3] == 0.0 and min(sc[:3]) > 0


def test_refusals_enqueue_nothing_and_roll_no_sbi(world):
    from mcptam_amd import chain_bundle
    from mcptam_amd.keyframe import KeyFrame
    from mcptam_amd.pvs import (TrackMapParams, TrackMapResult, TrackMotion, TrackRecord, TrackRecordParams, TrackRecover, TrackRecoverParams, _bind_track_recover,
                                _candidate_args, motion_params)
    from mcptam_amd.taylor_camera import camera_array
    w = world
    T, tg = _table(w["cols"]), _targets(2)
    _motion(T, w, tg, ["imgA"] * 2, w["sc"]["poseA"], apply=True)
    cd = _candidates(w, 10, 2)
    ok_out = _recover(T, w, tg, ["imgB"] * 2, w["lost_pose"], cd)       # a good call first: the handles hold a relocaliser SBI
    assert ok_out[7].recovered == 1
    sbis, counts, states = _sbis(T, 2), [a.tobytes() for a in T.get_counts()], [T.get_states(c).tobytes() for c in range(2)]
    handle_sbis = [[a.tobytes() for a in k.SBI()] for k in tg]
    L = _bind_track_recover(T._L)
    hs = (ctypes.c_void_p * 2)(*[k._h for k in tg])
    cs, css = camera_array([w["cam"]] * 2), camera_array([w["cam_sbi"]] * 2)
    bad = camera_array([w["cam_sbi"]] * 2)
    bad[1].n_inv = -1
    b = _p12(*w["lost_pose"]); b0 = b.copy()
    cfb = np.ascontiguousarray(np.concatenate([_p12(*c) for c in w["cfbs"][:2]]))
    prm = TrackMapParams(PRM["try_coarse"], PRM["coarse_max"], PRM["coarse_range"], PRM["coarse_min"], PRM["coarse_subpix_its"], PRM["max_patches"], 0, PRM["seed"])
    res, rec, mo, rv = TrackMapResult(), TrackRecord(), TrackMotion(), TrackRecover()
    for o in (mo, rv, rec):
        ctypes.memset(ctypes.byref(o), 0x5A, ctypes.sizeof(o))
    mo0, rv0, rec0 = bytes(mo), bytes(rv), bytes(rec)
    rp = TrackRecordParams(1, 1, 10, 20, 0.3, 0.13)
    ok_mp = motion_params(V0, DT, None, apply=False, ncam=2)
    ok_rq = TrackRecoverParams(2.5, 6, 1e5)
    ncand, ch, cc, cp = _candidate_args(cd["kfs"], cd["cams"], cd["poses"])
    scores = np.full(ncand, 7.25)
    bad_cam_hi, bad_cam_lo, nan_pose, inf_pose = cc.copy(), cc.copy(), cp.copy(), cp.copy()
    bad_cam_hi[3], bad_cam_lo[0], nan_pose[4, 2], inf_pose[9, 11] = 2, -1, np.nan, np.inf
    empty = KeyFrame(640, 480)                                         # holds no frame
    hs_empty = (ctypes.c_void_p * 2)(tg[0]._h, empty._h)

    def call(table=T._h, ncam=2, handles=hs, sbi_cams=ctypes.cast(css, ctypes.c_void_p), rp_=ctypes.byref(rp), rec_=ctypes.byref(rec), mp=ok_mp, out=ctypes.byref(mo),
             n=ncand, kfs=ctypes.cast(ch, ctypes.c_void_p), cams_=cc, poses_=cp, rq=ok_rq, rout=ctypes.byref(rv)):
        return L.mcp_track_frame_recover(table, ncam, handles, None, None, 0, None, ctypes.cast(cs, ctypes.c_void_p), sbi_cams, b.ctypes.data, cfb.ctypes.data,
                                         ctypes.byref(prm), ctypes.byref(res), rp_, rec_, ctypes.byref(mp) if mp is not None else None, out,
                                         n, kfs, None if cams_ is None else cams_.ctypes.data, None if poses_ is None else poses_.ctypes.data,
                                         ctypes.byref(rq) if rq is not None else None, rout, scores.ctypes.data)
    cases = [dict(table=None), dict(ncam=0), dict(ncam=9), dict(rp_=None), dict(rec_=None), dict(mp=None), dict(out=None), dict(sbi_cams=None),
             dict(sbi_cams=ctypes.cast(bad, ctypes.c_void_p)), dict(mp=motion_params(V0, DT, None, apply=False, blur=0.0, ncam=2)),
             dict(mp=motion_params(V0, DT, None, apply=False, sbi_iterations=-1, ncam=2)), dict(handles=hs_empty),
             dict(mp=motion_params(V0, DT, None, apply=True, ncam=2)),                                       # the motion model is not applied on a recovery frame
             dict(rq=None), dict(rout=None), dict(n=-1), dict(kfs=None), dict(cams_=None), dict(poses_=None),
             dict(cams_=bad_cam_hi), dict(cams_=bad_cam_lo), dict(poses_=nan_pose), dict(poses_=inf_pose),
             dict(rq=TrackRecoverParams(0.0, 6, 1e5)), dict(rq=TrackRecoverParams(-2.5, 6, 1e5)), dict(rq=TrackRecoverParams(float("nan"), 6, 1e5)),
             dict(rq=TrackRecoverParams(2.5, -1, 1e5)), dict(rq=TrackRecoverParams(2.5, 6, float("inf"))), dict(rq=TrackRecoverParams(2.5, 6, float("nan")))]
    if chain_bundle.device_count() > 1:
        other = KeyFrame(640, 480, device=1)
        other.MakeKeyFrame_Lite(w["imgs"]["imgA"]); other.MakeSBI(2.5)
        n2, ch2, cc2, cp2 = _candidate_args(cd["kfs"][:9] + [other], cd["cams"], cd["poses"])
        cases.append(dict(kfs=ctypes.cast(ch2, ctypes.c_void_p)))
    for kw in cases:
        assert call(**kw) == -1, kw
        assert chain_bundle.last_error(), kw
    assert np.array_equal(b, b0) and bytes(mo) == mo0 and bytes(rv) == rv0 and bytes(rec) == rec0 and (scores == 7.25).all()
    assert [a.tobytes() for a in T.get_counts()] == counts and [T.get_states(c).tobytes() for c in range(2)] == states
    assert _sbis(T, 2) == sbis
    assert [[a.tobytes() for a in k.SBI()] for k in tg] == handle_sbis
    for kw, word in ((dict(mp=motion_params(V0, DT, None, apply=True, ncam=2)), "apply"), (dict(cams_=bad_cam_hi), "camera out of range"), (dict(poses_=nan_pose), "not finite"),
                     (dict(rq=TrackRecoverParams(0.0, 6, 1e5)), "reloc_blur"), (dict(rq=TrackRecoverParams(2.5, 6, float("inf"))), "max_score"), (dict(n=-1), "candidate count")):
        call(**kw)
        assert word in chain_bundle.last_error(), (word, chain_bundle.last_error())
    # ... and the same arguments, unspoilt, are taken: the targets still hold imgB, so the relocaliser's SBI is imgB's again and `last` is the one before
    assert call() == 0 and rv.recovered == 1
    assert [[a.tobytes() for a in k.SBI()] for k in tg] == handle_sbis
    assert tg[0].SBIRotationFromLast(0)[2] == 0.0                      # two consecutive SBIs on the handle: the call did not throw


def test_a_target_listed_as_a_candidate_is_skipped(world):
    """A target's SBI is the one the call rewrites: listed as a candidate it reports DBL_MAX and never wins, with or without an earlier SBI."""
    from mcptam_amd.pvs import SCORE_SKIPPED
    w = world
    T, tg = _table(w["cols"]), _targets(1)
    for _ in range(2):                                                 # first without, then with an SBI on the handle from the call before
        cd = _candidates(w, 4, 1, specials={1: tg[0]})
        out = _recover(T, w, tg, ["imgB"], w["lost_pose"], cd)
        rv, scores = out[7], out[8]
        assert scores[1] == SCORE_SKIPPED and rv.best[0] in (0, 2, 3) and rv.recovered == 1
        assert (np.delete(scores, 1) < 1e300).all()
