"""mcp_track_map_record (include/mcp_img.h): mcp_track_map plus the bookkeeping Tracker::TrackMap leaves behind, in one submission.  Two
identical tables: A runs the existing calls (mcp_track_map, then mcp_scene_depth_robust on lists restated from its items), B the new call.
Pose, result, items, finders and PVS views must be mcp_track_map's bit for bit; notes, measurements, counters, quality and the count column
must equal the numpy restatement of A's items exactly; the scene depth must carry the bits of the same kernel on the same lists."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = 4
QUALITY = dict(min_patches=10, quality_coarse_min=20, quality_good=0.3, quality_bad=0.13)


@pytest.fixture(scope="module")
def world():
    """The scene of tests/test_track_map_gpu.py: four cameras, one looking away, about 4 % unusable and 2 % fixed rows -- plus counts the
    map maker would have left: 1-30 inliers, 0-30 outliers per row."""
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame, make_lite_batch
    from mcptam_amd.synth import so3_exp
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
    # (a prior six times further off than test_track_map_gpu.py's: points near the image border are in the PVS of the prior pose and outside
    # the image at the pose the coarse stage refines it to, which gives the restatement its unsearched items)
    prior = (so3_exp(np.array([0.012, -0.006, 0.009])) @ R, t + np.array([0.01, -0.006, 0.004]))
    return dict(sc=sc, cam=sc["cam"], src=src, cols=cols, cfbs=cfbs, targets=targets, prior=prior, n=n)


def _table(cols):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], cols["src"], cols["level"], cols["center"], cols["fixed"])
    t.set_counts(cols["inl"], cols["outl"])
    return t


def _params(**kw):
    p = dict(try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=10, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=12345)
    p.update(kw)
    return p


def _plain(t, w, prm, targets=None, cfbs=None):
    targets, cfbs = targets or w["targets"], cfbs or w["cfbs"]
    return t.track_map(targets, [w["cam"]] * len(targets), w["prior"], cfbs, **prm)


def _record(t, w, prm, targets=None, cfbs=None, **kw):
    targets, cfbs = targets or w["targets"], cfbs or w["cfbs"]
    return t.track_map_record(targets, [w["cam"]] * len(targets), w["prior"], cfbs, **dict(QUALITY, **kw), **prm)


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


def _depth_array(rec):
    from mcptam_amd.pvs import SCENE_DEPTH_DTYPE
    return np.frombuffer(bytes(rec.depth), dtype=SCENE_DEPTH_DTYPE).copy()


def _rec_counters(rec):
    return np.array([list(rec.attempted[c]) for c in range(8)]), np.array([list(rec.found[c]) for c in range(8)])


def _assert_record_is_restatement(rec, notes, meas, counts_after, rs, ncam):
    """The record of the new call against track_record_restate of the twin's items: exactly."""
    from mcptam_amd.pvs import tracking_quality
    att, fnd = _rec_counters(rec)
    print("attempted", att[:ncam].tolist(), "found", fnd[:ncam].tolist(), "restated", rs["attempted"][:ncam].tolist(), rs["found"][:ncam].tolist())
    print("n_inliers", rec.n_inliers, rs["n_inliers"], "outlier marks", rec.n_outlier_marks, rs["n_outlier_marks"], "n_meas", list(rec.n_meas), rs["n_meas"])
    assert np.array_equal(att, rs["attempted"]) and np.array_equal(fnd, rs["found"])
    assert rec.n_inliers == rs["n_inliers"] and rec.n_outlier_marks == rs["n_outlier_marks"]
    assert list(rec.n_items)[:ncam] == rs["n_items"] and list(rec.n_meas)[:ncam] == rs["n_meas"]
    q = [tracking_quality(rs["attempted"][c], rs["found"][c], QUALITY["min_patches"], QUALITY["quality_coarse_min"], QUALITY["quality_good"], QUALITY["quality_bad"])
         for c in range(ncam)]
    print("quality", list(rec.quality)[:ncam], q)
    assert list(rec.quality)[:ncam] == q and rec.quality_max == max(q)
    for c in range(ncam):
        assert notes[c].tobytes() == rs["notes"][c].tobytes(), c
        assert meas[c].tobytes() == rs["meas"][c].tobytes(), c
    assert np.array_equal(counts_after[0], rs["counts"][0]) and np.array_equal(counts_after[1], rs["counts"][1])


@pytest.fixture(scope="module")
def runs(gpu_required, world):
    """Table A: mcp_track_map.  Table B: mcp_track_map_record with items.  The restatement of A's items from the counts before."""
    from mcptam_amd.pvs import track_record_restate
    w = world
    prm = _params()
    A, B = _table(w["cols"]), _table(w["cols"])
    a = _plain(A, w, prm)
    b = _record(B, w, prm)
    rs = track_record_restate(a[0], (w["cols"]["inl"], w["cols"]["outl"]), False, 4)
    return dict(A=A, B=B, a=a, b=b, rs=rs, prm=prm)


def test_pose_result_items_states_and_pvs_are_track_maps(world, runs):
    a, b, A, B = runs["a"], runs["b"], runs["A"], runs["B"]
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])
    _same_result(a[2], b[2], 4)
    for c in range(4):
        assert _same_items(a[0][c], b[0][c]), c
        assert A.get_states(c).tobytes() == B.get_states(c).tobytes(), c
    assert _pvs_views(A, 4) == _pvs_views(B, 4)
    assert sum(len(i) for i in b[0]) > 500


def test_restatement_has_every_class(world, runs):
    """Preconditions on table A alone: the comparison below is not vacuous."""
    rs, a = runs["rs"], runs["a"]
    marks = np.concatenate([n["flags"] >> 6 for n in rs["notes"]])
    flags = np.concatenate([n["flags"] for n in rs["notes"]])
    found, searched, bad = (flags & 2) != 0, (flags & 1) != 0, (flags & 8) != 0
    classes = dict(inlier=int((marks == 1).sum()), weight_zero_outlier=int((found & (marks == 2)).sum()), searched_not_found=int((searched & ~found).sum()),
                   template_bad_or_unsearched=int((bad | ~searched).sum()))
    print("classes", classes)
    assert all(v > 0 for v in classes.values()), classes
    marked = [np.unique(n["row"][(n["flags"] >> 6) != 0]) for n in rs["notes"]]
    rows, times = np.unique(np.concatenate(marked), return_counts=True)
    print("rows marked by two or more cameras", int((times >= 2).sum()))
    assert (times >= 2).any()
    assert len(a[0][2]) == 0                                           # camera 2 looks away
    assert not np.array_equal(rs["counts"][0], world["cols"]["inl"]) and not np.array_equal(rs["counts"][1], world["cols"]["outl"])


def test_notes_measurements_counters_quality_and_counts(world, runs):
    b = runs["b"]
    _assert_record_is_restatement(b[5], b[3], b[4], runs["B"].get_counts(), runs["rs"], 4)
    # table A's column has not moved
    ia, oa = runs["A"].get_counts()
    assert np.array_equal(ia, world["cols"]["inl"]) and np.array_equal(oa, world["cols"]["outl"])


def test_scene_depth_carries_the_bits_of_the_same_kernel(world, runs):
    from mcptam_amd.keyframe import _pose12
    rec, rs, A = runs["b"][5], runs["rs"], runs["A"]
    cfw = np.array([list(rec.cam_from_world[c]) for c in range(4)])
    ref, _ = A.scene_depth(cfw, rs["seg_start"], rs["seg_rows"], rs["seg_w"])
    got = _depth_array(rec)
    print("depth", got[:4].tolist(), "reference", ref.tolist())
    assert got[:4].tobytes() == ref.tobytes()
    assert not got[4:].tobytes().strip(b"\0")
    assert sum(int(got[c]["refreshed"] == 1) for c in range(4)) >= 3 and got[2]["refreshed"] == 0 and got[2]["n"] == 0
    assert all(got[c]["n"] == rs["n_meas"][c] for c in range(4))
    # cam_from_base[c] * base_from_world at the refined pose.  Three-term dot products on O(1) entries: <= 3 x 2^-53 each, 100 x of room
    R, t = runs["b"][1]
    for c, (Rc, tc) in enumerate(world["cfbs"]):
        want = _pose12(Rc @ R, Rc @ t + tc)
        assert np.abs(cfw[c] - want).max() <= 1e-14, (c, np.abs(cfw[c] - want).max())


def test_lost_spares_the_not_found_items(world, runs):
    from mcptam_amd.pvs import track_record_restate
    w = world
    T = _table(w["cols"])
    got = _record(T, w, runs["prm"], lost=True)
    rs = track_record_restate(runs["a"][0], (w["cols"]["inl"], w["cols"]["outl"]), True, 4)
    _assert_record_is_restatement(got[5], got[3], got[4], T.get_counts(), rs, 4)
    assert rs["n_outlier_marks"] < runs["rs"]["n_outlier_marks"] and rs["n_inliers"] == runs["rs"]["n_inliers"]
    assert np.array_equal(got[1][0], runs["b"][1][0]) and np.array_equal(got[1][1], runs["b"][1][1])
    for c in range(4):
        assert _same_items(got[0][c], runs["b"][0][c])
        assert got[4][c].tobytes() == runs["b"][4][c].tobytes()


def test_without_items_the_record_is_the_same(world, runs):
    from mcptam_amd import chain_bundle
    w, b = world, runs["b"]
    T = _table(w["cols"])
    got = _record(T, w, runs["prm"], want_items=False)
    assert got[0] is None
    assert np.array_equal(got[1][0], b[1][0]) and np.array_equal(got[1][1], b[1][1])
    _same_result(got[2], b[2], 4)
    for c in range(4):
        assert got[3][c].tobytes() == b[3][c].tobytes() and got[4][c].tobytes() == b[4][c].tobytes()
        assert T.get_states(c).tobytes() == runs["B"].get_states(c).tobytes()
    assert bytes(got[5]) == bytes(b[5])
    ia, oa = T.get_counts()
    ib, ob = runs["B"].get_counts()
    assert np.array_equal(ia, ib) and np.array_equal(oa, ob)
    cnt = ctypes.c_int(-1)
    assert not T._L.mcp_track_map_view(T._h, 0, ctypes.byref(cnt)) and cnt.value == 0
    assert "want_items" in chain_bundle.last_error()
    # a plain mcp_track_map next: the items are back, the record's views are gone
    _plain(T, w, runs["prm"])
    assert T._L.mcp_track_map_view(T._h, 0, ctypes.byref(cnt)) and cnt.value == len(b[0][0])
    for fn in (T._L.mcp_track_map_notes_view, T._L.mcp_track_map_meas_view):
        cnt = ctypes.c_int(-1)
        assert not fn(T._h, 0, ctypes.byref(cnt)) and cnt.value == 0
        assert "mcp_track_map_record" in chain_bundle.last_error()


def test_two_runs_from_one_state_give_the_same_bytes(world, runs):
    w, b = world, runs["b"]
    T = _table(w["cols"])
    got = _record(T, w, runs["prm"])
    for c in range(4):
        assert got[3][c].tobytes() == b[3][c].tobytes() and got[4][c].tobytes() == b[4][c].tobytes()
    assert bytes(got[5]) == bytes(b[5])


def test_counts_column(gpu_required):
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    z = np.zeros((6, 3))
    t.set(z, z, z)
    assert [a.tolist() for a in t.get_counts()] == [[1] * 6, [0] * 6]                      # never set
    t.set_counts([3, 4, 5], [0, 7, 2], first=1)
    assert [a.tolist() for a in t.get_counts()] == [[1, 3, 4, 5, 1, 1], [0, 0, 7, 2, 0, 0]]
    t.update_counts([5, 0, 9], [8, 9, 2], [1, 0, 6])                                       # row 9 grows the table: 6 .. 8 are a gap
    assert t.rows == 10
    assert [a.tolist() for a in t.get_counts()] == [[9, 3, 4, 5, 1, 8, 1, 1, 1, 2], [0, 0, 7, 2, 0, 1, 0, 0, 0, 6]]
    assert t.get(6, 3)[3].tolist() == [0, 0, 0]                                            # (the gap's rows are unusable, as ever)
    t.set_counts([11, 12], [1, 2], first=10)                                               # set past the end grows too
    assert t.rows == 12 and [a.tolist() for a in t.get_counts(10, 2)] == [[11, 12], [1, 2]]
    t.resize(4); t.resize(12)                                                              # dropped and grown back
    assert [a.tolist() for a in t.get_counts()] == [[9, 3, 4, 5] + [1] * 8, [0, 0, 7, 2] + [0] * 8]
    # a key change leaves the counts alone
    t.set_source([70, 71], [None, None], [0, 0], [[1, 1], [2, 2]], first=1)
    assert [a.tolist() for a in t.get_counts(0, 4)] == [[9, 3, 4, 5], [0, 0, 7, 2]]
    # refusals: the column untouched, the size too
    before = [a.copy() for a in t.get_counts()]
    for call, err in ((lambda: t.set_counts([2, 0], [1, 1], first=2), "inlier"), (lambda: t.set_counts([2, 2], [1, -1], first=2), "outlier"),
                      (lambda: t.update_counts([1, 2, 1], [2, 2, 2], [0, 0, 0]), "twice"), (lambda: t.update_counts([1, 40], [2, 0], [0, 0]), "inlier"),
                      (lambda: t.update_counts([-1], [2], [0]), "row id")):
        with pytest.raises(RuntimeError) as e:
            call()
        assert err in str(e.value), (err, str(e.value))
        assert chain_bundle.last_error()
    after = t.get_counts()
    assert t.rows == 12 and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    with pytest.raises(RuntimeError):
        t.get_counts(5, 100)


def test_refusals_enqueue_nothing(world, runs):
    from mcptam_amd import chain_bundle
    from mcptam_amd.keyframe import _pose12
    from mcptam_amd.pvs import TrackMapParams, TrackMapResult, TrackRecord, TrackRecordParams, _bind_track_record
    from mcptam_amd.taylor_camera import camera_array
    w = world
    T = _table(w["cols"])
    got = _record(T, w, runs["prm"], copy=False)
    counts = [a.copy() for a in T.get_counts()]
    notes, meas = [n.tobytes() for n in got[3]], [m_.tobytes() for m_ in got[4]]
    L = _bind_track_record(T._L)
    hs = (ctypes.c_void_p * 4)(*[k._h for k in w["targets"]])
    cs = camera_array([w["cam"]] * 4)
    b = _pose12(*w["prior"]); b0 = b.copy()
    cfb = np.ascontiguousarray(np.concatenate([_pose12(*c) for c in w["cfbs"]]))
    p = runs["prm"]
    prm = TrackMapParams(p["try_coarse"], p["coarse_max"], p["coarse_range"], p["coarse_min"], p["coarse_subpix_its"], p["max_patches"], 0, p["seed"])
    res, rec = TrackMapResult(), TrackRecord()

    def call(rp, rec_ptr, table=T._h, ncam=4):
        return L.mcp_track_map_record(table, ncam, hs, None, None, 0, None, ctypes.cast(cs, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data, ctypes.byref(prm),
                                      ctypes.byref(res), rp, rec_ptr)
    ok = TrackRecordParams(0, 1, 10, 20, 0.3, 0.13)
    for rp, rec_ptr, kw in ((None, ctypes.byref(rec), {}), (ctypes.byref(ok), None, {}), (ctypes.byref(TrackRecordParams(0, 1, 10, 20, float("nan"), 0.13)), ctypes.byref(rec), {}),
                            (ctypes.byref(TrackRecordParams(0, 1, 10, 20, 0.3, float("inf"))), ctypes.byref(rec), {}), (ctypes.byref(ok), ctypes.byref(rec), dict(table=None)),
                            (ctypes.byref(ok), ctypes.byref(rec), dict(ncam=0)), (ctypes.byref(ok), ctypes.byref(rec), dict(ncam=9))):
        assert call(rp, rec_ptr, **kw) == -1
        assert chain_bundle.last_error()
    assert np.array_equal(b, b0)
    after = T.get_counts()
    assert np.array_equal(after[0], counts[0]) and np.array_equal(after[1], counts[1])
    # the last views stand as they were
    for c in range(4):
        for fn, dt, want in ((L.mcp_track_map_notes_view, 8, notes), (L.mcp_track_map_meas_view, 32, meas)):
            cnt = ctypes.c_int(0)
            ptr = fn(T._h, c, ctypes.byref(cnt))
            assert cnt.value * dt == len(want[c])
            if cnt.value:
                assert ctypes.string_at(ptr, cnt.value * dt) == want[c]


@pytest.mark.timeout(900)
def test_fifty_thousand_points_four_cameras(gpu_required, world):
    from mcptam_amd import synth_img
    from mcptam_amd.pvs import track_record_restate
    w = world
    base = [dict(world_pos=w["cols"]["wp"][r], pixel_right_w=w["cols"]["pr"][r], pixel_down_w=w["cols"]["pd"][r]) for r in range(w["n"])]
    wp, pr, pd, us = synth_img.make_map_cloud(base, 50000, seed=1)
    n = len(wp)
    rng = np.random.default_rng(9)
    level = rng.integers(0, 4, n).astype(np.int32)
    cols = dict(wp=wp, pr=pr, pd=pd, usable=us, keys=np.arange(n, dtype=np.int32), src=[w["src"]] * n, level=level,
                center=np.ascontiguousarray(np.stack([320 >> level, 240 >> level], axis=1).astype(np.int32)), fixed=np.zeros(n, dtype=np.uint8),
                inl=rng.integers(1, 31, n).astype(np.int32), outl=rng.integers(0, 31, n).astype(np.int32))
    cfbs = [w["cfbs"][0], w["cfbs"][1], w["cfbs"][3], w["cfbs"][1]]
    prm = _params(max_patches=1000)
    T, twin = _table(cols), _table(cols)
    got = _record(T, w, prm, cfbs=cfbs, want_items=False)
    ref = _plain(twin, w, prm, cfbs=cfbs)
    assert got[0] is None
    assert np.array_equal(got[1][0], ref[1][0]) and np.array_equal(got[1][1], ref[1][1])
    _same_result(got[2], ref[2], 4)
    rs = track_record_restate(ref[0], (cols["inl"], cols["outl"]), False, 4)
    _assert_record_is_restatement(got[5], got[3], got[4], T.get_counts(), rs, 4)
    cfw = np.array([list(got[5].cam_from_world[c]) for c in range(4)])
    depth, _ = twin.scene_depth(cfw, rs["seg_start"], rs["seg_rows"], rs["seg_w"])
    assert _depth_array(got[5])[:4].tobytes() == depth.tobytes()
    assert sum(sum(got[2].pvs_counts[c]) for c in range(4)) > 10000 and sum(rs["n_meas"]) > 100
