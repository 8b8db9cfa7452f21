"""The co-visible points of the nearest keyframe on the device (include/mcp_img.h mcp_map_collect_nearest, mcp_track_collect_nearest): on
every case of tests/collect_cases.py the device's report and mask are the host twin's bytes, run after run; with the frame mode on,
mcp_track_find_pvs and the one-call frames see exactly the rows whose near bit is set -- the PVS lists are the unfiltered lists filtered, a
one-camera TrackMap is the TrackMap of a twin table whose usable column is usable & near, the motion frame collects at the motion model's
prior, the recovery frame where nobody recovers collects nothing -- and with the mode off, after it was on or never, the bytes of before.

The world is tests/test_pvs_gpu.py's cloud (map points, rows behind the camera and outside the image, degenerate and rescaled patches,
unusable rows) with the sources tests/test_track_map_gpu.py gives its rows, and a store laid over the rows: eight MKFs on a line through the
tracker's pose, the rows in eight clusters by index, keyframe (j, c) measuring clusters j + 2c and j + 2c + 1 -- so a camera's set is four
clusters of eight, and two cameras' sets differ and overlap."""
import ctypes

import numpy as np
import pytest

import collect_cases as cl
from mcptam_amd import map_graph as mg

pytestmark = pytest.mark.gpu

LEVELS = 4
CASES = cl.all_cases()
K_MKFS, J0, STEP = 8, 3, 0.05
DT = 0.04
PRM = dict(try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=10, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=12345)


# ---- 1. the stand-alone call on every case ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_the_host_twin_byte_for_byte(gpu_required, c):
    from mcptam_amd.pvs import MapPointTable
    want, want_near = mg.collect_nearest_host(c["a"], raw=True, **cl.kwargs(c))
    runs = []
    for _ in range(2):                                   # a second run on a fresh graph gives the same bytes
        t = MapPointTable()
        g = cl.load(c, t)
        assert g.collect_last_timing() == -1.0
        rep, near = g.collect_nearest(raw=True, **cl.kwargs(c))
        assert bytes(rep) == bytes(want), (c["name"], rep.as_dict(), want.as_dict())
        assert near.tobytes() == want_near.tobytes() == g.collect_rows().tobytes(), c["name"]
        assert g.collect_last_timing() >= 0.0
        runs.append((bytes(rep), near.tobytes()))
        g.close()
    assert runs[0] == runs[1]
    if c["near"] is not None:
        assert want_near.tolist() == c["near"].tolist()


# ---- the world of the frame tests ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(gpu_required):
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame, _pose12, make_lite_batch
    from mcptam_amd.synth import so3_exp
    from mcptam_amd.taylor_camera import TaylorCamera
    sc = synth_img.make_tracking_scene()
    src = KeyFrame(640, 480)
    src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
    pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"])
    rng = np.random.default_rng(17)
    extra = []
    for k in range(40):
        p = pts[k * 7]
        extra.append(dict(p, world_pos=np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), -rng.uniform(0.5, 6)])))        # behind
        extra.append(dict(p, world_pos=p["world_pos"] + np.array([rng.choice([-1, 1]) * rng.uniform(6, 40), rng.uniform(-3, 3), 0.0])))   # outside
        extra.append(dict(p, pixel_right_w=np.zeros(3), pixel_down_w=np.zeros(3)))                                     # det 0
        extra.append(dict(p, pixel_right_w=p["pixel_right_w"] * 60.0, pixel_down_w=p["pixel_down_w"] * 60.0))         # det > 3 at level 3
        s = 2.0 ** (k % 4) * rng.uniform(0.9, 1.1)
        extra.append(dict(p, pixel_right_w=p["pixel_right_w"] * s, pixel_down_w=p["pixel_down_w"] * s))
    allp = pts + extra
    order = np.random.default_rng(3).permutation(len(allp))               # (the generated rows among the others: every cluster has some)
    allp = [allp[i] for i in order]
    wp, pr, pd = synth_img.points_soa(allp)
    n = len(allp)
    cfbs = [(np.eye(3), np.zeros(3)), (so3_exp(np.array([0.0, 0.35, 0.0])), np.array([0.05, 0.0, 0.0])),
            (so3_exp(np.array([0.0, -0.3, 0.1])), np.array([-0.05, 0.02, 0.0])), (so3_exp(np.array([0.25, 0.0, 0.0])), np.array([0.0, 0.03, 0.01]))]
    cols = dict(wp=wp, pr=pr, pd=pd, usable=(rng.random(n) >= 0.06).astype(np.uint8), keys=np.arange(n, dtype=np.int32) * 3 + 7, src=[src] * n,
                level=np.array([p["source_level"] for p in allp], dtype=np.int32), center=np.array([p["center"] for p in allp], dtype=np.int32),
                fixed=(rng.random(n) < 0.02).astype(np.uint8))
    targets = [KeyFrame(640, 480) for _ in range(4)]
    make_lite_batch(targets, [sc["imgB"]] * 4)
    R, t = sc["poseB"]
    prior = (so3_exp(np.array([0.002, -0.001, 0.0015])) @ R, t + np.array([0.01, -0.006, 0.004]))
    return dict(sc=sc, cam=sc["cam"], cam_sbi=TaylorCamera(sc["cam"].params, (640, 480), (640, 480), (40, 30)), cols=cols, cfbs=cfbs,
                cfb12=np.stack([_pose12(*q) for q in cfbs]), targets=targets, bfw=sc["poseB"], prior=prior, n=n, p12=_pose12)


def graph_arrays(w, ncam):
    """The store over the world's rows for a rig of the first ncam cameras."""
    n = w["n"]
    R, t = w["bfw"]
    pos, u = -R.T @ t, R.T @ np.array([1.0, 0.0, 0.0])               # a base translation of +x moves the base along -u in the world
    cluster = (np.arange(n) * K_MKFS) // n
    ent = [(j, c, r) for j in range(K_MKFS) for c in range(ncam) for q in (0, 1) for r in np.flatnonzero(cluster == (j + 2 * c + q) % K_MKFS)]
    a = cl.arrays([cl.P] * K_MKFS, ncam, n, ent)
    a["cam_from_base"] = w["cfb12"][:ncam].copy()
    a["base_from_world"] = np.stack([w["p12"](R, -R @ (pos + (j - J0) * STEP * u)) for j in range(K_MKFS)])
    a["kf_active"] = np.ones((K_MKFS, ncam), dtype=np.uint8)
    a["kf_depth_mean"] = np.full((K_MKFS, ncam), 2.0)
    return a


def _table(cols):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], cols["src"], cols["level"], cols["center"], cols["fixed"])
    return t


def _graph(t, a):
    g = mg.MapGraph(t, a["cam_from_base"])
    g.load_arrays(a)
    return g


def _depth(ncam):
    return np.linspace(1.5, 2.5, ncam)


def _host(w, a, pose, ncam):
    return mg.collect_nearest_host(a, w["p12"](*pose) if isinstance(pose, tuple) else pose, _depth(ncam), cam_from_base=w["cfb12"][:ncam])


def _same_report(got, want):
    assert got["valid"] == want["valid"]
    for k in cl.INT_FIELDS:
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got["nearest_dist"].tobytes() == want["nearest_dist"].tobytes()


def _filtered(lists, near):
    return [[lists[c][l][((near[lists[c][l]["point"]] >> c) & 1) == 1] for l in range(LEVELS)] for c in range(len(lists))]


def _flat(pvs):
    return b"".join(lv.tobytes() for cam in pvs for lv in cam)


def _pvs_views(t, ncam):
    from mcptam_amd.pvs import PVS_ENTRY_DTYPE
    out = []
    for c in range(ncam):
        out.append([])
        for l in range(LEVELS):
            cnt = ctypes.c_int(0)
            ptr = t._L.mcp_track_find_pvs_view(t._h, c, l, ctypes.byref(cnt))
            out[-1].append(np.frombuffer((ctypes.c_char * (cnt.value * PVS_ENTRY_DTYPE.itemsize)).from_address(ptr), dtype=PVS_ENTRY_DTYPE).copy() if cnt.value
                           else np.zeros(0, dtype=PVS_ENTRY_DTYPE))
    return out


def _same_items(a, b):
    """Field by field (numpy copies of structured arrays leave their padding bytes undefined)."""
    if len(a) != len(b):
        return False
    for f in ("point", "stage", "weight_last"):
        if not np.array_equal(a[f], b[f]):
            return False
    return all(np.array_equal(a["out"][f], b["out"][f], equal_nan=a["out"][f].dtype.kind == "f") for f in a["out"].dtype.names)


def _same_frame(t1, o1, t2, o2, ncam):
    assert np.array_equal(o1[1][0], o2[1][0]) and np.array_equal(o1[1][1], o2[1][1])
    assert bytes(o1[2]) == bytes(o2[2])
    for c in range(ncam):
        assert _same_items(o1[0][c], o2[0][c]), c
        assert t1.get_states(c).tobytes() == t2.get_states(c).tobytes(), c
    assert _flat(_pvs_views(t1, ncam)) == _flat(_pvs_views(t2, ncam))


def _find(t, w, ncam, pose=None):
    return t.find_pvs(w["targets"][:ncam], [w["cam"]] * ncam, w["bfw"] if pose is None else pose, w["cfbs"][:ncam])


def _track(t, w, ncam, pose=None):
    return t.track_map(w["targets"][:ncam], [w["cam"]] * ncam, w["prior"] if pose is None else pose, w["cfbs"][:ncam], **PRM)


# ---- 2. find_pvs with the mode on -------------------------------------------------------------------------------------------------------------
def test_find_pvs_is_the_unfiltered_pvs_filtered(world):
    w = world
    a = graph_arrays(w, 4)
    t = _table(w["cols"])
    g = _graph(t, a)
    off = _find(t, w, 4)
    t.collect_nearest(g, _depth(4))
    on = _find(t, w, 4)
    rep, near = _host(w, a, w["bfw"], 4)
    want = _filtered(off, near)
    masks = set()
    for c in range(4):
        for l in range(LEVELS):
            assert on[c][l].tobytes() == want[c][l].tobytes(), (c, l)
        kept, all_ = sum(len(x) for x in on[c]), sum(len(x) for x in off[c])
        assert 0 < kept < all_, (c, kept, all_)
        masks.add(((near >> c) & 1).tobytes())
    assert len(masks) > 1, "the cameras' sets differ"
    _same_report(t.collect_last(), rep)
    assert rep["status"][:4].tolist() == [0] * 4 and (rep["nearest_slot"][:4] == J0).all() and rep["nearest_cam"][:4].tolist() == [0, 1, 2, 3]
    assert g.collect_last_timing() >= 0.0 and len(g.collect_rows()) == 0
    # the stand-alone call at the same pose gives the mask the frame used
    rep2, near2 = g.collect_nearest(w["p12"](*w["bfw"]), _depth(4), cam_from_base=w["cfb12"])
    _same_report(rep2, rep)
    assert near2.tobytes() == near.tobytes()


# ---- 3. track_map, one camera, against a twin whose usable column is usable & near -----------------------------------------------------
def test_track_map_one_camera_is_the_twin_with_usable_and_near(world):
    w = world
    a = graph_arrays(w, 1)
    rep, near = _host(w, a, w["prior"], 1)
    A = _table(w["cols"])
    g = _graph(A, a)
    A.collect_nearest(g, _depth(1))
    oa = _track(A, w, 1)
    B = _table(dict(w["cols"], usable=w["cols"]["usable"] & (near & 1)))
    ob = _track(B, w, 1)
    _same_frame(A, oa, B, ob, 1)
    assert 0 < sum(oa[2].pvs_counts[0]) == int(sum(len(x) for x in _filtered(_find(_table(w["cols"]), w, 1, w["prior"]), near)[0]))
    assert len(oa[0][0]) > 20, "the frame tracks"
    _same_report(A.collect_last(), rep)
    with pytest.raises(RuntimeError, match="mcp_track_collect_last"):
        B.collect_last()


# ---- 4. track_map, two cameras with different winners ------------------------------------------------------------------------------------
def test_track_map_two_cameras_counts_views_and_report(world):
    w = world
    a = graph_arrays(w, 2)
    rep, near = _host(w, a, w["prior"], 2)
    assert (rep["nearest_slot"][0], rep["nearest_cam"][0]) != (rep["nearest_slot"][1], rep["nearest_cam"][1])
    assert ((near & 1) != ((near >> 1) & 1)).any()
    want = _filtered(_find(_table(w["cols"]), w, 2, w["prior"]), near)
    t = _table(w["cols"])
    g = _graph(t, a)
    t.collect_nearest(g, _depth(2))
    items, pose, res = _track(t, w, 2)
    views = _pvs_views(t, 2)
    for c in range(2):
        assert list(res.pvs_counts[c]) == [len(want[c][l]) for l in range(LEVELS)], c
        for l in range(LEVELS):
            assert views[c][l].tobytes() == want[c][l].tobytes(), (c, l)
        assert {int(r) for r in items[c]["point"]} <= set(np.flatnonzero((near >> c) & 1).tolist())
    _same_report(t.collect_last(), rep)


# ---- 5. the motion frame collects at the motion model's prior ----------------------------------------------------------------------------
def test_track_frame_motion_collects_at_the_prior(world):
    from mcptam_amd.keyframe import KeyFrame
    w = world
    a = graph_arrays(w, 2)
    t = _table(w["cols"])
    g = _graph(t, a)
    t.collect_nearest(g, _depth(2))
    vel = np.array([2.5, 0.0, 0.0, 0.0, 0.0, 0.0])                        # 0.1 along the base's x in one frame: two MKFs down the line
    targets = [KeyFrame(640, 480) for _ in range(2)]
    out = t.track_frame_motion(targets, [w["cam"]] * 2, [w["cam_sbi"]] * 2, w["bfw"], w["cfbs"][:2], velocity=vel, dt=DT, cam_good=[1, 1], imgs=[w["sc"]["imgB"]] * 2, **PRM)
    mo = out[6]
    at_start, _ = _host(w, a, np.array(mo.start), 2)
    at_prior, near = _host(w, a, np.array(mo.prior), 2)
    assert at_start["nearest_slot"][:2].tolist() == [J0, J0] and at_prior["nearest_slot"][:2].tolist() == [J0 - 2, J0 - 2], "the two poses have different winners"
    _same_report(t.collect_last(), at_prior)
    for c in range(2):
        assert sum(out[2].pvs_counts[c]) <= int(((near >> c) & 1).sum())


# ---- 6. the recovery frame where nobody recovers ------------------------------------------------------------------------------------------
def test_track_frame_recover_with_no_candidate_collects_nothing(world):
    from mcptam_amd.keyframe import KeyFrame
    w = world
    t = _table(w["cols"])
    g = _graph(t, graph_arrays(w, 2))
    t.collect_nearest(g, _depth(2))
    targets = [KeyFrame(640, 480) for _ in range(2)]
    out = t.track_frame_recover(targets, [w["cam"]] * 2, [w["cam_sbi"]] * 2, w["prior"], w["cfbs"][:2], [], [], np.zeros((0, 12)), imgs=[w["sc"]["imgB"]] * 2, **PRM)
    items, pose, res, notes, meas, rec, mo, rv, scores = out
    assert rv.recovered == 0 and rv.cam == -1
    assert np.array_equal(pose[0], w["prior"][0]) and np.array_equal(pose[1], w["prior"][1])
    assert not any(bytes(rec)) and sum(len(i) for i in items) == 0 and not any(any(res.pvs_counts[c]) for c in range(2))
    last = t.collect_last()
    assert last["valid"] == 0 and not last["status"].any() and (last["nearest_slot"] == -1).all() and (last["nearest_cam"] == -1).all()
    assert not last["nearest_dist"].any() and not any(last[k].any() for k in ("n_candidates", "n_seed_rows", "n_kfs", "n_rows"))
    # the table tracks (and collects) again afterwards
    _track(t, w, 2)
    assert t.collect_last()["valid"] == 1


# ---- 7. mode off after on ---------------------------------------------------------------------------------------------------------------------
def test_mode_off_after_on_gives_the_bytes_of_never_on(world):
    w = world
    a = graph_arrays(w, 2)
    never = _table(w["cols"]); g1 = _graph(never, a)
    toggled = _table(w["cols"]); g2 = _graph(toggled, a)
    toggled.collect_nearest(g2, _depth(2))
    on = _flat(_find(toggled, w, 2))
    toggled.collect_nearest_off()
    plain = _table(w["cols"])                                             # a twin that never saw a graph
    off = _flat(_find(plain, w, 2))
    assert _flat(_find(never, w, 2)) == off == _flat(_find(toggled, w, 2)) and on != off
    o1, o2, o3 = _track(never, w, 2), _track(toggled, w, 2), _track(plain, w, 2)
    _same_frame(never, o1, plain, o3, 2)
    _same_frame(toggled, o2, plain, o3, 2)
    for t in (never, toggled, plain):
        with pytest.raises(RuntimeError, match="mcp_track_collect_last"):
            t.collect_last()
    assert g1.collect_last_timing() == -1.0


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_a_destroyed_graph_switches_the_mode_off(world):
    from mcptam_amd.pvs import MapPointTable
    w = world
    a = graph_arrays(w, 2)
    t = _table(w["cols"])
    g = _graph(t, a)
    off = _flat(_find(t, w, 2))
    t.collect_nearest(g, _depth(2))
    on = _flat(_find(t, w, 2))
    report = t.collect_last()
    assert on != off
    # a frame whose camera count is not the graph's
    for call, name in ((lambda: _find(t, w, 1), "mcp_track_find_pvs"), (lambda: _track(t, w, 1), "mcp_track_map"), (lambda: _track(t, w, 3), "mcp_track_map")):
        with pytest.raises(RuntimeError, match=name + ".*cameras"):
            call()
    # a graph of another table, a bad depth mean, a bad fraction: the mode stays as it was
    other = MapPointTable()
    other.set(w["cols"]["wp"], w["cols"]["pr"], w["cols"]["pd"], w["cols"]["usable"])
    foreign = _graph(other, a)
    for call, word in ((lambda: t.collect_nearest(foreign, _depth(2)), "table"), (lambda: t.collect_nearest(g, [2.0, -1.0]), "depth mean"),
                       (lambda: t.collect_nearest(g, [np.nan, 1.0]), "depth mean"), (lambda: t.collect_nearest(g, _depth(2), mean_diff_fraction=np.inf), "mean_diff_fraction")):
        with pytest.raises(RuntimeError, match="mcp_track_collect_nearest.*" + word):
            call()
    for call, word in ((lambda: g.collect_nearest(np.full(12, np.nan), _depth(2)), "pose"), (lambda: g.collect_nearest(w["p12"](*w["bfw"]), [0.0, 1.0]), "depth mean")):
        with pytest.raises(RuntimeError, match="mcp_map_collect_nearest.*" + word):
            call()
    assert _flat(_find(t, w, 2)) == on, "after the refused calls a frame gives the bytes it gave before"
    _same_report(t.collect_last(), report)
    # destroying the graph switches the mode off on its table
    foreign.close()
    g.close()
    assert _flat(_find(t, w, 2)) == off
    with pytest.raises(RuntimeError, match="mcp_track_collect_last"):
        t.collect_last()
    assert len(_track(t, w, 2)[0][0]) > 20
