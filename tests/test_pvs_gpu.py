"""Tracker::FindPVS on the device (include/mcp_img.h mcp_map_points_*, mcp_track_find_pvs): membership, order and levels against the
CPU oracle's TrackerData::Project / CalcSearchLevelAndWarpMatrix, bits against the library's own per-point search, masks, the table's
life (growth, scattered updates, ordering), batches, determinism, caps and scale."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = 4
FIELDS = ("image", "cam_derivs", "warp_inverse")


@pytest.fixture(scope="module")
def world():
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame
    from mcptam_amd.synth import so3_exp
    from oracle import OracleKeyFrame
    sc = synth_img.make_tracking_scene()
    gA, oA = KeyFrame(640, 480), OracleKeyFrame(640, 480)
    gA.MakeKeyFrame_Lite(sc["imgA"]); oA.MakeKeyFrame_Lite(sc["imgA"])
    gA.MakeKeyFrame_Rest(); oA.MakeKeyFrame_Rest()
    pts = synth_img.make_map_points(sc["cam"], gA, oA, sc["poseA"], sc["depth"])
    gB, oB = KeyFrame(640, 480), OracleKeyFrame(640, 480)
    gB.MakeKeyFrame_Lite(sc["imgB"]); oB.MakeKeyFrame_Lite(sc["imgB"])
    # the generated part of the cloud: points behind the camera and outside the image, degenerate and oversized patch vectors
    # (level -1), copies with their patch vectors scaled onto every level 0..3
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
    wp, pr, pd = synth_img.points_soa(allp)
    usable = (rng.random(len(allp)) >= 0.06).astype(np.uint8)
    cfbs = [(np.eye(3), np.zeros(3)), (so3_exp(np.array([0.0, 0.35, 0.0])), np.array([0.05, 0.0, 0.0])),
            (so3_exp(np.array([0.0, -0.3, 0.1])), np.array([-0.05, 0.02, 0.0])), (so3_exp(np.array([0.25, 0.0, 0.0])), np.array([0.0, 0.03, 0.01]))]
    return dict(sc=sc, cam=sc["cam"], gA=gA, oA=oA, gB=gB, oB=oB, pts=pts, allp=allp, wp=wp, pr=pr, pd=pd, usable=usable, cfbs=cfbs,
                bfw=sc["poseB"])


def _table(wp, pr, pd, usable):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(wp, pr, pd, usable)
    return t


def _td_in(wp, pr, pd, src):
    """mcp_td_in records for the library's search, built without a Python loop per point."""
    from mcptam_amd.keyframe import TdIn
    dt = np.dtype([("world_pos", "f8", 3), ("pixel_right_w", "f8", 3), ("pixel_down_w", "f8", 3), ("source_kf", "u8"), ("source_level", "i4"),
                   ("center_x", "i4"), ("center_y", "i4"), ("fixed", "i4")], align=True)
    assert dt.itemsize == ctypes.sizeof(TdIn)
    a = np.zeros(len(wp), dtype=dt)
    a["world_pos"], a["pixel_right_w"], a["pixel_down_w"] = wp, pr, pd
    a["source_kf"] = src._h
    a["center_x"], a["center_y"] = 320, 240
    return (TdIn * len(wp)).from_buffer(a)


def _flat(pvs):
    return b"".join(lv.tobytes() for cam in pvs for lv in cam)


def _assert_pvs_is_search(pvs_c, out_c, usable, mask=None):
    """The PVS of one camera is the composition of the library's search results: usable, in image, search level >= 0 (and the mask),
    ascending rows, and image / cam_derivs / warp_inverse / level to the bit."""
    keep = (usable != 0) & (out_c["in_image"] == 1) & (out_c["search_level"] >= 0)
    if mask is not None:
        keep &= _mask_ok(mask, out_c["image"])
    for l in range(LEVELS):
        e = pvs_c[l]
        assert np.array_equal(e["point"], np.nonzero(keep & (out_c["search_level"] == l))[0]), "camera PVS membership / order at level %d" % l
        assert (e["level"] == l).all()
        r = out_c[e["point"]]
        for f in FIELDS:
            assert np.array_equal(e[f], r[f]), (l, f)


def _mask_ok(mask, image):
    h, w = mask.shape
    u, v = image[:, 0], image[:, 1]
    inside = (u >= 0) & (v >= 0) & (u < w) & (v < h)
    ok = np.zeros(len(u), dtype=bool)
    ok[inside] = mask[v[inside].astype(int), u[inside].astype(int)] != 0
    return ok


def _search_all(w, targets, wp, pr, pd):
    from mcptam_amd.keyframe import track_search_batch
    arr = _td_in(wp, pr, pd, w["gA"])
    return track_search_batch(targets, [w["cam"]] * len(targets), w["bfw"], w["cfbs"][:len(targets)], [arr] * len(targets), 2, 0)


def test_pvs_matches_oracle(gpu_required, world):
    """Membership, order and level exact against the CPU oracle's projection / warp level; the geometry to the track-search test's
    tolerance."""
    from oracle import oracle_track_search
    w = world
    t = _table(w["wp"], w["pr"], w["pd"], w["usable"])
    pvs = t.find_pvs([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    members = []
    seen_levels = set()
    for c in range(4):
        oo = oracle_track_search(w["oB"], w["cam"], w["bfw"], w["cfbs"][c], w["allp"], 2, 0)
        keep = (w["usable"] != 0) & (oo["in_image"] == 1) & (oo["search_level"] >= 0)
        for l in range(LEVELS):
            want = np.nonzero(keep & (oo["search_level"] == l))[0]
            e = pvs[c][l]
            assert np.array_equal(e["point"], want), (c, l)
            assert (e["level"] == l).all()
            for f in FIELDS:
                assert np.allclose(e[f], oo[f][want], rtol=1e-11, atol=1e-12), (c, l, f)
            if len(want):
                seen_levels.add(l)
        members.append(frozenset(np.nonzero(keep)[0].tolist()))
        # the generated cases do occur: unusable rows, rows outside, rejected warps
        assert ((w["usable"] == 0) & (oo["in_image"] == 1) & (oo["search_level"] >= 0)).any()
        assert (oo["in_image"] == 0).any() and ((oo["in_image"] == 1) & (oo["search_level"] < 0)).any()
    assert seen_levels == {0, 1, 2, 3}
    assert len(set(members)) == 4, "the four cameras should see different subsets"
    assert np.array_equal(t.counts, [[len(pvs[c][l]) for l in range(LEVELS)] for c in range(4)])


def test_pvs_is_the_library_search_to_the_bit(gpu_required, world):
    w = world
    t = _table(w["wp"], w["pr"], w["pd"], w["usable"])
    pvs = t.find_pvs([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    outs = _search_all(w, [w["gB"]] * 4, w["wp"], w["pr"], w["pd"])
    for c in range(4):
        _assert_pvs_is_search(pvs[c], outs[c], w["usable"])
    # the zero-copy view holds the same bytes
    v = t.find_pvs([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"], view=True)
    assert _flat(v) == _flat(pvs)


def test_pvs_masks(gpu_required, world):
    from mcptam_amd.keyframe import KeyFrame
    w = world
    mask = np.full((480, 640), 255, dtype=np.uint8)
    mask[:, 200:330] = 0
    mask[380:, :] = 0
    gM, g255 = KeyFrame(640, 480), KeyFrame(640, 480)
    gM.MakeKeyFrame_Lite(w["sc"]["imgB"], [mask, None, None, None])
    g255.MakeKeyFrame_Lite(w["sc"]["imgB"], [np.full((480, 640), 255, dtype=np.uint8), None, None, None])
    t = _table(w["wp"], w["pr"], w["pd"], w["usable"])
    plain = t.find_pvs([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    masked = t.find_pvs([gM] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    dropped = 0
    for c in range(4):
        for l in range(LEVELS):
            e = masked[c][l]
            assert _mask_ok(mask, e["image"]).all(), "a PVS entry projects onto a zero of the mask"
            want = plain[c][l][_mask_ok(mask, plain[c][l]["image"])]
            assert want.tobytes() == e.tobytes()
            dropped += len(plain[c][l]) - len(e)
    assert dropped > 50
    outs = _search_all(w, [gM] * 4, w["wp"], w["pr"], w["pd"])
    for c in range(4):
        _assert_pvs_is_search(masked[c], outs[c], w["usable"], mask)
    full = t.find_pvs([g255] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    assert _flat(full) == _flat(plain)


def test_pvs_table_life(gpu_required, world):
    """Moves, usable flips and rows appended past the first capacity (scattered and ranged, with a gap) give the PVS of a table
    uploaded fresh with the final contents; an update followed at once by a PVS call is seen by it."""
    from mcptam_amd import synth_img
    from mcptam_amd.pvs import MapPointTable
    w = world
    wp, pr, pd, us = synth_img.make_map_cloud(w["pts"], 3000, seed=3)
    t = MapPointTable()
    t.set(wp[:1500], pr[:1500], pd[:1500], us[:1500])
    assert t.rows == 1500
    rng = np.random.default_rng(8)
    wp, pr, pd, us = wp.copy(), pr.copy(), pd.copy(), us.copy()
    perm = rng.permutation(1500)
    moved, flipped = perm[:200], perm[200:300]
    wp[moved] += rng.normal(0, 0.05, (200, 3))
    pr[moved] *= 1.3
    us[flipped] ^= 1
    ids = np.concatenate([moved, flipped, np.arange(1500, 3000)])
    rng.shuffle(ids)
    t.update(ids, wp[ids], pr[ids], pd[ids], us[ids])
    assert t.rows == 3000
    # a ranged append that leaves a gap of 10 rows (never written: unusable)
    w2, p2, d2, u2 = synth_img.make_map_cloud(w["pts"], 400, seed=4)
    t.set(w2, p2, d2, u2, first=3010)
    assert t.rows == 3410
    fw = np.concatenate([wp, np.zeros((10, 3)), w2]); fr = np.concatenate([pr, np.zeros((10, 3)), p2])
    fd = np.concatenate([pd, np.zeros((10, 3)), d2]); fu = np.concatenate([us, np.zeros(10, np.uint8), u2])
    fresh = _table(fw, fr, fd, fu)
    args = ([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    a, b = t.find_pvs(*args), fresh.find_pvs(*args)
    assert _flat(a) == _flat(b) and sum(len(x) for cam in a for x in cam) > 500
    outs = _search_all(w, [w["gB"]] * 4, fw, fr, fd)
    for c in range(4):
        _assert_pvs_is_search(a[c], outs[c], fu)
    # a large update, then the PVS call at once
    big_w, big_r, big_d, big_u = synth_img.make_map_cloud(w["pts"], 60000, seed=5)
    t2 = _table(big_w, big_r, big_d, big_u)
    t2.find_pvs(*args)
    nw = big_w + np.array([0.01, -0.02, 0.0])
    nu = big_u.copy()
    nu[::2] = 0
    allids = np.arange(60000)
    t2.update(allids, nw, big_r, big_d, nu)
    got = t2.find_pvs(*args)
    want = _table(nw, big_r, big_d, nu).find_pvs(*args)
    assert _flat(got) == _flat(want)
    assert all((lv["point"] % 2 == 1).all() for cam in got for lv in cam)


@pytest.mark.parametrize("column", ["update", "update_source", "update_rays", "update_counts"])
def test_update_refuses_bad_row_ids(gpu_required, column):
    """Every upload by id refuses a row named twice, a negative row and row 0x7fffffff (it has no successor) with the matching message,
    and leaves the table's size and its columns as they were."""
    from mcptam_amd.pvs import MapPointTable
    rng = np.random.default_rng(21)
    t = MapPointTable()
    t.set(rng.normal(size=(8, 3)), rng.normal(size=(8, 3)), rng.normal(size=(8, 3)), np.arange(8) % 2)
    t.set_counts(np.arange(2, 10), np.arange(8))
    t.set_rays(rng.normal(size=(8, 3)), rng.normal(size=(8, 3)), rng.normal(size=(8, 3)))
    t.set_source(np.arange(8), [None] * 8, [0] * 8, np.zeros((8, 2), dtype=np.int32))
    snapshot = lambda: (t.rows, [a.tobytes() for a in t.get()], [a.tobytes() for a in t.get_counts()], t.get_states(0).tobytes())
    before = snapshot()
    for ids, err in (([1, 5, 1], "row 1 appears twice"), ([3, -1, 4], "bad row id"), ([2, 0x7fffffff, 6], "bad row id")):
        z = np.ones((3, 3))
        call = {"update": lambda: t.update(ids, z, z, z), "update_source": lambda: t.update_source(ids, [7, 8, 9], [None] * 3, [0] * 3, np.zeros((3, 2))),
                "update_rays": lambda: t.update_rays(ids, z, z, z), "update_counts": lambda: t.update_counts(ids, [5, 5, 5], [1, 1, 1])}[column]
        with pytest.raises(RuntimeError) as e:
            call()
        assert "mcp_map_points_" + column in str(e.value) and err in str(e.value), (ids, str(e.value))
        assert snapshot() == before
    # a read-back past the table's rows is refused before anything is sized from the count
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import _bind_track_map, _bind_track_record, _bind_write_back
    L = _bind_track_record(_bind_track_map(_bind_write_back(t._L)))
    for name, call in (("get", lambda: L.mcp_map_points_get(t._h, 0, 0x7fffffff, None, None, None, None)),
                       ("get", lambda: L.mcp_map_points_get(t._h, 7, 2, None, None, None, None)),
                       ("get_counts", lambda: L.mcp_map_points_get_counts(t._h, 0, 0x7fffffff, None, None)),
                       ("get_states", lambda: L.mcp_map_points_get_states(t._h, 0, 1, 8, None))):
        assert call() == -1 and chain_bundle.last_error() == "mcp_map_points_%s: bad arguments" % name
    assert snapshot() == before


def test_pvs_batch_equals_single_cameras_and_is_deterministic(gpu_required, world):
    w = world
    t = _table(w["wp"], w["pr"], w["pd"], w["usable"])
    args = ([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    runs = [_flat(t.find_pvs(*args)) for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]
    batch = t.find_pvs(*args)
    for c in range(4):
        single = t.find_pvs([w["gB"]], [w["cam"]], w["bfw"], [w["cfbs"][c]])
        assert b"".join(x.tobytes() for x in single[0]) == b"".join(x.tobytes() for x in batch[c])


def test_pvs_caps_and_refusals(gpu_required, world):
    from mcptam_amd import chain_bundle
    from mcptam_amd.keyframe import KeyFrame
    from mcptam_amd.pvs import PVS_ENTRY_DTYPE, MapPointTable, lib
    w = world
    t = _table(w["wp"], w["pr"], w["pd"], w["usable"])
    args = ([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    full = t.find_pvs(*args)
    need = t.counts.copy()
    tot = need.sum(axis=1)
    assert (tot > 0).all()
    caps = tot.copy()
    caps[2] -= 1
    sentinel = np.zeros(1, dtype=PVS_ENTRY_DTYPE)
    sentinel["point"], sentinel["level"], sentinel["image"] = -7, -9, 1234.5
    outs = [np.repeat(sentinel, caps[c] + 1) for c in range(4)]
    with pytest.raises(RuntimeError, match="camera 2"):
        t.find_pvs(*args, caps=caps, out=outs)
    assert np.array_equal(t.counts, need), "the needed counts are reported"
    assert outs[2].tobytes() == np.repeat(sentinel, caps[2] + 1).tobytes(), "nothing is written for the camera over its cap"
    for c in (0, 1, 3):
        assert outs[c][:tot[c]].tobytes() == b"".join(x.tobytes() for x in full[c])
        assert outs[c][tot[c]:].tobytes() == sentinel.tobytes()
    # exactly at the cap is fine
    ok = t.find_pvs(*args, caps=tot)
    assert _flat(ok) == _flat(full)
    # a NULL table is an error, not a crash
    counts = (ctypes.c_int * 4)()
    assert lib().mcp_track_find_pvs(None, 1, None, None, None, None, None, None, counts) == -1
    assert "NULL table" in chain_bundle.last_error()
    # a target on another device than the table's.  Only a box with two devices can make one: on a single-device box this branch
    # does not run (the refusal is a host-side comparison of the handles' device ordinals in mcp_track_find_pvs, before anything
    # is enqueued)
    if chain_bundle.device_count() > 1:
        other = KeyFrame(640, 480, device=1)
        other.MakeKeyFrame_Lite(w["sc"]["imgB"])
        with pytest.raises(RuntimeError, match="device"):
            t.find_pvs([w["gB"], other], [w["cam"]] * 2, w["bfw"], w["cfbs"][:2])
        t1 = MapPointTable(device=1)
        t1.set(w["wp"], w["pr"], w["pd"], w["usable"])
        with pytest.raises(RuntimeError, match="device"):
            t1.find_pvs([w["gB"]], [w["cam"]], w["bfw"], w["cfbs"][:1])
    # an empty table gives empty lists
    e = MapPointTable().find_pvs(*args)
    assert all(len(x) == 0 for cam in e for x in cam)


def test_pvs_at_scale_50k_points_4_cameras(gpu_required, world):
    from mcptam_amd import synth_img
    w = world
    wp, pr, pd, us = synth_img.make_map_cloud(w["pts"], 50000, seed=9)
    t = _table(wp, pr, pd, us)
    pvs = t.find_pvs([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    outs = _search_all(w, [w["gB"]] * 4, wp, pr, pd)
    for c in range(4):
        _assert_pvs_is_search(pvs[c], outs[c], us)
    sizes = t.counts.sum(axis=1)
    assert (sizes > 1000).all() and (sizes < 50000).all()


def test_pvs_table_shrinks_with_the_map(gpu_required, world):
    """A whole-map re-upload after the map lost points (Map::MoveBadPointsToTrash): resize to the new size, then set the rows.  No
    dropped row reaches the PVS; growing again brings them back unusable; an empty map gives empty lists."""
    from mcptam_amd import synth_img
    from mcptam_amd.pvs import MapPointTable
    w = world
    args = ([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    wp, pr, pd, us = synth_img.make_map_cloud(w["pts"], 4000, seed=12)
    t = MapPointTable()
    t.set(wp, pr, pd, us)
    full = t.find_pvs(*args)
    assert any((lv["point"] >= 2500).any() for cam in full for lv in cam)
    keep = np.random.default_rng(2).permutation(4000)[:2500]          # the map after some points went to the trash, in a new order
    t.resize(2500)
    t.set(wp[keep], pr[keep], pd[keep], us[keep])
    assert t.rows == 2500
    got = t.find_pvs(*args)
    want = _table(wp[keep], pr[keep], pd[keep], us[keep]).find_pvs(*args)
    assert _flat(got) == _flat(want)
    assert all((lv["point"] < 2500).all() for cam in got for lv in cam)
    assert sum(len(lv) for cam in got for lv in cam) > 200
    t.resize(4000)                                                     # grown again: rows 2500.. are unusable zero rows
    assert t.rows == 4000 and _flat(t.find_pvs(*args)) == _flat(want)
    t.resize(0)
    assert t.rows == 0 and all(len(lv) == 0 for cam in t.find_pvs(*args) for lv in cam)
    with pytest.raises(RuntimeError):
        t.resize(-1)


def test_pvs_mask_smaller_than_the_camera_image(gpu_required, world):
    """The documented deviation: with a level-0 mask, a projection at u >= mask width or v >= mask height -- u == w
    included, where the reference reads past the mask -- is dropped; without a mask the same target keeps it."""
    from mcptam_amd.keyframe import KeyFrame
    w = world
    small = np.ascontiguousarray(w["sc"]["imgB"][:240, :320])
    masked, plain = KeyFrame(320, 240), KeyFrame(320, 240)
    masked.MakeKeyFrame_Lite(small, [np.full((240, 320), 255, dtype=np.uint8), None, None, None])
    plain.MakeKeyFrame_Lite(small)
    t = _table(w["wp"], w["pr"], w["pd"], w["usable"])
    cams = [w["cam"]] * 4                                               # 640 x 480 camera model on 320 x 240 targets
    a = t.find_pvs([plain] * 4, cams, w["bfw"], w["cfbs"])
    b = t.find_pvs([masked] * 4, cams, w["bfw"], w["cfbs"])
    outside = 0
    for c in range(4):
        for l in range(LEVELS):
            u, v = a[c][l]["image"][:, 0], a[c][l]["image"][:, 1]
            inside = (u < 320) & (v < 240)
            assert b[c][l].tobytes() == a[c][l][inside].tobytes(), (c, l)
            outside += int((~inside).sum())
    assert outside > 100, "the camera sees past the mask"
