"""mcp_stereo_map_points (AddStereoMapPoints of one source keyframe and level whose created points stay on the device) against the composition it
replaces -- mcp_stereo_points followed by the five public upload calls for the same rows and keys -- on twin tables and graphs, byte for byte:
both sides run the same kernels on the same inputs.  The fixture is test_stereo_points_gpu.py's scene: 640x480, a source and targets, levels 1
and 2."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SRC_MKF, SRC_CAM = 0, 0
BASE_ROWS = 150                                # the map before the call: rows 0 .. 149 hold tracked points
TARGET_MKF, TARGET_CAM = np.array([1, 2, 3], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32)


@pytest.fixture(scope="module")
def scene():
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame
    sc = synth_img.make_stereo_scene()
    src = KeyFrame(640, 480)
    src.MakeKeyFrame_Lite(sc["img_src"]); src.MakeKeyFrame_Rest()
    tg = []
    for im in sc["imgs"][:3]:
        g = KeyFrame(640, 480)
        g.MakeKeyFrame_Lite(im)
        tg.append(g)
    pts = synth_img.make_map_points(sc["cam"], src, None, sc["pose_src"], sc["depth"], per_level=(60, 40, 30, 20))
    assert len(pts) == BASE_ROWS
    sc.update(src=src, tg=tg, pts=pts, cand={level: src.Candidates(level)[0] for level in (1, 2)})
    return sc


def _targets(sc, js):
    return [(sc["tg"][j], sc["cam"], sc["poses"][j]) for j in js]


def _base_store(n_rows=BASE_ROWS, seed=3):
    """two entries per row, about a quarter of them of the source keyframe (SRC_MKF, SRC_CAM), positions anywhere in the image"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n_rows), 2)
    k = r + np.tile([0, 1], n_rows)
    return dict(mkf=(k % 4).astype(np.int32), cam=(k % 2).astype(np.int32), row=r.astype(np.int32), uv=rng.uniform([0, 0], [640, 480], (2 * n_rows, 2)),
                level=rng.integers(0, 4, 2 * n_rows).astype(np.int32), source=np.tile([2, 0], n_rows).astype(np.int32))


def _world(sc, store=None, dead=(5, 40, 41, 200, 299), track=True):
    """A table of BASE_ROWS tracked points (their finders of camera 0 have seen a frame) and a graph of 4 present MKFs, a 2-camera rig and about 300
    store entries, a few of them dead."""
    from mcptam_amd import map_graph as mg, synth_img
    from mcptam_amd.pvs import MapPointTable
    pts = sc["pts"]
    n = len(pts)
    t = MapPointTable()
    wp, pr, pd = synth_img.points_soa(pts)
    t.set(wp, pr, pd, np.ones(n, dtype=np.uint8))
    t.set_source(np.arange(n, dtype=np.int32) * 3 + 7, [sc["src"]] * n, [p["source_level"] for p in pts], [p["center"] for p in pts])
    if track:
        t.track_map([sc["tg"][0]], [sc["cam"]], sc["poses"][0], [(np.eye(3), np.zeros(3))], seed=11)
    eye = mg.poses12(np.stack([np.eye(3)] * 4), np.array([[0.0, 0, 0], [-0.6, 0, 0], [0.5, -0.2, 0], [-0.3, 0.5, 0.1]]))
    g = mg.MapGraph(t, mg.poses12(np.stack([np.eye(3)] * 2), np.array([[0.0, 0, 0], [0.1, 0, 0]])))
    g.set_mkfs(eye, np.full(4, mg.MKF_PRESENT, dtype=np.int32), np.ones((4, 2), dtype=np.uint8), np.full((4, 2), 6.0))
    g.update_points(np.arange(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    s = _base_store() if store is None else store
    if len(s["mkf"]):
        g.add_meas(s["mkf"], s["cam"], s["row"], s["uv"], s["level"], s["source"])
        d = np.array([i for i in dead if i < len(s["mkf"])], dtype=np.int64)
        if len(d):
            assert g.erase_meas(s["mkf"][d], s["cam"][d], s["row"][d]) == len(d)
    return t, g


def _rows_keys(n_cand, first=BASE_ROWS, seed=1):
    """free rows for every candidate: past the table's end, out of order, with gaps"""
    rng = np.random.default_rng(seed)
    rows = first + rng.permutation(3 * n_cand)[:n_cand].astype(np.int32)
    return rows, (100000 + 7 * np.arange(n_cand)).astype(np.int32)


def _store_of(g):
    from mcptam_amd import map_graph as mg
    m = g.get_meas()
    s = np.zeros(len(m["mkf"]), dtype=mg.STORE_ENTRY_DTYPE)
    for k in ("mkf", "cam", "row", "uv", "level", "source", "alive"):
        s[k] = m[k]
    return s


def _snapshot(t, g):
    R = t.rows
    snap = dict(rows=R, num_meas=g.num_meas(), check=g.check())
    for k, v in zip(("world_pos", "pixel_right_w", "pixel_down_w", "usable"), t.get()):
        snap[k] = v.tobytes()
    snap["inlier"], snap["outlier"] = (a.tobytes() for a in t.get_counts())
    rays, has = t.get_rays()
    snap["rays"], snap["has_rays"] = rays.tobytes(), has.tobytes()
    for k, v in t.get_source().items():
        snap["src_" + k] = v.tobytes()
    snap["states0"] = t.get_states(0).tobytes()
    for k, v in g.get_points().items():
        snap["gp_" + k] = v.tobytes()
    snap["store"] = _store_of(g).tobytes()
    snap["good"] = g.good_counts().tobytes()
    return snap


def _one_call(sc, t, g, level, js, rows, keys, **kw):
    return g.add_stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, sc["cand"][level], _targets(sc, js), TARGET_MKF[js], TARGET_CAM[js], rows, keys,
                               SRC_MKF, SRC_CAM, **kw)


def _composition(sc, t, g, level, js, rows, keys, limit=1 << 30):
    """twin B: the host walk over the keyframe's measurements, mcp_stereo_points, then the five uploads for the rows and keys the points take"""
    from mcptam_amd import stereo as S
    cand = sc["cand"][level]
    first = g.num_meas()[1]
    busy = S.stereo_busy_ref(_store_of(g), SRC_MKF, SRC_CAM)
    pts, keep, oc = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, cand, _targets(sc, js), limit=limit, meas=busy)
    made = len(pts)
    t.resize(max(t.rows, int(rows.max()) + 1))                 # (the host assigned the rows: the table covers them)
    r = rows[:made]
    if made:
        t.update(r, pts["world_pos"], pts["pixel_right_w"], pts["pixel_down_w"], np.zeros(made, dtype=np.uint8))
        t.update_rays(r, pts["center_nc"], pts["one_right_nc"], pts["one_down_nc"])
        t.update_source(r, keys[:made], [sc["src"]] * made, np.full(made, level), cand[pts["candidate"]])
        g.update_points(r, np.full(made, SRC_MKF), np.full(made, SRC_CAM), np.zeros(made, dtype=np.int32))
        tm, tc = TARGET_MKF[js][pts["target"]], TARGET_CAM[js][pts["target"]]
        g.add_meas(np.stack([np.full(made, SRC_MKF), tm], axis=1).ravel(), np.stack([np.full(made, SRC_CAM), tc], axis=1).ravel(), np.repeat(r, 2),
                   np.stack([pts["root_pos"], pts["target_pos"]], axis=1).reshape(-1, 2), np.full(2 * made, level), np.tile([S.SRC_ROOT, S.SRC_EPIPOLAR], made))
    return pts, keep, oc, dict(made=made, first_store=first, n_busy=len(busy))


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k] == b[k], k


def _check_against_ref(sc, t, g, level, js, pts, rows, res):
    """the rows and the store's tail are what stereo_append_ref says the records become"""
    from mcptam_amd import stereo as S
    made = len(pts)
    want = S.stereo_append_ref(pts, rows, level, SRC_MKF, SRC_CAM, TARGET_MKF[js], TARGET_CAM[js], res["first_store"])
    assert g.num_meas()[1] == want["store_end"]
    assert _store_of(g)[res["first_store"]:].tobytes() == want["appended"].tobytes()
    assert np.array_equal(want["center_xy"], sc["cand"][level][pts["candidate"]])
    r = rows[:made]
    wp, pr, pd, us = t.get()
    rays, has = t.get_rays()
    src, gp = t.get_source(), g.get_points()
    inl, outl = t.get_counts()
    for got, k in ((wp, "world_pos"), (pr, "pixel_right_w"), (pd, "pixel_down_w"), (us, "usable"), (rays, "rays"), (inl, "inlier"), (outl, "outlier"),
                   (src["level"], "source_level"), (src["center"], "center_xy"), (src["fixed"], "fixed"), (gp["src_mkf"], "gp_src_mkf"), (gp["src_cam"], "gp_src_cam"),
                   (gp["flags"], "gp_flags")):
        assert got[r].tobytes() == want[k].tobytes(), k
    assert has[r].all() and src["has_source"][r].all()


@pytest.mark.parametrize("js", [[0], [0, 1, 2]], ids=["one_target", "three_targets"])
def test_equals_the_composition(gpu_required, scene, js):
    """5: one call on twin A = mcp_stereo_points + the five uploads on twin B, every read-back byte for byte, and both = stereo_append_ref"""
    from mcptam_amd import stereo as S
    sc = scene
    for level in (1, 2):
        rows, keys = _rows_keys(len(sc["cand"][level]), seed=level)
        (ta, ga), (tb, gb) = _world(sc), _world(sc)
        _same(_snapshot(ta, ga), _snapshot(tb, gb))
        pa, ka, oa, ra = _one_call(sc, ta, ga, level, js, rows, keys)
        pb, kb, ob, rb = _composition(sc, tb, gb, level, js, rows, keys)
        assert ra == rb and ra["made"] == len(pa) >= 10 and ra["n_busy"] > 20
        assert pa.tobytes() == pb.tobytes() and np.array_equal(ka, kb) and np.array_equal(oa, ob)
        A, B = _snapshot(ta, ga), _snapshot(tb, gb)
        _same(A, B)
        assert A["check"][0] == 0 and A["num_meas"][1] == ra["first_store"] + 2 * ra["made"] and A["rows"] == rows.max() + 1
        _check_against_ref(sc, ta, ga, level, js, pa, rows, ra)
        _check_against_ref(sc, tb, gb, level, js, pb, rows, rb)
        if len(js) == 3:
            assert set(pa["target"]) >= {0, 1}
        # the rows that were handed in and not taken keep their bytes: rows of a table that has just grown
        left = rows[ra["made"]:]
        assert not ta.get()[3][left].any() and not ta.get_rays()[1][left].any() and not ta.get_source()["has_source"][left].any()
        assert (ga.good_counts()[rows[:ra["made"]]] == 2).all() and (ga.good_counts()[left] == 0).all()


def test_busy_list_from_the_store(gpu_required, scene):
    """6: entries of (SRC_MKF, SRC_CAM) on top of candidates 0, 5, 10, ... at levels 0..3, some dead, some under another camera: the call with
    busy_from_store gives keep / outcome of the call with the equivalent host list; the dead ones and the other camera's do not thin"""
    from mcptam_amd import stereo as S
    sc = scene
    level = 1
    cand = sc["cand"][level]
    pick = np.arange(0, len(cand), 5)
    n = len(pick)
    roots = S.level_zero_pos(cand[pick], level)
    lv = (np.arange(n) % 4).astype(np.int32)
    other = (np.arange(n) % 7 == 3)                            # these sit under camera 1 of the same MKF
    dead = np.flatnonzero((np.arange(n) % 6 == 1) & ~other)
    store = dict(mkf=np.full(n, SRC_MKF, dtype=np.int32), cam=np.where(other, 1, SRC_CAM).astype(np.int32), row=np.arange(n, dtype=np.int32) % BASE_ROWS, uv=roots, level=lv,
                 source=np.zeros(n, dtype=np.int32))
    assert n <= BASE_ROWS                                      # (one entry per row: the keys are distinct)
    t, g = _world(sc, store=store, dead=tuple(dead), track=False)
    live = np.ones(n, dtype=bool); live[dead] = False; live[other] = False
    rows, keys = _rows_keys(len(cand))
    js = [0, 1]
    pa, ka, oa, ra = _one_call(sc, t, g, level, js, rows, keys, busy_from_store=True)
    meas = S.make_meas(roots[live], lv[live])
    ph, kh, oh = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, cand, _targets(sc, js), meas=meas)
    assert ra["n_busy"] == live.sum() == len(meas)
    assert pa.tobytes() == ph.tobytes() and np.array_equal(ka, kh) and np.array_equal(oa, oh)
    thin_live = S.thin_candidates(cand, level, roots[live], lv[live])
    thin_all = S.thin_candidates(cand, level, roots, lv)
    assert np.array_equal(oa[0] != S.THINNED, thin_live) and (thin_live != thin_all).any() and not thin_live.all()
    spared = pick[(~live) & ((lv == 1) | (lv == 2))]           # under a dead entry or the other camera's at a thinning level: only a live neighbour thins them
    assert len(spared) > 0 and np.array_equal(oa[0][spared] != S.THINNED, thin_live[spared]) and thin_live[spared].any() and not thin_all[spared].any()
    # the caller's list with the store's mode off gives the same; together they are refused
    t2, g2 = _world(sc, store=store, dead=tuple(dead), track=False)
    p2, k2, o2, r2 = _one_call(sc, t2, g2, level, js, rows, keys, meas=meas, busy_from_store=False)
    assert p2.tobytes() == pa.tobytes() and np.array_equal(o2, oa) and r2 == ra
    _same(_snapshot(t, g), _snapshot(t2, g2))


def test_rows_grow_recycle_and_stay(gpu_required, scene):
    """7: rows past the end grow the table (gaps read unusable); a recycled row comes back with the new key, zeroed finders and the new source, and a
    parcel filled for it before commits as stale; the rows not taken keep their bytes"""
    from mcptam_amd import map_graph as mg, stereo as S
    sc = scene
    level = 2
    cand = sc["cand"][level]
    t, g = _world(sc)
    st0 = t.get_states(0)
    old = int(np.flatnonzero(st0["valid"] != 0)[0])            # a row whose finder of camera 0 has seen a frame
    assert t.get_source(old, 1)["has_source"][0] and st0[old:old + 1].tobytes().strip(b"\0")
    t.update_counts([old], [5], [3])
    s = _store_of(g)
    mine = np.flatnonzero(s["row"] == old)                      # (no live store entry may name a row that is handed in)
    g.erase_meas(s["mkf"][mine], s["cam"][mine], s["row"][mine])
    parcel = mg.MeasParcel.from_host(t, [0], [old], [[10.0, 20.0]], [1])
    rows, keys = _rows_keys(len(cand), first=BASE_ROWS + 500)
    rows[0] = old
    before = _snapshot(t, g)
    pts, keep, oc, res = _one_call(sc, t, g, level, [0, 1], rows, keys)
    made = res["made"]
    assert made >= 10 and t.rows == rows.max() + 1 > BASE_ROWS + 500
    wp, pr, pd, us = t.get()
    gap = np.setdiff1d(np.arange(BASE_ROWS, t.rows), rows[:made])
    assert not us[gap].any() and not wp[gap].any() and (g.get_points()["flags"][gap] == mg.GP_BAD).all()
    src = t.get_source()
    assert src["key"][old] == keys[0] and src["level"][old] == level and np.array_equal(src["center"][old], cand[pts["candidate"][0]]) and src["has_source"][old]
    assert not t.get_states(0, old, 1).tobytes().strip(b"\0")
    assert [int(a[old]) for a in t.get_counts()] == [1, 0]
    keep_rows = np.setdiff1d(np.arange(BASE_ROWS), [old])       # every other old row keeps its finder
    assert t.get_states(0)[keep_rows].tobytes() == st0[keep_rows].tobytes()
    cres, lanes = g.commit_parcel(parcel, [1], [0])
    assert cres["n_stale"] == 1 and cres["n_appended"] == 0
    _check_against_ref(sc, t, g, level, [0, 1], pts, rows, res)
    # rows[made:] keep their bytes: they read as rows of a grown table, and a second call may take them
    left = rows[made:]
    assert not us[left].any() and not src["has_source"][left].any() and (src["key"][left] == 0).all()
    now = _snapshot(t, g)
    for k in ("world_pos", "pixel_right_w", "pixel_down_w", "usable", "inlier", "outlier", "src_key", "states0", "gp_src_mkf"):
        after = np.frombuffer(now[k], dtype=np.uint8).reshape(now["rows"], -1)
        b4 = np.frombuffer(before[k], dtype=np.uint8).reshape(before["rows"], -1)
        assert np.array_equal(after[keep_rows], b4[keep_rows]), k


def test_seams_of_made(gpu_required, scene):
    """8: no target: nothing appended; limit = 1: the quirk of mcp_stereo_points, store entries only for the points made; a store at exactly its
    capacity grows and keeps its entries"""
    from mcptam_amd import stereo as S
    sc = scene
    level = 2
    cand = sc["cand"][level]
    rows, keys = _rows_keys(len(cand))
    t, g = _world(sc)
    before = _snapshot(t, g)
    pts, keep, oc, res = _one_call(sc, t, g, level, [], rows, keys)
    after = _snapshot(t, g)
    assert res["made"] == 0 and len(pts) == 0 and res["first_store"] == before["num_meas"][1] and after["store"] == before["store"] and after["num_meas"] == before["num_meas"]
    assert after["rows"] == rows.max() + 1 and not np.frombuffer(after["usable"], dtype=np.uint8)[BASE_ROWS:].any()
    busy = S.stereo_busy_ref(_store_of(g), SRC_MKF, SRC_CAM)
    assert res["n_busy"] == len(busy) and np.array_equal(keep, S.thin_candidates(cand, level, busy["root_pos"], busy["level"]))
    # limit 1 over three targets
    js = [0, 1, 2]
    pts, keep, oc, res = _one_call(sc, t, g, level, js, rows, keys, limit=1)
    ph, kh, oh = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, cand, _targets(sc, js), limit=1, meas=busy)
    assert pts.tobytes() == ph.tobytes() and np.array_equal(oc, oh) and np.array_equal(keep, kh)
    assert (pts["target"] == 0).sum() == 1 and 1 <= res["made"] <= 3 and (oc == S.PAST_LIMIT).any()
    assert g.num_meas() == (before["num_meas"][0] + 2 * res["made"], before["num_meas"][1] + 2 * res["made"])
    _check_against_ref(sc, t, g, level, js, pts, rows, res)
    # a store of exactly 1024 entries (the first block's size)
    n = 1024
    i = np.arange(n)
    full = dict(mkf=(i % 4).astype(np.int32), cam=((i // 4) % 2).astype(np.int32), row=(i // 8).astype(np.int32), uv=np.stack([i * 0.5, 700.0 + i], axis=1), level=(i % 4).astype(np.int32),
                source=np.zeros(n, dtype=np.int32))
    t, g = _world(sc, store=full, dead=(3, 1000))
    old = _store_of(g)
    assert len(old) == n
    pts, keep, oc, res = _one_call(sc, t, g, level, [0], rows, keys)
    now = _store_of(g)
    assert res["first_store"] == n and res["made"] >= 10 and len(now) == n + 2 * res["made"] and now[:n].tobytes() == old.tobytes()
    _check_against_ref(sc, t, g, level, [0], pts, rows, res)


def test_downstream_calls_see_the_new_points(gpu_required, scene):
    """9: a select in ALL mode picks up the new rows; HandleOutliers on a new point's SRC_EPIPOLAR entry behaves as on a host-appended one"""
    from mcptam_amd import map_graph as mg
    sc = scene
    level, js = 2, [0, 1]
    rows, keys = _rows_keys(len(sc["cand"][level]))
    (ta, ga), (tb, gb) = _world(sc), _world(sc)
    pa, _, _, ra = _one_call(sc, ta, ga, level, js, rows, keys)
    pb, _, _, rb = _composition(sc, tb, gb, level, js, rows, keys)
    assert ra == rb and ra["made"] >= 10
    new = rows[:ra["made"]]
    prm = mg.select_params(mg.BUNDLE_ALL, min_points=1)
    va, vb = ga.select_raw(prm), gb.select_raw(prm)
    assert va[0].status == 0 and va[0].as_dict() == vb[0].as_dict()
    for x, y in zip(va[1:], vb[1:]):
        assert x.tobytes() == y.tobytes()
    assert np.isin(new, va[2]["row"]).all()
    k = 3
    key = (TARGET_MKF[js][pa["target"][k]], TARGET_CAM[js][pa["target"][k]], new[k])
    ca, cb = ga.cull_outliers([key[0]], [key[1]], [key[2]]), gb.cull_outliers([key[0]], [key[1]], [key[2]])
    assert ca[0] == cb[0] and np.array_equal(ca[1], cb[1]) and ca[1][0] == mg.CULL_POINT_BAD      # (good count 2 <= 2: the point goes bad, as a host-appended one)
    _same(_snapshot(ta, ga), _snapshot(tb, gb))
    assert ga.get_points(int(new[k]), 1)["flags"][0] & mg.GP_BAD


def test_refusals_enqueue_nothing(gpu_required, scene):
    """10: every refusal names the call, and leaves the store's length, the table's size and a sample row's bytes as they were"""
    from mcptam_amd import chain_bundle as cb, stereo as S
    from mcptam_amd.keyframe import KeyFrame
    sc = scene
    level = 1
    cand = np.ascontiguousarray(sc["cand"][level][:30].astype(np.int32))
    n = len(cand)
    t, g = _world(sc, track=False)
    L = S.lib()
    tab, cams = S._targets(_targets(sc, [0, 1]))
    cs = sc["cam"].to_struct()
    sp = S._pose12(sc["pose_src"])
    out = np.zeros(n, dtype=S.STEREO_POINT_DTYPE); keep = np.zeros(n, dtype=np.uint8)
    rows, keys = _rows_keys(n)
    tm, tc = TARGET_MKF[:2].copy(), TARGET_CAM[:2].copy()
    one = S.make_meas(np.ones((1, 2)), [1])
    res = S.StereoMapResult()

    def call(graph=g._h, src=sc["src"]._h, level=level, nc=n, meas=None, ntar=2, tabp=tab, tmk=tm, tca=tc, nrows=n, rws=rows, kys=keys, prm=(SRC_MKF, SRC_CAM, 1 << 30, 1), cam=cs,
             prm_null=False, res_null=False, keep_p=keep):
        p = S.StereoMapParams(*prm)
        return L.mcp_stereo_map_points(graph, src, ctypes.addressof(cam), sp.ctypes.data, level, nc, cand.ctypes.data, 0 if meas is None else len(meas),
                                       None if meas is None else meas.ctypes.data, ntar, ctypes.addressof(tabp), None if tmk is None else tmk.ctypes.data,
                                       None if tca is None else tca.ctypes.data, nrows, None if rws is None else rws.ctypes.data, None if kys is None else kys.ctypes.data,
                                       None if prm_null else ctypes.addressof(p), None if res_null else ctypes.addressof(res), out.ctypes.data,
                                       None if keep_p is None else keep_p.ctypes.data, None)
    dead = KeyFrame(640, 480); dh = dead._h; dead.close()
    bad_cam = sc["cam"].to_struct(); bad_cam.n_inv = 99
    bad_opa = S._targets([(sc["tg"][0], sc["cam"], sc["poses"][0], -1.0), (sc["tg"][1], sc["cam"], sc["poses"][1])])[0]
    dup, neg = rows.copy(), rows.copy()
    dup[5] = dup[2]; neg[7] = -1
    cases = [dict(graph=None), dict(prm_null=True), dict(res_null=True), dict(src=None), dict(src=dh), dict(level=4), dict(level=-1), dict(nc=-1), dict(ntar=-1), dict(cam=bad_cam),
             dict(tabp=bad_opa), dict(keep_p=None),                                                                       # what mcp_stereo_points refuses
             dict(prm=(7, SRC_CAM, 9, 1)), dict(prm=(-1, SRC_CAM, 9, 1)), dict(prm=(SRC_MKF, 2, 9, 1)), dict(prm=(SRC_MKF, -1, 9, 1)),      # the source as the graph names it
             dict(tmk=np.array([1, 9], dtype=np.int32)), dict(tca=np.array([0, 2], dtype=np.int32)), dict(tmk=None), dict(tca=None),
             dict(nrows=n - 1), dict(rws=neg), dict(rws=dup), dict(rws=None), dict(kys=None),
             dict(meas=one), dict(meas=S.make_meas(np.full((1, 2), np.nan), [1]), prm=(SRC_MKF, SRC_CAM, 9, 0))]
    before = _snapshot(t, g)
    for kw in cases:
        assert L.mcp_kf_level_size(sc["src"]._h, 99, None, None) == -1 and "mcp_stereo" not in cb.last_error()      # another message first
        assert call(**kw) == -1, kw
        assert cb.last_error().startswith("mcp_stereo_map_points:"), (kw, cb.last_error())
        assert g.num_meas() == before["num_meas"] and t.rows == before["rows"], kw
        assert t.get(17, 1)[0].tobytes() == np.frombuffer(before["world_pos"], dtype=np.float64).reshape(-1, 3)[17].tobytes()
    _same(_snapshot(t, g), before)
    assert call() >= 0 and res.made >= 0 and t.rows == rows.max() + 1
    # an empty candidate list: nothing to do, nothing changes
    mid = _snapshot(t, g)
    assert call(nc=0, nrows=0) == 0 and res.made == 0
    _same(_snapshot(t, g), mid)


def test_two_runs_give_identical_bytes(gpu_required, scene):
    """11: the whole of test 5's twin A, twice"""
    sc = scene
    level, js = 1, [0, 1, 2]
    rows, keys = _rows_keys(len(sc["cand"][level]))
    runs = []
    for _ in range(2):
        t, g = _world(sc)
        pts, keep, oc, res = _one_call(sc, t, g, level, js, rows, keys)
        runs.append((pts.tobytes(), keep.tobytes(), oc.tobytes(), res, _snapshot(t, g)))
    assert runs[0][:4] == runs[1][:4]
    _same(runs[0][4], runs[1][4])
