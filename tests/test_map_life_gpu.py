"""The map's beginning, rescale and re-alignment on the device (mcp_init_depth_map_points, mcp_map_mark_optimized, mcp_map_rescale,
mcp_map_transform) on twin tables and graphs, as tests/test_stereo_map_gpu.py: one twin makes the one call, the other composes the host twins
and the public uploads; the numpy restatements of mcptam_amd.map_graph state the values.  The init-depth twins are a map of 150 tracked rows, 4
MKFs and a 2-camera rig around the scene of test_stereo_points_gpu.py; the transform twins are the synthetic maps of tests/map_life_cases.py,
whose coordinates hold no zeros (an identity motion cannot flip the sign of one).

DOUBLES.  Device and host run the same __host__ __device__ bodies without contraction (+, -, *, / and sqrt only).  They were observed to agree bit
for bit on an MI355X in every comparison of this file (profiles/map_graph/README.md), so EXACT_DOUBLES is on and the comparison against the host
twins is equality; with it off the doubles are held to 1e-12 norm-relative per vector.  The numpy restatements are always held to 1e-12."""
import ctypes

import numpy as np
import pytest

import map_life_cases as mlc

pytestmark = pytest.mark.gpu

EXACT_DOUBLES = True
SRC_MKF = 2
BASE_ROWS = 150
INIT_CASES = mlc.init_cases()
XFORM_CASES = mlc.transform_cases()
DOUBLE_KEYS = ("world_pos", "pixel_right_w", "pixel_down_w", "rays", "mkf_bfw", "mkf_depth")


# ---- the init-depth twins ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame
    sc = synth_img.make_stereo_scene()
    kfs = []
    for im in (sc["img_src"], sc["imgs"][0]):                   # the source MKF's two keyframes (camera 0, camera 1)
        k = KeyFrame(640, 480)
        k.MakeKeyFrame_Lite(im); k.MakeKeyFrame_Rest()
        kfs.append(k)
    pts = synth_img.make_map_points(sc["cam"], kfs[0], None, sc["pose_src"], sc["depth"], per_level=(60, 40, 30, 20))
    assert len(pts) == BASE_ROWS
    sc.update(kfs=kfs, pts=pts, cams=mlc.cameras())
    return sc


def _base_store(n_rows=BASE_ROWS, seed=3):
    """two entries per row under the MKFs 0, 1 and 3: none of the source MKF's, so the call's busy lists are the case's own"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n_rows), 2)
    k = r + np.tile([0, 1], n_rows)
    return dict(mkf=np.array([0, 1, 3])[k % 3].astype(np.int32), cam=(k % 2).astype(np.int32), row=r.astype(np.int32), uv=rng.uniform([0, 0], [640, 480], (2 * n_rows, 2)),
                level=rng.integers(0, 4, 2 * n_rows).astype(np.int32), source=np.tile([2, 0], n_rows).astype(np.int32))


def _world(sc, busy=None, base=True, dead_on=None, track=True):
    """A table of BASE_ROWS tracked points (their finders of camera 0 have seen a frame) and a graph of 4 present MKFs at general poses with a
    2-camera rig.  The store: the base entries (base), then the busy positions of (SRC_MKF, c) one per row from row 0 on, then -- dead_on: (cam,
    level positions, level) -- entries of the source keyframe that are erased again: they may not thin."""
    from mcptam_amd import map_graph as mg, synth_img
    from mcptam_amd.pvs import MapPointTable
    pts = sc["pts"]
    n = len(pts)
    t = MapPointTable()
    wp, pr, pd = synth_img.points_soa(pts)
    t.set(wp, pr, pd, np.ones(n, dtype=np.uint8))
    t.set_source(np.arange(n, dtype=np.int32) * 3 + 7, [sc["kfs"][0]] * n, [p["source_level"] for p in pts], [p["center"] for p in pts])
    if track:
        t.track_map([sc["kfs"][1]], [sc["cam"]], sc["poses"][0], [(np.eye(3), np.zeros(3))], seed=11)
    g = mg.MapGraph(t, mlc.rig())
    g.set_mkfs(mlc.mkf_poses(4), np.full(4, mg.MKF_PRESENT, dtype=np.int32), np.ones((4, 2), dtype=np.uint8), np.full((4, 2), 6.0))
    g.update_points(np.arange(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
    if base:
        s = _base_store()
        g.add_meas(s["mkf"], s["cam"], s["row"], s["uv"], s["level"], s["source"])
        d = np.array([5, 40, 41, 200, 299])
        assert g.erase_meas(s["mkf"][d], s["cam"][d], s["row"][d]) == len(d)
    row = 0
    for c, b in enumerate(busy or []):
        if len(b):
            assert row + len(b) <= n
            g.add_meas(np.full(len(b), SRC_MKF), np.full(len(b), c), np.arange(row, row + len(b)), b["root_pos"], b["level"], np.zeros(len(b), dtype=np.int32))
            row += len(b)
    if dead_on is not None:
        from mcptam_amd import stereo as S
        c, pos, level = dead_on
        k = len(pos)
        assert row + k <= n
        g.add_meas(np.full(k, SRC_MKF), np.full(k, c), np.arange(row, row + k), S.level_zero_pos(pos, level), np.full(k, level), np.zeros(k, dtype=np.int32))
        assert g.erase_meas(np.full(k, SRC_MKF), np.full(k, c), np.arange(row, row + k)) == k
    return t, g


def _store_of(g):
    from mcptam_amd import map_graph as mg
    m = g.get_meas()
    s = np.zeros(len(m["mkf"]), dtype=mg.STORE_ENTRY_DTYPE)
    for k in ("mkf", "cam", "row", "uv", "level", "source", "alive"):
        s[k] = m[k]
    return s


def _snapshot(t, g, states=True):
    """every read-back of the table, the graph and the store as arrays"""
    snap = dict(rows=np.array([t.rows]), num_meas=np.array(g.num_meas()), check=np.array(g.check()))
    for k, v in zip(("world_pos", "pixel_right_w", "pixel_down_w", "usable"), t.get()):
        snap[k] = v
    snap["inlier"], snap["outlier"] = t.get_counts()
    snap["rays"], snap["has_rays"] = t.get_rays()
    for k, v in t.get_source().items():
        snap["src_" + k] = v
    if states:
        snap["states0"] = t.get_states(0)
    for k, v in g.get_points().items():
        snap["gp_" + k] = v
    snap["store"] = _store_of(g)
    snap["good"] = g.good_counts()
    m = g.get_mkfs()
    snap["mkf_bfw"], snap["mkf_flags"], snap["mkf_active"], snap["mkf_depth"] = m["base_from_world"], m["flags"], m["kf_active"], m["kf_depth_mean"]
    return snap


def _same(a, b, doubles_exact=True, what=""):
    """every read-back byte for byte; with doubles_exact off the double columns are held to 1e-12 norm-relative per vector instead"""
    assert sorted(a) == sorted(b)
    for k in a:
        if k in DOUBLE_KEYS and not doubles_exact:
            w = 1 if k == "mkf_depth" else 3
            x, y = np.asarray(a[k]).reshape(-1, w), np.asarray(b[k]).reshape(-1, w)
            d = np.linalg.norm(x - y, axis=1) / np.maximum(np.linalg.norm(y, axis=1), 1e-300)
            print("%s %s: max norm-relative difference %.3g, %d of %d vectors differ in a bit" % (what, k, d.max() if len(d) else 0.0, int((x != y).any(axis=1).sum()), len(x)))
            assert mlc.rel_close(x, y), (what, k)
        else:
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def _keys(n, first=100000):
    return (first + 7 * np.arange(n)).astype(np.int32)


def _one_call(sc, t, g, c, rows=None, keys=None, **kw):
    rows = c["rows"] if rows is None else rows
    return g.add_init_depth_points(sc["kfs"], sc["cams"], c["cands"], c["limits"], rows, _keys(len(rows)) if keys is None else keys, SRC_MKF, c["level"], c["init_depth"], **kw)


def _composition(sc, t, g, c, rows=None, keys=None):
    """twin B: the busy lists by mcp_stereo_busy_host, the points by mcp_init_depth_points_host at the graph's own pose, then the five uploads"""
    from mcptam_amd import map_graph as mg, stereo as S
    rows = c["rows"] if rows is None else rows
    keys = _keys(len(rows)) if keys is None else keys
    store = _store_of(g)
    first = g.num_meas()[1]
    busy = [S.stereo_busy_host(store, SRC_MKF, cam) if len(c["cands"][cam]) else S.make_meas(np.zeros((0, 2)), []) for cam in range(2)]
    h = mg.init_depth_host(mlc.rig(), g.get_mkfs(SRC_MKF, 1)["base_from_world"][0], sc["cams"], c["cands"], c["limits"], busy, rows, SRC_MKF, c["level"], c["init_depth"], first)
    made = h["made_total"]
    if len(rows):
        t.resize(max(t.rows, int(np.max(rows)) + 1))              # (the host assigned the rows: the table covers them)
    r = rows[:made]
    if made:
        pts = h["points"]
        cam_of = np.repeat([0, 1], h["made"])
        t.update(r, h["world_pos"], h["pixel_right_w"], h["pixel_down_w"], np.zeros(made, dtype=np.uint8))
        t.update_rays(r, h["rays"][:, :3], h["rays"][:, 3:6], h["rays"][:, 6:])
        t.update_counts(r, np.ones(made, dtype=np.int32), np.zeros(made, dtype=np.int32))
        t.update_source(r, keys[:made], [sc["kfs"][cam] for cam in cam_of], np.full(made, c["level"]), h["center_xy"])
        g.update_points(r, h["gp_src_mkf"], h["gp_src_cam"], h["gp_flags"])
        ap = h["appended"]
        g.add_meas(ap["mkf"], ap["cam"], ap["row"], ap["uv"], ap["level"], ap["source"])
        assert np.array_equal(pts["candidate"], np.concatenate([np.flatnonzero(h["keep"][cam])[:h["made"][cam]] for cam in range(2)]))
    res = dict(made_total=made, first_store=first, made=h["made"], n_busy=[len(b) for b in busy], n_alive=h["n_alive"])
    return h["points"], h["keep"], res


def _check_against_ref(sc, t, g, c, pts, keep, res, rows=None):
    """the records, the rows and the store's tail are what init_depth_ref says, at 1e-12 norm-relative for the doubles"""
    from mcptam_amd import map_graph as mg
    rows = c["rows"] if rows is None else rows
    w = mg.init_depth_ref(mlc.rig(), mlc.mkf_poses(4)[SRC_MKF], sc["cams"], c["cands"], c["limits"], c["busy"], rows, SRC_MKF, c["level"], c["init_depth"], res["first_store"])
    made = w["made_total"]
    assert res["made_total"] == made and res["made"] == w["made"] and res["n_alive"] == w["n_alive"] and res["n_busy"] == w["n_busy"]
    for a, b in zip(keep, w["keep"]):
        assert np.array_equal(a, b)
    for k in ("candidate", "target", "hypothesis", "score", "root_pos", "target_pos"):
        assert pts[k].tobytes() == w["points"][k].tobytes(), k
    assert g.num_meas()[1] == w["store_end"] and _store_of(g)[res["first_store"]:].tobytes() == w["appended"].tobytes()
    r = rows[:made]
    wp, pr, pd, us = t.get()
    rays, has = t.get_rays()
    src, gp = t.get_source(), g.get_points()
    inl, outl = t.get_counts()
    for got, k in ((us, "usable"), (inl, "inlier"), (outl, "outlier"), (src["level"], "source_level"), (src["center"], "center_xy"), (src["fixed"], "fixed"),
                   (gp["src_mkf"], "gp_src_mkf"), (gp["src_cam"], "gp_src_cam"), (gp["flags"], "gp_flags")):
        assert got[r].tobytes() == w[k].tobytes(), k
    for got, k in ((wp, "world_pos"), (pr, "pixel_right_w"), (pd, "pixel_down_w")):
        assert mlc.rel_close(got[r], w[k]), k
        assert got[r].tobytes() == pts[k].tobytes(), k              # the record handed back is the row
    assert mlc.rel_close(rays[r].reshape(-1, 3), w["rays"].reshape(-1, 3))
    assert has[r].all() and src["has_source"][r].all() and np.array_equal(src["key"][r], _keys(len(rows))[:made])
    assert (g.good_counts()[r] == 1).all()


@pytest.mark.parametrize("c", INIT_CASES, ids=[c["name"] for c in INIT_CASES])
def test_init_depth_equals_the_composition(gpu_required, scene, c):
    """one call on twin A = busy host + init-depth host + the uploads on twin B, every read-back, and both = init_depth_ref.  The seams are the
    cases' (tests/map_life_cases.py): 0 and 1 candidates, limit 0, limit past the survivors, 600 candidates cut at 255 / 256 / 257, camera 1's
    rows right behind camera 0's made, level 3, busy positions on both sides of the radius; rows past the table's end, out of order, with gaps."""
    sc = scene
    dead = (0, c["cands"][0][-3:], c["level"]) if len(c["cands"][0]) >= 3 else None      # dead entries on top of three candidates: they do not thin
    (ta, ga), (tb, gb) = _world(sc, c["busy"], dead_on=dead), _world(sc, c["busy"], dead_on=dead)
    before = _snapshot(ta, ga)
    _same(before, _snapshot(tb, gb))
    pa, ka, ra = _one_call(sc, ta, ga, c)
    pb, kb, rb = _composition(sc, tb, gb, c)
    assert ra == rb, (ra, rb)
    for a, b in zip(ka, kb):
        assert np.array_equal(a, b)
    A, B = _snapshot(ta, ga), _snapshot(tb, gb)
    _same(A, B, doubles_exact=EXACT_DOUBLES, what=c["name"])
    for k in pa.dtype.names:
        if pa[k].dtype.kind == "f" and not EXACT_DOUBLES:
            assert mlc.rel_close(pa[k], pb[k]), k
        else:
            assert pa[k].tobytes() == pb[k].tobytes(), k
    made = ra["made_total"]
    assert A["check"][0] == 0 and A["num_meas"][1] == ra["first_store"] + made and A["rows"][0] == max(BASE_ROWS, c["rows"].max() + 1)
    _check_against_ref(sc, ta, ga, c, pa, ka, ra)
    if "expect_keep" in c:
        for a, b in zip(ka, c["expect_keep"]):
            assert np.array_equal(a, b)
    # the rows handed in and not taken, and every old row, keep their bytes
    left = c["rows"][made:]
    assert not A["usable"][left].any() and not A["has_rays"][left].any() and not A["src_has_source"][left].any() and (A["good"][left] == 0).all()
    for k in ("world_pos", "pixel_right_w", "pixel_down_w", "usable", "inlier", "outlier", "src_key", "states0", "gp_src_mkf", "gp_flags", "mkf_bfw", "mkf_depth"):
        assert A[k][:BASE_ROWS if not k.startswith("mkf") else None].tobytes() == before[k][:BASE_ROWS if not k.startswith("mkf") else None].tobytes(), k
    assert A["store"][:ra["first_store"]].tobytes() == before["store"].tobytes()


def test_init_depth_into_an_empty_store_and_twice(gpu_required, scene):
    """an empty store: no gather has anything to read; the same call on a fresh twin gives the same bytes"""
    sc = scene
    c = INIT_CASES[2]
    runs = []
    for _ in range(2):
        t, g = _world(sc, base=False)
        assert g.num_meas() == (0, 0)
        pts, keep, res = _one_call(sc, t, g, c)
        assert res["first_store"] == 0 and res["n_busy"] == [0, 0] and res["made_total"] == sum(len(x) for x in c["cands"]) == g.num_meas()[1]
        _check_against_ref(sc, t, g, dict(c, busy=[np.zeros(0, dtype=c["busy"][0].dtype)] * 2), pts, keep, res)
        runs.append((pts.tobytes(), [k.tobytes() for k in keep], res, _snapshot(t, g)))
    assert runs[0][:3] == runs[1][:3]
    _same(runs[0][3], runs[1][3])


def test_second_call_is_thinned_by_the_first(gpu_required, scene):
    """a call at level 2, then one at level 1 whose candidates sit on the first call's points: the level + 1 rule thins them through the entries the
    first call left in the store, and twin B (host twins + uploads) agrees"""
    from mcptam_amd import stereo as S
    sc = scene
    c2 = dict(level=2, cands=[mlc.grid_candidates(12, 2, step=30), mlc.grid_candidates(5, 2, step=30)], limits=[8, 5], init_depth=2.0, rows=np.arange(200, 213, dtype=np.int32))
    first = c2["cands"][0]
    on_top = (2 * first + 1).astype(np.int32)                  # ir_rounded(LevelZeroPos(c, 2) / 2) = 2 c + 1
    far = on_top + np.array([20, 0], dtype=np.int32)
    c1 = dict(level=1, cands=[np.concatenate([on_top, far]).astype(np.int32), (2 * c2["cands"][1] + 1 + np.array([6, 8])).astype(np.int32)], limits=[100, 100], init_depth=2.0,
              rows=np.arange(300, 329, dtype=np.int32))
    (ta, ga), (tb, gb) = _world(sc), _world(sc)
    pa, ka, ra = _one_call(sc, ta, ga, c2)
    pb, kb, rb = _composition(sc, tb, gb, c2)
    assert ra == rb and ra["made"] == [8, 5]
    pa, ka, ra = _one_call(sc, ta, ga, c1, keys=_keys(29, 500000))
    pb, kb, rb = _composition(sc, tb, gb, c1, keys=_keys(29, 500000))
    assert ra == rb and ra["n_busy"] == [8, 5]
    want0 = np.concatenate([np.arange(12) >= 8, np.ones(12, dtype=bool)])      # the eight candidates on created points go; the four on uncreated ones and the far ones stay
    assert np.array_equal(ka[0], want0) and np.array_equal(kb[0], want0) and ka[1].all()      # (camera 1's sit at squared distance 100 from its points)
    assert ra["made"] == [16, 5]
    _same(_snapshot(ta, ga), _snapshot(tb, gb), doubles_exact=EXACT_DOUBLES, what="second call")
    assert np.array_equal(ka[0], S.thin_candidates(c1["cands"][0], 1, S.level_zero_pos(first[:8], 2), np.full(8, 2)))


def test_recycled_rows_keep_or_forget_their_finders(gpu_required, scene):
    """two rows of the old map are handed in again: one under a new key (every camera's finder state of the row is zeroed), one under the key it
    holds (the state is kept); both get the new source, counts (1, 0) and usable 0"""
    sc = scene
    t, g = _world(sc, base=False)
    st0 = t.get_states(0)
    seen = np.flatnonzero(st0["valid"] != 0)
    new_key_row, same_key_row = int(seen[0]), int(seen[1])
    old_keys = t.get_source()["key"]
    t.update_counts([new_key_row, same_key_row], [5, 6], [3, 2])
    c = dict(level=1, cands=[mlc.grid_candidates(4, 1, step=30), mlc.grid_candidates(0, 1)], limits=[4, 0], init_depth=1.5)
    rows = np.array([new_key_row, 400, same_key_row, 170], dtype=np.int32)
    keys = np.array([777777, 5, old_keys[same_key_row], 6], dtype=np.int32)
    pts, keep, res = _one_call(sc, t, g, c, rows=rows, keys=keys)
    assert res["made"] == [4, 0] and t.rows == 401
    st1 = t.get_states(0)
    assert st0[new_key_row:new_key_row + 1].tobytes().strip(b"\0") and not st1[new_key_row:new_key_row + 1].tobytes().strip(b"\0")
    assert st1[same_key_row:same_key_row + 1].tobytes() == st0[same_key_row:same_key_row + 1].tobytes()
    others = np.setdiff1d(np.arange(BASE_ROWS), [new_key_row, same_key_row])
    assert st1[others].tobytes() == st0[others].tobytes()
    src = t.get_source()
    assert np.array_equal(src["key"][rows], keys) and (src["level"][rows] == 1).all() and np.array_equal(src["center"][rows], c["cands"][0]) and src["has_source"][rows].all()
    assert [a[rows].tolist() for a in t.get_counts()] == [[1] * 4, [0] * 4] and not t.get()[3][rows].any()
    gap = np.setdiff1d(np.arange(BASE_ROWS, 400), [170])
    assert not t.get()[3][gap].any() and not t.get_rays()[1][gap].any()


def test_init_depth_refusals_change_nothing(gpu_required, scene):
    """every refusal names the call and leaves the table, the graph and the store byte-identical"""
    from mcptam_amd import chain_bundle as cb, map_graph as mg
    from mcptam_amd.keyframe import KeyFrame
    sc = scene
    t, g = _world(sc, track=False)
    L = mg._life_lib()
    cand = [np.ascontiguousarray(mlc.grid_candidates(20, 1)), np.ascontiguousarray(mlc.grid_candidates(7, 1))]
    structs = [c.to_struct() for c in sc["cams"]]
    bad_cam = sc["cams"][0].to_struct(); bad_cam.n_inv = 99
    outside = cand[0].copy(); outside[3] = (320, 5)            # level 1 is 320 wide
    rows = (BASE_ROWS + np.arange(27) * 2).astype(np.int32)
    keys = _keys(27)
    dup, neg = rows.copy(), rows.copy()
    dup[5] = dup[2]; neg[7] = -1
    dead = KeyFrame(640, 480); dh = dead._h; dead.close()
    empty = KeyFrame(640, 480)
    out = np.zeros(27, dtype=mg._point_dtype()); keep = np.zeros(27, dtype=np.uint8)
    res = mg.InitDepthResult()

    def call(graph=g._h, ncam=2, srcs=(sc["kfs"][0]._h, sc["kfs"][1]._h), cams=structs, cands=cand, ncand=None, limits=(20, 7), nrows=27, rws=rows, kys=keys, prm=(SRC_MKF, 1, 2.0),
             tab_null=False, prm_null=False, res_null=False, keep_p=keep):
        tab = (mg.InitDepthCam * 2)()
        for c in range(2):
            tab[c].src, tab[c].cam, tab[c].cand, tab[c].limit = srcs[c], ctypes.addressof(cams[c]), cands[c].ctypes.data, limits[c]
            tab[c].n_cand = len(cands[c]) if ncand is None else ncand[c]
        p = mg.InitDepthParams(*prm)
        return L.mcp_init_depth_map_points(graph, ncam, None if tab_null else ctypes.addressof(tab), nrows, None if rws is None else rws.ctypes.data,
                                           None if kys is None else kys.ctypes.data, None if prm_null else ctypes.addressof(p), None if res_null else ctypes.addressof(res),
                                           out.ctypes.data, None if keep_p is None else keep_p.ctypes.data)
    cases = [dict(graph=None), dict(prm_null=True), dict(res_null=True), dict(tab_null=True), dict(ncam=1), dict(ncam=3), dict(prm=(SRC_MKF, 4, 2.0)), dict(prm=(SRC_MKF, -1, 2.0)),
             dict(limits=(-1, 7)), dict(ncand=(20, -1)), dict(nrows=26), dict(nrows=-1), dict(prm=(SRC_MKF, 1, 0.0)), dict(prm=(SRC_MKF, 1, -2.0)), dict(prm=(SRC_MKF, 1, np.nan)),
             dict(prm=(SRC_MKF, 1, np.inf)), dict(prm=(7, 1, 2.0)), dict(prm=(-1, 1, 2.0)), dict(prm=(4096, 1, 2.0)),
             dict(srcs=(None, sc["kfs"][1]._h)), dict(srcs=(dh, sc["kfs"][1]._h)), dict(srcs=(empty._h, sc["kfs"][1]._h)), dict(cams=[bad_cam, structs[1]]),
             dict(cands=[outside, cand[1]]), dict(rws=neg), dict(rws=dup), dict(rws=None), dict(kys=None), dict(keep_p=None)]
    before = _snapshot(t, g, states=False)
    for kw in cases:
        assert L.mcp_kf_level_size(sc["kfs"][0]._h, 99, None, None) == -1 and "mcp_init_depth" not in cb.last_error()      # another message first
        assert call(**kw) == -1, kw
        assert cb.last_error().startswith("mcp_init_depth_map_points:"), (kw, cb.last_error())
        assert g.num_meas()[1] == before["num_meas"][1] and t.rows == before["rows"][0], kw
    _same(_snapshot(t, g, states=False), before)
    # no candidates at all: the arguments are checked, nothing is enqueued, nothing changes
    assert call(ncand=(0, 0), nrows=0, rws=None, kys=None, keep_p=None) == 0 and res.made_total == 0 and res.first_store == before["num_meas"][1]
    assert call(ncand=(0, 0), nrows=27) == 0
    _same(_snapshot(t, g, states=False), before)
    assert call() == 27 and res.made_total == 27 and t.rows == rows.max() + 1
    empty.close()


# ---- mark_optimized ----------------------------------------------------------------------------------------------------------------------------
def _load(a, store=True, table_rows=None):
    """a table and a graph from the flat arrays of map_life_cases.map_arrays; the store: two entries per written row under present MKFs"""
    from mcptam_amd import map_graph as mg
    from mcptam_amd.pvs import MapPointTable
    n = len(a["world_pos"])
    t = MapPointTable()
    if n:
        t.set(a["world_pos"], a["pixel_right_w"], a["pixel_down_w"], (np.arange(n) % 3 != 1).astype(np.uint8))
        has = np.flatnonzero(a["has_rays"])
        if len(has):
            t.update_rays(has, a["rays"][has, :3], a["rays"][has, 3:6], a["rays"][has, 6:])
        t.set_counts(1 + np.arange(n) % 5, np.arange(n) % 3)
    if table_rows is not None:
        t.resize(table_rows)
    g = mg.MapGraph(t, a["cam_from_base"])
    P, k = len(a["mkf_flags"]), len(a["src_mkf"])
    if P:
        g.set_mkfs(a["base_from_world"], a["mkf_flags"], a["kf_active"], a["kf_depth_mean"])
    written = np.flatnonzero(~((a["src_mkf"] == -1) & (a["pt_flags"] == mg.GP_BAD))) if k else np.zeros(0, dtype=np.int64)
    if len(written):
        g.update_points(written, a["src_mkf"][written], a["src_cam"][written], a["pt_flags"][written])
    pres = np.flatnonzero(a["mkf_flags"] & mg.MKF_PRESENT)
    if store and len(written) and len(pres):
        r = np.repeat(written, 2)
        j = np.arange(len(r))
        rng = np.random.default_rng(len(r))
        g.add_meas(pres[(r + j) % len(pres)], j % 2, r, rng.uniform([0, 0], [640, 480], (len(r), 2)), j % 4, np.zeros(len(r), dtype=np.int32))
    return t, g


def test_mark_optimized_sets_only_the_usable_bytes(gpu_required):
    """the usable bytes of written rows that are not bad change, nothing else; the count is numpy's.  300 table rows: the graph's columns cover
    257 (a workgroup seam), two of them were never written, some are bad, one is fixed"""
    from mcptam_amd import map_graph as mg
    a = mlc.map_arrays(257, never_written=(9, 256), fixed=(11,))
    a["pt_flags"][[3, 100, 255]] |= mg.GP_BAD
    t, g = _load(a, table_rows=300)
    before = _snapshot(t, g, states=False)
    flags = g.get_points()["flags"][:257]
    want_u, want_n = mg.mark_optimized_ref(before["usable"], flags)
    host_u, host_n = mg.mark_optimized_host(before["usable"], flags)
    n = g.mark_optimized()
    after = _snapshot(t, g, states=False)
    assert n == want_n == host_n == 257 - 5 and after["usable"].tobytes() == want_u.tobytes() == host_u.tobytes()
    assert (after["usable"][[3, 9, 100, 255, 256]] == before["usable"][[3, 9, 100, 255, 256]]).all()      # bad or never written: left alone
    assert (after["usable"][257:] == 0).all() and after["usable"][11] == 1
    for k in before:
        if k != "usable":
            assert after[k].tobytes() == before[k].tobytes(), k
    assert g.mark_optimized() == n                              # again: the same rows, the same bytes
    assert _snapshot(t, g, states=False)["usable"].tobytes() == after["usable"].tobytes()
    # an empty table
    t0, g0 = _load(mlc.map_arrays(0, n_mkfs=2))
    assert g0.mark_optimized() == 0


# ---- rescale and transform ---------------------------------------------------------------------------------------------------------------------
def _arrays_of(t, g, a):
    """the flat arrays map_transform_ref takes, from the device's state"""
    wp, pr, pd, _ = t.get()
    rays, has = t.get_rays()
    gp, m = g.get_points(), g.get_mkfs(0, len(a["mkf_flags"]))
    return dict(ncam=2, cam_from_base=a["cam_from_base"], base_from_world=m["base_from_world"], mkf_flags=m["flags"], src_mkf=gp["src_mkf"], src_cam=gp["src_cam"], has_rays=has,
                rays=rays, world_pos=wp, pixel_right_w=pr, pixel_down_w=pd)


def _present(a):
    from mcptam_amd import map_graph as mg
    return np.flatnonzero(a["mkf_flags"] & mg.MKF_PRESENT)


@pytest.mark.parametrize("c", XFORM_CASES, ids=[c["name"] for c in XFORM_CASES])
def test_transform_and_rescale_equal_numpy_and_the_host_twin(gpu_required, c):
    """3, 5: a general rigid motion, then a general scale: world positions, poses and pixel vectors agree with map_transform_ref to 1e-12
    norm-relative and with the host twin (EXACT_DOUBLES: bit for bit), the counters are exact, and everything else keeps every byte -- the empty
    table, 1 / 255 / 256 / 257 rows, a non-present slot between present ones, a bad present MKF, rows without rays, rows never written, a fixed
    point, columns shorter than the table, no present slot"""
    from mcptam_amd import map_graph as mg
    a = c["a"]
    n = len(a["world_pos"])
    t, g = _load(a, table_rows=n + 3 if c["name"] == "mixed" else None)
    R, tr = mlc.general_motion()
    for kw in (dict(new_from_old=(R, tr)), dict(scale=1.7)):
        before = _snapshot(t, g, states=False)
        now = _arrays_of(t, g, a)
        (want, wc), (host, hc) = mg.map_transform_ref(now, **kw), mg.map_transform_host(now, **kw)
        if "scale" in kw:
            res, depth = g.rescale(kw["scale"])
            assert len(depth) == 2 * len(_present(a))
        else:
            res = g.transform(R, tr)
        assert res == wc == hc, (res, wc)
        after = _snapshot(t, g, states=False)
        P = len(a["mkf_flags"])
        got = dict(base_from_world=after["mkf_bfw"][:P], world_pos=after["world_pos"], pixel_right_w=after["pixel_right_w"], pixel_down_w=after["pixel_down_w"])
        for k in ("world_pos", "pixel_right_w", "pixel_down_w"):
            assert mlc.rel_close(got[k], want[k]), (k, kw)
        assert mlc.rel_close(got["base_from_world"].reshape(-1, 3), want["base_from_world"].reshape(-1, 3))
        for k in got:
            same = got[k].tobytes() == host[k].tobytes()
            print("%s %s %s: device == host twin bit for bit: %s" % (c["name"], list(kw)[0], k, same))
            assert same or not EXACT_DOUBLES, k
        assert np.array_equal(g.base_from_world[:P], after["mkf_bfw"][:P])         # the class's own mirror follows
        # what may not change
        for k in before:
            if k in ("world_pos", "pixel_right_w", "pixel_down_w", "mkf_bfw") or (k == "mkf_depth" and "scale" in kw):
                continue
            assert after[k].tobytes() == before[k].tobytes(), (k, kw)
        sm, sc_, ok = mg._row_sources(now, t.rows)
        has = now["has_rays"].astype(bool)
        assert after["world_pos"][~ok].tobytes() == before["world_pos"][~ok].tobytes()
        for k in ("pixel_right_w", "pixel_down_w"):
            assert after[k][~(ok & has)].tobytes() == before[k][~(ok & has)].tobytes(), k
        absent = np.setdiff1d(np.arange(mg.MAX_MKFS), _present(a))
        assert after["mkf_bfw"][absent].tobytes() == before["mkf_bfw"][absent].tobytes() and after["mkf_depth"][absent].tobytes() == before["mkf_depth"][absent].tobytes()
    if c["name"] == "mixed":
        assert res == dict(n_rows=153, n_refreshed=145, n_no_rays=2, n_no_source=6, n_mkfs=4)
        assert (a["mkf_flags"][3] & mg.MKF_BAD) and not np.array_equal(after["mkf_bfw"][3], a["base_from_world"][3])      # a bad present MKF moves
        assert a["pt_flags"][11] == mg.GP_FIXED and after["world_pos"][11].tobytes() == want["world_pos"][11].tobytes() != a["world_pos"][11].tobytes()      # a fixed point like any other


def test_identity_and_round_trips_keep_every_bit(gpu_required):
    """1, 2: after one general motion (every row refreshed) and a depth refresh, an identity transform and rescale(1.0) leave every byte of table
    and graph unchanged; rescale(2.0) then rescale(0.5) returns world_pos, base_from_world and the pixel vectors to the snapshot's bits"""
    a = mlc.map_arrays(257)
    t, g = _load(a)
    R, tr = mlc.general_motion()
    res = g.transform(R, tr)
    assert res["n_refreshed"] == 257
    g.refresh_depth(_present(a))
    snap = _snapshot(t, g, states=False)
    assert not np.array_equal(snap["world_pos"], a["world_pos"])
    assert g.transform(np.eye(3), np.zeros(3))["n_refreshed"] == 257
    _same(_snapshot(t, g, states=False), snap, what="identity")
    assert g.rescale(1.0)[0]["n_refreshed"] == 257
    _same(_snapshot(t, g, states=False), snap, what="scale 1")
    g.rescale(2.0)
    mid = _snapshot(t, g, states=False)
    assert mid["world_pos"].tobytes() == (snap["world_pos"] * 2.0).tobytes() and mid["mkf_bfw"][:4, 9:].tobytes() == (snap["mkf_bfw"][:4, 9:] * 2.0).tobytes()
    assert mid["mkf_bfw"][:, :9].tobytes() == snap["mkf_bfw"][:, :9].tobytes() and mid["mkf_depth"].tobytes() != snap["mkf_depth"].tobytes()
    g.rescale(0.5)
    back = _snapshot(t, g, states=False)
    for k in ("world_pos", "mkf_bfw", "mkf_depth", "pixel_right_w", "pixel_down_w", "usable", "rays", "store", "gp_flags"):
        assert back[k].tobytes() == snap[k].tobytes(), k


def test_rescale_depths_equal_a_refresh_afterwards(gpu_required):
    """4: depth_out and the slots' stored means equal, bit for bit, an mcp_graph_refresh_depth over all present slots made afterwards on the same
    state; a non-present slot between present ones keeps its bytes"""
    from mcptam_amd import map_graph as mg
    a = mlc.map_arrays(300, n_mkfs=5, absent=(2,), bad_mkfs=(3,), no_rays=(4,))
    t, g = _load(a)
    before = g.get_mkfs(0, 5)
    res, depth = g.rescale(0.37)
    assert res["n_mkfs"] == 4 and len(depth) == 8 and (depth["refreshed"] == 1).all() and (depth["n"] > 3).all()
    stored = g.get_mkfs(0, 5)
    pres = _present(a)
    again = g.refresh_depth(pres)
    assert depth.tobytes() == again.tobytes()
    assert stored["kf_depth_mean"][pres].tobytes() == depth["mean"].reshape(4, 2).tobytes() == g.get_mkfs(0, 5)["kf_depth_mean"][pres].tobytes()
    assert stored["kf_depth_mean"][2].tobytes() == before["kf_depth_mean"][2].tobytes() and stored["base_from_world"][2].tobytes() == before["base_from_world"][2].tobytes()
    assert not np.array_equal(stored["kf_depth_mean"][pres], before["kf_depth_mean"][pres])
    t2, g2 = _load(a)                                            # (the lists are the ones a refresh before the rescale walks)
    assert np.array_equal(depth["n"], g2.refresh_depth(pres)["n"])


def test_a_select_after_a_transform_picks_the_same(gpu_required):
    """6: mcp_map_bundle_select returns the same integer selection before and after a transform and a rescale"""
    from mcptam_amd import map_graph as mg
    a = mlc.map_arrays(150, n_mkfs=5, absent=(2,), no_rays=(4, 77), never_written=(9,), fixed=(11,))
    t, g = _load(a)
    prm = mg.select_params(mg.BUNDLE_ALL, min_points=1)

    def pick():
        res, mkfs, points, meas = g.select_raw(prm)
        assert res.status == 0
        return (res.as_dict()["status"], mkfs.tobytes(), tuple(points[k].tobytes() for k in ("row", "src_mkf", "src_cam", "fixed")),
                tuple(meas[k].tobytes() for k in ("mkf", "cam", "point", "level", "source")), len(points))
    first = pick()
    assert first[4] > 100
    R, tr = mlc.general_motion()
    g.transform(R, tr)
    assert pick() == first
    g.rescale(3.0)
    assert pick() == first
    rp = mg.select_params(mg.BUNDLE_RECENT, newest=0, n_recent=2, recent_min_size=2, min_points=1)      # the distances move with the map: the closest stay the closest
    r0 = g.select_raw(rp)
    g.transform(R.T, -(R.T @ tr))
    r1 = g.select_raw(rp)
    assert r0[0].status == r1[0].status == 0 and list(r0[0].closest) == list(r1[0].closest) and r0[1].tobytes() == r1[1].tobytes()


def test_transform_refusals_change_nothing(gpu_required):
    from mcptam_amd import chain_bundle as cb, map_graph as mg
    a = mlc.map_arrays(40)
    t, g = _load(a)
    L = mg._life_lib()
    res = mg.MapTransformResult()
    eye = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.25, -1.0])
    skew, nan = eye.copy(), eye.copy()
    skew[1] = 1e-6; nan[4] = np.inf
    before = _snapshot(t, g, states=False)
    calls = [("mcp_map_rescale", lambda: L.mcp_map_rescale(None, 2.0, ctypes.addressof(res), None)), ("mcp_map_rescale", lambda: L.mcp_map_rescale(g._h, 2.0, None, None))]
    calls += [("mcp_map_rescale", lambda s=s: L.mcp_map_rescale(g._h, s, ctypes.addressof(res), None)) for s in (0.0, -1.0, np.nan, np.inf)]
    calls += [("mcp_map_transform", lambda: L.mcp_map_transform(None, eye.ctypes.data, ctypes.addressof(res))), ("mcp_map_transform", lambda: L.mcp_map_transform(g._h, eye.ctypes.data, None)),
              ("mcp_map_transform", lambda: L.mcp_map_transform(g._h, None, ctypes.addressof(res)))]
    calls += [("mcp_map_transform", lambda T=T: L.mcp_map_transform(g._h, T.ctypes.data, ctypes.addressof(res))) for T in (skew, nan)]
    for name, call in calls:
        assert call() == -1, name
        assert cb.last_error().startswith(name + ":"), cb.last_error()
    _same(_snapshot(t, g, states=False), before)
    assert L.mcp_map_transform(g._h, eye.ctypes.data, ctypes.addressof(res)) == 0 and res.n_refreshed == 40
