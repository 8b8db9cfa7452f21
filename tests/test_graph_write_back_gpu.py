"""The keyframe lists built on the device from the map graph's store, and the one-call write-back over the graph (include/mcp_img.h mcp_graph_*):
mcp_graph_debug_kf_lists against the numpy restatement of the read-back store, exactly, on the shared cases and at the size seams of the
passes (a tile is 256 entries, the default grid has up to 64 chunks) for every grid; mcp_graph_write_back against mcp_ba_write_back fed the
restated lists, byte for byte; the graph in step with what was written (a select right behind, mcp_graph_refresh_depth); the refusals; and
the existing calls unchanged by the new ones.

Nothing new is inexact: mean / sigma against the reference's sorted-order sums keep the bound stated for mcp_scene_depth_robust in
include/mcp_img.h (checked in tests/test_write_back_gpu.py::test_scene_depth); every comparison below is of bytes."""
import ctypes

import numpy as np
import pytest

import graph_list_cases as lc
import map_graph_cases as mc
from mcptam_amd import map_graph as mg

pytestmark = pytest.mark.gpu

CASES = lc.all_cases()
TILE, CHUNKS = mg.LIST_BLOCK, mg.LIST_MAX_BLOCKS


def _device(a, n_rows):
    """(table, graph) holding the case: the graph columns of `a`, its store (dead entries added and erased), its count column."""
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    load = int(a.get("load_rows", n_rows))
    if load:
        wp = np.zeros((load, 3)); wp[:len(a["world_pos"])] = a["world_pos"]
        t.set(wp, np.zeros((load, 3)), np.zeros((load, 3)), np.ones(load, dtype=np.uint8))
    g = mg.MapGraph(t, a["cam_from_base"])
    g.load_arrays(a)
    if a.get("inlier") is not None:
        t.set_counts(a["inlier"], a["outlier"])
    if load != n_rows:
        t.resize(n_rows)
    return t, g


def _read_back(t, g, a):
    """The flat arrays with the store and the count column as the device holds them."""
    b = mg.copy_arrays(a)
    m = g.get_meas()
    b.update(ms_mkf=m["mkf"], ms_cam=m["cam"], ms_row=m["row"], ms_uv=m["uv"], ms_level=m["level"], ms_source=m["source"], ms_alive=m["alive"])
    b["inlier"], b["outlier"] = t.get_counts()
    return b


@pytest.mark.parametrize("name,a,slots,n_rows", CASES, ids=[c[0] for c in CASES])
def test_lists_equal_the_restatement(gpu_required, name, a, slots, n_rows):
    t, g = _device(a, n_rows)
    assert t.rows == n_rows
    want = mg.kf_lists_ref(_read_back(t, g, a), slots, n_rows)
    lc.assert_same_lists(g.debug_kf_lists(slots), want)
    lc.assert_same_lists(want, mg.kf_lists_host(a, slots, n_rows))       # (the host twin saw the arrays the store was filled from)
    g.close(); t.close()


def _seam_map(seed, M):
    """M entries over 40 MKFs x 4 cameras and 700 rows: every fifth dead, bad rows, inactive keyframes, seeded counts."""
    a = lc.hand(100 + seed, 40, 4, 700, M)
    a["ms_alive"][4::5] = 0
    a["pt_flags"][::9] |= mg.GP_BAD
    a["kf_active"][::7, 1] = 0
    return a


# one below, at and one above the tile; the same around tile x the default grid's 64 chunks; a store with three tiles in every chunk
SEAMS = [TILE - 1, TILE, TILE + 1, TILE * CHUNKS - 1, TILE * CHUNKS, TILE * CHUNKS + 1, 40037]


@pytest.mark.parametrize("M", SEAMS)
def test_seams_and_grids(gpu_required, M):
    a = _seam_map(SEAMS.index(M), M)
    slots = np.random.default_rng(M).permutation(40)
    t, g = _device(a, 700)
    assert g.num_meas()[1] == M
    if M == SEAMS[-1]:
        assert -(-M // CHUNKS) > 2 * TILE                               # three tiles per chunk of the default grid

    def check():
        want = mg.kf_lists_ref(_read_back(t, g, a), slots, 700)
        first = g.debug_kf_lists(slots)
        lc.assert_same_lists(first, want)
        for blocks in (1, 2, 3, 0, 0, CHUNKS):                          # forced grids, the default twice in a row, the largest
            lc.assert_same_lists(g.debug_kf_lists(slots, blocks), first)
        return first
    before = check()
    assert len(before[1]) > 0 or M < 300
    live = np.flatnonzero(_read_back(t, g, a)["ms_alive"])[::3]
    assert g.erase_meas(a["ms_mkf"][live], a["ms_cam"][live], a["ms_row"][live]) == len(live)
    erased = check()
    assert len(erased[1]) <= len(before[1])
    g.compact()
    assert g.num_meas()[0] == g.num_meas()[1] < M or M < 3
    lc.assert_same_lists(check(), erased)                               # a stable compaction keeps every list
    g.close(); t.close()


# ---- the write-back ------------------------------------------------------------------------------------------------------------------------
class Twin:
    pass


def _bytes(cols):
    return b"".join(np.ascontiguousarray(c).tobytes() for c in cols)


def _pose12(b, pid):
    R, t = b.GetPose(int(pid))
    return np.concatenate([R.ravel(), t])


def _graph_arrays(w, rng):
    """The graph of test_write_back_gpu's smallest world: the solver's rig (the contract of mcp_graph_write_back), the MKFs at their poses
    before the adjustment, a column per table row (the bundle's points at their rows, the extra rows as points outside the bundle, the last
    row never written), the bundle's measurements plus three extra rows per keyframe, and three keyframes made special:
      (0, 0)  exactly three kept entries (one more dead, one more on the bad last row): left alone;
      (1, 0)  four entries whose depth is not finite -- the mean is not finite, refreshed == -1: left alone.  (Four entries whose weights are
              all zero would do the same, but cannot be formed here: the count column refuses inlier < 1, so no weight made from it is 0.
              Zero weights through the caller's lists are tests/test_write_back_gpu.py's `zero_w`.)
      (2, C-1) inactive, with entries: an empty list, left alone."""
    p = w.p
    P, C, n_rows = p.n_mkf, len(p.cams), w.n_rows
    a0 = mg.problem_arrays(p)
    a = dict(ncam=C, cam_from_base=np.array([_pose12(w.b, i) for i in w.ids["cam"]]), base_from_world=a0["base_from_world"].copy(), mkf_flags=a0["mkf_flags"].copy(),
             kf_active=np.ones((P, C), dtype=np.uint8), kf_depth_mean=a0["kf_depth_mean"].copy())
    a["kf_active"][2, C - 1] = 0
    nan_rows, free = w.extra[:4], w.extra[4:]
    pf, sm, sc = np.full(n_rows, mg.GP_BAD, dtype=np.int32), np.zeros(n_rows, dtype=np.int32), np.zeros(n_rows, dtype=np.int32)
    pf[w.rows], sm[w.rows], sc[w.rows] = a0["pt_flags"], a0["src_mkf"], a0["src_cam"]
    pf[w.extra] = 0
    a["pt_flags"], a["src_mkf"], a["src_cam"] = pf, sm, sc
    wp = w.init["wp"].copy(); wp[nan_rows] = np.inf
    a["world_pos"] = wp
    mkf, cam, row = list(a0["ms_mkf"]), list(a0["ms_cam"]), list(w.rows[a0["ms_row"]])
    for k in range(P):
        for c in range(C):
            for r in rng.choice(free, 3, replace=False):
                mkf.append(k); cam.append(c); row.append(int(r))
    mkf, cam, row = (np.array(v, dtype=np.int32) for v in (mkf, cam, row))
    alive = np.ones(len(mkf), dtype=np.uint8)
    k3, k4 = (mkf == 0) & (cam == 0), (mkf == 1) & (cam == 0)
    e3 = np.flatnonzero(k3)
    alive[e3[4:]] = 0                                                   # ... four stay alive,
    row[e3[3]] = n_rows - 1                                             # one of them on the bad row: three kept
    keep = ~k4
    mkf, cam, row, alive = mkf[keep], cam[keep], row[keep], alive[keep]
    mkf, cam, row = np.concatenate([mkf, [1] * 4]).astype(np.int32), np.concatenate([cam, [0] * 4]).astype(np.int32), np.concatenate([row, nan_rows]).astype(np.int32)
    alive = np.concatenate([alive, np.ones(4, dtype=np.uint8)])
    order = rng.permutation(len(mkf))                                   # store order is not keyframe order
    M = len(mkf)
    a.update(ms_mkf=mkf[order], ms_cam=cam[order], ms_row=row[order], ms_alive=alive[order], ms_uv=rng.uniform(0, 480, (M, 2)), ms_level=rng.integers(0, 4, M).astype(np.int32),
             ms_source=np.zeros(M, dtype=np.int32))
    a["inlier"], a["outlier"] = rng.integers(1, 50, n_rows).astype(np.int32), rng.integers(0, 50, n_rows).astype(np.int32)
    return a


def _table(w, a):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(a["world_pos"], w.init["pr"], w.init["pd"], w.init["us"])
    t.set_rays(*w.rays)
    t.set_counts(a["inlier"], a["outlier"])
    return t


def _side(w, a):
    t = _table(w, a)
    g = mg.MapGraph(t, a["cam_from_base"])
    g.load_arrays(a)
    return t, g


def _point_args(w):
    return dict(point_ids=w.ids["point"], rows=w.rows, src_chains=w.src if w.use_src else None, src_chain_len=w.src_len if w.use_src else None)


def _graph_wb(w, g, slots, bundle=None, **over):
    kw = dict(_point_args(w), slots=slots, cam_pose_ids=w.ids["cam"])
    kw.update(over)
    if "mkf_pose_ids" not in kw:
        kw["mkf_pose_ids"] = w.ids["mkf"][slots]
    return g.write_back(bundle if bundle is not None else w.b, **kw)


def _old_wb(w, t, a_read, slots, bundle=None):
    """mcp_ba_write_back with the lists restated in numpy from the read-back store."""
    C = int(a_read["ncam"])
    ss, sr, sw = mg.kf_lists_ref(a_read, slots, w.n_rows)
    kf = np.array([[w.ids["mkf"][s], w.ids["cam"][c]] for s in slots for c in range(C)], dtype=np.int32)
    res = t.write_back(bundle if bundle is not None else w.b, kf_chains=kf, kf_chain_len=np.full(len(kf), 2, dtype=np.int32), seg_start=ss, seg_rows=sr, seg_weights=sw, **_point_args(w))
    return res, (ss, sr, sw)


def _mkf_bytes(g):
    m = g.get_mkfs()
    return _bytes(m[k] for k in ("base_from_world", "flags", "kf_active", "kf_depth_mean"))


def _meas_bytes(g):
    m = g.get_meas()
    return _bytes(m[k] for k in sorted(m))


@pytest.fixture(scope="module")
def twin(gpu_required):
    import test_write_back_gpu as twb
    w = twb._build(twb.MAPS[0])
    assert w.p.mode == "multi"
    x = Twin()
    x.w = w
    rng = np.random.default_rng(5)
    x.a = _graph_arrays(w, rng)
    P, C = w.p.n_mkf, len(w.p.cams)
    x.P, x.C = P, C
    x.slots = rng.permutation(P).astype(np.int32)
    x.S = mc.recent(x.a, n_recent=1, recent_min_size=4)
    # side A: the one call on the graph, and a select right behind it (no host wait of the test's between the two)
    x.tA, x.gA = _side(w, x.a)
    x.read = _read_back(x.tA, x.gA, x.a)
    x.mkfs_before = x.gA.get_mkfs(0, P)
    x.resA = _graph_wb(w, x.gA, x.slots)
    x.selA = x.gA.select_raw(x.S)
    x.mkfs_after = x.gA.get_mkfs(0, P)
    # side B: the existing call on a twin table, the lists restated on the host
    x.tB = _table(w, x.a)
    x.resB, x.lists = _old_wb(w, x.tB, x.read, x.slots)
    yield x
    x.gA.close(); x.tA.close(); x.tB.close(); w.b.close()


def test_write_back_equals_the_existing_call(twin):
    x = twin
    n = np.diff(x.lists[0]).reshape(x.P, x.C)
    pos = {int(s): i for i, s in enumerate(x.slots)}
    assert n[pos[0], 0] == 3 and n[pos[1], 0] == 4 and n[pos[2], x.C - 1] == 0 and n.sum() > 100
    assert _bytes(x.tA.get()) == _bytes(x.tB.get())
    for k in ("world_pos", "pixel_right_w", "pixel_down_w", "kf_cam_from_world"):
        assert x.resA[k].tobytes() == x.resB[k].tobytes(), k
    assert x.resA["depth"].tobytes() == x.resB["depth"].tobytes()
    sd = x.resA["depth"].reshape(x.P, x.C)
    assert sd["refreshed"][pos[0], 0] == 0 and sd["n"][pos[0], 0] == 3
    assert sd["refreshed"][pos[1], 0] == -1 and sd["n"][pos[1], 0] == 4 and not np.isfinite(sd["mean"][pos[1], 0])
    assert sd["refreshed"][pos[2], x.C - 1] == 0 and sd["n"][pos[2], x.C - 1] == 0
    assert (sd["refreshed"] == 1).sum() == x.P * x.C - 3


def test_poses_and_depth_means_land_in_the_graph(twin):
    x = twin
    want = np.array([_pose12(x.w.b, x.w.ids["mkf"][s]) for s in x.slots])
    assert x.resA["base_from_world"].tobytes() == want.tobytes()
    assert np.ascontiguousarray(x.mkfs_after["base_from_world"][x.slots]).tobytes() == want.tobytes()
    assert not np.array_equal(x.mkfs_after["base_from_world"], x.mkfs_before["base_from_world"])          # (the adjustment moved something)
    assert x.gA.base_from_world[:x.P].tobytes() == x.mkfs_after["base_from_world"].tobytes()              # the binding's host copy follows
    sd = x.resA["depth"].reshape(x.P, x.C)
    got, old = x.mkfs_after["kf_depth_mean"][x.slots], x.mkfs_before["kf_depth_mean"][x.slots]
    fresh = sd["refreshed"] == 1
    assert fresh.sum() > 0 and (~fresh).sum() == 3
    assert got[fresh].tobytes() == np.ascontiguousarray(sd["mean"][fresh]).tobytes()
    assert got[~fresh].tobytes() == old[~fresh].tobytes()
    for k in ("flags", "kf_active"):
        assert np.array_equal(x.mkfs_after[k], x.mkfs_before[k])


def test_a_select_right_behind_sees_the_new_state(twin):
    """The select issued behind the write-back equals a select on a twin graph that got the same poses and depth means through
    mcp_map_graph_update_mkfs (the table rows of both sides are equal bytes: test_write_back_equals_the_existing_call)."""
    x = twin
    gC = mg.MapGraph(x.tB, x.a["cam_from_base"])
    gC.load_arrays(x.a)
    sd = x.resA["depth"].reshape(x.P, x.C)
    dep = x.mkfs_before["kf_depth_mean"][x.slots].copy()
    dep[sd["refreshed"] == 1] = sd["mean"][sd["refreshed"] == 1]
    gC.update_mkfs(x.slots, x.resA["base_from_world"], x.a["mkf_flags"][x.slots], x.a["kf_active"][x.slots], np.where(x.a["kf_active"][x.slots] != 0, dep, 1.0))
    assert _mkf_bytes(gC) == _mkf_bytes(x.gA)
    selC = gC.select_raw(x.S)
    assert x.selA[0].status == 0 and x.selA[0].n_points >= 10
    assert bytes(x.selA[0]) == bytes(selC[0])
    for u, v in zip(x.selA[1:], selC[1:]):
        assert u.tobytes() == v.tobytes()
    stale = mg.MapGraph(x.tB, x.a["cam_from_base"])                      # ... and a graph left at the old poses answers differently
    stale.load_arrays(x.a)
    old = stale.select_raw(x.S)
    assert old[2]["x"].tobytes() != x.selA[2]["x"].tobytes()
    stale.close(); gC.close()


def test_refresh_depth_equals_scene_depth_robust(twin):
    """mcp_graph_refresh_depth at the graph's own poses against mcp_scene_depth_robust on the restated lists.  The poses: behind the write-back
    the graph holds the solver's poses and its rig is the solver's, so CamFromWorld_j is the chain product the write-back returned
    (k_wb_chains forms the same product: (mkf * identity) is exact, then cam * mkf)."""
    x = twin
    before = x.gA.get_mkfs(0, x.P)
    got = x.gA.refresh_depth(x.slots)
    want, _ = x.tA.scene_depth(x.resA["kf_cam_from_world"], *x.lists)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() == x.resA["depth"].tobytes()                    # (the same table, poses and lists as the write-back's last step)
    after = x.gA.get_mkfs(0, x.P)
    assert _bytes(after[k] for k in sorted(after)) == _bytes(before[k] for k in sorted(before))
    # a subset, in another order, on a graph whose poses did not come from a solver: the records of those keyframes from restated poses
    t, g = _side(x.w, x.a)
    sub = x.slots[::-1][:3]
    old = g.get_mkfs(0, x.P)
    rec = g.refresh_depth(sub).reshape(3, x.C)
    cfb, bfw = x.a["cam_from_base"], x.a["base_from_world"]
    R, tt = mg._compose(cfb[None, :, :9].reshape(1, x.C, 3, 3), cfb[None, :, 9:], bfw[sub, None, :9].reshape(3, 1, 3, 3), bfw[sub, None, 9:])
    cfw = np.concatenate([R.reshape(3 * x.C, 9), tt.reshape(3 * x.C, 3)], axis=1)
    ref, _ = t.scene_depth(cfw, *mg.kf_lists_ref(_read_back(t, g, x.a), sub, x.w.n_rows))
    assert rec.tobytes() == ref.tobytes()
    new = g.get_mkfs(0, x.P)
    fresh = rec["refreshed"] == 1
    assert new["kf_depth_mean"][sub][fresh].tobytes() == np.ascontiguousarray(rec["mean"][fresh]).tobytes()
    rest = np.ones((x.P, x.C), dtype=bool); rest[sub] = ~fresh
    assert new["kf_depth_mean"][rest].tobytes() == old["kf_depth_mean"][rest].tobytes()
    assert new["base_from_world"].tobytes() == old["base_from_world"].tobytes()
    assert x.tA.last_timing()["depth"] > 0
    g.close(); t.close()


def test_bundle_that_numbers_one_pose_chains(twin):
    """A bundle in which {mkf} alone is a chain of the solver (a point and measurements added with it, as the calibration population and the
    single-camera adjuster do): the pose of every named MKF is still found, and the call equals mcp_ba_write_back byte for byte.  The state
    is the one added (Prepare alone); the graph starts at other poses, so the copied ones show."""
    from mcptam_amd import chain_bundle
    x = twin
    w = x.w
    b = chain_bundle.ChainBundle(w.p.cams, True, True, False)
    ids = w.p.populate(b)
    assert all(np.array_equal(ids[k], w.ids[k]) for k in ("mkf", "cam", "point"))
    rng = np.random.default_rng(11)
    for k in range(x.P):
        pid = b.AddPoint([0.1 * k, -0.2, 5.0], [ids["mkf"][k]], False)
        b.AddMeas([ids["mkf"][k]], pid, rng.uniform(100, 300, 2), 1.0, 0)
        b.AddMeas([ids["mkf"][(k + 1) % x.P]], pid, rng.uniform(100, 300, 2), 1.0, 0)
    b.Prepare()
    a = mg.copy_arrays(x.a)
    a["base_from_world"] = a["base_from_world"] + 0.25
    tA, gA = _side(w, a)
    tB = _table(w, a)
    resA = _graph_wb(w, gA, x.slots, bundle=b)
    resB, _ = _old_wb(w, tB, x.read, x.slots, bundle=b)
    want = np.array([_pose12(b, ids["mkf"][s]) for s in x.slots])
    assert resA["base_from_world"].tobytes() == want.tobytes()
    assert np.ascontiguousarray(gA.get_mkfs(0, x.P)["base_from_world"][x.slots]).tobytes() == want.tobytes()
    assert want.tobytes() != np.ascontiguousarray(a["base_from_world"][x.slots]).tobytes()
    assert _bytes(tA.get()) == _bytes(tB.get())
    for k in ("world_pos", "pixel_right_w", "pixel_down_w", "kf_cam_from_world", "depth"):
        assert resA[k].tobytes() == resB[k].tobytes(), k
    # without outputs the binding's copy of the poses follows all the same
    gA.base_from_world[:] = 0.0
    _graph_wb(w, gA, x.slots, bundle=b, outputs=False)
    assert gA.base_from_world[x.slots].tobytes() == want.tobytes()
    gA.close(); tA.close(); tB.close(); b.close()


def test_a_mean_that_is_not_positive_is_not_stored(gpu_required):
    """Keyframe (0, 0) sees five points at its own centre: every depth is exactly 0, the record is refreshed with mean 0, and the graph keeps
    the depth mean it had (MultiKeyFrame::Distance needs a positive one).  Keyframe (1, 0) next to it is stored."""
    a = lc._entries(lc.hand(30, 2, 1, 6, 0), [0] * 5 + [1] * 5, [0] * 10, [0, 1, 2, 3, 4, 0, 1, 2, 3, 5])
    a["world_pos"][:5] = 0.0                                             # (identity poses: the camera centre is the origin)
    t, g = _device(a, 6)
    rec = g.refresh_depth([0, 1])
    assert rec["refreshed"].tolist() == [1, 1] and rec["n"].tolist() == [5, 5]
    assert rec["mean"][0] == 0.0 and rec["mean"][1] > 0.0
    dep = g.get_mkfs(0, 2)["kf_depth_mean"]
    assert dep[0, 0] == a["kf_depth_mean"][0, 0] == 3.0
    assert dep[1, 0].tobytes() == rec["mean"][1].tobytes()
    g.close(); t.close()


def _raises(fn, needle):
    from mcptam_amd import chain_bundle
    with pytest.raises(RuntimeError):
        fn()
    assert needle in chain_bundle.last_error(), (needle, chain_bundle.last_error())


def test_refusals(twin):
    """Argument checks only: nothing is enqueued; table rows, slot poses, depth column and store keep every byte; a valid call follows."""
    from mcptam_amd import chain_bundle
    x = twin
    w = x.w
    t, g = _side(w, x.a)
    L = mg.lib()
    snap = lambda: (_bytes(t.get()), _mkf_bytes(g), _meas_bytes(g))
    before = snap()
    n_refused = [0]

    def refused(fn, needle):
        _raises(fn, needle)
        assert snap() == before, needle
        n_refused[0] += 1
    pid, rows, slots = w.ids["point"], w.rows, x.slots
    null = (0, None, None, None, 1, None, None, None, None, 0, None, None, None, None, None, None)
    assert L.mcp_graph_write_back(None, g._h, *null) == -1 and "NULL solver handle" in chain_bundle.last_error()
    assert L.mcp_graph_write_back(w.b._h, None, *null) == -1 and "NULL graph" in chain_bundle.last_error()
    assert L.mcp_graph_refresh_depth(None, 0, None, None) == -1 and "NULL graph" in chain_bundle.last_error()
    # every refusal of mcp_ba_write_back for the parts that are kept: the handle ...
    fresh = chain_bundle.ChainBundle(w.p.cams, True, True, False)
    w.p.populate(fresh)
    refused(lambda: _graph_wb(w, g, slots, bundle=fresh), "never prepared")
    fresh.Prepare()
    fresh.SetAllReduce(lambda buf, count, stream: None, 0, 1)
    refused(lambda: _graph_wb(w, g, slots, bundle=fresh), "all-reduce hook")
    fresh.close()
    # ... required pointers ...
    one = np.zeros(1, dtype=np.int32)
    assert L.mcp_graph_write_back(w.b._h, g._h, 1, one.ctypes.data, None, None, 1, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert "is NULL" in chain_bundle.last_error()
    assert L.mcp_graph_write_back(w.b._h, g._h, 0, None, None, None, 1, None, None, None, None, 1, one.ctypes.data, None, None, None, None, None) == -1
    assert "mkf_pose_ids / cam_pose_ids is NULL" in chain_bundle.last_error()
    assert L.mcp_graph_write_back(w.b._h, g._h, 0, None, None, None, 1, None, None, None, None, 1, None, None, None, None, None, None) == -1
    assert "slots is NULL" in chain_bundle.last_error()
    assert snap() == before
    # ... ids and chains ...
    bad = pid.copy(); bad[3] = w.ids["mkf"][0]
    refused(lambda: _graph_wb(w, g, slots, point_ids=bad), "is not a point")
    src = w.src.copy(); src[1, 0] = pid[1]
    refused(lambda: _graph_wb(w, g, slots, src_chains=src, src_chain_len=w.src_len), "not a chain of poses")
    refused(lambda: _graph_wb(w, g, slots, src_chains=np.zeros((len(pid), 9), dtype=np.int32) + w.ids["mkf"][0], src_chain_len=np.full(len(pid), 9, dtype=np.int32)), "not a chain of poses")
    # ... rows
    bad = rows.copy(); bad[5] = -1
    refused(lambda: _graph_wb(w, g, slots, rows=bad), "is negative")
    bad = rows.copy(); bad[5] = bad[6]
    refused(lambda: _graph_wb(w, g, slots, rows=bad), "appears twice")
    bad = rows.copy(); bad[5] = w.n_rows - 1
    refused(lambda: _graph_wb(w, g, slots, rows=bad), "no patch rays")
    bad = rows.copy(); bad[5] = w.n_rows + 10
    refused(lambda: _graph_wb(w, g, slots, rows=bad), "no patch rays")
    # a slot out of range, not present, or repeated -- in each of the three calls
    for call in (lambda s: _graph_wb(w, g, s, mkf_pose_ids=w.ids["mkf"][np.clip(s, 0, x.P - 1)]), g.refresh_depth, g.debug_kf_lists):
        s = slots.copy(); s[1] = mg.MAX_MKFS
        refused(lambda: call(s), "is outside 0..")
        s = slots.copy(); s[1] = -1
        refused(lambda: call(s), "is outside 0..")
        s = slots.copy(); s[1] = x.P + 3
        refused(lambda: call(s), "is not present")
        s = slots.copy(); s[1] = s[4]
        refused(lambda: call(s), "appears twice")
    # a pose id that is not a pose
    ids = w.ids["mkf"][slots].copy(); ids[2] = pid[0]
    refused(lambda: _graph_wb(w, g, slots, mkf_pose_ids=ids), "is not a pose")
    ids = w.ids["mkf"][slots].copy(); ids[2] = 1 << 30
    refused(lambda: _graph_wb(w, g, slots, mkf_pose_ids=ids), "is not a pose")
    ids = w.ids["cam"].copy(); ids[-1] = pid[0]
    refused(lambda: _graph_wb(w, g, slots, cam_pose_ids=ids), "is not a pose")
    # more MKFs than the graph has slots (refused before the array is read)
    many = np.zeros(mg.MAX_MKFS + 1, dtype=np.int32)
    assert L.mcp_graph_write_back(w.b._h, g._h, 0, None, None, None, 1, None, None, None, None, len(many), many.ctypes.data, many.ctypes.data, w.ids["cam"].ctypes.data,
                                  None, None, None) == -1 and "more than MCP_MAP_MAX_MKFS" in chain_bundle.last_error()
    assert L.mcp_graph_refresh_depth(g._h, len(many), many.ctypes.data, None) == -1 and "more than MCP_MAP_MAX_MKFS" in chain_bundle.last_error()
    assert L.mcp_graph_refresh_depth(g._h, -1, many.ctypes.data, None) == -1 and "negative MKF count" in chain_bundle.last_error()
    # the debug hook's own arguments
    refused(lambda: g.debug_kf_lists(slots, blocks=mg.LIST_MAX_BLOCKS + 1), "blocks outside")
    assert snap() == before and n_refused[0] >= 25
    # ... and a good call goes through, with the results of the first one; empty calls are allowed
    res = _graph_wb(w, g, slots)
    assert _bytes(t.get()) == _bytes(x.tA.get())
    for k in ("world_pos", "kf_cam_from_world", "depth", "base_from_world"):
        assert res[k].tobytes() == x.resA[k].tobytes(), k
    after = snap()
    assert g.write_back(w.b, [], []) is not None and len(g.refresh_depth([])) == 0
    only_kf = g.write_back(w.b, [], [], slots=slots, mkf_pose_ids=w.ids["mkf"][slots], cam_pose_ids=w.ids["cam"])
    assert only_kf["depth"].tobytes() == x.resA["depth"].tobytes()
    only_pts = g.write_back(w.b, **_point_args(w))
    assert only_pts["world_pos"].tobytes() == x.resA["world_pos"].tobytes()
    assert snap() == after
    g.close(); t.close()


def test_solver_on_another_device_is_refused(request, gpu_required):
    if gpu_required < 2:
        pytest.skip("a graph whose table is on another device than the solver needs a second GPU")
    from mcptam_amd.pvs import MapPointTable
    x = request.getfixturevalue("twin")
    t1 = MapPointTable(device=1)
    t1.set(x.a["world_pos"], x.w.init["pr"], x.w.init["pd"], x.w.init["us"]); t1.set_rays(*x.w.rays)
    g1 = mg.MapGraph(t1, x.a["cam_from_base"])
    g1.load_arrays(x.a)
    _raises(lambda: _graph_wb(x.w, g1, x.slots), "on device")
    g1.close(); t1.close()


def test_handle_destroyed_right_after_the_call(twin):
    from mcptam_amd import chain_bundle
    x = twin
    w = x.w
    b = chain_bundle.ChainBundle(w.p.cams, True, True, False)
    w.p.populate(b)
    assert b.Compute(5) == w.rc
    t, g = _side(w, x.a)
    _graph_wb(w, g, x.slots, bundle=b, outputs=False)
    b.close()
    b2 = chain_bundle.ChainBundle(w.p.cams, True, True, False)
    w.p.populate(b2)
    assert b2.Compute(2) > 0
    got = g.get_mkfs(0, x.P)
    assert _bytes(t.get()) == _bytes(x.tA.get()) and _bytes(got[k] for k in sorted(got)) == _bytes(x.mkfs_after[k] for k in sorted(got))
    b2.close(); g.close(); t.close()


def test_neighbours_keep_their_bytes(twin):
    """mcp_ba_write_back and mcp_map_bundle_select on a third twin, before and after the new calls have run."""
    x = twin
    w = x.w

    def old_calls():
        t, g = _side(w, x.a)
        res, _ = _old_wb(w, t, x.read, x.slots)
        sel = g.select_raw(x.S)
        sel_all = g.select_raw(mc.all_())
        out = (_bytes(t.get()), _bytes(res[k] for k in sorted(res)), bytes(sel[0]), _bytes(sel[1:]), bytes(sel_all[0]), _bytes(sel_all[1:]), _mkf_bytes(g), _meas_bytes(g))
        g.close(); t.close()
        return out
    first = old_calls()
    t, g = _side(w, x.a)
    g.debug_kf_lists(x.slots, 3); g.refresh_depth(x.slots[:2]); _graph_wb(w, g, x.slots)
    g.close(); t.close()
    assert old_calls() == first
    assert first[1] == _bytes(x.resB[k] for k in sorted(x.resB))
