"""Measurement parcels on the GPU (include/mcp_img.h mcp_meas_parcel_*): a parcel filled from the host, from a track call and from a ReFind,
committed to a graph's store, against a twin graph that is handed the surviving entries -- chosen in numpy by parcel_commit_ref -- through
mcp_map_graph_add_meas.  Everything is exact: the two stores byte for byte, the counters, the per-lane counts, the views of a following select.
Not covered: a store that would pass INT_MAX entries (80 GB of store)."""
import ctypes

import numpy as np
import pytest

import parcel_cases as pc
from mcptam_amd import map_graph as mg

pytestmark = pytest.mark.gpu

CASES = pc.all_cases()
QUALITY = dict(min_patches=10, quality_coarse_min=20, quality_good=0.3, quality_bad=0.13)
SEARCH = dict(try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=10, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=12345)


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------------
def _graph(t, ncam, n_slots, rows, src_mkf, src_cam, flags, pre_slot=None):
    """A graph on table t: n_slots present MKFs at the identity, the graph columns of `rows`, and -- pre_slot -- N_PRE entries of that slot."""
    ident = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    g = mg.MapGraph(t, np.tile(ident, (ncam, 1)))
    g.set_mkfs(np.tile(ident, (n_slots, 1)), np.full(n_slots, mg.MKF_PRESENT), np.ones((n_slots, ncam)), np.ones((n_slots, ncam)))
    if len(rows):
        g.update_points(rows, src_mkf, src_cam, flags)
    if pre_slot is not None:
        k = pc.N_PRE
        g.add_meas(np.full(k, pre_slot), np.zeros(k), np.arange(k), np.arange(2.0 * k).reshape(k, 2), np.zeros(k), np.full(k, mg.SRC_ROOT))
    return g


def _same_store(g, tw, n_dead=0):
    a, b = g.get_meas(), tw.get_meas()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert g.num_meas() == tw.num_meas()
    assert g.check() == (0, n_dead) and tw.check() == (0, n_dead)
    return a


def _same_select(g, tw):
    S = mg.select_params(mode=mg.BUNDLE_ALL, min_points=0)
    x, y = g.select_raw(S), tw.select_raw(S)
    assert bytes(x[0]) == bytes(y[0])
    for u, v in zip(x[1:], y[1:]):
        assert u.tobytes() == v.tobytes()
    return x


def _feed_twin(tw, recs):
    if len(recs):
        tw.add_meas(recs["mkf"], recs["cam"], recs["row"], recs["uv"], recs["level"], recs["source"])


def _seeded_device(c):
    """Table, graph and twin of a seeded case as they stand when the parcel is filled."""
    from mcptam_amd.pvs import MapPointTable
    nF, npr = c["n_rows_fill"], c["n_point_rows"]
    t = MapPointTable()
    z = np.zeros((nF, 3))
    t.set(z, z, z, np.ones(nF, dtype=np.uint8))
    t.set_source(c["keys_fill"], [None] * nF, np.zeros(nF), np.zeros((nF, 2)))
    early = c["pt_flags"].copy(); early[c["bad_late"]] &= ~mg.GP_BAD
    pair = [_graph(t, c["ncam"], c["P"], np.arange(npr), c["src_mkf"], c["src_cam"], early, pre_slot=c["P"] - 1) for _ in range(2)]
    return t, pair[0], pair[1]


def _seeded_mutate(c, t, graphs):
    """What happens between the fill and the commit: rows recycled for other points, rows gone bad, the table's tail dropped -- all enqueued
    on the table's stream with no wait."""
    n = c["n_rows"]
    changed = np.flatnonzero(c["keys_now"] != c["keys_fill"][:n])
    if len(changed):
        t.update_source(changed, c["keys_now"][changed], [None] * len(changed), np.zeros(len(changed)), np.zeros((len(changed), 2)))
    late = c["bad_late"]
    for g in graphs:
        if len(late):
            g.update_points(late, c["src_mkf"][late], c["src_cam"][late], c["pt_flags"][late])
    t.resize(n)


# ---- 1. seams --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_commit_equals_add_meas_of_the_survivors(gpu_required, c):
    t, g, tw = _seeded_device(c)
    e = c["entries"]
    p = mg.MeasParcel.from_host(t, e["lane"], e["row"], e["uv"], e["level"])
    assert len(p) == c["n"] and p.entries().tobytes() == e.tobytes()              # the keys were gathered on the device
    _seeded_mutate(c, t, (g, tw))
    vd, want, recs, want_lanes = pc.ref(c, first=pc.N_PRE)
    res, lanes = g.commit_parcel(p, c["lane_mkf"], c["lane_cam"], c["cross_camera"], c["source"])
    print(c["name"], res)
    assert res == want and np.array_equal(lanes, want_lanes)
    assert sum(res[k] for k in ("n_appended", "n_skipped_lane", "n_stale", "n_bad", "n_cross")) == c["n"]
    _feed_twin(tw, recs)
    st = _same_store(g, tw)
    assert g.num_meas() == (pc.N_PRE + res["n_appended"],) * 2
    assert st["uv"][pc.N_PRE:].tobytes() == recs["uv"].tobytes() and np.array_equal(st["row"][pc.N_PRE:], recs["row"])
    sel = _same_select(g, tw)
    assert sel[0].status == 0
    assert p.entries().tobytes() == e.tobytes()                                    # a commit leaves the parcel's entries alone
    p.close(); g.close(); tw.close(); t.close()


def _small(t_rows=12):
    """A table of t_rows rows with keys 100 + row, a graph (3 cameras, slots 0..3) and its twin with every row good, source (slot 0, camera row % 3)."""
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    z = np.zeros((t_rows, 3))
    t.set(z, z, z, np.ones(t_rows, dtype=np.uint8))
    t.set_source(100 + np.arange(t_rows), [None] * t_rows, np.zeros(t_rows), np.zeros((t_rows, 2)))
    r = np.arange(t_rows)
    g, tw = (_graph(t, 3, 4, r, np.zeros(t_rows), r % 3, np.zeros(t_rows), pre_slot=3) for _ in range(2))
    return t, g, tw


def _rekey(t, rows, keys):
    rows = np.asarray(rows)
    t.update_source(rows, keys, [None] * len(rows), np.zeros(len(rows)), np.zeros((len(rows), 2)))


def test_edge_cases(gpu_required):
    t, g, tw = _small()
    uv = np.arange(12.0).reshape(6, 2) + 0.25
    # an empty parcel
    p = mg.MeasParcel.from_host(t, [], [], np.zeros((0, 2)), [])
    res, lanes = g.commit_parcel(p, [0, 1], [0, 1])
    assert res == dict(first=pc.N_PRE, n_appended=0, n_skipped_lane=0, n_stale=0, n_bad=0, n_cross=0) and lanes.tolist() == [0, 0] and len(p.entries()) == 0
    # everything dropped: both lanes withheld
    assert p.fill_from_host([0, 1, 0, 1, 0, 1], [0, 1, 2, 3, 4, 5], uv, [0, 1, 2, 3, 0, 1]) == 6
    res, lanes = g.commit_parcel(p, [-1, -1], [0, 1])
    assert res == dict(first=pc.N_PRE, n_appended=0, n_skipped_lane=6, n_stale=0, n_bad=0, n_cross=0) and lanes.tolist() == [0, 0]
    _same_store(g, tw)
    # one lane skipped; row 2 recycled and row 4 gone bad between the fill and the commit; CrossCamera off: lane 0 is camera 0, rows 0 and 3 are its own
    p.fill_from_host([0, 1, 0, 0, 0, 0], [0, 1, 2, 3, 4, 5], uv, [0, 1, 2, 3, 0, 1])
    _rekey(t, [2], [999])
    for G in (g, tw):
        G.update_points([4], [0], [1], [mg.GP_BAD])
    res, lanes = g.commit_parcel(p, [1, -1], [0, 2], cross_camera=0, source=mg.SRC_REFIND)
    assert res == dict(first=pc.N_PRE, n_appended=2, n_skipped_lane=1, n_stale=1, n_bad=1, n_cross=1) and lanes.tolist() == [2, 0]
    tw.add_meas([1, 1], [0, 0], [0, 3], uv[[0, 3]], [0, 3], [mg.SRC_REFIND] * 2)
    _same_store(g, tw)
    ent = p.entries()
    assert ent["key"].tolist() == [100, 101, 102, 103, 104, 105]                 # the keys of the fill, not of the commit
    p.close(); g.close(); tw.close(); t.close()


# ---- 2. from a frame -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame_world(gpu_required):
    """The scene of tests/test_track_record_gpu.py: four cameras, one looking away (an empty PVS), about 4 % unusable and 2 % fixed rows, the
    counts the map maker would have left, and a second prior further along."""
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
            (so3_exp(np.array([0.0, np.pi, 0.0])), np.zeros(3)), (so3_exp(np.array([0.08, 0.0, 0.0])), np.array([0.0, 0.03, 0.01]))]
    targets = [KeyFrame(640, 480) for _ in range(4)]
    make_lite_batch(targets, [sc["imgB"]] * 4)
    cols = dict(wp=wp, pr=pr, pd=pd, usable=(rng.random(n) >= 0.04).astype(np.uint8), keys=np.arange(n, dtype=np.int32) * 3 + 7, src=[src] * n,
                level=np.array([p["source_level"] for p in pts], dtype=np.int32), center=np.array([p["center"] for p in pts], dtype=np.int32),
                fixed=(rng.random(n) < 0.02).astype(np.uint8))
    crng = np.random.default_rng(77)
    cols["inl"], cols["outl"] = crng.integers(1, 31, n).astype(np.int32), crng.integers(0, 31, n).astype(np.int32)
    R, t = sc["poseB"]
    prior = (so3_exp(np.array([0.012, -0.006, 0.009])) @ R, t + np.array([0.01, -0.006, 0.004]))
    prior2 = (so3_exp(np.array([-0.004, 0.003, -0.002])) @ R, t + np.array([-0.003, 0.002, 0.001]))
    grng = np.random.default_rng(11)
    fx = cols["fixed"] != 0
    graph_cols = dict(src_mkf=np.where(fx, -1, 0).astype(np.int32), src_cam=np.where(fx, 0, grng.integers(0, 4, n)).astype(np.int32),
                      flags=(np.where(fx, mg.GP_FIXED, 0) | np.where(grng.random(n) < 0.06, mg.GP_BAD, 0)).astype(np.int32))
    return dict(sc=sc, cam=sc["cam"], src=src, cols=cols, cfbs=cfbs, targets=targets, prior=prior, prior2=prior2, n=n, graph_cols=graph_cols)


def _frame_table(cols):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], cols["src"], cols["level"], cols["center"], cols["fixed"])
    t.set_counts(cols["inl"], cols["outl"])
    return t


def _entries_of_track(meas, keys):
    lane = np.concatenate([np.full(len(m), c) for c, m in enumerate(meas)]).astype(np.int32)
    allm = np.concatenate(meas)
    return mg.parcel_entries(lane, allm["row"], allm["found_pos"], allm["level"], keys[allm["row"]])


@pytest.mark.parametrize("want_items", [1, 0])
def test_parcel_of_a_frame_outlives_the_next_frame(frame_world, want_items):
    w = frame_world
    cols, gc, n = w["cols"], w["graph_cols"], w["n"]
    t = _frame_table(cols)
    g, tw = (_graph(t, 4, 3, np.arange(n), gc["src_mkf"], gc["src_cam"], gc["flags"]) for _ in range(2))
    cams = [w["cam"]] * 4
    first = t.track_map_record(w["targets"], cams, w["prior"], w["cfbs"], want_items=want_items, **QUALITY, **SEARCH)
    meas1, rec1 = first[4], first[5]
    p = mg.MeasParcel.from_track(t)                                               # enqueued, no wait
    second = t.track_map_record(w["targets"], cams, w["prior2"], w["cfbs"], want_items=want_items, **QUALITY, **dict(SEARCH, seed=999))      # rewrites the views
    meas2 = second[4]
    print("measurements per camera", [len(m) for m in meas1], "then", [len(m) for m in meas2])
    assert len(meas1[2]) == 0 and sum(len(m) for m in meas1) > 500
    assert b"".join(m.tobytes() for m in meas1) != b"".join(m.tobytes() for m in meas2)
    want_e = _entries_of_track(meas1, cols["keys"])
    assert len(p) == len(want_e) == sum(rec1.n_meas[c] for c in range(4))
    assert p.entries().tobytes() == want_e.tobytes()
    pair = want_e["lane"].astype(np.int64) * n + want_e["row"]
    assert len(np.unique(pair)) == len(pair)                                      # C, T, R of a camera are disjoint: (lane, row) is unique
    # a device fill's largest lane is read back by the commit: two lanes are too few, nothing is appended
    with pytest.raises(RuntimeError, match="lane 3"):
        g.commit_parcel(p, [1, 1], [0, 1])
    assert g.num_meas() == (0, 0)
    lane_mkf, lane_cam, cross = [1, 1, 1, -1 if want_items else 1], [0, 1, 2, 3], want_items
    vd, want, recs, want_lanes = mg.parcel_commit_ref(want_e, cols["keys"], gc["flags"], gc["src_mkf"], gc["src_cam"], lane_mkf, lane_cam, cross, mg.SRC_TRACKER, 0)
    res, lanes = g.commit_parcel(p, lane_mkf, lane_cam, cross, mg.SRC_TRACKER)
    print("commit", res, lanes.tolist())
    assert res == want and np.array_equal(lanes, want_lanes) and res["n_appended"] > 50 and res["n_bad"] > 0
    assert (res["n_cross"] > 0) == (not cross) and (res["n_skipped_lane"] > 0) == bool(want_items)
    _feed_twin(tw, recs)
    _same_store(g, tw)
    _same_select(g, tw)
    p.close(); g.close(); tw.close(); t.close()


# ---- 3. from a ReFind ----------------------------------------------------------------------------------------------------------------------------
def test_parcel_of_a_refind(gpu_required):
    from mcptam_amd.keyframe import KeyFrame
    from mcptam_amd.pvs import MapPointTable
    from refind_fixture import N_BASE, make_world, newly_made_targets
    w = make_world(KeyFrame)
    cols = w["cols"]
    nr = len(cols["wp"])
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], [w["A"]] * nr, cols["level"], cols["center"], cols["fixed"])
    rng = np.random.default_rng(3)
    sm, sc = rng.integers(0, 3, N_BASE).astype(np.int32), rng.integers(0, 2, N_BASE).astype(np.int32)
    fl = np.where(rng.random(N_BASE) < 0.07, mg.GP_BAD, 0).astype(np.int32)
    g, tw = (_graph(t, 2, 4, np.arange(N_BASE), sm, sc, fl) for _ in range(2))
    targets = newly_made_targets(w["sc"], w["B"])
    pairs = np.stack([np.repeat(np.arange(N_BASE), 4), np.tile(np.arange(4), N_BASE)], axis=1).astype(np.int32)
    _, meas, counts, _ = t.refind(targets, pairs, True, None, view=True)
    meas = meas.copy()
    p = mg.MeasParcel.from_refind(t)
    t.refind(targets, pairs[:40], False, None, view=True)                          # the next batch rewrites the pinned block
    want_e = mg.parcel_entries(meas["target"], meas["row"], meas["root_pos"], meas["level"], cols["keys"][meas["row"]])
    print("found", len(meas), "per target", np.bincount(meas["target"], minlength=4).tolist())
    assert len(p) == len(meas) > 500 and (np.diff(meas["pair"]) > 0).all()
    assert p.entries().tobytes() == want_e.tobytes()
    gone = np.arange(10, 41)
    _rekey(t, gone, gone + 1)                                                      # thirty-one points replaced before the commit, no wait
    keys_now = cols["keys"].copy(); keys_now[gone] = gone + 1
    lane_mkf, lane_cam = [0, -1, 3, 1], [0, 0, 1, 1]
    vd, want, recs, want_lanes = mg.parcel_commit_ref(want_e, keys_now, fl, sm, sc, lane_mkf, lane_cam, 1, mg.SRC_REFIND, 0)
    res, lanes = g.commit_parcel(p, lane_mkf, lane_cam, 1, mg.SRC_REFIND)
    print("commit", res, lanes.tolist())
    assert res == want and np.array_equal(lanes, want_lanes)
    assert res["n_appended"] > 200 and res["n_stale"] > 0 and res["n_bad"] > 0 and res["n_skipped_lane"] > 0 and res["n_cross"] == 0
    _feed_twin(tw, recs)
    _same_store(g, tw)
    _same_select(g, tw)
    # a ReFind that ran over its cap leaves nothing to take; the parcel keeps what it holds
    with pytest.raises(RuntimeError):
        t.refind(targets, pairs[:400], False, None, cap_meas=1)
    with pytest.raises(RuntimeError, match="no measurements to take"):
        p.fill_from_refind()
    assert p.entries().tobytes() == want_e.tobytes()
    p.close(); g.close(); tw.close(); t.close()


# ---- 4. life cycle and order -----------------------------------------------------------------------------------------------------------------------
def test_life_cycle_and_order(gpu_required):
    t, g, tw = _small(40)
    rows = np.arange(30)
    uv = np.stack([rows + 0.5, 100.0 - rows], axis=1)
    p = mg.MeasParcel.from_host(t, rows % 3, rows, uv, rows % 4)
    res, lanes = g.commit_parcel(p, [0, 0, 1], [0, 1, 2])
    assert res["n_appended"] == 30 and res["first"] == pc.N_PRE and lanes.tolist() == [10, 10, 10]
    tw.add_meas(np.where(rows % 3 == 2, 1, 0), rows % 3, rows, uv, rows % 4, np.zeros(30))
    # a second commit without a refill would duplicate every entry
    before = g.get_meas()
    with pytest.raises(RuntimeError, match="committed already"):
        g.commit_parcel(p, [0, 0, 1], [0, 1, 2])
    assert g.num_meas() == (pc.N_PRE + 30,) * 2 and all(before[k].tobytes() == v.tobytes() for k, v in g.get_meas().items())
    # a select right behind a commit sees the entries: rows 0..4 now have two measurements each (the store's own and the parcel's)
    sel = _same_select(g, tw)
    assert sel[0].n_points == pc.N_PRE and sel[0].n_meas == 2 * pc.N_PRE and sorted(sel[3]["store"].tolist()) == list(range(2 * pc.N_PRE))
    # erase, compact, refill, commit: store order is kept, new entries come last
    for G in (g, tw):
        assert G.erase_meas([0, 0, 1], [0, 1, 2], [3, 7, 11]) == 3
    _same_store(g, tw, n_dead=3)
    for G in (g, tw):
        G.compact()
    rows2 = np.arange(30, 40)
    uv2 = np.stack([rows2 * 2.0, rows2 * 3.0], axis=1)
    assert p.fill_from_host(np.zeros(10), rows2, uv2, np.ones(10)) == 10
    # rows 31 and 35 get other points right before the commit: enqueued on the same stream, no wait in between, and the commit sees the new keys
    _rekey(t, [31, 35], [5, 6])
    res, lanes = g.commit_parcel(p, [2], [1], source=mg.SRC_REFIND)
    assert res == dict(first=pc.N_PRE + 27, n_appended=8, n_skipped_lane=0, n_stale=2, n_bad=0, n_cross=0) and lanes.tolist() == [8]
    keep = ~np.isin(rows2, [31, 35])
    tw.add_meas(np.full(8, 2), np.ones(8), rows2[keep], uv2[keep], np.ones(8), np.full(8, mg.SRC_REFIND))
    st = _same_store(g, tw)
    assert st["row"].tolist() == list(range(pc.N_PRE)) + [r for r in range(30) if r not in (3, 7, 11)] + [r for r in range(30, 40) if r not in (31, 35)]
    _same_select(g, tw)
    # a parcel that grows past its block keeps working (the block is replaced behind a wait)
    big = np.arange(3000)
    assert p.fill_from_host(big % 2, big % 40, np.zeros((3000, 2)), np.zeros(3000)) == 3000 and len(p.entries()) == 3000
    p.close(); g.close(); tw.close(); t.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(gpu_required):
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import MapPointTable
    t, g, tw = _small()
    rows = np.arange(6)
    uv = np.arange(12.0).reshape(6, 2)
    p = mg.MeasParcel.from_host(t, rows % 2, rows, uv, rows % 4)
    ent0, store0, num0 = p.entries().tobytes(), g.get_meas(), g.num_meas()

    def unchanged():
        assert p.entries().tobytes() == ent0 and len(p) == 6
        assert g.num_meas() == num0 and all(store0[k].tobytes() == v.tobytes() for k, v in g.get_meas().items())

    def refused(needle, call):
        with pytest.raises(RuntimeError):
            call()
        assert needle in chain_bundle.last_error(), chain_bundle.last_error()
        unchanged()
    # the fills
    refused("names lane -1", lambda: p.fill_from_host([-1], [0], [[0.0, 0.0]], [0]))
    refused("names row 12", lambda: p.fill_from_host([0], [12], [[0.0, 0.0]], [0]))
    refused("names row -1", lambda: p.fill_from_host([0], [-1], [[0.0, 0.0]], [0]))
    refused("has level 4", lambda: p.fill_from_host([0], [0], [[0.0, 0.0]], [4]))
    refused("non-finite", lambda: p.fill_from_host([0], [0], [[0.0, np.inf]], [0]))
    refused("non-finite", lambda: p.fill_from_host([0, 0], [0, 1], [[0.0, 1.0], [np.nan, 0.0]], [0, 0]))
    refused("no successful mcp_track_map_record", p.fill_from_track)
    refused("no measurements to take", p.fill_from_refind)
    # the commit
    refused("lane 1, the call has 1 lanes", lambda: g.commit_parcel(p, [0], [0]))
    refused("which is not present", lambda: g.commit_parcel(p, [0, 7], [0, 1]))
    refused("which is not present", lambda: g.commit_parcel(p, [0, mg.MAX_MKFS], [0, 1]))
    refused("names camera 3", lambda: g.commit_parcel(p, [0, 1], [0, 3]))
    refused("names camera -1", lambda: g.commit_parcel(p, [0, 1], [-1, 0]))
    L = g._L
    prm, res = mg.ParcelCommitParams(1, 0), mg.ParcelCommitResult()
    two = np.zeros(2, dtype=np.int32)
    raw = lambda *a: mg._chk(L.mcp_meas_parcel_commit(*a), "meas_parcel_commit")
    refused("NULL parcel", lambda: raw(g._h, None, 2, two.ctypes.data, two.ctypes.data, ctypes.addressof(prm), ctypes.addressof(res), None))
    refused("NULL graph", lambda: raw(None, p._h, 2, two.ctypes.data, two.ctypes.data, ctypes.addressof(prm), ctypes.addressof(res), None))
    refused("NULL params or result", lambda: raw(g._h, p._h, 2, two.ctypes.data, two.ctypes.data, None, ctypes.addressof(res), None))
    refused("NULL params or result", lambda: raw(g._h, p._h, 2, two.ctypes.data, two.ctypes.data, ctypes.addressof(prm), None, None))
    refused("bad lane tables", lambda: raw(g._h, p._h, 2, None, two.ctypes.data, ctypes.addressof(prm), ctypes.addressof(res), None))
    refused("bad lane tables", lambda: raw(g._h, p._h, -1, two.ctypes.data, two.ctypes.data, ctypes.addressof(prm), ctypes.addressof(res), None))
    refused("holds 6 entries", lambda: mg._chk(L.mcp_meas_parcel_get(p._h, 5, np.zeros(5, dtype=mg.PARCEL_ENTRY_DTYPE).ctypes.data), "meas_parcel_get"))
    # a parcel of another table; a parcel never filled
    t2 = MapPointTable()
    z = np.zeros((12, 3))
    t2.set(z, z, z, np.ones(12, dtype=np.uint8))
    q = mg.MeasParcel.from_host(t2, rows % 2, rows, uv, rows % 4)
    refused("another table", lambda: g.commit_parcel(q, [0, 1], [0, 1]))
    assert q.entries()["key"].tolist() == [0] * 6                                  # (rows that were never given a source have key 0)
    fresh = mg.MeasParcel(t)
    refused("never filled", lambda: g.commit_parcel(fresh, [0, 1], [0, 1]))
    # and after all that the parcel commits as if nothing had happened
    res, lanes = g.commit_parcel(p, [0, 1], [0, 1])
    assert res["n_appended"] == 6 and lanes.tolist() == [3, 3]
    tw.add_meas(rows % 2, rows % 2, rows, uv, rows % 4, np.zeros(6))
    _same_store(g, tw)
    for x in (fresh, q, p, g, tw):
        x.close()
    t2.close(); t.close()
