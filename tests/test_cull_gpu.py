"""Outliers and bad points on the GPU (include/mcp_img.h mcp_map_cull_*): on every seeded map of tests/cull_cases.py a graph on a table runs
mcp_map_cull_outliers and mcp_map_cull_sweep, and a twin graph on the same table is fed the outcome the numpy restatement
(mcptam_amd.map_graph.cull_outliers_ref / cull_sweep_ref) computes through the calls that existed before (mcp_map_graph_update_points,
mcp_map_graph_erase_meas).  Everything is exact: the two stores byte for byte, the good counts, check(), the verdicts, the counters, the
reported rows, the table's usable column, the views of a following select; and a second run on fresh graphs gives the same bytes."""
import ctypes

import numpy as np
import pytest

import cull_cases as cc
from mcptam_amd import map_graph as mg

pytestmark = pytest.mark.gpu

CASES = cc.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
IDENT = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


# ---- helpers -----------------------------------------------------------------------------------------------------------------------------------
def _table(a):
    from mcptam_amd.pvs import MapPointTable
    R = a["n_rows"]
    t = MapPointTable()
    z = np.zeros((R, 3))
    t.set(z, z, z, a["usable"])
    t.set_counts(a["inlier"], a["outlier"])
    return t


def _graph(t, a):
    """A graph on table t holding the arrays `a`: the rows that were ever written, the store with its dead entries, the MKF flags last (an
    entry may be of a slot that has left the map since)."""
    C, Pn, Np = a["ncam"], len(a["mkf_flags"]), len(a["pt_flags"])
    g = mg.MapGraph(t, np.tile(IDENT, (C, 1)))
    holds = np.zeros(Pn, dtype=bool); holds[a["ms_mkf"]] = True
    early = np.where(holds, a["mkf_flags"] | mg.MKF_PRESENT, a["mkf_flags"])
    pose, act, dep = np.tile(IDENT, (Pn, 1)), np.ones((Pn, C)), np.ones((Pn, C))
    g.set_mkfs(pose, early, act, dep)
    written = np.flatnonzero((a["src_mkf"] >= 0) | ((a["pt_flags"] & mg.GP_FIXED) != 0))
    if len(written):
        g.update_points(written, a["src_mkf"][written], a["src_cam"][written], a["pt_flags"][written])
    if len(a["ms_mkf"]):
        g.add_meas(a["ms_mkf"], a["ms_cam"], a["ms_row"], a["ms_uv"], a["ms_level"], a["ms_source"])
        dead = np.flatnonzero(a["ms_alive"] == 0)
        if len(dead):
            assert g.erase_meas(a["ms_mkf"][dead], a["ms_cam"][dead], a["ms_row"][dead]) == len(dead)
    late = np.flatnonzero(early != a["mkf_flags"])
    if len(late):
        g.update_mkfs(late, pose[late], a["mkf_flags"][late], act[late], dep[late])
    return g


def _feed_twin(tw, before, after):
    """What a cull call changed, through the calls that existed before it: the flags of the rows that went bad, the entries that died."""
    rows = np.flatnonzero(before["pt_flags"] != after["pt_flags"])
    if len(rows):
        tw.update_points(rows, before["src_mkf"][rows], before["src_cam"][rows], after["pt_flags"][rows])
    died = np.flatnonzero((before["ms_alive"] != 0) & (after["ms_alive"] == 0))
    if len(died):
        assert tw.erase_meas(before["ms_mkf"][died], before["ms_cam"][died], before["ms_row"][died]) == len(died)


def _same_store(g, tw, want_alive):
    x, y = g.get_meas(), tw.get_meas()
    for k in x:
        assert x[k].tobytes() == y[k].tobytes(), k
    assert x["alive"].tobytes() == want_alive.tobytes()
    assert g.num_meas() == tw.num_meas() == (int(want_alive.sum()), len(want_alive))
    assert g.check() == tw.check() == (0, int((want_alive == 0).sum()))
    assert g.good_counts().tobytes() == tw.good_counts().tobytes()
    return b"".join(x[k].tobytes() for k in sorted(x)) + g.good_counts().tobytes()


def _same_select(g, tw):
    S = mg.select_params(mode=mg.BUNDLE_ALL, min_points=0)
    x, y = g.select_raw(S), tw.select_raw(S)
    assert bytes(x[0]) == bytes(y[0])
    for u, v in zip(x[1:], y[1:]):
        assert u.tobytes() == v.tobytes()
    return bytes(x[0]) + b"".join(u.tobytes() for u in x[1:])


def _turn(c):
    """One turn of a case on fresh graphs, checked against the twin at every step; returns every byte the device gave."""
    a, want = c["a"], cc.ref(c)
    t = _table(a)
    g, tw = _graph(t, a), _graph(t, a)
    out = [_same_store(g, tw, a["ms_alive"])]
    r1, vd = g.cull_outliers(c["mkf"], c["cam"], c["row"], c["bad_good_count"])
    print(c["name"], r1)
    assert r1 == want["r1"] and vd.tobytes() == want["vd"].tobytes()
    assert t.get()[3].tobytes() == a["usable"].tobytes()                          # the outliers leave the table alone
    _feed_twin(tw, a, want["a1"])
    out += [vd.tobytes(), _same_store(g, tw, want["a1"]["ms_alive"])]
    r2, rows = g.cull_sweep(**c["sweep"])
    print(c["name"], r2)
    assert r2 == want["r2"] and rows.dtype == np.int32 and rows.tobytes() == want["rows"].tobytes()
    assert t.get()[3].tobytes() == want["a2"]["usable"].tobytes()
    _feed_twin(tw, want["a1"], want["a2"])
    out += [rows.tobytes(), _same_store(g, tw, want["a2"]["ms_alive"]), _same_select(g, tw)]
    r3, rows3 = g.cull_sweep(**c["sweep"])                                        # nothing is reported twice
    assert r3 == want["r3"] and len(rows3) == 0
    out.append(_same_store(g, tw, want["a3"]["ms_alive"]))
    o_ms, s_ms = g.cull_last_timing()
    assert (o_ms >= 0.0) == (c["n"] > 0) and (o_ms >= 0.0 or o_ms == -1.0) and s_ms >= 0.0
    g.close(); tw.close(); t.close()
    return b"".join(out)


# ---- 1. every case, twice ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_cull_equals_the_numpy_outcome_fed_to_a_twin(gpu_required, c):
    first = _turn(c)
    assert _turn(c) == first                                                      # fresh graphs, the same bytes


# ---- 2. a whole turn of the map maker's loop -------------------------------------------------------------------------------------------------------
def test_a_whole_turn(gpu_required):
    """select -> cull_outliers (the outliers picked among the measurements the select listed) -> cull_sweep -> compact -> select."""
    a = cc.random_map(4242, 14, 3, 600, 600, per_row=(1, 9))
    t = _table(a)
    g, tw = _graph(t, a), _graph(t, a)
    S = mg.select_params(mode=mg.BUNDLE_ALL, min_points=0)
    res, mkfs, points, meas = g.select_raw(S)
    assert res.status == 0 and res.n_meas > 1000
    pick = np.random.default_rng(7).permutation(res.n_meas)[:300]                  # "outliers" in an order that is not the store's
    mkf, cam, row = mkfs["slot"][meas["mkf"][pick]], meas["cam"][pick], points["row"][meas["point"][pick]]
    r1w, vdw, a1 = mg.cull_outliers_ref(a, mkf, cam, row, n_rows=600)
    r2w, rowsw, a2 = mg.cull_sweep_ref(a1, n_rows=600)
    r1, vd = g.cull_outliers(mkf, cam, row)
    r2, rows = g.cull_sweep()
    print(r1, r2)
    assert r1 == r1w and vd.tobytes() == vdw.tobytes() and r2 == r2w and rows.tobytes() == rowsw.tobytes()
    assert r1["n_missing"] == 0 and min(r1["n_point_bad"], r1["n_retry"], r1["n_never_retry"], r1["n_already_bad"]) > 0 and r2["n_reported"] > r1["n_rows_marked"] > 0
    _feed_twin(tw, a, a1)
    _feed_twin(tw, a1, a2)
    _same_store(g, tw, a2["ms_alive"])
    g.compact(); tw.compact()
    live = np.flatnonzero(a2["ms_alive"])
    st = g.get_meas()
    assert st["row"].tobytes() == a2["ms_row"][live].tobytes() and st["alive"].all() and g.num_meas() == tw.num_meas() == (len(live), len(live))
    assert g.check() == tw.check() == (0, 0)
    _same_select(g, tw)
    res2, mkfs2, points2, meas2 = g.select_raw(S)
    bad = (a2["pt_flags"] & mg.GP_BAD) != 0
    assert not bad[points2["row"]].any() and res2.n_points < res.n_points and res2.n_meas < res.n_meas
    assert t.get()[3].tobytes() == a2["usable"].tobytes()
    g.close(); tw.close(); t.close()


# ---- 3. the report ---------------------------------------------------------------------------------------------------------------------------------
def test_what_the_report_holds(gpu_required):
    c = BY_NAME["good4_three_refind"]
    a = c["a"]
    t = _table(a)
    g = _graph(t, a)
    assert g.cull_rows().tolist() == [] and g.cull_last_timing() == (-1.0, -1.0)
    r1, vd = g.cull_outliers(c["mkf"], c["cam"], c["row"])
    assert vd.tolist() == [mg.CULL_NEVER_RETRY, mg.CULL_NEVER_RETRY, mg.CULL_POINT_BAD] and r1["n_rows_marked"] == 1
    assert g.cull_rows().tolist() == [] and g.num_meas() == (3, 5)                  # the report is the sweep's
    # the host rewrites the row before the sweep (a new point in a recycled row, or its own verdict): the pending mark goes, nothing is reported
    g.update_points([0], [0], [0], [mg.GP_BAD])
    r2, rows = g.cull_sweep()
    assert rows.tolist() == [] and r2 == dict(n_danglers=0, n_tracker_outliers=0, n_reported=0, n_bad_rows=1, n_meas_erased=3) and g.num_meas() == (0, 5)
    g.close()
    # the same without the rewrite: reported once
    g = _graph(t, a)
    g.cull_outliers(c["mkf"], c["cam"], c["row"])
    r2, rows = g.cull_sweep()
    assert rows.tolist() == [0] and r2["n_reported"] == 1 and g.cull_rows().tolist() == [0]
    assert g.cull_sweep()[1].tolist() == [] and g.cull_rows().tolist() == []
    # a reported row rewritten for a new point that dangles: reported again, by the sweep that marks it
    g.update_points([0], [0], [0], [0])
    r2, rows = g.cull_sweep()
    assert rows.tolist() == [0] and r2["n_danglers"] == 1
    # an empty list enqueues nothing and its timing reads as not run
    r1, vd = g.cull_outliers([], [], [])
    assert r1 == dict.fromkeys(r1, 0) and len(vd) == 0 and g.cull_last_timing()[0] == -1.0 and g.cull_last_timing()[1] >= 0.0
    g.close(); t.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(gpu_required):
    from mcptam_amd import chain_bundle
    c = BY_NAME["list65"]
    a = c["a"]
    t = _table(a)
    g = _graph(t, a)
    g.cull_outliers(c["mkf"][:9], c["cam"][:9], c["row"][:9])
    g.cull_sweep()
    store0, num0, good0, usable0, rows0, time0 = g.get_meas(), g.num_meas(), g.good_counts().tobytes(), t.get()[3].tobytes(), g.cull_rows().tobytes(), g.cull_last_timing()
    S = mg.select_params(mode=mg.BUNDLE_ALL, min_points=0)
    sel0 = g.select_raw(S)
    k = (c["mkf"][9:], c["cam"][9:], c["row"][9:])

    def refused(needle, call):
        with pytest.raises(RuntimeError):
            call()
        err = chain_bundle.last_error()
        assert needle in err and err.startswith("mcp_map_cull_"), err
        assert g.num_meas() == num0 and all(store0[q].tobytes() == v.tobytes() for q, v in g.get_meas().items())
        assert g.good_counts().tobytes() == good0 and t.get()[3].tobytes() == usable0 and g.cull_rows().tobytes() == rows0 and g.cull_last_timing() == time0
        sel = g.select_raw(S)
        assert bytes(sel[0]) == bytes(sel0[0]) and all(u.tobytes() == v.tobytes() for u, v in zip(sel[1:], sel0[1:]))
    refused("names slot", lambda: g.cull_outliers(np.r_[k[0][:-1], mg.MAX_MKFS], k[1], k[2]))
    refused("names slot", lambda: g.cull_outliers(np.r_[-1, k[0][1:]], k[1], k[2]))
    refused("names camera", lambda: g.cull_outliers(k[0], np.r_[k[1][:-1], a["ncam"]], k[2]))
    refused("names camera", lambda: g.cull_outliers(k[0], np.r_[-1, k[1][1:]], k[2]))
    refused("appears twice", lambda: g.cull_outliers(np.r_[k[0], k[0][3]], np.r_[k[1], k[1][3]], np.r_[k[2], k[2][3]]))
    refused("negative bad_good_count", lambda: g.cull_outliers(*k, bad_good_count=-1))
    refused("negative min_outliers", lambda: g.cull_sweep(min_outliers=-1))
    refused("not finite", lambda: g.cull_sweep(outlier_multiplier=np.inf))
    refused("not finite", lambda: g.cull_sweep(outlier_multiplier=np.nan))
    L = g._L
    po, ro, ps, rs = mg.CullOutliersParams(2), mg.CullOutliersResult(), mg.CullSweepParams(20, 1, 1.0), mg.CullSweepResult()
    one = np.zeros(1, dtype=np.int32)
    adr = ctypes.addressof
    refused("NULL params or result", lambda: mg._chk(L.mcp_map_cull_outliers(g._h, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, None, None, adr(ro)), "x"))
    refused("NULL params or result", lambda: mg._chk(L.mcp_map_cull_outliers(g._h, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, adr(po), None, None), "x"))
    refused("bad arguments", lambda: mg._chk(L.mcp_map_cull_outliers(g._h, 1, None, one.ctypes.data, one.ctypes.data, adr(po), None, adr(ro)), "x"))
    refused("bad arguments", lambda: mg._chk(L.mcp_map_cull_outliers(g._h, -1, one.ctypes.data, one.ctypes.data, one.ctypes.data, adr(po), None, adr(ro)), "x"))
    refused("NULL params or result", lambda: mg._chk(L.mcp_map_cull_sweep(g._h, None, adr(rs)), "x"))
    refused("NULL params or result", lambda: mg._chk(L.mcp_map_cull_sweep(g._h, adr(ps), None), "x"))
    # and after all that the rest of the list is judged as if nothing had happened
    _, _, a1 = mg.cull_outliers_ref(a, c["mkf"][:9], c["cam"][:9], c["row"][:9], n_rows=a["n_rows"])
    _, _, a2 = mg.cull_sweep_ref(a1, n_rows=a["n_rows"])
    want, vdw, _ = mg.cull_outliers_ref(a2, *k, n_rows=a["n_rows"])
    r1, vd = g.cull_outliers(*k)
    assert r1 == want and vd.tobytes() == vdw.tobytes()
    g.close(); t.close()
