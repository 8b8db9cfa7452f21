"""The closest-keyframe queries and the removal of an MKF on the GPU (include/mcp_img.h mcp_map_neighbours, mcp_map_mkf_cull): on every case of
tests/neighbour_cases.py the device's result struct equals the host twin's byte for byte (they share their bodies and neither build contracts),
and a second run on a fresh graph gives the same bytes; a removal on a graph is compared with a twin graph that is fed the numpy
restatement's outcome (mcptam_amd.map_graph.cull_mkf_ref) through the calls that existed before -- mcp_map_graph_update_mkfs, _update_points,
_erase_meas / _erase_mkf -- store, good counts, check() and a following select byte for byte; one whole turn of an MKF's removal; refusals."""
import ctypes

import numpy as np
import pytest

import neighbour_cases as nc
from mcptam_amd import map_graph as mg

pytestmark = pytest.mark.gpu

CASES = nc.all_cases()
BY_NAME = {c["name"]: c for c in CASES}


# ---- helpers (the pattern of tests/test_cull_gpu.py, with the map's own poses) ----------------------------------------------------------------------
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
    Pn = len(a["mkf_flags"])
    g = mg.MapGraph(t, a["cam_from_base"])
    holds = np.zeros(Pn, dtype=bool); holds[a["ms_mkf"]] = True
    early = np.where(holds, a["mkf_flags"] | mg.MKF_PRESENT, a["mkf_flags"])
    g.set_mkfs(a["base_from_world"], early, a["kf_active"], a["kf_depth_mean"])
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
        g.update_mkfs(late, a["base_from_world"][late], a["mkf_flags"][late], a["kf_active"][late], a["kf_depth_mean"][late])
    return g


def _feed_twin(tw, before, after, victim, erased):
    """What a removal changed, through the calls that existed before it: MKF flags, the flags of the rows that went bad, the entries that died."""
    mk = np.flatnonzero((before["mkf_flags"] | (mg.MKF_PRESENT if erased else 0)) != (after["mkf_flags"] | (mg.MKF_PRESENT if erased else 0)))
    if len(mk):                                                                   # (the erase takes the slot out of the map itself)
        tw.update_mkfs(mk, before["base_from_world"][mk], after["mkf_flags"][mk] | (before["mkf_flags"][mk] & mg.MKF_PRESENT), before["kf_active"][mk], before["kf_depth_mean"][mk])
    rows = np.flatnonzero(before["pt_flags"] != after["pt_flags"])
    if len(rows):
        tw.update_points(rows, before["src_mkf"][rows], before["src_cam"][rows], after["pt_flags"][rows])
    died = np.flatnonzero((before["ms_alive"] != 0) & (after["ms_alive"] == 0))
    if erased:
        assert tw.erase_mkf(victim) == len(died)
    else:
        assert len(died) == 0


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


def _same_mkfs(g, a):
    n = len(a["mkf_flags"])
    got = g.get_mkfs(0, n)
    assert got["flags"].tobytes() == a["mkf_flags"].tobytes()
    return got["flags"].tobytes()


def _queries(c):
    """Every query of a case on a fresh graph: the device's result structs, each equal to the host twin's."""
    a = c["a"]
    t = _table(a)
    g = _graph(t, a)
    assert g.neighbours_last_timing() == -1.0
    out = []
    for q in c["queries"]:
        got, want = g.neighbours(raw=True, **q), mg.neighbours_host(a, q, raw=True)
        assert bytes(got) == bytes(want), ({k: v for k, v in q.items() if k != "ext"}, got.as_dict(), want.as_dict(), got.items()[:4], want.items()[:4])
        assert g.neighbours_last_timing() >= 0.0
        out.append(bytes(got))
    g.close(); t.close()
    return b"".join(out)


def _removal(c, k):
    """One removal of a case on a fresh graph against the twin; returns every byte the device gave."""
    a = c["a"]
    want, after = mg.cull_mkf_ref(a, **k)
    host, after_h = mg.cull_mkf_host(a, **k)
    t = _table(a)
    g, tw = _graph(t, a), _graph(t, a)
    assert g.cull_mkf_last_timing() == -1.0
    got = g.cull_mkf(**k)
    print(c["name"], k, got)
    assert got == host and {x: v for x, v in got.items() if x != "victim_dist"} == {x: v for x, v in want.items() if x != "victim_dist"}
    np.testing.assert_allclose(got["victim_dist"], want["victim_dist"], rtol=1e-12, atol=0.0)
    assert all(after[col].tobytes() == after_h[col].tobytes() for col in nc.CULL_STATE) and g.cull_mkf_last_timing() >= 0.0
    erased = bool(k.get("erase", True)) and got["status"] == 0
    _feed_twin(tw, a, after, got["victim"], erased)
    out = [repr(sorted(got.items())).encode(), _same_store(g, tw, after["ms_alive"]), _same_mkfs(g, after), _same_mkfs(tw, after), _same_select(g, tw)]
    assert t.get()[3].tobytes() == a["usable"].tobytes()                          # the removal leaves the table alone: the sweep clears the rows
    # the rows it marked are the next sweep's report, and only they (nothing else is pending in these maps); the twin's rows were written by the host
    r2, rows = g.cull_sweep(min_outliers=1 << 30, danglers=False)
    marked = np.flatnonzero(after["pending"] != 0)
    assert rows.tolist() == marked.tolist() and r2["n_reported"] == got["n_rows_marked"]
    tw.cull_sweep(min_outliers=1 << 30, danglers=False)
    out += [rows.tobytes(), _same_store(g, tw, g.get_meas()["alive"]), _same_select(g, tw)]
    if got["status"] == 0 and not erased:                                         # erase = 0, then the separate call: the same end
        assert g.erase_mkf(got["victim"]) == tw.erase_mkf(got["victim"])
        out += [_same_store(g, tw, g.get_meas()["alive"]), _same_select(g, tw)]
        assert not (g.get_mkfs(got["victim"], 1)["flags"][0] & mg.MKF_PRESENT)
    g.close(); tw.close(); t.close()
    return b"".join(out)


# ---- 1. the queries: every case, twice ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c["queries"]], ids=[c["name"] for c in CASES if c["queries"]])
def test_queries_equal_the_host_twin_byte_for_byte(gpu_required, c):
    first = _queries(c)
    assert _queries(c) == first                                                   # a fresh graph, the same bytes


# ---- 2. the removals: every case, twice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c["culls"]], ids=[c["name"] for c in CASES if c["culls"]])
def test_removal_equals_the_numpy_outcome_fed_to_a_twin(gpu_required, c):
    for k in c["culls"]:
        first = _removal(c, k)
        assert _removal(c, k) == first


# ---- 3. one whole turn ---------------------------------------------------------------------------------------------------------------------------------
def test_a_whole_turn(gpu_required):
    """cull_mkf(slot = -1, furthest_from = newest) -> cull_sweep -> compact -> select: the selection names neither the victim nor a marked row."""
    c = BY_NAME["seeded32"]
    a = c["a"]
    newest = int(np.flatnonzero(a["mkf_flags"] & mg.MKF_PRESENT)[0])
    want, a1 = mg.cull_mkf_ref(a, slot=-1, furthest_from=newest)
    t = _table(a)
    g = _graph(t, a)
    far = g.furthest_multi_keyframe(src_slot=newest)
    got = g.cull_mkf(slot=-1, furthest_from=newest)
    assert got["status"] == 0 and got["victim"] == want["victim"] == int(far["slot"]) and got["victim_dist"] == float(far["dist"]) and got["n_rows_marked"] == want["n_rows_marked"] > 0
    marked = np.flatnonzero(a1["pending"] != 0)
    r2, rows = g.cull_sweep(min_outliers=1 << 30, danglers=False)
    assert rows.tolist() == marked.tolist()
    live, stored = g.num_meas()
    g.compact()
    assert g.num_meas() == (live, live) and g.check() == (0, 0) and live < stored
    res, mkfs, points, meas = g.select_raw(mg.select_params(mode=mg.BUNDLE_ALL, min_points=0))
    assert res.status == 0 and res.n_points > 50
    assert got["victim"] not in mkfs["slot"].tolist() and not np.isin(points["row"], marked).any()
    assert not (g.get_meas()["mkf"] == got["victim"]).any()
    # the thin methods over the same call
    ext = nc.ext_of(a, slot=newest)
    it = g.closest_multi_keyframe(ext=ext)
    assert int(it["slot"]) == newest and float(it["dist"]) == 0.0
    assert g.need_new_multi_keyframe(ext, 2.0, 9) is False and g.is_distance_to_nearest_mkf_excessive(ext, lambda s: 2.0) is False
    three = g.n_closest_multi_keyframes(3, ext=ext, want_meas=True)
    assert g.need_new_multi_keyframe_by_meas(ext, 0) == (0 < 0.7 * three["n_meas"].sum() / 3) and g.need_new_multi_keyframe_by_meas(ext, 1 << 20) is False
    cam = int(np.flatnonzero(a["kf_active"][newest])[0])
    near = g.closest_keyframes_within_dist(newest, cam, 1000.0, n_max=5, region=mg.NB_ONLY_OTHER)
    assert len(near) == 5 and (near["slot"] != newest).all() and g.closest_keyframe(newest, cam)["dist"] <= near["dist"][0]
    g.close(); t.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(gpu_required):
    from mcptam_amd import chain_bundle
    c = BY_NAME["rules"]
    a = c["a"]
    t = _table(a)
    g = _graph(t, a)
    assert g.neighbours_last_timing() == -1.0 and g.cull_mkf_last_timing() == -1.0
    g.neighbours(kind=mg.NB_MKF, src_slot=0, n_max=3)
    g.cull_mkf(slot=5, erase=False)
    S = mg.select_params(mode=mg.BUNDLE_ALL, min_points=0)
    store0, num0, good0, mk0, sel0, time0 = g.get_meas(), g.num_meas(), g.good_counts().tobytes(), g.get_mkfs(0, 8), g.select_raw(S), (g.neighbours_last_timing(), g.cull_mkf_last_timing())
    assert min(time0) >= 0.0

    def refused(prefix, needle, call):
        with pytest.raises(RuntimeError):
            call()
        err = chain_bundle.last_error()
        assert needle in err and err.startswith(prefix), err
        assert g.num_meas() == num0 and all(store0[q].tobytes() == v.tobytes() for q, v in g.get_meas().items()) and g.good_counts().tobytes() == good0
        assert all(mk0[q].tobytes() == v.tobytes() for q, v in g.get_mkfs(0, 8).items()) and (g.neighbours_last_timing(), g.cull_mkf_last_timing()) == time0
        sel = g.select_raw(S)
        assert bytes(sel[0]) == bytes(sel0[0]) and all(u.tobytes() == v.tobytes() for u, v in zip(sel[1:], sel0[1:]))
    good = dict(kind=mg.NB_KF, src_slot=0, src_cam=0, n_max=4)
    ext = nc.ext_of(a, slot=2)
    for needle, q in (("unknown kind", dict(good, kind=2)), ("unknown region", dict(good, region=3)), ("unknown order", dict(good, order=2)), ("present slot", dict(good, src_slot=6)),
                      ("present slot", dict(good, src_slot=-2)), ("present slot", dict(good, src_slot=mg.MAX_MKFS)), ("outside the rig", dict(good, src_cam=2)),
                      ("same_cam", dict(good, region=mg.NB_ONLY_SELF, same_cam=True)), ("n_max", dict(good, n_max=0)), ("n_max", dict(good, n_max=33)),
                      ("max_dist", dict(good, max_dist=np.nan)), ("max_dist", dict(good, max_dist=-0.5)), ("mean_diff_fraction", dict(good, mean_diff_fraction=np.nan)),
                      ("non-finite pose", dict(good, src_slot=-1, ext=dict(ext, base_from_world=np.full(12, np.inf)))),
                      ("finite and positive", dict(good, src_slot=-1, ext=dict(ext, kf_depth_mean=np.array([-1.0, 1.0])))),
                      ("not active", dict(good, src_slot=-1, ext=dict(ext, kf_active=np.array([0, 1]))))):
        refused("mcp_map_neighbours", needle, lambda: g.neighbours(**q))
    for needle, k in (("not a present slot", dict(slot=6)), ("not a present slot", dict(slot=-3)), ("not a present slot", dict(slot=mg.MAX_MKFS)),
                      ("furthest_from", dict(slot=-1, furthest_from=6)), ("negative max_kfs", dict(slot=3, max_kfs=-1)), ("not finite", dict(slot=3, mean_diff_fraction=np.inf))):
        refused("mcp_map_mkf_cull", needle, lambda: g.cull_mkf(**k))
    L, p = g._L, mg.neigh_params(**good)
    res = mg.NeighResult(); ctypes.memset(ctypes.addressof(res), 0x5a, ctypes.sizeof(res))
    refused("mcp_map_neighbours", "NULL params", lambda: mg._chk(L.mcp_map_neighbours(g._h, None, ctypes.addressof(res)), "x"))
    refused("mcp_map_neighbours", "NULL result", lambda: mg._chk(L.mcp_map_neighbours(g._h, ctypes.addressof(p), None), "x"))
    refused("mcp_map_mkf_cull", "NULL params or result", lambda: mg._chk(L.mcp_map_mkf_cull(g._h, None, None), "x"))
    assert bytes(res) == b"\x5a" * ctypes.sizeof(res)
    # a source keyframe that is not active is refused from the graph's own columns
    g.update_mkfs([1], a["base_from_world"][[1]], a["mkf_flags"][[1]], np.array([[0, 1]]), a["kf_depth_mean"][[1]])
    with pytest.raises(RuntimeError):
        g.neighbours(kind=mg.NB_KF, src_slot=1, src_cam=0)
    assert "not active" in chain_bundle.last_error()
    # and after all that a removal goes as if nothing had happened
    b = mg.cull_mkf_ref(a, slot=5, erase=False)[1]
    b["kf_active"] = a["kf_active"].copy(); b["kf_active"][1, 0] = 0
    assert g.cull_mkf(slot=-1, furthest_from=0) == mg.cull_mkf_host(b, slot=-1, furthest_from=0)[0]
    g.close(); t.close()
