"""The device-resident map graph on the GPU: the one-call bundle selection against mcp_map_bundle_select_host byte for byte, the size seams of
its passes, the store's life cycle, its ordering with the table's stream, the selection through the solver, and the refusals."""
import ctypes

import numpy as np
import pytest

import map_graph_cases as mc
from mcptam_amd import map_graph as mg

pytestmark = pytest.mark.gpu

CASES = [(n, a, S) for n, a, S in mc.plain_cases()] + [(n, a, S) for n, a, S, _ in mc.edited_cases()]


def _device(a, cams=None):
    """(table, graph) holding the flat arrays `a`."""
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    N = len(a["pt_flags"])
    z = np.zeros((N, 3))
    if N:
        t.set(a["world_pos"], z, z, np.ones(N, dtype=np.uint8))
    g = mg.MapGraph(t, a["cam_from_base"], cams=cams)
    g.load_arrays(a)
    return t, g


@pytest.mark.parametrize("name,a,S", CASES, ids=[c[0] for c in CASES])
def test_device_equals_host(gpu_required, name, a, S):
    t, g = _device(a)
    host = mg.bundle_select_host(a, S)
    dev = g.select_raw(S)
    mc.assert_same_selection(dev, host, exact=True)
    again = g.select_raw(S)
    assert bytes(again[0]) == bytes(dev[0])
    for x, y in zip(again[1:], dev[1:]):
        assert x.tobytes() == y.tobytes()
    g.close(); t.close()


def _random_map(seed, n_mkf, n_rows, n_store, ncam=2):
    """A seeded random bipartite map: MKFs along a wavy line, points around it, n_store distinct (mkf, cam, row) entries of which every third is
    dead, a few bad and fixed MKFs, bad and fixed points; a row's source is the keyframe of its first live entry."""
    rng = np.random.default_rng([20260927, seed])
    from mcptam_amd import synth
    cam_R, cam_t = synth.make_rig(ncam)
    a = dict(ncam=ncam, cam_from_base=mg.poses12(cam_R, cam_t))
    R = np.array([synth.so3_exp(rng.normal(size=3) * 0.3) for _ in range(n_mkf)])
    centre = np.stack([0.5 * np.arange(n_mkf), np.sin(0.3 * np.arange(n_mkf)), 0.1 * rng.normal(size=n_mkf)], axis=1)
    a["base_from_world"] = mg.poses12(R, -np.einsum("kij,kj->ki", R, centre))
    fl = np.full(n_mkf, mg.MKF_PRESENT, dtype=np.int32)
    fl[rng.random(n_mkf) < 0.1] |= mg.MKF_BAD
    fl[rng.random(n_mkf) < 0.1] |= mg.MKF_FIXED
    fl[n_mkf - 1] = mg.MKF_PRESENT
    a["mkf_flags"] = fl
    a["kf_active"] = (rng.random((n_mkf, ncam)) < 0.9).astype(np.uint8); a["kf_active"][:, 0] = 1
    a["kf_depth_mean"] = rng.uniform(2.0, 6.0, (n_mkf, ncam))
    a["world_pos"] = centre[rng.integers(0, n_mkf, n_rows)] + rng.normal(size=(n_rows, 3)) * 3
    keys = rng.choice(n_mkf * ncam * n_rows, n_store, replace=False)
    a["ms_row"] = (keys % n_rows).astype(np.int32)
    a["ms_cam"] = ((keys // n_rows) % ncam).astype(np.int32)
    a["ms_mkf"] = (keys // (n_rows * ncam)).astype(np.int32)
    if n_mkf > 8:                                                       # measurements are local: an MKF measures the rows of its stretch of the line
        a["ms_mkf"] = np.clip((a["ms_row"].astype(np.int64) * n_mkf) // max(n_rows, 1) + (a["ms_mkf"] % 5) - 2, 0, n_mkf - 1).astype(np.int32)
        k3 = (a["ms_mkf"].astype(np.int64) * ncam + a["ms_cam"]) * n_rows + a["ms_row"]
        _, first = np.unique(k3, return_index=True)                     # one entry per (mkf, cam, row)
        keep = np.sort(first)
        for k in ("ms_row", "ms_cam", "ms_mkf"):
            a[k] = a[k][keep]
        fill = n_store - len(keep)                                      # the store keeps its size: further distinct entries, anywhere
        if fill:
            free = np.setdiff1d(np.arange(n_mkf * ncam * n_rows), k3[keep])[:fill]
            a["ms_row"] = np.concatenate([a["ms_row"], (free % n_rows)]).astype(np.int32)
            a["ms_cam"] = np.concatenate([a["ms_cam"], (free // n_rows) % ncam]).astype(np.int32)
            a["ms_mkf"] = np.concatenate([a["ms_mkf"], free // (n_rows * ncam)]).astype(np.int32)
    M = len(a["ms_row"])
    assert M == n_store
    a["ms_uv"] = rng.uniform(0, 480, (M, 2)); a["ms_level"] = rng.integers(0, 4, M).astype(np.int32); a["ms_source"] = rng.integers(0, 5, M).astype(np.int32)
    a["ms_alive"] = np.ones(M, dtype=np.uint8); a["ms_alive"][2::3] = 0
    pf = np.zeros(n_rows, dtype=np.int32)
    pf[rng.random(n_rows) < 0.05] |= mg.GP_BAD
    pf[rng.random(n_rows) < 0.05] |= mg.GP_FIXED
    sm, sc = np.full(n_rows, -1, dtype=np.int32), np.zeros(n_rows, dtype=np.int32)
    for i in np.flatnonzero(a["ms_alive"])[::-1]:
        sm[a["ms_row"][i]], sc[a["ms_row"][i]] = a["ms_mkf"][i], a["ms_cam"][i]
    pf[(sm < 0) & ((pf & mg.GP_FIXED) == 0)] |= mg.GP_FIXED            # a row without a live entry has no source: only a fixed point may
    sm[(pf & mg.GP_FIXED) != 0] = -1
    a["src_mkf"], a["src_cam"], a["pt_flags"] = sm, sc, pf
    return a


SEAMS = [("store-%d" % m, 12, 300, m) for m in (1, 255, 256, 257, 513, 1025)] + [("rows-%d" % r, 12, r, min(600, 20 * r)) for r in (1, 255, 256, 257)] + \
        [("mkfs-%d" % p, p, 300, 1500) for p in (3, 64, 65, 256, 257)]


@pytest.mark.parametrize("name,n_mkf,n_rows,n_store", SEAMS, ids=[s[0] for s in SEAMS])
def test_seams(gpu_required, name, n_mkf, n_rows, n_store):
    a = _random_map(SEAMS.index((name, n_mkf, n_rows, n_store)), n_mkf, n_rows, n_store)
    t, g = _device(a)
    ok = ((a["mkf_flags"] & mg.MKF_PRESENT) != 0) & ((a["mkf_flags"] & mg.MKF_BAD) == 0)
    good = np.bincount(a["ms_row"][(a["ms_alive"] != 0) & ok[a["ms_mkf"]]], minlength=n_rows)
    assert np.array_equal(g.good_counts(), good)
    assert g.num_meas() == (int(a["ms_alive"].sum()), n_store)
    statuses = []
    for S in (mg.select_params(mg.BUNDLE_ALL, min_points=1), mc.recent(a, recent_min_size=2, min_points=1)):
        host = mg.bundle_select_host(a, S)
        mc.assert_same_selection(g.select_raw(S), host, exact=True)
        mc.assert_same_selection(host, mg.bundle_select_ref(a, S), a, exact=False)
        statuses.append(host[0].status)
    if n_store >= 255 and n_rows >= 255:
        assert statuses == [0, 0], statuses                            # (the seam sizes select something)
    g.close(); t.close()


def test_store_life_cycle(gpu_required):
    a = mc.arrays("tiny12")
    M = len(a["ms_mkf"])
    t, g = _device(a)
    assert g.num_meas() == (M, M) and g.check() == (0, 0)
    # erase: every fourth entry, plus keys that match nothing (a row the keyframe does not measure, a camera nobody uses)
    dead = np.arange(0, M, 4)
    km = np.concatenate([a["ms_mkf"][dead], [0, 11, 5]]); kc = np.concatenate([a["ms_cam"][dead], [0, 1, 7]])
    free = [r for r in range(300) if not ((a["ms_mkf"] == 0) & (a["ms_cam"] == 0) & (a["ms_row"] == r)).any()][0]
    free2 = [r for r in range(300) if not ((a["ms_mkf"] == 11) & (a["ms_cam"] == 1) & (a["ms_row"] == r)).any()][0]
    kr = np.concatenate([a["ms_row"][dead], [free, free2, 3]])
    assert g.erase_meas(km, kc, kr) == len(dead)
    assert g.erase_meas(km, kc, kr) == 0                                 # they are dead already
    a["ms_alive"][dead] = 0
    got = g.get_meas()
    for k in ("mkf", "cam", "row", "level", "source", "alive"):
        assert np.array_equal(got[k], a["ms_" + k]), k
    assert got["uv"].tobytes() == a["ms_uv"].tobytes()
    assert g.num_meas() == (M - len(dead), M) and g.check() == (0, len(dead))
    assert np.array_equal(g.good_counts(), np.bincount(a["ms_row"][a["ms_alive"] != 0], minlength=300))
    S = mc.recent(a)
    before = g.select_raw(S)
    mc.assert_same_selection(before, mg.bundle_select_host(a, S), exact=True)
    # compact: the live entries in their order; the same selection but for the store indices
    g.compact()
    live = np.flatnonzero(a["ms_alive"])
    got = g.get_meas()
    assert g.num_meas() == (len(live), len(live)) and got["alive"].all()
    for k in ("mkf", "cam", "row", "level", "source"):
        assert np.array_equal(got[k], a["ms_" + k][live]), k
    assert got["uv"].tobytes() == a["ms_uv"][live].tobytes()
    after = g.select_raw(S)
    assert bytes(after[0]) == bytes(before[0]) and after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()
    for f in mg.MEAS_DTYPE.names:
        if f == "store":
            assert np.array_equal(live[after[3]["store"]], before[3]["store"])
        else:
            assert after[3][f].tobytes() == before[3][f].tobytes(), f
    g.compact()                                                          # nothing dead: nothing happens
    assert g.num_meas() == (len(live), len(live))
    # erase_mkf: every entry of slot 4 dies, the slot is gone
    c = {k: a["ms_" + k][live] for k in ("mkf", "cam", "row", "uv", "level", "source")}
    n4 = int((c["mkf"] == 4).sum())
    assert n4 > 0 and g.erase_mkf(4) == n4
    assert g.num_meas() == (len(live) - n4, len(live))
    assert np.array_equal(g.get_meas()["alive"], (c["mkf"] != 4).astype(np.uint8))
    with pytest.raises(RuntimeError, match="not present"):
        g.add_meas([4], [0], [0], [[1.0, 2.0]], [0])
    b = mg.copy_arrays(a)
    for k in c:
        b["ms_" + k] = c[k]
    b["ms_alive"] = (c["mkf"] != 4).astype(np.uint8); b["mkf_flags"][4] = 0
    mc.assert_same_selection(g.select_raw(mg.select_params(mg.BUNDLE_ALL)), mg.bundle_select_host(b, mg.select_params(mg.BUNDLE_ALL)), exact=True)
    # a planted duplicate
    first = g.add_meas([c["mkf"][0], 2], [c["cam"][0], 1], [c["row"][0], 299], [[1.0, 2.0], [3.0, 4.0]], [0, 1], [1, 3])
    assert first == len(live)
    dup, n_dead = g.check()
    assert dup == 1 + int(((b["ms_mkf"] == 2) & (b["ms_cam"] == 1) & (b["ms_row"] == 299) & (b["ms_alive"] != 0)).any()) and n_dead == n4
    g.close(); t.close()


def test_ordering_with_the_tables_stream(gpu_required):
    from mcptam_amd import chain_bundle
    rng = np.random.default_rng(5)
    p = mc.problem("tiny")
    a = mc.arrays("tiny")
    N = 60
    t, g = _device(a)
    S = mg.select_params(mg.BUNDLE_ALL)
    mc.assert_same_selection(g.select_raw(S), mg.bundle_select_host(a, S), exact=True)
    # an update of some rows, then the select with no wait between
    ids = np.arange(3, N, 7)
    a["world_pos"][ids] += rng.normal(size=(len(ids), 3)) * 0.05
    z = np.zeros((len(ids), 3))
    t.update(ids, a["world_pos"][ids], z, z, np.ones(len(ids), dtype=np.uint8))
    moved = g.select_raw(S)
    mc.assert_same_selection(moved, mg.bundle_select_host(a, S), exact=True)
    # a write-back of an adjustment of the whole map, then the select: x is CamFromWorld_src * the rows the write-back left
    rays = np.tile(np.array([0.0, 0.0, 1.0]), (N, 1)), np.tile(np.array([0.0025, 0.0, 1.0]) / np.linalg.norm([0.0025, 0.0, 1.0]), (N, 1)), \
        np.tile(np.array([0.0, 0.0025, 1.0]) / np.linalg.norm([0.0, 0.0025, 1.0]), (N, 1))
    t.set_rays(*rays)
    b = chain_bundle.ChainBundle(p.cams, True, True, False)
    bids = p.populate(b)
    assert b.Compute(3) > 0
    wb = t.write_back(b, bids["point"], np.arange(N))
    written = g.select_raw(S)
    assert np.abs(wb["world_pos"] - a["world_pos"]).max() > 1e-6       # the adjustment moved the points
    a["world_pos"] = np.ascontiguousarray(wb["world_pos"])
    assert t.get()[0].tobytes() == a["world_pos"].tobytes()
    mc.assert_same_selection(written, mg.bundle_select_host(a, S), exact=True)
    assert written[2]["x"].tobytes() != moved[2]["x"].tobytes()
    g.close(); t.close()


def test_selection_through_the_solver(gpu_required):
    """tiny with 12 MKFs: from_problem -> select(ALL) -> populate -> Compute(10) against the same arrays through the host call (equal input bytes,
    so bit-equal logs and state) and against the Problem populated directly."""
    from helpers import run_bundle
    from mcptam_amd import chain_bundle, synth
    from mcptam_amd.pvs import MapPointTable
    p = synth.make_config("tiny", n_mkf=12)
    a = mg.problem_arrays(p)
    t = MapPointTable()
    g = mg.MapGraph.from_problem(t, p, arrays=a)
    res, q = g.select(mg.BUNDLE_ALL)
    assert res.status == 0 and (res.n_adjust, res.n_fixed, res.n_points, res.n_meas) == (12, 0, p.n_points, p.n_meas)
    assert np.array_equal(q.window["mkf"], np.arange(12)) and np.array_equal(q.window["points"], np.arange(p.n_points))
    hres, hm, hp, hs = mg.bundle_select_host(a, mg.select_params(mg.BUNDLE_ALL))
    qh = mg.selection_problem(hm, hp, hs, a["base_from_world"], a["cam_from_base"], p.cams)
    runs = [run_bundle(chain_bundle.ChainBundle(p.cams, True, True, False), x, 10) for x in (q, qh, p)]
    dev, host, direct = runs
    assert dev["rc"] == host["rc"] and dev["logs"] == host["logs"]
    for k in ("R", "t", "X"):
        assert dev[k].tobytes() == host[k].tobytes(), k
    assert sum(l["accepted"] for l in dev["logs"]) == sum(l["accepted"] for l in direct["logs"]) and dev["rc"] == direct["rc"]
    # The selection's x is CamFromWorld_src * (CamFromWorld_src^-1 * pt_x): pt_x to a few ulp (4.5e-16 relative here).  MEASURED, not derived: on
    # the CPU oracle (oracle.OracleBundle, Compute(10)) the final chi-squared of the host-selected Problem and of the Problem populated directly
    # differ by 4.5e-13 relative on this map; the bound is that with a margin of 10x.
    c_dev, c_dir = dev["logs"][-1]["chi2_end"], direct["logs"][-1]["chi2_end"]
    print("final chi2: selected %.17g direct %.17g relative difference %.3g" % (c_dev, c_dir, abs(c_dev - c_dir) / abs(c_dir)))
    assert abs(c_dev - c_dir) <= 4.5e-12 * abs(c_dir)
    g.close(); t.close()


def test_refusals(gpu_required):
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import MapPointTable
    a = mc.arrays("tiny12")
    t, g = _device(a)
    L = mg.lib()
    S = mc.recent(a)
    res0, mk0, pt0, ms0 = g.select_raw(S, copy=False)                    # views over the pinned block: they must keep their bytes
    keep = (bytes(res0), mk0.tobytes(), pt0.tobytes(), ms0.tobytes())
    store0 = {k: v.tobytes() for k, v in g.get_meas().items()}
    good0 = g.good_counts().tobytes()
    cfb = a["cam_from_base"]

    def refused(rc, needle=None):
        assert rc == -1 or rc is None, rc
        msg = chain_bundle.last_error()
        assert msg and (needle is None or needle in msg), msg

    def raises(fn, needle):
        with pytest.raises(RuntimeError, match=needle):
            fn()

    # create
    refused(L.mcp_map_graph_create(None, 2, cfb.ctypes.data), "NULL table")
    refused(L.mcp_map_graph_create(t._h, 0, cfb.ctypes.data), "ncam")
    refused(L.mcp_map_graph_create(t._h, 9, cfb.ctypes.data), "ncam")
    refused(L.mcp_map_graph_create(t._h, 2, None), "ncam")
    # MKF slots
    one = a["base_from_world"][:1], a["mkf_flags"][:1], a["kf_active"][:1], a["kf_depth_mean"][:1]
    raises(lambda: g.set_mkfs(*one, first=mg.MAX_MKFS), "MCP_MAP_MAX_MKFS")
    nf = a["base_from_world"][:1].copy(); nf[0, 4] = np.inf
    raises(lambda: g.set_mkfs(nf, *one[1:]), "non-finite")
    for d in (0.0, -1.0, np.nan, np.inf):
        raises(lambda: g.set_mkfs(one[0], one[1], one[2], np.full((1, 2), d)), "depth mean")
    raises(lambda: g.set_mkfs(one[0], np.array([64]), one[2], one[3]), "unknown flags")
    two = a["base_from_world"][:2], a["mkf_flags"][:2], a["kf_active"][:2], a["kf_depth_mean"][:2]
    raises(lambda: g.update_mkfs([3, 3], *two), "appears twice")
    raises(lambda: g.update_mkfs([3, mg.MAX_MKFS], *two), "outside")
    refused(L.mcp_map_graph_set_mkfs(None, 0, 0, None, None, None, None), "NULL graph")
    # point columns
    raises(lambda: g.update_points([300], [0], [0], [0]), "outside the table")
    raises(lambda: g.update_points([5], [-1], [0], [0]), "not fixed")
    raises(lambda: g.update_points([5, 5], [0, 0], [0, 0], [0, 0]), "appears twice")
    raises(lambda: g.update_points([5], [0], [2], [0]), "source camera")
    # measurement store
    raises(lambda: g.add_meas([12], [0], [0], [[1.0, 1.0]], [0]), "not present")
    raises(lambda: g.add_meas([0], [2], [0], [[1.0, 1.0]], [0]), "camera")
    raises(lambda: g.add_meas([0], [0], [300], [[1.0, 1.0]], [0]), "row")
    raises(lambda: g.add_meas([0], [0], [0], [[1.0, 1.0]], [4]), "level")
    raises(lambda: g.add_meas([0], [0], [0], [[1.0, np.nan]], [0]), "non-finite")
    raises(lambda: g.erase_meas([1, 1], [0, 0], [7, 7]), "twice")
    raises(lambda: g.erase_mkf(mg.MAX_MKFS), "outside")
    raises(lambda: g.get_meas(first=0, count=len(a["ms_mkf"]) + 1), "bad range")
    raises(lambda: g.good_counts(first=0, count=301), "bad arguments")
    # the select
    res = mg.SelectResult()
    refused(L.mcp_map_bundle_select(None, ctypes.addressof(S), ctypes.addressof(res)), "NULL graph")
    refused(L.mcp_map_bundle_select(g._h, None, ctypes.addressof(res)), "NULL params")
    refused(L.mcp_map_bundle_select(g._h, ctypes.addressof(S), None), "NULL result")
    for bad, needle in ((mg.select_params(5, 11), "unknown mode"), (mc.recent(a, newest=12), "not present"), (mc.recent(a, newest=-1), "not present"),
                        (mc.recent(a, n_recent=9), "n_recent"), (mc.recent(a, n_recent=-1), "n_recent"), (mc.recent(a, min_points=-1), "negative gate"),
                        (mc.recent(a, recent_min_size=-2), "negative gate"), (mc.recent(a, mean_diff_fraction=float("nan")), "not finite")):
        raises(lambda: g.select_raw(bad), needle)
    # nothing moved: the store, the columns, the views of the last select
    assert (bytes(res0), mk0.tobytes(), pt0.tobytes(), ms0.tobytes()) == keep
    views = g.views(copy=False)
    assert (views[0].tobytes(), views[1].tobytes(), views[2].tobytes()) == keep[1:]
    assert {k: v.tobytes() for k, v in g.get_meas().items()} == store0 and g.good_counts().tobytes() == good0
    again = g.select_raw(S)
    assert (bytes(again[0]), again[1].tobytes(), again[2].tobytes(), again[3].tobytes()) == keep
    g.close(); t.close()


def _every_call(t, g, a, rng, lane_mkf, lane_cam, n_parcel):
    """Every device call that sizes scratch from the map, once, on a live graph: each answer against its host twin on the flat arrays `a`
    (byte for byte, or equal integers).  Returns `a` as the calls leave the map."""
    import graph_list_cases as lc
    R, P, C = t.rows, len(a["mkf_flags"]), int(a["ncam"])
    assert len(a["pt_flags"]) == R
    for S in (mg.select_params(mg.BUNDLE_ALL, min_points=1), mc.recent(a, recent_min_size=2, min_points=1)):
        mc.assert_same_selection(g.select_raw(S), mg.bundle_select_host(a, S), exact=True)
    ok = ((a["mkf_flags"] & mg.MKF_PRESENT) != 0) & ((a["mkf_flags"] & mg.MKF_BAD) == 0)
    assert np.array_equal(g.good_counts(), np.bincount(a["ms_row"][(a["ms_alive"] != 0) & ok[a["ms_mkf"]]], minlength=R))
    # outliers: a handful of live entries and one key that matches nothing
    pick = np.flatnonzero(a["ms_alive"])[5::97][:6]
    km, kc, kr = np.r_[a["ms_mkf"][pick], 0], np.r_[a["ms_cam"][pick], 0], np.r_[a["ms_row"][pick], R + 7]
    r1, vd = g.cull_outliers(km, kc, kr)
    h1, hvd, a = mg.cull_outliers_host(a, km, kc, kr, n_rows=R)
    assert r1 == h1 and np.array_equal(vd, hvd)
    r2, rows = g.cull_sweep()
    h2, hrows, a = mg.cull_sweep_host(a, n_rows=R)
    assert r2 == h2 and np.array_equal(rows, hrows)
    for q in (dict(kind=mg.NB_MKF, src_slot=0, n_max=3, want_meas=True), dict(kind=mg.NB_KF, src_slot=1, src_cam=0, n_max=4)):
        assert bytes(g.neighbours(raw=True, **q)) == bytes(mg.neighbours_host(a, q, raw=True)), q
    slots = np.arange(P - 1, -1, -2)
    lists = mg.kf_lists_host(a, slots, R)
    lc.assert_same_lists(g.debug_kf_lists(slots), lists)
    # the scene depth at the graph's own poses against mcp_scene_depth_robust over the host twin's lists; the refreshed means go into the graph
    rec = g.refresh_depth(slots)
    cfb, bfw = a["cam_from_base"], a["base_from_world"]
    Rk, tk = mg._compose(cfb[None, :, :9].reshape(1, C, 3, 3), cfb[None, :, 9:], bfw[slots, None, :9].reshape(len(slots), 1, 3, 3), bfw[slots, None, 9:])
    want, _ = t.scene_depth(np.concatenate([Rk.reshape(-1, 9), tk.reshape(-1, 3)], axis=1), *lists)
    assert rec.tobytes() == want.tobytes()
    rec = rec.reshape(len(slots), C)
    fresh = rec["refreshed"] == 1
    dep = a["kf_depth_mean"][slots]; dep[fresh] = rec["mean"][fresh]; a["kf_depth_mean"][slots] = dep
    # a parcel of entries the store does not hold yet
    have = set(zip(a["ms_mkf"].tolist(), a["ms_cam"].tolist(), a["ms_row"].tolist()))
    free = [(l, r) for l in range(len(lane_mkf)) for r in range(R) if (lane_mkf[l], lane_cam[l], r) not in have]
    assert len(free) >= n_parcel
    lane, row = np.array([free[i] for i in rng.choice(len(free), n_parcel, replace=False)], dtype=np.int32).T
    uv, level = rng.uniform(0, 480, (n_parcel, 2)), rng.integers(0, 4, n_parcel)
    p = mg.MeasParcel.from_host(t, lane, row, uv, level)
    e = mg.parcel_entries(lane, row, uv, level, key=100 + row)
    assert p.entries().tobytes() == e.tobytes()
    res, lanes = g.commit_parcel(p, lane_mkf, lane_cam)
    _, hres, recs, hlanes = mg.parcel_commit_host(e, 100 + np.arange(R), a["pt_flags"], a["src_mkf"], a["src_cam"], lane_mkf, lane_cam, first=len(a["ms_mkf"]))
    assert res == hres and np.array_equal(lanes, hlanes)
    p.close()
    for k in ("mkf", "cam", "row", "level", "source"):
        a["ms_" + k] = np.concatenate([a["ms_" + k], recs[k]]).astype(np.int32)
    a["ms_uv"] = np.concatenate([a["ms_uv"], recs["uv"]]); a["ms_alive"] = np.concatenate([a["ms_alive"], recs["alive"] != 0]).astype(np.uint8)
    got = g.get_meas()
    for k in ("mkf", "cam", "row", "level", "source", "alive"):
        assert np.array_equal(got[k], a["ms_" + k]), k
    assert got["uv"].tobytes() == a["ms_uv"].tobytes() and g.num_meas() == (int(a["ms_alive"].sum()), len(a["ms_mkf"]))
    return a


def test_one_graph_lives_through_growth(gpu_required):
    """One graph stays alive while its table, point columns, store, slots and every call's scratch grow with work still queued: every call on
    it at 8 MKFs / 255 rows / 1000 entries, then growth to 9 MKFs / 513 rows / 2100 entries without a wait, then every call again.  The sizes
    cross one and two workgroups of rows, the store's first capacity and its doubling, and both formulas of the shared scratch."""
    rng = np.random.default_rng(20261020)
    R0, R1, M1 = 255, 513, 2100
    a = _random_map(77, 8, R0, 1000)
    t, g = _device(a)
    z = np.zeros((R1, 3))
    t.set_source(100 + np.arange(R0), [None] * R0, np.zeros(R0), np.zeros((R0, 2)))
    a = _every_call(t, g, a, rng, [2, 5], [0, 1], 40)
    # growth, nothing waited for in between: rows, point columns, store entries, an erase and a compaction, a ninth slot
    new = np.arange(R0, R1)
    world = a["base_from_world"][rng.integers(0, 8, len(new)), 9:] * -1.0 + rng.normal(size=(len(new), 3)) * 3
    t.resize(R1)
    t.set(world, z[:len(new)], z[:len(new)], np.ones(len(new), dtype=np.uint8), first=R0)
    t.update_source(new, 100 + new, [None] * len(new), np.zeros(len(new)), np.zeros((len(new), 2)))
    n_add = M1 - len(a["ms_mkf"])
    keys = rng.choice(8 * 2 * len(new), n_add, replace=False)                # distinct (mkf, cam, row) over the new rows: none is in the store
    am, ac, ar = (keys // (2 * len(new))).astype(np.int32), ((keys // len(new)) % 2).astype(np.int32), (R0 + keys % len(new)).astype(np.int32)
    sm, sc = rng.integers(0, 8, len(new)).astype(np.int32), rng.integers(0, 2, len(new)).astype(np.int32)
    g.update_points(new, sm, sc, np.zeros(len(new), dtype=np.int32))
    auv, alv, asrc = rng.uniform(0, 480, (n_add, 2)), rng.integers(0, 4, n_add).astype(np.int32), rng.integers(0, 5, n_add).astype(np.int32)
    assert g.add_meas(am, ac, ar, auv, alv, asrc) == len(a["ms_mkf"])
    a["world_pos"] = np.concatenate([a["world_pos"], world])
    a["src_mkf"], a["src_cam"] = np.concatenate([a["src_mkf"], sm]), np.concatenate([a["src_cam"], sc])
    a["pt_flags"] = np.concatenate([a["pt_flags"], np.zeros(len(new), dtype=np.int32)])
    a["pending"] = np.concatenate([a["pending"], np.zeros(len(new), dtype=np.uint8)]); a["usable"] = np.concatenate([a["usable"], np.ones(len(new), dtype=np.uint8)])
    for k, v in (("mkf", am), ("cam", ac), ("row", ar), ("level", alv), ("source", asrc)):
        a["ms_" + k] = np.concatenate([a["ms_" + k], v])
    a["ms_uv"] = np.concatenate([a["ms_uv"], auv]); a["ms_alive"] = np.concatenate([a["ms_alive"], np.ones(n_add, dtype=np.uint8)])
    assert len(a["ms_mkf"]) == M1
    dead = np.flatnonzero(a["ms_alive"])[3::211]
    assert g.erase_meas(a["ms_mkf"][dead], a["ms_cam"][dead], a["ms_row"][dead]) == len(dead)
    a["ms_alive"][dead] = 0
    g.compact()
    live = np.flatnonzero(a["ms_alive"])
    for k in ("mkf", "cam", "row", "uv", "level", "source", "alive"):
        a["ms_" + k] = a["ms_" + k][live]
    assert len(live) > 1024
    ninth = mg.poses12(np.eye(3)[None], np.array([[-4.0, 0.3, 0.0]])), np.array([mg.MKF_PRESENT], dtype=np.int32), np.ones((1, 2), dtype=np.uint8), np.array([[3.0, 4.0]])
    g.update_mkfs([8], *ninth)
    for k, v in zip(("base_from_world", "mkf_flags", "kf_active", "kf_depth_mean"), ninth):
        a[k] = np.concatenate([a[k], v])
    a = _every_call(t, g, a, rng, [3, 8, 8], [0, 0, 1], 1100)               # (a parcel past the 1024 entries its block starts with)
    g.close(); t.close()
