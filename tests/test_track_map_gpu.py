"""mcp_track_map (include/mcp_img.h): the whole Tracker::TrackMap of a frame from the resident table in one submission, bit for bit against
the composition of existing public calls on a twin table -- mcp_track_find_pvs, the Python selection (mcptam_amd.pvs.select_sets),
mcp_patch_sequences(MCP_PF_TRACK) with host-held finder states, mcp_track_pose_refine for the coarse stage, the two fine searches at the
updated pose, mcp_track_pose_refine over [C, T, R] -- plus the table's source and finder upkeep, stale sources, determinism, the fused
pyramids, refusals and the 50k-point map."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = 4
COARSE_NL = np.ones(10, dtype=np.uint8)
COARSE_OV = np.array([0.0] * 6 + [1.0] * 4)


@pytest.fixture(scope="module")
def world():
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
    from mcptam_amd.synth import so3_exp as ex
    R, t = sc["poseB"]
    prior = (ex(np.array([0.002, -0.001, 0.0015])) @ R, t + np.array([0.01, -0.006, 0.004]))
    return dict(sc=sc, cam=sc["cam"], src=src, cols=cols, cfbs=cfbs, targets=targets, prior=prior, n=n)


def _table(cols, first=0):
    from mcptam_amd.pvs import MapPointTable
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], cols["src"], cols["level"], cols["center"], cols["fixed"])
    return t


def _point(cols, r):
    return dict(world_pos=cols["wp"][r], pixel_right_w=cols["pr"][r], pixel_down_w=cols["pd"][r], source_kf=cols["src"][r],
                source_level=int(cols["level"][r]), center=tuple(int(v) for v in cols["center"][r]), fixed=int(cols["fixed"][r]))


def _search(cols, kf, cam, pose, cfb, rows, states_c, rng, its):
    from mcptam_amd import keyframe as K
    if len(rows) == 0:
        return np.zeros(0, dtype=K.TD_OUT_DTYPE)
    seqs = [[dict(point=_point(cols, r), point_key=int(cols["keys"][r]), target=0)] for r in rows]
    st = states_c[rows].copy()
    out = K.patch_sequences(K.PF_TRACK, [(kf, cam, pose, cfb)], seqs, st, rng, its)
    states_c[rows] = st
    return out


def compose(twin, cols, live, targets, cam, pose, cfbs, prm, states):
    """The host composition of existing calls.  live[row]: the row's source is alive.  states: per camera (rows,) PF_STATE_DTYPE, updated."""
    from mcptam_amd import keyframe as K
    from mcptam_amd.pvs import select_sets
    ncam = len(targets)
    cfb_arr = np.ascontiguousarray(np.stack([K._pose12(*c) for c in cfbs]))
    pvs = twin.find_pvs(targets, [cam] * ncam, pose, cfbs)
    counts = twin.counts.copy()
    sets, stale = [], []
    for c in range(ncam):
        lv = [pvs[c][l]["point"].astype(np.int64) for l in range(LEVELS)]
        stale.append(sum(int((~live[x]).sum()) for x in lv))
        sets.append(select_sets([x[live[x]] for x in lv], prm["seed"], c, prm["try_coarse"], prm["coarse_max"], prm["max_patches"]))
    outC = [_search(cols, targets[c], cam, pose, cfbs[c], sets[c][0], states[c], prm["coarse_range"], prm["coarse_subpix_its"]) for c in range(ncam)]
    found = sum(int(((o["found"] != 0) & (o["template_bad"] == 0)).sum()) for o in outC)
    did = found > prm["coarse_min"]
    recC = K.pose_points_frame([cols["wp"][sets[c][0]] for c in range(ncam)], outC)
    if did:
        pose, _, _, recC = K.track_pose_refine(recC, [cam] * ncam, cfb_arr, pose, nonlinear=COARSE_NL, override_sigma=COARSE_OV, estimator=prm["estimator"])
    rng = 5 if did else 10
    outT = [_search(cols, targets[c], cam, pose, cfbs[c], sets[c][1], states[c], rng, 8) for c in range(ncam)]
    outR = [_search(cols, targets[c], cam, pose, cfbs[c], sets[c][2], states[c], rng, 0) for c in range(ncam)]
    recs, o0 = [], 0
    for c in range(ncam):
        nC = len(sets[c][0])
        recs += [recC[o0:o0 + nC], K.pose_points(cols["wp"][sets[c][1]], outT[c], c), K.pose_points(cols["wp"][sets[c][2]], outR[c], c)]
        o0 += nC
    recs = np.concatenate(recs)
    pose, mu, w, _ = K.track_pose_refine(recs, [cam] * ncam, cfb_arr, pose, estimator=prm["estimator"])
    items, o0 = [], 0
    for c in range(ncam):
        C, T, R = sets[c]
        m = len(C) + len(T) + len(R)
        items.append(dict(point=np.concatenate([C, T, R]), stage=np.repeat([0, 1, 2], [len(C), len(T), len(R)]), weight_last=w[o0:o0 + m],
                          out=np.concatenate([outC[c], outT[c], outR[c]])))
        o0 += m
    return dict(items=items, pose=pose, mu=mu, did=did, found=found, counts=counts, sizes=[[len(s_) for s_ in sets[c]] for c in range(ncam)], stale=stale)


def _params(**kw):
    p = dict(try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=10, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=12345)
    p.update(kw)
    return p


def _run(table, targets, cam, pose, cfbs, prm, **kw):
    return table.track_map(targets, [cam] * len(targets), pose, cfbs, **prm, **kw)


def _assert_same(got, ref, ncam):
    items, pose, res = got
    assert np.array_equal(pose[0], ref["pose"][0]) and np.array_equal(pose[1], ref["pose"][1])
    assert np.array_equal(np.array(res.mu_last), ref["mu"])
    assert res.did_coarse == int(ref["did"]) and res.coarse_found == ref["found"]
    for c in range(ncam):
        assert list(res.pvs_counts[c]) == list(ref["counts"][c]), c
        assert list(res.set_sizes[c]) == ref["sizes"][c], c
        assert res.stale[c] == ref["stale"][c], c
        it, rf = items[c], ref["items"][c]
        assert np.array_equal(it["point"], rf["point"]) and np.array_equal(it["stage"], rf["stage"]), c
        assert np.array_equal(it["weight_last"], rf["weight_last"]), c
        for f in rf["out"].dtype.names:
            assert np.array_equal(it["out"][f], rf["out"][f], equal_nan=rf["out"][f].dtype.kind == "f"), (c, f)


def _same_items(a, b):
    """Field by field (numpy copies of structured arrays leave their padding bytes undefined)."""
    if len(a) != len(b):
        return False
    for f in ("point", "stage", "weight_last"):
        if not np.array_equal(a[f], b[f]):
            return False
    return all(np.array_equal(a["out"][f], b["out"][f], equal_nan=a["out"][f].dtype.kind == "f") for f in a["out"].dtype.names)


def _assert_states(table, states, ncam, n):
    for c in range(ncam):
        got = table.get_states(c, 0, n)
        for f in got.dtype.names:
            assert np.array_equal(got[f], states[c][f], equal_nan=got[f].dtype.kind == "f"), (c, f)


def _new_states(ncam, n):
    from mcptam_amd.keyframe import new_pf_states
    return [new_pf_states(n) for _ in range(ncam)]


CASES = {
    "coarse_taken": (dict(), 4),
    "coarse_not_reached": (dict(coarse_min=100000), 4),
    "no_coarse": (dict(try_coarse=0), 4),
    "budget_chops": (dict(max_patches=250), 4),
    "budget_no_chop": (dict(max_patches=100000), 1),
    "one_camera": (dict(), 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_track_map_equals_the_composition(gpu_required, world, case, monkeypatch):
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")      # (the composition's iterations past 1024 records: the kernel mcp_track_map runs)
    w = world
    kw, ncam = CASES[case]
    prm = _params(**kw)
    targets, cfbs = w["targets"][:ncam], w["cfbs"][:ncam]
    t, twin = _table(w["cols"]), _table(w["cols"])
    live = np.ones(w["n"], dtype=bool)
    states = _new_states(ncam, w["n"])
    got = _run(t, targets, w["cam"], w["prior"], cfbs, prm)
    ref = compose(twin, w["cols"], live, targets, w["cam"], w["prior"], cfbs, prm, states)
    _assert_same(got, ref, ncam)
    _assert_states(t, states, ncam, w["n"])
    res = got[2]
    if case == "coarse_taken":
        assert res.did_coarse == 1 and sum(res.set_sizes[c][0] for c in range(ncam)) > 0
    if case == "coarse_not_reached":
        assert res.did_coarse == 0 and res.coarse_found > 0
    if case == "no_coarse":
        assert all(res.set_sizes[c][0] == 0 for c in range(ncam))
    if ncam == 4:
        assert sum(res.pvs_counts[2]) == 0 and sum(res.pvs_counts[0]) > 0      # camera 2 looks away
    if case == "budget_chops":                                      # the chop ran: R filled the budget exactly, with entries left over
        for c in (0, 1, 3):
            C, T, R = res.set_sizes[c]
            assert C + T < 250 and R == 250 - C - T and sum(res.pvs_counts[c]) > 250
    assert sum(int((i["out"]["found"] != 0).sum()) for i in got[0]) > 50 and np.abs(np.array(res.mu_last)).max() > 0
    # this frame's PVS in place, as mcp_track_find_pvs gives it
    from mcptam_amd.pvs import PVS_ENTRY_DTYPE
    L = t._L
    ref_pvs = twin.find_pvs(targets, [w["cam"]] * ncam, w["prior"], cfbs)
    for c in range(ncam):
        for l in range(LEVELS):
            cnt = ctypes.c_int(0)
            ptr = L.mcp_track_find_pvs_view(t._h, c, l, ctypes.byref(cnt))
            assert cnt.value == len(ref_pvs[c][l])
            if cnt.value:
                v = np.frombuffer((ctypes.c_char * (cnt.value * PVS_ENTRY_DTYPE.itemsize)).from_address(ptr), dtype=PVS_ENTRY_DTYPE)
                assert v.tobytes() == ref_pvs[c][l].tobytes()


def test_states_carry_over_frames_and_reset_on_a_new_key(gpu_required, world, monkeypatch):
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    from mcptam_amd.synth import so3_exp
    w = world
    prm = _params()
    ncam = 4
    t, twin = _table(w["cols"]), _table(w["cols"])
    live = np.ones(w["n"], dtype=bool)
    states = _new_states(ncam, w["n"])
    p2 = (so3_exp(np.array([0.0005, 0.0, -0.0004])) @ w["prior"][0], w["prior"][1] + np.array([0.002, 0.0, -0.001]))
    for pose in (w["prior"], p2):
        got = _run(t, w["targets"], w["cam"], pose, w["cfbs"], prm)
        ref = compose(twin, w["cols"], live, w["targets"], w["cam"], pose, w["cfbs"], prm, states)
        _assert_same(got, ref, ncam)
        _assert_states(t, states, ncam, w["n"])
    before = [t.get_states(c) for c in range(ncam)]
    touched = np.nonzero(before[0]["valid"])[0][:5]
    assert len(touched) == 5
    cols = w["cols"]
    keys = cols["keys"][touched].copy()
    keys[:3] += 1000000                                                  # three rows become other points; two keep their key
    t.update_source(touched, keys, [cols["src"][r] for r in touched], cols["level"][touched], cols["center"][touched], cols["fixed"][touched])
    after = [t.get_states(c) for c in range(ncam)]
    for c in range(ncam):
        assert not after[c][touched[:3]].tobytes().strip(b"\0")
        assert after[c][touched[3:]].tobytes() == before[c][touched[3:]].tobytes()
        rest = np.setdiff1d(np.arange(w["n"]), touched[:3])
        assert after[c][rest].tobytes() == before[c][rest].tobytes()
    # shrinking drops the rows' finders: grown back, they are zero
    t.resize(w["n"] - 10)
    t.resize(w["n"])
    assert not t.get_states(0, w["n"] - 10, 10).tobytes().strip(b"\0")


def test_destroyed_source_rows_are_dropped_and_counted(gpu_required, world, monkeypatch):
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    from mcptam_amd.keyframe import KeyFrame
    w = world
    prm = _params()
    ncam = 4
    gone = KeyFrame(640, 480)
    gone.MakeKeyFrame_Lite(w["sc"]["imgA"])
    cols = dict(w["cols"])
    cols["src"] = [gone if (r % 4 == 1) else w["src"] for r in range(w["n"])]
    t, twin = _table(cols), _table(cols)
    # rows 3, 7, ... never get a source
    no_src = np.arange(3, w["n"], 8)
    t.update_source(no_src, cols["keys"][no_src], [None] * len(no_src), cols["level"][no_src], cols["center"][no_src], cols["fixed"][no_src])
    gone.close()
    live = np.array([(r % 4 != 1) for r in range(w["n"])])
    live[no_src] = False
    states = _new_states(ncam, w["n"])
    got = _run(t, w["targets"], w["cam"], w["prior"], w["cfbs"], prm)
    cols_ref = dict(cols, src=[w["src"]] * w["n"])                     # (only live rows reach the composition's searches)
    ref = compose(twin, cols_ref, live, w["targets"], w["cam"], w["prior"], w["cfbs"], prm, states)
    _assert_same(got, ref, ncam)
    assert got[2].stale[0] > 0
    for c in range(ncam):
        assert not np.isin(got[0][c]["point"], np.nonzero(~live)[0]).any()


def test_same_seed_same_bytes_other_seed_other_selection(gpu_required, world):
    w = world
    t = _table(w["cols"])
    runs = [_run(t, w["targets"], w["cam"], w["prior"], w["cfbs"], _params(seed=s, max_patches=300))[0] for s in (7, 7)]
    t2 = _table(w["cols"])
    a = _run(t2, w["targets"], w["cam"], w["prior"], w["cfbs"], _params(seed=7, max_patches=300))[0]
    b = _run(_table(w["cols"]), w["targets"], w["cam"], w["prior"], w["cfbs"], _params(seed=8, max_patches=300))[0]
    first = _run(_table(w["cols"]), w["targets"], w["cam"], w["prior"], w["cfbs"], _params(seed=7, max_patches=300))[0]
    for c in range(4):
        assert _same_items(a[c], first[c])
        assert np.array_equal(runs[0][c]["point"], runs[1][c]["point"])
    assert any(not np.array_equal(a[c]["point"], b[c]["point"]) for c in range(4) if len(a[c]))


def test_images_in_the_call_equal_pyramids_first(gpu_required, world):
    from mcptam_amd import hip_rt
    from mcptam_amd.keyframe import KeyFrame, make_lite_batch
    w = world
    prm = _params()
    kf_a = [KeyFrame(640, 480) for _ in range(4)]
    kf_b = [KeyFrame(640, 480) for _ in range(4)]
    img = np.ascontiguousarray(np.roll(w["sc"]["imgB"], 1, axis=1))
    ring = [hip_rt.dev_alloc(img.nbytes) for _ in range(4)]
    try:
        for r in ring:
            hip_rt.dev_upload(r, img)
        ta, tb = _table(w["cols"]), _table(w["cols"])
        a = _run(ta, kf_a, w["cam"], w["prior"], w["cfbs"], prm, imgs=ring, on_device=True)
        make_lite_batch(kf_b, [img] * 4)
        b = _run(tb, kf_b, w["cam"], w["prior"], w["cfbs"], prm)
        c_host = _run(ta, kf_a, w["cam"], w["prior"], w["cfbs"], prm, imgs=[img] * 4)      # (host images: the second frame of ta)
    finally:
        for r in ring:
            hip_rt.dev_free(r)
    for c in range(4):
        assert _same_items(a[0][c], b[0][c])
        for l in range(LEVELS):
            assert np.array_equal(kf_a[c].Image(l), kf_b[c].Image(l)) and np.array_equal(kf_a[c].Corners(l), kf_b[c].Corners(l))
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[1][1], b[1][1])
    assert kf_a[0].NumPrev() == 1 and len(c_host[0][0]) > 0


def test_refusals_enqueue_nothing(gpu_required, world):
    from mcptam_amd import chain_bundle
    from mcptam_amd.keyframe import _pose12
    from mcptam_amd.pvs import TrackMapParams, TrackMapResult, _bind_track_map
    from mcptam_amd.taylor_camera import camera_array
    w = world
    t = _table(w["cols"])
    _run(t, w["targets"], w["cam"], w["prior"], w["cfbs"], _params())
    before = [t.get_states(c).tobytes() for c in range(4)]
    L = _bind_track_map(t._L)
    hs = (ctypes.c_void_p * 9)(*([w["targets"][0]._h] * 9))
    cs = camera_array([w["cam"]] * 9)
    b = _pose12(*w["prior"]); b0 = b.copy()
    cfb = np.ascontiguousarray(np.concatenate([_pose12(np.eye(3), np.zeros(3))] * 9))
    res = TrackMapResult()

    def call(ncam=4, table=t._h, **kw):
        p = _params(**kw)
        prm = TrackMapParams(p["try_coarse"], p["coarse_max"], p["coarse_range"], p["coarse_min"], p["coarse_subpix_its"], p["max_patches"], 0, p["seed"])
        return L.mcp_track_map(table, ncam, hs, None, None, 0, None, ctypes.cast(cs, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data, ctypes.byref(prm), ctypes.byref(res))
    for kw in (dict(ncam=0), dict(ncam=9), dict(table=None), dict(coarse_max=-1), dict(coarse_range=-2), dict(max_patches=-5), dict(coarse_subpix_its=-1)):
        assert call(**kw) == -1, kw
        assert chain_bundle.last_error()
    assert np.array_equal(b, b0)
    assert [t.get_states(c).tobytes() for c in range(4)] == before


@pytest.mark.timeout(900)
def test_fifty_thousand_points_four_cameras(gpu_required, world, monkeypatch):
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    from mcptam_amd import synth_img
    w = world
    base = [dict(world_pos=w["cols"]["wp"][r], pixel_right_w=w["cols"]["pr"][r], pixel_down_w=w["cols"]["pd"][r]) for r in range(w["n"])]
    wp, pr, pd, us = synth_img.make_map_cloud(base, 50000, seed=1)
    n = len(wp)
    rng = np.random.default_rng(9)
    level = rng.integers(0, 4, n).astype(np.int32)
    cols = dict(wp=wp, pr=pr, pd=pd, usable=us, keys=np.arange(n, dtype=np.int32), src=[w["src"]] * n, level=level,
                center=np.ascontiguousarray(np.stack([320 >> level, 240 >> level], axis=1).astype(np.int32)), fixed=np.zeros(n, dtype=np.uint8))
    cfbs = [w["cfbs"][0], w["cfbs"][1], w["cfbs"][3], w["cfbs"][1]]
    prm = _params(max_patches=1000)
    t, twin = _table(cols), _table(cols)
    states = _new_states(4, n)
    got = _run(t, w["targets"], w["cam"], w["prior"], cfbs, prm)
    ref = compose(twin, cols, np.ones(n, dtype=bool), w["targets"], w["cam"], w["prior"], cfbs, prm, states)
    _assert_same(got, ref, 4)
    _assert_states(t, states, 4, n)
    assert sum(sum(got[2].pvs_counts[c]) for c in range(4)) > 10000


def test_pvs_view_after_the_table_shrinks(gpu_required, world):
    """mcp_track_find_pvs_view after mcp_track_map reads that call's PVS, laid out for the rows the table had then, also when the table has
    been cut since."""
    w = world
    t, twin = _table(w["cols"]), _table(w["cols"])
    _run(t, w["targets"], w["cam"], w["prior"], w["cfbs"], _params())
    t.resize(10)
    ref = twin.find_pvs(w["targets"], [w["cam"]] * 4, w["prior"], w["cfbs"])
    from mcptam_amd.pvs import PVS_ENTRY_DTYPE
    for c in range(4):
        for l in range(LEVELS):
            cnt = ctypes.c_int(0)
            ptr = t._L.mcp_track_find_pvs_view(t._h, c, l, ctypes.byref(cnt))
            assert cnt.value == len(ref[c][l])
            if cnt.value:
                v = np.frombuffer((ctypes.c_char * (cnt.value * PVS_ENTRY_DTYPE.itemsize)).from_address(ptr), dtype=PVS_ENTRY_DTYPE)
                assert v.tobytes() == ref[c][l].tobytes()
    # the next call starts from the cut table
    items, _, res = _run(t, w["targets"], w["cam"], w["prior"], w["cfbs"], _params())
    assert all(int(i["point"].max(initial=-1)) < 10 for i in items) and sum(res.pvs_counts[0]) <= 10


@pytest.mark.timeout(900)
def test_sets_longer_than_one_sort_go_in_chunks(gpu_required, world, monkeypatch):
    """More than 2048 keys in one set (k_tm_select sorts them in chunks of 2048): one camera, T and every level of R0 that long, no chop."""
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    from mcptam_amd import synth_img
    w = world
    base = [dict(world_pos=w["cols"]["wp"][r], pixel_right_w=w["cols"]["pr"][r], pixel_down_w=w["cols"]["pd"][r]) for r in range(w["n"])]
    wp, pr, pd, us = synth_img.make_map_cloud(base, 40000, seed=4, spread=0.5)
    n = len(wp)
    level = np.zeros(n, dtype=np.int32)
    cols = dict(wp=wp, pr=pr, pd=pd, usable=us, keys=np.arange(n, dtype=np.int32), src=[w["src"]] * n, level=level,
                center=np.tile(np.array([[320, 240]], dtype=np.int32), (n, 1)), fixed=np.zeros(n, dtype=np.uint8))
    prm = _params(max_patches=10 ** 6)
    t, twin = _table(cols), _table(cols)
    states = _new_states(1, n)
    got = _run(t, w["targets"][:1], w["cam"], w["prior"], w["cfbs"][:1], prm)
    ref = compose(twin, cols, np.ones(n, dtype=bool), w["targets"][:1], w["cam"], w["prior"], w["cfbs"][:1], prm, states)
    _assert_same(got, ref, 1)
    counts = list(got[2].pvs_counts[0])
    assert min(counts) > 2048 and got[2].set_sizes[0][1] > 2048, counts
    assert sum(ref["sizes"][0]) > 16384, ref["sizes"]              # k_tm_search's grid of 16 384 wavefronts strides once over the items
