"""mcp_map_refind (include/mcp_img.h): MapMakerServerBase::ReFind_Common of a list of (row, target) pairs over the resident table in one
submission -- bit for bit against the composition the map maker uses without it (mcp_patch_sequences(MCP_PF_REFIND, range 4) on items packed
from the same columns + mcptam_amd.refind.refind_verdicts; tests/refind_fixture.py; verdicts, every field of the measurements and every member
of the returned finder), against the CPU oracle (verdicts, integer fields, both templates bit for bit; positions to 1e-9, the tolerance of the
existing sub-pixel tests, and the finder's floating-point members -- last_warp, mean_diff: the same sub-pixel arithmetic -- to the same 1e-9), plus
the finder's rules, the table's rules, stream ordering, refusals and sizes."""
import ctypes

import numpy as np
import pytest

from refind_fixture import (EXPECTED, EXPECTED_FOUND_L0, EXPECTED_FOUND_UP, N_BASE, compose, make_world, moved, newly_made_targets, same_meas,
                            same_state)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(gpu_required):
    import oracle
    from mcptam_amd.keyframe import KeyFrame
    return make_world(KeyFrame, oracle.OracleKeyFrame)


def _table(w, cols=None, src=None):
    from mcptam_amd.pvs import MapPointTable
    cols = w["cols"] if cols is None else cols
    n = len(cols["wp"])
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], [w["A"]] * n if src is None else src, cols["level"], cols["center"], cols["fixed"])
    return t


def _finder(state=None):
    from mcptam_amd.keyframe import new_pf_states
    f = new_pf_states(1)
    if state is not None:
        f[0] = state[0]
    return f


def _all_rows(n, target=0):
    return np.stack([np.arange(n), np.full(n, target)], axis=1).astype(np.int32)


def _assert_equal(got, ref, states=True):
    v, m, counts, f = got
    rv, rm, rc, rf = ref[:4]
    assert np.array_equal(v, rv), np.nonzero(v != rv)[0][:10]
    assert same_meas(m, rm)
    assert list(counts) == list(rc)
    if states and f is not None:
        assert same_state(f, rf)


def _oracle(w, targets, pairs, per_row=False, finder=None):
    import oracle
    tg = [(w["B_o"], cam, pose) for _, cam, pose in targets]
    return compose(w["cols"], None, tg, pairs, per_row, finder, search=oracle.oracle_patch_sequences, src_oracle=w["A_o"])


def _assert_oracle(got, ref):
    v, m, counts, f = got
    rv, rm, rc, rf = ref[:4]
    assert np.array_equal(v, rv) and list(counts) == list(rc)
    assert same_meas(m, rm, pos_tol=1e-9)
    if f is not None:
        for name in f.dtype.names:
            if f[name].dtype.kind == "f":
                assert np.allclose(f[name], rf[name], rtol=0, atol=1e-9), name
            else:
                assert np.array_equal(f[name], rf[name]), name


def test_one_keyframe_the_whole_map(world):
    w = world
    targets = [(w["B"], w["cam"], w["sc"]["poseB"])]
    pairs = _all_rows(w["n"])
    t = _table(w)
    f = _finder()
    got = t.refind(targets, pairs, False, f)
    ref = compose(w["cols"], w["A"], targets, pairs, False, _finder())
    print("counts", list(got[2]))
    _assert_equal(got, ref)
    _assert_oracle(got, _oracle(w, targets, pairs, False, _finder()))
    for verdict, want in EXPECTED.items():
        assert got[2][verdict] == want, (verdict, int(got[2][verdict]), want)
    m = got[1]
    assert (int((m["level"] == 0).sum()), int((m["level"] > 0).sum())) == (EXPECTED_FOUND_L0, EXPECTED_FOUND_UP)
    assert np.array_equal(m["pair"], np.sort(m["pair"])) and np.array_equal(m["row"], pairs[m["pair"], 0])
    # in place: the same records in the library's pinned block
    v2, m2, c2, _ = t.refind(targets, pairs, False, None, view=True)
    assert np.array_equal(v2, got[0]) and same_meas(m2, m) and list(c2) == list(got[2])


def test_newly_made_points_share_templates_between_keyframes(world):
    w = world
    targets = newly_made_targets(w["sc"], w["B"])
    pairs = np.stack([np.repeat(np.arange(N_BASE), 4), np.tile(np.arange(4), N_BASE)], axis=1).astype(np.int32)
    t = _table(w)
    got = t.refind(targets, pairs, True, _finder())
    ref = compose(w["cols"], w["A"], targets, pairs, True, _finder())
    _assert_equal(got, ref)
    _assert_oracle(got, _oracle(w, targets, pairs, True, _finder()))
    alone = t.refind(targets, pairs, False, _finder())
    _assert_equal(alone, compose(w["cols"], w["A"], targets, pairs, False, _finder()))
    s1, s0 = dict(zip(got[1]["pair"], got[1]["score"])), dict(zip(alone[1]["pair"], alone[1]["score"]))
    differ = sum(1 for p in s1 if pairs[p, 1] == 1 and p in s0 and s0[p] != s1[p])
    print("pairs of target 1 whose score differs:", differ)
    assert differ >= 100
    from mcptam_amd.refind import OUTSIDE
    assert (got[0][pairs[:, 1] == 2] == OUTSIDE).all()


def test_the_static_finder_carries_over_calls(world):
    w = world
    from mcptam_amd.refind import FOUND
    pB = w["sc"]["poseB"]
    targets = [(w["B"], w["cam"], pB), (w["B"], w["cam"], moved(pB, (0.0003, -0.0002, 0.001), (0.003, -0.001, 0.002)))]
    t = _table(w)
    v_all = t.refind(targets, _all_rows(N_BASE), False, None)[0]
    r = int(np.nonzero(v_all == FOUND)[0][40])
    one = np.array([[q, 0] for q in range(r - 5, r + 1)], dtype=np.int32)          # call one ends on (row r, B)
    two = np.array([[r, 1]] + [[q, 1] for q in range(r + 1, r + 6)], dtype=np.int32)   # call two starts with (row r, moved B)
    f = _finder()
    got1 = t.refind(targets, one, False, f)
    ref1 = compose(w["cols"], w["A"], targets, one, False, _finder())
    _assert_equal(got1, ref1)
    assert f[0]["valid"] == 1 and f[0]["point_key"] == w["cols"]["keys"][r]
    for per_row in (False, True):
        f2 = _finder(f)
        got2 = t.refind(targets, two, per_row, f2)
        ref2 = compose(w["cols"], w["A"], targets, two, per_row, _finder(ref1[3]))
        _assert_equal(got2, ref2)
        # without the carried finder the first pair is what a fresh finder gives
        fresh = t.refind(targets, two, per_row, None)
        ref_fresh = compose(w["cols"], w["A"], targets, two, per_row, None)
        _assert_equal(fresh, ref_fresh, states=False)
    # the carried template is observable on that first pair
    a = t.refind(targets, two[:1], False, _finder(f))
    b = t.refind(targets, two[:1], False, None)
    assert a[0][0] == FOUND and b[0][0] == FOUND and a[1]["score"][0] != b[1]["score"][0]
    # a call whose pairs all fail the projection leaves the finder as it came
    away = [(w["B"], w["cam"], moved(pB, (0.0, np.pi, 0.0), (0, 0, 0)))]
    f3 = _finder(f)
    t.refind(away, np.array([[r, 0]], dtype=np.int32), False, f3)
    assert same_state(f3, f)
    f4 = _finder(f)
    t.refind(away, np.array([[r, 0], [r + 1, 0]], dtype=np.int32), False, f4)      # the last sequence is another one: a finder that has seen nothing
    assert not f4.tobytes().strip(b"\0")


@pytest.mark.timeout(900)
def test_fifty_thousand_rows_one_keyframe(world):
    from mcptam_amd import synth_img
    w = world
    wp, pr, pd, us = synth_img.make_map_cloud(w["base"], 50000, seed=1)
    n = len(wp)
    level = np.random.default_rng(9).integers(0, 4, n).astype(np.int32)
    cols = dict(wp=wp, pr=pr, pd=pd, usable=us, keys=np.arange(n, dtype=np.int32), level=level,
                center=np.ascontiguousarray(np.stack([320 >> level, 240 >> level], axis=1).astype(np.int32)), fixed=np.zeros(n, dtype=np.uint8))
    targets = [(w["B"], w["cam"], w["sc"]["poseB"])]
    t = _table(w, cols)
    got = t.refind(targets, _all_rows(n), False, _finder())
    ref = compose(cols, w["A"], targets, _all_rows(n), False, _finder())
    print("counts", list(got[2]))
    _assert_equal(got, ref)
    assert int(got[2].sum()) == n and got[2][1] > 0 and got[2][2] > 0 and got[2][4] > 0      # (not hollow: pairs that leave at the projection, searched ones, found ones)


@pytest.mark.timeout(900)
def test_sixty_four_rows_eight_hundred_keyframes(world):
    from mcptam_amd.keyframe import KeyFrame
    w = world
    B2 = KeyFrame(640, 480)
    B2.MakeKeyFrame_Lite(np.ascontiguousarray(np.roll(w["sc"]["imgB"], 2, axis=1)))
    rng = np.random.default_rng(21)
    targets = [((w["B"], B2)[k % 2], w["cam"], moved(w["sc"]["poseB"], rng.normal(size=3) * 0.004, rng.normal(size=3) * 0.01)) for k in range(800)]
    rows = np.arange(0, N_BASE, N_BASE // 64)[:64]
    pairs = np.stack([np.repeat(rows, 800), np.tile(np.arange(800), 64)], axis=1).astype(np.int32)
    t = _table(w)
    got = t.refind(targets, pairs, True, _finder())
    ref = compose(w["cols"], w["A"], targets, pairs, True, _finder())
    print("counts", list(got[2]))
    _assert_equal(got, ref)
    assert int(got[2].sum()) == len(pairs) and got[2][1] > 0 and got[2][4] > 0


def test_table_rules(world):
    from mcptam_amd.keyframe import KeyFrame
    from mcptam_amd.refind import FOUND, NO_SOURCE
    w = world
    cols = w["cols"]
    n = w["n"]
    targets = [(w["B"], w["cam"], w["sc"]["poseB"])]
    pairs = _all_rows(n)
    base = _table(w).refind(targets, pairs, False, None)
    # usable = 0 rows are searched
    unusable = dict(cols, usable=np.zeros(n, dtype=np.uint8))
    got = _table(w, unusable).refind(targets, pairs, False, None)
    assert np.array_equal(got[0], base[0]) and same_meas(got[1], base[1]) and got[2][FOUND] == EXPECTED[1]
    # rows without a source and rows whose source was destroyed: NO_SOURCE, counted, never searched
    gone = KeyFrame(640, 480)
    gone.MakeKeyFrame_Lite(w["sc"]["imgA"])
    src = [gone if r % 4 == 1 else (None if r % 8 == 3 else w["A"]) for r in range(n)]
    t = _table(w, src=src)
    gone.close()
    dead = np.array([(r % 4 == 1) or (r % 8 == 3) for r in range(n)])
    v, m, counts, _ = t.refind(targets, pairs, False, None)
    assert (v[dead] == NO_SOURCE).all() and (v[~dead] == base[0][~dead]).all()
    assert counts[NO_SOURCE] == int(dead.sum()) and int(counts.sum()) == n
    keep = base[1][~dead[base[1]["pair"]]]
    assert same_meas(m, keep)
    # the tracker's finders of the table are neither read nor written; a TrackMap after a re-find equals one without it
    prm = dict(try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=10, coarse_subpix_its=8, max_patches=400, estimator="Tukey", seed=3)
    ident = [(np.eye(3), np.zeros(3))]
    ta, tb = _table(w), _table(w)
    for tt in (ta, tb):
        tt.track_map([w["B"]], [w["cam"]], w["sc"]["poseB"], ident, **prm)
    before = [ta.get_states(c).tobytes() for c in range(8)]               # (cameras no TrackMap has used read as zeroed finders)
    assert before[0].strip(b"\0")
    ta.refind(targets, pairs, False, _finder())
    ta.refind(newly_made_targets(w["sc"], w["B"]), np.stack([np.repeat(np.arange(200), 4), np.tile(np.arange(4), 200)], axis=1), True, _finder())
    assert [ta.get_states(c).tobytes() for c in range(8)] == before
    ia, pa, ra = ta.track_map([w["B"]], [w["cam"]], w["sc"]["poseB"], ident, **prm)
    ib, pb, rb = tb.track_map([w["B"]], [w["cam"]], w["sc"]["poseB"], ident, **prm)
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]) and np.array_equal(ia[0]["point"], ib[0]["point"])
    for fld in ia[0]["out"].dtype.names:
        assert np.array_equal(ia[0]["out"][fld], ib[0]["out"][fld], equal_nan=True), fld
    assert ta.get_states(0).tobytes() == tb.get_states(0).tobytes()


def test_ordered_after_uploads_and_the_write_back(world):
    from mcptam_amd import chain_bundle, synth
    w = world
    cols = w["cols"]
    targets = [(w["B"], w["cam"], w["sc"]["poseB"])]
    pairs = _all_rows(N_BASE)
    t = _table(w)
    first = t.refind(targets, pairs, False, None)
    # an update enqueued just before the call is seen
    ids = np.arange(10, 400, 3).astype(np.int32)
    c2 = dict(cols, wp=cols["wp"].copy(), pr=cols["pr"].copy(), pd=cols["pd"].copy())
    c2["wp"][ids] += np.array([0.004, -0.003, 0.002])
    c2["pr"][ids] *= 1.02
    t.update(ids, c2["wp"][ids], c2["pr"][ids], c2["pd"][ids], cols["usable"][ids])
    got = t.refind(targets, pairs, False, _finder())
    _assert_equal(got, compose(c2, w["A"], targets, pairs, False, _finder()))
    assert not same_meas(got[1], first[1])
    # after mcp_ba_write_back: the rows as mcp_map_points_get reads them back
    p = synth.make_config("tiny")
    b = chain_bundle.ChainBundle(p.cams, True, True, False)
    bid = p.populate(b)
    assert b.Compute(3) > 0
    k = min(p.n_points, 200)
    rows = np.arange(5, 5 + 2 * k, 2).astype(np.int32)
    rng = np.random.default_rng(4)
    ce = np.stack([rng.uniform(-0.5, 0.5, k), rng.uniform(-0.4, 0.4, k), np.ones(k)], axis=1)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    t.update_rays(rows, unit(ce), unit(ce + np.array([0.003, 0, 0])), unit(ce + np.array([0, 0.003, 0])))
    t.write_back(b, bid["point"][:k], rows)
    got = t.refind(targets, pairs, False, _finder())
    wp, pr, pd, us = t.get(0, w["n"])
    c3 = dict(cols, wp=wp, pr=pr, pd=pd)
    assert not np.array_equal(wp[rows], c2["wp"][rows]) and np.array_equal(wp[4], c2["wp"][4])
    _assert_equal(got, compose(c3, w["A"], targets, pairs, False, _finder()))


def test_refusals_enqueue_nothing(world):
    from mcptam_amd import chain_bundle
    from mcptam_amd.refind import RefindResult, _bind, marshal_targets
    w = world
    t = _table(w)
    L = _bind(t._L)
    targets = [(w["B"], w["cam"], w["sc"]["poseB"])] * 2
    keep, tab = marshal_targets(targets)
    n = 50
    good = _all_rows(n)

    def call(pairs=good, n_pairs=n, n_targets=2, tab=tab, cap=n, table=t._h):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        v = np.full(n, 99, dtype=np.uint8)
        m = np.full(n * 10, -7, dtype=np.int32)
        res = RefindResult()
        f = _finder()
        rc = L.mcp_map_refind(table, n_targets, ctypes.cast(tab, ctypes.c_void_p), n_pairs, pairs.ctypes.data, 0, f.ctypes.data, v.ctypes.data, cap,
                              m.ctypes.data, ctypes.byref(res))
        return rc, v, m, res, f
    bad_row, bad_row2, bad_tgt, bad_tgt2 = good.copy(), good.copy(), good.copy(), good.copy()
    bad_row[7, 0] = w["n"]; bad_row2[0, 0] = -1; bad_tgt[49, 1] = 2; bad_tgt2[3, 1] = -1
    _, tab_nokf = marshal_targets(targets); tab_nokf[1].kf = None
    _, tab_nocam = marshal_targets(targets); tab_nocam[0].cam = None
    for kw in (dict(pairs=bad_row), dict(pairs=bad_row2), dict(pairs=bad_tgt), dict(pairs=bad_tgt2), dict(tab=tab_nokf), dict(tab=tab_nocam),
               dict(n_pairs=-1), dict(n_targets=-1), dict(cap=-1), dict(table=None)):
        rc, v, m, res, f = call(**kw)
        assert rc == -1 and chain_bundle.last_error(), list(kw)
        assert (v == 99).all() and (m == -7).all() and not f.tobytes().strip(b"\0"), list(kw)
        cnt = ctypes.c_int(3)
        assert L.mcp_map_refind_view(t._h, ctypes.byref(cnt)) is None and cnt.value == 0
    # a cap that is too small: -1, verdicts and counts filled, no measurement written
    rc, v, m, res, _ = call()
    assert rc == 0 and res.n_meas > 3 and (m[:10] != -7).any()
    found = res.n_meas
    rc, v2, m2, res2, _ = call(cap=found - 1)
    assert rc == -1 and "cap_meas" in chain_bundle.last_error()
    assert res2.n_meas == found and list(res2.counts) == list(res.counts) and np.array_equal(v2, v) and (m2 == -7).all()
    rc, v3, m3, res3, _ = call(cap=found)
    assert rc == 0 and np.array_equal(m3, m)
    # an empty pair list is no error
    rc, v4, m4, res4, f4 = call(n_pairs=0)
    assert rc == 0 and res4.n_meas == 0 and sum(res4.counts) == 0 and (v4 == 99).all() and (m4 == -7).all()
    del keep


def test_two_calls_give_the_same_bytes(world):
    w = world
    targets = newly_made_targets(w["sc"], w["B"])
    pairs = np.stack([np.repeat(np.arange(300, 700), 4), np.tile(np.arange(4), 400)], axis=1).astype(np.int32)
    t = _table(w)
    runs = []
    for _ in range(2):
        f = _finder()
        v, m, c, _ = t.refind(targets, pairs, True, f, view=True)
        runs.append((v.tobytes(), m.tobytes(), c.tobytes(), f.tobytes()))
    assert runs[0] == runs[1]
    other = _table(w).refind(targets, pairs, True, _finder())
    assert other[0].tobytes() == runs[0][0] and other[1].tobytes() == runs[0][1]
