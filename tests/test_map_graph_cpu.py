"""The bundle selection over the map graph without a device: the numpy restatement against a literal transcription of the reference's set
walks, mcp_map_bundle_select_host against the restatement, the edited maps, and the refusals of the host call."""
import ctypes

import numpy as np
import pytest

import map_graph_cases as mc
from mcptam_amd import map_graph as mg


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


PLAIN = mc.plain_cases()
EDITED = mc.edited_cases()


@pytest.mark.parametrize("name,a,S", PLAIN, ids=[c[0] for c in PLAIN])
def test_ref_against_literal_transcription(name, a, S):
    res, mkfs, points, meas = mg.bundle_select_ref(a, S)
    T = mc.transcription(a, S)
    assert res["status"] == T["status"] == 0
    na = res["n_adjust"]
    N = len(a["pt_flags"])
    # sets as sets
    assert set(mkfs["slot"][:na].tolist()) == T["adjust"]
    assert set(mkfs["slot"][na:].tolist()) == T["fixed"]
    assert set(points["row"].tolist()) == T["points"]
    assert set(meas["store"].tolist()) == T["meas"]
    assert res["n_dropped_source"] == T["dropped"]
    assert [k for k in res["closest"] if k >= 0] == T["closest"]
    # orders as specified: adjust set then fixed set in ascending slot, rows ascending, store order
    assert (np.diff(mkfs["slot"][:na]) > 0).all() and (np.diff(mkfs["slot"][na:]) > 0).all()
    assert (np.diff(points["row"]) > 0).all() and (np.diff(meas["store"]) > 0).all()
    assert res["n_fixed"] == len(mkfs) - na and res["n_points"] == len(points) and res["n_meas"] == len(meas)
    # the bundle's contents
    for k, f in zip(mkfs["slot"].tolist(), mkfs["fixed"].tolist()):
        assert bool(f) == T["fixed_in_bundle"][k]
    for q in points:
        r = int(q["row"])
        src = T["pt_src"][r]
        if src is None:
            assert q["fixed"] == 1 and q["src_mkf"] == -1
        else:
            assert q["fixed"] == 0 and (int(mkfs["slot"][q["src_mkf"]]), int(q["src_cam"])) == src
    # x: the transcription multiplies with numpy's matmul, the restatement writes the sums out: the bound of test 2 covers each side
    want = np.array([T["x"][int(r)] for r in points["row"]]).reshape(-1, 3)
    assert (np.abs(points["x"] - want) <= 2 * mc.x_bound(a, points) + 1e-300).all()
    # every measurement names its MKF, camera and point
    assert np.array_equal(mkfs["slot"][meas["mkf"]], a["ms_mkf"][meas["store"]])
    assert np.array_equal(points["row"][meas["point"]], a["ms_row"][meas["store"]])
    assert np.array_equal(meas["cam"], a["ms_cam"][meas["store"]])
    if S.mode == mg.BUNDLE_RECENT:
        assert 0 < res["n_points"] < N and res["n_fixed"] > 0, res


def test_band_selection_crosses_seams():
    """The band map's RECENT bundle is neither everything nor nothing and its measurement list crosses several 256 seams."""
    a = mc.arrays("band40")
    res = mg.bundle_select_ref(a, mc.recent(a))[0]
    assert 0 < res["n_adjust"] + res["n_fixed"] < 40 and 256 < res["n_points"] < 1500 and 3 * 256 < res["n_meas"] < 6000, res


# x = R w + t per component is three products, two adds and one add, each rounded once: the computed value is within gamma_4 (|R||w| + |t|)_i,
# gamma_4 = 4u / (1 - 4u), u = 2^-53, of the exact value for the R, t in hand.  R, t themselves are a two-step product (CamFromBase *
# BaseFromWorld) bounded the same way; the host library and the restatement form every sum in the same left-to-right order without
# contraction, so in practice they agree to the bit and the bound 4u (|R||w| + |t|) is what the issue sets for the comparison.
@pytest.mark.parametrize("name,a,S", PLAIN, ids=[c[0] for c in PLAIN])
def test_host_against_ref(name, a, S):
    mc.assert_same_selection(mg.bundle_select_host(a, S), mg.bundle_select_ref(a, S), a, exact=False)


@pytest.mark.parametrize("name,a,S,exp", EDITED, ids=[c[0] for c in EDITED])
def test_edited_maps(name, a, S, exp):
    ref = mg.bundle_select_ref(a, S)
    mc.check_expectation(exp, ref, a)
    host = mg.bundle_select_host(a, S)
    mc.check_expectation(exp, host, a)
    mc.assert_same_selection(host, ref, a, exact=False)
    T = mc.transcription(a, S)
    assert T["status"] == ref[0]["status"]
    if T["status"] == 0:
        na = ref[0]["n_adjust"]
        assert set(ref[1]["slot"][:na].tolist()) == T["adjust"] and set(ref[1]["slot"][na:].tolist()) == T["fixed"]
        assert set(ref[2]["row"].tolist()) == T["points"] and set(ref[3]["store"].tolist()) == T["meas"]
        assert ref[0]["n_dropped_source"] == T["dropped"]


def _host_raw(a, S, res, mk, pt, ms, ncam=None, params_ptr=None, res_ptr=None):
    P, N, M, C = len(a["mkf_flags"]), len(a["pt_flags"]), len(a["ms_mkf"]), int(a["ncam"])
    keep = [np.ascontiguousarray(a[k]) for k in ("cam_from_base", "base_from_world", "mkf_flags", "kf_active", "kf_depth_mean", "world_pos", "src_mkf", "src_cam",
                                                 "pt_flags", "ms_mkf", "ms_cam", "ms_row", "ms_uv", "ms_level", "ms_source", "ms_alive")]
    p = [v.ctypes.data for v in keep]
    return mg.lib().mcp_map_bundle_select_host(ctypes.addressof(S) if params_ptr is None else params_ptr, C if ncam is None else ncam, p[0], P, p[1], p[2], p[3], p[4],
                                               N, p[5], p[6], p[7], p[8], M, p[9], p[10], p[11], p[12], p[13], p[14], p[15],
                                               ctypes.addressof(res) if res_ptr is None else res_ptr, len(mk), mk.ctypes.data, len(pt), pt.ctypes.data, len(ms), ms.ctypes.data)


def test_host_refusals_leave_outputs_untouched():
    from mcptam_amd import chain_bundle
    a = mc.arrays("tiny12")
    P, N, M = 12, 300, len(a["ms_mkf"])
    bad = [("mode", mg.select_params(7, 11)), ("newest absent", mc.recent(a, newest=500)), ("newest negative", mc.recent(a, newest=-1)),
           ("n_recent", mc.recent(a, n_recent=9)), ("n_recent negative", mc.recent(a, n_recent=-1)), ("gate", mc.recent(a, min_points=-1)),
           ("gate 2", mc.recent(a, recent_min_size=-1)), ("fraction", mc.recent(a, mean_diff_fraction=float("nan"))),
           ("fraction inf", mg.select_params(mg.BUNDLE_ALL, mean_diff_fraction=float("inf")))]
    a2 = mc.arrays("tiny12"); a2["mkf_flags"][11] = 0
    for what, S in bad + [("newest not present", None)]:
        arr = a
        if S is None:
            arr, S = a2, mc.recent(a2, newest=11)
        res = mg.SelectResult(); ctypes.memset(ctypes.addressof(res), 0x5a, ctypes.sizeof(res))
        mk, pt, ms = np.full(P, 7, dtype=mg.MKF_DTYPE), np.full(N, 7, dtype=mg.POINT_DTYPE), np.full(M, 7, dtype=mg.MEAS_DTYPE)
        before = (bytes(res), mk.tobytes(), pt.tobytes(), ms.tobytes())
        assert _host_raw(arr, S, res, mk, pt, ms) == -1, what
        assert chain_bundle.last_error(), what
        assert (bytes(res), mk.tobytes(), pt.tobytes(), ms.tobytes()) == before, what
    # NULL structs, a bad camera count, views that do not fit
    S = mc.recent(a)
    res = mg.SelectResult()
    mk, pt, ms = np.full(P, 7, dtype=mg.MKF_DTYPE), np.full(N, 7, dtype=mg.POINT_DTYPE), np.full(M, 7, dtype=mg.MEAS_DTYPE)
    before = (mk.tobytes(), pt.tobytes(), ms.tobytes())
    assert _host_raw(a, S, res, mk, pt, ms, params_ptr=0) == -1
    assert _host_raw(a, S, res, mk, pt, ms, res_ptr=0) == -1
    assert _host_raw(a, S, res, mk, pt, ms, ncam=0) == -1
    assert _host_raw(a, S, res, mk, pt, ms[:3]) == -1 and "fit" in chain_bundle.last_error()
    assert (mk.tobytes(), pt.tobytes(), ms.tobytes()) == before
    assert _host_raw(a, S, res, mk, pt, ms) == 0 and res.status == 0
