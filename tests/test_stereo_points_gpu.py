"""mcp_stereo_points (MapMakerServerBase::AddStereoMapPoints of one source keyframe and level in one submission) against the composition of
existing calls -- mcp_stereo_hypotheses, mcp_patch_sequences(EPI_COARSE / EPI_REFINE), numpy selection / thinning / triangulation -- and the oracle."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stereo():
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame
    from oracle import OracleKeyFrame
    sc = synth_img.make_stereo_scene()
    src, osrc = KeyFrame(640, 480), OracleKeyFrame(640, 480)
    src.MakeKeyFrame_Lite(sc["img_src"]); osrc.MakeKeyFrame_Lite(sc["img_src"])
    src.MakeKeyFrame_Rest(); osrc.MakeKeyFrame_Rest()
    tg, otg = [], []
    for im in sc["imgs"]:
        g, o = KeyFrame(640, 480), OracleKeyFrame(640, 480)
        g.MakeKeyFrame_Lite(im); o.MakeKeyFrame_Lite(im)
        tg.append(g); otg.append(o)
    sc.update(src=src, osrc=osrc, tg=tg, otg=otg)
    return sc


def _targets(sc, js, kfs=None):
    kfs = sc["tg"] if kfs is None else kfs
    return [(kfs[j], sc["cam"], sc["poses"][j]) for j in js]


def _cand(sc, level, n=None):
    c, _ = sc["src"].Candidates(level)
    return c if n is None else c[:n]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300) if a.size else 0.0


def test_arc_matches_numpy(gpu_required, stereo):
    """1: the device's hypotheses (mcp_stereo_hypotheses) have numpy's step count, positions and pixel vectors to 1e-12 relative"""
    from mcptam_amd import stereo as S
    sc = stereo
    opa = sc["cam"].one_pixel_angle()
    for level in (0, 1, 2, 3):
        cand = _cand(sc, level, 40)
        for j in (0, 2):
            hyp, off = S.stereo_hypotheses(sc["src"], sc["cam"], sc["pose_src"], level, cand, _targets(sc, [j])[0])
            assert off[-1] == len(hyp) and len(hyp) > 0
            for i, c in enumerate(cand):
                a = S.arc(sc["cam"], sc["pose_src"], sc["poses"][j], opa, level, c)
                h = hyp[off[i]:off[i + 1]]
                assert len(h) == a["n"], (level, j, i)
                if a["n"] == 0:
                    continue
                assert _rel(h["world_pos"], a["world"]) < 1e-12
                assert _rel(h["pixel_right_w"], a["pixel_right_w"]) < 1e-12
                assert _rel(h["pixel_down_w"], a["pixel_down_w"]) < 1e-12
                assert (h["center_x"] == c[0]).all() and (h["source_level"] == level).all()


def _check_point_vectors(got, sc, level):
    from mcptam_amd import stereo as S
    cand = _cand(sc, level)
    for g in got:
        root, cen, rig, dow = S.probe(sc["cam"], level, cand[g["candidate"]])
        assert np.array_equal(g["root_pos"], root)
        for k, v in (("center_nc", cen), ("one_right_nc", rig), ("one_down_nc", dow)):
            assert _rel(g[k], v) < 1e-12
        pr, pd = S.pixel_vectors(sc["pose_src"], g["center_nc"], g["one_right_nc"], g["one_down_nc"], g["world_pos"])
        assert _rel(g["pixel_right_w"], pr[0]) < 1e-12 and _rel(g["pixel_down_w"], pd[0]) < 1e-12


def _compare(got, keep, made, keep_ref):
    assert np.array_equal(keep, keep_ref)
    assert len(got) == len(made), (len(got), len(made))
    for k in ("candidate", "target", "hypothesis", "score"):
        assert np.array_equal(got[k], np.array([m[k] for m in made], dtype=np.int32)), k
    assert np.array_equal(got["target_pos"], np.array([m["target_pos"] for m in made]).reshape(-1, 2))
    assert np.array_equal(got["root_pos"], np.array([m["root_pos"] for m in made]).reshape(-1, 2))
    for g, m in zip(got, made):
        assert _rel(g["world_pos"], m["world_pos"]) < 1e-9


def test_one_target_equals_composition_and_oracle(gpu_required, stereo):
    """2 + 3: one target, bit for bit against the composition of existing calls; the oracle's PatchFinder gives the same created set"""
    from mcptam_amd import keyframe as K, stereo as S
    from oracle import oracle_patch_sequences
    sc = stereo
    for level in (1, 2):
        cand = _cand(sc, level)
        tg = _targets(sc, [0])
        got, keep, oc = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, cand, tg)
        made, keep_ref = S.compose(K.patch_sequences, sc["src"], sc["cam"], sc["pose_src"], level, cand, tg)
        _compare(got, keep, made, keep_ref)
        _check_point_vectors(got, sc, level)
        assert len(got) >= 10 and (oc[0] == S.CREATED).sum() == len(got)
        omade, _ = S.compose(oracle_patch_sequences, sc["src"], sc["cam"], sc["pose_src"], level, cand, tg, src_oracle=sc["osrc"],
                             search_kfs=[sc["otg"][0]])
        assert [m["candidate"] for m in omade] == list(got["candidate"])
        assert np.allclose(np.array([m["target_pos"] for m in omade]), got["target_pos"], rtol=0, atol=1e-9)


def test_three_targets_thinning_and_keep(gpu_required, stereo):
    """4: three ordered targets = three single-target compositions with numpy thinning between them; measurements at L / L+1 thin, L-1 / L+2 do
    not; keep is the candidate list before the last target"""
    from mcptam_amd import keyframe as K, stereo as S
    sc = stereo
    level = 1
    cand = _cand(sc, level)
    # measurements at every level on top of candidates 0, 5, 10, ... (root positions of a level-1 candidate)
    pick = np.arange(0, len(cand), 5)
    roots = S.level_zero_pos(cand[pick], level)
    lv = np.array([0, 1, 2, 3])[pick % 4]
    meas = S.make_meas(roots, lv)
    tg = _targets(sc, [0, 1, 2])
    got, keep, oc = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, cand, tg, meas=meas)
    made, keep_ref = S.compose(K.patch_sequences, sc["src"], sc["cam"], sc["pose_src"], level, cand, tg, meas_root=roots, meas_level=lv)
    _compare(got, keep, made, keep_ref)
    thin0 = S.thin_candidates(cand, level, roots, lv)
    assert not thin0[pick[(lv == 1) | (lv == 2)]].any()
    assert (oc[0][~thin0] == S.THINNED).all() and (oc[0][thin0] != S.THINNED).all()
    only_far = S.thin_candidates(cand, level, roots[(lv == 0) | (lv == 3)], lv[(lv == 0) | (lv == 3)])
    assert only_far.all()
    assert set(got["target"]) >= {0, 1}
    # the points target 0 created thin the candidates of target 1
    assert (oc[1][got["candidate"][got["target"] == 0]] == S.THINNED).all()
    assert np.array_equal(keep, oc[2] != S.THINNED)


def test_limit_quirk(gpu_required, stereo):
    """5: nLimit counts over targets and only leaves the candidate loop"""
    from mcptam_amd import keyframe as K, stereo as S
    sc = stereo
    level = 1
    cand = _cand(sc, level)
    tg = _targets(sc, [0, 1, 2])
    for k in (1, 5):
        got, keep, oc = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, cand, tg, limit=k)
        made, keep_ref = S.compose(K.patch_sequences, sc["src"], sc["cam"], sc["pose_src"], level, cand, tg, limit=k)
        _compare(got, keep, made, keep_ref)
        assert (got["target"] == 0).sum() == k
        for j in (1, 2):
            sel = got["target"] == j
            assert sel.sum() <= 1
            live = np.nonzero(oc[j] != S.THINNED)[0]
            if sel.any():
                assert got["candidate"][sel][0] == live[0]
            assert (oc[j][live[1:]] == S.PAST_LIMIT).all()
        assert (oc == S.PAST_LIMIT).any()


def test_outcomes_mask_and_usefulness(gpu_required, stereo):
    """6 + 7: every outcome code on the fixture; a level-0 mask of the target gates hypotheses; created points lie on the plane"""
    from mcptam_amd import keyframe as K, stereo as S
    from mcptam_amd.keyframe import KeyFrame
    sc = stereo
    seen, good, per_level = set(), [], {}
    for level in (0, 1, 2, 3):
        cand = _cand(sc, level)
        pick = np.arange(0, len(cand), 7)
        meas = S.make_meas(S.level_zero_pos(cand[pick], level), np.full(len(pick), level))
        got, keep, oc = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], level, cand, _targets(sc, [0, 1, 2, 3]), limit=max(4, len(cand) // 3),
                                        meas=meas)
        seen |= set(np.unique(oc).tolist())
        ok = np.abs(got["world_pos"][:, 2] - sc["depth"]) < 0.02 * sc["depth"]      # the source is the world frame, the plane is z = depth
        good.append(ok); per_level[level] = (len(got), float(ok.mean()) if len(got) else None)
    # level 1 (the level AddMultiKeyFrameAndCreatePoints reaches first with most candidates here): >= 90 % on the plane.  The other levels are
    # recorded in DESIGN.md 5; they are what the reference's PatchFinder makes of this fixture (the walk equals it bit for bit, tests above).
    assert per_level[1][0] > 100 and per_level[1][1] >= 0.9, per_level
    assert np.concatenate(good).mean() >= 0.8, per_level
    # a target at the source's own position: no baseline, a non-finite arc, no hypotheses
    cand = _cand(sc, 2)
    got, keep, oc = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], 2, cand, [(sc["tg"][0], sc["cam"], sc["pose_src"])])
    assert (oc[0][keep] == S.NO_ARC).all() and len(got) == 0
    assert S.arc(sc["cam"], sc["pose_src"], sc["pose_src"], sc["cam"].one_pixel_angle(), 2, cand[0])["n"] == 0
    seen |= set(np.unique(oc).tolist())
    missing = set(range(1, 9)) - seen
    assert not missing, [S.OUTCOME_NAMES[m] for m in missing]
    # a mask over the right half of the target's level 0: no created point projects there
    mask = np.full((480, 640), 255, dtype=np.uint8); mask[:, 320:] = 0
    gm = KeyFrame(640, 480)
    gm.MakeKeyFrame_Lite(sc["imgs"][0], [mask, None, None, None])
    cand = _cand(sc, 1)
    got, _, _ = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], 1, cand, [(gm, sc["cam"], sc["poses"][0])])
    ref, _, _ = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], 1, cand, _targets(sc, [0]))
    assert len(got) > 0 and (got["target_pos"][:, 0] < 330).all() and (ref["target_pos"][:, 0] >= 330).any()
    made, _ = S.compose(K.patch_sequences, sc["src"], sc["cam"], sc["pose_src"], 1, cand, [(gm, sc["cam"], sc["poses"][0])])
    assert [m["candidate"] for m in made] == list(got["candidate"])


def test_determinism_and_scale(gpu_required):
    """8: two calls give identical bytes; 1280x960, level 0, all candidates against five targets equals the composition"""
    from mcptam_amd import keyframe as K, stereo as S, synth_img
    from mcptam_amd.keyframe import KeyFrame
    sc = synth_img.make_stereo_scene(size=(1280, 960))
    src = KeyFrame(1280, 960); src.MakeKeyFrame_Lite(sc["img_src"]); src.MakeKeyFrame_Rest()
    tg = []
    for im in sc["imgs"]:
        g = KeyFrame(1280, 960); g.MakeKeyFrame_Lite(im); tg.append(g)
    targets = [(tg[j % 4], sc["cam"], sc["poses"][j % 4]) for j in range(5)]
    cand, _ = src.Candidates(0)
    a = S.stereo_points(src, sc["cam"], sc["pose_src"], 0, cand, targets)
    b = S.stereo_points(src, sc["cam"], sc["pose_src"], 0, cand, targets)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    made, keep_ref = S.compose(K.patch_sequences, src, sc["cam"], sc["pose_src"], 0, cand, targets)
    _compare(a[0], a[1], made, keep_ref)
    assert len(a[0]) > 50


def test_refusals_enqueue_nothing(gpu_required, stereo):
    """9: every refusal happens before anything is enqueued and names itself in mcp_last_error"""
    from mcptam_amd import chain_bundle as cb, stereo as S
    from mcptam_amd.keyframe import KeyFrame
    sc = stereo
    L = S.lib()
    cand = np.ascontiguousarray(_cand(sc, 1, 30).astype(np.int32))
    n = len(cand)
    tab, cams = S._targets(_targets(sc, [0]))
    cs = sc["cam"].to_struct()
    sp = S._pose12(sc["pose_src"])
    out = np.zeros(n, dtype=S.STEREO_POINT_DTYPE); keep = np.zeros(n, dtype=np.uint8)
    meas = S.make_meas(np.zeros((0, 2)), [])

    def call(src=sc["src"]._h, level=1, nc=n, cap=n, ntar=1, tabp=None, cam=None):
        return L.mcp_stereo_points(src, ctypes.addressof(cam or cs), sp.ctypes.data, level, nc, cand.ctypes.data, 0, meas.ctypes.data, ntar,
                                   ctypes.addressof(tabp or tab), 1 << 30, cap, out.ctypes.data, keep.ctypes.data, None)
    dead = KeyFrame(640, 480); dh = dead._h; dead.close()
    bad_cam = sc["cam"].to_struct(); bad_cam.n_inv = 99
    other = S._targets([(sc["tg"][0], sc["cam"], sc["poses"][0], -1.0)])[0]
    cases = [dict(src=None), dict(src=dh), dict(level=4), dict(level=-1), dict(nc=-1), dict(ntar=-1), dict(cap=n - 1), dict(cam=bad_cam), dict(tabp=other)]
    dead_tab = S._targets([(sc["tg"][0], sc["cam"], sc["poses"][0])])[0]; dead_tab[0].kf = dh
    cases.append(dict(tabp=dead_tab))
    from mcptam_amd import keyframe as K
    for kw in cases:
        assert K.lib().mcp_kf_level_size(sc["src"]._h, 99, None, None) == -1 and "mcp_stereo" not in cb.last_error()      # another message first
        assert call(**kw) == -1, kw
        assert "mcp_stereo_points" in cb.last_error(), (kw, cb.last_error())
    assert call() >= 0
