"""The AddStereoMapPoints kernels (mcptam_amd/csrc/stereo_kernels.h) at their thinning, limit and pose seams: the cases of
tests/stereo_seam_cases.py (whose layout tests/test_stereo_seams_cpu.py proves on the reference alone) through mcp_stereo_points and
mcp_stereo_hypotheses.

1. k_stereo_thin_meas alone (no targets): keep == stereo.thin_candidates, bit for bit.
2. k_stereo_thin_new / k_stereo_commit: mcp_stereo_points == stereo.compose(keyframe.patch_sequences, ...) on the same list (bits; world_pos to
   1e-9) and the whole outcome table == the nLimit loop over the outcomes every position has alone.
3. the same under a moved world and with a second target camera.
4. the arc against its np.longdouble restatement.  The step count is exact; the vectors agree, per hypothesis and relative to its largest
   component, within 8 x the deviation stereo.arc (float64) has from the longdouble arc on that case, at least 1e-12.  Measured floors
   (level 0 / level 3): clamp_on_tight 3.5e-15 / 5.3e-15, clamp_off_tight 2.6e-15 / 5.7e-15, clamp_on 5.9e-14 / 5.7e-15, clamp_off 4.2e-14 /
   6.4e-15, min_t_neg 4.6e-14 / 5.8e-15, max_t_neg 1.5e-13 / 8.8e-14, one_step 2.9e-15 / 3.5e-15, guard_above 6.8e-12 / 6.8e-12 (the two end
   points are 1.1e-4 apart: rd, the direction between them, and with it alpha lose four digits), skew_src 1.9e-13 / 2.0e-14, moved_world
   below 2e-13; guard_below, through_* and same_centre have no hypotheses.  Only max_t_neg at level 0 (1.2e-12), guard_above (5.4e-11) and
   skew_src at level 0 (1.5e-12) have a bound above 1e-12.
   The dot3(d, d) < 1e-8 guard is reached from both sides (guard_below / guard_above: a 1 cm baseline, where the clamped start 0.2 and the end
   nearly coincide).  A ray through the target's centre is pinned where it is exact (the camera's axis, no rotation, integer translations): the
   arc's end is the target's centre itself, both end points normalise 0 or +-1 ulp, and every way that can round ends in n = 0.  Oblique rays
   through the centre are not pinned on the device: there the unit vectors of two rounding residues decide, legitimately differently, between
   evaluations (tests/test_stereo_seams_cpu.py shows only that stereo.arc stays total there)."""
import functools

import numpy as np
import pytest

import stereo_seam_cases as C

pytestmark = pytest.mark.gpu
L2 = C.SEAM_LEVEL


@pytest.fixture(scope="module")
def fr():
    from mcptam_amd import keyframe as K, stereo as S
    from mcptam_amd.keyframe import KeyFrame
    sc = C.scene()
    src = KeyFrame(C.W, C.H)
    src.MakeKeyFrame_Lite(sc["img_src"]); src.MakeKeyFrame_Rest()
    tg = []
    for im in sc["imgs"] + [sc["img_skew"]]:
        g = KeyFrame(C.W, C.H)
        g.MakeKeyFrame_Lite(im)
        tg.append(g)
    base, _ = src.Candidates(L2)
    out = dict(sc=sc, src=src, tg=tg[:4], skew=tg[4], base=base)

    @functools.lru_cache(maxsize=None)
    def codes_key(key):
        """outcomes of positions alone against targets 0..3, from the composition's pieces (stereo_hypotheses, patch_sequences, select_matches)"""
        cand = np.array(key, dtype=np.int32).reshape(-1, 2)
        tab = np.zeros((4, len(cand)), dtype=np.uint8)
        for j in range(4):
            t = (tg[j], sc["cam"], sc["poses"][j])
            hyp, off = S.stereo_hypotheses(src, sc["cam"], sc["pose_src"], L2, cand, t)
            res = S.compose_target(K.patch_sequences, tg[j], sc["cam"], sc["poses"][j], hyp, off, list(range(len(cand))), src)
            tab[j] = [res[i][0] for i in range(len(cand))]
        return tab
    out["codes_at"] = lambda p: codes_key(tuple(map(tuple, np.asarray(p).reshape(-1, 2).tolist())))
    out["codes"] = out["codes_at"](base)
    out["cases"] = {c["name"]: c for c in C.commit_cases(base, out["codes"], out["codes_at"])}
    return out


# ---- 1. thinning alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["radius", "rounding", "wide", "level", "size"])
def test_thinning_alone_equals_thin_candidates(gpu_required, fr, family):
    from mcptam_amd import stereo as S
    sc = fr["sc"]
    cases = getattr(C, "thin_%s_cases" % family)()
    assert cases
    for case in cases:
        meas = S.make_meas(case["meas_root"], case["meas_level"])
        got, keep, _ = S.stereo_points(fr["src"], sc["cam"], sc["pose_src"], case["level"], case["cand"], [], meas=meas)
        assert len(got) == 0
        assert np.array_equal(keep, C.thin_expected(case)), (case["name"], np.nonzero(keep != C.thin_expected(case))[0])


# ---- 2. thin_new and commit ----------------------------------------------------------------------------------------------------------------------
def _run(fr, case, sc=None, targets=None, level=L2):
    """mcp_stereo_points on a case against stereo.compose on the same list and the nLimit loop's outcome table"""
    import test_stereo_points_gpu as T
    from mcptam_amd import keyframe as K, stereo as S
    sc = fr["sc"] if sc is None else sc
    tg = [(fr["tg"][j], sc["cam"], sc["poses"][j]) for j in case["targets"]] if targets is None else targets
    meas = S.make_meas(case["meas_root"], case["meas_level"])
    got, keep, oc = S.stereo_points(fr["src"], sc["cam"], sc["pose_src"], level, case["cand"], tg, limit=case["limit"], meas=meas)
    made, keep_ref = S.compose(K.patch_sequences, fr["src"], sc["cam"], sc["pose_src"], level, case["cand"], tg, limit=case["limit"],
                               meas_root=case["meas_root"], meas_level=case["meas_level"])
    T._compare(got, keep, made, keep_ref)
    return got, keep, oc, made


def _run_commit(fr, name):
    from mcptam_amd import stereo as S
    case = fr["cases"][name]
    got, keep, oc, made = _run(fr, case)
    per, outcome, keep_model = C.check_commit_layout(case, C.case_codes(case, fr["base"], fr["codes"], fr["codes_at"]))
    assert [(m["candidate"], m["target"]) for m in made] == [(int(i), j) for j, p in enumerate(per) for i in np.nonzero(p["made"])[0]], name
    assert np.array_equal(oc, outcome), (name, np.argwhere(oc != outcome)[:8])
    assert np.array_equal(keep, keep_model)
    for j, p in enumerate(per):
        assert np.array_equal(oc[j] == S.PAST_LIMIT, p["alive"] & ~p["tried"]) and np.array_equal(oc[j] == S.THINNED, ~p["alive"])
        assert (got["target"] == j).sum() == p["made"].sum()
    return case, got, oc, per


@pytest.mark.parametrize("n", C.COMMIT_SIZES)
def test_limits_around_the_chunk_seam(gpu_required, fr, n):
    from mcptam_amd import stereo as S
    for kind in ("c0-1", "c0", "c0+1", "total", "total+1", "one", "zero", "minus3"):
        case, got, oc, per = _run_commit(fr, "n%d_%s" % (n, kind))
        if kind == "total+1":
            assert len(got) == case["total"] and not (oc == S.PAST_LIMIT).any()
        if kind == "c0" and n > C.COMMIT_NT:
            assert (oc[0][C.COMMIT_NT:] == S.PAST_LIMIT).all() and oc[0][C.COMMIT_NT - 1] == S.CREATED
        if kind == "c0+1" and n > C.COMMIT_NT:
            assert oc[0][C.COMMIT_NT] == S.CREATED and (oc[0][C.COMMIT_NT + 1:] == S.PAST_LIMIT).all()
        if kind in ("zero", "minus3"):
            assert all((oc[j] != S.THINNED).sum() == 1 + (oc[j] == S.PAST_LIMIT).sum() for j in range(len(oc)))


@pytest.mark.parametrize("name", ["survivor_creates_2t", "survivor_creates_3t", "survivor_fails_2t", "survivor_fails_3t"])
def test_first_survivor_in_the_second_chunk(gpu_required, fr, name):
    from mcptam_amd import stereo as S
    case, got, oc, per = _run_commit(fr, name)
    assert (oc[:, :C.COMMIT_NT] == S.THINNED).all()
    assert (oc[1][C.COMMIT_NT] == S.CREATED) == case["creates"] and oc[1][C.COMMIT_NT] != S.PAST_LIMIT
    assert ((got["target"] == 1).sum() == 1) == case["creates"]
    live = oc[1] != S.THINNED
    assert (oc[1][live][1:] == S.PAST_LIMIT).all() and live.sum() > 10


@pytest.mark.parametrize("name", ["dead_from_start", "dead_after_0"])
def test_dead_targets(gpu_required, fr, name):
    from mcptam_amd import stereo as S
    case, got, oc, per = _run_commit(fr, name)
    for j in range(case["dead_from"], len(case["targets"])):
        assert (oc[j] == S.THINNED).all() and (got["target"] == j).sum() == 0
    if name == "dead_after_0":
        # every copy created, in candidate order across the chunk seam; targets 1 and 2 are both dead and the call still ends with the same count
        assert len(got) == case["n"] and list(got["candidate"]) == list(range(case["n"])) and len(case["targets"]) == 3


def test_created_points_thin_their_neighbours_below_ten_pixels(gpu_required, fr):
    from mcptam_amd import stereo as S
    case, got, oc, per = _run_commit(fr, "neighbours")
    e = case["first_extra"]
    assert list(oc[1][e:] == S.THINNED) == [True, True, False, False] and (oc[0][e:] != S.THINNED).all()


# ---- 3. a moved world, a second camera -----------------------------------------------------------------------------------------------------------
def _plane_share(world, depth):
    return float((np.abs(world[:, 2] - depth) < 0.02 * depth).mean())


def test_moved_world(gpu_required, fr):
    import test_stereo_points_gpu as T
    from mcptam_amd import stereo as S
    sc = fr["sc"]
    mv = dict(cam=sc["cam"], pose_src=sc["pose_src_moved"], poses=sc["poses_moved"], src=fr["src"])
    case = dict(cand=fr["base"], targets=(0, 1, 2), limit=1 << 30, meas_root=np.zeros((0, 2)), meas_level=np.zeros(0, dtype=np.int32))
    got, keep, oc, made = _run(fr, case, sc=mv)
    assert len(got) > 50 and set(got["target"]) >= {0, 1}
    T._check_point_vectors(got, mv, L2)
    # G times the points of the fixture's own world (the last bits of the poses differ, so a borderline candidate may fall the other way)
    ref, _, _ = S.stereo_points(fr["src"], sc["cam"], sc["pose_src"], L2, fr["base"], [(fr["tg"][j], sc["cam"], sc["poses"][j]) for j in (0, 1, 2)])
    old = {(int(r["candidate"]), int(r["target"])): r["world_pos"] for r in ref}
    both = [g for g in got if (int(g["candidate"]), int(g["target"])) in old]
    assert len(both) >= 0.9 * max(len(got), len(ref))
    dev = np.array([np.abs(C.unmove_points(g["world_pos"])[0] - old[(int(g["candidate"]), int(g["target"]))]).max() for g in both])
    assert (dev < 1e-6).mean() >= 0.9, np.sort(dev)[-5:]
    # created points lie on the moved plane: level 1, as test_outcomes_mask_and_usefulness has it
    cand1, _ = fr["src"].Candidates(1)
    got1, _, _ = S.stereo_points(fr["src"], sc["cam"], mv["pose_src"], 1, cand1, [(fr["tg"][j], sc["cam"], mv["poses"][j]) for j in range(4)],
                                 limit=max(4, len(cand1) // 3))
    share = _plane_share(C.unmove_points(got1["world_pos"]), sc["depth"])
    print("moved world: level 1 created %d, on the plane %.3f" % (len(got1), share))
    assert len(got1) > 100 and share >= 0.9


def test_second_target_camera(gpu_required, fr):
    from mcptam_amd import keyframe as K, stereo as S
    from oracle import oracle_patch_sequences
    sc = fr["sc"]
    of = C.oracle_frames()
    skew = (fr["skew"], sc["cam_skew"], sc["poses"][0])
    case = dict(cand=fr["base"], targets=None, limit=1 << 30, meas_root=np.zeros((0, 2)), meas_level=np.zeros(0, dtype=np.int32))
    got, keep, oc, made = _run(fr, case, targets=[skew, (fr["tg"][1], sc["cam"], sc["poses"][1])])
    assert (got["target"] == 0).sum() >= 30
    got, keep, oc, made = _run(fr, case, targets=[(fr["tg"][1], sc["cam"], sc["poses"][1]), skew])      # the second camera in the table's second row
    assert (got["target"] == 0).sum() >= 30
    one, _, _, _ = _run(fr, case, targets=[skew])
    omade, _ = S.compose(oracle_patch_sequences, fr["src"], sc["cam"], sc["pose_src"], L2, fr["base"], [skew], src_oracle=of["src"], search_kfs=[of["skew"]])
    assert [m["candidate"] for m in omade] == list(one["candidate"])
    assert np.allclose(np.array([m["target_pos"] for m in omade]), one["target_pos"], rtol=0, atol=1e-9)
    # the plane: level 1, the skew camera's target first
    cand1, _ = fr["src"].Candidates(1)
    got1, _, _ = S.stereo_points(fr["src"], sc["cam"], sc["pose_src"], 1, cand1, [skew] + [(fr["tg"][j], sc["cam"], sc["poses"][j]) for j in (1, 2, 3)],
                                 limit=max(4, len(cand1) // 3))
    first = got1[got1["target"] == 0]
    share, share0 = _plane_share(got1["world_pos"], sc["depth"]), _plane_share(first["world_pos"], sc["depth"])
    print("second camera: level 1 created %d (%d by the skew target), on the plane %.3f (%.3f)" % (len(got1), len(first), share, share0))
    assert len(got1) > 100 and len(first) > 50 and share >= 0.9 and share0 >= 0.9


# ---- 4. the arc ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", C.ARC_LEVELS)
def test_arc_seams_match_the_longdouble_arc(gpu_required, fr, level):
    from mcptam_amd import stereo as S
    cases = [c for c in C.arc_cases() if c["level"] == level]
    assert len(cases) >= 14
    for case in cases:
        ref = C.arc_reference(case)
        bound = C.arc_bound(case, ref)
        hyp, off = S.stereo_hypotheses(fr["src"], case["cam"], case["pose_src"], level, case["cand"], (fr["tg"][0], case["cam"], case["pose_tgt"], case["opa"]))
        assert off[-1] == len(hyp)
        got = []
        for i, (c, r) in enumerate(zip(case["cand"], ref)):
            h = hyp[off[i]:off[i + 1]]
            assert len(h) == r["n"], (case["name"], i, len(h), r["n"])
            assert (h["center_x"] == c[0]).all() and (h["center_y"] == c[1]).all() and (h["source_level"] == level).all()
            got.append(dict(world=h["world_pos"], pixel_right_w=h["pixel_right_w"], pixel_down_w=h["pixel_down_w"]))
        dev = C.arc_deviation(ref, got)
        print("%-22s hypotheses %-28s deviation %.3g  bound %.3g" % (case["name"], [r["n"] for r in ref], dev, bound))
        assert dev <= bound, (case["name"], dev, bound)
        if case["claim"] == "no_arc" or case["claim"] == "guard_below":
            assert len(hyp) == 0
