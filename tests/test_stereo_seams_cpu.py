"""The cases of tests/stereo_seam_cases.py on the reference alone (numpy, np.longdouble, the CPU oracle): every case has the layout it is named
for, and the restatements tell the right rule from the wrong one.  Nothing here needs a GPU; tests/test_stereo_seams_gpu.py runs the same cases
on the device."""
import functools
import math
import warnings

import numpy as np

import stereo_seam_cases as C
from mcptam_amd import stereo as S


# ---- 1. thinning alone ---------------------------------------------------------------------------------------------------------------------------
def test_thin_radius_cases_hold_every_distance_and_only_below_100_thins():
    for case in C.thin_radius_cases():
        d = case["cand"].astype(np.int64) - np.array(case["busy"])
        d2 = (d * d).sum(axis=1)
        assert set(d2.tolist()) == {97, 98, 100, 101} and 99 not in d2
        for dist in C.RADIUS_OFFSETS.values():                   # every sign and axis combination is there
            for o in C.signed_offsets(*dist):
                assert (d == np.array(o)).all(axis=1).any(), (case["name"], o)
        keep = C.thin_expected(case)
        assert np.array_equal(keep, d2 >= 100) and keep.any() and (~keep).any()
        wrong = C.thin_restated(case["cand"], case["level"], case["meas_root"], case["meas_level"], le=True)
        assert np.array_equal(wrong, d2 > 100) and not np.array_equal(wrong, keep)


def test_thin_rounding_cases_hold_every_value_and_tell_the_roundings_apart():
    cases = C.thin_rounding_cases()
    assert {c["value"] for c in cases} == set(C.ROUND_VALUES) and {c["axis"] for c in cases} == {0, 1}
    assert [int(S.ir_rounded(v)) for v in C.ROUND_VALUES] == list(C.ROUND_EXPECT)
    assert 0.49999999999999994 < 0.5 and 0.49999999999999994 + 0.5 == 1.0
    caught = {m: set() for m in ("trunc", "floor_half", "plus_half", "even", "ceil")}
    for case in cases:
        sc = float(1 << case["level"])
        q = case["meas_root"][0] / sc
        assert q[case["axis"]] == case["value"] and q[1 - case["axis"]] == C.ROUND_OTHER          # the quotient is the value exactly
        keep = C.thin_expected(case)
        along = case["cand"][:, case["axis"]].astype(np.int64)
        assert np.array_equal(keep, np.abs(along - case["expect"]) >= 10)
        r = case["expect"]
        for p in (r - 1, r, r + 1):                              # 9 and 10 from the rounded position and from both neighbours
            assert {p + 9, p + 10} <= set(along.tolist())
        assert np.array_equal(keep, C.thin_restated(case["cand"], case["level"], case["meas_root"], case["meas_level"]))
        for m in caught:
            wrong_pos = int(C._round(case["value"], m))
            wrong = C.thin_restated(case["cand"], case["level"], case["meas_root"], case["meas_level"], rounding=m)
            assert np.array_equal(wrong, keep) == (wrong_pos == r), (case["name"], m)      # a busy position off by one always flips a bit
            if wrong_pos != r:
                caught[m].add(case["value"])
    neg_tie = -0.49999999999999994                               # - 0.5 makes it -1.0, + 0.5 a tiny positive number
    assert caught["trunc"] >= {0.5, -0.5, 1.5, -1.5, -2.51} and caught["plus_half"] == {-0.5, -1.5, -2.51, neg_tie}
    assert caught["floor_half"] == {-0.5, -1.5, neg_tie} and caught["even"] >= {0.5, -0.5}
    assert set().union(*caught.values()) == set(C.ROUND_VALUES)      # every value is told from at least one wrong rounding


def test_thin_wide_cases_need_64_bits():
    for case in C.thin_wide_cases():
        keep = C.thin_expected(case)
        assert keep.all()
        sc = float(1 << case["level"])
        q = case["meas_root"] / sc
        assert (q == np.trunc(q)).all() and np.abs(case["meas_root"]).max() > 0.99e9
        d = case["cand"][:, None, :].astype(np.int64) - q[None, :, :].astype(np.int64)
        assert ((d * d).sum(axis=2).max()) > (1 << 40)
        wrong = C.thin_restated(case["cand"], case["level"], case["meas_root"], case["meas_level"], wrap32=True)
        assert not wrong.any()


def test_thin_level_cases_hold_every_level_and_the_filter_is_level_and_level_plus_1():
    cases = C.thin_level_cases()
    assert [c["level"] for c in cases] == [0, 1, 2, 3]
    seen = set()
    for case in cases:
        lv = case["meas_level"]
        assert list(lv - case["level"]) == [-1, 0, 1, 2]
        seen |= set(lv.tolist())
        keep = C.thin_expected(case)
        assert np.array_equal(~keep, case["expect_thinned"]) and (~keep).sum() == 4
        wrong = C.thin_restated(case["cand"], case["level"], case["meas_root"], case["meas_level"], level_only=True)
        assert (~wrong).sum() == 2 and not np.array_equal(wrong, keep)
    assert {-1, 4, 5} <= seen


def test_thin_size_cases_hold_every_size_and_seat():
    cases = C.thin_size_cases()
    assert {len(c["cand"]) for c in cases} == set(C.THIN_SIZES) and {len(c["meas_root"]) for c in cases} == {0, 1, 300}
    seats = set()
    for case in cases:
        keep = C.thin_expected(case)
        t = case["thinned_at"]
        if t is None:
            assert keep.all() and len(case["meas_root"]) == 0
            continue
        seats.add((len(keep), t))
        assert list(np.nonzero(~keep)[0]) == [t]
        only_last = C.thin_restated(case["cand"], case["level"], case["meas_root"][-1:], case["meas_level"][-1:])
        assert np.array_equal(only_last, keep)                  # the only hit is the last measurement
        if len(case["meas_root"]) > 1:
            assert C.thin_restated(case["cand"], case["level"], case["meas_root"][:-1], case["meas_level"][:-1]).all()
    assert {(257, 255), (257, 256), (513, 512), (256, 255), (255, 254), (1, 0), (513, 0)} <= seats


# ---- 2. the nLimit loop and the chunk seam -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _commit():
    base, _ = C.oracle_frames()["src"].Candidates(C.SEAM_LEVEL)
    codes = C.oracle_codes(base)
    codes_at = functools.lru_cache(maxsize=None)(lambda key: C.oracle_codes(np.array(key)))
    at = lambda p: codes_at(tuple(map(tuple, np.asarray(p).tolist())))
    return base, codes, at, C.commit_cases(base, codes, at)


def test_commit_cases_fall_where_they_are_named():
    base, codes, at, cases = _commit()
    assert {c["n"] for c in cases if "c0" in c} == set(C.COMMIT_SIZES)
    assert {c["kind"] for c in cases} == {"c0-1", "c0", "c0+1", "total", "total+1", "one", "zero", "minus3", "survivor", "dead", "neighbours"}
    assert {c["limit"] for c in cases if c["kind"] in ("zero", "minus3")} == {0, -3}
    for case in cases:
        w, h = C.level_size(C.SEAM_LEVEL)
        assert (case["cand"] >= 0).all() and (case["cand"][:, 0] < w).all() and (case["cand"][:, 1] < h).all()
        C.check_commit_layout(case, C.case_codes(case, base, codes, at))
    surv = [c for c in cases if c["kind"] == "survivor"]
    assert {(c["creates"], len(c["targets"])) for c in surv} == {(True, 2), (True, 3), (False, 2), (False, 3)}


def test_limit_model_is_the_composition_on_the_oracle():
    """limit_model over the table of single outcomes is stereo.compose's loop: the same created list on a case that has duplicates, thinning
    between targets and a limit (composed here from stereo.arc and the oracle's PatchFinder, since stereo.compose needs the device)"""
    base, codes, at, cases = _commit()
    case = next(c for c in cases if c["name"] == "n257_c0+1")
    per, outcome, keep = C.limit_model(case["cand"], C.SEAM_LEVEL, C.case_codes(case, base, codes, at), case["limit"])
    sc, fr = C.scene(), C.oracle_frames()
    cand = case["cand"].astype(np.int64)
    alive, num, made = np.ones(len(cand), dtype=bool), 0, []
    for j in case["targets"]:
        new = [S.level_zero_pos(cand[i], C.SEAM_LEVEL) for i, t in made if t == j - 1]
        if new:
            alive &= S.thin_candidates(cand, C.SEAM_LEVEL, created_root=new)
        idx = np.nonzero(alive)[0]
        res = C.oracle_results(sc["cam"], sc["pose_src"], C.SEAM_LEVEL, cand[idx], (None, sc["cam"], sc["poses"][j]), fr["tg"][j], fr["src"])
        for q, i in enumerate(idx):
            if res[q][0] == S.CREATED:
                made.append((int(i), j)); num += 1
            if num >= case["limit"]:
                break
    assert made == [(int(i), j) for j, p in enumerate(per) for i in np.nonzero(p["made"])[0]] and np.array_equal(keep, alive)


# ---- 3. a moved world, a second camera -----------------------------------------------------------------------------------------------------------
def test_moved_world_is_a_rigid_motion_the_arc_does_not_see():
    Rg, tg = C.MOVE_G
    assert abs(math.acos((np.trace(Rg) - 1) / 2) - 0.7) < 0.01 and np.linalg.norm(tg) > 2.0 and np.abs(Rg - Rg.T).max() > 0.3
    sc = C.scene()
    base, _ = C.oracle_frames()["src"].Candidates(C.SEAM_LEVEL)
    opa = sc["cam"].one_pixel_angle()
    assert np.abs(sc["pose_src_moved"][0] - np.eye(3)).max() > 0.3 and np.linalg.norm(sc["pose_src_moved"][1]) > 2.0
    for c in base[::37]:
        a = S.arc(sc["cam"], sc["pose_src"], sc["poses"][1], opa, C.SEAM_LEVEL, c)
        b = S.arc(sc["cam"], sc["pose_src_moved"], sc["poses_moved"][1], opa, C.SEAM_LEVEL, c)
        assert a["n"] == b["n"] > 5
        assert C.row_rel(b["tc"], a["tc"]) < 1e-11                                # the same points in the target camera's frame
        assert C.row_rel(C.unmove_points(b["world"]), a["world"]) < 1e-11         # and G times the old ones in the world
        # a transposed source rotation is visible under the moved pose and was not under the identity
        Rs, ts = sc["pose_src_moved"]
        t = S.arc(sc["cam"], (Rs.T, ts), sc["poses_moved"][1], opa, C.SEAM_LEVEL, c)
        assert t["n"] != b["n"] or C.row_rel(t["tc"], b["tc"]) > 1e-3
    sk = sc["cam_skew"]
    assert np.abs(sk.center - sc["cam"].center).min() > 20 and abs(sk.affine[0, 1]) > 5e-3 and abs(sk.affine[1, 0]) > 5e-3
    assert not np.array_equal(sk.poly, sc["cam"].poly) and (sc["img_skew"] != sc["imgs"][0]).mean() > 0.5


def test_second_camera_composition_on_the_oracle_creates_points_on_the_plane():
    """the oracle's composition with the skew camera's target creates points, they lie on the plane, and taking the source camera for the target's
    (or the other way round) moves them off it"""
    sc, fr = C.scene(), C.oracle_frames()
    base, _ = fr["src"].Candidates(C.SEAM_LEVEL)
    tgt = (None, sc["cam_skew"], sc["poses"][0])
    res = C.oracle_results(sc["cam"], sc["pose_src"], C.SEAM_LEVEL, base, tgt, fr["skew"], fr["src"])
    made = [i for i in range(len(base)) if res[i][0] == S.CREATED]
    assert len(made) >= 30
    z = np.array([S.triangulate(sc["cam"], sc["cam_skew"], sc["pose_src"], sc["poses"][0], S.level_zero_pos(base[i], C.SEAM_LEVEL), res[i][3])[2] for i in made])
    zw = np.array([S.triangulate(sc["cam"], sc["cam"], sc["pose_src"], sc["poses"][0], S.level_zero_pos(base[i], C.SEAM_LEVEL), res[i][3])[2] for i in made])
    ok = np.abs(z - sc["depth"]) < 0.02 * sc["depth"]
    assert ok.mean() >= 0.8 and (np.abs(zw - sc["depth"]) < 0.02 * sc["depth"]).mean() < 0.5 * ok.mean()


# ---- 4. the arc ----------------------------------------------------------------------------------------------------------------------------------
def test_arc_cases_take_the_path_they_are_named_for():
    cases = C.arc_cases()
    assert {c["level"] for c in cases} == set(C.ARC_LEVELS)
    claims = set()
    for case in cases:
        ref = C.arc_reference(case)
        claims.add(case["claim"])
        with warnings.catch_warnings():
            warnings.simplefilter("error")                       # stereo.arc is total: it neither raises nor warns
            got = [S.arc(case["cam"], case["pose_src"], case["pose_tgt"], case["opa"], case["level"], c) for c in case["cand"]]
        for r, g in zip(ref, got):
            assert g["n"] == r["n"], case["name"]
            claim = case["claim"]
            if r["n"]:                                           # the step count is no coin toss
                assert abs(r["ratio"] - np.rint(r["ratio"])) >= 1e-9, case["name"]
            if claim == "clamp_on":
                assert 0.15 < r["start_raw"] < 0.2 and g["start_raw"] < 0.2 and g["start"] == 0.2 and r["n"] > 2
                if "tight" in case["name"]:
                    assert r["start_raw"] > 0.2 * (1 - 2e-3)
            elif claim == "clamp_off":
                assert 0.2 < r["start_raw"] < 0.25 and g["start"] == g["start_raw"] > 0.2 and r["n"] > 2
                if "tight" in case["name"]:
                    assert r["start_raw"] < 0.2 * (1 + 2e-3)
            elif claim == "min_t_neg":
                assert r["min_t"] < -0.1 and r["max_t"] > 0.1 and r["src_angle"] > 2 * math.pi / 3 and r["start_raw"] < 0 and r["n"] > 2
            elif claim == "max_t_neg":
                assert r["max_t"] < -0.01 and r["src_angle"] > math.pi - 0.05 and r["end"] < 0 and r["n"] >= 2
            elif claim == "one_step":
                assert r["n"] == 2 and 0.5 < r["ratio"] < 0.7
            elif claim == "guard_below":
                assert 0.7e-8 < r["dd"] < 0.9e-8 and r["n"] == 0
            elif claim == "guard_above":
                assert 1.1e-8 < r["dd"] < 1.4e-8 and r["n"] >= 2
            elif claim == "no_arc":
                assert r["n"] == 0 and not (r["dd"] >= 1e-8 and np.isfinite(r["ratio"]))
            elif claim == "plain":
                assert r["n"] > 2 and np.isfinite(r["world"].astype(np.float64)).all()
            else:
                raise AssertionError(claim)
        if any(r["n"] for r in ref):
            floor = C.arc_floor(case, ref)
            assert floor < 1e-6, (case["name"], floor)           # the restatement and its longdouble twin are the same function
    assert claims == {"clamp_on", "clamp_off", "min_t_neg", "max_t_neg", "one_step", "guard_below", "guard_above", "no_arc", "plain"}
    through = [c for c in cases if c["name"].startswith("through")]
    for case in through:                                         # the ray is the axis exactly and passes through the target's centre
        ray = case["cam"].unproject(S.level_zero_pos(case["cand"][0], case["level"]))[0]
        assert np.array_equal(ray, [0.0, 0.0, 1.0])
        d = case["pose_src"][1] - case["pose_tgt"][1]
        assert d[0] == 0 and d[1] == 0 and abs(d[2]) == 2.0
    assert {np.sign((c["pose_src"][1] - c["pose_tgt"][1])[2]) for c in through} == {1.0, -1.0}
    skew = [c for c in cases if c["name"].startswith("skew_src")]
    moved = [c for c in cases if c["name"].startswith("moved_world")]
    assert len(moved) == 4 and all(np.abs(c["pose_src"][0] - np.eye(3)).max() > 0.3 for c in moved)
    assert len(skew) == 2 and all(abs(c["cam"].affine[0, 1]) > 5e-3 and abs(c["cam"].affine[1, 0]) > 5e-3 for c in skew)


def test_arc_is_total_where_the_cosine_leaves_its_domain():
    """oblique rays through the target's centre: the cosine of the source angle is 1 +- an ulp; whichever way it rounds nothing raises or warns"""
    cam = C.make_camera()
    P = C.ARC_SRC_POSE
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for level in C.ARC_LEVELS:
            w, h = C.level_size(level)
            for c in [(x, y) for x in range(3, w, w // 7) for y in range(2, h, h // 5)]:
                ray = C._ray(cam, level, c)
                for z in (1.0, -1.0, 3.7):
                    a = S.arc(cam, P, C.target_pose(P, z * ray), cam.one_pixel_angle(), level, c)
                    assert a["n"] >= 0
