"""On the oracle and the numpy restatement alone: every case of tests/pose_route_cases.py has the layout it is named for -- the exit digit
of the multi-workgroup median, the slices without found records, the count of found records, the branch of the step's exponential -- and
sits far enough from the M-estimator's cut-off that tests/test_pose_routes_gpu.py may ask for identical zero sets."""
import numpy as np
import pytest

import pose_route_cases as prc

# the weight under which a found record counts as cut: Tukey's (1 - e/s^2)^2 >= 1e-12 is a relative distance of 1e-6 from the cut, six
# orders above what the rounding of s^2 (a handful of operations on the exact median) can move
MARGIN = 1e-12
# the route every case of a group must be predicted onto (None: the group mixes routes, its cases carry what they expect)
GROUP_ROUTE = {"hard-plain_1025": "plain", "hard-plain_2047": "plain", "hard-plain_2048": "plain", "hard-plain_2049": "plain", "hard-plain_9cam_130": "plain",
               "hard-multi_hist_5000": ("multi", 10, False), "hard-multi_hist_12500": ("multi", 25, False), "hard-multi_gather_5000": ("multi", 10, True),
               "cand_cap": ("multi", 11, False), "step-regs": "regs", "step-plain": "plain", "step-multi": ("multi", 6, False)}


def _oracle(case):
    from oracle import oracle_track_pose_refine
    r, cams, cfbs, bfw = case.rig()
    return r, oracle_track_pose_refine(r, cams, cfbs, bfw, estimator=case.est, **case.schedule())


def test_the_route_restatement_follows_the_documented_switches():
    R = prc.route
    assert R(1024) == ("regs", 0, False) and R(1025) == ("multi", 3, False) and R(1024, ncam=9) == ("plain", 0, False) and R(1024, ncam=8)[0] == "regs"
    assert R(1025, ncam=9) == ("multi", 3, False) and R(1025, multi=0) == ("plain", 0, False) and R(130, multi=0) == ("regs", 0, False)
    assert R(64, multi=2, ppw=1) == ("multi", 64, False) and R(63, multi=2) == ("regs", 0, False) and R(63, ncam=9, multi=2) == ("plain", 0, False)
    assert R(130, multi=2, ppw=2) == ("multi", 64, False) and R(6000, ppw=64) == ("multi", 64, False) and R(6000) == ("multi", 12, False)
    assert R(2000, n_iter=16)[0] == "multi" and R(2000, n_iter=17) == ("plain", 0, False) and R(64, n_iter=17, multi=2) == ("regs", 0, False)
    assert R(16384, gather=1) == ("multi", 32, True) and R(16385, gather=1) == ("multi", 33, False) and R(6000, ppw=-3) == R(6000)
    assert R(6000, giveup=True) == ("multi_redone", 12, False) and R(1025, multi=0, giveup=True) == ("plain", 0, False)
    assert prc.slices(130, 64)[0] == (0, 2) and prc.slices(130, 64)[-1] == (127, 130) and {b - a for a, b in prc.slices(130, 64)} == {2, 3}
    assert all(b - a == 1 for a, b in prc.slices(64, 64)) and max(b - a for a, b in prc.slices(6000, 64)) == 94


def test_the_key_restatement_is_the_sorted_squared_errors_median():
    """keys() against the oracle: sigma^2 of a one-iteration Tukey call is (4.6851 * 1.4826 (1 + 5/(2 nf - 6)))^2 times the [nf/2] key."""
    from oracle import oracle_track_pose_update
    for name in ("lognormal", "ties", "many_zero", "zero_and_huge"):
        r = prc.population(name, 1025)
        k = prc.keys(r)
        med = prc.median_key(k).view(np.float64)
        _, _, s2 = oracle_track_pose_update((r["found"] != 0).astype(np.uint8), r["found_pos"], r["image"], r["sqrt_inv_noise"], np.zeros((len(r), 12)))
        c = 4.6851*1.4826*(1 + 5.0/(2*len(k) - 6))
        assert abs(s2 - c*c*med) <= 1e-14*s2, name
    k = prc.keys(prc.population("zero_and_huge", 5000))
    assert k.min() == 0 and k.max().view(np.float64) == 1e150*1e150 and 0 < prc.median_key(k).view(np.float64) < 1e300      # (1e300 to an ulp)
    k = prc.keys(prc.population("zero_and_inf", 5000))
    assert k.min() == 0 and k.max() == 0x7ff0000000000000 and np.count_nonzero(k == k.max()) == 1


def test_the_candidate_cap_populations_put_4096_and_4097_keys_in_the_medians_bin():
    for name, want in (("bin_4096", 4096), ("bin_4097", 4097)):
        r = prc.population(name, prc.BIN_N[name])
        k = prc.keys(r)
        e2 = k.view(np.float64)
        assert len(k) == len(r) == want + 1400 and prc.prefix_counts(k)[0] == want
        assert np.count_nonzero(e2 < 0.4) == 700 and np.count_nonzero(e2 > 2.1) == 700 and np.count_nonzero((e2 >= 0.5) & (e2 < 2.0)) == want
        assert prc.exit_pass(k) == (0 if want == 4096 else 1)
    assert prc.MULTI_CAND_CAP == 4096


def test_nine_cameras_relabel_the_records_without_changing_the_oracle_s_result():
    from oracle import oracle_track_pose_refine
    cam, cfbs, bfw, _ = prc.scene()
    r = prc.population("lognormal", 130)
    r9, cams9, cfb9 = prc.spread_cameras(r, 9)
    assert len(cams9) == 9 and set(np.unique(r9["cam"])) == {0, 2, 4, 6, 8} and np.array_equal(r9["cam"] % 2, r["cam"])      # (the first 130 are camera 0's)
    big = prc.spread_cameras(prc.population("lognormal", 1025), 9)[0]
    assert set(np.unique(big["cam"])) == set(range(9)) and np.array_equal(big["cam"] % 2, prc.population("lognormal", 1025)["cam"])
    a, b = oracle_track_pose_refine(r, [cam, cam], cfbs, bfw), oracle_track_pose_refine(r9, cams9, cfb9, bfw)
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_the_step_scales_straddle_every_seam():
    sc = prc.step_scales()
    assert [b for _, b in sc] == ["one_term", "one_term", "two_terms", "two_terms", "series", "series", "closed_form", "closed_form"]
    assert abs(sc[1][0]/0.0402 - 0.99) < 2e-3 and abs(sc[3][0]/0.4017 - 0.99) < 2e-3 and abs(sc[5][0]/200.8 - 0.99) < 2e-3


@pytest.mark.parametrize("group", sorted(prc.REFINE_GROUPS))
def test_every_case_has_its_layout_and_its_margin(group):
    cases = prc.REFINE_GROUPS[group]()
    assert cases
    seen_finite = False
    for case in cases:
        r, ((Ro, to), mo, wo, _) = _oracle(case)
        f = r["found"] != 0
        rt = case.route()
        if group in GROUP_ROUTE:
            want = GROUP_ROUTE[group]
            assert (rt[0] == want) if isinstance(want, str) else (rt == want), (case, rt)
        ex = case.expect
        k = prc.keys(r)
        if "exit" in ex:
            assert prc.exit_pass(k) == ex["exit"], (case, prc.prefix_counts(k))
        if "in_bin" in ex:
            assert prc.prefix_counts(k)[0] == ex["in_bin"], case
        if "nwg" in ex:
            assert rt[0] == "multi" and rt[1] == ex["nwg"], (case, rt)
        if "empty" in ex:
            assert sum(1 for a, b in prc.slices(len(r), rt[1]) if not f[a:b].any()) == ex["empty"], case
        if "nf" in ex:
            assert f.sum() == ex["nf"], case
        assert np.all(wo[~f] == 0), case
        if not (np.isfinite(wo).all() and np.isfinite(mo).all()):
            assert case.hard and "zero_median" in case.name, case          # only a zero median may leave the reference without a number
            continue
        seen_finite = True
        assert np.isfinite(Ro).all() and np.isfinite(to).all(), case
        if case.est == "Tukey":
            assert np.all((wo[f] == 0) | (wo[f] >= MARGIN)), (case, wo[f][(wo[f] > 0)].min())
        else:
            assert np.all(wo[f] > 0), case
        if "branch" in ex:
            w2 = float(mo[3:] @ mo[3:])
            assert prc.step_branch(w2) == ex["branch"], (case, w2)
            assert np.all(wo[f] == 1.0), case
    assert seen_finite


def test_the_hard_routes_reach_every_exit_digit_and_every_slice_layout():
    ex = {c.expect["exit"] for g in ("hard-multi_hist_5000", "hard-multi_hist_12500", "cand_cap") for c in prc.REFINE_GROUPS[g]() if "exit" in c.expect}
    assert ex == {0, 1, 2, 3, 4, None}
    by = {c.name: c for c in prc.slice_cases()}
    assert by["one_record_per_workgroup"].route() == ("multi", 64, False) and by["two_sizes_of_slice"].route() == ("multi", 64, False)
    assert by["workgroup_cap"].route() == ("multi", 64, False) and by["below_the_forced_floor"].route() == ("regs", 0, False)
    assert [c.route() for c in prc.gather_cases()] == [("multi", 32, True), ("multi", 33, False)]
    assert [c.route() for c in prc.iteration_cases()] == [("multi", 4, False), ("plain", 0, False)]
    assert [c.route()[0] for c in prc.reuse_sequence()] == ["multi", "regs", "plain", "multi", "regs", "plain", "multi_redone"]
    masks = [c.rig()[0]["found"] for c in prc.reuse_sequence()]
    assert all(0 < m.sum() < len(m) for m in masks)


def test_the_single_update_inputs_cover_their_sizes():
    from oracle import oracle_track_pose_update
    for pop in prc.UPDATE_POPS:
        for n in prc.UPDATE_N:
            found, fp, ip, si, J = prc.update_inputs(pop, n)
            assert len(found) == n and found.sum() >= 1 and (pop != "one_found" or found.sum() == 1)
            mo, wo, so = oracle_track_pose_update(found, fp, ip, si, J)
            assert np.all(wo[found == 0] == 0)
            if np.isfinite(mo).all() and np.isfinite(wo).all():
                assert np.all((wo[found != 0] == 0) | (wo[found != 0] >= MARGIN)), (pop, n)
