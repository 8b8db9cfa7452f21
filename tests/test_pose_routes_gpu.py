"""Every route of Tracker::TrackMap's pose iterations -- register-held, plain, multi-workgroup (histogram and gathered median), sharded,
single update -- against the oracle at the seams of its counts and of its median: the cases of tests/pose_route_cases.py, whose layouts
and cut-off margins tests/test_pose_routes_cpu.py shows on the oracle alone.  After every call of mcp_track_pose_refine the route the
library reports (mcp_debug_last_pose_route) has to be the one the documented switches predict."""
import numpy as np
import pytest

import pose_route_cases as prc

pytestmark = pytest.mark.gpu


def _set_env(monkeypatch, env):
    for k in prc.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _noop_allreduce(buf, count, stream):
    """The other rank of a two-rank call holds no records: its part of every sum is zero, the sum is what is there already."""


def _run(case, monkeypatch, env=None):
    """(pose, mu, weights, records out) of the library for a case; a refine call's reported route is checked on the way."""
    from mcptam_amd.keyframe import last_pose_route, track_pose_refine, track_pose_refine_sharded
    r, cams, cfbs, bfw = case.rig()
    _set_env(monkeypatch, case.env if env is None else env)
    if case.kind == "sharded":
        world, rank = case.expect.get("world", 1), case.expect.get("rank", 0)
        return track_pose_refine_sharded(r, cams, cfbs, bfw, allreduce=_noop_allreduce if world > 1 else None, rank=rank, world=world, cap=len(r) + prc.SHARD_PAD,
                                         estimator=case.est, **case.schedule())
    out = track_pose_refine(r, cams, cfbs, bfw, estimator=case.est, **case.schedule())
    want = case.route() if env is None else prc.route_of_env(len(r), case.ncam, case.n_iter(), env)
    assert last_pose_route() == want, (case, last_pose_route(), want)
    return out


def _oracle(case):
    from oracle import oracle_track_pose_refine
    r, cams, cfbs, bfw = case.rig()
    return oracle_track_pose_refine(r, cams, cfbs, bfw, estimator=case.est, **case.schedule())


def _dev(got, ref):
    (Rg, tg), mg, wg, _ = got
    (Ro, to), mo, wo, _ = ref
    return max(np.abs(Rg - Ro).max(), np.abs(tg - to).max()), np.abs(mg - mo).max(), np.abs(wg - wo).max()


def _check(case, got, ref, pose_atol=1e-10, mu_atol=1e-10):
    """The project's tolerances (tests/test_img_gpu.py): pose 1e-10, weights rtol 1e-9 / atol 1e-12 with identical zero sets, mu rtol 1e-6 /
    atol 1e-9 max(1, |mu|) on the hard populations and atol 1e-10 otherwise; where the reference has no number the call has none either."""
    (Rg, tg), mg, wg, og = got
    (Ro, to), mo, wo, oo = ref
    r = case.rig()[0]
    f = r["found"] != 0
    assert np.all(wg[~f] == 0), case
    if not (np.isfinite(wo).all() and np.isfinite(mo).all()):
        assert not np.isfinite(mg).all(), case
        return
    dp, dm, dw = _dev(got, ref)
    print("%-44s pose %.3g  mu %.3g  weights %.3g" % (case, dp, dm, dw))
    assert np.array_equal(wg == 0, wo == 0), case
    assert np.allclose(wg, wo, rtol=1e-9, atol=1e-12), (case, dw)
    if case.hard:
        assert np.allclose(mg, mo, rtol=1e-6, atol=1e-9*max(1.0, np.abs(mo).max())), (case, dm)
    else:
        assert np.allclose(mg, mo, rtol=0, atol=mu_atol), (case, dm)
    assert np.allclose(Rg, Ro, rtol=0, atol=pose_atol) and np.allclose(tg, to, rtol=0, atol=pose_atol), (case, dp)
    assert np.allclose(og["image"][f], oo["image"][f], rtol=0, atol=1e-8), case
    assert np.array_equal(og["image"][~f], r["image"][~f]), case


@pytest.mark.parametrize("rname", sorted(prc.HARD_ROUTES))
def test_hard_populations_on_every_route(gpu_required, monkeypatch, rname):
    """Ties, sixty binades, zeros, a zero median, keys apart in their last bits, clusters that leave the multi-workgroup median's global
    passes after every digit (or never), all found records in one slice, one found record, keys of 0, 1e300 and infinity -- after one,
    two and three iterations on the plain kernel (1025, 2047 .. 2049 records with unfound gaps; nine cameras at 130), the multi-workgroup
    kernel (histograms at 5000 and 12500, gathered at 5000) and the sharded kernels (cap = n + 37); Huber and Cauchy on two populations
    each."""
    for case in prc.hard_cases(rname):
        _check(case, _run(case, monkeypatch), _oracle(case))


def test_candidate_cap_of_the_multi_workgroup_median(gpu_required, monkeypatch):
    """Exactly 4096 keys in the median's first bin are gathered, 4097 go through another global pass."""
    for case in prc.cand_cap_cases():
        _check(case, _run(case, monkeypatch), _oracle(case))


def test_slices_of_the_multi_workgroup_kernel(gpu_required, monkeypatch):
    """One record per workgroup, 64 workgroups with two sizes of slice, the cap of 64 workgroups with slices longer than asked for, slices
    without a found record (all found in one; one found; none found: null update, the pose's bytes, weights 0), and 63 records, which
    MCP_TRACK_REFINE_MULTI=2 does not force."""
    for case in prc.slice_cases():
        got = _run(case, monkeypatch)
        if case.expect.get("nf") == 0:
            (R, t), mu, w, out = got
            bfw = case.rig()[3]
            assert np.array_equal(R, bfw[0]) and np.array_equal(t, bfw[1]) and np.all(mu == 0) and np.all(w == 0), case
            assert np.array_equal(out["image"], case.rig()[0]["image"])
        _check(case, got, _oracle(case))


def test_gathered_median_at_its_largest_size_and_one_past_it(gpu_required, monkeypatch):
    """MCP_TRACK_REFINE_GATHER=1 at 16384 records (128 KB of dynamic LDS) and at 16385, where the histograms take over: both against the
    oracle, both bit for bit what the call gives without the switch (an exact median either way)."""
    for case in prc.gather_cases():
        got = _run(case, monkeypatch)
        _check(case, got, _oracle(case))
        plain = _run(case, monkeypatch, env={})
        assert np.array_equal(got[0][0], plain[0][0]) and np.array_equal(got[0][1], plain[0][1]) and np.array_equal(got[1], plain[1]), case
        assert np.array_equal(got[2], plain[2]) and np.array_equal(got[3]["image"], plain[3]["image"]), case


def test_sixteen_iterations_fill_the_multi_scratch_and_seventeen_leave_it(gpu_required, monkeypatch):
    """Iteration 16 uses the last slot of the multi-workgroup kernel's per-iteration buffers; a schedule of 17 runs on the plain kernel."""
    c16, c17 = prc.iteration_cases()
    a = _run(c16, monkeypatch)
    _check(c16, a, _oracle(c16))
    b = _run(c16, monkeypatch)
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    _check(c17, _run(c17, monkeypatch), _oracle(c17))


# largest deviation from the oracle seen on the MI355X over the four routes, per branch of se3_exp_step: (pose, mu)
STEP_SEEN = {"one_term": (8.33e-17, 8.11e-17), "two_terms": (7.42e-16, 7.43e-16), "series": (4.49e-13, 4.28e-13), "closed_form": (3.25e-12, 1.27e-12)}
# asserted on pose and mu alike: eight times the larger of the two, or 1e-10 where that is smaller
STEP_BOUND = {b: min(1e-10, 8*max(STEP_SEEN[b])) for b in prc.STEP_BRANCHES}


@pytest.mark.parametrize("rname", sorted(prc.STEP_ROUTES))
def test_step_size_seams_of_the_exponential(gpu_required, monkeypatch, rname):
    """pose_step_from_sums -> se3_exp_step branches on |omega|^2 at 1e-8, 1e-6 and 0.25; the scenes all step by |omega|^2 ~ 6e-6.  With all
    weights 1 and the found positions scaled about the projections, one iteration steps 1 % below and above every seam, far below the
    first and at |omega| ~ 2.5 rad, on the register-held, plain, multi-workgroup and sharded routes.

    Measured on the MI355X, largest |GPU - oracle| over the four routes, (pose, mu) per branch:
      one_term    (|omega|^2 < 1e-8:  scales 1e-4, 0.0398)   8.33e-17, 8.11e-17   (mu ~ 1e-4: 1e-12 relative)
      two_terms   (< 1e-6:            scales 0.0406, 0.398)  7.42e-16, 7.43e-16
      series      (< 0.25:            scales 0.406, 198.8)   4.49e-13, 4.28e-13   (mu ~ 0.5)
      closed_form (above:             scales 202.8, 1000)    3.25e-12, 1.27e-12   (mu ~ 2.5)
    i.e. mu agrees to about 1e-12 relative in every branch -- the reciprocal-square-root pivots against the oracle's square roots and
    divisions on a 6 x 6 of this conditioning -- and the exponential adds nothing visible on either side of a seam (0.99 and 1.01 times
    a seam differ by no more than their step sizes do).  The bound asserted per branch is eight times the larger figure, all below the
    1e-10 the other pose tests ask of pose and mu: 6.7e-16, 5.9e-15, 3.6e-12, 2.6e-11."""
    worst = {}
    for case in prc.step_cases(rname):
        got, ref = _run(case, monkeypatch), _oracle(case)
        dp, dm, _ = _dev(got, ref)
        b = case.expect["branch"]
        worst[b] = (max(worst.get(b, (0, 0))[0], dp), max(worst.get(b, (0, 0))[1], dm))
        _check(case, got, ref, pose_atol=STEP_BOUND[b], mu_atol=STEP_BOUND[b])
    print("step deviations on", rname, {b: ("%.3g" % p, "%.3g" % m) for b, (p, m) in worst.items()})


def test_few_found_records_leave_the_prior_and_a_rank_deficient_sum(gpu_required, monkeypatch):
    """One, two and three found records of 1025 (plain) and of 2048 (multi-workgroup): the 6 x 6 is the prior plus rank <= 6, the
    small-sample factor of sigma wraps (1, 2) or divides by zero (3) as the reference's does."""
    for case in prc.few_found_cases():
        _check(case, _run(case, monkeypatch), _oracle(case))


def test_sharded_slots_counts_and_zero_keys(gpu_required, monkeypatch):
    """Two ranks' table in one process, the other rank absent (its slot and count stay zero): as rank 0 and as rank 1, cap = n + 37, on a
    population with true zero keys beside the table's zero padding -- k_pr_accum's mask (i % cap) >= counts[i / cap] and the slot offset."""
    for case in prc.shard_slot_cases():
        _check(case, _run(case, monkeypatch), _oracle(case))


@pytest.mark.parametrize("n", prc.UPDATE_N)
def test_single_update_on_hard_populations(gpu_required, n):
    """mcp_track_pose_update (k_pose_errors, the select passes, k_pose_solve) on ties, zeros and one found record at 1, 255 .. 257 and 1025
    records, with the tolerances of test_pose_update_and_refine_with_the_other_m_estimators."""
    from mcptam_amd.keyframe import track_pose_update
    from oracle import oracle_track_pose_update
    for pop in prc.UPDATE_POPS:
        for est in ("Tukey", "Huber"):
            args = prc.update_inputs(pop, n)
            mg, wg, sg = track_pose_update(*args, -1.0, est)
            mo, wo, so = oracle_track_pose_update(*args, -1.0, est)
            assert np.all(wg[args[0] == 0] == 0), (pop, n, est)
            if not (np.isfinite(mo).all() and np.isfinite(wo).all()):
                assert not (np.isfinite(mg).all() and np.isfinite(wg).all()), (pop, n, est)
                continue
            assert abs(sg - so) <= 1e-13*so, (pop, n, est, sg, so)
            assert np.array_equal(wg == 0, wo == 0) and np.allclose(wg, wo, rtol=1e-12, atol=0), (pop, n, est)
            assert np.allclose(mg, mo, rtol=1e-9, atol=1e-13), (pop, n, est, np.abs(mg - mo).max())


def test_scratch_reuse_across_sizes_and_routes(gpu_required, monkeypatch):
    """The pose iterations' scratch lives across calls (device weights, pinned weights and parameter block, the kept copy of the records):
    a large multi-workgroup call, then small register-held ones, plain ones, a forced multi-workgroup one and the redo after a give-up,
    each with another found mask -- every one equals the oracle, and unfound records come back with weight exactly 0."""
    for case in prc.reuse_sequence():
        _check(case, _run(case, monkeypatch), _oracle(case))
