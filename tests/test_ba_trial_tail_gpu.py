"""The tail of an LM trial and the head it feeds (csrc/ba_kernels.h, ba_select.h, ba_solver.hip):

a. The iteration-start robust chi2 riding on the first trial (k_eval_start + the fourth array of k_final_sums) against the plain
   start sum (k_robust_sum + k_final_sums in front of the linearisation), SAME build: a default handle and a handle created under
   MCP_BA_MAILBOX=0 run Compute(4) on noisy maps; the iteration logs and the state must be equal in every bit.  Sizes: 255, 256 and
   257 measurements (one EVAL_BLOCK either side), and 65 537 measurements on 16 385 free points (257 partials of the evaluation
   and 257 of the back-substitution: one more than k_final_sums has threads).  The cases assert their own trial counts: an
   iteration after the first whose first trial is accepted, one whose first trial is rejected, a first trial whose factorisation
   "fails" (MCP_BA_TEST_FAIL_TRIAL: the start block arrives with a stale step), a handle without the robust kernel, and a handle
   that is re-entered.
b. k_final_sums beyond its thread count: DebugTrial on the large map against math.fsum of what it returns per measurement and per
   point, tolerances those of test_ba_trial_gpu.py; twice, same bits.
c. Pass 0 of the median's radix select at the wavefront seams: DebugHead("plain") on one-measurement-per-point handles, populations
   that make a wavefront's lanes share one LDS counter, two counters, 64 counters, and all but one lane a counter.  The median is
   element [n/2] of the sorted |chi2| bit for bit.  (Written for a pass 0 that counts by wavefront -- ballot, one add per distinct
   bin; measured slower than the per-lane adds and not kept, profiles/r06/README.md -- and kept as the pin for whoever tries again.)
"""
import copy
import math

import numpy as np
import pytest

import ba_medians as bm
import ba_trial_cases as tc
from test_ba_medians_gpu import _env, _handle
from test_ba_trial_gpu import TOL_ROBUST, TOL_SCALE, TOL_SS

pytestmark = pytest.mark.gpu

LOG_KEYS = ("chi2_start", "chi2_end", "lambda_end", "sigma_sq", "rms_update", "trials", "accepted")
PLAIN = {"MCP_BA_MAILBOX": "0"}
_MAPS = {}


def _trimmed(p, nmeas):
    """p without its last measurements that are not a point's own (source) one, one per point at most, down to nmeas"""
    drop = p.n_meas - nmeas
    assert drop >= 0
    own = (p.ms_mkf == p.pt_src[p.ms_pt, 0]) & (p.ms_cam == p.pt_src[p.ms_pt, 1])
    keep = np.ones(p.n_meas, dtype=bool)
    seen = set()
    for j in range(p.n_meas - 1, -1, -1):
        if drop == 0:
            break
        if not own[j] and int(p.ms_pt[j]) not in seen:
            keep[j] = False
            seen.add(int(p.ms_pt[j]))
            drop -= 1
    q = copy.copy(p)
    q.ms_mkf, q.ms_cam, q.ms_pt, q.ms_level = p.ms_mkf[keep], p.ms_cam[keep], p.ms_pt[keep], p.ms_level[keep]
    q.ms_uv = np.ascontiguousarray(p.ms_uv[keep])
    q.ids = {}
    return q


def _map(nmeas):
    """a noisy map (pixel noise, 2 % gross outliers, perturbed poses and depths) of exactly nmeas measurements, four per point but for
    the few points that lose one to reach the count: 64 or 65 points on 6 keyframes, or 16 385 points on 12"""
    if nmeas not in _MAPS:
        from mcptam_amd import synth
        big = nmeas > 1000
        n_points = -(-nmeas // 4)
        p = _trimmed(synth.make_problem(n_cams=2, n_mkf=12 if big else 6, n_points=n_points, per_point=4, arc_step=0.4), nmeas)
        assert p.n_meas == nmeas and p.n_points == n_points and not p.pt_fixed.any()
        _MAPS[nmeas] = p
    return _MAPS[nmeas]


def _solve(nmeas, env, calls=(4,), robust=True):
    """a fresh handle created under `env` (MCP_BA_SMALL=0: a small map takes the launches of a large one), Compute() once per entry of
    `calls` (a later call continues at the lambda the one before ended with) -> (logs of all calls, state bytes)"""
    from helpers import collect
    from mcptam_amd import chain_bundle
    p = _map(nmeas)
    chain_bundle.struct_cache_clear()
    with _env(dict({"MCP_BA_SMALL": "0"}, **env)):
        g = chain_bundle.ChainBundle(p.cams, robust, True, False, disable_convergence=True)
        ids = p.populate(g)
        g.Prepare()
        logs, rides = [], []
        for i, k in enumerate(calls):
            assert g.Compute(k, g.GetLambda() if i else -1.0) == k
            logs += g.IterLogs()
            rides.append(g.Timing()["n_start_rides"])
    R, t, X = collect(g, ids)
    g.close()
    # the case means what it says only if the handle took the path it is named for: the start sum rode on the first trial of every
    # iteration but a call's first (mcp_ba_timing.n_start_rides, counted where k_eval_start is launched), or on none
    assert rides == ([0] * len(calls) if env.get("MCP_BA_MAILBOX") == "0" else [k - 1 for k in calls]), (env, calls, rides)
    return logs, (R.tobytes(), t.tobytes(), X.tobytes())


def _same(a, b, what):
    la, lb = a[0], b[0]
    assert len(la) == len(lb), what
    for i, (x, y) in enumerate(zip(la, lb)):
        for k in LOG_KEYS:
            assert np.float64(x[k]).view(np.uint64) == np.float64(y[k]).view(np.uint64), (what, i, k, x[k], y[k])
    assert a[1] == b[1], (what, "state")


def _trials(run):
    return [l["trials"] for l in run[0]]


@pytest.mark.parametrize("nmeas", [255, 256, 257, 65537])
def test_start_sum_riding_on_the_first_trial_equals_the_plain_start_sum(gpu_required, nmeas):
    ride, plain = _solve(nmeas, {}), _solve(nmeas, PLAIN)
    print(nmeas, [(l["trials"], l["accepted"], l["chi2_start"]) for l in ride[0]])
    _same(ride, plain, nmeas)
    tr = _trials(ride)
    assert len(tr) == 4 and all(l["accepted"] for l in ride[0])
    if nmeas == 65537:      # iterations after the first whose first trial is rejected, and one whose first trial is accepted
        assert max(tr[1:]) >= 2 and min(tr[1:]) == 1, tr
    else:
        assert tr[1:] == [1, 1, 1], tr


def test_start_sum_riding_without_the_robust_kernel(gpu_required):
    ride, plain = _solve(257, {}, robust=False), _solve(257, PLAIN, robust=False)
    print([(l["trials"], l["accepted"], l["chi2_start"]) for l in ride[0]])
    _same(ride, plain, "non-robust")
    assert max(_trials(ride)[1:]) >= 2, _trials(ride)          # a first trial rejected after the first iteration


def test_start_block_arrives_with_a_stale_step(gpu_required):
    """the first trial of the second iteration is treated as a failed factorisation: its mailbox still carries the start block, the stale
    step follows on the same stream"""
    base = _solve(256, {})
    k = base[0][0]["trials"] + 1
    env = {"MCP_BA_TEST_FAIL_TRIAL": str(k)}
    ride, plain = _solve(256, env), _solve(256, dict(PLAIN, **env))
    print(k, [(l["trials"], l["accepted"], l["chi2_start"]) for l in ride[0]])
    _same(ride, plain, "stale")
    assert ride[0][0] == base[0][0] and ride[0][1]["trials"] >= 2 and _trials(base)[1] == 1, (_trials(ride), _trials(base))
    assert np.float64(ride[0][1]["chi2_start"]).view(np.uint64) == np.float64(base[0][1]["chi2_start"]).view(np.uint64)


def test_a_re_entered_handle_gives_the_log_of_one_call(gpu_required):
    once, twice, twice_plain = _solve(257, {}), _solve(257, {}, calls=(2, 2)), _solve(257, PLAIN, calls=(2, 2))
    _same(twice, once, "Compute(2) twice against Compute(4)")
    _same(twice, twice_plain, "re-entered, riding against plain")


def test_final_sums_beyond_the_thread_count(gpu_required):
    from mcptam_amd import chain_bundle
    from oracle import OracleBundle
    p = _map(65537)
    chain_bundle.struct_cache_clear()
    g = chain_bundle.ChainBundle(p.cams, True, True, False)
    p.populate(g)
    n = g.Prepare()
    chi2_cur = g.Eval(p.n_meas)[0]
    a = g.DebugTrial(tc.LAMBDA)
    b = g.DebugTrial(tc.LAMBDA)
    g.close()
    report = {k: a[k] for k in ("ncb", "nbb", "nfl", "np", "nmeas", "small_mode")}
    print(report)
    assert a["nmeas"] == 65537 and a["nfl"] == 16385 and a["nbb"] == 257 and not a["small_mode"], report
    assert -(-a["nmeas"] // 256) == 257
    for k in ("x", "poses", "points", "chi2", "robust_chi2", "scale", "scale_pose", "scale_point", "ss", "ss_pose", "ss_point"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    # robust chi2: the Huber sum of the trial's chi2 at the sigma block of the CURRENT state's median
    sig = bm.sigma_block(bm.reference(chi2_cur, p.n_meas // 2), p.n_meas)
    want = bm.robust_chi2(a["chi2"], sig)
    print("robust chi2 %r fsum %r (%.2e)" % (a["robust_chi2"], want, abs(a["robust_chi2"] - want) / want))
    assert abs(a["robust_chi2"] - want) <= TOL_ROBUST * want, (a["robust_chi2"], want)
    # the point parts of sum x^2 and of sum x (lambda x + b): the device's x, the oracle's b
    n_p = a["np"]
    xl = a["x"][n_p:]
    want = math.fsum((xl * xl).tolist())
    print("ss_point %r fsum %r (%.2e)" % (a["ss_point"], want, abs(a["ss_point"] - want) / want))
    assert abs(a["ss_point"] - want) <= TOL_SS * want, (a["ss_point"], want)
    o = OracleBundle(p.cams, True, True, False)
    p.populate(o)
    bl = o.DebugRhs()[n_p:]
    assert len(bl) == len(xl) == n - n_p
    t = np.asarray(xl, dtype=tc.LD) * (tc.LD(tc.LAMBDA) * np.asarray(xl, dtype=tc.LD) + np.asarray(bl, dtype=tc.LD))
    want, mag = float(t.sum()), float(np.abs(t).sum())
    print("scale_point %r reference %r (%.2e of the magnitude)" % (a["scale_point"], want, abs(a["scale_point"] - want) / mag))
    assert abs(a["scale_point"] - want) <= TOL_SCALE * mag, (a["scale_point"], want, mag)


def _pass0_populations(n):
    """name -> chi2 array: what the lanes of a wavefront (64 consecutive values) hold in the first digit (sign + ten exponent bits: a bin
    is a binade pair, [0.5, 2), [2, 8), ...)"""
    r = np.random.default_rng([20261020, n])
    i = np.arange(n)
    u = r.uniform(0.0, 1.0, n)
    one = 0.5 + 1.49 * u                                        # [0.5, 2): one bin
    pops = {
        "one_bin": one,
        "64_bins_cycled": 4.0 ** ((i % 64) - 32.0) * (1.0 + 0.99 * u),
        "two_bins_by_lane": np.where(i % 2 == 0, 1.0 + 0.9 * u, 5.0 + 2.0 * u),
        "stray_lane0": np.where(i % 64 == 0, 100.0 + u, one),
        "stray_lane63": np.where(i % 64 == 63, 100.0 + u, one),
    }
    x = r.lognormal(0.0, 2.0, n)
    x[r.random(n) < 0.3] *= -1.0
    z = r.random(n) < 0.2
    x[z] = np.where(i[z] % 2 == 0, 0.0, -0.0)
    pops["zeros_and_negatives"] = x
    x = r.lognormal(0.0, 2.0, n)
    x[n // 3] = np.inf
    pops["an_inf"] = x
    return pops


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_pass0_counting_at_the_wave_seams(gpu_required, n):
    g = _handle("single", n)
    fails = []
    for name, x in _pass0_populations(n).items():
        k = bm.keys(x) >> np.uint64(53)
        if name == "64_bins_cycled":
            assert len(np.unique(k[:64])) == min(n, 64)
        if name in ("one_bin",):
            assert len(np.unique(k)) == 1
        if name == "two_bins_by_lane":
            assert len(np.unique(k)) == min(n, 2)
        r = g.DebugHead("plain", x, 1.0)
        ref = bm.reference(x, n // 2)
        print("n=%d %-20s median %r" % (n, name, r["median"]))
        if r["rank"] != n // 2 or not bm.same_bits(r["median"], ref):
            fails.append((name, r["rank"], r["median"], ref))
    assert not fails, fails
