"""The six routes to the bundle adjuster's Huber median (csrc/ba_select.h, ba_trial.h, ba_small.h, ba_head.h, ba_headl.h) at their
candidate-table caps and guess seams: every route is fed the hard chi2 populations of tests/ba_medians.py through the hook
`ChainBundle.DebugHead` (which runs the member functions the solver calls) and must return element [size/2] of the sorted |chi2|
bit for bit, the sigma block of that element, the robust chi2 at that block, and -- where the host learns which branch was taken --
the branch the model of ba_medians.py predicts."""
import contextlib
import math
import os
import subprocess

import numpy as np
import pytest

import ba_medians as bm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# which handle serves which route: the scheduling knobs are read when the handle is created / prepared
ENVS = {
    "single": dict(MCP_BA_HEAD_AHEAD="1", MCP_BA_HEAD_LARGE="1", MCP_BA_NEAR_MISS="0"),
    "multi": dict(MCP_BA_FORCE_MULTI="1", MCP_BA_SELECT_CAP=str(bm.SELECT_CAP), MCP_BA_NEAR_MISS="0"),
}
ROUTE_ENV = {"plain": "single", "small": "single", "ahead": "single", "large": "single", "ranks": "multi", "ride": "multi"}
MULTI_COUNTS = (3, 1025) + bm.LARGE_COUNTS          # ranks and ride also on two small maps (the n = 3 denominator, more than one block)
SENTINEL = 0x7ff8000000c0ffee

_handles = {}
_results = {}


@contextlib.contextmanager
def _env(vals):
    old = {k: os.environ.get(k) for k in vals}
    os.environ.update(vals)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(kind, n):
    """the cheapest map with exactly n measurements (chi2 is overridden: the geometry does not matter): n free points expressed in a
    fixed pose, each measured once from the one free pose; cached per (environment, count)"""
    if (kind, n) not in _handles:
        from mcptam_amd import chain_bundle, synth
        from mcptam_amd.taylor_camera import TaylorCamera
        cam = TaylorCamera(synth.DEFAULT_CAM_PARAMS, (640, 480), (640, 480), (640, 480))
        rng = np.random.default_rng([5, n])
        with _env(ENVS[kind]):
            g = chain_bundle.ChainBundle([cam], True, True, False)
            fixed = g.AddPose(np.eye(3), np.zeros(3), True)
            free = g.AddPose(np.eye(3), np.array([0.05, 0.0, 0.0]), False)
            X = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(4, 9, n)], axis=1)
            ids = g.AddPointBatch(X, np.full((n, 1), fixed, dtype=np.int32), np.ones(n, dtype=np.int32), np.zeros(n, dtype=np.uint8))
            uv = np.stack([rng.uniform(100, 540, n), rng.uniform(100, 380, n)], axis=1)
            g.AddMeasBatch(np.full((n, 1), free, dtype=np.int32), np.ones(n, dtype=np.int32), ids, uv, np.ones(n), np.zeros(n, dtype=np.int32))
            if kind == "multi":
                g.SetAllReduce(lambda ptr, count, stream: None, 0, 1)          # one rank: the sum over the ranks changes nothing
            g.Prepare()
        _handles[(kind, n)] = g
    return _handles[(kind, n)]


def _close(a, b, rel):
    if np.isnan(b):
        return bool(np.isnan(a))
    if np.isinf(b):
        return a == b
    return abs(a - b) <= rel * abs(b)


def _check(route, n, p, r, fails):
    """one DebugHead report `r` of population `p` against the reference and the model; appends what is wrong to `fails`"""
    rank = n // 2
    ref = bm.reference(p.x, rank)
    md = bm.model(route, p.x, rank, p.prev_median)
    tag = "%s n=%d %s" % (route, n, p.name)
    print("%-60s median %-24r cand %-6d %s" % (tag, r["median"], md["cand"], " ".join(sorted(md["branches"]))))

    def bad(what, *a):
        fails.append((tag, what) + a)
    if r["rank"] != rank:
        bad("rank", r["rank"])
    if not bm.same_bits(r["median"], ref) or not bm.same_bits(r["sigma"][3], ref):
        bad("median", r["median"], r["sigma"][3], ref)
    want = bm.sigma_block(ref, n)
    for i in range(3):
        if not _close(r["sigma"][i], want[i], 2e-15):          # seven correctly rounded operations
            bad("sigma[%d]" % i, r["sigma"][i], want[i])
    if ref > 0 and n == 3 and r["sigma"][0] != np.inf:
        bad("n = 3: sigma^2 is infinite", r["sigma"][0])
    if ref > 0 and n in (1, 2) and not (np.isfinite(r["sigma"][0]) and _close(r["sigma"][0], (1.345 * (1.4826 * math.sqrt(ref))) ** 2, 2e-15)):
        bad("n = 1, 2: the wrapped denominator", r["sigma"][0])
    if ref == 0 and n != 3 and not (r["sigma"][0] == 0.0 and r["sigma"][1] == bm.MIN_SIGMA_SQ and r["sigma"][2] == 0.5):
        bad("min_sigma_sq floor", list(r["sigma"]))
    # robust chi2: the route's own sum is the separate kernels' bit for bit, and both are the exactly rounded sum to 1e-13
    if not bm.same_bits(r["robust_chi2"], r["robust_chi2_plain"]) and not (np.isnan(r["robust_chi2"]) and np.isnan(r["robust_chi2_plain"])):
        bad("robust chi2: route vs k_robust_sum + k_final_sums", r["robust_chi2"], r["robust_chi2_plain"])
    exact = bm.robust_chi2(p.x, r["sigma"])
    if not _close(r["robust_chi2_plain"], exact, 1e-13):
        bad("robust chi2 vs fsum", r["robust_chi2_plain"], exact)
    if np.isinf(p.x).any() and n != 3 and r["robust_chi2"] != np.inf:
        bad("robust chi2 of a population holding inf", r["robust_chi2"])
    # what the host learns
    written = r["route_sigma"].view(np.uint64) != np.uint64(SENTINEL)
    if route == "ahead":
        if r["head_status"] != md["status"] or r["declined"] != (md["status"] == 2):
            bad("head status", r["head_status"], md["status"])
        if md["status"] == 2 and written.any():
            bad("a head that declined wrote its sigma block", list(r["route_sigma"]))
        if md["status"] == 1 and not np.array_equal(r["route_sigma"].view(np.uint64), r["sigma"].view(np.uint64)):
            bad("the head's sigma block", list(r["route_sigma"]))
    else:
        if r["head_status"] != 0 or written.any():
            bad("head status of a route without a head", r["head_status"])
    if route == "ranks" and (r["overflow"] != int(md["overflow"]) or r["n_median_fast"] != 0):
        bad("overflow flag", r["overflow"], md["overflow"])
    if route == "ride":
        if r["pred_ok"] != int(md["pred_ok"]) or r["overflow"] != int(md["overflow"]):
            bad("prediction held / overflow", r["pred_ok"], r["overflow"], md["pred_ok"], md["overflow"])
        if r["n_median_fast"] != int(md["fast"]) or r["declined"] != int(not md["fast"]):
            bad("n_median_fast", r["n_median_fast"], md["fast"])
        if not md["fast"] and r["select_overflow"] != int(md["select_overflow"]):
            bad("overflow flag of the selection behind a declined ride", r["select_overflow"], md["select_overflow"])
    if route in ("plain", "small", "large") and (r["overflow"] != -1 or r["pred_ok"] != -1 or r["n_median_fast"] != 0 or r["declined"]):
        bad("host-visible fields of a route that reports none", r["overflow"], r["pred_ok"], r["n_median_fast"], r["declined"])


def _run(route, n):
    """every population of (route, n) on the cached handle, in list order (clusters of cap - 1, cap, cap + 1 follow each other: tables
    that overflow alternate with tables that hold); -> ({name: (median bits, sigma bytes)}, failures)"""
    if (route, n) not in _results:
        g = _handle(ROUTE_ENV[route], n)
        out, fails = {}, []
        for p in bm.populations(n, route):
            r = g.DebugHead(route, p.x, p.prev_median)
            _check(route, n, p, r, fails)
            out[p.name] = (np.float64(r["median"]).view(np.uint64), r["sigma"].tobytes())
        _results[(route, n)] = (out, fails)
    return _results[(route, n)]


def _routes_of(n):
    rs = ["plain"] + (["small"] if n <= bm.SMALL_MEAS else ["ahead", "large"])
    return rs + (["ranks", "ride"] if n in MULTI_COUNTS else [])


CASES = [(r, n) for n in bm.SMALL_COUNTS + bm.LARGE_COUNTS for r in _routes_of(n)]


@pytest.mark.parametrize("route,n", CASES, ids=["%s-%d" % c for c in CASES])
def test_route_takes_the_exact_median_of_hard_populations(gpu_required, route, n):
    """Per route x measurement count x population: median bit for bit, sigma block to 2e-15 (with the n = 1, 2 wrap, the n = 3 infinity
    and the min_sigma_sq floor), robust chi2 bit-identical to the separate kernels and within 1e-13 of math.fsum, and the host-visible
    outcome (head status, overflow flags, prediction held, n_median_fast) equal to the model's.  A route that declines (ahead with
    status 2, ride with the prediction missed or the table overflowed) is seen to decline, to have written no sigma block, and the
    plain selection behind it gives the right element."""
    out, fails = _run(route, n)
    assert len(out) >= 25
    assert not fails, fails[:12]


@pytest.mark.parametrize("n", bm.SMALL_COUNTS + bm.LARGE_COUNTS)
def test_median_and_sigma_block_are_bit_identical_across_routes(gpu_required, n):
    routes = _routes_of(n)
    res = {r: _run(r, n)[0] for r in routes}
    base = res["plain"]
    compared = 0
    for r in routes[1:]:
        for name, v in res[r].items():
            if name in base:
                assert v == base[name], (r, n, name)
                compared += 1
    assert compared >= 25 * (len(routes) - 1)


@pytest.mark.parametrize("route,n", [("plain", 70001), ("ranks", 32769), ("ride", 32769), ("small", 32768), ("ahead", 32769), ("large", 32769)])
def test_second_call_on_a_handle_finds_the_counters_zeroed(gpu_required, route, n):
    """The routes leave their counters zero for the next use (hist_clean, headl_clean, k_head_finish's re-arming): a stale counter
    shows only on the NEXT call, so populations that overflow a table alternate with ones that do not, twice round."""
    g = _handle(ROUTE_ENV[route], n)
    pops = {p.name: p for p in bm.populations(n, route)}
    cap = bm.CAPS[route][-1]
    order = ["cluster_distinct_%d" % (cap + 1), "lognormal", "cluster_equal_%d" % (cap + 1), "cluster_distinct_%d" % (cap - 1), "all_equal",
             "prev_far_above", "cluster_distinct_%d" % (cap + 1), "prev_two_below", "all_zero", "cluster_equal_%d" % cap, "binades60"]
    fails = []
    for rnd in range(2):
        for name in order:
            _check(route, n, pops[name], g.DebugHead(route, pops[name].x, pops[name].prev_median), fails)
    assert not fails, fails[:12]


def test_routes_the_handle_is_not_configured_for_are_refused_by_name(gpu_required):
    big, small, multi = _handle("single", 32769), _handle("single", 1025), _handle("multi", 1025)
    x = np.ones(32769)
    for g, m, route in ((big, 32769, "small"), (big, 32769, "ranks"), (big, 32769, "ride"), (small, 1025, "ahead"), (small, 1025, "large"),
                        (small, 1025, "ranks"), (multi, 1025, "plain"), (multi, 1025, "small"), (multi, 1025, "ahead"), (multi, 1025, "large")):
        with pytest.raises(RuntimeError, match="route %s refused" % route):
            g.DebugHead(route, x[:m], 1.0)
    with pytest.raises(RuntimeError, match="chi2 holds 1024 values, the handle has 1025 measurements"):
        small.DebugHead("small", x[:1024], 1.0)
    # ... and a refusal enqueues nothing: the next call is as right as any
    fails = []
    p = bm.populations(1025, "small")[0]
    _check("small", 1025, p, small.DebugHead("small", p.x, p.prev_median), fails)
    assert not fails, fails


def test_compute_after_hook_calls_gives_the_bytes_of_a_fresh_handle(gpu_required):
    """The hook overwrites chi2, the prediction and the sigma block -- all of which Compute() recomputes -- and leaves poses and points
    alone: a solve after a series of hook calls equals the solve of a fresh handle in every byte."""
    import ba_shapes
    from helpers import run_bundle, collect
    from mcptam_amd import chain_bundle
    p = ba_shapes.get_map("pts129")
    fresh = run_bundle(chain_bundle.ChainBundle(p.cams, True, True, False, disable_convergence=True), p, 6)
    for kind in ("single", "multi"):
        with _env(ENVS[kind]):
            g = chain_bundle.ChainBundle(p.cams, True, True, False, disable_convergence=True)
            ids = p.populate(g)
            if kind == "multi":
                g.SetAllReduce(lambda ptr, count, stream: None, 0, 1)
            g.Prepare()
        n = p.n_meas
        R0, t0, X0 = collect(g, ids)
        for route in (("small", "plain") if kind == "single" else ("ranks", "ride")):
            fails = []
            for q in bm.populations(n, route):
                _check(route, n, q, g.DebugHead(route, q.x, q.prev_median), fails)
            assert not fails, fails[:12]
        R1, t1, X1 = collect(g, ids)
        assert np.array_equal(R0, R1) and np.array_equal(t0, t1) and np.array_equal(X0, X1)
        rc = g.Compute(6)
        R, t, X = collect(g, ids)
        assert rc == fresh["rc"] == 6 and g.IterLogs() == fresh["logs"]
        assert R.tobytes() == fresh["R"].tobytes() and t.tobytes() == fresh["t"].tobytes() and X.tobytes() == fresh["X"].tobytes()
        assert g.GetSigmaSquared() == fresh["sigma_sq"] and g.GetOutlierMeasurements() == fresh["outliers"]


def test_ba_select_unit_against_sort(gpu_required, tmp_path):
    """The building blocks of csrc/ba_select.h alone (tests/cpp/ba_select_check.hip): block_find_rank, sel_find_bin, lds_find_bin and
    lds_radix_select in kernels of their own, and the full chain k_select_pass x 6 + k_select_final on grids of 1, 2 and 1024
    workgroups, against std::sort / std::nth_element."""
    exe = str(tmp_path / "ba_select_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-I", os.path.join(ROOT, "mcptam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ba_select_check.hip"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("ok "), out.stdout[-3000:] + out.stderr[-500:]
    print(out.stdout.strip().splitlines()[-1])
