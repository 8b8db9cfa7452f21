"""Parity of the HIP ChainBundle path (through the C ABI) against the CPU oracle, on a real MI355X."""
import numpy as np
import pytest

from helpers import compare_runs, rel_err, rel_err_elem, run_bundle

pytestmark = pytest.mark.gpu


def _gpu(cams, **kw):
    from mcptam_amd.chain_bundle import ChainBundle
    return ChainBundle(cams, kw.pop("robust", True), kw.pop("tukey", True), kw.pop("verbose", False), **kw)


def _orc(cams, robust=True, tukey=True, verbose=False):
    from oracle import OracleBundle
    return OracleBundle(cams, robust, tukey, verbose)


@pytest.mark.parametrize("cfg", ["tiny", "c1", "c2small"])
def test_eval_and_sigma_match_oracle(gpu_required, cfg):
    from mcptam_amd import synth
    p = synth.make_config("c2", n_mkf=12, n_points=1500) if cfg == "c2small" else synth.make_config(cfg)
    g, o = _gpu(p.cams), _orc(p.cams)
    p.populate(g)
    p.populate(o)
    n = g.Prepare()
    assert n == o.Prepare()
    chi_g, err_g = g.Eval(p.n_meas)
    chi_o, err_o = o.Eval()
    assert rel_err(err_g, err_o) < 1e-10
    assert rel_err(chi_g, chi_o) < 1e-10
    cg, sg = g.DebugRobustChi2()
    co, so = o.DebugRobustChi2()
    assert abs(sg - so) <= 1e-12 * so          # the median is an exact element
    assert abs(cg - co) <= 1e-11 * co


@pytest.mark.parametrize("cfg", ["tiny", "c1", "c2small"])
def test_normal_equations_solution_matches_oracle(gpu_required, cfg):
    from mcptam_amd import synth
    p = synth.make_config("c2", n_mkf=12, n_points=1500) if cfg == "c2small" else synth.make_config(cfg)
    g, o = _gpu(p.cams), _orc(p.cams)
    p.populate(g)
    p.populate(o)
    for lam in (1e-3, 10.0):
        xg = g.DebugSolve(lam)
        rc, xs, xd = o.DebugSolve(lam)
        assert rc == 0
        assert rel_err(xg, xs) < 1e-7, (cfg, lam)


@pytest.mark.parametrize("cfg,iters", [("tiny", 15), ("c1", 25), ("c2small", 12)])
def test_compute_matches_oracle(gpu_required, cfg, iters):
    from mcptam_amd import synth
    p = synth.make_config("c2", n_mkf=12, n_points=1500) if cfg == "c2small" else synth.make_config(cfg)
    gpu = run_bundle(_gpu(p.cams), p, iters)
    ref = run_bundle(_orc(p.cams), p, iters)
    rep = compare_runs(gpu, ref)
    assert rep["branch_flips"] == 0
    assert gpu["outliers"] == ref["outliers"]
    assert abs(gpu["sigma_sq"] - ref["sigma_sq"]) <= 1e-6 * ref["sigma_sq"]
    assert abs(gpu["mean_chi2"] - ref["mean_chi2"]) <= 1e-6 * ref["mean_chi2"]
    assert abs(gpu["lam"] - ref["lam"]) <= 1e-6 * ref["lam"]


def test_c2_full_size_matches_oracle(gpu_required):
    """BASELINE config c2: 4 cameras, 50 MKF, 10k points, 80k measurements."""
    from mcptam_amd import synth
    p = synth.make_config("c2")
    assert p.n_meas == 80000
    gpu = run_bundle(_gpu(p.cams), p, 8)
    ref = run_bundle(_orc(p.cams), p, 8)
    rep = compare_runs(gpu, ref)
    assert rep["branch_flips"] == 0
    assert gpu["outliers"] == ref["outliers"]


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 64, 65, 100, 1194])
def test_dense_cholesky_solve_matches_numpy(gpu_required, n):
    """ba_chol.h (MFMA tile updates, in-register panel factor, fused forward solve) against numpy."""
    from mcptam_amd.chain_bundle import dense_spd_solve
    rng = np.random.default_rng(n)
    B = rng.normal(size=(n, n))
    A = B @ B.T + n * np.eye(n)
    b = rng.normal(size=n)
    x = dense_spd_solve(np.tril(A), b)          # only the lower triangle is read
    ref = np.linalg.solve(A, b)
    err = rel_err(x, ref)
    assert err < 1e-11, (n, err, int(np.argmax(np.abs(x - ref))))
    with pytest.raises(RuntimeError):
        dense_spd_solve(-A, b)                  # not positive definite -> loud failure


def test_zero_noise_recovers_ground_truth(gpu_required):
    from mcptam_amd import synth
    p = synth.make_config("c2", n_mkf=16, n_points=2000, noise=False)
    gpu = run_bundle(_gpu(p.cams), p, 40)
    assert gpu["rc"] > 0 and gpu["converged"]
    assert np.abs(gpu["R"] - p.true_base_R).max() < 1e-9
    assert np.abs(gpu["t"] - p.true_base_t).max() < 1e-8
    assert gpu["mean_chi2"] < 1e-12


def test_non_robust_and_verbose_modes(gpu_required):
    from mcptam_amd import synth
    p = synth.make_config("tiny", n_points=120)
    for robust, verbose in ((False, False), (True, True)):
        gpu = run_bundle(_gpu(p.cams, robust=robust, tukey=True, verbose=verbose), p, 10)
        ref = run_bundle(_orc(p.cams, robust, True, verbose), p, 10)
        compare_runs(gpu, ref)
        assert gpu["outliers"] == ref["outliers"]


def test_more_free_poses_than_the_reduced_solver_takes_is_an_error_not_a_wrong_answer(gpu_required):
    """include/mcp_ba.h, MCP_BA_MAX_FREE_POSES: the reduced system is dense in tiles with its solution vector in LDS, so 6 P <= 6144.
    A map with more free poses (the reference has no such limit: CHOLMOD goes on, src/ChainBundle.cc:1150-1158) must come back as an
    error with a message that says so -- from Prepare() and from Compute() -- and one pose less must still solve."""
    from mcptam_amd import synth
    for n_free, ok in ((1025, False), (1024, True)):
        p = synth.make_problem(n_cams=4, n_mkf=n_free + 1, n_points=3000, per_point=4, mode="multi", outlier_frac=0.0)
        assert int((~p.base_fixed).sum()) == n_free
        g = _gpu(p.cams, disable_convergence=True)
        p.populate(g)
        if ok:
            assert g.Prepare() == 6 * n_free + 3 * p.n_points
            assert g.Compute(2) == 2
        else:
            with pytest.raises(RuntimeError, match="too many free poses"):
                g.Prepare()
            with pytest.raises(RuntimeError, match="too many free poses"):
                g.Compute(2)
        g.close()


def test_fixed_points_and_single_chain(gpu_required):
    """Calibration-style fixed points use the chain {world} and chi2 < 0 forces weight 1 (ChainBundle.cc:401-417)."""
    from mcptam_amd import synth
    p = synth.make_config("c1", n_fixed_points=40)
    g, o = _gpu(p.cams), _orc(p.cams)
    p.populate(g)
    p.populate(o)
    chi_g, _ = g.Eval(p.n_meas)
    chi_o, _ = o.Eval()
    assert (chi_g < 0).sum() == (chi_o < 0).sum() > 0
    gpu = run_bundle(_gpu(p.cams), p, 12)
    ref = run_bundle(_orc(p.cams), p, 12)
    compare_runs(gpu, ref)
    fixed = p.pt_fixed
    assert np.array_equal(gpu["X"][fixed], p.pt_x[fixed])      # fixed points never move


def test_all_poses_fixed_and_small_cov(gpu_required):
    """Fewer than 3 free poses: the depth-covariance median is produced (ChainBundle.cc:1419-1437)."""
    from mcptam_amd import synth
    p = synth.make_config("tiny", n_mkf=3, n_points=80, n_fixed_mkf=1, per_point=3)
    gpu = run_bundle(_gpu(p.cams), p, 10)
    ref = run_bundle(_orc(p.cams), p, 10)
    compare_runs(gpu, ref)
    assert ref["max_cov"] > 0
    assert abs(gpu["max_cov"] - ref["max_cov"]) <= 1e-6 * ref["max_cov"]
    q = synth.make_config("tiny", n_mkf=3, n_points=80, n_fixed_mkf=3, per_point=3)      # points only
    gpu = run_bundle(_gpu(q.cams), q, 10)
    ref = run_bundle(_orc(q.cams), q, 10)
    compare_runs(gpu, ref)
    assert abs(gpu["max_cov"] - ref["max_cov"]) <= 1e-6 * max(ref["max_cov"], 1e-300)


def test_abort_flag_and_two_step(gpu_required):
    from mcptam_amd import synth
    p = synth.make_config("c1")
    g = _gpu(p.cams)
    p.populate(g)
    g.abort.value = 1
    assert g.Compute(10) == 0                  # aborted before any step (ChainBundle.cc:1365-1366)
    g.abort.value = 0
    # two-step mode (BundleAdjusterMulti.cc:210-224): 10 iterations, then to convergence on the same object
    g2, g3, o2 = _gpu(p.cams), _gpu(p.cams), _orc(p.cams)
    ids = p.populate(g2)
    p.populate(g3)
    p.populate(o2)
    a, a3, b = g2.Compute(10), g3.Compute(10), o2.Compute(10)
    assert a == a3 == b == 10
    if not g2.Converged():
        for h in (g2, g3, o2):
            h.abort.value = 0
        a, a3, b = g2.Compute(), g3.Compute(), o2.Compute()
        assert a > 0 and b > 0
        # two device runs are the same run: same stopping iteration, same log, bit for bit (fixed accumulation order)
        assert a == a3 and g2.IterLogs() == g3.IterLogs()
        # device vs oracle: the stopping test (0 <= dchi2/chi2 <= 1e-10, ChainBundle.cc:1101) compares numbers that agree
        # to ~1e-13 relative between the two arithmetic orders, so at the flat end of the descent the two may stop
        # some iterations apart (observed: 77 vs 70); they must agree while chi2 still moves and land on the same state
        lg, lo = g2.IterLogs(), o2.IterLogs()
        for x, y in zip(lg[:3], lo[:3]):
            assert (x["trials"], x["accepted"]) == (y["trials"], y["accepted"])
            assert abs(x["chi2_start"] - y["chi2_start"]) <= 1e-9 * y["chi2_start"]
        assert abs(lg[-1]["chi2_end"] - lo[-1]["chi2_end"]) <= 1e-9 * lo[-1]["chi2_end"]
    Rg, tg = g2.GetPoses(ids["mkf"])
    R3, t3 = g3.GetPoses(ids["mkf"])
    assert np.array_equal(Rg, R3) and np.array_equal(tg, t3)
    Ro = np.array([o2.GetPose(int(i))[0] for i in ids["mkf"]])
    assert rel_err_elem(Rg, Ro) < 1e-6


def test_empty_and_degenerate_inputs(gpu_required):
    from mcptam_amd import synth
    p = synth.make_config("tiny")
    g = _gpu(p.cams)
    assert g.Compute(5) == -1                  # nothing to optimise: the reference returns -1 (:1362-1363)
    g = _gpu(p.cams)
    a = g.AddPose(np.eye(3), np.zeros(3), True)
    with pytest.raises(RuntimeError):
        g.AddPoint(np.ones(3), [a + 7], False)                  # unknown pose id in the chain
    pid = g.AddPoint(np.array([0.1, 0.2, 3.0]), [a], False)
    with pytest.raises(RuntimeError):
        g.AddMeas([a], pid + 5, np.zeros(2), 1.0, 0)            # unknown point id
    with pytest.raises(RuntimeError):
        g.AddMeas([a], pid, np.zeros(2), 1.0, 9)                # unknown camera


def test_metric_size_properties(gpu_required):
    """BASELINE metric configuration (4-cam, 200 MKF, 50k points, 400k measurements): size-independent
    properties -- zero-noise recovery of the true trajectory and exactness of the selected median."""
    from mcptam_amd import synth
    p = synth.make_config("metric", noise=False)
    assert p.n_meas == 400000 and p.n_points == 50000
    g = _gpu(p.cams)
    ids = p.populate(g)
    chi2, _ = g.Eval(p.n_meas)
    _, s_raw = g.DebugRobustChi2()
    med = np.sort(np.abs(chi2))[p.n_meas // 2]
    expect = (1.345 * 1.4826 * (1 + 5.0 / (2 * p.n_meas - 6)) * np.sqrt(med)) ** 2
    assert abs(s_raw - expect) <= 1e-12 * expect
    rc = g.Compute(30)
    assert rc > 0 and g.Converged()
    R, t = g.GetPoses(ids["mkf"])
    assert np.abs(R - p.true_base_R).max() < 1e-8
    assert np.abs(t - p.true_base_t).max() < 1e-7
    logs = g.IterLogs()
    chis = [l["chi2_end"] for l in logs if l["accepted"]]
    assert chis[-1] < 1e-10 * logs[0]["chi2_start"]


def test_point_seen_from_many_poses_uses_generic_path(gpu_required):
    """A point observed from more than 16 free poses cannot live in a 16-pose group tile and is
    routed through the generic (global atomic) kernels; results must not change."""
    from mcptam_amd import synth
    p = synth.make_config("c2", n_mkf=30, n_points=300, per_point=24, k_near=30, radius=2.0)
    g, o = _gpu(p.cams), _orc(p.cams)
    p.populate(g)
    p.populate(o)
    xg = g.DebugSolve(1e-2)
    rc, xs, _ = o.DebugSolve(1e-2)
    assert rc == 0 and rel_err(xg, xs) < 1e-7
    gpu = run_bundle(_gpu(p.cams), p, 8)
    ref = run_bundle(_orc(p.cams), p, 8)
    compare_runs(gpu, ref)


@pytest.mark.parametrize("layout", ["auto", "large"])
def test_calibration_chain_shapes(gpu_required, layout, monkeypatch):
    """BundleAdjusterCalib's problem (src/BundleAdjusterCalib.cc:118-219): free relative camera poses that sit as the
    *second* link of every chain of that camera (a dense block row of the reduced system), chains of length 1 for the
    first camera, fixed board points on a world chain, Compute(abort, 10).  layout "large": the kernels of a large map (groups of
    64 points, k_linearize_pipe with its deferred W blocks -- here one pose vertex sits at two positions of an edge, i.e. two slots
    of one measurement feed the same block) instead of the quarter-size groups a map of 600 points gets."""
    from mcptam_amd import synth
    if layout == "large":
        monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")
    p = synth.make_config("calib")
    g, o = _gpu(p.cams), _orc(p.cams)
    p.populate(g)
    p.populate(o)
    for lam in (1e-3, 10.0):
        xg = g.DebugSolve(lam)
        rc, xs, xd = o.DebugSolve(lam)
        assert rc == 0 and rel_err(xg, xs) < 1e-7
    gpu = run_bundle(_gpu(p.cams), p, 10)
    ref = run_bundle(_orc(p.cams), p, 10)
    rep = compare_runs(gpu, ref)
    assert rep["branch_flips"] == 0
    # the calibrated relative poses (what CalibrateAndUpdate writes back) agree, and moved towards the truth
    for c in range(1, len(p.cams)):
        Rg, tg = _pose(gpu, p, c)
        Rr, tr = _pose(ref, p, c)
        assert rel_err_elem(Rg, Rr) < 1e-6 and rel_err_elem(tg, tr) < 1e-6
        Rt = p.cam_R[c] @ p.cam_R[0].T
        tt = p.cam_t[c] - Rt @ p.cam_t[0]
        # (ten iterations with g2o's one-sided block for the doubly-present relative pose, DESIGN.md 2: slower than the complete
        # Gauss-Newton block, which covered three quarters of the way in the same ten iterations)
        assert np.abs(tg - tt).max() < 0.5 * np.abs(p.rel_t[c] - tt).max()


def _pose(run, p, c):
    return run["cam_R"][c], run["cam_t"][c]


def test_two_rank_sharded_solve_equals_merged_single_rank(gpu_required):
    """points/measurements sharded over ranks, poses replicated, reduced pose system summed with
    the all-reduce hook.  Two processes share this GPU and reduce through gloo; the result must equal the
    single-rank solve of the merged map."""
    import os
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import dist_workers
    from mcptam_amd import synth
    cfg = dict(name="c2", n_mkf=16, n_points=1200)
    iters = 6
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(dist_workers.sharded_solve_on_one_gpu, args=(2, port, d, cfg, iters), nprocs=2, join=True)
        r0, r1 = np.load(os.path.join(d, "shard_0.npz")), np.load(os.path.join(d, "shard_1.npz"))
    merged = synth.merge_shards([synth.make_config(shard=0, **cfg), synth.make_config(shard=1, **cfg)])
    ref = run_bundle(_gpu(merged.cams), merged, iters)
    assert int(r0["rc"]) == int(r1["rc"]) == ref["rc"]
    assert np.array_equal(r0["R"], r1["R"]) and np.array_equal(r0["t"], r1["t"])        # replicas stay bit-identical
    assert rel_err_elem(r0["R"], ref["R"]) < 1e-8 and rel_err_elem(r0["t"], ref["t"]) < 1e-8
    n0 = r0["X"].shape[0]
    assert rel_err_elem(r0["X"], ref["X"][:n0]) < 1e-8 and rel_err_elem(r1["X"], ref["X"][n0:]) < 1e-8
    logs = np.array([[l["chi2_start"], l["chi2_end"], l["lambda_end"], l["sigma_sq"], l["trials"], l["accepted"]] for l in ref["logs"]])
    assert np.allclose(r0["logs"], logs, rtol=1e-9)
    assert abs(float(r0["sigma_sq"]) - ref["sigma_sq"]) <= 1e-12 * ref["sigma_sq"]        # global median is exact
    assert int(r0["n_out"]) + int(r1["n_out"]) == len(ref["outliers"])
    # the multi-rank solve is the single-rank machine: speculative systems + trials ahead on the second lane, and the collective
    # budget of DESIGN.md 6 -- per iteration one packed-tile all-reduce per solve and lane, one block per trial, one gather per median
    for r in (r0, r1):
        assert int(r["coll_spec"]) > 0, "no collective on the speculative lane: the second stream is off"
        assert int(r["median_fast"]) >= iters - 2, "the medians should ride on the accepted trials' all-reduces"
        # main lane: prepare 2, first iteration 6 (three-collective median, start chi2, pose diagonal, lambda), final statistics <= 4;
        # then per iteration ONE for the median (three if its prediction missed) and per solve TWO (packed tiles, the trial's block)
        slow = max(0, iters - 1 - int(r["median_fast"]))
        assert int(r["coll_main"]) <= 12 + (iters - 1) + 2 * slow + 2 * int(r["solves"]), (int(r["coll_main"]), int(r["solves"]), int(r["median_fast"]))
        assert int(r["solves"]) <= iters + 1
    assert int(r0["coll_main"]) == int(r1["coll_main"]) and int(r0["coll_spec"]) == int(r1["coll_spec"])


def _logs_array(logs):
    return np.array([[l["chi2_start"], l["chi2_end"], l["lambda_end"], l["sigma_sq"], l["trials"], l["accepted"]] for l in logs])


def test_forced_multi_rank_machine_with_identity_hook_is_bit_identical(gpu_required, monkeypatch):
    """MCP_BA_FORCE_MULTI=1 drives a ONE-rank solve through everything a multi-rank solve does (packed tiles, both lanes, trial
    blocks + riding median histograms + k_trial_post, slot-table gather); the hook sums over one rank, i.e. changes nothing, so
    logs, poses and points must equal the plain single-rank solve bit for bit -- on the noisy metric map, whose iterations reject."""
    from mcptam_amd import synth
    p = synth.make_config("metric")
    base = run_bundle(_gpu(p.cams, disable_convergence=True), p, 7)
    monkeypatch.setenv("MCP_BA_FORCE_MULTI", "1")
    calls = []
    g = _gpu(p.cams, disable_convergence=True)
    g.SetAllReduce(lambda ptr, count, stream: calls.append(count), 0, 1)
    alt = run_bundle(g, p, 7)
    tm = g.Timing()
    assert base["rc"] == alt["rc"] == 7 and sum(l["trials"] for l in base["logs"]) > 10
    assert base["logs"] == alt["logs"]
    assert np.array_equal(base["R"], alt["R"]) and np.array_equal(base["t"], alt["t"]) and np.array_equal(base["X"], alt["X"])
    assert base["outliers"] == alt["outliers"] and base["sigma_sq"] == alt["sigma_sq"] and base["lam"] == alt["lam"]
    assert tm["n_collectives_spec"] > 0 and tm["n_median_fast"] >= 5 and len(calls) == tm["n_collectives_main"] + tm["n_collectives_spec"]
    # the riding histograms can be switched off (three-collective medians): same numbers
    monkeypatch.setenv("MCP_BA_SELECT_RIDE", "0")
    g2 = _gpu(p.cams, disable_convergence=True)
    g2.SetAllReduce(lambda ptr, count, stream: None, 0, 1)
    alt2 = run_bundle(g2, p, 7)
    assert g2.Timing()["n_median_fast"] == 0
    assert base["logs"] == alt2["logs"] and np.array_equal(base["X"], alt2["X"])
    # ... and a gather table too small for the selected bin sends every median down the remaining-digits path
    monkeypatch.setenv("MCP_BA_SELECT_RIDE", "1")
    monkeypatch.setenv("MCP_BA_SELECT_CAP", "1")
    g3 = _gpu(p.cams, disable_convergence=True)
    g3.SetAllReduce(lambda ptr, count, stream: None, 0, 1)
    alt3 = run_bundle(g3, p, 7)
    assert g3.Timing()["n_median_fast"] == 0
    assert base["logs"] == alt3["logs"] and np.array_equal(base["X"], alt3["X"])


@pytest.mark.timeout(300)
def test_forced_multi_rank_machine_on_native_rccl_lanes(gpu_required):
    """The same on the real transport: a one-rank RCCL communicator with its two lanes (ncclCommSplit), all-reduces enqueued on
    the solver's two streams, no host synchronisation inside the LM loop."""
    import os
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import dist_workers
    from mcptam_amd import synth
    cfg = dict(name="c2")
    iters = 8
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(dist_workers.forced_multi_native_rccl, args=(1, port, d, cfg, iters), nprocs=1, join=True)
        r = np.load(os.path.join(d, "forced.npz"))
    assert np.array_equal(r["t"], np.arange(4096) * 0.25)
    p = synth.make_config(**cfg)
    ref = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    assert int(r["rc"]) == ref["rc"] == iters
    assert np.array_equal(r["logs"], _logs_array(ref["logs"]))
    assert np.array_equal(r["R"], ref["R"]) and np.array_equal(r["tt"], ref["t"]) and np.array_equal(r["X"], ref["X"])
    assert int(r["coll_spec"]) > 0 and int(r["median_fast"]) >= iters - 2


@pytest.mark.timeout(300)
def test_watchdog_bounds_a_stalled_collective(gpu_required):
    """A rank that never arrives leaves the others' streams stuck behind a collective.  Simulated with a hook that parks a
    long sleep kernel on the solver's stream: the solve must come back with MCP_BA_ERR_RUNTIME and say where it waited
    (worker process: torch has to own the HIP runtime it launches the sleep kernel with)."""
    import os
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import dist_workers
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(dist_workers.watchdog_stall, args=(1, port, d), nprocs=1, join=True)
        r = np.load(os.path.join(d, "watchdog.npz"))
    msg = str(r["msg"])
    assert "no progress within" in msg and "rank 0 of 1" in msg and "lane" in msg, msg
    assert float(r["seconds"]) < 30.0


def test_rccl_hook_on_device_buffer(gpu_required):
    """The production all-reduce hook (torch.distributed backend nccl == RCCL) on a 1-rank group."""
    import os
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import dist_workers
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(dist_workers.rccl_hook_single_rank, args=(1, port, d), nprocs=1, join=True)
        r = np.load(os.path.join(d, "rccl.npz"))
    assert np.array_equal(r["t"], np.arange(5000) * 0.5) and int(r["calls"]) == 2


def test_c4_size_single_rank_properties(gpu_required):
    """BASELINE config c4 map (4-cam, 500 MKF, 100k points, 800k measurements) on one GPU: the 2994-unknown reduced
    system (94 block steps) converges to the noise-free ground truth."""
    from mcptam_amd import synth
    p = synth.make_config("c4", noise=False)
    assert p.n_meas == 800000 and p.n_mkf == 500
    g = _gpu(p.cams)
    ids = p.populate(g)
    rc = g.Compute(25)
    assert rc > 0 and g.Converged()
    R, t = g.GetPoses(ids["mkf"])
    assert np.abs(R - p.true_base_R).max() < 1e-8 and np.abs(t - p.true_base_t).max() < 1e-7


def test_c4_size_with_noise_matches_the_oracle_and_repeats_bit_for_bit(gpu_required):
    """The c4 map WITH measurement noise and outliers (800 k measurements, 2994-unknown reduced system, 94 block steps): the first LM
    iterations against the oracle (Schur path of oracle/ba_baseline.inc, one thread: the same numbers as the oracle proper to 1e-12) --
    same accept / reject sequence, chi2, lambda, state -- and a second GPU run identical to the first bit for bit."""
    from mcptam_amd import synth
    p = synth.make_config("c4")
    iters = 2
    a = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    b = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    assert a["logs"] == b["logs"] and np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["X"], b["X"])
    o = _orc(p.cams); o.DisableConvergence(True); o.SetSolver(2, 1)
    ref = run_bundle(o, p, iters)
    assert [l["trials"] for l in a["logs"]] == [l["trials"] for l in ref["logs"]] and [l["accepted"] for l in a["logs"]] == [l["accepted"] for l in ref["logs"]]
    for x, y in zip(a["logs"], ref["logs"]):
        assert abs(x["chi2_end"] - y["chi2_end"]) <= 1e-9*abs(y["chi2_end"]) and abs(x["lambda_end"] - y["lambda_end"]) <= 1e-9*y["lambda_end"]
        assert abs(x["sigma_sq"] - y["sigma_sq"]) <= 1e-9*y["sigma_sq"]
    assert rel_err_elem(a["R"], ref["R"]) < 1e-6 and rel_err_elem(a["t"], ref["t"]) < 1e-6 and rel_err_elem(a["X"], ref["X"]) < 1e-6
    assert a["outliers"] == ref["outliers"]


def test_native_rccl_communicator_single_rank(gpu_required):
    import os
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import dist_workers
    from mcptam_amd import synth
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(dist_workers.native_rccl_single_rank, args=(1, port, d), nprocs=1, join=True)
        r = np.load(os.path.join(d, "native.npz"))
    assert np.array_equal(r["t"], np.arange(4096) * 0.25)
    p = synth.make_config("tiny")
    ref = run_bundle(_gpu(p.cams), p, 8)
    assert int(r["rc"]) == ref["rc"]
    assert rel_err_elem(r["R"], ref["R"]) < 1e-9 and rel_err_elem(r["X"], ref["X"]) < 1e-9


@pytest.mark.parametrize("name", ["tiny", "c1", "calib"])
def test_gpu_matches_committed_golden_fixture(gpu_required, name):
    """The HIP path against the committed expected outputs (tests/golden/ba_*.npz, written by
    tests/golden/make_golden.py): no oracle build involved."""
    import os
    from mcptam_amd import synth
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_%s.npz" % name))
    p = synth.make_config(name)
    b = _gpu(p.cams)
    p.populate(b)
    b.Prepare()
    chi2, _ = b.Eval(p.n_meas)
    assert rel_err(chi2, g["chi2_init"]) < 1e-10
    csum, sig = b.DebugRobustChi2()
    assert abs(sig - float(g["sigma_sq_init"])) <= 1e-12 * float(g["sigma_sq_init"])
    assert abs(csum - float(g["robust_chi2_init"])) <= 1e-11 * float(g["robust_chi2_init"])
    r = run_bundle(_gpu(p.cams), p, int(g["iters"]))
    assert r["rc"] == int(g["rc"])
    logs = np.array([[l["chi2_start"], l["chi2_end"], l["lambda_end"], l["sigma_sq"], l["trials"], l["accepted"]] for l in r["logs"]])
    assert np.array_equal(logs[:, 4:], g["logs"][:, 4:])                     # same LM accept/reject sequence
    assert np.allclose(logs[:, :4], g["logs"][:, :4], rtol=1e-6, atol=0)
    assert rel_err_elem(r["R"], g["R"]) < 1e-6 and rel_err_elem(r["t"], g["t"]) < 1e-6 and rel_err_elem(r["X"], g["X"]) < 1e-6
    assert np.array_equal(np.array(r["outliers"], dtype=np.int32).reshape(-1, 3), g["outliers"])
    assert abs(r["sigma_sq"] - float(g["sigma_sq"])) <= 1e-6 * float(g["sigma_sq"])


def test_replayed_map_dump_through_the_hip_path(gpu_required, tmp_path):
    """A map in the reference's DumpToFile layout (src/MapMakerBase.cc:475-577) with the camera dump
    (src/SystemBase.cc:166-215), loaded, populated in BundleAdjusterMulti order and adjusted on the GPU: same result
    as the oracle on the same files."""
    from mcptam_amd import map_io, synth
    p = synth.make_config("c2", n_mkf=10, n_points=800)
    names = ["camera%d" % (i + 1) for i in range(len(p.cams))]
    map_io.dump_map(str(tmp_path / "map.dat"), map_io.map_from_problem(p, names), precision=17)
    map_io.dump_cameras(str(tmp_path / "cameras.dat"), dict(zip(names, p.cams)), precision=17)
    q = map_io.problem_from_map(map_io.load_map(str(tmp_path / "map.dat")), map_io.load_cameras(str(tmp_path / "cameras.dat")))
    gpu = run_bundle(_gpu(q.cams), q, 8)
    ref = run_bundle(_orc(q.cams), q, 8)
    rep = compare_runs(gpu, ref)
    assert rep["branch_flips"] == 0 and gpu["outliers"] == ref["outliers"]
    # and the adjusted map written back in the reference's own (6-digit) formatting still parses into the same map
    out = map_io.map_from_problem(q, names, state=(gpu["R"], gpu["t"], _world_points(q, gpu)))
    map_io.dump_map(str(tmp_path / "adjusted.dat"), out)
    back = map_io.load_map(str(tmp_path / "adjusted.dat"))
    assert np.allclose(back.mkf_pos, out.mkf_pos, rtol=1e-5, atol=1e-5) and len(back.ms_pt) == q.n_meas


def _world_points(q, run):
    R = np.einsum("nij,njk->nik", q.cam_R[q.pt_src[:, 1]], run["R"][q.pt_src[:, 0]])
    t = np.einsum("nij,nj->ni", q.cam_R[q.pt_src[:, 1]], run["t"][q.pt_src[:, 0]]) + q.cam_t[q.pt_src[:, 1]]
    return np.einsum("nji,nj->ni", R, run["X"] - t)


def test_speculative_solves_do_not_change_the_iteration(gpu_required, monkeypatch):
    """A trial served by a speculative system (the next lambdas of the rejection branch factored alongside the current one,
    DESIGN.md 4) must be indistinguishable from one solved on demand: same accept/reject sequence, same lambdas, same state."""
    from mcptam_amd import synth
    p = synth.make_config("c2", n_mkf=14, n_points=2000, pose_sigma=(0.2, 5.0), depth_sigma=0.2)     # rough start: rejected trials early on
    runs = {}
    for depth in ("0", "1", "3"):
        monkeypatch.setenv("MCP_BA_SPECULATE", depth)
        g = _gpu(p.cams, profile=True)
        runs[depth] = run_bundle(g, p, 9)
        runs[depth]["timing"] = g.Timing()
    base = runs["0"]
    assert base["timing"]["n_spec_hits"] == 0 and base["timing"]["n_solves"] == base["timing"]["n_trials"]
    assert sum(l["trials"] for l in base["logs"]) > len(base["logs"])            # the run does contain rejected trials
    for depth in ("1", "3"):
        r = runs[depth]
        assert r["timing"]["n_spec_hits"] > 0 and r["timing"]["n_solves"] + r["timing"]["n_spec_hits"] == r["timing"]["n_trials"]
        assert [(l["trials"], l["accepted"]) for l in r["logs"]] == [(l["trials"], l["accepted"]) for l in base["logs"]]
        assert np.allclose([l["lambda_end"] for l in r["logs"]], [l["lambda_end"] for l in base["logs"]], rtol=1e-9)
        assert rel_err_elem(r["R"], base["R"]) < 1e-9 and rel_err_elem(r["t"], base["t"]) < 1e-9 and rel_err_elem(r["X"], base["X"]) < 1e-9
        assert r["outliers"] == base["outliers"]


@pytest.mark.parametrize("layout", ["auto", "large"])
@pytest.mark.parametrize("extra_links", [0, 2, 4])
def test_long_chains_with_mixed_fixed_and_free_links(gpu_required, extra_links, layout, monkeypatch):
    """Generic pose chains (the reference accepts any length, src/ChainBundle.cc:1220-1230; here up to MCP_MAX_CHAIN = 8, any
    link fixed or free): chain {base_k, arm (free, shared by all), mount (fixed), [joints: free / fixed alternating],
    camera_c (c = 0 free, c = 1 fixed)} -- 4, 6 and 8 links.  PoseChainHelper's first/second transforms, MoveTogether's
    structural zeros and the Jacobians of inner links (src/ChainBundle.cc:120-199, 485-586) against the oracle."""
    if layout == "large":
        monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")          # (groups of 64 points: k_linearize_pipe, more than two slots per measurement)
    from mcptam_amd import synth
    from mcptam_amd.taylor_camera import TaylorCamera
    rng = np.random.default_rng(11)
    cam = TaylorCamera(synth.DEFAULT_CAM_PARAMS, (640, 480), (640, 480), (640, 480))

    def rand_pose(sr, st):
        R, t = synth.se3_exp(np.concatenate([rng.normal(size=3)*st, rng.normal(size=3)*sr]))
        return R, t

    def mul(a, b):
        return a[0] @ b[0], a[0] @ b[1] + a[1]

    nb = 6
    bases = [rand_pose(0.15, 0.4) for _ in range(nb)]
    arm, mount = rand_pose(0.05, 0.05), rand_pose(0.05, 0.05)
    cams2 = [rand_pose(0.02, 0.02), (synth.rot_z(0.3) @ np.eye(3), np.array([0.1, 0.0, 0.0]))]
    joints = [rand_pose(0.03, 0.03) for _ in range(extra_links)]          # joint j is free for even j, fixed for odd j

    def chain_T(k, c):
        T = mul(mount, mul(arm, bases[k]))
        for J in joints:
            T = mul(J, T)
        return mul(cams2[c], T)

    world = np.stack([rng.uniform(-2, 2, 400), rng.uniform(-1.5, 1.5, 400), rng.uniform(4, 9, 400)], axis=1)

    def build(bundle, perturb):
        pert = np.random.default_rng(5)                      # the same perturbation for both bundles

        def P(T, s):
            if not perturb or s == 0:
                return T
            R, t = synth.se3_exp(np.concatenate([pert.normal(size=3)*0.02*s, pert.normal(size=3)*0.01*s]))
            return R @ T[0], R @ T[1] + t
        b_id = [bundle.AddPose(*P(bases[k], 1 if k else 0), k == 0) for k in range(nb)]
        arm_id = bundle.AddPose(*P(arm, 1), False)
        mount_id = bundle.AddPose(*mount, True)
        joint_id = [bundle.AddPose(*P(J, 0.5 if j % 2 == 0 else 0), j % 2 == 1) for j, J in enumerate(joints)]
        cam_id = [bundle.AddPose(*P(cams2[0], 1), False), bundle.AddPose(*cams2[1], True)]
        pts = []
        for i, X in enumerate(world):
            k, c = i % nb, (i // nb) % 2
            R, t = chain_T(k, c)
            x = (R @ X + t) * (1.0 + (0.03*pert.normal() if perturb else 0.0))
            pts.append(bundle.AddPoint(x, [b_id[k], arm_id, mount_id] + joint_id + [cam_id[c]], False))
        nm = 0
        for i, X in enumerate(world):
            for k in range(nb):
                for c in range(2):
                    if (i + k + c) % 3 == 0:
                        continue
                    R, t = chain_T(k, c)
                    uv, inv = cam.project((R @ X + t)[None, :])
                    if inv[0]:
                        continue
                    lvl = (i + k) % 3
                    bundle.AddMeas([b_id[k], arm_id, mount_id] + joint_id + [cam_id[c]], pts[i], uv[0] + 0.3*np.array([np.sin(i + k), np.cos(i*c + 1)]), 4.0**lvl, 0)
                    nm += 1
        return b_id + [arm_id, cam_id[0]] + joint_id[::2], pts, nm

    g, o = _gpu([cam]), _orc([cam])
    ids_g, pts_g, nm = build(g, True)
    ids_o, pts_o, _ = build(o, True)
    assert nm > 2000
    # the shared free arm makes the undamped system poorly conditioned (the oracle's own two solvers differ by 2e-6 at
    # lambda = 1e-3, 2e-9 at lambda = 1): compare where the arithmetic, not the conditioning, is what is measured
    for lam, tol in ((1.0, 1e-7), (100.0, 1e-9)):
        xg = g.DebugSolve(lam)
        rc, xs, xd = o.DebugSolve(lam)
        assert rc == 0 and rel_err(xs, xd) < tol and rel_err(xg, xs) < tol, (lam, rel_err(xg, xs))
    ng, no = g.Compute(8), o.Compute(8)
    assert ng == no
    lg, lo = g.IterLogs(), o.IterLogs()
    assert [l["trials"] for l in lg] == [l["trials"] for l in lo]
    assert lg[-1]["chi2_end"] < 0.5 * lg[0]["chi2_start"]
    for a, b in zip(ids_g, ids_o):
        Rg, tg = g.GetPose(a)
        Ro, to = o.GetPose(b)
        assert np.abs(Rg - Ro).max() < 1e-6 and np.abs(tg - to).max() < 1e-6
    Xg = np.array([g.GetPoint(i) for i in pts_g[:50]])
    Xo = np.array([o.GetPoint(i) for i in pts_o[:50]])
    assert rel_err_elem(Xg, Xo) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# round 2: reproducibility (fixed-order accumulation, no same-launch read/write in the factorisation) and the
# noisy BASELINE metric map against the oracle

@pytest.mark.parametrize("n,nsys,reps", [(1194, 1, 200), (1194, 4, 200), (2994, 4, 200), (70, 2, 50)])
def test_cholesky_chain_is_bit_reproducible(gpu_required, n, nsys, reps):
    """The factorisation + back-substitution launches give the same bits every time: the diagonal tile of a step is no
    longer rewritten in the launch that other workgroups read it in (ba_chol.h, side array of diagonal tiles), and the
    back-substitution combines its partial sums in a fixed order."""
    from mcptam_amd.chain_bundle import dense_spd_stress
    rng = np.random.default_rng(100 + n)
    B = rng.normal(size=(n, n))
    A = B @ B.T + n * np.eye(n)
    b = rng.normal(size=n)
    x, bad = dense_spd_stress(np.tril(A), b, nsys=nsys, reps=reps)
    assert bad == 0, "%d of %d repetitions differ from the first" % (bad, reps - 1)
    for q in range(nsys):
        ref = np.linalg.solve(A + q * np.eye(n), b)
        assert rel_err(x[q], ref) < 1e-11, (n, q)


def _plan_mask(S_gpu):
    """Entries the assembly wrote (the tiles of the factorisation plan show up as non-zero or explicit zeros; compare
    the lower triangle only)."""
    return np.tril(np.ones_like(S_gpu, dtype=bool))


@pytest.mark.parametrize("layout", ["auto", "large"])
@pytest.mark.parametrize("cfg", ["tiny", "c1", "c2small", "c2"])
def test_reduced_system_matches_oracle_and_is_reproducible(gpu_required, cfg, layout, monkeypatch):
    """S = U + lambda I - W V^-1 W^T and its right-hand side, entry by entry against the oracle's reduced system, and
    bit-identical between two independent builds (staged group blocks summed in ascending group order).  layout "large": through
    the kernels of a large map (groups of 64 points, k_linearize_pipe, four-chunk groups in k_schur4) instead of the quarter-size
    groups these maps get on their own."""
    from mcptam_amd import synth
    if layout == "large":
        monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")
    p = synth.make_config("c2", n_mkf=12, n_points=1500) if cfg == "c2small" else synth.make_config(cfg)
    o = _orc(p.cams)
    p.populate(o)
    So, ro, bo = o.DebugSystem(1e-2)
    outs = []
    for _ in range(2):
        g = _gpu(p.cams)
        p.populate(g)
        outs.append(g.DebugSystem(1e-2))
        g.close()
    Sg, rg, bg = outs[0]
    low = np.tril(np.ones_like(So, dtype=bool))
    scale = np.abs(So).max()
    assert np.abs(Sg[low] - So[low]).max() <= 1e-10 * scale
    assert rel_err(rg, ro) < 1e-9 and rel_err(bg, bo) < 1e-9
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


def test_metric_noisy_matches_oracle(gpu_required):
    """The map bench.py times -- 4 cameras, 200 MKF, 50k points, 400k noisy measurements with 2 % gross outliers --
    through 8 LM iterations: per-iteration trial counts, accept/reject, lambda, chi2 and the final state against the
    oracle (ChainBundle.cc:1305-1451)."""
    from mcptam_amd import synth
    p = synth.make_config("metric")
    assert p.n_meas == 400000 and p.n_points == 50000
    gpu = run_bundle(_gpu(p.cams, disable_convergence=True), p, 8)
    o = _orc(p.cams)
    o.DisableConvergence(True)
    ref = run_bundle(o, p, 8)
    rep = compare_runs(gpu, ref)
    assert rep["branch_flips"] == 0
    assert gpu["outliers"] == ref["outliers"]
    assert abs(gpu["sigma_sq"] - ref["sigma_sq"]) <= 1e-9 * ref["sigma_sq"]


def test_metric_runs_are_bit_identical(gpu_required):
    """Two independent solves of the noisy metric map: identical iteration logs (every double) and identical poses and
    points, bit for bit."""
    from mcptam_amd import synth
    p = synth.make_config("metric")
    runs = [run_bundle(_gpu(p.cams, disable_convergence=True), p, 6) for _ in range(2)]
    a, b = runs
    assert a["rc"] == b["rc"] == 6
    assert a["logs"] == b["logs"]
    assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["X"], b["X"])
    assert a["outliers"] == b["outliers"] and a["sigma_sq"] == b["sigma_sq"] and a["lam"] == b["lam"]


@pytest.mark.parametrize("n_meas", [1, 2])
def test_sigma_small_sample_factor_wraps_like_size_t(gpu_required, n_meas):
    """Huber::FindSigmaSquared computes 5/(2n - 6) with n a size_t (MEstimator.h:201): for n = 1, 2 the denominator
    wraps to ~1.8e19 and the factor is 1, not 1 + 5/(-4) or 1 + 5/(-2)."""
    from mcptam_amd import synth
    p = synth.make_config("tiny")
    keep = np.flatnonzero(p.ms_pt == p.ms_pt[0])[:n_meas]
    assert keep.size == n_meas
    for name in ("ms_mkf", "ms_cam", "ms_pt", "ms_uv", "ms_level"):
        setattr(p, name, getattr(p, name)[keep])
    g, o = _gpu(p.cams), _orc(p.cams)
    p.populate(g)
    p.populate(o)
    chi_g, _ = g.Eval(n_meas)
    cg, sg = g.DebugRobustChi2()
    co, so = o.DebugRobustChi2()
    med = np.sort(np.abs(chi_g))[n_meas // 2]
    expect = (1.345 * 1.4826 * (1 + 5.0 / float(np.uint64(2 * n_meas - 6 + 2 ** 64))) * np.sqrt(med)) ** 2
    assert abs(sg - expect) <= 1e-12 * expect
    assert abs(sg - so) <= 1e-12 * so and abs(cg - co) <= 1e-11 * max(co, 1e-300)


def test_zero_iterations_and_runtime_error_code(gpu_required):
    """optimize(0) runs nothing: -1 without an external abort, 0 with one (ChainBundle.cc:1355-1366)."""
    from mcptam_amd import synth
    p = synth.make_config("tiny")
    g = _gpu(p.cams)
    p.populate(g)
    assert g.Compute(0) == -1
    g.abort.value = 1
    assert g.Compute(0) == 0


@pytest.mark.parametrize("cfg,iters", [("tiny", 10), ("c2small", 8)])
def test_newton_fallback_camera(gpu_required, cfg, iters):
    """Cameras without an inverse polynomial (n_inv == 0): linear inverse model + FindRootWithNewton in the kernels
    (TaylorCamera.cc:159-176, 258-270, 293-315)."""
    from mcptam_amd import synth
    kw = dict(newton_camera=True)
    p = synth.make_config("c2", n_mkf=12, n_points=1500, **kw) if cfg == "c2small" else synth.make_config(cfg, **kw)
    assert p.cams[0].to_struct().n_inv == 0
    g, o = _gpu(p.cams), _orc(p.cams)
    p.populate(g)
    p.populate(o)
    chi_g, err_g = g.Eval(p.n_meas)
    chi_o, err_o = o.Eval()
    assert rel_err(err_g, err_o) < 1e-9
    gpu = run_bundle(_gpu(p.cams), p, iters)
    ref = run_bundle(_orc(p.cams), p, iters)
    rep = compare_runs(gpu, ref)
    assert rep["branch_flips"] == 0 and gpu["outliers"] == ref["outliers"]


def test_recent_window_of_the_metric_map_matches_oracle(gpu_required):
    """The bundle MCPTAM runs most: BundleAdjusterBase::BundleAdjustRecent (src/BundleAdjusterBase.cc:188-265) on the metric map --
    the newest MKF and its movable neighbours free, every other MKF that sees their points fixed -- two-step as the map maker
    calls it (10 iterations, then to convergence, BundleAdjusterMulti.cc:210-224 is per call; here one call of 10)."""
    from mcptam_amd import synth
    p = synth.recent_window(synth.make_config("metric"))
    assert 2 <= (~p.base_fixed).sum() <= 4 and p.base_fixed.sum() >= 10 and p.n_meas > 10000
    gpu = run_bundle(_gpu(p.cams), p, 10)
    ref = run_bundle(_orc(p.cams), p, 10)
    rep = compare_runs(gpu, ref)
    assert rep["branch_flips"] == 0 and gpu["outliers"] == ref["outliers"]
    assert abs(gpu["sigma_sq"] - ref["sigma_sq"]) <= 1e-9 * ref["sigma_sq"]
    assert gpu["max_cov"] == 0.0 and ref["max_cov"] == 0.0          # three free poses: no marginals (:1419,1444-1448)


def _spawn2(fn, *args):
    import os
    import socket
    import tempfile
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    d = tempfile.mkdtemp()
    mp.spawn(fn, args=(2, port, d) + args, nprocs=2, join=True)
    return d


@pytest.mark.timeout(300)
def test_rank_with_an_empty_shard_joins_every_collective(gpu_required):
    """A rank whose shard holds no measurement must not take a local shortcut past the all-reduces (the other ranks would wait for
    ever): emptiness is decided on the global totals.  Two ranks, rank 1 empty = the single-rank solve of rank 0's map."""
    import os
    import dist_workers
    from mcptam_amd import synth
    cfg = dict(name="c2", n_mkf=12, n_points=900)
    d = _spawn2(dist_workers.sharded_solve_with_an_empty_rank, cfg, 5)
    r0, r1 = np.load(os.path.join(d, "empty_0.npz")), np.load(os.path.join(d, "empty_1.npz"))
    p = synth.make_config(shard=0, **cfg)
    ref = run_bundle(_gpu(p.cams), p, 5)
    assert int(r0["rc"]) == int(r1["rc"]) == ref["rc"] == 5
    assert np.array_equal(r0["R"], r1["R"]) and np.array_equal(r0["t"], r1["t"])
    assert rel_err_elem(r0["R"], ref["R"]) < 1e-9 and rel_err_elem(r0["t"], ref["t"]) < 1e-9
    assert list(r0["trials"]) == [l["trials"] for l in ref["logs"]] == list(r1["trials"])
    assert int(r0["n_out"]) == len(ref["outliers"]) and int(r1["n_out"]) == 0
    assert abs(float(r1["sigma_sq"]) - ref["sigma_sq"]) <= 1e-12 * ref["sigma_sq"]


@pytest.mark.timeout(300)
def test_multi_rank_max_cov_is_the_global_median(gpu_required):
    """ChainBundle.cc:1401-1448 with the points sharded: every rank inverts the all-reduced pose system, the depth covariances are
    rank-local and their median is the global order statistic."""
    import os
    import dist_workers
    from mcptam_amd import synth
    cfg = dict(name="tiny", n_mkf=3, n_points=80, n_fixed_mkf=1, per_point=3)
    d = _spawn2(dist_workers.sharded_max_cov, cfg, 8)
    r0, r1 = np.load(os.path.join(d, "cov_0.npz")), np.load(os.path.join(d, "cov_1.npz"))
    merged = synth.merge_shards([synth.make_config(shard=0, **cfg), synth.make_config(shard=1, **cfg)])
    ref = run_bundle(_gpu(merged.cams), merged, 8)
    assert int(r0["rc"]) == int(r1["rc"]) == ref["rc"]
    assert ref["max_cov"] > 0
    assert float(r0["max_cov"]) == float(r1["max_cov"])
    assert abs(float(r0["max_cov"]) - ref["max_cov"]) <= 1e-8 * ref["max_cov"]


@pytest.mark.timeout(600)
def test_bench_two_rank_path_end_to_end(gpu_required):
    """bench.py as the driver launches it for N = 2 (torch.distributed.run, one process per rank), with both ranks on this box's
    single GPU and the gloo transport (--debug-single-device): the multi-rank code path of the headline benchmark end to end."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--config", "c2", "--cpu-iters", "0", "--debug-single-device"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=500, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["steps"] == 4 and d["value"] > 0
    assert "debug" in d["config"] and d["config"]["chi2_last"] < d["config"]["chi2_first"]


@pytest.mark.parametrize("knob", ["MCP_BA_SMALL", "MCP_BA_CHOL_FUSE1", "MCP_BA_SPECULATE_ADAPT"])
@pytest.mark.parametrize("cfg,iters", [("c1", 12), ("c2small", 10), ("window", 10)])
def test_small_bundle_scheduling_does_not_change_a_single_bit(gpu_required, cfg, iters, knob, monkeypatch):
    """A small bundle (BundleAdjustRecent's window) gets the trial's pose update and chain transforms in one launch and the next
    iteration's head (median, sigma block, robust chi2) enqueued behind every trial before the host has seen its result
    (ba_small.h, mcp_ba::head_ahead); a reduced system of one tile (<= 5 free poses) is factored and back-substituted in one launch
    (k_chol_step, fuse_back).  Scheduling only: with MCP_BA_SMALL=0 / MCP_BA_CHOL_FUSE1=0 the same problem runs the general
    sequence of launches and must give the same iteration logs, poses, points and outliers, bit for bit -- rejected trials (whose
    head is thrown away) included.  MCP_BA_SPECULATE_ADAPT=0: the rejection branch's systems solved ahead in every iteration, not
    only after a trial has been rejected (what a small bundle does by default)."""
    from mcptam_amd import synth
    p = (synth.recent_window(synth.make_config("metric")) if cfg == "window" else
         synth.make_config("c2", n_mkf=12, n_points=1500) if cfg == "c2small" else synth.make_config(cfg))
    small = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    monkeypatch.setenv(knob, "0")
    plain = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    assert small["rc"] == plain["rc"] == iters
    assert small["logs"] == plain["logs"]
    assert np.array_equal(small["R"], plain["R"]) and np.array_equal(small["t"], plain["t"]) and np.array_equal(small["X"], plain["X"])
    assert small["outliers"] == plain["outliers"] and small["sigma_sq"] == plain["sigma_sq"] and small["lam"] == plain["lam"]


def test_head_of_a_rejected_trial_never_reaches_the_next_iteration(gpu_required, monkeypatch):
    """The head enqueued behind a trial that is then rejected leaves its robust-chi2 sum on the second stream; the head the next
    iteration takes itself must be ordered behind it, or the stale sum lands last and becomes that iteration's chi2_start (seen once
    in a round-end pass: a race).  Thirty runs of a bundle whose iterations reject trials, each against the general sequence of
    launches, bit for bit."""
    from mcptam_amd import synth
    p = synth.make_config("tiny", n_points=120)
    monkeypatch.setenv("MCP_BA_SMALL", "0")
    plain = run_bundle(_gpu(p.cams, robust=False, tukey=True), p, 10)
    monkeypatch.delenv("MCP_BA_SMALL")
    assert sum(l["trials"] for l in plain["logs"]) > len(plain["logs"]), "the run must contain rejected trials for this to mean anything"
    for rep in range(30):
        small = run_bundle(_gpu(p.cams, robust=False, tukey=True), p, 10)
        assert small["logs"] == plain["logs"], rep
        assert np.array_equal(small["X"], plain["X"]) and np.array_equal(small["R"], plain["R"])


@pytest.mark.parametrize("cfg,iters,force", [("window", 10, "0"), ("c1", 10, "1"), ("c2small", 8, "1")])
def test_split_assembly_agrees_with_one_thread_per_entry(gpu_required, cfg, iters, force, monkeypatch):
    """k_assemble_long (eight lanes per entry of the reduced system, fixed tree over their partial sums; chosen when the lists of
    staged blocks are long -- the window) against k_assemble (one thread per entry): other summation order, same system.  Forced
    the other way round with MCP_BA_ASM_LONG on each problem."""
    from mcptam_amd import synth
    p = (synth.recent_window(synth.make_config("metric")) if cfg == "window" else
         synth.make_config("c2", n_mkf=12, n_points=1500) if cfg == "c2small" else synth.make_config(cfg))
    a = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    monkeypatch.setenv("MCP_BA_ASM_LONG", force)
    b = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    rep = compare_runs(a, b, tol_state=1e-7, tol_chi=1e-9)
    assert rep["branch_flips"] == 0, rep


@pytest.mark.parametrize("cfg,iters", [("c1", 10), ("c2small", 8)])
def test_quarter_groups_agree_with_full_groups(gpu_required, cfg, iters, monkeypatch):
    """Maps of few points are cut into groups of 16 points with four lanes per point in the linearisation (k_linearize_quad) instead
    of groups of 64 with one lane each: other summation orders, same mathematics.  MCP_BA_SMALL_POINTS=0 forces the large-map
    layout; the two runs agree to rounding, and both are within the oracle's tolerance of each other's state."""
    from mcptam_amd import synth
    p = synth.make_config("c2", n_mkf=12, n_points=1500) if cfg == "c2small" else synth.make_config(cfg)
    quad = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")
    full = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    rep = compare_runs(quad, full, tol_state=1e-7, tol_chi=1e-9)
    assert rep["branch_flips"] == 0, rep
    # groups of 16 points through the one-lane-per-point kernel (what a map whose groups need more LDS than a launch gets falls back to)
    import json
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", "import sys, json; sys.path[:0] = %r; import numpy as np; from mcptam_amd import synth, chain_bundle; from helpers import run_bundle; "
                          "p = synth.make_config('c2', n_mkf=12, n_points=1500) if %r == 'c2small' else synth.make_config(%r); "
                          "r = run_bundle(chain_bundle.ChainBundle(p.cams, True, True, False, disable_convergence=True), p, %d); "
                          "print(json.dumps(dict(X=r['X'].tolist(), logs=r['logs'])))" % ([ROOT, os.path.join(ROOT, "tests")], cfg, cfg, iters)],
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, MCP_BA_SMALL_POINTS="16384", MCP_BA_LIN_QUAD="0"))
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert [(l["trials"], l["accepted"]) for l in r["logs"]] == [(l["trials"], l["accepted"]) for l in quad["logs"]]
    assert rel_err_elem(np.array(r["X"]), quad["X"]) < 1e-8


@pytest.mark.parametrize("env", [dict(MCP_BA_SPEC_TRIALS="0"), dict(MCP_BA_MAILBOX="0"), dict(MCP_BA_OVERLAP="0"), dict(MCP_BA_SPECULATE="0"),
                                 dict(MCP_BA_GRAPH="1"), dict(MCP_BA_OVERLAP="2", MCP_BA_MAIN_SYS="2"), dict(MCP_BA_LIN_JOIN="1"),
                                 dict(MCP_BA_STREAM_POOL="0"), dict(MCP_BA_SCHUR4_ORDER="0"), dict(MCP_BA_HEAD_AHEAD="1"), dict(MCP_BA_HEAD_AHEAD="2"),
                                 dict(MCP_BA_TRIAL_FUSE="0"), dict(MCP_BA_SPEC_TRIALS="1"), dict(MCP_BA_CHOL_SPREAD="0"), dict(MCP_BA_HEAD_LARGE="1"),
                                 dict(MCP_BA_CHOL_BACK_CHAINS="0")])
def test_scheduling_knobs_do_not_change_a_single_bit(gpu_required, env, monkeypatch):
    """Speculative multi-lambda solves, the second stream, the trial evaluated one ahead, the result mailbox, graph replay and the
    iteration head (median, sigma^2 -- ba_head.h) enqueued behind every trial before the host has accepted one are
    scheduling: the same kernels see the same inputs whichever of them is on, so iteration logs, poses and points are identical
    to the default configuration's, bit for bit (the knobs are read when the handle is created).  Likewise the launch order of the
    Schur groups, the step of a trial as one launch or three (k_trial_apply: same arithmetic per pose, chain and point), every trial
    evaluated ahead on its own stream, the number of workers a factorisation is launched with, the head of an iteration (median,
    sigma^2, robust chi2) as one launch with grid barriers or six (ba_headl.h), and the back-substitution of the reduced system with a
    workgroup per chain of the plan or one for all block columns (the metric map is two chains + separator)."""
    from mcptam_amd import synth
    p = synth.make_config("metric")
    base = run_bundle(_gpu(p.cams, disable_convergence=True), p, 7)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    alt = run_bundle(_gpu(p.cams, disable_convergence=True), p, 7)
    assert base["rc"] == alt["rc"] == 7
    assert sum(l["trials"] for l in base["logs"]) > 10, "the run must contain rejected trials for this to mean anything"
    assert base["logs"] == alt["logs"]
    assert np.array_equal(base["R"], alt["R"]) and np.array_equal(base["t"], alt["t"]) and np.array_equal(base["X"], alt["X"])
    assert base["outliers"] == alt["outliers"] and base["sigma_sq"] == alt["sigma_sq"] and base["lam"] == alt["lam"]


_GENERAL_MAPS = {"tiny120": (lambda synth: synth.make_config("tiny", n_points=120), 12), "ring": (lambda synth: synth.make_config("ring"), 10)}
_general_base = {}


def _general_sequence_base(name):
    """The map and its default-knob run through the general launch sequence (MCP_BA_SMALL=0 is set by the caller), computed once."""
    if name not in _general_base:
        from mcptam_amd import synth
        make, iters = _GENERAL_MAPS[name]
        p = make(synth)
        g = _gpu(p.cams, disable_convergence=True)
        _general_base[name] = (p, iters, run_bundle(g, p, iters), g.Timing())
    return _general_base[name]


@pytest.mark.parametrize("env", [dict(MCP_BA_OVERLAP="1"), dict(MCP_BA_OVERLAP="1", MCP_BA_SPEC_TRIALS="1"), dict(MCP_BA_OVERLAP="1", MCP_BA_SPEC_TRIALS="0"),
                                 dict(MCP_BA_OVERLAP="2", MCP_BA_MAIN_SYS="2"), dict(MCP_BA_OVERLAP="1", MCP_BA_TRIAL_FUSE="0"), dict(MCP_BA_TRIAL_FUSE="0"),
                                 dict(MCP_BA_MAILBOX="0"), dict(MCP_BA_SPECULATE="0"), dict(MCP_BA_GRAPH="1"), dict(MCP_BA_OVERLAP="1", MCP_BA_HEAD_AHEAD="1"),
                                 dict(MCP_BA_HEAD_LARGE="1"), dict(MCP_BA_FORCE_MULTI="1"), dict(MCP_BA_FORCE_MULTI="1", MCP_BA_OVERLAP="1")],
                         ids=lambda e: ",".join("%s=%s" % (k[7:], v) for k, v in e.items()))
@pytest.mark.parametrize("name", ["tiny120", "ring"])
def test_general_launch_sequence_on_small_maps_does_not_change_a_single_bit(gpu_required, name, env, monkeypatch):
    """The knob test above runs on the metric map, which by default never splits a batch over two streams.  Here the general
    (non-small: MCP_BA_SMALL=0) sequence of launches runs on two small maps whose iterations reject trials -- a robust bundle of 480
    measurements and a ring of 24 000 with a several-chain plan -- under the knobs, alone and in the pairs that reach a branch of
    their own: the split batch with every trial ahead, one, or none; two systems on the main stream; the step in three launches; no
    mailbox; no speculation; graph replay; the per-trial and the one-launch iteration head; the multi-rank machine over one rank
    (identity hook) with and without the split.  Scheduling only: everything a run returns equals the default run's, bit for bit."""
    monkeypatch.setenv("MCP_BA_SMALL", "0")
    p, iters, base, base_tm = _general_sequence_base(name)
    assert max(l["trials"] for l in base["logs"]) >= 3 and base_tm["n_spec_hits"] > 0, "the run must reject trials and consume speculative systems for this to mean anything"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = _gpu(p.cams, disable_convergence=True)
    if "MCP_BA_FORCE_MULTI" in env:
        g.SetAllReduce(lambda ptr, count, stream: None, 0, 1)
    alt = run_bundle(g, p, iters)
    assert base["rc"] == alt["rc"]
    assert base["logs"] == alt["logs"]
    assert np.array_equal(base["R"], alt["R"]) and np.array_equal(base["t"], alt["t"]) and np.array_equal(base["X"], alt["X"])
    assert base["outliers"] == alt["outliers"] and base["sigma_sq"] == alt["sigma_sq"] and base["lam"] == alt["lam"]


@pytest.mark.parametrize("cfg,iters", [("c2", 6), ("metric", 6)])
def test_pipelined_linearisation_agrees_with_the_plain_loop(gpu_required, cfg, iters, monkeypatch):
    """k_linearize_pipe issues every load of a measurement at the head of its round and lets the W block of the round before leave
    behind them (an accumulating block as a no-return atomic add); k_linearize_group is the plain loop.  The same operations on the
    same numbers -- but two compilations contract multiply-adds differently, so the two agree to rounding, not bit for bit: same
    accept / reject sequence, state to 1e-9 (each of them is bit-reproducible on its own)."""
    from mcptam_amd import synth
    monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")         # (the large-map layout at both sizes: the quad form has no global W stores in its loop)
    p = synth.make_config(cfg)
    pipe = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    pipe2 = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    monkeypatch.setenv("MCP_BA_LIN_PIPE", "0")
    plain = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    assert pipe["logs"] == pipe2["logs"] and np.array_equal(pipe["X"], pipe2["X"])
    assert [(l["trials"], l["accepted"]) for l in pipe["logs"]] == [(l["trials"], l["accepted"]) for l in plain["logs"]]
    assert rel_err_elem(pipe["R"], plain["R"]) < 1e-9 and rel_err_elem(pipe["t"], plain["t"]) < 1e-9 and rel_err_elem(pipe["X"], plain["X"]) < 1e-9


@pytest.mark.parametrize("cfg,iters", [("tiny", 6), ("c1", 8), ("calib", 6), ("c2", 6), ("metric", 5)])
def test_threaded_prepare_builds_the_serial_structure(gpu_required, cfg, iters, monkeypatch):
    """Prepare() builds the solver's structure on the host's worker pool (ranges of points per thread, positions known beforehand);
    the serial reference implementation stays behind MCP_BA_PREPARE_LEGACY=1.  Same arrays => the same solve, bit for bit:
    reduced system, iteration logs, poses, points, outlier list."""
    from mcptam_amd import synth
    monkeypatch.setenv("MCP_BA_CHOL_CHAINS", "1")      # (the serial builder keeps the free poses in add order; the threaded one re-orders a long trajectory for two chains)
    p = synth.make_config(cfg)
    g = _gpu(p.cams, disable_convergence=True)
    p.populate(g)
    S1 = g.DebugSystem(1e-3)
    new = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    monkeypatch.setenv("MCP_BA_PREPARE_LEGACY", "1")
    g = _gpu(p.cams, disable_convergence=True)
    p.populate(g)
    S0 = g.DebugSystem(1e-3)
    old = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    for a, b in zip(S0, S1):
        assert np.array_equal(a, b)
    assert new["logs"] == old["logs"] and new["outliers"] == old["outliers"]
    assert np.array_equal(new["R"], old["R"]) and np.array_equal(new["t"], old["t"]) and np.array_equal(new["X"], old["X"])


def test_a_refused_launch_is_reported_by_kernel_name(gpu_required, monkeypatch):
    """A launch the runtime refuses (here: the linearisation asked for more LDS than a compute unit has -- a test hook) leaves no trace
    in the stream; Compute() must not return the untouched state as a result.  The check sits at the launch site, so the message names
    the kernel, and the next solve on a healthy configuration is not affected by anything sticky."""
    from mcptam_amd import synth, chain_bundle
    p = synth.make_config("c2", n_mkf=20, n_points=20000)      # (large-map layout: k_linearize_group)
    monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")
    monkeypatch.setenv("MCP_BA_TEST_REFUSE_LAUNCH", "1")
    g = _gpu(p.cams, disable_convergence=True)
    p.populate(g)
    with pytest.raises(RuntimeError) as ei:
        g.Compute(2)
    assert "k_linearize" in str(ei.value)
    monkeypatch.delenv("MCP_BA_TEST_REFUSE_LAUNCH")
    r = run_bundle(_gpu(p.cams, disable_convergence=True), p, 2)
    assert r["rc"] == 2


@pytest.mark.parametrize("cfg,iters", [("c1", 6), ("c2", 6), ("metric", 5), ("band", 6), ("ring", 6)])
def test_a_map_that_lost_its_outliers_adopts_the_cached_structure_of_the_call_before(gpu_required, cfg, iters, monkeypatch):
    """Near miss (include/mcp_ba.h): MCPTAM erases the measurements an adjustment flagged (MapMakerServerBase::HandleOutliers,
    /root/reference/src/MapMakerServerBase.cc:1198-1238) and adjusts again -- same poses, points, chains, the measurements minus a few.
    The second call adopts the first one's cached structure, the erased measurements staying in the device arrays with weight 0.  Against
    a COLD Prepare() of the smaller map (MCP_BA_NEAR_MISS=0): the same accept / reject sequence, state, sigma^2 and chi2 to rounding
    (the order of some sums is the superset's), the same outlier list, chi2 per measurement in the smaller map's add order -- and against
    the oracle on the smaller map within the usual tolerance."""
    from mcptam_amd import synth, chain_bundle
    p = synth.make_config(cfg)
    chain_bundle.struct_cache_clear()
    first = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)
    assert len(first["outliers"]) > 0
    # (a point all of whose measurements were flagged keeps them here: a map that lost a point is built cold, see the end of this test)
    from collections import Counter
    flagged = Counter(o[0] for o in first["outliers"])
    per_point = p.n_meas // p.n_points
    first["outliers"] = [o for o in first["outliers"] if flagged[o[0]] < per_point]
    q = synth.erase_measurements(p, first["outliers"], first["ids"])
    assert q.n_meas == p.n_meas - len(first["outliers"])
    n0 = chain_bundle.struct_cache_near_hits()
    g = _gpu(q.cams, disable_convergence=True)
    near = run_bundle(g, q, iters)
    assert chain_bundle.struct_cache_near_hits() == n0 + 1
    chi_near, _ = g.Eval(q.n_meas)
    g.close()
    monkeypatch.setenv("MCP_BA_NEAR_MISS", "0")
    g2 = _gpu(q.cams, disable_convergence=True)
    cold = run_bundle(g2, q, iters)
    chi_cold, _ = g2.Eval(q.n_meas)
    g2.close()
    assert chain_bundle.struct_cache_near_hits() == n0 + 1
    assert near["rc"] == cold["rc"] == iters
    assert [(l["trials"], l["accepted"]) for l in near["logs"]] == [(l["trials"], l["accepted"]) for l in cold["logs"]]
    for a, b in zip(near["logs"], cold["logs"]):
        assert abs(a["chi2_end"] - b["chi2_end"]) <= 1e-9 * abs(b["chi2_end"]) and abs(a["sigma_sq"] - b["sigma_sq"]) <= 1e-9 * abs(b["sigma_sq"])
    # (a map whose factorisation is cut into chains: the cold Prepare() of the smaller map cuts ITS coupling graph, not the superset's --
    #  another elimination order, state to 1e-8 as in test_a_trajectory_band_is_factorised_as_two_chains)
    tol = 1e-8 if cfg in ("metric", "band", "ring") else 1e-9
    assert rel_err_elem(near["R"], cold["R"]) < tol and rel_err_elem(near["t"], cold["t"]) < tol and rel_err_elem(near["X"], cold["X"]) < tol
    assert abs(near["sigma_sq"] - cold["sigma_sq"]) <= 1e-9 * cold["sigma_sq"] and abs(near["mean_chi2"] - cold["mean_chi2"]) <= 1e-9 * cold["mean_chi2"]
    assert sorted(near["outliers"]) == sorted(cold["outliers"])
    assert np.allclose(chi_near, chi_cold, rtol=1e-7, atol=1e-12)
    if cfg != "metric":
        o = _orc(q.cams)
        o.DisableConvergence(True)
        ref = run_bundle(o, q, iters)
        rep = compare_runs(near, ref)
        assert rep["branch_flips"] == 0, rep
    # a map that lost ALL measurements of a point is not a near miss (its unknowns differ): built cold, still correct
    monkeypatch.setenv("MCP_BA_NEAR_MISS", "1")
    pt0 = int(q.ms_pt[0])
    gone = [(int(first["ids"]["point"][pt0]), int(first["ids"]["mkf"][int(k)]), int(c)) for k, c in zip(q.ms_mkf[q.ms_pt == pt0], q.ms_cam[q.ms_pt == pt0])]
    r = synth.erase_measurements(q, gone, first["ids"])
    n1 = chain_bundle.struct_cache_near_hits()
    lone = run_bundle(_gpu(r.cams, disable_convergence=True), r, 2)
    assert lone["rc"] == 2 and chain_bundle.struct_cache_near_hits() == n1


def test_a_near_miss_handle_prepared_again_by_the_serial_builder_forgets_its_masked_measurements(gpu_required, monkeypatch):
    """What a Prepare() leaves for Compute() is reset at the top of every Prepare(), whichever path follows.  A handle that adopted a
    superset's structure (near miss: n_masked erased measurements stay in the device arrays with weight 0, and the median of the
    squared errors is taken at rank n_masked + m/2) and is then prepared again by the serial builder -- which builds the smaller map's
    own arrays, nothing masked -- must solve exactly like a fresh handle under the serial builder: same arrays => same solve, bit for
    bit, as in test_threaded_prepare_builds_the_serial_structure."""
    from mcptam_amd import synth, chain_bundle
    from helpers import collect
    iters = 6
    p = synth.make_config("c1")
    chain_bundle.struct_cache_clear()
    first = run_bundle(_gpu(p.cams, disable_convergence=True), p, iters)          # fills the cache with the full map
    from collections import Counter
    flagged = Counter(o[0] for o in first["outliers"])
    per_point = p.n_meas // p.n_points
    gone = [o for o in first["outliers"] if flagged[o[0]] < per_point]             # (a map that lost a point is built cold)
    assert len(gone) > 0
    q = synth.erase_measurements(p, gone, first["ids"])
    n0 = chain_bundle.struct_cache_near_hits()
    g = _gpu(q.cams, disable_convergence=True)
    ids = q.populate(g)
    g.Prepare()
    assert chain_bundle.struct_cache_near_hits() == n0 + 1
    monkeypatch.setenv("MCP_BA_PREPARE_LEGACY", "1")
    g.SetComm(None)                                                                # marks the handle dirty; the map is unchanged
    rc = g.Compute(iters)
    R, t, X = collect(g, ids)
    again = dict(rc=rc, logs=g.IterLogs(), outliers=g.GetOutlierMeasurements(), sigma_sq=g.GetSigmaSquared())
    g.close()
    fresh = run_bundle(_gpu(q.cams, disable_convergence=True), q, iters)
    assert chain_bundle.struct_cache_near_hits() == n0 + 1
    assert again["rc"] == fresh["rc"] == iters
    assert again["logs"] == fresh["logs"] and again["sigma_sq"] == fresh["sigma_sq"] and again["outliers"] == fresh["outliers"]
    assert np.array_equal(R, fresh["R"]) and np.array_equal(t, fresh["t"]) and np.array_equal(X, fresh["X"])


@pytest.mark.parametrize("cfg,iters", [("tiny", 6), ("c1", 6), ("calib", 6), ("c2", 5), ("metric", 4), ("band", 5)])
def test_cached_prepare_equals_a_cold_one(gpu_required, cfg, iters):
    """Structure cache (include/mcp_ba.h): a handle that brings the topology of an earlier Prepare() adopts that structure (host
    results + a device clone of the packed block) and uploads only its numbers.  The reduced system, iteration logs, poses, points and
    outlier list of a cached Prepare() equal a cold one's bit for bit -- also when the NUMBERS differ between the call that filled
    the cache and the call that hits it (other measurement noise, other initial state), which is how MCPTAM repeats an adjustment
    (/root/reference/src/BundleAdjusterMulti.cc:75: a fresh bundle per call; src/MapMaker.cc: called again until converged)."""
    from mcptam_amd import synth, chain_bundle
    p = synth.make_config(cfg)
    q = synth.make_config(cfg)                         # same topology, other numbers
    rng = np.random.default_rng(5)
    q.ms_uv = q.ms_uv + rng.normal(size=q.ms_uv.shape) * 0.05
    q.pt_x = q.pt_x * (1.0 + 1e-3 * rng.normal(size=(q.n_points, 1)))
    q.base_t = q.base_t + 1e-4 * rng.normal(size=q.base_t.shape) * (~q.base_fixed)[:, None]

    def solve(prob, cold=False):
        if cold:
            chain_bundle.struct_cache_clear()
        g = _gpu(prob.cams, disable_convergence=True)
        prob.populate(g)
        S = g.DebugSystem(1e-3)
        if cold:
            chain_bundle.struct_cache_clear()
        return S, run_bundle(_gpu(prob.cams, disable_convergence=True), prob, iters)

    chain_bundle.struct_cache_clear()
    h0, m0 = chain_bundle.struct_cache_stats()
    cold_q = solve(q)                                    # fills the cache with q's numbers
    h1, m1 = chain_bundle.struct_cache_stats()
    assert m1 == m0 + 1 and h1 == h0 + 1                 # (the second handle of solve() already hits)
    warm_p = solve(p)                                    # cached structure (built from q), p's numbers
    h2, m2 = chain_bundle.struct_cache_stats()
    assert h2 == h1 + 2 and m2 == m1
    cold_p = solve(p, cold=True)                         # the same two Prepare() calls, each on an empty cache
    h3, m3 = chain_bundle.struct_cache_stats()
    assert h3 == h2 and m3 == m2 + 2
    for a, b in zip(cold_p[0], warm_p[0]):
        assert np.array_equal(a, b)
    a, b = cold_p[1], warm_p[1]
    assert a["logs"] == b["logs"] and a["outliers"] == b["outliers"]
    assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"]) and np.array_equal(a["X"], b["X"])
    assert not np.array_equal(a["X"], cold_q[1]["X"])    # (the two problems do differ)


@pytest.mark.parametrize("k,max_trials", [(4, 100), (2, 2)])
def test_failed_factorisation_applies_the_stale_step_like_g2o(gpu_required, k, max_trials, monkeypatch):
    """When the linear solver fails, g2o's x keeps the last successful solve's content, update(x) applies it, the trial is rejected
    and popped -- but the edges keep that trial's errors, which the residual action reads if it was the iteration's last trial
    (OptimizationAlgorithmLevenberg::solve [3P-memory], src/ChainBundle.cc:1096-1116).  Forced on the k-th trial on both sides; with
    max_trials = 2 the failed trial IS the last one of its iteration, so chi2_end is the stale step's chi2."""
    from mcptam_amd import synth
    from mcptam_amd.chain_bundle import ChainBundle
    p = synth.make_config("c2small") if "c2small" in synth.CONFIGS else synth.make_config("c2", n_mkf=16, n_points=1200)
    monkeypatch.setattr(ChainBundle, "snMaxTrialsAfterFailure", max_trials)
    monkeypatch.setenv("MCP_BA_TEST_FAIL_TRIAL", str(k))
    g = _gpu(p.cams, disable_convergence=True)
    o = _orc(p.cams); o.DisableConvergence(True); o.SetFailTrial(k); o.SetLimits(max_trials)
    gpu = run_bundle(g, p, 5)
    ref = run_bundle(o, p, 5)
    assert gpu["rc"] == ref["rc"]
    assert [l["trials"] for l in gpu["logs"]] == [l["trials"] for l in ref["logs"]] and [l["accepted"] for l in gpu["logs"]] == [l["accepted"] for l in ref["logs"]]
    for a, b in zip(gpu["logs"], ref["logs"]):
        assert abs(a["chi2_end"] - b["chi2_end"]) <= 1e-9 * abs(b["chi2_end"]) and abs(a["lambda_end"] - b["lambda_end"]) <= 1e-9 * b["lambda_end"]
        assert abs(a["rms_update"] - b["rms_update"]) <= 1e-7 * max(b["rms_update"], 1e-30)
    assert rel_err_elem(gpu["R"], ref["R"]) < 1e-8 and rel_err_elem(gpu["X"], ref["X"]) < 1e-8
    plain = run_bundle(_orc_nc(p.cams), p, 5)
    assert plain["logs"] != ref["logs"], "the forced failure must be visible in the iteration log"
    # the same through the multi-rank machine (one-rank communicator semantics: identity all-reduce): an ACCEPTED stale step must not
    # leave the riding median pointed at the failed trial's histograms (the next sigma^2 would be silently wrong)
    monkeypatch.setenv("MCP_BA_FORCE_MULTI", "1")
    gm = _gpu(p.cams, disable_convergence=True)
    gm.SetAllReduce(lambda ptr, count, stream: None, 0, 1)
    multi = run_bundle(gm, p, 5)
    assert [l["trials"] for l in multi["logs"]] == [l["trials"] for l in gpu["logs"]] and [l["accepted"] for l in multi["logs"]] == [l["accepted"] for l in gpu["logs"]]
    for a, b in zip(multi["logs"], gpu["logs"]):
        assert a["sigma_sq"] == b["sigma_sq"] and a["chi2_end"] == b["chi2_end"]
    assert np.array_equal(multi["R"], gpu["R"]) and np.array_equal(multi["X"], gpu["X"])


def _orc_nc(cams):
    o = _orc(cams); o.DisableConvergence(True)
    return o


# ---------------------------------------------------------------------------------------------------------------------
# round 4: the reduced system factored in ONE persistent launch (ba_chol2.h)

@pytest.mark.parametrize("n", [1, 32, 33, 97, 200, 1194])
def test_one_launch_factorisation_matches_numpy(gpu_required, n):
    """k_chol_persist seen from outside: every off-diagonal tile of L, L_kk^-1 in place of the diagonal tiles (what the kernels keep)
    and y = L^-1 b against numpy, no hand-off time-out, no failure flag."""
    from mcptam_amd.chain_bundle import chol_debug_factor
    rng = np.random.default_rng(4000 + n)
    B = rng.normal(size=(n, n))
    A = B @ B.T + n * np.eye(n)
    b = rng.normal(size=n)
    L, y, err, fail = chol_debug_factor(np.tril(A), b)
    assert err == 0 and fail == 0
    Lr = np.linalg.cholesky(A)
    ntc = (n + 31) // 32
    for i in range(ntc):
        for j in range(i + 1):
            g, r = L[32 * i:32 * i + 32, 32 * j:32 * j + 32], Lr[32 * i:32 * i + 32, 32 * j:32 * j + 32]
            if i == j:
                r = np.linalg.inv(r)
            assert np.abs(g - r).max() <= 1e-11 * np.abs(r).max(), (i, j)
    yr = np.linalg.solve(Lr, b)
    assert np.abs(y - yr).max() <= 1e-11 * np.abs(yr).max()


@pytest.mark.parametrize("n,nsys,band", [(1194, 1, 6), (1194, 4, 6), (1194, 3, 2), (700, 2, 0), (2994, 2, 6)])
def test_one_launch_factorisation_on_banded_plans(gpu_required, n, nsys, band):
    """Banded + bordered tile plans (a loop trajectory's co-visibility; band 2 < the critical workgroup's own band: tiles it owns
    that the assembly never writes start from zero), several systems in one launch; the solutions against numpy."""
    from mcptam_amd.chain_bundle import chol_time
    rng = np.random.default_rng(77 + n + band)
    B = rng.normal(size=(n, n))
    A = B @ B.T + n * np.eye(n)
    if band:
        ntc = (n + 31) // 32
        for i in range(ntc):
            for j in range(ntc):
                lo, hi = max(i, j), min(i, j)
                if not (lo - hi <= band or lo >= ntc - band):
                    A[32 * i:32 * i + 32, 32 * j:32 * j + 32] = 0.0
        A += 4 * n * np.eye(n)
    b = rng.normal(size=n)
    tf, tb, x = chol_time(np.tril(A), b, nsys=nsys, reps=5, band=band)
    for q in range(nsys):
        ref = np.linalg.solve(A + q * np.eye(n), b)
        assert rel_err(x[q], ref) < 1e-11, (q, rel_err(x[q], ref))


def test_one_launch_and_step_kernels_agree_on_the_metric_map(gpu_required, monkeypatch):
    """Same LM run with the one-launch factorisation and with the per-step kernels: another summation order inside the factorisation,
    so not the same bits -- but the same branches and the same state to 1e-9."""
    from mcptam_amd import synth
    p = synth.make_config("metric")
    a = run_bundle(_gpu(p.cams, disable_convergence=True), p, 6)
    monkeypatch.setenv("MCP_BA_CHOL_PERSIST", "0")
    b = run_bundle(_gpu(p.cams, disable_convergence=True), p, 6)
    assert [(l["trials"], l["accepted"]) for l in a["logs"]] == [(l["trials"], l["accepted"]) for l in b["logs"]]
    assert rel_err_elem(a["R"], b["R"]) < 1e-9 and rel_err_elem(a["t"], b["t"]) < 1e-9 and rel_err_elem(a["X"], b["X"]) < 1e-9
    assert a["outliers"] == b["outliers"]


@pytest.mark.parametrize("cfg", ["c2", "ring"])
def test_handoff_timeout_falls_back_to_the_step_kernels(gpu_required, cfg, monkeypatch):
    """A hand-off of the one-launch factorisation that never arrives (forced: the critical workgroup of the third factorisation raises
    the error word) must not hang and must not be taken for a result: every spinner leaves, the failure flag says so, the host
    redoes that solve with the per-step kernels and keeps them.  `ring`: a plan of several chains (k_chol_persist_seg, a chain
    workgroup per arc in the back-substitution) -- every one of its critical workgroups has to leave."""
    from mcptam_amd import synth
    p = synth.make_config(cfg)
    ref = run_bundle(_gpu(p.cams, disable_convergence=True), p, 6)
    monkeypatch.setenv("MCP_BA_TEST_PERSIST_FAIL", "3")
    bundle = _gpu(p.cams, disable_convergence=True)
    alt = run_bundle(bundle, p, 6)
    assert bundle.Timing()["n_persist_fallbacks"] == 1
    assert alt["rc"] == ref["rc"] == 6
    assert [(l["trials"], l["accepted"]) for l in alt["logs"]] == [(l["trials"], l["accepted"]) for l in ref["logs"]]
    assert rel_err_elem(alt["R"], ref["R"]) < 1e-9 and rel_err_elem(alt["t"], ref["t"]) < 1e-9 and rel_err_elem(alt["X"], ref["X"]) < 1e-9


@pytest.mark.timeout(900)
def test_partitioned_map_on_two_ranks_equals_the_oracle_on_the_whole_map(gpu_required):
    """SURVEY.md 8(e) as BundleAdjusterMulti needs it: ONE population (src/BundleAdjusterMulti.cc:90-200) split by synth.partition --
    points sorted by source MKF, contiguous blocks balancing the measurement counts -- at the per-rank size of BASELINE c4 over 8 GPUs
    (12.5k points, 100k measurements per rank), two ranks sharing this GPU through gloo; against the ORACLE's run of the whole map."""
    import os
    import socket
    import tempfile
    import torch.multiprocessing as mp
    import dist_workers
    from mcptam_amd import synth
    cfg = dict(name="c4", n_mkf=60, n_points=25000)
    iters = 3
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(dist_workers.partitioned_solve_on_one_gpu, args=(2, port, d, cfg, iters), nprocs=2, join=True)
        r = [dict(np.load(os.path.join(d, "part_%d.npz" % k))) for k in range(2)]
    p = synth.make_config(**cfg)
    assert r[0]["X"].shape[0] >= 12000 and r[1]["X"].shape[0] >= 12000
    assert abs(int(r[0]["n_meas"]) - int(r[1]["n_meas"])) <= 16 and int(r[0]["n_meas"]) + int(r[1]["n_meas"]) == p.n_meas
    ref = run_bundle(_orc(p.cams), p, iters)
    assert int(r[0]["rc"]) == int(r[1]["rc"]) == ref["rc"]
    assert np.array_equal(r[0]["R"], r[1]["R"]) and np.array_equal(r[0]["t"], r[1]["t"])
    from helpers import rel_err_elem
    assert rel_err_elem(r[0]["R"], ref["R"]) < 1e-6 and rel_err_elem(r[0]["t"], ref["t"]) < 1e-6
    for k in range(2):
        assert rel_err_elem(r[k]["X"], ref["X"][r[k]["points"]]) < 1e-6
    logs = np.array([[l["chi2_start"], l["chi2_end"], l["lambda_end"], l["sigma_sq"], l["trials"], l["accepted"]] for l in ref["logs"]])
    assert np.array_equal(r[0]["logs"][:, 4:], logs[:, 4:]) and np.allclose(r[0]["logs"][:, :4], logs[:, :4], rtol=1e-7)
    assert int(r[0]["n_out"]) + int(r[1]["n_out"]) == len(ref["outliers"])


@pytest.mark.timeout(600)
def test_bench_spawns_its_own_ranks(gpu_required):
    """`python bench.py --gpus 2` WITHOUT the launcher (how a driver may call it) re-executes itself under torch.distributed.run;
    here with both ranks on this box's single GPU (--debug-single-device) and the strong-scaling partition of ONE map."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--config", "c2", "--cpu-iters", "0",
                          "--scaling", "strong", "--debug-single-device"], capture_output=True, text=True, timeout=500, cwd=root, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["value"] > 0 and d["scaling"] == "strong"
    assert "5000 points, 40000 measurements per rank" in d["config"]["workload"]


@pytest.mark.timeout(600)
def test_bench_dumps_what_the_timed_run_computed(gpu_required, tmp_path):
    """`bench.py --dump-outputs DIR` (a plain run, no --full): the result line carries the step count and the time of one step, and
    DIR holds what a caller of the timed run reads back -- the same poses, points, outliers and iteration log as a ChainBundle that
    runs the same seeded map for the same number of iterations here."""
    import json
    import os
    import subprocess
    import sys
    from mcptam_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--config", "c2",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=500, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 4 and d["ms_per_step"] > 0 and abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-9 * d["value"]
    assert "cpu_baseline" not in d and "roofline" not in d          # what takes runs of its own waits for --full
    p = synth.make_config("c2")
    ref = run_bundle(_gpu(p.cams, disable_convergence=True), p, 4)
    got = {n: np.load(str(tmp_path / (n + ".npy"))) for n in ("poses_R", "poses_t", "points", "outlier_measurements", "iteration_log")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert rel_err(got["poses_R"], ref["R"]) < 1e-12 and rel_err(got["poses_t"], ref["t"]) < 1e-12 and rel_err(got["points"], ref["X"]) < 1e-12
    assert np.array_equal(got["outlier_measurements"], np.array(sorted(ref["outliers"]), dtype=np.float64).reshape(-1, 3))
    assert got["iteration_log"].shape == (4, 7)
    assert np.array_equal(got["iteration_log"][:, 5:], [[l["trials"], l["accepted"]] for l in ref["logs"]])


@pytest.mark.parametrize("shape", ["arc", "ring", "chains_that_couple", "ring_in_another_add_order"])
def test_a_trajectory_band_is_factorised_as_two_chains(gpu_required, shape, monkeypatch):
    """A trajectory whose poses see only points of their neighbours -- an open arc, or a loop walked once -- has a banded (cyclic-banded)
    reduced system: prepare() orders its poses [one half | the other half, reversed | the poses between them (| where the ring closes)]
    and the one-launch factorisation walks the two halves beside each other (CholPersist::build, k_chol_persist_seg).  Another elimination
    order: the iteration agrees with the one-chain order's to rounding, not bit for bit -- same accept / reject sequence, state to 1e-8 --
    and with the oracle's as every map does; each order is bit-reproducible.  A cut in the wrong place (forced here: the last two
    tiles of the first half handed to the second) breaks the promise the plan was given -- chains that do not couple: it must notice and
    build one chain, not hang or return another answer."""
    from mcptam_amd import synth
    p = synth.make_config("ring" if shape.startswith("ring") else "band")
    if shape == "ring_in_another_add_order":      # MKFs handed over in a random order: relabelled breadth-first before the cut
        p = synth.shuffle_mkfs(p)
    if shape == "chains_that_couple":
        monkeypatch.setenv("MCP_BA_TEST_CHOL_CUT", "2")
    b = _gpu(p.cams, disable_convergence=True)
    two = run_bundle(b, p, 8)
    assert b.Timing()["chol_chains"] == 1 if shape == "chains_that_couple" else b.Timing()["chol_chains"] in (3, 4, 5, 6, 7)      # (two to six arcs + the separator)
    two_again = run_bundle(_gpu(p.cams, disable_convergence=True), p, 8)
    assert two["logs"] == two_again["logs"] and np.array_equal(two["X"], two_again["X"]) and np.array_equal(two["t"], two_again["t"])
    if shape == "ring":      # the coupling graph from masks taken with atomics (an add order that is not KeyFrame by KeyFrame): the same cut
        from mcptam_amd import chain_bundle
        chain_bundle.struct_cache_clear()
        monkeypatch.setenv("MCP_BA_TEST_CHOL_ATOMIC", "1")
        alt = run_bundle(_gpu(p.cams, disable_convergence=True), p, 8)
        monkeypatch.delenv("MCP_BA_TEST_CHOL_ATOMIC")
        assert two["logs"] == alt["logs"] and np.array_equal(two["X"], alt["X"]) and np.array_equal(two["t"], alt["t"])
    monkeypatch.setenv("MCP_BA_CHOL_CHAINS", "1")
    b1 = _gpu(p.cams, disable_convergence=True)
    one = run_bundle(b1, p, 8)
    assert b1.Timing()["chol_chains"] == 1
    assert [(l["trials"], l["accepted"]) for l in two["logs"]] == [(l["trials"], l["accepted"]) for l in one["logs"]]
    errs = (rel_err_elem(two["R"], one["R"]), rel_err_elem(two["t"], one["t"]), rel_err_elem(two["X"], one["X"]))
    assert max(errs) < 1e-8, errs
    assert two["outliers"] == one["outliers"]
    o = _orc(p.cams)
    o.DisableConvergence(True)
    ref = run_bundle(o, p, 8)
    rep = compare_runs(two, ref)
    assert rep["branch_flips"] == 0
    assert two["outliers"] == ref["outliers"]
    assert abs(two["sigma_sq"] - ref["sigma_sq"]) <= 1e-9 * ref["sigma_sq"]


def test_a_map_without_a_small_separator_stays_one_chain(gpu_required, monkeypatch):
    """A tight loop whose poses all see the same points: every cut of the pose coupling graph needs a separator as large as the arcs, so
    `Prepare()` keeps the add order and the one-chain plan -- the solve is the one `MCP_BA_CHOL_CHAINS=1` gives, bit for bit."""
    from mcptam_amd import synth
    p = synth.make_problem(n_cams=2, n_mkf=110, n_points=4000, per_point=6, radius=1.5, k_near=110)
    b = _gpu(p.cams, disable_convergence=True)
    auto = run_bundle(b, p, 6)
    assert b.Timing()["chol_chains"] == 1
    monkeypatch.setenv("MCP_BA_CHOL_CHAINS", "1")
    one = run_bundle(_gpu(p.cams, disable_convergence=True), p, 6)
    assert auto["rc"] == one["rc"] == 6 and auto["logs"] == one["logs"]
    assert np.array_equal(auto["R"], one["R"]) and np.array_equal(auto["t"], one["t"]) and np.array_equal(auto["X"], one["X"])


@pytest.mark.parametrize("n,nsys", [(1216, 1), (1216, 4), (3008, 2), (416, 1)])
def test_dissected_band_through_the_chain_kernels(gpu_required, n, nsys):
    """k_chol_persist_seg + the back-substitution with a workgroup per chain, outside the solver: a band of six tiles ordered [left half |
    right half reversed | the six block columns between them] and the plan told so (mcp_chol_time, band = -6: chains {0, h, ntc - 6}).
    Solutions of (A + q I) x = b against numpy; two calls give the same bits."""
    from mcptam_amd.chain_bundle import chol_time
    ntc = n // 32
    rng = np.random.default_rng(31 + n)
    B = rng.normal(size=(n, n))
    A = B @ B.T
    for i in range(ntc):
        for j in range(ntc):
            if abs(i - j) > 6:
                A[32 * i:32 * i + 32, 32 * j:32 * j + 32] = 0.0
    A += 5 * n * np.eye(n)
    h = (ntc - 6) // 2
    order = list(range(h)) + list(range(ntc - 1, h + 5, -1)) + list(range(h, h + 6))
    idx = np.concatenate([np.arange(32 * o, 32 * o + 32) for o in order])
    A = A[np.ix_(idx, idx)]
    b = rng.normal(size=n)
    _, _, x = chol_time(np.tril(A), b, nsys=nsys, reps=20, band=-6)
    _, _, x2 = chol_time(np.tril(A), b, nsys=nsys, reps=20, band=-6)
    assert np.array_equal(x, x2)
    for q in range(nsys):
        ref = np.linalg.solve(A + q * np.eye(n), b)
        assert rel_err(x[q], ref) < 1e-11, (n, q)
