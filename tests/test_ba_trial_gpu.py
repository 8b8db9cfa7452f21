"""One LM trial step (mcp_ba::launch_trial_step in csrc/ba_solver.hip: k_trial_apply, or k_update_poses + k_backsub /
k_apply_point_step + k_chains; then k_eval and k_final_sums) through ChainBundle.DebugTrial(), at the size seams of its kernels and at
the value branches of the state update.

a. The solver's own step on the maps of ba_shapes.py, each under three paths -- the default (small bundle: one chain workgroup),
   MCP_BA_SMALL=0 (ceil(nchain / 64) chain workgroups) and MCP_BA_SMALL=0 MCP_BA_TRIAL_FUSE=0 (the separate kernels):
     pts1 ... pts129                      free points against the 64 points of a back-substitution workgroup (nbb = 1, 1, 1, 2, 3)
     shared*_66, roll5, big_*, meas, calib17    1, 2, 5, 6, 13 and 17 incidences per point, and points with none, on 4 lanes
     chains64 ... chains129               chains against the 64 of a chain workgroup (ncb = 1, 2, 2, 3 under MCP_BA_SMALL=0)
     poses255, poses256, poses257         poses against the 256 a chain workgroup keeps in LDS (257: the separate kernels, always)
   DebugTrial()'s report is asserted first: the case means what its name says only if it took that path.
b. A given step at the value edges (ba_trial_cases.edge_step): the exponential either side of theta^2 = 1e-8 and 1e-6, |w| = 3,
   the clamps of a point's distance to [1e-5, 1e5] and a point that flips through infinity.
c. The handle afterwards: nothing was accepted, nothing the next Compute() reads was touched.

References: ba_trial_cases.oplus_reference in longdouble (closed forms, written from the mathematics) for the state; the oracle
for x, b and -- on a second OracleBundle populated with the device's trial state -- for chi2.  Tolerances are the project's
(x 1e-7, chi2 1e-10, robust sum 1e-11, sum x^2 1e-12, sum x (lambda x + b) ten times the 1e-9 of the right-hand sides) but one:

THE STATE TOLERANCE is taken from the reference alone.  F = the float64 run of oplus_reference against its longdouble run (per
row -- a rotation, a translation, a point -- element-wise relative with a floor of 1e-3 of the row's largest entry), the maximum
over all cases of a. and b.; the tolerance is max(16 F, 64 * 2^-53).  Measured by test_ba_trial_cpu.py (x86-64, glibc 2.35, numpy 2.2,
numpy longdouble = 80-bit extended), which also asserts the constants below against what it measures:
    poses                F = 6.82e-14   tolerance 1.10e-12
    points               F = 6.07e-14   tolerance 9.8e-13
    depth-edge points    F = 1.19e-12   tolerance 1.91e-11   (value-edge step only: the new inverse depth rho + u2 is a difference
                                                              that loses up to five digits in any float64 evaluation)
One difference to the closed form is no rounding error and is allowed for by its formula, not by a tolerance
(ba_trial_cases.series_allowance): below theta^2 = 1e-8 SE3::exp -- TooN's, hence the oracle's and the solver's -- takes
t + (w x t) / 2 for the translation of the step, which leaves out up to theta^2 / 6 = 1.7e-9 of it.
"""
import numpy as np
import pytest

import ba_trial_cases as tc
from ba_shapes import get_map
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL_X, TOL_CHI2, TOL_ROBUST, TOL_SS, TOL_SCALE = 1e-7, 1e-10, 1e-11, 1e-12, 1e-8
TOL_POSE, TOL_POINT, TOL_POINT_DEPTH = 1.10e-12, 9.8e-13, 1.91e-11
MIN_SIGMA_SQ = 0.5 ** 2                     # ChainBundle.sdMinMEstimatorSigma squared: the floor of the Huber kernel's sigma^2
PATHS = {"small": {}, "fused": {"MCP_BA_SMALL": "0"}, "separate": {"MCP_BA_SMALL": "0", "MCP_BA_TRIAL_FUSE": "0"}}
BYTES = ("x", "poses", "points", "chi2", "robust_chi2", "scale", "scale_pose", "scale_point", "ss", "ss_pose", "ss_point")
_ORACLE = {}


def _oracle(name):
    """What the oracle says about map `name` at its start state, computed once and never modified."""
    if name not in _ORACLE:
        from oracle import OracleBundle
        p = get_map(name)
        o = OracleBundle(p.cams, True, True, False)
        lay = tc.layout(p, p.populate(o))
        poses, points = tc.current_state(o, lay)
        rc, xs, xd = o.DebugSolve(tc.LAMBDA)
        assert rc == 0
        b = o.DebugRhs()
        _, sigma_sq_raw = o.DebugRobustChi2()
        for a in (poses, points, xs, xd, b):
            a.setflags(write=False)
        _ORACLE[name] = dict(lay=lay, poses=poses, points=points, xs=xs, xd=xd, b=b, sigma_sq=max(sigma_sq_raw, MIN_SIGMA_SQ))
    return _ORACLE[name]


def _setup(monkeypatch, path):
    from mcptam_amd import chain_bundle
    chain_bundle.struct_cache_clear()
    for k in ("MCP_BA_SMALL", "MCP_BA_TRIAL_FUSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def _gpu(name):
    from mcptam_amd.chain_bundle import ChainBundle
    p = get_map(name)
    g = ChainBundle(p.cams, True, True, False)
    p.populate(g)
    return g


def _trial_chi2_of_the_oracle(name, lay, poses, points):
    """chi2 per measurement of the oracle on a second bundle populated with the trial state (poses, points)."""
    from oracle import OracleBundle
    p = get_map(name)
    q = tc.replaced_problem(p, lay, poses, points)
    o2 = OracleBundle(q.cams, True, True, False)
    lay2 = tc.layout(q, q.populate(o2))
    P2, X2 = tc.current_state(o2, lay2)
    assert np.array_equal(P2, poses) and np.array_equal(X2, points)          # the second bundle holds the device's trial state, bit for bit
    return o2.Eval()[0]


def _huber_sum(chi2, sigma_sq):
    """sum of the Huber-robustified chi2 (MEstimator.h / g2o RobustKernelHuber: e^2 below sigma^2, 2 sigma e - sigma^2 above) in longdouble"""
    c = np.asarray(chi2, dtype=tc.LD)
    s2 = tc.LD(sigma_sq)
    return float(np.where(c <= s2, np.abs(c), 2 * np.sqrt(s2) * np.sqrt(np.maximum(c, 0)) - s2).sum())


def _expected_ncb(path, nchain, npose):
    if npose > 256 or path == "separate":
        return 0
    return 1 if path == "small" else max(1, -(-nchain // 64))


def _incidences(p):
    """free keyframes a free point touches, per free point (multi maps)"""
    import ba_shapes
    return [len(ba_shapes.problem_poses(p, i)) for i in range(p.n_points) if not p.pt_fixed[i]]


EXPECT = {          # name -> report entries that make the case mean what it is named for
    "pts1": dict(nfl=1, nbb=1), "pts63": dict(nfl=63, nbb=1), "pts64": dict(nfl=64, nbb=1), "pts65": dict(nfl=65, nbb=2), "pts129": dict(nfl=129, nbb=3),
    "chains64": dict(nchain=64), "chains65": dict(nchain=65), "chains128": dict(nchain=128), "chains129": dict(nchain=129),
    "poses255": dict(npose=255), "poses256": dict(npose=256), "poses257": dict(npose=257),
}
INCIDENCES = {"shared1_66": {1}, "shared2_66": {2}, "shared13_66": {13}, "roll5": {5}, "big_all": {17}, "big_one": {6, 17},
              "meas": {0, 1, 2, 3, 4, 5, 6}}


@pytest.mark.parametrize("name", tc.SOLVER_STEP_MAPS)
def test_solver_step_at_the_size_seams(gpu_required, name, monkeypatch):
    ref = _oracle(name)
    lay, p = ref["lay"], get_map(name)
    if name in INCIDENCES:
        assert set(_incidences(p)) == INCIDENCES[name], name
    outs = {}
    for path in PATHS:
        _setup(monkeypatch, path)
        g = _gpu(name)
        cur_poses, cur_points = tc.current_state(g, lay)
        assert np.array_equal(cur_poses, ref["poses"]) and np.array_equal(cur_points, ref["points"])
        d = g.DebugTrial(tc.LAMBDA)
        g.close()
        what = "%s/%s" % (name, path)
        report = {k: d[k] for k in ("ncb", "nbb", "nchain", "npose", "npoint", "nfl", "np", "nmeas", "small_mode", "given_step")}
        print(what, report)
        # 1. the path
        assert not d["given_step"] and d["small_mode"] == (path == "small"), report
        assert d["ncb"] == _expected_ncb(path, d["nchain"], d["npose"]), report
        assert d["nbb"] == -(-4 * d["nfl"] // 256) and d["npose"] == len(lay.pose_ids) and d["nfl"] == len(lay.free_point) and d["np"] == 6 * len(lay.free_pose), report
        for k, v in EXPECT.get(name, {}).items():
            assert d[k] == v, (what, k, report)
        if name == "poses257":
            assert d["ncb"] == 0, report
        n_p = d["np"]
        x = d["x"]
        # 2. the step that was applied is the oracle's solution, pose part and point part each under its own norm
        xs, xd = ref["xs"], ref["xd"]
        assert rel_err(xs[:n_p], xd[:n_p]) < TOL_X and rel_err(xs[n_p:], xd[n_p:]) < TOL_X          # the oracle's two solvers agree part by part
        e_xp, e_xl = rel_err(x[:n_p], xs[:n_p]), rel_err(x[n_p:], xs[n_p:])
        print("%s: x pose part %.2e point part %.2e" % (what, e_xp, e_xl))
        assert e_xp < TOL_X and e_xl < TOL_X, (what, e_xp, e_xl)
        # 3. the trial state is the reference's oplus of the device's own step
        PL, XL = tc.oplus_reference(ref["poses"][lay.free_pose], ref["points"][lay.free_point], x, tc.LD)
        e_p = tc.pose_error(d["poses"][lay.free_pose], PL, tc.series_allowance(ref["poses"][lay.free_pose], x))
        e_x = tc.state_error(d["points"][lay.free_point], XL)
        print("%s: trial state against the reference: poses %.2e points %.2e" % (what, e_p, e_x))
        assert e_p <= TOL_POSE, (what, e_p)
        assert e_x <= TOL_POINT, (what, e_x)
        # 4. what is fixed stays, bit for bit
        assert np.array_equal(d["poses"][lay.fixed_pose], ref["poses"][lay.fixed_pose]), what
        assert np.array_equal(d["points"][lay.fixed_point], ref["points"][lay.fixed_point]), what
        # 5. the trial chi2 is the oracle's on that state (chain transforms of the trial state + k_eval)
        chi_o = _trial_chi2_of_the_oracle(name, lay, d["poses"], d["points"])
        e_c = rel_err(d["chi2"], chi_o)
        print("%s: chi2 %.2e" % (what, e_c))
        assert e_c < TOL_CHI2, (what, e_c)
        # 6. sum x^2 over the device's x
        xl = np.asarray(x, dtype=tc.LD)
        for key, part in (("ss_pose", xl[:n_p]), ("ss_point", xl[n_p:]), ("ss", xl)):
            want = float((part * part).sum())
            assert abs(d[key] - want) <= TOL_SS * want, (what, key, d[key], want)
        # 7. sum x (lambda x + b) with the device's x and the oracle's b
        t = xl * (tc.LD(tc.LAMBDA) * xl + np.asarray(ref["b"], dtype=tc.LD))
        for key, part in (("scale_pose", t[:n_p]), ("scale_point", t[n_p:]), ("scale", t)):
            want, mag = float(part.sum()), float(np.abs(part).sum())
            assert abs(d[key] - want) <= TOL_SCALE * mag, (what, key, d[key], want, mag)
        # 8. the robust chi2 sum of the result block: the oracle's chi2 of the trial state under the Huber kernel at the sigma of the
        #    CURRENT state (a trial is robustified with the sigma its iteration started with; the oracle's DebugRobustChi2() on the
        #    second bundle would take the trial state's own median)
        want = _huber_sum(chi_o, ref["sigma_sq"])
        assert abs(d["robust_chi2"] - want) <= TOL_ROBUST * want, (what, d["robust_chi2"], want)
        outs[path] = d
    # 9. the three paths give the same bytes
    for path in ("fused", "separate"):
        for k in BYTES:
            assert np.array_equal(np.asarray(outs[path][k]), np.asarray(outs["small"][k])), (name, path, k)


@pytest.mark.parametrize("name", tc.EDGE_MAPS)
def test_given_step_at_the_value_edges(gpu_required, name, monkeypatch):
    _setup(monkeypatch, "small")
    ref = _oracle(name)
    lay, p = ref["lay"], get_map(name)
    x, th2s, kinds = tc.edge_step(p, lay, ref["points"])
    by_kind = tc.assert_edge_branches(ref["poses"], ref["points"], lay, x, th2s, kinds)
    assert {"far_clamped", "near_clamped", "flipped"} <= set(by_kind)
    g = _gpu(name)
    d = g.DebugTrial(tc.LAMBDA, x=x)
    g.close()
    assert d["given_step"] and d["ncb"] == 0, d
    assert np.array_equal(d["x"], x)
    for k in ("scale", "scale_pose", "scale_point", "ss", "ss_pose", "ss_point"):
        assert d[k] == 0.0
    PL, XL = tc.oplus_reference(ref["poses"][lay.free_pose], ref["points"][lay.free_point], x, tc.LD)
    e_p = tc.pose_error(d["poses"][lay.free_pose], PL, tc.series_allowance(ref["poses"][lay.free_pose], x))
    depth = np.array([k in tc.DEPTH_KINDS for k in kinds])
    X = d["points"][lay.free_point]
    e_x, e_d = tc.state_error(X[~depth], XL[~depth]), tc.state_error(X[depth], XL[depth])
    print("%s: edge step against the reference: poses %.2e points %.2e depth-edge points %.2e" % (name, e_p, e_x, e_d))
    assert e_p <= TOL_POSE, (name, e_p)
    assert e_x <= TOL_POINT, (name, e_x)
    assert e_d <= TOL_POINT_DEPTH, (name, e_d)
    assert np.array_equal(d["poses"][lay.fixed_pose], ref["poses"][lay.fixed_pose]) and np.array_equal(d["points"][lay.fixed_point], ref["points"][lay.fixed_point])
    # the clamped points lie at 1e5 and 1e-5, the flipped ones in the reference's direction
    dist = np.sqrt((np.asarray(X, dtype=tc.LD) ** 2).sum(axis=1))
    for kind, want in (("far_clamped", tc.DIST_MAX), ("very_far_clamped", tc.DIST_MAX), ("near_clamped", tc.DIST_MIN), ("very_near_clamped", tc.DIST_MIN)):
        for j in by_kind.get(kind, []):
            assert abs(float(dist[j]) - want) <= 1e-12 * want, (name, kind, j, float(dist[j]))
    for j in by_kind["flipped"]:
        cosang = float((np.asarray(X[j], dtype=tc.LD) @ XL[j]) / (dist[j] * np.sqrt(XL[j] @ XL[j])))
        assert cosang > 1 - 1e-12 and float(X[j] @ ref["points"][lay.free_point[j]]) < 0, (name, j, cosang)
    # chi2 against the oracle on that state: over the measurements of ordinary points, and over those of clamped / flipped points
    chi_o = _trial_chi2_of_the_oracle(name, lay, d["poses"], d["points"])
    wild = np.zeros(p.n_points, dtype=bool)
    for kind in ("far_clamped", "very_far_clamped", "near_clamped", "very_near_clamped", "flipped"):
        wild[lay.free_point[by_kind.get(kind, [])]] = True
    mw = wild[p.ms_pt]
    assert mw.any() and (~mw).any()
    e_o, e_w = rel_err(d["chi2"][~mw], chi_o[~mw]), rel_err(d["chi2"][mw], chi_o[mw])
    print("%s: chi2 ordinary %.2e clamped / flipped %.2e (largest %.1e / %.1e)" % (name, e_o, e_w, np.abs(chi_o[~mw]).max(), np.abs(chi_o[mw]).max()))
    assert e_o < TOL_CHI2 and e_w < TOL_CHI2, (name, e_o, e_w)
    want = _huber_sum(chi_o, ref["sigma_sq"])
    assert abs(d["robust_chi2"] - want) <= TOL_ROBUST * want, (name, d["robust_chi2"], want)


def _run(g, ids):
    rc = g.Compute(5)
    R, t = g.GetPoses(ids["mkf"])
    return rc, g.IterLogs(), R.tobytes(), t.tobytes(), g.GetPoints(ids["point"]).tobytes(), g.GetLambda()


@pytest.mark.parametrize("path", ["small", "fused"])
@pytest.mark.parametrize("name", ["meas", "chains65"])
def test_the_handle_afterwards(gpu_required, name, path, monkeypatch):
    """Two DebugTrial() calls in a row give the same bytes; after solver steps and a given step, Compute(5) gives the logs and the
    state bytes a fresh handle gives."""
    from mcptam_amd.chain_bundle import ChainBundle
    _setup(monkeypatch, path)
    ref = _oracle(name)
    p = get_map(name)
    x, _, _ = tc.edge_step(p, ref["lay"], ref["points"])
    g = ChainBundle(p.cams, True, True, False)
    ids = p.populate(g)
    a = g.DebugTrial(tc.LAMBDA)
    b = g.DebugTrial(tc.LAMBDA)
    for k in BYTES:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (name, k)
    e1 = g.DebugTrial(tc.LAMBDA, x=x)
    c = g.DebugTrial(10.0)
    e2 = g.DebugTrial(tc.LAMBDA, x=x)
    for k in BYTES:
        assert np.array_equal(np.asarray(e1[k]), np.asarray(e2[k])), (name, k)
    assert not np.array_equal(c["x"], a["x"])
    cur_poses, cur_points = tc.current_state(g, ref["lay"])
    assert np.array_equal(cur_poses, ref["poses"]) and np.array_equal(cur_points, ref["points"])
    after = _run(g, ids)
    g.close()
    f = ChainBundle(p.cams, True, True, False)
    fresh = _run(f, p.populate(f))
    f.close()
    assert after[0] == fresh[0] > 0
    assert after[1] == fresh[1], (name, after[1], fresh[1])
    assert after[2:] == fresh[2:], name


def test_a_handle_with_several_ranks_is_refused(gpu_required, monkeypatch):
    from mcptam_amd.chain_bundle import ChainBundle
    _setup(monkeypatch, "small")
    monkeypatch.setenv("MCP_BA_FORCE_MULTI", "1")
    p = get_map("pts1")
    g = ChainBundle(p.cams, True, True, False)
    p.populate(g)
    g.SetAllReduce(lambda ptr, count, stream: None, 0, 1)
    with pytest.raises(RuntimeError, match="mcp_ba_debug_trial: refused"):
        g.DebugTrial(tc.LAMBDA)
    g.close()


def test_outputs_sized_for_another_map_are_refused(gpu_required, monkeypatch):
    from mcptam_amd.chain_bundle import ChainBundle
    _setup(monkeypatch, "small")
    p = get_map("pts1")
    g = ChainBundle(p.cams, True, True, False)
    p.populate(g)
    g._n_added[2] += 1
    with pytest.raises(RuntimeError, match="outputs sized for 9 poses, 1 points, 8 measurements, the handle has 9, 1, 7"):
        g.DebugTrial(tc.LAMBDA)
    with pytest.raises(ValueError, match="the step has 3 entries"):
        g.DebugTrial(tc.LAMBDA, x=np.zeros(3))
    g.close()
