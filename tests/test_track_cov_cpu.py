"""CPU-side checks of the tracker's pose covariance (include/mcp_img.h: mcp_track_pose_cov_enable, mcp_track_pose_cov_last,
mcp_track_pose_cov, mcp_track_pose_cov_host, mcp_debug_track_fine_records): the declarations exist and are exported, the ctypes layout is
the host compiler's, and the host entry -- track_cov.h under the host compiler, in the device's order -- agrees with the numpy restatement
pvs.pose_covariance_restate (math.fsum, numpy.linalg.eigh) and, through the CPU oracle's iterations cut to nine, with the pose the
reference linearises its last iteration at (src/Tracker.cc:1441, 1498-1502).

Bounds.  info: max|d| <= 1e-9 max|info|, the project's standing bound for doubles across math libraries.  cov: against the truncated
pseudo-inverse numpy gives for the RETURNED info, |d|_F <= 64 kappa 2^-52 |cov|_F with kappa numpy's condition number of that info: both
eigen-decompositions are backward stable (a relative perturbation of a few 2^-52 of info each), the inverse amplifies a relative
perturbation by kappa, and 64 covers the constants of two 6 x 6 decompositions; |cov info - I|_max by the same bound.  Inputs are chosen
and asserted to have kappa <= 1e6.

Measured: largest max|info - restatement| / max|info| = 3.2e-15 over the generated cases, 1.8e-16 against info rebuilt at the oracle's
nine-iteration pose (the rebuilt pose is 1.1e-16 from it); largest |cov - numpy pinv|_F / |cov|_F = 1.4 kappa 2^-52, largest
|cov info - I|_max = 0.5 kappa 2^-52; 3 to 6 sweeps."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from track_cov_cases import EPS, check_against_numpy, check_nan, check_rank2, make_records, nan_case, rank2_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd.pvs import _bind_track_cov, lib
    return _bind_track_cov(lib())


def test_cov_entry_points_declared_and_exported(built):
    from mcptam_amd import keyframe
    from mcptam_amd.pvs import POSE_COV_MAX_SWEEPS, TRACK_COV_SYMBOLS
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)
    assert re.search(r"#define MCP_POSE_COV_MAX_SWEEPS\s+%d\b" % POSE_COV_MAX_SWEEPS, txt)
    assert sorted(TRACK_COV_SYMBOLS) == ["mcp_debug_track_fine_records", "mcp_track_pose_cov", "mcp_track_pose_cov_enable", "mcp_track_pose_cov_host",
                                         "mcp_track_pose_cov_last"]
    L = ctypes.CDLL(os.path.join(ROOT, "mcptam_amd", "libmcptam_hip.so"))
    for n in TRACK_COV_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS


def test_cov_struct_layout_matches_the_header(tmp_path):
    from mcptam_amd.pvs import TrackPoseCov
    fs = ["valid", "n_used", "rank", "sweeps", "info", "cov", "eig", "norm_fro"]
    body = ['printf("%d\\n", (int)sizeof(mcp_track_pose_cov_record));'] + ['printf("%%d\\n", (int)offsetof(mcp_track_pose_cov_record, %s));' % f for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(TrackPoseCov)] + [getattr(TrackPoseCov, f).offset for f in fs]


def test_cpp_pose_cov_mirror_compiles_and_links(built, tmp_path):
    """include/mcptam_hip/KeyFrame.hpp's MapPointTable::PoseCovEnable / PoseCovLast / PoseCov / PoseCovHost, linked against libmcptam_hip.so;
    the host entry runs (it needs no GPU), the others are only linked."""
    src = tmp_path / "track_cov_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'static double use() {\n'
                   '  mcptam_hip::MapPointTable t(-1); t.PoseCovEnable(true);\n'
                   '  const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, mu[6] = {0};\n'
                   '  return t.PoseCovLast().norm_fro + mcptam_hip::MapPointTable::PoseCov({}, {}, std::vector<double>(I, I + 12), I, mu).norm_fro;\n}\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) {\n'
                   '    const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, mu[6] = {0};\n'
                   '    const mcp_track_pose_cov_record r = mcptam_hip::MapPointTable::PoseCovHost({}, {}, std::vector<double>(I, I + 12), I, mu);\n'
                   '    std::printf("linked %d %d %g %g\\n", r.valid, r.rank, r.cov[0], r.cov[1]); return 0;\n  }\n'
                   '  return use() > 0;\n}\n')
    exe = tmp_path / "track_cov_link"
    lib = os.path.join(ROOT, "mcptam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lmcptam_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linked 1 6 0.01 0" in out.stdout      # no record: the prior's covariance


@pytest.mark.parametrize("ncam", [1, 4])
@pytest.mark.parametrize("n", [1, 2, 64, 300])
def test_host_entry_is_the_numpy_restatement(built, n, ncam):
    from mcptam_amd.pvs import pose_cov_arrays, pose_cov_host, pose_covariance_restate
    worst = 0.0
    for seed in (3, 4):
        pts, w, cfbs, refined, mu = make_records(n, ncam, 1000 * n + 10 * ncam + seed)
        if n <= 2:
            pts["found"] = 1; w[:] = 0.7                                  # (the mixed cases are the larger ones; below, the not-found / zero-weight singles)
        rec = pose_cov_host(pts, w, cfbs, refined, mu)
        ref = pose_covariance_restate(pts, w, cfbs, refined, mu)
        info = pose_cov_arrays(rec)[0]
        d = np.abs(info - ref["info"]).max() / np.abs(info).max()
        worst = max(worst, d)
        print("n %d ncam %d seed %d: n_used %d  max|info - restatement| / max|info| = %.3g" % (n, ncam, seed, rec.n_used, d))
        assert rec.valid == 1 and rec.n_used == ref["n_used"] == int(((pts["found"] != 0) & (w != 0)).sum())
        assert d <= 1e-9
        check_against_numpy(rec, "n %d ncam %d seed %d:" % (n, ncam, seed))
    if n >= 64:
        assert 0 < rec.n_used < n                                         # both kinds of unused record took part
    print("largest relative info difference", worst)


def test_no_usable_record_gives_the_prior_exactly(built):
    from mcptam_amd.pvs import pose_cov_arrays, pose_cov_host
    pts, w, cfbs, refined, mu = make_records(5, 2, 7)
    for found, weight in ((0, 0.5), (1, 0.0)):
        q = pts.copy(); q["found"] = found
        rec = pose_cov_host(q, np.full(5, weight), cfbs, refined, mu)
        info, cov, eig = pose_cov_arrays(rec)
        assert rec.valid == 1 and rec.n_used == 0 and rec.rank == 6 and rec.sweeps == 0
        assert np.array_equal(info, 100.0 * np.eye(6)) and np.array_equal(cov, 0.01 * np.eye(6)) and np.array_equal(eig, np.full(6, 100.0))
    rec = pose_cov_host(pts[:0], w[:0], cfbs, refined, mu)                 # no record at all
    assert rec.valid == 1 and rec.n_used == 0 and rec.rank == 6 and rec.sweeps == 0 and np.array_equal(pose_cov_arrays(rec)[1], 0.01 * np.eye(6))


def test_one_heavy_record_truncates_the_prior(built):
    from mcptam_amd.pvs import pose_cov_host
    check_rank2(pose_cov_host(*rank2_case()))


def test_a_nan_derivative_is_reported_and_returns(built):
    from mcptam_amd.pvs import pose_cov_host
    check_nan(pose_cov_host(*nan_case()))


def test_dense_spd_sums_stay_under_the_sweep_cap(built):
    """Dense information matrices of every scale mix the generator reaches: four cameras, strong rotations between them, derivatives with
    large off-diagonal parts."""
    from mcptam_amd.pvs import pose_cov_arrays, pose_cov_host
    most = 0
    for seed in range(12):
        pts, w, cfbs, refined, mu = make_records(40 + 17 * seed, 4, 500 + seed, found_frac=1.0, zero_w_frac=0.0)
        rng = np.random.default_rng(seed)
        pts["cam_derivs"] = rng.normal(0, 80.0, (len(pts), 4))
        rec = pose_cov_host(pts, w, cfbs, refined, mu)
        info = pose_cov_arrays(rec)[0]
        off = np.abs(info - np.diag(np.diag(info))).max() / np.abs(np.diag(info)).min()
        assert rec.valid == 1 and off > 0.05, off                         # (dense: off-diagonal entries comparable to the smallest diagonal one)
        assert 1 <= rec.sweeps <= 16
        most = max(most, rec.sweeps)
        check_against_numpy(rec, "dense %d:" % seed)
    print("most sweeps", most)


def test_refusals(built):
    from mcptam_amd import chain_bundle
    from mcptam_amd.keyframe import _pose12
    from mcptam_amd.pvs import TrackPoseCov
    L = built
    pts, w, cfbs, refined, mu = make_records(4, 2, 17)
    cfb = np.ascontiguousarray(np.stack([_pose12(*c) for c in cfbs]))
    ref = _pose12(*refined).copy()
    out = TrackPoseCov()
    good = [4, pts.ctypes.data, w.ctypes.data, 2, cfb.ctypes.data, ref.ctypes.data, mu.ctypes.data, ctypes.byref(out)]
    assert L.mcp_track_pose_cov_host(*good) == 0
    for k, v in ((0, -1), (1, None), (2, None), (3, 0), (4, None), (5, None), (6, None), (7, None)):
        a = list(good); a[k] = v
        assert L.mcp_track_pose_cov_host(*a) == -1 and chain_bundle.last_error()
    bad = pts.copy(); bad["cam"][2] = 2
    a = list(good); a[1] = bad.ctypes.data
    assert L.mcp_track_pose_cov_host(*a) == -1 and "camera index" in chain_bundle.last_error()
    assert L.mcp_track_pose_cov_enable(None, 1) == -1 and L.mcp_track_pose_cov_last(None, ctypes.byref(out)) == -1
    n = ctypes.c_int(0)
    assert L.mcp_debug_track_fine_records(None, 0, None, None, mu.ctypes.data, ctypes.byref(n)) == -1


def _refine_scene():
    """The two-camera refinement scene of tests/test_oracle_cpu.py: 280 map points searched by the CPU oracle from a slightly wrong pose."""
    from mcptam_amd import synth, synth_img
    from mcptam_amd.keyframe import pose_points
    from oracle import OracleKeyFrame, oracle_track_search
    sc = synth_img.make_tracking_scene(size=(320, 240))
    cam = sc["cam"]
    A, B = OracleKeyFrame(320, 240), OracleKeyFrame(320, 240)
    A.MakeKeyFrame_Lite(sc["imgA"]); B.MakeKeyFrame_Lite(sc["imgB"]); A.MakeKeyFrame_Rest()
    pts = synth_img.make_map_points(cam, A, A, sc["poseA"], sc["depth"], per_level=(150, 80, 40, 10))
    cfbs = [(np.eye(3), np.zeros(3)), (synth.so3_exp(np.array([0.0, 0.02, 0.0])), np.array([0.01, 0.0, 0.0]))]
    RB, tB = sc["poseB"]
    dR, dt = synth.se3_exp(np.array([0.004, -0.003, 0.002, 0.001, -0.0015, 0.0008]))
    bfw = (dR @ RB, dR @ tB + dt)
    recs = []
    for c, cfb in enumerate(cfbs):
        sub = pts if c == 0 else pts[::2]
        out = oracle_track_search(B, cam, bfw, cfb, sub, 10, 8)
        recs.append(pose_points(np.array([p["world_pos"] for p in sub]), out, c))
    return cam, cfbs, bfw, np.concatenate(recs)


def test_linearisation_point_is_the_references(built):
    """The reference linearises its last iteration at the pose it then holds.  The CPU oracle's iterations cut to nine give that pose; the
    full ten give the refined pose, mu, the weights and the records as the last re-projection left them.  info rebuilt in numpy AT THE
    NINE-ITERATION POSE against the host entry fed the ten-iteration results (which rebuilds the pose as exp(-mu) * refined): 1e-9."""
    from mcptam_amd.keyframe import FINE_NONLINEAR, FINE_OVERRIDE
    from mcptam_amd.pvs import pose_cov_arrays, pose_cov_host, pose_covariance_restate
    from oracle import oracle_track_pose_refine
    cam, cfbs, bfw, recs = _refine_scene()
    assert recs["found"].sum() > 150
    pose9, _, _, _ = oracle_track_pose_refine(recs, [cam, cam], cfbs, bfw, FINE_NONLINEAR[:9], FINE_OVERRIDE[:9])
    pose10, mu, w, out = oracle_track_pose_refine(recs, [cam, cam], cfbs, bfw)
    assert np.abs(mu).max() > 0 and (w > 0).sum() > 100 and (w == 0).sum() > 0
    ref = pose_covariance_restate(out, w, cfbs, pose10, mu, pose_before=pose9)
    rebuilt = pose_covariance_restate(out, w, cfbs, pose10, mu)["pose_before"]
    dp = max(np.abs(rebuilt[0] - pose9[0]).max(), np.abs(rebuilt[1] - pose9[1]).max())
    rec = pose_cov_host(out, w, cfbs, pose10, mu)
    info = pose_cov_arrays(rec)[0]
    d = np.abs(info - ref["info"]).max() / np.abs(info).max()
    print("|exp(-mu) refined - pose before update 9| = %.3g   max|info - info at that pose| / max|info| = %.3g   n_used %d" % (dp, d, rec.n_used))
    assert rec.valid == 1 and rec.n_used == int((w != 0).sum()) == ref["n_used"]
    assert d <= 1e-9
    check_against_numpy(rec, "oracle scene:")
