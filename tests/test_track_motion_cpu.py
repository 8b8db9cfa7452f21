"""CPU-side checks of the one-call TrackFrame's motion model (include/mcp_img.h: mcp_track_frame_motion, mcp_track_motion_reset,
mcp_track_motion_get_sbi, mcp_track_motion_prior_host, mcp_track_motion_update_host): the declarations exist and are exported, the ctypes
layouts are the host compiler's, the C++ mirror links, the logarithms invert the exponentials, and the host entries -- the source the two
motion kernels run, under the host compiler -- agree with the numpy restatement of Tracker::ApplyMotionModel / CalcSBIRotation /
FindAverageRotation / UpdateMotionModel (src/Tracker.cc:1516-1555, 1687-1749), SE3fromSE2 taken from the CPU oracle."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = [np.array(a, dtype=np.float64) / np.linalg.norm(a) for a in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, -2, 3], [-0.3, 0.5, 0.81])]
ANGLES = [0.0, 1e-9, 1e-4, 0.3, 1.5, 3.0]
TRANSLATIONS = [np.zeros(3), np.array([1e-3, 0.0, 0.0]), np.array([0.3, -0.4, 0.5]), np.array([-6.0, 0.0, 8.0])]      # norms 0 .. 10


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    return cc


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd.pvs import _bind_track_motion, lib
    return _bind_track_motion(lib())


def _sbi_cam():
    from mcptam_amd.synth import DEFAULT_CAM_PARAMS
    from mcptam_amd.taylor_camera import TaylorCamera
    return TaylorCamera(DEFAULT_CAM_PARAMS, (640, 480), (640, 480), (40, 30))


def _se2(angle, tx, ty):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c, -s, s, c, tx, ty])


def _p12(R, t):
    return np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3)])


def test_motion_entry_points_declared_and_exported(built):
    from mcptam_amd.pvs import TRACK_MOTION_SYMBOLS
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)
    for s in ("mcp_track_motion_params", "mcp_track_motion"):
        assert re.search(r"typedef struct %s\s*\{" % s, txt), s
    assert len(TRACK_MOTION_SYMBOLS) == 5
    L = ctypes.CDLL(os.path.join(ROOT, "mcptam_amd", "libmcptam_hip.so"))
    for n in TRACK_MOTION_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n


def test_motion_struct_layouts_match_the_header(tmp_path):
    from mcptam_amd.pvs import TrackMotion, TrackMotionParams
    fields = {"mcp_track_motion_params": (TrackMotionParams, ["apply", "use_rotation_estimator", "sbi_iterations", "blur", "dt", "velocity", "cam_good"]),
              "mcp_track_motion": (TrackMotion, ["start", "prior", "se2", "sbi_score", "cam_rot", "sbi_rot", "n_used", "avg_rounds", "first_frame", "v_new", "velocity"])}
    body = []
    for s, (_, fs) in fields.items():
        body.append('printf("%%d\\n", (int)sizeof(%s));' % s)
        body += ['printf("%%d\\n", (int)offsetof(%s, %s));' % (s, f) for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_cc(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for s, (cls, fs) in fields.items():
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f).offset for f in fs]
    assert got == want


def test_cpp_track_frame_motion_mirror_compiles_and_links(built, tmp_path):
    """include/mcptam_hip/KeyFrame.hpp's MapPointTable::TrackFrameMotion / MotionReset / MotionSBI, linked against libmcptam_hip.so (not run: no GPU)."""
    src = tmp_path / "track_motion_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'static int use(int argc) {\n'
                   '  mcptam_hip::MapPointTable t(-1);\n'
                   '  mcptam_hip::KeyFrame kf(640, 480); std::vector<mcptam_hip::KeyFrame*> ks{&kf};\n'
                   '  std::vector<mcp_camera> cams(1), sbi(1); double bfw[12] = {0}; std::vector<double> cfb(12);\n'
                   '  mcp_track_map_params p; std::memset(&p, 0, sizeof p); mcp_track_record_params rp; std::memset(&rp, 0, sizeof rp);\n'
                   '  mcp_track_motion_params mp; std::memset(&mp, 0, sizeof mp); mp.blur = 0.75; mp.dt = 0.03; mp.apply = argc;\n'
                   '  mcp_track_map_result r; mcp_track_record rec; mcp_track_motion mo;\n'
                   '  t.TrackFrameMotion(ks, {}, {}, false, cams, sbi, bfw, cfb, p, rp, mp, &r, &rec, &mo);\n'
                   '  std::vector<float> templ(1200); t.MotionSBI(0, 1, nullptr, templ.data(), nullptr); t.MotionReset();\n'
                   '  return mo.n_used + (int)templ[0];\n}\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) { std::printf("linked\\n"); return 0; }\n'
                   '  return use(argc);\n}\n')
    exe = tmp_path / "track_motion_link"
    lib = os.path.join(ROOT, "mcptam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lmcptam_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linked" in out.stdout


def test_logarithms_invert_the_exponentials():
    """so3_exp(so3_ln(R)) == R and se3_exp(se3_ln(T)) == T to 1e-12 (the suite's orthogonality bound), over 0 .. 3 rad about five axes."""
    from mcptam_amd.pvs import se3_exp, se3_ln, so3_exp, so3_ln
    worst_r = worst_t = 0.0
    for ax in AXES:
        for th in ANGLES:
            R = so3_exp(ax * th)
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
            w = so3_ln(R)
            assert abs(np.linalg.norm(w) - th) <= 1e-12
            worst_r = max(worst_r, np.abs(so3_exp(w) - R).max())
            for t in TRANSLATIONS:
                R2, t2 = se3_exp(se3_ln(R, t))
                worst_r = max(worst_r, np.abs(R2 - R).max())
                worst_t = max(worst_t, np.abs(t2 - t).max())
    print("largest round-trip difference: rotation %.3g, translation %.3g" % (worst_r, worst_t))
    assert worst_r <= 1e-12 and worst_t <= 1e-12


def test_update_host_logarithm_exponentiates_back(built):
    """mcp_track_motion_update_host with dt = 1 and no old velocity: v_new = SE3::ln(refined * start^-1) must exponentiate back to that
    product to 1e-12, and the velocity is 0.45 v_new."""
    from mcptam_amd.pvs import motion_params, motion_update, motion_update_host, se3_exp, so3_exp
    Rs, ts = so3_exp(np.array([0.2, -0.1, 0.4])), np.array([0.5, -0.2, 0.3])
    worst = worst_np = 0.0
    for ax in AXES:
        for th in ANGLES:
            for t in TRANSLATIONS:
                Rd = so3_exp(ax * th)
                Rr, tr = Rd @ Rs, Rd @ ts + t                            # refined = (Rd, t) * start
                Rd_, td_ = Rr @ Rs.T, tr - Rr @ Rs.T @ ts                # ... and the product the C code forms, in double
                v_new, vel = motion_update_host(_p12(Rs, ts), _p12(Rr, tr), motion_params(np.zeros(6), dt=1.0))
                Re, te = se3_exp(v_new)
                worst = max(worst, np.abs(Re - Rd_).max(), np.abs(te - td_).max())
                assert np.array_equal(vel, (0.5 * v_new + 0.5 * np.zeros(6)) * 0.9)
                v_np, _ = motion_update((Rs, ts), (Rr, tr), np.zeros(6), 1.0)
                worst_np = max(worst_np, np.abs(v_np - v_new).max())
    print("largest |exp(v_new) - refined * start^-1| %.3g; largest |v_new - numpy restatement| %.3g" % (worst, worst_np))
    assert worst <= 1e-12
    assert worst_np <= 1e-9
    # a non-zero old velocity and dt: 0.9 (0.5 v / dt + 0.5 old); apply = 0: the velocity as given, v_new zeros
    old = np.array([0.1, -0.2, 0.3, 0.01, 0.02, -0.03])
    Rd = so3_exp(np.array([0.02, 0.01, -0.03]))
    start, refined = _p12(Rs, ts), _p12(Rd @ Rs, Rd @ ts + np.array([0.01, 0.0, -0.02]))
    v1, _ = motion_update_host(start, refined, motion_params(np.zeros(6), dt=1.0))
    v_new, vel = motion_update_host(start, refined, motion_params(old, dt=0.04))
    assert np.allclose(v_new, v1 / 0.04, rtol=1e-15, atol=0) and np.allclose(vel, 0.9 * (0.5 * v_new + 0.5 * old), rtol=1e-15, atol=0)
    v_new, vel = motion_update_host(start, refined, motion_params(old, dt=0.04, apply=False))
    assert np.array_equal(v_new, np.zeros(6)) and np.array_equal(vel, old)


def _prior_case(ncam, kind, rng):
    from mcptam_amd.pvs import so3_exp
    good = [1] * ncam
    apply_, use = True, True
    se2 = np.array([_se2(rng.uniform(0.02, 0.06) * (-1) ** c, rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0)) for c in range(ncam)])
    if kind == "one_unused":
        good[ncam - 1] = 0
    elif kind == "none_used":
        good = [0] * ncam
    elif kind == "no_estimator":
        use = False
    elif kind == "identity_se2":
        se2 = np.array([_se2(0.0, 0.0, 0.0) for _ in range(ncam)])
    elif kind == "no_apply":
        apply_ = False
    # CamFromBase: distinct rotations of 0.01 rad and more; start: a rotation of 0.3 rad and a translation of norm 0.62, so exp * start and
    # start * exp differ by far more than 1e-4 (checked below)
    cfb = [(so3_exp(np.array([0.01 + 0.3 * c, -0.2 * c, 0.05 * (c % 3)])), rng.uniform(-0.1, 0.1, 3)) for c in range(ncam)]
    start = (so3_exp(np.array([0.2, -0.1, 0.2])), np.array([0.5, -0.2, 0.3]))
    velocity = np.array([0.6, -0.9, 0.45, 0.5, -0.4, 0.7])            # x dt = 0.04: 0.05 in translation, 0.04 rad in rotation
    return dict(se2=se2, good=good, apply=apply_, use=use, cfb=cfb, start=start, velocity=velocity, dt=0.04)


@pytest.mark.parametrize("ncam", [1, 2, 8])
@pytest.mark.parametrize("kind", ["all_used", "one_unused", "none_used", "no_estimator", "identity_se2", "no_apply"])
def test_prior_host_is_the_numpy_restatement(built, ncam, kind):
    """mcp_track_motion_prior_host against motion_prior (numpy, SE3fromSE2 from the CPU oracle): atol 1e-9 on prior, cam_rot and sbi_rot --
    what tests/test_img_gpu.py grants SE3fromSE2 across implementations."""
    from mcptam_amd.pvs import average_rotation, motion_params, motion_prior, motion_prior_host, se3_exp, so3_exp, so3_ln
    from oracle import oracle_sbi_se3_from_se2
    rng = np.random.default_rng(100 * ncam + len(kind))
    k = _prior_case(ncam, kind, rng)
    cam = _sbi_cam()
    mp = motion_params(k["velocity"], k["dt"], k["good"], k["apply"], k["use"], 6, 0.75, ncam)
    got = motion_prior_host(k["se2"], [cam] * ncam, np.array([_p12(*c) for c in k["cfb"]]), _p12(*k["start"]), mp)
    ref = motion_prior(k["se2"], [cam] * ncam, k["cfb"], k["start"], k["velocity"], k["dt"], k["good"], k["apply"], k["use"], se3_from_se2=oracle_sbi_se3_from_se2)
    prior, cam_rot, sbi_rot = np.array(got.prior), np.array([list(r) for r in got.cam_rot]), np.array(got.sbi_rot)
    d = max(np.abs(prior - _p12(*ref["prior"])).max(), np.abs(cam_rot[:ncam] - ref["cam_rot"]).max(), np.abs(sbi_rot - ref["sbi_rot"]).max())
    print("ncam %d %s: largest difference %.3g, n_used %d, rounds %d (numpy %d)" % (ncam, kind, d, got.n_used, got.avg_rounds, ref["avg_rounds"]))
    assert d <= 1e-9
    assert np.array_equal(np.array(got.start), _p12(*k["start"]))
    assert got.n_used == ref["n_used"] and not cam_rot[ncam:].any()
    n_used = 0 if kind in ("none_used", "no_estimator", "no_apply") else (ncam - 1 if kind == "one_unused" else ncam)
    assert got.n_used == n_used
    if n_used:
        # the loop's own stopping test holds for the mean reported, within the cap
        assert 1 <= got.avg_rounds <= 32
        used = [cam_rot[c] for c in range(ncam) if k["good"][c]]
        R = so3_exp(sbi_rot)
        r = sum(so3_ln(R.T @ so3_exp(q)) for q in used) / len(used)
        assert r @ r < 1e-3 * 1e-3
        assert np.abs(average_rotation(used)[0] - sbi_rot).max() <= 1e-9
    else:
        assert got.avg_rounds == 0 and not sbi_rot.any() and not cam_rot.any()
    Rs, ts = k["start"]
    if kind == "no_apply":
        assert prior.tobytes() == _p12(Rs, ts).tobytes()
        return
    v6 = k["velocity"] * k["dt"]
    if kind == "identity_se2":
        assert not cam_rot.any() and not sbi_rot.any()                 # exactly zero, and it replaces the velocity's rotation
        v6[3:] = 0
    elif n_used:
        v6[3:] = sbi_rot
    if kind in ("none_used", "no_estimator"):
        assert np.array_equal(v6[3:], k["velocity"][3:] * k["dt"])      # the rotation comes from the velocity
    # exp(v6) * start, not start * exp(v6): the two orders are more than 1e-4 apart here
    Re, te = se3_exp(v6)
    left, right = _p12(Re @ Rs, Re @ ts + te), _p12(Rs @ Re, Rs @ te + ts)
    assert np.abs(left - right).max() > 1e-4
    assert np.abs(prior - left).max() <= 1e-9 and np.abs(prior - right).max() > 1e-4


def test_a_non_converging_average_stops_at_the_cap():
    """Two rotations half a turn apart about one axis have no unique mean: the loop is cut off, never left to spin."""
    from mcptam_amd.pvs import average_rotation
    mean, rounds = average_rotation([np.array([0.0, 0.0, 3.0]), np.array([0.0, 0.0, -3.0]), np.array([0.0, 3.0, 0.0])], max_rounds=32)
    assert 1 <= rounds <= 32 and np.isfinite(mean).all()


def test_host_entries_refuse_bad_arguments(built):
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import TrackMotion, motion_params
    from mcptam_amd.taylor_camera import camera_array
    L = built
    cam = _sbi_cam()
    cs = camera_array([cam, cam])
    bad = camera_array([cam, cam])
    bad[1].n_inv = 99
    se2 = np.array([_se2(0.03, 0.5, -0.2), _se2(-0.02, 0.1, 0.3)])
    cfb = np.array([_p12(np.eye(3), np.zeros(3))] * 2)
    start = _p12(np.eye(3), np.array([0.5, 0.0, 0.0]))
    vel = np.array([0.1, 0.2, 0.3, 0.01, 0.02, 0.03])
    ok = motion_params(vel, 0.04, [1, 1], ncam=2)

    def prior(ncam=2, se2_=se2.ctypes.data, cams=ctypes.cast(cs, ctypes.c_void_p), cfb_=cfb.ctypes.data, start_=start.ctypes.data, mp=ok, out=True):
        o = TrackMotion()
        ctypes.memset(ctypes.byref(o), 0x5A, ctypes.sizeof(o))
        before = bytes(o)
        rc = L.mcp_track_motion_prior_host(ncam, se2_, cams, cfb_, start_, ctypes.byref(mp) if mp is not None else None, ctypes.byref(o) if out else None)
        return rc, bytes(o) == before

    def update(a=start.ctypes.data, b=start.ctypes.data, mp=ok, out=True):
        o = TrackMotion()
        ctypes.memset(ctypes.byref(o), 0x5A, ctypes.sizeof(o))
        before = bytes(o)
        rc = L.mcp_track_motion_update_host(a, b, ctypes.byref(mp) if mp is not None else None, ctypes.byref(o) if out else None)
        return rc, bytes(o) == before
    assert prior()[0] == 0 and update()[0] == 0
    nan_v, inf_v = vel.copy(), vel.copy()
    nan_v[4], inf_v[0] = np.nan, np.inf
    refusals = [("NULL params", prior(mp=None)), ("NULL out", prior(out=False)), ("NULL cams", prior(cams=None)), ("bad camera", prior(cams=ctypes.cast(bad, ctypes.c_void_p))),
                ("ncam 0", prior(ncam=0)), ("ncam 9", prior(ncam=9)), ("NULL se2", prior(se2_=None)), ("NULL cfb", prior(cfb_=None)), ("NULL start", prior(start_=None)),
                ("blur 0", prior(mp=motion_params(vel, 0.04, [1, 1], blur=0.0))), ("blur < 0", prior(mp=motion_params(vel, 0.04, [1, 1], blur=-1.0))),
                ("iterations < 0", prior(mp=motion_params(vel, 0.04, [1, 1], sbi_iterations=-1))),
                ("dt 0", prior(mp=motion_params(vel, 0.0, [1, 1]))), ("dt < 0", prior(mp=motion_params(vel, -0.04, [1, 1]))),
                ("dt nan", prior(mp=motion_params(vel, float("nan"), [1, 1]))), ("dt inf", prior(mp=motion_params(vel, float("inf"), [1, 1]))),
                ("velocity nan", prior(mp=motion_params(nan_v, 0.04, [1, 1]))), ("velocity inf", prior(mp=motion_params(inf_v, 0.04, [1, 1]))),
                ("update NULL params", update(mp=None)), ("update NULL out", update(out=False)), ("update NULL start", update(a=None)), ("update NULL refined", update(b=None)),
                ("update dt 0", update(mp=motion_params(vel, 0.0, [1, 1]))), ("update dt nan", update(mp=motion_params(vel, float("nan"), [1, 1]))),
                ("update velocity nan", update(mp=motion_params(nan_v, 0.04, [1, 1])))]
    for what, (rc, untouched) in refusals:
        assert rc == -1 and untouched, what
    # every refusal leaves a message that names what was wrong
    for call, word in ((lambda: prior(mp=None), "NULL motion"), (lambda: prior(cams=None), "NULL SBI cameras"), (lambda: prior(mp=motion_params(vel, 0.0, [1, 1])), "dt"),
                       (lambda: prior(mp=motion_params(vel, 0.04, [1, 1], blur=0.0)), "blur"), (lambda: update(mp=motion_params(nan_v, 0.04, [1, 1])), "velocity")):
        call()
        assert word in chain_bundle.last_error(), (word, chain_bundle.last_error())
    # dt is not looked at when the motion model is not applied (the frame after a recovery)
    assert prior(mp=motion_params(vel, 0.0, [1, 1], apply=False))[0] == 0 and update(mp=motion_params(vel, 0.0, [1, 1], apply=False))[0] == 0
    # the frame call refuses a NULL table before it looks at anything else
    assert L.mcp_track_frame_motion(None, 1, None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert "NULL table" in chain_bundle.last_error()
    assert L.mcp_track_motion_reset(None) == -1 and L.mcp_track_motion_get_sbi(None, 0, 0, None, None, None) == -1
