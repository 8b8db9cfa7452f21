"""CPU-side checks of the one-call recovery frame (include/mcp_img.h: mcp_track_frame_recover, mcp_track_recover_pose_host): the
declarations exist and are exported, the ctypes layouts are the host compiler's, the C++ mirror links, and the host entry -- the source
k_reloc_align / k_reloc_pick run, under the host compiler -- agrees with the numpy restatement of Relocaliser::AttemptRecovery's and
Tracker::AttemptRecovery's poses (src/Relocaliser.cc:76-85, src/Tracker.cc:538), SE3fromSE2 taken from the CPU oracle."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd.pvs import _bind_track_recover, lib
    return _bind_track_recover(lib())


def _sbi_cam(newton=False):
    from mcptam_amd.synth import DEFAULT_CAM_PARAMS
    from mcptam_amd.taylor_camera import TaylorCamera
    return TaylorCamera(DEFAULT_CAM_PARAMS, (640, 480), (640, 480), (40, 30), force_newton=newton)


def _se2(angle, tx, ty):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([c, -s, s, c, tx, ty])


def _p12(R, t):
    return np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3)])


def _poses():
    from mcptam_amd.pvs import so3_exp
    kf = (so3_exp(np.array([0.4, -0.7, 0.2])), np.array([0.8, -1.3, 2.1]))              # the candidate's CamFromWorld
    cfb = (so3_exp(np.array([0.05, 0.12, -0.3])), np.array([0.05, -0.02, 0.11]))        # CamFromBase: no identity, so the order of the product shows
    return kf, cfb


def test_recover_entry_points_declared_and_exported(built):
    from mcptam_amd import keyframe
    from mcptam_amd.pvs import TRACK_RECOVER_SYMBOLS
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)
    for s in ("mcp_track_recover_params", "mcp_track_recover"):
        assert re.search(r"typedef struct %s\s*\{" % s, txt), s
    assert sorted(TRACK_RECOVER_SYMBOLS) == ["mcp_track_frame_recover", "mcp_track_recover_pose_host"]
    L = ctypes.CDLL(os.path.join(ROOT, "mcptam_amd", "libmcptam_hip.so"))
    for n in TRACK_RECOVER_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS


def test_recover_struct_layouts_match_the_header(tmp_path):
    from mcptam_amd.pvs import TrackRecover, TrackRecoverParams
    fields = {"mcp_track_recover_params": (TrackRecoverParams, ["reloc_blur", "reloc_iterations", "max_score"]),
              "mcp_track_recover": (TrackRecover, ["recovered", "cam", "best", "best_zmssd", "se2", "align_score", "cam_pose", "base_from_world"])}
    body = []
    for s, (_, fs) in fields.items():
        body.append('printf("%%d\\n", (int)sizeof(%s));' % s)
        body += ['printf("%%d\\n", (int)offsetof(%s, %s));' % (s, f) for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for s, (cls, fs) in fields.items():
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f).offset for f in fs]
    assert got == want


def test_cpp_track_frame_recover_mirror_compiles_and_links(built, tmp_path):
    """include/mcptam_hip/KeyFrame.hpp's MapPointTable::TrackFrameRecover and RecoverPoseHost, linked against libmcptam_hip.so; the host entry
    runs (it needs no GPU), the frame call is only linked."""
    src = tmp_path / "track_recover_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'static int use(int argc) {\n'
                   '  mcptam_hip::MapPointTable t(-1);\n'
                   '  mcptam_hip::KeyFrame kf(640, 480), cand(640, 480); std::vector<mcptam_hip::KeyFrame*> ks{&kf}, cs{&cand, nullptr};\n'
                   '  std::vector<mcp_camera> cams(1), sbi(1); double bfw[12] = {0}; std::vector<double> cfb(12), cposes(24); std::vector<int> ccam{0, 0};\n'
                   '  mcp_track_map_params p; std::memset(&p, 0, sizeof p); mcp_track_record_params rp; std::memset(&rp, 0, sizeof rp);\n'
                   '  mcp_track_motion_params mp; std::memset(&mp, 0, sizeof mp); mp.blur = 0.75; mp.apply = argc - 1;\n'
                   '  mcp_track_recover_params rq; rq.reloc_blur = 2.5; rq.reloc_iterations = 6; rq.max_score = 1e5;\n'
                   '  mcp_track_map_result r; mcp_track_record rec; mcp_track_motion mo; mcp_track_recover rv; std::vector<double> scores;\n'
                   '  t.TrackFrameRecover(ks, {}, {}, false, cams, sbi, bfw, cfb, p, rp, mp, cs, ccam, cposes, rq, &r, &rec, &mo, &rv, &scores);\n'
                   '  return rv.cam + (int)scores.size();\n}\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) {\n'
                   '    const double se2[6] = {1, 0, 0, 1, 0, 0}, k[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, -0.25, 2}, c[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0, 0};\n'
                   '    mcp_camera cam; std::memset(&cam, 0, sizeof cam); double pose[12], b[12];\n'
                   '    mcptam_hip::MapPointTable::RecoverPoseHost(se2, cam, k, c, pose, b);\n'
                   '    std::printf("linked %g %g\\n", pose[9], b[9]); return 0;\n  }\n'
                   '  return use(argc);\n}\n')
    exe = tmp_path / "track_recover_link"
    lib = os.path.join(ROOT, "mcptam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lmcptam_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linked 0.5 0" in out.stdout      # an identity alignment: the candidate's pose; 0.5 - 0.5 in the base frame


# the alignments: the identity, small and large rotations, translations up to +-5 SBI pixels, and mixtures
ALIGNMENTS = [(0.0, 0.0, 0.0), (1e-6, 0.0, 0.0), (0.01, 0.0, 0.0), (-0.03, 0.2, -0.1), (0.3, 0.0, 0.0), (-0.8, 1.0, 2.0), (1.5, -3.0, 1.0),
              (0.0, 5.0, 0.0), (0.0, -5.0, 0.0), (0.0, 0.0, 5.0), (0.0, 0.0, -5.0), (0.05, 5.0, -5.0), (-0.2, -5.0, 5.0), (0.0, 1e-3, -1e-3)]


@pytest.mark.parametrize("newton", [False, True], ids=["inverse_polynomial", "newton_fallback"])
def test_pose_host_is_the_numpy_restatement(built, newton):
    """mcp_track_recover_pose_host against recover_restate (numpy, SE3fromSE2 from the CPU oracle): atol 1e-9 on cam_pose and
    base_from_world, the bound mcp_track_motion_prior_host has against the same kind of restatement.  The candidate's translation has norm
    2.6, so the bound is on numbers of order one."""
    from mcptam_amd.pvs import recover_pose_host, recover_restate
    from oracle import oracle_sbi_se3_from_se2
    cam = _sbi_cam(newton)
    kf, cfb = _poses()
    worst = 0.0
    for a, tx, ty in ALIGNMENTS:
        se2 = _se2(a, tx, ty)
        pose, bfw = recover_pose_host(se2, cam, _p12(*kf), _p12(*cfb))
        ref = recover_restate([None], [np.zeros(1)], [0], [kf], lambda c, k: (se2, 1.0), [cam], [cfb], se3_from_se2=oracle_sbi_se3_from_se2, scores=[3.0])
        assert ref["recovered"] and ref["cam"] == 0 and ref["best"] == [0]
        d = max(np.abs(pose - _p12(*ref["cam_pose"][0])).max(), np.abs(bfw - _p12(*ref["base_from_world"])).max())
        worst = max(worst, d)
        # a rotation about the camera centre: orthonormal, and the translation is the candidate's, rotated
        R = pose[:9].reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12
        assert abs(np.linalg.norm(pose[9:]) - np.linalg.norm(kf[1])) <= 1e-12
        if a != 0.0 or tx != 0.0 or ty != 0.0:
            assert pose.tobytes() != _p12(*kf).tobytes()
    print("%s: largest |host - restatement| over %d alignments %.3g" % ("newton" if newton else "polynomial", len(ALIGNMENTS), worst))
    assert worst <= 1e-9
    # a turn of 0.3 rad in the image is a roll of about that much: the rotation is no small-angle leftover
    pose, _ = recover_pose_host(_se2(0.3, 0.0, 0.0), cam, _p12(np.eye(3), np.zeros(3)), _p12(*cfb))
    assert 0.25 < np.arccos((np.trace(pose[:9].reshape(3, 3)) - 1) / 2) < 0.35


def test_identity_alignment_is_exactly_the_candidates_pose(built):
    """se2 exactly the identity: cam_pose is the candidate's pose bit for bit, base_from_world exactly CamFromBase^-1 composed with it
    (R^T R_k, R^T (t_k - t)) up to the rounding of that one product.  Every entry is a sum of three products of magnitude below 2.6 (the
    candidate's translation): three roundings of at most 2.6 * 2^-53 and two of the sums, under 1.5e-15 per implementation, 4e-15 between two."""
    from mcptam_amd.pvs import recover_pose_host
    kf, cfb = _poses()
    for cam in (_sbi_cam(), _sbi_cam(True)):
        pose, bfw = recover_pose_host(_se2(0.0, 0.0, 0.0), cam, _p12(*kf), _p12(*cfb))
        assert pose.tobytes() == _p12(*kf).tobytes()
        want = _p12(cfb[0].T @ kf[0], cfb[0].T @ (kf[1] - cfb[1]))
        assert np.abs(bfw - want).max() <= 4e-15
        # ... and it is the inverse that was applied, not CamFromBase itself
        assert np.abs(bfw - _p12(cfb[0] @ kf[0], cfb[0] @ kf[1] + cfb[1])).max() > 1e-2
    # an identity CamFromBase on top: everything comes back bit for bit
    pose, bfw = recover_pose_host(_se2(0.0, 0.0, 0.0), _sbi_cam(), _p12(*kf), _p12(np.eye(3), np.zeros(3)))
    assert bfw.tobytes() == _p12(*kf).tobytes()


def test_restatement_picks_the_first_smallest_and_the_first_camera_under_the_threshold():
    """recover_restate on hand-made scores: strict <, skipped entries, cameras in order."""
    from mcptam_amd.pvs import SCORE_SKIPPED, recover_restate, zmssd
    cam = _sbi_cam()
    kf, cfb = _poses()
    ident = (np.eye(3), np.zeros(3))
    templs = [np.zeros(4), None, np.zeros(4), np.zeros(4), np.zeros(4)]
    cams_ = [0, 0, 0, 1, 1]
    scores = [5.0, SCORE_SKIPPED, 5.0, 9.0, 2.0]
    al = {(0, 0): (_se2(0, 0, 0), 7.0), (1, 4): (_se2(0, 0, 0), 3.0)}
    r = recover_restate([None, None], templs, cams_, [kf] * 5, lambda c, k: al[(c, k)], [cam, cam], [ident, cfb], max_score=7.0, scores=scores)
    assert r["best"] == [0, 4] and r["cam"] == 1 and r["recovered"]                    # camera 0: 7 < 7 fails
    r = recover_restate([None, None], templs, cams_, [kf] * 5, lambda c, k: al[(c, k)], [cam, cam], [ident, cfb], max_score=7.5, scores=scores)
    assert r["cam"] == 0 and _p12(*r["base_from_world"]).tobytes() == _p12(*kf).tobytes()
    r = recover_restate([None, None], templs, cams_, [kf] * 5, lambda c, k: al[(c, k)], [cam, cam], [ident, cfb], max_score=0.0, scores=scores)
    assert not r["recovered"] and r["cam"] == -1 and r["base_from_world"] is None
    r = recover_restate([None, None], [None] * 5, cams_, [kf] * 5, None, [cam, cam], [ident, cfb], scores=[SCORE_SKIPPED] * 5)
    assert r["best"] == [-1, -1] and not r["recovered"]
    # the raster-order double sum of float differences
    a, b = np.array([1.5, 2.25, -3.0], dtype=np.float32), np.array([0.5, 0.25, 1.0], dtype=np.float32)
    assert zmssd(a, b) == 1.0 + 4.0 + 16.0


def test_host_entry_refuses_bad_arguments(built):
    from mcptam_amd import chain_bundle
    L = built
    cam = _sbi_cam().to_struct()
    bad = _sbi_cam().to_struct()
    bad.n_inv = 99
    kf, cfb = _poses()
    se2, k12, c12 = _se2(0.03, 0.5, -0.2), _p12(*kf), _p12(*cfb)
    nan_se2, inf_k, nan_c = se2.copy(), k12.copy(), c12.copy()
    nan_se2[4], inf_k[10], nan_c[0] = np.nan, np.inf, np.nan

    def call(se2_=se2, cam_=cam, k=k12, c=c12, want_pose=True, want_bfw=True):
        pose, bfw = np.full(12, 7.25), np.full(12, 7.25)
        rc = L.mcp_track_recover_pose_host(None if se2_ is None else se2_.ctypes.data, None if cam_ is None else ctypes.addressof(cam_), None if k is None else k.ctypes.data,
                                           None if c is None else c.ctypes.data, pose.ctypes.data if want_pose else None, bfw.ctypes.data if want_bfw else None)
        return rc, bool((pose == 7.25).all() and (bfw == 7.25).all())
    assert call() == (0, False)
    assert call(want_pose=False)[0] == 0 and call(want_bfw=False)[0] == 0 and call(c=None, want_bfw=False)[0] == 0
    for what, got, word in (("NULL se2", call(se2_=None), "NULL alignment"), ("NULL camera", call(cam_=None), "camera"), ("bad camera", call(cam_=bad), "camera"),
                            ("NULL candidate pose", call(k=None), "candidate pose"), ("NULL CamFromBase", call(c=None), "CamFromBase"),
                            ("se2 nan", call(se2_=nan_se2), "not finite"), ("pose inf", call(k=inf_k), "not finite"), ("CamFromBase nan", call(c=nan_c), "not finite")):
        assert got == (-1, True), what
    for kw, word in ((dict(se2_=None), "NULL alignment"), (dict(cam_=bad), "camera"), (dict(c=None), "CamFromBase"), (dict(k=inf_k), "not finite")):
        call(**kw)
        assert word in chain_bundle.last_error(), (word, chain_bundle.last_error())
    # the frame call refuses a NULL table before it looks at anything else
    assert L.mcp_track_frame_recover(None, 1, None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None, 0, None, None, None, None, None, None) == -1
    assert "NULL table" in chain_bundle.last_error()
