"""CPU-side checks of the one-call AddStereoMapPoints (include/mcp_img.h: mcp_stereo_points, mcp_stereo_hypotheses): the declarations exist and
are exported, the ctypes layouts are the host compiler's, the C++ mirror links, and the numpy restatements the GPU tests compose with follow
src/MapMakerServerBase.cc (ThinCandidates :411-446, the arc :611-723, the selection :798-825, ReprojectPoint :123-143) and TaylorCamera.cc:194-196."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    return cc


def test_stereo_entry_points_declared_and_exported():
    from mcptam_amd.stereo import STEREO_SYMBOLS
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)
    for s in ("mcp_stereo_target", "mcp_stereo_meas", "mcp_stereo_point"):
        assert re.search(r"typedef struct %s\s*\{" % s, txt), s
    for n in STEREO_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
    for m in ("THINNED", "NO_ARC", "NO_MATCH", "TOO_MANY", "INDEX_FAR", "NO_SUBPIX", "CREATED", "PAST_LIMIT"):
        assert re.search(r"#define MCP_STEREO_%s \d" % m, txt), m
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    for n in STEREO_SYMBOLS:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n


def test_stereo_struct_layouts_match_the_header(tmp_path):
    from mcptam_amd import stereo as S
    fields = {"mcp_stereo_target": (S.StereoTarget, ["kf", "cam", "cam_from_world", "one_pixel_angle"]),
              "mcp_stereo_meas": (S.StereoMeas, ["root_pos", "level"]),
              "mcp_stereo_point": (S.StereoPoint, [f[0] for f in S.StereoPoint._fields_])}
    body = []
    for s, (_, fs) in fields.items():
        body.append('printf("%%d\\n", (int)sizeof(%s));' % s)
        body += ['printf("%%d\\n", (int)offsetof(%s, %s));' % (s, f) for f in fs]
    body += ['printf("%%d\\n", MCP_STEREO_%s);' % m for m in ("THINNED", "NO_ARC", "NO_MATCH", "TOO_MANY", "INDEX_FAR", "NO_SUBPIX", "CREATED", "PAST_LIMIT")]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_cc(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for s, (cls, fs) in fields.items():
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f).offset for f in fs]
    want += [S.THINNED, S.NO_ARC, S.NO_MATCH, S.TOO_MANY, S.INDEX_FAR, S.NO_SUBPIX, S.CREATED, S.PAST_LIMIT]
    assert got == want
    assert [S.STEREO_POINT_DTYPE.fields[f[0]][1] for f in S.StereoPoint._fields_] == [getattr(S.StereoPoint, f[0]).offset for f in S.StereoPoint._fields_]


def test_cpp_mirror_add_stereo_points_compiles_and_links(tmp_path):
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "stereo_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) {\n'
                   '    auto f = &mcptam_hip::KeyFrame::AddStereoPoints; (void)f; std::printf("linked\\n"); return 0; }\n'
                   '  try { mcptam_hip::KeyFrame src(640, 480); mcp_camera cam{}; double T[12] = {1,0,0, 0,1,0, 0,0,1, 0,0,0};\n'
                   '    auto r = src.AddStereoPoints(cam, T, 1, {}, {}, {}, 10); std::printf("%zu\\n", r.vPoints.size()); }\n'
                   '  catch (const std::exception& e) { std::printf("%s\\n", e.what()); }\n'
                   '  return 0; }\n')
    exe = str(tmp_path / "stereo_link")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", os.path.join(ROOT, "mcptam_amd"),
                           "-lmcptam_hip", "-Wl,-rpath," + os.path.join(ROOT, "mcptam_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe, "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "linked" in out.stdout, out.stdout + out.stderr


def test_selection_rules_every_branch():
    from mcptam_amd import stereo as S
    p = np.zeros(2)
    # best > 0: every later match counts, so four matches anywhere are too many and three must be within one index of the best
    assert S.select_matches([(900, 3, p), (500, 4, p), (800, 5, p), (2000, 40, p)])[0] == S.TOO_MANY
    code, kept = S.select_matches([(900, 3, p), (500, 4, p), (800, 5, p)])
    assert code == 0 and [m[1] for m in kept] == [4, 5, 3]
    assert S.select_matches([(900, 3, p), (500, 4, p), (9000, 40, p)])[0] == S.INDEX_FAR
    # best == 0: only positive scores count -- many zeros can survive, the first zeros by index are kept
    zeros = [(0, i, p) for i in range(10, 30)]
    code, kept = S.select_matches(zeros + [(70, 31, p)])
    assert code == 0 and [m[1] for m in kept] == [10, 11]
    assert S.select_matches(zeros + [(70, 31, p), (90, 32, p), (95, 9, p)])[0] == S.TOO_MANY
    # index distance 2 from the best is ambiguous
    assert S.select_matches([(0, 5, p), (0, 7, p)])[0] == 0            # best == 0 and no positive: only the best is kept
    assert S.select_matches([(10, 5, p), (11, 7, p)])[0] == S.INDEX_FAR
    # ties go by hypothesis index: the first index with the minimal score is the best
    code, kept = S.select_matches([(50, 7, p), (40, 8, p), (40, 9, p)])
    assert code == 0 and [m[1] for m in kept] == [8, 9, 7]
    assert S.select_matches([(40, 8, p), (40, 9, p), (40, 10, p)])[0] == S.INDEX_FAR      # 10 is two from the first best
    assert S.select_matches([])[0] == S.NO_MATCH


def test_thin_candidates_levels_boundary_rounding():
    from mcptam_amd import stereo as S
    cand = np.array([[50, 50], [60, 50], [59, 50], [50, 40], [0, 0]])
    L = 1
    root = S.level_zero_pos([50, 50], L)                  # a measurement on candidate 0 at level L
    for lv, thins in ((L - 1, False), (L, True), (L + 1, True), (L + 2, False)):
        keep = S.thin_candidates(cand, L, [root], [lv])
        assert keep[0] == (not thins) and keep[4]
        if thins:
            assert keep[1] and not keep[2] and keep[3]      # exactly 10 px away survives (mag_squared >= 100), 9 px does not
    # ir_rounded: half away from zero, negative values included
    assert list(S.ir_rounded([0.5, 1.5, -0.5, -1.5, 2.49, -2.51])) == [1, 2, -1, -2, 2, -3]
    keep = S.thin_candidates(np.array([[0, 0], [0, 10], [10, 0]]), 0, [[-0.5, -0.5]], [0])      # busy at (-1, -1)
    assert list(keep) == [False, True, True]
    # created points (SRC_ROOT at level L) round back to their own candidate
    for lvl in range(4):
        for c in ([7, 9], [0, 0], [100, 3]):
            assert list(S.ir_rounded(S.level_zero_pos(c, lvl) / (1 << lvl))) == c


def test_arc_on_the_ray_and_equal_angles():
    from mcptam_amd import stereo as S, synth_img
    from mcptam_amd.synth import so3_exp
    cam = synth_img.TaylorCamera(synth_img.DEFAULT_CAM_PARAMS[:4] + (320.0, 240.0) + synth_img.DEFAULT_CAM_PARAMS[6:], (640, 480), (640, 480), (640, 480))
    ps = (np.eye(3), np.zeros(3))
    R = so3_exp(np.array([0.01, 0.04, 0.0]))
    pt = (R, -R @ np.array([0.6, 0.02, 0.0]))
    opa = cam.one_pixel_angle()
    for level in range(4):
        for c in ([40, 30], [10, 100], [70, 5]):
            c = np.array(c) >> level if level else np.array(c)
            a = S.arc(cam, ps, pt, opa, level, c)
            assert a["n"] > 2
            ray = cam.unproject(S.level_zero_pos(c, level))[0]
            w = a["world"]
            d = np.linalg.norm(w, axis=1)
            assert np.abs(w / d[:, None] - ray).max() < 1e-9                    # on the source ray (source = world frame)
            assert (np.diff(d) > 0).all() and d[0] >= 0.2 - 1e-12
            u = a["tc"] / np.linalg.norm(a["tc"], axis=1)[:, None]              # equally spaced angles seen from the target
            ang = np.arccos(np.clip((u[1:] * u[:-1]).sum(axis=1), -1, 1))
            assert np.allclose(ang, a["step"], rtol=1e-6, atol=1e-9)
            assert a["step"] <= opa * (1 << level) * 3 + 1e-15


def test_one_pixel_angle_is_the_references():
    from mcptam_amd import synth_img
    cam = synth_img.TaylorCamera(synth_img.DEFAULT_CAM_PARAMS, (640, 480), (640, 480), (640, 480))
    c = cam.image_size / 2
    a = cam.unproject(c)[0]
    b = cam.unproject(c + np.array([1.0, 1.0]))[0]
    assert cam.one_pixel_angle() == math.acos(float(a @ b)) / math.sqrt(2.0)
    assert 0.003 < cam.one_pixel_angle() < 0.005                        # about 1 / a0 for a0 = 250
