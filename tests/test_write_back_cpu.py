"""CPU-side checks of the AdjustAndUpdate write-back (include/mcp_img.h: mcp_map_points_set_rays / _update_rays / _get, mcp_scene_depth_robust,
mcp_ba_write_back): the boundary exists and refuses NULL handles without touching a device, and the numpy restatement of
KeyFrame::RefreshSceneDepthRobust (mcptam_amd.pvs.scene_depth_robust) gives what a hand computation gives."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcp_map_points_set_rays", "mcp_map_points_update_rays", "mcp_map_points_get", "mcp_scene_depth_robust", "mcp_ba_write_back",
           "mcp_map_points_last_timing"]


def test_write_back_entry_points_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "mcp_img.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"typedef struct mcp_scene_depth\s*\{", txt)
    for n in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe, pvs
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    for n in SYMBOLS:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
    assert sorted(pvs.WRITE_BACK_SYMBOLS) == sorted(SYMBOLS)


def test_scene_depth_layout_matches_the_header(tmp_path):
    from mcptam_amd.pvs import SCENE_DEPTH_DTYPE, SceneDepth
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    names = ("mean", "sigma", "median", "sigma_sq", "n", "refreshed")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) { printf("%d", (int)sizeof(mcp_scene_depth));\n'
                   + "".join('printf(" %%d", (int)offsetof(mcp_scene_depth, %s));\n' % f for f in names) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(SceneDepth)] + [getattr(SceneDepth, f).offset for f in names]
    assert got[0] == SCENE_DEPTH_DTYPE.itemsize and [SCENE_DEPTH_DTYPE.fields[f][1] for f in names] == got[1:]


def test_write_back_refuses_null_handles():
    """NULL handles are errors with a message, not crashes; no device is touched before the check."""
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import _bind_write_back, lib
    L = _bind_write_back(lib())
    x = np.zeros(9)
    assert L.mcp_map_points_set_rays(None, 0, 1, x.ctypes.data, x.ctypes.data, x.ctypes.data) == -1
    assert "NULL table" in chain_bundle.last_error()
    ids = np.zeros(1, dtype=np.int32)
    assert L.mcp_map_points_update_rays(None, 1, ids.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data) == -1
    assert "mcp_map_points_update_rays: NULL table" in chain_bundle.last_error()
    assert L.mcp_map_points_get(None, 0, 0, None, None, None, None) == -1
    assert "mcp_map_points_get: NULL table" in chain_bundle.last_error()
    assert L.mcp_scene_depth_robust(None, 0, None, None, None, None, None, None) == -1
    assert "mcp_scene_depth_robust: NULL table" in chain_bundle.last_error()
    assert L.mcp_map_points_last_timing(None, None, None, None) == -1
    assert "mcp_map_points_last_timing: NULL table" in chain_bundle.last_error()
    assert L.mcp_ba_write_back(None, None, 0, None, None, None, 1, None, None, None, None, 0, None, None, None, None, None, None, None, None) == -1
    assert "NULL solver handle" in chain_bundle.last_error()


def _by_hand(d, w):
    """RefreshSceneDepthRobust written out with Python floats on (depth, weight) tuples, sorted as std::pair sorts."""
    pairs = sorted(zip([float(v) for v in d], [float(v) for v in w]))
    n = len(pairs)
    med = pairs[n // 2][0]
    e2 = [(p[0] - med) * (p[0] - med) for p in pairs]
    m2 = sorted(e2)[n // 2]
    sg = 1.345 * (1.4826 * (1 + 5.0 / (n * 2 - 6)) * math.sqrt(m2))
    raw = sg * sg
    s2 = max(raw, 0.4)
    hw = [math.sqrt(1.0 if e < s2 else math.sqrt(s2 / e)) for e in e2]
    sd = sdd = sw = 0.0
    for p, h in zip(pairs, hw):
        c = p[1] * h
        sd += c * p[0]; sdd += c * p[0] * p[0]; sw += c
    mean = sd / sw
    return dict(median=med, raw=raw, sigma_sq=s2, mean=mean, sigma=math.sqrt(sdd / sw - mean * mean), hw=hw, order=pairs)


def test_scene_depth_robust_hand_computed_lists():
    from mcptam_amd.pvs import scene_depth_robust
    # n = 3 is left alone
    r = scene_depth_robust([1.0, 2.0, 3.0], [1.0, 1.0, 1.0])
    assert r == dict(n=3, refreshed=0)
    assert scene_depth_robust([], []) == dict(n=0, refreshed=0)
    # n = 4 (even): element [2] of the sorted list, not the mean of the middle two.  depths 1 2 4 8 -> median 4; distances^2 9 4 0 16 -> sorted
    # 0 4 9 16, element [2] = 9; sigma = 1.345 * 1.4826 * (1 + 5/2) * 3
    r = scene_depth_robust([8.0, 1.0, 4.0, 2.0], [1.0, 1.0, 1.0, 1.0])
    assert r["n"] == 4 and r["refreshed"] == 1 and r["median"] == 4.0
    sg = 1.345 * (1.4826 * (1 + 5.0 / 2) * 3.0)
    assert r["sigma_sq"] == sg * sg
    # every distance^2 is below sigma^2 (~438): all Huber weights 1, plain weighted mean
    assert r["mean"] == 15.0 / 4 and abs(r["sigma"] - math.sqrt(85.0 / 4 - (15.0 / 4) ** 2)) < 1e-15
    # odd n = 5: element [2]
    r = scene_depth_robust([5.0, 3.0, 9.0, 1.0, 7.0], [1.0] * 5)
    assert r["median"] == 5.0
    h = _by_hand([5.0, 3.0, 9.0, 1.0, 7.0], [1.0] * 5)
    assert (r["sigma_sq"], r["mean"], r["sigma"]) == (h["sigma_sq"], h["mean"], h["sigma"])
    # even n = 6: element [3] = 4.0 (the mean of the middle two would be 3.5)
    r = scene_depth_robust([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [1.0] * 6)
    assert r["median"] == 4.0
    # equal depths with different weights: the pair order puts the smaller weight first, which fixes the order of summation
    d, w = [2.0, 2.0, 2.0, 3.0, 1.0], [0.9, 0.1, 0.5, 1.0, 1.0]
    h = _by_hand(d, w)
    assert [p[1] for p in h["order"]] == [1.0, 0.1, 0.5, 0.9, 1.0]
    r = scene_depth_robust(d, w)
    assert (r["median"], r["sigma_sq"], r["mean"], r["sigma"]) == (2.0, h["sigma_sq"], h["mean"], h["sigma"])
    # a tight list: the raw sigma^2 falls below 0.4 and is clamped
    d = [5.0, 5.01, 5.02, 4.99, 4.98, 5.0, 5.03]
    h = _by_hand(d, [1.0] * 7)
    assert h["raw"] < 0.4
    r = scene_depth_robust(d, [1.0] * 7)
    assert r["sigma_sq"] == 0.4 and r["mean"] == h["mean"]
    # one gross outlier: its Huber weight is below 1 and pulls the mean less than a plain mean would
    d = [4.0, 4.1, 3.9, 4.05, 3.95, 4.0, 50.0]
    h = _by_hand(d, [1.0] * 7)
    assert h["sigma_sq"] == 0.4 and h["hw"][-1] < 1.0 and all(x == 1.0 for x in h["hw"][:-1])
    assert abs(h["hw"][-1] - (0.4 / 46.0 ** 2) ** 0.25) < 1e-15
    r = scene_depth_robust(d, [1.0] * 7)
    assert (r["mean"], r["sigma"]) == (h["mean"], h["sigma"]) and r["mean"] < sum(d) / 7
    # all weights 0: the mean is 0 / 0 -- where the reference stops the process
    r = scene_depth_robust([1.0, 2.0, 3.0, 4.0], [0.0] * 4)
    assert r["refreshed"] == -1 and math.isnan(r["mean"])


def test_huber_sigma_squared_equals_the_oracle():
    import oracle
    from mcptam_amd.pvs import huber_sigma_squared
    L = oracle.lib()
    rng = np.random.default_rng(3)
    for n in (4, 5, 6, 7, 50, 501, 2000):
        e = np.ascontiguousarray(rng.uniform(0, 3, n) ** 2)
        want = L.orc_huber_sigma_squared(e.copy().ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n)
        assert huber_sigma_squared(e) == want, n


def test_point_step_restatements_agree():
    """write_back_points (vectorised, the device's order of operations) against the composition of stereo.pixel_vectors point by point."""
    from mcptam_amd.pvs import chain_pose, write_back_point, write_back_points
    from mcptam_amd.synth import so3_exp
    rng = np.random.default_rng(11)
    n = 200
    poses = [chain_pose([(so3_exp(rng.normal(size=3) * 0.5), rng.normal(size=3)), (so3_exp(rng.normal(size=3) * 0.5), rng.normal(size=3) * 0.1)]) for _ in range(n)]
    R, t = np.array([p[0] for p in poses]), np.array([p[1] for p in poses])
    x = rng.normal(size=(n, 3)) + np.array([0, 0, 8.0])
    fixed = rng.random(n) < 0.2
    rays = [rng.normal(size=(n, 3)) * 0.1 + np.array([0, 0, 1.0]) for _ in range(3)]
    w, pr, pd = write_back_points(x, R, t, fixed, *rays)
    for k in range(n):
        w1, pr1, pd1 = write_back_point(x[k], poses[k], fixed[k], rays[0][k], rays[1][k], rays[2][k])
        assert np.abs(w[k] - w1).max() <= 1e-14 * np.abs(w1).max()
        assert np.abs(pr[k] - pr1).max() <= 1e-12 * np.abs(pr1).max() and np.abs(pd[k] - pd1).max() <= 1e-12 * np.abs(pd1).max()
    assert np.array_equal(w[fixed], x[fixed])
    Rc, tc = chain_pose([(R[0], t[0]), (R[1], t[1])])
    assert np.allclose(Rc, R[1] @ R[0], atol=1e-15) and np.allclose(tc, R[1] @ t[0] + t[1], atol=1e-14)


def test_cpp_write_back_compiles_and_links(tmp_path):
    """include/mcptam_hip/KeyFrame.hpp: MapPointTable's rays / Get / SceneDepthRobust / WriteBack instantiated and linked (not run: no GPU)."""
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "wb_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/ChainBundle.hpp"\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'static int use(int argc) {\n'
                   '  mcptam_hip::MapPointTable t(-1);\n'
                   '  std::vector<double> a(3*argc), b(3*argc), c(3*argc); std::vector<int> ids(argc), rows(argc);\n'
                   '  t.SetRays(0, a, b, c); t.UpdateRays(ids, a, b, c);\n'
                   '  std::vector<uint8_t> us; t.Get(0, argc, a, b, c, us);\n'
                   '  mcp_camera cam; std::memset(&cam, 0, sizeof cam); std::vector<mcp_camera> cams(1, cam);\n'
                   '  mcptam_hip::ChainBundle bundle(cams, true, true, false);\n'
                   '  mcptam_hip::WriteBackLists lists; lists.seg_start.push_back(0);\n'
                   '  mcptam_hip::WriteBackResult res = t.WriteBack(bundle, ids, rows, lists);\n'
                   '  std::vector<double> cfw; std::vector<double> depths;\n'
                   '  std::vector<mcp_scene_depth> sd = t.SceneDepthRobust(cfw, lists.seg_start, lists.seg_rows, lists.seg_weights, &depths);\n'
                   '  return (int)res.world_pos.size() + (int)sd.size();\n}\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) { std::printf("linked\\n"); return 0; }\n'
                   '  return use(argc);\n}\n')
    exe = tmp_path / "wb_link"
    lib = os.path.join(ROOT, "mcptam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lmcptam_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linked" in out.stdout
