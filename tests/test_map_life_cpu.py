"""The map's beginning, rescale and re-alignment without a device: the new symbols are declared, exported and bound and refuse bad arguments with a
prefixed message; the new structs have the header's layout; the host twins mcp_init_depth_points_host, mcp_map_mark_optimized_host and
mcp_map_transform_host (the bodies the kernels call, under the host compiler) equal the numpy restatements mcptam_amd.map_graph.init_depth_ref /
mark_optimized_ref / map_transform_ref on the shapes of tests/map_life_cases.py -- everything integer byte for byte, the doubles to 1e-12
norm-relative per vector, the tolerance tests/test_write_back_gpu.py and tests/test_stereo_points_gpu.py use for stereo_unproject and
stereo_pixel_vectors against numpy; and the host unit under the sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import map_life_cases as mlc
from mcptam_amd import map_graph as mg
from mcptam_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcp_init_depth_map_points", "mcp_map_mark_optimized", "mcp_map_rescale", "mcp_map_transform", "mcp_init_depth_points_host", "mcp_map_mark_optimized_host",
       "mcp_map_transform_host", "mcp_map_life_last_timing"]
INIT_CASES = mlc.init_cases()
XFORM_CASES = mlc.transform_cases()
INT_KEYS = ("center_xy", "gp_src_mkf", "gp_src_cam", "gp_flags")
VEC_KEYS = ("world_pos", "pixel_right_w", "pixel_down_w")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe
    h = _header()
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    B = mg._life_lib()
    assert sorted(NEW) == sorted(mg.LIFE_SYMBOLS)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, h), n + " is not declared in include/mcp_img.h"
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
        assert getattr(B, n).argtypes is not None, n
    for s in ("mcp_init_depth_cam", "mcp_init_depth_params", "mcp_init_depth_result", "mcp_map_transform_result"):
        assert re.search(r"typedef struct %s\s*\{" % s, h), s
    for fn in ("init_depth_ref", "init_depth_host", "mark_optimized_ref", "mark_optimized_host", "map_transform_ref", "map_transform_host"):
        assert callable(getattr(mg, fn))
    for fn in ("add_init_depth_points", "mark_optimized", "rescale", "transform", "life_last_timing"):
        assert callable(getattr(mg.MapGraph, fn))


def test_bad_arguments_are_refused_with_a_message():
    from mcptam_amd import chain_bundle
    L = mg._life_lib()
    prm, res, tr = mg.InitDepthParams(0, 0, 1.0), mg.InitDepthResult(), mg.MapTransformResult()
    eye = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    skew = eye.copy(); skew[1] = 1e-6                       # R R^T - I = 1e-6 off the diagonal
    nan = eye.copy(); nan[10] = np.nan
    cfb = mlc.rig()
    one = np.ones(1, dtype=np.int32)
    calls = [("mcp_init_depth_map_points", lambda: L.mcp_init_depth_map_points(None, 0, None, 0, None, None, ctypes.addressof(prm), ctypes.addressof(res), None, None), "NULL graph"),
             ("mcp_map_mark_optimized", lambda: L.mcp_map_mark_optimized(None, None), "NULL graph"),
             ("mcp_map_rescale", lambda: L.mcp_map_rescale(None, 1.0, ctypes.addressof(tr), None), "NULL graph"),
             ("mcp_map_transform", lambda: L.mcp_map_transform(None, eye.ctypes.data, ctypes.addressof(tr)), "NULL graph"),
             ("mcp_init_depth_points_host", lambda: L.mcp_init_depth_points_host(0, None, None, None, None, None, None, None, None, 0, None, None, 0, None, None, None, None, None, None,
                                                                                 None, None, None, None, None, None), "bad arguments"),
             ("mcp_map_life_last_timing", lambda: L.mcp_map_life_last_timing(None, None, None), "bad arguments"),
             ("mcp_map_mark_optimized_host", lambda: L.mcp_map_mark_optimized_host(3, 0, None, None), "bad arguments"),
             ("mcp_map_transform_host", lambda: L.mcp_map_transform_host(0, 1.0, None, 2, cfb.ctypes.data, 0, None, None, 0, 0, None, None, None, None, None, None, None, None),
              "bad arguments")]
    for kind, scale, T, needle in ((0, 0.0, None, "scale"), (0, -2.0, None, "scale"), (0, np.inf, None, "scale"), (0, np.nan, None, "scale"), (1, 1.0, None, "NULL"),
                                   (1, 1.0, nan, "non-finite"), (1, 1.0, skew, "orthonormal"), (2, 1.0, eye, "kind")):
        calls.append(("mcp_map_transform_host", lambda kind=kind, scale=scale, T=T: L.mcp_map_transform_host(
            kind, scale, None if T is None else T.ctypes.data, 2, cfb.ctypes.data, 0, None, None, 0, 0, None, None, None, None, None, None, None, ctypes.addressof(tr)), needle))
    cams = mlc.cameras()
    from mcptam_amd.taylor_camera import camera_array
    arr = camera_array(cams)
    z2 = np.zeros(2, dtype=np.int32)
    for level, depth, needle in ((4, 1.0, "level"), (-1, 1.0, "level"), (1, 0.0, "init_depth"), (1, -1.0, "init_depth"), (1, np.nan, "init_depth"), (1, np.inf, "init_depth")):
        p = mg.InitDepthParams(0, level, depth)
        calls.append(("mcp_init_depth_points_host", lambda p=p: L.mcp_init_depth_points_host(2, cfb.ctypes.data, eye.ctypes.data, ctypes.addressof(arr), z2.ctypes.data, None, z2.ctypes.data,
                                                                                             z2.ctypes.data, None, 0, None, ctypes.addressof(p), 0, ctypes.addressof(res), None, None, None, None,
                                                                                             None, None, None, None, None, None, None), needle))
    neg = np.array([0, -1], dtype=np.int32)
    calls.append(("mcp_init_depth_points_host", lambda: L.mcp_init_depth_points_host(2, cfb.ctypes.data, eye.ctypes.data, ctypes.addressof(arr), neg.ctypes.data, None, z2.ctypes.data, z2.ctypes.data,
                                                                                     None, 0, None, ctypes.addressof(prm), 0, ctypes.addressof(res), None, None, None, None, None, None, None, None,
                                                                                     None, None, None), "negative"))
    del one
    for name, call, needle in calls:
        assert call() == -1, (name, needle)
        err = chain_bundle.last_error()
        assert err.startswith(name + ":") and needle in err, err


def test_struct_layouts_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = {"mcp_init_depth_cam": mg.InitDepthCam, "mcp_init_depth_params": mg.InitDepthParams, "mcp_init_depth_result": mg.InitDepthResult,
              "mcp_map_transform_result": mg.MapTransformResult}
    body = []
    for s, cls in fields.items():
        body.append('printf("%%d\\n", (int)sizeof(%s));' % s)
        body += ['printf("%%d\\n", (int)offsetof(%s, %s));' % (s, f[0]) for f in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")      # (the header as C)
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for s, cls in fields.items():
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f[0]).offset for f in cls._fields_]
    assert got == want


def _init_args(c):
    return (mlc.rig(), mlc.mkf_poses()[c["src_mkf"]], mlc.cameras(), c["cands"], c["limits"], c["busy"], c["rows"], c["src_mkf"], c["level"], c["init_depth"], c["first_store"])


@pytest.mark.parametrize("c", INIT_CASES, ids=[c["name"] for c in INIT_CASES])
def test_init_depth_host_equals_numpy(c):
    got, want = mg.init_depth_host(*_init_args(c)), mg.init_depth_ref(*_init_args(c))
    n = want["made_total"]
    # structure: byte for byte
    assert got["made_total"] == n == sum(want["made"]) and got["first_store"] == c["first_store"] and got["store_end"] == want["store_end"] == c["first_store"] + n
    for k in ("made", "n_alive", "n_busy"):
        assert list(got[k]) == list(want[k]), k
    for a, b in zip(got["keep"], want["keep"]):
        assert a.tobytes() == b.tobytes()
    for k in INT_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["appended"].tobytes() == want["appended"].tobytes()                  # uv included: LevelZeroPos is exact
    gp, wp = got["points"], want["points"]
    for k in ("candidate", "target", "hypothesis", "score", "root_pos", "target_pos"):
        assert gp[k].tobytes() == wp[k].tobytes(), k
    # doubles: norm-relative per vector
    for k in VEC_KEYS:
        assert mlc.rel_close(got[k], want[k]), k
        assert got[k].tobytes() == gp[k].tobytes()                                  # the row's columns are the record's
    for k in ("center_nc", "one_right_nc", "one_down_nc"):
        assert mlc.rel_close(gp[k], wp[k]), k
    assert mlc.rel_close(got["rays"].reshape(-1, 3), want["rays"].reshape(-1, 3))
    # what the case is for
    made = want["made"]
    assert made == [min(int(k.sum()), l) for k, l in zip(want["keep"], c["limits"])]
    ap = got["appended"]
    assert (ap["source"] == mg.SRC_ROOT).all() and (ap["alive"] == 1).all() and (ap["level"] == c["level"]).all() and (ap["mkf"] == c["src_mkf"]).all()
    assert np.array_equal(ap["row"], c["rows"][:n]) and np.array_equal(ap["cam"], np.repeat([0, 1], made))      # camera 1's rows start right behind camera 0's made
    if n:
        assert np.allclose(np.linalg.norm(got["rays"].reshape(-1, 3), axis=1), 1.0, atol=1e-15)
        cfb, bfw = mlc.rig(), mlc.mkf_poses()[c["src_mkf"]]
        for cam in (0, 1):                                                          # the point sits at init_depth along the ray, in the camera's frame
            sel = ap["cam"] == cam
            Rw, tw = mg._compose(cfb[cam, :9].reshape(3, 3), cfb[cam, 9:], bfw[:9].reshape(3, 3), bfw[9:])
            pc = got["world_pos"][sel] @ Rw.T + tw
            assert np.allclose(np.linalg.norm(pc, axis=1), c["init_depth"], rtol=1e-12)
    if "expect_keep" in c:
        for a, b in zip(got["keep"], c["expect_keep"]):
            assert np.array_equal(a, b)
    if c["name"].startswith("n600"):
        assert made[0] == c["limits"][0] and want["n_alive"][0] == 600 and made[1] == 5
        assert np.array_equal(gp["candidate"][:made[0]], np.arange(made[0])) and np.array_equal(gp["candidate"][made[0]:], np.arange(5))
    if c["name"] == "level3_no_level4":
        assert not want["keep"][0][0] and want["keep"][0][1:].all()                 # the level-2 and level-0 positions on top of candidates 1 and 2 do not thin at level 3
    if c["name"] == "limit_zero":
        assert made == [0, 3] and want["keep"][0].all()
    if c["name"] == "zero_and_one_candidate":
        assert made == [0, 1]


def test_mark_optimized_host_equals_numpy():
    rng = np.random.default_rng(4)
    for n_rows, n_prows in ((0, 0), (1, 1), (255, 255), (256, 200), (257, 257), (300, 0)):
        usable = (rng.integers(0, 3, n_rows) == 0).astype(np.uint8)
        flags = rng.choice([0, mg.GP_FIXED, mg.GP_BAD, mg.GP_BAD | mg.GP_FIXED], n_prows).astype(np.int32)
        (gu, gn), (wu, wn) = mg.mark_optimized_host(usable, flags), mg.mark_optimized_ref(usable, flags)
        assert gu.tobytes() == wu.tobytes() and gn == wn == int(((flags & mg.GP_BAD) == 0).sum())
        assert (gu[n_prows:] == usable[n_prows:]).all() and (gu >= usable).all()   # rows the columns do not cover keep their byte; nothing is cleared


@pytest.mark.parametrize("c", XFORM_CASES, ids=[c["name"] for c in XFORM_CASES])
def test_transform_host_equals_numpy(c):
    a = c["a"]
    R, t = mlc.general_motion()
    for kw in (dict(scale=1.7), dict(scale=0.013), dict(new_from_old=(R, t))):
        (g, gc), (w, wc) = mg.map_transform_host(a, **kw), mg.map_transform_ref(a, **kw)
        assert gc == wc, kw                                                         # the counters are exact
        assert mlc.rel_close(g["base_from_world"][:, 9:], w["base_from_world"][:, 9:]) and mlc.rel_close(g["base_from_world"][:, :9].reshape(-1, 3), w["base_from_world"][:, :9].reshape(-1, 3))
        for k in VEC_KEYS:
            assert mlc.rel_close(g[k], w[k]), (k, kw)
        # the rows and slots that may not change keep every bit
        sm, sc, ok = mg._row_sources(a, len(a["world_pos"]))
        has = a["has_rays"].astype(bool)
        assert g["world_pos"][~ok].tobytes() == a["world_pos"][~ok].tobytes()
        for k in ("pixel_right_w", "pixel_down_w"):
            assert g[k][~(ok & has)].tobytes() == a[k][~(ok & has)].tobytes(), k
        absent = (a["mkf_flags"] & mg.MKF_PRESENT) == 0
        assert g["base_from_world"][absent].tobytes() == a["base_from_world"][absent].tobytes()
        if "scale" in kw:
            assert g["base_from_world"][:, :9].tobytes() == a["base_from_world"][:, :9].tobytes()     # a rescale leaves every rotation alone
            assert g["world_pos"][ok].tobytes() == (a["world_pos"][ok] * kw["scale"]).tobytes()
    if c["name"] == "mixed":
        assert wc == dict(n_rows=150, n_refreshed=145, n_no_rays=2, n_no_source=3, n_mkfs=4)


def test_transform_host_round_trips():
    """the properties the device tests rely on, on the host twin: after one general motion (every row refreshed) an identity motion and a scale of 1
    keep every bit, and a scale of 2 followed by one of 0.5 returns to the same bits"""
    a = mlc.map_arrays(150)
    R, t = mlc.general_motion()

    def apply(a, **kw):
        g, _ = mg.map_transform_host(a, **kw)
        b = dict(a)
        b.update(g)
        return b

    def same(x, y):
        return all(x[k].tobytes() == y[k].tobytes() for k in ("base_from_world",) + VEC_KEYS)
    b = apply(a, new_from_old=(R, t))
    assert not same(a, b)
    assert same(b, apply(b, new_from_old=(np.eye(3), np.zeros(3)))) and same(b, apply(b, scale=1.0))
    c = apply(b, scale=2.0)
    assert not same(b, c) and same(b, apply(c, scale=0.5))


def test_cpp_mirror_compiles_and_links(tmp_path):
    """include/mcptam_hip/MapGraph.hpp (AddInitDepthMapPoints, MarkOptimized, ApplyGlobalScaleToMap, ApplyGlobalTransformationToMap): every member
    is instantiated by tests/cpp/map_graph_mirror_link.cpp and must link against the C ABI; the program checks the mirror's own refusals"""
    import __graft_entry__ as g
    g.build()
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "map_graph_mirror_link")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "map_graph_mirror_link.cpp"),
                           "-L", os.path.join(ROOT, "mcptam_amd"), "-lmcptam_hip", "-Wl,-rpath," + os.path.join(ROOT, "mcptam_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe, "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "map graph mirror linked" in out.stdout


def test_host_unit_under_the_sanitizers(tmp_path):
    """tests/cpp/map_life_host_check.cpp has its own main with exactly sized arrays: it calls the three host entry points against rules written out
    there.  The host unit shares __host__ __device__ bodies with the kernels, so both are built as the host half of a HIP source, with
    AddressSanitizer and UndefinedBehaviorSanitizer on the host side; the program runs on its own (nothing sanitized is loaded into Python)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "map_life_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-x", "hip", "--cuda-host-only"] + san + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "map_life_host_check.cpp"), os.path.join(ROOT, "mcptam_amd", "csrc", "map_life_host.cpp"),
                           "-fsanitize=address,undefined", "-static-libsan", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "map life host ok" in out.stdout
