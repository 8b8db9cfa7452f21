"""mcp_stereo_map_points without a device: the new symbols are declared, exported and bound and refuse NULL handles with a prefixed message; the two
new structs have the header's layout; mcp_stereo_append_host and mcp_stereo_busy_host (the bodies the kernels call, under the host compiler) equal
the numpy restatements mcptam_amd.stereo.stereo_append_ref / stereo_busy_ref byte for byte on the seeded inputs of tests/stereo_map_cases.py; and
the host unit under the sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stereo_map_cases as smc
from mcptam_amd import map_graph as mg
from mcptam_amd import stereo as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcp_stereo_map_points", "mcp_stereo_busy_host", "mcp_stereo_append_host", "mcp_map_points_get_rays", "mcp_map_points_get_source", "mcp_map_gp_get"]
APPEND_CASES = smc.append_cases()
BUSY_CASES = smc.busy_cases()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe, pvs
    h = _header()
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    B = S.lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, h), n + " is not declared in include/mcp_img.h"
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS and n in S.STEREO_SYMBOLS
        assert getattr(B, n).argtypes is not None, n
    for s in ("mcp_stereo_map_params", "mcp_stereo_map_result"):
        assert re.search(r"typedef struct %s\s*\{" % s, h), s
    for fn in ("stereo_map_points", "stereo_busy_ref", "stereo_busy_host", "stereo_append_ref", "stereo_append_host"):
        assert callable(getattr(S, fn))
    assert callable(mg.MapGraph.add_stereo_points) and callable(mg.MapGraph.get_points)
    assert callable(pvs.MapPointTable.get_rays) and callable(pvs.MapPointTable.get_source)


def test_null_handles_are_refused_with_a_message():
    from mcptam_amd import chain_bundle
    L = S.lib()
    prm, res = S.StereoMapParams(0, 0, 1, 1), S.StereoMapResult()
    calls = [("mcp_stereo_map_points", lambda: L.mcp_stereo_map_points(None, None, None, None, 0, 0, None, 0, None, 0, None, None, None, 0, None, None, ctypes.addressof(prm),
                                                                        ctypes.addressof(res), None, None, None), "NULL graph"),
             ("mcp_map_points_get_rays", lambda: L.mcp_map_points_get_rays(None, 0, 0, None, None), "NULL table"),
             ("mcp_map_points_get_source", lambda: L.mcp_map_points_get_source(None, 0, 0, None, None, None, None, None), "NULL table"),
             ("mcp_map_gp_get", lambda: L.mcp_map_gp_get(None, 0, 0, None, None, None), "NULL graph"),
             ("mcp_stereo_busy_host", lambda: L.mcp_stereo_busy_host(3, None, 0, 0, 0, None), "bad arguments"),
             ("mcp_stereo_append_host", lambda: L.mcp_stereo_append_host(2, None, None, 0, 0, 0, None, None, 0, None, None, None, None, None, None, None, None, None), "NULL array")]
    for name, call, needle in calls:
        assert call() == -1, name
        err = chain_bundle.last_error()
        assert err.startswith(name + ":") and needle in err, err


def test_struct_layouts_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    fields = {"mcp_stereo_map_params": (S.StereoMapParams, [f[0] for f in S.StereoMapParams._fields_]),
              "mcp_stereo_map_result": (S.StereoMapResult, [f[0] for f in S.StereoMapResult._fields_])}
    body = []
    for s, (_, fs) in fields.items():
        body.append('printf("%%d\\n", (int)sizeof(%s));' % s)
        body += ['printf("%%d\\n", (int)offsetof(%s, %s));' % (s, f) for f in fs]
    body += ['printf("%d\\n", MCP_SRC_ROOT);', 'printf("%d\\n", MCP_SRC_EPIPOLAR);']
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")      # (the header as C)
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for s, (cls, fs) in fields.items():
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f).offset for f in fs]
    assert got == want + [S.SRC_ROOT, S.SRC_EPIPOLAR]
    assert S.SRC_ROOT == mg.SRC_ROOT


@pytest.mark.parametrize("c", APPEND_CASES, ids=[c["name"] for c in APPEND_CASES])
def test_append_host_equals_numpy(c):
    args = (c["pts"], c["rows"], c["level"], c["src_mkf"], c["src_cam"], c["target_mkf"], c["target_cam"], c["first_store"])
    got, want = S.stereo_append_host(*args), S.stereo_append_ref(*args)
    made = len(c["pts"])
    for k, v in got.items():
        if k == "store_end":
            assert v == want[k] == c["first_store"] + 2 * made
        else:
            assert v.dtype == want[k].dtype and v.shape == want[k].shape and v.tobytes() == want[k].tobytes(), k      # (bit for bit: -0.0 and the subnormal included)
    ap = got["appended"]
    assert len(ap) == 2 * made and np.array_equal(got["center_xy"], c["cxy"])      # the centre is the level position the record's root came from
    assert (ap["source"][0::2] == S.SRC_ROOT).all() and (ap["source"][1::2] == S.SRC_EPIPOLAR).all() and (ap["alive"] == 1).all() and (ap["level"] == c["level"]).all()
    assert np.array_equal(ap["row"][0::2], c["rows"][:made]) and np.array_equal(ap["row"][1::2], c["rows"][:made])
    assert (ap["mkf"][0::2] == c["src_mkf"]).all() and (ap["cam"][0::2] == c["src_cam"]).all()
    assert np.array_equal(ap["mkf"][1::2], c["target_mkf"][c["pts"]["target"]]) and np.array_equal(ap["cam"][1::2], c["target_cam"][c["pts"]["target"]])
    assert ap["uv"][0::2].tobytes() == c["pts"]["root_pos"].tobytes() and ap["uv"][1::2].tobytes() == c["pts"]["target_pos"].tobytes()
    assert (want["usable"] == 0).all() and (want["inlier"] == 1).all() and (want["outlier"] == 0).all() and (want["fixed"] == 0).all()


@pytest.mark.parametrize("c", BUSY_CASES, ids=[c["name"] for c in BUSY_CASES])
def test_busy_host_equals_numpy(c):
    s = c["store"]
    got, want = S.stereo_busy_host(s, c["src_mkf"], c["src_cam"]), S.stereo_busy_ref(s, c["src_mkf"], c["src_cam"])
    assert got.tobytes() == want.tobytes() and len(got) == len(want)
    hit = (s["alive"] != 0) & (s["mkf"] == c["src_mkf"]) & (s["cam"] == c["src_cam"])
    assert len(got) == hit.sum()
    assert np.array_equal(got["root_pos"], s["uv"][hit])                          # store order (the positions are distinct and ascending)
    assert (np.diff(got["root_pos"][:, 0]) > 0).all()


def test_what_the_seeded_stores_were_made_for():
    """Dead entries among the matching ones, the same MKF under another camera and the reverse, and every level L-1 .. L+2 among the gathered: the
    gather keeps every level, the thinning filters."""
    for c in BUSY_CASES:
        s, m, cam, L = c["store"], c["src_mkf"], c["src_cam"], c["level"]
        if len(s) < 255 or c["name"].endswith("_all"):
            continue
        own = (s["mkf"] == m) & (s["cam"] == cam)
        assert (own & (s["alive"] == 0)).any() and (own & (s["alive"] != 0)).any()
        assert ((s["mkf"] == m) & (s["cam"] != cam) & (s["alive"] != 0)).any() and ((s["mkf"] != m) & (s["cam"] == cam) & (s["alive"] != 0)).any()
        got = S.stereo_busy_ref(s, m, cam)
        assert set(got["level"].tolist()) == set(range(max(L - 1, 0), min(L + 2, 3) + 1))
    full = [c for c in BUSY_CASES if c["name"].endswith("_all")][0]
    assert len(S.stereo_busy_host(full["store"], 3, 0)) == 256
    assert {c["store"].shape[0] for c in BUSY_CASES} == set(smc.BUSY_SIZES)


def test_host_unit_under_the_sanitizers(tmp_path):
    """tests/cpp/stereo_append_host_check.cpp has its own main: it calls the two host entry points on the shapes above against the rules written
    out there.  Built from the host unit alone with AddressSanitizer and UndefinedBehaviorSanitizer (nothing sanitized is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "stereo_append_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it needs nothing preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "stereo_append_host_check.cpp"), os.path.join(ROOT, "mcptam_amd", "csrc", "stereo_append_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stereo append host ok" in out.stdout
