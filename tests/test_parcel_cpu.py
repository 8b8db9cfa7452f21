"""Measurement parcels without a device: the new symbols are exported, bound and declared and refuse NULL handles with a message;
mcp_parcel_commit_host (the bodies the kernels call, under the host compiler) equals the numpy restatement mcptam_amd.map_graph.parcel_commit_ref
exactly -- verdicts, counters, per-lane counts and the appended records byte for byte -- on the seeded maps of tests/parcel_cases.py; the struct
sizes are the header's; and the host unit under the sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import parcel_cases as pc
from mcptam_amd import map_graph as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = pc.all_cases()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)


def test_symbols_are_exported_bound_and_declared():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe
    declared = sorted(set(re.findall(r"\b(mcp_meas_parcel_[a-z0-9_]+|mcp_parcel_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(mg.PARCEL_SYMBOLS) and len(declared) == 9
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    B = mg.lib()
    for n in declared:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
        assert getattr(B, n).argtypes is not None, n
    for n in ("from_track", "from_refind", "from_host", "entries"):
        assert callable(getattr(mg.MeasParcel, n))
    assert callable(mg.MapGraph.commit_parcel)
    import mcptam_amd
    assert mcptam_amd.MeasParcel is mg.MeasParcel and mcptam_amd.parcel_commit_ref is mg.parcel_commit_ref and mcptam_amd.parcel_commit_host is mg.parcel_commit_host


def test_null_handles_are_refused_with_a_message():
    from mcptam_amd import chain_bundle
    L = mg.lib()
    prm, res = mg.ParcelCommitParams(1, 0), mg.ParcelCommitResult()
    one = np.zeros(1, dtype=np.int32)
    calls = [("mcp_meas_parcel_create", lambda: L.mcp_meas_parcel_create(None), None, "NULL table"),
             ("mcp_meas_parcel_from_track", lambda: L.mcp_meas_parcel_from_track(None), -1, "NULL parcel"),
             ("mcp_meas_parcel_from_refind", lambda: L.mcp_meas_parcel_from_refind(None), -1, "NULL parcel"),
             ("mcp_meas_parcel_from_host", lambda: L.mcp_meas_parcel_from_host(None, 0, None, None, None, None), -1, "NULL parcel"),
             ("mcp_meas_parcel_size", lambda: L.mcp_meas_parcel_size(None), -1, "NULL parcel"),
             ("mcp_meas_parcel_get", lambda: L.mcp_meas_parcel_get(None, 0, None), -1, "NULL parcel"),
             ("mcp_meas_parcel_commit", lambda: L.mcp_meas_parcel_commit(None, None, 1, one.ctypes.data, one.ctypes.data, ctypes.addressof(prm), ctypes.addressof(res), None), -1, "NULL graph"),
             ("mcp_parcel_commit_host", lambda: L.mcp_parcel_commit_host(0, None, 0, None, 0, None, None, None, 0, None, None, None, 0, None, None, ctypes.addressof(res), None), -1, "NULL params")]
    for name, call, want, needle in calls:
        assert call() == want, name
        err = chain_bundle.last_error()
        assert err.startswith(name + ":") and needle in err, err
    L.mcp_meas_parcel_destroy(None)                        # (a no-op)


def test_constants_and_struct_sizes_match_the_header(tmp_path):
    h = _header()
    for name, value in dict(MCP_PARCEL_APPENDED=mg.PARCEL_APPENDED, MCP_PARCEL_SKIPPED=mg.PARCEL_SKIPPED, MCP_PARCEL_STALE=mg.PARCEL_STALE, MCP_PARCEL_BAD=mg.PARCEL_BAD,
                            MCP_PARCEL_CROSS=mg.PARCEL_CROSS).items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value, name
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read include/mcp_img.h with"
    names = sorted(mg.PARCEL_STRUCT_SIZES)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                   '  printf("key %zu\\n", offsetof(mcp_parcel_entry, key));\n  printf("source %zu\\n", offsetof(mcp_store_entry, source));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for n in names:
        assert int(out[n]) == mg.PARCEL_STRUCT_SIZES[n], (n, out[n])
    assert int(out["key"]) == mg.PARCEL_ENTRY_DTYPE.fields["key"][1] and int(out["source"]) == mg.STORE_ENTRY_DTYPE.fields["source"][1]
    assert mg.PARCEL_ENTRY_DTYPE.itemsize == 32 and mg.STORE_ENTRY_DTYPE.itemsize == 40


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_numpy(c):
    got, want = pc.host(c, first=11), pc.ref(c, first=11)
    pc.same_commit(got, want)
    vd, res, recs, lanes = got
    assert len(vd) == c["n"] and res["first"] == 11
    assert res["n_appended"] + res["n_skipped_lane"] + res["n_stale"] + res["n_bad"] + res["n_cross"] == c["n"]
    assert len(recs) == res["n_appended"] == int(lanes.sum()) and (recs["alive"] == 1).all() and (recs["source"] == c["source"]).all()
    if c["cross_camera"]:
        assert res["n_cross"] == 0
    keep = np.flatnonzero(vd == mg.PARCEL_APPENDED)
    assert recs["uv"].tobytes() == c["entries"]["uv"][keep].tobytes()          # (bit for bit: -0.0 and the subnormals included)


def test_what_the_seeded_maps_were_made_for():
    """Over the three cases of every size from 63 up, every verdict occurs; the rule order is the stated one on entries that several rules fit."""
    by_size = {}
    for c in CASES:
        by_size.setdefault(c["n"], np.zeros(5, dtype=np.int64))
        by_size[c["n"]] += np.bincount(pc.ref(c)[0], minlength=5)
    assert sorted(by_size) == list(pc.SIZES)
    for n, seen in by_size.items():
        if n >= 63:
            assert (seen > 0).all(), (n, seen.tolist())
        assert seen.sum() == 3 * n
    # one row that is recycled, bad and of another camera; one lane withheld: the first rule that applies names the verdict
    keys, flags, sm, sc = np.array([7, 10], np.int32), np.array([mg.GP_BAD, 0], np.int32), np.array([0, 0], np.int32), np.array([1, 1], np.int32)
    e = mg.parcel_entries([0, 1, 1, 1, 1], [0, 0, 1, 1, 5], np.zeros((5, 2)), [0, 1, 2, 3, 0], [99, 99, 10, 11, 0])
    for fn in (mg.parcel_commit_ref, mg.parcel_commit_host):
        vd, res, recs, lanes = fn(e, keys, flags, sm, sc, [-1, 2], [0, 0], cross_camera=0, source=mg.SRC_REFIND, first=3)
        assert vd.tolist() == [mg.PARCEL_SKIPPED, mg.PARCEL_STALE, mg.PARCEL_CROSS, mg.PARCEL_STALE, mg.PARCEL_STALE]
        vd, res, recs, lanes = fn(e, keys, flags, sm, sc, [4, 2], [0, 1], cross_camera=0, source=mg.SRC_REFIND, first=3)
        assert vd.tolist() == [mg.PARCEL_STALE, mg.PARCEL_STALE, mg.PARCEL_APPENDED, mg.PARCEL_STALE, mg.PARCEL_STALE]
        assert res == dict(first=3, n_appended=1, n_skipped_lane=0, n_stale=4, n_bad=0, n_cross=0) and lanes.tolist() == [0, 1]
        assert recs[0]["mkf"] == 2 and recs[0]["cam"] == 1 and recs[0]["row"] == 1 and recs[0]["level"] == 2 and recs[0]["source"] == mg.SRC_REFIND and recs[0]["alive"] == 1
        e2 = e.copy(); e2["key"][0] = 7
        vd = fn(e2, keys, flags, sm, sc, [4, 2], [0, 1], cross_camera=0)[0]
        assert vd[0] == mg.PARCEL_BAD                      # bad comes before cross


def test_host_refusals():
    from mcptam_amd import chain_bundle
    c = CASES[6]
    assert c["n"] > 0
    e = c["entries"].copy(); e["lane"][0] = len(c["lane_mkf"])
    with pytest.raises(RuntimeError):
        mg.parcel_commit_host(e, c["keys_now"], c["pt_flags"], c["src_mkf"], c["src_cam"], c["lane_mkf"], c["lane_cam"])
    assert "names lane" in chain_bundle.last_error()
    e["lane"][0] = -1
    with pytest.raises(RuntimeError):
        mg.parcel_commit_host(e, c["keys_now"], c["pt_flags"], c["src_mkf"], c["src_cam"], c["lane_mkf"], c["lane_cam"])
    with pytest.raises(RuntimeError):                      # more graph columns than table rows
        mg.parcel_commit_host(c["entries"], c["keys_now"][:3], c["pt_flags"], c["src_mkf"], c["src_cam"], c["lane_mkf"], c["lane_cam"])
    assert "bad arguments" in chain_bundle.last_error()


def test_host_unit_under_the_sanitizers(tmp_path):
    """tests/cpp/parcel_commit_host_check.cpp has its own main: it calls mcp_parcel_commit_host on seam-sized parcels against the rules written
    out there.  Built from the host unit alone with AddressSanitizer and UndefinedBehaviorSanitizer (nothing sanitized is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "parcel_commit_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it needs nothing preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "parcel_commit_host_check.cpp"), os.path.join(ROOT, "mcptam_amd", "csrc", "map_graph_parcel_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "parcel commit host ok" in out.stdout
