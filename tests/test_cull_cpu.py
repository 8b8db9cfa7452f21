"""Outliers and bad points without a device (include/mcp_img.h mcp_map_cull_*): the new symbols are exported, bound and declared and refuse NULL
handles with a message; the constants and struct sizes are the header's; mcp_map_cull_outliers_host / mcp_map_cull_sweep_host (the bodies the
kernels call, under the host compiler) equal the numpy restatements mcptam_amd.map_graph.cull_outliers_ref / cull_sweep_ref byte for byte --
verdicts, counters, flags, pending marks, alive and usable columns, the reported rows -- on the seeded maps of tests/cull_cases.py; the
verdicts the issue spells out; every refusal leaves its outputs untouched; and the host unit under the sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cull_cases as cc
from mcptam_amd import map_graph as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cc.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
M_, FX, PB, RE, NR, AB = mg.CULL_MISSING, mg.CULL_FIXED, mg.CULL_POINT_BAD, mg.CULL_RETRY, mg.CULL_NEVER_RETRY, mg.CULL_ALREADY_BAD


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)


def test_symbols_are_exported_bound_and_declared():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe
    declared = sorted(set(re.findall(r"\b(mcp_map_cull_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(mg.CULL_SYMBOLS) and len(declared) == 6
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    B = mg.lib()
    for n in declared:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
        assert getattr(B, n).argtypes is not None, n
    for n in ("cull_outliers", "cull_sweep", "cull_rows", "cull_last_timing"):
        assert callable(getattr(mg.MapGraph, n))
    import mcptam_amd
    for n in ("cull_outliers_ref", "cull_outliers_host", "cull_sweep_ref", "cull_sweep_host"):
        assert getattr(mcptam_amd, n) is getattr(mg, n)


def test_null_handles_are_refused_with_a_message():
    from mcptam_amd import chain_bundle
    L = mg.lib()
    po, ro, ps, rs = mg.CullOutliersParams(2), mg.CullOutliersResult(), mg.CullSweepParams(20, 1, 1.0), mg.CullSweepResult()
    cnt = ctypes.c_int(7)
    ms = ctypes.c_double(0.0)
    adr = ctypes.addressof
    calls = [("mcp_map_cull_outliers", lambda: L.mcp_map_cull_outliers(None, 0, None, None, None, adr(po), None, adr(ro)), -1, "NULL graph"),
             ("mcp_map_cull_sweep", lambda: L.mcp_map_cull_sweep(None, adr(ps), adr(rs)), -1, "NULL graph"),
             ("mcp_map_cull_rows_view", lambda: L.mcp_map_cull_rows_view(None, ctypes.byref(cnt)), None, "NULL graph"),
             ("mcp_map_cull_last_timing", lambda: L.mcp_map_cull_last_timing(None, adr(ms), adr(ms)), -1, "NULL graph"),
             ("mcp_map_cull_outliers_host", lambda: L.mcp_map_cull_outliers_host(0, None, None, None, None, 1, 0, None, 0, 0, None, None, None, 0, None, None, None, None, None, None, adr(ro)), -1, "NULL params"),
             ("mcp_map_cull_outliers_host", lambda: L.mcp_map_cull_outliers_host(0, None, None, None, adr(po), 1, 0, None, 0, 0, None, None, None, 0, None, None, None, None, None, None, None), -1, "NULL params or result"),
             ("mcp_map_cull_sweep_host", lambda: L.mcp_map_cull_sweep_host(None, 0, None, 0, 0, None, None, None, None, None, 0, None, None, None, adr(rs), 0, None), -1, "NULL params"),
             ("mcp_map_cull_sweep_host", lambda: L.mcp_map_cull_sweep_host(adr(ps), 0, None, 0, 0, None, None, None, None, None, 0, None, None, None, None, 0, None), -1, "NULL params or result")]
    for name, call, want, needle in calls:
        assert call() == want, name
        err = chain_bundle.last_error()
        assert err.startswith(name + ":") and needle in err, err
    assert cnt.value == 0
    # an empty map and an empty list are not refusals
    assert L.mcp_map_cull_outliers_host(0, None, None, None, adr(po), 1, 0, None, 0, 0, None, None, None, 0, None, None, None, None, None, None, adr(ro)) == 0
    assert L.mcp_map_cull_sweep_host(adr(ps), 0, None, 0, 0, None, None, None, None, None, 0, None, None, None, adr(rs), 0, None) == 0


def test_constants_and_struct_sizes_match_the_header(tmp_path):
    h = _header()
    want = dict(MCP_SRC_TRACKER=mg.SRC_TRACKER, MCP_SRC_REFIND=mg.SRC_REFIND, MCP_SRC_ROOT=mg.SRC_ROOT, MCP_SRC_TRAIL=mg.SRC_TRAIL, MCP_SRC_EPIPOLAR=mg.SRC_EPIPOLAR,
                MCP_CULL_MISSING=M_, MCP_CULL_FIXED=FX, MCP_CULL_POINT_BAD=PB, MCP_CULL_RETRY=RE, MCP_CULL_NEVER_RETRY=NR, MCP_CULL_ALREADY_BAD=AB)
    for name, value in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value, name
    assert [want[k] for k in ("MCP_SRC_TRACKER", "MCP_SRC_REFIND", "MCP_SRC_ROOT", "MCP_SRC_TRAIL", "MCP_SRC_EPIPOLAR")] == [0, 1, 2, 3, 4]      # Measurement::Src, KeyFrame.h:109
    cc_ = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc_, "no C compiler to read include/mcp_img.h with"
    names = sorted(mg.CULL_STRUCT_SIZES)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                   '  printf("multiplier %zu\\n", offsetof(mcp_cull_sweep_params, outlier_multiplier));\n  printf("marked %zu\\n", offsetof(mcp_cull_outliers_result, n_rows_marked));\n'
                   '  printf("erased %zu\\n", offsetof(mcp_cull_sweep_result, n_meas_erased));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc_, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for n in names:
        assert int(out[n]) == mg.CULL_STRUCT_SIZES[n], (n, out[n])
    assert int(out["multiplier"]) == mg.CullSweepParams.outlier_multiplier.offset and int(out["marked"]) == mg.CullOutliersResult.n_rows_marked.offset == 28
    assert int(out["erased"]) == mg.CullSweepResult.n_meas_erased.offset == 16


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_numpy(c):
    got, want = cc.turn(c, mg.cull_outliers_host, mg.cull_sweep_host), cc.ref(c)
    cc.same_turn(got, want)
    r1, r2, r3 = got["r1"], got["r2"], got["r3"]
    assert len(got["vd"]) == c["n"] == sum(r1[k] for k in ("n_missing", "n_fixed", "n_point_bad", "n_retry", "n_never_retry", "n_already_bad"))
    a0, a1, a2 = c["a"], got["a1"], got["a2"]
    assert int(a0["ms_alive"].sum()) - int(a1["ms_alive"].sum()) == r1["n_retry"] + r1["n_never_retry"]
    assert int(a1["ms_alive"].sum()) - int(a2["ms_alive"].sum()) == r2["n_meas_erased"]
    assert int(a1["pending"].sum()) == r1["n_rows_marked"] and not a2["pending"].any()
    assert r2["n_reported"] == len(got["rows"]) == r1["n_rows_marked"] + r2["n_danglers"] + r2["n_tracker_outliers"] and (np.diff(got["rows"]) > 0).all()
    Np = len(a0["pt_flags"])
    bad = np.ones(a0["n_rows"], dtype=bool); bad[:Np] = (a2["pt_flags"] & mg.GP_BAD) != 0
    assert r2["n_bad_rows"] == int(bad.sum()) and not a2["usable"][bad].any() and a2["usable"][~bad].tobytes() == a0["usable"][~bad].tobytes()
    in_table = (a0["ms_row"] >= 0) & (a0["ms_row"] < a0["n_rows"])
    assert not a2["ms_alive"][in_table][bad[a0["ms_row"][in_table]]].any()          # no bad row keeps a live measurement
    # a second sweep finds nothing new to mark, to erase or to report
    assert r3 == dict(n_danglers=0, n_tracker_outliers=0, n_reported=0, n_bad_rows=r2["n_bad_rows"], n_meas_erased=0) and len(got["rows3"]) == 0


def _verdicts(name):
    c = BY_NAME[name]
    out = []
    for fn in (mg.cull_outliers_ref, mg.cull_outliers_host):
        res, vd, a1 = fn(c["a"], c["mkf"], c["cam"], c["row"], c["bad_good_count"], n_rows=c["a"]["n_rows"])
        out.append((res, vd.tolist(), a1))
    assert out[0][:2] == out[1][:2]
    return out[1]


def test_the_order_of_the_list_decides():
    res, vd, a1 = _verdicts("good4_three_refind")
    assert vd == [NR, NR, PB] and res["n_rows_marked"] == 1 and a1["pt_flags"][0] == mg.GP_BAD and a1["pending"][0] == 1
    assert a1["ms_alive"].tolist() == [1, 0, 0, 1, 1]                               # the third entry stays alive, as in the reference: the sweep erases it
    res, vd, a1 = _verdicts("good4_three_refind_reversed")
    assert vd == [NR, NR, PB] and a1["ms_alive"].tolist() == [1, 1, 0, 0, 1]        # the same verdicts, other entries dead
    assert _verdicts("root_in_the_middle")[1] == [RE, RE, PB, AB, AB]
    assert _verdicts("root_then_count_at_most_two")[1] == [RE, PB, PB]
    assert _verdicts("good_exactly_2")[1] == [PB] and _verdicts("good_exactly_3")[1] == [RE, PB]
    res, vd, a1 = _verdicts("outlier_of_a_bad_mkf")
    assert vd == [RE, RE, RE, PB] and a1["ms_alive"].tolist() == [1, 0, 1, 0, 0]     # two deaths that leave the count at 3, one that lowers it to 2, then 2 <= 2
    res, vd, a1 = _verdicts("fixed_row_named_twice")
    assert vd == [FX, RE, FX] and res["n_fixed"] == 2 and res["n_fixed_rows"] == 1 and a1["ms_alive"].tolist() == [1, 1, 1, 1, 1, 0, 1, 1]
    res, vd, a1 = _verdicts("missing")
    assert vd == [M_] * 7 + [RE] and res["n_missing"] == 7 and a1["pt_flags"].tolist() == BY_NAME["missing"]["a"]["pt_flags"].tolist()
    res, vd, a1 = _verdicts("bad_by_the_host")
    assert vd == [AB, PB, PB] and res["n_rows_marked"] == 0 and not a1["pending"].any() and a1["ms_alive"].all()
    assert _verdicts("every_source")[1] == [RE, NR, PB, NR, RE]
    assert _verdicts("bad_good_count_3")[1] == [NR, PB, PB]
    res, vd, a1 = _verdicts("one_row_257")
    assert vd[200] == PB and set(vd[:200]) == {RE, NR} and set(vd[201:]) == {AB} and res["n_rows_marked"] == 1


def test_the_sweep_thresholds():
    def marks(name):
        c = BY_NAME[name]
        out = [fn(c["a"], n_rows=c["a"]["n_rows"], **c["sweep"]) for fn in (mg.cull_sweep_ref, mg.cull_sweep_host)]
        assert out[0][0] == out[1][0] and out[0][1].tolist() == out[1][1].tolist()
        return out[1][0], out[1][1].tolist()
    # rows 0..5: outlier 20 | 21 against inlier 20, 21, 22; 6, 7: (14, 21), (14, 22); 8: (1, 40); 9, 10 fixed; 11..13 danglers; 14 one good measurement
    res, rows = marks("thresholds_mult_1")
    assert rows == [3, 6, 7, 8, 11, 12, 13, 14] and res["n_danglers"] == 4 and res["n_tracker_outliers"] == 4      # 21 > 20 and 21 > 20 * 1.0; 21 > 21 is false
    res, rows = marks("thresholds_mult_1p5")
    assert rows == [7, 8, 11, 12, 13, 14] and res["n_tracker_outliers"] == 2       # 21 > 14 * 1.5 is false, 22 > 21.0 is true
    res, rows = marks("thresholds_min_0")
    assert rows == list(range(9)) + [11, 12, 13, 14] and res["n_danglers"] == 4    # every row with an outlier count above 0 -- but not the fixed ones
    res, rows = marks("danglers_off")
    assert rows == [3, 6, 7, 8, 13] and res["n_danglers"] == 0 and res["n_tracker_outliers"] == 5
    res, rows = marks("one_mkf_present")
    assert rows == [2] and res == dict(n_danglers=0, n_tracker_outliers=1, n_reported=1, n_bad_rows=1, n_meas_erased=1)
    res, rows = marks("one_good_one_bad_mkf")
    assert rows == [0, 1] and res["n_danglers"] == 2 and res["n_meas_erased"] == 3


def test_what_the_report_holds():
    """Rows the host marked bad are swept and not reported; rows a cull_outliers call marked are reported once; a marked row the host rewrites
    (mcp_map_graph_update_points clears the pending mark) is not reported."""
    c = BY_NAME["good4_three_refind"]
    for outl, sweep in ((mg.cull_outliers_ref, mg.cull_sweep_ref), (mg.cull_outliers_host, mg.cull_sweep_host)):
        _, _, a1 = outl(c["a"], c["mkf"], c["cam"], c["row"])
        res, rows, a2 = sweep(a1)
        assert rows.tolist() == [0] and res == dict(n_danglers=0, n_tracker_outliers=0, n_reported=1, n_bad_rows=1, n_meas_erased=3) and not a2["ms_alive"].any()
        assert sweep(a2)[1].tolist() == []
        rewritten = mg.copy_arrays(a1); rewritten["pending"][0] = 0
        res, rows, _ = sweep(rewritten)
        assert rows.tolist() == [] and res["n_bad_rows"] == 1 and res["n_meas_erased"] == 3
        h = BY_NAME["bad_by_the_host"]
        res, rows, a2 = sweep(h["a"])
        assert rows.tolist() == [] and res == dict(n_danglers=0, n_tracker_outliers=0, n_reported=0, n_bad_rows=2, n_meas_erased=6) and not a2["usable"].any()
    for n in cc.ROW_SIZES:
        assert cc.ref(BY_NAME["rows%d_none" % n])["rows"].tolist() == [] and cc.ref(BY_NAME["rows%d_all" % n])["rows"].tolist() == list(range(n))
        assert cc.ref(BY_NAME["rows%d_last" % n])["rows"].tolist() == [n - 1]
        mixed = cc.ref(BY_NAME["rows%d_mixed" % n])
        assert mixed["r1"]["n_rows_marked"] > 0 and mixed["r2"]["n_danglers"] > 0 and mixed["r2"]["n_tracker_outliers"] > 0 and mixed["r2"]["n_bad_rows"] > mixed["r2"]["n_reported"]


def test_what_the_seeded_lists_were_made_for():
    seen = np.zeros(6, dtype=np.int64)
    for n in cc.LIST_SIZES:
        for name in ("list%d_distinct_rows" % n, "list%d" % n):
            c = BY_NAME[name]
            assert c["n"] == n
            seen += np.bincount(cc.ref(c)["vd"], minlength=6)
        assert len(set(BY_NAME["list%d_distinct_rows" % n]["row"].tolist())) == n
    assert (seen > 0).all(), seen.tolist()
    c = BY_NAME["one_row_257"]
    assert c["n"] == 257 and set(c["row"].tolist()) == {0} and int((c["a"]["ms_row"] == 0).sum()) >= 260
    s = BY_NAME["scattered_row"]
    at = np.flatnonzero(s["row"] == 7)
    assert len(at) >= 4 and (np.diff(at) == 7).all()
    assert sorted(len(BY_NAME["store%d" % m]["a"]["ms_mkf"]) for m in cc.STORE_SIZES) == list(cc.STORE_SIZES)
    assert all(len(c["a"]["ms_mkf"]) <= 4000 for c in CASES)


def test_refusals_leave_their_outputs_untouched():
    from mcptam_amd import chain_bundle
    c = BY_NAME["list65"]
    a = c["a"]

    def refused(needle, call):
        with pytest.raises(RuntimeError):
            call()
        assert needle in chain_bundle.last_error(), chain_bundle.last_error()
    k = (c["mkf"], c["cam"], c["row"])
    refused("names slot", lambda: mg.cull_outliers_host(a, np.r_[k[0][:-1], mg.MAX_MKFS], k[1], k[2]))
    refused("names slot", lambda: mg.cull_outliers_host(a, np.r_[k[0][:-1], -1], k[1], k[2]))
    refused("names camera", lambda: mg.cull_outliers_host(a, k[0], np.r_[k[1][:-1], a["ncam"]], k[2]))
    refused("names camera", lambda: mg.cull_outliers_host(a, k[0], np.r_[-1, k[1][1:]], k[2]))
    refused("appears twice", lambda: mg.cull_outliers_host(a, np.r_[k[0], k[0][3]], np.r_[k[1], k[1][3]], np.r_[k[2], k[2][3]]))
    refused("negative bad_good_count", lambda: mg.cull_outliers_host(a, *k, bad_good_count=-1))
    refused("negative min_outliers", lambda: mg.cull_sweep_host(a, min_outliers=-1))
    refused("not finite", lambda: mg.cull_sweep_host(a, outlier_multiplier=np.inf))
    refused("not finite", lambda: mg.cull_sweep_host(a, outlier_multiplier=np.nan))
    # the raw calls: every in-place array and every output keeps its bytes
    b = mg._cull_state(a, a["n_rows"])
    n = c["n"]
    m2 = c["mkf"].copy(); m2[n // 2] = m2[n // 2 - 1]
    c2 = c["cam"].copy(); c2[n // 2] = c2[n // 2 - 1]
    r2 = c["row"].copy(); r2[n // 2] = r2[n // 2 - 1]                              # a repeated key in the middle of the list
    vd = np.full(n, 99, dtype=np.uint8)
    po, ro = mg.CullOutliersParams(2), mg.CullOutliersResult(*([-5] * 8))
    before = {k_: b[k_].tobytes() for k_ in ("pt_flags", "pending", "ms_alive", "usable")}
    L = mg.lib()
    rc = L.mcp_map_cull_outliers_host(n, m2.ctypes.data, c2.ctypes.data, r2.ctypes.data, ctypes.addressof(po), b["ncam"], len(b["mkf_flags"]), b["mkf_flags"].ctypes.data, b["n_rows"],
                                      len(b["pt_flags"]), b["src_mkf"].ctypes.data, b["pt_flags"].ctypes.data, b["pending"].ctypes.data, len(b["ms_mkf"]), b["ms_mkf"].ctypes.data,
                                      b["ms_cam"].ctypes.data, b["ms_row"].ctypes.data, b["ms_source"].ctypes.data, b["ms_alive"].ctypes.data, vd.ctypes.data, ctypes.addressof(ro))
    assert rc == -1 and "appears twice" in chain_bundle.last_error()
    assert (vd == 99).all() and ro.as_dict() == {k_: -5 for k_ in ro.as_dict()} and all(b[k_].tobytes() == v for k_, v in before.items())
    # a report that does not fit is found before anything is written
    want_rows = cc.ref(BY_NAME["rows257_all"])["rows"]
    b = mg._cull_state(BY_NAME["rows257_all"]["a"])
    before = {k_: b[k_].tobytes() for k_ in ("pt_flags", "pending", "ms_alive", "usable")}
    ps, rs = mg.CullSweepParams(20, 1, 1.0), mg.CullSweepResult(*([-5] * 5))
    rows = np.full(len(want_rows) - 1, -7, dtype=np.int32)
    rc = L.mcp_map_cull_sweep_host(ctypes.addressof(ps), len(b["mkf_flags"]), b["mkf_flags"].ctypes.data, b["n_rows"], len(b["pt_flags"]), b["pt_flags"].ctypes.data, b["pending"].ctypes.data,
                                   b["inlier"].ctypes.data, b["outlier"].ctypes.data, b["usable"].ctypes.data, len(b["ms_mkf"]), b["ms_mkf"].ctypes.data, b["ms_row"].ctypes.data,
                                   b["ms_alive"].ctypes.data, ctypes.addressof(rs), len(rows), rows.ctypes.data)
    assert rc == -1 and "257 rows are reported, cap_rows is 256" in chain_bundle.last_error()
    assert (rows == -7).all() and rs.as_dict() == {k_: -5 for k_ in rs.as_dict()} and all(b[k_].tobytes() == v for k_, v in before.items())


def test_host_unit_under_the_sanitizers(tmp_path):
    """tests/cpp/cull_host_check.cpp has its own main: it calls the two host twins on seam-sized maps against the rules written out there.  Built
    from the host unit alone with AddressSanitizer and UndefinedBehaviorSanitizer (nothing sanitized is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "cull_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it needs nothing preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cull_host_check.cpp"), os.path.join(ROOT, "mcptam_amd", "csrc", "map_graph_cull_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cull host ok" in out.stdout
