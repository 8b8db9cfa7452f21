"""The co-visible points of the nearest keyframe without a device (include/mcp_img.h mcp_map_collect_nearest, mcp_track_collect_nearest):
the new symbols are exported, bound and declared and the struct sizes are the header's; on every case of tests/collect_cases.py the host
twin (the bodies the kernels call, under the host compiler) equals the set restatement mcptam_amd.map_graph.collect_nearest_ref -- the mask
and every integer of the report exactly, nearest_dist to rtol 1e-12 (what victim_dist is allowed against its restatement) -- and the answers
that can be read off a case's description; every refusal of the host twin leaves its outputs untouched."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import collect_cases as cl
from mcptam_amd import map_graph as mg
from mcptam_amd import pvs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cl.all_cases()
BY_NAME = {c["name"]: c for c in CASES}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)


def test_symbols_are_exported_bound_and_declared():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe
    declared = sorted(set(re.findall(r"\b(mcp_(?:map|track)_collect_[a-z0-9_]*)\s*\(", _header())))
    assert declared == sorted(mg.COLLECT_SYMBOLS) and len(declared) == 6
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    Bd = pvs._bind_collect(mg.lib())
    for n in declared:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
        assert getattr(Bd, n).argtypes is not None, n
    for n in ("collect_nearest", "collect_rows", "collect_last_timing"):
        assert callable(getattr(mg.MapGraph, n)), n
    for n in ("collect_nearest", "collect_nearest_off", "collect_last"):
        assert callable(getattr(pvs.MapPointTable, n)), n
    import mcptam_amd
    for n in ("collect_nearest_ref", "collect_nearest_host"):
        assert getattr(mcptam_amd, n) is getattr(mg, n)


def test_struct_sizes_match_the_header(tmp_path):
    cc_ = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc_, "no C compiler to read include/mcp_img.h with"
    names = sorted(mg.COLLECT_STRUCT_SIZES)
    offs = [("mcp_collect_params", pvs.CollectParams, f) for f in ("depth_mean", "active")] + \
           [("mcp_collect_report", pvs.CollectReport, f) for f in ("status", "nearest_slot", "nearest_cam", "nearest_dist", "n_candidates", "n_seed_rows", "n_kfs", "n_rows")]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                   "".join('  printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (s, f, s, f) for s, _, f in offs) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call([cc_, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for n in names:
        assert int(out[n]) == mg.COLLECT_STRUCT_SIZES[n], (n, out[n])
    for s, cls, f in offs:
        assert int(out["%s.%s" % (s, f)]) == getattr(cls, f).offset, (s, f)
    assert mg.MAX_CAMS == pvs.MAX_FRAME_CAMS == 8 and ctypes.sizeof(pvs.CollectReport) == 296


def _same(got, want, what):
    assert got["valid"] == want["valid"] == 1, what
    for k in cl.INT_FIELDS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    np.testing.assert_allclose(got["nearest_dist"], want["nearest_dist"], rtol=1e-12, atol=0.0, err_msg=str(what))


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_host_twin_equals_the_set_restatement(c):
    rep, near = mg.collect_nearest_host(c["a"], **cl.kwargs(c))
    want, want_near = cl.ref(c)
    _same(rep, want, c["name"])
    assert near.dtype == np.uint8 and near.tobytes() == want_near.tobytes(), c["name"]
    C = int(c["a"]["ncam"])
    assert not (near >> C).any(), "a bit past the camera count"
    off = np.flatnonzero(c["active"][:C] == 0)
    assert not ((near[:, None] >> off[None, :]) & 1).any(), "a bit of a camera that is switched off"
    for cam in range(C):
        assert int(((near >> cam) & 1).sum()) == rep["n_rows"][cam]
    assert (rep["status"][C:] == 0).all() and (rep["nearest_slot"][C:] == -1).all() and (rep["nearest_cam"][C:] == -1).all()


@pytest.mark.parametrize("c", [c for c in CASES if c["near"] is not None], ids=[c["name"] for c in CASES if c["near"] is not None])
def test_the_answers_read_off_the_description(c):
    rep, near = mg.collect_nearest_host(c["a"], **cl.kwargs(c))
    assert near.tolist() == c["near"].tolist(), c["name"]
    n = len(c["status"])
    assert rep["status"][:n].tolist() == c["status"]
    assert list(zip(rep["nearest_slot"][:n].tolist(), rep["nearest_cam"][:n].tolist())) == c["winners"]


def test_two_hops_marks_k1_and_not_k2():
    rep, near = mg.collect_nearest_host(BY_NAME["two_hops_not_three"]["a"], **cl.kwargs(BY_NAME["two_hops_not_three"]))
    assert rep["n_seed_rows"][0] == 1 and rep["n_kfs"][0] == 2 and rep["n_rows"][0] == 2 and near.tolist() == [1, 1, 0, 0]
    rep, _ = mg.collect_nearest_host(BY_NAME["nearest_without_an_entry"]["a"], **cl.kwargs(BY_NAME["nearest_without_an_entry"]))
    assert rep["status"][0] == 0 and rep["n_kfs"][0] == 0 and rep["n_rows"][0] == 0 and rep["nearest_dist"][0] == 1.5
    rep, _ = mg.collect_nearest_host(BY_NAME["last_slot_last_camera"]["a"], **cl.kwargs(BY_NAME["last_slot_last_camera"]))
    assert rep["nearest_slot"][7] == mg.MAX_MKFS - 1 and rep["nearest_cam"][7] == 7 and rep["n_candidates"][7] == 24


def test_entries_outside_the_table_or_the_rig_do_not_count():
    """What mcp_map_graph_add_meas never lets into a device store, so only the twins see it: rows past the table, negative ids, a camera of 8."""
    c = BY_NAME["two_hops_not_three"]
    a = mg.copy_arrays(c["a"])
    extra = np.array([(0, 0, 4), (0, 0, -1), (-1, 0, 2), (mg.MAX_MKFS, 0, 2), (0, 8, 2), (0, -1, 2)], dtype=np.int32)
    for k, col in enumerate(("ms_mkf", "ms_cam", "ms_row")):
        a[col] = np.concatenate([a[col], extra[:, k]]).astype(np.int32)
    a["ms_alive"] = np.concatenate([a["ms_alive"], np.ones(len(extra), np.uint8)])
    rep, near = mg.collect_nearest_host(a, **cl.kwargs(c))
    want, want_near = mg.collect_nearest_ref(a, **cl.kwargs(c))
    _same(rep, want, "extra entries")
    assert near.tolist() == want_near.tolist() == [1, 1, 0, 0]


def test_the_seeded_map_keeps_a_part_of_the_rows():
    c = BY_NAME["seeded_32x2"]
    rep, near = cl.ref(c)
    assert len(c["a"]["ms_mkf"]) == 4000 and len(near) == 600 and len(c["a"]["mkf_flags"]) == 32
    for cam in range(2):
        assert 30 <= rep["n_rows"][cam] <= 570 and rep["n_seed_rows"][cam] < rep["n_rows"][cam] and rep["n_kfs"][cam] > 1


def test_refusals_of_the_host_twin_leave_the_outputs_untouched():
    c = BY_NAME["two_cameras_two_winners"]
    a, k = c["a"], cl.kwargs(c)
    L = pvs._bind_collect(mg.lib())
    C, P_, cfb, bfw, mf, act, dep = mg._mkf_columns(a)
    M = len(a["ms_mkf"])
    mm, mc, mr = (np.ascontiguousarray(a[q], dtype=np.int32) for q in ("ms_mkf", "ms_cam", "ms_row"))
    al = np.ascontiguousarray(a["ms_alive"], dtype=np.uint8)

    def call(pose=None, prm=None, ncam=C, rep=True, n_rows=6, cur=None):
        pose = np.ascontiguousarray(c["pose"] if pose is None else pose, dtype=np.float64)
        prm = pvs.collect_params(k["depth_mean"], k["mean_diff_fraction"], k["active"]) if prm is None else prm
        out = pvs.CollectReport(); ctypes.memset(ctypes.addressof(out), 0x5a, ctypes.sizeof(out))
        near = np.full(6, 0x5a, dtype=np.uint8)
        rc = L.mcp_map_collect_nearest_host(pose.ctypes.data, None if cur is None else cur.ctypes.data, ctypes.addressof(prm) if prm else None, ncam, cfb.ctypes.data, P_, bfw.ctypes.data,
                                            mf.ctypes.data, act.ctypes.data, dep.ctypes.data, n_rows, M, mm.ctypes.data, mc.ctypes.data, mr.ctypes.data, al.ctypes.data,
                                            ctypes.addressof(out) if rep else None, near.ctypes.data)
        from mcptam_amd import chain_bundle
        return rc, chain_bundle.last_error(), bytes(out), near
    rc, _, out, near = call()
    assert rc == 0 and near.tolist() == c["near"].tolist()
    bad_pose = c["pose"].copy(); bad_pose[10] = np.nan
    nan_frac = pvs.collect_params(k["depth_mean"], np.inf, k["active"])
    zero_depth = pvs.collect_params([2.0, 0.0], 0.5, [1, 1])
    nan_depth = pvs.collect_params([np.nan, 2.0], 0.5, [1, 1])
    bad_cur = np.tile(cl.nc.IDENT, (2, 1)); bad_cur[1, 3] = np.inf
    for kw, word in ((dict(pose=bad_pose), "pose"), (dict(prm=nan_frac), "mean_diff_fraction"), (dict(prm=zero_depth), "depth mean"), (dict(prm=nan_depth), "depth mean"),
                     (dict(prm=0), "NULL"), (dict(rep=False), "NULL"), (dict(ncam=0), "bad arguments"), (dict(ncam=9), "bad arguments"), (dict(n_rows=-1), "bad arguments"),
                     (dict(cur=bad_cur), "CamFromBase")):
        rc, err, out, near = call(**kw)
        assert rc == -1 and err.startswith("mcp_map_collect_nearest_host") and word in err, (kw, err)
        assert out == b"\x5a" * len(out) and (near == 0x5a).all(), kw
    # the depth mean of a camera that is switched off is not looked at
    rc, _, _, near = call(prm=pvs.collect_params([2.0, -1.0], 0.5, [1, 0]))
    assert rc == 0 and near.tolist() == BY_NAME["a_camera_switched_off"]["near"].tolist()
    with pytest.raises(RuntimeError, match="mcp_map_collect_nearest_host"):
        mg.collect_nearest_host(a, bad_pose, k["depth_mean"])


def test_host_unit_under_the_sanitizers(tmp_path):
    """tests/cpp/collect_host_check.cpp has its own main with exactly sized arrays: it calls the host twin against answers written out there.  The
    host unit shares __host__ __device__ bodies with the kernels, so both are built as the host half of a HIP source, with AddressSanitizer and
    UndefinedBehaviorSanitizer on the host side; the program runs on its own (nothing sanitized is loaded into Python)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "no hipcc"
    exe = str(tmp_path / "collect_host_check")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-x", "hip", "--cuda-host-only"] + san + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "collect_host_check.cpp"), os.path.join(ROOT, "mcptam_amd", "csrc", "map_graph_collect_host.cpp"),
                           "-fsanitize=address,undefined", "-static-libsan", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "collect host ok" in out.stdout
