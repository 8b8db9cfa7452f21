"""The keyframe lists of the map graph without a device: mcp_graph_kf_lists_host (the bodies the kernels call, under the host compiler) equals
the numpy restatement mcptam_amd.map_graph.kf_lists_ref exactly -- integers and the weights' bit patterns -- on the three synthetic maps and on
hand-made stores; the refusals; the new symbols are exported, bound and declared; and the host unit under the sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import graph_list_cases as lc
from mcptam_amd import map_graph as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lc.all_cases()


@pytest.mark.parametrize("name,a,slots,n_rows", CASES, ids=[c[0] for c in CASES])
def test_host_equals_numpy(name, a, slots, n_rows):
    got, want = mg.kf_lists_host(a, slots, n_rows), mg.kf_lists_ref(a, slots, n_rows)
    lc.assert_same_lists(got, want)
    ss, sr, sw = got
    assert ss[0] == 0 and ss[-1] == len(sr) == len(sw) and (np.diff(ss) >= 0).all()
    assert ((sw >= 0) & (sw <= 1)).all()


def test_what_the_hand_made_stores_were_made_for():
    """The cases do what their names say (so that equality above is not equality of two empty answers)."""
    got = {name: (a, np.asarray(slots), mg.kf_lists_ref(a, slots, n_rows)) for name, a, slots, n_rows in lc.hand_cases()}
    assert got["empty-store"][2][0].tolist() == [0] * 5 and len(got["empty-store"][2][1]) == 0
    ss, sr, sw = got["one-entry"][2]
    assert ss.tolist() == [0, 0, 0, 0, 1] and sr.tolist() == [4]
    ss, sr, _ = got["one-keyframe"][2]
    assert ss.tolist() == [0, 0, 0, 50, 50, 50, 50] and sr.tolist() == list(range(49, -1, -1))              # store order, not row order
    ss, sr, _ = got["64x8-one-each"][2]
    assert (np.diff(ss) == 1).all() and len(sr) == 512
    a, _, (ss, sr, _) = got["dead-entries"]
    assert 0 < len(sr) < int(a["ms_alive"].sum())
    a, _, (ss, sr, _) = got["bad-rows"]
    assert len(sr) == int(((a["pt_flags"][a["ms_row"]] & mg.GP_BAD) == 0).sum()) < len(a["ms_row"])
    a, _, (ss, sr, _) = got["rows-past-the-graph-columns"]
    assert len(sr) == int((a["ms_row"] < 20).sum()) and (a["ms_row"] >= 20).any()
    a, _, (ss, sr, _) = got["rows-past-the-table"]
    assert len(sr) == int((a["ms_row"] < 25).sum()) and (a["ms_row"] >= 25).any()
    a, _, (ss, sr, _) = got["inactive-camera"]
    n = np.diff(ss).reshape(4, 3)
    assert n[1, 1] == 0 and (n[3] == 0).all() and ((a["ms_mkf"] == 1) & (a["ms_cam"] == 1)).any() and (a["ms_mkf"] == 3).any() and n[1, 0] > 0
    _, slots, (ss, _, _) = got["listed-mkf-without-entries"]
    assert (np.diff(ss).reshape(3, 2)[1] == 0).all() and slots[1] == 2
    a, slots, (ss, sr, _) = got["mkfs-not-listed"]
    assert len(sr) == int(np.isin(a["ms_mkf"], slots).sum()) < len(a["ms_mkf"])
    ss, sr, _ = got["row-seen-by-several-cameras"][2]
    assert ss.tolist() == [0, 1, 1, 2, 2, 3, 5, 6, 7] and sr.tolist() == [3, 3, 3, 3, 5, 3, 3]
    ss, sr, sw = got["counts"][2]
    assert sr.tolist() == [2, 0, 1] and sw.tolist() == [1.0 / 1001.0, 1.0, 0.75]


def test_refusals():
    from mcptam_amd import chain_bundle
    a = lc.hand(20, 4, 2, 30, 100)

    def refused(needle, slots, **edit):
        b = mg.copy_arrays(a); b.update(edit)
        with pytest.raises(RuntimeError):
            mg.kf_lists_host(b, slots)
        assert needle in chain_bundle.last_error(), chain_bundle.last_error()
    refused("outside the MKF columns", [0, 4])
    refused("outside the MKF columns", [-1])
    refused("appears twice", [2, 1, 2])
    fl = a["mkf_flags"].copy(); fl[3] = 0
    refused("not present", [3], mkf_flags=fl)
    refused("inlier < 1", [0], inlier=-np.ones(30, dtype=np.int32))
    refused("inlier < 1", [0], inlier=np.zeros(30, dtype=np.int32), outlier=np.zeros(30, dtype=np.int32))      # (0, 0): what the table's column refuses too
    refused("outlier < 0", [0], outlier=-np.ones(30, dtype=np.int32))
    big = mg.copy_arrays(a); big["inlier"][:], big["outlier"][:] = 2 ** 30, 2 ** 31 - 1                         # a sum past the int range
    got = mg.kf_lists_host(big, [0, 3])
    lc.assert_same_lists(got, mg.kf_lists_ref(big, [0, 3]))
    assert len(got[2]) and (got[2] == 2.0 ** 30 / (2.0 ** 30 + 2.0 ** 31 - 1)).all()
    lc.assert_same_lists(mg.kf_lists_host(a, [0, 3]), mg.kf_lists_ref(a, [0, 3]))


def test_new_symbols_are_exported_bound_and_declared():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mcp_graph_[a-z0-9_]+)\s*\(", txt)))
    assert declared == sorted(mg.GRAPH_LIST_SYMBOLS) and len(declared) == 5
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    B = mg.lib()
    for n in declared:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
        assert getattr(B, n).argtypes is not None, n
    for n in ("debug_kf_lists", "refresh_depth", "write_back", "get_mkfs"):
        assert callable(getattr(mg.MapGraph, n))
    import mcptam_amd
    assert mcptam_amd.kf_lists_ref is mg.kf_lists_ref and mcptam_amd.kf_lists_host is mg.kf_lists_host


def test_host_unit_under_the_sanitizers(tmp_path):
    """tests/cpp/kf_lists_host_check.cpp has its own main: it calls mcp_graph_kf_lists_host on seam-sized stores against a sort of its own.
    Built from the host unit alone with AddressSanitizer and UndefinedBehaviorSanitizer (nothing sanitized is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "kf_lists_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it needs nothing preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "kf_lists_host_check.cpp"), os.path.join(ROOT, "mcptam_amd", "csrc", "map_graph_lists_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kf lists host ok" in out.stdout
