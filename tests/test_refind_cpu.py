"""CPU-side checks of the one-call re-find (include/mcp_img.h: mcp_map_refind, mcp_map_refind_view): the boundary exists, the ctypes layouts
are the host compiler's, the C++ mirror links, NULL tables are refused without touching a device, and the numpy derivation of verdicts
(mcptam_amd.refind.refind_verdicts) on the CPU oracle's records of the tests' map gives the classes the GPU comparison relies on."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from refind_fixture import EXPECTED, EXPECTED_FOUND_L0, EXPECTED_FOUND_UP, N_BASE, compose, make_world, newly_made_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mcp_map_refind", "mcp_map_refind_view"]
CONSTANTS = dict(MCP_REFIND_FOUND=1, MCP_REFIND_OUTSIDE=2, MCP_REFIND_TEMPLATE_BAD=3, MCP_REFIND_NOT_FOUND=4, MCP_REFIND_NO_SOURCE=5)


def test_refind_entry_points_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "mcp_img.h")).read()
    assert "duplicates are not detected" in txt.lower()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for s in ("mcp_refind_target", "mcp_refind_meas", "mcp_refind_result"):
        assert re.search(r"typedef struct %s\s*\{" % s, txt), s
    for n in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe, refind
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    for n in SYMBOLS:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
    assert sorted(refind.REFIND_SYMBOLS) == sorted(SYMBOLS)


def test_layouts_and_constants_match_the_header(tmp_path):
    from mcptam_amd import refind as R
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    structs = [("mcp_refind_target", R.RefindTarget, ("kf", "cam", "cam_from_world")),
               ("mcp_refind_meas", R.RefindMeas, ("pair", "row", "target", "level", "subpix", "score", "root_pos")),
               ("mcp_refind_result", R.RefindResult, ("counts", "n_meas"))]
    body = ""
    for cname, _, names in structs:
        body += 'printf("%%d", (int)sizeof(%s));\n' % cname + "".join('printf(" %%d", (int)offsetof(%s, %s));\n' % (cname, f) for f in names) + 'printf("\\n");\n'
    body += 'printf("' + " ".join(["%d"] * len(CONSTANTS)) + '\\n", ' + ", ".join(CONSTANTS) + ");\n"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + body + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = [[int(v) for v in ln.split()] for ln in subprocess.check_output([str(exe)]).decode().strip().split("\n")]
    for (cname, cls, names), got in zip(structs, lines):
        assert got == [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f in names], cname
    assert lines[1][0] == R.REFIND_MEAS_DTYPE.itemsize and [R.REFIND_MEAS_DTYPE.fields[f][1] for f in structs[1][2]] == lines[1][1:]
    assert lines[3] == list(CONSTANTS.values())
    assert [R.FOUND, R.OUTSIDE, R.TEMPLATE_BAD, R.NOT_FOUND, R.NO_SOURCE] == list(CONSTANTS.values())


def test_refind_refuses_a_null_table():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import lib
    from mcptam_amd.refind import RefindResult, _bind
    L = _bind(lib())
    res = RefindResult()
    res.n_meas = 77
    assert L.mcp_map_refind(None, 0, None, 0, None, 0, None, None, 0, None, ctypes.byref(res)) == -1
    assert "mcp_map_refind: NULL table" in chain_bundle.last_error()
    assert res.n_meas == 77
    cnt = ctypes.c_int(5)
    assert L.mcp_map_refind_view(None, ctypes.byref(cnt)) is None and cnt.value == 0
    assert "mcp_map_refind_view" in chain_bundle.last_error()


def test_cpp_refind_compiles_and_links(tmp_path):
    """include/mcptam_hip/KeyFrame.hpp: MapPointTable::ReFindPairs instantiated and linked (not run: no GPU)."""
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "refind_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'static int use(int argc) {\n'
                   '  mcptam_hip::MapPointTable t(-1);\n'
                   '  mcp_camera cam; std::memset(&cam, 0, sizeof cam);\n'
                   '  std::vector<mcp_refind_target> targets(argc);\n'
                   '  for (int k = 0; k < argc; ++k) { targets[k].kf = NULL; targets[k].cam = &cam; }\n'
                   '  std::vector<int> pairs(2*argc, 0);\n'
                   '  mcp_pf_state finder; std::memset(&finder, 0, sizeof finder);\n'
                   '  mcptam_hip::ReFindResult a = t.ReFindPairs(targets, pairs, true, &finder);\n'
                   '  mcptam_hip::ReFindResult b = t.ReFindPairs(targets, pairs, false, NULL, true);\n'
                   '  return (int)a.verdict.size() + a.counts[MCP_REFIND_FOUND] + b.n_meas + (b.view ? 1 : 0);\n}\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) { std::printf("linked\\n"); return 0; }\n'
                   '  return use(argc);\n}\n')
    exe = tmp_path / "refind_link"
    lib = os.path.join(ROOT, "mcptam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lmcptam_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linked" in out.stdout


def test_refind_verdicts_by_hand():
    from mcptam_amd.keyframe import TD_OUT_DTYPE
    from mcptam_amd.refind import FOUND, NOT_FOUND, OUTSIDE, TEMPLATE_BAD, refind_verdicts, verdict_counts
    o = np.zeros(5, dtype=TD_OUT_DTYPE)
    o["in_image"] = [0, 1, 1, 1, 1]
    o["template_bad"] = [1, 1, 0, 0, 0]          # (outside wins over a bad template: the reference returns at :945-956 first)
    o["found"] = [1, 1, 0, 1, 1]
    o["search_level"] = [0, 0, 0, 0, 2]
    o["did_subpix"] = [0, 0, 0, 0, 1]
    o["score"] = [0, 0, 0, 123, 456]
    o["found_pos"] = [[0, 0], [0, 0], [0, 0], [10.5, 20.5], [33.25, 44.75]]
    pairs = np.array([[9, 0], [8, 1], [7, 0], [6, 1], [5, 2]])
    v, m = refind_verdicts(o, pairs)
    assert list(v) == [OUTSIDE, TEMPLATE_BAD, NOT_FOUND, FOUND, FOUND]
    assert list(m["pair"]) == [3, 4] and list(m["row"]) == [6, 5] and list(m["target"]) == [1, 2]
    assert list(m["level"]) == [0, 2] and list(m["subpix"]) == [0, 1] and list(m["score"]) == [123, 456]
    assert m["root_pos"].tolist() == [[10.5, 20.5], [33.25, 44.75]]
    assert list(verdict_counts(v)) == [0, 2, 1, 1, 1, 0]
    v0, m0 = refind_verdicts(o[:0])
    assert len(v0) == 0 and len(m0) == 0


def test_the_map_of_the_gpu_tests_fills_every_class():
    """The oracle's records of the tests' map against B: the classes of the issue, none of them hollow."""
    import oracle
    from mcptam_amd.refind import FOUND
    w = make_world(oracle.OracleKeyFrame)
    pairs = np.stack([np.arange(w["n"]), np.zeros(w["n"], dtype=int)], axis=1)
    v, m, counts, _, _ = compose(w["cols"], None, [(w["B"], w["cam"], w["sc"]["poseB"])], pairs, search=oracle.oracle_patch_sequences, src_oracle=w["A"])
    l0, up = int((m["level"] == 0).sum()), int((m["level"] > 0).sum())
    print("counts", counts.tolist(), "found at level 0", l0, "above", up)
    for verdict, want in EXPECTED.items():
        assert counts[verdict] == want, (verdict, int(counts[verdict]), want)
        assert counts[verdict] >= 100
    assert (l0, up) == (EXPECTED_FOUND_L0, EXPECTED_FOUND_UP) and l0 >= 100 and up >= 100
    assert counts[FOUND] == len(m) and (m["subpix"] == (m["level"] > 0)).all()


def test_shared_templates_are_observable_on_the_oracle():
    """The ReFindNewlyMade shape on the oracle: one finder per row changes what the slightly moved view scores; the view turned by pi sees nothing."""
    import oracle
    from mcptam_amd.refind import OUTSIDE
    w = make_world(oracle.OracleKeyFrame)
    targets = newly_made_targets(w["sc"], w["B"])
    pairs = np.stack([np.repeat(np.arange(N_BASE), 4), np.tile(np.arange(4), N_BASE)], axis=1)
    kw = dict(search=oracle.oracle_patch_sequences, src_oracle=w["A"])
    v1, m1, _, _, _ = compose(w["cols"], None, targets, pairs, per_row_finders=True, **kw)
    v0, m0, _, _, _ = compose(w["cols"], None, targets, pairs, per_row_finders=False, **kw)
    s1, s0 = dict(zip(m1["pair"], m1["score"])), dict(zip(m0["pair"], m0["score"]))
    differ = sum(1 for p in s1 if pairs[p, 1] == 1 and p in s0 and s0[p] != s1[p])
    print("pairs of target 1 whose score differs:", differ)
    assert differ >= 100
    assert (v1[pairs[:, 1] == 2] == OUTSIDE).all() and (v0[pairs[:, 1] == 2] == OUTSIDE).all()


def test_walk_kernel_keeps_its_registers(tmp_path):
    """The compiler's own report for gfx950: none of the four re-find kernels spills to scratch (the walk carries a finder, a survivor record and
    patch_item's live values in registers)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    csrc = os.path.join(ROOT, "mcptam_amd", "csrc")
    out = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-ffp-contract=off", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-c", "-o", str(tmp_path / "img_api.dev.o"), os.path.join(csrc, "img_api.hip")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    seen = {}
    name = None
    for ln in out.stderr.split("\n"):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            for k in ("k_rf_mark", "k_rf_scatter", "k_rf_walk", "k_rf_commit"):
                if k in name:
                    seen[k] = int(m.group(1))
    print(seen)
    assert seen == dict(k_rf_mark=0, k_rf_scatter=0, k_rf_walk=0, k_rf_commit=0)
