"""CPU-side checks of the one-call TrackMap (include/mcp_img.h: mcp_map_points_set_source / _update_source / _get_states, mcp_track_map,
mcp_track_map_view): the declarations exist and are exported, the ctypes layouts are the host compiler's, the keyed shuffle of every
layer is the header's, the Python selection is TestForCoarse + SetupFineTracking (src/Tracker.cc:726-770, 840-883) with the shuffles
given, and the C++ mirror links."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cc():
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    return cc


def test_track_map_entry_points_declared_and_exported():
    from mcptam_amd.pvs import TRACK_MAP_SYMBOLS
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcp_img.h")).read(), flags=re.S)
    for s in ("mcp_track_map_params", "mcp_track_map_result", "mcp_track_map_item"):
        assert re.search(r"typedef struct %s\s*\{" % s, txt), s
    for n in TRACK_MAP_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    for n in TRACK_MAP_SYMBOLS:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n


def test_track_map_struct_layouts_match_the_header(tmp_path):
    from mcptam_amd.pvs import TRACK_MAP_ITEM_DTYPE, TrackMapItem, TrackMapParams, TrackMapResult
    fields = {"mcp_track_map_params": (TrackMapParams, ["try_coarse", "coarse_max", "coarse_range", "coarse_min", "coarse_subpix_its", "max_patches",
                                                        "estimator", "seed"]),
              "mcp_track_map_result": (TrackMapResult, ["did_coarse", "coarse_found", "pvs_counts", "set_sizes", "stale", "mu_last"]),
              "mcp_track_map_item": (TrackMapItem, ["point", "stage", "weight_last", "out"])}
    body = []
    for s, (_, fs) in fields.items():
        body.append('printf("%%d\\n", (int)sizeof(%s));' % s)
        body += ['printf("%%d\\n", (int)offsetof(%s, %s));' % (s, f) for f in fs]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(body) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([_cc(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for s, (cls, fs) in fields.items():
        want.append(ctypes.sizeof(cls))
        want += [getattr(cls, f).offset for f in fs]
    assert got == want
    assert TRACK_MAP_ITEM_DTYPE.itemsize == ctypes.sizeof(TrackMapItem)
    assert [TRACK_MAP_ITEM_DTYPE.fields[f][1] for f in ("point", "stage", "weight_last", "out")] == [getattr(TrackMapItem, f).offset for f in ("point", "stage", "weight_last", "out")]


def test_python_shuffle_key_is_the_headers(tmp_path):
    from mcptam_amd.pvs import shuffle_key
    rng = np.random.default_rng(3)
    seeds = [0, 1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0] + [int(v) for v in rng.integers(0, 2**63, 4, dtype=np.uint64)]
    cases = [(s, st, c, r) for s in seeds for st in (0, 1, 7) for c in (0, 3, 7) for r in (0, 1, 999, 49999, 0x7FFFFFFE)]
    src = tmp_path / "keys.c"
    lines = ['printf("%%llu\\n", (unsigned long long)mcp_track_shuffle_key(%dull, %d, %d, %d));' % c for c in cases]
    src.write_text('#include <stdio.h>\n#include "mcp_img.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "keys"
    subprocess.check_call([_cc(), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [int(shuffle_key(s, st, c, [r])[0]) for s, st, c, r in cases]
    assert got == want
    # ... and the library's exported copy (for callers that do not compile the header)
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    L.mcp_track_shuffle_key.restype = ctypes.c_uint64
    L.mcp_track_shuffle_key.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.mcp_mix64.restype = ctypes.c_uint64
    L.mcp_mix64.argtypes = [ctypes.c_uint64]
    assert [int(L.mcp_track_shuffle_key(s, st, c, r)) for s, st, c, r in cases] == got
    from mcptam_amd.pvs import _mix64
    assert [int(L.mcp_mix64(s)) for s in seeds] == [int(_mix64(np.uint64(s))) for s in seeds]
    # distinct rows give distinct keys (mcp_mix64 is a bijection): the order is total without ties
    k = shuffle_key(42, 0, 1, np.arange(200000))
    assert len(np.unique(k)) == 200000


def _reference_sets(pvs_levels, perm0, chop, try_coarse, coarse_max, max_patches):
    """TestForCoarse + SetupFineTracking as list code, the shuffles given: perm0(list) = the per-level shuffle (:983), chop(list) = the
    random_shuffle before the chop (:879)."""
    levels = [perm0(list(pvs_levels[l])) for l in range(4)]
    iteration = []
    if try_coarse:
        nxt = []
        if len(levels[3]) <= coarse_max:
            nxt = list(levels[3]); levels[3] = []
        else:
            nxt = levels[3][:coarse_max]; del levels[3][:coarse_max]
        if len(nxt) < coarse_max:
            more = coarse_max - len(nxt)
            if len(levels[2]) <= more:
                nxt += levels[2]; levels[2] = []
            else:
                nxt += levels[2][:more]; del levels[2][:more]
        iteration = list(nxt)
    C = list(iteration)
    T = list(levels[3])
    iteration += T
    nxt = []
    for l in (2, 1, 0):
        nxt += levels[l]
    use = max(0, max_patches - len(iteration))
    if len(nxt) > use:
        nxt = chop(nxt)[:use]
    return C, T, nxt


@pytest.mark.parametrize("case", ["l3_le_max", "l3_gt_max", "l2_topup", "no_coarse", "k_clamped", "no_chop"])
def test_python_selection_is_test_for_coarse_and_setup_fine_tracking(case):
    from mcptam_amd.pvs import select_sets, shuffle_key
    rng = np.random.default_rng(11)
    sizes, try_coarse, coarse_max, max_patches = {
        "l3_le_max": ((300, 200, 100, 20), True, 60, 400),        # all of L3 and a top-up from L2 in C
        "l3_gt_max": ((300, 200, 100, 90), True, 60, 400),        # L3 alone fills C; T = the rest of L3
        "l2_topup": ((300, 200, 30, 5), True, 60, 400),           # L2 smaller than the top-up: all of it
        "no_coarse": ((300, 200, 100, 40), False, 60, 400),
        "k_clamped": ((300, 200, 100, 500), True, 60, 400),       # |C| + |T| > max_patches: K = 0, R empty
        "no_chop": ((30, 20, 10, 8), True, 6, 400),               # |R0| <= K: R0 whole, in stage-0 order
    }[case]
    rows = rng.permutation(100000)[:sum(sizes)]
    lv, o = [], 0
    for s in sizes:
        lv.append(np.sort(rows[o:o + s])); o += s
    seed, cam = 0xC0FFEE, 2

    def perm_by(stage):
        def f(lst):
            k = shuffle_key(seed, stage, cam, lst)
            return [lst[i] for i in np.lexsort((np.asarray(lst), k))]
        return f
    C, T, R = select_sets(lv, seed, cam, try_coarse, coarse_max, max_patches)
    rC, rT, rR = _reference_sets(lv, perm_by(0), perm_by(1), try_coarse, coarse_max, max_patches)
    assert list(C) == rC and list(T) == rT and list(R) == rR
    if case == "k_clamped":
        assert len(R) == 0
    if case == "no_chop":
        assert len(R) == sizes[0] + sizes[1] + sizes[2] - max(0, min(coarse_max - sizes[3], sizes[2]))
    if case == "no_coarse":
        assert len(C) == 0 and len(T) == sizes[3]


def test_track_map_refuses_without_a_table():
    """A NULL table is an error with a message, not a crash."""
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import TrackMapParams, TrackMapResult, _bind_track_map, lib
    L = _bind_track_map(lib())
    prm, res = TrackMapParams(), TrackMapResult()
    assert L.mcp_track_map(None, 1, None, None, None, 0, None, None, None, None, ctypes.byref(prm), ctypes.byref(res)) == -1
    assert "NULL table" in chain_bundle.last_error()
    assert L.mcp_map_points_set_source(None, 0, 0, None, None, None, None, None) == -1
    assert L.mcp_map_points_get_states(None, 0, 0, 0, None) == -1
    n = ctypes.c_int(5)
    assert L.mcp_track_map_view(None, 0, ctypes.byref(n)) is None and n.value == 0


def test_cpp_track_map_mirror_compiles_and_links(tmp_path):
    """include/mcptam_hip/KeyFrame.hpp's MapPointTable TrackMap members, linked against libmcptam_hip.so (not run: no GPU)."""
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "track_map_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'static int use(int argc) {\n'
                   '  mcptam_hip::MapPointTable t(-1);\n'
                   '  mcptam_hip::KeyFrame kf(640, 480); std::vector<mcptam_hip::KeyFrame*> ks{&kf};\n'
                   '  std::vector<int> keys(argc), lv(argc), cxy(2*argc), ids(argc); std::vector<uint8_t> fx(argc); std::vector<mcptam_hip::KeyFrame*> src(argc, &kf);\n'
                   '  t.SetSource(0, keys, src, lv, cxy, fx); t.UpdateSource(ids, keys, src, lv, cxy, fx);\n'
                   '  std::vector<mcp_camera> cams(1); double bfw[12] = {0}; std::vector<double> cfb(12);\n'
                   '  mcp_track_map_params p; std::memset(&p, 0, sizeof p); mcp_track_map_result r;\n'
                   '  auto items = t.TrackMap(ks, {}, {}, false, cams, bfw, cfb, p, &r);\n'
                   '  auto st = t.States(0, 0, 1);\n'
                   '  return (int)items.size() + (int)st.size() + (int)(mcp_track_shuffle_key(1, 0, 0, argc) & 1);\n}\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) { std::printf("linked\\n"); return 0; }\n'
                   '  return use(argc);\n}\n')
    exe = tmp_path / "track_map_link"
    lib = os.path.join(ROOT, "mcptam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lmcptam_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linked" in out.stdout
