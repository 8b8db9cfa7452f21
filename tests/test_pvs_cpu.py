"""CPU-side checks of the FindPVS boundary (include/mcp_img.h: mcp_map_points_*, mcp_track_find_pvs): the declarations exist and
are exported, and the ctypes layout of mcp_pvs_entry is the one the host compiler gives the header."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PVS_SYMBOLS = ["mcp_map_points_create", "mcp_map_points_destroy", "mcp_map_points_rows", "mcp_map_points_resize", "mcp_map_points_set", "mcp_map_points_update",
               "mcp_track_find_pvs", "mcp_track_find_pvs_view"]


def test_pvs_entry_points_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "mcp_img.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "typedef struct mcp_map_points mcp_map_points;" in txt
    assert re.search(r"typedef struct mcp_pvs_entry\s*\{", txt)
    for n in PVS_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, txt), n + " is not declared in include/mcp_img.h"
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    for n in PVS_SYMBOLS:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS


def test_pvs_entry_layout_matches_the_header(tmp_path):
    from mcptam_amd.pvs import PVS_ENTRY_DTYPE, PvsEntry
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d\\n", (int)sizeof(mcp_pvs_entry), (int)offsetof(mcp_pvs_entry, point),'
                   ' (int)offsetof(mcp_pvs_entry, level), (int)offsetof(mcp_pvs_entry, image), (int)offsetof(mcp_pvs_entry, cam_derivs),'
                   ' (int)offsetof(mcp_pvs_entry, warp_inverse)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(PvsEntry)] + [getattr(PvsEntry, f).offset for f in ("point", "level", "image", "cam_derivs", "warp_inverse")]
    assert got == want
    assert got[0] == PVS_ENTRY_DTYPE.itemsize
    assert [PVS_ENTRY_DTYPE.fields[f][1] for f in ("point", "level", "image", "cam_derivs", "warp_inverse")] == got[1:]


def test_pvs_refuses_without_a_table():
    """A NULL table is an error with a message, not a crash (no device is touched before the check)."""
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle
    from mcptam_amd.pvs import lib
    L = lib()
    counts = (ctypes.c_int * 4)()
    assert L.mcp_track_find_pvs(None, 1, None, None, None, None, None, None, counts) == -1
    assert "NULL table" in chain_bundle.last_error()
    assert L.mcp_map_points_rows(None) == -1
    assert L.mcp_map_points_set(None, 0, 0, None, None, None, None) == -1
    assert L.mcp_map_points_resize(None, 0) == -1
    n = ctypes.c_int(5)
    assert L.mcp_track_find_pvs_view(None, 0, 0, ctypes.byref(n)) is None and n.value == 0
    # the read-backs refuse before they size anything from `count`
    from mcptam_amd.pvs import _bind_track_map, _bind_track_record, _bind_write_back
    L = _bind_track_record(_bind_track_map(_bind_write_back(L)))
    for call in (lambda: L.mcp_map_points_get(None, 0, 0x7fffffff, None, None, None, None), lambda: L.mcp_map_points_get_counts(None, 0, 0x7fffffff, None, None),
                 lambda: L.mcp_map_points_get_states(None, 0, 0, 0x7fffffff, None)):
        assert call() == -1 and "NULL table" in chain_bundle.last_error()


def test_cpp_map_point_table_compiles_and_links(tmp_path):
    """include/mcptam_hip/KeyFrame.hpp's MapPointTable: every member instantiated, linked against libmcptam_hip.so (not run: no GPU)."""
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "pvs_link.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "mcptam_hip/KeyFrame.hpp"\n'
                   'static int use(int argc) {\n'
                   '  mcptam_hip::MapPointTable t(-1);\n'
                   '  std::vector<double> p(3*argc), r(3*argc), d(3*argc); std::vector<uint8_t> u(argc, 1); std::vector<int> ids(argc);\n'
                   '  t.Set(0, p, r, d, u); t.Update(ids, p, r, d, u); t.Resize(argc);\n'
                   '  mcptam_hip::KeyFrame kf(640, 480); std::vector<mcptam_hip::KeyFrame*> ks{&kf}; std::vector<mcp_camera> cams(1);\n'
                   '  double bfw[12] = {0}; std::vector<double> cfb(12);\n'
                   '  auto pvs = t.FindPVS(ks, cams, bfw, cfb);\n'
                   '  return (int)pvs.size() + t.Rows() + (t.Handle() != nullptr);\n}\n'
                   'int main(int argc, char** argv) {\n'
                   '  if (argc > 1 && std::strcmp(argv[1], "--link-only") == 0) { std::printf("linked\\n"); return 0; }\n'
                   '  return use(argc);\n}\n')
    exe = tmp_path / "pvs_link"
    lib = os.path.join(ROOT, "mcptam_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", lib, "-lmcptam_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    out = subprocess.run([str(exe), "--link-only"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "linked" in out.stdout
