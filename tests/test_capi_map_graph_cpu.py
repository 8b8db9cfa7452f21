"""The map graph's C ABI without a device: every new symbol is exported and bound, and the struct sizes of mcptam_amd.map_graph are the
header's (compiled from include/mcp_img.h with the host compiler)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    txt = open(os.path.join(ROOT, "include", "mcp_img.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_every_new_symbol_is_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from mcptam_amd import chain_bundle, keyframe, map_graph
    declared = sorted(set(re.findall(r"\b(mcp_map_graph_[a-z0-9_]+|mcp_map_bundle_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 19 and set(declared) == set(map_graph.GRAPH_SYMBOLS)
    L = ctypes.CDLL(chain_bundle.LIB_PATH)
    for n in declared:
        assert hasattr(L, n), "libmcptam_hip.so does not export " + n
        assert n in keyframe.IMG_SYMBOLS
    B = map_graph.lib()
    for n in declared:
        assert getattr(B, n).argtypes is not None, n + " has no argument types"
    import mcptam_amd
    assert mcptam_amd.MapGraph is map_graph.MapGraph and mcptam_amd.bundle_select_ref is map_graph.bundle_select_ref


def test_constants_match_the_header():
    from mcptam_amd import map_graph
    h = _header()
    want = dict(MCP_MAP_MAX_MKFS=map_graph.MAX_MKFS, MCP_MKF_PRESENT=map_graph.MKF_PRESENT, MCP_MKF_FIXED=map_graph.MKF_FIXED, MCP_MKF_BAD=map_graph.MKF_BAD,
                MCP_GP_FIXED=map_graph.GP_FIXED, MCP_GP_BAD=map_graph.GP_BAD, MCP_BUNDLE_ALL=map_graph.BUNDLE_ALL, MCP_BUNDLE_RECENT=map_graph.BUNDLE_RECENT,
                MCP_MAX_FRAME_CAMS=map_graph.MAX_CAMS)
    for name, value in want.items():
        m = re.search(r"#define\s+%s\s+(\d+)" % name, h)
        assert m and int(m.group(1)) == value, name


def test_struct_sizes_match_the_header(tmp_path):
    from mcptam_amd import map_graph
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler to read include/mcp_img.h with")
    names = sorted(map_graph.STRUCT_SIZES)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "mcp_img.h"\nint main(void) {\n' +
                   "".join('  printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in names) +
                   '  printf("closest_dist %zu\\n", (size_t)&((mcp_bundle_select_result*)0)->closest_dist);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for n in names:
        assert int(out[n]) == map_graph.STRUCT_SIZES[n], (n, out[n], map_graph.STRUCT_SIZES[n])
    assert int(out["closest_dist"]) == map_graph.SelectResult.closest_dist.offset
