"""The MCP_* environment switches have one home: mcptam_amd/csrc/mcp_knobs.h reads them (nothing else in csrc calls getenv), the
table of INTEGRATION.md section 7 lists exactly the names the header reads, one row each, with the moment the library reads it;
and every reader gives what the reads gave when they were written out at their sites (tests/cpp/knobs_check.cpp, under the
sanitizers)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mcptam_amd", "csrc")
READ_AT = ("process", "device (first use)", "handle", "Prepare", "every call")


def _header_names():
    return set(re.findall(r'"(MCP_[A-Z0-9_]+)"', open(os.path.join(CSRC, "mcp_knobs.h")).read()))


def _table_rows():
    """(names, read at, line) of every row of section 7's table that is about environment switches."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = text[text.index("## 7. Run-time knobs"):]
    rows = [l for l in sec.splitlines() if l.startswith("|")]
    head = [c.strip() for c in rows[0].strip("|").split("|")]
    assert head == ["knob", "read at", "effect"], head
    out = []
    for l in rows[2:]:
        cells = [c.strip() for c in l.strip("|").split("|")]
        assert len(cells) == 3, l
        if "-D" in cells[0] or "mcp_ba_params" in cells[0]:
            continue
        out.append((re.findall(r"MCP_[A-Z0-9_]+", cells[0]), cells[1], l))
    return out


def test_getenv_lives_in_the_knob_header_only():
    sources = [f for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".cpp", ".c", ".hpp")) or f == "Makefile"]
    assert len(sources) > 30
    found = sorted(f for f in sources if re.search(r"\bgetenv\b", open(os.path.join(CSRC, f)).read()))
    assert found == ["mcp_knobs.h"], found


def test_the_table_lists_what_the_header_reads():
    rows = _table_rows()
    listed = [n for names, _, _ in rows for n in names]
    assert len(listed) == len(set(listed)), sorted(n for n in set(listed) if listed.count(n) > 1)      # no name in two rows
    assert all(len(names) == 1 for names, _, _ in rows), [l for names, _, l in rows if len(names) != 1]      # one row per switch
    header = _header_names()
    assert len(header) >= 60
    assert set(listed) == header, (sorted(header - set(listed)), sorted(set(listed) - header))


def test_every_row_says_when_the_switch_is_read():
    for names, read_at, line in _table_rows():
        assert read_at in READ_AT, line


def test_readers_under_the_sanitizers(tmp_path):
    """tests/cpp/knobs_check.cpp has its own main; built from the header alone with the host compiler, AddressSanitizer and
    UndefinedBehaviorSanitizer (nothing sanitized is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "knobs_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]      # the runtimes inside the program: it needs nothing preloaded
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + static +
                          ["-I", CSRC, os.path.join(ROOT, "tests", "cpp", "knobs_check.cpp"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("MCP_")}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "knobs ok" in out.stdout
