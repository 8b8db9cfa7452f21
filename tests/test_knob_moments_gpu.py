"""When the MCP_* switches are read (column "read at"; the readers are csrc/mcp_knobs.h), pinned on the `tiny` map
of mcptam_amd/synth.py through DebugStructure() and Timing(): a knob of the handle is taken when the handle is made, a knob of
Prepare() at the Prepare() that follows -- and one that is absent then keeps what an earlier Prepare() of the handle took --, the
test hook of the linearisation's launch at every call.  MCP_BA_SMALL_POINTS=0 throughout: the large-map layout (groups of 64
points, k_linearize_pipe / k_linearize_group), where the kernels the knobs choose between are the ones reported."""
import pytest

pytestmark = pytest.mark.gpu

_TINY = {}


def _tiny(rough=False):
    """The tiny map (2 cameras, 6 MKFs, 60 points), built once; `rough`: from a start far enough off that trials are rejected."""
    if rough not in _TINY:
        from mcptam_amd import synth
        _TINY[rough] = synth.make_config("tiny", pose_sigma=(0.2, 5.0), depth_sigma=0.2) if rough else synth.make_config("tiny")
    return _TINY[rough]


@pytest.fixture
def large_layout(gpu_required, monkeypatch):
    from mcptam_amd import chain_bundle
    for k in ("MCP_BA_LIN_PIPE", "MCP_BA_SCHUR4", "MCP_BA_ASM_PAIR", "MCP_BA_ASM_LONG", "MCP_BA_SPECULATE", "MCP_BA_TEST_REFUSE_LAUNCH", "MCP_BA_SMALL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCP_BA_SMALL_POINTS", "0")
    chain_bundle.struct_cache_clear()
    yield monkeypatch
    chain_bundle.struct_cache_clear()


def _handle(**kw):
    from mcptam_amd.chain_bundle import ChainBundle
    return ChainBundle(_tiny().cams, True, True, False, **kw)


def test_handle_knobs_are_taken_when_the_handle_is_made(large_layout):
    mp = large_layout
    g = _handle()
    mp.setenv("MCP_BA_LIN_PIPE", "0")
    mp.setenv("MCP_BA_SCHUR4", "0")
    _tiny().populate(g)
    st = g.DebugStructure()                     # (the handle's first Prepare())
    assert st["grp_pts"] == 64 and st["ngroup"] > 0 and st["nfl"] > 0, st
    assert (st["lin_kernel"], st["schur_kernel"]) == ("pipe", "schur4"), st
    g.close()
    g = _handle()
    _tiny().populate(g)
    st = g.DebugStructure()
    assert (st["lin_kernel"], st["schur_kernel"]) == ("group", "schur_group"), st
    g.close()


def test_prepare_knobs_are_taken_at_prepare(large_layout):
    mp = large_layout
    g = _handle()
    _tiny().populate(g)
    assert g.DebugStructure()["asm_kernel"] == "pair"          # (what the map takes when nothing is said)
    g.close()
    g = _handle()
    mp.setenv("MCP_BA_ASM_PAIR", "0")
    _tiny().populate(g)
    st = g.DebugStructure()
    assert st["asm_kernel"] == "tiles", st
    g.close()


def test_an_absent_prepare_knob_keeps_what_the_handle_took_before(large_layout):
    """MCP_BA_SPECULATE=0 at the handle's first Prepare(), absent at its second one (a measurement was added in between): the
    Compute() behind the second solves no system ahead -- every trial has a solve of its own, none is served by a speculative
    system -- on a run that does reject trials, and whose trials a handle that never saw the knob does serve from speculative
    systems."""
    mp = large_layout
    mp.setenv("MCP_BA_SMALL", "0")              # (the general launch sequence speculates in every solve)
    p = _tiny(rough=True)
    from mcptam_amd.chain_bundle import ChainBundle

    def run(knob_at_first_prepare):
        g = ChainBundle(p.cams, True, True, False, disable_convergence=True)
        ids = p.populate(g)
        if knob_at_first_prepare:
            mp.setenv("MCP_BA_SPECULATE", "0")
        g.Prepare()
        mp.delenv("MCP_BA_SPECULATE", raising=False)
        g.AddMeas([int(ids["mkf"][p.ms_mkf[0]]), int(ids["cam"][p.ms_cam[0]])], int(ids["point"][p.ms_pt[0]]), p.ms_uv[0], float(4.0 ** p.ms_level[0]), int(p.ms_cam[0]))
        assert g.Compute(12) == 12              # (the measurement added: Prepare() again, the knob absent)
        tm, logs = g.Timing(), g.IterLogs()
        g.close()
        print(knob_at_first_prepare, [l["trials"] for l in logs], {k: tm[k] for k in ("n_trials", "n_solves", "n_spec_hits")})
        assert sum(l["trials"] for l in logs) > len(logs), "the run must reject trials for this to mean anything"
        return tm

    tm = run(False)
    assert tm["n_spec_hits"] > 0 and tm["n_solves"] + tm["n_spec_hits"] == tm["n_trials"], tm
    tm = run(True)
    assert tm["n_spec_hits"] == 0 and tm["n_solves"] == tm["n_trials"], tm


def test_the_launch_test_hook_is_read_at_every_call(large_layout):
    """Set and read through DebugStructure() alone: no launch is made while it is set."""
    mp = large_layout
    g = _handle()
    _tiny().populate(g)
    assert g.DebugStructure()["lin_kernel"] == "pipe"
    mp.setenv("MCP_BA_TEST_REFUSE_LAUNCH", "1")
    assert g.DebugStructure()["lin_kernel"] == "group"
    mp.delenv("MCP_BA_TEST_REFUSE_LAUNCH")
    assert g.DebugStructure()["lin_kernel"] == "pipe"
    g.close()
