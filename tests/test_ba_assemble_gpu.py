"""k_assemble (csrc/ba_group.h: one wavefront per 6 x 6 pose block and system, walking a task table built at Prepare()) against
k_assemble_tiles (one workgroup per 32 x 32 tile, MCP_BA_ASM_PAIR=0) on the same map: the same additions in the same order for
every entry, so every comparison here is bit for bit -- the whole DebugSystems(BATCH_LAMBDAS) output (every entry of every tile of
the factorisation plan, rhs, J^T r) as 64-bit patterns.  No tolerance anywhere.

The knob is read at Prepare(), so each side is a handle of its own.  Every comparison takes the new kernel twice: on a handle that
adopts the structure the tiles handle left in the structure cache (the cached task table) and on a cold one."""
import numpy as np
import pytest

from ba_shapes import BATCH_LAMBDAS, DESIGNS, build, get_map, rolling_design, shared_design
from helpers import run_bundle

pytestmark = pytest.mark.gpu

LIST_SEAMS = (1, 7, 8, 9, 15, 16, 17, 33)      # staged blocks per pose pair against the 16-deep and the 4-deep rounds of the walk
_MAPS = {}


def _map(name):
    """`name` of ba_shapes, or one of the shapes only this file needs (built once)."""
    if name not in _MAPS:
        if name in DESIGNS or name.startswith("calib"):
            _MAPS[name] = get_map(name)
        elif name.startswith("shared"):            # "shared<k>": 66 points on k shared free poses; "shared6x<L>": 16 L points, L groups
            k, _, L = name[6:].partition("x")
            _MAPS[name] = build(shared_design(name, 16 * int(L) if L else 66, int(k)))
        else:
            k = int(name[4:])
            _MAPS[name] = build(rolling_design(name, 66, k, 66))
    return _MAPS[name]


def _handle(name):
    from mcptam_amd.chain_bundle import ChainBundle
    p = _map(name)
    g = ChainBundle(p.cams, True, True, False)
    p.populate(g)
    return g


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _assert_same_systems(got, ref, what):
    assert len(got) == len(ref)
    for q, (x, y) in enumerate(zip(got, ref)):
        for part, a, b in zip(("S", "rhs", "b"), x, y):
            if not _same_bits(a, b):
                bad = np.argwhere(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))
                raise AssertionError("%s: system %d, %s differs in %d entries, first at %s" % (what, q, part, len(bad), bad[0]))


def _systems(name, monkeypatch, pair, lams=BATCH_LAMBDAS):
    """(DebugSystems(lams), DebugStructure()) of a fresh handle on map `name` with MCP_BA_ASM_PAIR=0 (pair False) or unset."""
    if pair:
        monkeypatch.delenv("MCP_BA_ASM_PAIR", raising=False)
    else:
        monkeypatch.setenv("MCP_BA_ASM_PAIR", "0")
    g = _handle(name)
    st = g.DebugStructure()
    out = g.DebugSystems(lams)
    g.close()
    return out, st


def _compare(name, monkeypatch, expect_default="pair", expect_forced="tiles"):
    """tiles (cold) | default adopting the cached structure | default cold: identical bits.  Returns the default's structure."""
    from mcptam_amd import chain_bundle
    chain_bundle.struct_cache_clear()
    ref, st0 = _systems(name, monkeypatch, False)
    assert st0["asm_kernel"] == expect_forced, st0
    h0 = chain_bundle.struct_cache_stats()[0]
    hit, st1 = _systems(name, monkeypatch, True)
    assert chain_bundle.struct_cache_stats()[0] == h0 + 1          # (the task table came with the cached block)
    assert st1["asm_kernel"] == expect_default, st1
    _assert_same_systems(hit, ref, name + " (cached structure)")
    chain_bundle.struct_cache_clear()
    cold, st2 = _systems(name, monkeypatch, True)
    assert st2["asm_kernel"] == expect_default, st2
    _assert_same_systems(cold, ref, name + " (cold)")
    print(name, st2)
    return st2


@pytest.mark.parametrize("name,np_", [("shared1", 6), ("shared2", 12), ("shared6", 36), ("shared13_130", 78), ("roll5", 396), ("roll13", 396)])
def test_tile_seams(gpu_required, name, np_, monkeypatch):
    """Pose blocks against the 32-wide tiles: one tile with a single diagonal block and a right-hand-side task of fewer than ten
    poses (np = 6, 12); pose 5 across the first seam (36); seams at 32 and 64 with a partial last tile (78); 13 tile rows with
    plan tiles that hold pose blocks without a staged contribution, and fill-in tiles (396)."""
    st = _compare(name, monkeypatch)
    assert st["np"] == np_ and st["nbig"] == 0 and not st["asm_long"], st


@pytest.mark.parametrize("L", LIST_SEAMS)
def test_list_length_seams(gpu_required, L, monkeypatch):
    """All points share six free poses, L groups of 16 points: every pose pair's list has L staged blocks -- one short of, at and
    one beyond the 16-deep round, the same around the 4-deep rounds of the remainder, two 16-deep rounds and one."""
    st = _compare("shared6x%d" % L, monkeypatch)
    assert st["ngroup"] == L and st["grp_pts"] == 16 and st["np"] == 36 and not st["asm_long"], st


def test_zero_schur_blocks_under_nonzero_pose_blocks(gpu_required, monkeypatch):
    """calib17: poses co-observed only through fixed points -- staged U blocks whose Schur blocks are zero."""
    st = _compare("calib17", monkeypatch)
    assert st["nbig"] == 0 and not st["asm_long"], st


@pytest.mark.parametrize("name", ["shared13_130", "roll13"])
def test_each_system_of_a_batch_is_the_single_system(gpu_required, name, monkeypatch):
    """blockIdx.y = system: each of the four systems of a batch equals the one system a fresh handle builds for that lambda."""
    batch, st = _systems(name, monkeypatch, True)
    assert st["asm_kernel"] == "pair" and st["max_systems"] >= 4, st
    for q, lam in enumerate(BATCH_LAMBDAS):
        single, _ = _systems(name, monkeypatch, True, [lam])
        _assert_same_systems(single, [batch[q]], "%s lambda %g" % (name, lam))


def test_routing_of_the_other_kernels(gpu_required, monkeypatch):
    """Generic-path points (nbig > 0: Ubig is added entry by entry) keep k_assemble_tiles, long lists k_assemble_long, whatever
    MCP_BA_ASM_PAIR says; their systems do not depend on it."""
    st = _compare("big_mixed", monkeypatch, expect_default="tiles", expect_forced="tiles")
    assert st["nbig"] > 0, st
    monkeypatch.setenv("MCP_BA_ASM_LONG", "1")
    st = _compare("shared6", monkeypatch, expect_default="long", expect_forced="long")
    assert st["asm_long"], st


def test_compute_is_unchanged_cold_cached_and_after_the_outliers_are_erased(gpu_required, monkeypatch):
    """Compute(4) on a c2-shaped map: iteration logs, poses, points and outlier lists identical with k_assemble_tiles and with
    k_assemble -- on a cold Prepare(), on a structure-cache hit, and on the map minus the first call's outliers, which adopts the
    cached structure of the call before (near miss): the task table of the cache entry under erased measurements."""
    from collections import Counter
    from mcptam_amd import synth, chain_bundle
    from mcptam_amd.chain_bundle import ChainBundle
    p = synth.make_config("c2", n_mkf=12, n_points=1500)

    def three_runs(pair):
        if pair:
            monkeypatch.delenv("MCP_BA_ASM_PAIR", raising=False)
        else:
            monkeypatch.setenv("MCP_BA_ASM_PAIR", "0")
        chain_bundle.struct_cache_clear()
        runs, maps = [], [p, p]
        for i in range(3):
            if i == 2:
                first = runs[0]
                flagged = Counter(o[0] for o in first["outliers"])
                gone = [o for o in first["outliers"] if flagged[o[0]] < p.n_meas // p.n_points]      # (a map that lost a point is built cold)
                assert len(gone) > 0
                maps.append(synth.erase_measurements(p, gone, first["ids"]))
            hits, near = chain_bundle.struct_cache_stats()[0], chain_bundle.struct_cache_near_hits()
            g = ChainBundle(maps[i].cams, True, True, False, disable_convergence=True)
            r = run_bundle(g, maps[i], 4)
            assert g.DebugStructure()["asm_kernel"] == ("pair" if pair else "tiles")
            g.close()
            assert r["rc"] == 4
            assert chain_bundle.struct_cache_stats()[0] - hits == (1 if i == 1 else 0) and chain_bundle.struct_cache_near_hits() - near == (1 if i == 2 else 0)
            runs.append(r)
        return runs

    tiles, pairs = three_runs(False), three_runs(True)
    for what, a, b in zip(("cold", "cache hit", "near miss"), tiles, pairs):
        assert a["logs"] == b["logs"], what
        assert a["outliers"] == b["outliers"], what
        for k in ("R", "t", "X"):
            assert _same_bits(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64)), (what, k)
