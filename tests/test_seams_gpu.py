"""The selection and compaction kernels at their size seams: counts of 63 / 64 / 65, 255 / 256 / 257, 511 / 512 / 513, tiles and wavefronts
that are wholly empty or wholly full, more than 256 tiles (the second trip of the "tiles before mine" sums), the register / plain switch of
the pose iterations at 1023 / 1024 / 1025 records, crafted keys for tm_emit, and k_stereo_commit across its chunks of 256 candidates.

Every case compares the HIP path with a reference that does not run the code under test -- the CPU oracle, the numpy restatements, the
per-point search or the compositions the per-feature test files pin -- and first asserts, on the reference alone, that it hits the seam it is
named for."""
import os
import subprocess

import numpy as np
import pytest

import test_pvs_gpu as tp
import test_refind_gpu as trf
import test_stereo_points_gpu as tsp
import test_track_map_gpu as tm
import test_track_record_gpu as tr
from refind_fixture import compose as refind_compose
from refind_fixture import moved, same_state, sequences_of
from test_pvs_gpu import world as pvs_world            # noqa: F401  (module-scoped fixtures of the per-feature files, under their own names)
from test_refind_gpu import world as refind_world      # noqa: F401
from test_stereo_points_gpu import stereo as stereo_world   # noqa: F401
from test_track_map_gpu import world as tm_world       # noqa: F401

pytestmark = pytest.mark.gpu

LEVELS = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. tm_emit alone --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tm_select_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tm_select") / "tm_select_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I", os.path.join(ROOT, "mcptam_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "tm_select_check.hip"), "-o", exe])
    return exe


@pytest.mark.timeout(60)
def test_tm_emit_unit_against_sort(gpu_required, tm_select_check):
    """tm_emit (csrc/track_map_kernels.h) alone, in a 1024-thread kernel of its own (tests/cpp/tm_select_check.hip), against std::sort on
    (key, index): uniform keys, keys sharing their top 8 .. 56 bits, keys that differ in the top byte only, 0 and ~0 as real keys; the
    crafted digit with exactly the needed keys in its bucket and with one more, at every depth; every third entry dead, [a, b) away from 0,
    has_lo on a present key, the excl window with thr2 on a present key, other keys to select on than to exclude on; k = 1, 2, 63, 64, 65,
    1023 .. 1025, 2047 .. 2049, 4095 .. 4097, count - 1, count.  out[0..k), the returned key and 64 untouched words after out[k).
    3954 launches in 0.74 s on the MI355X (the subprocess gets 10 s); the compile took 3.8 s there and 12 s on a slower host, which with
    3x headroom on top gives the test's 60 s."""
    out = subprocess.run([tm_select_check], capture_output=True, text=True, timeout=10)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    print(last)
    assert out.returncode == 0 and last.startswith("ok "), out.stdout[-3000:] + out.stderr[-500:]
    assert last == "ok 3954", last                    # (fixed seed: a population that is dropped shows in the count)


# ---- 2. PVS ------------------------------------------------------------------------------------------------------------------------------
PVS_SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513]


def _pvs_patterns(n):
    r = np.arange(n)
    return {"all": np.ones(n, dtype=bool), "none": np.zeros(n, dtype=bool), "row_0": r == 0, "last_row": r == n - 1, "multiples_of_256": r % 256 == 0,
            "lane_63": r % 64 == 63, "lane_0": r % 64 == 0, "every_other": r % 2 == 0}


@pytest.fixture(scope="module")
def pvs_base(gpu_required, pvs_world):
    """513 rows the oracle accepts on camera 0, levels 0, 1, 2, 3 in turn, and the oracle's search of them on the four cameras."""
    from mcptam_amd import synth_img
    from oracle import oracle_track_search
    w = pvs_world
    wp, pr, pd, _ = synth_img.make_map_cloud(w["pts"], 1500, seed=23, spread=1.0)
    cloud = [dict(w["pts"][0], world_pos=wp[i], pixel_right_w=pr[i], pixel_down_w=pd[i]) for i in range(len(wp))]
    oo = oracle_track_search(w["oB"], w["cam"], w["bfw"], w["cfbs"][0], cloud, 2, 0)
    ok = (oo["in_image"] == 1) & (oo["search_level"] >= 0)
    by_level = [np.nonzero(ok & (oo["search_level"] == l))[0] for l in range(LEVELS)]
    assert all(len(x) > 0 for x in by_level), [len(x) for x in by_level]
    rows = np.array([by_level[i % LEVELS][(i // LEVELS) % len(by_level[i % LEVELS])] for i in range(513)])
    pts = [cloud[r] for r in rows]
    outs = [oracle_track_search(w["oB"], w["cam"], w["bfw"], w["cfbs"][c], pts, 2, 0) for c in range(4)]
    return dict(wp=wp[rows], pr=pr[rows], pd=pd[rows], outs=outs)


@pytest.mark.parametrize("n", PVS_SIZES)
def test_pvs_small_tables_on_the_tile_and_wavefront_seams(gpu_required, pvs_world, pvs_base, n):
    """k_pvs_mark / k_pvs_scatter with n rows on 63 .. 65, 255 .. 257, 511 .. 513 under eight acceptance patterns (all, none, row 0, the last
    row, multiples of 256, lane 63, lane 0, every other row) over rows the oracle accepts on camera 0: membership, order, level and counts
    exactly, the geometry to test_pvs_matches_oracle's tolerance, against oracle_track_search."""
    w, b = pvs_world, pvs_base
    outs = [o[:n] for o in b["outs"]]
    acc = [(o["in_image"] == 1) & (o["search_level"] >= 0) for o in outs]
    assert acc[0].all(), "the oracle accepts every row of the base on camera 0"
    if n >= 64:
        assert set(outs[0]["search_level"].tolist()) == {0, 1, 2, 3}
    if n in (257, 513):
        assert int(acc[0][256 * ((n - 1) // 256):].sum()) == 1, "the last tile holds one accepted row"
    args = ([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    for name, usable in _pvs_patterns(n).items():
        want = [[np.nonzero(usable & acc[c] & (outs[c]["search_level"] == l))[0] for l in range(LEVELS)] for c in range(4)]
        if name == "none":
            assert all(len(x) == 0 for cam in want for x in cam)
        if name == "all":
            assert [len(x) for x in want[0]] == [int((outs[0]["search_level"] == l).sum()) for l in range(LEVELS)]
        t = tp._table(b["wp"][:n], b["pr"][:n], b["pd"][:n], usable.astype(np.uint8))
        pvs = t.find_pvs(*args)
        for c in range(4):
            for l in range(LEVELS):
                e = pvs[c][l]
                assert np.array_equal(e["point"], want[c][l]), (name, c, l)
                assert (e["level"] == l).all()
                for f in tp.FIELDS:
                    assert np.allclose(e[f], outs[c][f][want[c][l]], rtol=1e-11, atol=1e-12), (name, c, l, f)
        assert np.array_equal(t.counts, [[len(pvs[c][l]) for l in range(LEVELS)] for c in range(4)]), name
        assert np.array_equal(t.counts, [[len(x) for x in cam] for cam in want]), name


@pytest.mark.timeout(30)
def test_pvs_66000_rows_sum_the_tiles_before_in_two_trips(gpu_required, pvs_world):
    """258 tiles: k_pvs_scatter's loop over the tiles before its own takes a second trip for tiles 256 and 257.  Sparse usable rows (whole
    tiles empty), to the bit against the library's per-point search.  0.05 s on the MI355X, 0.9 s with the world's set-up when run alone:
    with 3x headroom under 4 s; the timeout leaves room for a loaded host."""
    from mcptam_amd import synth_img
    w = pvs_world
    n = 66000
    wp, pr, pd, us = synth_img.make_map_cloud(w["pts"], n, seed=29, spread=1.0)
    row = np.arange(n)
    usable = ((us != 0) & (np.isin(row // 256, [0, 1, 7, 128, 255, 256, 257]) | (row % 1024 == 5))).astype(np.uint8)
    outs = tp._search_all(w, [w["gB"]] * 4, wp, pr, pd)
    keep = [(usable != 0) & (o["in_image"] == 1) & (o["search_level"] >= 0) for o in outs]
    regions = (slice(0, 256), slice(65536, 65792), slice(65792, n))
    cams_ok = [c for c in range(4) if all(keep[c][r].any() for r in regions)]
    assert len(cams_ok) >= 2, cams_ok
    for r in regions:
        assert len(set(np.concatenate([outs[c]["search_level"][r][keep[c][r]] for c in cams_ok]).tolist())) >= 2
    tiles_hit = np.unique(row[keep[cams_ok[0]]] // 256)
    assert len(tiles_hit) < 258 - 100, "whole tiles are empty"
    t = tp._table(wp, pr, pd, usable)
    pvs = t.find_pvs([w["gB"]] * 4, [w["cam"]] * 4, w["bfw"], w["cfbs"])
    for c in range(4):
        tp._assert_pvs_is_search(pvs[c], outs[c], usable)
    assert np.array_equal(t.counts, [[int((keep[c] & (outs[c]["search_level"] == l)).sum()) for l in range(LEVELS)] for c in range(4)])


# ---- 3. ReFind ---------------------------------------------------------------------------------------------------------------------------
FOUND, OUTSIDE = 1, 2


def _rf_targets(w):
    """B, B moved a little, and the two turned by pi (everything OUTSIDE)."""
    pB = w["sc"]["poseB"]
    near = moved(pB, (0.0003, -0.0002, 0.001), (0.003, -0.001, 0.002))
    return [(w["B"], w["cam"], pB), (w["B"], w["cam"], near), (w["B"], w["cam"], moved(pB, (0.0, np.pi, 0.0), (0, 0, 0))),
            (w["B"], w["cam"], moved(near, (0.0, np.pi, 0.0), (0, 0, 0)))]


@pytest.fixture(scope="module")
def refind_pass(refind_world):
    """The first reference pass over the whole map: every row against B and moved B, one finder per pair and one per row; the pools the pair
    lists are drawn from; a finder that has found something."""
    w = refind_world
    T = _rf_targets(w)
    n = w["n"]
    pairs = np.stack([np.repeat(np.arange(n), 2), np.tile([0, 1], n)], axis=1).astype(np.int32)
    va = refind_compose(w["cols"], w["A"], T, pairs, False, None)[0].reshape(n, 2)
    vb = refind_compose(w["cols"], w["A"], T, pairs, True, None)[0].reshape(n, 2)
    found = np.nonzero((va == FOUND).all(axis=1) & (vb == FOUND).all(axis=1))[0]
    outside = np.nonzero((va == OUTSIDE).all(axis=1) & (vb == OUTSIDE).all(axis=1))[0]
    other = np.nonzero((va > OUTSIDE).all(axis=1) & (vb > OUTSIDE).all(axis=1) & (va < 5).all(axis=1))[0]      # searched, not found
    assert len(found) >= 300 and len(outside) >= 600 and len(other) >= 300, (len(found), len(outside), len(other))
    carried = refind_compose(w["cols"], w["A"], T, np.array([[found[0], 0]], dtype=np.int32), False, None)[3]
    assert carried[0]["valid"] == 1
    return dict(T=T, found=found, outside=outside, other=other, carried=carried, table=trf._table(w))


def _rf_run(w, P, pairs, per_row, layout):
    """One list, one mode: the layout on the composition alone, then mcp_map_refind bit for bit against it with a carried finder; up to 257
    pairs also against the oracle with a fresh one."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32)
    ref = refind_compose(w["cols"], w["A"], P["T"], pairs, per_row, trf._finder(P["carried"]))
    layout(ref)
    got = P["table"].refind(P["T"], pairs, per_row, trf._finder(P["carried"]))
    trf._assert_equal(got, ref)
    if len(pairs) <= 257:
        fresh = P["table"].refind(P["T"], pairs, per_row, trf._finder())
        trf._assert_oracle(fresh, trf._oracle(w, P["T"], pairs, per_row, trf._finder()))
    return got, ref


def _two(rows):
    """(r, 0), (r, 1) for every row: sequences of two in per-row mode."""
    return np.stack([np.repeat(rows, 2), np.tile([0, 1], len(rows))], axis=1)


@pytest.mark.parametrize("per_row", [False, True])
def test_refind_nothing_survives_the_mark(refind_world, refind_pass, per_row):
    """(a) 257 pairs, all OUTSIDE: no survivor in any tile.  Distinct rows: the last sequence is not the first, the finder comes back zero.
    One row 257 times: one sequence in per-row mode, the finder comes back as it went in."""
    w, P = refind_world, refind_pass
    zero = lambda f: not f.tobytes().strip(b"\0")

    def all_outside_zero(ref):
        assert (ref[0] == OUTSIDE).all() and len(ref[1]) == 0 and zero(ref[3])
    got, _ = _rf_run(w, P, np.stack([P["outside"][:257], np.zeros(257, dtype=np.int64)], axis=1), per_row, all_outside_zero)
    assert zero(got[3])
    one_row = np.stack([np.full(257, P["outside"][3]), np.arange(257) % 2], axis=1)

    def one_sequence(ref):
        assert (ref[0] == OUTSIDE).all() and len(sequences_of(one_row, per_row)) == (1 if per_row else 257)
        assert same_state(ref[3], P["carried"]) if per_row else zero(ref[3])
    got, _ = _rf_run(w, P, one_row, per_row, one_sequence)
    assert same_state(got[3], P["carried"]) if per_row else zero(got[3])


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_refind_only_the_last_pair_survives(refind_world, refind_pass, n, per_row):
    """(b) n - 1 OUTSIDE pairs, then one FOUND: the only survivor sits in the last lane of the list."""
    w, P = refind_world, refind_pass
    pairs = np.stack([np.concatenate([P["outside"][:n - 1], P["found"][5:6]]), np.zeros(n, dtype=np.int64)], axis=1)

    def layout(ref):
        assert (ref[0][:n - 1] == OUTSIDE).all() and ref[0][n - 1] == FOUND and list(ref[1]["pair"]) == [n - 1]
    _rf_run(w, P, pairs, per_row, layout)


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("n", [257, 513])
def test_refind_found_pairs_only_in_the_second_block(refind_world, refind_pass, n, per_row):
    """(c) pairs 0 .. 255: OUTSIDE and searched-but-not-found; the FOUND ones from pair 256 on."""
    w, P = refind_world, refind_pass
    head = np.where(np.arange(256) % 3 == 0, P["other"][:256], P["outside"][:256])
    tail = np.where(np.arange(n - 256) % 2 == 0, P["found"][:n - 256], P["outside"][300:300 + n - 256])
    pairs = np.stack([np.concatenate([head, tail]), np.zeros(n, dtype=np.int64)], axis=1)

    def layout(ref):
        v = ref[0]
        assert not (v[:256] == FOUND).any() and (v[:256] != OUTSIDE).any() and (v[:256] == OUTSIDE).any()
        assert v[256] == FOUND and int((v[256:] == FOUND).sum()) == (n - 256 + 1) // 2
    _rf_run(w, P, pairs, per_row, layout)


@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("n", [257, 513])
def test_refind_a_sequence_straddles_the_block_boundary(refind_world, refind_pass, n, per_row):
    """(d) a row's sequence starts at pair 250; its pairs in the first block all fail the mark; its first survivor is pair 256."""
    w, P = refind_world, refind_pass
    R = P["found"][7]
    filler = np.concatenate([P["found"][10:70], P["other"][:65]])
    mid = [[R, 2], [R, 3], [R, 2], [R, 3], [R, 2], [R, 3], [R, 0], [R, 1]]
    pairs = np.concatenate([_two(filler), mid, _two(P["found"][70:200])])[:n]

    def layout(ref):
        v = ref[0]
        heads = sequences_of(pairs, True)
        assert 250 in heads and not np.isin(np.arange(251, min(n, 258)), heads).any()
        assert (v[250:256] == OUTSIDE).all() and v[256] == FOUND and (v[:250] != OUTSIDE).all()
        if n > 257:
            assert v[257] == FOUND
    _rf_run(w, P, pairs, per_row, layout)


@pytest.mark.parametrize("per_row", [False, True])
def test_refind_a_sequence_head_in_lane_63(refind_world, refind_pass, per_row):
    """(e) 257 pairs; a sequence whose head is pair 63 (fails the mark), its survivors pairs 64 and 65; the sequence before it has its
    survivors in lanes 61 and 62."""
    w, P = refind_world, refind_pass
    Q, R = P["found"][8], P["found"][9]
    mid = [[Q, 2], [Q, 0], [Q, 1], [R, 2], [R, 0], [R, 1]]
    pairs = np.concatenate([_two(P["found"][20:50]), mid, _two(P["found"][50:146])])[:257]
    assert len(pairs) == 257

    def layout(ref):
        v = ref[0]
        heads = sequences_of(pairs, True)
        assert 60 in heads and 63 in heads and not np.isin([61, 62, 64, 65], heads).any()
        assert v[60] == OUTSIDE and v[61] == FOUND and v[62] == FOUND and v[63] == OUTSIDE and v[64] == FOUND and v[65] == FOUND
    _rf_run(w, P, pairs, per_row, layout)


@pytest.mark.parametrize("per_row", [False, True])
def test_refind_every_pair_found(refind_world, refind_pass, per_row):
    """(f) 256 pairs, every one FOUND: one full tile, every wavefront full."""
    w, P = refind_world, refind_pass
    pairs = _two(P["found"][100:228])

    def layout(ref):
        assert (ref[0] == FOUND).all() and np.array_equal(ref[1]["pair"], np.arange(256))
    _rf_run(w, P, pairs, per_row, layout)


@pytest.mark.timeout(30)
def test_refind_66000_pairs_take_the_second_trips(refind_world, refind_pass):
    """The 6000 rows against 11 moved views, one finder per pair: 258 tiles (the sums of k_rf_scatter and k_rf_commit over the tiles before
    take a second trip) and 66 000 sequences (k_rf_walk's grid of 65 536 strides once).  Bit for bit against the composition.  0.41 s on
    the MI355X, 0.9 s with the world's set-up when run alone: with 3x headroom under 4 s; the timeout leaves room for a loaded host."""
    w, P = refind_world, refind_pass
    rng = np.random.default_rng(33)
    targets = [(w["B"], w["cam"], moved(w["sc"]["poseB"], rng.normal(size=3) * 0.004, rng.normal(size=3) * 0.01)) for _ in range(11)]
    n = w["n"]
    rows = np.concatenate([np.arange(n)] + [np.arange(n)[::-1]] * 10)                  # (the findable rows 0 .. 935 open and close the list)
    pairs = np.stack([rows, np.repeat(np.arange(11), n)], axis=1).astype(np.int32)
    assert len(pairs) == 66000
    ref = refind_compose(w["cols"], w["A"], targets, pairs, False, trf._finder())
    assert (ref[0][65536:] == FOUND).any() and (ref[0][:256] == FOUND).any()
    got = P["table"].refind(targets, pairs, False, trf._finder())
    trf._assert_equal(got, ref)


# ---- 4. TrackMap and its record ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tm_cloud(gpu_required, tm_world):
    """The scene's own 936 points and 3000 copies moved by up to half a metre; of the rows any camera sees at level 3, forty stay usable (T is
    never chopped: the budget can only be met exactly when T is short)."""
    from mcptam_amd import synth_img
    w = tm_world
    c0 = w["cols"]
    nb = w["n"]
    base = [dict(world_pos=c0["wp"][r], pixel_right_w=c0["pr"][r], pixel_down_w=c0["pd"][r]) for r in range(nb)]
    wp, pr, pd, us = synth_img.make_map_cloud(base, 3000, seed=6, spread=0.5)
    n = nb + len(wp)
    like = np.arange(n) % nb
    rng = np.random.default_rng(15)
    cols = dict(wp=np.concatenate([c0["wp"], wp]), pr=np.concatenate([c0["pr"], pr]), pd=np.concatenate([c0["pd"], pd]),
                usable=np.concatenate([c0["usable"], us]), keys=np.arange(n, dtype=np.int32) * 3 + 7, src=[w["src"]] * n,
                level=c0["level"][like], center=np.ascontiguousarray(c0["center"][like]), fixed=np.zeros(n, dtype=np.uint8),
                inl=rng.integers(1, 31, n).astype(np.int32), outl=rng.integers(0, 31, n).astype(np.int32))
    cfbs = [w["cfbs"][0], w["cfbs"][1], w["cfbs"][3]]
    pvs = tm._table(cols).find_pvs(w["targets"][:3], [w["cam"]] * 3, w["prior"], cfbs)
    top = np.unique(np.concatenate([pvs[c][3]["point"] for c in range(3)]))
    cols["usable"] = cols["usable"].copy()
    cols["usable"][top[40:]] = 0
    return dict(cols=cols, n=n, cfbs=cfbs)


def _as_items(d):
    from mcptam_amd.pvs import TRACK_MAP_ITEM_DTYPE
    a = np.zeros(len(d["point"]), dtype=TRACK_MAP_ITEM_DTYPE)
    a["point"], a["stage"], a["weight_last"], a["out"] = d["point"], d["stage"], d["weight_last"], d["out"]
    return a


def _tm_case(w, cl, targets, cfbs, prm, layout):
    """layout(composition, restatement): the case's seam, asserted on the references alone.  Then mcp_track_map against the composition,
    mcp_track_map_record on a twin table against the restatement of the composition's items, the scene depth against mcp_scene_depth_robust
    on the restated lists: all exact.  Returns (track_map's result, the composition, the restatement)."""
    from mcptam_amd.pvs import track_record_restate
    cols, n, ncam = cl["cols"], cl["n"], len(targets)
    t, twin, B = tm._table(cols), tm._table(cols), tr._table(cols)
    ref = tm.compose(twin, cols, np.ones(n, dtype=bool), targets, w["cam"], w["prior"], cfbs, prm, tm._new_states(ncam, n))
    rs = track_record_restate([_as_items(d) for d in ref["items"]], (cols["inl"], cols["outl"]), False, ncam)
    layout(ref, rs)
    got = tm._run(t, targets, w["cam"], w["prior"], cfbs, prm)
    tm._assert_same(got, ref, ncam)
    b = B.track_map_record(targets, [w["cam"]] * ncam, w["prior"], cfbs, **tr.QUALITY, **prm)
    assert np.array_equal(b[1][0], ref["pose"][0]) and np.array_equal(b[1][1], ref["pose"][1])
    tr._assert_record_is_restatement(b[5], b[3], b[4], B.get_counts(), rs, ncam)
    cfw = np.array([list(b[5].cam_from_world[c]) for c in range(ncam)])
    depth, _ = twin.scene_depth(cfw, rs["seg_start"], rs["seg_rows"], rs["seg_w"])
    assert tr._depth_array(b[5])[:ncam].tobytes() == depth.tobytes()
    return got, ref, rs


@pytest.mark.parametrize("max_patches", [63, 64, 65, 255, 256, 257, 512, 1023, 1024, 1025])
def test_track_map_one_camera_with_the_budget_on_a_seam(gpu_required, tm_world, tm_cloud, max_patches, monkeypatch):
    """One camera, no coarse stage, n_fine = max_patches exactly: the chop's k, the item count of k_tr_mark / k_tr_scatter and the record
    count of the pose iterations on 63 .. 65, 255 .. 257, 512 and 1023 .. 1025.  At 1024 the device picks the register-held iterations, at
    1025 the plain ones: both also against the oracle's iterations on the composition's records, to test_pose_refine_matches_oracle's 1e-10."""
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    from mcptam_amd import keyframe as K
    from oracle import oracle_track_pose_refine
    w, cl = tm_world, tm_cloud
    prm = tm._params(try_coarse=0, max_patches=max_patches)

    def layout(ref, rs):
        assert sum(ref["counts"][0]) - ref["stale"][0] > 1100 and ref["counts"][0][3] <= 40
        assert sum(ref["sizes"][0]) == max_patches and ref["sizes"][0][0] == 0 and rs["n_items"] == [max_patches]
        assert rs["n_meas"][0] > 0
    got, ref, rs = _tm_case(w, cl, w["targets"][:1], cl["cfbs"][:1], prm, layout)
    if max_patches >= 1024:
        it = ref["items"][0]
        recs = K.pose_points(cl["cols"]["wp"][it["point"]], it["out"], 0)
        cfb = np.ascontiguousarray(np.stack([K._pose12(*c) for c in cl["cfbs"][:1]]))
        po, mo, _, _ = oracle_track_pose_refine(recs, [w["cam"]], cfb, w["prior"])
        assert np.allclose(got[1][0], po[0], rtol=0, atol=1e-10) and np.allclose(got[1][1], po[1], rtol=0, atol=1e-10)
        assert np.allclose(np.array(got[2].mu_last), mo, rtol=0, atol=1e-10)


def test_track_map_camera_boundaries_on_and_inside_the_tiles(gpu_required, tm_world, tm_cloud, monkeypatch):
    """Two cameras of 128 items each (the boundary on lane 0 of a wavefront, the list one full tile) and three of 100 (boundaries inside
    wavefronts and tiles)."""
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    w, cl = tm_world, tm_cloud
    for ncam, mp in ((2, 128), (3, 100)):
        def layout(ref, rs):
            assert [sum(s_) for s_ in ref["sizes"]] == [mp] * ncam and rs["n_items"] == [mp] * ncam
            assert rs["n_meas"][0] > 0 and sum(rs["n_meas"]) > rs["n_meas"][0], "measurements on both sides of a camera boundary"
        _tm_case(w, cl, w["targets"][:ncam], cl["cfbs"][:ncam], tm._params(try_coarse=0, max_patches=mp), layout)


def test_track_map_a_blind_camera_in_front(gpu_required, tm_world, tm_cloud, monkeypatch):
    """Camera 0 looks at a constant image: its 256 items, one whole tile, hold nothing found; camera 1's measurements start at 0."""
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    from mcptam_amd.keyframe import KeyFrame
    w, cl = tm_world, tm_cloud
    blind = KeyFrame(640, 480)
    blind.MakeKeyFrame_Lite(np.full((480, 640), 128, dtype=np.uint8))
    # (camera 1 is the one whose view the image was rendered for: it finds its points)

    def layout(ref, rs):
        assert rs["n_items"] == [256, 256] and rs["n_meas"][0] == 0 and rs["n_meas"][1] > 0
        assert list(rs["seg_start"]) == [0, 0, rs["n_meas"][1]]
    _tm_case(w, cl, [blind, w["targets"][0]], [cl["cfbs"][1], cl["cfbs"][0]], tm._params(try_coarse=0, max_patches=256), layout)


def test_track_map_the_chop_excludes_the_coarse_part_of_level_two(gpu_required, tm_world, tm_cloud, monkeypatch):
    """With the coarse stage: coarse_max = |S_3| + 20, so C takes all of level 3 and twenty of level 2, and the chop selects on stage-1 keys
    while it excludes, inside the level-2 window, on stage-0 keys."""
    monkeypatch.setenv("MCP_TRACK_REFINE_MULTI", "0")
    w, cl = tm_world, tm_cloud
    # a first pass of the composition, without the coarse stage: the live level counts coarse_max is chosen from
    first = tm.compose(tm._table(cl["cols"]), cl["cols"], np.ones(cl["n"], dtype=bool), w["targets"][:1], w["cam"], w["prior"], cl["cfbs"][:1],
                       tm._params(try_coarse=0, max_patches=300), tm._new_states(1, cl["n"]))
    assert first["stale"][0] == 0
    n3, n2 = int(first["counts"][0][3]), int(first["counts"][0][2])
    assert 0 < n3 <= 40 and n2 > 40
    cmax = n3 + 20

    def layout(ref, rs):
        assert ref["stale"][0] == 0 and list(ref["counts"][0]) == list(first["counts"][0])
        k3 = min(int(ref["counts"][0][3]), cmax)
        assert k3 < cmax and ref["sizes"][0][0] - k3 == 20, "twenty of C come from level 2"
        assert ref["sizes"][0] == [cmax, 0, 300 - cmax] and sum(ref["counts"][0]) - cmax > 300 - cmax, "the chop runs"
    _tm_case(w, cl, w["targets"][:1], cl["cfbs"][:1], tm._params(try_coarse=1, coarse_max=cmax, max_patches=300), layout)


# ---- 5. the stereo commit -------------------------------------------------------------------------------------------------------------------
STEREO_LEVEL = 1


def _stereo_outcomes(sc, cand, targets, limit, meas_root=(), meas_level=()):
    """The outcome of every (target, candidate) restated: numpy thinning, the composition's verdict of every surviving candidate
    (stereo.compose_target) and the reference's nLimit loop (:486-493) -- a candidate is tried, then the loop leaves once numSuccess >= limit."""
    from mcptam_amd import keyframe as K, stereo as S
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    alive = S.thin_candidates(cand, STEREO_LEVEL, meas_root, meas_level)
    oc = np.zeros((len(targets), len(cand)), dtype=np.uint8)
    num, new = 0, []
    for j, t in enumerate(targets):
        if new:
            alive &= S.thin_candidates(cand, STEREO_LEVEL, created_root=new)
        new = []
        oc[j][~alive] = S.THINNED
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            continue
        hyp, off = S.stereo_hypotheses(sc["src"], sc["cam"], sc["pose_src"], STEREO_LEVEL, cand[idx], t)
        res = S.compose_target(K.patch_sequences, t[0], t[1], t[2], hyp, off, list(range(len(idx))), sc["src"])
        oc[j][idx] = S.PAST_LIMIT
        for q, i in enumerate(idx):
            oc[j][i] = res[q][0]
            if res[q][0] == S.CREATED:
                num += 1
                new.append(S.level_zero_pos(cand[i], STEREO_LEVEL))
            if num >= limit:
                break
    return oc


def _stereo_check(sc, cand, js, limit, layout, meas=None, roots=(), lv=()):
    """layout(restated outcomes, the composition's points): the case's seam, asserted on the references alone.  Then mcp_stereo_points against
    the composition (created points in order, keep), the restated outcomes, and the oracle's created set."""
    from mcptam_amd import keyframe as K, stereo as S
    from oracle import oracle_patch_sequences
    tg = tsp._targets(sc, js)
    oc_ref = _stereo_outcomes(sc, cand, tg, limit, roots, lv)
    made, keep_ref = S.compose(K.patch_sequences, sc["src"], sc["cam"], sc["pose_src"], STEREO_LEVEL, cand, tg, limit=limit, meas_root=roots, meas_level=lv)
    assert [(m["target"], m["candidate"]) for m in made] == [(j, int(i)) for j in range(len(js)) for i in np.nonzero(oc_ref[j] == S.CREATED)[0]]
    layout(oc_ref, made)
    got, keep, oc = S.stereo_points(sc["src"], sc["cam"], sc["pose_src"], STEREO_LEVEL, cand, tg, limit=limit, meas=meas)
    tsp._compare(got, keep, made, keep_ref)
    assert np.array_equal(oc, oc_ref), [np.nonzero(oc[j] != oc_ref[j])[0][:10] for j in range(len(js))]
    omade, _ = S.compose(oracle_patch_sequences, sc["src"], sc["cam"], sc["pose_src"], STEREO_LEVEL, cand, tg, limit=limit, meas_root=roots, meas_level=lv,
                         src_oracle=sc["osrc"], search_kfs=[sc["otg"][j] for j in js])
    assert [(m["target"], m["candidate"]) for m in omade] == list(zip(got["target"].tolist(), got["candidate"].tolist()))
    assert np.allclose(np.array([m["target_pos"] for m in omade]).reshape(-1, 2), got["target_pos"], rtol=0, atol=1e-9)


@pytest.fixture(scope="module")
def stereo_pass(gpu_required, stereo_world):
    """The first reference pass: the verdict of every level-1 candidate against target 0, without a limit."""
    from mcptam_amd import stereo as S
    sc = stereo_world
    cand = np.asarray(tsp._cand(sc, STEREO_LEVEL), dtype=np.int64)
    assert len(cand) >= 560
    oc = _stereo_outcomes(sc, cand, tsp._targets(sc, [0]), 1 << 30)[0]
    return dict(cand=cand, created=oc == S.CREATED)


def _stereo_list(P, n):
    """The first n candidates, with candidate 256 a created one and candidate 255 not (swapped in from further down the list)."""
    order = np.arange(len(P["cand"]))
    cr = P["created"]
    for pos, want in ((255, False), (256, True)):
        if cr[order[pos]] != want:
            k = next(k for k in range(520, len(order)) if cr[order[k]] == want)
            order[[pos, k]] = order[[k, pos]]
    return P["cand"][order[:n]], cr[order[:n]]


@pytest.mark.parametrize("n_cand", [255, 256, 257, 513])
def test_stereo_limit_reached_by_the_last_creation_of_the_first_chunk(gpu_required, stereo_world, stereo_pass, n_cand):
    """(a) limit = the creations among candidates 0 .. 255: every surviving candidate from 256 on is PAST_LIMIT, none before."""
    from mcptam_amd import stereo as S
    cand, cr = _stereo_list(stereo_pass, n_cand)
    limit = int(cr[:256].sum())
    assert limit > 5 and (n_cand < 256 or not cr[255])
    last = np.nonzero(cr[:256])[0][-1]

    def layout(oc, made):
        assert len(made) == limit and made[-1]["candidate"] == last and not (oc[0][:last + 1] == S.PAST_LIMIT).any()
        assert (oc[0][last + 1:] == S.PAST_LIMIT).all() and (n_cand <= 256 or (oc[0][256:] == S.PAST_LIMIT).all())
    _stereo_check(stereo_world, cand, [0], limit, layout)


@pytest.mark.parametrize("n_cand", [257, 513])
def test_stereo_limit_reached_by_the_first_creation_of_the_second_chunk(gpu_required, stereo_world, stereo_pass, n_cand):
    """(b) limit = the creations among candidates 0 .. 255 plus one; candidate 256 is created and is the last one tried."""
    from mcptam_amd import stereo as S
    cand, cr = _stereo_list(stereo_pass, n_cand)
    limit = int(cr[:256].sum()) + 1
    assert cr[256] and not cr[255]

    def layout(oc, made):
        assert made[-1]["candidate"] == 256 and len(made) == limit and not (oc[0][:257] == S.PAST_LIMIT).any() and (oc[0][257:] == S.PAST_LIMIT).all()
    _stereo_check(stereo_world, cand, [0], limit, layout)


@pytest.mark.parametrize("n_cand", [257, 513])
def test_stereo_first_survivor_is_candidate_256_past_the_limit(gpu_required, stereo_world, stereo_pass, n_cand):
    """(c) candidates 0 .. 255 thinned by measurements, so the first survivor is candidate 256, in the second chunk, and it is tried although
    the count has reached the limit.  513 candidates: limit 1, target 0 creates its one point from a later candidate, target 1 starts at the
    limit, tries candidate 256 and nothing else.  257 candidates: candidate 256 is the only survivor, so the limit is 0 -- reached before
    anything is created -- and both targets try it."""
    from mcptam_amd import stereo as S
    P = stereo_pass
    c, cr = P["cand"], P["created"]
    split = int(np.median(c[:, 0]))
    left, right = np.nonzero(c[:, 0] < split - 11)[0], np.nonzero(c[:, 0] > split + 11)[0]
    assert len(left) >= 256
    first = right[~cr[right]][0]                                    # not created on target 0: still alive for target 1
    if n_cand == 257:
        order, limit = np.concatenate([left[:256], [first]]), 0
    else:
        rest = np.setdiff1d(right, [first])[:n_cand - 257]
        assert cr[rest].any()
        order, limit = np.concatenate([left[:256], [first], rest]), 1
    cand = c[order]
    assert len(cand) == n_cand
    roots = S.level_zero_pos(cand[:256], STEREO_LEVEL)
    lv = np.full(256, STEREO_LEVEL)
    alive = S.thin_candidates(cand, STEREO_LEVEL, roots, lv)
    assert not alive[:256].any() and alive[256]

    def layout(oc, made):
        assert sum(1 for m in made if m["target"] == 0) == limit, "target 1 starts at the limit"
        for j in ((0, 1) if limit == 0 else (1,)):
            live = np.nonzero(oc[j] != S.THINNED)[0]
            assert live[0] == 256 and oc[j][256] != S.PAST_LIMIT and (oc[j][live[1:]] == S.PAST_LIMIT).all()
        if n_cand == 513:
            assert made[0]["candidate"] > 256 and int((oc[1] == S.PAST_LIMIT).sum()) > 10
    _stereo_check(stereo_world, cand, [0, 1], limit, layout, meas=S.make_meas(roots, lv), roots=roots, lv=lv)
