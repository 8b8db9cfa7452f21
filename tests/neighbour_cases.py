"""Seeded and hand-built maps for the closest-keyframe queries and the removal of an MKF (include/mcp_img.h mcp_map_neighbours,
mcp_map_mkf_cull), shared by tests/test_neighbours_cpu.py and tests/test_neighbours_gpu.py.

A case is the flat arrays of a small map (tests/cull_cases.py's, extended with the rig, the MKF poses, active bytes and depth means), a list of
queries (mcptam_amd.map_graph.neigh_params' keywords) and a list of removals (MapGraph.cull_mkf's keywords).  The sizes are the seams of the
kernels: 1, 2, 255, 256, 257 present slots, one map with all 4096 slots and 8 cameras (more keyframes than a workgroup's LDS holds distances
for), stores of 0, 1, 63..65, 255..257 entries, present slots with gaps, n_max of 1, of the candidate count, above it and 32.  The value edges
are hand-built on a lattice (identity rotations, integer translations, so every distance is exact in any arithmetic): exact ties, distance 0
under FURTHEST, an MKF without an active keyframe, max_dist equal to a distance, bad and fixed candidates, every region with and without
same_cam, external sources, a translation of 1e200.

THE CONDITION ON THE SEEDED MAPS: the numpy restatement and the C bodies can only name the same keyframes where rounding cannot reorder them,
so separated() asserts for every query of a case that any two distinct distances among its candidates differ by more than 1e-9 relative.  A
seed that violated this was replaced here; nothing is skipped at run time."""
import numpy as np

import cull_cases as cc
from mcptam_amd import map_graph as mg

P, F, B = mg.MKF_PRESENT, mg.MKF_FIXED, mg.MKF_BAD
T, RF, RT = mg.SRC_TRACKER, mg.SRC_REFIND, mg.SRC_ROOT
MKF, KF = mg.NB_MKF, mg.NB_KF
ALL, SELF, OTHER = mg.NB_ALL, mg.NB_ONLY_SELF, mg.NB_ONLY_OTHER
NEAR, FAR = mg.NB_NEAREST, mg.NB_FURTHEST
STORE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
PRESENT_SIZES = (1, 2, 255, 256, 257)
IDENT = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


# ---- poses -------------------------------------------------------------------------------------------------------------------------------------
def _rotations(rng, n, angle):
    w = rng.normal(size=(n, 3))
    w *= (rng.random(n) * angle / np.linalg.norm(w, axis=1))[:, None]
    th = np.linalg.norm(w, axis=1)[:, None, None]
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    with np.errstate(all="ignore"):
        A, Bc = np.where(th > 1e-12, np.sin(th) / th, 1.0), np.where(th > 1e-12, (1 - np.cos(th)) / (th * th), 0.5)
    return np.eye(3)[None] + A * K + Bc * (K @ K)


def with_poses(a, seed, spread=8.0, inactive=0.15):
    """`a` with a random rig, random MKF poses, active bytes (about one keyframe in seven inactive) and depth means."""
    rng = np.random.default_rng(seed)
    n, C = len(a["mkf_flags"]), int(a["ncam"])
    a = dict(a)
    a["cam_from_base"] = mg.poses12(_rotations(rng, C, 3.0), rng.normal(size=(C, 3)) * 0.3)
    a["base_from_world"] = mg.poses12(_rotations(rng, n, 3.0), rng.normal(size=(n, 3)) * spread)
    a["kf_active"] = (rng.random((n, C)) >= inactive).astype(np.uint8)
    a["kf_depth_mean"] = 0.5 + rng.random((n, C)) * 6.0
    return a


def lattice(a, xyz, depth=2.0, active=None, cam_xyz=None):
    """`a` with identity rotations, the given integer MKF translations (n, 3), one depth mean and every keyframe active unless given."""
    n, C = len(a["mkf_flags"]), int(a["ncam"])
    a = dict(a)
    a["cam_from_base"] = np.tile(IDENT, (C, 1))
    a["cam_from_base"][:, 9:] = np.zeros((C, 3)) if cam_xyz is None else np.asarray(cam_xyz, dtype=np.float64).reshape(C, 3)
    a["base_from_world"] = np.tile(IDENT, (n, 1))
    a["base_from_world"][:, 9:] = np.asarray(xyz, dtype=np.float64).reshape(n, 3)
    a["kf_active"] = np.ones((n, C), dtype=np.uint8) if active is None else np.asarray(active, dtype=np.uint8).reshape(n, C)
    a["kf_depth_mean"] = np.broadcast_to(np.asarray(depth, dtype=np.float64), (n, C)).copy()
    return a


def ext_of(a, slot=None, xyz=None, seed=None, active=None, depth=None):
    """An external MKF: a copy of a slot's columns, a lattice pose, or a seeded random one."""
    C = int(a["ncam"])
    if slot is not None:
        return dict(base_from_world=a["base_from_world"][slot].copy(), kf_active=a["kf_active"][slot].copy(), kf_depth_mean=a["kf_depth_mean"][slot].copy())
    if xyz is not None:
        b = IDENT.copy(); b[9:] = xyz
        return dict(base_from_world=b, kf_active=np.ones(C, np.uint8) if active is None else np.asarray(active, np.uint8), kf_depth_mean=np.full(C, 2.0 if depth is None else depth))
    rng = np.random.default_rng(seed)
    act = np.ones(C, np.uint8) if active is None else np.asarray(active, np.uint8)
    return dict(base_from_world=mg.poses12(_rotations(rng, 1, 3.0), rng.normal(size=(1, 3)) * 8.0)[0], kf_active=act, kf_depth_mean=0.5 + rng.random(C) * 6.0)


def small_store(mf, ncam, M, n_rows=None):
    """A map whose store has exactly M entries: row i is measured from four keyframes of present MKFs, the first its source."""
    present = np.flatnonzero(np.asarray(mf) & P)
    n = len(present)
    rows, left, i = [], M, 0
    while left > 0:
        k = min(4, left, n * ncam)
        keys = [(int(present[(i + q) % n]), int((i + q) // n % ncam)) for q in range(k)]
        rows.append(dict(src=keys[0][0], meas=[(m, c, RT if q == 0 else (T if q % 2 else RF)) for q, (m, c) in enumerate(keys)]))
        left -= k
        i += 1
    while len(rows) < (n_rows or 1):
        rows.append(dict(src=int(present[0]), meas=[]))
    a = cc.build(mf, ncam, rows, dead=tuple(range(2, M, 7)))
    for r in range(len(rows)):
        if rows[r]["meas"]:
            a["src_cam"][r] = rows[r]["meas"][0][1]
    assert len(a["ms_mkf"]) == M
    return a


def case(name, a, queries=(), culls=()):
    return dict(name=name, a=a, queries=[dict(q) for q in queries], culls=[dict(c) for c in culls], seeded=False)


def all_dists(a, q):
    """Every candidate's distance of a query, nearest first, by the numpy restatement (no threshold, no cut)."""
    res, items = mg.neighbours_ref(a, dict(q, n_max=1 << 30, max_dist=np.inf, order=NEAR, want_meas=False))
    return res, items


def separated(c):
    """The condition on a seeded case: any two distinct distances of a query differ by more than 1e-9 relative."""
    for q in c["queries"] + [dict(kind=MKF, src_slot=s) for k in c["culls"] for s in ([k["furthest_from"]] if k.get("slot", -1) == -1 else [k["slot"]])]:
        res, items = all_dists(c["a"], q)
        d = np.unique(items["dist"])
        assert res["status"] == 0 and (np.diff(d) > 1e-9 * d[1:]).all(), (c["name"], q)
    c["seeded"] = True
    return c


def _first_present(a, k=0):
    return int(np.flatnonzero(a["mkf_flags"] & P)[k])


def _active_cam(a, slot):
    return int(np.flatnonzero(a["kf_active"][slot])[0])


def standard_queries(a, ext_seed):
    """A source slot with an active keyframe and an external MKF, through every kind, region and order."""
    pres = np.flatnonzero((a["mkf_flags"] & P) != 0)
    s = int(next(k for k in pres if a["kf_active"][k].any()))
    c = _active_cam(a, s)
    e = ext_of(a, seed=ext_seed)
    ec = _active_cam(dict(kf_active=e["kf_active"][None]), 0)
    n_other = len(pres) - 1
    qs = [dict(kind=MKF, order=NEAR, src_slot=s, n_max=1), dict(kind=MKF, order=NEAR, src_slot=s, n_max=max(1, min(n_other, 32)), want_meas=True),
          dict(kind=MKF, order=NEAR, src_slot=s, n_max=min(n_other + 3, 32)), dict(kind=MKF, order=NEAR, src_slot=s, n_max=32, want_meas=True),
          dict(kind=MKF, order=FAR, src_slot=s, n_max=1), dict(kind=MKF, order=FAR, src_slot=s, n_max=5, want_meas=True),
          dict(kind=MKF, order=NEAR, src_slot=-1, ext=e, n_max=3, want_meas=True), dict(kind=MKF, order=FAR, src_slot=-1, ext=e, n_max=1)]
    for region in (ALL, SELF, OTHER):
        for same in (False, True):
            if region == SELF and same:
                continue
            qs.append(dict(kind=KF, order=NEAR, src_slot=s, src_cam=c, region=region, same_cam=same, n_max=5, want_meas=True))
            qs.append(dict(kind=KF, order=NEAR, src_slot=-1, ext=e, src_cam=ec, region=region, same_cam=same, n_max=32))
    qs.append(dict(kind=KF, order=FAR, src_slot=s, src_cam=c, n_max=4))
    # a threshold between two distances: half of the candidates stay
    _, it = all_dists(a, dict(kind=KF, src_slot=s, src_cam=c))
    if len(it) >= 2:
        qs.append(dict(kind=KF, order=NEAR, src_slot=s, src_cam=c, n_max=32, max_dist=float(0.5 * (it["dist"][len(it) // 2 - 1] + it["dist"][len(it) // 2]))))
    return qs


# ---- seeded maps at the size seams ----------------------------------------------------------------------------------------------------------------
def size_cases():
    out = []
    for n in PRESENT_SIZES:                               # present slots, contiguous
        mf = np.full(n, P, dtype=np.int32)
        a = with_poses(small_store(mf, 2, 40), 1000 + n)
        out.append(separated(case("present%d" % n, a, standard_queries(a, 2000 + n))))
    for n in (255, 257):                                  # the same counts with gaps: every third slot empty, some bad, some fixed
        mf = np.zeros(n + n // 2 + 2, dtype=np.int32)
        mf[np.flatnonzero(np.arange(len(mf)) % 3 != 1)[:n]] = P
        mf[5] |= B; mf[9] |= F; mf[12] |= B | F
        a = with_poses(small_store(mf, 3, 120), 1100 + n)
        out.append(separated(case("gaps%d" % n, a, standard_queries(a, 2100 + n))))
    for m in STORE_SIZES:                                 # the store's seams: what k_mgn_count walks
        mf = np.array([P, P, 0, P | B, P, P | F, P], dtype=np.int32)
        a = with_poses(small_store(mf, 2, m), 1200 + m, inactive=0.0)
        out.append(separated(case("store%d" % m, a, [dict(kind=MKF, src_slot=0, n_max=32, want_meas=True), dict(kind=KF, src_slot=0, src_cam=1, n_max=32, want_meas=True),
                                                     dict(kind=KF, src_slot=-1, ext=ext_of(a, seed=1300 + m), src_cam=0, n_max=7, want_meas=True)],
                               [dict(slot=4), dict(slot=-1, furthest_from=0)])))
    return out


def full_case():
    """All 4096 slots, 8 cameras, on a lattice: 32767 candidates of a keyframe query, with exact ties by the thousand."""
    n, C = mg.MAX_MKFS, mg.MAX_CAMS
    rng = np.random.default_rng(4096)
    mf = np.full(n, P, dtype=np.int32)
    mf[rng.choice(n, 300, replace=False)] |= B
    a = small_store(mf, C, 257)
    xyz = rng.integers(-40, 41, size=(n, 3))
    xyz[4095], xyz[4094], xyz[17], xyz[18] = (0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0)      # the nearest to slot 0 sit at both ends of the index range
    xyz[0] = 0
    a = lattice(a, xyz, depth=rng.integers(1, 5, size=(n, C)).astype(np.float64), active=rng.random((n, C)) < 0.9, cam_xyz=rng.integers(-2, 3, size=(C, 3)))
    a["kf_active"][0, 0] = a["kf_active"][4095, 7] = 1
    e = ext_of(a, xyz=(3, -2, 5))
    qs = [dict(kind=KF, src_slot=0, src_cam=0, n_max=32, want_meas=True), dict(kind=KF, src_slot=4095, src_cam=7, n_max=32, region=OTHER, same_cam=True),
          dict(kind=KF, src_slot=-1, ext=e, src_cam=3, n_max=32), dict(kind=KF, order=FAR, src_slot=0, src_cam=0, n_max=32),
          dict(kind=MKF, src_slot=0, n_max=32, want_meas=True), dict(kind=MKF, order=FAR, src_slot=-1, ext=e, n_max=32), dict(kind=KF, src_slot=0, src_cam=0, n_max=5, max_dist=3.0)]
    return case("full_4096x8", a, qs)


# ---- value edges, on a lattice ----------------------------------------------------------------------------------------------------------------------
def edge_cases():
    out = []
    mf = np.array([P, P, P | B, 0, P | F, P, P | B | F, P], dtype=np.int32)
    base = small_store(mf, 2, 30)
    # slots 2 and 5 bit-identical; slot 1 at the source's own pose (distance 0); slot 7 without an active keyframe (DBL_MAX)
    xyz = [(0, 0, 0), (0, 0, 0), (3, 0, 0), (9, 9, 9), (6, 0, 0), (3, 0, 0), (0, 4, 0), (1, 1, 1)]
    act = np.ones((8, 2), np.uint8); act[7] = 0
    a = lattice(base, xyz, active=act)
    out.append(case("ties_zero_and_no_active", a, [
        dict(kind=MKF, src_slot=0, n_max=32), dict(kind=MKF, src_slot=0, n_max=2), dict(kind=MKF, src_slot=0, n_max=3), dict(kind=MKF, order=FAR, src_slot=0, n_max=32),
        dict(kind=MKF, order=FAR, src_slot=0, n_max=1), dict(kind=MKF, order=FAR, src_slot=0, n_max=1, max_dist=1e300), dict(kind=MKF, src_slot=0, n_max=32, max_dist=4.5),
        dict(kind=MKF, src_slot=0, n_max=32, max_dist=4.499999999999999), dict(kind=MKF, src_slot=0, n_max=32, max_dist=0.0), dict(kind=MKF, order=FAR, src_slot=1, n_max=32, max_dist=0.0),
        dict(kind=KF, src_slot=0, src_cam=0, n_max=32), dict(kind=KF, src_slot=0, src_cam=1, n_max=32, same_cam=True), dict(kind=KF, order=FAR, src_slot=0, src_cam=0, n_max=32),
        dict(kind=KF, src_slot=0, src_cam=0, region=SELF, n_max=32), dict(kind=KF, order=FAR, src_slot=0, src_cam=0, region=SELF, n_max=32),
        dict(kind=KF, src_slot=0, src_cam=0, region=OTHER, n_max=32, max_dist=4.5), dict(kind=KF, src_slot=0, src_cam=0, region=OTHER, same_cam=True, n_max=32, want_meas=True),
        dict(kind=MKF, src_slot=7, n_max=32), dict(kind=MKF, order=FAR, src_slot=7, n_max=32),
        # external sources: one equal to slot 2's (and 5's) columns, one at the origin, one without an active keyframe of its own
        dict(kind=MKF, src_slot=-1, ext=ext_of(a, slot=2), n_max=32, want_meas=True), dict(kind=MKF, order=FAR, src_slot=-1, ext=ext_of(a, slot=2), n_max=32),
        dict(kind=KF, src_slot=-1, ext=ext_of(a, slot=2), src_cam=1, n_max=32), dict(kind=KF, src_slot=-1, ext=ext_of(a, slot=2), src_cam=1, region=SELF, n_max=32),
        dict(kind=KF, src_slot=-1, ext=ext_of(a, slot=2), src_cam=0, region=OTHER, same_cam=True, n_max=32),
        dict(kind=KF, src_slot=-1, ext=ext_of(a, xyz=(0, 0, 0), active=(0, 1)), src_cam=1, region=SELF, n_max=32), dict(kind=MKF, src_slot=-1, ext=ext_of(a, xyz=(0, 0, 0), active=(0, 0)), n_max=32)]))
    # one present slot: no candidate at all; two: one
    one = lattice(small_store(np.array([0, P], np.int32), 2, 5), [(0, 0, 0), (1, 2, 3)])
    out.append(case("one_present", one, [dict(kind=MKF, src_slot=1, n_max=4), dict(kind=MKF, order=FAR, src_slot=1), dict(kind=KF, src_slot=1, src_cam=0, n_max=4, want_meas=True),
                                         dict(kind=KF, src_slot=1, src_cam=0, region=OTHER, n_max=4), dict(kind=MKF, src_slot=-1, ext=ext_of(one, slot=1), n_max=4)]))
    # a translation of 1e200: the squares overflow, the reference stops the process
    big = lattice(base, xyz, active=act)
    big["base_from_world"][4, 9] = 1e200
    out.append(case("overflow", big, [dict(kind=MKF, src_slot=0, n_max=8), dict(kind=KF, src_slot=0, src_cam=0, n_max=8, want_meas=True), dict(kind=MKF, order=FAR, src_slot=4, n_max=1),
                                      dict(kind=KF, src_slot=0, src_cam=0, region=SELF, n_max=8), dict(kind=MKF, src_slot=-1, ext=ext_of(big, xyz=(1e200, 0, 0)), n_max=8)],
                    [dict(slot=-1, furthest_from=0), dict(slot=4), dict(slot=0)]))
    return out


# ---- the removal of an MKF --------------------------------------------------------------------------------------------------------------------------
def cull_cases():
    out = []
    # slots on a line; 3 is fixed and the furthest from 0; 4 is bad and the nearest to 3; 5 sits on 0's pose
    mf = np.array([P, P, P, P | F, P | B, P, 0], dtype=np.int32)
    xyz = [(0, 0, 0), (2, 0, 0), (5, 0, 0), (20, 0, 0), (17, 0, 0), (0, 0, 0), (50, 0, 0)]
    V = 3
    rows = [dict(src=0, meas=[(0, 0, RT), (V, 0, T)]),                                        # 0: two entries = max_kfs: marked by count
            dict(src=0, meas=[(0, 0, RT), (1, 0, T), (V, 1, T)]),                             # 1: max_kfs + 1: stays
            dict(src=V, meas=[(V, 0, RT), (0, 0, T), (1, 0, T), (2, 0, T)]),                  # 2: its source keyframe is the victim's: marked by source
            dict(src=V, meas=[(V, 0, T), (0, 0, T), (1, 0, T), (2, 0, T)]),                   # 3: source (V, cam 1), measured from (V, cam 0) only: stays
            dict(flags=mg.GP_FIXED, src=-1, meas=[(V, 0, T), (0, 0, T)]),                     # 4: fixed, at the limit: stays
            dict(flags=mg.GP_FIXED, src=V, meas=[(V, 0, RT), (0, 0, T), (1, 0, T)]),          # 5: fixed, but its source is the victim's keyframe: marked by source
            dict(flags=mg.GP_BAD, src=0, meas=[(0, 0, RT), (V, 0, T)]),                       # 6: bad already: counts nowhere
            dict(src=V, meas=[(V, 0, RT), (V, 1, T)]),                                        # 7: by source and by count, two entries of the victim: one row, by source
            dict(src=0, meas=[(0, 0, RT), (4, 0, T), (V, 1, T)]),                             # 8: three entries, one from a bad MKF: every live entry counts, stays
            dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T)]),                             # 9: not seen from the victim
            dict(src=0, meas=[(0, 0, RT), (1, 0, T), (V, 0, T)]),                             # 10: three entries, one dead: two live, marked by count
            dict(cc.NEVER, meas=[(V, 0, T)])]                                                 # 11: never written
    a = cc.build(mf, 2, rows, n_rows=14)
    a["src_cam"][3] = 1
    a["ms_alive"][(a["ms_row"] == 10) & (a["ms_mkf"] == 1)] = 0
    a = lattice(a, xyz)
    assert int((a["ms_alive"] == 0).sum()) == 1
    both = [dict(slot=V), dict(slot=-1, furthest_from=0), dict(slot=V, mark_points=False), dict(slot=V, erase=False), dict(slot=V, max_kfs=3), dict(slot=V, max_kfs=0),
            dict(slot=-1, furthest_from=5, erase=False), dict(slot=0), dict(slot=4), dict(slot=-1, furthest_from=3)]
    out.append(case("rules", a, [dict(kind=MKF, order=FAR, src_slot=0), dict(kind=MKF, src_slot=V)], both))
    # a fixed victim alone in the map, and with one bad neighbour; no victim at all
    alone = lattice(cc.build(np.array([0, P | F], np.int32), 1, [dict(src=1, meas=[(1, 0, RT)])]), [(0, 0, 0), (1, 0, 0)])
    out.append(case("fixed_alone", alone, [], [dict(slot=1), dict(slot=-1, furthest_from=1)]))
    pair = lattice(cc.build(np.array([P | F, P | B], np.int32), 1, [dict(src=0, meas=[(0, 0, RT), (1, 0, T)])]), [(0, 0, 0), (1, 0, 0)])
    out.append(case("fixed_with_a_bad_neighbour", pair, [], [dict(slot=0), dict(slot=-1, furthest_from=1)]))
    same = lattice(cc.build(np.array([P, P, P], np.int32), 1, [dict(src=0, meas=[(0, 0, RT), (1, 0, T)])]), [(4, 4, 4)] * 3)
    out.append(case("everything_at_distance_0", same, [dict(kind=MKF, order=FAR, src_slot=0, n_max=3)], [dict(slot=-1, furthest_from=0), dict(slot=2)]))
    # seeded maps: tests/cull_cases.py's, with poses
    for seed, n_mkfs, ncam, rows_, per in ((31, 9, 2, 255, (0, 6)), (32, 14, 3, 257, (1, 9)), (33, 40, 2, 513, (0, 5))):
        a = with_poses(cc.random_map(seed, n_mkfs, ncam, rows_, rows_ + 20, per_row=per), 3000 + seed)
        pres = np.flatnonzero(a["mkf_flags"] & P)
        src = a["src_mkf"][(a["src_mkf"] >= 0)]
        a["src_cam"][:] = np.random.default_rng(seed).integers(0, ncam, len(a["src_cam"]))
        fixed = int(pres[(a["mkf_flags"][pres] & F) != 0][0]) if ((a["mkf_flags"][pres] & F) != 0).any() else int(pres[-1])
        a["mkf_flags"][fixed] |= F
        culls = [dict(slot=-1, furthest_from=int(pres[0])), dict(slot=fixed), dict(slot=int(np.bincount(src).argmax())), dict(slot=int(pres[2]), max_kfs=3, erase=False),
                 dict(slot=int(pres[1]), mark_points=False)]
        out.append(separated(case("seeded%d" % seed, a, [dict(kind=MKF, src_slot=int(pres[0]), n_max=32, want_meas=True)], culls)))
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = size_cases() + [full_case()] + edge_cases() + cull_cases()
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


_REF = {}


def ref(c):
    """The numpy restatement's answers of a case, computed once: (the queries' (result, items), the removals' (result, arrays after))."""
    if c["name"] not in _REF:
        _REF[c["name"]] = ([mg.neighbours_ref(c["a"], q) for q in c["queries"]], [mg.cull_mkf_ref(c["a"], **k) for k in c["culls"]])
    return _REF[c["name"]]


CULL_STATE = ("mkf_flags", "pt_flags", "pending", "ms_alive")
