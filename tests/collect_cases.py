"""Hand-built and seeded maps for the co-visible points of the nearest keyframe (include/mcp_img.h mcp_map_collect_nearest,
mcp_track_collect_nearest), shared by tests/test_collect_cpu.py and tests/test_collect_gpu.py.

A case is the flat arrays of a small map (tests/neighbour_cases.py's layout), the tracker's pose, one depth mean and one active byte per
camera, optionally the current keyframes' own CamFromBase, and -- where the answer can be read off the description -- the expected mask.
The hand-built maps sit on neighbour_cases.lattice (identity rotations, integer translations), so their distances are exact in any
arithmetic and ties are exact ties.  The shapes are the smallest at which a stage can go wrong: two hops and not three, a winner without a
live entry, dead and erased links, candidates that must be ignored or must win, exact ties, the first and the last byte of kf_mark, stores
of 0, 1, 255, 256, 257 and 513 entries, 1, 63, 64, 65, 256 and 257 rows, one row hit by 300 entries, two and eight cameras.

THE CONDITIONS ON THE SEEDED MAPS: margin() asserts with the numpy restatement that every used camera's winner is closer than the runner-up
by more than 1e-6 relative, so that rounding cannot make the restatement and the C bodies name different keyframes; the 32-MKF map also
asserts that every used camera keeps between 5 % and 95 % of the rows.  A seed that violated a condition was replaced here; nothing is
skipped at run time.

An entry of a case that is dead has a key (mkf, cam, row) no live entry shares, so that load() can bring the store to the device by adding
every entry and erasing the dead ones by key; `erased` names slots that load() removes with MapGraph.erase_mkf after loading them."""
import numpy as np

import cull_cases as cc
import neighbour_cases as nc
from mcptam_amd import map_graph as mg

P, F, B = mg.MKF_PRESENT, mg.MKF_FIXED, mg.MKF_BAD
T = mg.SRC_TRACKER
STORE_SIZES = (0, 1, 255, 256, 257, 513)
ROW_SIZES = (1, 63, 64, 65, 256, 257)


def arrays(mf, ncam, n_rows, entries, dead=()):
    """Flat arrays with the store in the given order: entries [(mkf, cam, row), ...], dead: indices into it."""
    mf = np.asarray(mf, dtype=np.int32)
    src = int(np.flatnonzero(mf & P)[0]) if (mf & P).any() else -1
    a = cc.build(mf, ncam, [dict(src=src, flags=0 if src >= 0 else mg.GP_FIXED) for _ in range(n_rows)])
    e = np.array(list(entries), dtype=np.int32).reshape(-1, 3)
    M = len(e)
    a["ms_mkf"], a["ms_cam"], a["ms_row"] = (np.ascontiguousarray(e[:, k]) for k in range(3))
    a["ms_source"] = np.full(M, T, dtype=np.int32)
    a["ms_alive"] = np.ones(M, dtype=np.uint8)
    a["ms_alive"][list(dead)] = 0
    a["ms_uv"] = np.stack([np.arange(M) * 0.5 + 0.25, 480.0 - np.arange(M) * 0.125], axis=1).reshape(M, 2)
    a["ms_level"] = (np.arange(M) % 4).astype(np.int32)
    live = {tuple(k) for k in e[a["ms_alive"] != 0]}
    gone = [tuple(k) for k in e[a["ms_alive"] == 0]]
    assert not (set(gone) & live) and len(set(gone)) == len(gone), "a dead entry shares its key"
    return a


def pose_at(xyz):
    b = nc.IDENT.copy()
    b[9:] = -np.asarray(xyz, dtype=np.float64)          # identity rotation: the base sits at xyz
    return b


def mkf_at(xyz):
    """MKF translations that put the bases at the given world positions (identity rotations)."""
    return -np.asarray(xyz, dtype=np.float64)


def case(name, a, pose, depth_mean=None, active=None, cam_from_base=None, frac=0.5, near=None, winners=None, status=None, erased=()):
    C = int(a["ncam"])
    d = np.full(C, 2.0) if depth_mean is None else np.asarray(depth_mean, dtype=np.float64)
    return dict(name=name, a=a, pose=np.asarray(pose, dtype=np.float64), depth_mean=d, active=np.ones(C, np.uint8) if active is None else np.asarray(active, np.uint8),
                cam_from_base=cam_from_base, frac=frac, near=None if near is None else np.asarray(near, dtype=np.uint8), winners=winners, status=status, erased=tuple(erased))


def kwargs(c):
    """What collect_nearest_ref / collect_nearest_host / MapGraph.collect_nearest take after the arrays / the graph."""
    return dict(base_from_world=c["pose"], depth_mean=c["depth_mean"], mean_diff_fraction=c["frac"], active=c["active"], cam_from_base=c["cam_from_base"])


def margin(c, rel=1e-6):
    """The condition on a seeded case: every used camera's winner beats the runner-up by more than `rel` relative."""
    a, k = c["a"], kwargs(c)
    rep, _ = mg.collect_nearest_ref(a, **k)
    C = int(a["ncam"])
    for cam in np.flatnonzero(c["active"][:C]):
        assert rep["status"][cam] == 0, (c["name"], cam)
        b = mg.copy_arrays(a)
        b["kf_active"][rep["nearest_slot"][cam], rep["nearest_cam"][cam]] = 0
        second, _ = mg.collect_nearest_ref(b, **k)
        if second["status"][cam] == 0:
            assert second["nearest_dist"][cam] - rep["nearest_dist"][cam] > rel * second["nearest_dist"][cam], (c["name"], cam)
    return c


# ---- the seams of the walk, on a lattice ------------------------------------------------------------------------------------------------------
def walk_cases():
    out = []
    line = mkf_at([(0, 0, 0), (5, 0, 0), (10, 0, 0), (15, 0, 0)])
    # K0 (nearest), K1, K2, K3; p0 {K0, K1}, p1 {K1, K2}, p2 {K2, K3}, p3 {K3}: exactly {p0, p1}; K1 is marked, K2 is not
    a = nc.lattice(arrays([P] * 4, 1, 4, [(0, 0, 0), (1, 0, 0), (1, 0, 1), (2, 0, 1), (2, 0, 2), (3, 0, 2), (3, 0, 3)]), line)
    out.append(case("two_hops_not_three", a, pose_at((0, 0, 0)), near=[1, 1, 0, 0], winners=[(0, 0)], status=[0]))
    # the nearest keyframe measures nothing / only through a dead entry
    a = nc.lattice(arrays([P] * 4, 1, 4, [(1, 0, 0), (1, 0, 1), (2, 0, 1)]), line)
    out.append(case("nearest_without_an_entry", a, pose_at((1, 0, 0)), near=[0, 0, 0, 0], winners=[(0, 0)], status=[0]))
    a = nc.lattice(arrays([P] * 4, 1, 4, [(0, 0, 0), (1, 0, 0), (1, 0, 1)], dead=[0]), line)
    out.append(case("the_only_seed_link_is_dead", a, pose_at((0, 0, 0)), near=[0, 0, 0, 0], winners=[(0, 0)], status=[0]))
    # a live path only: K0 - r2 - K1 - r4; K1's entry on r3 is dead; slot 2 (r4, r5) has been erased; slot 3 measures r3 and r5 alone
    a = nc.lattice(arrays([P, P, 0, P], 1, 6, [(0, 0, 2), (1, 0, 2), (1, 0, 3), (1, 0, 4), (2, 0, 4), (2, 0, 5), (3, 0, 3), (3, 0, 5)], dead=[2, 4, 5]), line)
    out.append(case("dead_and_erased_entries_do_not_link", a, pose_at((0, 0, 0)), near=[0, 0, 1, 0, 1, 0], winners=[(0, 0)], status=[0], erased=[2]))
    return out


def candidate_cases():
    out = []
    ent = [(0, 0, 0), (1, 0, 1), (2, 0, 2), (0, 0, 3), (1, 0, 3)]
    xyz = mkf_at([(1, 0, 0), (3, 0, 0), (6, 0, 0)])
    act = np.ones((3, 1), np.uint8); act[0, 0] = 0
    a = nc.lattice(arrays([P, P, P], 1, 4, ent), xyz, active=act)
    # (slot 0's keyframe is closer but not active: no candidate; its entries are measurements all the same, so r3 brings r0 in)
    out.append(case("an_inactive_keyframe_is_no_candidate", a, pose_at((0, 0, 0)), near=[1, 1, 0, 1], winners=[(1, 0)], status=[0]))
    a = nc.lattice(arrays([P | B, P, P | F], 1, 4, ent), xyz)
    out.append(case("a_bad_mkf_wins", a, pose_at((0, 0, 0)), near=[1, 1, 0, 1], winners=[(0, 0)], status=[0]))
    a = nc.lattice(arrays([0, 0], 1, 3, []), mkf_at([(0, 0, 0), (1, 0, 0)]))
    out.append(case("no_present_slot", a, pose_at((0, 0, 0)), near=[0, 0, 0], winners=[(-1, -1)], status=[1]))
    # one candidate beyond 1e10 breaks the query although another sits next to the tracker
    a = nc.lattice(arrays([P, P, P], 1, 4, ent), mkf_at([(1, 0, 0), (3e10, 0, 0), (6, 0, 0)]))
    out.append(case("a_distance_above_1e10", a, pose_at((0, 0, 0)), near=[0, 0, 0, 0], winners=[(-1, -1)], status=[3]))
    a = nc.lattice(arrays([P, P, P], 1, 4, ent), mkf_at([(1, 0, 0), (1e200, 0, 0), (6, 0, 0)]))
    out.append(case("a_distance_that_overflows", a, pose_at((0, 0, 0)), near=[0, 0, 0, 0], winners=[(-1, -1)], status=[3]))
    return out


def tie_cases():
    out = []
    # slots 1 and 3 have the same pose bits and depth and are the nearest: the smaller slot; the two cameras of the rig coincide: the smaller camera
    xyz = mkf_at([(9, 0, 0), (2, 0, 0), (7, 0, 0), (2, 0, 0)])
    ent = [(1, 0, 0), (3, 0, 1), (1, 1, 2), (3, 1, 3), (0, 0, 4)]
    a = nc.lattice(arrays([P] * 4, 2, 5, ent), xyz)
    out.append(case("ties_go_to_the_smaller_slot_and_camera", a, pose_at((0, 0, 0)), near=[3, 0, 0, 0, 0], winners=[(1, 0), (1, 0)], status=[0, 0]))
    act = np.ones((4, 2), np.uint8); act[1, 0] = 0
    a = nc.lattice(arrays([P] * 4, 2, 5, ent), xyz, active=act)          # (1, 0) gone: (1, 1) before (3, 0)
    out.append(case("ties_within_a_slot_before_the_next_slot", a, pose_at((0, 0, 0)), near=[0, 0, 3, 0, 0], winners=[(1, 1), (1, 1)], status=[0, 0]))
    return out


def camera_cases():
    out = []
    # two cameras 100 apart; slot 0 has only camera 0, slot 1 only camera 1, slot 2 (far) links a row of each: r0 is camera 0's alone, r2 camera 1's
    cam_xyz = [(0, 0, 0), (-100, 0, 0)]
    act = np.array([[1, 0], [0, 1], [1, 1]], np.uint8)
    ent = [(0, 0, 0), (0, 0, 1), (1, 1, 2), (1, 1, 3), (2, 0, 1), (2, 0, 3), (2, 1, 4)]
    a = nc.lattice(arrays([P, P, P], 2, 6, ent), mkf_at([(0, 0, 0), (0, 1, 0), (0, 40, 0)]), active=act, cam_xyz=cam_xyz)
    out.append(case("two_cameras_two_winners", a, pose_at((0, 0, 0)), near=[1, 3, 2, 3, 0, 0], winners=[(0, 0), (1, 1)], status=[0, 0]))
    out.append(case("a_camera_switched_off", a, pose_at((0, 0, 0)), active=[1, 0], near=[1, 1, 0, 1, 0, 0], winners=[(0, 0), (-1, -1)], status=[0, 0]))
    # the current keyframes' own CamFromBase: camera 1 sits where the rig's camera 0 is, so it too picks (0, 0)
    own = np.tile(nc.IDENT, (2, 1))
    out.append(case("the_frames_own_cam_from_base", a, pose_at((0, 0, 0)), cam_from_base=own, near=[3, 3, 0, 3, 0, 0], winners=[(0, 0), (0, 0)], status=[0, 0]))
    return out


def index_edge_case():
    """All 4096 slots and 8 cameras in the arrays; the winners are (4095, c): camera 7's mark is the last byte of kf_mark."""
    n, C = mg.MAX_MKFS, mg.MAX_CAMS
    mf = np.zeros(n, dtype=np.int32)
    mf[[0, 7, n - 1]] = P
    xyz = np.zeros((n, 3))
    xyz[0], xyz[7], xyz[n - 1] = (0, 0, 0), (0, 50, 0), (0, 0, 7)
    ent = [(n - 1, c, c) for c in range(C)] + [(0, c, c) for c in range(0, C, 2)] + [(0, c, 8 + c) for c in range(C)] + [(7, 0, 20), (7, 7, 21)]
    a = nc.lattice(arrays(mf, C, 24, ent), mkf_at(xyz), cam_xyz=[(-100 * c, 0, 0) for c in range(C)])
    near = np.zeros(24, np.uint8)
    for c in range(C):
        near[c] |= 1 << c
        if c % 2 == 0:
            near[8 + c] |= 1 << c
    return case("last_slot_last_camera", a, pose_at((0, 0, 7)), depth_mean=np.full(C, 2.0), near=near, winners=[(n - 1, c) for c in range(C)], status=[0] * C)


# ---- seeded maps ---------------------------------------------------------------------------------------------------------------------------------
def seeded(name, seed, n_mkf, ncam, n_rows, n_entries, window=8.0, step=3.0, dead_frac=0.1, at=None):
    """MKFs along a line (random rotations, `step` apart, jittered), rows along the same line, each entry a (keyframe, row) pair no further
    apart than `window` where the map has that many such pairs (otherwise keys repeat and no entry is dead); the tracker near MKF `at`."""
    rng = np.random.default_rng(seed)
    mf = np.full(n_mkf, P, dtype=np.int32)
    mf[rng.random(n_mkf) < 0.15] |= B
    pos = np.stack([np.arange(n_mkf) * step, rng.normal(size=n_mkf), rng.normal(size=n_mkf)], axis=1)
    R = nc._rotations(rng, n_mkf, 3.0)
    bfw = mg.poses12(R, -np.einsum("nij,nj->ni", R, pos))
    row_x = rng.random(n_rows) * (n_mkf - 1) * step
    m, r = np.nonzero(np.abs(pos[:, 0][:, None] - row_x[None, :]) <= window)
    pairs = np.array([(mm, c, rr) for mm, rr in zip(m, r) for c in range(ncam)], dtype=np.int32).reshape(-1, 3)
    unique = len(pairs) >= n_entries
    pick = rng.choice(len(pairs), size=n_entries, replace=not unique) if n_entries else np.zeros(0, dtype=np.int64)
    ent = pairs[pick]
    dead = np.flatnonzero(rng.random(n_entries) < dead_frac) if unique else ()
    a = arrays(mf, ncam, n_rows, ent, dead=dead)
    a["cam_from_base"] = mg.poses12(nc._rotations(rng, ncam, 3.0), rng.normal(size=(ncam, 3)) * 0.3)
    a["base_from_world"] = bfw
    a["kf_active"] = (rng.random((n_mkf, ncam)) >= 0.1).astype(np.uint8)
    a["kf_depth_mean"] = 0.5 + rng.random((n_mkf, ncam)) * 6.0
    k = n_mkf // 3 if at is None else at
    Rt = nc._rotations(rng, 1, 0.2)[0] @ R[k]
    pose = mg.poses12(Rt[None], -(Rt @ (pos[k] + rng.normal(size=3) * 0.4))[None])[0]
    return margin(case(name, a, pose, depth_mean=0.5 + rng.random(ncam) * 6.0))


def size_cases():
    out = [seeded("store%d" % m, 100 + m, 6, 2, 40, m) for m in STORE_SIZES]
    out += [seeded("rows%d" % n, 200 + n, 6, 2, n, 300) for n in ROW_SIZES]          # rows1: one row hit by 300 entries
    out.append(seeded("eight_cameras", 300, 5, 8, 70, 400, window=5.0))
    return out


def seeded_map():
    """About 32 MKFs x 2 cameras, 600 rows and 4000 entries with clustered visibility: neither nothing nor everything."""
    c = seeded("seeded_32x2", 7, 32, 2, 600, 4000)
    rep, near = ref(c)
    for cam in range(2):
        kept = int(((near >> cam) & 1).sum())
        assert 0.05 * 600 <= kept <= 0.95 * 600 and kept == rep["n_rows"][cam], (cam, kept)
    return c


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = walk_cases() + candidate_cases() + tie_cases() + camera_cases() + [index_edge_case()] + size_cases() + [seeded_map()]
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


_REF = {}


def ref(c):
    """The numpy restatement's answer of a case, computed once and left unchanged: (report dict, near)."""
    if c["name"] not in _REF:
        _REF[c["name"]] = mg.collect_nearest_ref(c["a"], **kwargs(c))
    return _REF[c["name"]]


INT_FIELDS = ("status", "nearest_slot", "nearest_cam", "n_candidates", "n_seed_rows", "n_kfs", "n_rows")


def load(c, table):
    """The case's map on the device: the table's rows, a fresh MapGraph with the MKFs, the point columns and the store; the slots of
    `erased` are loaded present with their entries alive and then removed with erase_mkf."""
    a = mg.copy_arrays(c["a"])
    for s in c["erased"]:
        a["mkf_flags"][s] |= P
        a["ms_alive"][a["ms_mkf"] == s] = 1
    n = int(a["n_rows"])
    z = np.zeros((n, 3))
    table.resize(0)
    table.set(z, z, z, np.ones(n, dtype=np.uint8))
    g = mg.MapGraph(table, a["cam_from_base"])
    g.load_arrays(a)
    for s in c["erased"]:
        g.erase_mkf(s)
    return g
