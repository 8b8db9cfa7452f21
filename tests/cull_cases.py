"""Seeded maps for the outlier and bad-point calls (include/mcp_img.h mcp_map_cull_*), shared by tests/test_cull_cpu.py and tests/test_cull_gpu.py.

A case is the flat arrays of a small map (mcptam_amd.map_graph's keys: MKF flags, the graph columns written so far, the store with its alive
flags, the table's count and usable columns), an outlier list in the solver's order, and the sweep's parameters.  The shapes are the smallest at
which the kernels can go wrong: lists and stores of 0, 1, 63..65, 255..257 entries (a wavefront, a workgroup), point rows of 255, 256, 257 and
513, all of a list on one row, one row's outliers scattered through the list, and the value edges of the two rules.  No case has more than a
few thousand store entries."""
import numpy as np

from mcptam_amd import map_graph as mg

LIST_SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
ROW_SIZES = (255, 256, 257, 513)
STORE_SIZES = (1, 256, 257)
P, F, B = mg.MKF_PRESENT, mg.MKF_FIXED, mg.MKF_BAD
T, RF, RT, TR, EP = mg.SRC_TRACKER, mg.SRC_REFIND, mg.SRC_ROOT, mg.SRC_TRAIL, mg.SRC_EPIPOLAR
NEVER = dict(flags=mg.GP_BAD, src=-1)          # a row never written: (no source, bad, not fixed)


def build(mkf_flags, ncam, rows, n_rows=None, dead=(), order=None):
    """Flat arrays from a description.  rows: one dict per graph column written so far -- flags, src (source MKF slot; -1 with GP_FIXED or for
    NEVER), counts (inlier, outlier), usable, meas: [(mkf, cam, source), ...] -- n_rows: the table's rows (>= len(rows)); dead: store indices (in
    description order) of entries that are dead already; order: a permutation of the store."""
    Np = len(rows)
    R = Np if n_rows is None else int(n_rows)
    a = dict(ncam=int(ncam), mkf_flags=np.asarray(mkf_flags, dtype=np.int32))
    a["src_mkf"] = np.array([r.get("src", 0) for r in rows], dtype=np.int32).reshape(Np)
    a["src_cam"] = np.zeros(Np, dtype=np.int32)
    a["pt_flags"] = np.array([r.get("flags", 0) for r in rows], dtype=np.int32).reshape(Np)
    a["pending"] = np.zeros(Np, dtype=np.uint8)
    cnt = np.array([r.get("counts", (1, 0)) for r in rows] + [(1, 0)] * (R - Np), dtype=np.int32).reshape(R, 2)
    a["inlier"], a["outlier"] = np.ascontiguousarray(cnt[:, 0]), np.ascontiguousarray(cnt[:, 1])
    a["usable"] = np.array([r.get("usable", 1) for r in rows] + [1] * (R - Np), dtype=np.uint8).reshape(R)
    ms = [(m, c, i, s) for i, r in enumerate(rows) for (m, c, s) in r.get("meas", ())]
    ms = np.array(ms, dtype=np.int32).reshape(-1, 4)
    alive = np.ones(len(ms), dtype=np.uint8)
    alive[list(dead)] = 0
    if order is not None:
        ms, alive = ms[order], alive[order]
    M = len(ms)
    a["ms_mkf"], a["ms_cam"], a["ms_row"], a["ms_source"] = (np.ascontiguousarray(ms[:, k]) for k in range(4))
    a["ms_alive"] = alive
    a["ms_uv"] = np.stack([np.arange(M) * 0.5 + 0.25, 480.0 - np.arange(M) * 0.125], axis=1).reshape(M, 2)
    a["ms_level"] = (np.arange(M) % 4).astype(np.int32)
    a["n_rows"] = R
    return a


def case(name, a, keys=(), sweep=None, bad_good_count=2):
    k = np.array(list(keys), dtype=np.int32).reshape(-1, 3)
    return dict(name=name, a=a, mkf=np.ascontiguousarray(k[:, 0]), cam=np.ascontiguousarray(k[:, 1]), row=np.ascontiguousarray(k[:, 2]), n=len(k),
                bad_good_count=bad_good_count, sweep=dict(dict(min_outliers=20, outlier_multiplier=1.0, danglers=True), **(sweep or {})))


# ---- seeded maps ---------------------------------------------------------------------------------------------------------------------------------
def random_map(seed, n_mkfs, ncam, n_point_rows, n_rows, per_row=(0, 7), dead_frac=0.12):
    """MKFs present (about one in six bad, one in eight fixed, slot 1 empty), rows good / fixed / bad by the host / never written, between
    per_row[0] and per_row[1] - 1 measurements per row from distinct keyframes with every source, some dead, the store shuffled; counts on both
    sides of the tracker rule."""
    rng = np.random.default_rng(seed)
    mf = np.where(rng.random(n_mkfs) < 1 / 6, P | B, P) | np.where(rng.random(n_mkfs) < 1 / 8, F, 0)
    if n_mkfs > 3:
        mf[1] = 0
    present = np.flatnonzero(mf & P)
    rows = []
    for i in range(n_rows):
        u = rng.random()
        r = dict(NEVER) if u < 0.06 else dict(flags=mg.GP_FIXED, src=-1 if rng.random() < 0.5 else int(rng.choice(present))) if u < 0.14 else \
            dict(flags=mg.GP_BAD if u < 0.22 else 0, src=int(rng.choice(present)))
        r["counts"] = (int(rng.integers(1, 30)), int(rng.integers(0, 45)))
        r["usable"] = int(rng.random() < 0.9)
        k = min(int(rng.integers(per_row[0], per_row[1])), len(present) * ncam)
        kf = rng.choice(len(present) * ncam, size=k, replace=False)
        r["meas"] = [(int(present[q // ncam]), int(q % ncam), int(rng.integers(0, 5))) for q in kf]
        rows.append(r)
    tail = rows[n_point_rows:]                            # rows of the table past the graph columns: they may hold measurements all the same
    a = build(mf, ncam, rows[:n_point_rows], n_rows)
    extra = np.array([(m, c, n_point_rows + i, s) for i, r in enumerate(tail) for (m, c, s) in r["meas"]], dtype=np.int32).reshape(-1, 4)
    for k, col in enumerate(("ms_mkf", "ms_cam", "ms_row", "ms_source")):
        a[col] = np.concatenate([a[col], extra[:, k]]).astype(np.int32)
    M = len(a["ms_mkf"])
    perm = rng.permutation(M)
    for col in ("ms_mkf", "ms_cam", "ms_row", "ms_source"):
        a[col] = np.ascontiguousarray(a[col][perm])
    a["ms_alive"] = (rng.random(M) >= dead_frac).astype(np.uint8)
    a["ms_uv"] = np.ascontiguousarray(rng.random((M, 2)) * 400.0)
    a["ms_level"] = rng.integers(0, 4, M).astype(np.int32)
    for i, r in enumerate(tail):
        a["inlier"][n_point_rows + i], a["outlier"][n_point_rows + i] = r["counts"]
        a["usable"][n_point_rows + i] = r["usable"]
    return a


def random_keys(seed, a, n, distinct_rows=False):
    """n distinct keys in a shuffled order: mostly live entries, some dead ones, some that no entry has (a camera the keyframe does not measure
    the row with, the empty slot 1, a row past the table, row -1)."""
    rng = np.random.default_rng(seed)
    M, R, C = len(a["ms_mkf"]), a["n_rows"], a["ncam"]
    have = {(int(m), int(c), int(r)) for m, c, r in zip(a["ms_mkf"], a["ms_cam"], a["ms_row"])}
    keys, rows_used = [], set()
    for i in rng.permutation(M):
        if len(keys) >= n:
            break
        k = (int(a["ms_mkf"][i]), int(a["ms_cam"][i]), int(a["ms_row"][i]))
        if rng.random() < 0.08:                          # a key that nothing has
            k = [(1, 0, k[2]), (k[0], k[1], R + int(rng.integers(0, 3))), (k[0], k[1], -1), (k[0], (k[1] + 1) % C, k[2])][int(rng.integers(0, 4))]
            if k in have:
                continue
        if k in keys or (distinct_rows and k[2] in rows_used):
            continue
        keys.append(k)
        rows_used.add(k[2])
    assert len(keys) == n, (len(keys), n)
    return keys


def one_row_map(n_list=257):
    """Row 0 measured by 264 keyframes (264 MKFs, one camera), forty of them bad; n_list of its measurements are outliers.  The walk of that
    row is one thread's: REFIND and TRACKER entries die one after the other until list position 200 names the ROOT measurement."""
    n_mkfs = 264
    mf = np.full(n_mkfs, P, dtype=np.int32)
    mf[np.arange(3, n_mkfs, 7)[:40]] |= B
    src = [RF if k % 3 else T for k in range(n_mkfs)]
    rows = [dict(src=0, meas=[(k, 0, src[k]) for k in range(n_mkfs)])] + [dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T)]) for _ in range(1, 5)]
    rng = np.random.default_rng(264)
    order = rng.permutation(n_mkfs + 12)
    a = build(mf, 1, rows, order=order)
    listed = [int(k) for k in rng.permutation(np.arange(1, n_mkfs))[:n_list]]      # (slot 0 holds the row's ROOT measurement: kept for position 200)
    if n_list > 200:
        listed[200] = 0
        a["ms_source"][(a["ms_row"] == 0) & (a["ms_mkf"] == 0)] = RT
    return a, [(k, 0, 0) for k in listed]


def scattered_case():
    """Row 7's ten outliers at every seventh place of a list of 70; the rest on distinct rows."""
    a = random_map(70, 12, 2, 90, 90, per_row=(4, 9), dead_frac=0.0)
    a["pt_flags"][7], a["src_mkf"][7] = 0, int(np.flatnonzero(a["mkf_flags"] & P)[0])
    on7 = [(int(m), int(c), 7) for m, c, r in zip(a["ms_mkf"], a["ms_cam"], a["ms_row"]) if r == 7]
    assert len(on7) >= 4
    others = [k for k in random_keys(71, a, 80, distinct_rows=True) if k[2] != 7]
    keys = []
    for i in range(70):
        keys.append(on7[i // 7] if i % 7 == 0 and i // 7 < len(on7) else others.pop())
    return case("scattered_row", a, keys)


# ---- the order of the list ------------------------------------------------------------------------------------------------------------------------
def order_cases():
    mf = [P, P, P, P, P | B, P, 0, P]                     # slot 4 bad, slot 6 not in the map
    out = []
    four = [dict(src=0, meas=[(0, 0, RT), (1, 0, RF), (2, 0, RF), (3, 0, RF), (4, 0, T)])]      # good count 4: the bad MKF's entry does not count
    keys = [(1, 0, 0), (2, 0, 0), (3, 0, 0)]
    out.append(case("good4_three_refind", build(mf, 2, four), keys))                       # NEVER_RETRY, NEVER_RETRY, POINT_BAD
    out.append(case("good4_three_refind_reversed", build(mf, 2, four), keys[::-1]))
    six = [dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, EP), (3, 0, TR), (5, 0, RF), (7, 0, T), (1, 1, T), (2, 1, T)])]
    out.append(case("root_in_the_middle", build(mf, 2, six), [(1, 0, 0), (2, 0, 0), (0, 0, 0), (3, 0, 0), (5, 0, 0)]))      # RETRY, RETRY, POINT_BAD, ALREADY_BAD x 2
    three = [dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T)])]
    out.append(case("root_then_count_at_most_two", build(mf, 2, three), [(1, 0, 0), (0, 0, 0), (2, 0, 0)]))      # RETRY (3 -> 2), POINT_BAD, POINT_BAD
    out.append(case("good_exactly_2", build(mf, 2, [dict(src=0, meas=[(0, 0, RT), (1, 0, T)])]), [(1, 0, 0)]))      # POINT_BAD
    out.append(case("good_exactly_3", build(mf, 2, three), [(1, 0, 0), (2, 0, 0)]))                                   # RETRY, POINT_BAD
    badk = [dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T), (4, 0, T), (4, 1, T)])]
    out.append(case("outlier_of_a_bad_mkf", build(mf, 2, badk), [(4, 0, 0), (4, 1, 0), (1, 0, 0), (2, 0, 0)]))      # RETRY x 3 (the count stays 3, stays 3, drops to 2), POINT_BAD
    fixed = [dict(flags=mg.GP_FIXED, src=-1, meas=[(0, 0, T), (1, 0, T), (2, 1, T)]), dict(flags=mg.GP_FIXED, src=2, meas=[(3, 0, RT)]), dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T), (3, 0, T)])]
    out.append(case("fixed_row_named_twice", build(mf, 2, fixed), [(0, 0, 0), (1, 0, 2), (2, 1, 0)]))               # FIXED, RETRY, FIXED: one distinct fixed row
    miss = [dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T), (3, 0, T)]), dict(NEVER, meas=[(1, 0, T), (2, 0, T), (3, 0, T)]), dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T), (3, 0, T), (6, 0, T)])]      # (slot 6 left the map, its entry did not)
    a = build(mf, 2, miss, n_rows=5, dead=(2,))
    out.append(case("missing", a, [(5, 0, 0), (2, 0, 0), (1, 0, 1), (6, 0, 2), (1, 0, 4), (1, 0, 9), (1, 0, -1), (1, 0, 2)]))      # seven MISSING, then RETRY
    al = [dict(flags=mg.GP_BAD, src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T), (3, 0, T)]), dict(flags=mg.GP_BAD, src=0, meas=[(0, 0, RT), (1, 0, T)])]
    out.append(case("bad_by_the_host", build(mf, 2, al), [(1, 0, 0), (0, 0, 0), (1, 0, 1)]))                         # ALREADY_BAD, POINT_BAD (ROOT), POINT_BAD (count): none marked
    srcs = [dict(src=0, meas=[(0, 0, RT), (1, 0, T), (2, 0, T), (3, 0, T), (5, 0, s)]) for s in (T, RF, RT, TR, EP)]
    out.append(case("every_source", build(mf, 2, srcs), [(5, 0, r) for r in range(5)]))                              # RETRY, NEVER, POINT_BAD, NEVER, RETRY
    out.append(case("bad_good_count_3", build(mf, 2, four), keys, bad_good_count=3))                                 # NEVER_RETRY (4 -> 3), POINT_BAD, POINT_BAD (3 <= 3 comes before the bad flag)
    return out


# ---- the sweep's thresholds -----------------------------------------------------------------------------------------------------------------------
def _threshold_rows():
    ok = [(0, 0, RT), (1, 0, T), (2, 0, T)]
    rows = [dict(src=0, counts=(i, o), meas=ok) for o in (20, 21) for i in (20, 21, 22)]
    rows += [dict(src=0, counts=(14, 21), meas=ok), dict(src=0, counts=(14, 22), meas=ok), dict(src=0, counts=(1, 40), meas=ok)]
    rows += [dict(flags=mg.GP_FIXED, src=-1, counts=(1, 100), meas=[]), dict(flags=mg.GP_FIXED, src=0, counts=(1, 100), meas=[(0, 0, RT)])]      # exempt from both rules
    rows += [dict(src=0, counts=(30, 0), meas=[(0, 0, RT)]), dict(src=0, counts=(30, 0), meas=[]), dict(src=0, counts=(1, 40), meas=[(0, 0, RT)])]  # danglers (the last one by both rules)
    rows += [dict(src=0, counts=(30, 0), meas=[(0, 0, RT), (3, 0, T)])]                                            # one measurement from a bad MKF: good count 1
    return rows


def sweep_cases():
    out = []
    two, one, good_bad = [P, P, P, P | B], [P], [P, 0, 0, P | B]
    out.append(case("thresholds_mult_1", build(two, 1, _threshold_rows())))
    out.append(case("thresholds_mult_1p5", build(two, 1, _threshold_rows()), sweep=dict(outlier_multiplier=1.5)))
    out.append(case("thresholds_min_0", build(two, 1, _threshold_rows()), sweep=dict(min_outliers=0, outlier_multiplier=0.0)))
    out.append(case("danglers_off", build(two, 1, _threshold_rows()), sweep=dict(danglers=False)))
    single = [dict(src=0, counts=(30, 0), meas=[(0, 0, RT)]), dict(src=0, counts=(30, 0), meas=[]), dict(src=0, counts=(1, 40), meas=[(0, 0, RT)])]
    out.append(case("one_mkf_present", build(one, 1, single)))                                                      # the dangler rule is off; the tracker rule is not
    gb = [dict(src=0, counts=(30, 0), meas=[(0, 0, RT), (3, 0, T)]), dict(src=0, counts=(30, 0), meas=[(0, 0, RT)])]
    out.append(case("one_good_one_bad_mkf", build(good_bad, 1, gb)))                                                # present count 2: both rows dangle
    return out


# ---- the report and the store at their seams -----------------------------------------------------------------------------------------------------
def report_cases():
    out = []
    mf = [P, P, P]
    ok = [(0, 0, RT), (1, 0, T), (2, 0, T)]
    for n in ROW_SIZES:
        out.append(case("rows%d_none" % n, build(mf, 1, [dict(src=0, meas=ok) for _ in range(n)])))
        out.append(case("rows%d_all" % n, build(mf, 1, [dict(src=0, meas=[(0, 0, RT)]) for _ in range(n)])))
        out.append(case("rows%d_last" % n, build(mf, 1, [dict(src=0, meas=ok) for _ in range(n - 1)] + [dict(src=0, counts=(1, 50), meas=ok)])))
        a = random_map(900 + n, 9, 2, n, n + 40, per_row=(0, 5))                    # graph columns shorter than the table
        out.append(case("rows%d_mixed" % n, a, random_keys(901 + n, a, 65)))
    for m in STORE_SIZES:
        rows = [dict(src=0, meas=[(k % 3, k // 3 % 2, RT if k % 3 == 0 else T) for k in range(min(6, m - 6 * i))]) for i in range((m + 5) // 6)]
        a = build(mf, 2, rows, dead=tuple(range(0, m, 5)) if m > 1 else ())
        assert len(a["ms_mkf"]) == m
        keys = [(int(a["ms_mkf"][i]), int(a["ms_cam"][i]), int(a["ms_row"][i])) for i in range(0, m, 4)]
        out.append(case("store%d" % m, a, keys))
    return out


def list_cases():
    out = []
    for n in LIST_SIZES:
        a = random_map(100 + n, 10, 3, 300, 310, per_row=(3, 8))
        out.append(case("list%d_distinct_rows" % n, a, random_keys(200 + n, a, n, distinct_rows=True)))
        a = random_map(300 + n, 7, 2, 120, 120, per_row=(2, 9))
        out.append(case("list%d" % n, a, random_keys(400 + n, a, n)))
    a, keys = one_row_map(257)
    out.append(case("one_row_257", a, keys))
    a, keys = one_row_map(64)
    out.append(case("one_row_64", a, keys))
    out.append(scattered_case())
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = list_cases() + order_cases() + sweep_cases() + report_cases()
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


# ---- one turn of a case in numpy, by the host twins, and their comparison ----------------------------------------------------------------------------
def turn(c, outliers, sweep):
    """outliers, then the sweep, then a second sweep, by the given pair of functions: the results and the arrays after each step."""
    a = c["a"]
    r1, vd, a1 = outliers(a, c["mkf"], c["cam"], c["row"], c["bad_good_count"], n_rows=a["n_rows"])
    r2, rows, a2 = sweep(a1, n_rows=a["n_rows"], **c["sweep"])
    r3, rows3, a3 = sweep(a2, n_rows=a["n_rows"], **c["sweep"])
    return dict(r1=r1, vd=vd, a1=a1, r2=r2, rows=rows, a2=a2, r3=r3, rows3=rows3, a3=a3)


_REF = {}


def ref(c):
    """The numpy restatement's turn of a case, computed once."""
    if c["name"] not in _REF:
        _REF[c["name"]] = turn(c, mg.cull_outliers_ref, mg.cull_sweep_ref)
    return _REF[c["name"]]


STATE = ("pt_flags", "pending", "usable", "ms_alive")


def same_turn(x, y):
    for k in ("r1", "r2", "r3"):
        assert x[k] == y[k], (k, x[k], y[k])
    for k in ("vd", "rows", "rows3"):
        assert x[k].dtype == y[k].dtype and x[k].tobytes() == y[k].tobytes(), k
    for s in ("a1", "a2", "a3"):
        for k in STATE:
            assert x[s][k].dtype == y[s][k].dtype and x[s][k].tobytes() == y[s][k].tobytes(), (s, k)
