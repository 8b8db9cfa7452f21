"""What the map maker does with an adjustment's outliers and with bad points (HandleOutliers, then the point half of HandleBadEntities), two ways,
on the metric map (200 MKFs, 50k rows, 400k store entries) with 2 000 outliers and about 500 rows for the sweep to turn bad:
  (a) the route through the calls that existed before: mcp_map_graph_good_counts read back (map-sized), the verdicts decided on the host in
      numpy, mcp_map_graph_update_points + mcp_map_graph_erase_meas; then good counts and mcp_map_points_get_counts read back (map-sized), the
      sweep decided in numpy, update_points + erase_meas again;
  (b) mcp_map_cull_outliers + mcp_map_cull_sweep.
Both leave the same store and the same point flags (checked once, before timing; (a) does not touch the table's usable column, (b) clears it for
the bad rows).  Every turn starts from fresh graphs loaded outside the timed region.  Wall time around each route, alternating which goes first:
10 warm-up turns, then the median and the inter-quartile range of 50; the device times are mcp_map_cull_last_timing's.  Prints one JSON line.
  bench_cull.py [turns] [warmup]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _stats(ts, unit=1e3):
    q = statistics.quantiles(ts, n=4)
    return {"median_ms": statistics.median(ts) * unit, "q1_ms": q[0] * unit, "q3_ms": q[2] * unit, "iqr_ms": (q[2] - q[0]) * unit, "min_ms": min(ts) * unit, "max_ms": max(ts) * unit}


def main(turns=50, warmup=10, n_outliers=2000, n_bad=500):
    from mcptam_amd import map_graph as mg
    from mcptam_amd import synth
    from mcptam_amd.pvs import MapPointTable
    p = synth.make_config("metric")
    a = mg.problem_arrays(p)
    N, M = p.n_points, p.n_meas
    rng = np.random.default_rng(11)
    # sources as a map maker leaves them: the ROOT measurement from problem_arrays, the others from the tracker, ReFind or the epipolar search
    other = rng.choice([mg.SRC_TRACKER, mg.SRC_REFIND, mg.SRC_EPIPOLAR], size=M).astype(np.int32)
    a["ms_source"] = np.where(a["ms_source"] == mg.SRC_ROOT, mg.SRC_ROOT, other).astype(np.int32)
    inl, outl = rng.integers(5, 40, N).astype(np.int32), rng.integers(0, 5, N).astype(np.int32)
    marked = rng.choice(N, size=n_bad, replace=False)
    outl[marked] = 60                                    # the rows MarkOutliersAsBad takes
    usable = np.ones(N, dtype=np.uint8)
    pick = rng.choice(M, size=n_outliers, replace=False)
    k_mkf, k_cam, k_row = (np.ascontiguousarray(a[c][pick]) for c in ("ms_mkf", "ms_cam", "ms_row"))
    t = MapPointTable()
    z = np.zeros((N, 3))
    t.set(a["world_pos"], z, z, usable)
    t.set_counts(inl, outl)
    mkf_ok = ((a["mkf_flags"] & mg.MKF_PRESENT) != 0) & ((a["mkf_flags"] & mg.MKF_BAD) == 0)
    fixed = (a["pt_flags"] & mg.GP_FIXED) != 0
    order = np.argsort(k_row, kind="stable")             # the list grouped by row, list order kept within a row
    heads = np.r_[True, np.diff(k_row[order]) != 0]
    single = np.zeros(n_outliers, dtype=bool)
    single[order[heads & np.r_[heads[1:], True]]] = True
    several = [order[s:e] for s, e in zip(np.flatnonzero(heads), np.r_[np.flatnonzero(heads)[1:], n_outliers]) if e - s > 1]

    def fresh():
        g = mg.MapGraph(t, a["cam_from_base"])
        g.load_arrays(a)
        g.num_meas()                                     # (waits: the timed region starts on an idle stream)
        return g

    def route_a(g):
        """The host's own copies: flags, alive, sources (the adapter has them in its MapPoint / Measurement objects)."""
        flags, alive = a["pt_flags"].copy(), a["ms_alive"].copy()
        good = g.good_counts()
        src, ok = a["ms_source"][pick], mkf_ok[k_mkf]
        vd = np.full(n_outliers, mg.CULL_ALREADY_BAD, dtype=np.uint8)
        # rows named once: the first verdict that applies, all at once
        s = single
        fx, bad = fixed[k_row], (flags[k_row] & mg.GP_BAD) != 0
        pb = ~fx & ((good[k_row] <= 2) | (src == mg.SRC_ROOT))
        retry = (src == mg.SRC_TRACKER) | (src == mg.SRC_EPIPOLAR)
        vd[s & fx] = mg.CULL_FIXED
        vd[s & pb] = mg.CULL_POINT_BAD
        vd[s & ~fx & ~pb & ~bad] = np.where(retry, mg.CULL_RETRY, mg.CULL_NEVER_RETRY)[s & ~fx & ~pb & ~bad]
        # rows named several times: in list order, the count re-read after every erasure
        for run in several:
            r = int(k_row[run[0]])
            gcount, isbad = int(good[r]), bool(flags[r] & mg.GP_BAD)
            for i in run:
                if fixed[r]:
                    vd[i] = mg.CULL_FIXED
                elif gcount <= 2 or src[i] == mg.SRC_ROOT:
                    vd[i], isbad = mg.CULL_POINT_BAD, True
                elif not isbad:
                    vd[i] = mg.CULL_RETRY if retry[i] else mg.CULL_NEVER_RETRY
                    gcount -= int(ok[i])
        went_bad = np.unique(k_row[vd == mg.CULL_POINT_BAD])
        went_bad = went_bad[(flags[went_bad] & mg.GP_BAD) == 0]
        flags[went_bad] |= mg.GP_BAD
        died = (vd == mg.CULL_RETRY) | (vd == mg.CULL_NEVER_RETRY)
        if len(went_bad):
            g.update_points(went_bad, a["src_mkf"][went_bad], a["src_cam"][went_bad], flags[went_bad])
        if died.any():
            g.erase_meas(k_mkf[died], k_cam[died], k_row[died])
            alive[pick[died]] = 0
        # the sweep
        good = g.good_counts()
        i_, o_ = t.get_counts()
        nb = (flags & mg.GP_BAD) == 0
        dang = nb & ~fixed & (good < 2)
        trk = nb & ~dang & ~fixed & (o_ > 20) & (o_.astype(np.float64) > i_.astype(np.float64) * 1.0)
        new = np.flatnonzero(dang | trk)
        flags[new] |= mg.GP_BAD
        if len(new):
            g.update_points(new, a["src_mkf"][new], a["src_cam"][new], flags[new])
        gone = np.flatnonzero((alive != 0) & ((flags[a["ms_row"]] & mg.GP_BAD) != 0))
        if len(gone):
            g.erase_meas(a["ms_mkf"][gone], a["ms_cam"][gone], a["ms_row"][gone])
        return vd, np.union1d(went_bad, new)

    def route_b(g):
        _, vd = g.cull_outliers(k_mkf, k_cam, k_row)
        _, rows = g.cull_sweep()
        return vd, rows

    ga, gb = fresh(), fresh()
    (va, ra), (vb, rb) = route_a(ga), route_b(gb)
    sa, sb = ga.get_meas(), gb.get_meas()
    assert va.tobytes() == vb.tobytes() and np.array_equal(ra, rb) and all(sa[f].tobytes() == sb[f].tobytes() for f in sa) and ga.num_meas() == gb.num_meas(), "the two routes disagree"
    S = mg.select_params(mode=mg.BUNDLE_ALL)
    xa, xb = ga.select_raw(S), gb.select_raw(S)
    assert bytes(xa[0]) == bytes(xb[0]) and all(u.tobytes() == v.tobytes() for u, v in zip(xa[1:], xb[1:])), "the selections after the two routes disagree"
    n_bad_rows = len(rb)
    ga.close(); gb.close()
    ta, tb, dev_o, dev_s = [], [], [], []
    for i in range(warmup + turns):
        t.set(a["world_pos"], z, z, usable)              # (route (b) cleared the usable bytes of the bad rows)
        ga, gb = fresh(), fresh()
        pair = ((route_a, ga, ta), (route_b, gb, tb))
        for fn, g, acc in (pair if i % 2 == 0 else pair[::-1]):
            t0 = time.perf_counter(); fn(g); dt = time.perf_counter() - t0
            if i >= warmup:
                acc.append(dt)
        if i >= warmup:
            o, s_ = gb.cull_last_timing()
            dev_o.append(o * 1e-3); dev_s.append(s_ * 1e-3)
        ga.close(); gb.close()
    A, B = _stats(ta), _stats(tb)
    gap = A["median_ms"] - B["median_ms"]
    res = {"bench": "cull", "n_mkf": p.n_mkf, "rows": N, "store": M, "outliers": n_outliers, "rows_turned_bad": n_bad_rows, "turns": turns, "warmup": warmup,
           "verdicts": np.bincount(vb, minlength=6).tolist(), "a_read_back_numpy_upload": A, "b_two_calls": B, "a_minus_b_ms": gap,
           "within_spread_of_a": bool(abs(gap) <= A["iqr_ms"]), "device_outliers": _stats(dev_o), "device_sweep": _stats(dev_s)}
    print(json.dumps(res))
    t.close()
    return res


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
