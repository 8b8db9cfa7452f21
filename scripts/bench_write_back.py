"""BundleAdjusterMulti::AdjustAndUpdate's write-back at the headline map (`metric`: 200 MKF x 4 cameras = 800 keyframes, 50 k points, the lists
of its 400 k measurements): one mcp_ba_write_back after a solve against the host composition of the calls that existed before it --
mcp_ba_get_points / _get_poses, the numpy point step (mcptam_amd.pvs.write_back_points), mcp_map_points_update, and RefreshSceneDepthRobust
per keyframe with np.sort.  The two are timed alternately in one run (median of `reps`), after a check that they agree.  Also: the device spans
of the one-call path from HIP events on the table's stream, and the share of HBM bandwidth the point kernel reaches on its algorithmic bytes
(per point 24 B state + 72 B rays in, 80 B row + 72 B vectors out).  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_PEAK = 8.0e12          # bytes / s, MI355X
POINT_BYTES = 24 + 72 + 80 + 72


def _rays(rng, n):
    c = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.7, 0.7, n), np.ones(n)], axis=1)
    px = 1.0 / rng.uniform(250.0, 400.0, n)
    z = np.zeros(n)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    return unit(c), unit(c + np.stack([px, z, z], axis=1)), unit(c + np.stack([z, px, z], axis=1))


def _scene_depth_host(d, w):
    """RefreshSceneDepthRobust of one list with numpy (np.sort twice, as the reference sorts twice)."""
    n = len(d)
    if n <= 3:
        return None
    order = np.lexsort((w, d))
    d, w = d[order], w[order]
    med = d[n // 2]
    e2 = (d - med) * (d - med)
    m2 = np.sort(e2)[n // 2]
    sg = 1.345 * (1.4826 * (1 + 5.0 / (n * 2 - 6)) * np.sqrt(m2))
    s2 = max(sg * sg, 0.4)
    hw = np.sqrt(np.where(e2 < s2, 1.0, np.sqrt(s2 / np.maximum(e2, 1e-300))))
    cw = w * hw
    s0 = cw.sum()
    mean = (cw * d).sum() / s0
    return mean, np.sqrt((cw * d * d).sum() / s0 - mean * mean), med, s2


def main(config="metric", iters=20, reps=15, seed=5):
    from mcptam_amd import chain_bundle, synth
    from mcptam_amd.pvs import MapPointTable, _mat3_vec, write_back_points
    p = synth.make_config(config)
    assert p.mode == "multi"
    b = chain_bundle.ChainBundle(p.cams, True, True, False)
    ids = p.populate(b)
    rc = b.Compute(iters)
    N, P, C = p.n_points, p.n_mkf, len(p.cams)
    rng = np.random.default_rng(seed)
    rows = rng.permutation(N).astype(np.int32)
    ce, ri, dn = _rays(rng, N)
    # keyframe (k, c) = index k * C + c; its list: the rows of the points it measures, weights = inlier ratios
    kf_chains = np.stack([np.repeat(ids["mkf"], C), np.tile(ids["cam"], P)], axis=1).astype(np.int32)
    kf_len = np.full(P * C, 2, dtype=np.int32)
    kf_of_meas = p.ms_mkf.astype(np.int64) * C + p.ms_cam
    order = np.argsort(kf_of_meas, kind="stable")
    seg_rows = rows[p.ms_pt[order]].astype(np.int32)
    seg_start = np.concatenate([[0], np.cumsum(np.bincount(kf_of_meas, minlength=P * C))]).astype(np.int32)
    seg_w = rng.uniform(0.3, 1.0, len(seg_rows))
    seg_kf = np.repeat(np.arange(P * C), np.diff(seg_start))
    pt_kf = p.pt_src[:, 0].astype(np.int64) * C + p.pt_src[:, 1]
    init = (rng.normal(size=(N, 3)), rng.normal(size=(N, 3)) * 0.01, rng.normal(size=(N, 3)) * 0.01, np.zeros(N, dtype=np.uint8))

    def table():
        t = MapPointTable()
        t.set(*init)
        t.set_rays(ce, ri, dn)
        return t
    ta, tb = table(), table()
    ones = np.ones(N, dtype=np.uint8)

    def one_call():
        return ta.write_back(b, ids["point"], rows, kf_chains=kf_chains, kf_chain_len=kf_len, seg_start=seg_start, seg_rows=seg_rows, seg_weights=seg_w)

    def host():
        X = b.GetPoints(ids["point"])
        bR, bt = b.GetPoses(ids["mkf"])
        cR, ct = b.GetPoses(ids["cam"])
        kR = np.einsum("cij,kjl->kcil", cR, bR).reshape(P * C, 3, 3)                  # CamFromBase * BaseFromWorld
        kt = (np.einsum("cij,kj->kci", cR, bt) + ct[None]).reshape(P * C, 3)
        world, pr, pd = write_back_points(X, kR[pt_kf], kt[pt_kf], p.pt_fixed, ce[rows], ri[rows], dn[rows])
        tb.update(rows, world, pr, pd, ones)
        wp = np.empty((N, 3)); wp[rows] = world                                      # the host's MapPoints (every row is in the bundle here)
        xc = _mat3_vec(kR[seg_kf], wp[seg_rows]) + kt[seg_kf]
        dep = np.sqrt(xc[:, 0] * xc[:, 0] + xc[:, 1] * xc[:, 1] + xc[:, 2] * xc[:, 2])
        sd = [_scene_depth_host(dep[seg_start[j]:seg_start[j + 1]], seg_w[seg_start[j]:seg_start[j + 1]]) for j in range(P * C)]
        return world, pr, pd, sd, dep

    # warm-up (code objects, buffers at their final sizes) and agreement of the two paths at the size that is timed
    for _ in range(3):
        res = one_call()
        ref = host()
    ga, gb = ta.get(), tb.get()
    agree = [float(np.abs(ga[k] - gb[k]).max() / np.abs(gb[k]).max()) for k in range(3)]
    assert max(agree) <= 1e-12, agree
    dep_rel = float((np.abs(res["seg_depths"] - ref[4]) / ref[4]).max())
    means = np.array([s[0] if s else np.nan for s in ref[3]])
    ok = res["depth"]["refreshed"] == 1
    mean_rel = float(np.nanmax(np.abs(res["depth"]["mean"][ok] - means[ok]) / means[ok]))
    assert dep_rel <= 1e-12 and mean_rel <= 1e-9, (dep_rel, mean_rel)
    t_one, t_host, spans = [], [], []
    for _ in range(reps):                                                            # alternating: both see the same machine
        t0 = time.perf_counter(); one_call(); t1 = time.perf_counter(); host(); t2 = time.perf_counter()
        t_one.append((t1 - t0) * 1e3); t_host.append((t2 - t1) * 1e3)
        spans.append(ta.last_timing())
    med = statistics.median
    sp = {k: med([s[k] for s in spans]) for k in ("copy", "points", "depth")}
    lens = np.diff(seg_start)
    out = {"metric": "AdjustAndUpdate write-back, %s map" % config, "points": N, "keyframes": P * C, "list_entries": int(len(seg_rows)),
           "list_len_median": int(np.median(lens)), "list_len_max": int(lens.max()), "solve_rc": int(rc), "reps": reps,
           "one_call_ms_median": med(t_one), "one_call_ms_min": min(t_one), "one_call_ms_max": max(t_one),
           "host_composition_ms_median": med(t_host), "host_composition_ms_min": min(t_host), "host_composition_ms_max": max(t_host),
           "speedup": med(t_host) / med(t_one),
           "device_ms_median": {"input_copy": sp["copy"], "chains_and_points": sp["points"], "scene_depth": sp["depth"], "span": sum(sp.values())},
           "point_kernel_algorithmic_bytes": N * POINT_BYTES,
           "point_kernel_hbm_fraction": N * POINT_BYTES / (sp["points"] * 1e-3) / HBM_PEAK if sp["points"] > 0 else None,
           "agreement": {"rows_max_rel": max(agree), "depths_max_rel": dep_rel, "mean_max_rel": mean_rel},
           "note": "one_call: MapPointTable.write_back (host-observed, ends in the call's own wait).  host_composition: get_points + get_poses + numpy "
                   "point step + mcp_map_points_update (enqueue only: its completion is not waited for) + per-keyframe scene depth with np.sort.  "
                   "chains_and_points includes the 64-lane chain-table launch; hbm fraction = algorithmic bytes over that span over %.1f TB/s." % (HBM_PEAK / 1e12)}
    ta.close(); tb.close(); b.close()
    return out


if __name__ == "__main__":
    print(json.dumps(main()))
