"""The closest-keyframe queries and the removal of an MKF on the metric map (200 MKFs x 4 cameras, 50k rows, 400k store entries), each two ways:
  (device) mcp_map_neighbours / mcp_map_mkf_cull over the resident graph: one submission, at most 32 items back;
  (host)   what an adapter without them pays: the columns the answer needs read back from the graph (mcp_graph_get_mkfs; for the measurement
           counts and the removal the store as well, mcp_map_graph_get_meas), then the host twin (mcp_map_neighbours_host /
           mcp_map_mkf_cull_host: the same bodies under the host compiler).
Three calls: the keyframe query behind AddStereoMapPoints (KF kind, n_max 5, from the newest MKF's first camera), the MKF query of
NeedNewMultiKeyFrame(mkf, nNumMeas) (MKF kind from an external MKF, n_max 3, want_meas), and MarkFurthestMultiKeyFrameAsBad with the erase
(slot -1, furthest from the newest).  A check first that device and host give the same bytes.  Wall time around each route, alternating which
goes first, warm-up turns, then the median and the inter-quartile range; device times from mcp_map_neighbours_last_timing /
mcp_map_mkf_cull_last_timing.  The removal changes the map, so each of its turns starts from a fresh graph loaded outside the timed region.
Prints one JSON line.
  bench_neighbours.py [turns] [warmup] [cull_turns]"""
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


def main(turns=200, warmup=20, cull_turns=20):
    from mcptam_amd import map_graph as mg
    from mcptam_amd import synth
    from mcptam_amd.pvs import MapPointTable
    p = synth.make_config("metric")
    a = mg.problem_arrays(p)
    N, M, P = p.n_points, p.n_meas, p.n_mkf
    a["n_rows"] = N
    newest = P - 1
    t = MapPointTable()
    z = np.zeros((N, 3))
    t.set(a["world_pos"], z, z, np.ones(N, dtype=np.uint8))

    def fresh():
        g = mg.MapGraph(t, a["cam_from_base"])
        g.load_arrays(a)
        g.num_meas()                                     # (waits: the timed region starts on an idle stream)
        return g

    def columns(g, store):
        """The host's copy of what the twins read, fetched from the graph."""
        k = g.get_mkfs(0, P)
        b = dict(a, base_from_world=k["base_from_world"], mkf_flags=k["flags"], kf_active=k["kf_active"], kf_depth_mean=k["kf_depth_mean"])
        if store:
            s = g.get_meas()
            b.update(ms_mkf=s["mkf"], ms_cam=s["cam"], ms_row=s["row"], ms_alive=s["alive"])
        return b
    ext = dict(base_from_world=a["base_from_world"][newest].copy(), kf_active=a["kf_active"][newest].copy(), kf_depth_mean=a["kf_depth_mean"][newest].copy())
    ext["base_from_world"][9:] += 0.05
    q_kf = mg.neigh_params(kind=mg.NB_KF, src_slot=newest, src_cam=0, n_max=5, max_dist=1000.0)
    q_mkf = mg.neigh_params(kind=mg.NB_MKF, src_slot=-1, ext=ext, n_max=3, want_meas=True)
    g = fresh()
    out = {"map": {"mkfs": P, "cams": int(a["ncam"]), "rows": N, "store": M}, "turns": turns, "warmup": warmup, "cull_turns": cull_turns}
    for name, q, store in (("kf_query_n5", q_kf, False), ("mkf_query_n3_meas", q_mkf, True)):
        dev = lambda: g.neighbours(q, raw=True)
        host = lambda: mg.neighbours_host(columns(g, store), q, raw=True)
        assert bytes(dev()) == bytes(host()), name + ": device and host disagree"
        td, th, tk = [], [], []
        for i in range(warmup + turns):
            pair = ((dev, td), (host, th))
            for fn, acc in (pair if i % 2 == 0 else pair[::-1]):
                t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
                if i >= warmup:
                    acc.append(dt)
                if fn is dev and i >= warmup:
                    tk.append(g.neighbours_last_timing() * 1e-3)
        r = dev()
        out[name] = {"device_wall": _stats(td), "device_events": _stats(tk), "host_with_read_back": _stats(th), "count": int(r.count), "n_candidates": int(r.n_candidates)}
    g.close()
    # the removal: fresh graphs every turn
    k = dict(slot=-1, furthest_from=newest, mark_points=True, max_kfs=2, erase=True)
    ga, gb = fresh(), fresh()
    ra, rb = ga.cull_mkf(**k), mg.cull_mkf_host(columns(gb, True), **k)[0]
    assert ra == rb and ra["status"] == 0, "the removal: device and host disagree"
    ga.close(); gb.close()
    td, th, tk = [], [], []
    for i in range(3 + cull_turns):
        ga, gb = fresh(), fresh()
        dev, host = (lambda: ga.cull_mkf(**k)), (lambda: mg.cull_mkf_host(columns(gb, True), **k))
        pair = ((dev, td), (host, th))
        for fn, acc in (pair if i % 2 == 0 else pair[::-1]):
            t0 = time.perf_counter(); fn(); dt = time.perf_counter() - t0
            if i >= 3:
                acc.append(dt)
        if i >= 3:
            tk.append(ga.cull_mkf_last_timing() * 1e-3)
        ga.close(); gb.close()
    out["cull_mkf_furthest_erase"] = {"device_wall": _stats(td), "device_events": _stats(tk), "host_with_read_back": _stats(th), "result": ra}
    print(json.dumps(out))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
