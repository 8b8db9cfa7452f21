"""The one-call bundle selection (mcp_map_bundle_select) over the device-resident map graph at the metric (200 MKFs, 50k points, 400k
measurements) and c4 (500 MKFs, 100k points, 800k measurements) maps, BundleAdjustRecent and BundleAdjustAll:
  device   the select's submission between two events on the table's stream (mcp_map_bundle_select_last_timing)
  wall     the call as the host sees it, views in the pinned block (nothing copied)
  host     mcp_map_bundle_select_host on the same box: the same bodies under the host compiler over flat host arrays
  numpy    bundle_select_ref on the same box
Medians of alternating rounds with [min, max].  The host figures are NOT the reference's set walks (std::set / std::map of pointers cannot be
built here); they are the flat-array floor a host population could reach.  Prints one JSON line.
  bench_bundle_select.py [metric|c4|both] [rounds]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


def bench_map(name, rounds):
    from mcptam_amd import map_graph as mg
    from mcptam_amd import synth
    from mcptam_amd.pvs import MapPointTable
    p = synth.make_config(name)
    a = mg.problem_arrays(p)
    t = MapPointTable()
    g = mg.MapGraph.from_problem(t, p, arrays=a)
    out = {"n_mkf": p.n_mkf, "n_points": p.n_points, "n_meas": p.n_meas}
    for mode, S in (("recent", mg.select_params(mg.BUNDLE_RECENT, p.n_mkf - 1)), ("all", mg.select_params(mg.BUNDLE_ALL))):
        dev = g.select_raw(S, copy=True)
        host = mg.bundle_select_host(a, S)
        assert bytes(dev[0]) == bytes(host[0]) and all(x.tobytes() == y.tobytes() for x, y in zip(dev[1:], host[1:])), "device and host selections differ"
        for _ in range(3):
            g.select_raw(S, copy=False)
        T = {"device": [], "wall": [], "host": [], "numpy": []}
        for _ in range(rounds):
            t0 = time.perf_counter(); g.select_raw(S, copy=False); T["wall"].append(time.perf_counter() - t0)
            T["device"].append(g.last_timing() * 1e-3)
            t0 = time.perf_counter(); mg.bundle_select_host(a, S); T["host"].append(time.perf_counter() - t0)
            t0 = time.perf_counter(); mg.bundle_select_ref(a, S); T["numpy"].append(time.perf_counter() - t0)
        r = dev[0]
        out[mode] = {"status": r.status, "n_adjust": r.n_adjust, "n_fixed": r.n_fixed, "n_points": r.n_points, "n_meas": r.n_meas,
                     **{k: _stats(v) for k, v in T.items()}}
    g.close(); t.close()
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "both"
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    maps = ["metric", "c4"] if which == "both" else [which]
    res = {"bench": "bundle_select", "rounds": rounds}
    for m in maps:
        res[m] = bench_map(m, rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
