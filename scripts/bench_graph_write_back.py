"""AdjustAndUpdate's write-back with the keyframe lists built on the device (mcp_graph_write_back) against the path it replaces, at the
metric map (200 MKFs x 4 cameras = 800 keyframes, 50 k points, 400 k measurements) and at the small map c2 (50 x 4, 10 k points, 80 k):
  (a) what an adapter did before: the keyframe-major lists grouped on the host by a stable numpy sort of its copy of the store (inside the
      timed region: they change with every map update), mcp_ba_write_back with them, then the adjusted poses read back and pushed into the
      graph with mcp_map_graph_update_mkfs together with the new depth means;
  (b) the one call on the graph.
Host-observed milliseconds, medians with [min, max] over `reps` alternating pairs, after a check that both leave the same bytes in the table,
the depth records and the graph.  `device_ms` are the spans mcp_map_points_last_timing reports for each path.

  python scripts/bench_graph_write_back.py [reps]          one JSON line, both maps
  python scripts/bench_graph_write_back.py trace [map]     the kernel split of (b) from a rocprofv3 --kernel-trace --stats run of its own"""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

KERNELS = ("k_wb_chains", "k_wb_points", "k_mgl_pose_store", "k_mgl_count", "k_mgl_scan", "k_mgl_scatter", "k_wb_scene_depth", "k_mgl_depth_store")


def _rays(rng, n):
    c = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(-0.7, 0.7, n), np.ones(n)], axis=1)
    px = 1.0 / rng.uniform(250.0, 400.0, n)
    z = np.zeros(n)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    return unit(c), unit(c + np.stack([px, z, z], axis=1)), unit(c + np.stack([z, px, z], axis=1))


class Setup:
    """One solved bundle of `config`, and two (table, graph) sides holding its map: rows = point indices, slots = MKF indices."""

    def __init__(self, config, iters=20, seed=5):
        from mcptam_amd import chain_bundle, synth
        from mcptam_amd import map_graph as mg
        from mcptam_amd.pvs import MapPointTable
        self.mg = mg
        p = self.p = synth.make_config(config)
        assert p.mode == "multi"
        self.b = chain_bundle.ChainBundle(p.cams, True, True, False)
        self.ids = p.populate(self.b)
        self.rc = self.b.Compute(iters)
        N, P, C = p.n_points, p.n_mkf, len(p.cams)
        rng = np.random.default_rng(seed)
        a = self.a = mg.problem_arrays(p)
        cR, ct = self.b.GetPoses(self.ids["cam"])
        a["cam_from_base"] = mg.poses12(cR, ct)                                     # the contract: the graph's rig is the solver's
        a["inlier"], a["outlier"] = rng.integers(1, 60, N).astype(np.int32), rng.integers(0, 20, N).astype(np.int32)
        rays = _rays(rng, N)
        init = (a["world_pos"], rng.normal(size=(N, 3)) * 0.01, rng.normal(size=(N, 3)) * 0.01, np.ones(N, dtype=np.uint8))
        self.sides = []
        for _ in range(2):
            t = MapPointTable()
            t.set(*init); t.set_rays(*rays); t.set_counts(a["inlier"], a["outlier"])
            g = mg.MapGraph(t, a["cam_from_base"])
            g.load_arrays(a)
            self.sides.append((t, g))
        self.rows = np.arange(N, dtype=np.int32)
        self.slots = np.arange(P, dtype=np.int32)
        self.kf_chains = np.stack([np.repeat(self.ids["mkf"], C), np.tile(self.ids["cam"], P)], axis=1).astype(np.int32)
        self.kf_len = np.full(P * C, 2, dtype=np.int32)
        self.N, self.P, self.C = N, P, C

    def old(self):
        """(a)"""
        t, g = self.sides[0]
        a, mg = self.a, self.mg
        ss, sr, sw = mg.kf_lists_ref(a, self.slots)
        res = t.write_back(self.b, self.ids["point"], self.rows, kf_chains=self.kf_chains, kf_chain_len=self.kf_len, seg_start=ss, seg_rows=sr, seg_weights=sw)
        bR, bt = self.b.GetPoses(self.ids["mkf"])
        sd = res["depth"].reshape(self.P, self.C)
        dep = np.where(sd["refreshed"] == 1, sd["mean"], a["kf_depth_mean"])
        g.update_mkfs(self.slots, mg.poses12(bR, bt), a["mkf_flags"], a["kf_active"], dep)
        a["kf_depth_mean"] = dep                                                    # (the adapter's copy follows, as the graph's does)
        return res

    def new(self):
        """(b)"""
        t, g = self.sides[1]
        return g.write_back(self.b, self.ids["point"], self.rows, slots=self.slots, mkf_pose_ids=self.ids["mkf"], cam_pose_ids=self.ids["cam"])

    def close(self):
        for t, g in self.sides:
            g.close(); t.close()
        self.b.close()


def _same(s, ra, rb):
    (ta, ga), (tb, gb) = s.sides
    cols = lambda t: b"".join(np.ascontiguousarray(c).tobytes() for c in t.get())
    assert cols(ta) == cols(tb), "the two paths leave different table rows"
    for k in ("world_pos", "pixel_right_w", "pixel_down_w", "kf_cam_from_world", "depth"):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    ma, mb = ga.get_mkfs(0, s.P), gb.get_mkfs(0, s.P)
    for k in ma:
        assert ma[k].tobytes() == mb[k].tobytes(), "the graphs differ in " + k


def run(config, reps):
    s = Setup(config)
    for _ in range(3):                                                              # code objects, buffers at their final sizes
        ra, rb = s.old(), s.new()
    _same(s, ra, rb)
    t_old, t_new, d_old, d_new = [], [], [], []
    for _ in range(reps):                                                           # alternating: both see the same machine
        t0 = time.perf_counter(); s.old(); t1 = time.perf_counter()
        d_old.append(s.sides[0][0].last_timing())
        t2 = time.perf_counter(); s.new(); t3 = time.perf_counter()
        d_new.append(s.sides[1][0].last_timing())
        t_old.append((t1 - t0) * 1e3); t_new.append((t3 - t2) * 1e3)
    med = statistics.median
    span = lambda ds: {k: med([d[k] for d in ds]) for k in ("copy", "points", "depth")}
    lens = np.diff(s.mg.kf_lists_ref(s.a, s.slots)[0])
    out = {"map": config, "points": s.N, "mkfs": s.P, "keyframes": s.P * s.C, "store_entries": int(len(s.a["ms_mkf"])), "list_entries": int(lens.sum()),
           "list_len_median": int(np.median(lens)), "list_len_max": int(lens.max()), "solve_rc": int(s.rc), "reps": reps,
           "host_lists_ms": {"median": med(t_old), "min": min(t_old), "max": max(t_old)},
           "one_call_ms": {"median": med(t_new), "min": min(t_new), "max": max(t_new)},
           "ratio_a_over_b": med(t_old) / med(t_new),
           "device_ms_median": {"host_lists": span(d_old), "one_call": span(d_new)},
           "same_bytes": True}
    s.close()
    return out


def kernels(config, reps=10):
    """What the trace run executes: the one call alone."""
    s = Setup(config)
    for _ in range(3 + reps):
        s.new()
    s.close()


def trace(config):
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "kernels", config],
                       check=True, stdout=subprocess.DEVNULL, timeout=900)
        rows = []
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    out = {"map": config, "kernel_us_median": {}}
    for name in KERNELS:
        ts = [e - b for b, e, k in rows if name in k]
        ts = ts[3:] if len(ts) > 3 else ts                                          # (the first three calls warm the caches)
        out["kernel_us_median"][name] = {"launches": len(ts), "median": statistics.median(ts) / 1e3, "min": min(ts) / 1e3, "max": max(ts) / 1e3} if ts else None
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        kernels(sys.argv[2] if len(sys.argv) > 2 else "metric")
    elif mode == "trace":
        print(json.dumps(trace(sys.argv[2] if len(sys.argv) > 2 else "metric")))
    else:
        reps = int(mode) if mode else 15
        print(json.dumps({"metric": "AdjustAndUpdate write-back over the map graph", "maps": [run(c, reps) for c in ("metric", "c2")]}))
