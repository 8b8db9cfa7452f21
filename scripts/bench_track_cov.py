"""The pose covariance of the one-call frame (mcp_track_pose_cov_enable) against the host sum it replaces, per frame, at the c3 map and at
the 50k-point map of scripts/bench_track_record.py (same scene, cameras, images in HBM, parameters):
  (a) mcp_track_map_record with the switch OFF and want_items = 1 -- the 320-byte items are what carries Jacobians, noise and weights to the
      host -- then shim/Tracker_gpu.cc's host sum in numpy: 100 I + sum of w (s J)^T (s J) over the found items with weight != 0 and the
      pseudo-inverse of the 6 x 6.  (The items hold the search stage's Jacobians, not the last iteration's: (a) has the data movement and
      the arithmetic of the host path, not its values.)
  (b) mcp_track_map_record with the switch ON and want_items = 0, then mcp_track_pose_cov_last: two more launches behind the same wait.
  (c) as (b) with the switch OFF: the frame without any covariance, which shows what the two launches add.
Host-observed medians of alternating rounds (a, b, c, a, b, c, ...) with [min, max].  Prints one JSON line.
  bench_track_cov.py [c3|big]      the timing
  bench_track_cov.py trace [c3|big] k_pose_cov_tiles / k_pose_cov_finish per frame from a kernel trace of `kernels` taken in a child process
  bench_track_cov.py kernels [c3|big] [N]   N frames with the switch on, nothing timed (what the trace runs)"""
import csv
import ctypes
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


def _stats(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3}


class Bench:
    def __init__(self, size=(640, 480), cams=4, per_level=(100, 80, 50, 20)):
        from mcptam_amd import hip_rt, synth_img
        from mcptam_amd.keyframe import KeyFrame, _pose12, make_lite_batch
        from mcptam_amd.taylor_camera import camera_array
        self.hip_rt, self.synth_img, self.size, self.cams = hip_rt, synth_img, size, cams
        sc = synth_img.make_tracking_scene(size=size)
        self.src = KeyFrame(*size)
        self.src.MakeKeyFrame_Lite(sc["imgA"]); self.src.MakeKeyFrame_Rest()
        self.base_pts = synth_img.make_map_points(sc["cam"], self.src, None, sc["poseA"], sc["depth"], per_level=per_level)
        self.cur = [KeyFrame(*size) for _ in range(cams)]
        self.carr = camera_array([sc["cam"]] * cams)
        self.cfb = np.ascontiguousarray(np.stack([_pose12(np.eye(3), np.zeros(3)) for _ in range(cams)]))
        frame_img = np.ascontiguousarray(sc["imgB"])
        self.ring = [hip_rt.dev_alloc(frame_img.nbytes) for _ in range(cams)]
        for r in self.ring:
            hip_rt.dev_upload(r, frame_img)
        make_lite_batch(self.cur, self.ring, on_device=True)
        self.hs = (ctypes.c_void_p * cams)(*[k._h for k in self.cur])
        self.ip = (ctypes.c_void_p * cams)(*self.ring)
        self.st = (ctypes.c_int * cams)(*([size[0]] * cams))
        self.bfw0 = _pose12(*sc["poseB"])

    def map_columns(self, which, big=50000, seed=1):
        if which == "c3":
            pts = self.base_pts * self.cams
            wp, pr, pd = self.synth_img.points_soa(pts)
            return ("c3 scene", wp, pr, pd, np.ones(len(wp), np.uint8), np.array([p["source_level"] for p in pts], dtype=np.int32),
                    np.array([p["center"] for p in pts], dtype=np.int32))
        wp, pr, pd, us = self.synth_img.make_map_cloud(self.base_pts, big, seed=seed)
        return "%d points" % big, wp, pr, pd, us, np.zeros(big, dtype=np.int32), np.tile(np.array([[320, 240]], dtype=np.int32), (big, 1))

    def table(self, cols, on):
        from mcptam_amd.pvs import MapPointTable
        _, wp, pr, pd, us, level, center = cols
        n = len(wp)
        rng = np.random.default_rng(3)
        t = MapPointTable()
        t.set(wp, pr, pd, us)
        t.set_source(np.arange(n, dtype=np.int32), [self.src] * n, level, center, np.zeros(n, dtype=np.uint8))
        t.set_counts(rng.integers(1, 31, n).astype(np.int32), rng.integers(0, 31, n).astype(np.int32))
        t.pose_cov_enable(on)
        return t

    def frame(self, t, want_items):
        """One mcp_track_map_record on table t; returns (res, rec)."""
        from mcptam_amd.pvs import TrackMapParams, TrackMapResult, TrackRecord, TrackRecordParams, _bind_track_cov, _bind_track_map, _bind_track_record
        L = _bind_track_cov(_bind_track_record(_bind_track_map(t._L)))
        prm = TrackMapParams(1, 60, 30, 20, 8, 1000, 0, 12345)
        rp = TrackRecordParams(0, int(want_items), 10, 20, 0.3, 0.13)
        res, rec = TrackMapResult(), TrackRecord()
        b = self.bfw0.copy()
        if L.mcp_track_map_record(t._h, self.cams, self.hs, self.ip, self.st, 1, None, ctypes.cast(self.carr, ctypes.c_void_p), b.ctypes.data, self.cfb.ctypes.data,
                                  ctypes.byref(prm), ctypes.byref(res), ctypes.byref(rp), ctypes.byref(rec)) != 0:
            raise RuntimeError("track_map_record failed")
        return res, rec

    def path_a(self, t):
        from mcptam_amd.pvs import TRACK_MAP_ITEM_DTYPE, _view
        self.frame(t, True)
        info = 100.0 * np.eye(6)
        for c in range(self.cams):
            it = _view(t._L.mcp_track_map_view, (t._h, c), TRACK_MAP_ITEM_DTYPE)            # in place: the pinned block
            use = (it["out"]["found"] != 0) & (it["weight_last"] != 0)
            J = (it["out"]["jacobian"][use] * it["out"]["sqrt_inv_noise"][use][:, None]).reshape(-1, 2, 6)
            info += np.einsum("n,nrx,nry->xy", it["weight_last"][use], J, J)
        return np.linalg.pinv(info, hermitian=True)

    def path_b(self, t):
        self.frame(t, False)
        return t.pose_cov_last()

    def close(self):
        for r in self.ring:
            self.hip_rt.dev_free(r)


def main(pairs=15, only=None):
    b = Bench()
    maps = []
    for which in ("c3", "big"):
        if only not in (None, which):
            continue
        cols = b.map_columns(which)
        A, B, C = b.table(cols, False), b.table(cols, True), b.table(cols, False)
        for _ in range(3):
            b.path_a(A); last = b.path_b(B); b.frame(C, False)
        ta, tb, tc = [], [], []
        for _ in range(pairs):
            t0 = time.perf_counter(); b.path_a(A); t1 = time.perf_counter(); last = b.path_b(B); t2 = time.perf_counter(); b.frame(C, False); t3 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1); tc.append(t3 - t2)
        res, rec = b.frame(B, False)
        n_items, n_meas = sum(rec.n_items[c] for c in range(b.cams)), sum(rec.n_meas[c] for c in range(b.cams))
        maps.append({"map": cols[0], "points": len(cols[1]), "cameras": b.cams, "a_items_then_host_sum": _stats(ta), "b_switch_on_no_items": _stats(tb),
                     "c_switch_off_no_items": _stats(tc),
                     "items": n_items, "found": n_meas, "bytes_down_a": 320 * n_items + 8 * n_items + 32 * n_meas, "bytes_down_b": 8 * n_items + 32 * n_meas + 648,
                     "n_used": last.n_used, "n_inliers": rec.n_inliers, "valid": last.valid, "sweeps": last.sweeps, "norm_fro": last.norm_fro})
        A.close(); B.close(); C.close()
    b.close()
    return {"metric": "TrackMap of a frame with its bookkeeping and mm6PoseCovariance (%d cameras %dx%d, images in HBM)" % (b.cams, b.size[0], b.size[1]), "maps": maps,
            "note": "host-observed, %d alternating rounds after 3 warm-up rounds; (a) = mcp_track_map_record, switch off, items + the host sum and pseudo-inverse in numpy, "
                    "(b) = mcp_track_map_record, switch on, want_items = 0 + mcp_track_pose_cov_last, (c) = (b) with the switch off and no covariance" % pairs}


def kernels(which, reps=10):
    b = Bench()
    t = b.table(b.map_columns(which), True)
    for _ in range(reps):
        b.path_b(t)
    t.close(); b.close()


def trace(which):
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "kernels", which],
                       check=True, stdout=subprocess.DEVNULL, timeout=600)
        rows = []
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    out = {"map": which}
    for name in ("k_pose_cov_tiles", "k_pose_cov_finish"):
        ts = [e - s for s, e, k in rows if name in k][3:]                                    # (the first three frames warm the caches)
        out[name + "_us"] = {"frames": len(ts), "median": statistics.median(ts) / 1e3, "min": min(ts) / 1e3, "max": max(ts) / 1e3} if ts else None
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        kernels(sys.argv[2] if len(sys.argv) > 2 else "c3", int(sys.argv[3]) if len(sys.argv) > 3 else 10)
    elif mode == "trace":
        print(json.dumps(trace(sys.argv[2] if len(sys.argv) > 2 else "c3")))
    else:
        print(json.dumps(main(only=mode or None)))
