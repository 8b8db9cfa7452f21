"""mcp_track_frame_recover against the split sequence it replaces, per lost frame, at the c3 map (4 cameras 640x480, 1000 tracked points,
images in HBM; the scene and parameters of scripts/bench_track_frame_motion.py), with 8 and with 800 candidate keyframes (160x120 handles
with distinct images, spread evenly over the cameras; the SBI is 40x30 whatever the frame):
  (a) the split sequence, 3C + 2 waits: mcp_kf_make_lite_batch (the relocaliser's SBI needs level 0 of the new frame); per camera
      mcp_kf_make_sbi (blur 2.5), mcp_sbi_score over that camera's candidates, mcp_sbi_iterate against the winner, mcp_sbi_se3_from_se2 and
      mcp_track_recover_pose_host (the two pose products) on the host; then mcp_track_frame_motion with apply = 0 and imgs = NULL from the
      first recovered camera's pose;
  (b) mcp_track_frame_recover with the frame's images: one submission, one wait.
Both with want_items = 0 and the doubled coarse caps.  Host-observed medians of alternating pairs (a, b, a, b, ...) with their ranges; the
run-to-run spread is the larger of the two (max - min) / median.  Prints one JSON line.
  `split-only`   times (a) alone with nothing this entry added but the host pose products (done in numpy then): the form to run on a commit
                 that has no mcp_track_frame_recover, as the baseline.
  `kernels N`    runs both sides a few times at N candidates and prints nothing of interest: the workload of a kernel trace.
  `trace [N]`    starts `rocprofv3 --kernel-trace` on `kernels N` (default 800) in a child process and reports, per frame, the median of
                 k_reloc_score's duration and of the sum of the C launches of k_sbi_score."""
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
    med = statistics.median(ts)
    return {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "frames_per_s": 1.0 / med, "spread": (max(ts) - min(ts)) / med}


class Bench:
    def __init__(self, size=(640, 480), cams=4, per_level=(100, 80, 50, 20), split_only=False):
        from mcptam_amd import hip_rt, synth_img
        from mcptam_amd.keyframe import KeyFrame, _pose12
        from mcptam_amd.keyframe import lib as kf_lib
        from mcptam_amd.pvs import MapPointTable, TrackMapParams, TrackMapResult, TrackMotion, TrackRecord, TrackRecordParams, _bind_track_map, _bind_track_motion, \
            _bind_track_record, motion_params
        from mcptam_amd.taylor_camera import TaylorCamera, camera_array
        self.hip_rt, self.KeyFrame, self.cams, self.size, self.split_only = hip_rt, KeyFrame, cams, size, split_only
        sc = self.sc = synth_img.make_tracking_scene(size=size)
        src = self.src = KeyFrame(*size)
        src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
        pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"], per_level=per_level) * cams
        wp, pr, pd = synth_img.points_soa(pts)
        n = self.n = len(wp)
        level = np.array([p["source_level"] for p in pts], dtype=np.int32)
        center = np.array([p["center"] for p in pts], dtype=np.int32)
        rng = np.random.default_rng(3)
        inl, outl = rng.integers(1, 31, n).astype(np.int32), rng.integers(0, 31, n).astype(np.int32)
        self.carr = camera_array([sc["cam"]] * cams)
        self.cam_sbi = TaylorCamera(sc["cam"].params, size, size, (40, 30))
        self.sarr = camera_array([self.cam_sbi] * cams)
        self.cfb = np.ascontiguousarray(np.stack([_pose12(np.eye(3), np.zeros(3)) for _ in range(cams)]))
        frame_img = np.ascontiguousarray(sc["imgB"])
        self.ring = [hip_rt.dev_alloc(frame_img.nbytes) for _ in range(cams)]
        for r in self.ring:
            hip_rt.dev_upload(r, frame_img)
        self.ip = (ctypes.c_void_p * cams)(*self.ring)
        self.st = (ctypes.c_int * cams)(*([size[0]] * cams))
        self.prm = TrackMapParams(1, 120, 60, 20, 8, 1000, 0, 12345)       # mbJustRecoveredSoUseCoarse: try_coarse, the doubled caps
        self.rp = TrackRecordParams(1, 0, 10, 20, 0.3, 0.13)
        self.lost = _pose12(np.eye(3), np.array([3.0, 2.0, 1.0]))           # where the lost tracker believes it is
        self.kf_pose = _pose12(*sc["poseA"])
        self.res, self.rec, self.mo = TrackMapResult(), TrackRecord(), TrackMotion()
        self.mp = motion_params(np.zeros(6), 1.0 / 30, [1] * cams, apply=False, ncam=cams)

        def table():
            t = MapPointTable()
            t.set(wp, pr, pd, np.ones(n, np.uint8))
            t.set_source(np.arange(n, dtype=np.int32), [src] * n, level, center, np.zeros(n, dtype=np.uint8))
            t.set_counts(inl, outl)
            return t
        self.A, self.ka = table(), [KeyFrame(*size) for _ in range(cams)]
        self.L = _bind_track_motion(_bind_track_record(_bind_track_map(self.A._L)))
        self.K = kf_lib()
        self.ha = (ctypes.c_void_p * cams)(*[k._h for k in self.ka])
        if not split_only:
            from mcptam_amd.pvs import TrackRecover, TrackRecoverParams, _bind_track_recover
            _bind_track_recover(self.L)
            self.B, self.kb = table(), [KeyFrame(*size) for _ in range(cams)]
            self.hb = (ctypes.c_void_p * cams)(*[k._h for k in self.kb])
            self.rq, self.rv = TrackRecoverParams(2.5, 6, 1e5), TrackRecover()
        self.pool = []

    def candidates(self, ncand):
        """ncand small keyframes with distinct images (windows of the scene's first image at different offsets) and the relocaliser's SBI;
        entry i belongs to camera i % C; every pose is the scene's first pose, so whoever wins, TrackMap has a map in view."""
        a = self.sc["imgA"]
        while len(self.pool) < ncand:
            i = len(self.pool)
            y, x = (37 * i) % (a.shape[0] - 120), (53 * i) % (a.shape[1] - 160)
            k = self.KeyFrame(160, 120)
            k.MakeKeyFrame_Lite(np.ascontiguousarray(a[y:y + 120, x:x + 160])); k.MakeSBI(2.5)
            self.pool.append(k)
        C = self.cams
        self.ncand = ncand
        self.cand_h = (ctypes.c_void_p * max(ncand, 1))(*[k._h for k in self.pool[:ncand]])
        self.cand_cam = np.array([i % C for i in range(ncand)], dtype=np.int32)
        self.cand_pose = np.ascontiguousarray(np.tile(self.kf_pose, (max(ncand, 1), 1)))
        self.per_cam = []
        for c in range(C):
            idx = [i for i in range(ncand) if i % C == c]
            self.per_cam.append((idx, (ctypes.c_void_p * max(len(idx), 1))(*[self.pool[i]._h for i in idx]), np.zeros(max(len(idx), 1))))

    def split(self):
        K, L, C = self.K, self.L, self.cams
        se2, score, best, R3 = np.zeros(6), ctypes.c_double(0), ctypes.c_int(-1), np.zeros(9)
        pose, bfw, start = np.zeros(12), np.zeros(12), None
        ok = K.mcp_kf_make_lite_batch(C, self.ha, self.ip, self.st, 1, None) == 0
        for c in range(C):
            idx, hs, sc = self.per_cam[c]
            ok = ok and K.mcp_kf_make_sbi(self.ka[c]._h, ctypes.c_double(2.5)) == 0
            ok = ok and K.mcp_sbi_score(self.ka[c]._h, len(idx), hs, sc.ctypes.data, ctypes.byref(best)) == 0
            if not ok or best.value < 0:
                continue
            ok = ok and K.mcp_sbi_iterate(self.ka[c]._h, hs[best.value], 6, se2.ctypes.data, ctypes.byref(score)) == 0
            if self.split_only:      # SE3fromSE2 from the library, the two products in numpy
                ok = ok and K.mcp_sbi_se3_from_se2(se2.ctypes.data, ctypes.byref(self.sarr[c]), ctypes.byref(self.sarr[c]), R3.ctypes.data) == 0
                Rr, Rk, tk = R3.reshape(3, 3), self.kf_pose[:9].reshape(3, 3), self.kf_pose[9:]
                Rc, tc = self.cfb[c][:9].reshape(3, 3), self.cfb[c][9:]
                bfw = np.concatenate([(Rc.T @ Rr @ Rk).ravel(), Rc.T @ (Rr @ tk - tc)])
            else:
                ok = ok and L.mcp_track_recover_pose_host(se2.ctypes.data, ctypes.byref(self.sarr[c]), self.kf_pose.ctypes.data, self.cfb[c].ctypes.data, pose.ctypes.data,
                                                          bfw.ctypes.data) == 0
            if start is None and score.value < 1e5:
                start = bfw.copy()
        if ok and start is not None:
            ok = L.mcp_track_frame_motion(self.A._h, C, self.ha, None, None, 0, None, ctypes.cast(self.carr, ctypes.c_void_p), ctypes.cast(self.sarr, ctypes.c_void_p),
                                          start.ctypes.data, self.cfb.ctypes.data, ctypes.byref(self.prm), ctypes.byref(self.res), ctypes.byref(self.rp), ctypes.byref(self.rec),
                                          ctypes.byref(self.mp), ctypes.byref(self.mo)) == 0
        if not ok:
            raise RuntimeError("the split sequence failed")
        return start is not None

    def one(self):
        b = self.lost.copy()
        if self.L.mcp_track_frame_recover(self.B._h, self.cams, self.hb, self.ip, self.st, 1, None, ctypes.cast(self.carr, ctypes.c_void_p), ctypes.cast(self.sarr, ctypes.c_void_p),
                                          b.ctypes.data, self.cfb.ctypes.data, ctypes.byref(self.prm), ctypes.byref(self.res), ctypes.byref(self.rp), ctypes.byref(self.rec),
                                          ctypes.byref(self.mp), ctypes.byref(self.mo), self.ncand, self.cand_h, self.cand_cam.ctypes.data, self.cand_pose.ctypes.data,
                                          ctypes.byref(self.rq), ctypes.byref(self.rv), None) != 0:
            raise RuntimeError("track_frame_recover failed")
        return self.rv.recovered != 0

    def timed(self, ncand, pairs):
        self.candidates(ncand)
        for _ in range(3):
            rec_a = self.split()
            rec_b = None if self.split_only else self.one()
        ta, tb = [], []
        for _ in range(pairs):
            t0 = time.perf_counter(); self.split(); t1 = time.perf_counter()
            ta.append(t1 - t0)
            if not self.split_only:
                self.one(); tb.append(time.perf_counter() - t1)
        out = {"candidates": ncand, "a_split_sequence": _stats(ta), "waits_a": 3 * self.cams + 2, "recovered_a": bool(rec_a),
               "items": sum(self.rec.n_items[c] for c in range(self.cams)), "found": sum(self.rec.n_meas[c] for c in range(self.cams))}
        if not self.split_only:
            sa, sb = _stats(ta), _stats(tb)
            out.update(b_track_frame_recover=sb, waits_b=1, recovered_b=bool(rec_b), speedup_b_over_a=sa["median_ms"] / sb["median_ms"], spread=max(sa["spread"], sb["spread"]),
                       cam=self.rv.cam, best=[self.rv.best[c] for c in range(self.cams)])
        return out

    def close(self):
        for r in self.ring:
            self.hip_rt.dev_free(r)


def main(pairs=30, split_only=False):
    b = Bench(split_only=split_only)
    out = {"metric": "TrackFrame's lost branch per frame, c3 (%d cameras %dx%d, %d tracked points, images in HBM)" % (b.cams, b.size[0], b.size[1], b.n),
           "note": "host-observed, %d alternating pairs after 3 warm-up pairs" % pairs, "runs": [b.timed(8, pairs), b.timed(800, pairs)]}
    b.close()
    return out


def kernels(ncand, reps=10):
    b = Bench()
    b.candidates(ncand)
    for _ in range(reps):
        b.split(); b.one()
    b.close()


def trace(ncand):
    """k_reloc_score against k_sbi_score per frame, from a kernel trace of `kernels ncand` taken in a child process."""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "kernels", str(ncand)],
                       check=True, stdout=subprocess.DEVNULL, timeout=600)
        rows = []
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    new = [e - s for s, e, k in rows if "k_reloc_score" in k]
    old = [e - s for s, e, k in rows if "k_sbi_score" in k]
    cams = len(old) // max(len(new), 1)
    old_frames = [sum(old[i:i + cams]) for i in range(0, len(old) - cams + 1, cams)] if cams else []
    out = {"candidates": ncand, "frames": len(new), "k_sbi_score_launches_per_frame": cams}
    if len(new) > 3 and len(old_frames) > 3:      # (the first three frames warm the caches)
        a, b_ = old_frames[3:], new[3:]
        out.update(k_sbi_score_us_per_frame={"median": statistics.median(a) / 1e3, "min": min(a) / 1e3, "max": max(a) / 1e3},
                   k_reloc_score_us_per_frame={"median": statistics.median(b_) / 1e3, "min": min(b_) / 1e3, "max": max(b_) / 1e3},
                   ratio_old_over_new=statistics.median(a) / statistics.median(b_))
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 800)
    elif mode == "trace":
        print(json.dumps(trace(int(sys.argv[2]) if len(sys.argv) > 2 else 800)))
    else:
        print(json.dumps(main(split_only=mode == "split-only")))
