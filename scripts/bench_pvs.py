"""Tracker::FindPVS on the device (mcp_track_find_pvs over a resident mcp_map_points table): time per call, PVS sizes per level, the
cost of keeping the table current, and a tracker frame that starts from the whole map -- MakeKeyFrame_Lite of every camera, the PVS,
a seeded per-level shuffle with a 1000-point budget, mcp_track_frame(imgs = NULL) -- next to the c3 frame of scripts/bench_tracker.py
(which is handed its ~1000 points).  Two maps: the c3 scene's points, and 50 k points grown from them.  Prints one JSON line."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _med_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main(reps=50, frames=30, size=(640, 480), cams=4, per_level=(100, 80, 50, 20), budget=1000, big=50000, seed=1):
    from mcptam_amd import hip_rt, synth_img
    from mcptam_amd.keyframe import MEST, FINE_NONLINEAR, FINE_OVERRIDE, KeyFrame, TdIn, TrackFrame, _pose12, lib, make_lite_batch, pack_points
    from mcptam_amd.pvs import MapPointTable
    from mcptam_amd.taylor_camera import camera_array
    sc = synth_img.make_tracking_scene(size=size)
    I = (np.eye(3), np.zeros(3))
    src = KeyFrame(*size)
    src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
    base_pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"], per_level=per_level)
    c3_pts = base_pts * cams                                   # bench_tracker's c3: every camera tracks the same scene's points
    cur = [KeyFrame(*size) for _ in range(cams)]
    carr = camera_array([sc["cam"]] * cams)
    cfb = np.ascontiguousarray(np.stack([_pose12(*I) for _ in range(cams)]))
    frame_img = np.ascontiguousarray(sc["imgB"])
    ring = [hip_rt.dev_alloc(frame_img.nbytes) for _ in range(cams)]
    for r in ring:
        hip_rt.dev_upload(r, frame_img)
    make_lite_batch(cur, ring, on_device=True)
    L = lib()
    bfw = _pose12(*sc["poseB"])

    # the c3 frame as bench_tracker times it (mcp_track_frame, images in HBM, results read in place), for comparison
    packed = [pack_points(base_pts, lambda kf: kf._h) for _ in range(cams)]
    tf = TrackFrame(cur, carr, cfb, packed)
    tf.run(ring, sc["poseB"], 10, 8, on_device=True, want_points=False, view=True)
    c3_frame_ms = _med_ms(lambda: tf.run(ring, sc["poseB"], 10, 8, on_device=True, want_points=False, view=True), frames)

    td_dt = np.dtype([("world_pos", "f8", 3), ("pixel_right_w", "f8", 3), ("pixel_down_w", "f8", 3), ("source_kf", "u8"), ("source_level", "i4"),
                      ("center_x", "i4"), ("center_y", "i4"), ("fixed", "i4")], align=True)
    assert td_dt.itemsize == ctypes.sizeof(TdIn)
    nl = np.ascontiguousarray(FINE_NONLINEAR, dtype=np.uint8)
    ov = np.ascontiguousarray(FINE_OVERRIDE, dtype=np.float64)

    def run_map(label, wp, pr, pd, us):
        n = len(wp)
        t = MapPointTable()
        t.set(wp, pr, pd, us)
        hs = (ctypes.c_void_p * cams)(*[k._h for k in cur])
        caps = np.full(cams, n, dtype=np.int32)
        counts = np.zeros((cams, 4), dtype=np.int32)
        fn = L.mcp_track_find_pvs

        def pvs_call():
            if fn(t._h, cams, hs, ctypes.cast(carr, ctypes.c_void_p), bfw.ctypes.data, cfb.ctypes.data, caps.ctypes.data, None, counts.ctypes.data) != 0:
                raise RuntimeError("find_pvs failed")

        pvs_call()
        pvs_ms = _med_ms(pvs_call, reps)
        py_ms = _med_ms(lambda: t.find_pvs(cur, carr, sc["poseB"], cfb, view=True), reps)
        sizes = counts.copy()
        # table maintenance: a full upload, and an update of 5 % of the rows; each timed to completion (the PVS call that follows waits
        # for it: its median is subtracted)
        full_ms = _med_ms(lambda: (t.set(wp, pr, pd, us), pvs_call()), max(5, reps // 5)) - pvs_ms
        rng = np.random.default_rng(seed)
        ids = np.sort(rng.choice(n, max(1, n // 20), replace=False)).astype(np.int32)
        upd_ms = _med_ms(lambda: (t.update(ids, wp[ids], pr[ids], pd[ids], us[ids]), pvs_call()), max(5, reps // 5)) - pvs_ms
        full_call_ms = _med_ms(lambda: t.set(wp, pr, pd, us), 5)
        upd_call_ms = _med_ms(lambda: t.update(ids, wp[ids], pr[ids], pd[ids], us[ids]), 5)
        pvs_call()
        # the frame that starts from the map
        recs = np.zeros(n, dtype=td_dt)
        recs["world_pos"], recs["pixel_right_w"], recs["pixel_down_w"] = wp, pr, pd
        recs["source_kf"] = src._h
        recs["center_x"], recs["center_y"] = 320, 240
        shuf = np.random.default_rng(seed)
        per_cam = budget // cams
        mu = np.zeros(6)
        wl = np.zeros(budget)
        stage = {"lite": [], "pvs": [], "select": [], "track": []}

        def frame():
            t0 = time.perf_counter()
            make_lite_batch(cur, ring, on_device=True)
            t1 = time.perf_counter()
            pvs_call()
            t2 = time.perf_counter()
            sel, ns = [], []
            for c in range(cams):
                picks = []
                for l in (3, 2, 1, 0):                          # coarse levels first, each shuffled (Tracker.cc:983)
                    cnt = int(counts[c, l])
                    if cnt == 0:
                        continue
                    ptr = L.mcp_track_find_pvs_view(t._h, c, l, None)
                    rows = np.frombuffer((ctypes.c_int * (cnt * 22)).from_address(ptr), dtype=np.int32)[::22]      # mcp_pvs_entry.point (88 B = 22 ints)
                    picks.append(rows[shuf.permutation(cnt)])
                p = np.concatenate(picks)[:per_cam] if picks else np.zeros(0, dtype=np.int32)
                sel.append(recs[p])
                ns.append(len(p))
            arrs = [(TdIn * max(1, len(a))).from_buffer(a if len(a) else np.zeros(1, dtype=td_dt)) for a in sel]
            t3 = time.perf_counter()
            b = bfw.copy()
            rc = L.mcp_track_frame(cams, hs, None, None, 0, None, ctypes.cast(carr, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data,
                                   (ctypes.c_int * cams)(*ns), (ctypes.c_void_p * cams)(*[ctypes.cast(a, ctypes.c_void_p) for a in arrs]), None, None,
                                   10, 8, 0, len(nl), nl.ctypes.data, ov.ctypes.data, MEST["Tukey"], None, None, mu.ctypes.data, wl.ctypes.data)
            if rc != 0:
                raise RuntimeError("track_frame failed")
            t4 = time.perf_counter()
            for k, a, z in (("lite", t0, t1), ("pvs", t1, t2), ("select", t2, t3), ("track", t3, t4)):
                stage[k].append((z - a) * 1e3)
            return sum(ns)

        tracked = frame()
        for v in stage.values():
            v.clear()
        frame_ms = _med_ms(frame, frames)
        t.close()
        return {"map": label, "points": n, "cameras": cams, "find_pvs_ms_median": pvs_ms, "find_pvs_python_view_ms_median": py_ms,
                "pvs_per_level": sizes.sum(axis=0).tolist(), "pvs_per_camera": sizes.sum(axis=1).tolist(),
                "table_full_upload_ms": full_ms, "table_update_5pct_ms": upd_ms, "table_full_upload_call_ms": full_call_ms,
                "table_update_5pct_call_ms": upd_call_ms, "frame_with_pvs_ms_median": frame_ms, "frame_tracked_points": tracked,
                "frame_stage_ms_median": {k: statistics.median(v) for k, v in stage.items()}}

    wp3, pr3, pd3 = synth_img.points_soa(c3_pts)
    r_c3 = run_map("c3 scene", wp3, pr3, pd3, np.ones(len(wp3), np.uint8))
    wpb, prb, pdb, usb = synth_img.make_map_cloud(base_pts, big, seed=seed)
    r_big = run_map("%d points" % big, wpb, prb, pdb, usb)
    for r in ring:
        hip_rt.dev_free(r)
    return {"metric": "FindPVS on the device (mcp_track_find_pvs, %d cameras %dx%d)" % (cams, size[0], size[1]),
            "c3_frame_without_pvs_ms_median": c3_frame_ms, "maps": [r_c3, r_big],
            "note": "find_pvs_ms_median: the C call alone (out = NULL, lists read in place), host-observed, median of %d; _python_view: the "
                    "Python binding around it.  table_*_ms: the call plus its completion (the next PVS call waits for it; that call's median "
                    "subtracted); _call_ms: the call returning (enqueue).  frame_with_pvs: make_lite_batch (images in HBM) + PVS + per-level "
                    "shuffle and %d-point budget on the host + mcp_track_frame(imgs = NULL, 10 pose iterations, results read in place); "
                    "c3_frame_without_pvs: bench_tracker's zero-copy mcp_track_frame on its fixed ~1000 points (median here)." % (reps, budget)}


if __name__ == "__main__":
    print(json.dumps(main()))
