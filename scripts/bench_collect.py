"""The co-visible points of the nearest keyframe (tracker_collect_all_points = false) over the metric map's store (200 MKFs x 4 cameras, 50k rows,
400k store entries):
  (stand-alone) mcp_map_collect_nearest over the resident graph: wall time of the call and device time of its launches
                (mcp_map_collect_last_timing), next to the host twin over host arrays (mcp_map_collect_nearest_host: the same bodies under the
                host compiler, no read-back counted);
  (frame)       mcp_track_map of scripts/bench_track_map.py's frame (4 cameras 640x480, images in HBM) over a 50k-row table with that graph on
                it, the mode off and on in alternation: wall time of the call, and the device time of the collection launches inside the frame.
A check first that device and host give the same bytes.  Warm-up turns, then the median and the inter-quartile range.  Prints one JSON line.
  bench_collect.py [turns] [warmup] [frames]"""
import ctypes
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


def main(turns=100, warmup=10, frames=60):
    from mcptam_amd import hip_rt, synth, synth_img
    from mcptam_amd import map_graph as mg
    from mcptam_amd.keyframe import KeyFrame, _pose12, make_lite_batch
    from mcptam_amd.pvs import MapPointTable, TrackMapParams, TrackMapResult, _bind_track_map
    from mcptam_amd.taylor_camera import camera_array
    p = synth.make_config("metric")
    a = mg.problem_arrays(p)
    N, M, P, cams = p.n_points, p.n_meas, p.n_mkf, len(p.cams)
    a["n_rows"] = N
    size = (640, 480)
    sc = synth_img.make_tracking_scene(size=size)
    src = KeyFrame(*size)
    src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
    base_pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"], per_level=(100, 80, 50, 20))
    wp, pr, pd, us = synth_img.make_map_cloud(base_pts, N, seed=1)
    t = MapPointTable()
    t.set(wp, pr, pd, us)
    t.set_source(np.arange(N, dtype=np.int32), [src] * N, np.zeros(N, dtype=np.int32), np.tile(np.array([[320, 240]], dtype=np.int32), (N, 1)), np.zeros(N, dtype=np.uint8))
    g = mg.MapGraph(t, a["cam_from_base"])
    g.load_arrays(a)
    g.num_meas()                                         # (waits: the timed region starts on an idle stream)
    depth = np.full(cams, 2.0)
    out = {"map": {"mkfs": P, "cams": cams, "rows": N, "store": M}, "turns": turns, "warmup": warmup, "frames": frames}

    # ---- the stand-alone call, at the pose of an MKF in the middle of the map
    pose = a["base_from_world"][P // 2].copy()
    dev = lambda: g.collect_nearest(pose, depth, raw=True)
    host = lambda: mg.collect_nearest_host(a, pose, depth, raw=True)
    (rd, nd), (rh, nh) = dev(), host()
    assert bytes(rd) == bytes(rh) and nd.tobytes() == nh.tobytes(), "device and host disagree"
    td, tk, th = [], [], []
    for i in range(warmup + turns):
        t0 = time.perf_counter(); dev(); dt = time.perf_counter() - t0
        if i >= warmup:
            td.append(dt); tk.append(g.collect_last_timing() * 1e-3)
    for i in range(3 + max(turns // 10, 5)):
        t0 = time.perf_counter(); host(); dt = time.perf_counter() - t0
        if i >= 3:
            th.append(dt)
    rep = rd.as_dict()
    out["stand_alone"] = {"device_wall": _stats(td), "device_events": _stats(tk), "host_twin": _stats(th), "nearest_slot": rep["nearest_slot"][:cams].tolist(),
                          "n_seed_rows": rep["n_seed_rows"][:cams].tolist(), "n_kfs": rep["n_kfs"][:cams].tolist(), "n_rows": rep["n_rows"][:cams].tolist()}

    # ---- the frame of scripts/bench_track_map.py over this table, the mode off and on
    cur = [KeyFrame(*size) for _ in range(cams)]
    carr = camera_array([sc["cam"]] * cams)
    cfb = np.ascontiguousarray(np.stack([_pose12(np.eye(3), np.zeros(3)) for _ in range(cams)]))      # (the frame's own CamFromBase, as bench_track_map's)
    img = np.ascontiguousarray(sc["imgB"])
    ring = [hip_rt.dev_alloc(img.nbytes) for _ in range(cams)]
    for r in ring:
        hip_rt.dev_upload(r, img)
    make_lite_batch(cur, ring, on_device=True)
    hs = (ctypes.c_void_p * cams)(*[k._h for k in cur])
    ip = (ctypes.c_void_p * cams)(*ring)
    st = (ctypes.c_int * cams)(*([size[0]] * cams))
    prm = TrackMapParams(1, 60, 30, 20, 8, 1000, 0, 12345)
    bfw0 = _pose12(*sc["poseB"])
    # MKF P // 2 sits at the tracker's pose, so that its keyframes win
    k = a["base_from_world"].copy(); k[P // 2] = bfw0
    g.update_mkfs([P // 2], k[P // 2][None], a["mkf_flags"][P // 2][None], a["kf_active"][P // 2][None], a["kf_depth_mean"][P // 2][None])
    L = _bind_track_map(t._L)
    res = TrackMapResult()

    def frame():
        b = bfw0.copy()
        if L.mcp_track_map(t._h, cams, hs, ip, st, 1, None, ctypes.cast(carr, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data, ctypes.byref(prm), ctypes.byref(res)) != 0:
            raise RuntimeError("track_map failed")
    t_off, t_on, t_ev, pvs = [], [], [], {}
    for i in range(5 + frames):
        for on in ((False, True) if i % 2 == 0 else (True, False)):
            if on:
                t.collect_nearest(g, depth)
            else:
                t.collect_nearest_off()
            t0 = time.perf_counter(); frame(); dt = time.perf_counter() - t0
            if i >= 5:
                (t_on if on else t_off).append(dt)
                if on:
                    t_ev.append(g.collect_last_timing() * 1e-3)
            pvs[on] = [sum(res.pvs_counts[c]) for c in range(cams)]
    t.collect_nearest(g, depth)
    frame()
    last = t.collect_last()
    out["frame"] = {"mode_off": _stats(t_off), "mode_on": _stats(t_on), "collection_events_in_frame": _stats(t_ev), "pvs_per_camera_off": pvs[False], "pvs_per_camera_on": pvs[True],
                    "nearest_slot": last["nearest_slot"][:cams].tolist(), "n_rows": last["n_rows"][:cams].tolist()}
    for r in ring:
        hip_rt.dev_free(r)
    g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
