"""mcp_track_map: the whole Tracker::TrackMap of a frame from the resident map-point table in one call (MakeKeyFrame_Lite of every camera
from images in HBM, FindPVS, the keyed selection, coarse search + gate + iterations, fine searches, fine iterations), per-frame median at
the c3 map and at the 50k-point map of scripts/bench_pvs.py, next to the composition of existing calls and bench_pvs's frame_with_pvs (the same frame with the PVS lists copied to
the host, shuffled and budgeted there, then mcp_track_frame).  Prints one JSON line."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np


def _med_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def _composition(table, n, wp, pr, pd, level, center, src, cur, carr, cfb, sc, prm):
    """The same frame as the composition of existing public calls, driven from Python with everything per row packed once: mcp_track_find_pvs
    (read in place), the selection in numpy (pvs.select_sets), mcp_patch_sequences per camera and stage with host-held finder states,
    mcp_track_pose_refine_m for the coarse and the fine iterations (the iterations past 1024 records: the multi-workgroup kernel)."""
    from mcptam_amd import keyframe as K
    from mcptam_amd.pvs import PVS_ENTRY_DTYPE, select_sets
    L = K.lib()
    cams = len(cur)
    isz = ctypes.sizeof(K.PfItem)
    items = (K.PfItem * n)()
    for r in range(n):
        it = items[r]
        it.point.source_kf = src._h
        it.point.source_level = int(level[r]); it.point.center_x = int(center[r][0]); it.point.center_y = int(center[r][1])
        it.point_key = r
    geo = np.zeros(n, dtype=[("wp", "f8", 3), ("pr", "f8", 3), ("pd", "f8", 3)])          # mcp_td_in starts with these 72 bytes
    geo["wp"], geo["pr"], geo["pd"] = wp, pr, pd
    np.frombuffer(items, dtype=np.uint8).reshape(n, isz)[:, :72] = geo.view(np.uint8).reshape(n, 72)
    rec = np.frombuffer(items, dtype=np.dtype((np.void, isz)))
    cs = [ctypes.pointer(carr[c]) for c in range(cams)]
    states = [K.new_pf_states(n) for _ in range(cams)]
    seq = np.arange(n + 1, dtype=np.int32)
    counts = np.zeros((cams, 4), dtype=np.int32)
    caps = np.full(cams, n, dtype=np.int32)
    hs = (ctypes.c_void_p * cams)(*[k._h for k in cur])
    nl_c, ov_c = np.ones(10, dtype=np.uint8), np.array([0.0] * 6 + [1.0] * 4)

    def search(c, rows, pose12, rng, its):
        m = len(rows)
        out = np.zeros(max(m, 1), dtype=K.TD_OUT_DTYPE)
        if m == 0:
            return out[:0]
        tab = K.PfTarget(cur[c]._h, ctypes.cast(cs[c], ctypes.c_void_p), (ctypes.c_double * 12)(*pose12), (ctypes.c_double * 12)(*cfb[c]))
        sub = np.ascontiguousarray(rec[rows])
        st = np.ascontiguousarray(states[c][rows])
        if L.mcp_patch_sequences(K.PF_TRACK, 1, ctypes.byref(tab), m, seq.ctypes.data, sub.ctypes.data, st.ctypes.data, rng, its, 0, out.ctypes.data) != 0:
            raise RuntimeError("patch_sequences failed")
        states[c][rows] = st
        return out[:m]

    def frame():
        pose12 = _pose12_of(sc["poseB"])
        if L.mcp_track_find_pvs(table._h, cams, hs, ctypes.cast(carr, ctypes.c_void_p), pose12.ctypes.data, cfb.ctypes.data, caps.ctypes.data, None,
                                counts.ctypes.data) != 0:
            raise RuntimeError("find_pvs failed")
        sets = []
        for c in range(cams):
            lv = []
            for l in range(4):
                cnt = ctypes.c_int(0)
                ptr = L.mcp_track_find_pvs_view(table._h, c, l, ctypes.byref(cnt))
                lv.append(np.frombuffer((ctypes.c_char * (cnt.value * PVS_ENTRY_DTYPE.itemsize)).from_address(ptr), dtype=PVS_ENTRY_DTYPE)["point"].astype(np.int64)
                          if cnt.value else np.zeros(0, dtype=np.int64))
            sets.append(select_sets(lv, prm.seed, c, prm.try_coarse, prm.coarse_max, prm.max_patches))
        outC = [search(c, sets[c][0], pose12, prm.coarse_range, prm.coarse_subpix_its) for c in range(cams)]
        found = sum(int(((o["found"] != 0) & (o["template_bad"] == 0)).sum()) for o in outC)
        pose = sc["poseB"]
        recC = K.pose_points_frame([wp[sets[c][0]] for c in range(cams)], outC)
        if found > prm.coarse_min:
            pose, _, _, recC = K.track_pose_refine(recC, carr, cfb, pose, nonlinear=nl_c, override_sigma=ov_c)
        p12 = _pose12_of(pose)
        rng = 5 if found > prm.coarse_min else 10
        recs, o0 = [], 0
        for c in range(cams):
            nC = len(sets[c][0])
            recs += [recC[o0:o0 + nC], K.pose_points(wp[sets[c][1]], search(c, sets[c][1], p12, rng, 8), c),
                     K.pose_points(wp[sets[c][2]], search(c, sets[c][2], p12, rng, 0), c)]
            o0 += nC
        K.track_pose_refine(np.concatenate(recs), carr, cfb, pose)
    return frame


def _pose12_of(pose):
    from mcptam_amd.keyframe import _pose12
    return _pose12(*pose)


def main(frames=50, size=(640, 480), cams=4, per_level=(100, 80, 50, 20), big=50000, seed=1, with_pvs_bench=True):
    from mcptam_amd import hip_rt, synth_img
    from mcptam_amd.keyframe import KeyFrame, _pose12, make_lite_batch
    from mcptam_amd.pvs import MapPointTable, TrackMapParams, TrackMapResult, _bind_track_map
    from mcptam_amd.taylor_camera import camera_array
    sc = synth_img.make_tracking_scene(size=size)
    src = KeyFrame(*size)
    src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
    base_pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"], per_level=per_level)
    cur = [KeyFrame(*size) for _ in range(cams)]
    carr = camera_array([sc["cam"]] * cams)
    cfb = np.ascontiguousarray(np.stack([_pose12(np.eye(3), np.zeros(3)) for _ in range(cams)]))
    frame_img = np.ascontiguousarray(sc["imgB"])
    ring = [hip_rt.dev_alloc(frame_img.nbytes) for _ in range(cams)]
    for r in ring:
        hip_rt.dev_upload(r, frame_img)
    make_lite_batch(cur, ring, on_device=True)
    hs = (ctypes.c_void_p * cams)(*[k._h for k in cur])
    ip = (ctypes.c_void_p * cams)(*ring)
    st = (ctypes.c_int * cams)(*([size[0]] * cams))
    prm = TrackMapParams(1, 60, 30, 20, 8, 1000, 0, 12345)
    bfw0 = _pose12(*sc["poseB"])

    def run_map(label, wp, pr, pd, us, level, center):
        n = len(wp)
        t = MapPointTable()
        t.set(wp, pr, pd, us)
        t.set_source(np.arange(n, dtype=np.int32), [src] * n, level, center, np.zeros(n, dtype=np.uint8))
        L = _bind_track_map(t._L)
        res = TrackMapResult()

        def call():
            b = bfw0.copy()
            if L.mcp_track_map(t._h, cams, hs, ip, st, 1, None, ctypes.cast(carr, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data,
                               ctypes.byref(prm), ctypes.byref(res)) != 0:
                raise RuntimeError("track_map failed")
        call()
        ms = _med_ms(call, frames)
        comp = _composition(t, n, wp, pr, pd, level, center, src, cur, carr, cfb, sc, prm)
        comp()
        comp_ms = _med_ms(comp, max(5, frames // 5))
        out = {"map": label, "points": n, "cameras": cams, "track_map_ms_median": ms, "composition_ms_median": comp_ms, "did_coarse": res.did_coarse, "coarse_found": res.coarse_found,
               "pvs_per_camera": [sum(res.pvs_counts[c]) for c in range(cams)], "sets_per_camera": [list(res.set_sizes[c]) for c in range(cams)]}
        t.close()
        return out

    c3_pts = base_pts * cams
    wp3, pr3, pd3 = synth_img.points_soa(c3_pts)
    lv3 = np.array([p["source_level"] for p in c3_pts], dtype=np.int32)
    cx3 = np.array([p["center"] for p in c3_pts], dtype=np.int32)
    r_c3 = run_map("c3 scene", wp3, pr3, pd3, np.ones(len(wp3), np.uint8), lv3, cx3)
    wpb, prb, pdb, usb = synth_img.make_map_cloud(base_pts, big, seed=seed)
    r_big = run_map("%d points" % big, wpb, prb, pdb, usb, np.zeros(big, dtype=np.int32), np.tile(np.array([[320, 240]], dtype=np.int32), (big, 1)))
    for r in ring:
        hip_rt.dev_free(r)
    line = {"metric": "TrackMap of a frame from the map (mcp_track_map, %d cameras %dx%d, images in HBM)" % (cams, size[0], size[1]),
            "maps": [r_c3, r_big]}
    if with_pvs_bench:
        import bench_pvs
        pv = bench_pvs.main()
        for r, m in zip(line["maps"], pv["maps"]):
            r["bench_pvs_frame_with_pvs_ms_median"] = m["frame_with_pvs_ms_median"]
            r["bench_pvs_frame_stage_ms_median"] = m["frame_stage_ms_median"]
    line["note"] = ("track_map_ms_median: the C call alone, host-observed, median of %d frames (coarse_max 60, range 30, min 20, budget 1000).  "
                    "composition_ms_median: the same frame as existing public calls driven from Python (per-row records packed once; the numpy "
                    "selection, the gathers of records and finder states and the ctypes calls are in it).  "
                    "bench_pvs_frame_with_pvs: scripts/bench_pvs.py's frame in the same process -- PVS lists to the host, a numpy shuffle and "
                    "1000-point budget, mcp_track_frame (one stage, no coarse stage, no level-3 rule)." % frames)
    return line


if __name__ == "__main__":
    print(json.dumps(main()))
