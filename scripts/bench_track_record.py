"""mcp_track_map_record against the device-side path it replaces, per frame, at the c3 map and at the 50k-point map of
scripts/bench_track_map.py (same scene, cameras, images in HBM, parameters):
  (a) mcp_track_map with its 320-byte items in pinned memory, then mcp_scene_depth_robust on lists prepared OUTSIDE the timed region -- the
      device side of the earlier path without its host walk over the items, the bar hardest to beat;
  (b) mcp_track_map_record with want_items = 0: notes (8 B per item), measurements (32 B per found item), counters, quality, marks into
      the count column and the scene depth in the same submission.
Host-observed medians of alternating pairs (a, b, a, b, ...) with their ranges.  Prints one JSON line."""
import ctypes
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


def main(pairs=15, size=(640, 480), cams=4, per_level=(100, 80, 50, 20), big=50000, seed=1, only=None):
    from mcptam_amd import hip_rt, synth_img
    from mcptam_amd.keyframe import KeyFrame, _pose12, make_lite_batch
    from mcptam_amd.pvs import (TRACK_MAP_ITEM_DTYPE, MapPointTable, SCENE_DEPTH_DTYPE, TrackMapParams, TrackMapResult, TrackRecord, TrackRecordParams,
                                _bind_track_map, _bind_track_record, _bind_write_back, track_record_restate)
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
    rp = TrackRecordParams(0, 0, 10, 20, 0.3, 0.13)
    bfw0 = _pose12(*sc["poseB"])

    def run_map(label, wp, pr, pd, us, level, center):
        n = len(wp)
        rng = np.random.default_rng(3)
        inl, outl = rng.integers(1, 31, n).astype(np.int32), rng.integers(0, 31, n).astype(np.int32)
        tabs = []
        for _ in range(2):
            t = MapPointTable()
            t.set(wp, pr, pd, us)
            t.set_source(np.arange(n, dtype=np.int32), [src] * n, level, center, np.zeros(n, dtype=np.uint8))
            t.set_counts(inl, outl)
            tabs.append(t)
        A, B = tabs
        L = _bind_write_back(_bind_track_record(_bind_track_map(A._L)))
        res, rec = TrackMapResult(), TrackRecord()

        def plain():
            b = bfw0.copy()
            if L.mcp_track_map(A._h, cams, hs, ip, st, 1, None, ctypes.cast(carr, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data, ctypes.byref(prm), ctypes.byref(res)) != 0:
                raise RuntimeError("track_map failed")
            return b
        # the lists of (a)'s scene-depth call, from a first frame's items: prepared once, outside the timed region
        b = plain()
        items = []
        for c in range(cams):
            cnt = ctypes.c_int(0)
            ptr = L.mcp_track_map_view(A._h, c, ctypes.byref(cnt))
            items.append(np.frombuffer((ctypes.c_char * (cnt.value * TRACK_MAP_ITEM_DTYPE.itemsize)).from_address(ptr), dtype=TRACK_MAP_ITEM_DTYPE).copy()
                         if cnt.value else np.zeros(0, dtype=TRACK_MAP_ITEM_DTYPE))
        rs = track_record_restate(items, (inl, outl), False, cams)
        ss, sr, sw = rs["seg_start"], np.ascontiguousarray(rs["seg_rows"]), np.ascontiguousarray(rs["seg_w"])
        cfw = np.ascontiguousarray(np.tile(b, (cams, 1)))                       # (CamFromBase is the identity here)
        depth = np.zeros(cams, dtype=SCENE_DEPTH_DTYPE)

        def path_a():
            plain()
            if L.mcp_scene_depth_robust(A._h, cams, cfw.ctypes.data, ss.ctypes.data, sr.ctypes.data, sw.ctypes.data, depth.ctypes.data, None) != 0:
                raise RuntimeError("scene_depth_robust failed")

        def path_b():
            b2 = bfw0.copy()
            if L.mcp_track_map_record(B._h, cams, hs, ip, st, 1, None, ctypes.cast(carr, ctypes.c_void_p), b2.ctypes.data, cfb.ctypes.data, ctypes.byref(prm), ctypes.byref(res),
                                      ctypes.byref(rp), ctypes.byref(rec)) != 0:
                raise RuntimeError("track_map_record failed")
        for _ in range(3):
            path_a(); path_b()
        ta, tb = [], []
        for _ in range(pairs):
            t0 = time.perf_counter(); path_a(); t1 = time.perf_counter(); path_b(); t2 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1)
        n_items, n_meas = sum(rec.n_items[c] for c in range(cams)), sum(rec.n_meas[c] for c in range(cams))
        out = {"map": label, "points": n, "cameras": cams, "a_track_map_items_then_scene_depth": _stats(ta), "b_track_map_record_no_items": _stats(tb),
               "items": n_items, "found": n_meas, "bytes_down_a": 320 * n_items, "bytes_down_b": 8 * n_items + 32 * n_meas,
               "n_inliers": rec.n_inliers, "quality": [rec.quality[c] for c in range(cams)], "depth_refreshed": [rec.depth[c].refreshed for c in range(cams)]}
        for t in tabs:
            t.close()
        return out

    maps = []
    if only in (None, "c3"):
        c3_pts = base_pts * cams
        wp3, pr3, pd3 = synth_img.points_soa(c3_pts)
        lv3 = np.array([p["source_level"] for p in c3_pts], dtype=np.int32)
        cx3 = np.array([p["center"] for p in c3_pts], dtype=np.int32)
        maps.append(run_map("c3 scene", wp3, pr3, pd3, np.ones(len(wp3), np.uint8), lv3, cx3))
    if only in (None, "big"):
        wpb, prb, pdb, usb = synth_img.make_map_cloud(base_pts, big, seed=seed)
        maps.append(run_map("%d points" % big, wpb, prb, pdb, usb, np.zeros(big, dtype=np.int32), np.tile(np.array([[320, 240]], dtype=np.int32), (big, 1))))
    for r in ring:
        hip_rt.dev_free(r)
    return {"metric": "TrackMap of a frame with its bookkeeping (%d cameras %dx%d, images in HBM)" % (cams, size[0], size[1]), "maps": maps,
            "note": "host-observed, %d alternating pairs after 3 warm-up pairs; (a) = mcp_track_map with items + mcp_scene_depth_robust on lists prepared outside "
                    "the timed region, (b) = mcp_track_map_record with want_items = 0" % pairs}


if __name__ == "__main__":
    print(json.dumps(main(only=sys.argv[1] if len(sys.argv) > 1 else None)))
