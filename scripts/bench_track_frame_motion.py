"""mcp_track_frame_motion against the split sequence it replaces, per frame, at the c3 map (4 cameras 640x480, 1000 tracked points, images in
HBM; the scene and parameters of scripts/bench_track_record.py):
  (a) the split sequence, 2C + 2 waits: mcp_kf_make_lite_batch; mcp_kf_make_sbi (blur 0.75) and mcp_sbi_iterate_last per camera;
      mcp_sbi_se3_from_se2 per camera on the host (the averaging and the prior are left out of the timed region: the frame repeats, so the
      alignment is the identity and the prior is the start pose -- this favours (a)); mcp_track_map_record with imgs = NULL;
  (b) mcp_track_frame_motion with the frame's images: one submission, one wait.
Both with want_items = 0.  Host-observed medians of alternating pairs (a, b, a, b, ...) with their ranges; the run-to-run spread is the
larger of the two (max - min) / median.  `split-only` times (a) alone and uses nothing this entry added: the form to run on a commit that
has no mcp_track_frame_motion, as the baseline.  Prints one JSON line."""
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
    med = statistics.median(ts)
    return {"median_ms": med * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3, "frames_per_s": 1.0 / med, "spread": (max(ts) - min(ts)) / med}


def main(pairs=30, size=(640, 480), cams=4, per_level=(100, 80, 50, 20), split_only=False):
    from mcptam_amd import hip_rt, synth_img
    from mcptam_amd.keyframe import KeyFrame, _pose12, make_lite_batch
    from mcptam_amd.keyframe import lib as kf_lib
    from mcptam_amd.pvs import MapPointTable, TrackMapParams, TrackMapResult, TrackRecord, TrackRecordParams, _bind_track_map, _bind_track_record
    from mcptam_amd.taylor_camera import TaylorCamera, camera_array
    sc = synth_img.make_tracking_scene(size=size)
    src = KeyFrame(*size)
    src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
    pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"], per_level=per_level) * cams
    wp, pr, pd = synth_img.points_soa(pts)
    n = len(wp)
    level = np.array([p["source_level"] for p in pts], dtype=np.int32)
    center = np.array([p["center"] for p in pts], dtype=np.int32)
    rng = np.random.default_rng(3)
    inl, outl = rng.integers(1, 31, n).astype(np.int32), rng.integers(0, 31, n).astype(np.int32)
    carr = camera_array([sc["cam"]] * cams)
    cam_sbi = TaylorCamera(sc["cam"].params, size, size, (40, 30))
    sarr = camera_array([cam_sbi] * cams)
    cfb = np.ascontiguousarray(np.stack([_pose12(np.eye(3), np.zeros(3)) for _ in range(cams)]))
    frame_img = np.ascontiguousarray(sc["imgB"])
    ring = [hip_rt.dev_alloc(frame_img.nbytes) for _ in range(cams)]
    for r in ring:
        hip_rt.dev_upload(r, frame_img)
    ip = (ctypes.c_void_p * cams)(*ring)
    st = (ctypes.c_int * cams)(*([size[0]] * cams))
    prm = TrackMapParams(1, 60, 30, 20, 8, 1000, 0, 12345)
    rp = TrackRecordParams(0, 0, 10, 20, 0.3, 0.13)
    bfw0 = _pose12(*sc["poseB"])
    res, rec = TrackMapResult(), TrackRecord()

    def table():
        t = MapPointTable()
        t.set(wp, pr, pd, np.ones(n, np.uint8))
        t.set_source(np.arange(n, dtype=np.int32), [src] * n, level, center, np.zeros(n, dtype=np.uint8))
        t.set_counts(inl, outl)
        return t
    A, ka = table(), [KeyFrame(*size) for _ in range(cams)]
    L = _bind_track_record(_bind_track_map(A._L))
    K = kf_lib()
    ha = (ctypes.c_void_p * cams)(*[k._h for k in ka])
    make_lite_batch(ka, ring, on_device=True)
    for k in ka:
        k.MakeSBI(0.75)
    se2, score, R3 = np.zeros(6), ctypes.c_double(0), np.zeros(9)

    def split():
        b = bfw0.copy()
        ok = K.mcp_kf_make_lite_batch(cams, ha, ip, st, 1, None) == 0
        for c in range(cams):
            ok = ok and K.mcp_kf_make_sbi(ka[c]._h, ctypes.c_double(0.75)) == 0
        for c in range(cams):
            ok = ok and K.mcp_sbi_iterate_last(ka[c]._h, 6, se2.ctypes.data, ctypes.byref(score)) == 0
            ok = ok and K.mcp_sbi_se3_from_se2(se2.ctypes.data, ctypes.byref(sarr[c]), ctypes.byref(sarr[c]), R3.ctypes.data) == 0
        ok = ok and L.mcp_track_map_record(A._h, cams, ha, None, None, 0, None, ctypes.cast(carr, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data, ctypes.byref(prm),
                                           ctypes.byref(res), ctypes.byref(rp), ctypes.byref(rec)) == 0
        if not ok:
            raise RuntimeError("the split sequence failed")
    one = None
    if not split_only:
        from mcptam_amd.pvs import TrackMotion, _bind_track_motion, motion_params
        B, kb = table(), [KeyFrame(*size) for _ in range(cams)]
        _bind_track_motion(L)
        hb = (ctypes.c_void_p * cams)(*[k._h for k in kb])
        mp, mo = motion_params(np.zeros(6), 1.0 / 30, [1] * cams, ncam=cams), TrackMotion()

        def one():
            b = bfw0.copy()
            if L.mcp_track_frame_motion(B._h, cams, hb, ip, st, 1, None, ctypes.cast(carr, ctypes.c_void_p), ctypes.cast(sarr, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data,
                                        ctypes.byref(prm), ctypes.byref(res), ctypes.byref(rp), ctypes.byref(rec), ctypes.byref(mp), ctypes.byref(mo)) != 0:
                raise RuntimeError("track_frame_motion failed")
    for _ in range(3):
        split()
        if one:
            one()
    ta, tb = [], []
    for _ in range(pairs):
        t0 = time.perf_counter(); split(); t1 = time.perf_counter()
        ta.append(t1 - t0)
        if one:
            one(); tb.append(time.perf_counter() - t1)
    out = {"metric": "TrackFrame's tracking branch per frame, c3 (%d cameras %dx%d, %d tracked points, images in HBM)" % (cams, size[0], size[1], n),
           "a_split_sequence": _stats(ta), "waits_a": 2 * cams + 2, "items": sum(rec.n_items[c] for c in range(cams)), "found": sum(rec.n_meas[c] for c in range(cams)),
           "note": "host-observed, %d alternating pairs after 3 warm-up pairs" % pairs}
    if one:
        sa, sb = _stats(ta), _stats(tb)
        out["b_track_frame_motion"] = sb
        out["waits_b"] = 1
        out["speedup_b_over_a"] = sa["median_ms"] / sb["median_ms"]
        out["spread"] = max(sa["spread"], sb["spread"])
        out["n_used"] = mo.n_used
    for r in ring:
        hip_rt.dev_free(r)
    return out


if __name__ == "__main__":
    print(json.dumps(main(split_only=len(sys.argv) > 1 and sys.argv[1] == "split-only")))
