"""The two ways a tracked frame's measurements reach the map graph's store, at the c3 frame (4 cameras, about 1000 measurements):
  (a) mcp_meas_parcel_from_track + mcp_meas_parcel_commit: one launch, then one copy of the lane tables, two launches and one wait;
  (b) the earlier way: read the four measurement views, drop the measurements of bad points, pack the six arrays and hand them to
      mcp_map_graph_add_meas (which packs them again into pinned memory and copies them up), then wait for the stream.
Both end in a device synchronise and append the same entries (checked once, before timing).  Each timed call starts from the same store: the
MKF's entries are erased and the store compacted outside the timed region.  Host-observed times of alternating pairs (a, b, a, b, ...), warmed
up, with their ranges.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np


def _stats(ts):
    return {"median_us": statistics.median(ts) * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6}


def main(pairs=1000, warmup=50, size=(640, 480), cams=4, per_level=(100, 80, 50, 20)):
    from mcptam_amd import map_graph as mg
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame, make_lite_batch
    from mcptam_amd.pvs import MapPointTable
    sc = synth_img.make_tracking_scene(size=size)
    src = KeyFrame(*size)
    src.MakeKeyFrame_Lite(sc["imgA"]); src.MakeKeyFrame_Rest()
    pts = synth_img.make_map_points(sc["cam"], src, None, sc["poseA"], sc["depth"], per_level=per_level)
    wp, pr, pd = synth_img.points_soa(pts)
    n = len(pts)
    targets = [KeyFrame(*size) for _ in range(cams)]
    make_lite_batch(targets, [sc["imgB"]] * cams)
    rng = np.random.default_rng(3)
    t = MapPointTable()
    t.set(wp, pr, pd, np.ones(n, dtype=np.uint8))
    keys = np.arange(n, dtype=np.int32) * 3 + 7
    t.set_source(keys, [src] * n, np.array([p["source_level"] for p in pts], dtype=np.int32), np.array([p["center"] for p in pts], dtype=np.int32), np.zeros(n, dtype=np.uint8))
    t.set_counts(rng.integers(1, 31, n).astype(np.int32), rng.integers(0, 31, n).astype(np.int32))
    ident = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    flags = np.where(rng.random(n) < 0.05, mg.GP_BAD, 0).astype(np.int32)
    slot = 1

    def graph():
        g = mg.MapGraph(t, np.tile(ident, (cams, 1)))
        g.set_mkfs(np.tile(ident, (3, 1)), np.full(3, mg.MKF_PRESENT), np.ones((3, cams)), np.ones((3, cams)))
        g.update_points(np.arange(n), np.zeros(n), rng.integers(0, cams, n), flags)
        return g

    def reset(g):
        g.erase_mkf(slot); g.compact()
        g.set_mkfs(ident[None], [mg.MKF_PRESENT], np.ones((1, cams)), np.ones((1, cams)), first=slot)
        g.num_meas()                                   # (waits: the timed region starts on an idle stream)
    ga, gb = graph(), graph()
    cfbs = [(np.eye(3), np.zeros(3))] * cams
    out = t.track_map_record(targets, [sc["cam"]] * cams, sc["poseB"], cfbs, want_items=False, try_coarse=1, coarse_max=60, coarse_range=30, coarse_min=20,
                             coarse_subpix_its=8, max_patches=1000, seed=12345, copy=False)
    meas = out[4]                                      # views of the pinned block, as the shim reads them
    n_meas = sum(len(m) for m in meas)
    parcel = mg.MeasParcel(t)
    lane_mkf, lane_cam = np.full(cams, slot, dtype=np.int32), np.arange(cams, dtype=np.int32)
    bad = (flags & mg.GP_BAD) != 0

    def path_a():
        parcel.fill_from_track()
        return ga.commit_parcel(parcel, lane_mkf, lane_cam, 1, mg.SRC_TRACKER)[0]["n_appended"]

    def path_b():
        row = np.concatenate([m["row"] for m in meas])
        keep = ~bad[row]
        cam = np.concatenate([np.full(len(m), c, dtype=np.int32) for c, m in enumerate(meas)])[keep]
        uv = np.concatenate([m["found_pos"] for m in meas])[keep]
        level = np.concatenate([m["level"] for m in meas])[keep]
        k = int(keep.sum())
        gb.add_meas(np.full(k, slot, dtype=np.int32), cam, row[keep], uv, level, np.zeros(k, dtype=np.int32))
        gb.num_meas()                                  # the wait (add_meas only enqueues its copy)
        return k
    ka, kb = path_a(), path_b()
    sa, sb = ga.get_meas(), gb.get_meas()
    assert ka == kb and all(sa[f].tobytes() == sb[f].tobytes() for f in sa), "the two paths disagree"
    ta, tb = [], []
    for i in range(warmup + pairs):
        reset(ga); reset(gb)
        first, second = (path_a, path_b) if i % 2 == 0 else (path_b, path_a)      # (which of the two goes first alternates as well)
        t0 = time.perf_counter(); first(); t1 = time.perf_counter()
        second(); t2 = time.perf_counter()
        if i >= warmup:
            (ta if i % 2 == 0 else tb).append(t1 - t0); (tb if i % 2 == 0 else ta).append(t2 - t1)
    res = {"bench": "parcel_commit", "cams": cams, "rows": n, "measurements": n_meas, "appended": ka, "pairs": pairs,
           "parcel_from_track_commit": _stats(ta), "views_pack_add_meas": _stats(tb), "ratio_b_over_a": statistics.median(tb) / statistics.median(ta)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
