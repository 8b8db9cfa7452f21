"""The ways the points of one AddStereoMapPoints call (one source keyframe, one level, three targets, the 640x480 fixture) reach the map:
  (a) mcp_stereo_map_points with busy_from_store = 1: the keyframe's busy positions gathered from the store, the points appended on the device,
      one wait;
  (b) mcp_stereo_map_points with busy_from_store = 0: the host packs its own measurement list, the points are appended on the device, one wait;
  (c) the composition it replaces: the host packs its measurement list, mcp_stereo_points (one wait, the records come down), then
      mcp_map_points_update, _update_rays, _update_source, mcp_map_graph_update_points, mcp_map_graph_add_meas and the wait that ends them.
The host's measurement list is a numpy copy here; the adapter walks a std::map for it, which costs more.  All three leave the same rows and the
same store (checked once, before timing).  Each timed call starts from the same state: the new entries are erased and the store compacted
outside the timed region.  Two stores: the fixture's (about 300 entries) and one of 400k entries, the size of a metric map, which costs the
gather of (a) a full pass.  Host-observed times of rotating triples, warmed up, with their ranges.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SRC_MKF, SRC_CAM = 0, 0
N_MKF = 64


def _stats(ts):
    return {"median_us": statistics.median(ts) * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6}


def _store(n_store, n_rows, n_src, rng):
    """n_src entries of the source keyframe at random image positions and levels, the rest spread over the other MKFs; distinct (mkf, cam, row)"""
    n_other = n_store - n_src
    i = np.arange(n_other)
    layer, row = i // n_rows, i % n_rows
    assert layer.max(initial=0) < 4
    mkf = 1 + (row + 17 * layer) % (N_MKF - 1)
    return dict(mkf=np.concatenate([np.full(n_src, SRC_MKF), mkf]).astype(np.int32), cam=np.concatenate([np.full(n_src, SRC_CAM), layer % 2]).astype(np.int32),
                row=np.concatenate([np.arange(n_src), row]).astype(np.int32), uv=rng.uniform([0, 0], [640, 480], (n_store, 2)),
                level=rng.integers(0, 4, n_store).astype(np.int32), source=np.zeros(n_store, dtype=np.int32))


def run(sc, src, tg, level, n_store, n_rows, rounds, warmup):
    from mcptam_amd import map_graph as mg, stereo as S
    from mcptam_amd.pvs import MapPointTable
    rng = np.random.default_rng(n_store)
    cand = src.Candidates(level)[0]
    targets = [(tg[j], sc["cam"], sc["poses"][j]) for j in range(3)]
    tmkf, tcam = np.array([1, 2, 3], dtype=np.int32), np.array([0, 1, 0], dtype=np.int32)
    st = _store(n_store, n_rows, 300, rng)
    rows = (n_rows + rng.permutation(2 * len(cand))[:len(cand)]).astype(np.int32)
    keys = (100000 + np.arange(len(cand))).astype(np.int32)
    ident = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])

    def world():
        t = MapPointTable()
        t.resize(int(rows.max()) + 1)
        g = mg.MapGraph(t, np.tile(ident, (2, 1)))
        g.set_mkfs(np.tile(ident, (N_MKF, 1)), np.full(N_MKF, mg.MKF_PRESENT), np.ones((N_MKF, 2)), np.ones((N_MKF, 2)))
        g.add_meas(st["mkf"], st["cam"], st["row"], st["uv"], st["level"], st["source"])
        return t, g
    worlds = [world() for _ in range(3)]
    own = st["mkf"] == SRC_MKF                               # the host's copy of the source keyframe's measurements (the adapter's mmpMeasurements)
    own_uv, own_level = st["uv"][own & (st["cam"] == SRC_CAM)], st["level"][own & (st["cam"] == SRC_CAM)]

    def path_a(t, g):
        return g.add_stereo_points(src, sc["cam"], sc["pose_src"], level, cand, targets, tmkf, tcam, rows, keys, SRC_MKF, SRC_CAM, busy_from_store=True, outcomes=False)[0]

    def path_b(t, g):
        meas = S.make_meas(own_uv, own_level)
        return g.add_stereo_points(src, sc["cam"], sc["pose_src"], level, cand, targets, tmkf, tcam, rows, keys, SRC_MKF, SRC_CAM, meas=meas, busy_from_store=False, outcomes=False)[0]

    def path_c(t, g):
        meas = S.make_meas(own_uv, own_level)
        pts = S.stereo_points(src, sc["cam"], sc["pose_src"], level, cand, targets, meas=meas, outcomes=False)[0]
        made = len(pts)
        r = rows[:made]
        t.update(r, pts["world_pos"], pts["pixel_right_w"], pts["pixel_down_w"], np.zeros(made, dtype=np.uint8))
        t.update_rays(r, pts["center_nc"], pts["one_right_nc"], pts["one_down_nc"])
        t.update_source(r, keys[:made], [src] * made, np.full(made, level), cand[pts["candidate"]])
        g.update_points(r, np.full(made, SRC_MKF), np.full(made, SRC_CAM), np.zeros(made, dtype=np.int32))
        g.add_meas(np.stack([np.full(made, SRC_MKF), tmkf[pts["target"]]], axis=1).ravel(), np.stack([np.full(made, SRC_CAM), tcam[pts["target"]]], axis=1).ravel(), np.repeat(r, 2),
                   np.stack([pts["root_pos"], pts["target_pos"]], axis=1).reshape(-1, 2), np.full(2 * made, level), np.tile([S.SRC_ROOT, S.SRC_EPIPOLAR], made))
        g.num_meas()                                       # the wait (the uploads only enqueue)
        return pts

    def reset(t, g, pts):
        made = len(pts)
        g.erase_meas(np.concatenate([np.full(made, SRC_MKF), tmkf[pts["target"]]]), np.concatenate([np.full(made, SRC_CAM), tcam[pts["target"]]]), np.tile(rows[:made], 2))
        g.compact()
        assert g.num_meas() == (n_store, n_store)          # (waits: the timed region starts on an idle stream)
    paths = (path_a, path_b, path_c)
    first = [p(*w) for p, w in zip(paths, worlds)]
    snaps = []
    for t, g in worlds:
        m = g.get_meas()
        snaps.append([m[k].tobytes() for k in sorted(m)] + [a.tobytes() for a in t.get()] + [v.tobytes() for v in t.get_source().values()] + [t.get_rays()[0].tobytes()])
    assert snaps[0] == snaps[1] == snaps[2] and first[0].tobytes() == first[2].tobytes(), "the three paths disagree"
    times = ([], [], [])
    for i in range(warmup + rounds):
        for w, pts in zip(worlds, first):
            reset(*w, pts)
        for k in range(3):                                  # (which of the three goes first rotates)
            q = (i + k) % 3
            t0 = time.perf_counter(); paths[q](*worlds[q]); t1 = time.perf_counter()
            if i >= warmup:
                times[q].append(t1 - t0)
    a, b, c = (statistics.median(x) for x in times)
    return {"level": level, "candidates": len(cand), "made": len(first[0]), "store": n_store, "busy": int(len(own_uv)), "rounds": rounds,
            "one_call_busy_from_store": _stats(times[0]), "one_call_host_list": _stats(times[1]), "composition": _stats(times[2]),
            "composition_over_store_mode": c / a, "composition_over_host_list_mode": c / b}


def main(rounds=200, warmup=20, level=1):
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame
    sc = synth_img.make_stereo_scene()
    src = KeyFrame(640, 480)
    src.MakeKeyFrame_Lite(sc["img_src"]); src.MakeKeyFrame_Rest()
    tg = []
    for im in sc["imgs"][:3]:
        g = KeyFrame(640, 480)
        g.MakeKeyFrame_Lite(im)
        tg.append(g)
    res = {"bench": "stereo_map", "size": [640, 480], "targets": 3,
           "fixture_store": run(sc, src, tg, level, 300 + 300, 1000, rounds, warmup), "map_store": run(sc, src, tg, level, 400000, 100000, rounds, warmup)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
