"""How a device map begins and is rescaled, against the upload paths these calls replace, in one run:
  init-depth  mcp_init_depth_map_points of one MKF at level 1, 4 cameras x 300 candidates (one submission, one wait), against the composition: the
              busy lists from a host copy of the store, the points on the host (mcp_init_depth_points_host, the reference's loop), then
              mcp_map_points_update, _update_rays, _update_counts, _update_source, mcp_map_graph_update_points, mcp_map_graph_add_meas and a wait;
  rescale     mcp_map_rescale of a 50k-row / 200-MKF map (one submission, one wait), against the host scaling its own arrays
              (mcp_map_transform_host), sending every row and every MKF up again (mcp_map_points_set, mcp_map_graph_set_mkfs) and refreshing the
              depths (mcp_graph_refresh_depth).
Each timed call starts from the same state (the init-depth entries are erased and the store compacted outside the timed region; the rescale
alternates s and 1/s).  Device milliseconds are the calls' own event pairs (MapGraph.life_last_timing); the comparison is in host-observed
times, warmed up, with their ranges, because the upload paths are several calls.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SRC_MKF = 0
LEVEL = 1


def _stats(ts, scale=1e3):
    return {"median_ms": statistics.median(ts) * scale, "min_ms": min(ts) * scale, "max_ms": max(ts) * scale}


def bench_init(rounds, warmup, ncam=4, n_cand=300):
    import map_life_cases as mlc
    from mcptam_amd import map_graph as mg, stereo as S, synth_img
    from mcptam_amd.keyframe import KeyFrame
    from mcptam_amd.pvs import MapPointTable
    from mcptam_amd.synth import so3_exp
    sc = synth_img.make_stereo_scene()
    kfs = []
    for im in [sc["img_src"]] + list(sc["imgs"][:ncam - 1]):
        k = KeyFrame(640, 480)
        k.MakeKeyFrame_Lite(im)
        kfs.append(k)
    cams = [mlc.cameras()[c % 2] for c in range(ncam)]
    rng = np.random.default_rng(5)
    cfb = mg.poses12(np.stack([so3_exp(rng.uniform(-0.5, 0.5, 3)) for _ in range(ncam)]), rng.uniform(-0.1, 0.1, (ncam, 3)))
    cands = [mlc.grid_candidates(n_cand, LEVEL, x0=6 + c) for c in range(ncam)]
    limits = [n_cand] * ncam
    n_store, n_old = 20000, 5000                               # a store the gather has to pass over, none of it the source MKF's
    i = np.arange(n_store)
    st = dict(mkf=(1 + i % 7).astype(np.int32), cam=((i // 7) % ncam).astype(np.int32), row=(i // (7 * ncam) + (i % 7) * 700).astype(np.int32) % n_old,
              uv=rng.uniform([0, 0], [640, 480], (n_store, 2)), level=rng.integers(0, 4, n_store).astype(np.int32), source=np.zeros(n_store, dtype=np.int32))
    key = st["mkf"].astype(np.int64) * 10**7 + st["cam"] * 10**5 + st["row"]
    uniq = np.unique(key, return_index=True)[1]
    st = {k: v[np.sort(uniq)] for k, v in st.items()}
    n_store = len(st["mkf"])
    total = ncam * n_cand
    rows = (n_old + rng.permutation(2 * total)[:total]).astype(np.int32)
    keys = (100000 + np.arange(total)).astype(np.int32)
    bfw = mlc.mkf_poses(8)

    def world():
        t = MapPointTable()
        t.resize(int(rows.max()) + 1)
        g = mg.MapGraph(t, cfb)
        g.set_mkfs(bfw, np.full(8, mg.MKF_PRESENT), np.ones((8, ncam)), np.ones((8, ncam)))
        g.add_meas(st["mkf"], st["cam"], st["row"], st["uv"], st["level"], st["source"])
        return t, g
    worlds = [world(), world()]
    host_store = np.zeros(n_store, dtype=mg.STORE_ENTRY_DTYPE)
    for k in ("mkf", "cam", "row", "uv", "level", "source"):
        host_store[k] = st[k]
    host_store["alive"] = 1
    dev_ms = []

    def one_call(t, g):
        pts = g.add_init_depth_points(kfs, cams, cands, limits, rows, keys, SRC_MKF, LEVEL, 2.0)[0]
        dev_ms.append(g.life_last_timing()[0])
        return pts

    def composition(t, g):
        busy = [S.stereo_busy_ref(host_store, SRC_MKF, c) for c in range(ncam)]
        h = mg.init_depth_host(cfb, bfw[SRC_MKF], cams, cands, limits, busy, rows, SRC_MKF, LEVEL, 2.0, n_store)
        made = h["made_total"]
        r = rows[:made]
        t.update(r, h["world_pos"], h["pixel_right_w"], h["pixel_down_w"], np.zeros(made, dtype=np.uint8))
        t.update_rays(r, h["rays"][:, :3], h["rays"][:, 3:6], h["rays"][:, 6:])
        t.update_counts(r, np.ones(made, dtype=np.int32), np.zeros(made, dtype=np.int32))
        t.update_source(r, keys[:made], [kfs[c] for c in np.repeat(np.arange(ncam), h["made"])], np.full(made, LEVEL), h["center_xy"])
        g.update_points(r, h["gp_src_mkf"], h["gp_src_cam"], h["gp_flags"])
        ap = h["appended"]
        g.add_meas(ap["mkf"], ap["cam"], ap["row"], ap["uv"], ap["level"], ap["source"])
        g.num_meas()                                           # the wait (the uploads only enqueue)
        return h["points"]

    def reset(t, g, pts):
        made = len(pts)
        g.erase_meas(np.full(made, SRC_MKF), np.repeat(np.arange(ncam), n_cand)[:made], rows[:made])
        g.compact()
        assert g.num_meas() == (n_store, n_store)              # (waits: the timed region starts on an idle stream)
    paths = (one_call, composition)
    first = [p(*w) for p, w in zip(paths, worlds)]
    assert len(first[0]) == len(first[1]) == total, "the two paths disagree"
    snaps = []
    for t, g in worlds:
        m = g.get_meas()
        snaps.append([m[k].tobytes() for k in sorted(m)] + [a.tobytes() for a in t.get()] + [v.tobytes() for v in t.get_source().values()] + [t.get_rays()[0].tobytes()])
    same = snaps[0] == snaps[1] and first[0].tobytes() == first[1].tobytes()      # (reported, not required: the tests hold the two to each other)
    del dev_ms[:]
    times = ([], [])
    for i in range(warmup + rounds):
        for w, pts in zip(worlds, first):
            reset(*w, pts)
        for k in range(2):
            q = (i + k) % 2
            t0 = time.perf_counter(); paths[q](*worlds[q]); t1 = time.perf_counter()
            if i >= warmup:
                times[q].append(t1 - t0)
    dev = dev_ms[warmup:]
    return {"cameras": ncam, "candidates_per_camera": n_cand, "made": total, "level": LEVEL, "store": n_store, "rounds": rounds, "paths_leave_the_same_bytes": bool(same),
            "one_call_device_ms": {"median_ms": statistics.median(dev), "min_ms": min(dev), "max_ms": max(dev)},
            "one_call_host_observed": _stats(times[0]), "composition_host_observed": _stats(times[1]),
            "composition_over_one_call": statistics.median(times[1]) / statistics.median(times[0])}


def bench_rescale(rounds, warmup, n_rows=50000, n_mkfs=200):
    import map_life_cases as mlc
    from mcptam_amd import map_graph as mg
    from mcptam_amd.pvs import MapPointTable
    a = mlc.map_arrays(n_rows, n_mkfs=n_mkfs)
    rng = np.random.default_rng(9)
    per_row = 3
    r = np.repeat(np.arange(n_rows), per_row)
    j = np.arange(len(r))
    st = dict(mkf=((r * 7 + j) % n_mkfs).astype(np.int32), cam=(j % 2).astype(np.int32), row=r.astype(np.int32), uv=rng.uniform([0, 0], [640, 480], (len(r), 2)),
              level=(j % 4).astype(np.int32), source=np.zeros(len(r), dtype=np.int32))
    key = st["mkf"].astype(np.int64) * 10**7 + st["cam"] * 10**6 + st["row"]
    keep = np.sort(np.unique(key, return_index=True)[1])
    st = {k: v[keep] for k, v in st.items()}
    slots = np.arange(n_mkfs, dtype=np.int32)

    def world():
        t = MapPointTable()
        t.set(a["world_pos"], a["pixel_right_w"], a["pixel_down_w"], np.ones(n_rows, dtype=np.uint8))
        t.set_rays(a["rays"][:, :3], a["rays"][:, 3:6], a["rays"][:, 6:])
        g = mg.MapGraph(t, a["cam_from_base"])
        g.set_mkfs(a["base_from_world"], a["mkf_flags"], a["kf_active"], a["kf_depth_mean"])
        g.update_points(np.arange(n_rows), a["src_mkf"], a["src_cam"], a["pt_flags"])
        g.add_meas(st["mkf"], st["cam"], st["row"], st["uv"], st["level"], st["source"])
        g.refresh_depth(slots)
        return t, g
    (ta, ga), (tb, gb) = world(), world()
    host = dict(a)                                              # the host's own copy of the map, which the upload path scales and sends
    dev_ms, host_ms = [], []

    def one_call(s):
        res = ga.rescale(s)[0]
        dev_ms.append(ga.life_last_timing()[1])
        return res

    def upload_path(s):
        t0 = time.perf_counter()
        out, _ = mg.map_transform_host(host, scale=s)
        host.update(out)
        host_ms.append(time.perf_counter() - t0)
        tb.set(host["world_pos"], host["pixel_right_w"], host["pixel_down_w"], np.ones(n_rows, dtype=np.uint8))
        gb.set_mkfs(host["base_from_world"], a["mkf_flags"], a["kf_active"], a["kf_depth_mean"])
        return gb.refresh_depth(slots)                         # (waits)
    res = one_call(2.0)
    upload_path(2.0)
    assert res["n_refreshed"] == n_rows and res["n_mkfs"] == n_mkfs
    same = all(x.tobytes() == y.tobytes() for x, y in zip(ta.get(), tb.get()))      # (reported, not required: the tests hold the two to each other)
    for k in ("base_from_world", "kf_depth_mean"):
        same = same and ga.get_mkfs(0, n_mkfs)[k].tobytes() == gb.get_mkfs(0, n_mkfs)[k].tobytes()
    del dev_ms[:], host_ms[:]
    times = ([], [])
    paths = (one_call, upload_path)
    for i in range(warmup + rounds):
        s = 0.5 if i % 2 == 0 else 2.0
        for k in range(2):
            q = (i + k) % 2
            ga.num_meas(); gb.num_meas()
            t0 = time.perf_counter(); paths[q](s); t1 = time.perf_counter()
            if i >= warmup:
                times[q].append(t1 - t0)
    dev, hm = dev_ms[warmup:], host_ms[warmup:]
    return {"rows": n_rows, "mkfs": n_mkfs, "store": int(len(st["mkf"])), "rounds": rounds, "paths_leave_the_same_bytes": bool(same),
            "one_call_device_ms": {"median_ms": statistics.median(dev), "min_ms": min(dev), "max_ms": max(dev)},
            "one_call_host_observed": _stats(times[0]), "upload_path_host_observed": _stats(times[1]), "upload_path_host_arithmetic": _stats(hm),
            "upload_path_over_one_call": statistics.median(times[1]) / statistics.median(times[0])}


def main(rounds=60, warmup=6):
    res = {"bench": "map_lifecycle", "init_depth": bench_init(rounds, warmup), "rescale": bench_rescale(max(rounds // 3, 10), 3)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
