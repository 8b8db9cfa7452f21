"""MapMakerServerBase::ReFind_Common over the resident map-point table: one mcp_map_refind against the composition the map maker's
ReFindBatch used before it -- mcp_patch_sequences(MCP_PF_REFIND, range 4) on items packed from the same columns, one mcp_pf_item and (per
sequence) one mcp_pf_state up, one mcp_td_out per pair down, verdicts derived on the host.  The packing is inside the timed region, since the
map maker pays it on every call; it is done with vectorised numpy stores into the C structs (no Python loop), as a native caller's loop of
struct stores would.  The target tables of both paths are marshalled once, outside.  Two shapes:
  single_keyframe   ReFindInSingleKeyFrame: 50 000 rows x 1 target, every pair its own finder;
  newly_made        ReFindNewlyMade: 64 rows x 800 targets (two keyframe handles alternating, poses jittered around view B), one finder per row.
Both paths are timed alternately in one process after warm-up and a check that they agree; host clock around calls that end in their own wait;
medians.  The kernel split comes from a separate `rocprofv3 --kernel-trace --stats -- python scripts/bench_refind.py` run.  One JSON line."""
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

TD_IN_DTYPE = np.dtype([("world_pos", "f8", 3), ("pixel_right_w", "f8", 3), ("pixel_down_w", "f8", 3), ("source_kf", "u8"), ("source_level", "i4"),
                        ("center_x", "i4"), ("center_y", "i4"), ("fixed", "i4")], align=True)
PF_ITEM_DTYPE = np.dtype([("point", TD_IN_DTYPE), ("point_key", "i4"), ("target", "i4"), ("start_pos", "f8", 2)], align=True)


def _shape(name, table, cols, src_handle, targets, pairs, per_row, reps, warm):
    from mcptam_amd import keyframe as K
    from mcptam_amd.refind import marshal_targets, refind_verdicts
    assert PF_ITEM_DTYPE.itemsize == ctypes.sizeof(K.PfItem) and TD_IN_DTYPE.itemsize == ctypes.sizeof(K.TdIn)
    L = K.lib()
    n = len(pairs)
    rf_targets = marshal_targets(targets)
    ident = (np.eye(3), np.zeros(3))
    keep, ntar, tab, _, _, _ = K.marshal_patch_sequences([(kf, cam, pose, ident) for kf, cam, pose in targets], [], lambda k: k._h, lambda k: k._h)

    def one_call():
        return table.refind(rf_targets, pairs, per_row, K.new_pf_states(1), view=True)

    def composition():
        rows = pairs[:, 0]
        head = np.ones(n, dtype=bool)
        if per_row:
            head[1:] = rows[1:] != rows[:-1]
        seq_start = np.concatenate([np.nonzero(head)[0], [n]]).astype(np.int32)
        items = np.zeros(n, dtype=PF_ITEM_DTYPE)
        pt = items["point"]
        pt["world_pos"] = cols["wp"][rows]; pt["pixel_right_w"] = cols["pr"][rows]; pt["pixel_down_w"] = cols["pd"][rows]
        pt["source_kf"] = src_handle; pt["source_level"] = cols["level"][rows]
        pt["center_x"] = cols["center"][rows, 0]; pt["center_y"] = cols["center"][rows, 1]; pt["fixed"] = cols["fixed"][rows]
        items["point_key"] = cols["keys"][rows]; items["target"] = pairs[:, 1]
        states = K.new_pf_states(len(seq_start) - 1)
        out = np.zeros(n, dtype=K.TD_OUT_DTYPE)
        rc = L.mcp_patch_sequences(K.PF_REFIND, ntar, tab, len(states), seq_start.ctypes.data, items.ctypes.data, states.ctypes.data, 4, 8, 0, out.ctypes.data)
        assert rc == 0
        v, m = refind_verdicts(out, pairs)
        return v, m, states[-1:]

    for _ in range(warm):
        a = one_call()
        b = composition()
    assert np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1])
    for f in a[1].dtype.names:
        assert np.array_equal(a[1][f], b[1][f]), f
    assert a[3].tobytes() == b[2].tobytes()
    counts = [int(c) for c in a[2]]
    t_one, t_comp = [], []
    for _ in range(reps):                                  # alternating: both see the same machine
        t0 = time.perf_counter(); one_call(); t1 = time.perf_counter(); composition(); t2 = time.perf_counter()
        t_one.append((t1 - t0) * 1e3); t_comp.append((t2 - t1) * 1e3)
    med = statistics.median
    del keep
    return {"shape": name, "pairs": n, "targets": len(targets), "per_row_finders": bool(per_row), "counts": counts, "reps": reps,
            "one_call_ms_median": med(t_one), "one_call_ms_min": min(t_one), "one_call_ms_max": max(t_one),
            "composition_ms_median": med(t_comp), "composition_ms_min": min(t_comp), "composition_ms_max": max(t_comp),
            "ratio": med(t_comp) / med(t_one),
            "bytes_up_one_call": 8 * n + 184, "bytes_down_one_call": n + 40 * counts[1] + 184,
            "bytes_up_composition": PF_ITEM_DTYPE.itemsize * n + 184 * (int(n) if not per_row else len(np.unique(pairs[:, 0]))),
            "bytes_down_composition": K.TD_OUT_DTYPE.itemsize * n + 184 * (int(n) if not per_row else len(np.unique(pairs[:, 0])))}


def main(reps=15, warm=3):
    from mcptam_amd import synth_img
    from mcptam_amd.keyframe import KeyFrame
    from mcptam_amd.pvs import MapPointTable
    from mcptam_amd.synth import so3_exp
    sc = synth_img.make_tracking_scene()
    A = KeyFrame(640, 480)
    A.MakeKeyFrame_Lite(sc["imgA"]); A.MakeKeyFrame_Rest()
    B = KeyFrame(640, 480)
    B.MakeKeyFrame_Lite(sc["imgB"])
    B2 = KeyFrame(640, 480)
    B2.MakeKeyFrame_Lite(np.ascontiguousarray(np.roll(sc["imgB"], 2, axis=1)))
    base = synth_img.make_map_points(sc["cam"], A, None, sc["poseA"], sc["depth"])
    nb = len(base)
    bw, bp, bd = synth_img.points_soa(base)
    wp, pr, pd, us = synth_img.make_map_cloud(base, 50000, seed=1)
    n = len(wp)
    level = np.random.default_rng(9).integers(0, 4, n).astype(np.int32)
    # rows 0 .. n-1: the 50 k cloud (sources at the level image's centre); rows n ..: the scene's own points
    cols = dict(wp=np.concatenate([wp, bw]), pr=np.concatenate([pr, bp]), pd=np.concatenate([pd, bd]), usable=np.concatenate([us, np.ones(nb, dtype=np.uint8)]),
                keys=np.arange(n + nb, dtype=np.int32),
                level=np.concatenate([level, [p["source_level"] for p in base]]).astype(np.int32),
                center=np.ascontiguousarray(np.concatenate([np.stack([320 >> level, 240 >> level], axis=1), [p["center"] for p in base]]).astype(np.int32)),
                fixed=np.zeros(n + nb, dtype=np.uint8))
    t = MapPointTable()
    t.set(cols["wp"], cols["pr"], cols["pd"], cols["usable"])
    t.set_source(cols["keys"], [A] * (n + nb), cols["level"], cols["center"], cols["fixed"])
    pB = sc["poseB"]
    single = _shape("single_keyframe", t, cols, A._h, [(B, sc["cam"], pB)], np.stack([np.arange(n), np.zeros(n, dtype=int)], axis=1).astype(np.int32), False, reps, warm)
    rng = np.random.default_rng(21)
    targets = [((B, B2)[k % 2], sc["cam"], (so3_exp(rng.normal(size=3) * 0.004) @ pB[0], pB[1] + rng.normal(size=3) * 0.01)) for k in range(800)]
    rows = n + np.arange(0, nb, nb // 64)[:64]
    pairs = np.stack([np.repeat(rows, 800), np.tile(np.arange(800), 64)], axis=1).astype(np.int32)
    newly = _shape("newly_made", t, cols, A._h, targets, pairs, True, reps, warm)
    t.close()
    return {"metric": "ReFind_Common over the resident table: one mcp_map_refind against mcp_patch_sequences(MCP_PF_REFIND) with its packing",
            "shapes": [single, newly],
            "note": "host-observed medians of alternating pairs; both calls end in their own wait; the composition's packing (numpy, vectorised) and its "
                    "verdict derivation are inside its time, the target tables of both paths are built once outside"}


if __name__ == "__main__":
    print(json.dumps(main()))
