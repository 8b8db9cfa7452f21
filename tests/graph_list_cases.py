"""Stores shared by the keyframe-list tests (tests/test_graph_lists_cpu.py, tests/test_graph_write_back_gpu.py): the three synthetic maps of
map_graph_cases and hand-made stores, each as (name, flat arrays, slots named by the call, rows of the table).  The flat arrays are
mcptam_amd.map_graph.problem_arrays' keys plus "inlier" / "outlier", the table's count column (absent: every row reads (1, 0))."""
import numpy as np

import map_graph_cases as mc
from mcptam_amd import map_graph as mg


def hand(seed, P, C, N, M, n_rows=None):
    """A seeded store of M distinct (mkf, cam, row) entries over P present MKFs, C cameras and N written graph columns of an n_rows table, all
    alive, every keyframe active, no bad row, seeded counts."""
    rng = np.random.default_rng([20261019, seed])
    n_rows = N if n_rows is None else n_rows
    a = dict(ncam=C, cam_from_base=np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (C, 1)))
    a["base_from_world"] = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (P, 1))
    a["mkf_flags"] = np.full(P, mg.MKF_PRESENT, dtype=np.int32)
    a["kf_active"] = np.ones((P, C), dtype=np.uint8)
    a["kf_depth_mean"] = np.full((P, C), 3.0)
    a["world_pos"] = rng.normal(size=(N, 3)) + np.array([0.0, 0.0, 5.0])
    a["src_mkf"], a["src_cam"], a["pt_flags"] = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    keys = rng.choice(P * C * max(N, 1), M, replace=False) if M else np.zeros(0, dtype=np.int64)
    a["ms_row"] = (keys % max(N, 1)).astype(np.int32)
    a["ms_cam"] = ((keys // max(N, 1)) % C).astype(np.int32)
    a["ms_mkf"] = (keys // (max(N, 1) * C)).astype(np.int32)
    a["ms_uv"] = rng.uniform(0, 480, (M, 2)); a["ms_level"] = rng.integers(0, 4, M).astype(np.int32); a["ms_source"] = np.zeros(M, dtype=np.int32)
    a["ms_alive"] = np.ones(M, dtype=np.uint8)
    a["inlier"] = rng.integers(1, 50, n_rows).astype(np.int32)
    a["outlier"] = rng.integers(0, 50, n_rows).astype(np.int32)
    return a


def _entries(a, mkf, cam, row):
    M = len(mkf)
    a["ms_mkf"], a["ms_cam"], a["ms_row"] = (np.asarray(v, dtype=np.int32) for v in (mkf, cam, row))
    a["ms_uv"], a["ms_level"], a["ms_source"], a["ms_alive"] = np.zeros((M, 2)), np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32), np.ones(M, dtype=np.uint8)
    return a


def map_cases():
    """The three maps: every MKF named in slot order, and a scrambled subset of them."""
    out = []
    for k, name in enumerate(("tiny", "tiny12", "band40")):
        a = mc.arrays(name)
        P = len(a["mkf_flags"])
        out.append((name + "-all", a, np.arange(P), len(a["pt_flags"])))
        out.append((name + "-some", a, np.random.default_rng(k).permutation(P)[:max(2, P // 3)], len(a["pt_flags"])))
    return out


def hand_cases():
    out = []
    out.append(("empty-store", hand(0, 2, 2, 5, 0), [1, 0], 5))
    out.append(("one-entry", _entries(hand(1, 3, 2, 5, 0), [2], [1], [4]), [0, 2], 5))
    out.append(("one-keyframe", _entries(hand(2, 3, 2, 50, 0), [1] * 50, [0] * 50, np.arange(50)[::-1]), [0, 1, 2], 50))
    k = np.random.default_rng(3).permutation(64 * 8)
    out.append(("64x8-one-each", _entries(hand(3, 64, 8, 600, 0), k // 8, k % 8, np.arange(512)), np.arange(64)[::-1], 600))
    a = hand(4, 6, 3, 80, 500); a["ms_alive"][::3] = 0
    out.append(("dead-entries", a, [5, 0, 3], 80))
    a = hand(5, 6, 3, 80, 500); a["pt_flags"][::4] |= mg.GP_BAD
    out.append(("bad-rows", a, np.arange(6), 80))
    a = hand(6, 4, 2, 40, 200, n_rows=40)                               # graph columns written for rows 0..19 only
    for k_ in ("world_pos", "src_mkf", "src_cam", "pt_flags"):
        a[k_] = a[k_][:20]
    out.append(("rows-past-the-graph-columns", a, np.arange(4), 40))
    a = hand(7, 4, 2, 40, 200, n_rows=25)                               # a table cut down to 25 rows under a store that names 40
    for k_ in ("world_pos", "src_mkf", "src_cam", "pt_flags"):
        a[k_] = a[k_][:25]
    a["load_rows"] = 40                                                 # (a device table has this many rows while the store is filled)
    out.append(("rows-past-the-table", a, np.arange(4), 25))
    a = hand(8, 4, 3, 40, 300); a["kf_active"][1, 1] = 0; a["kf_active"][3, :] = 0
    out.append(("inactive-camera", a, np.arange(4), 40))
    a = hand(9, 5, 2, 40, 200); keep = a["ms_mkf"] != 2
    _u = {k_: a[k_][keep] for k_ in ("ms_mkf", "ms_cam", "ms_row", "ms_uv", "ms_level", "ms_source", "ms_alive")}; a.update(_u)
    out.append(("listed-mkf-without-entries", a, [4, 2, 0], 40))
    out.append(("mkfs-not-listed", hand(10, 9, 2, 60, 600), [7, 1], 60))
    out.append(("row-seen-by-several-cameras", _entries(hand(11, 2, 4, 6, 0), [0, 0, 0, 0, 1, 1, 0], [0, 1, 2, 3, 0, 2, 1], [3, 3, 3, 3, 3, 3, 5]), [1, 0], 6))
    a = _entries(hand(12, 1, 1, 3, 0), [0, 0, 0], [0, 0, 0], [2, 0, 1])
    a["inlier"], a["outlier"] = np.array([1, 3, 1], dtype=np.int32), np.array([0, 1, 1000], dtype=np.int32)
    out.append(("counts", a, [0], 3))
    return out


def all_cases():
    return map_cases() + hand_cases()


def assert_same_lists(got, want):
    """(seg_start, seg_rows, seg_w): the integers equal, the weights equal in their bit patterns."""
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if k < 2:
            assert np.array_equal(g, w), k
        else:
            assert g.astype(np.float64).tobytes() == w.astype(np.float64).tobytes()
