"""The host side of mcp_track_map_record (include/mcp_img.h): AssessTrackingQuality's arithmetic, the numpy restatement of the marks,
counters, measurements and scene-depth lists on hand-built items, and the record layouts against the header."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = dict(min_patches=10, coarse_min=20, good=0.3, bad=0.13)


def test_quality_below_min_patches_is_bad():
    from mcptam_amd.pvs import QUALITY_BAD, tracking_quality
    # 9 found of 9 attempted: every fraction is 1, only the count decides
    assert tracking_quality([3, 3, 3, 0], [3, 3, 3, 0], **Q) == QUALITY_BAD
    assert tracking_quality([0, 0, 0, 0], [0, 0, 0, 0], **Q) == QUALITY_BAD


def test_quality_good_dodgy_bad():
    from mcptam_amd.pvs import QUALITY_BAD, QUALITY_DODGY, QUALITY_GOOD, tracking_quality
    # total 40 / 100 > 0.3
    assert tracking_quality([50, 30, 10, 10], [20, 10, 5, 5], **Q) == QUALITY_GOOD
    # exactly 0.3 is not "> good"; large levels 10 / 40 = 0.25 >= 0.13
    assert tracking_quality([30, 30, 20, 20], [10, 10, 5, 5], **Q) == QUALITY_DODGY
    # total 20 / 100; large levels 2 / 40 = 0.05 < 0.13
    assert tracking_quality([30, 30, 20, 20], [10, 8, 1, 1], **Q) == QUALITY_BAD


def test_quality_large_level_fraction_needs_more_than_coarse_min():
    from mcptam_amd.pvs import QUALITY_BAD, QUALITY_DODGY, tracking_quality
    # 21 large attempts (> 20): their fraction 1 / 21 < 0.13 decides -> BAD
    assert tracking_quality([60, 19, 11, 10], [10, 9, 1, 0], **Q) == QUALITY_BAD
    # 20 large attempts (not > 20): the total fraction 20 / 99 = 0.2 stands in -> DODGY although the large fraction is 1 / 20
    assert tracking_quality([60, 19, 10, 10], [10, 9, 1, 0], **Q) == QUALITY_DODGY
    # nothing attempted with min_patches 0: 0 / 0 passes neither test
    assert tracking_quality([0, 0, 0, 0], [0, 0, 0, 0], 0, 20, 0.3, 0.13) == QUALITY_DODGY


def _items(rows):
    """rows: (point, stage, weight, searched, found, template_bad, level, did_subpix, found_pos)"""
    from mcptam_amd.pvs import TRACK_MAP_ITEM_DTYPE
    a = np.zeros(len(rows), dtype=TRACK_MAP_ITEM_DTYPE)
    for i, (p, st, w, s, f, b, l, sp, fp) in enumerate(rows):
        a[i]["point"], a[i]["stage"], a[i]["weight_last"] = p, st, w
        o = a[i]["out"]
        o["searched"], o["found"], o["template_bad"], o["search_level"], o["did_subpix"], o["found_pos"], o["in_image"] = s, f, b, l, sp, fp, 1
    return a


def _hand_built():
    cam0 = _items([(5, 0, 0.7, 1, 1, 0, 3, 1, (10.5, 20.25)),      # inlier
                   (2, 1, 0.0, 1, 1, 0, 3, 1, (1.0, 2.0)),         # found, weight 0: outlier
                   (9, 2, 0.0, 1, 0, 0, 1, 0, (0.0, 0.0)),         # searched, not found: outlier unless lost
                   (4, 2, 0.0, 0, 0, 1, 0, 0, (0.0, 0.0)),         # template bad, never searched: no mark, not attempted
                   (7, 2, 0.0, 0, 0, 0, -1, 0, (0.0, 0.0)),        # rejected warp: no mark, not attempted
                   (1, 2, 0.4, 1, 1, 0, 0, 0, (3.0, 4.0))])        # inlier
    cam1 = _items([(1, 1, 0.9, 1, 1, 0, 2, 1, (30.0, 40.0)),       # row 1 again: a second inlier mark
                   (5, 2, 0.0, 1, 1, 0, 1, 0, (7.0, 8.0)),         # row 5 again: an outlier mark
                   (9, 2, 0.0, 1, 0, 0, 1, 0, (0.0, 0.0))])        # row 9 again
    before = (np.array([1, 4, 2, 1, 3, 6, 1, 1, 1, 5]), np.array([0, 1, 0, 0, 2, 3, 0, 0, 0, 5]))
    return [cam0, cam1], before


def test_restate_marks_and_counts():
    from mcptam_amd.pvs import track_record_restate
    items, before = _hand_built()
    r = track_record_restate(items, before, lost=False, ncam=2)
    marks = [list(n["flags"] >> 6) for n in r["notes"]]
    assert marks == [[1, 2, 2, 0, 0, 1], [1, 2, 2]]
    inl, outl = r["counts"]
    assert list(inl - before[0]) == [0, 2, 0, 0, 0, 1, 0, 0, 0, 0]        # row 1: one inlier mark per camera
    assert list(outl - before[1]) == [0, 0, 1, 0, 0, 1, 0, 0, 0, 2]       # row 9: searched-not-found in both cameras
    assert r["n_inliers"] == 3 and r["n_outlier_marks"] == 4
    assert before[0][1] == 4                                              # (the input arrays are left alone)


def test_restate_lost_spares_the_not_found():
    from mcptam_amd.pvs import track_record_restate
    items, before = _hand_built()
    a, b = track_record_restate(items, before, lost=False, ncam=2), track_record_restate(items, before, lost=True, ncam=2)
    assert [list(n["flags"] >> 6) for n in b["notes"]] == [[1, 2, 0, 0, 0, 1], [1, 2, 0]]
    assert list(b["counts"][1] - before[1]) == [0, 0, 1, 0, 0, 1, 0, 0, 0, 0]
    assert b["n_outlier_marks"] == 2 and b["n_inliers"] == a["n_inliers"]
    assert np.array_equal(a["attempted"], b["attempted"]) and np.array_equal(a["found"], b["found"])
    for c in range(2):
        assert a["meas"][c].tobytes() == b["meas"][c].tobytes()


def test_restate_counters_measurements_and_lists():
    from mcptam_amd.pvs import TN_ATTEMPTED, TN_FOUND, TN_TEMPLATE_BAD, track_record_restate
    items, before = _hand_built()
    r = track_record_restate(items, before, lost=False, ncam=2)
    assert r["attempted"][0].tolist() == [1, 1, 0, 2] and r["found"][0].tolist() == [1, 0, 0, 2]      # template-bad and level -1 excluded
    assert r["attempted"][1].tolist() == [0, 2, 1, 0] and r["found"][1].tolist() == [0, 1, 1, 0]
    assert not r["attempted"][2:].any()
    n0 = r["notes"][0]
    assert n0["level"].tolist() == [3, 3, 1, 0, 255, 0] and n0["row"].tolist() == [5, 2, 9, 4, 7, 1] and set(r["notes"][1]["cam"]) == {1}
    assert (n0["flags"][3] & TN_TEMPLATE_BAD) and not (n0["flags"][3] & TN_ATTEMPTED) and not (n0["flags"][4] & TN_ATTEMPTED)
    assert (n0["flags"][0] & TN_FOUND) and (n0["flags"][0] & TN_ATTEMPTED)
    # measurements: the found items in item order
    assert r["meas"][0]["item"].tolist() == [0, 1, 5] and r["meas"][0]["row"].tolist() == [5, 2, 1]
    assert r["meas"][0]["found_pos"].tolist() == [[10.5, 20.25], [1.0, 2.0], [3.0, 4.0]] and r["meas"][0]["subpix"].tolist() == [1, 1, 0]
    assert r["meas"][1]["item"].tolist() == [0, 1] and r["meas"][1]["level"].tolist() == [2, 1]
    assert r["n_items"] == [6, 3] and r["n_meas"] == [3, 2]
    # scene-depth lists: weights from the counts after all marks of both cameras
    assert r["seg_start"].tolist() == [0, 3, 5] and r["seg_rows"].tolist() == [5, 2, 1, 1, 5]
    inl, outl = r["counts"]
    assert r["seg_w"].tolist() == [7 / 11, 2 / 3, 6 / 7, 6 / 7, 7 / 11]
    assert np.array_equal(r["seg_w"], inl[r["seg_rows"]] / (inl[r["seg_rows"]] + outl[r["seg_rows"]]))


def test_record_layouts_match_the_header(tmp_path):
    from mcptam_amd import pvs
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcp_img.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mcp_track_note), sizeof(mcp_track_meas), sizeof(mcp_track_record), '
                   'sizeof(mcp_track_record_params), offsetof(mcp_track_record, cam_from_world), offsetof(mcp_track_record, depth), '
                   'offsetof(mcp_track_meas, found_pos)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got[0] == 8 and got[1] == 32
    assert got == [ctypes.sizeof(pvs.TrackNote), ctypes.sizeof(pvs.TrackMeas), ctypes.sizeof(pvs.TrackRecord), ctypes.sizeof(pvs.TrackRecordParams),
                   pvs.TrackRecord.cam_from_world.offset, pvs.TrackRecord.depth.offset, pvs.TrackMeas.found_pos.offset]
    assert pvs.TRACK_NOTE_DTYPE.itemsize == 8 and pvs.TRACK_MEAS_DTYPE.itemsize == 32
    assert pvs.TRACK_MEAS_DTYPE.fields["found_pos"][1] == got[6]


def test_symbols_are_listed():
    from mcptam_amd import keyframe, pvs
    assert set(pvs.TRACK_RECORD_SYMBOLS) <= set(keyframe.IMG_SYMBOLS)
