"""The keyframe image front end (csrc/img_kernels.h) at its tile, row and block seams, bit-exact against the CPU oracle on the inputs of
tests/img_seam_cases.py (checked on the CPU, against plain numpy references, by tests/test_img_seams_cpu.py):

  1. k_pyr_fast's segment test and score on designed stamps: arcs of 9, 10, 11 and 16 ring pixels at each of the 16 starts, both
     polarities, contrast at and one above the threshold, centres on both sides of the 64 / 32 / 16 / 8 pixel tile edges of levels
     0 .. 3, the score cap of 254 and the last histogram bin;
  2. the pyramid and detection at sizes whose last tile column or row has 1 or 7 pixels (none at level 3), noise and low-contrast
     frames, both half-sampling variants, adaptive and fixed thresholds, masks, and the three ways a frame reaches the device;
  3. the row tables on both routes (k_row_tables, and k_row_count + k_row_compact in a child process with MCP_IMG_ROW_TABLES=0): heights
     around the look-back trips, widths around the ballot chunks, sparse frames, a batch of cameras of different heights, handle reuse;
  4. k_candidates at n_corners of 1, 255, 256, 257, 512, 513, non-maximum pairs across the 256-corner block seam, the border-10 line;
  5. k_minipatch's LUT range clamps, windows over the image edges, several corners per lane, exact SSD ties;
  6. k_dilate5 / k_glare_mask at the image borders, through their effect on the corner list.

No tolerance but the project's rtol = 1e-12 on Shi-Tomasi scores."""
import os
import subprocess
import sys

import numpy as np
import pytest

import img_seam_cases as ic

pytestmark = pytest.mark.gpu


def _pair(w, h, **kw):
    from mcptam_amd.keyframe import KeyFrame
    from oracle import OracleKeyFrame
    return KeyFrame(w, h, **kw), OracleKeyFrame(w, h, **kw)


def _assert_lite_equal(g, o, what=""):
    for l in range(4):
        assert g.LevelSize(l) == o.LevelSize(l)
        assert np.array_equal(g.Image(l), o.Image(l)), "%s: pyramid level %d differs" % (what, l)
        assert g.FastThresh(l) == o.FastThresh(l), "%s: threshold of level %d" % (what, l)
        assert np.array_equal(g.FastFrequency(l), o.FastFrequency(l)), "%s: histogram of level %d" % (what, l)
        cg, co = g.Corners(l), o.Corners(l)
        assert cg.shape == co.shape and np.array_equal(cg, co), "%s: corner list/order differs at level %d" % (what, l)
        assert np.array_equal(g.RowLUT(l), o.RowLUT(l)), "%s: row LUT of level %d" % (what, l)


def _both(img, masks=None, **kw):
    g, o = _pair(img.shape[1], img.shape[0], **kw)
    g.MakeKeyFrame_Lite(img, masks)
    o.MakeKeyFrame_Lite(img, masks)
    return g, o


def _has(corners, p):
    return bool(((corners[:, 0] == p[0]) & (corners[:, 1] == p[1])).any())


def _assert_candidates_equal(g, o, use_shi, what=""):
    for l in range(4):
        pg, sg = g.Candidates(l)
        po, so = o.Candidates(l)
        assert np.array_equal(pg, po), "%s: candidate set/order differs at level %d" % (what, l)
        if use_shi:
            assert np.allclose(sg, so, rtol=1e-12, atol=0), what
        else:
            assert np.array_equal(sg, so), what


# ------------------------------------------------------------------------------------------------ 1. stamps
def test_level0_stamps_at_every_start_and_tile_edge(gpu_required):
    for frame, centres, expect in ic.level0_frames():
        g, o = _both(frame, adaptive=False)
        _assert_lite_equal(g, o)
        c0 = g.Corners(0)
        assert np.array_equal(np.array([_has(c0, p) for p in centres]), expect)


@pytest.mark.parametrize("l", [1, 2, 3])
def test_level_stamps_through_the_lds_pyramid(gpu_required, l):
    for frame, sheet, centres, expect in ic.level_frames(l):
        for pavgb in (False, True):
            g, o = _both(frame, adaptive=False, pavgb=pavgb)
            _assert_lite_equal(g, o)
            assert np.array_equal(g.Image(l), sheet)
            cl = g.Corners(l)
            assert np.array_equal(np.array([_has(cl, p) for p in centres]), expect)


def test_score_stamps_and_the_cap(gpu_required):
    frame, centres, expect = ic.score_frame()
    g, o = _both(frame)
    _assert_lite_equal(g, o)                                     # FastFrequency included: the histogram bin is capped at 30
    assert g.FastThresh(0) == ic.MIN_T
    g.MakeKeyFrame_Rest(False, False, 0.8, 0.0, 0)
    o.MakeKeyFrame_Rest(False, False, 0.8, 0.0, 0)
    _assert_candidates_equal(g, o, False)
    pos, sc = g.Candidates(0)
    for p, e in zip(centres, expect):
        k = np.nonzero((pos[:, 0] == p[0]) & (pos[:, 1] == p[1]))[0]
        assert len(k) == 1 and sc[k[0]] == e


# ------------------------------------------------------------------------------------------------ 2. tile-size seams
@pytest.mark.parametrize("w,h", ic.SEAM_SIZES)
def test_pyramid_and_detection_at_tile_size_seams(gpu_required, w, h):
    masks = ic.level_masks(w, h, w + h)
    for name, img in ic.seam_images(w, h).items():
        for pavgb in (False, True):
            for adaptive in (True, False):
                g, o = _pair(w, h, adaptive=adaptive, pavgb=pavgb)
                for m in (None, masks, None):                     # the third frame: the masks of the second are gone again
                    g.MakeKeyFrame_Lite(img, m)
                    o.MakeKeyFrame_Lite(img, m)
                    _assert_lite_equal(g, o, "%s pavgb=%d adaptive=%d masks=%d" % (name, pavgb, adaptive, m is not None))
    g, o = _both(ic.seam_images(w, h)["noise"])
    for (use_shi, use_percent, nm) in ic.REST_PARAMS:
        g.MakeKeyFrame_Rest(use_shi, use_percent, 0.8, 70.0, nm)
        o.MakeKeyFrame_Rest(use_shi, use_percent, 0.8, 70.0, nm)
        _assert_candidates_equal(g, o, use_shi)


@pytest.mark.parametrize("w,h", ic.SEAM_SIZES)
def test_three_load_paths_give_the_same_frame(gpu_required, w, h):
    """The host array, a row-strided host view, and a device-resident frame -- base address odd and stride w + 3 (the byte-wise branch of
    the level-0 load), and base and stride multiples of 4 (the word branch)."""
    from mcptam_amd import hip_rt
    from mcptam_amd.keyframe import KeyFrame, make_lite_batch
    from oracle import OracleKeyFrame
    img = ic.seam_images(w, h)["octaves"]
    o = OracleKeyFrame(w, h)
    o.MakeKeyFrame_Lite(img)
    g = KeyFrame(w, h)
    g.MakeKeyFrame_Lite(img)
    _assert_lite_equal(g, o, "host array")
    view = ic.strided(img, 3)
    assert view.strides == (w + 3, 1)
    g = KeyFrame(w, h)
    g.MakeKeyFrame_Lite(view)
    _assert_lite_equal(g, o, "strided host view")
    g = KeyFrame(w, h)
    make_lite_batch([g], [view])
    _assert_lite_equal(g, o, "strided host view, batch entry")
    for offset, stride in ((1, w + 3), (0, (w + 7) & ~3)):
        buf = np.full(offset + stride * h, 255, dtype=np.uint8)
        buf[offset:].reshape(h, stride)[:, :w] = img
        p = hip_rt.dev_alloc(buf.nbytes)
        try:
            assert p % 4 == 0
            hip_rt.dev_upload(p, buf)
            g = KeyFrame(w, h)
            make_lite_batch([g], [p + offset], on_device=True, strides=[stride])
            _assert_lite_equal(g, o, "device frame at offset %d, stride %d" % (offset, stride))
            del g
        finally:
            hip_rt.dev_free(p)


# ------------------------------------------------------------------------------------------------ 3. row tables
@pytest.fixture(scope="module")
def row_tables(gpu_required):
    """(device tables on the default route, oracle tables) of every section-3 case, computed once"""
    from mcptam_amd.keyframe import KeyFrame, make_lite_batch
    from oracle import OracleKeyFrame
    return ic.run_row_cases(KeyFrame, make_lite_batch), ic.run_row_cases(OracleKeyFrame)


def _assert_tables_equal(a, b, what):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), "%s: %s" % (what, k)


def _assert_lut_is_searchsorted(t):
    for k in t:
        if "/lut" in k:
            c = t[k.replace("/lut", "/corners")]
            lut = t[k]
            last = int(c[-1, 1]) if len(c) else -1
            assert np.array_equal(lut[:last + 1], ic.row_lut(c, len(lut))[:last + 1]), k      # (rows past the last corner: the oracle's word)


def test_row_tables_one_launch_route(row_tables):
    dev, orc = row_tables
    assert len(dev) == 4 * 4 * (len(ic.ROW_SHAPES) + len(ic.SPARSE_NAMES) + 2 * len(ic.BATCH_SHAPES) + 3)
    _assert_tables_equal(dev, orc, "k_row_tables against the oracle")
    _assert_lut_is_searchsorted(dev)
    for k in ("corners0", "lut0", "thresh0", "hist0"):            # handle reuse: noise, black, the same noise again
        assert np.array_equal(dev["reuse2/" + k], dev["reuse0/" + k])
    assert len(dev["reuse1/corners0"]) == 0


def test_row_tables_two_kernel_route_in_a_child_process(row_tables, tmp_path):
    """MCP_IMG_ROW_TABLES is read once per process: one fresh child runs the same cases on k_row_count + k_row_compact."""
    dev, orc = row_tables
    out = str(tmp_path / "route0.npz")
    env = dict(os.environ, MCP_IMG_ROW_TABLES="0")
    r = subprocess.run([sys.executable, os.path.abspath(ic.__file__), out], env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-2000:]
    z = np.load(out)
    assert str(z["knob"]) == "0"
    child = {k: z[k] for k in z.files if k != "knob"}
    _assert_tables_equal(child, orc, "k_row_count + k_row_compact against the oracle")
    _assert_tables_equal(child, dev, "the two routes against each other")
    _assert_lut_is_searchsorted(child)


# ------------------------------------------------------------------------------------------------ 4. candidates
@pytest.fixture(scope="module")
def cand():
    return ic.candidate_cases()


@pytest.mark.parametrize("name", ic.CAND_NAMES)
def test_candidates_at_the_block_seams(gpu_required, cand, name):
    img, sub, _ssc = cand[name]
    h, w = img.shape
    g, o = _both(img, ic.subset_masks(w, h, sub))
    _assert_lite_equal(g, o)
    assert np.array_equal(g.Corners(0), sub)
    if name.startswith("count_"):
        assert len(g.Corners(0)) == int(name[6:])
    for (use_shi, use_percent, nm) in ic.REST_PARAMS:
        g.MakeKeyFrame_Rest(use_shi, use_percent, 0.8, 70.0, nm)
        o.MakeKeyFrame_Rest(use_shi, use_percent, 0.8, 70.0, nm)
        _assert_candidates_equal(g, o, use_shi, name)
    g.MakeKeyFrame_Rest(False, False, 0.8, 0.0, 0)               # every non-maximum survivor inside the border, in corner order
    o.MakeKeyFrame_Rest(False, False, 0.8, 0.0, 0)
    _assert_candidates_equal(g, o, False, name)
    pos = g.Candidates(0)[0]
    if name.startswith("pair"):
        got = (_has(pos, sub[255]), _has(pos, sub[256]))
        assert got == {"gt": (True, False), "lt": (False, True), "eq": (True, True)}[name[-2:]]
    if name.startswith("border_only"):
        assert len(pos) == 1 and tuple(pos[0]) == tuple(sub[-1])


def test_candidates_second_frame_on_the_same_handle(gpu_required, cand):
    """the score image is rebuilt for the second frame's corners: no neighbour left over from the first"""
    img, first, _s = cand["count_513"]
    second = cand["second_frame"][1]
    w, h = ic.CAND_SIZE
    g, o = _pair(w, h)
    for sub in (first, second):
        m = ic.subset_masks(w, h, sub)
        g.MakeKeyFrame_Lite(img, m)
        o.MakeKeyFrame_Lite(img, m)
        _assert_lite_equal(g, o)
        for (use_shi, use_percent, nm) in ic.REST_PARAMS:
            g.MakeKeyFrame_Rest(use_shi, use_percent, 0.8, 70.0, nm)
            o.MakeKeyFrame_Rest(use_shi, use_percent, 0.8, 70.0, nm)
            _assert_candidates_equal(g, o, use_shi)
    assert g.NumPrev() == o.NumPrev() == 1


# ------------------------------------------------------------------------------------------------ 5. MiniPatch
def test_minipatch_range_clamps_and_full_lanes(gpu_required):
    from mcptam_amd.keyframe import minipatch_find
    from oracle import oracle_minipatch_find
    src, dst = ic.minipatch_images()
    gs, os_ = _both(src)
    gd, od = _both(dst)
    _assert_lite_equal(gd, od)
    nfound = 0
    for r, (sp, dp) in ic.minipatch_positions(od.Corners(0)).items():
        pg, fg, sg = minipatch_find(gs, gd, 0, sp, dp, r)
        po, fo, so = oracle_minipatch_find(os_, od, 0, sp, dp, r)
        assert np.array_equal(fg, fo) and np.array_equal(pg, po) and np.array_equal(sg, so), "range %d" % r
        nfound += int(fg.sum())
    assert nfound > 10


def test_minipatch_exact_ties_first_corner_wins(gpu_required):
    from mcptam_amd.keyframe import minipatch_find
    from oracle import OracleKeyFrame, oracle_minipatch_find
    img = ic.periodic_image()
    w, h = ic.MP_SIZE
    full = OracleKeyFrame(w, h)
    full.MakeKeyFrame_Lite(img)
    idx, _pts, sp, dp, r, win = ic.tie_case(full.Corners(0))
    g, o = _both(img, ic.subset_masks(w, h, full.Corners(0)[idx]))
    _assert_lite_equal(g, o)
    pg, fg, sg = minipatch_find(g, g, 0, sp, dp, r)
    po, fo, so = oracle_minipatch_find(o, o, 0, sp, dp, r)
    assert np.array_equal(fg, fo) and np.array_equal(pg, po) and np.array_equal(sg, so)
    assert fg.all() and (sg == 0).all() and np.array_equal(pg, win)


# ------------------------------------------------------------------------------------------------ 6. glare
@pytest.mark.parametrize("w,h", ic.GLARE_SIZES)
def test_glare_mask_at_the_borders(gpu_required, w, h):
    caller = ic.glare_caller_masks(w, h)
    for name, f in ic.glare_frames(w, h).items():
        for cm in (None, caller):
            g, o = _both(f, cm, glare=True)
            _assert_lite_equal(g, o, name)
            for l in range(4):
                c = g.Corners(l)
                gl = ic.glare(g.Image(l))
                assert not gl[c[:, 1], c[:, 0]].any(), (name, l)
                if cm is not None:
                    assert (cm[l][c[:, 1], c[:, 0]] == 255).all()
        assert len(g.Corners(0)) > 0
