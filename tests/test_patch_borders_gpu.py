"""patch_item (csrc/img_kernels.h) and k_minipatch at the image borders, with clipped windows and with equal scores: the HIP path
(track_search, track_search_batch, patch_sequences, minipatch_find) against the oracle on every point of every launch that
tests/patch_border_cases.py builds -- sets A (same frame), B (target shifted by 8 pixels), C (periodic frame: the first-best tie-break
across lanes), D (the stateful callers) and E (MiniPatch).  tests/test_patch_borders_cpu.py pins the oracle at the same cases against
numpy.  The comparisons are those of tests/test_img_gpu.py, through its own functions: templates and integer fields bit for bit,
found_pos to 1e-9, the projection and its derivatives to rtol 1e-11 / atol 1e-12, the finders' states with _assert_states_equal."""
import numpy as np
import pytest

import patch_border_cases as pbc
from test_img_gpu import _assert_states_equal, assert_track_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=pbc.SIZES, ids=lambda s: "%dx%d" % s)
def cases(request, gpu_required):
    from mcptam_amd.keyframe import KeyFrame
    return pbc.build_cases(request.param, make_gpu=lambda w, h, **kw: KeyFrame(w, h, **kw))


def _same_nans(a, b, what):
    """A template without gradient (a flat patch) has no sub-pixel normal matrix to invert: both sides carry NaN from there on.  The NaNs
    must sit in the same places; everything else goes through the project's comparisons unchanged."""
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), what
    if not na.any():
        return a, b
    a, b = a.copy(), b.copy()
    a[na] = 0.0; b[nb] = 0.0
    return a, b


def assert_outputs_equal(og, oo):
    oo = oo.copy()
    og = og.copy()
    og["found_pos"], oo["found_pos"] = _same_nans(og["found_pos"], oo["found_pos"], "found_pos")
    assert_track_equal(og, oo)
    assert np.array_equal(og["sqrt_inv_noise"], oo["sqrt_inv_noise"])
    assert np.allclose(og["found_pos"], oo["found_pos"], rtol=0, atol=1e-9)
    for f in ("image", "cam_derivs", "jacobian", "warp_inverse"):
        assert np.allclose(og[f], oo[f], rtol=1e-11, atol=1e-12), f


def assert_states_equal(sg, so):
    sg, so = sg.copy(), so.copy()
    sg["mean_diff"], so["mean_diff"] = _same_nans(sg["mean_diff"], so["mean_diff"], "mean_diff")
    _assert_states_equal(sg, so)


@pytest.mark.parametrize("k", range(9))
def test_set_a_same_frame(cases, k):
    from mcptam_amd.keyframe import track_search
    la = cases["A"][k]
    og = track_search(cases["F"].g[la["target"]], cases["cam"], la["pose"], pbc.IDENT, la["points"], la["rng"], la["its"], la["exh"])
    assert_outputs_equal(og, la["ref"])


def test_set_b_shifted_target_and_set_c_ties(cases):
    from mcptam_amd.keyframe import track_search
    assert len(cases["B"]) == 4 and len(cases["C"]) == (2 if cases["size"] == (320, 240) else 0)
    for la in cases["B"] + cases["C"]:
        og = track_search(cases["F"].g[la["target"]], cases["cam"], la["pose"], pbc.IDENT, la["points"], la["rng"], la["its"], la["exh"])
        assert_outputs_equal(og, la["ref"])


@pytest.mark.parametrize("rng,its,exh", [(10, 8, False), (30, 0, True)])
def test_batch_of_two_cameras(cases, rng, its, exh):
    """track_search_batch: the second camera looks from a CamFromBase that moves every projection about 16 pixels left and 12 up, so the
    first camera's border points are interior points of the second and the other way round; every third point is a fixed one."""
    from mcptam_amd.keyframe import track_search_batch
    from oracle import oracle_track_search
    F, cam = cases["F"], cases["cam"]
    pts = cases["A"][-3]["points"]                               # the mixed launch's points
    assert cases["A"][-3]["name"] == "A mixed"
    cfbs = [pbc.IDENT, pbc.shift_pose(cam, -16.0, -12.0)]
    outs = track_search_batch([F.g["A"], F.g["A"]], [cam, cam], pbc.IDENT, cfbs, [pts, pts[::-1]], rng, its, exh)
    refs = [oracle_track_search(F.o["A"], cam, pbc.IDENT, cfbs[0], pts, rng, its, exh),
            oracle_track_search(F.o["A"], cam, pbc.IDENT, cfbs[1], pts[::-1], rng, its, exh)]
    for og, oo in zip(outs, refs):
        assert_outputs_equal(og, oo)
    a, b = pbc.window_clipped(F.o["A"], refs[0], rng).any(axis=1), pbc.window_clipped(F.o["A"], refs[1], rng).any(axis=1)[::-1]
    s0, s1 = refs[0]["searched"] == 1, refs[1]["searched"][::-1] == 1
    assert (a & s1 & ~b).sum() >= 4 and (b & s0 & ~a).sum() >= 4 and (s0 & ~s1).sum() >= 4       # cut for one camera, whole or off the frame for the other


def test_set_d_stateful_callers(cases):
    """Every call of every chain, outputs and finder states.  The "D epi refine" chain starts a finder that holds an interior template at
    the border, where template and image have nothing to do with each other: at 322x250, level 3, one pixel is less than half as bright
    as its template pixel, IterateSubPix's `fPixel - mimTemplate[ir]` (a FLOAT subtraction, src/PatchFinder.cc:456) rounds, and a kernel
    that subtracts in double ends 8e-8 pixels away from the oracle (which this test found)."""
    from mcptam_amd import keyframe as kf
    F, cam = cases["F"], cases["cam"]
    assert len(cases["D"]) == 8
    for chain, ref in zip(cases["D"], cases["D_ref"]):
        sg = kf.new_pf_states(len(chain[0]["seqs"]))
        for ca, (oo, so) in zip(chain, ref):
            tg = [(F.g[n], cam, pose, cfb) for n, pose, cfb in ca["targets"]]
            og = kf.patch_sequences(ca["mode"], tg, ca["seqs"], sg, ca["rng"], ca["its"], ca["exh"])
            assert len(og) == len(oo) == sum(len(s_) for s_ in ca["seqs"]), ca["name"]
            assert_outputs_equal(og, oo)
            assert_states_equal(sg, so)


def test_set_e_minipatch(cases):
    from mcptam_amd.keyframe import minipatch_find
    from oracle import oracle_minipatch_find
    F = cases["F"]
    for ca in cases["E"]:
        pg, fg, sg = minipatch_find(F.g["A"], F.g["A"], ca["level"], ca["src_pos"], ca["dst_pos"], ca["rng"])
        po, fo, so = oracle_minipatch_find(F.o["A"], F.o["A"], ca["level"], ca["src_pos"], ca["dst_pos"], ca["rng"])
        assert np.array_equal(fg, fo) and np.array_equal(pg, po) and np.array_equal(sg, so), (ca["level"], ca["rng"])
        assert np.array_equal(fo, ca["numpy"][1]) and np.array_equal(po, ca["numpy"][0])
