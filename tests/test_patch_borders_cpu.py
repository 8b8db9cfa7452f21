"""The oracle's PatchFinder and MiniPatch at the image borders, with clipped windows and with equal scores, against numpy.

tests/patch_border_cases.py builds the cases and asserts (on the oracle alone, while it builds) that each seam is reached; here every
point of every launch of sets A, B and C goes through the numpy restatements of the template, the coarse search -- corner list and
exhaustive -- and the sub-pixel step, with the tolerances tests/test_oracle_cpu.py holds the interior to.  Two rules of the
restatements were taken from the reference, not from the oracle: a template is bad as soon as CVD::transform reports one pixel outside
the source image (src/PatchFinder.cc:162-170; the pixel test 0 <= p < size - 1 is libCVD's), and IterateSubPix gives up unless the
ROUNDED level position lies inside a border of mnPatchSize / 2 + 1 = 5 (:421), which ends IterateSubPixToConvergence with false (:404)."""
import numpy as np
import pytest

import patch_border_cases as pbc


@pytest.fixture(scope="module", params=pbc.SIZES, ids=lambda s: "%dx%d" % s)
def cases(request):
    return pbc.oracle_cases(request.param)


def test_seams_are_reached_on_the_oracle(cases):
    """Building the cases asserts the seams (build_a, build_b, check_d_seams, check_e_seams); what is left is the size of the sets."""
    assert len(cases["A"]) == 9 and len(cases["B"]) == 4 and len(cases["E"]) == 9
    assert all(200 <= len(la["points"]) <= 900 for la in cases["A"])
    for la in cases["B"]:
        assert len(la["points"]) > 0, la["name"]
    kinds = [sum(1 for p in cases["A"][0]["points"] if p["tag"][0] == "fast" and p["tag"][2] == L) for L in range(4)]
    assert min(kinds[:3]) >= 2, kinds                            # border corners for the corner-mode search


@pytest.mark.parametrize("k", range(9))
def test_set_a_against_numpy(cases, k):
    la = cases["A"][k]
    info = pbc.check_search_against_numpy(la["ref"], la["points"], cases["F"].o[la["target"]], la["rng"], la["its"], la["exh"])
    pbc.assert_templates_rarely_differ([info])
    o = la["ref"]
    left = [r["conv"] == -1 for r in info]
    if la["exh"]:
        assert sum(left) >= 8                                    # lw - 5 and lh - 5 of every level: the sub-pixel step left the image
    if not la["exh"] and la["name"] != "A mixed":
        fast = np.array([p["tag"][0] == "fast" for p in la["points"]])
        assert (o["found"][fast] == 1).sum() >= 5 or la["its"] > 0, la["name"]


def test_set_b_against_numpy(cases):
    infos = []
    for la in cases["B"]:
        info = pbc.check_search_against_numpy(la["ref"], la["points"], cases["F"].o[la["target"]], la["rng"], la["its"], la["exh"])
        infos.append(info)
        if la["exh"]:
            at4 = [i for i, p in enumerate(la["points"]) if p["tag"][1] == 4]
            assert sum(1 for i in at4 if info[i]["conv"] == -1) >= 6, la["name"]       # a valid score at 4, refused by the sub-pixel step's 5
    pbc.assert_templates_rarely_differ(infos)


def test_set_c_ties_against_numpy():
    c = pbc.oracle_cases((320, 240))
    exh, fast = c["C"]
    # exhaustive: the period (8, 4, 2, 1 pixels) fits the window of every level several times
    hits = pbc.check_ties(c["F"], exh, (2, 2, 2, 2))
    o = exh["ref"]
    for i, p in enumerate(exh["points"]):                        # the first in raster order lies one or more periods above the centre
        L, per = p["tag"][2], max(8 >> p["tag"][2], 1)
        if o[i]["score"] < pbc.MAXSSD:
            assert o[i]["coarse_y"] < p["center"][1] and (p["center"][1] - o[i]["coarse_y"]) % per == 0, (i, L)
    # corner list: the kept corners repeat with the period too (levels 0 and 1; the flat levels above have no corners)
    hits_f = pbc.check_ties(c["F"], fast, (2, 2, 0, 0))
    print("ties: exhaustive %s corner list %s" % (hits, hits_f))


def test_stateful_callers_reduce_to_the_search_at_the_borders(cases):
    """Set D on the oracle: fresh finders in tracker mode give the stateless search's records at every border point."""
    for chain, res in zip(cases["D"], cases["D_ref"]):
        if chain[0]["name"] != "D track one":
            continue
        ref = {la["name"]: la for la in cases["A"]}["A r10 i8 fast"]["ref"]
        out, st = res[0]
        for f in ref.dtype.names:
            assert np.array_equal(ref[f], out[f]), f
        assert st["valid"].sum() == (ref["search_level"] >= 0).sum()
        return
    raise AssertionError("no tracker chain")


def test_minipatch_against_numpy(cases):
    from oracle import oracle_minipatch_find
    F = cases["F"]
    for ca in cases["E"]:
        pos, found, ssd = oracle_minipatch_find(F.o["A"], F.o["A"], ca["level"], ca["src_pos"], ca["dst_pos"], ca["rng"])
        npos, nfound, nssd = ca["numpy"]
        assert np.array_equal(found, nfound) and np.array_equal(pos, npos) and np.array_equal(ssd, nssd), (ca["level"], ca["rng"])
