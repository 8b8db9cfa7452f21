"""The chi2 populations of tests/ba_medians.py reach the branches their names claim -- checked on the model of the six routes to the
bundle adjuster's median, without a GPU.  A population that misses its branch is a failure of the generator, not a measurement."""
import numpy as np
import pytest

import ba_medians as bm


def _counts(route):
    return bm.SMALL_COUNTS if route == "small" else bm.LARGE_COUNTS


@pytest.mark.parametrize("route", bm.ROUTES)
def test_every_population_reaches_the_branch_its_name_claims(route):
    for n in _counts(route):
        pops = bm.populations(n, route)
        assert len({p.name for p in pops}) == len(pops)
        for p in pops:
            assert p.x.shape == (n,) and p.x.dtype == np.float64 and not np.isnan(p.x).any()
            md = bm.check_claim(p, route, n)
            assert md["branches"], (p.name, n)


@pytest.mark.parametrize("route", bm.ROUTES)
def test_the_list_as_a_whole_reaches_every_branch_of_every_route(route):
    seen = {}
    for n in _counts(route):
        for p in bm.populations(n, route):
            for b in bm.model(route, p.x, n // 2, p.prev_median)["branches"]:
                seen.setdefault(b, (n, p.name))
    missing = bm.BRANCHES[route] - set(seen)
    assert not missing, (route, sorted(missing))
    print(route, {b: seen[b] for b in sorted(bm.BRANCHES[route])})


def test_every_cap_is_met_from_both_sides():
    """cap - 1, cap, cap + 1 candidates for every table: the model's candidate count is exactly the cluster's size, so `cap` holds and
    `cap + 1` is the first to overflow"""
    for route, n in (("plain", 70001), ("ranks", 32769), ("ride", 32769), ("small", 32768), ("ahead", 32769), ("large", 32769)):
        pops = {p.name: p for p in bm.populations(n, route)}
        for cap in bm.CAPS[route]:
            for m in (cap - 1, cap, cap + 1):
                for kind in ("distinct", "equal"):
                    p = pops["cluster_%s_%d" % (kind, m)]
                    md = bm.model(route, p.x, n // 2, p.prev_median)
                    assert md["cand"] == m, (route, p.name, md["cand"])
                    ks = bm.keys(p.x)
                    top = np.count_nonzero((ks >> np.uint64(42)) == np.uint64(bm.key_of(bm.reference(p.x, n // 2)) >> 42))
                    assert top == m
                    if kind == "equal":
                        assert np.count_nonzero(ks == np.uint64(bm.key_of(bm.reference(p.x, n // 2)))) == m


def test_stash_populations_fill_one_wavefront():
    for n in (16383, 32768):
        pops = {p.name: p for p in bm.populations(n, "small")}
        for w in (0, 15):
            for cnt in (896, 897):
                p = pops["stash_wave%d_%d" % (w, cnt)]
                md = bm.model("small", p.x, n // 2, p.prev_median)
                assert md["wave_max"] == cnt and md["stash_overflow"] == (cnt == 897) and md["guess_hit"]
                c = (bm.keys(p.x) >> np.uint64(53)) == np.uint64(bm.coarse_bin(1.0))
                per = np.bincount(((np.arange(n) // 64) % 16)[c], minlength=16)
                assert per[w] == cnt and per.sum() == cnt + 5


def test_common_populations_do_not_depend_on_the_route():
    """the routes are compared with each other on these: same name, same bits"""
    a = {p.name: p for p in bm.populations(32769, "plain")}
    for route in ("ranks", "ride", "ahead", "large"):
        b = {p.name: p for p in bm.populations(32769, route)}
        common = [k for k in a if k in b and not k.startswith("cluster_")]
        assert len(common) >= 25
        for k in common:
            assert np.array_equal(a[k].x.view(np.uint64), b[k].x.view(np.uint64)) and a[k].prev_median == b[k].prev_median


def test_sigma_block_reference_shows_the_small_sample_cases():
    assert bm.sigma_block(2.0, 3)[0] == np.inf and np.isnan(bm.sigma_block(0.0, 3)[0])
    for n in (1, 2):
        s = bm.sigma_block(2.0, n)
        assert np.isfinite(s[0]) and s[0] == (1.345 * (1.4826 * np.sqrt(2.0))) ** 2          # the wrapped denominator: factor 1 + 5/1.8e19 = 1
    z = bm.sigma_block(0.0, 100)
    assert z[0] == 0.0 and z[1] == 0.25 and z[2] == 0.5 and z[3] == 0.0
    assert bm.robust_chi2([1.0, np.inf], bm.sigma_block(1.0, 100)) == np.inf
