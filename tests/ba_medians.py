"""Hard chi2 populations for the six routes to the bundle adjuster's Huber median, and a model of the branch each must take
(test_ba_medians_cpu.py, test_ba_medians_gpu.py).

The mapper scales its robust kernel with element [size/2] of the sorted |chi2| (MEstimator.h:194-204).  The solver reaches
that element by six routes (csrc/ba_select.h, ba_trial.h, ba_small.h, ba_head.h, ba_headl.h), each with a fixed-size candidate
table and a fallback behind it, three of them starting from a guess.  `populations(n, route)` builds, in pure numpy from a fixed
seed, the arrays that drive a route through every one of those branches; `model(route, x, rank, prev_median)` says -- from the
array alone, in plain integer arithmetic on the bit patterns -- which branch that is.  The reference for the selected value is
always `np.sort(np.abs(x))[rank]`, compared bit for bit.

A population common to all routes depends on (n, name) only, so that the routes can be compared with each other on it.
"""
import math
import zlib
from collections import namedtuple

import numpy as np

# the tables of the kernels (csrc/*.h); the multi-rank slot table is what the GPU test sets MCP_BA_SELECT_CAP to
SEL_GATHER_CAP = 65536
SELECT_CAP = 64
HS_RANK = 64
HS_CAND = 2048
HS_STASH_WAVE = 14336 // 16          # 896 stashed values per wavefront
HEAD_CAND = 4096
HEAD_WIN = 32
HL_CAP = 16384
SMALL_MEAS = 32768
MIN_SIGMA_SQ = 0.25                  # ChainBundle.sdMinMEstimatorSigma ** 2

ROUTES = ("plain", "ranks", "ride", "small", "ahead", "large")
SMALL_COUNTS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 32767, 32768)
LARGE_COUNTS = (32769, 70001)
CAPS = {"plain": (SEL_GATHER_CAP,), "ranks": (SELECT_CAP,), "ride": (SELECT_CAP,), "small": (HS_RANK, HS_CAND),
        "ahead": (HEAD_CAND,), "large": (HL_CAP,)}

# every branch a route has; test_ba_medians_cpu.py demands that the populations reach each of them
BRANCHES = {
    "plain": {"held", "overflow"},
    "ranks": {"held", "overflow"},
    "ride": {"hit0", "hit-1", "hit+1", "miss", "no_prediction", "hit_overflow", "miss_overflow"},
    "small": {"guess_hit", "guess_miss", "guess_from_element", "stash_complete", "stash_overflow", "rank_path", "lds_path", "array_path",
              "guess_hit+array_path", "guess_miss+array_path", "guess_miss+lds_path", "stash_overflow+rank_path"},
    "ahead": {"accept0", "accept-1", "accept+1", "decline-2", "decline+2", "decline_below_window", "decline_above_window", "decline_overflow"},
    "large": {"held", "overflow"},
}

Pop = namedtuple("Pop", "name x prev_median claim")      # claim: branches the name promises, {route or "*": set of branch names}


def keys(x):
    """bit patterns of |x|: monotone in the value for non-negative doubles"""
    return np.abs(np.asarray(x, dtype=np.float64)).view(np.uint64)


def key_of(v):
    return int(np.abs(np.float64(v)).view(np.uint64))


def coarse_bin(v):
    """sign + ten exponent bits: a bin spans a factor of four, [0.5, 2), [2, 8), ..."""
    return key_of(v) >> 53


def reference(x, rank):
    return np.sort(np.abs(np.asarray(x, dtype=np.float64)))[rank]


def same_bits(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# the model: which branch the kernels must take

def model(route, x, rank, prev_median, cap=None):
    """dict(branches=set of names from BRANCHES[route], + what the host learns from the route)"""
    k = keys(x)
    n = len(k)
    med = int(np.sort(k)[rank])
    c22 = int(np.count_nonzero((k >> np.uint64(42)) == np.uint64(med >> 42)))        # values sharing the median's first two digits
    out = dict(cand=c22)
    if route in ("plain", "large", "ranks"):
        cap = cap or CAPS[route][0]
        out["overflow"] = c22 > cap
        out["branches"] = {"overflow" if c22 > cap else "held"}
        return out
    if route == "ride":
        cap = cap or SELECT_CAP
        pred = coarse_bin(prev_median) if prev_median >= 0 else -1
        d = (med >> 53) - pred
        hit = pred >= 0 and -1 <= d <= 1
        ovf = c22 > cap
        out.update(pred_ok=hit, overflow=hit and ovf, fast=hit and not ovf, select_overflow=ovf)
        if pred < 0:
            b = {"no_prediction"}
        elif hit:
            b = {"hit%+d" % d if d else "hit0"}
        else:
            b = {"miss"}
        if ovf:
            b.add("hit_overflow" if hit else "miss_overflow")
        out["branches"] = b
        return out
    if route == "small":
        from_elem = not (prev_median > 0)                          # a zero (or no) last median: the guess is chi2[n/2]
        guess = abs(float(x[n // 2])) if from_elem else prev_median
        pred = coarse_bin(guess)
        c = (k >> np.uint64(53)).astype(np.int64)
        below, equal = int(np.count_nonzero(c < pred)), int(np.count_nonzero(c == pred))
        hit = below <= rank < below + equal
        wave = (np.arange(n) // 64) % 16                           # element 64 (w + 16 j) + lane belongs to wavefront w
        per_wave = np.bincount(wave[c == pred], minlength=16)
        spilled = bool(per_wave.max() > HS_STASH_WAVE)
        b = {"guess_hit" if hit else "guess_miss"}
        if from_elem:
            b.add("guess_from_element")
        if hit:
            b.add("stash_overflow" if spilled else "stash_complete")
        path = "rank_path" if c22 <= HS_RANK else ("lds_path" if c22 <= HS_CAND else "array_path")
        b.add(path)
        b.add(("guess_hit+" if hit else "guess_miss+") + path)
        if hit and spilled:
            b.add("stash_overflow+" + path)
        out.update(guess_hit=hit, stash_overflow=hit and spilled, branches=b, wave_max=int(per_wave.max()))
        return out
    if route == "ahead":
        pred = coarse_bin(prev_median) if prev_median >= 0 else 0
        d = (med >> 53) - pred
        in1 = int(np.count_nonzero((k >> np.uint64(46)) == np.uint64(med >> 46)))     # 11 + 7 bits
        out["cand"] = in1
        if d < -HEAD_WIN // 2:
            b, status = "decline_below_window", 2
        elif d >= HEAD_WIN // 2:
            b, status = "decline_above_window", 2
        elif abs(d) >= 2:
            b, status = ("decline%+d" % d if abs(d) == 2 else "decline_far"), 2
        elif in1 > HEAD_CAND:
            b, status = "decline_overflow", 2
        else:
            b, status = ("accept%+d" % d if d else "accept0"), 1
        out.update(status=status, branches={b})
        return out
    raise ValueError(route)


def sigma_block(med, n):
    """k_select_small's expression in float64: [raw sigma^2, limited, its root, median]; the denominator 2n - 6 in 64-bit unsigned
    arithmetic as the reference evaluates it (wraps for n = 1, 2; zero for n = 3)."""
    den = np.float64((2 * n - 6) % 2 ** 64)
    with np.errstate(all="ignore"):
        s = np.float64(1.4826) * (np.float64(1) + np.float64(5.0) / den) * np.sqrt(np.float64(med))
        s = np.float64(1.345) * s
        s2 = s * s
        lim = np.float64(MIN_SIGMA_SQ) if s2 < MIN_SIGMA_SQ else s2
        return np.array([s2, lim, np.sqrt(lim), med], dtype=np.float64)


def robust_chi2(x, sig):
    """activeRobustChi2 at the sigma block `sig`: the exactly rounded sum of the robustified values"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = np.where(x <= sig[1], np.abs(x), 2.0 * sig[2] * np.sqrt(np.where(x > 0, x, 0.0)) - sig[1])
        if np.isnan(sig[1]):
            return float("nan")
    if np.isnan(r).any():
        return float("nan")
    if np.isinf(r).any():
        return float("inf")
    return math.fsum(r.tolist())


# ---------------------------------------------------------------------------------------------------------------------
# populations

def _rng(n, name):
    return np.random.default_rng([20261019, n, zlib.crc32(name.encode())])


def _signed(rng, x, frac=0.1):
    """chi2 is signed (EdgeChainMeas::chi2): the kernels select |x|"""
    x = np.array(x, dtype=np.float64)
    neg = rng.random(len(x)) < frac
    x[neg] = -x[neg]
    return x


def _around(rng, n, rank, mid, lo=(1e-3, 0.4), hi=(4.0, 1000.0), place=None):
    """`mid` (values in [0.5, 2)) with element [rank] of the whole inside it: `below` values from lo under it, the rest from hi above;
    place: how many of mid lie under the rank (default half)"""
    m = len(mid)
    want = m // 2 if place is None else place
    below = min(max(rank - want, 0), n - m)
    assert below <= rank < below + m
    x = np.concatenate([rng.uniform(lo[0], lo[1], below), mid, rng.uniform(hi[0], hi[1], n - m - below)])
    return x


def _boundary(rng, n, rank, lo_val, hi_val, which):
    """lo_val and hi_val are neighbouring keys; which = "last": element [rank] is lo_val, "first": it is hi_val"""
    n_lo = min(rank + 1, n) if which == "last" else rank
    n_hi = n - n_lo
    ulp = np.spacing(lo_val)

    def fill(cnt, edge, sign):
        if cnt <= 0:
            return np.zeros(0)
        near = min(cnt // 4, 1500)                               # (few enough for every table but the 64-slot ones)
        v = np.concatenate([edge + sign * ulp * rng.integers(0, 1000, near), edge * (1.0 + sign * rng.uniform(0, 0.9 if sign > 0 else 0.45, cnt - near))])
        v[:min(3, cnt)] = edge                                  # the edge itself, up to three times
        return v
    return np.concatenate([fill(n_lo, lo_val, -1.0), fill(n_hi, hi_val, 1.0)])


def populations(n, route):
    """[Pop(name, x, prev_median, claim)] for a map of n measurements on `route` (the rank is n // 2)."""
    assert route in ROUTES and n >= 1
    rank = n // 2
    pops = []

    def add(name, x, prev, claim=None, shuffle=True):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (n,) and not np.isnan(x).any(), name
        if shuffle:
            x = x[_rng(n, name + "/perm").permutation(n)]
        pops.append(Pop(name, x, float(prev), claim or {}))

    # 1. baseline
    r = _rng(n, "lognormal")
    logn = _signed(r, r.lognormal(0.0, 2.0, n))
    add("lognormal", logn, reference(logn, rank))
    r = _rng(n, "binades60")
    b60 = 2.0 ** r.uniform(-30, 30, n)
    add("binades60", b60, reference(b60, rank))
    if n >= 2:
        s = np.sort(np.abs(logn))
        s[rank - 1] = s[rank]
        add("tie_across_rank", s, s[rank])
    add("all_equal", np.full(n, 1.2345), 1.2345)
    add("all_zero", np.where(np.arange(n) % 2 == 0, 0.0, -0.0), 0.0)

    # 2. zeros around the rank
    for z, tag in ((rank - 1, "rank-1"), (rank, "rank"), (rank + 1, "rank+1")):
        if not 0 <= z <= n:
            continue
        r = _rng(n, "zeros_" + tag)
        zs = np.where(np.arange(z) % 2 == 0, 0.0, -0.0)
        x = np.concatenate([zs, _signed(r, r.lognormal(0.0, 1.0, n - z), 0.3)])
        add("zeros_" + tag, x, 0.0 if z % 2 else 1.0, {"*": {"median_zero"} if rank < z else {"median_positive"}})

    # 3. clusters sharing the median's top 22 bits, cap - 1, cap, cap + 1 strong, distinct or equal in all 64 bits
    for cap in CAPS[route]:
        for m in (cap - 1, cap, cap + 1):
            if m > n:
                continue
            for kind in ("distinct", "equal"):
                name = "cluster_%s_%d" % (kind, m)
                r = _rng(n, name)
                mid = 1.0 + np.arange(m) * 2.0 ** -52 if kind == "distinct" else np.full(m, 1.0 + 2.0 ** -30)
                x = _around(r, n, rank, mid)
                claim = {"plain": {"overflow" if m > cap else "held"}, "large": {"overflow" if m > cap else "held"},
                         "ranks": {"overflow" if m > cap else "held"}, "ride": {"hit0"} | ({"hit_overflow"} if m > cap else set()),
                         "ahead": {"decline_overflow" if m > cap else "accept0"},
                         "small": {"guess_hit", "stash_complete", "rank_path" if m <= HS_RANK else ("lds_path" if m <= HS_CAND else "array_path")}}
                add(name, x, 1.0, {route: claim[route]})
                if route == "small" and cap == HS_CAND:      # the same with a guess far off: the candidates come from the sweep over the array
                    add(name + "_guess_off", x, 1e300, {"small": {"guess_miss", "lds_path" if m <= HS_CAND else "array_path"}})
                if route == "ride":                           # ... and with the prediction missed: the three-collective selection meets the table
                    add(name + "_pred_off", x, 1e-300, {"ride": {"miss"} | ({"miss_overflow"} if m > cap else set())})

    # 4. small: 896 / 897 guess-bin values inside ONE wavefront's elements, few elsewhere
    if route == "small":
        for w in (0, 15):
            own = np.flatnonzero((np.arange(n) // 64) % 16 == w)
            other = np.flatnonzero((np.arange(n) // 64) % 16 != w)
            for cnt in (HS_STASH_WAVE, HS_STASH_WAVE + 1):
                if len(own) < cnt or len(other) < 5 or n < cnt + 5 + 2:
                    continue
                name = "stash_wave%d_%d" % (w, cnt)
                r = _rng(n, name)
                hot = np.concatenate([r.choice(own, cnt, replace=False), r.choice(other, 5, replace=False)])
                m = len(hot)
                below = min(max(rank - m // 2, 0), n - m)
                rest = np.concatenate([r.uniform(1e-3, 0.4, below), r.uniform(4.0, 1000.0, n - m - below)])
                x = np.zeros(n)
                x[hot] = r.uniform(0.5, 1.999, m)
                mask = np.ones(n, dtype=bool)
                mask[hot] = False
                x[mask] = r.permutation(rest)
                add(name, x, 1.0, {"small": {"guess_hit", "stash_overflow" if cnt > HS_STASH_WAVE else "stash_complete", "rank_path"}}, shuffle=False)

    # 5. the median on a boundary: of a coarse bin, of the 18-bit and 22-bit prefixes, of the last 9-bit digit
    for tag, hi_val in (("coarse", 2.0), ("prefix18", 1.0 + 2.0 ** -6), ("prefix22", 1.0 + 2.0 ** -10), ("digit9", 1.0 + 512 * 2.0 ** -52)):
        lo_val = float(np.nextafter(hi_val, 0.0))
        for which in ("last", "first"):
            name = "boundary_%s_%s" % (tag, which)
            x = _boundary(_rng(n, name), n, rank, lo_val, hi_val, which)
            # the prediction sits on the OTHER side of the boundary
            d = 0 if tag != "coarse" else (-1 if which == "last" else 1)
            add(name, x, hi_val if which == "last" else lo_val,
                {"*": {"median=" + repr(lo_val if which == "last" else hi_val)}, "ride": {"hit%+d" % d if d else "hit0"},
                 "ahead": {"accept%+d" % d if d else "accept0"}, "small": {"guess_miss" if d else "guess_hit"}})

    # 6. extremes
    r = _rng(n, "denormals")
    add("denormals", r.integers(1, 2 ** 52, n).astype(np.uint64).view(np.float64), 0.0, {"*": {"median_denormal"}})
    if n >= 4:
        r = _rng(n, "huge_top")
        x = np.sort(r.lognormal(0.0, 2.0, n))
        x[-1], x[-2] = np.inf, np.finfo(np.float64).max
        add("huge_top", x, reference(x, rank), {"*": {"holds_inf"}})
    r = _rng(n, "median_denormal")
    nd = min(rank + 1, n)
    x = np.concatenate([r.integers(0, 2 ** 52, nd).astype(np.uint64).view(np.float64), r.lognormal(0.0, 2.0, n - nd)])
    add("median_denormal", x, 1.0, {"*": {"median_denormal_or_zero"}})

    # 7. the prediction near and far: the median lies in [0.5, 2)
    r = _rng(n, "spread")
    x = np.abs(r.lognormal(0.0, 1.5, n))
    x = x * (1.2 / reference(x, rank))
    x[np.argsort(x)[rank]] = 1.2                      # (exactly, whatever the scaling rounded to)
    x = _signed(r, x)
    for tag, prev, ride, ahead in (("same_bin", 1.0, "hit0", "accept0"), ("one_below", 0.3, "hit+1", "accept+1"), ("one_above", 3.0, "hit-1", "accept-1"),
                                   ("two_below", 0.1, "miss", "decline+2"), ("two_above", 10.0, "miss", "decline-2"),
                                   ("far_above", 1e300, "miss", "decline_below_window"), ("far_below", 1e-300, "miss", "decline_above_window"),
                                   ("none", -1.0, "no_prediction", None)):
        add("prev_" + tag, x, prev, {"ride": {ride}, "small": {"guess_hit" if tag in ("same_bin",) else ("guess_from_element" if tag == "none" else "guess_miss")},
                                    **({"ahead": {ahead}} if ahead else {})})
    # a zero last median: k_head_small takes chi2[n/2] as its guess -- once in the median's bin, once not
    xs = x[_rng(n, "prev_zero/perm").permutation(n)]
    inside = np.flatnonzero((keys(xs) >> np.uint64(53)) == np.uint64(coarse_bin(1.2)))
    outside = np.flatnonzero((keys(xs) >> np.uint64(53)) != np.uint64(coarse_bin(1.2)))
    for tag, idx, claim in (("right", inside, "guess_hit"), ("wrong", outside, "guess_miss")):
        if len(idx) == 0:
            continue
        y = xs.copy()
        j = int(idx[0])
        y[n // 2], y[j] = y[j], y[n // 2]
        add("prev_zero_guess_" + tag, y, 0.0, {"small": {claim, "guess_from_element"}}, shuffle=False)
    return pops


def check_claim(pop, route, n):
    """the branches `pop` promises for `route`, checked against the model and the reference; returns the model's dict"""
    rank = n // 2
    md = model(route, pop.x, rank, pop.prev_median)
    ref = reference(pop.x, rank)
    for who in (route, "*"):
        for c in pop.claim.get(who, ()):
            if c == "median_zero":
                assert ref == 0.0, (pop.name, n, ref)
            elif c == "median_positive":
                assert ref > 0.0, (pop.name, n, ref)
            elif c == "median_denormal":
                assert 0.0 < ref < np.finfo(np.float64).tiny, (pop.name, n, ref)
            elif c == "median_denormal_or_zero":
                assert 0.0 <= ref < np.finfo(np.float64).tiny, (pop.name, n, ref)
            elif c == "holds_inf":
                assert np.isinf(pop.x).any() and np.isfinite(ref), (pop.name, n)
            elif c.startswith("median="):
                assert same_bits(ref, float(c[7:])), (pop.name, n, ref, c)
            else:
                assert c in md["branches"], (pop.name, route, n, c, sorted(md["branches"]))
    return md
