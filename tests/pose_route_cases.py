"""The cases that pin every route of Tracker::TrackMap's pose iterations at its count and median seams: records, the squared-error keys
restated in numpy, the populations, and the route the library has to take for a call -- shared by tests/test_pose_routes_cpu.py (which
shows on the oracle alone that every case has the layout it is named for) and tests/test_pose_routes_gpu.py (which runs them).

Pure numpy + the CPU oracle's scene: nothing here needs a GPU.

The five routes (run-time switches): register-held k_pose_refine_regs (n <= 1024, <= 8 cameras), plain k_pose_refine,
multi-workgroup k_pose_refine_multi (histogram or gathered median), the sharded k_pr_project / k_pr_accum / k_pr_solve, and the single
update k_pose_errors / k_pose_solve."""
import functools

import numpy as np

# ---- constants of the routes, as INTEGRATION.md's switch table states them ---------------------------------------------------------------
REGS_MAX_N, REGS_MAX_CAMS = 1024, 8          # the register-held kernel: records, cameras
MULTI_MIN_N = 64                             # MCP_TRACK_REFINE_MULTI=2 forces the multi route from here
MULTI_MAX_WG, MULTI_MAX_ITER = 64, 16        # workgroups of one launch; iterations a multi launch has slots for
MULTI_CAND_CAP = 4096                        # keys sharing the median's prefix that are gathered instead of counted once more
GATHER_MAX_N = 16384                         # MCP_TRACK_REFINE_GATHER=1 up to here
PPW_DEFAULT = 512
SHIFTS = (53, 42, 31, 20, 9, 0)              # the digits of the radix select: 5 x 11 bits, then 9

K_MULTI, K_PPW, K_GATHER, K_GIVEUP = "MCP_TRACK_REFINE_MULTI", "MCP_TRACK_REFINE_PPW", "MCP_TRACK_REFINE_GATHER", "MCP_TRACK_TEST_PRM_GIVEUP"
KNOBS = (K_MULTI, K_PPW, K_GATHER, K_GIVEUP)


def route(n, ncam=2, n_iter=10, multi=1, ppw=PPW_DEFAULT, gather=0, giveup=False):
    """(route, workgroups, median gathered) of mcp_track_pose_refine for a call, from the documented switches."""
    regs = n <= REGS_MAX_N and ncam <= REGS_MAX_CAMS
    is_multi = n_iter <= MULTI_MAX_ITER and ((multi == 2 and n >= MULTI_MIN_N) or (multi == 1 and not regs and n > REGS_MAX_N))
    if is_multi:
        ppw = ppw if ppw > 0 else PPW_DEFAULT
        return ("multi_redone" if giveup else "multi", max(1, min(MULTI_MAX_WG, (n + ppw - 1)//ppw)), bool(gather) and n <= GATHER_MAX_N)
    return ("regs" if regs else "plain", 0, False)


def route_of_env(n, ncam, n_iter, env):
    return route(n, ncam, n_iter, int(env.get(K_MULTI, 1)), int(env.get(K_PPW, 0)), int(env.get(K_GATHER, 0)), K_GIVEUP in env)


def slices(n, nwg):
    """[i0, i1) of every workgroup of the multi route."""
    return [(n*w//nwg, n*(w + 1)//nwg) for w in range(nwg)]


# ---- records -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    import test_oracle_cpu as toc
    return toc._refine_scene()


def records(n, err, found=None, unfound=0.15, rng=None):
    """n records: the scene's found records tiled, unit noise, found position = projection + (err, 0); `found` (a 0/1 array) or a share
    `unfound` of them knocked out with `rng`."""
    cam, cfbs, bfw, recs0 = scene()
    base = recs0[recs0["found"] != 0]
    r = np.tile(base, n//len(base) + 1)[:n].copy()
    r["sqrt_inv_noise"] = 1.0
    r["found_pos"] = r["image"] + np.stack([np.asarray(err, dtype=np.float64), np.zeros(n)], axis=1)
    if found is not None:
        r["found"] = found
    elif unfound > 0:
        r["found"][rng.random(n) < unfound] = 0
    return r


def spread_cameras(r, ncam):
    """The same records for a rig of `ncam` cameras = the scene's two repeated: camera c becomes c, c + 2, c + 4 ... in turn."""
    cam, cfbs, bfw, _ = scene()
    r = r.copy()
    per = [np.arange(c, ncam, 2) for c in (0, 1)]
    idx = np.arange(len(r))
    for c in (0, 1):
        m = r["cam"] == c
        r["cam"][m] = per[c][idx[m] % len(per[c])]
    return r, [cam]*ncam, [cfbs[c % 2] for c in range(ncam)]


# ---- the keys of iteration 0 ---------------------------------------------------------------------------------------------------------------
def keys(r):
    """The squared errors of the found records as the kernels form them at iteration 0 (a first, re-projecting iteration keeps the
    records' image positions), as their 64-bit patterns -- the radix select's keys."""
    f = r["found"] != 0
    s = r["sqrt_inv_noise"][f]
    e0 = s*(r["found_pos"][f, 0] - r["image"][f, 0])
    e1 = s*(r["found_pos"][f, 1] - r["image"][f, 1])
    with np.errstate(over="ignore"):           # (a square may overflow to infinity: a key like any other)
        e2 = e0*e0 + e1*e1
    return np.abs(e2).view(np.uint64)


def median_key(k):
    return np.sort(k)[len(k)//2]


def prefix_counts(k):
    """Per digit of the select: how many keys share the median's bits from that digit's shift up."""
    med = median_key(k)
    return [int(np.count_nonzero((k >> np.uint64(s)) == (med >> np.uint64(s)))) for s in SHIFTS]


def exit_pass(k):
    """The digit after which k_pose_refine_multi's histogram median gathers its candidates (at most MULTI_CAND_CAP keys share the
    prefix); None: it counts all six digits."""
    for p, c in enumerate(prefix_counts(k)[:5]):
        if c <= MULTI_CAND_CAP:
            return p
    return None


# ---- populations -------------------------------------------------------------------------------------------------------------------------
def _cluster(n, step):
    # errors 1 + 2^-20 + j step: squared, 1 + 2^-19 + ~2 j step -- with step = 2^-25 the keys share 22 top bits and spread over 33, with
    # 2^-36 they share 33 and spread over 44
    return 1.0 + 2.0**-20 + np.arange(n)*step


def _bin_population(rng, in_bin):
    # `in_bin` squared errors in [0.5, 2) -- the digit-0 bin of the median --, 700 below 0.4 and 700 above 2.1, shuffled
    err = np.concatenate([rng.uniform(0.75, 1.35, in_bin), rng.uniform(0.05, 0.6, 700), rng.uniform(1.5, 3.0, 700)])
    rng.shuffle(err)
    return err


BIN_N = {"bin_4096": 4096 + 1400, "bin_4097": 4097 + 1400}
EXTRA = ("exit_pass_2", "exit_pass_3", "found_in_one_slice", "one_found", "zero_and_huge", "zero_and_inf")
MEDIAN = ("ties", "sixty_binades", "all_equal", "many_zero", "zero_median", "lognormal", "dense_cluster", "outlier_first", "tiny_first")
HARD = MEDIAN + EXTRA
ONE_SLICE_NWG, ONE_SLICE_WG = 16, 5        # found_in_one_slice: the records of workgroup 5 of 16


@functools.lru_cache(maxsize=None)
def _populations(n, seed):
    import test_img_gpu as tig
    rng = np.random.default_rng([seed, n])
    out = {name: (err, None) for name, err in tig._median_cases(rng, n)}
    out["exit_pass_2"] = (_cluster(n, 2.0**-25), None)
    out["exit_pass_3"] = (_cluster(n, 2.0**-36), None)
    i0, i1 = slices(n, ONE_SLICE_NWG)[ONE_SLICE_WG]
    f = np.zeros(n, dtype=np.int32); f[i0:i1] = 1
    out["found_in_one_slice"] = (np.exp(rng.normal(0.0, 1.0, n)), f)
    f = np.zeros(n, dtype=np.int32); f[(3*n)//4] = 1
    out["one_found"] = (np.exp(rng.normal(0.0, 1.0, n)), f)
    zh = np.exp(rng.normal(0.0, 1.0, n))
    f = (rng.random(n) >= 0.15).astype(np.int32)
    if n >= 3:
        zh[n//3] = 0.0; zh[(2*n)//3] = 1e150; f[n//3] = f[(2*n)//3] = 1
    out["zero_and_huge"] = (zh, f)
    zi = zh.copy()
    if n >= 3:
        zi[(2*n)//3] = 1e200           # squared: infinity, the key 0x7ff0 0000 0000 0000 in the last bin of the first digit
    out["zero_and_inf"] = (zi, f)
    return out


@functools.lru_cache(maxsize=None)
def population(name, n, seed=0):
    """The records of a named population at n records (bin_4096 / bin_4097 have their own n)."""
    rng = np.random.default_rng([seed, n, 1])
    if name in BIN_N:
        assert n == BIN_N[name]
        r = records(n, _bin_population(rng, n - 1400), unfound=0)
    else:
        err, f = _populations(n, seed)[name]
        r = records(n, err, found=f, unfound=0.15 if n > 100 else 0.0, rng=rng)
    r.setflags(write=False)
    return r


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One call: `kind` refine / sharded, the records, the rig, the schedule, the estimator, the switches, and what the case is there for
    (`expect`: exit = the histogram median's exit digit, nf, empty = a slice without found records, branch = se3_exp_step's)."""

    def __init__(self, name, recs, env=None, ncam=2, nit=None, nl=None, ov=None, est="Tukey", kind="refine", hard=True, **expect):
        self.name, self._recs, self.env, self.ncam, self.est, self.kind, self.hard, self.expect = name, recs, dict(env or {}), ncam, est, kind, hard, expect
        if nit is not None:
            nl, ov = np.array([1, 0, 0][:nit], dtype=np.uint8), np.zeros(nit)
        self.nl, self.ov = nl, ov              # None: the fine stage's ten iterations

    def rig(self):
        """(records, cameras, CamFromBase, BaseFromWorld)"""
        cam, cfbs, bfw, _ = scene()
        r = self._recs() if callable(self._recs) else self._recs
        if self.ncam == 2:
            return r, [cam, cam], cfbs, bfw
        r, cams, cf = spread_cameras(r, self.ncam)
        return r, cams, cf, bfw

    def schedule(self):
        return {} if self.nl is None else dict(nonlinear=self.nl, override_sigma=self.ov)

    def n_iter(self):
        return 10 if self.nl is None else len(self.nl)

    def route(self):
        r = self._recs() if callable(self._recs) else self._recs
        return route_of_env(len(r), self.ncam, self.n_iter(), self.env)

    def __repr__(self):
        return self.name


def _pop(name, n):
    return lambda: population(name, n)


# the routes the hard populations run on: name -> (n, cameras, switches, kind, populations)
HARD_ROUTES = {
    "plain_1025": (1025, 2, {K_MULTI: "0"}, "refine", HARD),
    "plain_2047": (2047, 2, {K_MULTI: "0"}, "refine", ("ties", "many_zero", "lognormal")),
    "plain_2048": (2048, 2, {K_MULTI: "0"}, "refine", ("ties", "many_zero", "lognormal")),
    "plain_2049": (2049, 2, {K_MULTI: "0"}, "refine", HARD),
    "plain_9cam_130": (130, 9, {}, "refine", HARD),
    "multi_hist_5000": (5000, 2, {}, "refine", HARD),
    "multi_hist_12500": (12500, 2, {}, "refine", ("outlier_first",)),
    "multi_gather_5000": (5000, 2, {K_GATHER: "1"}, "refine", HARD),
    "sharded_1025": (1025, 2, {}, "sharded", HARD),
}
# the digit after which the histogram median leaves the global passes (None: never), where the case is there for it
EXITS = {("multi_hist_5000", "lognormal"): 0, ("multi_hist_12500", "outlier_first"): 1, ("multi_hist_5000", "exit_pass_2"): 2,
         ("multi_hist_5000", "exit_pass_3"): 3, ("multi_hist_5000", "dense_cluster"): 4, ("multi_hist_5000", "all_equal"): None}


def hard_cases(rname):
    n, ncam, env, kind, pops = HARD_ROUTES[rname]
    out = []
    for p in pops:
        for nit in (1, 2, 3):
            ex = {"exit": EXITS[(rname, p)]} if (rname, p) in EXITS else {}
            out.append(Case("%s-%s-%d" % (rname, p, nit), _pop(p, n), env, ncam, nit=nit, kind=kind, **ex))
    for est in ("Huber", "Cauchy"):
        for p in [q for q in ("ties", "lognormal") if q in pops]:
            for nit in (1, 2, 3):
                out.append(Case("%s-%s-%s-%d" % (rname, p, est, nit), _pop(p, n), env, ncam, nit=nit, est=est, kind=kind))
    return out


def cand_cap_cases():
    # 4096 keys in the median's bin are gathered after digit 0, 4097 take another global pass
    return [Case("%s-%d" % (p, nit), _pop(p, BIN_N[p]), nit=nit, exit=x, in_bin=BIN_N[p] - 1400) for p, x in (("bin_4096", 0), ("bin_4097", 1)) for nit in (1, 2, 3)]


def _plain_recs(n, seed, unfound=0.1):
    """n records of the scene with found positions jittered (no two alike) and a share unfound -- well-behaved data."""
    def make():
        cam, cfbs, bfw, recs0 = scene()
        rng = np.random.default_rng([seed, n, 2])
        r = np.tile(recs0, n//len(recs0) + 1)[:n].copy()
        r["found_pos"] += rng.normal(size=(n, 2))*0.3
        r["found"][rng.random(n) < unfound] = 0
        return r
    return functools.lru_cache(maxsize=None)(make)


def slice_cases():
    m2 = {K_MULTI: "2"}
    none = _plain_recs(2048, 7)

    def nothing_found():
        r = none().copy(); r["found"] = 0
        return r
    return [Case("one_record_per_workgroup", _plain_recs(64, 1), dict(m2, **{K_PPW: "1"}), hard=False, nwg=64),
            Case("two_sizes_of_slice", _plain_recs(130, 2), dict(m2, **{K_PPW: "2"}), hard=False, nwg=64),
            Case("workgroup_cap", _plain_recs(6000, 3), {K_PPW: "64"}, hard=False, nwg=64),
            Case("found_in_one_slice", _pop("found_in_one_slice", 2048), {K_PPW: "128"}, nit=3, nwg=ONE_SLICE_NWG, empty=ONE_SLICE_NWG - 1),
            Case("one_found", _pop("one_found", 2048), {K_PPW: "128"}, nit=3, nwg=16, empty=15, nf=1),
            Case("nothing_found", nothing_found, {K_PPW: "128"}, hard=False, nwg=16, empty=16, nf=0),
            Case("below_the_forced_floor", _plain_recs(63, 4), m2, hard=False)]


def gather_cases():
    return [Case("gather_%d" % n, _plain_recs(n, 5), {K_GATHER: "1"}, hard=False) for n in (GATHER_MAX_N, GATHER_MAX_N + 1)]


def iteration_cases():
    out = []
    for k in (MULTI_MAX_ITER, MULTI_MAX_ITER + 1):
        nl = np.zeros(k, dtype=np.uint8); nl[[0, 4, 9, 15]] = 1
        ov = np.where(np.arange(k) % 3 == 2, 16.0, -1.0); ov[-1] = -1.0      # the last slot's median is taken
        out.append(Case("iterations_%d" % k, _plain_recs(2000, 6), {}, nl=nl, ov=ov, hard=False))
    return out


# se3_exp_step's branches on |omega|^2 and the seams between them; on the scene with all weights 1 one iteration from found positions
# image + s (found - image) steps by |omega|^2 = STEP_W2 s^2
STEP_SEAMS = (1e-8, 1e-6, 0.25)
STEP_BRANCHES = ("one_term", "two_terms", "series", "closed_form")
STEP_W2 = 6.198e-6


def step_branch(w2):
    return STEP_BRANCHES[sum(1 for s in STEP_SEAMS if not w2 < s)]


def step_scales():
    """(scale, branch) pairs: 1 % below and above every seam, one deep in the first branch, one deep in the last."""
    out = [(1e-4, "one_term")]
    for k, seam in enumerate(STEP_SEAMS):
        s = float(np.sqrt(seam/STEP_W2))
        out += [(0.99*s, STEP_BRANCHES[k]), (1.01*s, STEP_BRANCHES[k + 1])]
    return out + [(1000.0, "closed_form")]


def _step_recs(s):
    def make():
        r = scene()[3].copy()
        r["found_pos"] = r["image"] + s*(r["found_pos"] - r["image"])
        return r
    return functools.lru_cache(maxsize=None)(make)


STEP_ROUTES = {"regs": (2, {}, "refine"), "plain": (9, {}, "refine"), "multi": (2, {K_MULTI: "2", K_PPW: "64"}, "refine"), "sharded": (2, {}, "sharded")}


def step_cases(rname):
    ncam, env, kind = STEP_ROUTES[rname]
    return [Case("step-%s-%.6g" % (rname, s), _step_recs(s), env, ncam, nl=np.array([1], dtype=np.uint8), ov=np.array([1e30]), kind=kind, hard=False, branch=b)
            for s, b in step_scales()]


def few_found_cases():
    out = []
    for n, env in ((1025, {K_MULTI: "0"}), (2048, {})):
        for nf in (1, 2, 3):
            def make(n=n, nf=nf):
                rng = np.random.default_rng([nf, n, 3])
                f = np.zeros(n, dtype=np.int32); f[rng.choice(n, nf, replace=False)] = 1
                return records(n, np.exp(rng.normal(0.0, 1.0, n)), found=f)
            for nit in (1, 3):
                out.append(Case("few-%d-of-%d-%d" % (nf, n, nit), functools.lru_cache(maxsize=None)(make), env, nit=nit, nf=nf))
    return out


SHARD_PAD = 37            # the sharded cases' cap = n + SHARD_PAD: the table's rows are longer than any rank's list


def shard_slot_cases():
    return [Case("shard-rank%d-%d" % (rank, nit), _pop("many_zero", 1025), nit=nit, kind="sharded", rank=rank, world=2) for rank in (0, 1) for nit in (1, 2, 3)]


UPDATE_POPS, UPDATE_N = ("ties", "many_zero", "one_found"), (1, 255, 256, 257, 1025)


def update_inputs(pop, n):
    """track_pose_update's arrays for a population: (found, found_pos, image, sqrt_inv_noise, jacobian)."""
    r = population(pop, n)
    J = np.random.default_rng([n, 4]).normal(size=(n, 12))*30
    return (r["found"] != 0).astype(np.uint8), r["found_pos"].copy(), r["image"].copy(), r["sqrt_inv_noise"].copy(), J


def reuse_sequence():
    """One process, one scratch: a large multi call, small register-held ones, plain ones, forced multi, the redo after a give-up -- each
    with its own found mask."""
    m2 = {K_MULTI: "2"}
    return [Case("reuse-1-multi-6000", _plain_recs(6000, 11, 0.1), {}, hard=False),
            Case("reuse-2-regs-280", _plain_recs(280, 12, 0.3), {}, hard=False),
            Case("reuse-3-plain-1025", _plain_recs(1025, 13, 0.2), {K_MULTI: "0"}, hard=False),
            Case("reuse-4-multi-130", _plain_recs(130, 14, 0.4), m2, hard=False),
            Case("reuse-5-regs-64", _plain_recs(64, 15, 0.25), {}, hard=False),
            Case("reuse-6-plain-9cam-130", _plain_recs(130, 16, 0.35), {}, ncam=9, hard=False),
            Case("reuse-7-redo-6000", _plain_recs(6000, 17, 0.15), {K_GIVEUP: "1"}, hard=False)]


REFINE_GROUPS = {**{"hard-" + r: functools.partial(hard_cases, r) for r in HARD_ROUTES}, "cand_cap": cand_cap_cases, "slices": slice_cases,
                 "gather": gather_cases, "iterations": iteration_cases, **{"step-" + r: functools.partial(step_cases, r) for r in STEP_ROUTES},
                 "few_found": few_found_cases, "shard_slots": shard_slot_cases, "reuse": reuse_sequence}
