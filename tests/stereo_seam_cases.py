"""The cases that pin the AddStereoMapPoints kernels (mcptam_amd/csrc/stereo_kernels.h) at their thinning, limit and pose seams, and the numpy
restatements they are compared with -- shared by tests/test_stereo_seams_cpu.py (which shows on the reference alone that every case has the
layout it is named for) and tests/test_stereo_seams_gpu.py (which runs them).

Pure numpy + the CPU oracle: nothing here needs a GPU.

1. thinning alone (k_stereo_thin_meas, n_targets = 0): hand-made integer candidates against hand-made measurements -- the 10-pixel radius, the
   rounding of v2RootPos / LevelScale, the level filter, the block sizes.  `thin_restated` is ThinCandidates with one deliberate error switched
   on, to show that a case tells the right rule from the wrong one.
2. k_stereo_thin_new / k_stereo_commit: candidate lists made of the fixture's level-2 candidates by repetition, `limit_model` the nLimit loop
   (:486-493) over a table of which (target, position) creates.
3. a moved world, a second target camera, a skewed source camera.
4. the epipolar arc at its clamp, sign, step-count and guard seams, `arc_ld` the arc in np.longdouble.
"""
import functools
import math

import numpy as np

from mcptam_amd import stereo as S
from mcptam_amd.synth import DEFAULT_CAM_PARAMS, so3_exp
from mcptam_amd.taylor_camera import TaylorCamera

LD = np.longdouble
W, H = 640, 480
COMMIT_NT = 256                               # stereo_kernels.h STEREO_COMMIT_NT: candidates of one chunk of k_stereo_commit, and of a thinning block
SEAM_LEVEL = 2                                # the level of every case with an image search


def level_size(level):
    return W >> level, H >> level


# =================================================================================================================================================
# 1. thinning alone
# =================================================================================================================================================
def _round(v, rounding):
    v = np.asarray(v, dtype=np.float64)
    if rounding == "away":                    # CVD::ir_rounded
        return S.ir_rounded(v)
    if rounding == "trunc":
        return np.trunc(v).astype(np.int64)
    if rounding == "floor_half":              # floor(v + 0.5): half towards +inf
        return np.floor(v + 0.5).astype(np.int64)
    if rounding == "plus_half":               # (int)(v + 0.5) on both sides of zero
        return np.trunc(v + 0.5).astype(np.int64)
    if rounding == "even":                    # rint
        return np.rint(v).astype(np.int64)
    if rounding == "ceil":
        return np.ceil(v).astype(np.int64)
    raise ValueError(rounding)


def thin_restated(cand, level, meas_root, meas_level, le=False, rounding="away", level_only=False, wrap32=False):
    """ThinCandidates (:411-446) with one error switched on: `le` thins at distance 10 too, `rounding` another rounding of the busy position,
    `level_only` drops the level + 1 measurements, `wrap32` squares the distance in 32-bit integers.  With none it is stereo.thin_candidates."""
    c = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    sc = float(1 << level)
    keep = np.ones(len(c), dtype=bool)
    for r, l in zip(meas_root, meas_level):
        if not (l == level or (l == level + 1 and not level_only)):
            continue
        d = c - _round(np.asarray(r, dtype=np.float64) / sc, rounding)
        d2 = (d * d).sum(axis=1)
        if wrap32:
            d2 = ((d2 + (1 << 31)) % (1 << 32)) - (1 << 31)
        keep &= ~(d2 <= 100 if le else d2 < 100)
    return keep


def _thin_case(name, level, cand, meas_root, meas_level, **kw):
    cand = np.asarray(cand, dtype=np.int32).reshape(-1, 2)
    w, h = level_size(level)
    assert len(cand) and (cand >= 0).all() and (cand[:, 0] < w).all() and (cand[:, 1] < h).all(), name
    root = np.asarray(meas_root, dtype=np.float64).reshape(-1, 2)
    lv = np.asarray(meas_level, dtype=np.int32).reshape(-1)
    assert len(root) == len(lv) and (np.abs(root) <= 1e9).all(), name
    return dict(name=name, level=level, cand=cand, meas_root=root, meas_level=lv, **kw)


RADIUS_OFFSETS = {97: (9, 4), 98: (7, 7), 100: (10, 0), 1000: (6, 8), 101: (10, 1)}      # (1000: the second way to write 100)


def signed_offsets(dx, dy):
    """every sign and axis combination of (dx, dy)"""
    out = set()
    for a, b in ((dx, dy), (dy, dx)):
        for sa in (1, -1):
            for sb in (1, -1):
                out.add((sa * a, sb * b))
    return sorted(out)


def thin_radius_cases():
    """one busy position, candidates at squared distances 97, 98, 100 (both ways) and 101 in every sign and axis combination"""
    out = []
    for level, b in ((0, (300, 200)), (2, (80, 60)), (3, (30, 30))):
        offs = [o for d in RADIUS_OFFSETS.values() for o in signed_offsets(*d)]
        cand = np.array(b) + np.array(offs)
        out.append(_thin_case("radius_L%d" % level, level, cand, [np.array(b, dtype=np.float64) * (1 << level)], [level], busy=b, offsets=offs))
    return out


ROUND_VALUES = (0.5, -0.5, 1.5, -1.5, 0.49999999999999994, -0.49999999999999994, 2.49, -2.51)
ROUND_EXPECT = (1, -1, 2, -2, 1, -1, 2, -3)   # ir_rounded: (int)(v +- 0.5); 0.49999999999999994 + 0.5 is 1.0 in float64, and so is the C++ sum
ROUND_OTHER = 20                              # the busy position's other coordinate


def thin_rounding_cases():
    """One measurement whose quotient v2RootPos / LevelScale is exactly v along one axis; candidates 9 and 10 away (along that axis) from the
    rounded position and from both its neighbours, where the image has them: a busy position off by one flips a keep bit."""
    out = []
    for level in (0, 2):
        sc = float(1 << level)
        for axis in (0, 1):
            for v, r in zip(ROUND_VALUES, ROUND_EXPECT):
                q = np.array([ROUND_OTHER, ROUND_OTHER], dtype=np.float64)
                q[axis] = v
                pos = sorted({p + d for p in (r - 1, r, r + 1) for d in (9, 10, -9, -10) if p + d >= 0})
                cand = np.full((len(pos), 2), ROUND_OTHER)
                cand[:, axis] = pos
                out.append(_thin_case("round_L%d_axis%d_%r" % (level, axis, v), level, cand, [q * sc], [level], value=v, expect=r, axis=axis))
    return out


def thin_wide_cases():
    """A measurement near the entry's bound (|root_pos| <= 1e9) against candidates at the corners: the difference of the positions squared needs
    64 bits.  The offsets are multiples of 65536, whose squares are 0 in 32-bit arithmetic -- a 32-bit stereo_busy would thin."""
    out = []
    for level, k in ((0, 15258), (3, 1907)):
        w, h = level_size(level)
        sc = float(1 << level)
        far = k * 65536
        cand = np.array([[0, 0], [w - 1, h - 1], [w - 1, 0], [5, 7]])
        roots = np.array([[w - 1 + far, h - 1 + far], [-far, -far], [w - 1 - far, far], [5 + 65536, 7]], dtype=np.float64) * sc
        assert (np.abs(roots) < 1e9).all() and np.abs(roots).max() > 0.99e9
        out.append(_thin_case("wide_L%d" % level, level, cand, roots, [level, level + 1, level, level]))
    return out


def thin_level_cases():
    """for every call level, measurements at level - 1 .. level + 2 (-1 and 4, 5 among them), each on top of one candidate and 9 from another"""
    out = []
    for level in range(4):
        bx = np.array([10, 30, 50, 70])
        lv = np.array([level - 1, level, level + 1, level + 2])
        busy = np.stack([bx, np.full(4, 30)], axis=1)
        cand = np.concatenate([busy, busy + [0, 9]])
        out.append(_thin_case("levels_L%d" % level, level, cand, busy.astype(np.float64) * (1 << level), lv, expect_thinned=np.tile((lv == level) | (lv == level + 1), 2)))
    return out


THIN_SIZES = (1, 255, 256, 257, 513)


def thin_size_cases():
    """n_cand at the block seams with the only thinned candidate at index 0, 255, 256 or last; n_meas 0, 1 or 300 with the only hit last"""
    out = []
    for n in THIN_SIZES:
        i = np.arange(n)
        cand = np.stack([20 + (i % 40) * 15, 20 + (i // 40) * 15], axis=1)
        for t in sorted({t for t in (0, 255, 256, n - 1) if t < n}):
            for n_meas in (0, 1, 300):
                hit = cand[t] + [3, -2]
                m = np.arange(max(n_meas - 1, 0))
                miss = np.stack([15.0 + (m % 100) * 6, 300.0 + (m // 100) * 40], axis=1)      # below the candidate grid, more than 10 from all of it
                roots = np.concatenate([miss, hit[None, :].astype(np.float64)])[:n_meas] if n_meas else np.zeros((0, 2))
                out.append(_thin_case("size_n%d_t%d_m%d" % (n, t, n_meas), 0, cand, roots, np.zeros(n_meas, dtype=np.int32), thinned_at=t if n_meas else None))
    return out


def thin_cases():
    return thin_radius_cases() + thin_rounding_cases() + thin_wide_cases() + thin_level_cases() + thin_size_cases()


def thin_expected(case):
    return S.thin_candidates(case["cand"], case["level"], case["meas_root"], case["meas_level"])


# =================================================================================================================================================
# 4. the arc: np.longdouble restatement, cases
# =================================================================================================================================================
def _unproject_ld(cam, uv):
    a = np.asarray(cam.affine, dtype=LD)
    det = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
    dx, dy = LD(uv[0]) - LD(cam.center[0]), LD(uv[1]) - LD(cam.center[1])
    x, y = (a[1, 1] * dx - a[0, 1] * dy) / det, (-a[1, 0] * dx + a[0, 0] * dy) / det
    rho = np.sqrt(x * x + y * y)
    z = LD(0)
    for c in np.asarray(cam.poly, dtype=LD)[::-1]:
        z = z * rho + c
    v = np.array([x, y, z], dtype=LD)
    return v / np.sqrt(v @ v)


def _unit_ld(v):
    return v / np.sqrt(v @ v)


def arc_ld(cam_src, pose_src, pose_tgt, one_pixel_angle, level, c):
    """AddPointEpipolar's hypotheses (:611-723) and their pixel vectors (MapPoint.cc:62-87) in np.longdouble, the same formulas as stereo.arc with
    the same float64 constants (M_PI, 0.05, 0.2): the reference of the arc tests.  Returns the facts a case is named for as well: start_raw (before
    the clamp), min_t, max_t, dd (v3BetweenEndpoints squared), ratio (max_angle / (opa s 3), whose ceiling is the step count)."""
    with np.errstate(all="ignore"):
        Rs, ts = np.asarray(pose_src[0], dtype=LD), np.asarray(pose_src[1], dtype=LD)
        Rt, tt = np.asarray(pose_tgt[0], dtype=LD), np.asarray(pose_tgt[1], dtype=LD)
        s = 1 << level
        pi = LD(math.pi)
        root = S.level_zero_pos(c, level)
        ray = _unproject_ld(cam_src, root)
        cen, rig, dow = ray, _unproject_ld(cam_src, root + [s, 0.0]), _unproject_ld(cam_src, root + [0.0, s])
        dirn = Rt @ (Rs.T @ ray)
        cc_tc = Rt @ (-(Rs.T @ ts)) + tt
        cc_sc = Rs @ (-(Rt.T @ tt)) + ts
        sep = np.sqrt(cc_sc @ cc_sc)
        res = dict(n=0, sep=sep, start_raw=LD("nan"), min_t=LD("nan"), max_t=LD("nan"), dd=LD("nan"), ratio=LD("nan"))
        src_angle = np.arccos((cc_sc @ ray) / sep)
        min_t, max_t = pi - src_angle - pi / 3, pi - src_angle - LD(0.05)
        start = sep * np.sin(min_t) / np.sin(pi / 3)
        end = sep * np.sin(max_t) / np.sin(LD(0.05))
        res.update(start_raw=start, min_t=min_t, max_t=max_t, end=end, src_angle=src_angle)
        if start < LD(0.2):
            start = LD(0.2)
        RS, RE = cc_tc + start * dirn, cc_tc + end * dirn
        a, b = _unit_ld(RS), _unit_ld(RE)
        d = a - b
        res.update(dd=d @ d)
        if d @ d < LD(1e-8):
            return res
        nrm = _unit_ld(np.cross(a, b))
        J = np.cross(nrm, a)
        max_angle = np.arccos((a @ b) * 1 + (J @ b) * 0)
        ratio = max_angle / (LD(one_pixel_angle) * s * 3)
        res.update(ratio=ratio, max_angle=max_angle)
        if not np.isfinite(ratio) or not (-2147483648.0 <= np.ceil(ratio) <= 2147483646.0):
            return res
        n_steps = int(np.ceil(ratio))
        step = max_angle / n_steps
        rs = np.array([a @ RS, J @ RS])
        rd = np.array([a @ RE, J @ RE]) - rs
        rd = rd / np.sqrt(rd @ rd)
        ang = np.arange(n_steps + 1).astype(LD) * step
        cs, sn = np.cos(ang), np.sin(ang)
        alpha = (rs[0] * sn - rs[1] * cs) / (rd[1] * cs - rd[0] * sn)
        tc = RS[None, :] + alpha[:, None] * dirn[None, :]
        world = (tc - tt) @ Rt
        h = np.abs((world @ Rs.T + ts)[:, 2])
        cc = cen[None, :] * h[:, None] / abs(cen[2])
        pr = (rig[None, :] * h[:, None] / abs(rig[2]) - cc) @ Rs
        pd = (dow[None, :] * h[:, None] / abs(dow[2]) - cc) @ Rs
        res.update(n=n_steps + 1, world=world, pixel_right_w=pr, pixel_down_w=pd, alpha=alpha)
        return res


def row_rel(a, b):
    """largest relative deviation of a row of a from the row of b (max norm); b is the reference"""
    a, b = np.atleast_2d(np.asarray(a, dtype=LD)), np.atleast_2d(np.asarray(b, dtype=LD))
    if a.shape != b.shape:
        return float("inf")
    if a.size == 0:
        return 0.0
    return float((np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), LD(1e-300))).max())


ARC_FIELDS = ("world", "pixel_right_w", "pixel_down_w")


def make_camera(center=(W / 2.0, H / 2.0), poly=None, affine=(1.0, 0.0, 0.0)):
    p = DEFAULT_CAM_PARAMS[:4] if poly is None else tuple(poly)
    return TaylorCamera(p + tuple(center) + tuple(affine), (W, H), (W, H), (W, H))


def skew_camera():
    """a camera whose centre, polynomial and affine all differ from the fixture's; the affine's off-diagonal terms are about 1e-2"""
    return make_camera(center=(W / 2.0 + 31.0, H / 2.0 - 23.0), poly=(262.0, -1.1e-3, 1.4e-7, -1.2e-10), affine=(1.004, 0.011, -0.013))


def axis_camera(level):
    """a camera whose centre is the root position of AXIS_CAND[level]: that candidate's ray is (0, 0, 1) exactly"""
    c = S.level_zero_pos(np.array(AXIS_CAND[level]), level)
    return make_camera(center=(float(c[0]), float(c[1])))


AXIS_CAND = {0: (320, 240), 3: (40, 30)}
ARC_LEVELS = (0, 3)
ARC_SRC_POSE = (so3_exp(np.array([0.3, -0.5, 0.4])), np.array([1.5, -2.0, 0.7]))


def _ray(cam, level, c):
    return cam.unproject(S.level_zero_pos(np.asarray(c), level))[0]


def target_pose(pose_src, centre_sc, turn=(0.02, -0.03, 0.01)):
    """CamFromWorld of a target whose centre is centre_sc in the source camera's frame, turned by `turn` against the source"""
    Rs, ts = pose_src
    Rt = so3_exp(np.asarray(turn, dtype=np.float64)) @ Rs
    cw = Rs.T @ (np.asarray(centre_sc, dtype=np.float64) - ts)
    return Rt, -Rt @ cw


def centre_at(ray, phi, sep):
    """a point at distance sep whose direction makes the angle phi with ray"""
    p = np.cross(ray, [0.3, 1.0, -0.2])
    p /= np.linalg.norm(p)
    return sep * (math.cos(phi) * ray + math.sin(phi) * p)


def _around(level, c, spread):
    w, h = level_size(level)
    pts = [c] + [(c[0] + dx, c[1] + dy) for dx, dy in ((spread, 0), (-spread, 0), (0, spread), (0, -spread))] if spread else [c]
    return np.array([p for p in pts if 0 <= p[0] < w and 0 <= p[1] < h], dtype=np.int32)


def _sep_for_start(cam, level, c, phi, start):
    """the baseline at which the ray of c, at angle phi to it, starts at `start` (:646-652)"""
    return start * math.sin(math.pi / 3) / math.sin(math.pi - phi - math.pi / 3)


def _sep_for_dd(cam, pose_src, level, c, phi, want):
    """the baseline, a little below the one at which the arc's two end points coincide (end = 0.2), at which v3BetweenEndpoints squared is `want`:
    bisection on the longdouble arc"""
    ray = _ray(cam, level, c)

    def dd(sep):
        return float(arc_ld(cam, pose_src, target_pose(pose_src, centre_at(ray, phi, sep)), 1.0, level, c)["dd"])
    hi = 0.2 * math.sin(0.05) / math.sin(math.pi - phi - 0.05)      # end == 0.2: dd == 0
    lo = 0.5 * hi
    assert dd(lo) > want > dd(hi * (1 - 1e-9))
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if dd(mid) > want:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def arc_cases():
    """Every arc case: dict(name, level, cam, pose_src, pose_tgt, opa, cand, claim).  `claim` names the path the CPU test proves the case takes."""
    out = []

    def add(name, level, cam, pose_src, pose_tgt, cand, claim, opa=None):
        out.append(dict(name="%s_L%d" % (name, level), level=level, cam=cam, pose_src=pose_src, pose_tgt=pose_tgt,
                        opa=cam.one_pixel_angle() if opa is None else float(opa), cand=np.asarray(cand, dtype=np.int32).reshape(-1, 2), claim=claim))
    cam = make_camera()
    for level in ARC_LEVELS:
        w, h = level_size(level)
        mid = (w // 2 + 7, h // 2 - 5)
        ray = _ray(cam, level, mid)
        P = ARC_SRC_POSE
        side = math.pi / 2
        # the start < 0.2 clamp: a hair either side for one candidate, comfortably either side for five
        for name, start, spread in (("clamp_on_tight", 0.2 * (1 - 1e-3), 0), ("clamp_off_tight", 0.2 * (1 + 1e-3), 0), ("clamp_on", 0.17, 1), ("clamp_off", 0.23, 1)):
            sep = _sep_for_start(cam, level, mid, side, start)
            add(name, level, cam, P, target_pose(P, centre_at(ray, side, sep)), _around(level, mid, spread), name.replace("_tight", ""))
        # rays that point away from the target: more than 2 pi / 3, and more than pi - 0.05, from the baseline
        add("min_t_neg", level, cam, P, target_pose(P, centre_at(ray, 2 * math.pi / 3 + 0.2, 1.0)), _around(level, mid, 1), "min_t_neg")
        add("max_t_neg", level, cam, P, target_pose(P, centre_at(ray, math.pi - 0.02, 1.0)), _around(level, mid, 1 if level == 0 else 0), "max_t_neg")
        # two hypotheses: a one_pixel_angle for which the arc is 0.6 steps long
        tp = target_pose(P, centre_at(ray, side, 1.0))
        ma = float(arc_ld(cam, P, tp, 1.0, level, mid)["max_angle"])
        add("one_step", level, cam, P, tp, _around(level, mid, 1), "one_step", opa=ma / (3 * (1 << level)) / 0.6)
        # the v3BetweenEndpoints guard, 1e-8, from both sides
        for name, want in (("guard_below", 0.8e-8), ("guard_above", 1.25e-8)):
            sep = _sep_for_dd(cam, P, level, mid, side, want)
            add(name, level, cam, P, target_pose(P, centre_at(ray, side, sep)), [mid], name)
        # the target on the candidate's ray, before and behind the source: exact (the ray is the camera's axis, no rotation, integer translations)
        ac = axis_camera(level)
        I3, ts = np.eye(3), np.array([1.0, 2.0, 3.0])
        for name, z in (("through_fwd", 2.0), ("through_bwd", -2.0)):
            add(name, level, ac, (I3, ts), (I3, ts - np.array([0.0, 0.0, z])), [AXIS_CAND[level]], "no_arc")
        # the target at the source's centre, turned: quarter turns and integer translations, so that the baseline is 0 exactly
        Rq, Rq2 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
        add("same_centre", level, cam, (Rq, ts), (Rq2, -Rq2 @ (-Rq.T @ ts)), _around(level, mid, 3), "no_arc")
        # a source camera with a non-trivial affine, candidates all over the image
        sk = skew_camera()
        grid = np.array([(x, y) for x in (2, w // 3, w // 2, w - 3) for y in (1, h // 2, h - 2)], dtype=np.int32)
        add("skew_src", level, sk, P, target_pose(P, np.array([0.5, -0.2, 0.1])), grid, "plain")
        # the fixture's poses in the moved world
        sc = scene()
        for j in (0, 2):
            add("moved_world_t%d" % j, level, sc["cam"], sc["pose_src_moved"], sc["poses_moved"][j], grid, "plain")
    return tuple(out)


def arc_reference(case):
    """[arc_ld of every candidate of the case]"""
    return [arc_ld(case["cam"], case["pose_src"], case["pose_tgt"], case["opa"], case["level"], c) for c in case["cand"]]


def arc_deviation(ref, got):
    """largest row_rel over the candidates and the three exported vectors; ref: arc_reference, got: per candidate a dict with ARC_FIELDS' keys"""
    dev = 0.0
    for r, g in zip(ref, got):
        if r["n"]:
            dev = max([dev] + [row_rel(g[k], r[k]) for k in ARC_FIELDS])
    return dev


def arc_floor(case, ref=None):
    """how far stereo.arc (float64) lies from arc_ld on this case: the floor a float64 evaluation of these formulas has"""
    ref = arc_reference(case) if ref is None else ref
    got = [S.arc(case["cam"], case["pose_src"], case["pose_tgt"], case["opa"], case["level"], c) for c in case["cand"]]
    return arc_deviation(ref, got)


def arc_bound(case, ref=None):
    """the device's bound: 8 x the float64 floor (the margin test_pose_routes gives another evaluation order), at least 1e-12"""
    return max(8.0 * arc_floor(case, ref), 1e-12)


# =================================================================================================================================================
# 2. / 3. the scene, which (target, position) creates, and the nLimit loop
# =================================================================================================================================================
MOVE_G = (so3_exp(0.7 * np.array([0.48, -0.6, 0.64])), np.array([2.5, -1.5, 3.0]))      # the moved world: x' = G x, 0.7 rad about an oblique axis


def move_pose(pose, G=MOVE_G):
    """CamFromWorld * G^-1"""
    R, t = pose
    Rg, tg = G
    Rn = R @ Rg.T
    return Rn, t - Rn @ tg


def unmove_points(x, G=MOVE_G):
    """G^-1 x for rows x"""
    Rg, tg = G
    return (np.atleast_2d(x) - tg) @ Rg


@functools.lru_cache(maxsize=None)
def scene():
    """make_stereo_scene() plus target 0 rendered once more through skew_camera() (`img_skew`) and the moved poses"""
    from mcptam_amd import synth_img
    sc = synth_img.make_stereo_scene()
    sk = skew_camera()
    sc["cam_skew"] = sk
    sc["img_skew"] = synth_img.render_plane(sk, sc["poses"][0][0], sc["poses"][0][1], sc["tex"], sc["depth"])
    sc["pose_src_moved"] = move_pose(sc["pose_src"])
    sc["poses_moved"] = [move_pose(p) for p in sc["poses"]]
    return sc


@functools.lru_cache(maxsize=None)
def oracle_frames():
    """the oracle's keyframes of scene(): source (with candidates), the four targets, the skew-camera target"""
    from oracle import OracleKeyFrame
    sc = scene()
    src = OracleKeyFrame(W, H)
    src.MakeKeyFrame_Lite(sc["img_src"]); src.MakeKeyFrame_Rest()
    tg = []
    for im in sc["imgs"] + [sc["img_skew"]]:
        o = OracleKeyFrame(W, H)
        o.MakeKeyFrame_Lite(im)
        tg.append(o)
    return dict(src=src, tg=tg[:4], skew=tg[4])


def hyp_from_arc(cam_src, pose_src, level, cand, target):
    """the export of stereo.stereo_hypotheses from stereo.arc: (TD_IN_DTYPE array, offsets)"""
    opa = target[3] if len(target) > 3 else target[1].one_pixel_angle()
    arcs = [S.arc(cam_src, pose_src, target[2], opa, level, c) for c in cand]
    off = np.concatenate([[0], np.cumsum([a["n"] for a in arcs])]).astype(np.int32)
    hyp = np.zeros(off[-1], dtype=S.TD_IN_DTYPE)
    for i, (a, c) in enumerate(zip(arcs, cand)):
        h = hyp[off[i]:off[i + 1]]
        h["world_pos"], h["pixel_right_w"], h["pixel_down_w"] = a["world"], a["pixel_right_w"], a["pixel_down_w"]
        h["source_level"], h["center_x"], h["center_y"] = level, c[0], c[1]
    return hyp, off


def oracle_results(cam_src, pose_src, level, cand, target, search_kf, src_oracle):
    """{i: (code, hypothesis, score, sub-pixel position)} of every candidate alone against one target, by the oracle's PatchFinder"""
    from oracle import oracle_patch_sequences
    hyp, off = hyp_from_arc(cam_src, pose_src, level, cand, target)
    return S.compose_target(oracle_patch_sequences, search_kf, target[1], target[2], hyp, off, list(range(len(cand))), None, src_oracle)


def oracle_codes(cand, js=(0, 1, 2, 3), level=SEAM_LEVEL):
    """(len(js) x n) outcome codes of the positions cand, each alone against the fixture's target js[k], on the CPU"""
    sc, fr = scene(), oracle_frames()
    cand = np.asarray(cand, dtype=np.int32).reshape(-1, 2)
    out = np.zeros((len(js), len(cand)), dtype=np.uint8)
    for k, j in enumerate(js):
        res = oracle_results(sc["cam"], sc["pose_src"], level, cand, (None, sc["cam"], sc["poses"][j]), fr["tg"][j], fr["src"])
        out[k] = [res[i][0] for i in range(len(cand))]
    return out


def limit_model(cand, level, codes, limit, meas_root=(), meas_level=()):
    """AddStereoMapPoints' loops (:456-496) over a table codes[j][i] of what candidate i gives against target j when it is tried: per target
    dict(alive, tried, made, base, first), the expected outcome table and the keep mask.  numSuccess counts over the targets and only leaves the
    candidate loop, after the candidate that was tried."""
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    n = len(cand)
    alive = S.thin_candidates(cand, level, meas_root, meas_level)
    num, new, per = 0, [], []
    outcome = np.zeros((len(codes), n), dtype=np.uint8)
    for j in range(len(codes)):
        if len(new):
            alive = alive & S.thin_candidates(cand, level, created_root=new)
        tried, made = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        base = num
        for i in np.nonzero(alive)[0]:
            tried[i] = True
            if codes[j][i] == S.CREATED:
                made[i] = True
                num += 1
            if num >= limit:
                break
        new = S.level_zero_pos(cand[made], level)
        live = np.nonzero(alive)[0]
        per.append(dict(alive=alive.copy(), tried=tried, made=made, base=base, first=int(live[0]) if len(live) else -1))
        outcome[j] = np.where(~alive, S.THINNED, np.where(tried, codes[j], S.PAST_LIMIT))
    return per, outcome, alive.copy()


def expand(codes_unique, inverse):
    return np.asarray(codes_unique)[:, inverse]


def unique_positions(cand):
    """(unique positions, inverse) of a candidate list with repetitions"""
    u, inv = np.unique(np.asarray(cand, dtype=np.int32).reshape(-1, 2), axis=0, return_inverse=True)
    return u, np.asarray(inv).reshape(-1)


COMMIT_SIZES = (255, 256, 257, 512, 513)
COMMIT_TARGETS = (0, 1)


def seam_order(base, codes0):
    """The fixture's candidates in an order whose tiling puts a creation (under the first target) on both sides of the chunk seam: list indices
    COMMIT_NT - 1 and COMMIT_NT hold creating candidates."""
    nb = len(base)
    order = np.arange(nb)
    c = np.nonzero(codes0 == S.CREATED)[0]
    assert len(c) >= 2
    for want, pick in (((COMMIT_NT - 1) % nb, c[0]), (COMMIT_NT % nb, c[1])):
        at = int(np.nonzero(order == pick)[0][0])
        order[[want, at]] = order[[at, want]]
    return order


def limit_cases(base, codes):
    """Lists of n_cand in COMMIT_SIZES made of the fixture's candidates by repetition, two targets, and the limits around the chunk seam.
    base: the level-2 candidates; codes: (>= 2 x len(base)) their outcomes alone against the targets COMMIT_TARGETS."""
    out = []
    order = seam_order(base, codes[0])
    for n in COMMIT_SIZES:
        idx = np.resize(order, n)
        cand, cd = base[idx], codes[:2][:, idx]
        per, _, _ = limit_model(cand, SEAM_LEVEL, cd, 1 << 30)
        c0 = int(per[0]["made"][:COMMIT_NT].sum())
        total = int(per[0]["made"].sum() + per[1]["made"].sum())
        for name, limit in (("c0-1", c0 - 1), ("c0", c0), ("c0+1", c0 + 1), ("total", total), ("total+1", total + 1), ("one", 1), ("zero", 0), ("minus3", -3)):
            out.append(dict(name="n%d_%s" % (n, name), kind=name, n=n, cand=cand, index=idx, targets=COMMIT_TARGETS, limit=limit, c0=c0, total=total,
                            meas_root=np.zeros((0, 2)), meas_level=np.zeros(0, dtype=np.int32)))
    return out


def _far(base, i, others, r2):
    d = base[others] - base[i]
    return ((d * d).sum(axis=1) >= r2).all()


def survivor_cases(base, codes):
    """Candidates 0 .. 255 all thinned by one measurement (256 copies of the candidate it sits on); then F, which target 0 tries without creating,
    then candidates that create under target 0, then the rest.  limit = 2: target 0 stops after its second creation, base = 2 >= limit when target
    1 starts, and target 1's one exempt candidate is F at index 256, in chunk 1.  `creates`: F creates under target 1; two and three targets."""
    created0 = np.nonzero(codes[0] == S.CREATED)[0]
    out = []
    for creates in (True, False):
        f_ok = (codes[0] != S.CREATED) & ((codes[1] == S.CREATED) == creates)
        pick = None
        for f in np.nonzero(f_ok)[0]:
            xs = [x for x in created0 if _far(base, x, [f], 400)][:2]
            ms = [m for m in range(len(base)) if m != f and _far(base, m, [f] + xs, 400)]
            if len(xs) == 2 and ms:
                pick = (int(f), [int(x) for x in xs], int(ms[0]))
                break
        assert pick is not None
        f, xs, m = pick
        rest = [i for i in range(len(base)) if i not in (f, m, xs[0], xs[1]) and _far(base, i, [m], 100)]
        idx = np.array([m] * COMMIT_NT + [f] + xs + rest)
        for nt in (2, 3):
            out.append(dict(name="survivor_%s_%dt" % ("creates" if creates else "fails", nt), kind="survivor", creates=creates, n=len(idx), cand=base[idx], index=idx,
                            targets=tuple(range(nt)), limit=2, meas_root=S.level_zero_pos(base[[m]], SEAM_LEVEL), meas_level=np.array([SEAM_LEVEL], dtype=np.int32)))
    return out


def dead_cases(base, codes):
    """Targets for which no candidate is alive.  from_start: a measurement on every candidate.  after_0: 257 copies of one candidate that creates
    under target 0 -- they all create (the reference does not thin within a target), across the chunk seam, and thin each other for targets 1, 2."""
    x = int(np.nonzero(codes[0] == S.CREATED)[0][0])
    idx = np.resize(np.arange(len(base)), COMMIT_NT + 1)
    return [dict(name="dead_from_start", kind="dead", n=len(idx), cand=base[idx], index=idx, targets=(0, 1), limit=1 << 30,
                 meas_root=S.level_zero_pos(base, SEAM_LEVEL), meas_level=np.full(len(base), SEAM_LEVEL, dtype=np.int32), dead_from=0),
            dict(name="dead_after_0", kind="dead", n=COMMIT_NT + 1, cand=base[[x] * (COMMIT_NT + 1)], index=np.array([x] * (COMMIT_NT + 1)), targets=(0, 1, 2),
                 limit=1 << 30, meas_root=np.zeros((0, 2)), meas_level=np.zeros(0, dtype=np.int32), dead_from=1)]


NEIGHBOUR_D2 = (97, 98, 100, 101)


def neighbour_case(base, codes, codes_at):
    """The fixture's candidates plus four hand-made positions at squared distances 97, 98, 100, 101 from candidates that create under target 0.
    Each hand-made position is at least 10 from every other creation of target 0 and does not create under target 0 itself (codes_at(positions)
    says so), so after target 0 exactly the first two are thinned.  The four are the list's last entries."""
    w, h = level_size(SEAM_LEVEL)
    created0 = base[codes[0] == S.CREATED]
    extra, hosts = [], []
    for d2 in NEIGHBOUR_D2:
        found = None
        for x in created0:
            others = created0[(created0 != x).any(axis=1)]
            for o in signed_offsets(*RADIUS_OFFSETS[d2]):
                p = x + np.array(o)
                if not (12 <= p[0] < w - 12 and 12 <= p[1] < h - 12):
                    continue
                if ((others - p) ** 2).sum(axis=1).min() < 100 or any(((np.array(e) - p) ** 2).sum() < 100 for e in extra):
                    continue
                if ((base - p) ** 2).sum(axis=1).min() == 0 or codes_at(p[None, :])[0][0] == S.CREATED:
                    continue
                found = (p, x)
                break
            if found:
                break
        assert found is not None, d2
        extra.append(found[0]); hosts.append(found[1])
    cand = np.concatenate([base, np.array(extra)]).astype(np.int32)
    return dict(name="neighbours", kind="neighbours", n=len(cand), cand=cand, targets=(0, 1), limit=1 << 30, hosts=np.array(hosts), first_extra=len(base),
                meas_root=np.zeros((0, 2)), meas_level=np.zeros(0, dtype=np.int32))


def commit_cases(base, codes, codes_at):
    """every case of section 2.  codes_at(positions) -> (n_targets x n) codes of arbitrary positions alone (for the hand-made neighbours)"""
    return limit_cases(base, codes) + survivor_cases(base, codes) + dead_cases(base, codes) + [neighbour_case(base, codes, codes_at)]


def case_codes(case, base, codes, codes_at):
    """the codes table of a case's own list: (len(targets) x n)"""
    js = list(case["targets"])
    if "index" in case:
        return codes[js][:, case["index"]]
    nb = case["first_extra"]
    return np.concatenate([codes[js][:, :nb], codes_at(case["cand"][nb:])[js]], axis=1)


def check_commit_layout(case, cd):
    """Asserts, from the nLimit loop over the codes table cd of the case's list, that the case's limit falls where its name says."""
    per, outcome, keep = limit_model(case["cand"], SEAM_LEVEL, cd, case["limit"], case["meas_root"], case["meas_level"])
    n, kind = case["n"], case["kind"]
    t0 = per[0]
    last_tried = int(np.nonzero(t0["tried"])[0][-1]) if t0["tried"].any() else -1
    if kind in ("c0-1", "c0", "c0+1", "total", "total+1", "one", "zero", "minus3"):
        made0 = np.nonzero(cd[0] == S.CREATED)[0]
        assert n < COMMIT_NT or cd[0][COMMIT_NT - 1] == S.CREATED          # a creation on either side of the seam
        assert n <= COMMIT_NT or cd[0][COMMIT_NT] == S.CREATED
        assert case["c0"] == (made0 < COMMIT_NT).sum() and case["c0"] > 2
        if kind == "c0":                       # the limit is reached on the last creation of chunk 0, the chunk's last candidate
            assert last_tried == made0[made0 < COMMIT_NT][-1] and (n < COMMIT_NT or last_tried == COMMIT_NT - 1) and t0["made"].sum() == case["c0"]
            assert n <= COMMIT_NT or (outcome[0][COMMIT_NT:] == S.PAST_LIMIT).all()
        elif kind == "c0+1" and n > COMMIT_NT:  # ... on the first creation of chunk 1, its first candidate
            assert last_tried == COMMIT_NT and t0["made"].sum() == case["c0"] + 1
        elif kind == "c0+1":                   # no chunk 1: target 0 never reaches the limit, target 1's first creation does
            assert last_tried == n - 1 and per[1]["made"].sum() == 1
        elif kind == "c0-1":
            assert last_tried < COMMIT_NT - 1 and t0["made"].sum() == case["c0"] - 1
        elif kind == "total":                  # reached on the very last creation: nothing that would create is left untried
            assert sum(p["made"].sum() for p in per) == case["total"]
        elif kind == "total+1":
            assert sum(p["made"].sum() for p in per) == case["total"] and not (outcome == S.PAST_LIMIT).any()
        elif kind == "one":
            assert t0["made"].sum() == 1 and all(p["tried"].sum() == 1 for p in per[1:])
        else:                                  # limit <= 0: the loop is left after the first candidate of every target
            assert all(p["tried"].sum() == 1 and p["tried"][p["first"]] for p in per)
        if kind in ("c0", "c0-1", "one") or (kind == "c0+1" and n > COMMIT_NT):
            assert per[1]["base"] >= case["limit"] and per[1]["tried"].sum() == 1
    elif kind == "survivor":
        assert not per[0]["alive"][:COMMIT_NT].any() and per[0]["first"] == COMMIT_NT
        assert per[0]["made"].sum() == 2 and not per[0]["made"][COMMIT_NT]
        t1 = per[1]
        assert t1["base"] >= case["limit"] and t1["first"] == COMMIT_NT and t1["tried"].sum() == 1
        assert bool(t1["made"][COMMIT_NT]) == case["creates"]
        assert (outcome[1][COMMIT_NT + 1:] != S.THINNED).sum() > 10          # there is something to refuse
    elif kind == "dead":
        for j, p in enumerate(per):
            if j >= case["dead_from"]:
                assert not p["alive"].any() and p["first"] == -1 and not p["made"].any()
        if case["dead_from"] == 1:
            assert per[0]["made"].all() and n > COMMIT_NT
    elif kind == "neighbours":
        e = case["first_extra"]
        assert (outcome[0][e:] != S.THINNED).all() and (outcome[0][e:] != S.CREATED).all()
        assert list(outcome[1][e:] == S.THINNED) == [True, True, False, False]
        d2 = ((case["cand"][e:] - case["hosts"]) ** 2).sum(axis=1)
        assert tuple(d2) == NEIGHBOUR_D2
    else:
        raise AssertionError(kind)
    # PAST_LIMIT on exactly the live, untried candidates and THINNED on exactly ~alive
    for j, p in enumerate(per):
        assert np.array_equal(outcome[j] == S.THINNED, ~p["alive"]) and np.array_equal(outcome[j] == S.PAST_LIMIT, p["alive"] & ~p["tried"])
    return per, outcome, keep
