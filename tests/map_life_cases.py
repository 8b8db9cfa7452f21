"""Seeded shapes for the tests of the map's beginning, rescale and re-alignment (mcptam_amd/csrc/map_life.h): rigs, candidate lists whose seams sit
where stated, busy positions at chosen distances, and maps as flat arrays for the transform.  Shared by tests/test_map_life_cpu.py and
tests/test_map_life_gpu.py; tests/cpp/map_life_host_check.cpp walks shapes of its own under the sanitizers."""
import numpy as np

from mcptam_amd import map_graph as mg
from mcptam_amd import stereo as S
from mcptam_amd.synth import so3_exp
from mcptam_amd.synth_img import DEFAULT_CAM_PARAMS
from mcptam_amd.taylor_camera import TaylorCamera

SIZE = (640, 480)
ROW_SIZES = (0, 1, 255, 256, 257)             # the workgroup seams of the row pass (map_graph.LIFE_BLOCK rows per workgroup)
LIMITS_AT_THE_EDGE = (255, 256, 257)          # the cut inside and at a 256-lane workgroup edge, with 600 candidates
assert mg.LIFE_BLOCK == 256


def cameras():
    """the rig's two cameras: the scene's, and one with another centre and polynomial"""
    p = DEFAULT_CAM_PARAMS
    return [TaylorCamera(p[:4] + (SIZE[0] / 2.0, SIZE[1] / 2.0) + p[6:], SIZE, SIZE, SIZE),
            TaylorCamera((245.0, -0.0011, 1.2e-07, -1.1e-10, SIZE[0] / 2.0 + 3.5, SIZE[1] / 2.0 - 2.25) + p[6:], SIZE, SIZE, SIZE)]


def rig():
    """cam_from_base of the two cameras (2 x 12): neither is the identity"""
    R = np.stack([so3_exp(np.array([0.01, -0.02, 0.015])), so3_exp(np.array([-0.3, 0.8, 0.1]))])
    return mg.poses12(R, np.array([[0.02, -0.01, 0.03], [0.11, 0.02, -0.04]]))


def mkf_poses(n=4, seed=5):
    """base_from_world of n MKFs (n x 12): general rotations, translations without zeros"""
    rng = np.random.default_rng([seed, n])
    R = np.stack([so3_exp(rng.uniform(-0.4, 0.4, 3)) for _ in range(n)]) if n else np.zeros((0, 3, 3))
    return mg.poses12(R, rng.uniform(0.2, 1.5, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3)))


def grid_candidates(n, level, step=11, x0=6, y0=5):
    """n distinct level positions on a grid `step` apart (further than ThinCandidates' 10 px from each other), row-major"""
    w = SIZE[0] >> level
    per_row = max((w - x0 - 3) // step, 1)
    i = np.arange(n)
    c = np.stack([x0 + (i % per_row) * step, y0 + (i // per_row) * step], axis=1).astype(np.int32)
    assert n == 0 or c[:, 1].max() < (SIZE[1] >> level), "the grid leaves the level image"
    return c


def dense_candidates(n, level, seed=2):
    """n level positions anywhere in the level image (duplicates allowed): a list where the limit cuts at a chosen count"""
    rng = np.random.default_rng([seed, n, level])
    return np.stack([rng.integers(3, (SIZE[0] >> level) - 3, n), rng.integers(3, (SIZE[1] >> level) - 3, n)], axis=1).astype(np.int32)


def busy_at(cand, level, d2s, levels=None):
    """busy positions (STEREO_MEAS_DTYPE) at squared level distance d2s[j] from cand[j] (d2 = dx^2 + 0), exact level-zero positions"""
    c = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    off = np.array([[int(round(np.sqrt(d))), 0] for d in d2s], dtype=np.int64)
    for o, d in zip(off, d2s):
        assert o[0] * o[0] == d, "squared distances along one axis must be squares"
    levels = [level] * len(d2s) if levels is None else levels
    return S.make_meas(S.level_zero_pos(c[:len(d2s)] + off, level), np.asarray(levels, dtype=np.int32))


def init_cases():
    """dict(name, level, cands (per camera), limits, busy (per camera), init_depth, src_mkf, first_store).  What each is for is in its name."""
    out = []

    def case(name, level, cands, limits, busy=None, init_depth=2.0, first_store=0):
        busy = [S.make_meas(np.zeros((0, 2)), [])] * 2 if busy is None else busy
        n = sum(min(len(c), l) for c, l in zip(cands, limits))
        rng = np.random.default_rng([len(out), n])
        rows = (160 + rng.permutation(3 * n + 5)[:n + 2]).astype(np.int32)      # past a 150-row table's end, out of order, with gaps, two more than needed
        out.append(dict(name=name, level=level, cands=cands, limits=limits, busy=busy, init_depth=init_depth, src_mkf=2, first_store=first_store, rows=rows))
    g1 = grid_candidates(40, 1)
    case("zero_and_one_candidate", 1, [grid_candidates(0, 1), grid_candidates(1, 1)], [5, 5])
    case("limit_zero", 1, [g1, g1[:7]], [0, 3], first_store=17)
    case("limit_past_the_survivors", 2, [grid_candidates(30, 2), grid_candidates(12, 2)], [1000, 1 << 30])
    for lim in LIMITS_AT_THE_EDGE:
        case("n600_limit%d" % lim, 0, [dense_candidates(600, 0), dense_candidates(300, 0, seed=3)], [lim, 5], first_store=4099)
    case("level3_no_level4", 3, [grid_candidates(20, 3, step=11, x0=4, y0=4)] * 2, [20, 20],
         busy=[busy_at(grid_candidates(20, 3, step=11, x0=4, y0=4), 3, [0, 0, 0], levels=[3, 2, 0]), S.make_meas(np.zeros((0, 2)), [])], init_depth=0.75)
    # Squared distance 99 is not a sum of two integer squares, and both the busy positions (ir_rounded) and the candidates are integers, so the
    # values on both sides of the rule `< 100` that exist are used: 98 = 49 + 49 and 97 = 81 + 16 (thinned), 100 = 100 + 0 = 36 + 64 (kept).
    c = grid_candidates(6, 1, step=40)
    b = S.make_meas(S.level_zero_pos(c[:5] + np.array([[7, 7], [10, 0], [0, 0], [6, 8], [9, 4]]), 1), np.array([1, 2, 3, 1, 2], dtype=np.int32))      # (level 3 is not looked at)
    b2 = S.make_meas(S.level_zero_pos(c[:2] + np.array([[-7, -7], [-8, 6]]), 1), np.array([2, 1], dtype=np.int32))
    case("busy_at_the_radius", 1, [c, c], [6, 6], busy=[b, b2], init_depth=3.5)
    out[-1]["expect_keep"] = [np.array([0, 1, 1, 1, 0, 1], dtype=bool), np.array([0, 1, 1, 1, 1, 1], dtype=bool)]
    return out


def map_arrays(n_rows, n_mkfs=4, seed=3, absent=(), bad_mkfs=(), no_rays=(), never_written=(), fixed=(), point_rows=None):
    """A map as the flat arrays map_transform_ref takes: a 2-camera rig, n_mkfs slots (`absent` ones not present, `bad_mkfs` present and bad),
    n_rows rows with rays and pixel vectors, coordinates without zeros; rows in `no_rays` have none, rows in `never_written` read as rows the
    graph never saw (-1, 0, GP_BAD), rows in `fixed` are fixed points with a source.  point_rows: how many rows the graph's columns cover."""
    rng = np.random.default_rng([seed, n_rows, n_mkfs])
    flags = np.full(n_mkfs, mg.MKF_PRESENT, dtype=np.int32)
    flags[list(absent)] = 0
    flags[list(bad_mkfs)] |= mg.MKF_BAD
    pres = np.flatnonzero(flags & mg.MKF_PRESENT)
    nz = lambda *shape: rng.uniform(0.3, 4.0, shape) * rng.choice([-1.0, 1.0], shape)      # noqa: E731
    rays = nz(n_rows, 9)
    rays[:, [2, 5, 8]] = np.abs(rays[:, [2, 5, 8]]) + 1.0                      # (the patch rays look forward)
    rays /= np.repeat(np.sqrt((rays.reshape(n_rows, 3, 3) ** 2).sum(axis=2)), 3, axis=1)
    a = dict(ncam=2, cam_from_base=rig(), base_from_world=mkf_poses(n_mkfs), mkf_flags=flags, kf_active=np.ones((n_mkfs, 2), dtype=np.uint8),
             kf_depth_mean=np.full((n_mkfs, 2), 5.0), world_pos=nz(n_rows, 3), pixel_right_w=nz(n_rows, 3) * 1e-2, pixel_down_w=nz(n_rows, 3) * 1e-2,
             rays=rays, has_rays=np.ones(n_rows, dtype=np.uint8),
             src_mkf=(pres[rng.integers(0, len(pres), n_rows)] if len(pres) else np.zeros(n_rows)).astype(np.int32),      # (no present slot: every row names an absent one)
             src_cam=rng.integers(0, 2, n_rows).astype(np.int32), pt_flags=np.zeros(n_rows, dtype=np.int32))
    a["has_rays"][list(no_rays)] = 0
    a["pt_flags"][list(fixed)] = mg.GP_FIXED
    nw = list(never_written)
    a["src_mkf"][nw], a["src_cam"][nw], a["pt_flags"][nw] = -1, 0, mg.GP_BAD
    if point_rows is not None:
        for k in ("src_mkf", "src_cam", "pt_flags"):
            a[k] = a[k][:point_rows]
    return a


def transform_cases():
    out = []
    for n in ROW_SIZES:
        out.append(dict(name="rows%d" % n, a=map_arrays(n)))
    out.append(dict(name="mixed", a=map_arrays(150, n_mkfs=5, absent=(2,), bad_mkfs=(3,), no_rays=(4, 77), never_written=(9, 149), fixed=(11,))))
    out[-1]["a"]["src_mkf"][20] = 2                            # a row whose column names the slot that is not present: no source
    out.append(dict(name="columns_shorter_than_the_table", a=map_arrays(40, point_rows=25)))
    out.append(dict(name="no_present_slot", a=map_arrays(10, n_mkfs=2, absent=(0, 1))))
    return out


def general_motion(seed=1):
    rng = np.random.default_rng([seed, 99])
    return so3_exp(rng.uniform(-0.7, 0.7, 3)), rng.uniform(-2.0, 2.0, 3)


def rel_close(got, want, tol=1e-12):
    """norm-relative difference per vector (last axis) at most tol"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    if got.size == 0:
        return True
    d = np.linalg.norm(got - want, axis=-1)
    return bool((d <= tol * np.linalg.norm(want, axis=-1)).all())
