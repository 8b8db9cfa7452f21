"""Shaped bundle maps for the seam tests of the linearisation, Schur and assembly kernels (test_ba_shapes_cpu.py,
test_ba_shapes_gpu.py).

`synth.make_problem` draws maps like the ones MCPTAM adjusts: a point sees 3 to 8 poses, a rig has up to 4 cameras, a point
has 4, 6 or 8 measurements.  The kernels branch on exactly those numbers (poses per group: 13 and 16; points per group: 16 and
64; measurements per point: the quad kernel deals them to 4 lanes; cameras: 8 live in LDS), so the maps here are built from a
per-point DESIGN instead: the keyframe and camera a point is expressed in, the (keyframe, camera) pairs that measure it, and
whether it is fixed.  `build()` turns a design into a `synth.Problem` (mode "multi"), which populates a ChainBundle and an
OracleBundle alike.

Geometry: keyframe 0 is fixed, keyframes 1.. are free; they sit on a small lattice in the plane x = 0 and look along +x at a
cloud 4 to 9 m away, every camera of the rig (a fan of a few degrees per camera) sees every point from every keyframe, so any
design is realisable.  Which free poses a point touches follows the solver's rule (a link that moves the observer chain and
the source chain together drops out, src/ChainBundle.cc MoveTogether): the free keyframes that measure it other than its own
source keyframe, plus the source keyframe if it is free and anybody else measures the point.
"""
import dataclasses
import math
from dataclasses import dataclass, field

import numpy as np

from mcptam_amd import synth
from mcptam_amd.taylor_camera import TaylorCamera

MEAS_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9)
POINT_SEAMS = (1, 15, 16, 17, 63, 64, 65, 129)
POSE_SEAMS = (1, 2, 12, 13, 14, 16)
BATCH_LAMBDAS = (1e-3, 1e-2, 1.0, 100.0)


@dataclass
class PointDesign:
    src: tuple                       # (keyframe, camera) the point is expressed in (ignored for a fixed point: world chain)
    obs: list                        # [(keyframe, camera)] one entry per measurement (a pair may repeat: two features)
    fixed: bool = False


@dataclass
class MapDesign:
    name: str
    n_mkf: int                       # keyframes, keyframe 0 fixed
    n_cams: int
    points: list = field(default_factory=list)


def design_poses(d, pt):
    """The free keyframes point design `pt` touches (the solver's `poses of a point`)."""
    src = None if pt.fixed else pt.src[0]
    others = [k for k, _ in pt.obs if k != src]
    s = {k for k in others if k > 0}
    if src is not None and src > 0 and others:
        s.add(src)
    return s


def problem_poses(p, i):
    """The same set, recomputed from the arrays of a built Problem (point index i)."""
    ms = np.flatnonzero(p.ms_pt == i)
    src = None if p.pt_fixed[i] else int(p.pt_src[i, 0])
    others = [int(k) for k in p.ms_mkf[ms] if int(k) != src]
    s = {k for k in others if not p.base_fixed[k]}
    if src is not None and not p.base_fixed[src] and others:
        s.add(src)
    return s


def _rig(n_cams):
    """Cameras looking along the base's +x, fanned 5 degrees apart, on lever arms of ~0.1 m."""
    R0 = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    Rs, ts = [], []
    for c in range(n_cams):
        yaw = math.radians(5.0) * (c - 0.5 * (n_cams - 1))
        R = R0 @ synth.rot_z(-yaw)
        a = 2 * math.pi * c / max(n_cams, 1)
        pos = np.array([0.02 * c, 0.1 * math.cos(a), 0.1 * math.sin(a)])
        Rs.append(R)
        ts.append(-R @ pos)
    return np.array(Rs), np.array(ts)


def build(d, seed=7):
    """MapDesign -> synth.Problem (measurements keyframe-major, then camera, then point, as the adapters add them)."""
    rng = np.random.default_rng([20261019, seed, len(d.points), d.n_mkf, d.n_cams])
    cam = TaylorCamera(synth.DEFAULT_CAM_PARAMS, (640, 480), (640, 480), (640, 480))
    cam_R, cam_t = _rig(d.n_cams)
    K, N = d.n_mkf, len(d.points)
    side = int(math.ceil(math.sqrt(K)))
    centres = np.array([[0.05 * math.sin(1.3 * k), 0.3 * (k % side - 0.5 * (side - 1)), 0.25 * (k // side - 0.5 * (side - 1))] for k in range(K)])
    tR = np.array([(synth.rot_z(0.04 * math.sin(2.1 * k)) @ synth.so3_exp([0.0, 0.03 * math.cos(1.7 * k), 0.0])).T for k in range(K)])
    tt = np.array([-tR[k] @ centres[k] for k in range(K)])
    world = np.stack([rng.uniform(4.0, 9.0, N), rng.uniform(-2.0, 2.0, N), rng.uniform(-1.5, 1.5, N)], axis=1)

    def cam_frame(k, c, X):
        return cam_R[c] @ (tR[k] @ X + tt[k]) + cam_t[c]

    obs = [(k, c, i) for i, pt in enumerate(d.points) for k, c in pt.obs]
    order = sorted(range(len(obs)), key=lambda j: obs[j])          # stable: repeated (keyframe, camera, point) keep their order
    obs = [obs[j] for j in order]
    M = len(obs)
    ms_mkf = np.array([o[0] for o in obs], dtype=np.int32)
    ms_cam = np.array([o[1] for o in obs], dtype=np.int32)
    ms_pt = np.array([o[2] for o in obs], dtype=np.int32)
    uv = np.zeros((M, 2))
    for j, (k, c, i) in enumerate(obs):
        p2, inv = cam.project(cam_frame(k, c, world[i])[None, :])
        assert not inv[0], "design not realisable: point %d is not seen from keyframe %d camera %d" % (i, k, c)
        uv[j] = p2[0]
    ms_level = rng.choice(4, size=M, p=[0.55, 0.25, 0.15, 0.05]).astype(np.int32)
    uv = uv + rng.normal(size=(M, 2)) * (0.5 * (2.0 ** ms_level))[:, None]
    n_out = M // 40                                                  # 2.5 % gross outliers: robust weights of every size
    if n_out:
        oi = rng.choice(M, n_out, replace=False)
        uv[oi] = rng.uniform([0, 0], (640, 480), size=(n_out, 2))
    base_R, base_t = tR.copy(), tt.copy()
    base_fixed = np.zeros(K, dtype=bool)
    base_fixed[0] = True
    for k in range(1, K):
        R, t = synth.se3_exp(np.concatenate([rng.normal(size=3) * 0.02, rng.normal(size=3) * math.radians(0.5)]))
        base_R[k], base_t[k] = R @ tR[k], R @ tt[k] + t
    pt_fixed = np.array([pt.fixed for pt in d.points], dtype=bool)
    pt_src = np.array([pt.src for pt in d.points], dtype=np.int32).reshape(N, 2)
    pt_x = np.array([cam_frame(int(pt_src[i, 0]), int(pt_src[i, 1]), world[i]) for i in range(N)]).reshape(N, 3)
    pt_x = pt_x * (1.0 + rng.normal(size=(N, 1)) * 0.05)
    pt_x[pt_fixed] = world[pt_fixed]
    p = synth.Problem(cams=[cam] * d.n_cams, mode="multi", n_mkf=K, base_R=base_R, base_t=base_t, base_fixed=base_fixed,
                      cam_R=cam_R, cam_t=cam_t, pt_x=pt_x, pt_src=pt_src, pt_fixed=pt_fixed, ms_mkf=ms_mkf, ms_cam=ms_cam,
                      ms_pt=ms_pt, ms_uv=np.ascontiguousarray(uv), ms_level=ms_level, true_base_R=tR, true_base_t=tt, true_world=world)
    p.design = d
    return p


def permuted(p, seed=3):
    """The same map with its measurements handed over in another order (the reference's own rounding floor: same sums,
    other order)."""
    perm = np.random.default_rng([99, seed]).permutation(p.n_meas)
    q = dataclasses.replace(p, ms_mkf=p.ms_mkf[perm], ms_cam=p.ms_cam[perm], ms_pt=p.ms_pt[perm],
                            ms_uv=np.ascontiguousarray(p.ms_uv[perm]), ms_level=p.ms_level[perm], ids={})
    return q


# ---------------------------------------------------------------------------------------------------------------------
# designs

def shared_design(name, n_points, k, n_cams=2):
    """Every point touches the same k free keyframes (1..k): groups close on the point count alone.  Points with an even
    index are expressed in the fixed keyframe, points with an odd index in one of the k free ones (its own measurement from
    there has no free slot); k = 1 has only the first kind (a point expressed in its only observer touches no pose)."""
    d = MapDesign(name, k + 1, n_cams)
    for i in range(n_points):
        free_src = (i % 2 == 1) and k >= 2
        src = (1 + (i // 2) % k, i % n_cams) if free_src else (0, 0)
        obs = [(1 + j, (i + j) % n_cams) for j in range(k)]
        if not free_src and i % 4 == 0:
            obs.append((0, (i // 4) % n_cams))            # the fixed keyframe measures it too: a measurement without a free slot
        d.points.append(PointDesign(src, obs))
    return d


def rolling_design(name, n_points, k, n_poses):
    """Point i touches the free keyframes {i mod P, ..., + k - 1} (mod P): groups close on the pose budget."""
    d = MapDesign(name, n_poses + 1, 2)
    for i in range(n_points):
        obs = [(1 + (i % n_poses + j) % n_poses, (i + j) % 2) for j in range(k)]
        obs.append((0, i % 2))
        d.points.append(PointDesign((0, 0), obs))
    return d


def big_design(name, pattern):
    """pattern: per point 17 (all 17 free keyframes: more than a group holds, the generic path) or 6 (the first six)."""
    d = MapDesign(name, 18, 2)
    for i, k in enumerate(pattern):
        obs = [(1 + j, (i + j) % 2) for j in range(k)] + [(0, i % 2)]
        d.points.append(PointDesign((1 + i % 6, 0), obs))          # expressed in one of the first six: the solver orders points by that pose, so the two kinds stay mixed
    return d


MEAS_KINDS = ("regular_fixed_src", "regular_free_src", "own_source_only", "fixed_keyframe_only", "fixed_point", "fixed_point_fixed_only")


def meas_design(name="meas", n_cams=3, n_free=6):
    """Measurement counts 1, 2, 3, 4, 5, 7, 8, 9 for each of six kinds of point (point i: count MEAS_COUNTS[i % 8], kind
    MEAS_KINDS[(i // 8) % 6]; two rounds of the 48 combinations)."""
    d = MapDesign(name, n_free + 1, n_cams)
    for i in range(96):
        n, kind = MEAS_COUNTS[i % 8], MEAS_KINDS[(i // 8) % 6]
        ring = [(1 + (i + j) % n_free, (j // n_free + i) % n_cams) for j in range(n)]
        if kind == "regular_fixed_src":
            pt = PointDesign((0, 0), ring)
        elif kind == "regular_free_src":            # expressed in a free keyframe, whose own measurement (no free slot) comes first
            s = 1 + i % n_free
            pt = PointDesign((s, i % n_cams), [(s, i % n_cams)] + [(k if k != s else 1 + s % n_free, c) for k, c in ring[:n - 1]])
        elif kind == "own_source_only":             # V and g, no incidence
            s = 1 + i % n_free
            pt = PointDesign((s, 0), [(s, j % n_cams) for j in range(n)])
        elif kind == "fixed_keyframe_only":
            pt = PointDesign((0, 0), [(0, j % n_cams) for j in range(n)])
        elif kind == "fixed_point":
            pt = PointDesign((0, 0), ring, fixed=True)
        else:
            pt = PointDesign((0, 0), [(0, j % n_cams) for j in range(n)], fixed=True)
        d.points.append(pt)
    return d


def tencam_design(name="tencam", n_points=40, k=6):
    d = MapDesign(name, k + 1, 10)
    for i in range(n_points):
        src = (1 + i % k, (3 * i) % 10) if i % 2 else (0, i % 10)
        obs = [(1 + j, (i + 3 * j) % 10) for j in range(k)] + [(0, (i + 7) % 10)]
        d.points.append(PointDesign(src, obs))
    return d


def calib_cut(n_points):
    """The `calib` map (free relative camera poses as the second link of every chain of that camera: one pose vertex at two
    positions of an edge; fixed board points on a world chain) cut to n_points points: for every keyframe and for every camera the
    first point measured from it, two fixed points, then the points of lowest index."""
    p = synth.make_config("calib")
    keep = []

    def take(i):
        if i not in keep:
            keep.append(int(i))
    for k in range(p.n_mkf):
        take(p.ms_pt[p.ms_mkf == k].min())
    for c in range(len(p.cams)):
        take(p.ms_pt[p.ms_cam == c].min())
    for i in np.flatnonzero(p.pt_fixed)[:2]:
        take(i)
    for i in range(p.n_points):
        if len(keep) >= n_points:
            break
        take(i)
    assert len(keep) == n_points
    keep = np.sort(np.array(keep))
    pmap = -np.ones(p.n_points, dtype=np.int64)
    pmap[keep] = np.arange(n_points)
    ms = pmap[p.ms_pt] >= 0
    q = dataclasses.replace(p, pt_x=p.pt_x[keep].copy(), pt_src=p.pt_src[keep].copy(), pt_fixed=p.pt_fixed[keep].copy(),
                            ms_mkf=p.ms_mkf[ms].copy(), ms_cam=p.ms_cam[ms].copy(), ms_pt=pmap[p.ms_pt[ms]].astype(p.ms_pt.dtype),
                            ms_uv=p.ms_uv[ms].copy(), ms_level=p.ms_level[ms].copy(), true_world=p.true_world[keep], ids={})
    q.design = None
    return q


CHAIN_SEAMS = (64, 65, 128, 129)      # pose chains of a map against the 64 chains a chain workgroup of the one-launch trial step takes
POSE_COUNT_SEAMS = (255, 256, 257)     # poses of a map against the 256 poses such a workgroup keeps in LDS


def chain_design(name, n_chains):
    """A map with exactly n_chains pose chains: every (keyframe, camera) pair of n_chains // 2 keyframes with two cameras is a chain
    (pair j = keyframe j // 2, camera j % 2; point j is measured from pairs j, j + 21 and j + 42, so every pair measures three
    points), and for an odd count one fixed point, which brings the world chain."""
    pairs = n_chains // 2 * 2
    d = MapDesign(name, pairs // 2, 2)
    for j in range(pairs):
        d.points.append(PointDesign((0, 0), [(((j + 21 * m) % pairs) // 2, ((j + 21 * m) % pairs) % 2) for m in range(3)]))
    if n_chains % 2:
        d.points.append(PointDesign((0, 0), [(1, 0), (2, 1), (3, 0)], fixed=True))
    return d


def pose_count_design(name, n_poses):
    """A map with exactly n_poses poses: n_poses - 1 keyframes (keyframe 0 fixed) and the pose of the one camera.  128 points in
    the fixed keyframe's frame; keyframe k measures points k + 0, 7, 29, 53, 71 and 101 (mod 128): every free keyframe has a pose
    block that six measurements determine, and a point touches 12 poses at most."""
    d = MapDesign(name, n_poses - 1, 1)
    obs = [[] for _ in range(128)]
    for k in range(n_poses - 1):
        for off in (0, 7, 29, 53, 71, 101):
            obs[(k + off) % 128].append((k, 0))
    for i in range(128):
        d.points.append(PointDesign((0, 0), obs[i]))
    return d


# ---------------------------------------------------------------------------------------------------------------------
# the committed maps, by name (built once per process)

def _designs():
    out = {}
    for n in POINT_SEAMS:
        out["pts%d" % n] = lambda n=n: shared_design("pts%d" % n, n, 6)
    for k in POSE_SEAMS:
        out["shared%d_66" % k] = lambda k=k: shared_design("shared%d_66" % k, 66, k)
        out["shared%d_130" % k] = lambda k=k: shared_design("shared%d_130" % k, 130, k)
    for k in (5, 13):
        out["roll%d" % k] = lambda k=k: rolling_design("roll%d" % k, 66, k, 66)
    out["big_all"] = lambda: big_design("big_all", [17] * 20)
    out["big_mixed"] = lambda: big_design("big_mixed", [17 if i % 2 else 6 for i in range(40)])
    out["big_one"] = lambda: big_design("big_one", [17 if i == 10 else 6 for i in range(33)])
    out["meas"] = meas_design
    out["tencam"] = tencam_design
    return out


DESIGNS = _designs()
MAP_NAMES = tuple(DESIGNS) + ("calib17", "calib65")
# the maps of the trial-step tests (ba_trial_cases.py): kept out of MAP_NAMES, the pose-count maps have 1500 pose unknowns
TRIAL_DESIGNS = dict([("chains%d" % n, lambda n=n: chain_design("chains%d" % n, n)) for n in CHAIN_SEAMS] +
                     [("poses%d" % n, lambda n=n: pose_count_design("poses%d" % n, n)) for n in POSE_COUNT_SEAMS])
_MAPS = {}


def get_map(name):
    """The committed map `name` (a synth.Problem; `.design` is its MapDesign, None for the cut calibration maps)."""
    if name not in _MAPS:
        _MAPS[name] = calib_cut(int(name[5:])) if name.startswith("calib") else build((DESIGNS.get(name) or TRIAL_DESIGNS[name])())
    return _MAPS[name]


def block_scaled_error(S, S_ref):
    """max over the lower triangle of |S - S_ref| / sqrt(max|S_ref,aa| max|S_ref,bb|), a and b the 6 x 6 pose blocks of the entry."""
    n = S_ref.shape[0]
    assert n % 6 == 0 and S.shape == S_ref.shape
    d = np.array([np.abs(S_ref[6 * a:6 * a + 6, 6 * a:6 * a + 6]).max() for a in range(n // 6)])
    scale = np.kron(np.sqrt(np.outer(d, d)), np.ones((6, 6)))
    low = np.tril(np.ones((n, n), dtype=bool))
    assert (scale[low] > 0).all()
    return float((np.abs(S - S_ref)[low] / scale[low]).max()) if n else 0.0


def rel_err_2(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))
