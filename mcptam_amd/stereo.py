"""MapMakerServerBase::AddStereoMapPoints of one source keyframe and level on the GPU (include/mcp_img.h mcp_stereo_points), its hypothesis
export (mcp_stereo_hypotheses), and numpy restatements of the pieces the device runs -- ThinCandidates, the epipolar arc, the ambiguity rules,
ReprojectPoint -- with which the tests compose the same result from existing calls.  src/MapMakerServerBase.cc:123-143, 411-496, 604-918.

stereo_map_points (mcp_stereo_map_points) is the form whose created points stay on the device, in the rows of a MapPointTable and the store of its
MapGraph; stereo_busy_host / stereo_append_host are its two host twins (no device) and stereo_busy_ref / stereo_append_ref the numpy restatements
of the busy list it gathers from the store and of what a created point becomes in the map (:855-914)."""
import ctypes
import math

import numpy as np

from . import chain_bundle as _cb
from . import keyframe as K

THINNED, NO_ARC, NO_MATCH, TOO_MANY, INDEX_FAR, NO_SUBPIX, CREATED, PAST_LIMIT = range(1, 9)
OUTCOME_NAMES = {THINNED: "THINNED", NO_ARC: "NO_ARC", NO_MATCH: "NO_MATCH", TOO_MANY: "TOO_MANY", INDEX_FAR: "INDEX_FAR", NO_SUBPIX: "NO_SUBPIX",
                 CREATED: "CREATED", PAST_LIMIT: "PAST_LIMIT"}
STEREO_SYMBOLS = ["mcp_stereo_points", "mcp_stereo_hypotheses", "mcp_stereo_map_points", "mcp_stereo_busy_host", "mcp_stereo_append_host",
                  "mcp_map_points_get_rays", "mcp_map_points_get_source", "mcp_map_gp_get"]
SRC_ROOT, SRC_EPIPOLAR = 2, 4                 # Measurement::eSource of a created point's two measurements (include/mcp_img.h MCP_SRC_*)
BUSY_BLOCK = 256                              # stereo_append.h: store entries of a workgroup of the busy gather


class StereoMapParams(ctypes.Structure):
    _fields_ = [("src_mkf", ctypes.c_int), ("src_cam", ctypes.c_int), ("limit", ctypes.c_int), ("busy_from_store", ctypes.c_int)]


class StereoMapResult(ctypes.Structure):
    _fields_ = [("made", ctypes.c_int), ("first_store", ctypes.c_int), ("n_busy", ctypes.c_int)]

    def as_dict(self):
        return dict(made=self.made, first_store=self.first_store, n_busy=self.n_busy)


class StereoTarget(ctypes.Structure):
    _fields_ = [("kf", ctypes.c_void_p), ("cam", ctypes.c_void_p), ("cam_from_world", ctypes.c_double * 12), ("one_pixel_angle", ctypes.c_double)]


class StereoMeas(ctypes.Structure):
    _fields_ = [("root_pos", ctypes.c_double * 2), ("level", ctypes.c_int), ("pad_", ctypes.c_int)]


class StereoPoint(ctypes.Structure):
    _fields_ = [("candidate", ctypes.c_int), ("target", ctypes.c_int), ("hypothesis", ctypes.c_int), ("score", ctypes.c_int),
                ("world_pos", ctypes.c_double * 3), ("root_pos", ctypes.c_double * 2), ("target_pos", ctypes.c_double * 2),
                ("center_nc", ctypes.c_double * 3), ("one_right_nc", ctypes.c_double * 3), ("one_down_nc", ctypes.c_double * 3),
                ("pixel_right_w", ctypes.c_double * 3), ("pixel_down_w", ctypes.c_double * 3)]


STEREO_POINT_DTYPE = np.dtype([("candidate", "i4"), ("target", "i4"), ("hypothesis", "i4"), ("score", "i4"), ("world_pos", "f8", 3),
                               ("root_pos", "f8", 2), ("target_pos", "f8", 2), ("center_nc", "f8", 3), ("one_right_nc", "f8", 3),
                               ("one_down_nc", "f8", 3), ("pixel_right_w", "f8", 3), ("pixel_down_w", "f8", 3)], align=True)
STEREO_MEAS_DTYPE = np.dtype([("root_pos", "f8", 2), ("level", "i4"), ("pad_", "i4")], align=True)
TD_IN_DTYPE = np.dtype([("world_pos", "f8", 3), ("pixel_right_w", "f8", 3), ("pixel_down_w", "f8", 3), ("source_kf", "u8"), ("source_level", "i4"),
                        ("center_x", "i4"), ("center_y", "i4"), ("fixed", "i4")], align=True)
assert STEREO_POINT_DTYPE.itemsize == ctypes.sizeof(StereoPoint)
assert STEREO_MEAS_DTYPE.itemsize == ctypes.sizeof(StereoMeas)
assert TD_IN_DTYPE.itemsize == ctypes.sizeof(K.TdIn)
_BOUND = False


def lib():
    global _BOUND
    L = K.lib()
    if not _BOUND:
        vp, ip = ctypes.c_void_p, ctypes.c_int
        L.mcp_stereo_points.argtypes = [vp, vp, vp, ip, ip, vp, ip, vp, ip, vp, ip, ip, vp, vp, vp]
        L.mcp_stereo_points.restype = ip
        L.mcp_stereo_hypotheses.argtypes = [vp, vp, vp, ip, ip, vp, vp, ip, vp, vp]
        L.mcp_stereo_hypotheses.restype = ip
        L.mcp_stereo_map_points.argtypes = [vp, vp, vp, vp, ip, ip, vp, ip, vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp]
        L.mcp_stereo_busy_host.argtypes = [ip, vp, ip, ip, ip, vp]
        L.mcp_stereo_append_host.argtypes = [ip, vp, vp, ip, ip, ip, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.mcp_map_points_get_rays.argtypes = [vp, ip, ip, vp, vp]
        L.mcp_map_points_get_source.argtypes = [vp, ip, ip, vp, vp, vp, vp, vp]
        L.mcp_map_gp_get.argtypes = [vp, ip, ip, vp, vp, vp]
        for n in STEREO_SYMBOLS[2:]:
            getattr(L, n).restype = ip
        _BOUND = True
    return L


def _pose12(pose):
    R, t = pose
    return np.ascontiguousarray(np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)]))


def _targets(targets):
    """targets: list of (keyframe, camera, CamFromWorld (R, t)[, one_pixel_angle]) -> ctypes table + keep-alive"""
    cams = [t[1].to_struct() for t in targets]
    tab = (StereoTarget * max(len(targets), 1))()
    for i, t in enumerate(targets):
        tab[i].kf = t[0]._h if t[0] is not None else None
        tab[i].cam = ctypes.addressof(cams[i])
        p = _pose12(t[2])
        for k in range(12):
            tab[i].cam_from_world[k] = p[k]
        tab[i].one_pixel_angle = float(t[3]) if len(t) > 3 else t[1].one_pixel_angle()
    return tab, cams


def _cand(cand):
    return np.ascontiguousarray(np.asarray(cand, dtype=np.int32).reshape(-1, 2))


def make_meas(root_pos, levels):
    m = np.zeros(len(levels), dtype=STEREO_MEAS_DTYPE)
    m["root_pos"] = np.asarray(root_pos, dtype=np.float64).reshape(-1, 2)
    m["level"] = levels
    return m


def stereo_points(src, src_cam, src_pose, level, cand, targets, limit=1 << 30, meas=None, outcomes=True, cap=None):
    """mcp_stereo_points.  Returns (points: STEREO_POINT_DTYPE array in creation order, keep mask (bool, n_cand), outcome (n_targets x n_cand uint8 or
    None))."""
    L = lib()
    c = _cand(cand)
    n = len(c)
    meas = make_meas(np.zeros((0, 2)), []) if meas is None else meas
    tab, keep_cams = _targets(targets)
    cs = src_cam.to_struct()
    sp = _pose12(src_pose)
    out = np.zeros(max(n, 1), dtype=STEREO_POINT_DTYPE)
    keep = np.zeros(max(n, 1), dtype=np.uint8)
    oc = np.zeros((max(len(targets), 1), max(n, 1)), dtype=np.uint8) if outcomes else None
    rc = L.mcp_stereo_points(src._h, ctypes.addressof(cs), sp.ctypes.data, int(level), n, c.ctypes.data, len(meas), meas.ctypes.data, len(targets),
                             ctypes.addressof(tab), int(limit), n if cap is None else int(cap), out.ctypes.data, keep.ctypes.data,
                             oc.ctypes.data if oc is not None else None)
    if rc < 0:
        raise RuntimeError("mcp_stereo_points failed: " + _cb.last_error())
    del keep_cams
    if oc is not None:
        oc = oc[:len(targets), :n]
    return out[:rc].copy(), keep[:n].astype(bool), oc


def stereo_hypotheses(src, src_cam, src_pose, level, cand, target):
    """mcp_stereo_hypotheses: (TD_IN_DTYPE array of every hypothesis, offsets (n_cand + 1))."""
    L = lib()
    c = _cand(cand)
    n = len(c)
    tab, keep_cams = _targets([target])
    cs = src_cam.to_struct()
    sp = _pose12(src_pose)
    off = np.zeros(n + 1, dtype=np.int32)
    tot = L.mcp_stereo_hypotheses(src._h, ctypes.addressof(cs), sp.ctypes.data, int(level), n, c.ctypes.data, ctypes.addressof(tab), 0, None, off.ctypes.data)
    if tot < 0:
        raise RuntimeError("mcp_stereo_hypotheses failed: " + _cb.last_error())
    out = np.zeros(max(tot, 1), dtype=TD_IN_DTYPE)
    if tot > 0:
        rc = L.mcp_stereo_hypotheses(src._h, ctypes.addressof(cs), sp.ctypes.data, int(level), n, c.ctypes.data, ctypes.addressof(tab), tot,
                                     out.ctypes.data, off.ctypes.data)
        if rc != tot:
            raise RuntimeError("mcp_stereo_hypotheses failed: " + _cb.last_error())
    del keep_cams
    return out[:tot], off


# ---- AddStereoMapPoints into the map (include/mcp_img.h mcp_stereo_map_points): the call, its host twins, its numpy restatements ----------------
def _store_dtype():
    from .map_graph import STORE_ENTRY_DTYPE
    return STORE_ENTRY_DTYPE


def stereo_map_points(graph, src, src_cam, src_pose, level, cand, targets, target_mkf, target_cam, rows, keys, src_mkf, src_cam_index, limit=1 << 30,
                      meas=None, busy_from_store=None, outcomes=True, want_points=True):
    """mcp_stereo_map_points: mcp_stereo_points of one source keyframe and level whose created points stay on the device -- point k (creation order)
    takes rows[k] / keys[k] of graph.table and two entries of the graph's store.  targets as for stereo_points, target_mkf / target_cam their MKF
    slots and camera indices; busy_from_store defaults to `no meas given`.  Returns (points or None, keep mask, outcome or None, dict(made,
    first_store, n_busy))."""
    L = lib()
    c = _cand(cand)
    n = len(c)
    busy_from_store = meas is None if busy_from_store is None else bool(busy_from_store)
    tab, keep_cams = _targets(targets)
    tm, tc = np.ascontiguousarray(target_mkf, dtype=np.int32), np.ascontiguousarray(target_cam, dtype=np.int32)
    r, k = np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(keys, dtype=np.int32)
    if len(tm) != len(targets) or len(tc) != len(targets) or len(r) != len(k):
        raise ValueError("stereo_map_points: lengths differ")
    cs = src_cam.to_struct()
    sp = _pose12(src_pose)
    out = np.zeros(max(n, 1), dtype=STEREO_POINT_DTYPE) if want_points else None
    keep = np.zeros(max(n, 1), dtype=np.uint8)
    oc = np.zeros((max(len(targets), 1), max(n, 1)), dtype=np.uint8) if outcomes else None
    prm, res = StereoMapParams(int(src_mkf), int(src_cam_index), int(limit), 1 if busy_from_store else 0), StereoMapResult()
    rc = L.mcp_stereo_map_points(graph._h, src._h if src is not None else None, ctypes.addressof(cs), sp.ctypes.data, int(level), n, c.ctypes.data if n else None,
                                 0 if meas is None else len(meas), None if meas is None or len(meas) == 0 else meas.ctypes.data,
                                 len(targets), ctypes.addressof(tab) if len(targets) else None, tm.ctypes.data if len(tm) else None, tc.ctypes.data if len(tc) else None,
                                 len(r), r.ctypes.data if len(r) else None, k.ctypes.data if len(k) else None, ctypes.addressof(prm), ctypes.addressof(res),
                                 out.ctypes.data if out is not None else None, keep.ctypes.data, oc.ctypes.data if oc is not None else None)
    if rc < 0:
        raise RuntimeError("mcp_stereo_map_points failed: " + _cb.last_error())
    del keep_cams
    if oc is not None:
        oc = oc[:len(targets), :n]
    return (out[:rc].copy() if out is not None else None), keep[:n].astype(bool), oc, res.as_dict()


def stereo_busy_ref(store, src_mkf, src_cam):
    """ThinCandidates' measurement list of the keyframe (src_mkf, src_cam) as the store holds it: every live entry of it, in store order, every
    level (the thinning filters).  store: STORE_ENTRY_DTYPE.  Returns STEREO_MEAS_DTYPE."""
    s = np.asarray(store, dtype=_store_dtype())
    hit = np.flatnonzero((s["alive"] != 0) & (s["mkf"] == src_mkf) & (s["cam"] == src_cam))
    out = np.zeros(len(hit), dtype=STEREO_MEAS_DTYPE)
    out["root_pos"], out["level"] = s["uv"][hit], s["level"][hit]
    return out


def stereo_busy_host(store, src_mkf, src_cam):
    """mcp_stereo_busy_host: the same list by the body the gather kernel calls, under the host compiler.  Needs no device."""
    s = np.ascontiguousarray(store, dtype=_store_dtype())
    L = lib()
    n = L.mcp_stereo_busy_host(len(s), s.ctypes.data if len(s) else None, int(src_mkf), int(src_cam), 0, None)
    if n < 0:
        raise RuntimeError("mcp_stereo_busy_host failed: " + _cb.last_error())
    out = np.zeros(max(n, 1), dtype=STEREO_MEAS_DTYPE)
    if n and L.mcp_stereo_busy_host(len(s), s.ctypes.data, int(src_mkf), int(src_cam), n, out.ctypes.data) != n:
        raise RuntimeError("mcp_stereo_busy_host failed: " + _cb.last_error())
    return out[:n]


def _append_args(pts, rows, target_mkf, target_cam):
    p = np.ascontiguousarray(pts, dtype=STEREO_POINT_DTYPE)
    r = np.ascontiguousarray(rows, dtype=np.int32)[:len(p)]
    if len(r) != len(p):
        raise ValueError("stereo_append: fewer rows than points")
    return p, r, np.ascontiguousarray(target_mkf, dtype=np.int32), np.ascontiguousarray(target_cam, dtype=np.int32)


def stereo_append_ref(pts, rows, level, src_mkf, src_cam, target_mkf, target_cam, first_store=0):
    """What created points pts (STEREO_POINT_DTYPE, creation order) become in the map (src/MapMakerServerBase.cc:855-914): per point the table's
    columns (world_pos, pixel_right_w, pixel_down_w, usable 0, counts (1, 0), rays, the source's level / centre / fixed 0), the graph's columns
    (src_mkf, src_cam, flags 0) and two store entries -- the source's SRC_ROOT, then the target's SRC_EPIPOLAR -- at first_store + 2k.  Returns a
    dict of arrays; `store_end` is the store's length afterwards."""
    p, r, tm, tc = _append_args(pts, rows, target_mkf, target_cam)
    n = len(p)
    if n and (p["target"].min() < 0 or p["target"].max() >= len(tm)):
        raise ValueError("stereo_append_ref: a record names a target outside the target tables")
    s = float(1 << level)
    ap = np.zeros(2 * n, dtype=_store_dtype())
    ap["uv"][0::2], ap["uv"][1::2] = p["root_pos"], p["target_pos"]
    ap["mkf"][0::2], ap["cam"][0::2] = src_mkf, src_cam
    ap["mkf"][1::2], ap["cam"][1::2] = tm[p["target"]], tc[p["target"]]
    ap["row"][0::2] = ap["row"][1::2] = r
    ap["level"], ap["alive"] = level, 1
    ap["source"][0::2], ap["source"][1::2] = SRC_ROOT, SRC_EPIPOLAR
    return dict(world_pos=p["world_pos"].copy(), pixel_right_w=p["pixel_right_w"].copy(), pixel_down_w=p["pixel_down_w"].copy(),
                usable=np.zeros(n, dtype=np.uint8), inlier=np.ones(n, dtype=np.int32), outlier=np.zeros(n, dtype=np.int32),
                rays=np.concatenate([p["center_nc"], p["one_right_nc"], p["one_down_nc"]], axis=1).reshape(n, 9),
                source_level=np.full(n, level, dtype=np.int32), center_xy=np.trunc((p["root_pos"] + 0.5) / s - 0.5).astype(np.int32).reshape(n, 2),
                fixed=np.zeros(n, dtype=np.uint8), gp_src_mkf=np.full(n, src_mkf, dtype=np.int32), gp_src_cam=np.full(n, src_cam, dtype=np.int32),
                gp_flags=np.zeros(n, dtype=np.int32), appended=ap, store_end=int(first_store) + 2 * n)


def stereo_append_host(pts, rows, level, src_mkf, src_cam, target_mkf, target_cam, first_store=0):
    """mcp_stereo_append_host: the body the append kernel calls, under the host compiler.  Needs no device.  Returns the arrays of
    stereo_append_ref that the call writes (the constant columns -- usable, counts, level, fixed -- are the kernel's own)."""
    p, r, tm, tc = _append_args(pts, rows, target_mkf, target_cam)
    n, m = len(p), max(len(p), 1)
    o = dict(world_pos=np.zeros((m, 3)), pixel_right_w=np.zeros((m, 3)), pixel_down_w=np.zeros((m, 3)), rays=np.zeros((m, 9)), center_xy=np.zeros((m, 2), np.int32),
             gp_src_mkf=np.zeros(m, np.int32), gp_src_cam=np.zeros(m, np.int32), gp_flags=np.zeros(m, np.int32), appended=np.zeros(2 * m, dtype=_store_dtype()))
    rc = lib().mcp_stereo_append_host(n, p.ctypes.data, r.ctypes.data, int(level), int(src_mkf), int(src_cam), tm.ctypes.data, tc.ctypes.data, int(first_store),
                                      *[o[k].ctypes.data for k in ("world_pos", "pixel_right_w", "pixel_down_w", "rays", "center_xy", "gp_src_mkf", "gp_src_cam", "gp_flags",
                                                                   "appended")])
    if rc < 0:
        raise RuntimeError("mcp_stereo_append_host failed: " + _cb.last_error())
    o = {k: (v[:2 * n] if k == "appended" else v[:n]) for k, v in o.items()}
    o["store_end"] = rc
    return o


# ---- numpy restatements (test infrastructure) ------------------------------------------------------------------------------------------------
def level_zero_pos(c, level):
    """LevelZeroPos (include/mcptam/LevelHelpers.h:61-82)"""
    return (np.asarray(c, dtype=np.float64) + 0.5) * (1 << level) - 0.5


def ir_rounded(v):
    """CVD::ir_rounded: half away from zero.  [3P-memory] restated from memory of libCVD (v > 0 ? v + 0.5 : v - 0.5, then truncated), not checked
    against its source here."""
    v = np.asarray(v, dtype=np.float64)
    return np.trunc(np.where(v > 0.0, v + 0.5, v - 0.5)).astype(np.int64)


def thin_candidates(cand, level, meas_root=(), meas_level=(), created_root=()):
    """ThinCandidates (:411-446): keep mask of the candidates (level positions) further than 10 px from every busy position -- measurements at
    level or level + 1 (v2RootPos / LevelScale, ir_rounded) and the SRC_ROOT positions of points created since (level `level`)."""
    c = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    sc = float(1 << level)
    busy = [ir_rounded(np.asarray(r, dtype=np.float64) / sc) for r, l in zip(meas_root, meas_level) if l == level or l == level + 1]
    busy += [ir_rounded(np.asarray(r, dtype=np.float64) / sc) for r in created_root]
    keep = np.ones(len(c), dtype=bool)
    for b in busy:
        d = c - b
        keep &= (d * d).sum(axis=1) >= 100
    return keep


def _unit(v):
    """TooN normalize: a zero or non-finite vector becomes NaN / inf as in C++, without a warning"""
    with np.errstate(all="ignore"):
        return v / math.sqrt(float(v @ v))


def _acos(x):
    """acos as the C library has it: NaN outside [-1, 1] and for NaN, where math.acos raises"""
    return math.acos(x) if -1.0 <= x <= 1.0 else float("nan")


def pixel_vectors(pose_src, center, right, down, world):
    """MapPoint::RefreshPixelVectors (src/MapPoint.cc:62-87), normal (0, 0, -1); world: (n, 3) -> (pixel_right_w, pixel_down_w), (n, 3) each"""
    Rs, ts = pose_src
    w = np.atleast_2d(world)
    h = np.abs(-(w @ Rs.T + ts)[:, 2])
    c = center[None, :] * h[:, None] / abs(center[2])
    r = right[None, :] * h[:, None] / abs(right[2]) - c
    d = down[None, :] * h[:, None] / abs(down[2]) - c
    return r @ Rs, d @ Rs


def probe(cam_src, level, c):
    """the probe MapPoint's root position and NC vectors (:726-738)"""
    s = 1 << level
    root = level_zero_pos(c, level)
    vs = cam_src.unproject(np.stack([root, root + [s, 0.0], root + [0.0, s]]))
    return root, _unit(vs[0]), _unit(vs[1]), _unit(vs[2])


def arc(cam_src, pose_src, pose_tgt, one_pixel_angle, level, c):
    """The hypotheses of AddPointEpipolar (:611-723) for candidate c: dict(n, world (n x 3), tc (n x 3), pixel_right_w, pixel_down_w, root,
    center, right, down); n = 0 when the v3BetweenEndpoints guard or a non-finite step count stops it.  Total: where the C++ carries NaN or inf
    (no baseline, a cosine past 1 by rounding, an end point on the target's centre) this carries it too and returns n = 0; nothing raises or warns."""
    with np.errstate(all="ignore"):
        return _arc(cam_src, pose_src, pose_tgt, one_pixel_angle, level, c)


def _arc(cam_src, pose_src, pose_tgt, one_pixel_angle, level, c):
    Rs, ts = pose_src
    Rt, tt = pose_tgt
    s = 1 << level
    nan = float("nan")
    root, cen, rig, dow = probe(cam_src, level, c)
    ray = cam_src.unproject(root)[0]
    dirn = Rt @ (Rs.T @ ray)
    cc_tc = Rt @ (-(Rs.T @ ts)) + tt
    cc_sc = Rs @ (-(Rt.T @ tt)) + ts
    sep = math.sqrt(float(cc_sc @ cc_sc))
    res = dict(n=0, world=np.zeros((0, 3)), tc=np.zeros((0, 3)), pixel_right_w=np.zeros((0, 3)), pixel_down_w=np.zeros((0, 3)), root=root,
               center=cen, right=rig, down=dow, step=0.0)
    if sep == 0.0:                    # the device divides by zero here and gets NaN all the way to the step count: no hypotheses
        return res
    src_angle = _acos(float(cc_sc @ ray) / sep)
    if math.isnan(src_angle):         # NaN all the way to the step count
        return res
    start = sep * math.sin(math.pi - src_angle - math.pi / 3) / math.sin(math.pi / 3)
    end = sep * math.sin(math.pi - src_angle - 0.05) / math.sin(0.05)
    res.update(start_raw=start)
    if start < 0.2:
        start = 0.2
    RS, RE = cc_tc + start * dirn, cc_tc + end * dirn
    a, b = _unit(RS), _unit(RE)
    res.update(start=start, end=end)
    d = a - b
    if d @ d < 1e-8:
        return res
    nrm = _unit(np.cross(a, b))
    J = np.cross(nrm, a)
    max_angle = _acos(float(a @ b) * 1 + float(J @ b) * 0)      # v2PlaneB * (1, 0) (:697): a NaN in the plane's y axis reaches the angle
    q = math.ceil(max_angle / (one_pixel_angle * s * 3)) if math.isfinite(max_angle) else nan
    if not (-2147483648.0 <= q <= 2147483646.0):
        return res
    n_steps = int(q)
    step = max_angle / n_steps if n_steps else nan            # 0 / 0 in C++ (not reachable: the guard above keeps max_angle above 1e-4)
    rs = np.array([a @ RS, J @ RS])
    rd = np.array([a @ RE, J @ RE]) - rs
    rd = rd / math.sqrt(float(rd @ rd))
    ang = np.arange(max(n_steps + 1, 0)) * step
    cs, sn = np.cos(ang), np.sin(ang)
    alpha = (rs[0] * sn - rs[1] * cs) / (rd[1] * cs - rd[0] * sn)
    tc = RS[None, :] + alpha[:, None] * dirn[None, :]
    world = (tc - tt) @ Rt
    pr, pd = pixel_vectors(pose_src, cen, rig, dow, world)
    res.update(n=len(ang), world=world, tc=tc, pixel_right_w=pr, pixel_down_w=pd, step=step, max_angle=max_angle)
    return res


def select_matches(matches):
    """The ambiguity rules of :798-825 as the code has them.  matches: [(score, hypothesis, coarse_pos)] in hypothesis order.  Returns
    (outcome code or 0, kept matches in sorted order).  Python's sort is stable (libstdc++'s std::sort is a stable insertion sort up to 16 entries)."""
    if not matches:
        return NO_MATCH, []
    best = min(m[0] for m in matches)
    n_best = next(m[1] for m in matches if m[0] == best)
    srt = sorted(matches, key=lambda m: m[0])
    n_resize = 1 + sum(1 for m in srt[1:] if m[0] > best * 0.9)
    if n_resize > 3:
        return TOO_MANY, []
    kept = srt[:n_resize]
    if any(abs(m[1] - n_best) > 1 for m in kept[1:]):
        return INDEX_FAR, []
    return 0, kept


def reproject_point(pose_ab, vA, vB):
    """ReprojectPoint (:123-143): point in frame B from the rays vA (frame A) and vB (frame B), se3AfromB = pose_ab"""
    R, t = pose_ab
    P = np.hstack([R, np.asarray(t).reshape(3, 1)])
    A = np.zeros((4, 4))
    A[0] = [-vB[2], 0.0, vB[0], 0.0]
    A[1] = [0.0, -vB[2], vB[1], 0.0]
    A[2] = vA[0] * P[2] - vA[2] * P[0]
    A[3] = vA[1] * P[2] - vA[2] * P[1]
    v = np.linalg.svd(A)[2][3].copy()
    if v[3] == 0.0:
        v[3] = 0.00001
    return v[:3] / v[3]


def triangulate(cam_src, cam_tgt, pose_src, pose_tgt, root, sub):
    """:857-860: world position of the new point"""
    Rs, ts = pose_src
    Rt, tt = pose_tgt
    Rab = Rs @ Rt.T
    tab = ts - Rab @ tt
    xb = reproject_point((Rab, tab), cam_src.unproject(root)[0], cam_tgt.unproject(sub)[0])
    return Rt.T @ (xb - tt)


def hypothesis_points(hyp, off, i, src, src_oracle=None):
    """point dicts (keyframe.patch_sequences / oracle_patch_sequences) of candidate i's hypotheses from a stereo_hypotheses export"""
    pts = []
    for h in hyp[off[i]:off[i + 1]]:
        pts.append(dict(world_pos=h["world_pos"], pixel_right_w=h["pixel_right_w"], pixel_down_w=h["pixel_down_w"], source_kf=src,
                        source_kf_oracle=src_oracle, source_level=int(h["source_level"]), center=(int(h["center_x"]), int(h["center_y"])), fixed=0))
    return pts


def compose_target(patch_sequences, tgt, cam_tgt, pose_tgt, hyp, off, idx, src, src_oracle=None):
    """One target of AddStereoMapPoints as the composition of existing calls for the candidates idx: their hypotheses (a stereo_hypotheses export
    hyp / off) as one MCP_PF_EPI_COARSE sequence each with fresh finders, select_matches, the kept matches as MCP_PF_EPI_REFINE sequences on the
    returned states.  patch_sequences: keyframe.patch_sequences, or the oracle's with tgt = its keyframe.  Returns {candidate: (code, hypothesis,
    score, sub-pixel position or None)}."""
    I = (np.eye(3), np.zeros(3))
    targets = [(tgt, cam_tgt, pose_tgt, I)]
    seqs, pts = [], {}
    for i in idx:
        pts[i] = hypothesis_points(hyp, off, i, src, src_oracle)
        seqs.append([dict(point=p, point_key=1, target=0) for p in pts[i]])
    res = {}
    if not seqs:
        return res
    states = K.new_pf_states(len(seqs))
    co = patch_sequences(K.PF_EPI_COARSE, targets, seqs, states, 3)
    pos, kept = 0, {}
    for q, i in enumerate(idx):
        n = len(seqs[q])
        o = co[pos:pos + n]
        pos += n
        if off[i + 1] == off[i]:
            res[i] = (NO_ARC, -1, 0, None)
            continue
        m = [(int(o[h]["score"]), h, o[h]["found_pos"].copy()) for h in range(n) if o[h]["found"]]
        code, k = select_matches(m)
        if code:
            res[i] = (code, -1, 0, None)
        else:
            kept[q] = k
    ref_seqs = [[dict(point=pts[idx[q]][m[1]], point_key=1, target=0, start_pos=m[2]) for m in kept.get(q, [])] for q in range(len(idx))]
    ro = patch_sequences(K.PF_EPI_REFINE, targets, ref_seqs, states, 3, 10)
    pos = 0
    for q, i in enumerate(idx):
        n = len(ref_seqs[q])
        o = ro[pos:pos + n]
        pos += n
        if q not in kept:
            continue
        win = next((k for k in range(n) if o[k]["found"]), None)
        if win is None:
            res[i] = (NO_SUBPIX, -1, 0, None)
        else:
            m = kept[q][win]
            res[i] = (CREATED, m[1], m[0], o[win]["found_pos"].copy())
    return res


def compose(patch_sequences, src, src_cam, src_pose, level, cand, targets, limit=1 << 30, meas_root=(), meas_level=(), src_oracle=None,
            search_kfs=None):
    """AddStereoMapPoints of one source and level composed from existing calls: numpy ThinCandidates before every target, stereo_hypotheses of the
    survivors, compose_target, the reference's nLimit loop (:486-493) and triangulate.  targets: (keyframe, camera, CamFromWorld[, one_pixel_angle])
    as for stereo_points; search_kfs: the keyframes patch_sequences searches in (default: the targets' own).  Returns (list of created point dicts in
    creation order, keep mask)."""
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    alive = thin_candidates(cand, level, meas_root, meas_level)
    keep = alive.copy()
    made, num = [], 0
    for j, t in enumerate(targets):
        new = [p["root_pos"] for p in made if p["target"] == j - 1]
        if new:
            alive &= thin_candidates(cand, level, created_root=new)
        keep = alive.copy()
        idx = np.nonzero(alive)[0]
        if len(idx) == 0:
            continue
        hyp, off = stereo_hypotheses(src, src_cam, src_pose, level, cand[idx], t)
        sk = t[0] if search_kfs is None else search_kfs[j]
        res = compose_target(patch_sequences, sk, t[1], t[2], hyp, off, list(range(len(idx))), src, src_oracle)
        for q, i in enumerate(idx):
            code, h, score, sub = res[q]
            if code == CREATED:
                root = level_zero_pos(cand[i], level)
                made.append(dict(candidate=int(i), target=j, hypothesis=h, score=score, root_pos=root, target_pos=sub,
                                 world_pos=triangulate(src_cam, t[1], src_pose, t[2], root, sub)))
                num += 1
            if num >= limit:
                break
    return made, keep
