"""ctypes binding of Tracker::FindPVS and TrackMap over a device-resident map-point table (include/mcp_img.h: mcp_map_points_*,
mcp_track_find_pvs, mcp_track_map).  The table holds, per row, what FindPVS reads of a MapPoint (world position, the two pixel vectors, usable =
!mbBad && mbOptimized); one find_pvs call gives the potentially visible set of every camera of a frame, level by level."""
import ctypes

import numpy as np

from . import chain_bundle as _cb
from .keyframe import LEVELS, MEST, PF_STATE_DTYPE, TD_OUT_DTYPE, TdOut, _chk, _pose12
from .keyframe import lib as _kf_lib
from .taylor_camera import camera_array


class PvsEntry(ctypes.Structure):
    _fields_ = [("point", ctypes.c_int), ("level", ctypes.c_int), ("image", ctypes.c_double * 2), ("cam_derivs", ctypes.c_double * 4),
                ("warp_inverse", ctypes.c_double * 4)]


PVS_ENTRY_DTYPE = np.dtype([("point", "i4"), ("level", "i4"), ("image", "f8", 2), ("cam_derivs", "f8", 4), ("warp_inverse", "f8", 4)], align=True)
assert PVS_ENTRY_DTYPE.itemsize == ctypes.sizeof(PvsEntry)

_BOUND = False


def lib():
    global _BOUND
    L = _kf_lib()
    if not _BOUND:
        vp, ip, dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p
        L.mcp_map_points_create.restype = vp
        L.mcp_map_points_create.argtypes = [ip]
        L.mcp_map_points_destroy.argtypes = [vp]
        L.mcp_map_points_rows.argtypes = [vp]
        L.mcp_map_points_resize.argtypes = [vp, ip]
        L.mcp_map_points_set.argtypes = [vp, ip, ip, dp, dp, dp, vp]
        L.mcp_map_points_update.argtypes = [vp, ip, vp, dp, dp, dp, vp]
        L.mcp_track_find_pvs.argtypes = [vp, ip, vp, vp, dp, dp, vp, vp, vp]
        L.mcp_track_find_pvs_view.restype = vp
        L.mcp_track_find_pvs_view.argtypes = [vp, ip, ip, ctypes.POINTER(ctypes.c_int)]
        _BOUND = True
    return L


def _soa(a, n, what):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n, 3):
        raise ValueError("%s: expected shape (%d, 3), got %s" % (what, n, a.shape))
    return a


def _usable(u, n):
    if u is None:
        return np.ones(n, dtype=np.uint8)
    u = np.ascontiguousarray(np.asarray(u) != 0, dtype=np.uint8)
    if u.shape != (n,):
        raise ValueError("usable: expected shape (%d,), got %s" % (n, u.shape))
    return u


class MapPointTable:
    """Device-resident map-point table (one device).  Row = point index in the caller's order.  Inputs are numpy SoA arrays."""

    def __init__(self, device=-1):
        self._L = lib()
        self._h = self._L.mcp_map_points_create(int(device))
        if not self._h:
            raise RuntimeError("mcp_map_points_create failed: " + _cb.last_error())
        self.counts = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.mcp_map_points_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    @property
    def rows(self):
        return _chk(self._L.mcp_map_points_rows(self._h), "map_points_rows")

    def resize(self, rows):
        """The table's size becomes `rows`: rows past it are dropped (no later PVS sees them; a later growth brings them back as
        unusable zero rows); a larger size appends unusable rows."""
        _chk(self._L.mcp_map_points_resize(self._h, int(rows)), "map_points_resize")

    def set(self, world_pos, pixel_right_w, pixel_down_w, usable=None, first=0):
        """Rows first .. first+n-1 (the table grows past its end; rows never written are unusable)."""
        n = len(world_pos)
        wp, pr, pd = _soa(world_pos, n, "world_pos"), _soa(pixel_right_w, n, "pixel_right_w"), _soa(pixel_down_w, n, "pixel_down_w")
        us = _usable(usable, n)
        _chk(self._L.mcp_map_points_set(self._h, int(first), n, wp.ctypes.data, pr.ctypes.data, pd.ctypes.data, us.ctypes.data), "map_points_set")

    def update(self, ids, world_pos, pixel_right_w, pixel_down_w, usable=None):
        """Rows ids (distinct) -- points the map maker moved, flagged or added."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        n = len(ids)
        wp, pr, pd = _soa(world_pos, n, "world_pos"), _soa(pixel_right_w, n, "pixel_right_w"), _soa(pixel_down_w, n, "pixel_down_w")
        us = _usable(usable, n)
        _chk(self._L.mcp_map_points_update(self._h, n, ids.ctypes.data, wp.ctypes.data, pr.ctypes.data, pd.ctypes.data, us.ctypes.data),
             "map_points_update")

    def find_pvs(self, targets, cams, base_from_world, cams_from_base, caps=None, out=None, view=False):
        """Tracker::FindPVS for every camera of a frame in one call.  targets: KeyFrame per camera; cams: TaylorCamera per camera (or a
        ctypes camera array); base_from_world: (R, t); cams_from_base: (R, t) per camera or an (ncam, 12) array.  caps: entries per
        camera (default: the table's rows); out: per-camera PVS_ENTRY_DTYPE arrays of at least caps[c] entries, or None.
        view=True: the lists are views of the library's pinned block, valid until the next call on this table.
        Returns, per camera, the four per-level arrays (rows ascending).  self.counts = (ncam, LEVELS) counts, set even when the call fails."""
        ncam = len(targets)
        hs = (ctypes.c_void_p * ncam)(*[t._h for t in targets])
        cs = cams if isinstance(cams, ctypes.Array) else camera_array(cams)
        b = _pose12(*base_from_world)
        cfb = np.ascontiguousarray(cams_from_base, dtype=np.float64).reshape(-1) if isinstance(cams_from_base, np.ndarray) else \
            np.ascontiguousarray(np.concatenate([_pose12(*c) for c in cams_from_base]))
        rows = self.rows
        caps = np.ascontiguousarray([rows] * ncam if caps is None else caps, dtype=np.int32)
        counts = np.zeros((ncam, LEVELS), dtype=np.int32)
        self.counts = counts
        ops = None
        if not view:
            if out is None:
                whole = np.empty(int(caps.sum()), dtype=PVS_ENTRY_DTYPE)
                offs = np.concatenate([[0], np.cumsum(caps)]).astype(int)
                out = [whole[offs[c]:offs[c + 1]] for c in range(ncam)]
            for c in range(ncam):
                assert out[c].dtype == PVS_ENTRY_DTYPE and len(out[c]) >= caps[c] and out[c].flags.c_contiguous
            ops = (ctypes.c_void_p * ncam)(*[o.ctypes.data for o in out])
        _chk(self._L.mcp_track_find_pvs(self._h, ncam, hs, ctypes.cast(cs, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data, caps.ctypes.data,
                                        ops, counts.ctypes.data), "track_find_pvs")
        res = []
        for c in range(ncam):
            if view:
                lv = []
                for l in range(LEVELS):
                    cnt = ctypes.c_int(0)
                    ptr = self._L.mcp_track_find_pvs_view(self._h, c, l, ctypes.byref(cnt))
                    if cnt.value != counts[c, l]:
                        raise RuntimeError("mcp_track_find_pvs_view: " + _cb.last_error())
                    lv.append(np.frombuffer((ctypes.c_char * (cnt.value * PVS_ENTRY_DTYPE.itemsize)).from_address(ptr), dtype=PVS_ENTRY_DTYPE)
                              if cnt.value else np.zeros(0, dtype=PVS_ENTRY_DTYPE))
                res.append(lv)
            else:
                offs = np.concatenate([[0], np.cumsum(counts[c])]).astype(int)
                res.append([out[c][offs[l]:offs[l + 1]] for l in range(LEVELS)])
        return res

    def set_source(self, keys, sources, levels, centers, fixed=None, first=0):
        """Rows first .. first+n-1: patch source keyframe (None = no source), level, centre (n x 2), fixed flag, and the row's identity key."""
        L = _bind_track_map(self._L)
        n = len(keys)
        k, hs, lv, cx, fx = _source_arrays(n, keys, sources, levels, centers, fixed)
        _chk(L.mcp_map_points_set_source(self._h, int(first), n, k.ctypes.data, hs, lv.ctypes.data, cx.ctypes.data, fx.ctypes.data), "map_points_set_source")

    def update_source(self, ids, keys, sources, levels, centers, fixed=None):
        L = _bind_track_map(self._L)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        n = len(ids)
        k, hs, lv, cx, fx = _source_arrays(n, keys, sources, levels, centers, fixed)
        _chk(L.mcp_map_points_update_source(self._h, n, ids.ctypes.data, k.ctypes.data, hs, lv.ctypes.data, cx.ctypes.data, fx.ctypes.data), "map_points_update_source")

    def get_states(self, cam, first=0, count=None):
        L = _bind_track_map(self._L)
        count = self.rows - first if count is None else count
        out = np.zeros(max(count, 1), dtype=PF_STATE_DTYPE)
        _chk(L.mcp_map_points_get_states(self._h, int(cam), int(first), int(count), out.ctypes.data), "map_points_get_states")
        return out[:count]

    def track_map(self, targets, cams, base_from_world, cams_from_base, try_coarse=True, coarse_max=60, coarse_range=30, coarse_min=20, coarse_subpix_its=8,
                   max_patches=1000, estimator="Tukey", seed=0, imgs=None, on_device=False, strides=None, copy=True):
        """mcp_track_map: the whole TrackMap of a frame.  Returns (items per camera (TRACK_MAP_ITEM_DTYPE; copies unless copy=False: views of
        the library's pinned block), (R, t), TrackMapResult)."""
        L = _bind_track_map(self._L)
        ncam = len(targets)
        hs = (ctypes.c_void_p * ncam)(*[t._h for t in targets])
        cs = cams if isinstance(cams, ctypes.Array) else camera_array(cams)
        b = _pose12(*base_from_world).copy()
        cfb = np.ascontiguousarray(cams_from_base, dtype=np.float64).reshape(-1) if isinstance(cams_from_base, np.ndarray) else \
            np.ascontiguousarray(np.concatenate([_pose12(*c) for c in cams_from_base]))
        prm = TrackMapParams(int(try_coarse), int(coarse_max), int(coarse_range), int(coarse_min), int(coarse_subpix_its), int(max_patches),
                             MEST[estimator] if isinstance(estimator, str) else int(estimator), int(seed))
        res = TrackMapResult()
        ip = st = keep = None
        if imgs is not None:
            if on_device:
                ip = (ctypes.c_void_p * ncam)(*[int(a) for a in imgs])
                st = (ctypes.c_int * ncam)(*[int(s_) for s_ in (strides or [k.w for k in targets])])
            else:
                keep = [np.ascontiguousarray(a, dtype=np.uint8) for a in imgs]
                ip = (ctypes.c_void_p * ncam)(*[a.ctypes.data for a in keep])
                st = (ctypes.c_int * ncam)(*[a.strides[0] for a in keep])
        _chk(L.mcp_track_map(self._h, ncam, hs, ip, st, int(on_device), None, ctypes.cast(cs, ctypes.c_void_p), b.ctypes.data, cfb.ctypes.data,
                             ctypes.byref(prm), ctypes.byref(res)), "track_map")
        del keep
        items = []
        for c in range(ncam):
            cnt = ctypes.c_int(0)
            ptr = L.mcp_track_map_view(self._h, c, ctypes.byref(cnt))
            a = np.frombuffer((ctypes.c_char * (cnt.value * TRACK_MAP_ITEM_DTYPE.itemsize)).from_address(ptr), dtype=TRACK_MAP_ITEM_DTYPE) \
                if cnt.value else np.zeros(0, dtype=TRACK_MAP_ITEM_DTYPE)
            items.append(a.copy() if copy else a)
        return items, (b[:9].reshape(3, 3).copy(), b[9:].copy()), res


# ---- Tracker::TrackMap of a frame from the table (include/mcp_img.h mcp_track_map) ---------------------------------------------------
TRACK_MAP_SYMBOLS = ["mcp_map_points_set_source", "mcp_map_points_update_source", "mcp_map_points_get_states", "mcp_track_map", "mcp_track_map_view",
                     "mcp_mix64", "mcp_track_shuffle_key"]
MAX_FRAME_CAMS = 8


class TrackMapParams(ctypes.Structure):
    _fields_ = [("try_coarse", ctypes.c_int), ("coarse_max", ctypes.c_int), ("coarse_range", ctypes.c_int), ("coarse_min", ctypes.c_int),
                ("coarse_subpix_its", ctypes.c_int), ("max_patches", ctypes.c_int), ("estimator", ctypes.c_int), ("seed", ctypes.c_ulonglong)]


class TrackMapResult(ctypes.Structure):
    _fields_ = [("did_coarse", ctypes.c_int), ("coarse_found", ctypes.c_int), ("pvs_counts", (ctypes.c_int * LEVELS) * MAX_FRAME_CAMS),
                ("set_sizes", (ctypes.c_int * 3) * MAX_FRAME_CAMS), ("stale", ctypes.c_int * MAX_FRAME_CAMS), ("mu_last", ctypes.c_double * 6)]


class TrackMapItem(ctypes.Structure):
    _fields_ = [("point", ctypes.c_int), ("stage", ctypes.c_int), ("weight_last", ctypes.c_double), ("out", TdOut)]


TRACK_MAP_ITEM_DTYPE = np.dtype([("point", "i4"), ("stage", "i4"), ("weight_last", "f8"), ("out", TD_OUT_DTYPE)], align=True)
assert TRACK_MAP_ITEM_DTYPE.itemsize == ctypes.sizeof(TrackMapItem)


def _mix64(z):
    """mcp_mix64 on a uint64 array (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def shuffle_key(seed, stage, cam, rows):
    """mcp_track_shuffle_key(seed, stage, cam, row) for an array of rows."""
    inner = _mix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64((int(stage) << 40) & 0xFFFFFFFFFFFFFFFF) ^ np.uint64((int(cam) << 32) & 0xFFFFFFFFFFFFFFFF))
    r = np.asarray(rows, dtype=np.int64).astype(np.uint32).astype(np.uint64)
    return _mix64(inner ^ r)


def shuffled(rows, seed, stage, cam):
    """rows in ascending (key, row) order."""
    rows = np.asarray(rows, dtype=np.int64)
    k = shuffle_key(seed, stage, cam, rows)
    return rows[np.lexsort((rows, k))]


def select_sets(levels, seed, cam, try_coarse, coarse_max, max_patches):
    """The sets C, T, R of one camera (include/mcp_img.h mcp_track_map): `levels` = its four PVS row lists (ascending, rows without a live
    source removed).  Returns three int arrays in iteration order."""
    S = [shuffled(levels[l], seed, 0, cam) for l in range(LEVELS)]
    C = np.zeros(0, dtype=np.int64)
    if try_coarse:
        k3 = min(len(S[3]), coarse_max)
        k2 = min(len(S[2]), coarse_max - k3)
        C = np.concatenate([S[3][:k3], S[2][:k2]])
        S[3], S[2] = S[3][k3:], S[2][k2:]
    T = S[3]
    R0 = np.concatenate([S[2], S[1], S[0]])
    K = max(0, max_patches - len(C) - len(T))
    if len(R0) > K:
        k1 = shuffle_key(seed, 1, cam, R0)
        R0 = R0[np.lexsort((R0, k1))][:K]
    return C.astype(np.int64), T.astype(np.int64), R0.astype(np.int64)


def _bind_track_map(L):
    if getattr(L, "_track_map_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_map_points_set_source.argtypes = [vp, ip, ip, vp, vp, vp, vp, vp]
    L.mcp_map_points_update_source.argtypes = [vp, ip, vp, vp, vp, vp, vp, vp]
    L.mcp_map_points_get_states.argtypes = [vp, ip, ip, ip, vp]
    L.mcp_track_map.argtypes = [vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp]
    L.mcp_track_map_view.restype = vp
    L.mcp_track_map_view.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int)]
    L._track_map_bound = True
    return L


def _source_arrays(n, keys, sources, levels, centers, fixed):
    keys = np.ascontiguousarray(keys, dtype=np.int32)
    hs = (ctypes.c_void_p * max(n, 1))(*[(None if s is None else (s if isinstance(s, int) else s._h)) for s in sources])
    lv = np.ascontiguousarray(levels, dtype=np.int32)
    cx = np.ascontiguousarray(np.asarray(centers, dtype=np.int32).reshape(n, 2))
    fx = np.ascontiguousarray(np.zeros(n) if fixed is None else fixed, dtype=np.uint8)
    if not (len(keys) == len(sources) == len(lv) == len(fx) == n):
        raise ValueError("source arrays: lengths differ")
    return keys, hs, lv, cx, fx


