"""ctypes binding of Tracker::FindPVS over a device-resident map-point table (include/mcp_img.h: mcp_map_points_*,
mcp_track_find_pvs).  The table holds, per row, what FindPVS reads of a MapPoint (world position, the two pixel vectors, usable =
!mbBad && mbOptimized); one find_pvs call gives the potentially visible set of every camera of a frame, level by level."""
import ctypes

import numpy as np

from . import chain_bundle as _cb
from .keyframe import LEVELS, _chk, _pose12
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
