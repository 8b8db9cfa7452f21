"""ctypes binding of Tracker::FindPVS and TrackMap over a device-resident map-point table (include/mcp_img.h: mcp_map_points_*,
mcp_track_find_pvs, mcp_track_map).  The table holds, per row, what FindPVS reads of a MapPoint (world position, the two pixel vectors, usable =
!mbBad && mbOptimized); one find_pvs call gives the potentially visible set of every camera of a frame, level by level.  track_map runs the
whole TrackMap of a frame from the table; track_map_record also leaves its bookkeeping (marks into the table's count column, level counters,
quality, found measurements, scene depth), with track_record_restate / tracking_quality as the numpy restatements.  track_frame_motion is
track_map_record started from the pose the tracker's motion model gives on the device (SmallBlurryImage rotation estimate, velocity), with
so3_ln / se3_ln / average_rotation / motion_prior / motion_update as the numpy restatements.  track_frame_recover is the lost branch: the
relocaliser (SmallBlurryImage scores over a candidate list, alignment against the winner, the recovered pose) on the device in front of the
same frame, with recover_restate as the numpy restatement."""
import ctypes
import math

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


def _frame_args(targets, cams, base_from_world, cams_from_base, imgs=None, on_device=False, strides=None):
    """What every frame call passes: (ncam, target handles, camera array as void*, BaseFromWorld as 12 doubles (a copy: track_map refines it),
    CamFromBase (ncam x 12), image pointers or None, strides or None, and whatever must stay alive until the call returns)."""
    ncam = len(targets)
    hs = (ctypes.c_void_p * ncam)(*[t._h for t in targets])
    cs = cams if isinstance(cams, ctypes.Array) else camera_array(cams)
    b = _pose12(*base_from_world).copy()
    cfb = np.ascontiguousarray(cams_from_base, dtype=np.float64).reshape(-1) if isinstance(cams_from_base, np.ndarray) else \
        np.ascontiguousarray(np.concatenate([_pose12(*c) for c in cams_from_base]))
    ip = st = keep = None
    if imgs is not None:
        if on_device:
            ip = (ctypes.c_void_p * ncam)(*[int(a) for a in imgs])
            st = (ctypes.c_int * ncam)(*[int(s_) for s_ in (strides or [k.w for k in targets])])
        else:
            keep = [np.ascontiguousarray(a, dtype=np.uint8) for a in imgs]
            ip = (ctypes.c_void_p * ncam)(*[a.ctypes.data for a in keep])
            st = (ctypes.c_int * ncam)(*[a.strides[0] for a in keep])
    return ncam, hs, ctypes.cast(cs, ctypes.c_void_p), b, cfb, ip, st, (cs, keep)


def _view(fn, args, dtype, expect=None, copy=False, mismatch=""):
    """The array behind one of the library's *_view calls: fn(*args, &count) -> pointer into a pinned block that stays valid until the next
    call on the table.  expect: the count the call's own results announce; mismatch: the error's text when the view disagrees, a format
    of (got, expect), followed by the library's last error."""
    cnt = ctypes.c_int(0)
    ptr = fn(*args, ctypes.byref(cnt))
    if expect is not None and cnt.value != expect:
        raise RuntimeError(mismatch % dict(got=cnt.value, expect=expect) + _cb.last_error())
    a = np.frombuffer((ctypes.c_char * (cnt.value * dtype.itemsize)).from_address(ptr), dtype=dtype) if cnt.value else np.zeros(0, dtype=dtype)
    return a.copy() if copy else a


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
            if getattr(self, "_open_graphs", 0) > 0:           # a map graph (map_graph.MapGraph) is still open on this table and reads it when it
                self._close_pending = True                     # is destroyed: the table's handle goes when the last of them has been closed
                return
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
        ncam, hs, cs, b, cfb, _, _, keep = _frame_args(targets, cams, base_from_world, cams_from_base)
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
        _chk(self._L.mcp_track_find_pvs(self._h, ncam, hs, cs, b.ctypes.data, cfb.ctypes.data, caps.ctypes.data, ops, counts.ctypes.data), "track_find_pvs")
        del keep
        res = []
        for c in range(ncam):
            if view:
                res.append([_view(self._L.mcp_track_find_pvs_view, (self._h, c, l), PVS_ENTRY_DTYPE, counts[c, l], mismatch="mcp_track_find_pvs_view: ")
                            for l in range(LEVELS)])
            else:
                offs = np.concatenate([[0], np.cumsum(counts[c])]).astype(int)
                res.append([out[c][offs[l]:offs[l + 1]] for l in range(LEVELS)])
        return res

    # ---- AdjustAndUpdate: patch rays, read-back, the write-back of an adjustment (include/mcp_img.h mcp_ba_write_back) ----
    def set_rays(self, center_nc, one_right_nc, one_down_nc, first=0):
        """Patch rays (mv3Center_NC, mv3OneRightFromCenter_NC, mv3OneDownFromCenter_NC) of rows first .. first+n-1."""
        L = _bind_write_back(self._L)
        n = len(center_nc)
        ce, ri, dn = _soa(center_nc, n, "center_nc"), _soa(one_right_nc, n, "one_right_nc"), _soa(one_down_nc, n, "one_down_nc")
        _chk(L.mcp_map_points_set_rays(self._h, int(first), n, ce.ctypes.data, ri.ctypes.data, dn.ctypes.data), "map_points_set_rays")

    def update_rays(self, ids, center_nc, one_right_nc, one_down_nc):
        L = _bind_write_back(self._L)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        n = len(ids)
        ce, ri, dn = _soa(center_nc, n, "center_nc"), _soa(one_right_nc, n, "one_right_nc"), _soa(one_down_nc, n, "one_down_nc")
        _chk(L.mcp_map_points_update_rays(self._h, n, ids.ctypes.data, ce.ctypes.data, ri.ctypes.data, dn.ctypes.data), "map_points_update_rays")

    def get(self, first=0, count=None):
        """Rows first .. first+count-1 read back: (world_pos, pixel_right_w, pixel_down_w, usable)."""
        L = _bind_write_back(self._L)
        count = self.rows - first if count is None else int(count)
        wp, pr, pd = (np.zeros((count, 3)) for _ in range(3))
        us = np.zeros(count, dtype=np.uint8)
        _chk(L.mcp_map_points_get(self._h, int(first), count, wp.ctypes.data, pr.ctypes.data, pd.ctypes.data, us.ctypes.data), "map_points_get")
        return wp, pr, pd, us

    def get_rays(self, first=0, count=None):
        """Patch rays of rows first .. first+count-1 read back: (rays (count, 9): center, one right, one down; has: which rows have them)."""
        from .stereo import lib as _stereo_lib
        count = self.rows - first if count is None else int(count)
        rays, has = np.zeros((max(count, 1), 9)), np.zeros(max(count, 1), dtype=np.uint8)
        _chk(_stereo_lib().mcp_map_points_get_rays(self._h, int(first), count, rays.ctypes.data, has.ctypes.data), "map_points_get_rays")
        return rays[:count], has[:count]

    def get_source(self, first=0, count=None):
        """The source column of rows first .. first+count-1 read back: dict(key, level, center (count, 2), fixed, has_source)."""
        from .stereo import lib as _stereo_lib
        count = self.rows - first if count is None else int(count)
        n = max(count, 1)
        o = dict(key=np.zeros(n, np.int32), level=np.zeros(n, np.int32), center=np.zeros((n, 2), np.int32), fixed=np.zeros(n, np.uint8), has_source=np.zeros(n, np.uint8))
        _chk(_stereo_lib().mcp_map_points_get_source(self._h, int(first), count, *[o[k].ctypes.data for k in ("key", "level", "center", "fixed", "has_source")]),
             "map_points_get_source")
        return {k: v[:count] for k, v in o.items()}

    def last_timing(self):
        """Device milliseconds of the last write_back / scene_depth on this table: dict(copy, points, depth)."""
        L = _bind_write_back(self._L)
        v = (ctypes.c_double * 3)()
        _chk(L.mcp_map_points_last_timing(self._h, ctypes.byref(v, 0), ctypes.byref(v, 8), ctypes.byref(v, 16)), "map_points_last_timing")
        return dict(copy=v[0], points=v[1], depth=v[2])

    def scene_depth(self, cam_from_world, seg_start, seg_rows, seg_weights, depths=True):
        """mcp_scene_depth_robust: KeyFrame::RefreshSceneDepthRobust of every keyframe j with pose cam_from_world[j] (12 doubles) over the rows
        seg_rows[seg_start[j]:seg_start[j+1]].  Returns (SCENE_DEPTH_DTYPE array, depths in list order or None)."""
        L = _bind_write_back(self._L)
        ss, sr, sw = _csr(seg_start, seg_rows, seg_weights)
        n_kf = len(ss) - 1
        cfw = np.ascontiguousarray(cam_from_world, dtype=np.float64).reshape(n_kf, 12)
        out = np.zeros(n_kf, dtype=SCENE_DEPTH_DTYPE)
        dep = np.zeros(len(sr)) if depths else None
        _chk(L.mcp_scene_depth_robust(self._h, n_kf, cfw.ctypes.data, ss.ctypes.data, sr.ctypes.data, sw.ctypes.data, out.ctypes.data,
                                      dep.ctypes.data if depths else None), "scene_depth_robust")
        return out, dep

    def write_back(self, bundle, point_ids, rows, src_chains=None, src_chain_len=None, kf_chains=None, kf_chain_len=None, seg_start=None,
                   seg_rows=None, seg_weights=None, outputs=True):
        """mcp_ba_write_back: AdjustAndUpdate from `bundle` (a ChainBundle that was prepared or solved) into this table.  point_ids: bundle point
        ids, rows: their table rows; src_chains (n, stride) / src_chain_len: the chain RefreshPixelVectors uses (length 0: the point's own);
        kf_chains (n_kf, stride) / kf_chain_len: every keyframe's CamFromWorld as a chain; seg_*: the keyframes' lists (CSR) of rows and weights.
        Returns a dict: world_pos, pixel_right_w, pixel_down_w (n, 3), kf_cam_from_world (n_kf, 12), depth (SCENE_DEPTH_DTYPE), seg_depths --
        or None with outputs=False."""
        L = _bind_write_back(self._L)
        pid = np.ascontiguousarray(point_ids, dtype=np.int32)
        rw = np.ascontiguousarray(rows, dtype=np.int32)
        n = len(pid)
        if len(rw) != n:
            raise ValueError("write_back: point_ids and rows differ in length")
        stride = 1
        sc = sl = None
        if src_chains is not None:
            sc = np.ascontiguousarray(src_chains, dtype=np.int32).reshape(n, -1)
            sl = np.ascontiguousarray(src_chain_len, dtype=np.int32)
            stride = sc.shape[1]
        n_kf = 0 if kf_chains is None else len(kf_chains)
        kc = kl = ss = sr = sw = None
        if n_kf:
            kc = np.ascontiguousarray(kf_chains, dtype=np.int32).reshape(n_kf, -1)
            kl = np.ascontiguousarray(kf_chain_len, dtype=np.int32)
            if sc is not None and kc.shape[1] != stride:      # one stride for both chain arrays
                w = max(stride, kc.shape[1])
                sc = np.ascontiguousarray(np.pad(sc, ((0, 0), (0, w - stride))))
                kc = np.ascontiguousarray(np.pad(kc, ((0, 0), (0, w - kc.shape[1]))))
            stride = kc.shape[1]
            ss, sr, sw = _csr(seg_start, seg_rows, seg_weights)
            if len(ss) != n_kf + 1:
                raise ValueError("write_back: seg_start must have n_kf + 1 entries")
        res = None
        ptr = lambda a: None if a is None else a.ctypes.data
        if outputs:
            res = dict(world_pos=np.zeros((n, 3)), pixel_right_w=np.zeros((n, 3)), pixel_down_w=np.zeros((n, 3)), kf_cam_from_world=np.zeros((n_kf, 12)),
                       depth=np.zeros(n_kf, dtype=SCENE_DEPTH_DTYPE), seg_depths=np.zeros(0 if sr is None else len(sr)))
        o = (lambda k: res[k].ctypes.data) if outputs else (lambda k: None)
        _chk(L.mcp_ba_write_back(bundle._h, self._h, n, ptr(pid), ptr(rw), ptr(sc), stride, ptr(sl), o("world_pos"), o("pixel_right_w"), o("pixel_down_w"),
                                 n_kf, ptr(kc), ptr(kl), ptr(ss), ptr(sr), ptr(sw), o("kf_cam_from_world"), o("depth"), o("seg_depths")), "ba_write_back")
        return res

    def refind(self, targets, pairs, per_row_finders=False, finder=None, view=False, cap_meas=None):
        """mcp_map_refind: MapMakerServerBase::ReFind_Common of (row, target) pairs in one call -- see mcptam_amd.refind.refind.  Returns
        (verdicts, measurements, counts, finder)."""
        from .refind import refind
        return refind(self, targets, pairs, per_row_finders, finder, view, cap_meas)

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
        return self._track_frame(_bind_track_map(self._L), "track_map", (targets, cams, base_from_world, cams_from_base, imgs, on_device, strides),
                                 (try_coarse, coarse_max, coarse_range, coarse_min, coarse_subpix_its, max_patches, estimator, seed), copy)

    def _track_frame(self, L, name, frame, search, copy, record=None, cams_sbi=None, more=()):
        """What the four one-call frames share: L.mcp_<name> over frame (_frame_args' arguments) with the TrackMapParams of search, the 40x30
        cameras behind the cameras where given, the TrackRecordParams of record (lost, want_items, min_patches, quality_coarse_min,
        quality_good, quality_bad) and a TrackRecord behind the result where given, then `more`.  Returns track_map's tuple, or with record
        track_map_record's."""
        ncam, hs, cs, b, cfb, ip, st, keep = _frame_args(*frame)
        prm = TrackMapParams(*[int(v) for v in search[:6]], MEST[search[6]] if isinstance(search[6], str) else int(search[6]), int(search[7]))
        res = TrackMapResult()
        args = [self._h, ncam, hs, ip, st, int(frame[5]), None, cs]
        if cams_sbi is not None:
            keep += (cams_sbi if isinstance(cams_sbi, ctypes.Array) else camera_array(cams_sbi),)
            args.append(ctypes.cast(keep[-1], ctypes.c_void_p))
        args += [b.ctypes.data, cfb.ctypes.data, ctypes.byref(prm), ctypes.byref(res)]
        if record is not None:
            lost, want_items, min_patches, quality_coarse_min, quality_good, quality_bad = record
            rp, rec = TrackRecordParams(int(bool(lost)), int(bool(want_items)), int(min_patches), int(quality_coarse_min), float(quality_good), float(quality_bad)), TrackRecord()
            args += [ctypes.byref(rp), ctypes.byref(rec)]
        _chk(getattr(L, "mcp_" + name)(*args, *more), name)
        del keep
        pose = (b[:9].reshape(3, 3).copy(), b[9:].copy())
        if record is None:
            return [_view(L.mcp_track_map_view, (self._h, c), TRACK_MAP_ITEM_DTYPE, copy=copy) for c in range(ncam)], pose, res

        def views(fn, dtype, expect):
            text = name + ": view of camera %d has %%(got)d entries, the record says %%(expect)d: "
            return [_view(fn, (self._h, c), dtype, expect[c], copy, text % c) for c in range(ncam)]
        items = views(L.mcp_track_map_view, TRACK_MAP_ITEM_DTYPE, rec.n_items) if want_items else None
        notes = views(L.mcp_track_map_notes_view, TRACK_NOTE_DTYPE, rec.n_items)
        meas = views(L.mcp_track_map_meas_view, TRACK_MEAS_DTYPE, rec.n_meas)
        return items, pose, res, notes, meas, rec

    # ---- TrackMap with its bookkeeping (include/mcp_img.h mcp_track_map_record) ----
    def set_counts(self, inlier, outlier, first=0):
        """mnMEstimatorInlierCount / mnMEstimatorOutlierCount of rows first .. first+n-1 (inlier >= 1, outlier >= 0)."""
        L = _bind_track_record(self._L)
        i, o = _counts_arrays(inlier, outlier)
        _chk(L.mcp_map_points_set_counts(self._h, int(first), len(i), i.ctypes.data, o.ctypes.data), "map_points_set_counts")

    def update_counts(self, ids, inlier, outlier):
        L = _bind_track_record(self._L)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        i, o = _counts_arrays(inlier, outlier)
        if len(i) != len(ids):
            raise ValueError("update_counts: ids and counts differ in length")
        _chk(L.mcp_map_points_update_counts(self._h, len(ids), ids.ctypes.data, i.ctypes.data, o.ctypes.data), "map_points_update_counts")

    def get_counts(self, first=0, count=None):
        """(inlier, outlier) of rows first .. first+count-1; a row whose counts were never set reads (1, 0)."""
        L = _bind_track_record(self._L)
        count = self.rows - first if count is None else int(count)
        i, o = np.zeros(max(count, 1), dtype=np.int32), np.zeros(max(count, 1), dtype=np.int32)
        _chk(L.mcp_map_points_get_counts(self._h, int(first), count, i.ctypes.data, o.ctypes.data), "map_points_get_counts")
        return i[:count], o[:count]

    def track_map_record(self, targets, cams, base_from_world, cams_from_base, lost=False, want_items=True, min_patches=10, quality_coarse_min=20,
                         quality_good=0.3, quality_bad=0.13, try_coarse=True, coarse_max=60, coarse_range=30, coarse_min=20, coarse_subpix_its=8,
                         max_patches=1000, estimator="Tukey", seed=0, imgs=None, on_device=False, strides=None, copy=True):
        """mcp_track_map_record: track_map plus what TrackMap leaves behind -- marks into the count column, level counters and quality, the
        found measurements, the scene depth per camera.  quality_coarse_min is AssessTrackingQuality's snCoarseMin (coarse_min: the coarse
        gate's).  Returns (items per camera, or None with want_items=False; (R, t); TrackMapResult; notes per camera (TRACK_NOTE_DTYPE);
        measurements per camera (TRACK_MEAS_DTYPE); TrackRecord) -- copies unless copy=False."""
        return self._track_frame(_bind_track_record(_bind_track_map(self._L)), "track_map_record",
                                 (targets, cams, base_from_world, cams_from_base, imgs, on_device, strides),
                                 (try_coarse, coarse_max, coarse_range, coarse_min, coarse_subpix_its, max_patches, estimator, seed), copy,
                                 (lost, want_items, min_patches, quality_coarse_min, quality_good, quality_bad))

    # ---- TrackFrame's tracking branch: motion model + TrackMap + its bookkeeping (include/mcp_img.h mcp_track_frame_motion) ----
    def track_frame_motion(self, targets, cams, cams_sbi, base_from_world, cams_from_base, velocity=None, dt=1.0 / 30, cam_good=None, apply=True,
                           use_rotation_estimator=True, sbi_iterations=6, blur=0.75, lost=False, want_items=True, min_patches=10, quality_coarse_min=20,
                           quality_good=0.3, quality_bad=0.13, try_coarse=True, coarse_max=60, coarse_range=30, coarse_min=20, coarse_subpix_its=8,
                           max_patches=1000, estimator="Tukey", seed=0, imgs=None, on_device=False, strides=None, copy=True):
        """mcp_track_frame_motion: ApplyMotionModel (with the SBI rotation estimate), TrackMap with its bookkeeping and UpdateMotionModel in one
        call.  base_from_world: last frame's pose (mse3StartPose); cams_sbi: the 40x30 camera per camera; velocity: mv6BaseVelocity [t; w];
        cam_good: per camera, was its tracking quality GOOD after the previous frame (default: all).  Returns track_map_record's tuple plus the
        TrackMotion report (start, prior, se2, sbi_score, cam_rot, sbi_rot, n_used, avg_rounds, first_frame, v_new, velocity)."""
        mp, mo = motion_params(velocity, dt, cam_good, apply, use_rotation_estimator, sbi_iterations, blur, len(targets)), TrackMotion()
        return self._track_frame(_bind_track_motion(_bind_track_record(_bind_track_map(self._L))), "track_frame_motion",
                                 (targets, cams, base_from_world, cams_from_base, imgs, on_device, strides),
                                 (try_coarse, coarse_max, coarse_range, coarse_min, coarse_subpix_its, max_patches, estimator, seed), copy,
                                 (lost, want_items, min_patches, quality_coarse_min, quality_good, quality_bad), cams_sbi,
                                 (ctypes.byref(mp), ctypes.byref(mo))) + (mo,)

    # ---- TrackFrame's lost branch: relocaliser + TrackMap + its bookkeeping (include/mcp_img.h mcp_track_frame_recover) ----
    def track_frame_recover(self, targets, cams, cams_sbi, base_from_world, cams_from_base, cand_kfs, cand_cams, cand_poses, reloc_blur=2.5,
                            reloc_iterations=6, max_score=1e5, want_scores=True, velocity=None, use_rotation_estimator=True, sbi_iterations=6, blur=0.75,
                            lost=True, want_items=True, min_patches=10, quality_coarse_min=20, quality_good=0.3, quality_bad=0.13, try_coarse=True, coarse_max=60,
                            coarse_range=30, coarse_min=20, coarse_subpix_its=8, max_patches=1000, estimator="Tukey", seed=0, imgs=None, on_device=False,
                            strides=None, copy=True):
        """mcp_track_frame_recover: Tracker::AttemptRecovery with the relocaliser, then TrackMap with its bookkeeping from the recovered pose, in
        one call.  cand_kfs: the map's keyframes (KeyFrame, None, or a raw handle value), cand_cams: each one's camera index among the
        targets, cand_poses: each one's CamFromWorld ((R, t) pairs or an (n, 12) array).  The caller sets try_coarse and the doubled coarse
        caps.  Returns track_frame_motion's tuple plus the TrackRecover report and the scores (None with want_scores=False)."""
        mp, mo = motion_params(velocity, 1.0, None, False, use_rotation_estimator, sbi_iterations, blur, len(targets)), TrackMotion()
        ncand, ch, cc, cp = _candidate_args(cand_kfs, cand_cams, cand_poses)
        rq, rv = TrackRecoverParams(float(reloc_blur), int(reloc_iterations), float(max_score)), TrackRecover()
        scores = np.zeros(max(ncand, 1)) if want_scores else None
        more = (ctypes.byref(mp), ctypes.byref(mo), ncand, ctypes.cast(ch, ctypes.c_void_p), cc.ctypes.data, cp.ctypes.data, ctypes.byref(rq), ctypes.byref(rv),
                scores.ctypes.data if want_scores else None)
        return self._track_frame(_bind_track_recover(_bind_track_motion(_bind_track_record(_bind_track_map(self._L)))), "track_frame_recover",
                                 (targets, cams, base_from_world, cams_from_base, imgs, on_device, strides),
                                 (try_coarse, coarse_max, coarse_range, coarse_min, coarse_subpix_its, max_patches, estimator, seed), copy,
                                 (lost, want_items, min_patches, quality_coarse_min, quality_good, quality_bad), cams_sbi,
                                 more) + (mo, rv, scores[:ncand] if want_scores else None)

    def motion_reset(self):
        """Tracker::Reset: every camera index forgets its SmallBlurryImages."""
        _chk(_bind_track_motion(self._L).mcp_track_motion_reset(self._h), "track_motion_reset")

    def motion_sbi(self, cam, which=0):
        """The tracker's SBI of camera index cam, which = 0 this frame's, 1 last frame's: (small u8 30x40, template f32 30x40, jacs f32 30x40x2)."""
        small = np.zeros((30, 40), dtype=np.uint8)
        templ = np.zeros((30, 40), dtype=np.float32)
        jacs = np.zeros((30, 40, 2), dtype=np.float32)
        _chk(_bind_track_motion(self._L).mcp_track_motion_get_sbi(self._h, int(cam), int(which), small.ctypes.data, templ.ctypes.data, jacs.ctypes.data), "track_motion_get_sbi")
        return small, templ, jacs


    # ---- the pose covariance of the last fine iteration (include/mcp_img.h mcp_track_pose_cov_enable) ----
    def pose_cov_enable(self, on=True):
        """With it on, track_map / track_map_record / track_frame_motion / track_frame_recover also leave mm6PoseCovariance (pose_cov_last)."""
        _chk(_bind_track_cov(self._L).mcp_track_pose_cov_enable(self._h, int(bool(on))), "track_pose_cov_enable")

    def pose_cov_last(self):
        """The TrackPoseCov of the last track call on this table; raises unless that call succeeded with pose_cov_enable on."""
        out = TrackPoseCov()
        _chk(_bind_track_cov(self._L).mcp_track_pose_cov_last(self._h, ctypes.byref(out)), "track_pose_cov_last")
        return out

    # ---- FindPVS over the co-visible points of the nearest keyframe (include/mcp_img.h mcp_track_collect_nearest) ----
    def collect_nearest(self, graph, depth_mean, mean_diff_fraction=0.5):
        """tracker_collect_all_points = false: while it is on, find_pvs and the four one-call frames judge a row for camera c only if it is a
        co-visible point of the map keyframe nearest to the current keyframe c (map_graph.MapGraph.collect_nearest, at the pose the PVS launch
        reads).  graph: the MapGraph of this table; depth_mean: mdSceneDepthMean per frame camera.  Host-only: call it before every frame with
        fresh depth means.  A refusal raises RuntimeError and leaves the mode as it was."""
        prm = collect_params(depth_mean, mean_diff_fraction)
        _chk(_bind_collect(self._L).mcp_track_collect_nearest(self._h, graph._h, ctypes.byref(prm)), "track_collect_nearest")

    def collect_nearest_off(self):
        """tracker_collect_all_points = true (the default): every usable row."""
        _chk(_bind_collect(self._L).mcp_track_collect_nearest(self._h, None, None), "track_collect_nearest")

    def collect_last(self):
        """The CollectReport of the last find_pvs / track call on this table as a dict; raises unless that call succeeded with the mode on."""
        out = CollectReport()
        _chk(_bind_collect(self._L).mcp_track_collect_last(self._h, ctypes.byref(out)), "track_collect_last")
        return out.as_dict()

    def debug_fine_records(self):
        """(records (POSE_POINT_DTYPE), weights, mu_last) of the last track call's fine iterations, copied from the device; for tests."""
        from .keyframe import POSE_POINT_DTYPE
        L = _bind_track_cov(self._L)
        cap = max(MAX_FRAME_CAMS * max(self.rows, 1), 1)
        pts, w, mu, n = np.zeros(cap, dtype=POSE_POINT_DTYPE), np.zeros(cap), np.zeros(6), ctypes.c_int(0)
        _chk(L.mcp_debug_track_fine_records(self._h, cap, pts.ctypes.data, w.ctypes.data, mu.ctypes.data, ctypes.byref(n)), "debug_track_fine_records")
        return pts[:n.value].copy(), w[:n.value].copy(), mu

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


# ---- AdjustAndUpdate write-back (include/mcp_img.h mcp_ba_write_back) and its numpy restatement ----------------------------------------
WRITE_BACK_SYMBOLS = ["mcp_map_points_set_rays", "mcp_map_points_update_rays", "mcp_map_points_get", "mcp_scene_depth_robust", "mcp_ba_write_back", "mcp_map_points_last_timing"]


class SceneDepth(ctypes.Structure):
    _fields_ = [("mean", ctypes.c_double), ("sigma", ctypes.c_double), ("median", ctypes.c_double), ("sigma_sq", ctypes.c_double),
                ("n", ctypes.c_int), ("refreshed", ctypes.c_int)]


SCENE_DEPTH_DTYPE = np.dtype([("mean", "f8"), ("sigma", "f8"), ("median", "f8"), ("sigma_sq", "f8"), ("n", "i4"), ("refreshed", "i4")], align=True)
assert SCENE_DEPTH_DTYPE.itemsize == ctypes.sizeof(SceneDepth)


def _bind_write_back(L):
    if getattr(L, "_write_back_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_map_points_set_rays.argtypes = [vp, ip, ip, vp, vp, vp]
    L.mcp_map_points_update_rays.argtypes = [vp, ip, vp, vp, vp, vp]
    L.mcp_map_points_get.argtypes = [vp, ip, ip, vp, vp, vp, vp]
    L.mcp_scene_depth_robust.argtypes = [vp, ip, vp, vp, vp, vp, vp, vp]
    L.mcp_ba_write_back.argtypes = [vp, vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mcp_map_points_last_timing.argtypes = [vp, vp, vp, vp]
    L._write_back_bound = True
    return L


def _csr(seg_start, seg_rows, seg_weights):
    ss = np.ascontiguousarray(seg_start, dtype=np.int32)
    sr = np.ascontiguousarray(seg_rows, dtype=np.int32)
    sw = np.ascontiguousarray(seg_weights, dtype=np.float64)
    if len(sr) != len(sw):
        raise ValueError("seg_rows and seg_weights differ in length")
    return ss, sr, sw


def huber_sigma_squared(err_sq):
    """Huber::FindSigmaSquared (include/mcptam/MEstimator.h:194-204)."""
    e = np.sort(np.asarray(err_sq, dtype=np.float64))
    n = len(e)
    sigma = 1.4826 * (1 + 5.0 / (n * 2 - 6)) * math.sqrt(e[n // 2])
    sigma = 1.345 * sigma
    return sigma * sigma


def scene_depth_robust(depths, weights):
    """KeyFrame::RefreshSceneDepthRobust(vector&) (src/KeyFrame.cc:585-645) on one list, summing in the reference's order (the list sorted as
    std::pair<double, double> sorts).  Returns a dict with the fields of mcp_scene_depth; n <= 3: refreshed = 0 and nothing else."""
    d = np.asarray(depths, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    n = len(d)
    if n <= 3:
        return dict(n=n, refreshed=0)
    order = np.lexsort((w, d))
    d, w = d[order], w[order]
    median = float(d[n // 2])
    e2 = (d - median) * (d - median)
    sigma_sq = max(huber_sigma_squared(e2), 0.4)
    s_d = s_dd = s_w = 0.0
    for i in range(n):
        hw = math.sqrt(1.0 if e2[i] < sigma_sq else math.sqrt(sigma_sq / e2[i]))
        cw = float(w[i]) * hw
        s_d += cw * float(d[i])
        s_dd += cw * float(d[i]) * float(d[i])
        s_w += cw
    with np.errstate(all="ignore"):
        mean = float(np.float64(s_d) / np.float64(s_w))
        sigma = float(np.sqrt(np.float64(s_dd) / np.float64(s_w) - np.float64(mean) * np.float64(mean)))
    return dict(n=n, refreshed=1 if math.isfinite(mean) else -1, mean=mean, sigma=sigma, median=median, sigma_sq=sigma_sq)


def _mat3_vec(R, v):
    """R v for batches R (n, 3, 3), v (n, 3), every row summed left to right (no fused multiply-add, no BLAS): the device's order."""
    return np.stack([R[:, i, 0] * v[:, 0] + R[:, i, 1] * v[:, 1] + R[:, i, 2] * v[:, 2] for i in range(3)], axis=1)


def _mat3t_vec(R, v):
    return np.stack([R[:, 0, i] * v[:, 0] + R[:, 1, i] * v[:, 1] + R[:, 2, i] * v[:, 2] for i in range(3)], axis=1)


def chain_pose(poses):
    """Product of a chain of (R, t) poses as the solver composes it: starting from the identity, every link multiplied on from the left
    (CamFromBase * BaseFromWorld for {MKF, camera}), sums left to right -- the bits of the device's chain table."""
    R, t = np.eye(3), np.zeros(3)
    for Rk, tk in poses:
        Rk, tk = np.asarray(Rk, dtype=np.float64), np.asarray(tk, dtype=np.float64)
        Rn = np.array([[Rk[i, 0] * R[0, j] + Rk[i, 1] * R[1, j] + Rk[i, 2] * R[2, j] for j in range(3)] for i in range(3)])
        tn = np.array([(Rk[i, 0] * t[0] + Rk[i, 1] * t[1] + Rk[i, 2] * t[2]) + tk[i] for i in range(3)])
        R, t = Rn, tn
    return R, t


def write_back_point(x, own_pose, fixed, center_nc, one_right_nc, one_down_nc, src_pose=None):
    """The point step of AdjustAndUpdate (src/BundleAdjusterMulti.cc:307-319) for one point: world = own_pose^-1 * x (a fixed point: x), then
    MapPoint::RefreshPixelVectors at src_pose (default: own_pose) -- stereo.pixel_vectors.  Returns (world, pixel_right_w, pixel_down_w)."""
    from .stereo import pixel_vectors
    x = np.asarray(x, dtype=np.float64)
    Ro, to = own_pose
    world = x.copy() if fixed else Ro.T @ (x - to)
    pr, pd = pixel_vectors(own_pose if src_pose is None else src_pose, np.asarray(center_nc, dtype=np.float64), np.asarray(one_right_nc, dtype=np.float64),
                           np.asarray(one_down_nc, dtype=np.float64), world)
    return world, pr[0], pd[0]


def write_back_points(x, own_R, own_t, fixed, center_nc, one_right_nc, one_down_nc, src_R=None, src_t=None):
    """write_back_point for n points at once, in the device's order of operations (IEEE double, no contraction: the same bits): x (n, 3),
    own_R (n, 3, 3) / own_t (n, 3) the product of each point's own chain, fixed (n,), the rays (n, 3) each, src_R / src_t the pose
    RefreshPixelVectors uses (default: own).  Returns (world, pixel_right_w, pixel_down_w), (n, 3) each."""
    x = np.asarray(x, dtype=np.float64)
    fixed = np.asarray(fixed, dtype=bool)
    world = np.where(fixed[:, None], x, _mat3t_vec(own_R, x - own_t))
    Rs, ts = (own_R, own_t) if src_R is None else (src_R, src_t)
    h = np.abs((_mat3_vec(Rs, world) + ts)[:, 2])
    c = center_nc * h[:, None] / np.abs(center_nc[:, 2])[:, None]
    r = one_right_nc * h[:, None] / np.abs(one_right_nc[:, 2])[:, None] - c
    d = one_down_nc * h[:, None] / np.abs(one_down_nc[:, 2])[:, None] - c
    return world, _mat3t_vec(Rs, r), _mat3t_vec(Rs, d)


def scene_depths(cam_from_world, world_pos):
    """norm(CamFromWorld * mv3WorldPos) (src/KeyFrame.cc:561-567) for an (n, 3) array of positions."""
    R, t = cam_from_world
    w = np.asarray(world_pos, dtype=np.float64)
    xc = _mat3_vec(np.broadcast_to(R, (len(w), 3, 3)), w) + t
    return np.sqrt(xc[:, 0] * xc[:, 0] + xc[:, 1] * xc[:, 1] + xc[:, 2] * xc[:, 2])


# ---- TrackMap's bookkeeping (include/mcp_img.h mcp_track_map_record) and its numpy restatement -------------------------------------------
TRACK_RECORD_SYMBOLS = ["mcp_map_points_set_counts", "mcp_map_points_update_counts", "mcp_map_points_get_counts", "mcp_track_map_record",
                        "mcp_track_map_notes_view", "mcp_track_map_meas_view"]
TN_SEARCHED, TN_FOUND, TN_DID_SUBPIX, TN_TEMPLATE_BAD, TN_IN_IMAGE, TN_ATTEMPTED, TN_MARK_SHIFT = 1, 2, 4, 8, 16, 32, 6
MARK_NONE, MARK_INLIER, MARK_OUTLIER = 0, 1, 2
QUALITY_BAD, QUALITY_DODGY, QUALITY_GOOD = 0, 1, 2


class TrackRecordParams(ctypes.Structure):
    _fields_ = [("lost", ctypes.c_int), ("want_items", ctypes.c_int), ("min_patches", ctypes.c_int), ("coarse_min", ctypes.c_int),
                ("quality_good", ctypes.c_double), ("quality_bad", ctypes.c_double)]


class TrackNote(ctypes.Structure):
    _fields_ = [("row", ctypes.c_int), ("cam", ctypes.c_uint8), ("stage", ctypes.c_uint8), ("level", ctypes.c_uint8), ("flags", ctypes.c_uint8)]


class TrackMeas(ctypes.Structure):
    _fields_ = [("item", ctypes.c_int), ("row", ctypes.c_int), ("level", ctypes.c_int), ("subpix", ctypes.c_int), ("found_pos", ctypes.c_double * 2)]


class TrackRecord(ctypes.Structure):
    _fields_ = [("attempted", (ctypes.c_int * LEVELS) * MAX_FRAME_CAMS), ("found", (ctypes.c_int * LEVELS) * MAX_FRAME_CAMS),
                ("quality", ctypes.c_int * MAX_FRAME_CAMS), ("quality_max", ctypes.c_int), ("n_items", ctypes.c_int * MAX_FRAME_CAMS),
                ("n_meas", ctypes.c_int * MAX_FRAME_CAMS), ("n_inliers", ctypes.c_int), ("n_outlier_marks", ctypes.c_int),
                ("cam_from_world", (ctypes.c_double * 12) * MAX_FRAME_CAMS), ("depth", SceneDepth * MAX_FRAME_CAMS)]


TRACK_NOTE_DTYPE = np.dtype([("row", "i4"), ("cam", "u1"), ("stage", "u1"), ("level", "u1"), ("flags", "u1")], align=True)
TRACK_MEAS_DTYPE = np.dtype([("item", "i4"), ("row", "i4"), ("level", "i4"), ("subpix", "i4"), ("found_pos", "f8", 2)], align=True)
assert TRACK_NOTE_DTYPE.itemsize == ctypes.sizeof(TrackNote) == 8 and TRACK_MEAS_DTYPE.itemsize == ctypes.sizeof(TrackMeas) == 32


def _bind_track_record(L):
    if getattr(L, "_track_record_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_map_points_set_counts.argtypes = [vp, ip, ip, vp, vp]
    L.mcp_map_points_update_counts.argtypes = [vp, ip, vp, vp, vp]
    L.mcp_map_points_get_counts.argtypes = [vp, ip, ip, vp, vp]
    L.mcp_track_map_record.argtypes = [vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp]
    for f in (L.mcp_track_map_notes_view, L.mcp_track_map_meas_view):
        f.restype = vp
        f.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int)]
    L._track_record_bound = True
    return L


def _counts_arrays(inlier, outlier):
    i, o = np.ascontiguousarray(inlier, dtype=np.int32), np.ascontiguousarray(outlier, dtype=np.int32)
    if i.ndim != 1 or i.shape != o.shape:
        raise ValueError("counts: inlier and outlier must be 1-d arrays of one length")
    return i, o


def tracking_quality(attempted, found, min_patches, coarse_min, good, bad):
    """Tracker::AssessTrackingQuality (src/Tracker.cc:1618-1658) of one camera from its per-level counters: 0 BAD, 1 DODGY, 2 GOOD."""
    a, f = [int(v) for v in attempted], [int(v) for v in found]
    ta, tf, la, lf = sum(a), sum(f), sum(a[2:]), sum(f[2:])
    if tf < min_patches:
        return QUALITY_BAD
    with np.errstate(all="ignore"):                          # (0 / 0 is a NaN that passes neither test: DODGY, as in C++)
        total = np.float64(tf) / np.float64(ta)
        large = np.float64(lf) / np.float64(la) if la > coarse_min else total
    if total > good:
        return QUALITY_GOOD
    return QUALITY_BAD if large < bad else QUALITY_DODGY


def track_record_restate(items, counts_before, lost, ncam):
    """What mcp_track_map_record leaves behind, restated from the items of mcp_track_map (one TRACK_MAP_ITEM_DTYPE array per camera) and the
    count column before the call, counts_before = (inlier, outlier).  Returns a dict: notes, meas (per camera), attempted, found
    (MAX_FRAME_CAMS x LEVELS), n_items, n_meas, n_inliers, n_outlier_marks, counts = (inlier, outlier) after the marks, and the scene-depth
    lists seg_start (ncam + 1), seg_rows, seg_w -- camera c's found items in item order, weighted inlier / (inlier + outlier) after ALL
    marks of all cameras."""
    inl, outl = np.array(counts_before[0], dtype=np.int64), np.array(counts_before[1], dtype=np.int64)
    attempted, found = np.zeros((MAX_FRAME_CAMS, LEVELS), dtype=np.int32), np.zeros((MAX_FRAME_CAMS, LEVELS), dtype=np.int32)
    notes, meas, n_inliers, n_out = [], [], 0, 0
    for c in range(ncam):
        it = items[c]
        o = it["out"]
        level = o["search_level"].astype(np.int64)
        fnd, srch, bad = o["found"] != 0, o["searched"] != 0, o["template_bad"] != 0
        att = ~bad & (level >= 0)
        mark = np.where(fnd, np.where(it["weight_last"] == 0.0, MARK_OUTLIER, MARK_INLIER), np.where(srch & (not lost), MARK_OUTLIER, MARK_NONE))
        nt = np.zeros(len(it), dtype=TRACK_NOTE_DTYPE)
        nt["row"], nt["cam"], nt["stage"], nt["level"] = it["point"], c, it["stage"], level & 255
        nt["flags"] = (srch * TN_SEARCHED + fnd * TN_FOUND + (o["did_subpix"] != 0) * TN_DID_SUBPIX + bad * TN_TEMPLATE_BAD + (o["in_image"] != 0) * TN_IN_IMAGE +
                       att * TN_ATTEMPTED + (mark << TN_MARK_SHIFT)).astype(np.uint8)
        notes.append(nt)
        for l in range(LEVELS):
            attempted[c, l] = int((att & (level == l)).sum())
            found[c, l] = int((att & fnd & (level == l)).sum())
        np.add.at(inl, it["point"][mark == MARK_INLIER], 1)
        np.add.at(outl, it["point"][mark == MARK_OUTLIER], 1)
        n_inliers += int((mark == MARK_INLIER).sum())
        n_out += int((mark == MARK_OUTLIER).sum())
        k = np.nonzero(fnd)[0]
        ms = np.zeros(len(k), dtype=TRACK_MEAS_DTYPE)
        ms["item"], ms["row"], ms["level"], ms["subpix"], ms["found_pos"] = k, it["point"][k], level[k], o["did_subpix"][k] != 0, o["found_pos"][k]
        meas.append(ms)
    seg_start = np.concatenate([[0], np.cumsum([len(m_) for m_ in meas])]).astype(np.int32)
    seg_rows = np.concatenate([m_["row"] for m_ in meas] + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
    seg_w = inl[seg_rows].astype(np.float64) / (inl[seg_rows] + outl[seg_rows]).astype(np.float64)
    return dict(notes=notes, meas=meas, attempted=attempted, found=found, n_items=[len(items[c]) for c in range(ncam)], n_meas=[len(m_) for m_ in meas],
                n_inliers=n_inliers, n_outlier_marks=n_out, counts=(inl.astype(np.int32), outl.astype(np.int32)), seg_start=seg_start, seg_rows=seg_rows, seg_w=seg_w)


# ---- the tracker's motion model (include/mcp_img.h mcp_track_frame_motion) and its numpy restatement -------------------------------------
TRACK_MOTION_SYMBOLS = ["mcp_track_frame_motion", "mcp_track_motion_reset", "mcp_track_motion_get_sbi", "mcp_track_motion_prior_host",
                        "mcp_track_motion_update_host"]
MOTION_AVG_ROUNDS, MOTION_AVG_EPS = 32, 1e-3


class TrackMotionParams(ctypes.Structure):
    _fields_ = [("apply", ctypes.c_int), ("use_rotation_estimator", ctypes.c_int), ("sbi_iterations", ctypes.c_int), ("blur", ctypes.c_double),
                ("dt", ctypes.c_double), ("velocity", ctypes.c_double * 6), ("cam_good", ctypes.c_uint8 * MAX_FRAME_CAMS)]


class TrackMotion(ctypes.Structure):
    _fields_ = [("start", ctypes.c_double * 12), ("prior", ctypes.c_double * 12), ("se2", (ctypes.c_double * 6) * MAX_FRAME_CAMS),
                ("sbi_score", ctypes.c_double * MAX_FRAME_CAMS), ("cam_rot", (ctypes.c_double * 3) * MAX_FRAME_CAMS), ("sbi_rot", ctypes.c_double * 3),
                ("n_used", ctypes.c_int), ("avg_rounds", ctypes.c_int), ("first_frame", ctypes.c_int * MAX_FRAME_CAMS),
                ("v_new", ctypes.c_double * 6), ("velocity", ctypes.c_double * 6)]


def motion_params(velocity=None, dt=1.0 / 30, cam_good=None, apply=True, use_rotation_estimator=True, sbi_iterations=6, blur=0.75, ncam=MAX_FRAME_CAMS):
    """A TrackMotionParams; cam_good defaults to every one of the ncam cameras."""
    good = [1] * ncam if cam_good is None else [int(bool(g)) for g in cam_good]
    good = (good + [0] * MAX_FRAME_CAMS)[:MAX_FRAME_CAMS]
    v = np.zeros(6) if velocity is None else np.asarray(velocity, dtype=np.float64).reshape(6)
    return TrackMotionParams(int(bool(apply)), int(bool(use_rotation_estimator)), int(sbi_iterations), float(blur), float(dt), (ctypes.c_double * 6)(*v),
                             (ctypes.c_uint8 * MAX_FRAME_CAMS)(*good))


def _bind_track_motion(L):
    if getattr(L, "_track_motion_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_track_frame_motion.argtypes = [vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mcp_track_motion_reset.argtypes = [vp]
    L.mcp_track_motion_get_sbi.argtypes = [vp, ip, ip, vp, vp, vp]
    L.mcp_track_motion_prior_host.argtypes = [ip, vp, vp, vp, vp, vp, vp]
    L.mcp_track_motion_update_host.argtypes = [vp, vp, vp, vp]
    L._track_motion_bound = True
    return L


def motion_prior_host(se2, cams_sbi, cams_from_base, start, mp):
    """mcp_track_motion_prior_host: se2 (ncam, 6), cams_sbi: TaylorCameras (or a ctypes camera array), cams_from_base (ncam, 12), start: 12
    doubles, mp: TrackMotionParams.  Returns the TrackMotion it filled."""
    L = _bind_track_motion(lib())
    se2 = np.ascontiguousarray(se2, dtype=np.float64).reshape(-1, 6)
    css = cams_sbi if isinstance(cams_sbi, ctypes.Array) else camera_array(cams_sbi)
    cfb = np.ascontiguousarray(cams_from_base, dtype=np.float64).reshape(-1)
    st = np.ascontiguousarray(start, dtype=np.float64).reshape(12)
    out = TrackMotion()
    _chk(L.mcp_track_motion_prior_host(len(se2), se2.ctypes.data, ctypes.cast(css, ctypes.c_void_p), cfb.ctypes.data, st.ctypes.data, ctypes.byref(mp), ctypes.byref(out)),
         "track_motion_prior_host")
    return out


def motion_update_host(start, refined, mp):
    """mcp_track_motion_update_host: (v_new, velocity) from two poses of 12 doubles."""
    L = _bind_track_motion(lib())
    a, b = np.ascontiguousarray(start, dtype=np.float64).reshape(12), np.ascontiguousarray(refined, dtype=np.float64).reshape(12)
    out = TrackMotion()
    _chk(L.mcp_track_motion_update_host(a.ctypes.data, b.ctypes.data, ctypes.byref(mp), ctypes.byref(out)), "track_motion_update_host")
    return np.array(out.v_new), np.array(out.velocity)


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _abc(th):
    """sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3: series below 0.03 rad (the next term is under 1e-17), closed forms above."""
    t2 = th * th
    if th < 0.03:
        return (1 - t2 / 6 * (1 - t2 / 20 * (1 - t2 / 42)), 0.5 - t2 / 24 * (1 - t2 / 30 * (1 - t2 / 56)), 1.0 / 6 - t2 / 120 * (1 - t2 / 42 * (1 - t2 / 72)))
    A = math.sin(th) / th
    return A, 2 * math.sin(th / 2) ** 2 / t2, (1 - A) / t2


def so3_exp(w):
    """Rodrigues' formula, no truncation thresholds: I + A [w]x + B [w]x^2."""
    w = np.asarray(w, dtype=np.float64)
    A, B, _ = _abc(float(np.linalg.norm(w)))
    K = _hat(w)
    return np.eye(3) + A * K + B * (K @ K)


def se3_exp(mu):
    """(R, t) of the twist mu = [t; w]: R = exp(w), t = (I + B [w]x + C [w]x^2) mu_t."""
    mu = np.asarray(mu, dtype=np.float64)
    w = mu[3:]
    A, B, C = _abc(float(np.linalg.norm(w)))
    K = _hat(w)
    return np.eye(3) + A * K + B * (K @ K), (np.eye(3) + B * K + C * (K @ K)) @ mu[:3]


def so3_ln(R):
    """Axis-angle of a rotation matrix: the angle is atan2(|a|, (tr R - 1) / 2) with a the vector of the antisymmetric part; towards pi, where
    a vanishes, the axis is the largest column of R + I, signed by a."""
    R = np.asarray(R, dtype=np.float64)
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(a)), 0.5 * (np.trace(R) - 1.0)
    th = math.atan2(s, c)
    if s < 1e-4 and c > 0:
        return a * (1 + s * s / 6 * (1 + 9 * s * s / 20))          # asin(s) / s
    if s < 1e-4:
        S = 0.5 * (R + R.T) + np.eye(3)                              # (1 - cos t)(n n^T) + (1 + cos t) I, cos t ~ -1
        k = int(np.argmax(np.diag(S)))
        n = S[:, k] / np.linalg.norm(S[:, k])
        return th * (-n if n @ a < 0 else n)
    return a * (th / s)


def se3_ln(R, t):
    """The twist [t; w] with se3_exp = (R, t): w = so3_ln(R), mu_t = (I - [w]x / 2 + D [w]x^2) t, D = (1 - A / 2B) / |w|^2."""
    w = so3_ln(R)
    th = float(np.linalg.norm(w))
    if th < 0.03:
        D = 1.0 / 12 + th * th / 720 * (1 + th * th / 42)
    else:
        A, B, _ = _abc(th)
        D = (1 - A / (2 * B)) / (th * th)
    K = _hat(w)
    return np.concatenate([(np.eye(3) - 0.5 * K + D * (K @ K)) @ np.asarray(t, dtype=np.float64), w])


def average_rotation(rots, eps=MOTION_AVG_EPS, max_rounds=MOTION_AVG_ROUNDS):
    """Tracker::FindAverageRotation (src/Tracker.cc:1723-1749), the geodesic L2 mean of axis-angle rotations, ended after max_rounds
    evaluations of the mean residual at the latest.  Returns (mean, rounds)."""
    rots = [np.asarray(r, dtype=np.float64) for r in rots]
    R = so3_exp(rots[0])
    rounds = 0
    while rounds < max_rounds:
        r = sum(so3_ln(R.T @ so3_exp(q)) for q in rots) / len(rots)
        rounds += 1
        if r @ r < eps * eps:
            break
        R = R @ so3_exp(r)
    return so3_ln(R), rounds


def motion_prior(se2, cams_sbi, cams_from_base, start, velocity, dt, cam_good, apply=True, use_rotation_estimator=True, se3_from_se2=None):
    """Tracker::ApplyMotionModel with CalcSBIRotation (src/Tracker.cc:1516-1536, 1687-1721): se2 (ncam, 6) = the alignments [R row-major; t],
    cams_sbi: the 40x30 TaylorCameras, cams_from_base: (R, t) per camera, start: (R, t).  se3_from_se2(R2, t2, cam, cam) -> 3x3 rotation,
    default the library's host entry.  Returns dict(prior=(R, t), cam_rot (ncam, 3), sbi_rot, n_used, avg_rounds)."""
    if se3_from_se2 is None:
        from .keyframe import sbi_se3_from_se2 as se3_from_se2
    se2 = np.asarray(se2, dtype=np.float64).reshape(-1, 6)
    ncam = len(se2)
    cam_rot, used = np.zeros((ncam, 3)), []
    for c in range(ncam):
        if not (apply and use_rotation_estimator and cam_good[c]):
            continue
        if not np.array_equal(se2[c], [1, 0, 0, 1, 0, 0]):              # (an SBI against itself: exactly no rotation)
            Rc = se3_from_se2(se2[c, :4].reshape(2, 2), se2[c, 4:], cams_sbi[c], cams_sbi[c])
            cam_rot[c] = np.asarray(cams_from_base[c][0]).T @ so3_ln(Rc)
        used.append(cam_rot[c])
    Rs, ts = np.asarray(start[0], dtype=np.float64), np.asarray(start[1], dtype=np.float64)
    sbi_rot, rounds = (average_rotation(used) if used else (np.zeros(3), 0))
    if not apply:
        return dict(prior=(Rs.copy(), ts.copy()), cam_rot=cam_rot, sbi_rot=sbi_rot, n_used=len(used), avg_rounds=rounds)
    v6 = np.asarray(velocity, dtype=np.float64) * dt
    if used:
        v6[3:] = sbi_rot
    Re, te = se3_exp(v6)
    return dict(prior=(Re @ Rs, Re @ ts + te), cam_rot=cam_rot, sbi_rot=sbi_rot, n_used=len(used), avg_rounds=rounds)


def motion_update(start, refined, velocity, dt, apply=True):
    """Tracker::UpdateMotionModel (src/Tracker.cc:1539-1547): (v_new, velocity) from mse3StartPose and the refined pose, both (R, t)."""
    velocity = np.asarray(velocity, dtype=np.float64)
    if not apply:
        return np.zeros(6), velocity.copy()
    (Rs, ts), (Rr, tr) = start, refined
    Rd = np.asarray(Rr) @ np.asarray(Rs).T
    v_new = se3_ln(Rd, np.asarray(tr) - Rd @ np.asarray(ts)) / dt
    return v_new, 0.9 * (0.5 * v_new + 0.5 * velocity)


# ---- the lost branch: relocaliser + recovered pose (include/mcp_img.h mcp_track_frame_recover) and its numpy restatement ------------------
TRACK_RECOVER_SYMBOLS = ["mcp_track_frame_recover", "mcp_track_recover_pose_host"]
SCORE_SKIPPED = float(np.finfo(np.float64).max)      # DBL_MAX: the score of a skipped candidate, as mcp_sbi_score


class TrackRecoverParams(ctypes.Structure):
    _fields_ = [("reloc_blur", ctypes.c_double), ("reloc_iterations", ctypes.c_int), ("max_score", ctypes.c_double)]


class TrackRecover(ctypes.Structure):
    _fields_ = [("recovered", ctypes.c_int), ("cam", ctypes.c_int), ("best", ctypes.c_int * MAX_FRAME_CAMS), ("best_zmssd", ctypes.c_double * MAX_FRAME_CAMS),
                ("se2", (ctypes.c_double * 6) * MAX_FRAME_CAMS), ("align_score", ctypes.c_double * MAX_FRAME_CAMS),
                ("cam_pose", (ctypes.c_double * 12) * MAX_FRAME_CAMS), ("base_from_world", ctypes.c_double * 12)]


def _bind_track_recover(L):
    if getattr(L, "_track_recover_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_track_frame_recover.argtypes = [vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp]
    L.mcp_track_recover_pose_host.argtypes = [vp, vp, vp, vp, vp, vp]
    L._track_recover_bound = True
    return L


def _candidate_args(cand_kfs, cand_cams, cand_poses):
    """(ncand, handle array, camera indices int32, poses (ncand, 12) float64) of a candidate list; a keyframe may be a KeyFrame, None or a raw
    handle value."""
    n = len(cand_kfs)
    hs = (ctypes.c_void_p * max(n, 1))(*[k if k is None or isinstance(k, int) else k._h for k in cand_kfs])
    cc = np.ascontiguousarray(cand_cams, dtype=np.int32).reshape(-1)
    cp = cand_poses if isinstance(cand_poses, np.ndarray) else np.array([_pose12(*q) for q in cand_poses], dtype=np.float64).reshape(-1, 12)
    cp = np.ascontiguousarray(cp, dtype=np.float64).reshape(-1, 12)
    if len(cc) != n or len(cp) != n:
        raise ValueError("candidate list: %d keyframes, %d camera indices, %d poses" % (n, len(cc), len(cp)))
    if n == 0:
        cc, cp = np.zeros(1, dtype=np.int32), np.zeros((1, 12))
    return n, hs, cc, cp


def recover_pose_host(se2, cam_sbi, cam_from_world_best, cam_from_base):
    """mcp_track_recover_pose_host: se2 = 6 doubles [R row-major; t], cam_sbi: the 40x30 TaylorCamera, the two poses as 12 doubles.  Returns
    (cam_pose, base_from_world), 12 doubles each."""
    L = _bind_track_recover(lib())
    se2 = np.ascontiguousarray(se2, dtype=np.float64).reshape(6)
    k, c = np.ascontiguousarray(cam_from_world_best, dtype=np.float64).reshape(12), np.ascontiguousarray(cam_from_base, dtype=np.float64).reshape(12)
    cs = cam_sbi.to_struct()
    pose, bfw = np.zeros(12), np.zeros(12)
    _chk(L.mcp_track_recover_pose_host(se2.ctypes.data, ctypes.byref(cs), k.ctypes.data, c.ctypes.data, pose.ctypes.data, bfw.ctypes.data), "track_recover_pose_host")
    return pose, bfw


def zmssd(cur, other):
    """SmallBlurryImage::ZMSSD (src/SmallBlurryImage.cc:122-134): the float differences, squared and summed in double in raster order."""
    d = (np.asarray(cur, dtype=np.float32).ravel() - np.asarray(other, dtype=np.float32).ravel()).astype(np.float64)
    s = 0.0
    for v in d * d:
        s += v
    return s


def recover_restate(cur_templs, cand_templs, cand_cams, cand_poses, aligns, cams_sbi, cams_from_base, max_score=1e5, se3_from_se2=None, scores=None):
    """Relocaliser::ScoreKFs / AttemptRecovery and Tracker::AttemptRecovery (src/Relocaliser.cc:61-120, src/Tracker.cc:526-552) restated.
    cur_templs: the cameras' current templates; cand_templs: one template per candidate, None for a skipped one; cand_poses: (R, t) per
    candidate; aligns(c, best) -> (se2 as 6 doubles, score): the alignment of camera c against candidate best; cams_sbi: the 40x30
    TaylorCameras; cams_from_base: (R, t) per camera; se3_from_se2(R2, t2, cam, cam) -> 3x3 rotation, default the library's host entry;
    scores: taken as given instead of summed here.  Returns dict(scores, best, best_zmssd, se2, align_score, cam_pose [(R, t) or None],
    recovered, cam, base_from_world (R, t) or None)."""
    if se3_from_se2 is None:
        from .keyframe import sbi_se3_from_se2 as se3_from_se2
    ncam, ncand = len(cur_templs), len(cand_cams)
    if scores is None:
        scores = np.array([SCORE_SKIPPED if cand_templs[i] is None else zmssd(cur_templs[cand_cams[i]], cand_templs[i]) for i in range(ncand)])
    out = dict(scores=np.asarray(scores, dtype=np.float64), best=[-1] * ncam, best_zmssd=[0.0] * ncam, se2=np.zeros((ncam, 6)), align_score=[0.0] * ncam,
               cam_pose=[None] * ncam, recovered=False, cam=-1, base_from_world=None)
    for c in range(ncam):
        b = SCORE_SKIPPED
        for i in range(ncand):
            if cand_cams[i] == c and cand_templs[i] is not None and out["scores"][i] < b:      # strict: the first smallest
                b, out["best"][c] = out["scores"][i], i
        k = out["best"][c]
        if k < 0:
            continue
        se2, score = aligns(c, k)
        se2 = np.asarray(se2, dtype=np.float64).reshape(6)
        out["best_zmssd"][c], out["se2"][c], out["align_score"][c] = b, se2, score
        Rk, tk = np.asarray(cand_poses[k][0], dtype=np.float64), np.asarray(cand_poses[k][1], dtype=np.float64)
        Rr = np.eye(3) if np.array_equal(se2, [1, 0, 0, 1, 0, 0]) else se3_from_se2(se2[:4].reshape(2, 2), se2[4:], cams_sbi[c], cams_sbi[c])
        out["cam_pose"][c] = (Rr @ Rk, Rr @ tk)
        if not out["recovered"] and score < max_score:
            Rc, tc = np.asarray(cams_from_base[c][0], dtype=np.float64), np.asarray(cams_from_base[c][1], dtype=np.float64)
            Rp, tp = out["cam_pose"][c]
            out["recovered"], out["cam"], out["base_from_world"] = True, c, (Rc.T @ Rp, Rc.T @ (tp - tc))
    return out


# ---- the pose covariance of the last fine iteration (include/mcp_img.h mcp_track_pose_cov) and its numpy restatement ----------------------
TRACK_COV_SYMBOLS = ["mcp_track_pose_cov_enable", "mcp_track_pose_cov_last", "mcp_track_pose_cov", "mcp_track_pose_cov_host", "mcp_debug_track_fine_records"]
POSE_COV_MAX_SWEEPS, POSE_COV_PRIOR, POSE_COV_CONDITION = 16, 100.0, 1e9


class TrackPoseCov(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_int), ("n_used", ctypes.c_int), ("rank", ctypes.c_int), ("sweeps", ctypes.c_int), ("info", ctypes.c_double * 36),
                ("cov", ctypes.c_double * 36), ("eig", ctypes.c_double * 6), ("norm_fro", ctypes.c_double)]


def _bind_track_cov(L):
    if getattr(L, "_track_cov_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_track_pose_cov_enable.argtypes = [vp, ip]
    L.mcp_track_pose_cov_last.argtypes = [vp, vp]
    L.mcp_track_pose_cov.argtypes = [ip, vp, vp, ip, vp, vp, vp, ip, vp]
    L.mcp_track_pose_cov_host.argtypes = [ip, vp, vp, ip, vp, vp, vp, vp]
    L.mcp_debug_track_fine_records.argtypes = [vp, ip, vp, vp, vp, vp]
    L._track_cov_bound = True
    return L


def _cov_args(pts, weights, cams_from_base, refined, mu_last):
    from .keyframe import POSE_POINT_DTYPE
    pts = np.ascontiguousarray(pts, dtype=POSE_POINT_DTYPE)
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if len(w) != len(pts):
        raise ValueError("pose covariance: %d records, %d weights" % (len(pts), len(w)))
    cfb = np.ascontiguousarray(cams_from_base, dtype=np.float64).reshape(-1, 12) if isinstance(cams_from_base, np.ndarray) else \
        np.ascontiguousarray(np.stack([_pose12(*c) for c in cams_from_base]))
    ref = np.ascontiguousarray(refined, dtype=np.float64).reshape(12) if isinstance(refined, np.ndarray) else _pose12(*refined).copy()
    mu = np.ascontiguousarray(mu_last, dtype=np.float64).reshape(6)
    return pts, w, cfb, ref, mu


def pose_cov(pts, weights, cams_from_base, refined, mu_last, max_workgroups=0):
    """mcp_track_pose_cov on the GPU: records (POSE_POINT_DTYPE), one weight per record, CamFromBase per camera ((R, t) pairs or (ncam, 12)),
    the refined pose ((R, t) or 12 doubles) and the last update.  Returns the TrackPoseCov."""
    pts, w, cfb, ref, mu = _cov_args(pts, weights, cams_from_base, refined, mu_last)
    out = TrackPoseCov()
    _chk(_bind_track_cov(lib()).mcp_track_pose_cov(len(pts), pts.ctypes.data, w.ctypes.data, len(cfb), cfb.ctypes.data, ref.ctypes.data, mu.ctypes.data,
                                                   int(max_workgroups), ctypes.byref(out)), "track_pose_cov")
    return out


def pose_cov_host(pts, weights, cams_from_base, refined, mu_last):
    """mcp_track_pose_cov_host: the same source under the host compiler, in the device's order; needs no GPU."""
    pts, w, cfb, ref, mu = _cov_args(pts, weights, cams_from_base, refined, mu_last)
    out = TrackPoseCov()
    _chk(_bind_track_cov(lib()).mcp_track_pose_cov_host(len(pts), pts.ctypes.data, w.ctypes.data, len(cfb), cfb.ctypes.data, ref.ctypes.data, mu.ctypes.data,
                                                        ctypes.byref(out)), "track_pose_cov_host")
    return out


def pose_cov_arrays(rec):
    """(info 6x6, cov 6x6, eig) of a TrackPoseCov as numpy arrays."""
    return np.array(rec.info).reshape(6, 6), np.array(rec.cov).reshape(6, 6), np.array(rec.eig)


def pinv_truncated(info, condition=POSE_COV_CONDITION):
    """TooN SVD::get_pinv of a symmetric matrix: eigenvalue i is kept iff lambda_i * condition > lambda_max.  Returns (pinv, eigenvalues
    descending, rank)."""
    lam, V = np.linalg.eigh(np.asarray(info, dtype=np.float64))
    keep = lam * condition > lam.max()
    P = (V[:, keep] / lam[keep]) @ V[:, keep].T
    return 0.5 * (P + P.T), lam[::-1].copy(), int(keep.sum())


def pose_jacobian(world_pos, cam_derivs, cam_from_base, pose):
    """The 2 x 6 Jacobian of Tracker::CalcJacobian (TrackerData.h) at the pose (R, t): cam_derivs (2x2) * [dtheta; dphi] / d(xc) * Rc *
    [I | -[xb]x], twist order [t; w]."""
    R, t = pose
    Rc, tc = np.asarray(cam_from_base[0], dtype=np.float64), np.asarray(cam_from_base[1], dtype=np.float64)
    xb = np.asarray(R) @ np.asarray(world_pos, dtype=np.float64) + np.asarray(t)
    x, y, z = Rc @ xb + tc
    n2 = x * x + y * y
    n = math.sqrt(n2)
    S = np.zeros((2, 3))
    if n != 0.0:
        S[0] = [-z * x / (n * (n2 + z * z)), -z * y / (n * (n2 + z * z)), n / (n2 + z * z)]
        S[1] = [-y / n2, x / n2, 0.0]
    G = np.concatenate([np.eye(3), -_hat(xb)], axis=1)
    return np.asarray(cam_derivs, dtype=np.float64).reshape(2, 2) @ S @ Rc @ G


def pose_covariance_restate(pts, weights, cams_from_base, refined, mu_last, pose_before=None):
    """mm6PoseCovariance (src/Tracker.cc:1441, 1498-1502) in numpy: the pose before the last update as exp(-mu_last) * refined (or given),
    every found record's weighted Jacobian products summed with math.fsum, the prior 100 I, numpy.linalg.eigh with TooN's truncation.
    cams_from_base: (R, t) per camera.  Returns dict(info, cov, eig, rank, n_used, pose_before)."""
    if pose_before is None:
        Re, te = se3_exp(-np.asarray(mu_last, dtype=np.float64))
        Rr, tr = np.asarray(refined[0], dtype=np.float64), np.asarray(refined[1], dtype=np.float64)
        pose_before = (Re @ Rr, Re @ tr + te)
    terms = [[[] for _ in range(6)] for _ in range(6)]
    n_used = 0
    for p, w in zip(pts, weights):
        if not p["found"] or w == 0.0:
            continue
        n_used += 1
        J = float(p["sqrt_inv_noise"]) * pose_jacobian(p["world_pos"], p["cam_derivs"], cams_from_base[int(p["cam"])], pose_before)
        for r in range(2):
            for x in range(6):
                for y in range(x + 1):
                    terms[x][y].append(float(w) * J[r, x] * J[r, y])
    info = np.zeros((6, 6))
    for x in range(6):
        for y in range(x + 1):
            info[x, y] = info[y, x] = math.fsum(terms[x][y]) + (POSE_COV_PRIOR if x == y else 0.0)
    if not np.all(np.isfinite(info)):
        return dict(info=info, cov=np.zeros((6, 6)), eig=np.zeros(6), rank=0, n_used=n_used, pose_before=pose_before, valid=-1)
    cov, eig, rank = pinv_truncated(info)
    return dict(info=info, cov=cov, eig=eig, rank=rank, n_used=n_used, pose_before=pose_before, valid=1)


# ---- the co-visible points of the nearest keyframe (include/mcp_img.h mcp_map_collect_nearest, mcp_track_collect_nearest) ------------------
COLLECT_SYMBOLS = ["mcp_map_collect_nearest", "mcp_map_collect_rows_view", "mcp_map_collect_last_timing", "mcp_map_collect_nearest_host", "mcp_track_collect_nearest",
                   "mcp_track_collect_last"]


class CollectParams(ctypes.Structure):
    _fields_ = [("mean_diff_fraction", ctypes.c_double), ("depth_mean", ctypes.c_double * MAX_FRAME_CAMS), ("active", ctypes.c_uint8 * MAX_FRAME_CAMS)]


class CollectReport(ctypes.Structure):
    _fields_ = [("valid", ctypes.c_int), ("status", ctypes.c_int * MAX_FRAME_CAMS), ("nearest_slot", ctypes.c_int * MAX_FRAME_CAMS), ("nearest_cam", ctypes.c_int * MAX_FRAME_CAMS),
                ("pad_", ctypes.c_int), ("nearest_dist", ctypes.c_double * MAX_FRAME_CAMS)] + \
               [(k, ctypes.c_int * MAX_FRAME_CAMS) for k in ("n_candidates", "n_seed_rows", "n_kfs", "n_rows")]

    def as_dict(self):
        """valid as an int, every other field as an array of MAX_FRAME_CAMS."""
        out = {k: np.array(getattr(self, k)) for k, _ in self._fields_ if k not in ("valid", "pad_")}
        out["valid"] = int(self.valid)
        return out


COLLECT_STRUCT_SIZES = {"mcp_collect_params": ctypes.sizeof(CollectParams), "mcp_collect_report": ctypes.sizeof(CollectReport)}


def collect_params(depth_mean, mean_diff_fraction=0.5, active=None):
    """mcp_collect_params: one depth mean per camera looked at; active (the stand-alone call): which of them, None for all."""
    d = np.asarray(depth_mean, dtype=np.float64).reshape(-1)
    use = np.ones(len(d), dtype=bool) if active is None else np.asarray(active).reshape(-1) != 0
    if len(d) > MAX_FRAME_CAMS or len(use) != len(d):
        raise ValueError("collect_params: one depth mean and one active byte per camera, at most %d" % MAX_FRAME_CAMS)
    p = CollectParams(float(mean_diff_fraction))
    for c in range(len(d)):
        p.depth_mean[c], p.active[c] = d[c], int(use[c])
    return p


def _bind_collect(L):
    if getattr(L, "_collect_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_map_collect_nearest.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mcp_map_collect_rows_view.restype = vp
    L.mcp_map_collect_rows_view.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L.mcp_map_collect_last_timing.argtypes = [vp, vp]
    L.mcp_map_collect_nearest_host.argtypes = [vp, vp, vp, ip, vp, ip, vp, vp, vp, vp, ip, ip, vp, vp, vp, vp, vp, vp]
    L.mcp_track_collect_nearest.argtypes = [vp, vp, vp]
    L.mcp_track_collect_last.argtypes = [vp, vp]
    L._collect_bound = True
    return L
