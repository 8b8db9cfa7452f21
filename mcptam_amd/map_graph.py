"""ctypes binding of the device-resident map graph (include/mcp_img.h: mcp_map_graph_*, mcp_map_bundle_select): the MKF slots, the rig, the
per-point graph columns and the measurement store next to a MapPointTable, and the one call that runs BundleAdjusterBase::BundleAdjustRecent /
BundleAdjustAll on it and returns the arrays BundleAdjusterMulti::BundleAdjust populates its ChainBundle from.

MapGraph is the class over the ABI; problem_arrays turns a multi-mode synth.Problem into the flat arrays every layer takes (slots = MKF
indices, rows = point indices); bundle_select_host is mcp_map_bundle_select_host (no device); bundle_select_ref is the numpy restatement,
written from the reference (src/BundleAdjusterBase.cc:141-265, src/BundleAdjusterMulti.cc:81-200, src/KeyFrame.cc:715-747, 903-927);
selection_problem makes the synth.Problem a selection describes, which Problem.populate replays into a ChainBundle as it is.

The keyframe lists of AdjustAndUpdate's write-back come from the same store (mcp_graph_*): MapGraph.debug_kf_lists / refresh_depth / write_back
on the device, kf_lists_host (mcp_graph_kf_lists_host, no device) and kf_lists_ref, the numpy restatement (src/KeyFrame.cc:549-570, 851-869).

Measurement parcels (mcp_meas_parcel_*) feed the store from the device: MeasParcel takes the measurements of a track call, a ReFind or the
caller into device memory with the keys of their rows, MapGraph.commit_parcel appends the ones that are still good when the map maker gets to
them; parcel_commit_host (mcp_parcel_commit_host, no device) and parcel_commit_ref, the numpy restatement (src/Tracker.cc:1237-1274,
src/MapMaker.cc:407-418), state the verdicts.

Outliers and bad points (mcp_map_cull_*): MapGraph.cull_outliers is MapMakerServerBase::HandleOutliers over the store, MapGraph.cull_sweep the
point half of MapMaker::HandleBadEntities (danglers, tracker outliers, the bad points' measurements erased, their rows unusable, the rows the
device turned bad reported); cull_outliers_host / cull_sweep_host are the host twins (no device) and cull_outliers_ref / cull_sweep_ref the
numpy restatements (src/MapMakerServerBase.cc:1198-1238, src/MapMakerClientBase.cc:73-108, src/Map.cc:93-116).

Closest-keyframe queries and the removal of an MKF (mcp_map_neighbours, mcp_map_mkf_cull): MapGraph.neighbours is the one call behind
closest_multi_keyframe, n_closest_multi_keyframes, furthest_multi_keyframe, closest_keyframe, closest_keyframes_within_dist and
n_closest_keyframes (src/MapMakerBase.cc:90-339) and the tracker's need_new_multi_keyframe / is_distance_to_nearest_mkf_excessive
(src/MapMakerClientBase.cc:111-226); MapGraph.cull_mkf is MarkFurthestMultiKeyFrameAsBad with the MKF half of HandleBadEntities
(src/MapMakerServerBase.cc:264-318, src/Map.cc:119-187); neighbours_host / cull_mkf_host are the host twins (no device), neighbours_ref /
cull_mkf_ref the numpy restatements.

The co-visible points of the nearest keyframe (mcp_map_collect_nearest): MapGraph.collect_nearest is Tracker::CollectNearestPoints with
tracker_collect_all_points false (src/Tracker.cc:1797-1854) for every camera of a frame at once -- a byte per row whose bit c is camera c's;
pvs.MapPointTable.collect_nearest switches the same walk on in front of the PVS launch of find_pvs and the one-call frames;
collect_nearest_host is the host twin (no device), collect_nearest_ref the restatement over sets of keyframes and points.

How the map begins and how it is rescaled or moved (mcp_init_depth_map_points, mcp_map_mark_optimized, mcp_map_rescale, mcp_map_transform):
MapGraph.add_init_depth_points is MapMakerServerBase::AddInitDepthMapPoints of one MKF and level for every camera of the rig, mark_optimized the
mbOptimized loop at the end of InitFromMultiKeyFrame, rescale / transform ApplyGlobalScaleToMap / ApplyGlobalTransformationToMap over the resident
map (src/MapMakerServerBase.cc:212-215, 499-596); init_depth_host / mark_optimized_host / map_transform_host are the host twins (no device),
init_depth_ref / mark_optimized_ref / map_transform_ref the numpy restatements."""
import ctypes

import numpy as np

from . import chain_bundle as _cb
from . import synth
from .keyframe import _chk
from .pvs import lib as _pvs_lib
from .pvs import COLLECT_STRUCT_SIZES, COLLECT_SYMBOLS, CollectParams, CollectReport, _bind_collect, collect_params

MAX_MKFS = 4096
MAX_CAMS = 8
MKF_PRESENT, MKF_FIXED, MKF_BAD = 1, 2, 4
GP_FIXED, GP_BAD = 1, 2
BUNDLE_ALL, BUNDLE_RECENT = 0, 1
SRC_ROOT = 2          # Measurement::eSource values (include/mcptam/KeyFrame.h): stored and returned, not interpreted
SRC_TRACKER = 0


class SelectParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("newest", ctypes.c_int), ("n_recent", ctypes.c_int), ("recent_min_size", ctypes.c_int),
                ("min_points", ctypes.c_int), ("mean_diff_fraction", ctypes.c_double)]


class SelectResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("n_adjust", ctypes.c_int), ("n_fixed", ctypes.c_int), ("n_points", ctypes.c_int), ("n_meas", ctypes.c_int),
                ("has_fixed_points", ctypes.c_int), ("n_dropped_source", ctypes.c_int), ("closest", ctypes.c_int * 8), ("closest_dist", ctypes.c_double * 8)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_[:7]}
        d["closest"] = [int(v) for v in self.closest]
        d["closest_dist"] = [float(v) for v in self.closest_dist]
        return d


MKF_DTYPE = np.dtype([("slot", "i4"), ("fixed", "i4")], align=True)
POINT_DTYPE = np.dtype([("x", "f8", 3), ("row", "i4"), ("src_mkf", "i4"), ("src_cam", "i4"), ("fixed", "i4")], align=True)
MEAS_DTYPE = np.dtype([("uv", "f8", 2), ("mkf", "i4"), ("cam", "i4"), ("point", "i4"), ("level", "i4"), ("source", "i4"), ("store", "i4")], align=True)
STRUCT_SIZES = {"mcp_bundle_select_params": ctypes.sizeof(SelectParams), "mcp_bundle_select_result": ctypes.sizeof(SelectResult),
                "mcp_bundle_mkf": MKF_DTYPE.itemsize, "mcp_bundle_point": POINT_DTYPE.itemsize, "mcp_bundle_meas": MEAS_DTYPE.itemsize}

GRAPH_SYMBOLS = [
    "mcp_map_graph_create", "mcp_map_graph_destroy", "mcp_map_graph_set_mkfs", "mcp_map_graph_update_mkfs", "mcp_map_graph_update_points",
    "mcp_map_graph_add_meas", "mcp_map_graph_erase_meas", "mcp_map_graph_erase_mkf", "mcp_map_graph_compact", "mcp_map_graph_num_meas",
    "mcp_map_graph_get_meas", "mcp_map_graph_good_counts", "mcp_map_graph_check", "mcp_map_bundle_select", "mcp_map_bundle_mkfs_view",
    "mcp_map_bundle_points_view", "mcp_map_bundle_meas_view", "mcp_map_bundle_select_host", "mcp_map_bundle_select_last_timing",
]

GRAPH_LIST_SYMBOLS = ["mcp_graph_refresh_depth", "mcp_graph_write_back", "mcp_graph_debug_kf_lists", "mcp_graph_kf_lists_host", "mcp_graph_get_mkfs"]
LIST_BLOCK, LIST_MAX_BLOCKS = 256, 64          # map_graph_lists.h: entries of a tile, chunks at the most (the default grid: one tile per chunk up to that)

# measurement parcels (include/mcp_img.h mcp_meas_parcel_*, map_graph_parcel.h)
PARCEL_SYMBOLS = ["mcp_meas_parcel_create", "mcp_meas_parcel_destroy", "mcp_meas_parcel_from_track", "mcp_meas_parcel_from_refind", "mcp_meas_parcel_from_host",
                  "mcp_meas_parcel_size", "mcp_meas_parcel_get", "mcp_meas_parcel_commit", "mcp_parcel_commit_host"]
PARCEL_APPENDED, PARCEL_SKIPPED, PARCEL_STALE, PARCEL_BAD, PARCEL_CROSS = range(5)
PARCEL_BLOCK = 256                            # map_graph_parcel.h: entries of a workgroup
SRC_REFIND = 1                                # Measurement::eSource (include/mcptam/KeyFrame.h): SRC_TRACKER, SRC_REFIND, SRC_ROOT, SRC_TRAIL, SRC_EPIPOLAR
PARCEL_ENTRY_DTYPE = np.dtype([("uv", "f8", 2), ("lane", "i4"), ("row", "i4"), ("key", "i4"), ("level", "i4")], align=True)
STORE_ENTRY_DTYPE = np.dtype([("uv", "f8", 2), ("mkf", "i4"), ("cam", "i4"), ("row", "i4"), ("level", "i4"), ("source", "i4"), ("alive", "i4")], align=True)


class ParcelCommitParams(ctypes.Structure):
    _fields_ = [("cross_camera", ctypes.c_int), ("source", ctypes.c_int)]


class ParcelCommitResult(ctypes.Structure):
    _fields_ = [("first", ctypes.c_int), ("n_appended", ctypes.c_int), ("n_skipped_lane", ctypes.c_int), ("n_stale", ctypes.c_int), ("n_bad", ctypes.c_int),
                ("n_cross", ctypes.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


PARCEL_STRUCT_SIZES = {"mcp_parcel_entry": PARCEL_ENTRY_DTYPE.itemsize, "mcp_store_entry": STORE_ENTRY_DTYPE.itemsize,
                       "mcp_parcel_commit_params": ctypes.sizeof(ParcelCommitParams), "mcp_parcel_commit_result": ctypes.sizeof(ParcelCommitResult)}

# outliers and bad points (include/mcp_img.h mcp_map_cull_*, map_graph_cull.h)
CULL_SYMBOLS = ["mcp_map_cull_outliers", "mcp_map_cull_sweep", "mcp_map_cull_rows_view", "mcp_map_cull_last_timing", "mcp_map_cull_outliers_host",
                "mcp_map_cull_sweep_host"]
SRC_TRAIL, SRC_EPIPOLAR = 3, 4
CULL_MISSING, CULL_FIXED, CULL_POINT_BAD, CULL_RETRY, CULL_NEVER_RETRY, CULL_ALREADY_BAD = range(6)
CULL_BLOCK = 256                              # map_graph_cull.h: keys, rows or entries of a workgroup


class CullOutliersParams(ctypes.Structure):
    _fields_ = [("bad_good_count", ctypes.c_int)]


class CullOutliersResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("n_missing", "n_fixed", "n_point_bad", "n_retry", "n_never_retry", "n_already_bad", "n_fixed_rows", "n_rows_marked")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CullSweepParams(ctypes.Structure):
    _fields_ = [("min_outliers", ctypes.c_int), ("danglers", ctypes.c_int), ("outlier_multiplier", ctypes.c_double)]


class CullSweepResult(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("n_danglers", "n_tracker_outliers", "n_reported", "n_bad_rows", "n_meas_erased")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


CULL_STRUCT_SIZES = {"mcp_cull_outliers_params": ctypes.sizeof(CullOutliersParams), "mcp_cull_outliers_result": ctypes.sizeof(CullOutliersResult),
                     "mcp_cull_sweep_params": ctypes.sizeof(CullSweepParams), "mcp_cull_sweep_result": ctypes.sizeof(CullSweepResult)}

# closest-keyframe queries and the removal of an MKF (include/mcp_img.h mcp_map_neighbours, mcp_map_mkf_cull; map_graph_neigh.h)
NEIGH_SYMBOLS = ["mcp_map_neighbours", "mcp_map_neighbours_last_timing", "mcp_map_neighbours_host", "mcp_map_mkf_cull", "mcp_map_mkf_cull_last_timing",
                 "mcp_map_mkf_cull_host"]
NB_MKF, NB_KF = 0, 1
NB_ALL, NB_ONLY_SELF, NB_ONLY_OTHER = 0, 1, 2
NB_NEAREST, NB_FURTHEST = 0, 1
NB_MAX = 32
NEIGH_BLOCK = 256                             # map_graph_neigh.h: candidates or entries of a workgroup
DBL_MAX = float(np.finfo(np.float64).max)
NEIGH_ITEM_DTYPE = np.dtype([("dist", "f8"), ("slot", "i4"), ("cam", "i4"), ("flags", "i4"), ("n_meas", "i4")], align=True)


class NeighParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("kind", "region", "order", "src_slot", "src_cam", "same_cam", "n_max", "want_meas")] + \
               [("max_dist", ctypes.c_double), ("mean_diff_fraction", ctypes.c_double), ("ext_base_from_world", ctypes.c_double * 12),
                ("ext_active", ctypes.c_uint8 * MAX_CAMS), ("ext_depth_mean", ctypes.c_double * MAX_CAMS)]


class NeighItem(ctypes.Structure):
    _fields_ = [("dist", ctypes.c_double), ("slot", ctypes.c_int), ("cam", ctypes.c_int), ("flags", ctypes.c_int), ("n_meas", ctypes.c_int)]


class NeighResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("count", ctypes.c_int), ("n_candidates", ctypes.c_int), ("pad_", ctypes.c_int), ("item", NeighItem * NB_MAX)]

    def as_dict(self):
        return dict(status=int(self.status), count=int(self.count), n_candidates=int(self.n_candidates))

    def items(self):
        """The `count` winners as a NEIGH_ITEM_DTYPE array (a copy)."""
        return np.frombuffer(bytes(self), dtype=NEIGH_ITEM_DTYPE, offset=NeighResult.item.offset)[:self.count].copy()


class MkfCullParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("slot", "furthest_from", "mark_points", "max_kfs", "erase")] + [("mean_diff_fraction", ctypes.c_double)]


class MkfCullResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("victim", ctypes.c_int), ("victim_dist_valid", ctypes.c_int), ("victim_dist", ctypes.c_double)] + \
               [(k, ctypes.c_int) for k in ("n_victim_meas", "n_rows_marked", "n_by_count", "n_by_source", "new_fixed", "n_meas_erased")]

    def as_dict(self):
        return {k: (float if k == "victim_dist" else int)(getattr(self, k)) for k, _ in self._fields_}


NEIGH_STRUCT_SIZES = {"mcp_neigh_params": ctypes.sizeof(NeighParams), "mcp_neigh_item": ctypes.sizeof(NeighItem), "mcp_neigh_result": ctypes.sizeof(NeighResult),
                      "mcp_mkf_cull_params": ctypes.sizeof(MkfCullParams), "mcp_mkf_cull_result": ctypes.sizeof(MkfCullResult)}
assert NEIGH_ITEM_DTYPE.itemsize == ctypes.sizeof(NeighItem)

_BOUND = False


def lib():
    global _BOUND
    L = _pvs_lib()
    if not _BOUND:
        vp, ip = ctypes.c_void_p, ctypes.c_int
        L.mcp_map_graph_create.restype = vp
        L.mcp_map_graph_create.argtypes = [vp, ip, vp]
        L.mcp_map_graph_destroy.argtypes = [vp]
        L.mcp_map_graph_set_mkfs.argtypes = [vp, ip, ip, vp, vp, vp, vp]
        L.mcp_map_graph_update_mkfs.argtypes = [vp, ip, vp, vp, vp, vp, vp]
        L.mcp_map_graph_update_points.argtypes = [vp, ip, vp, vp, vp, vp]
        L.mcp_map_graph_add_meas.argtypes = [vp, ip, vp, vp, vp, vp, vp, vp]
        L.mcp_map_graph_erase_meas.argtypes = [vp, ip, vp, vp, vp]
        L.mcp_map_graph_erase_mkf.argtypes = [vp, ip]
        L.mcp_map_graph_compact.argtypes = [vp]
        L.mcp_map_graph_num_meas.argtypes = [vp, vp, vp]
        L.mcp_map_graph_get_meas.argtypes = [vp, ip, ip, vp, vp, vp, vp, vp, vp, vp]
        L.mcp_map_graph_good_counts.argtypes = [vp, ip, ip, vp]
        L.mcp_map_graph_check.argtypes = [vp, vp, vp]
        L.mcp_map_bundle_select.argtypes = [vp, vp, vp]
        L.mcp_map_bundle_select_last_timing.argtypes = [vp, vp]
        for f in (L.mcp_map_bundle_mkfs_view, L.mcp_map_bundle_points_view, L.mcp_map_bundle_meas_view):
            f.restype = vp
            f.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        L.mcp_map_bundle_select_host.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, ip, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, ip, vp, ip, vp, ip, vp]
        L.mcp_graph_refresh_depth.argtypes = [vp, ip, vp, vp]
        L.mcp_graph_write_back.argtypes = [vp, vp, ip, vp, vp, vp, ip, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp]
        L.mcp_graph_debug_kf_lists.argtypes = [vp, ip, vp, ip, vp, ip, vp, vp]
        L.mcp_graph_get_mkfs.argtypes = [vp, ip, ip, vp, vp, vp, vp]
        L.mcp_graph_kf_lists_host.argtypes = [ip, ip, vp, vp, ip, ip, vp, vp, vp, ip, vp, vp, vp, vp, ip, vp, vp, ip, vp, vp]
        L.mcp_meas_parcel_create.restype = vp
        L.mcp_meas_parcel_create.argtypes = [vp]
        L.mcp_meas_parcel_destroy.argtypes = [vp]
        L.mcp_meas_parcel_from_track.argtypes = [vp]
        L.mcp_meas_parcel_from_refind.argtypes = [vp]
        L.mcp_meas_parcel_from_host.argtypes = [vp, ip, vp, vp, vp, vp]
        L.mcp_meas_parcel_size.argtypes = [vp]
        L.mcp_meas_parcel_get.argtypes = [vp, ip, vp]
        L.mcp_meas_parcel_commit.argtypes = [vp, vp, ip, vp, vp, vp, vp, vp]
        L.mcp_parcel_commit_host.argtypes = [ip, vp, ip, vp, ip, vp, vp, vp, ip, vp, vp, vp, ip, vp, vp, vp, vp]
        L.mcp_map_cull_outliers.argtypes = [vp, ip, vp, vp, vp, vp, vp, vp]
        L.mcp_map_cull_sweep.argtypes = [vp, vp, vp]
        L.mcp_map_cull_rows_view.restype = vp
        L.mcp_map_cull_rows_view.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
        L.mcp_map_cull_last_timing.argtypes = [vp, vp, vp]
        L.mcp_map_cull_outliers_host.argtypes = [ip, vp, vp, vp, vp, ip, ip, vp, ip, ip, vp, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp]
        L.mcp_map_cull_sweep_host.argtypes = [vp, ip, vp, ip, ip, vp, vp, vp, vp, vp, ip, vp, vp, vp, vp, ip, vp]
        L.mcp_map_neighbours.argtypes = [vp, vp, vp]
        L.mcp_map_neighbours_last_timing.argtypes = [vp, vp]
        L.mcp_map_neighbours_host.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, ip, vp, vp, vp, vp]
        L.mcp_map_mkf_cull.argtypes = [vp, vp, vp]
        L.mcp_map_mkf_cull_last_timing.argtypes = [vp, vp]
        L.mcp_map_mkf_cull_host.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, ip, ip, vp, vp, vp, vp, ip, vp, vp, vp, vp, vp]
        _BOUND = True
    return L


def select_params(mode=BUNDLE_RECENT, newest=-1, n_recent=3, recent_min_size=8, min_points=10, mean_diff_fraction=0.5):
    """BundleAdjusterBase's statics (snRecentNum, snRecentMinSize, snMinMapPoints) and KeyFrame::sdDistanceMeanDiffFraction at their defaults."""
    return SelectParams(int(mode), int(newest), int(n_recent), int(recent_min_size), int(min_points), float(mean_diff_fraction))


def _i32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if shape is not None and a.shape != shape:
        raise ValueError("expected shape %s, got %s" % (shape, a.shape))
    return a


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError("expected shape %s, got %s" % (shape, a.shape))
    return a


def _u8(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a) != 0, dtype=np.uint8)
    if shape is not None and a.shape != shape:
        raise ValueError("expected shape %s, got %s" % (shape, a.shape))
    return a


def poses12(R, t):
    """(n, 3, 3), (n, 3) -> (n, 12): R row-major then t."""
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([R.reshape(-1, 9), t.reshape(-1, 3)], axis=1))


# ---- a Problem as the graph's flat arrays ------------------------------------------------------------------------------------------------
def _compose(Ra, ta, Rb, tb):
    """(Ra Rb, Ra tb + ta) over leading axes, each sum written out left to right."""
    R = Ra[..., :, 0, None] * Rb[..., None, 0, :] + Ra[..., :, 1, None] * Rb[..., None, 1, :] + Ra[..., :, 2, None] * Rb[..., None, 2, :]
    t = Ra[..., :, 0] * tb[..., None, 0] + Ra[..., :, 1] * tb[..., None, 1] + Ra[..., :, 2] * tb[..., None, 2]
    return R, t + ta


def _apply(R, t, v):
    return R[..., :, 0] * v[..., None, 0] + R[..., :, 1] * v[..., None, 1] + R[..., :, 2] * v[..., None, 2] + t


def problem_arrays(p, depth_mean=None):
    """The flat arrays of a multi-mode synth.Problem: MKF columns (every MKF present, base_fixed as MCP_MKF_FIXED, every keyframe active),
    the rig, point columns with world positions computed from pt_x (CamFromWorld_src^-1 * pt_x; a fixed point's pt_x is its world position),
    the measurements in the Problem's order, all alive, the first measurement of a point from its source keyframe marked SRC_ROOT.
    depth_mean: (P, C) or None for the mean depth of the points each keyframe measures (1 where it measures none)."""
    assert p.mode == "multi"
    P, C, N, M = p.n_mkf, len(p.cams), p.n_points, p.n_meas
    a = dict(ncam=C, cam_from_base=poses12(p.cam_R, p.cam_t), base_from_world=poses12(p.base_R, p.base_t))
    a["mkf_flags"] = (MKF_PRESENT | np.where(np.asarray(p.base_fixed, dtype=bool), MKF_FIXED, 0)).astype(np.int32)
    a["kf_active"] = np.ones((P, C), dtype=np.uint8)
    fx = np.asarray(p.pt_fixed, dtype=bool)
    sm, sc = p.pt_src[:, 0].astype(np.int64), p.pt_src[:, 1].astype(np.int64)
    Rs, ts = _compose(p.cam_R[sc], p.cam_t[sc], p.base_R[sm], p.base_t[sm])
    world = np.einsum("nji,nj->ni", Rs, p.pt_x - ts)
    world[fx] = p.pt_x[fx]
    a["world_pos"] = np.ascontiguousarray(world)
    a["src_mkf"] = np.where(fx, -1, sm).astype(np.int32)
    a["src_cam"] = np.where(fx, 0, sc).astype(np.int32)
    a["pt_flags"] = np.where(fx, GP_FIXED, 0).astype(np.int32)
    a["ms_mkf"], a["ms_cam"], a["ms_row"] = _i32(p.ms_mkf), _i32(p.ms_cam), _i32(p.ms_pt)
    a["ms_uv"], a["ms_level"] = _f64(p.ms_uv), _i32(p.ms_level)
    root = (p.ms_mkf == p.pt_src[p.ms_pt, 0]) & (p.ms_cam == p.pt_src[p.ms_pt, 1]) & ~fx[p.ms_pt]
    a["ms_source"] = np.where(root, SRC_ROOT, SRC_TRACKER).astype(np.int32)
    a["ms_alive"] = np.ones(M, dtype=np.uint8)
    if depth_mean is None:
        Rk, tk = _compose(p.cam_R[p.ms_cam], p.cam_t[p.ms_cam], p.base_R[p.ms_mkf], p.base_t[p.ms_mkf])
        z = np.abs(_apply(Rk, tk, world[p.ms_pt])[:, 2])
        key = p.ms_mkf.astype(np.int64) * C + p.ms_cam
        s = np.bincount(key, weights=z, minlength=P * C)
        n = np.bincount(key, minlength=P * C)
        depth_mean = np.where(n > 0, s / np.maximum(n, 1), 1.0).reshape(P, C)
        depth_mean = np.where(depth_mean > 0, depth_mean, 1.0)
    a["kf_depth_mean"] = _f64(depth_mean, (P, C))
    return a


def copy_arrays(a):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


# ---- mcp_map_bundle_select_host ------------------------------------------------------------------------------------------------------------
def bundle_select_host(a, params):
    """mcp_map_bundle_select_host over the flat arrays `a` (problem_arrays' keys): (SelectResult, mkfs, points, meas) with the views as
    structured arrays (MKF_DTYPE, POINT_DTYPE, MEAS_DTYPE).  Needs no device.  A refusal raises RuntimeError."""
    P, N, M, C = len(a["mkf_flags"]), len(a["pt_flags"]), len(a["ms_mkf"]), int(a["ncam"])
    cfb, bfw = _f64(a["cam_from_base"], (C, 12)), _f64(a["base_from_world"], (P, 12))
    mf, act, dep = _i32(a["mkf_flags"], (P,)), _u8(a["kf_active"], (P, C)), _f64(a["kf_depth_mean"], (P, C))
    wp, sm, sc, pf = _f64(a["world_pos"], (N, 3)), _i32(a["src_mkf"], (N,)), _i32(a["src_cam"], (N,)), _i32(a["pt_flags"], (N,))
    mm, mc, mr = _i32(a["ms_mkf"], (M,)), _i32(a["ms_cam"], (M,)), _i32(a["ms_row"], (M,))
    uv, ml, msrc, al = _f64(a["ms_uv"], (M, 2)), _i32(a["ms_level"], (M,)), _i32(a["ms_source"], (M,)), _u8(a["ms_alive"], (M,))
    res = SelectResult()
    mk, pt, ms = np.zeros(max(P, 1), dtype=MKF_DTYPE), np.zeros(max(N, 1), dtype=POINT_DTYPE), np.zeros(max(M, 1), dtype=MEAS_DTYPE)
    rc = lib().mcp_map_bundle_select_host(ctypes.addressof(params), C, cfb.ctypes.data, P, bfw.ctypes.data, mf.ctypes.data, act.ctypes.data, dep.ctypes.data,
                                          N, wp.ctypes.data, sm.ctypes.data, sc.ctypes.data, pf.ctypes.data, M, mm.ctypes.data, mc.ctypes.data, mr.ctypes.data,
                                          uv.ctypes.data, ml.ctypes.data, msrc.ctypes.data, al.ctypes.data, ctypes.addressof(res), P, mk.ctypes.data, N, pt.ctypes.data,
                                          M, ms.ctypes.data)
    _chk(rc, "map_bundle_select_host")
    return res, mk[:res.n_adjust + res.n_fixed].copy(), pt[:res.n_points].copy(), ms[:res.n_meas].copy()


# ---- the keyframe lists: mcp_graph_kf_lists_host and the numpy restatement ----------------------------------------------------------------------
def _list_counts(a, n_rows):
    """(inlier, outlier) of the n_rows table rows: a["inlier"] / a["outlier"] where given, (1, 0) otherwise."""
    i = np.ones(n_rows, dtype=np.int32) if a.get("inlier") is None else _i32(a["inlier"], (n_rows,))
    o = np.zeros(n_rows, dtype=np.int32) if a.get("outlier") is None else _i32(a["outlier"], (n_rows,))
    return i, o


def kf_lists_host(a, slots, n_rows=None):
    """mcp_graph_kf_lists_host over the flat arrays `a` (problem_arrays' keys; optional "inlier" / "outlier" count columns, (1, 0) without):
    (seg_start, seg_rows, seg_w) of the keyframes (slots[i], c).  n_rows: the table's rows when it has more than the len(a["pt_flags"]) graph
    columns written.  Needs no device.  A refusal raises RuntimeError."""
    P, Np, M, C = len(a["mkf_flags"]), len(a["pt_flags"]), len(a["ms_mkf"]), int(a["ncam"])
    n_rows = Np if n_rows is None else int(n_rows)
    mf, act, pf = _i32(a["mkf_flags"], (P,)), _u8(a["kf_active"], (P, C)), _i32(a["pt_flags"], (Np,))
    inl, outl = _list_counts(a, n_rows)
    mm, mc, mr, al = _i32(a["ms_mkf"], (M,)), _i32(a["ms_cam"], (M,)), _i32(a["ms_row"], (M,)), _u8(a["ms_alive"], (M,))
    sl = _i32(slots)
    ss = np.zeros(len(sl) * C + 1, dtype=np.int32)
    sr, sw = np.zeros(max(M, 1), dtype=np.int32), np.zeros(max(M, 1))
    tot = _chk(lib().mcp_graph_kf_lists_host(C, P, mf.ctypes.data, act.ctypes.data, n_rows, Np, pf.ctypes.data, inl.ctypes.data, outl.ctypes.data, M, mm.ctypes.data,
                                             mc.ctypes.data, mr.ctypes.data, al.ctypes.data, len(sl), sl.ctypes.data, ss.ctypes.data, M, sr.ctypes.data, sw.ctypes.data),
               "graph_kf_lists_host")
    return ss, sr[:tot].copy(), sw[:tot].copy()


def kf_lists_ref(a, slots, n_rows=None):
    """KeyFrame::GetPointDepthsAndWeights (src/KeyFrame.cc:549-570) with the mbActive filter of MultiKeyFrame::RefreshSceneDepthRobust
    (:851-869) over the flat arrays, in numpy: keyframe j = i * ncam + c is (slots[i], c); its list is the alive store entries of that keyframe,
    if it is active, whose row is in the table and not bad (a row past the written graph columns is bad), in store order -- a stable argsort
    over the keys of the kept entries.  Weights: inlier / (inlier + outlier), sum and quotient in double.  Returns (seg_start, seg_rows, seg_w) as kf_lists_host does."""
    P, Np, C = len(a["mkf_flags"]), len(a["pt_flags"]), int(a["ncam"])
    n_rows = Np if n_rows is None else int(n_rows)
    sl = np.asarray(slots, dtype=np.int64)
    pos = -np.ones(MAX_MKFS, dtype=np.int64)
    pos[sl] = np.arange(len(sl))
    mm, mc, mr = (np.asarray(a[k]).astype(np.int64) for k in ("ms_mkf", "ms_cam", "ms_row"))
    ok = (np.asarray(a["ms_alive"]) != 0) & (mm >= 0) & (mm < MAX_MKFS) & (mc >= 0) & (mc < C) & (mr >= 0) & (mr < n_rows)
    e = np.flatnonzero(ok)
    act = np.zeros((MAX_MKFS, C), dtype=bool); act[:P] = np.asarray(a["kf_active"]).reshape(P, C) != 0
    bad = np.ones(n_rows, dtype=bool); bad[:Np] = (np.asarray(a["pt_flags"]) & GP_BAD) != 0
    e = e[(pos[mm[e]] >= 0) & act[mm[e], mc[e]] & ~bad[mr[e]]]
    key = pos[mm[e]] * C + mc[e]
    e = e[np.argsort(key, kind="stable")]
    seg_start = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=len(sl) * C))]).astype(np.int32)
    inl, outl = _list_counts(a, n_rows)
    rows = mr[e].astype(np.int32)
    return seg_start, rows, inl[rows].astype(np.float64) / (inl[rows].astype(np.float64) + outl[rows].astype(np.float64))


# ---- the commit of a measurement parcel: mcp_parcel_commit_host and the numpy restatement --------------------------------------------------
def parcel_entries(lane, row, uv, level, key=None):
    """PARCEL_ENTRY_DTYPE records from columns (key: zeros when not given)."""
    n = len(np.asarray(lane))
    e = np.zeros(n, dtype=PARCEL_ENTRY_DTYPE)
    e["lane"], e["row"], e["level"] = _i32(lane, (n,)), _i32(row, (n,)), _i32(level, (n,))
    e["uv"] = _f64(uv).reshape(n, 2)
    if key is not None:
        e["key"] = _i32(key, (n,))
    return e


def _parcel_args(entries, keys, pt_flags, src_mkf, src_cam, lane_mkf, lane_cam):
    e = np.ascontiguousarray(entries, dtype=PARCEL_ENTRY_DTYPE)
    k, pf = _i32(keys), _i32(pt_flags)
    sm, sc = _i32(src_mkf, pf.shape), _i32(src_cam, pf.shape)
    lm = _i32(lane_mkf)
    return e, k, pf, sm, sc, lm, _i32(lane_cam, lm.shape)


def parcel_commit_host(entries, keys, pt_flags, src_mkf, src_cam, lane_mkf, lane_cam, cross_camera=1, source=SRC_TRACKER, first=0):
    """mcp_parcel_commit_host: the commit of parcel `entries` (PARCEL_ENTRY_DTYPE) against a map given as plain arrays -- keys: the table's key
    column now; pt_flags / src_mkf / src_cam: the graph columns written so far (rows past them are bad).  Returns (verdicts uint8 (n,),
    dict of mcp_parcel_commit_result, appended records (STORE_ENTRY_DTYPE), lane_appended).  Needs no device.  A refusal raises RuntimeError."""
    e, k, pf, sm, sc, lm, lc = _parcel_args(entries, keys, pt_flags, src_mkf, src_cam, lane_mkf, lane_cam)
    n, L = len(e), len(lm)
    prm, res = ParcelCommitParams(int(cross_camera), int(source)), ParcelCommitResult()
    vd, out, la = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=STORE_ENTRY_DTYPE), np.zeros(max(L, 1), dtype=np.int32)
    got = _chk(lib().mcp_parcel_commit_host(n, e.ctypes.data, len(k), k.ctypes.data, len(pf), pf.ctypes.data, sm.ctypes.data, sc.ctypes.data, L, lm.ctypes.data, lc.ctypes.data,
                                            ctypes.addressof(prm), int(first), vd.ctypes.data, out.ctypes.data, ctypes.addressof(res), la.ctypes.data), "parcel_commit_host")
    return vd[:n], res.as_dict(), out[:got].copy(), la[:L]


def parcel_commit_ref(entries, keys, pt_flags, src_mkf, src_cam, lane_mkf, lane_cam, cross_camera=1, source=SRC_TRACKER, first=0):
    """The commit in numpy, from the reference: Tracker::RecordMeasurements (src/Tracker.cc:1237-1274: the mbBad and CrossCamera tests) and the
    sweep of AddMultiKeyFrameFromTopOfQueue (src/MapMaker.cc:407-418), with the two rules a row-indexed table adds in front (a withheld lane;
    a row recycled for another point).  Per entry the first verdict that applies; the appended records in parcel order.  Returns what
    parcel_commit_host returns."""
    e, k, pf, sm, sc, lm, lc = _parcel_args(entries, keys, pt_flags, src_mkf, src_cam, lane_mkf, lane_cam)
    n, R, Rp = len(e), len(k), len(pf)
    lane, row = e["lane"].astype(np.int64), e["row"].astype(np.int64)
    if n and (lane.min() < 0 or lane.max() >= len(lm)):
        raise ValueError("parcel_commit_ref: an entry names a lane outside the lane tables")
    vd = np.full(n, PARCEL_APPENDED, dtype=np.uint8)
    open_ = np.ones(n, dtype=bool)                         # no verdict yet

    def rule(cond, verdict):
        hit = open_ & cond
        vd[hit] = verdict
        open_[hit] = False
    mkf_of = lm[lane] if n else np.zeros(0, dtype=np.int32)
    rule(mkf_of < 0, PARCEL_SKIPPED)
    in_table = (row >= 0) & (row < R)
    key_now = np.where(in_table, k[np.clip(row, 0, max(R - 1, 0))] if R else 0, 0)
    rule(~in_table | (key_now != e["key"]), PARCEL_STALE)
    has_col = row < Rp
    rp = np.clip(row, 0, max(Rp - 1, 0))
    bad = ~has_col | ((pf[rp] & GP_BAD) != 0 if Rp else True)
    rule(bad, PARCEL_BAD)
    if not cross_camera:
        cross = (sm[rp] < 0) | (sc[rp] != lc[lane]) if Rp else np.ones(n, dtype=bool)
        rule(cross, PARCEL_CROSS)
    keep = np.flatnonzero(vd == PARCEL_APPENDED)
    out = np.zeros(len(keep), dtype=STORE_ENTRY_DTYPE)
    out["uv"], out["mkf"], out["cam"], out["row"], out["level"] = e["uv"][keep], lm[lane[keep]], lc[lane[keep]], e["row"][keep], e["level"][keep]
    out["source"], out["alive"] = int(source), 1
    cnt = np.bincount(vd, minlength=5)
    res = dict(first=int(first), n_appended=int(cnt[PARCEL_APPENDED]), n_skipped_lane=int(cnt[PARCEL_SKIPPED]), n_stale=int(cnt[PARCEL_STALE]), n_bad=int(cnt[PARCEL_BAD]),
               n_cross=int(cnt[PARCEL_CROSS]))
    return vd, res, out, np.bincount(lane[keep], minlength=len(lm)).astype(np.int32)[:len(lm)]


# ---- outliers and bad points: the host twins and the numpy restatements -------------------------------------------------------------------------
def _cull_state(a, n_rows=None):
    """The arrays the two calls read and write, copied out of the flat arrays `a` (problem_arrays' keys; optional "pending", "inlier", "outlier",
    "usable"): n_rows table rows (default: the len(a["pt_flags"]) graph columns written), pending 0, counts (1, 0) and usable 1 where not given."""
    Np = len(a["pt_flags"])
    n_rows = Np if n_rows is None else int(n_rows)
    inl, outl = _list_counts(a, n_rows)
    b = dict(ncam=int(a["ncam"]), n_rows=n_rows, mkf_flags=_i32(a["mkf_flags"]).copy(), src_mkf=_i32(a["src_mkf"], (Np,)).copy(), pt_flags=_i32(a["pt_flags"]).copy(),
             pending=(np.zeros(Np, dtype=np.uint8) if a.get("pending") is None else _u8(a["pending"], (Np,)).copy()), inlier=inl.copy(), outlier=outl.copy(),
             usable=(np.ones(n_rows, dtype=np.uint8) if a.get("usable") is None else _u8(a["usable"], (n_rows,)).copy()))
    M = len(a["ms_mkf"])
    for k in ("ms_mkf", "ms_cam", "ms_row", "ms_source"):
        b[k] = _i32(a[k], (M,)).copy()
    b["ms_alive"] = _u8(a["ms_alive"], (M,)).copy()
    return b


def _cull_merge(a, b):
    """`a` with the columns a cull call changed taken from the state b."""
    out = copy_arrays(a)
    for k in ("pt_flags", "pending", "usable", "ms_alive"):
        out[k] = b[k]
    return out


def _cull_keys(mkf, cam, row):
    m = _i32(mkf)
    return m, _i32(cam, m.shape), _i32(row, m.shape)


def cull_outliers_host(a, mkf, cam, row, bad_good_count=2, n_rows=None):
    """mcp_map_cull_outliers_host over the flat arrays `a` (see _cull_state) for the outlier keys in list order: (dict of
    mcp_cull_outliers_result, verdicts uint8 (n,), the arrays afterwards -- a copy of `a` with pt_flags, pending, usable, ms_alive as the call
    leaves them).  Needs no device.  A refusal raises RuntimeError."""
    b = _cull_state(a, n_rows)
    m, c, r = _cull_keys(mkf, cam, row)
    n = len(m)
    prm, res = CullOutliersParams(int(bad_good_count)), CullOutliersResult()
    vd = np.zeros(max(n, 1), dtype=np.uint8)
    _chk(lib().mcp_map_cull_outliers_host(n, m.ctypes.data, c.ctypes.data, r.ctypes.data, ctypes.addressof(prm), b["ncam"], len(b["mkf_flags"]), b["mkf_flags"].ctypes.data,
                                          b["n_rows"], len(b["pt_flags"]), b["src_mkf"].ctypes.data, b["pt_flags"].ctypes.data, b["pending"].ctypes.data, len(b["ms_mkf"]),
                                          b["ms_mkf"].ctypes.data, b["ms_cam"].ctypes.data, b["ms_row"].ctypes.data, b["ms_source"].ctypes.data, b["ms_alive"].ctypes.data,
                                          vd.ctypes.data, ctypes.addressof(res)), "map_cull_outliers_host")
    return res.as_dict(), vd[:n], _cull_merge(a, b)


def cull_sweep_host(a, min_outliers=20, outlier_multiplier=1.0, danglers=True, n_rows=None):
    """mcp_map_cull_sweep_host over the flat arrays `a`: (dict of mcp_cull_sweep_result, the reported rows ascending, the arrays afterwards).
    Needs no device.  A refusal raises RuntimeError."""
    b = _cull_state(a, n_rows)
    prm, res = CullSweepParams(int(min_outliers), int(bool(danglers)), float(outlier_multiplier)), CullSweepResult()
    rows = np.zeros(max(b["n_rows"], 1), dtype=np.int32)
    got = _chk(lib().mcp_map_cull_sweep_host(ctypes.addressof(prm), len(b["mkf_flags"]), b["mkf_flags"].ctypes.data, b["n_rows"], len(b["pt_flags"]), b["pt_flags"].ctypes.data,
                                             b["pending"].ctypes.data, b["inlier"].ctypes.data, b["outlier"].ctypes.data, b["usable"].ctypes.data, len(b["ms_mkf"]),
                                             b["ms_mkf"].ctypes.data, b["ms_row"].ctypes.data, b["ms_alive"].ctypes.data, ctypes.addressof(res), b["n_rows"], rows.ctypes.data),
               "map_cull_sweep_host")
    return res.as_dict(), rows[:got].copy(), _cull_merge(a, b)


def _cull_good(b):
    """GoodMeasCount() of every table row (MapPoint.h:80-87): the live measurements whose MKF is in the map and not bad."""
    mf = np.zeros(MAX_MKFS, dtype=np.int64); mf[:len(b["mkf_flags"])] = b["mkf_flags"]
    ok = ((mf & MKF_PRESENT) != 0) & ((mf & MKF_BAD) == 0)
    mm, mr = b["ms_mkf"].astype(np.int64), b["ms_row"].astype(np.int64)
    live = (b["ms_alive"] != 0) & (mr >= 0) & (mr < b["n_rows"]) & (mm >= 0) & (mm < MAX_MKFS)
    return np.bincount(mr[live & ok[np.clip(mm, 0, MAX_MKFS - 1)]], minlength=b["n_rows"])[:b["n_rows"]], ok, mf


def cull_outliers_ref(a, mkf, cam, row, bad_good_count=2, n_rows=None):
    """MapMakerServerBase::HandleOutliers (src/MapMakerServerBase.cc:1198-1238) as its loop reads: one outlier after the other in the list's
    order, GoodMeasCount() counted afresh from the store each time.  On top of it the rules a row-indexed store adds: a key without a live
    measurement, a row outside the table or never written (no source, bad, not fixed) or a slot that is not in the map is MISSING.  Returns what
    cull_outliers_host returns."""
    b = _cull_state(a, n_rows)
    m, c, r = _cull_keys(mkf, cam, row)
    n, Np = len(m), len(b["pt_flags"])
    if n and (m.min() < 0 or m.max() >= MAX_MKFS or c.min() < 0 or c.max() >= b["ncam"]):
        raise ValueError("cull_outliers_ref: a key names a slot or a camera out of range")
    if len({(int(x), int(y), int(z)) for x, y, z in zip(m, c, r)}) != n:
        raise ValueError("cull_outliers_ref: a key appears twice")
    where = {}
    for i in np.flatnonzero(b["ms_alive"]):
        where[(int(b["ms_mkf"][i]), int(b["ms_cam"][i]), int(b["ms_row"][i]))] = int(i)        # kf.mmpMeasurements[&point]
    flags, alive = b["pt_flags"], b["ms_alive"]
    vd = np.zeros(n, dtype=np.uint8)
    fixed_rows, bad_points = set(), set()
    mf = _cull_good(b)[2]
    for i in range(n):
        k, p = int(m[i]), int(r[i])
        e = where.get((k, int(c[i]), p))
        written = 0 <= p < Np and (b["src_mkf"][p] >= 0 or (flags[p] & GP_FIXED))
        if e is None or not alive[e] or not written or not (mf[k] & MKF_PRESENT):
            vd[i] = CULL_MISSING
        elif flags[p] & GP_FIXED:                                                  # :1210-1214
            fixed_rows.add(p)
            vd[i] = CULL_FIXED
        elif _cull_good(b)[0][p] <= bad_good_count or b["ms_source"][e] == SRC_ROOT:   # :1216-1220
            if not flags[p] & GP_BAD:
                bad_points.add(p)
                b["pending"][p] = 1
            flags[p] |= GP_BAD
            vd[i] = CULL_POINT_BAD
        elif not flags[p] & GP_BAD:                                                 # :1221-1235
            vd[i] = CULL_RETRY if b["ms_source"][e] in (SRC_TRACKER, SRC_EPIPOLAR) else CULL_NEVER_RETRY
            alive[e] = 0                                                            # kf.EraseMeasurementOfPoint, spMeasurementKFs.erase
        else:
            vd[i] = CULL_ALREADY_BAD
    cnt = np.bincount(vd, minlength=6)
    res = dict(n_missing=int(cnt[0]), n_fixed=int(cnt[1]), n_point_bad=int(cnt[2]), n_retry=int(cnt[3]), n_never_retry=int(cnt[4]), n_already_bad=int(cnt[5]),
               n_fixed_rows=len(fixed_rows), n_rows_marked=len(bad_points))
    return res, vd, _cull_merge(a, b)


def cull_sweep_ref(a, min_outliers=20, outlier_multiplier=1.0, danglers=True, n_rows=None):
    """MarkDanglersAsBad, MarkOutliersAsBad (src/MapMakerClientBase.cc:73-108) and Map::MoveBadPointsToTrash (src/Map.cc:93-116) over the flat
    arrays, in numpy; the report is the rows these two marked plus the bad rows whose pending mark an earlier cull_outliers left.  Rows past the
    graph columns written are bad and never reported.  Returns what cull_sweep_host returns."""
    b = _cull_state(a, n_rows)
    R, Np = b["n_rows"], len(b["pt_flags"])
    good, _, mf = _cull_good(b)
    fl = b["pt_flags"]
    bad0, fixed = (fl & GP_BAD) != 0, (fl & GP_FIXED) != 0
    dang = np.zeros(Np, dtype=bool)
    if danglers and int(((mf & MKF_PRESENT) != 0).sum()) >= 2:                      # mlpMultiKeyFrames.size() < 2: return
        dang = ~bad0 & ~fixed & (good[:Np] < 2)
    o, i = b["outlier"][:Np], b["inlier"][:Np]
    trk = ~bad0 & ~dang & ~fixed & (o > min_outliers) & (o.astype(np.float64) > i.astype(np.float64) * float(outlier_multiplier))
    rows = np.flatnonzero(dang | trk | (bad0 & (b["pending"] != 0))).astype(np.int32)
    fl[dang | trk] |= GP_BAD
    b["pending"][:] = 0
    bad = np.ones(R, dtype=bool); bad[:Np] = (fl & GP_BAD) != 0
    b["usable"][bad] = 0
    mr = b["ms_row"].astype(np.int64)
    dies = (b["ms_alive"] != 0) & (mr >= 0) & (mr < R)
    dies[dies] = bad[mr[dies]]                                                     # MapPoint::EraseAllMeasurements
    b["ms_alive"][dies] = 0
    res = dict(n_danglers=int(dang.sum()), n_tracker_outliers=int(trk.sum()), n_reported=len(rows), n_bad_rows=int(bad.sum()), n_meas_erased=int(dies.sum()))
    return res, rows, _cull_merge(a, b)


# ---- closest-keyframe queries and the removal of an MKF: parameters, the host twins, the numpy restatements -------------------------------------
def neigh_params(kind=NB_MKF, region=NB_ALL, order=NB_NEAREST, src_slot=-1, src_cam=0, same_cam=False, n_max=1, want_meas=False, max_dist=np.inf,
                 mean_diff_fraction=0.5, ext=None):
    """mcp_neigh_params.  ext: the external MKF (src_slot == -1) as dict(base_from_world (12,), kf_active (ncam,), kf_depth_mean (ncam,))."""
    p = NeighParams(int(kind), int(region), int(order), int(src_slot), int(src_cam), int(bool(same_cam)), int(n_max), int(bool(want_meas)), float(max_dist),
                    float(mean_diff_fraction))
    if ext is not None:
        b, a, d = _f64(ext["base_from_world"]).reshape(12), np.asarray(ext["kf_active"]).reshape(-1), _f64(ext["kf_depth_mean"]).reshape(-1)
        if len(a) > MAX_CAMS or len(a) != len(d):
            raise ValueError("neigh_params: the external MKF has one active byte and one depth mean per camera of the rig")
        for k in range(12):
            p.ext_base_from_world[k] = b[k]
        for c in range(len(a)):
            p.ext_active[c], p.ext_depth_mean[c] = int(a[c] != 0), d[c]
    return p


def _as_neigh_params(params):
    return params if isinstance(params, NeighParams) else neigh_params(**params)


def _mkf_columns(a):
    P, C = len(a["mkf_flags"]), int(a["ncam"])
    return (C, P, _f64(a["cam_from_base"], (C, 12)), _f64(a["base_from_world"], (P, 12)), _i32(a["mkf_flags"], (P,)), _u8(a["kf_active"], (P, C)),
            _f64(a["kf_depth_mean"], (P, C)))


def neighbours_host(a, params, raw=False):
    """mcp_map_neighbours_host over the flat arrays `a` (problem_arrays' keys): (dict of status / count / n_candidates, the winners as a
    NEIGH_ITEM_DTYPE array), or with raw the NeighResult itself.  params: a NeighParams or neigh_params' keywords.  Needs no device.  A refusal
    raises RuntimeError."""
    p = _as_neigh_params(params)
    C, P, cfb, bfw, mf, act, dep = _mkf_columns(a)
    M = len(a["ms_mkf"])
    mm, mc, al = _i32(a["ms_mkf"], (M,)), _i32(a["ms_cam"], (M,)), _u8(a["ms_alive"], (M,))
    res = NeighResult()
    _chk(lib().mcp_map_neighbours_host(ctypes.addressof(p), C, cfb.ctypes.data, P, bfw.ctypes.data, mf.ctypes.data, act.ctypes.data, dep.ctypes.data, M, mm.ctypes.data,
                                       mc.ctypes.data, al.ctypes.data, ctypes.addressof(res)), "map_neighbours_host")
    return res if raw else (res.as_dict(), res.items())


def _cull_mkf_state(a):
    """The columns mcp_map_mkf_cull changes, copied out of `a`: (mkf_flags, pt_flags, pending, ms_alive)."""
    Np = len(a["pt_flags"])
    return (_i32(a["mkf_flags"]).copy(), _i32(a["pt_flags"]).copy(), (np.zeros(Np, dtype=np.uint8) if a.get("pending") is None else _u8(a["pending"], (Np,)).copy()),
            _u8(a["ms_alive"]).copy())


def _cull_mkf_merge(a, mf, pf, pend, alive):
    out = copy_arrays(a)
    out["mkf_flags"], out["pt_flags"], out["pending"], out["ms_alive"] = mf, pf, pend, alive
    return out


def cull_mkf_host(a, slot=-1, furthest_from=-1, mark_points=True, max_kfs=2, erase=True, mean_diff_fraction=0.5, n_rows=None):
    """mcp_map_mkf_cull_host over the flat arrays `a`: (dict of mcp_mkf_cull_result, the arrays afterwards -- a copy of `a` with mkf_flags,
    pt_flags, pending and ms_alive as the call leaves them).  Needs no device.  A refusal raises RuntimeError."""
    C, P, cfb, bfw, _, act, dep = _mkf_columns(a)
    mf, pf, pend, alive = _cull_mkf_state(a)
    Np, M = len(pf), len(alive)
    n_rows = int(a.get("n_rows", Np)) if n_rows is None else int(n_rows)
    sm, sc = _i32(a["src_mkf"], (Np,)), _i32(a["src_cam"], (Np,))
    mm, mc, mr = _i32(a["ms_mkf"], (M,)), _i32(a["ms_cam"], (M,)), _i32(a["ms_row"], (M,))
    prm, res = MkfCullParams(int(slot), int(furthest_from), int(bool(mark_points)), int(max_kfs), int(bool(erase)), float(mean_diff_fraction)), MkfCullResult()
    _chk(lib().mcp_map_mkf_cull_host(ctypes.addressof(prm), C, cfb.ctypes.data, P, bfw.ctypes.data, mf.ctypes.data, act.ctypes.data, dep.ctypes.data, n_rows, Np, sm.ctypes.data,
                                     sc.ctypes.data, pf.ctypes.data, pend.ctypes.data, M, mm.ctypes.data, mc.ctypes.data, mr.ctypes.data, alive.ctypes.data,
                                     ctypes.addressof(res)), "map_mkf_cull_host")
    return res.as_dict(), _cull_mkf_merge(a, mf, pf, pend, alive)


def _kf_frames(cfb, bfw, dep):
    """Per (MKF, camera): the camera centre and the mean scene point in the world, each product and sum in the order KeyFrame::Distance's
    callers take them (CamFromWorld = CamFromBase * BaseFromWorld; inverse(); inverse * (0, 0, depth)).  bfw (n, 12), dep (n, C) -> two (n, C, 3)."""
    C = len(cfb)
    cR, ct = cfb[:, :9].reshape(C, 3, 3)[None], cfb[:, 9:][None]
    bR, bt = bfw[:, :9].reshape(-1, 3, 3)[:, None], bfw[:, 9:][:, None]
    R = [[cR[..., i, 0] * bR[..., 0, j] + cR[..., i, 1] * bR[..., 1, j] + cR[..., i, 2] * bR[..., 2, j] for j in range(3)] for i in range(3)]
    t = [cR[..., i, 0] * bt[..., 0] + cR[..., i, 1] * bt[..., 1] + cR[..., i, 2] * bt[..., 2] + ct[..., i] for i in range(3)]
    with np.errstate(all="ignore"):
        centre = [-(R[0][i] * t[0] + R[1][i] * t[1] + R[2][i] * t[2]) for i in range(3)]            # -(R^T t)
        mean = [R[0][i] * 0.0 + R[1][i] * 0.0 + R[2][i] * dep + centre[i] for i in range(3)]        # R^T (0, 0, depth) + centre
    return np.stack(centre, axis=-1), np.stack(mean, axis=-1)


def _kf_dist(c1, m1, c2, m2, frac):
    """KeyFrame::Distance (src/KeyFrame.cc:715-747) from centres and mean points (..., 3), 1: the source, 2: the candidate."""
    with np.errstate(all="ignore"):
        d, e = c2 - c1, m2 - m1
        return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]) + \
            np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]) * frac


def neighbours_ref(a, params):
    """The reference's closest-keyframe queries (src/MapMakerBase.cc:90-339 over src/KeyFrame.cc:715-747, 903-927) in numpy, over the flat
    arrays, with the documented deviations ((slot, cam) as the tie-breaker, kf_active as the record that a keyframe exists, status 3).  The
    external MKF is row 0 of every column here, slot -1.  Returns what neighbours_host returns."""
    p = _as_neigh_params(params)
    C, P, cfb, bfw, mf, act, dep = _mkf_columns(a)
    kf = p.kind == NB_KF
    ext = p.src_slot == -1
    bfw = np.concatenate([np.array(p.ext_base_from_world, dtype=np.float64).reshape(1, 12), bfw])
    ea = np.array(p.ext_active[:C], dtype=np.uint8) != 0
    act = np.concatenate([ea.reshape(1, C), act != 0])
    dep = np.concatenate([np.where(ea, np.array(p.ext_depth_mean[:C]), 0.0).reshape(1, C), np.where(act[1:], dep, 0.0)])
    flags = np.concatenate([[0], mf]).astype(np.int64)
    present = (flags & MKF_PRESENT) != 0
    slot = np.arange(-1, P)
    centre, mean = _kf_frames(cfb, bfw, dep)
    s = p.src_slot + 1
    if kf:
        own = (slot == p.src_slot)[:, None]
        cam = np.arange(C)[None, :]
        cand = (present[:, None] | (own & ext)) & act & ~(own & (cam == p.src_cam))
        if p.region == NB_ONLY_SELF:
            cand &= own
        if p.region == NB_ONLY_OTHER:
            cand &= ~own
        if p.same_cam:
            cand &= cam == p.src_cam
        j, c = np.nonzero(cand)                                                     # ascending (slot, cam)
        d = _kf_dist(centre[s, p.src_cam], mean[s, p.src_cam], centre[j, c], mean[j, c], p.mean_diff_fraction)
        broken = ~np.isfinite(d) | (d > 1e10)
    else:
        j = np.flatnonzero(present & (slot != p.src_slot) & (slot >= 0))
        c = np.zeros(len(j), dtype=np.int64)
        pd = _kf_dist(centre[s][None, :, None, :], mean[s][None, :, None, :], centre[j][:, None, :, :], mean[j][:, None, :, :], p.mean_diff_fraction)   # (n, c1, c2)
        pair = act[s][None, :, None] & act[j][:, None, :]
        broken = (pair & (~np.isfinite(pd) | (pd > 1e10))).reshape(len(j), C * C).any(axis=1)
        d = np.where(pair & ~np.isnan(pd), pd, DBL_MAX).reshape(len(j), C * C).min(axis=1)
    res = dict(status=0, count=0, n_candidates=len(j))
    if broken.any():
        res["status"] = 3
        return res, np.zeros(0, dtype=NEIGH_ITEM_DTYPE)
    ok = d <= p.max_dist
    if p.order == NB_FURTHEST:
        ok &= d > 0.0
    k = np.flatnonzero(ok)
    k = k[np.lexsort((c[k], j[k], d[k] if p.order == NB_NEAREST else -d[k]))][:p.n_max]
    items = np.zeros(len(k), dtype=NEIGH_ITEM_DTYPE)
    items["dist"], items["slot"], items["cam"], items["flags"], items["n_meas"] = d[k], slot[j[k]], (c[k] if kf else -1), flags[j[k]], -1
    if p.want_meas:
        al = np.asarray(a["ms_alive"]) != 0
        mm, mc = np.asarray(a["ms_mkf"]), np.asarray(a["ms_cam"])
        items["n_meas"] = [int((al & (mm == it["slot"]) & ((mc == it["cam"]) if kf else True)).sum()) for it in items]
    res["count"] = len(k)
    return res, items


def cull_mkf_ref(a, slot=-1, furthest_from=-1, mark_points=True, max_kfs=2, erase=True, mean_diff_fraction=0.5, n_rows=None):
    """MarkFurthestMultiKeyFrameAsBad (src/MapMakerServerBase.cc:264-318) and what Map::MoveBadMultiKeyFramesToTrash (src/Map.cc:119-187)
    does to the victim's measurements, over the flat arrays, as the reference's loops read: the victim's keyframes, their measurements, the
    point rule on the counts on entry.  Returns what cull_mkf_host returns."""
    mf, pf, pend, alive = _cull_mkf_state(a)
    Np, M = len(pf), len(alive)
    n_rows = int(a.get("n_rows", Np)) if n_rows is None else int(n_rows)
    res = dict(status=0, victim=-1, victim_dist_valid=0, victim_dist=0.0, n_victim_meas=0, n_rows_marked=0, n_by_count=0, n_by_source=0, new_fixed=-1, n_meas_erased=0)
    victim = int(slot)
    dist, valid = 0.0, 0
    if victim == -1:                                                                # FurthestMultiKeyFrame
        r, it = neighbours_ref(a, dict(kind=NB_MKF, order=NB_FURTHEST, src_slot=furthest_from, mean_diff_fraction=mean_diff_fraction))
        if r["status"] != 0 or r["count"] == 0:
            res["status"] = 3 if r["status"] else 1
            return res, _cull_mkf_merge(a, mf, pf, pend, alive)
        victim, dist, valid = int(it["slot"][0]), float(it["dist"][0]), 1
    new_fixed = -1
    if mf[victim] & MKF_FIXED:                                                      # :313-317
        r, it = neighbours_ref(a, dict(kind=NB_MKF, order=NB_NEAREST, src_slot=victim, mean_diff_fraction=mean_diff_fraction))
        if r["status"] != 0:
            res["status"] = 3
            return res, _cull_mkf_merge(a, mf, pf, pend, alive)
        if r["count"]:
            new_fixed = int(it["slot"][0])
    mm, mc, mr = (np.asarray(a[k]).astype(np.int64) for k in ("ms_mkf", "ms_cam", "ms_row"))
    sm, sc = np.asarray(a["src_mkf"]), np.asarray(a["src_cam"])
    live = (alive != 0) & (mr >= 0) & (mr < n_rows) & (mm >= 0) & (mm < MAX_MKFS)
    size = np.bincount(mr[live], minlength=max(n_rows, 1))                          # spMeasurementKFs.size() on entry
    was_bad = (pf & GP_BAD) != 0
    for i in np.flatnonzero(live & (mm == victim)):
        res["n_victim_meas"] += 1
        r = int(mr[i])
        if not mark_points or r >= Np:
            continue
        by_source = sm[r] == victim and sc[r] == mc[i]
        if (size[r] <= max_kfs and not pf[r] & GP_FIXED) or by_source:              # :281-283
            pf[r] |= GP_BAD
    marked = np.flatnonzero(((pf & GP_BAD) != 0) & ~was_bad)
    pend[marked] = 1
    src_rows = set(int(mr[i]) for i in np.flatnonzero(live & (mm == victim) & (mr < Np)) if sm[mr[i]] == victim and sc[mr[i]] == mc[i])
    res["n_rows_marked"] = len(marked)
    res["n_by_source"] = sum(1 for r in marked if int(r) in src_rows)
    res["n_by_count"] = len(marked) - res["n_by_source"]
    mf[victim] |= MKF_BAD
    if new_fixed >= 0:
        mf[new_fixed] |= MKF_FIXED
    if erase:
        dies = (alive != 0) & (mm == victim)
        res["n_meas_erased"] = int(dies.sum())
        alive[dies] = 0
        mf[victim] &= ~MKF_PRESENT
    res.update(victim=victim, victim_dist_valid=valid, victim_dist=dist, new_fixed=new_fixed)
    return res, _cull_mkf_merge(a, mf, pf, pend, alive)


# ---- the numpy restatement, from the reference -----------------------------------------------------------------------------------------------
# ---- the co-visible points of the nearest keyframe (mcp_map_collect_nearest; the structs and the binding live in pvs.py) ------------------
def _collect_args(a, base_from_world, depth_mean, mean_diff_fraction, active, cam_from_base, n_rows):
    C = int(a["ncam"])
    prm = collect_params(depth_mean, mean_diff_fraction, active)
    if len(np.asarray(depth_mean).reshape(-1)) != C:
        raise ValueError("collect_nearest: one depth mean per camera of the rig")
    cur = None if cam_from_base is None else _f64(cam_from_base).reshape(C, 12)
    n_rows = int(a.get("n_rows", len(a["pt_flags"]))) if n_rows is None else int(n_rows)
    return prm, _f64(base_from_world).reshape(12), cur, n_rows


def collect_nearest_host(a, base_from_world, depth_mean, mean_diff_fraction=0.5, active=None, cam_from_base=None, n_rows=None, raw=False):
    """mcp_map_collect_nearest_host over the flat arrays `a` (problem_arrays' keys): (the report as a dict, the near mask, one byte per row), or
    with raw the CollectReport itself in place of the dict.  base_from_world (12,): the tracker's pose; depth_mean, active: per camera of the
    rig; cam_from_base: the current keyframes', None for the rig's.  Needs no device.  A refusal raises RuntimeError."""
    prm, b, cur, n_rows = _collect_args(a, base_from_world, depth_mean, mean_diff_fraction, active, cam_from_base, n_rows)
    C, P, cfb, bfw, mf, act, dep = _mkf_columns(a)
    M = len(a["ms_mkf"])
    mm, mc, mr, al = _i32(a["ms_mkf"], (M,)), _i32(a["ms_cam"], (M,)), _i32(a["ms_row"], (M,)), _u8(a["ms_alive"], (M,))
    rep, near = CollectReport(), np.zeros(n_rows, dtype=np.uint8)
    _chk(_bind_collect(lib()).mcp_map_collect_nearest_host(b.ctypes.data, None if cur is None else cur.ctypes.data, ctypes.addressof(prm), C, cfb.ctypes.data, P, bfw.ctypes.data,
                                                           mf.ctypes.data, act.ctypes.data, dep.ctypes.data, n_rows, M, mm.ctypes.data, mc.ctypes.data, mr.ctypes.data,
                                                           al.ctypes.data, ctypes.addressof(rep), near.ctypes.data), "map_collect_nearest_host")
    return (rep if raw else rep.as_dict()), near


def collect_nearest_ref(a, base_from_world, depth_mean, mean_diff_fraction=0.5, active=None, cam_from_base=None, n_rows=None):
    """Tracker::CollectNearestPoints with tracker_collect_all_points false (src/Tracker.cc:1785-1854) over the flat arrays, as the reference's
    loops read: ClosestKeyFrame (src/MapMakerBase.cc:115-140) walks the keyframes of the map in list order -- here (slot, cam) -- and keeps the
    first strict minimum; then the set of keyframes that measure one of its points, then the set of points those measure.  The documented
    deviations: an empty set with status 1 where the reference asserts and with status 3 where KeyFrame::Distance stops the process.  Returns
    what collect_nearest_host returns."""
    prm, b, cur, n_rows = _collect_args(a, base_from_world, depth_mean, mean_diff_fraction, active, cam_from_base, n_rows)
    C, P, cfb, bfw, mf, act, dep = _mkf_columns(a)
    cur = cfb if cur is None else cur
    # the map as the reference holds it: KeyFrame::mmpMeasurements and MapPoint::mMMData.spMeasurementKFs
    kf_points, point_kfs = {}, {}
    for al, m, c, r in zip(np.asarray(a["ms_alive"]), np.asarray(a["ms_mkf"]), np.asarray(a["ms_cam"]), np.asarray(a["ms_row"])):
        if al and 0 <= r < n_rows and 0 <= m < MAX_MKFS and 0 <= c < MAX_CAMS:
            kf_points.setdefault((int(m), int(c)), set()).add(int(r))
            point_kfs.setdefault(int(r), set()).add((int(m), int(c)))
    keyframes = [(s, c) for s in range(P) if mf[s] & MKF_PRESENT for c in range(C) if act[s, c]]
    centre, mean = _kf_frames(cfb, bfw, np.where(act != 0, dep, 0.0))
    own_centre, own_mean = _kf_frames(cur, b.reshape(1, 12), np.array(prm.depth_mean[:C]).reshape(1, C))
    rep = {k: np.zeros(MAX_CAMS, dtype=np.int32) for k in ("status", "n_candidates", "n_seed_rows", "n_kfs", "n_rows")}
    rep.update(valid=1, nearest_slot=np.full(MAX_CAMS, -1, dtype=np.int32), nearest_cam=np.full(MAX_CAMS, -1, dtype=np.int32), nearest_dist=np.zeros(MAX_CAMS))
    near = np.zeros(n_rows, dtype=np.uint8)
    for c in range(C):
        if not prm.active[c]:
            continue
        closest, closest_dist, broken = None, 0.0, False
        for kf in keyframes:
            d = float(_kf_dist(own_centre[0, c], own_mean[0, c], centre[kf], mean[kf], prm.mean_diff_fraction))
            broken = broken or not np.isfinite(d) or d > 1e10
            if closest is None or d < closest_dist:
                closest, closest_dist = kf, d
        rep["n_candidates"][c] = len(keyframes)
        rep["status"][c] = 3 if broken else (1 if closest is None else 0)
        if rep["status"][c] != 0:
            continue
        rep["nearest_slot"][c], rep["nearest_cam"][c], rep["nearest_dist"][c] = closest[0], closest[1], closest_dist
        seed = kf_points.get(closest, set())
        kfs = set().union(*[point_kfs[r] for r in seed])
        rows = set().union(*[kf_points[k] for k in kfs])
        rep["n_seed_rows"][c], rep["n_kfs"][c], rep["n_rows"][c] = len(seed), len(kfs), len(rows)
        near[sorted(rows)] |= np.uint8(1 << c)
    return rep, near


def mkf_distances(a, newest, mean_diff_fraction):
    """MultiKeyFrame::Distance(newest, k) for every slot k (KeyFrame.cc:903-927 over KeyFrame::Distance, :715-747): (P,) distances (DBL_MAX
    without a pair of active keyframes) and whether any pair's distance is one the reference stops the process on (:734-744)."""
    C = int(a["ncam"])
    cfb, bfw = _f64(a["cam_from_base"]).reshape(C, 12), _f64(a["base_from_world"])
    P = len(bfw)
    cR, ct = cfb[:, :9].reshape(C, 3, 3), cfb[:, 9:]
    bR, bt = bfw[:, :9].reshape(P, 3, 3), bfw[:, 9:]
    R, t = _compose(cR[None], ct[None], bR[:, None], bt[:, None])                   # (P, C): mse3CamFromWorld
    Rt = np.swapaxes(R, -1, -2)
    zero = np.zeros(3)
    centre = -_apply(Rt, zero, t)                                                   # inverse().get_translation()
    mean_c = np.zeros((P, C, 3)); mean_c[..., 2] = _f64(a["kf_depth_mean"])
    mean_w = _apply(Rt, centre, mean_c)                                             # se3KF_inv * v3MeanInCam
    act = _u8(a["kf_active"]).astype(bool)
    dC = centre[:, None, :, :] - centre[newest][None, :, None, :]                   # (P, c1 of newest, c2 of k, 3)
    dM = mean_w[:, None, :, :] - mean_w[newest][None, :, None, :]
    with np.errstate(all="ignore"):
        d = np.sqrt((dC * dC).sum(-1)) + np.sqrt((dM * dM).sum(-1)) * mean_diff_fraction
    pair = act[newest][None, :, None] & act[:, None, :]
    broken = pair & (~np.isfinite(d) | (d > 1e10))
    d = np.where(pair & ~np.isnan(d), d, np.finfo(np.float64).max)
    return d.reshape(P, -1).min(axis=1), broken.reshape(P, -1).any(axis=1)


def bundle_select_ref(a, params):
    """BundleAdjustAll / BundleAdjustRecent and the population loops of BundleAdjusterMulti::BundleAdjust over the flat arrays, in numpy, with
    the documented deviations (orders by slot / row / store index, slot as the tie-breaker, the short closest list, the dropped-source rule,
    status 3).  Returns (dict of the result's fields, mkfs, points, meas) as bundle_select_host does."""
    S = params
    P, N, M, C = len(a["mkf_flags"]), len(a["pt_flags"]), len(a["ms_mkf"]), int(a["ncam"])
    mf = np.asarray(a["mkf_flags"])
    present, mbad, mfixed = (mf & MKF_PRESENT) != 0, (mf & MKF_BAD) != 0, (mf & MKF_FIXED) != 0
    ok = present & ~mbad
    res = dict(status=0, n_adjust=0, n_fixed=0, n_points=0, n_meas=0, has_fixed_points=0, n_dropped_source=0, closest=[-1] * 8, closest_dist=[0.0] * 8)
    empty = (np.zeros(0, dtype=MKF_DTYPE), np.zeros(0, dtype=POINT_DTYPE), np.zeros(0, dtype=MEAS_DTYPE))
    if S.mode == BUNDLE_ALL:
        adjust = ok.copy()                                                         # :154-162
    else:
        if int(present.sum()) < S.recent_min_size:                                 # :196-201
            res["status"] = 1
            return (res,) + empty
        dist, broken = mkf_distances(a, S.newest, S.mean_diff_fraction)
        others = present.copy(); others[S.newest] = False
        if broken[others].any():
            res["status"] = 3
            return (res,) + empty
        cand = np.flatnonzero(others)
        order = cand[np.lexsort((cand, dist[cand]))][:S.n_recent]                  # NClosestMultiKeyFrames; fewer others: a shorter list
        for r, k in enumerate(order):
            res["closest"][r], res["closest_dist"][r] = int(k), float(dist[k])
        adjust = np.zeros(P, dtype=bool)
        adjust[S.newest] = True                                                    # :205-206
        adjust[order[~mbad[order] & ~mfixed[order]]] = True                        # :208-215
    mm, mr = np.asarray(a["ms_mkf"]).astype(np.int64), np.asarray(a["ms_row"]).astype(np.int64)
    live = (np.asarray(a["ms_alive"]) != 0) & (mr >= 0) & (mr < N)
    good = np.bincount(mr[live & ok[mm]], minlength=N)[:N]                         # GoodMeasCount, MapPoint.h:80-87
    pf = np.asarray(a["pt_flags"])
    pbad, pfixed = (pf & GP_BAD) != 0, (pf & GP_FIXED) != 0
    if S.mode == BUNDLE_ALL:
        sel = ~pbad & ((good >= 2) | pfixed)                                       # :170-176
    else:
        seen = np.zeros(N, dtype=bool)
        seen[mr[live & adjust[mm]]] = True                                         # :218-240
        sel = seen & ~pbad & (good >= 2)
    sm, sc = np.asarray(a["src_mkf"]).astype(np.int64), np.asarray(a["src_cam"]).astype(np.int64)
    src_ok = (sm >= 0) & (sm < P) & (sc >= 0) & (sc < C)
    src_ok[src_ok] = ok[sm[src_ok]]
    dropped = sel & ~pfixed & ~src_ok
    res["n_dropped_source"] = int(dropped.sum())
    sel &= ~dropped
    rows = np.flatnonzero(sel)
    if len(rows) < S.min_points:
        res["status"] = 2
        return (res,) + empty
    keep = live & sel[np.clip(mr, 0, max(N - 1, 0))] & ok[mm]                      # BundleAdjusterMulti.cc:168-200
    in_bundle = np.zeros(P, dtype=bool)
    in_bundle[mm[keep]] = True                                                     # :243-261: the parents of spAffectedKeyFrames
    in_bundle[sm[sel & ~pfixed]] = True                                            # the source MKF of a selected non-fixed row
    fixed_set = in_bundle & ok & ~adjust
    slots = np.concatenate([np.flatnonzero(adjust), np.flatnonzero(fixed_set)])
    mkfs = np.zeros(len(slots), dtype=MKF_DTYPE)
    mkfs["slot"] = slots
    mkfs["fixed"] = np.concatenate([mfixed[adjust], np.ones(int(fixed_set.sum()), dtype=bool)])
    mkf_idx = -np.ones(P, dtype=np.int64); mkf_idx[slots] = np.arange(len(slots))
    pt_idx = -np.ones(N, dtype=np.int64); pt_idx[rows] = np.arange(len(rows))
    points = np.zeros(len(rows), dtype=POINT_DTYPE)
    fx = pfixed[rows]
    points["row"], points["fixed"] = rows, fx
    points["src_mkf"] = np.where(fx, -1, mkf_idx[np.where(fx, 0, sm[rows])])
    points["src_cam"] = np.where(fx, -1, sc[rows])
    cfb, bfw = _f64(a["cam_from_base"]).reshape(C, 12), _f64(a["base_from_world"])
    wp = _f64(a["world_pos"])[rows]
    k, c = np.where(fx, 0, sm[rows]), np.where(fx, 0, sc[rows])
    R, t = _compose(cfb[c, :9].reshape(-1, 3, 3), cfb[c, 9:], bfw[k, :9].reshape(-1, 3, 3), bfw[k, 9:])   # kf.mse3CamFromWorld = CamFromBase * BaseFromWorld
    points["x"] = np.where(fx[:, None], wp, _apply(R, t, wp))                       # BundleAdjusterMulti.cc:145-158
    store = np.flatnonzero(keep)
    meas = np.zeros(len(store), dtype=MEAS_DTYPE)
    meas["uv"], meas["mkf"], meas["cam"] = _f64(a["ms_uv"])[store], mkf_idx[mm[store]], np.asarray(a["ms_cam"])[store]
    meas["point"], meas["level"], meas["source"], meas["store"] = pt_idx[mr[store]], np.asarray(a["ms_level"])[store], np.asarray(a["ms_source"])[store], store
    res.update(n_adjust=int(adjust.sum()), n_fixed=int(fixed_set.sum()), n_points=len(rows), n_meas=len(store), has_fixed_points=int(fx.any()))
    return res, mkfs, points, meas


def selection_problem(mkfs, points, meas, base_from_world, cam_from_base, cams):
    """The multi-mode synth.Problem a selection describes: base_* of the bundle's MKFs (base_fixed = fixed in the bundle), pt_* and ms_* from
    the views, and .window = dict(mkf=slots, adjust=the slots adjusted, points=rows, store=store indices).  Problem.populate replays it."""
    bfw, cfb = _f64(base_from_world), _f64(cam_from_base).reshape(-1, 12)
    slots = mkfs["slot"].astype(np.int64)
    fx = points["fixed"] != 0
    src = np.stack([np.where(fx, 0, points["src_mkf"]), np.where(fx, 0, points["src_cam"])], axis=1).astype(np.int32)
    q = synth.Problem(cams=list(cams), mode="multi", n_mkf=len(slots), base_R=bfw[slots, :9].reshape(-1, 3, 3).copy(), base_t=bfw[slots, 9:].copy(),
                      base_fixed=mkfs["fixed"] != 0, cam_R=cfb[:, :9].reshape(-1, 3, 3).copy(), cam_t=cfb[:, 9:].copy(), pt_x=np.ascontiguousarray(points["x"]),
                      pt_src=src, pt_fixed=fx, ms_mkf=meas["mkf"].astype(np.int32), ms_cam=meas["cam"].astype(np.int32), ms_pt=meas["point"].astype(np.int32),
                      ms_uv=np.ascontiguousarray(meas["uv"]), ms_level=meas["level"].astype(np.int32))
    q.window = dict(mkf=slots, adjust=slots[mkfs["fixed"] == 0] if len(slots) else slots, points=points["row"].astype(np.int64), store=meas["store"].astype(np.int64))
    return q


# ---- the map's beginning, its rescale and its re-alignment (include/mcp_img.h mcp_init_depth_map_points, mcp_map_mark_optimized, mcp_map_rescale, ----
# ---- mcp_map_transform; map_life.h): structs, host twins (no device) and numpy restatements (src/MapMakerServerBase.cc:212-215, 499-596) -----------
LIFE_SYMBOLS = ["mcp_init_depth_map_points", "mcp_map_mark_optimized", "mcp_map_rescale", "mcp_map_transform", "mcp_init_depth_points_host",
                "mcp_map_mark_optimized_host", "mcp_map_transform_host", "mcp_map_life_last_timing"]
XFORM_SCALE, XFORM_RIGID = 0, 1
LIFE_BLOCK = 256                              # map_life.h: candidates / rows of a workgroup


class InitDepthCam(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("cam", ctypes.c_void_p), ("n_cand", ctypes.c_int), ("cand", ctypes.c_void_p), ("limit", ctypes.c_int)]


class InitDepthParams(ctypes.Structure):
    _fields_ = [("src_mkf", ctypes.c_int), ("level", ctypes.c_int), ("init_depth", ctypes.c_double)]


class InitDepthResult(ctypes.Structure):
    _fields_ = [("made_total", ctypes.c_int), ("first_store", ctypes.c_int), ("made", ctypes.c_int * MAX_CAMS), ("n_busy", ctypes.c_int * MAX_CAMS),
                ("n_alive", ctypes.c_int * MAX_CAMS)]

    def as_dict(self, ncam=MAX_CAMS):
        return dict(made_total=self.made_total, first_store=self.first_store, made=list(self.made)[:ncam], n_busy=list(self.n_busy)[:ncam],
                    n_alive=list(self.n_alive)[:ncam])


class MapTransformResult(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int), ("n_refreshed", ctypes.c_int), ("n_no_rays", ctypes.c_int), ("n_no_source", ctypes.c_int), ("n_mkfs", ctypes.c_int)]

    def as_dict(self):
        return {f[0]: getattr(self, f[0]) for f in self._fields_}


def _life_lib():
    L = lib()
    if getattr(L, "_mcp_life_bound", False):
        return L
    vp, ip, dp = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    L.mcp_init_depth_map_points.argtypes = [vp, ip, vp, ip, vp, vp, vp, vp, vp, vp]
    L.mcp_map_mark_optimized.argtypes = [vp, vp]
    L.mcp_map_rescale.argtypes = [vp, dp, vp, vp]
    L.mcp_map_transform.argtypes = [vp, vp, vp]
    L.mcp_init_depth_points_host.argtypes = [ip, vp, vp, vp, vp, vp, vp, vp, vp, ip, vp, vp, ip, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mcp_map_mark_optimized_host.argtypes = [ip, ip, vp, vp]
    L.mcp_map_transform_host.argtypes = [ip, dp, vp, ip, vp, ip, vp, vp, ip, ip, vp, vp, vp, vp, vp, vp, vp, vp]
    L.mcp_map_life_last_timing.argtypes = [vp, vp, vp]
    for n in LIFE_SYMBOLS:
        getattr(L, n).restype = ip
    L._mcp_life_bound = True
    return L


def _cand_lists(cands):
    from .stereo import _cand
    cs = [_cand(c) for c in cands]
    return cs, np.array([len(c) for c in cs], dtype=np.int32)


def _point_dtype():
    from .stereo import STEREO_POINT_DTYPE
    return STEREO_POINT_DTYPE


def init_depth_ref(cam_from_base, src_base_from_world, cams, cands, limits, busy, rows, src_mkf, level, init_depth, first_store=0):
    """AddInitDepthMapPoints (src/MapMakerServerBase.cc:499-546) of one MKF at one level over flat arrays: per camera c ThinCandidates against busy[c]
    (STEREO_MEAS_DTYPE, the keyframe's measurements), then the first limits[c] survivors in candidate order become points at init_depth along
    their unprojected ray, with the three patch rays and RefreshPixelVectors.  cams: TaylorCamera objects; cands: per camera (n, 2) level
    positions.  Point k (camera-major, then candidate order) takes rows[k].  Returns a dict: keep (per camera bool arrays), made, n_alive, n_busy,
    points (STEREO_POINT_DTYPE) and what the points become in the map, as stereo_append_ref names it, with ONE store entry each."""
    from . import stereo as S
    cfb = _f64(cam_from_base).reshape(-1, 12)
    bfw = _f64(src_base_from_world).reshape(12)
    cs, _ = _cand_lists(cands)
    r = _i32(rows)
    keep, made, alive, nbusy, recs, cam_of = [], [], [], [], [], []
    for c, cam in enumerate(cams):
        Rw, tw = _compose(cfb[c, :9].reshape(3, 3), cfb[c, 9:], bfw[:9].reshape(3, 3), bfw[9:])      # CamFromWorld = CamFromBase * BaseFromWorld
        b = np.asarray(busy[c], dtype=S.STEREO_MEAS_DTYPE)
        k = S.thin_candidates(cs[c], level, b["root_pos"], b["level"]) if len(cs[c]) else np.zeros(0, dtype=bool)
        keep.append(k)
        take = np.flatnonzero(k)[:int(limits[c])]
        alive.append(int(k.sum())); made.append(len(take)); nbusy.append(len(b))
        p = np.zeros(len(take), dtype=S.STEREO_POINT_DTYPE)
        for j, i in enumerate(take):
            root, ce, ri, dn = S.probe(cam, level, cs[c][i])
            ray = cam.unproject(root)[0]                                   # v3UnProj = UnProject(v2RootPos) * dInitDepth
            world = Rw.T @ (ray * float(init_depth) - tw)                  # mse3CamFromWorld.inverse() * v3UnProj
            pr, pd = S.pixel_vectors((Rw, tw), ce, ri, dn, world)
            p[j] = (i, -1, 0, 0, world, root, (0.0, 0.0), ce, ri, dn, pr[0], pd[0])
        recs.append(p); cam_of += [c] * len(take)
    pts = np.concatenate(recs) if recs else np.zeros(0, dtype=S.STEREO_POINT_DTYPE)
    n = len(pts)
    if n > len(r):
        raise ValueError("init_depth_ref: fewer rows than points")
    cam_of = np.array(cam_of, dtype=np.int32)
    ap = np.zeros(n, dtype=STORE_ENTRY_DTYPE)
    ap["uv"], ap["mkf"], ap["cam"], ap["row"], ap["level"], ap["source"], ap["alive"] = pts["root_pos"], src_mkf, cam_of, r[:n], level, SRC_ROOT, 1
    centre = np.concatenate([cs[c][np.flatnonzero(keep[c])[:made[c]]] for c in range(len(cams))]).astype(np.int32).reshape(n, 2) if n else np.zeros((0, 2), np.int32)
    return dict(keep=keep, made=made, n_alive=alive, n_busy=nbusy, made_total=n, points=pts, world_pos=pts["world_pos"].copy(),
                pixel_right_w=pts["pixel_right_w"].copy(), pixel_down_w=pts["pixel_down_w"].copy(), usable=np.zeros(n, dtype=np.uint8),
                inlier=np.ones(n, dtype=np.int32), outlier=np.zeros(n, dtype=np.int32),
                rays=np.concatenate([pts["center_nc"], pts["one_right_nc"], pts["one_down_nc"]], axis=1).reshape(n, 9),
                source_level=np.full(n, level, dtype=np.int32), center_xy=centre, fixed=np.zeros(n, dtype=np.uint8),
                gp_src_mkf=np.full(n, src_mkf, dtype=np.int32), gp_src_cam=cam_of, gp_flags=np.zeros(n, dtype=np.int32), appended=ap,
                store_end=int(first_store) + n)


def init_depth_host(cam_from_base, src_base_from_world, cams, cands, limits, busy, rows, src_mkf, level, init_depth, first_store=0):
    """mcp_init_depth_points_host: the bodies the kernels call, under the host compiler.  Needs no device.  Arguments and result as init_depth_ref
    (the constant columns -- usable, counts, level, fixed -- are the kernel's own and are not returned).  A refusal raises RuntimeError."""
    from .stereo import STEREO_MEAS_DTYPE
    from .taylor_camera import camera_array
    cfb = _f64(cam_from_base).reshape(-1, 12)
    nc = len(cfb)
    bfw = _f64(src_base_from_world).reshape(12)
    cs, ncand = _cand_lists(cands)
    cand = np.ascontiguousarray(np.concatenate(cs)) if nc else np.zeros((0, 2), np.int32)
    bs = [np.ascontiguousarray(b, dtype=STEREO_MEAS_DTYPE) for b in busy]
    nb = np.array([len(b) for b in bs], dtype=np.int32)
    bcat = np.ascontiguousarray(np.concatenate(bs)) if nc else np.zeros(0, dtype=STEREO_MEAS_DTYPE)
    lim = _i32(limits, (nc,))
    r = _i32(rows)
    m = max(len(r), 1)
    arr = camera_array(cams)
    prm, res = InitDepthParams(int(src_mkf), int(level), float(init_depth)), InitDepthResult()
    keep = np.zeros(max(len(cand), 1), dtype=np.uint8)
    o = dict(points=np.zeros(m, dtype=_point_dtype()), world_pos=np.zeros((m, 3)), pixel_right_w=np.zeros((m, 3)), pixel_down_w=np.zeros((m, 3)), rays=np.zeros((m, 9)),
             center_xy=np.zeros((m, 2), np.int32), gp_src_mkf=np.zeros(m, np.int32), gp_src_cam=np.zeros(m, np.int32), gp_flags=np.zeros(m, np.int32),
             appended=np.zeros(m, dtype=STORE_ENTRY_DTYPE))
    n = _chk(_life_lib().mcp_init_depth_points_host(nc, cfb.ctypes.data, bfw.ctypes.data, ctypes.addressof(arr), ncand.ctypes.data, cand.ctypes.data if len(cand) else None,
                                                    lim.ctypes.data, nb.ctypes.data, bcat.ctypes.data if len(bcat) else None, len(r), r.ctypes.data if len(r) else None,
                                                    ctypes.addressof(prm), int(first_store), ctypes.addressof(res), keep.ctypes.data,
                                                    *[o[k].ctypes.data for k in ("points", "world_pos", "pixel_right_w", "pixel_down_w", "rays", "center_xy", "gp_src_mkf",
                                                                                 "gp_src_cam", "gp_flags", "appended")]), "init_depth_points_host")
    out = {k: v[:n] for k, v in o.items()}
    off = np.concatenate([[0], np.cumsum(ncand)])
    out.update(res.as_dict(nc), keep=[keep[off[c]:off[c + 1]].astype(bool) for c in range(nc)], store_end=int(first_store) + n)
    return out


def mark_optimized_ref(usable, point_flags):
    """The loop at src/MapMakerServerBase.cc:212-215 over the table: usable = 1 on every row the graph's point columns cover and do not call bad.
    point_flags: the columns of the rows written or filled so far (the rest of the table was never written).  Returns (usable, count)."""
    u = np.array(usable, dtype=np.uint8)
    pf = _i32(point_flags)
    hit = np.zeros(len(u), dtype=bool)
    n = min(len(u), len(pf))
    hit[:n] = (pf[:n] & GP_BAD) == 0
    u[hit] = 1
    return u, int(hit.sum())


def mark_optimized_host(usable, point_flags):
    """mcp_map_mark_optimized_host (no device): (usable, count)."""
    u = np.ascontiguousarray(usable, dtype=np.uint8).copy()
    pf = _i32(point_flags)
    n = _chk(_life_lib().mcp_map_mark_optimized_host(len(u), len(pf), pf.ctypes.data if len(pf) else None, u.ctypes.data if len(u) else None), "map_mark_optimized_host")
    return u, n


def _xform_args(scale, new_from_old):
    if (scale is None) == (new_from_old is None):
        raise ValueError("give either scale or new_from_old (R, t)")
    if scale is not None:
        return XFORM_SCALE, float(scale), None
    R, t = new_from_old
    return XFORM_RIGID, 1.0, np.ascontiguousarray(np.concatenate([np.asarray(R, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)]))


def _row_sources(a, n_rows):
    """(src_mkf, src_cam, has a present source keyframe of the rig) per table row; rows past the graph's point columns have no source"""
    sm, sc = np.full(n_rows, -1, dtype=np.int64), np.zeros(n_rows, dtype=np.int64)
    k = min(n_rows, len(a["src_mkf"]))
    sm[:k], sc[:k] = np.asarray(a["src_mkf"])[:k], np.asarray(a["src_cam"])[:k]
    mf = np.asarray(a["mkf_flags"])
    ok = (sm >= 0) & (sm < len(mf)) & (sc >= 0) & (sc < a["ncam"])
    ok[ok] = (mf[sm[ok]] & MKF_PRESENT) != 0
    return sm, sc, ok


def map_transform_ref(a, scale=None, new_from_old=None):
    """ApplyGlobalScaleToMap (src/MapMakerServerBase.cc:549-574) or ApplyGlobalTransformationToMap (:577-596) over flat arrays, without the scene
    depths.  a: ncam, cam_from_base, base_from_world (P, 12), mkf_flags, src_mkf / src_cam (the graph's point columns), has_rays, rays (N, 9),
    world_pos, pixel_right_w, pixel_down_w (N, 3).  Every present MKF moves; a row whose column names a present MKF and a camera of the rig gets
    its new world position and, with rays, RefreshPixelVectors at its source keyframe's NEW CamFromWorld; other rows keep their values.  Returns
    (dict(base_from_world, world_pos, pixel_right_w, pixel_down_w), counters)."""
    from .stereo import pixel_vectors
    kind, s, T = _xform_args(scale, new_from_old)
    bfw = _f64(a["base_from_world"]).reshape(-1, 12).copy()
    mf = _i32(a["mkf_flags"])
    pres = (mf & MKF_PRESENT) != 0
    if kind == XFORM_SCALE:
        bfw[pres, 9:] *= s                                                         # mse3BaseFromWorld.get_translation() *= dScale
    else:
        Rn, tn = T[:9].reshape(3, 3), T[9:]
        Ri, ti = Rn.T, -(Rn.T @ tn)                                                # se3NewFromOld.inverse()
        for k in np.flatnonzero(pres):
            Rb, tb = bfw[k, :9].reshape(3, 3), bfw[k, 9:]
            bfw[k, :9], bfw[k, 9:] = (Rb @ Ri).reshape(9), Rb @ ti + tb            # mse3BaseFromWorld * se3NewFromOld.inverse()
    wp, pr, pd = (_f64(a[k]).reshape(-1, 3).copy() for k in ("world_pos", "pixel_right_w", "pixel_down_w"))
    N = len(wp)
    rays, has = _f64(a["rays"]).reshape(-1, 9), np.asarray(a["has_rays"]).astype(bool)
    cfb = _f64(a["cam_from_base"]).reshape(-1, 12)
    sm, sc, ok = _row_sources(a, N)
    for r in np.flatnonzero(ok):
        wp[r] = wp[r] * s if kind == XFORM_SCALE else Rn @ wp[r] + tn
        if has[r]:
            Rw, tw = _compose(cfb[sc[r], :9].reshape(3, 3), cfb[sc[r], 9:], bfw[sm[r], :9].reshape(3, 3), bfw[sm[r], 9:])
            a_, b_ = pixel_vectors((Rw, tw), rays[r, :3], rays[r, 3:6], rays[r, 6:], wp[r])
            pr[r], pd[r] = a_[0], b_[0]
    cnt = dict(n_rows=N, n_refreshed=int((ok & has).sum()), n_no_rays=int((ok & ~has).sum()), n_no_source=int((~ok).sum()), n_mkfs=int(pres.sum()))
    return dict(base_from_world=bfw, world_pos=wp, pixel_right_w=pr, pixel_down_w=pd), cnt


def map_transform_host(a, scale=None, new_from_old=None):
    """mcp_map_transform_host: the bodies the kernels call, under the host compiler.  Needs no device.  Arguments and result as map_transform_ref."""
    kind, s, T = _xform_args(scale, new_from_old)
    cfb = _f64(a["cam_from_base"]).reshape(-1, 12)
    bfw = _f64(a["base_from_world"]).reshape(-1, 12).copy()
    mf = _i32(a["mkf_flags"], (len(bfw),))
    wp, pr, pd = (_f64(a[k]).reshape(-1, 3).copy() for k in ("world_pos", "pixel_right_w", "pixel_down_w"))
    N = len(wp)
    rays, has = _f64(a["rays"]).reshape(-1, 9), _u8(a["has_rays"], (N,))
    sm, sc = _i32(a["src_mkf"]), _i32(a["src_cam"], (len(a["src_mkf"]),))
    res = MapTransformResult()
    p = lambda x: x.ctypes.data if x.size else None      # noqa: E731
    _chk(_life_lib().mcp_map_transform_host(kind, s, None if T is None else T.ctypes.data, int(a["ncam"]), cfb.ctypes.data, len(bfw), p(bfw), p(mf), N, len(sm), p(sm), p(sc),
                                            p(has), p(rays), p(wp), p(pr), p(pd), ctypes.addressof(res)), "map_transform_host")
    return dict(base_from_world=bfw, world_pos=wp, pixel_right_w=pr, pixel_down_w=pd), res.as_dict()


# ---- the device graph ----------------------------------------------------------------------------------------------------------------------
class MapGraph:
    """The device-resident map graph of one MapPointTable (which must outlive it).  Slots are MKF indices, rows are the table's rows."""

    def __init__(self, table, cam_from_base, cams=None):
        self._L = lib()
        self.table = table
        self.cam_from_base = _f64(cam_from_base).reshape(-1, 12).copy()
        self.ncam = len(self.cam_from_base)
        self.cams = cams
        self.base_from_world = np.zeros((MAX_MKFS, 12))          # the host's copy of the poses uploaded (what select() builds its Problem from)
        self._h = self._L.mcp_map_graph_create(table._h, self.ncam, self.cam_from_base.ctypes.data)
        if not self._h:
            raise RuntimeError("mcp_map_graph_create failed: " + _cb.last_error())
        table._open_graphs = getattr(table, "_open_graphs", 0) + 1     # the table's handle is destroyed after its last graph's (MapPointTable.close)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mcp_map_graph_destroy(self._h)
            self._h = None
            self.table._open_graphs -= 1
            if self.table._open_graphs == 0 and getattr(self.table, "_close_pending", False):
                self.table.close()

    def __del__(self):
        self.close()

    @classmethod
    def from_problem(cls, table, p, depth_mean=None, arrays=None):
        """The graph (and the table's rows) of a multi-mode synth.Problem: slots = MKF indices, rows = point indices, world positions computed
        on the host from pt_x, measurements appended in the Problem's order.  arrays: problem_arrays(p) when the caller has them already."""
        a = problem_arrays(p, depth_mean) if arrays is None else arrays
        N = len(a["pt_flags"])
        z = np.zeros((N, 3))
        if N:
            table.set(a["world_pos"], z, z, np.ones(N, dtype=np.uint8))
        g = cls(table, a["cam_from_base"], cams=p.cams)
        g.load_arrays(a)
        return g

    def load_arrays(self, a):
        """MKF columns, point columns and the store from flat arrays (problem_arrays' keys); dead entries of `a` are added and erased."""
        P, N, M = len(a["mkf_flags"]), len(a["pt_flags"]), len(a["ms_mkf"])
        if P:
            self.set_mkfs(a["base_from_world"], a["mkf_flags"], a["kf_active"], a["kf_depth_mean"])
        if N:
            self.update_points(np.arange(N), a["src_mkf"], a["src_cam"], a["pt_flags"])
        if M:
            self.add_meas(a["ms_mkf"], a["ms_cam"], a["ms_row"], a["ms_uv"], a["ms_level"], a["ms_source"])
            dead = np.flatnonzero(np.asarray(a["ms_alive"]) == 0)
            if len(dead):
                died = self.erase_meas(np.asarray(a["ms_mkf"])[dead], np.asarray(a["ms_cam"])[dead], np.asarray(a["ms_row"])[dead])
                assert died == len(dead), (died, len(dead))

    def _mkf_args(self, n, base_from_world, flags, kf_active, kf_depth_mean):
        return _f64(base_from_world, (n, 12)), _i32(flags, (n,)), _u8(kf_active, (n, self.ncam)), _f64(kf_depth_mean, (n, self.ncam))

    def set_mkfs(self, base_from_world, flags, kf_active, kf_depth_mean, first=0):
        n = len(flags)
        b, f, a, d = self._mkf_args(n, base_from_world, flags, kf_active, kf_depth_mean)
        _chk(self._L.mcp_map_graph_set_mkfs(self._h, int(first), n, b.ctypes.data, f.ctypes.data, a.ctypes.data, d.ctypes.data), "map_graph_set_mkfs")
        self.base_from_world[first:first + n] = b

    def update_mkfs(self, slots, base_from_world, flags, kf_active, kf_depth_mean):
        s = _i32(slots)
        n = len(s)
        b, f, a, d = self._mkf_args(n, base_from_world, flags, kf_active, kf_depth_mean)
        _chk(self._L.mcp_map_graph_update_mkfs(self._h, n, s.ctypes.data, b.ctypes.data, f.ctypes.data, a.ctypes.data, d.ctypes.data), "map_graph_update_mkfs")
        self.base_from_world[s] = b

    def update_points(self, rows, src_mkf, src_cam, flags):
        r = _i32(rows)
        n = len(r)
        sm, sc, f = _i32(src_mkf, (n,)), _i32(src_cam, (n,)), _i32(flags, (n,))
        _chk(self._L.mcp_map_graph_update_points(self._h, n, r.ctypes.data, sm.ctypes.data, sc.ctypes.data, f.ctypes.data), "map_graph_update_points")

    def add_meas(self, mkf, cam, row, uv, level, source=None):
        """Appends in the given order; returns the store index of the first new entry."""
        m = _i32(mkf)
        n = len(m)
        c, r, u, l = _i32(cam, (n,)), _i32(row, (n,)), _f64(uv, (n, 2)), _i32(level, (n,))
        s = np.zeros(n, dtype=np.int32) if source is None else _i32(source, (n,))
        return _chk(self._L.mcp_map_graph_add_meas(self._h, n, m.ctypes.data, c.ctypes.data, r.ctypes.data, u.ctypes.data, l.ctypes.data, s.ctypes.data), "map_graph_add_meas")

    def get_points(self, first=0, count=None):
        """mcp_map_gp_get: the point columns of rows first .. first+count-1 read back, dict(src_mkf, src_cam, flags); a row they do not cover yet
        reads as never written (-1, 0, GP_BAD)."""
        from .stereo import lib as _stereo_lib
        count = self.table.rows - first if count is None else int(count)
        n = max(count, 1)
        o = dict(src_mkf=np.zeros(n, np.int32), src_cam=np.zeros(n, np.int32), flags=np.zeros(n, np.int32))
        _chk(_stereo_lib().mcp_map_gp_get(self._h, int(first), count, *[o[k].ctypes.data for k in ("src_mkf", "src_cam", "flags")]), "map_gp_get")
        return {k: v[:count] for k, v in o.items()}

    def add_stereo_points(self, src, src_cam, src_pose, level, cand, targets, target_mkf, target_cam, rows, keys, src_mkf, src_cam_index, **kw):
        """mcp_stereo_map_points: AddStereoMapPoints of one source keyframe and level whose created points take rows[k] / keys[k] of the table and
        two entries of the store on the device -- see mcptam_amd.stereo.stereo_map_points, whose result it returns."""
        from .stereo import stereo_map_points
        return stereo_map_points(self, src, src_cam, src_pose, level, cand, targets, target_mkf, target_cam, rows, keys, src_mkf, src_cam_index, **kw)

    # ---- the map's beginning, its rescale and its re-alignment (mcp_init_depth_map_points, mcp_map_mark_optimized, mcp_map_rescale, mcp_map_transform) ----
    def add_init_depth_points(self, srcs, cams, cands, limits, rows, keys, src_mkf, level, init_depth, want_points=True):
        """mcp_init_depth_map_points: AddInitDepthMapPoints of MKF slot src_mkf at `level`, every camera of the rig in one call.  srcs: the
        keyframes (KeyFrame or None for a camera without candidates), cams: their TaylorCameras, cands: per camera (n, 2) level positions,
        limits: nLimit per camera.  Created point k (camera-major, then candidate order) takes rows[k] / keys[k] and one store entry.  Returns
        (points (STEREO_POINT_DTYPE) or None, keep masks per camera, dict of mcp_init_depth_result)."""
        L = _life_lib()
        cs, ncand = _cand_lists(cands)
        nc = len(cs)
        if not (len(srcs) == len(cams) == len(limits) == nc):
            raise ValueError("add_init_depth_points: lengths differ")
        structs = [c.to_struct() for c in cams]
        tab = (InitDepthCam * max(nc, 1))()
        for c in range(nc):
            tab[c].src = srcs[c]._h if srcs[c] is not None else None
            tab[c].cam = ctypes.addressof(structs[c])
            tab[c].n_cand, tab[c].cand, tab[c].limit = int(ncand[c]), (cs[c].ctypes.data if len(cs[c]) else None), int(limits[c])
        r, k = _i32(rows), _i32(keys)
        if len(r) != len(k):
            raise ValueError("add_init_depth_points: rows and keys differ in length")
        total = int(ncand.sum())
        out = np.zeros(max(len(r), 1), dtype=_point_dtype()) if want_points else None
        keep = np.zeros(max(total, 1), dtype=np.uint8)
        prm, res = InitDepthParams(int(src_mkf), int(level), float(init_depth)), InitDepthResult()
        n = _chk(L.mcp_init_depth_map_points(self._h, nc, ctypes.addressof(tab), len(r), r.ctypes.data if len(r) else None, k.ctypes.data if len(k) else None,
                                             ctypes.addressof(prm), ctypes.addressof(res), out.ctypes.data if out is not None else None, keep.ctypes.data),
                 "init_depth_map_points")
        del structs
        off = np.concatenate([[0], np.cumsum(ncand)])
        return (out[:n].copy() if out is not None else None), [keep[off[c]:off[c + 1]].astype(bool) for c in range(nc)], res.as_dict(nc)

    def mark_optimized(self):
        """mcp_map_mark_optimized: usable = 1 on every row whose graph column has been written and is not GP_BAD (the end of
        InitFromMultiKeyFrame).  Returns the number of rows named."""
        n = ctypes.c_int(0)
        _chk(_life_lib().mcp_map_mark_optimized(self._h, ctypes.addressof(n)), "map_mark_optimized")
        return n.value

    def _refresh_pose_mirror(self):
        m = self.get_mkfs()
        pres = (m["flags"] & MKF_PRESENT) != 0
        self.base_from_world[pres] = m["base_from_world"][pres]

    def rescale(self, scale, want_depth=True):
        """mcp_map_rescale: ApplyGlobalScaleToMap over the resident map.  Returns (dict of mcp_map_transform_result, SCENE_DEPTH_DTYPE records of
        the present slots x ncam in ascending slot order, or None)."""
        from .pvs import SCENE_DEPTH_DTYPE
        res = MapTransformResult()
        depth = np.zeros(MAX_MKFS * self.ncam, dtype=SCENE_DEPTH_DTYPE) if want_depth else None
        _chk(_life_lib().mcp_map_rescale(self._h, float(scale), ctypes.addressof(res), depth.ctypes.data if depth is not None else None), "map_rescale")
        self._refresh_pose_mirror()
        return res.as_dict(), (depth[:res.n_mkfs * self.ncam].copy() if depth is not None else None)

    def transform(self, R, t):
        """mcp_map_transform: ApplyGlobalTransformationToMap with se3NewFromOld = (R, t).  Returns the dict of mcp_map_transform_result."""
        T = _xform_args(None, (R, t))[2]
        res = MapTransformResult()
        _chk(_life_lib().mcp_map_transform(self._h, T.ctypes.data, ctypes.addressof(res)), "map_transform")
        self._refresh_pose_mirror()
        return res.as_dict()

    def life_last_timing(self):
        """Device times in ms of the last add_init_depth_points() and of the last rescale() / transform(); -1 before the first."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _chk(_life_lib().mcp_map_life_last_timing(self._h, ctypes.addressof(a), ctypes.addressof(b)), "map_life_last_timing")
        return a.value, b.value

    def erase_meas(self, mkf, cam, row):
        """KeyFrame::EraseMeasurementOfPoint for distinct keys; returns how many live entries died."""
        m = _i32(mkf)
        n = len(m)
        c, r = _i32(cam, (n,)), _i32(row, (n,))
        return _chk(self._L.mcp_map_graph_erase_meas(self._h, n, m.ctypes.data, c.ctypes.data, r.ctypes.data), "map_graph_erase_meas")

    def erase_mkf(self, slot):
        return _chk(self._L.mcp_map_graph_erase_mkf(self._h, int(slot)), "map_graph_erase_mkf")

    def compact(self):
        """Stable removal of the dead entries: store indices change."""
        _chk(self._L.mcp_map_graph_compact(self._h), "map_graph_compact")

    def num_meas(self):
        live, stored = ctypes.c_int(0), ctypes.c_int(0)
        _chk(self._L.mcp_map_graph_num_meas(self._h, ctypes.addressof(live), ctypes.addressof(stored)), "map_graph_num_meas")
        return live.value, stored.value

    def get_meas(self, first=0, count=None):
        count = self.num_meas()[1] - first if count is None else int(count)
        n = max(count, 1)
        o = dict(mkf=np.zeros(n, np.int32), cam=np.zeros(n, np.int32), row=np.zeros(n, np.int32), uv=np.zeros((n, 2)), level=np.zeros(n, np.int32),
                 source=np.zeros(n, np.int32), alive=np.zeros(n, np.uint8))
        _chk(self._L.mcp_map_graph_get_meas(self._h, int(first), count, *[o[k].ctypes.data for k in ("mkf", "cam", "row", "uv", "level", "source", "alive")]), "map_graph_get_meas")
        return {k: v[:count] for k, v in o.items()}

    def good_counts(self, first=0, count=None):
        count = self.table.rows - first if count is None else int(count)
        out = np.zeros(max(count, 1), dtype=np.int32)
        _chk(self._L.mcp_map_graph_good_counts(self._h, int(first), count, out.ctypes.data), "map_graph_good_counts")
        return out[:count]

    def check(self):
        """(duplicates among the live entries, dead entries): a host sort of the read-back keys, for tests and adapters under development."""
        d, x = ctypes.c_int(0), ctypes.c_int(0)
        _chk(self._L.mcp_map_graph_check(self._h, ctypes.addressof(d), ctypes.addressof(x)), "map_graph_check")
        return d.value, x.value

    def views(self, copy=True):
        """(mkfs, points, meas) of the last select: structured arrays over the library's pinned block (valid until the next select) or copies."""
        out = []
        for fn, dt in ((self._L.mcp_map_bundle_mkfs_view, MKF_DTYPE), (self._L.mcp_map_bundle_points_view, POINT_DTYPE), (self._L.mcp_map_bundle_meas_view, MEAS_DTYPE)):
            cnt = ctypes.c_int(0)
            ptr = fn(self._h, ctypes.byref(cnt))
            v = np.frombuffer((ctypes.c_char * (cnt.value * dt.itemsize)).from_address(ptr), dtype=dt) if cnt.value else np.zeros(0, dtype=dt)
            out.append(v.copy() if copy else v)
        return tuple(out)

    def last_timing(self):
        """Device time of the last select's submission in ms (between two events on the table's stream)."""
        ms = ctypes.c_double(0.0)
        _chk(self._L.mcp_map_bundle_select_last_timing(self._h, ctypes.addressof(ms)), "map_bundle_select_last_timing")
        return ms.value

    # ---- the keyframe lists and the write-back over the graph (mcp_graph_*) ----
    def get_mkfs(self, first=0, count=MAX_MKFS):
        """MKF slots first .. first+count-1 read back: dict(base_from_world (count, 12), flags, kf_active (count, ncam), kf_depth_mean)."""
        n = max(int(count), 1)
        o = dict(base_from_world=np.zeros((n, 12)), flags=np.zeros(n, dtype=np.int32), kf_active=np.zeros((n, self.ncam), dtype=np.uint8), kf_depth_mean=np.zeros((n, self.ncam)))
        _chk(self._L.mcp_graph_get_mkfs(self._h, int(first), int(count), *[o[k].ctypes.data for k in ("base_from_world", "flags", "kf_active", "kf_depth_mean")]), "graph_get_mkfs")
        return {k: v[:count] for k, v in o.items()}

    def debug_kf_lists(self, slots, blocks=0):
        """mcp_graph_debug_kf_lists: (seg_start, seg_rows, seg_w) of the keyframes (slots[i], c) as the device builds them; blocks: the chunk
        count forced (1..LIST_MAX_BLOCKS), 0 for the default grid."""
        sl = _i32(slots)
        cap = max(self.num_meas()[1], 1)
        ss = np.zeros(len(sl) * self.ncam + 1, dtype=np.int32)
        sr, sw = np.zeros(cap, dtype=np.int32), np.zeros(cap)
        tot = _chk(self._L.mcp_graph_debug_kf_lists(self._h, len(sl), sl.ctypes.data, int(blocks), ss.ctypes.data, cap, sr.ctypes.data, sw.ctypes.data), "graph_debug_kf_lists")
        return ss, sr[:tot].copy(), sw[:tot].copy()

    def refresh_depth(self, slots):
        """mcp_graph_refresh_depth: MultiKeyFrame::RefreshSceneDepthRobust of the named MKFs at the graph's own poses; the means go into the
        graph.  Returns the (len(slots) * ncam,) SCENE_DEPTH_DTYPE records."""
        from .pvs import SCENE_DEPTH_DTYPE
        sl = _i32(slots)
        out = np.zeros(len(sl) * self.ncam, dtype=SCENE_DEPTH_DTYPE)
        _chk(self._L.mcp_graph_refresh_depth(self._h, len(sl), sl.ctypes.data, out.ctypes.data), "graph_refresh_depth")
        return out

    def write_back(self, bundle, point_ids, rows, src_chains=None, src_chain_len=None, slots=(), mkf_pose_ids=(), cam_pose_ids=(), outputs=True):
        """mcp_graph_write_back: AdjustAndUpdate from `bundle` into the table and the graph.  The point half is MapPointTable.write_back's;
        keyframe i * ncam + c is the chain {mkf_pose_ids[i], cam_pose_ids[c]} and the graph's (slots[i], c).  Returns a dict: world_pos,
        pixel_right_w, pixel_down_w (n, 3), kf_cam_from_world (n_kf, 12), depth (SCENE_DEPTH_DTYPE), base_from_world (n_mkfs, 12) -- or None
        with outputs=False.  The adjusted poses (96 B per MKF) are fetched either way: the host's copy self.base_from_world follows."""
        from .pvs import SCENE_DEPTH_DTYPE
        pid, rw = _i32(point_ids), _i32(rows)
        n = len(pid)
        if len(rw) != n:
            raise ValueError("write_back: point_ids and rows differ in length")
        stride, sc, sl_ = 1, None, None
        if src_chains is not None:
            sc = np.ascontiguousarray(np.asarray(src_chains, dtype=np.int32).reshape(n, -1))
            sl_ = _i32(src_chain_len, (n,))
            stride = sc.shape[1]
        s, mp, cp = _i32(slots), _i32(mkf_pose_ids), _i32(cam_pose_ids)
        if len(mp) != len(s) or (len(s) and len(cp) != self.ncam):
            raise ValueError("write_back: one pose id per slot and one per camera of the rig")
        n_kf = len(s) * self.ncam
        res = None
        if outputs:
            res = dict(world_pos=np.zeros((n, 3)), pixel_right_w=np.zeros((n, 3)), pixel_down_w=np.zeros((n, 3)), kf_cam_from_world=np.zeros((n_kf, 12)),
                       depth=np.zeros(n_kf, dtype=SCENE_DEPTH_DTYPE), base_from_world=np.zeros((len(s), 12)))
        bfw = res["base_from_world"] if outputs else np.zeros((len(s), 12))
        ptr = lambda a: None if a is None else a.ctypes.data
        o = (lambda k: res[k].ctypes.data) if outputs else (lambda k: None)
        _chk(self._L.mcp_graph_write_back(bundle._h, self._h, n, ptr(pid), ptr(rw), ptr(sc), stride, ptr(sl_), o("world_pos"), o("pixel_right_w"), o("pixel_down_w"),
                                          len(s), ptr(s), ptr(mp), ptr(cp), o("kf_cam_from_world"), o("depth"), bfw.ctypes.data), "graph_write_back")
        if len(s):
            self.base_from_world[s] = bfw
        return res

    def commit_parcel(self, parcel, lane_mkf, lane_cam, cross_camera=1, source=SRC_TRACKER):
        """mcp_meas_parcel_commit: the entries of `parcel` that are still good, judged by the map as it is now, appended to the store in parcel
        order.  lane_mkf / lane_cam: the MKF slot (< 0: the lane is withheld) and camera index of each lane.  Returns (dict of
        mcp_parcel_commit_result, lane_appended)."""
        lm = _i32(lane_mkf)
        lc = _i32(lane_cam, lm.shape)
        prm, res = ParcelCommitParams(int(cross_camera), int(source)), ParcelCommitResult()
        la = np.zeros(max(len(lm), 1), dtype=np.int32)
        _chk(self._L.mcp_meas_parcel_commit(self._h, parcel._h, len(lm), lm.ctypes.data, lc.ctypes.data, ctypes.addressof(prm), ctypes.addressof(res), la.ctypes.data),
             "meas_parcel_commit")
        return res.as_dict(), la[:len(lm)]

    # ---- outliers and bad points (mcp_map_cull_*) ----
    def cull_outliers(self, mkf, cam, row, bad_good_count=2):
        """mcp_map_cull_outliers: MapMakerServerBase::HandleOutliers for the keys (mkf slot, cam, row) in the solver's order.  Returns (dict of
        mcp_cull_outliers_result, verdicts uint8 (n,): CULL_*)."""
        m, c, r = _cull_keys(mkf, cam, row)
        n = len(m)
        prm, res = CullOutliersParams(int(bad_good_count)), CullOutliersResult()
        vd = np.zeros(max(n, 1), dtype=np.uint8)
        _chk(self._L.mcp_map_cull_outliers(self._h, n, m.ctypes.data, c.ctypes.data, r.ctypes.data, ctypes.addressof(prm), vd.ctypes.data, ctypes.addressof(res)), "map_cull_outliers")
        return res.as_dict(), vd[:n]

    def cull_sweep(self, min_outliers=20, outlier_multiplier=1.0, danglers=True):
        """mcp_map_cull_sweep: danglers and tracker outliers marked bad, the measurements of every bad row erased, its table row made unusable.
        Returns (dict of mcp_cull_sweep_result, the rows the device turned bad since the last sweep, ascending: a copy of the pinned view)."""
        prm, res = CullSweepParams(int(min_outliers), int(bool(danglers)), float(outlier_multiplier)), CullSweepResult()
        _chk(self._L.mcp_map_cull_sweep(self._h, ctypes.addressof(prm), ctypes.addressof(res)), "map_cull_sweep")
        return res.as_dict(), self.cull_rows()

    def cull_rows(self):
        """The report of the last sweep (mcp_map_cull_rows_view), copied."""
        cnt = ctypes.c_int(0)
        ptr = self._L.mcp_map_cull_rows_view(self._h, ctypes.byref(cnt))
        if not cnt.value:
            return np.zeros(0, dtype=np.int32)
        return np.frombuffer((ctypes.c_char * (4 * cnt.value)).from_address(ptr), dtype=np.int32).copy()

    def cull_last_timing(self):
        """(outliers_ms, sweep_ms): device time of the last submission of each call, -1 for one that has not run."""
        a, b = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _chk(self._L.mcp_map_cull_last_timing(self._h, ctypes.addressof(a), ctypes.addressof(b)), "map_cull_last_timing")
        return a.value, b.value

    # ---- closest-keyframe queries and the removal of an MKF (mcp_map_neighbours, mcp_map_mkf_cull) ----
    def neighbours(self, params=None, raw=False, **kw):
        """mcp_map_neighbours: (dict of status / count / n_candidates, the winners as a NEIGH_ITEM_DTYPE array), or with raw the NeighResult
        itself.  params: a NeighParams, or neigh_params' keywords."""
        p = _as_neigh_params(kw if params is None else params)
        res = NeighResult()
        _chk(self._L.mcp_map_neighbours(self._h, ctypes.addressof(p), ctypes.addressof(res)), "map_neighbours")
        return res if raw else (res.as_dict(), res.items())

    def neighbours_last_timing(self):
        """Device time of the last neighbours() submission in ms; -1 before the first."""
        ms = ctypes.c_double(0.0)
        _chk(self._L.mcp_map_neighbours_last_timing(self._h, ctypes.addressof(ms)), "map_neighbours_last_timing")
        return ms.value

    # ---- the co-visible points of the nearest keyframe (mcp_map_collect_nearest) ----
    def collect_nearest(self, base_from_world, depth_mean, mean_diff_fraction=0.5, active=None, cam_from_base=None, raw=False):
        """mcp_map_collect_nearest at the tracker's pose base_from_world (12,): (the report as a dict, the near mask, one byte per table row
        whose bit c says that the row is a co-visible point of the map keyframe nearest to current keyframe c), or with raw the CollectReport
        itself in place of the dict.  depth_mean, active: per camera of the rig; cam_from_base: the current keyframes', None for the rig's."""
        prm = collect_params(depth_mean, mean_diff_fraction, active)
        if len(np.asarray(depth_mean).reshape(-1)) != self.ncam:
            raise ValueError("collect_nearest: one depth mean per camera of the rig")
        b = _f64(base_from_world).reshape(12)
        cur = None if cam_from_base is None else _f64(cam_from_base).reshape(self.ncam, 12)
        rep, near = CollectReport(), np.zeros(self.table.rows, dtype=np.uint8)
        _chk(_bind_collect(self._L).mcp_map_collect_nearest(self._h, b.ctypes.data, None if cur is None else cur.ctypes.data, ctypes.addressof(prm), ctypes.addressof(rep),
                                                            near.ctypes.data), "map_collect_nearest")
        return (rep if raw else rep.as_dict()), near

    def collect_rows(self):
        """The near mask of the last collect_nearest (mcp_map_collect_rows_view), copied; empty after a frame's collection."""
        cnt = ctypes.c_int(0)
        ptr = _bind_collect(self._L).mcp_map_collect_rows_view(self._h, ctypes.byref(cnt))
        if not cnt.value:
            return np.zeros(0, dtype=np.uint8)
        return np.frombuffer((ctypes.c_char * cnt.value).from_address(ptr), dtype=np.uint8).copy()

    def collect_last_timing(self):
        """Device time of the collection launches of the last collection on the graph in ms (a frame's included); -1 before the first."""
        ms = ctypes.c_double(0.0)
        _chk(_bind_collect(self._L).mcp_map_collect_last_timing(self._h, ctypes.addressof(ms)), "map_collect_last_timing")
        return ms.value

    def n_closest_multi_keyframes(self, n, src_slot=-1, ext=None, want_meas=False, mean_diff_fraction=0.5):
        """MapMakerBase::NClosestMultiKeyFrames: the items, nearest first (bad MKFs included, with their flags)."""
        return self.neighbours(kind=NB_MKF, order=NB_NEAREST, src_slot=src_slot, ext=ext, n_max=n, want_meas=want_meas, mean_diff_fraction=mean_diff_fraction)[1]

    def closest_multi_keyframe(self, src_slot=-1, ext=None, **kw):
        """MapMakerBase::ClosestMultiKeyFrame: the item, or None where the reference asserts."""
        it = self.n_closest_multi_keyframes(1, src_slot, ext, **kw)
        return it[0] if len(it) else None

    def furthest_multi_keyframe(self, src_slot=-1, ext=None, mean_diff_fraction=0.5):
        """MapMakerBase::FurthestMultiKeyFrame: the item, or None (no other MKF at a distance > 0)."""
        it = self.neighbours(kind=NB_MKF, order=NB_FURTHEST, src_slot=src_slot, ext=ext, n_max=1, mean_diff_fraction=mean_diff_fraction)[1]
        return it[0] if len(it) else None

    def n_closest_keyframes(self, n, src_slot, src_cam, region=NB_ALL, same_cam=False, ext=None, max_dist=np.inf, want_meas=False, mean_diff_fraction=0.5):
        """MapMakerBase::NClosestKeyFrames: the items, nearest first."""
        return self.neighbours(kind=NB_KF, order=NB_NEAREST, src_slot=src_slot, src_cam=src_cam, region=region, same_cam=same_cam, ext=ext, n_max=n, max_dist=max_dist,
                               want_meas=want_meas, mean_diff_fraction=mean_diff_fraction)[1]

    def closest_keyframes_within_dist(self, src_slot, src_cam, max_dist, n_max=NB_MAX, region=NB_ALL, **kw):
        """MapMakerBase::ClosestKeyFramesWithinDist: at most n_max keyframes with distance <= max_dist, nearest first."""
        return self.n_closest_keyframes(n_max, src_slot, src_cam, region=region, max_dist=max_dist, **kw)

    def closest_keyframe(self, src_slot, src_cam, region=NB_ALL, same_cam=False, **kw):
        """MapMakerBase::ClosestKeyFrame: the item, or None (the reference returns NULL)."""
        it = self.n_closest_keyframes(1, src_slot, src_cam, region=region, same_cam=same_cam, **kw)
        return it[0] if len(it) else None

    def need_new_multi_keyframe(self, ext, total_depth_mean, n_present, max_scaled_dist=0.1, mean_diff_fraction=0.5):
        """MapMakerClientBase::NeedNewMultiKeyFrame(mkf) without the queue (src/MapMakerClientBase.cc:125-147): ext is the tracker's MKF,
        total_depth_mean its mdTotalDepthMean, n_present mlpMultiKeyFrames.size(), max_scaled_dist sdMaxScaledMKFDist."""
        it = self.closest_multi_keyframe(ext=ext, mean_diff_fraction=mean_diff_fraction)
        if it is None:
            raise ValueError("need_new_multi_keyframe: the map holds no MKF")
        dist = float(it["dist"]) * (1.0 / total_depth_mean)
        size = 1 if n_present == 2 else n_present
        return dist > max_scaled_dist * (1.0 - (1.0 / (0.5 + size)))

    def need_new_multi_keyframe_by_meas(self, ext, n_meas, mean_diff_fraction=0.5):
        """MapMakerClientBase::NeedNewMultiKeyFrame(mkf, nNumMeas) without the queue (:163-177): fewer measurements than 70% of the mean of
        the three closest MKFs'."""
        it = self.n_closest_multi_keyframes(3, ext=ext, want_meas=True, mean_diff_fraction=mean_diff_fraction)
        if not len(it):
            raise ValueError("need_new_multi_keyframe_by_meas: the map holds no MKF")
        return n_meas < 0.7 * (float(int(it["n_meas"].sum())) / len(it))

    def is_distance_to_nearest_mkf_excessive(self, ext, total_depth_mean_of, max_scaled_dist=0.1, mean_diff_fraction=0.5):
        """MapMakerClientBase::IsDistanceToNearestMultiKeyFrameExcessive (:203-211).  total_depth_mean_of: slot -> mdTotalDepthMean of that MKF
        (a callable, or something indexed by slot): the graph holds the keyframes' means, not the MKF's."""
        it = self.closest_multi_keyframe(ext=ext, mean_diff_fraction=mean_diff_fraction)
        if it is None:
            raise ValueError("is_distance_to_nearest_mkf_excessive: the map holds no MKF")
        tdm = total_depth_mean_of(int(it["slot"])) if callable(total_depth_mean_of) else total_depth_mean_of[int(it["slot"])]
        return float(it["dist"]) * (1.0 / tdm) > max_scaled_dist * 3

    def cull_mkf(self, slot=-1, furthest_from=-1, mark_points=True, max_kfs=2, erase=True, mean_diff_fraction=0.5):
        """mcp_map_mkf_cull: MarkFurthestMultiKeyFrameAsBad (slot == -1: the victim is the furthest MKF from furthest_from) and the removal of the
        victim from the store and the map, in one submission.  Returns the dict of mcp_mkf_cull_result.  The rows it marks are reported by the
        next cull_sweep."""
        prm, res = MkfCullParams(int(slot), int(furthest_from), int(bool(mark_points)), int(max_kfs), int(bool(erase)), float(mean_diff_fraction)), MkfCullResult()
        _chk(self._L.mcp_map_mkf_cull(self._h, ctypes.addressof(prm), ctypes.addressof(res)), "map_mkf_cull")
        return res.as_dict()

    def cull_mkf_last_timing(self):
        """Device time of the last cull_mkf() submission in ms; -1 before the first."""
        ms = ctypes.c_double(0.0)
        _chk(self._L.mcp_map_mkf_cull_last_timing(self._h, ctypes.addressof(ms)), "map_mkf_cull_last_timing")
        return ms.value

    def select_raw(self, params, copy=True):
        """mcp_map_bundle_select: (SelectResult, mkfs, points, meas)."""
        res = SelectResult()
        _chk(self._L.mcp_map_bundle_select(self._h, ctypes.addressof(params), ctypes.addressof(res)), "map_bundle_select")
        return (res,) + self.views(copy)

    def select(self, mode=BUNDLE_RECENT, newest=-1, params=None, **kw):
        """BundleAdjustRecent / BundleAdjustAll over the graph in one call: (SelectResult, synth.Problem or None when status != 0).  The Problem
        holds base_* (base_fixed = fixed in the bundle), pt_*, ms_* and .window = dict(mkf=slots, adjust=..., points=rows, store=store indices);
        Problem.populate(bundle) replays it.  kw: select_params' fields."""
        params = select_params(mode, newest, **kw) if params is None else params
        res, mkfs, points, meas = self.select_raw(params)
        if res.status != 0:
            return res, None
        return res, selection_problem(mkfs, points, meas, self.base_from_world, self.cam_from_base, self.cams)


class MeasParcel:
    """A measurement parcel of one MapPointTable (which must outlive it): the measurements of a track call, a ReFind or the caller, kept in
    device memory with the keys their rows held when the parcel was filled, until MapGraph.commit_parcel appends them to a store."""

    def __init__(self, table):
        self._L = lib()
        self.table = table
        self._h = self._L.mcp_meas_parcel_create(table._h)
        if not self._h:
            raise RuntimeError("mcp_meas_parcel_create failed: " + _cb.last_error())
        table._open_graphs = getattr(table, "_open_graphs", 0) + 1     # as a graph: the table's handle is destroyed after the last parcel's

    def close(self):
        if getattr(self, "_h", None):
            self._L.mcp_meas_parcel_destroy(self._h)
            self._h = None
            self.table._open_graphs -= 1
            if self.table._open_graphs == 0 and getattr(self.table, "_close_pending", False):
                self.table.close()

    def __del__(self):
        self.close()

    @classmethod
    def from_track(cls, table):
        """A new parcel filled from the last track call with bookkeeping on `table`."""
        p = cls(table)
        p.fill_from_track()
        return p

    @classmethod
    def from_refind(cls, table):
        """A new parcel filled from the FOUND pairs of the last refind on `table`."""
        p = cls(table)
        p.fill_from_refind()
        return p

    @classmethod
    def from_host(cls, table, lane, row, uv, level):
        p = cls(table)
        p.fill_from_host(lane, row, uv, level)
        return p

    def fill_from_track(self):
        return _chk(self._L.mcp_meas_parcel_from_track(self._h), "meas_parcel_from_track")

    def fill_from_refind(self):
        return _chk(self._L.mcp_meas_parcel_from_refind(self._h), "meas_parcel_from_refind")

    def fill_from_host(self, lane, row, uv, level):
        ln = _i32(lane)
        n = len(ln)
        r, u, lv = _i32(row, (n,)), _f64(uv).reshape(n, 2), _i32(level, (n,))
        return _chk(self._L.mcp_meas_parcel_from_host(self._h, n, ln.ctypes.data, r.ctypes.data, u.ctypes.data, lv.ctypes.data), "meas_parcel_from_host")

    def __len__(self):
        return _chk(self._L.mcp_meas_parcel_size(self._h), "meas_parcel_size")

    def entries(self):
        """The entries read back (PARCEL_ENTRY_DTYPE); waits for the table's stream."""
        n = len(self)
        out = np.zeros(max(n, 1), dtype=PARCEL_ENTRY_DTYPE)
        _chk(self._L.mcp_meas_parcel_get(self._h, n, out.ctypes.data), "meas_parcel_get")
        return out[:n]
