"""ctypes binding of MapMakerServerBase::ReFind_Common over the resident map-point table (include/mcp_img.h: mcp_map_refind), and the
pure-numpy derivation of its verdicts and measurements from the records of mcp_patch_sequences(MCP_PF_REFIND) -- what the map maker's
ReFindBatch does with them (src/MapMakerServerBase.cc:941-1001)."""
import ctypes

import numpy as np

from . import chain_bundle as _cb
from .keyframe import PF_STATE_DTYPE, _chk, _pose12

REFIND_SYMBOLS = ["mcp_map_refind", "mcp_map_refind_view"]
FOUND, OUTSIDE, TEMPLATE_BAD, NOT_FOUND, NO_SOURCE = 1, 2, 3, 4, 5
VERDICT_NAMES = {FOUND: "FOUND", OUTSIDE: "OUTSIDE", TEMPLATE_BAD: "TEMPLATE_BAD", NOT_FOUND: "NOT_FOUND", NO_SOURCE: "NO_SOURCE"}


class RefindTarget(ctypes.Structure):
    _fields_ = [("kf", ctypes.c_void_p), ("cam", ctypes.c_void_p), ("cam_from_world", ctypes.c_double * 12)]


class RefindMeas(ctypes.Structure):
    _fields_ = [("pair", ctypes.c_int), ("row", ctypes.c_int), ("target", ctypes.c_int), ("level", ctypes.c_int), ("subpix", ctypes.c_int),
                ("score", ctypes.c_int), ("root_pos", ctypes.c_double * 2)]


class RefindResult(ctypes.Structure):
    _fields_ = [("counts", ctypes.c_int * 6), ("n_meas", ctypes.c_int)]


REFIND_MEAS_DTYPE = np.dtype([("pair", "i4"), ("row", "i4"), ("target", "i4"), ("level", "i4"), ("subpix", "i4"), ("score", "i4"),
                              ("root_pos", "f8", 2)], align=True)
assert REFIND_MEAS_DTYPE.itemsize == ctypes.sizeof(RefindMeas)


def refind_verdicts(td_out, pairs=None):
    """Verdict and measurement per record of mcp_patch_sequences(MCP_PF_REFIND) (TD_OUT_DTYPE), as ReFind_Common decides them: not in the
    image -> OUTSIDE, TemplateBad -> TEMPLATE_BAD, FindPatchCoarse failed -> NOT_FOUND, else FOUND with (nLevel, bSubPix, nBestSSD,
    v2RootPos) = (search_level, did_subpix, score, found_pos).  pairs: (n, 2) (row, target) of the records, or None (row = target = -1).
    Returns (verdicts uint8 (n,), REFIND_MEAS_DTYPE array of the FOUND records in ascending order)."""
    n = len(td_out)
    v = np.full(n, FOUND, dtype=np.uint8)
    v[td_out["found"] == 0] = NOT_FOUND
    v[td_out["template_bad"] != 0] = TEMPLATE_BAD
    v[td_out["in_image"] == 0] = OUTSIDE
    idx = np.nonzero(v == FOUND)[0]
    m = np.zeros(len(idx), dtype=REFIND_MEAS_DTYPE)
    m["pair"] = idx
    if pairs is None:
        m["row"] = -1
        m["target"] = -1
    else:
        pairs = np.asarray(pairs, dtype=np.int32).reshape(n, 2)
        m["row"] = pairs[idx, 0]
        m["target"] = pairs[idx, 1]
    m["level"] = td_out["search_level"][idx]
    m["subpix"] = td_out["did_subpix"][idx]
    m["score"] = td_out["score"][idx]
    m["root_pos"] = td_out["found_pos"][idx]
    return v, m


def verdict_counts(verdicts):
    """counts[v] for v = 0..5, as mcp_refind_result::counts."""
    return np.bincount(np.asarray(verdicts, dtype=np.int64), minlength=6)[:6]


def _bind(L):
    if getattr(L, "_refind_bound", False):
        return L
    vp, ip = ctypes.c_void_p, ctypes.c_int
    L.mcp_map_refind.argtypes = [vp, ip, vp, ip, vp, ip, vp, vp, ip, vp, vp]
    L.mcp_map_refind_view.restype = vp
    L.mcp_map_refind_view.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L._refind_bound = True
    return L


def marshal_targets(targets):
    """targets: list of (KeyFrame, TaylorCamera, (R, t) = CamFromWorld).  Returns (keep-alive, mcp_refind_target array)."""
    cams = [t[1].to_struct() for t in targets]
    tab = (RefindTarget * max(len(targets), 1))()
    for i, (kf, _cam, cfw) in enumerate(targets):
        tab[i].kf = kf._h
        tab[i].cam = ctypes.addressof(cams[i])
        p = _pose12(*cfw)
        for k in range(12):
            tab[i].cam_from_world[k] = p[k]
    return cams, tab


def refind(table, targets, pairs, per_row_finders=False, finder=None, view=False, cap_meas=None):
    """mcp_map_refind on a MapPointTable.  targets: list of (KeyFrame, TaylorCamera, CamFromWorld (R, t)) or the pair marshal_targets
    returned; pairs: (n, 2) int array of (row, target index), processed as given.  finder: a PF_STATE_DTYPE array of one element -- the
    map maker's static finder, updated in place -- or None (a fresh one).  view=True: the measurements are a view of the library's pinned
    block, valid until the next call on this table.  Returns (verdicts uint8 (n,), REFIND_MEAS_DTYPE measurements, counts (6,), finder)."""
    L = _bind(table._L)
    keep, tab = targets if isinstance(targets, tuple) else marshal_targets(targets)
    n_targets = len(keep)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n = len(pairs)
    cap = n if cap_meas is None else int(cap_meas)
    verdict = np.zeros(max(n, 1), dtype=np.uint8)
    meas = None if view else np.zeros(max(cap, 1), dtype=REFIND_MEAS_DTYPE)
    res = RefindResult()
    if finder is not None:
        assert finder.dtype == PF_STATE_DTYPE and finder.shape == (1,) and finder.flags.c_contiguous
    rc = L.mcp_map_refind(table._h, n_targets, ctypes.cast(tab, ctypes.c_void_p), n, pairs.ctypes.data, int(bool(per_row_finders)),
                          None if finder is None else finder.ctypes.data, verdict.ctypes.data, cap, None if view else meas.ctypes.data, ctypes.byref(res))
    table.refind_counts = np.array(res.counts[:], dtype=np.int64)
    _chk(rc, "map_refind")
    if view:
        cnt = ctypes.c_int(0)
        ptr = L.mcp_map_refind_view(table._h, ctypes.byref(cnt))
        if cnt.value != res.n_meas:
            raise RuntimeError("mcp_map_refind_view: " + _cb.last_error())
        meas = np.frombuffer((ctypes.c_char * (cnt.value * REFIND_MEAS_DTYPE.itemsize)).from_address(ptr), dtype=REFIND_MEAS_DTYPE) \
            if cnt.value else np.zeros(0, dtype=REFIND_MEAS_DTYPE)
    else:
        meas = meas[:res.n_meas]
    return verdict[:n], meas, table.refind_counts, finder
