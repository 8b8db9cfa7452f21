"""The seeded maps of the measurement-parcel tests (tests/test_parcel_cpu.py, tests/test_parcel_gpu.py): for every parcel size at a seam of the
256-entry workgroups and their 64-lane wavefronts, three cases with 1-8 lanes.

A case is a dict:
  n_rows_fill / n_rows     the table's rows when the parcel is filled / when it is committed (the last N_DROPPED rows are dropped in between:
                           entries on them are stale as "past the table's rows")
  keys_fill / keys_now     the key column then and now (about one row in ten was recycled for another point in between)
  n_point_rows, pt_flags, src_mkf, src_cam
                           the graph columns now: the first n_point_rows rows (the rows after them were never written: bad); about one row in
                           ten went bad, one in twenty is fixed and has no source
  bad_late                 the rows of pt_flags that went bad only after the fill (what the GPU test uploads in between)
  P, ncam, lane_mkf, lane_cam, cross_camera, source
                           the graph's present slots 0..P-1, its rig size, and the commit's arguments; lanes name distinct (slot, camera) pairs,
                           slot P-1 is left to the entries the store holds before the commit (`pre`: rows 0..4, camera 0)
  entries                  PARCEL_ENTRY_DTYPE, distinct (lane, row), key = keys_fill[row]
Every size from 63 up has, over its three cases, every verdict at least once (all_cases() checks it with the numpy restatement)."""
import numpy as np

from mcptam_amd import map_graph as mg

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 513, 1031)
N_DROPPED = 5
N_PRE = 5
P, NCAM = 6, 4


def make_case(n, lanes, cross_camera, withhold, seed):
    rng = np.random.default_rng(seed)
    n_rows_fill = max(40, -(-n // lanes) + 23)
    n_rows = n_rows_fill - N_DROPPED
    keys_fill = (np.arange(n_rows_fill, dtype=np.int32) * 3 + 7)
    recycled = rng.random(n_rows_fill) < 0.1
    keys_now = np.where(recycled, keys_fill + 100000, keys_fill).astype(np.int32)[:n_rows]
    n_point_rows = n_rows - 7
    fixed = rng.random(n_point_rows) < 0.05
    bad_early, bad_late = rng.random(n_point_rows) < 0.05, rng.random(n_point_rows) < 0.06
    pt_flags = (np.where(fixed, mg.GP_FIXED, 0) | np.where(bad_early | bad_late, mg.GP_BAD, 0)).astype(np.int32)
    src_mkf = np.where(fixed, -1, rng.integers(0, P, n_point_rows)).astype(np.int32)
    src_cam = np.where(fixed, 0, rng.integers(0, NCAM, n_point_rows)).astype(np.int32)
    pairs = rng.permutation((P - 1) * NCAM)[:lanes]
    lane_mkf, lane_cam = (pairs // NCAM).astype(np.int32), (pairs % NCAM).astype(np.int32)
    if withhold:
        lane_mkf[rng.integers(0, lanes)] = -1
    pick = rng.permutation(lanes * n_rows_fill)[:n]            # distinct (lane, row), in no particular order
    lane, row = (pick % lanes).astype(np.int32), (pick // lanes).astype(np.int32)
    uv = rng.normal(0.0, 300.0, (n, 2))
    if n >= 3:
        uv[0], uv[1], uv[2] = (0.0, -0.0), (1e-310, -1e-310), (639.999999999, 479.5)
    e = mg.parcel_entries(lane, row, uv, rng.integers(0, 4, n), keys_fill[row] if n else None)
    return dict(name="n%d-l%d-x%d-s%d" % (n, lanes, cross_camera, seed), n=n, n_rows_fill=n_rows_fill, n_rows=n_rows, keys_fill=keys_fill, keys_now=keys_now,
                n_point_rows=n_point_rows, pt_flags=pt_flags, src_mkf=src_mkf, src_cam=src_cam, bad_late=np.flatnonzero(bad_late & ~bad_early).astype(np.int32),
                P=P, ncam=NCAM, lane_mkf=lane_mkf, lane_cam=lane_cam, cross_camera=cross_camera, source=mg.SRC_TRACKER if seed % 2 else mg.SRC_REFIND, entries=e)


def ref(c, first=0):
    """parcel_commit_ref of a case."""
    return mg.parcel_commit_ref(c["entries"], c["keys_now"], c["pt_flags"], c["src_mkf"], c["src_cam"], c["lane_mkf"], c["lane_cam"], c["cross_camera"], c["source"], first)


def host(c, first=0):
    """parcel_commit_host of a case."""
    return mg.parcel_commit_host(c["entries"], c["keys_now"], c["pt_flags"], c["src_mkf"], c["src_cam"], c["lane_mkf"], c["lane_cam"], c["cross_camera"], c["source"], first)


def all_cases():
    out = []
    for i, n in enumerate(SIZES):
        trio = [make_case(n, 1, 1, False, 1000 + n), make_case(n, 2 + (i * 5) % 7, 0, True, 2000 + n), make_case(n, 8, i % 2, i % 3 == 0, 3000 + n)]
        if n >= 63:
            seen = np.zeros(5, dtype=np.int64)
            for c in trio:
                seen += np.bincount(ref(c)[0], minlength=5)
            assert (seen > 0).all(), (n, seen.tolist())
        out += trio
    return out


def same_commit(a, b):
    """Two (verdicts, result, appended, lane_appended) tuples, exactly: the records byte for byte."""
    assert np.array_equal(a[0], b[0])
    assert a[1] == b[1], (a[1], b[1])
    assert a[2].dtype == b[2].dtype == mg.STORE_ENTRY_DTYPE and a[2].tobytes() == b[2].tobytes()
    assert np.array_equal(a[3], b[3])
