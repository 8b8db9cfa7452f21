// map_graph_parcel.h -- measurement parcels (include/mcp_img.h mcp_meas_parcel_*): the tracker's and ReFind's measurements taken from the pinned
// blocks their kernels wrote into device memory of the parcel, and committed to the map graph's store when the map maker gets to the MKF
// (Tracker::RecordMeasurements, src/Tracker.cc:1237-1274; MapMaker::AddMultiKeyFrameFromTopOfQueue, src/MapMaker.cc:389-423), gfx950.
//
// The conventions are map_graph_kernels.h's: every count is an integer and every atomic adds or maximises an integer (LDS or global); the
// compaction ranks by index (per-workgroup counts, then mg_rank's ballot scatter), so the store does not depend on the order workgroups are
// dispatched in; no workgroup waits for another; 256-thread workgroups.  The verdict and the store record are host / device bodies that
// mcp_parcel_commit_host (map_graph_parcel_host.cpp) walks under the host compiler: integer comparisons and copies, so the bytes are the same.
// This header compiles with a plain C++ compiler; the kernels appear under hipcc, unless MGP_HOST_ONLY is defined.
//
// A fill is one launch on the table's stream (k_mgp_from_track / k_mgp_from_refind read the pinned list a kernel on that stream wrote;
// k_mgp_keys completes entries copied up from the host): an entry takes its row's key as it stands then, and the largest lane goes to a
// word of the parcel.  A commit is two launches:
//   k_mgp_judge    one thread per entry: the verdict byte, the five counters and the per-lane counts (one integer atomic per wavefront and
//                  counter, one per appended entry and lane), the appended count of the workgroup
//   k_mgp_append   one thread per entry: an appended entry's rank (mg_rank) and its record into the store
// The boundary is the grid-wide one: every workgroup's count must be known before an entry is ranked.  A device fill whose largest lane is not
// below n_lanes makes both launches return at once (the test is uniform over the grid); the host reads the flag with the result.
#pragma once
#include <cstdint>
#include <cstddef>
#include "../../include/mcp_img.h"

#if defined(__HIPCC__) && !defined(MGP_HOST_ONLY)
#define MGP_HD __host__ __device__
#else
#define MGP_HD
#endif

namespace mcp {

// the map as a commit reads it: the key column and the graph's point columns, as plain arrays (stride 1) or as the device's records
// (TmSrc: 6 ints, key first; MgPoint: src_mkf, src_cam, flags, pad).  Rows from n_prows on have no graph column yet: they read as bad.
struct MgpMap {
  int n_rows, n_prows;
  const int* key; int key_stride;
  const int* src_mkf; const int* src_cam; const int* pflags; int pt_stride;
};

// the verdict of one entry, the rules in the order of include/mcp_img.h; each rule reads only what it needs (a stale row's new point is not
// looked at beyond its key).  A lane outside the tables (refused by the callers) reads as withheld.
MGP_HD inline int mgp_verdict(const mcp_parcel_entry& e, int n_lanes, const int* lane_mkf, const int* lane_cam, const MgpMap& M, int cross_camera) {
  if (e.lane < 0 || e.lane >= n_lanes || lane_mkf[e.lane] < 0) return MCP_PARCEL_SKIPPED;
  if (e.row < 0 || e.row >= M.n_rows || M.key[(size_t)e.row*M.key_stride] != e.key) return MCP_PARCEL_STALE;
  if (e.row >= M.n_prows || (M.pflags[(size_t)e.row*M.pt_stride] & MCP_GP_BAD)) return MCP_PARCEL_BAD;
  if (!cross_camera && (M.src_mkf[(size_t)e.row*M.pt_stride] < 0 || M.src_cam[(size_t)e.row*M.pt_stride] != lane_cam[e.lane])) return MCP_PARCEL_CROSS;
  return MCP_PARCEL_APPENDED;
}
// the store entry of an appended one: mcp_map_graph_add_meas's record, field by field
MGP_HD inline void mgp_record(const mcp_parcel_entry& e, int mkf, int cam, int source, mcp_store_entry& o) {
  o.uv[0] = e.uv[0]; o.uv[1] = e.uv[1]; o.mkf = mkf; o.cam = cam; o.row = e.row; o.level = e.level; o.source = source; o.alive = 1;
}
// a row's key for a parcel entry (0 for a row outside the table: the commit calls such an entry stale before it compares keys)
MGP_HD inline int mgp_key_of(int row, int n_rows, const int* key, int key_stride) { return (row >= 0 && row < n_rows) ? key[(size_t)row*key_stride] : 0; }

// what a commit's launches leave for the host (the graph's device block, copied out with the per-lane counts behind it)
struct MgpCtl { int counts[5]; int refused, max_lane, pad_; };

#if defined(__HIPCC__) && !defined(MGP_HOST_ONLY)
constexpr int MGP_BLOCK = MG_BLOCK;
static_assert(sizeof(mcp_store_entry) == sizeof(MgMeas) && offsetof(mcp_store_entry, mkf) == offsetof(MgMeas, mkf) && offsetof(mcp_store_entry, row) == offsetof(MgMeas, row) &&
              offsetof(mcp_store_entry, source) == offsetof(MgMeas, source) && offsetof(mcp_store_entry, alive) == offsetof(MgMeas, alive), "mcp_store_entry is the store's record");
static_assert(sizeof(mcp_parcel_entry) == 32 && sizeof(TmSrc) == 6*sizeof(int) && offsetof(TmSrc, key) == 0 && sizeof(MgPoint) == 4*sizeof(int) &&
              offsetof(MgPoint, src_cam) == 4 && offsetof(MgPoint, flags) == 8, "the strides MgpMap walks the device's records with");

// the largest lane of a fill: the workgroup's maximum in LDS, then one global atomicMax per workgroup that has an entry
__device__ __forceinline__ void mgp_max_lane(bool has, int lane_of, int* __restrict__ max_lane /* the parcel's, -1 before the fill */) {
  __shared__ int wg_max;
  if (threadIdx.x == 0) wg_max = -1;
  __syncthreads();
  if (has) atomicMax(&wg_max, lane_of);
  __syncthreads();
  if (threadIdx.x == 0 && wg_max >= 0) atomicMax(max_lane, wg_max);
}

struct MgpFirst { int v[MCP_MAX_FRAME_CAMS + 1]; };      // where each camera's measurements start in the pinned list

// entry i of the parcel from measurement i of the last track call: lane = the camera whose range holds i
__global__ void __launch_bounds__(MGP_BLOCK)
k_mgp_from_track(const mcp_track_meas* __restrict__ meas /* pinned */, int n, int ncam, MgpFirst first, const TmSrc* __restrict__ src, int n_rows,
                 mcp_parcel_entry* __restrict__ out, int* __restrict__ max_lane) {
  const int i = blockIdx.x*MGP_BLOCK + threadIdx.x;
  int lane = 0;
  if (i < n) {
    while (lane + 1 < ncam && i >= first.v[lane + 1]) ++lane;
    const mcp_track_meas M = meas[i];
    mcp_parcel_entry E;
    E.uv[0] = M.found_pos[0]; E.uv[1] = M.found_pos[1]; E.lane = lane; E.row = M.row; E.level = M.level;
    E.key = mgp_key_of(M.row, n_rows, reinterpret_cast<const int*>(src), 6);
    out[i] = E;
  }
  mgp_max_lane(i < n, lane, max_lane);
}

// entry i from FOUND pair i of the last mcp_map_refind: lane = the pair's target
__global__ void __launch_bounds__(MGP_BLOCK)
k_mgp_from_refind(const mcp_refind_meas* __restrict__ meas /* pinned */, int n, const TmSrc* __restrict__ src, int n_rows, mcp_parcel_entry* __restrict__ out,
                  int* __restrict__ max_lane) {
  const int i = blockIdx.x*MGP_BLOCK + threadIdx.x;
  int lane = 0;
  if (i < n) {
    const mcp_refind_meas M = meas[i];
    lane = M.target;
    mcp_parcel_entry E;
    E.uv[0] = M.root_pos[0]; E.uv[1] = M.root_pos[1]; E.lane = lane; E.row = M.row; E.level = M.level;
    E.key = mgp_key_of(M.row, n_rows, reinterpret_cast<const int*>(src), 6);
    out[i] = E;
  }
  mgp_max_lane(i < n, lane, max_lane);
}

// the keys of entries that came up from the host (their rows were checked there)
__global__ void __launch_bounds__(MGP_BLOCK)
k_mgp_keys(mcp_parcel_entry* __restrict__ ent, int n, const TmSrc* __restrict__ src, int n_rows) {
  const int i = blockIdx.x*MGP_BLOCK + threadIdx.x;
  if (i < n) ent[i].key = mgp_key_of(ent[i].row, n_rows, reinterpret_cast<const int*>(src), 6);
}

struct MgpCommit { int n, n_lanes, cross_camera, source, first; long long cap; };      // cap: the store's room in entries

__global__ void __launch_bounds__(MGP_BLOCK)
k_mgp_judge(MgpCommit Q, const mcp_parcel_entry* __restrict__ ent, const int* __restrict__ lane_mkf, const int* __restrict__ lane_cam, const TmSrc* __restrict__ src, int n_rows,
            const MgPoint* __restrict__ pts, int n_prows, const int* __restrict__ max_lane, uint8_t* __restrict__ verdict, int* __restrict__ blk_cnt,
            MgpCtl* __restrict__ ctl /* zeroed */, int* __restrict__ lane_appended /* zeroed */) {
  __shared__ int cnt[5];
  const int top = *max_lane;
  if (blockIdx.x == 0 && threadIdx.x == 0) { ctl->max_lane = top; if (top >= Q.n_lanes) ctl->refused = 1; }
  if (top >= Q.n_lanes) return;                        // (uniform over the grid: a device fill with a lane the tables do not have)
  const int i = blockIdx.x*MGP_BLOCK + threadIdx.x;
  if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
  __syncthreads();
  int v = -1;
  if (i < Q.n) {
    const mcp_parcel_entry E = ent[i];
    const int* p = reinterpret_cast<const int*>(pts);
    const MgpMap M{n_rows, n_prows, reinterpret_cast<const int*>(src), 6, p, p + 1, p + 2, 4};
    v = mgp_verdict(E, Q.n_lanes, lane_mkf, lane_cam, M, Q.cross_camera);
    verdict[i] = (uint8_t)v;
    if (v == MCP_PARCEL_APPENDED) atomicAdd(&lane_appended[E.lane], 1);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned long long m = __ballot(v == k);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[k], __popcll(m));
  }
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt[MCP_PARCEL_APPENDED];
  if (threadIdx.x < 5 && cnt[threadIdx.x]) atomicAdd(&ctl->counts[threadIdx.x], cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(MGP_BLOCK)
k_mgp_append(MgpCommit Q, const mcp_parcel_entry* __restrict__ ent, const int* __restrict__ lane_mkf, const int* __restrict__ lane_cam, const uint8_t* __restrict__ verdict,
             const int* __restrict__ blk_cnt, int nblk, const int* __restrict__ max_lane, mcp_store_entry* __restrict__ store) {
  if (*max_lane >= Q.n_lanes) return;                  // (uniform over the grid)
  const int i = blockIdx.x*MGP_BLOCK + threadIdx.x;
  const bool keep = i < Q.n && verdict[i] == MCP_PARCEL_APPENDED;
  const int at = mg_rank(keep, blk_cnt, nblk, blockIdx.x, nullptr);
  if (!keep || at < 0 || at >= Q.n || (long long)Q.first + at >= Q.cap) return;      // (at < the appended count <= n; the store was grown to first + n)
  const mcp_parcel_entry E = ent[i];
  mcp_store_entry O;
  mgp_record(E, lane_mkf[E.lane], lane_cam[E.lane], Q.source, O);
  store[(size_t)Q.first + at] = O;
}
#endif  // __HIPCC__

// ---- the host's statement of a commit -------------------------------------------------------------------------------------------------------
struct MgpHostIn {
  int n; const mcp_parcel_entry* ent; MgpMap map; int n_lanes; const int* lane_mkf; const int* lane_cam; int cross_camera, source;
};
// verdict: NULL or n bytes; appended: NULL or n records; counts: 5; lane_appended: NULL or n_lanes (zeroed here).  Returns the appended count.
inline int mgp_host_commit(const MgpHostIn& I, uint8_t* verdict, mcp_store_entry* appended, int* counts, int* lane_appended) {
  for (int k = 0; k < 5; ++k) counts[k] = 0;
  for (int l = 0; lane_appended && l < I.n_lanes; ++l) lane_appended[l] = 0;
  int at = 0;
  for (int i = 0; i < I.n; ++i) {
    const mcp_parcel_entry& E = I.ent[i];
    const int v = mgp_verdict(E, I.n_lanes, I.lane_mkf, I.lane_cam, I.map, I.cross_camera);
    ++counts[v];
    if (verdict) verdict[i] = (uint8_t)v;
    if (v != MCP_PARCEL_APPENDED) continue;
    if (appended) mgp_record(E, I.lane_mkf[E.lane], I.lane_cam[E.lane], I.source, appended[at]);
    if (lane_appended) ++lane_appended[E.lane];
    ++at;
  }
  return at;
}

}  // namespace mcp
