// stereo_append.h -- what mcp_stereo_map_points (include/mcp_img.h) adds around the kernels of stereo_kernels.h: the source keyframe's busy
// positions gathered from the map graph's store, and the created points appended to the table's columns, the graph's point columns and the
// store (src/MapMakerServerBase.cc:855-914: the new MapPoint and its two AddMeasurement calls), gfx950.
//
// The conventions are map_graph_kernels.h's: every count is an integer; the gather ranks by index (per-workgroup counts, then mg_rank's ballot
// scatter), so the busy list is in store order whatever order the workgroups are dispatched in; no workgroup waits for another; 256-thread
// workgroups.  What one point becomes -- its row's column values, its graph column, its two store entries -- and which store entries are busy
// positions are host / device bodies that mcp_stereo_append_host / mcp_stereo_busy_host (stereo_append_host.cpp) walk under the host compiler:
// copies, integer comparisons and four exact operations on doubles (sa_center), so the bytes are the same.  This header compiles with a plain
// C++ compiler; the kernels appear under hipcc, unless SA_HOST_ONLY is defined.
//
// With busy_from_store the call enqueues, in front of the walk:
//   k_sa_busy_mark     one thread per store entry: the workgroup's count of live entries of (src_mkf, src_cam)
//   k_sa_busy_gather   one thread per store entry: a matching entry's rank (mg_rank) and its {uv, level} into the busy list; the length
//   k_sa_thin_busy     one thread per candidate: k_stereo_thin_meas's loop with the list's length read from device memory (the host never
//                      learns it before the call's one wait, so it cannot be a launch argument)
// and behind the last k_stereo_commit, in both modes:
//   k_sa_append        one thread per created point: the record is read once from the pinned block k_stereo_commit compacted it into
// The boundaries are the grid-wide ones: every workgroup's count before an entry is ranked, the whole list before a candidate is thinned, the
// last target's count before a point is appended.
#pragma once
#include <cstdint>
#include <cstddef>
#include "../../include/mcp_img.h"

#if defined(__HIPCC__) && !defined(SA_HOST_ONLY)
#define SA_HD __host__ __device__
#else
#define SA_HD
#endif

namespace mcp {

// ---- the busy filter: ThinCandidates' measurement list of the keyframe (src_mkf, src_cam) as the store holds it ---------------------------
SA_HD inline bool sa_busy_match(const mcp_store_entry& E, int src_mkf, int src_cam) { return E.alive && E.mkf == src_mkf && E.cam == src_cam; }
// (every level is kept: the level filter is the thinning's)
SA_HD inline void sa_busy_record(const mcp_store_entry& E, mcp_stereo_meas& o) { o.root_pos[0] = E.uv[0]; o.root_pos[1] = E.uv[1]; o.level = E.level; o.pad_ = 0; }

// ---- one created point ---------------------------------------------------------------------------------------------------------------------
// the candidate's level position back from LevelZeroPos, root = (c + 0.5)*2^level - 0.5: adding 0.5, dividing by a power of two and subtracting
// 0.5 are exact for every position an image can have, so this is the integer the walk started from
SA_HD inline int sa_center(double root, int level) { return (int)((root + 0.5)/(double)(1 << level) - 0.5); }

// what the row of a created point holds afterwards (the table's columns, then the graph's) ...
struct SaRow {
  double world_pos[3], pixel_right_w[3], pixel_down_w[3]; int usable;      // mcp_map_points_update; usable 0: mbOptimized is false until an adjustment
  int inlier, outlier;                                                     // the MapPoint constructor's (1, 0)
  double rays[9];                                                          // mcp_map_points_update_rays: center, one right, one down
  int level, cx, cy, fixed;                                                // mcp_map_points_update_source (the key and the keyframe's slot are the caller's)
  int gp_src_mkf, gp_src_cam, gp_flags, gp_pending;                        // mcp_map_graph_update_points
};
// ... and its two store entries, in the order of the reference's AddMeasurement calls (:901-902): the source's SRC_ROOT, the target's SRC_EPIPOLAR
SA_HD inline void sa_point(const mcp_stereo_point& P, int row, int level, int src_mkf, int src_cam, int target_mkf, int target_cam, SaRow& R,
                           mcp_store_entry& root, mcp_store_entry& epi) {
  for (int a = 0; a < 3; ++a) {
    R.world_pos[a] = P.world_pos[a]; R.pixel_right_w[a] = P.pixel_right_w[a]; R.pixel_down_w[a] = P.pixel_down_w[a];
    R.rays[a] = P.center_nc[a]; R.rays[3 + a] = P.one_right_nc[a]; R.rays[6 + a] = P.one_down_nc[a];
  }
  R.usable = 0; R.inlier = 1; R.outlier = 0;
  R.level = level; R.cx = sa_center(P.root_pos[0], level); R.cy = sa_center(P.root_pos[1], level); R.fixed = 0;
  R.gp_src_mkf = src_mkf; R.gp_src_cam = src_cam; R.gp_flags = 0; R.gp_pending = 0;
  root.uv[0] = P.root_pos[0]; root.uv[1] = P.root_pos[1]; root.mkf = src_mkf; root.cam = src_cam; root.row = row; root.level = level;
  root.source = MCP_SRC_ROOT; root.alive = 1;
  epi.uv[0] = P.target_pos[0]; epi.uv[1] = P.target_pos[1]; epi.mkf = target_mkf; epi.cam = target_cam; epi.row = row; epi.level = level;
  epi.source = MCP_SRC_EPIPOLAR; epi.alive = 1;
}

#if defined(__HIPCC__) && !defined(SA_HOST_ONLY)
constexpr int SA_BLOCK = MG_BLOCK;
static_assert(sizeof(mcp_store_entry) == sizeof(MgMeas) && offsetof(mcp_store_entry, cam) == offsetof(MgMeas, cam) && offsetof(mcp_store_entry, level) == offsetof(MgMeas, level) &&
              offsetof(mcp_store_entry, alive) == offsetof(MgMeas, alive), "mcp_store_entry is the store's record");
static_assert(sizeof(mcp_stereo_meas) == 24, "the busy list's record, no padding left unwritten");

__global__ void __launch_bounds__(SA_BLOCK)
k_sa_busy_mark(const mcp_store_entry* __restrict__ store, int n, int src_mkf, int src_cam, int* __restrict__ blk_cnt) {
  __shared__ int cnt;
  const int i = blockIdx.x*SA_BLOCK + threadIdx.x;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const unsigned long long m = __ballot(i < n && sa_busy_match(store[i], src_mkf, src_cam));
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt, __popcll(m));
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt;
}
// n == 0 runs one workgroup that only writes the length (0)
__global__ void __launch_bounds__(SA_BLOCK)
k_sa_busy_gather(const mcp_store_entry* __restrict__ store, int n, int nblk, const int* __restrict__ blk_cnt, int src_mkf, int src_cam, mcp_stereo_meas* __restrict__ out,
                 int cap, int* __restrict__ n_busy) {
  const int i = blockIdx.x*SA_BLOCK + threadIdx.x;
  const bool keep = i < n && sa_busy_match(store[i], src_mkf, src_cam);
  int total = 0;
  const int at = mg_rank(keep, blk_cnt, nblk, blockIdx.x, &total);
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_busy = total;
  if (!keep || at < 0 || at >= cap) return;            // (at < the matching count <= n <= cap)
  mcp_stereo_meas M;
  sa_busy_record(store[i], M);
  out[at] = M;
}
// k_stereo_thin_meas with n_meas where k_sa_busy_gather left it
__global__ void __launch_bounds__(256)
k_sa_thin_busy(int n_cand, const mcp_int2* __restrict__ cand, const int* __restrict__ n_busy, int cap, const mcp_stereo_meas* __restrict__ meas, int level,
               uint8_t* __restrict__ alive) {
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= n_cand) return;
  const int n_meas = min(*n_busy, cap);
  const double sc = (double)(1 << level);
  bool good = true;
  for (int m = 0; m < n_meas && good; ++m) {
    const mcp_stereo_meas M = meas[m];
    if (!(M.level == level || M.level == level + 1)) continue;
    if (stereo_busy(ir_round(M.root_pos[0]/sc), ir_round(M.root_pos[1]/sc), cand[i].x, cand[i].y)) good = false;
  }
  alive[i] = good ? 1 : 0;
}

// one created point's row into the table's columns and the graph's: what k_sa_append and k_ml_create (map_life.h) both leave in a row
__device__ __forceinline__ void sa_write_row(const SaRow& R, int row, int key, int slot1, int ncam_states, PvsPoint* __restrict__ pts, TmSrc* __restrict__ src, TmStates states,
                                             int* __restrict__ cnt, double* __restrict__ rays, MgPoint* __restrict__ gp) {
  PvsPoint O;
  for (int a = 0; a < 3; ++a) { O.world_pos[a] = R.world_pos[a]; O.pixel_right_w[a] = R.pixel_right_w[a]; O.pixel_down_w[a] = R.pixel_down_w[a]; }
  O.usable = R.usable; O.pad_ = 0;
  pts[row] = O;
  cnt[2*(size_t)row] = R.inlier; cnt[2*(size_t)row + 1] = R.outlier;
#pragma unroll
  for (int a = 0; a < 9; ++a) rays[9*(size_t)row + a] = R.rays[a];
  // the source, as k_tm_source_scatter writes it: a row whose key changes forgets what its finders saw
  if (src[row].key != key)
    for (int c = 0; c < ncam_states; ++c) {
      unsigned long long* s = reinterpret_cast<unsigned long long*>(states.s[c] + row);
      for (int q = 0; q < (int)(sizeof(mcp_pf_state)/8); ++q) s[q] = 0ull;
    }
  TmSrc S; S.key = key; S.slot1 = slot1; S.level = R.level; S.cx = R.cx; S.cy = R.cy; S.fixed = R.fixed;
  src[row] = S;
  MgPoint G; G.src_mkf = R.gp_src_mkf; G.src_cam = R.gp_src_cam; G.flags = R.gp_flags; G.pending = R.gp_pending;
  gp[row] = G;
}

// where an append writes, and how far it may: the blocks were grown on the host to cover every row handed in and 2*n_rows store entries
struct SaAppend {
  int n_targets, n_rows, level, src_mkf, src_cam, slot1, first_store, table_rows, graph_rows, ncam_states;
  long long store_cap;
};
__global__ void __launch_bounds__(SA_BLOCK)
k_sa_append(SaAppend Q, const int* __restrict__ counts /* k_stereo_commit's: counts[n_targets] = made */, const mcp_stereo_point* __restrict__ recs /* pinned */,
            const int* __restrict__ rows, const int* __restrict__ keys, const int* __restrict__ target_mkf, const int* __restrict__ target_cam,
            PvsPoint* __restrict__ pts, TmSrc* __restrict__ src, TmStates states, int* __restrict__ cnt, double* __restrict__ rays, MgPoint* __restrict__ gp,
            mcp_store_entry* __restrict__ store) {
  const int k = blockIdx.x*SA_BLOCK + threadIdx.x;
  const int made = counts[Q.n_targets];
  if (k >= made || k >= Q.n_rows) return;
  const mcp_stereo_point P = recs[k];
  const int row = rows[k];
  const long long at = (long long)Q.first_store + 2*(long long)k;
  if (row < 0 || row >= Q.table_rows || row >= Q.graph_rows || P.target < 0 || P.target >= Q.n_targets || at + 1 >= Q.store_cap) return;      // (never: checked and grown on the host)
  SaRow R; mcp_store_entry root, epi;
  sa_point(P, row, Q.level, Q.src_mkf, Q.src_cam, target_mkf[P.target], target_cam[P.target], R, root, epi);
  sa_write_row(R, row, keys[k], Q.slot1, Q.ncam_states, pts, src, states, cnt, rays, gp);
  store[at] = root; store[at + 1] = epi;
}
#endif  // __HIPCC__

// ---- the host's statement -------------------------------------------------------------------------------------------------------------------
// the busy list of a store in store order; out: NULL (count only) or cap records.  Returns the length (it may pass cap: nothing is written past it)
inline int sa_host_busy(int n_store, const mcp_store_entry* store, int src_mkf, int src_cam, int cap, mcp_stereo_meas* out) {
  int n = 0;
  for (int i = 0; i < n_store; ++i) {
    if (!sa_busy_match(store[i], src_mkf, src_cam)) continue;
    if (out && n < cap) sa_busy_record(store[i], out[n]);
    ++n;
  }
  return n;
}

}  // namespace mcp
