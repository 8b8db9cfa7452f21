// track_record_kernels.h -- what Tracker::TrackMap leaves behind, from the items of mcp_track_map while they are still in device memory
// (src/Tracker.cc:1157-1274, 1322-1361, 1452-1489, 1618-1658), gfx950.
//
// mcp_track_map_record (img_api.hip) enqueues, after the fine iterations of track_map_kernels.h and on the same stream:
//   k_tr_mark         one thread per item, tiles of TR_BLOCK items taken grid-stride up to ctl->n_fine (known on the device only).  Reads the
//                     item's flag words and the weight of the last fine iteration; writes the 8-byte note to pinned memory, the mark into the
//                     row's count column (integer atomicAdd: a row seen by several cameras gets one per camera, in any order the same sum),
//                     the found flag for the next kernel.  The 2 x ncam x 4 level counters, the per-camera found counts and the two mark
//                     totals are summed in LDS and flushed once per workgroup; every tile leaves its number of found items.  Workgroup 0
//                     composes the cam_from_world table at the refined pose (se3_compose, the product FindPVS uses).
//   k_tr_scatter      the same tiles.  Items are camera-major, so the found items in item order ARE the cameras' lists one after the other: a
//                     found item goes to (found items of the tiles before) + (its ballot rank in the tile).  Writes its mcp_track_meas to
//                     pinned memory, row and weight inlier / (inlier + outlier) -- the column after ALL marks, the kernel boundary sees to that
//                     -- to the scene-depth lists; workgroup 0 writes seg_start, the counters and the quality of every camera.
//   k_wb_scene_depth  <<<ncam>>>, unchanged (write_back_kernels.h), its output in the pinned record.
//   k_tm_finish       as in mcp_track_map, or k_tr_finish: the result block without the item copy.
// No workgroup waits for another; nothing depends on dispatch order; no floating-point atomics: same state, same bytes.
#pragma once
#include "track_map_kernels.h"
#include "write_back_kernels.h"

namespace mcp {

constexpr int TR_BLOCK = 256;

// sums of one call (device memory, zeroed before k_tr_mark)
struct TrAcc { int attempted[MCP_MAX_FRAME_CAMS][MCP_LEVELS], found[MCP_MAX_FRAME_CAMS][MCP_LEVELS]; int n_meas[MCP_MAX_FRAME_CAMS]; int n_inliers, n_outlier_marks; };
constexpr int TR_ACC_WORDS = (int)(sizeof(TrAcc)/sizeof(int));
struct TrParams { int ncam, lost, min_patches, coarse_min; double good, bad; };

static_assert(sizeof(mcp_track_note) == 8 && sizeof(mcp_track_meas) == 32, "the notes and measurements cross as 8- and 32-byte records");

// rows [first, first + count) of the count column <- (1, 0): the MapPoint constructor's values
__global__ void __launch_bounds__(256)
k_tr_counts_fill(int* __restrict__ cnt, int first, int count) {
  const int k = blockIdx.x*256 + threadIdx.x;
  if (k < count) *reinterpret_cast<int2*>(cnt + 2*(size_t)(first + k)) = make_int2(1, 0);
}
// mcp_map_points_update_counts: rows ids[k] <- recs[k] (ids distinct, checked on the host)
__global__ void __launch_bounds__(256)
k_tr_counts_scatter(int* __restrict__ cnt, int count, const int* __restrict__ ids, const int* __restrict__ recs) {
  const int k = blockIdx.x*256 + threadIdx.x;
  if (k < count) *reinterpret_cast<int2*>(cnt + 2*(size_t)ids[k]) = *reinterpret_cast<const int2*>(recs + 2*(size_t)k);
}

// AssessTrackingQuality (:1620-1657) of one camera: 0 BAD, 1 DODGY, 2 GOOD
__host__ __device__ inline int tr_quality(const int* attempted, const int* found, int min_patches, int coarse_min, double good, double bad) {
  int ta = 0, tf = 0, la = 0, lf = 0;
  for (int l = 0; l < MCP_LEVELS; ++l) { ta += attempted[l]; tf += found[l]; if (l >= 2) { la += attempted[l]; lf += found[l]; } }
  if (tf < min_patches) return 0;
  const double tfrac = (double)tf/(double)ta;
  const double lfrac = la > coarse_min ? (double)lf/(double)la : tfrac;
  if (tfrac > good) return 2;
  return lfrac < bad ? 0 : 1;
}

__global__ void __launch_bounds__(TR_BLOCK)
k_tr_mark(TrParams P, const TmCtl* __restrict__ ctl, const TmCam* __restrict__ cams, const double* __restrict__ pose, const mcp_track_map_item* __restrict__ items,
          const double* __restrict__ weights, int* __restrict__ cnt /* the count column */, mcp_track_note* __restrict__ notes /* pinned */, uint8_t* __restrict__ found_flag,
          int* __restrict__ tile_found, TrAcc* __restrict__ acc, double* __restrict__ cfw /* ncam x 12 */, double* __restrict__ cfw_host /* pinned, ncam x 12 */) {
  __shared__ int s_acc[TR_ACC_WORDS];
  __shared__ int s_tile;
  const int t = threadIdx.x, lane = t & 63;
  TrAcc& A = *reinterpret_cast<TrAcc*>(s_acc);
  for (int k = t; k < TR_ACC_WORDS; k += TR_BLOCK) s_acc[k] = 0;
  const TmCtl& C = *ctl;
  const int n = C.n_fine, ntile = (n + TR_BLOCK - 1)/TR_BLOCK;
  if (blockIdx.x == 0 && t < P.ncam) {                               // CamFromWorld of camera t at the refined pose
    Se3 bfw, T;
#pragma unroll
    for (int k = 0; k < 9; ++k) bfw.R[k] = pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) bfw.t[k] = pose[9 + k];
    se3_compose(cams[t].cfb, bfw, T);
#pragma unroll
    for (int k = 0; k < 12; ++k) { const double x = k < 9 ? T.R[k] : T.t[k - 9]; cfw[12*t + k] = x; cfw_host[12*t + k] = x; }
  }
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    if (t == 0) s_tile = 0;
    __syncthreads();
    const int i = tile*TR_BLOCK + t;
    bool is_found = false;
    if (i < n) {
      int j, first;
      const int c = tm_locate(P.ncam, i, [&](int q) { return C.sizes[q][0] + C.sizes[q][1] + C.sizes[q][2]; }, &j, &first);
      const mcp_track_map_item& It = items[i];
      const mcp_td_out& O = It.out;
      const int row = It.point, level = O.search_level;
      const bool searched = O.searched != 0, bad = O.template_bad != 0;
      is_found = O.found != 0;
      const bool attempted = !bad && level >= 0 && level < MCP_LEVELS;
      int mark = 0;                                                   // :1452-1489
      if (!is_found) { if (searched && !P.lost) mark = 2; }
      else mark = weights[i] == 0.0 ? 2 : 1;
      unsigned int flags = (searched ? MCP_TN_SEARCHED : 0) | (is_found ? MCP_TN_FOUND : 0) | (O.did_subpix ? MCP_TN_DID_SUBPIX : 0) | (bad ? MCP_TN_TEMPLATE_BAD : 0) |
                           (O.in_image ? MCP_TN_IN_IMAGE : 0) | (attempted ? MCP_TN_ATTEMPTED : 0) | ((unsigned int)mark << MCP_TN_MARK_SHIFT);
      const unsigned long long hi = (unsigned long long)(unsigned int)(c & 255) | ((unsigned long long)(unsigned int)(It.stage & 255) << 8) |
                                    ((unsigned long long)(unsigned int)(level & 255) << 16) | ((unsigned long long)flags << 24);
      reinterpret_cast<unsigned long long*>(notes)[i] = (unsigned long long)(unsigned int)row | (hi << 32);      // one 8-byte store
      found_flag[i] = is_found ? 1 : 0;
      if (mark) atomicAdd(&cnt[2*(size_t)row + (mark == 2 ? 1 : 0)], 1);
      if (c >= 0) {
        if (attempted) { atomicAdd(&A.attempted[c][level], 1); if (is_found) atomicAdd(&A.found[c][level], 1); }
        if (is_found) atomicAdd(&A.n_meas[c], 1);
      }
      if (mark == 1) atomicAdd(&A.n_inliers, 1);
      if (mark == 2) atomicAdd(&A.n_outlier_marks, 1);
    }
    const unsigned long long m = __ballot(is_found);
    if (lane == 0 && m) atomicAdd(&s_tile, __popcll(m));
    __syncthreads();
    if (t == 0) tile_found[tile] = s_tile;
  }
  __syncthreads();
  for (int k = t; k < TR_ACC_WORDS; k += TR_BLOCK) { const int v = s_acc[k]; if (v) atomicAdd(reinterpret_cast<int*>(acc) + k, v); }
}

__global__ void __launch_bounds__(TR_BLOCK)
k_tr_scatter(TrParams P, const TmCtl* __restrict__ ctl, const mcp_track_map_item* __restrict__ items, const uint8_t* __restrict__ found_flag, const int* __restrict__ tile_found,
             const TrAcc* __restrict__ acc, const int* __restrict__ cnt, mcp_track_meas* __restrict__ meas /* pinned */, int* __restrict__ seg_start /* ncam + 1 */,
             int* __restrict__ seg_rows, double* __restrict__ seg_w, mcp_track_record* __restrict__ rec /* pinned */) {
  constexpr int NW = TR_BLOCK/64;
  __shared__ int s_before, s_wcnt[NW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const TmCtl& C = *ctl;
  const int n = C.n_fine, ntile = (n + TR_BLOCK - 1)/TR_BLOCK;
  if (blockIdx.x == 0) {
    if (t == 0) {
      int s = 0, qmax = 0;
      for (int c = 0; c < P.ncam; ++c) {
        seg_start[c] = s; s += acc->n_meas[c];
        rec->n_items[c] = C.sizes[c][0] + C.sizes[c][1] + C.sizes[c][2]; rec->n_meas[c] = acc->n_meas[c];
        const int q = tr_quality(acc->attempted[c], acc->found[c], P.min_patches, P.coarse_min, P.good, P.bad);
        rec->quality[c] = q; qmax = max(qmax, q);
      }
      seg_start[P.ncam] = s;
      rec->quality_max = qmax; rec->n_inliers = acc->n_inliers; rec->n_outlier_marks = acc->n_outlier_marks;
    }
    if (t < MCP_MAX_FRAME_CAMS*MCP_LEVELS) { (&rec->attempted[0][0])[t] = (&acc->attempted[0][0])[t]; (&rec->found[0][0])[t] = (&acc->found[0][0])[t]; }
  }
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    if (t == 0) s_before = 0;
    __syncthreads();
    int mb = 0;
    for (int q = t; q < tile; q += TR_BLOCK) mb += tile_found[q];
    if (mb) atomicAdd(&s_before, mb);
    const int i = tile*TR_BLOCK + t;
    const bool f = i < n && found_flag[i] != 0;
    const unsigned long long m = __ballot(f);
    const int rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wcnt[wave] = __popcll(m);
    __syncthreads();
    if (f) {
      int pos = s_before + rank;
      for (int w = 0; w < wave; ++w) pos += s_wcnt[w];                // pos < (all found items) <= n
      int j, first;
      tm_locate(P.ncam, i, [&](int q) { return C.sizes[q][0] + C.sizes[q][1] + C.sizes[q][2]; }, &j, &first);
      const mcp_track_map_item& It = items[i];
      const int row = It.point;
      mcp_track_meas M;
      M.item = j; M.row = row; M.level = It.out.search_level; M.subpix = It.out.did_subpix ? 1 : 0;
      M.found_pos[0] = It.out.found_pos[0]; M.found_pos[1] = It.out.found_pos[1];
      meas[pos] = M;
      const int2 io = *reinterpret_cast<const int2*>(cnt + 2*(size_t)row);
      seg_rows[pos] = row;
      seg_w[pos] = (double)io.x/(double)(io.x + io.y);                // :1202
    }
    __syncthreads();
  }
}

// the result block of mcp_track_map without the item copy
__global__ void __launch_bounds__(64)
k_tr_finish(TmParams P, const TmCtl* __restrict__ ctl, const double* __restrict__ pose_mu, const int* __restrict__ counts, TmOut* __restrict__ res) {
  tm_write_out(P, ctl, pose_mu, counts, res, threadIdx.x);
}

}  // namespace mcp
