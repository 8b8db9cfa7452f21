// pvs_kernels.h -- Tracker::FindPVS over a device-resident map-point table (src/Tracker.cc:662-723), gfx950.
//
// One thread per (row, camera).  k_pvs_mark (k_pvs_mark_at: the same body with the pose read from device memory; k_pvs_mark_gated: that behind a device-side word) runs the per-point part of FindPVS -- TrackerData::Project, the level-0 mask test,
// GetDerivsUnsafe, PatchFinder::CalcSearchLevelAndWarpMatrix -- through the same __device__ helpers the per-point search uses
// (track_project / track_warp_level, img_kernels.h), so the results carry the search's bits; it leaves every accepted entry in a
// (camera, row) slot and the per-workgroup counts of each level.  k_pvs_scatter (same stream, next launch) sums the counts of the
// workgroups before its own, ranks its rows within each level by ballot and copies the entries to their place in the pinned block:
// camera c's list starts at out_first, level by level, rows ascending.  No workgroup waits for another, nothing depends on the
// order workgroups are dispatched in; LDS atomics only add integers, so the result is the same bytes on every run.
#pragma once
#include "img_kernels.h"

namespace mcp {

struct PvsPoint { double world_pos[3], pixel_right_w[3], pixel_down_w[3]; int usable, pad_; };      // one table row (80 B)
struct PvsCam {
  mcp_camera cam; Se3 cfb;
  const uint8_t* mask0; int mask_w, mask_h;      // level-0 mask of the target, or null
  int cap, out_first;                            // room for this camera's entries (<= rows) and where they start in the pinned block
};
constexpr int PVS_BLOCK = 256;

// (the body of k_pvs_mark and k_pvs_mark_at; cnt: MCP_LEVELS ints of the caller's LDS; near: NULL, or one byte per row whose bit c says
// whether camera c judges the row at all -- mcp_track_collect_nearest)
__device__ __forceinline__ void pvs_mark_body(const PvsCam* __restrict__ tab, const Se3& bfw, const PvsPoint* __restrict__ pts, int n, int nblk, signed char* __restrict__ lvl,
                                              mcp_pvs_entry* __restrict__ ent, int* __restrict__ blk_cnt, int* cnt, const uint8_t* __restrict__ near) {
  const int c = blockIdx.y, i = blockIdx.x*PVS_BLOCK + threadIdx.x;
  if (threadIdx.x < MCP_LEVELS) cnt[threadIdx.x] = 0;
  __syncthreads();
  if (i < n) {
    const PvsPoint& P = pts[i];
    const PvsCam& C = tab[c];
    int level = -1;
    if (P.usable && (!near || ((near[i] >> c) & 1))) {                                   // !mbBad && mbOptimized, Tracker.cc:680; near: the collected set (map_graph_collect.h)
      Se3 cfw; double xc[3]; Projection pr;
      bool keep = track_project(C.cam, bfw, C.cfb, P.world_pos, cfw, xc, pr);             // mbInImage, :693-695
      // :698: mask[ir(v2Image)] == 0 drops the point.  The reference reads past the mask for u == w or v == h; here such a point is
      // dropped (u, v >= 0 once the projection is in the image)
      if (keep && C.mask0) keep = pr.u < (double)C.mask_w && pr.v < (double)C.mask_h && C.mask0[(size_t)(int)pr.v*C.mask_w + (int)pr.u] != 0;
      if (keep) {
        double dT[3], dP[3], WI[4]; bool rejected;
        const int lv = track_warp_level(cfw, xc, pr, P.pixel_right_w, P.pixel_down_w, dT, dP, WI, &rejected);     // :702-706
        if (!rejected) {
          level = lv;
          mcp_pvs_entry& E = ent[(size_t)c*n + i];
          E.point = i; E.level = lv; E.image[0] = pr.u; E.image[1] = pr.v;
#pragma unroll
          for (int k = 0; k < 4; ++k) { E.cam_derivs[k] = pr.D[k]; E.warp_inverse[k] = WI[k]; }
          atomicAdd(&cnt[lv], 1);
        }
      }
    }
    lvl[(size_t)c*n + i] = (signed char)level;
  }
  __syncthreads();
  if (threadIdx.x < MCP_LEVELS) blk_cnt[((size_t)c*nblk + blockIdx.x)*MCP_LEVELS + threadIdx.x] = cnt[threadIdx.x];
}
__global__ void __launch_bounds__(PVS_BLOCK)
k_pvs_mark(const PvsCam* __restrict__ tab, Se3 bfw, const PvsPoint* __restrict__ pts, int n, int nblk, signed char* __restrict__ lvl /* ncam x n */,
           mcp_pvs_entry* __restrict__ ent /* ncam x n, written where lvl >= 0 */, int* __restrict__ blk_cnt /* ncam x nblk x MCP_LEVELS */,
           const uint8_t* __restrict__ near /* n, or null */) {
  __shared__ int cnt[MCP_LEVELS];
  pvs_mark_body(tab, bfw, pts, n, nblk, lvl, ent, blk_cnt, cnt, near);
}
// the same pass with BaseFromWorld read from device memory (12 doubles, R row-major then t): the pose an earlier kernel of the same stream left
// there (mcp_track_frame_motion: k_motion_prior)
__global__ void __launch_bounds__(PVS_BLOCK)
k_pvs_mark_at(const PvsCam* __restrict__ tab, const double* __restrict__ bfw12, const PvsPoint* __restrict__ pts, int n, int nblk, signed char* __restrict__ lvl,
              mcp_pvs_entry* __restrict__ ent, int* __restrict__ blk_cnt, const uint8_t* __restrict__ near) {
  __shared__ int cnt[MCP_LEVELS];
  Se3 bfw;
#pragma unroll
  for (int k = 0; k < 9; ++k) bfw.R[k] = bfw12[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) bfw.t[k] = bfw12[9 + k];
  pvs_mark_body(tab, bfw, pts, n, nblk, lvl, ent, blk_cnt, cnt, near);
}
// k_pvs_mark_at behind a device-side word an earlier kernel of the stream left (mcp_track_frame_recover: k_reloc_pick).  *gate == 0: nobody
// recovered, the reference runs no TrackMap -- every (row, camera) is marked outside and every count is zero, the empty-PVS case for all
// later launches.  *gate != 0: k_pvs_mark_at's pass, the same body
__global__ void __launch_bounds__(PVS_BLOCK)
k_pvs_mark_gated(const int* __restrict__ gate, const PvsCam* __restrict__ tab, const double* __restrict__ bfw12, const PvsPoint* __restrict__ pts, int n, int nblk,
                 signed char* __restrict__ lvl, mcp_pvs_entry* __restrict__ ent, int* __restrict__ blk_cnt, const uint8_t* __restrict__ near) {
  __shared__ int cnt[MCP_LEVELS];
  if (*gate == 0) {      // (uniform over the grid)
    const int c = blockIdx.y, i = blockIdx.x*PVS_BLOCK + threadIdx.x;
    if (i < n) lvl[(size_t)c*n + i] = (signed char)-1;
    if (threadIdx.x < MCP_LEVELS) blk_cnt[((size_t)c*nblk + blockIdx.x)*MCP_LEVELS + threadIdx.x] = 0;
    return;
  }
  Se3 bfw;
#pragma unroll
  for (int k = 0; k < 9; ++k) bfw.R[k] = bfw12[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) bfw.t[k] = bfw12[9 + k];
  pvs_mark_body(tab, bfw, pts, n, nblk, lvl, ent, blk_cnt, cnt, near);
}

__global__ void __launch_bounds__(PVS_BLOCK)
k_pvs_scatter(const PvsCam* __restrict__ tab, int n, int nblk, const signed char* __restrict__ lvl, const mcp_pvs_entry* __restrict__ ent,
              const int* __restrict__ blk_cnt, mcp_pvs_entry* __restrict__ out /* pinned host */, int* __restrict__ counts /* pinned host, ncam x MCP_LEVELS */) {
  constexpr int NW = PVS_BLOCK/64;
  __shared__ int before[MCP_LEVELS], total[MCP_LEVELS], wcnt[NW][MCP_LEVELS];
  const int c = blockIdx.y, b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < MCP_LEVELS) { before[t] = 0; total[t] = 0; }
  __syncthreads();
  // this camera's level counts: all workgroups (the list sizes) and those before this one (where this workgroup's rows go)
  int mb[MCP_LEVELS], mt[MCP_LEVELS];
#pragma unroll
  for (int l = 0; l < MCP_LEVELS; ++l) { mb[l] = 0; mt[l] = 0; }
  for (int j = t; j < nblk; j += PVS_BLOCK) {
    const int* q = blk_cnt + ((size_t)c*nblk + j)*MCP_LEVELS;
#pragma unroll
    for (int l = 0; l < MCP_LEVELS; ++l) { const int v = q[l]; mt[l] += v; if (j < b) mb[l] += v; }
  }
#pragma unroll
  for (int l = 0; l < MCP_LEVELS; ++l) { if (mt[l]) atomicAdd(&total[l], mt[l]); if (mb[l]) atomicAdd(&before[l], mb[l]); }
  const int i = b*PVS_BLOCK + t;
  const int my = i < n ? (int)lvl[(size_t)c*n + i] : -1;
  int rank = 0;
#pragma unroll
  for (int l = 0; l < MCP_LEVELS; ++l) {
    const unsigned long long m = __ballot(my == l);
    if (my == l) rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[wave][l] = __popcll(m);
  }
  __syncthreads();
  const PvsCam& C = tab[c];
  int all = 0;
#pragma unroll
  for (int l = 0; l < MCP_LEVELS; ++l) all += total[l];
  if (b == 0 && t < MCP_LEVELS) counts[c*MCP_LEVELS + t] = total[t];
  if (my < 0 || all > C.cap) return;                    // over the cap: nothing of this camera is written (the host reports it)
  int off = before[my];
  for (int l = 0; l < my; ++l) off += total[l];
  for (int w = 0; w < wave; ++w) off += wcnt[w][my];
  out[C.out_first + off + rank] = ent[(size_t)c*n + i];   // off + rank < all <= cap
}

// mcp_map_points_update: rows ids[k] <- recs[k] (ids distinct, checked on the host)
__global__ void __launch_bounds__(256)
k_map_points_scatter(PvsPoint* __restrict__ rows, int count, const int* __restrict__ ids, const PvsPoint* __restrict__ recs) {
  const int k = blockIdx.x*256 + threadIdx.x;
  if (k < count) rows[ids[k]] = recs[k];
}

// mcp_map_points_update_rays: the patch rays (9 doubles) of rows ids[k] <- recs[k] (ids distinct, checked on the host)
__global__ void __launch_bounds__(256)
k_map_rays_scatter(double* __restrict__ rays, int count, const int* __restrict__ ids, const double* __restrict__ recs) {
  const int k = blockIdx.x*256 + threadIdx.x;
  if (k >= count) return;
  double* o = rays + 9*(size_t)ids[k];
#pragma unroll
  for (int a = 0; a < 9; ++a) o[a] = recs[9*(size_t)k + a];
}

}  // namespace mcp
