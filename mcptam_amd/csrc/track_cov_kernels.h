// track_cov_kernels.h -- the pose covariance of the last fine iteration (mcp_track_pose_cov, the one-call frames with
// mcp_track_pose_cov_enable; include/mcp_img.h), gfx950.
//
//   k_pose_cov_tiles   per tile of COV_TILE records in record order, one thread per record: the 21 products w Jr[x] Jr[y] of the record's
//                      2 x 6 Jacobian at the pose the last iteration linearised at (thread 0 rebuilds it into LDS), summed over each wavefront
//                      by wave_reduce_scatter32, the four wavefront sums added in wavefront order: one 21-double partial and one count of
//                      used records PER TILE, whatever the grid -- the bits do not depend on how many workgroups ran
//   k_pose_cov_finish  one wavefront: lane k < 21 adds the tile partials in ascending tile order, lane 0 adds the prior, takes the
//                      pseudo-inverse and writes the record to pinned host memory
// The arithmetic is track_cov.h's (__host__ __device__: mcp_track_pose_cov_host runs the same source in the same order).  No floating-point
// atomics, no workgroup waits for another, nothing loops on data without a cap (the Jacobi sweeps end after MCP_POSE_COV_MAX_SWEEPS).
#pragma once
#include "track_cov.h"

namespace mcp {

__global__ void __launch_bounds__(COV_TILE)
k_pose_cov_tiles(int n, const int* __restrict__ n_dev /* the record count from device memory, or NULL: n */, const int* __restrict__ gate /* 0: nothing runs; NULL: open */,
                 int cap /* records the buffers hold */, const mcp_pose_point* __restrict__ pts, const double* __restrict__ weights, const double* __restrict__ cfb_all,
                 const double* __restrict__ refined /* 12 */, const double* __restrict__ mu_last /* 6 */, double* __restrict__ part /* tiles x 21 */,
                 int* __restrict__ used /* tiles */) {
  __shared__ double pose[12];
  __shared__ double red[COV_TILE/64][COV_NPROD];
  __shared__ int cnt[COV_TILE/64];
  if (gate && *gate == 0) return;
  if (n_dev) n = *n_dev;
  if (n > cap) n = cap;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) cov_pose_before(refined, mu_last, pose);
  __syncthreads();
  const int tiles = (n + COV_TILE - 1)/COV_TILE;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // (uniform per workgroup: the barriers below are reached by all)
    const int i = tile*COV_TILE + t;
    double w32[32];
    bool u = false;
    if (i < n) u = cov_record_products(pts[i], weights[i], pose, cfb_all, w32);
    else {
#pragma unroll
      for (int k = 0; k < COV_NPROD; ++k) w32[k] = 0.0;
    }
#pragma unroll
    for (int k = COV_NPROD; k < 32; ++k) w32[k] = 0.0;
    int idx; const double total = wave_reduce_scatter32(w32, lane, idx);
    if (!(lane & 1) && idx < COV_NPROD) red[wave][idx] = total;
    const unsigned long long b = __ballot(u);
    if (lane == 0) cnt[wave] = __popcll(b);
    __syncthreads();
    if (t < COV_NPROD) {
      double sum = 0.0;
#pragma unroll
      for (int wv = 0; wv < COV_TILE/64; ++wv) sum += red[wv][t];
      part[(size_t)COV_NPROD*tile + t] = sum;
    }
    if (t == 32) { int c = 0; for (int wv = 0; wv < COV_TILE/64; ++wv) c += cnt[wv]; used[tile] = c; }
    __syncthreads();                                                    // (red and cnt are rewritten by the next tile)
  }
}

__global__ void __launch_bounds__(64)
k_pose_cov_finish(int n, const int* __restrict__ n_dev, const int* __restrict__ gate, int cap, const double* __restrict__ part, const int* __restrict__ used,
                  mcp_track_pose_cov_record* __restrict__ out /* pinned; zeros (valid = 0) when the gate is closed: the host cleared it */) {
  __shared__ double sums[COV_NPROD];
  __shared__ CovWork W;
  __shared__ int n_used;
  if (gate && *gate == 0) return;
  if (n_dev) n = *n_dev;
  if (n > cap) n = cap;
  const int tiles = (n + COV_TILE - 1)/COV_TILE;
  const int t = threadIdx.x;
  if (t < COV_NPROD) {
    // eight loads in flight, added in tile order: the additions are those of a plain loop, the load latencies overlap
    double sum = 0.0;
    int tile = 0;
    for (; tile + 8 <= tiles; tile += 8) {
      double v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = part[(size_t)COV_NPROD*(tile + j) + t];
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += v[j];
    }
    for (; tile < tiles; ++tile) sum += part[(size_t)COV_NPROD*tile + t];
    sums[t] = sum;
  }
  if (t >= 32) {      // the counts: lane 32 + j takes the tiles j, j + 32, ...; integer sums, any order the same
    int c = 0;
    for (int tile = t - 32; tile < tiles; tile += 32) c += used[tile];
    for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (t == 32) n_used = c;
  }
  __syncthreads();
  if (t == 0) cov_finish(sums, n_used, W, out);
}

}  // namespace mcp
