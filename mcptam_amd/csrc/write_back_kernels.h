// write_back_kernels.h -- BundleAdjusterMulti::AdjustAndUpdate's write-back over the resident map-point table
// (src/BundleAdjusterMulti.cc:286-334, src/MapPoint.cc:62-87, src/KeyFrame.cc:547-645), gfx950.
//
//   k_wb_chains       one lane per distinct pose chain of the call: the product of its poses at the solver's current state (the order of
//                     k_chains, ba_kernels.h) -- the source pose of every point and the CamFromWorld of every keyframe come from this table.
//   k_wb_points       one lane per point: world = Ts^-1 x (a fixed point: x), RefreshPixelVectors with the row's patch rays
//                     (stereo_pixel_vectors, the device function mcp_stereo_points uses), the whole row, and the three vectors to the host.
//   k_wb_scene_depth  one workgroup per keyframe: RefreshSceneDepthRobust.  The reference sorts the list twice only to read element [n/2] of each
//                     order; here both are exact radix selects over the 64-bit patterns of the (non-negative) values -- eight 8-bit passes with an
//                     integer LDS histogram -- so a list of any length takes the same path (values in LDS up to SD_LDS entries, from the
//                     workgroup's own global scratch beyond).  The three weighted sums have a FIXED order: thread t of SD_BLOCK adds entries
//                     t, t + SD_BLOCK, ... in ascending position, a wavefront folds its 64 partials by halving (lane l += lane l + 32, 16, ... 1)
//                     and thread 0 adds the wavefronts' totals 0, 1, 2, 3.  No floating-point atomics anywhere: same state, same bits.
#pragma once
#include "pvs_kernels.h"
#include "stereo_kernels.h"

namespace mcp {

struct WbChain { int len; int v[MCP_MAX_CHAIN]; };        // pose indices into the solver's pose array
// one point of a write-back: index into the solver's point array, table row, slot of its own chain, 2 * (slot of the chain RefreshPixelVectors uses) + fixed
struct WbItem { int pt, row, own, src2_fixed; };
constexpr int WB_BLOCK = 256;
constexpr int SD_BLOCK = 256;
constexpr int SD_LDS = 2048;                              // depths kept in LDS (16 KB); longer lists are re-read from global memory

__device__ inline void wb_load_se3(const double* __restrict__ p, Se3& T) {
#pragma unroll
  for (int k = 0; k < 9; ++k) T.R[k] = p[k];
  T.t[0] = p[9]; T.t[1] = p[10]; T.t[2] = p[11];
}

__global__ void __launch_bounds__(64)
k_wb_chains(int nchain, const WbChain* __restrict__ chains, const double* __restrict__ pose_T, double* __restrict__ T /* nchain x 12 */,
            double* __restrict__ T_host /* pinned mirror, or null */) {
  const int c = blockIdx.x*64 + threadIdx.x;
  if (c >= nchain) return;
  const WbChain C = chains[c];
  Se3 acc; se3_identity(acc);
  for (int i = 0; i < C.len; ++i) { Se3 v; wb_load_se3(pose_T + 12*(size_t)C.v[i], v); se3_compose(v, acc, acc); }
#pragma unroll
  for (int k = 0; k < 12; ++k) { const double x = k < 9 ? acc.R[k] : acc.t[k - 9]; T[12*(size_t)c + k] = x; if (T_host) T_host[12*(size_t)c + k] = x; }
}

__global__ void __launch_bounds__(WB_BLOCK)
k_wb_points(int n, const WbItem* __restrict__ items, const double* __restrict__ pt_x, const double* __restrict__ T, const double* __restrict__ rays /* rows x 9 */,
            PvsPoint* __restrict__ rows, double* __restrict__ world_out, double* __restrict__ right_out, double* __restrict__ down_out /* pinned, n x 3 each, or null */) {
  const int k = blockIdx.x*WB_BLOCK + threadIdx.x;
  if (k >= n) return;
  const WbItem it = items[k];
  const int src = it.src2_fixed >> 1;
  Se3 To; wb_load_se3(T + 12*(size_t)it.own, To);
  const double x[3] = { pt_x[3*(size_t)it.pt], pt_x[3*(size_t)it.pt + 1], pt_x[3*(size_t)it.pt + 2] };
  double world[3];
  if (it.src2_fixed & 1) { world[0] = x[0]; world[1] = x[1]; world[2] = x[2]; }          // mbFixed: GetPoint as is
  else se3_apply_inv(To, x, world);                                                       // CamFromWorld_src^-1 * GetPoint
  Se3 Ts = To;
  if (src != it.own) wb_load_se3(T + 12*(size_t)src, Ts);
  const double* r = rays + 9*(size_t)it.row;
  const double ce[3] = { r[0], r[1], r[2] }, ri[3] = { r[3], r[4], r[5] }, dn[3] = { r[6], r[7], r[8] };
  double pr[3], pd[3];
  stereo_pixel_vectors(Ts, ce, ri, dn, world, pr, pd);
  PvsPoint P;
#pragma unroll
  for (int a = 0; a < 3; ++a) { P.world_pos[a] = world[a]; P.pixel_right_w[a] = pr[a]; P.pixel_down_w[a] = pd[a]; }
  P.usable = 1; P.pad_ = 0;                                                               // mbOptimized = true (the caller names no bad points)
  rows[it.row] = P;
  if (world_out) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { world_out[3*(size_t)k + a] = world[a]; right_out[3*(size_t)k + a] = pr[a]; down_out[3*(size_t)k + a] = pd[a]; }
  }
}

// exact k-th smallest (0-based) of key(0) .. key(n-1), 64-bit keys; all SD_BLOCK threads call it with the same arguments
template <class F>
__device__ inline unsigned long long sd_select(int n, int k, F key, int* hist /* 256 */, int* wtot /* SD_BLOCK/64 */, unsigned long long* s_prefix, int* s_k) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned long long prefix = 0, mask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += SD_BLOCK) { const unsigned long long q = key(i); if ((q & mask) == prefix) atomicAdd(&hist[(int)((q >> shift) & 255ull)], 1); }
    __syncthreads();
    const int c = hist[t];
    int incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += wtot[w];
    const int excl = incl - c;
    if (excl <= k && k < incl) { *s_prefix = prefix | ((unsigned long long)t << shift); *s_k = k - excl; }      // exactly one thread: k < the number of keys left
    __syncthreads();
    prefix = *s_prefix; k = *s_k; mask |= 0xFFull << shift;
  }
  return prefix;
}

// Huber::SquareRootWeight (include/mcptam/MEstimator.h:168-179)
__host__ __device__ inline double huber_sqrt_weight(double e2, double s2) { return sqrt(e2 < s2 ? 1.0 : sqrt(s2/e2)); }

__global__ void __launch_bounds__(SD_BLOCK)
k_wb_scene_depth(const double* __restrict__ T /* 12 per pose */, const int* __restrict__ slot /* pose of keyframe j, or null: j */, const int* __restrict__ seg_start,
                 const int* __restrict__ seg_rows, const double* __restrict__ seg_w, const PvsPoint* __restrict__ rows,
                 double* depth /* device scratch, one per list entry; read back by this workgroup */, mcp_scene_depth* __restrict__ out /* pinned */,
                 double* __restrict__ depths_host /* pinned, or null */) {
  __shared__ double cache[SD_LDS];
  __shared__ int hist[256];
  __shared__ int wtot[SD_BLOCK/64];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_k;
  __shared__ double red[3][SD_BLOCK/64];
  const int j = blockIdx.x, t = threadIdx.x;
  const int s0 = seg_start[j], n = seg_start[j + 1] - s0;
  const bool in_lds = n <= SD_LDS;
  Se3 cfw; wb_load_se3(T + 12*(size_t)(slot ? slot[j] : j), cfw);
  for (int i = t; i < n; i += SD_BLOCK) {                       // GetPointDepthsAndWeights (:549-570): norm(CamFromWorld * mv3WorldPos)
    double xc[3]; se3_apply(cfw, rows[seg_rows[s0 + i]].world_pos, xc);
    const double d = sqrt(xc[0]*xc[0] + xc[1]*xc[1] + xc[2]*xc[2]);
    depth[s0 + i] = d;
    if (depths_host) depths_host[s0 + i] = d;
    if (in_lds) cache[i] = d;
  }
  if (n <= 3) {                                                 // :587-591: the keyframe is left alone
    if (t == 0) { mcp_scene_depth o; o.mean = 0; o.sigma = 0; o.median = 0; o.sigma_sq = 0; o.n = n; o.refreshed = 0; out[j] = o; }
    return;
  }
  __syncthreads();
  const double* dv = in_lds ? cache : depth + s0;
  // element [n/2] of the sorted depths (:595-596) ...
  const double med = __longlong_as_double((long long)sd_select(n, n/2, [&](int i) { return (unsigned long long)__double_as_longlong(dv[i]); }, hist, wtot, &s_prefix, &s_k));
  // ... and of the sorted squared distances from it (Huber::FindSigmaSquared, MEstimator.h:194-204)
  const double med2 = __longlong_as_double((long long)sd_select(n, n/2, [&](int i) { const double e = dv[i] - med; return (unsigned long long)__double_as_longlong(e*e); },
                                                                hist, wtot, &s_prefix, &s_k));
  double sg = 1.4826*(1 + 5.0/(double)((long long)n*2 - 6))*sqrt(med2);
  sg = 1.345*sg;
  double s2 = sg*sg;
  if (s2 < 0.4) s2 = 0.4;                                       // :612-613
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = t; i < n; i += SD_BLOCK) {                       // :619-630
    const double d = dv[i], e = d - med;
    const double cw = seg_w[s0 + i]*huber_sqrt_weight(e*e, s2);
    a0 += cw*d; a1 += cw*d*d; a2 += cw;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a0 += __shfl_down(a0, o, 64); a1 += __shfl_down(a1, o, 64); a2 += __shfl_down(a2, o, 64); }
  if ((t & 63) == 0) { red[0][t >> 6] = a0; red[1][t >> 6] = a1; red[2][t >> 6] = a2; }
  __syncthreads();
  if (t == 0) {
    double S0 = 0.0, S1 = 0.0, S2 = 0.0;
    for (int w = 0; w < SD_BLOCK/64; ++w) { S0 += red[0][w]; S1 += red[1][w]; S2 += red[2][w]; }
    mcp_scene_depth o;
    o.mean = S0/S2;                                             // :632-633
    o.sigma = sqrt(S1/S2 - o.mean*o.mean);
    o.median = med; o.sigma_sq = s2; o.n = n;
    o.refreshed = isfinite(o.mean) ? 1 : -1;                    // :635-644: the reference stops the process here; the host decides
    out[j] = o;
  }
}

}  // namespace mcp
