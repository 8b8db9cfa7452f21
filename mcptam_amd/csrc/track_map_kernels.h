// track_map_kernels.h -- Tracker::TrackMap of a frame from the resident map-point table (src/Tracker.cc:938-1075), gfx950.
//
// mcp_track_map (img_api.hip) enqueues on the table's stream, after the two PVS launches of pvs_kernels.h (their lists and counts left in
// device memory):
//   k_tm_select     one workgroup per camera: the keyed shuffle and the sets C / T / R of mcp_img.h (TestForCoarse :726-770,
//                   SetupFineTracking :876-883).  Radix select of the k smallest 64-bit keys (8-bit digits, most significant first,
//                   stopping as soon as the digit bucket holds exactly what is still needed), then a bitonic sort of at most TM_SORT keys
//                   in LDS; longer runs go in chunks of TM_SORT.  Keys of distinct rows are distinct: every run gives the same bytes.
//   k_tm_search     one wavefront per item, grid-stride over a device count: MCP_PF_TRACK finders of the table (patch_item, img_kernels.h),
//                   coarse (C) or fine (T, R; range from the coarse gate); states back into the table, records for the pose iterations.
//   k_tm_gate       one thread: coarse_found > coarse_min, the fine range, the record counts of the two iteration stages.
//   the pose iterations: k_pose_refine_regs / k_pose_refine with the count and the gate read from device memory.
//   k_tm_finish     the items with their weights and the result block into pinned host memory.
// Hand-offs between stages are kernel boundaries on one stream; no workgroup waits for another.  Launch bounds come from the host's
// knowledge of the table: rows, cameras, coarse_max.
#pragma once
#include "img_kernels.h"
#include "pvs_kernels.h"

namespace mcp {

__device__ __forceinline__ unsigned long long tm_key(unsigned long long seed, int stage, int cam, int row) {
  return mcp_track_shuffle_key(seed, stage, cam, row);        // include/mcp_img.h: the one definition every layer uses
}

struct TmSrc { int key, slot1, level, cx, cy, fixed; };           // patch source of a row; slot1 = 1 + index into the slot table, 0 = none
struct TmSlot { const uint8_t* img[MCP_LEVELS]; int w[MCP_LEVELS], h[MCP_LEVELS]; int live, pad_; };     // a source keyframe, resolved per call
struct TmCam { DevKfView T; const uint8_t* mask0; mcp_camera cam; Se3 cfb; };
struct TmStates { mcp_pf_state* s[MCP_MAX_FRAME_CAMS]; };        // per camera: one state per row
// what the device decides and the later stages read (device memory, rewritten by every call)
struct TmCtl {
  int sizes[MCP_MAX_FRAME_CAMS][3];                              // |C|, |T|, |R|
  int stale[MCP_MAX_FRAME_CAMS];
  int coarse_found, did_coarse, fine_range, n_coarse, n_fine, pad_;
};
// the result block the host reads after the wait (pinned)
struct TmOut {
  double pose[12], mu[6];
  int counts[MCP_MAX_FRAME_CAMS][MCP_LEVELS];
  TmCtl ctl;
};
struct TmParams { int ncam, rows, try_coarse, coarse_max, coarse_range, coarse_subpix_its, coarse_min, max_patches; unsigned long long seed; };

constexpr int TM_SEL_NT = 1024, TM_SORT = 2048;

struct TmSelLds {
  unsigned long long skey[TM_SORT]; int sidx[TM_SORT];
  unsigned int hist[256];
  int n_live[MCP_LEVELS], stale, gathered;
  unsigned long long prefix; int need, exact;
};

// the candidates of one selection: entries [a, b) of the camera's PVS that are live, not in the coarse set taken from level 2 (entries
// [e2a, e2b) with stage-0 key <= thr2, when excl), and -- has_lo -- whose sort key is above lo
struct TmCand {
  int a, b, e2a, e2b; bool excl; unsigned long long thr2; bool has_lo; unsigned long long lo;
  __device__ bool in(int i, const unsigned long long* K0, const unsigned long long* Ks, const uint8_t* live) const {
    if (!live[i]) return false;
    if (excl && i >= e2a && i < e2b && K0[i] <= thr2) return false;
    return !has_lo || Ks[i] > lo;
  }
};

// the k smallest sort keys among the candidates, ascending, their rows to out[0..k); returns the largest key written (k > 0)
__device__ unsigned long long tm_emit(TmCand cd, int k, const unsigned long long* __restrict__ K0, const unsigned long long* __restrict__ Ks,
                                      const uint8_t* __restrict__ live, const mcp_pvs_entry* __restrict__ E, int* __restrict__ out, TmSelLds& S) {
  const int t = threadIdx.x, lane = t & 63;
  unsigned long long last = 0ull;
  for (int done = 0; done < k; ) {
    const int kk = min(k - done, TM_SORT);
    // radix select of the kk-th smallest key
    if (t == 0) { S.prefix = 0ull; S.need = kk; S.exact = 0; }
    __syncthreads();
    unsigned long long thr = ~0ull;
    for (int shift = 56; shift >= 0; shift -= 8) {
      for (int j = t; j < 256; j += TM_SEL_NT) S.hist[j] = 0u;
      __syncthreads();
      const unsigned long long himask = shift == 56 ? 0ull : (~0ull << (shift + 8)), prefix = S.prefix;
      for (int i = cd.a + t; i < cd.b; i += TM_SEL_NT)
        if (cd.in(i, K0, Ks, live) && (Ks[i] & himask) == prefix) atomicAdd(&S.hist[(unsigned int)(Ks[i] >> shift) & 255u], 1u);
      __syncthreads();
      if (t < 64) {                                              // the digit whose bucket holds the need-th key: one wavefront scans
        const int need = S.need;
        unsigned int h4[4], s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { h4[q] = S.hist[4*lane + q]; s += h4[q]; }
        unsigned int incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
        unsigned int below = incl - s;
        const bool mine = below < (unsigned int)need && (unsigned int)need <= incl;
        if (mine) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (below + h4[q] >= (unsigned int)need) {
              const int rest = need - (int)below;
              S.prefix = prefix | ((unsigned long long)(4*lane + q) << shift);
              S.need = rest; S.exact = (h4[q] == (unsigned int)rest) ? 1 : 0;
              break;
            }
            below += h4[q];
          }
        }
      }
      __syncthreads();
      if (S.exact) { thr = S.prefix | (shift ? ((1ull << shift) - 1ull) : 0ull); break; }
      if (shift == 0) thr = S.prefix;
    }
    // gather the kk keys at or below the threshold, sort them (ties cannot happen; the padding sorts last by its index)
    if (t == 0) S.gathered = 0;
    __syncthreads();
    for (int i = cd.a + t; i < cd.b; i += TM_SEL_NT)
      if (cd.in(i, K0, Ks, live) && Ks[i] <= thr) { const int p = atomicAdd(&S.gathered, 1); if (p < TM_SORT) { S.skey[p] = Ks[i]; S.sidx[p] = i; } }
    __syncthreads();
    int P = 1; while (P < kk) P <<= 1;
    for (int j = kk + t; j < P; j += TM_SEL_NT) { S.skey[j] = ~0ull; S.sidx[j] = 0x7fffffff; }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int q = t; q < P/2; q += TM_SEL_NT) {
          const int lo_i = 2*q - (q & (stride - 1)), hi_i = lo_i + stride;
          const bool up = (lo_i & size) == 0;
          const unsigned long long ka = S.skey[lo_i], kb = S.skey[hi_i];
          const int ia = S.sidx[lo_i], ib = S.sidx[hi_i];
          const bool gt = ka > kb || (ka == kb && ia > ib);
          if (gt == up) { S.skey[lo_i] = kb; S.skey[hi_i] = ka; S.sidx[lo_i] = ib; S.sidx[hi_i] = ia; }
        }
        __syncthreads();
      }
    for (int r = t; r < kk; r += TM_SEL_NT) out[done + r] = E[S.sidx[r]].point;
    last = S.skey[kk - 1];
    __syncthreads();
    cd.has_lo = true; cd.lo = last;
    done += kk;
  }
  return last;
}

// per camera (blockIdx.x): keys, liveness of the rows' sources, the sets.  pvs / counts: k_pvs_scatter's output for cap = rows,
// out_first = c*rows.  sel + c*rows receives [C | T | R].
__global__ void __launch_bounds__(TM_SEL_NT)
k_tm_select(TmParams P, const mcp_pvs_entry* __restrict__ pvs, const int* __restrict__ counts, const TmSrc* __restrict__ src, const TmSlot* __restrict__ slots,
            unsigned long long* __restrict__ K0all, unsigned long long* __restrict__ K1all, uint8_t* __restrict__ liveall, int* __restrict__ sel, TmCtl* __restrict__ ctl) {
  __shared__ TmSelLds S;
  const int c = blockIdx.x, t = threadIdx.x, n = P.rows;
  const mcp_pvs_entry* E = pvs + (size_t)c*n;
  unsigned long long* K0 = K0all + (size_t)c*n; unsigned long long* K1 = K1all + (size_t)c*n; uint8_t* live = liveall + (size_t)c*n;
  int* out = sel + (size_t)c*n;
  int cnt[MCP_LEVELS], off[MCP_LEVELS + 1];
  off[0] = 0;
#pragma unroll
  for (int l = 0; l < MCP_LEVELS; ++l) { cnt[l] = counts[c*MCP_LEVELS + l]; off[l + 1] = off[l] + cnt[l]; }
  const int tot = off[MCP_LEVELS];
  if (t < MCP_LEVELS) S.n_live[t] = 0;
  if (t == 0) S.stale = 0;
  if (c == 0 && t == 0) ctl->coarse_found = 0;                 // (k_tm_search adds to it next)
  __syncthreads();
  for (int i = t; i < tot; i += TM_SEL_NT) {
    const int row = E[i].point;
    const TmSrc& R = src[row];
    const bool ok = R.slot1 > 0 && slots[R.slot1 - 1].live;
    live[i] = ok ? 1 : 0;
    K0[i] = tm_key(P.seed, 0, c, row); K1[i] = tm_key(P.seed, 1, c, row);
    if (ok) { int l = 0; while (i >= off[l + 1]) ++l; atomicAdd(&S.n_live[l], 1); } else atomicAdd(&S.stale, 1);
  }
  __syncthreads();
  const int n3 = S.n_live[3], n2 = S.n_live[2], n1 = S.n_live[1], n0 = S.n_live[0];
  const int cmax = P.try_coarse ? P.coarse_max : 0;
  const int k3 = min(n3, cmax), k2 = min(n2, cmax - k3);
  unsigned long long thr3 = 0ull, thr2 = 0ull;
  TmCand cd{0, 0, off[2], off[3], false, 0ull, false, 0ull};
  int w = 0;
  if (k3 > 0) { cd.a = off[3]; cd.b = off[4]; thr3 = tm_emit(cd, k3, K0, K0, live, E, out + w, S); w += k3; }
  if (k2 > 0) { cd.a = off[2]; cd.b = off[3]; thr2 = tm_emit(cd, k2, K0, K0, live, E, out + w, S); w += k2; }
  const int nC = w, nT = n3 - k3;
  if (nT > 0) { cd.a = off[3]; cd.b = off[4]; cd.has_lo = k3 > 0; cd.lo = thr3; tm_emit(cd, nT, K0, K0, live, E, out + w, S); w += nT; }
  const int K = max(0, P.max_patches - nC - nT), r0 = (n2 - k2) + n1 + n0;
  int nR = 0;
  if (r0 <= K) {                                                   // no chop: the rest of S_2, then S_1, then S_0, each in stage-0 order
    if (n2 - k2 > 0) { cd.a = off[2]; cd.b = off[3]; cd.has_lo = k2 > 0; cd.lo = thr2; tm_emit(cd, n2 - k2, K0, K0, live, E, out + w, S); w += n2 - k2; }
    cd.has_lo = false;
    if (n1 > 0) { cd.a = off[1]; cd.b = off[2]; tm_emit(cd, n1, K0, K0, live, E, out + w, S); w += n1; }
    if (n0 > 0) { cd.a = off[0]; cd.b = off[1]; tm_emit(cd, n0, K0, K0, live, E, out + w, S); w += n0; }
    nR = r0;
  } else if (K > 0) {                                              // the chop: the K smallest stage-1 keys of R0
    cd.a = off[0]; cd.b = off[3]; cd.excl = k2 > 0; cd.thr2 = thr2; cd.has_lo = false;
    tm_emit(cd, K, K0, K1, live, E, out + w, S); nR = K;
  }
  if (t == 0) { ctl->sizes[c][0] = nC; ctl->sizes[c][1] = nT; ctl->sizes[c][2] = nR; ctl->stale[c] = S.stale; }
}

// camera of item i of a camera-major list whose per-camera lengths are len(c); *j = index inside the camera
template <class F>
__device__ __forceinline__ int tm_locate(int ncam, int i, F len, int* j, int* first) {
  int f = 0;
  for (int c = 0; c < ncam; ++c) { const int m = len(c); if (i < f + m) { *j = i - f; *first = f; return c; } f += m; }
  *j = 0; *first = f; return -1;
}
__device__ __forceinline__ int tm_fine_first(const TmCtl& C, int c) { int f = 0; for (int q = 0; q < c; ++q) f += C.sizes[q][0] + C.sizes[q][1] + C.sizes[q][2]; return f; }

// One search stage.  fine = 0: the C items (one per coarse record, camera-major); fine = 1: every item [C_c, T_c, R_c] of every camera --
// C items copy their record from the coarse stage (as its iterations left it), T / R items are searched.  One wavefront per item.
__global__ void __launch_bounds__(64)
k_tm_search(TmParams P, int fine, const TmCam* __restrict__ cams, const double* __restrict__ pose, const PvsPoint* __restrict__ pts, const TmSrc* __restrict__ src,
            const TmSlot* __restrict__ slots, const int* __restrict__ sel, TmStates states, TmCtl* __restrict__ ctl, mcp_track_map_item* __restrict__ items,
            mcp_pose_point* __restrict__ coarse_recs, mcp_pose_point* __restrict__ fine_recs, double* __restrict__ weights) {
  __shared__ uint8_t tmpl[64], jtmpl[64];
  __shared__ double dprod[3][36];
  const int lane = threadIdx.x, ncam = P.ncam;
  const TmCtl& C = *ctl;
  int total = 0;
  for (int c = 0; c < ncam; ++c) total += fine ? C.sizes[c][0] + C.sizes[c][1] + C.sizes[c][2] : C.sizes[c][0];
  Se3 bfw;
#pragma unroll
  for (int k = 0; k < 9; ++k) bfw.R[k] = pose[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) bfw.t[k] = pose[9 + k];
  int coarse_found = 0;
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    int j, first;
    const int c = fine ? tm_locate(ncam, i, [&](int q) { return C.sizes[q][0] + C.sizes[q][1] + C.sizes[q][2]; }, &j, &first)
                       : tm_locate(ncam, i, [&](int q) { return C.sizes[q][0]; }, &j, &first);
    const int row = sel[(size_t)c*P.rows + j];
    const int stage = j < C.sizes[c][0] ? 0 : (j < C.sizes[c][0] + C.sizes[c][1] ? 1 : 2);
    const int slot = fine ? i : tm_fine_first(C, c) + j;             // the item's place: camera-major [C_c, T_c, R_c]
    mcp_track_map_item& It = items[slot];
    if (fine && stage == 0) {                                        // a coarse record: as the coarse stage left it
      int cf = 0; for (int q = 0; q < c; ++q) cf += C.sizes[q][0];
      if (lane == 0) { fine_recs[i] = coarse_recs[cf + j]; weights[i] = 0.0; }
      continue;
    }
    const PvsPoint& Pt = pts[row];
    const TmSrc& R = src[row];
    const TmSlot& Sl = slots[R.slot1 - 1];                           // (every selected row has a live source)
    DevTdIn D;
#pragma unroll
    for (int k = 0; k < 3; ++k) { D.world_pos[k] = Pt.world_pos[k]; D.pixel_right_w[k] = Pt.pixel_right_w[k]; D.pixel_down_w[k] = Pt.pixel_down_w[k]; }
    D.src_img = Sl.img[R.level]; D.src_w = Sl.w[R.level]; D.src_h = Sl.h[R.level]; D.center_x = R.cx; D.center_y = R.cy; D.fixed = R.fixed;
    mcp_pf_state& G = states.s[c][row];
    PfRegs S; S.valid = G.valid; S.key = G.point_key; S.bad = G.template_bad; S.jvalid = G.jacs_valid; S.mean = G.mean_diff;
    S.lw[0] = G.last_warp[0]; S.lw[1] = G.last_warp[1]; S.lw[2] = G.last_warp[2]; S.lw[3] = G.last_warp[3];
    tmpl[lane] = G.templ[lane]; jtmpl[lane] = G.jac_templ[lane];
    __syncthreads();
    const TmCam& T = cams[c];
    const int range = fine ? C.fine_range : P.coarse_range, its = fine ? (stage == 1 ? 8 : 0) : P.coarse_subpix_its;
    mcp_pose_point* PP = fine ? fine_recs + i : coarse_recs + i;
    patch_item(PF_TRACK, T.T, T.mask0, T.cam, bfw, T.cfb, D, R.key, 0.0, 0.0, S, tmpl, jtmpl, It.out, range, its, 0, dprod, lane, nullptr, PP, c);
    __syncthreads();
    G.templ[lane] = tmpl[lane]; G.jac_templ[lane] = jtmpl[lane];
    if (lane == 0) {
      G.valid = S.valid; G.point_key = S.key; G.template_bad = S.bad; G.jacs_valid = S.jvalid; G.mean_diff = S.mean;
      G.last_warp[0] = S.lw[0]; G.last_warp[1] = S.lw[1]; G.last_warp[2] = S.lw[2]; G.last_warp[3] = S.lw[3];
      It.point = row; It.stage = stage; It.weight_last = 0.0;
      if (fine) weights[i] = 0.0;
      if (!fine && PP->found && !S.bad) ++coarse_found;
    }
    __syncthreads();
  }
  if (!fine && lane == 0 && coarse_found) atomicAdd(&ctl->coarse_found, coarse_found);      // (integers: any order gives the same sum)
}

// the coarse gate (Tracker.cc:1012) and the record counts the pose iterations read
__global__ void k_tm_gate(TmParams P, TmCtl* __restrict__ ctl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  TmCtl& C = *ctl;
  int nc = 0, nf = 0;
  for (int c = 0; c < P.ncam; ++c) { nc += C.sizes[c][0]; nf += C.sizes[c][0] + C.sizes[c][1] + C.sizes[c][2]; }
  C.n_coarse = nc; C.n_fine = nf;
  C.did_coarse = C.coarse_found > P.coarse_min ? 1 : 0;
  C.fine_range = C.did_coarse ? 5 : 10;                            // SetupFineTracking :851-853
}

// the result block (pinned), by threads 0 .. 63 of one workgroup
__device__ __forceinline__ void tm_write_out(const TmParams& P, const TmCtl* __restrict__ ctl, const double* __restrict__ pose_mu, const int* __restrict__ counts,
                                             TmOut* __restrict__ res, int t) {
  if (t < 18) { if (t < 12) res->pose[t] = pose_mu[t]; else res->mu[t - 12] = pose_mu[t]; }
  if (t < P.ncam*MCP_LEVELS) (&res->counts[0][0])[t] = counts[t];
  if (t == 0) res->ctl = *ctl;
}

// the items, with the weights of the last fine iteration, and the result block to pinned host memory.  The search kernels write the items
// to device memory; they cross as 8-byte words, a wavefront's 64 consecutive words at a time.
__global__ void __launch_bounds__(256)
k_tm_finish(TmParams P, const TmCtl* __restrict__ ctl, const double* __restrict__ weights, const mcp_track_map_item* __restrict__ items, mcp_track_map_item* __restrict__ host_items,
            const double* __restrict__ pose_mu, const int* __restrict__ counts, TmOut* __restrict__ res) {
  static_assert(sizeof(mcp_track_map_item) % 8 == 0 && offsetof(mcp_track_map_item, weight_last) == 8, "the items are copied as 8-byte words");
  constexpr int W = (int)(sizeof(mcp_track_map_item)/8);
  // (mcp_td_out ends in 4 bytes of padding that patch_item never writes: zeroed, so that the items are the same bytes on every run)
  constexpr int PAD = (int)(sizeof(mcp_track_map_item) - (offsetof(mcp_track_map_item, out) + offsetof(mcp_td_out, templ) + 64));
  static_assert(PAD >= 0 && PAD < 8, "the padding lies in the last word");
  const unsigned long long last_mask = PAD ? (~0ull >> (8*PAD)) : ~0ull;
  const long long nw = (long long)ctl->n_fine*W;
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(items);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(host_items);
  for (long long g = blockIdx.x*256ll + threadIdx.x; g < nw; g += gridDim.x*256ll) {
    const long long i = g/W; const int q = (int)(g - i*W);
    dst[g] = q == 1 ? (unsigned long long)__double_as_longlong(weights[i]) : (q == W - 1 ? src[g] & last_mask : src[g]);
  }
  if (blockIdx.x == 0) tm_write_out(P, ctl, pose_mu, counts, res, threadIdx.x);
}

// mcp_map_points_set_source / _update_source: rows (ids[k], or first + k) <- recs[k]; a row whose key changes gets zeroed finders
__global__ void __launch_bounds__(256)
k_tm_source_scatter(TmSrc* __restrict__ rows, int count, int first, const int* __restrict__ ids, const TmSrc* __restrict__ recs, TmStates states, int ncam_states) {
  const int k = blockIdx.x*256 + threadIdx.x;
  if (k >= count) return;
  const int row = ids ? ids[k] : first + k;
  const TmSrc r = recs[k];
  if (rows[row].key != r.key)
    for (int c = 0; c < ncam_states; ++c) {
      unsigned long long* s = reinterpret_cast<unsigned long long*>(states.s[c] + row);
      for (int q = 0; q < (int)(sizeof(mcp_pf_state)/8); ++q) s[q] = 0ull;
    }
  rows[row] = r;
}

}  // namespace mcp
