// map_graph_kernels.h -- the device-resident map graph (MKF slots, rig, per-point graph columns, measurement store) and the selection of
// BundleAdjusterBase::BundleAdjustRecent / BundleAdjustAll over it (src/BundleAdjusterBase.cc:141-265, src/BundleAdjusterMulti.cc:81-200,
// src/KeyFrame.cc:715-747 and 903-927), gfx950.
//
// The arithmetic (keyframe distance, the selection predicate, the source rule, the point coordinates) lives in __host__ __device__ bodies that
// the kernels and mcp_map_bundle_select_host both call; this translation unit is built without fused multiply-add contraction, so the two give
// the same bits.  Every count is an integer, every atomic adds or ors an integer (LDS or global); the compactions rank by index (per-workgroup
// counts, then a scatter that sums the counts before its own and ranks by ballot), so the views do not depend on the order workgroups are
// dispatched in and no workgroup waits for another.
//
// One select is six launches on the table's stream (behind one memset of the marks):
//   k_mg_closest     one workgroup: the size gate, MultiKeyFrame::Distance to the newest MKF, the n_recent smallest, the adjust set
//   k_mg_edges_count store pass: good count per row, seen-from-adjust mark per row
//   k_mg_rows_mark   row pass: selection predicate + source rule, per-workgroup counts, source MKFs marked
//   k_mg_rank_mark   row blocks: bundle index of each row; store blocks: MKFs with a live entry on a bundle row marked, per-workgroup counts
//   k_mg_mkfs        one workgroup: the points gate, slots to bundle MKFs (adjust set then fixed set, ascending slot), the result struct
//   k_mg_emit        row blocks: the points view; store blocks: the measurement view
// The boundaries are the grid-wide marks: the good counts and seen marks must be complete before a row is judged, the row verdicts before an
// edge is kept or an MKF marked, the MKF marks before the slots are ranked, the bundle indices of rows and MKFs before a view names them.
#pragma once
#include <cfloat>
#include "ba_device.h"
#include "stereo_kernels.h"
#include "map_graph_dist.h"      // se3_inverse, MgRig, the keyframe distances

namespace mcp {

constexpr int MG_BLOCK = 256;
constexpr int MG_MAX_MKFS = MCP_MAP_MAX_MKFS;

struct MgMkf { double bfw[12]; double depth[MCP_MAX_FRAME_CAMS]; int flags; uint8_t active[MCP_MAX_FRAME_CAMS]; int pad_; };      // one slot (176 B)
struct MgPoint { int src_mkf, src_cam, flags, pending; };      // one row (16 B); pending: the device turned the row bad and no sweep has reported it yet (map_graph_cull.h)
struct MgMeas { double uv[2]; int mkf, cam, row, level, source, alive; };                                                         // one store entry (40 B)

// what the launches of one select hand to each other
struct MgCtl {
  int status, n_present, n_dropped, has_fixed_points, n_points;
  int closest[8]; double closest_dist[8];
  int erased;                      // mcp_map_graph_erase_meas / _erase_mkf: entries that died
};

__host__ __device__ inline bool mg_mkf_ok(int flags) { return (flags & MCP_MKF_PRESENT) && !(flags & MCP_MKF_BAD); }
// (MgRig, mg_se3_of12, mg_kf_distance, mg_mkf_distance: map_graph_dist.h)

// BundleAdjusterBase.cc:170-176 (ALL) and :231-237 (RECENT): is the row taken (before the source rule)
__host__ __device__ inline bool mg_row_selected(int mode, int pflags, int good, int seen) {
  if (pflags & MCP_GP_BAD) return false;
  if (mode == MCP_BUNDLE_ALL) return good >= 2 || (pflags & MCP_GP_FIXED);
  return seen && good >= 2;
}
// the source rule: a selected non-fixed row needs a source MKF that is a slot (and then present and not bad: mg_mkf_ok) and a camera of the rig
__host__ __device__ inline bool mg_source_in_range(const MgPoint& P, int ncam, int n_slots) {
  return P.src_mkf >= 0 && P.src_mkf < n_slots && P.src_cam >= 0 && P.src_cam < ncam;
}
// BundleAdjusterMulti.cc:145-158: world position for a fixed point, CamFromWorld_src * world otherwise (the two products in that order)
__host__ __device__ inline void mg_point_x(const MgRig& rig, const MgPoint& P, const double* src_bfw, const double* world, double* x) {
  if (P.flags & MCP_GP_FIXED) { x[0] = world[0]; x[1] = world[1]; x[2] = world[2]; return; }
  Se3 B, cfw;
  mg_se3_of12(src_bfw, B);
  se3_compose(rig.cfb[P.src_cam], B, cfw);
  se3_apply(cfw, world, x);
}
// does a store entry count at all: alive, its row in the table, its MKF a slot
__host__ __device__ inline bool mg_edge_live(int alive, int mkf, int row, int n_rows) { return alive && row >= 0 && row < n_rows && mkf >= 0 && mkf < MG_MAX_MKFS; }
__host__ __device__ inline unsigned long long mg_key(int mkf, int cam, int row) {
  return ((unsigned long long)(unsigned)(mkf*MCP_MAX_FRAME_CAMS + cam) << 32) | (unsigned)row;
}

#if defined(__HIPCC__)
// ---- uploads ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_mkfs_scatter(MgMkf* __restrict__ slots, int count, const int* __restrict__ ids, const MgMkf* __restrict__ recs) {
  const int k = blockIdx.x*MG_BLOCK + threadIdx.x;
  if (k < count) slots[ids[k]] = recs[k];
}
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_points_scatter(MgPoint* __restrict__ rows, int count, const int* __restrict__ ids, const MgPoint* __restrict__ recs) {
  const int k = blockIdx.x*MG_BLOCK + threadIdx.x;
  if (k < count) rows[ids[k]] = recs[k];
}
// rows first .. first+count-1 of the point columns read as rows never written do: bad, without a source
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_points_fill(MgPoint* __restrict__ rows, int first, int count) {
  const int k = blockIdx.x*MG_BLOCK + threadIdx.x;
  if (k < count) { MgPoint P; P.src_mkf = -1; P.src_cam = 0; P.flags = MCP_GP_BAD; P.pending = 0; rows[first + k] = P; }
}

// ---- erase and compact -----------------------------------------------------------------------------------------------------------------
// one thread per entry: a live entry whose key is among the sorted keys (binary search) -- or, keys == NULL, whose MKF is `slot` -- dies.
// slot_from: NULL, or where an earlier launch left the slot (mcp_map_mkf_cull; < 0: there is none and nothing dies)
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_erase(MgMeas* __restrict__ store, int n, const unsigned long long* __restrict__ keys, int n_keys, int slot, MgMkf* __restrict__ slots, MgCtl* __restrict__ ctl,
           const int* __restrict__ slot_from) {
  if (slot_from) { slot = *slot_from; if (slot < 0) return; }      // (uniform over the grid)
  const int i = blockIdx.x*MG_BLOCK + threadIdx.x;
  bool dies = false;
  if (i < n && store[i].alive) {
    if (!keys) dies = store[i].mkf == slot;
    else {
      const unsigned long long k = mg_key(store[i].mkf, store[i].cam, store[i].row);
      int lo = 0, hi = n_keys;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < k) lo = mid + 1; else hi = mid; }
      dies = lo < n_keys && keys[lo] == k;
    }
    if (dies) store[i].alive = 0;
  }
  const unsigned long long m = __ballot(dies);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl->erased, __popcll(m));
  if (!keys && i == 0) slots[slot].flags &= ~MCP_MKF_PRESENT;
}
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_compact_mark(const MgMeas* __restrict__ store, int n, int* __restrict__ blk_cnt) {
  __shared__ int cnt;
  const int i = blockIdx.x*MG_BLOCK + threadIdx.x;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const unsigned long long m = __ballot(i < n && store[i].alive);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt, __popcll(m));
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt;
}
// where this workgroup's kept items go: the counts of the workgroups before it (*total: of all of them), then wave by wave, lane by lane
__device__ __forceinline__ int mg_rank(bool keep, const int* __restrict__ blk_cnt, int nblk, int b, int* total) {
  constexpr int NW = MG_BLOCK/64;
  __shared__ int before, all, wcnt[NW];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  __syncthreads();                                     // (a second call in one kernel may still be reading these)
  if (t == 0) { before = 0; all = 0; }
  __syncthreads();
  int mb = 0, mt = 0;
  for (int j = t; j < nblk; j += MG_BLOCK) { const int v = blk_cnt[j]; mt += v; if (j < b) mb += v; }
  if (mt) atomicAdd(&all, mt);
  if (mb) atomicAdd(&before, mb);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  int off = before;
  for (int w = 0; w < wave; ++w) off += wcnt[w];
  if (total) *total = all;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_compact_scatter(const MgMeas* __restrict__ store, int n, int nblk, const int* __restrict__ blk_cnt, MgMeas* __restrict__ out, int cap) {
  const int i = blockIdx.x*MG_BLOCK + threadIdx.x;
  const bool keep = i < n && store[i].alive;
  const int at = mg_rank(keep, blk_cnt, nblk, blockIdx.x, nullptr);
  if (keep && at < cap) out[at] = store[i];
}

// ---- good counts (also mcp_map_graph_good_counts: ctl == NULL, seen == NULL) ------------------------------------------------------------
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_edges_count(const MgCtl* __restrict__ ctl, const MgMeas* __restrict__ store, int n_store, int n_rows, const MgMkf* __restrict__ slots,
                 const uint8_t* __restrict__ adjust, int* __restrict__ good, int* __restrict__ seen) {
  if (ctl && ctl->status != 0) return;                 // (uniform over the grid)
  const int i = blockIdx.x*MG_BLOCK + threadIdx.x;
  if (i >= n_store) return;
  const MgMeas E = store[i];
  if (!mg_edge_live(E.alive, E.mkf, E.row, n_rows)) return;
  if (mg_mkf_ok(slots[E.mkf].flags)) atomicAdd(&good[E.row], 1);
  if (seen && adjust[E.mkf]) atomicOr(&seen[E.row], 1);
}

// ---- the select ------------------------------------------------------------------------------------------------------------------------
struct MgSelect { int mode, newest, n_recent, recent_min_size, min_points; double frac; };

// one workgroup: the size gate, the distances to the newest MKF, the n_recent smallest by (distance, slot), the adjust set
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_closest(MgSelect S, MgRig rig, const MgMkf* __restrict__ slots, uint8_t* __restrict__ adjust /* MG_MAX_MKFS */, MgCtl* __restrict__ ctl) {
  __shared__ double dist[MG_MAX_MKFS];
  __shared__ uint8_t cand[MG_MAX_MKFS];                // 1: another present MKF not yet taken
  __shared__ double wd[MG_BLOCK]; __shared__ int ws[MG_BLOCK];
  __shared__ int n_present, broken;
  const int t = threadIdx.x;
  if (t == 0) { n_present = 0; broken = 0; }
  __syncthreads();
  int mine = 0;
  for (int k = t; k < MG_MAX_MKFS; k += MG_BLOCK) {
    const int f = slots[k].flags;
    cand[k] = 0; dist[k] = 0.0;
    if (f & MCP_MKF_PRESENT) ++mine;
    adjust[k] = (S.mode == MCP_BUNDLE_ALL && mg_mkf_ok(f)) ? 1 : 0;
  }
  if (mine) atomicAdd(&n_present, mine);
  __syncthreads();
  if (t < 8) { ctl->closest[t] = -1; ctl->closest_dist[t] = 0.0; }
  if (t == 0) { ctl->n_present = n_present; ctl->n_dropped = 0; ctl->has_fixed_points = 0; ctl->n_points = 0; ctl->status = 0; }
  if (S.mode == MCP_BUNDLE_ALL) return;
  if (n_present < S.recent_min_size) { if (t == 0) ctl->status = 1; return; }      // BundleAdjusterBase.cc:196-201
  const MgMkf& N = slots[S.newest];
  for (int k = t; k < MG_MAX_MKFS; k += MG_BLOCK) {
    if (k == S.newest || !(slots[k].flags & MCP_MKF_PRESENT)) continue;
    bool br;
    dist[k] = mg_mkf_distance(rig, N.bfw, N.active, N.depth, slots[k].bfw, slots[k].active, slots[k].depth, S.frac, &br);
    cand[k] = 1;
    if (br) atomicOr(&broken, 1);
  }
  __syncthreads();
  if (broken) { if (t == 0) ctl->status = 3; return; }                              // KeyFrame.cc:734-744
  if (t == 0) adjust[S.newest] = 1;
  for (int r = 0; r < S.n_recent; ++r) {
    double bd = 0.0; int bs = -1;
    for (int k = t; k < MG_MAX_MKFS; k += MG_BLOCK) if (cand[k] && (bs < 0 || dist[k] < bd)) { bd = dist[k]; bs = k; }      // (ascending k: ties keep the smaller slot)
    wd[t] = bd; ws[t] = bs;
    __syncthreads();
    for (int h = MG_BLOCK/2; h > 0; h >>= 1) {
      if (t < h) {
        const int o = ws[t + h];
        if (o >= 0 && (ws[t] < 0 || wd[t + h] < wd[t] || (wd[t + h] == wd[t] && o < ws[t]))) { wd[t] = wd[t + h]; ws[t] = o; }
      }
      __syncthreads();
    }
    const int win = ws[0];
    if (win < 0) break;                                // fewer than n_recent other MKFs: a shorter list (uniform)
    if (t == 0) {
      ctl->closest[r] = win; ctl->closest_dist[r] = wd[0];
      cand[win] = 0;
      const int f = slots[win].flags;
      if (!(f & MCP_MKF_BAD) && !(f & MCP_MKF_FIXED)) adjust[win] = 1;              // :208-215
    }
    __syncthreads();
  }
}

// row pass: verdict per row (1: in the bundle), the rows the source rule drops, the source MKFs of the kept rows, per-workgroup counts
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_rows_mark(MgSelect S, int ncam, MgCtl* __restrict__ ctl, const MgMkf* __restrict__ slots, const MgPoint* __restrict__ pts, int n_rows,
               const int* __restrict__ good, const int* __restrict__ seen, uint8_t* __restrict__ sel, int* __restrict__ mkf_in, int* __restrict__ blk_cnt) {
  __shared__ int cnt, dropped, fixedp;
  if (ctl->status != 0) return;
  const int i = blockIdx.x*MG_BLOCK + threadIdx.x;
  if (threadIdx.x == 0) { cnt = 0; dropped = 0; fixedp = 0; }
  __syncthreads();
  bool keep = false, drop = false, fixed = false;
  if (i < n_rows) {
    const MgPoint P = pts[i];
    if (mg_row_selected(S.mode, P.flags, good[i], seen[i])) {
      fixed = P.flags & MCP_GP_FIXED;
      const bool src_ok = fixed || (mg_source_in_range(P, ncam, MG_MAX_MKFS) && mg_mkf_ok(slots[P.src_mkf].flags));
      keep = src_ok; drop = !src_ok;
      if (keep && !fixed) atomicOr(&mkf_in[P.src_mkf], 1);
    }
    sel[i] = keep ? 1 : 0;
  }
  const unsigned long long mk = __ballot(keep), md = __ballot(drop), mf = __ballot(keep && fixed);
  if ((threadIdx.x & 63) == 0) { if (mk) atomicAdd(&cnt, __popcll(mk)); if (md) atomicAdd(&dropped, __popcll(md)); if (mf) atomicOr(&fixedp, 1); }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_cnt[blockIdx.x] = cnt;
    if (dropped) atomicAdd(&ctl->n_dropped, dropped);
    if (fixedp) atomicOr(&ctl->has_fixed_points, 1);
  }
}

// row blocks [0, nblk_rows): the bundle index of each row (-1: not in the bundle); store blocks after them: the MKFs with a live entry on a
// bundle row, and the per-workgroup counts of the measurements kept
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_rank_mark(const MgCtl* __restrict__ ctl, int n_rows, int nblk_rows, const uint8_t* __restrict__ sel, const int* __restrict__ blk_rows, int* __restrict__ bidx,
               const MgMeas* __restrict__ store, int n_store, const MgMkf* __restrict__ slots, int* __restrict__ mkf_in, uint8_t* __restrict__ mkeep, int* __restrict__ blk_meas) {
  if (ctl->status != 0) return;
  if ((int)blockIdx.x < nblk_rows) {
    const int i = blockIdx.x*MG_BLOCK + threadIdx.x;
    const bool keep = i < n_rows && sel[i];
    const int at = mg_rank(keep, blk_rows, nblk_rows, blockIdx.x, nullptr);
    if (i < n_rows) bidx[i] = keep ? at : -1;
    return;
  }
  __shared__ int cnt;
  const int b = blockIdx.x - nblk_rows, i = b*MG_BLOCK + threadIdx.x;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  bool keep = false;
  if (i < n_store) {
    const MgMeas E = store[i];
    keep = mg_edge_live(E.alive, E.mkf, E.row, n_rows) && sel[E.row] && mg_mkf_ok(slots[E.mkf].flags);
    if (keep) atomicOr(&mkf_in[E.mkf], 1);
    mkeep[i] = keep ? 1 : 0;
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt, __popcll(m));
  __syncthreads();
  if (threadIdx.x == 0) blk_meas[b] = cnt;
}

// one workgroup: the points gate, the slots ranked (adjust set, then fixed set, ascending slot), the MKF view and the result
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_mkfs(MgSelect S, MgCtl* __restrict__ ctl, const MgMkf* __restrict__ slots, const uint8_t* __restrict__ adjust, const int* __restrict__ mkf_in,
          const int* __restrict__ blk_rows, int nblk_rows, const int* __restrict__ blk_meas, int nblk_meas, int* __restrict__ mkf_bidx /* MG_MAX_MKFS */,
          mcp_bundle_mkf* __restrict__ out_mkfs /* pinned */, mcp_bundle_select_result* __restrict__ res /* pinned */) {
  constexpr int PER = MG_MAX_MKFS/MG_BLOCK;            // consecutive slots per thread
  __shared__ int n_points, n_meas, sa[MG_BLOCK], sf[MG_BLOCK];
  const int t = threadIdx.x;
  if (t == 0) { n_points = 0; n_meas = 0; }
  __syncthreads();
  int status = ctl->status;
  if (status == 0) {
    int p = 0, m = 0;
    for (int j = t; j < nblk_rows; j += MG_BLOCK) p += blk_rows[j];
    for (int j = t; j < nblk_meas; j += MG_BLOCK) m += blk_meas[j];
    if (p) atomicAdd(&n_points, p);
    if (m) atomicAdd(&n_meas, m);
  }
  __syncthreads();
  if (status == 0 && n_points < S.min_points) status = 2;
  // class of each of this thread's slots: 1 adjust, 2 fixed set, 0 neither
  int cls[PER], na = 0, nf = 0;
  for (int q = 0; q < PER; ++q) {
    const int k = t*PER + q;
    cls[q] = 0;
    if (status == 0) {
      if (adjust[k]) cls[q] = 1;
      else if (mkf_in[k] && mg_mkf_ok(slots[k].flags)) cls[q] = 2;
    }
    na += cls[q] == 1; nf += cls[q] == 2;
  }
  sa[t] = na; sf[t] = nf;
  __syncthreads();
  int ba = 0, bf = 0, ta = 0, tf = 0;
  for (int j = 0; j < MG_BLOCK; ++j) { if (j < t) { ba += sa[j]; bf += sf[j]; } ta += sa[j]; tf += sf[j]; }
  for (int q = 0; q < PER; ++q) {
    const int k = t*PER + q;
    int at = -1;
    if (cls[q] == 1) at = ba++;
    else if (cls[q] == 2) at = ta + bf++;
    mkf_bidx[k] = at;
    if (at >= 0) { out_mkfs[at].slot = k; out_mkfs[at].fixed = cls[q] == 2 ? 1 : ((slots[k].flags & MCP_MKF_FIXED) ? 1 : 0); }
  }
  if (t == 0) {
    const bool ok = status == 0;
    res->status = status; res->n_adjust = ok ? ta : 0; res->n_fixed = ok ? tf : 0; res->n_points = ok ? n_points : 0; res->n_meas = ok ? n_meas : 0;
    res->has_fixed_points = ok ? ctl->has_fixed_points : 0;
    res->n_dropped_source = (status == 0 || status == 2) ? ctl->n_dropped : 0;
    ctl->status = status; ctl->n_points = n_points;
  }
  if (t < 8) { res->closest[t] = ctl->closest[t]; res->closest_dist[t] = ctl->closest_dist[t]; }
}

// row blocks: the points view; store blocks: the measurement view (both into the pinned block)
__global__ void __launch_bounds__(MG_BLOCK)
k_mg_emit(const MgCtl* __restrict__ ctl, MgRig rig, const MgMkf* __restrict__ slots, const int* __restrict__ mkf_bidx, const MgPoint* __restrict__ pts,
          const PvsPoint* __restrict__ table, int n_rows, int nblk_rows, const int* __restrict__ bidx, const MgMeas* __restrict__ store, int n_store,
          const uint8_t* __restrict__ mkeep, const int* __restrict__ blk_meas, int nblk_meas, mcp_bundle_point* __restrict__ out_points, int cap_points,
          mcp_bundle_meas* __restrict__ out_meas, int cap_meas) {
  if (ctl->status != 0) return;
  if ((int)blockIdx.x < nblk_rows) {
    const int i = blockIdx.x*MG_BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const int at = bidx[i];
    if (at < 0 || at >= cap_points) return;
    const MgPoint P = pts[i];
    const bool fixed = P.flags & MCP_GP_FIXED;
    mcp_bundle_point O;
    mg_point_x(rig, P, slots[fixed ? 0 : P.src_mkf].bfw, table[i].world_pos, O.x);
    O.row = i; O.src_mkf = fixed ? -1 : mkf_bidx[P.src_mkf]; O.src_cam = fixed ? -1 : P.src_cam; O.fixed = fixed ? 1 : 0;
    out_points[at] = O;
    return;
  }
  const int b = blockIdx.x - nblk_rows, i = b*MG_BLOCK + threadIdx.x;
  const bool keep = i < n_store && mkeep[i];
  const int at = mg_rank(keep, blk_meas, nblk_meas, b, nullptr);
  if (!keep || at >= cap_meas) return;
  const MgMeas E = store[i];
  mcp_bundle_meas O;
  O.uv[0] = E.uv[0]; O.uv[1] = E.uv[1]; O.mkf = mkf_bidx[E.mkf]; O.cam = E.cam; O.point = bidx[E.row]; O.level = E.level; O.source = E.source; O.store = i;
  out_meas[at] = O;
}
#endif  // __HIPCC__

}  // namespace mcp
