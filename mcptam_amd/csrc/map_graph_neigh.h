// map_graph_neigh.h -- the closest-keyframe queries and the removal of an MKF on the device (include/mcp_img.h mcp_map_neighbours,
// mcp_map_mkf_cull): MapMakerBase::ClosestKeyFrame .. FurthestMultiKeyFrame (src/MapMakerBase.cc:90-339), MarkFurthestMultiKeyFrameAsBad
// (src/MapMakerServerBase.cc:264-318) and the MKF half of HandleBadEntities (src/Map.cc:119-187) over the map graph's own columns, gfx950.
//
// The conventions are map_graph_kernels.h's: every count is an integer, every atomic adds or ors an integer (LDS or global), nothing depends
// on the order workgroups are dispatched in, no workgroup waits for another, 256-thread workgroups.  The candidate rule, the distance, the
// order and the point rule are host / device bodies that the host twins (map_graph_neigh_host.cpp) call too; both units are built without
// fused multiply-add contraction, so the bytes are the same.  The kernels are left out where MGN_HOST_ONLY is defined.
//
// A candidate has the index (slot + 1) * W + cam, W = MCP_MAX_FRAME_CAMS in the keyframe kind (cam 0 and W = 1 in the MKF kind), so ascending
// index is ascending (slot, cam) with the external MKF's keyframes (slot -1) first.  The keyframe kind has up to (4096 + 1) * 8 candidates:
// 256 KB of distances, more than the 160 KB of LDS a workgroup has, so distances and candidate bytes live in a scratch the graph owns.
//
// mcp_map_neighbours is two or three launches on the table's stream:
//   k_mgn_dist    a grid over the indices, one candidate per thread: the candidate byte, the distance, the candidate count, the broken flag
//   k_mgn_select  one workgroup: at most n_max rounds of a strided arg-min / arg-max over the scratch with the LDS tree of k_mg_closest and
//                 its tie rule (the smaller index); the winner is marked taken and written to the result
//   k_mgn_count   (want_meas) one thread per store entry: a ballot per winner, lane 0 adds to at most 32 integer counters
// The boundaries: every distance and the broken flag before the selection reads them; the winners before an entry is counted.
// mcp_map_mkf_cull: [slot == -1: k_mgn_dist, k_mgn_select: the furthest MKF] k_mgn_dist, k_mgn_select (the nearest MKF to the victim, its
// source read from the device), k_mgn_decide (one thread: victim, status, MKF flags), [k_mgn_rows_count], k_mgn_mark, [k_mg_erase].
// Here the live counts of every row must be complete before a row is judged, and the marks before an entry dies.
#pragma once
#include <cstdint>
#include <cstddef>
#include <cmath>
#include <string>
#include "map_graph_dist.h"

namespace mcp {

struct MgnQuery { int kind, region, order, src_slot, src_cam, same_cam, n_max, want_meas; double max_dist, frac; };

__host__ __device__ inline int mgn_width(int kind) { return kind == MCP_NB_KF ? MCP_MAX_FRAME_CAMS : 1; }
// the indices of the slots below n_slots (and of the external MKF before them)
__host__ __device__ inline int mgn_indices(int kind, int n_slots) { return (n_slots + 1)*mgn_width(kind); }
__host__ __device__ inline void mgn_slot_cam(int kind, int idx, int* slot, int* cam) {
  if (kind == MCP_NB_KF) { *slot = idx/MCP_MAX_FRAME_CAMS - 1; *cam = idx % MCP_MAX_FRAME_CAMS; } else { *slot = idx - 1; *cam = 0; }
}

// is (slot, cam) a candidate.  flags / act: of that slot (slot -1: the external MKF's active bytes, flags ignored)
__host__ __device__ inline bool mgn_is_candidate(const MgnQuery& Q, int ncam, int slot, int cam, int flags, const uint8_t* act) {
  if (Q.kind == MCP_NB_MKF) return slot >= 0 && slot != Q.src_slot && (flags & MCP_MKF_PRESENT);
  if (cam >= ncam) return false;
  if (slot < 0) { if (Q.src_slot != -1) return false; }      // the external MKF's siblings: only of an external source
  else if (!(flags & MCP_MKF_PRESENT)) return false;
  if (!act[cam]) return false;
  const bool own = slot == Q.src_slot;
  if (own && cam == Q.src_cam) return false;
  if (Q.region == MCP_NB_ONLY_SELF && !own) return false;
  if (Q.region == MCP_NB_ONLY_OTHER && own) return false;
  if (Q.same_cam && cam != Q.src_cam) return false;
  return true;
}

// the distance from the source (s_*) to the candidate (c_*, camera cam)
__host__ __device__ inline double mgn_distance(const MgnQuery& Q, const MgRig& rig, const double* s_bfw, const uint8_t* s_act, const double* s_dep,
                                               const double* c_bfw, const uint8_t* c_act, const double* c_dep, int cam, bool* broken) {
  if (Q.kind == MCP_NB_MKF) return mg_mkf_distance(rig, s_bfw, s_act, s_dep, c_bfw, c_act, c_dep, Q.frac, broken);
  Se3 A, B, w1, w2;
  mg_se3_of12(s_bfw, A); mg_se3_of12(c_bfw, B);
  se3_compose(rig.cfb[Q.src_cam], A, w1); se3_compose(rig.cfb[cam], B, w2);
  return mg_kf_distance(w1, s_dep[Q.src_cam], w2, c_dep[cam], Q.frac, broken);
}

// may a candidate at distance d be chosen at all
__host__ __device__ inline bool mgn_eligible(const MgnQuery& Q, double d) { return d <= Q.max_dist && (Q.order == MCP_NB_NEAREST || d > 0.0); }
// is (d, i) chosen before (bd, bi); bi < 0: there is nothing yet
__host__ __device__ inline bool mgn_before(int order, double d, int i, double bd, int bi) {
  if (bi < 0) return true;
  if (order == MCP_NB_NEAREST ? d < bd : d > bd) return true;
  return d == bd && i < bi;
}

// the point rule of MarkFurthestMultiKeyFrameAsBad (:281-283) for a live entry of the victim under camera `cam`; live: the row's live entries
__host__ __device__ inline bool mgn_point_rule(int pflags, int src_mkf, int src_cam, int live, int max_kfs, int victim, int cam, bool* by_source) {
  *by_source = src_mkf == victim && src_cam == cam;
  return (!(pflags & MCP_GP_FIXED) && live <= max_kfs) || *by_source;
}

// the refusals that need no map (host): "" or what is wrong.  The source slot is the caller's to check (mgn_source_check)
inline std::string mgn_params_check(const mcp_neigh_params* p, int ncam) {
  if (!p) return "NULL params";
  if (p->kind != MCP_NB_MKF && p->kind != MCP_NB_KF) return "unknown kind " + std::to_string(p->kind);
  if (p->region != MCP_NB_ALL && p->region != MCP_NB_ONLY_SELF && p->region != MCP_NB_ONLY_OTHER) return "unknown region " + std::to_string(p->region);
  if (p->order != MCP_NB_NEAREST && p->order != MCP_NB_FURTHEST) return "unknown order " + std::to_string(p->order);
  if (p->src_slot < -1 || p->src_slot >= MCP_MAP_MAX_MKFS) return "the source (slot " + std::to_string(p->src_slot) + ") is neither -1 nor a present slot";
  if (p->kind == MCP_NB_KF && (p->src_cam < 0 || p->src_cam >= ncam)) return "src_cam " + std::to_string(p->src_cam) + " is outside the rig";
  if (p->kind == MCP_NB_KF && p->region == MCP_NB_ONLY_SELF && p->same_cam) return "MCP_NB_ONLY_SELF with same_cam names no keyframe";
  if (p->n_max < 1 || p->n_max > MCP_NB_MAX) return "n_max outside 1.." + std::to_string(MCP_NB_MAX);
  if (!(p->max_dist >= 0.0)) return "max_dist is NaN or negative";
  if (!std::isfinite(p->mean_diff_fraction)) return "mean_diff_fraction is not finite";
  if (p->src_slot == -1) {
    for (int k = 0; k < 12; ++k) if (!std::isfinite(p->ext_base_from_world[k])) return "the external MKF has a non-finite pose";
    for (int c = 0; c < ncam; ++c)
      if (p->ext_active[c] && !(std::isfinite(p->ext_depth_mean[c]) && p->ext_depth_mean[c] > 0.0))
        return "the external MKF, camera " + std::to_string(c) + ": the depth mean of an active keyframe must be finite and positive";
  }
  return "";
}
// flags / act: of the source slot (src_slot >= 0), or NULL act with src_slot == -1
inline std::string mgn_source_check(const mcp_neigh_params* p, int flags, const uint8_t* act) {
  if (p->src_slot >= 0 && !(flags & MCP_MKF_PRESENT)) return "the source (slot " + std::to_string(p->src_slot) + ") is neither -1 nor a present slot";
  if (p->kind == MCP_NB_KF && !(p->src_slot >= 0 ? act[p->src_cam] : p->ext_active[p->src_cam])) return "the source keyframe (camera " + std::to_string(p->src_cam) + ") is not active";
  return "";
}
inline MgnQuery mgn_query(const mcp_neigh_params& p) {
  MgnQuery Q;
  Q.kind = p.kind; Q.region = p.kind == MCP_NB_KF ? p.region : MCP_NB_ALL; Q.order = p.order; Q.src_slot = p.src_slot; Q.src_cam = p.kind == MCP_NB_KF ? p.src_cam : 0;
  Q.same_cam = p.kind == MCP_NB_KF && p.same_cam ? 1 : 0; Q.n_max = p.n_max; Q.want_meas = p.want_meas ? 1 : 0; Q.max_dist = p.max_dist; Q.frac = p.mean_diff_fraction;
  return Q;
}

#if defined(__HIPCC__) && !defined(MGN_HOST_ONLY)
constexpr int MGN_BLOCK = MG_BLOCK;

// what the launches of one query hand to each other (zeroed before the first)
struct MgnCtl { int broken, n_candidates, first_slot, pad_; };
// the removal of an MKF: what k_mgn_decide settles and the marks count (zeroed before the first launch)
struct MgnCull { int status, victim, dist_valid, new_fixed; double dist; int n_victim_meas, n_rows_marked, n_by_count, n_by_source; };

// n_idx: mgn_indices up to the last present slot.  src_from: NULL, or where an earlier launch left the source slot (< 0: there is none, and no candidate)
__global__ void __launch_bounds__(MGN_BLOCK)
k_mgn_dist(MgnQuery Q, int n_idx, MgRig rig, const MgMkf* __restrict__ slots, const MgMkf* __restrict__ ext, const int* __restrict__ src_from,
           double* __restrict__ dist, uint8_t* __restrict__ cand, MgnCtl* __restrict__ ctl) {
  const int idx = blockIdx.x*MGN_BLOCK + threadIdx.x;
  bool none = false;
  if (src_from) { Q.src_slot = *src_from; none = Q.src_slot < 0; }
  bool is = false, br = false;
  if (idx < n_idx) {
    double d = 0.0;
    if (!none) {
      int slot, cam;
      mgn_slot_cam(Q.kind, idx, &slot, &cam);
      const MgMkf* C = slot >= 0 ? slots + slot : ext;
      if (slot >= 0 || Q.src_slot < 0) is = mgn_is_candidate(Q, rig.ncam, slot, cam, C->flags, C->active);      // (ext is read only where it was uploaded)
      if (is) {
        const MgMkf* S = Q.src_slot >= 0 ? slots + Q.src_slot : ext;
        d = mgn_distance(Q, rig, S->bfw, S->active, S->depth, C->bfw, C->active, C->depth, cam, &br);
      }
    }
    dist[idx] = d; cand[idx] = is ? 1 : 0;
  }
  const unsigned long long m = __ballot(is), mb = __ballot(br);
  if ((threadIdx.x & 63) == 0) { if (m) atomicAdd(&ctl->n_candidates, __popcll(m)); if (mb) atomicOr(&ctl->broken, 1); }
}

// one workgroup: the n_max best by (distance, index) among the eligible candidates; a winner is marked taken (one bit per index, LDS)
__global__ void __launch_bounds__(MGN_BLOCK)
k_mgn_select(MgnQuery Q, int n_idx, const MgMkf* __restrict__ slots, const double* __restrict__ dist, const uint8_t* __restrict__ cand, MgnCtl* __restrict__ ctl,
             mcp_neigh_result* __restrict__ res /* device, zeroed */) {
  __shared__ double wd[MGN_BLOCK]; __shared__ int wi[MGN_BLOCK];
  __shared__ unsigned taken[((MCP_MAP_MAX_MKFS + 1)*MCP_MAX_FRAME_CAMS + 31)/32];
  const int t = threadIdx.x;
  if (ctl->broken) {                                   // KeyFrame.cc:734-744 (uniform)
    if (t == 0) { res->status = 3; res->count = 0; res->n_candidates = ctl->n_candidates; ctl->first_slot = -1; }
    return;
  }
  for (int k = t; k < (n_idx + 31)/32; k += MGN_BLOCK) taken[k] = 0u;
  __syncthreads();
  int count = 0;
  for (int r = 0; r < Q.n_max; ++r) {
    double bd = 0.0; int bi = -1;
    for (int k = t; k < n_idx; k += MGN_BLOCK) {
      if (!cand[k] || ((taken[k >> 5] >> (k & 31)) & 1u)) continue;
      const double d = dist[k];
      if (mgn_eligible(Q, d) && mgn_before(Q.order, d, k, bd, bi)) { bd = d; bi = k; }
    }
    wd[t] = bd; wi[t] = bi;
    __syncthreads();
    for (int h = MGN_BLOCK/2; h > 0; h >>= 1) {
      if (t < h) {
        const int o = wi[t + h];
        if (o >= 0 && mgn_before(Q.order, wd[t + h], o, wd[t], wi[t])) { wd[t] = wd[t + h]; wi[t] = o; }
      }
      __syncthreads();
    }
    const int win = wi[0];
    const double wdist = wd[0];
    __syncthreads();                                   // (wd, wi are rewritten by the next round)
    if (win < 0) break;                                // fewer eligible candidates than n_max: a shorter list (uniform)
    if (t == 0) {
      int slot, cam;
      mgn_slot_cam(Q.kind, win, &slot, &cam);
      mcp_neigh_item I;
      I.dist = wdist; I.slot = slot; I.cam = Q.kind == MCP_NB_KF ? cam : -1; I.flags = slot >= 0 ? slots[slot].flags : 0; I.n_meas = Q.want_meas ? 0 : -1;
      res->item[r] = I;
      taken[win >> 5] |= 1u << (win & 31);
      if (r == 0) ctl->first_slot = slot;
    }
    ++count;
    __syncthreads();                                   // (the taken mark, before the next round reads it)
  }
  if (t == 0) { res->status = 0; res->count = count; res->n_candidates = ctl->n_candidates; if (count == 0) ctl->first_slot = -1; }
}

// one thread per store entry: the alive entries of each winner
__global__ void __launch_bounds__(MGN_BLOCK)
k_mgn_count(int kind, const MgMeas* __restrict__ store, int n_store, mcp_neigh_result* __restrict__ res) {
  __shared__ int ws[MCP_NB_MAX], wc[MCP_NB_MAX];
  const int count = res->count;                        // (0 with status 3)
  if (threadIdx.x < MCP_NB_MAX && (int)threadIdx.x < count) { ws[threadIdx.x] = res->item[threadIdx.x].slot; wc[threadIdx.x] = res->item[threadIdx.x].cam; }
  __syncthreads();
  const int i = blockIdx.x*MGN_BLOCK + threadIdx.x;
  int mkf = -2, cam = -2;
  if (i < n_store && store[i].alive) { mkf = store[i].mkf; cam = store[i].cam; }
  if (!__ballot(mkf != -2)) return;                    // (per wavefront)
  for (int w = 0; w < count; ++w) {
    const unsigned long long m = __ballot(mkf == ws[w] && (kind == MCP_NB_MKF || cam == wc[w]));
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&res->item[w].n_meas, __popcll(m));
  }
}

struct MgnCullIn { int slot, mark_points, max_kfs, erase; };

// one thread: the victim, the status, the MKF flags.  far: the furthest query's result (NULL with a given slot); near: the hand-over's
__global__ void k_mgn_decide(MgnCullIn P, const mcp_neigh_result* __restrict__ far, const mcp_neigh_result* __restrict__ near, MgMkf* __restrict__ slots,
                             MgnCull* __restrict__ cc /* zeroed */) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int status = 0, victim = P.slot, new_fixed = -1;
  if (far) {
    if (far->status != 0) status = 3;
    else if (far->count == 0) status = 1;
    else { victim = far->item[0].slot; cc->dist = far->item[0].dist; cc->dist_valid = 1; }
  }
  if (status == 0 && (slots[victim].flags & MCP_MKF_FIXED)) {      // :313-317
    if (near->status != 0) status = 3;
    else if (near->count > 0) new_fixed = near->item[0].slot;
  }
  if (status != 0) { victim = -1; new_fixed = -1; cc->dist = 0.0; cc->dist_valid = 0; }
  else {
    slots[victim].flags |= MCP_MKF_BAD;
    if (new_fixed >= 0) slots[new_fixed].flags |= MCP_MKF_FIXED;
  }
  cc->status = status; cc->victim = victim; cc->new_fixed = new_fixed;
}

// store pass: the live entries of every row (spMeasurementKFs.size()), and the rows whose patch source is a keyframe of the victim that
// measures them
__global__ void __launch_bounds__(MGN_BLOCK)
k_mgn_rows_count(const MgnCull* __restrict__ cc, const MgMeas* __restrict__ store, int n_store, int n_rows, int n_prows, const MgPoint* __restrict__ pts,
                 int* __restrict__ live /* n_rows, zeroed */, int* __restrict__ by_src /* n_rows, zeroed */) {
  const int victim = cc->victim;
  if (victim < 0) return;                              // (uniform over the grid)
  const int i = blockIdx.x*MGN_BLOCK + threadIdx.x;
  if (i >= n_store) return;
  const MgMeas E = store[i];
  if (!mg_edge_live(E.alive, E.mkf, E.row, n_rows)) return;
  atomicAdd(&live[E.row], 1);
  if (E.mkf == victim && E.row < n_prows && pts[E.row].src_mkf == victim && pts[E.row].src_cam == E.cam) atomicOr(&by_src[E.row], 1);
}

// store pass: one thread per live entry of the victim applies the point rule; whoever turns the row bad counts it
__global__ void __launch_bounds__(MGN_BLOCK)
k_mgn_mark(MgnCullIn P, MgnCull* __restrict__ cc, const MgMeas* __restrict__ store, int n_store, int n_rows, int n_prows, MgPoint* __restrict__ pts,
           const int* __restrict__ live, const int* __restrict__ by_src) {
  __shared__ int cnt[4];                               // the victim's entries | rows marked | by count | by source
  const int victim = cc->victim;
  if (victim < 0) return;                              // (uniform over the grid)
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x*MGN_BLOCK + threadIdx.x;
  bool mine = false, marked = false, src = false;
  if (i < n_store) {
    const MgMeas E = store[i];
    mine = mg_edge_live(E.alive, E.mkf, E.row, n_rows) && E.mkf == victim;
    if (mine && P.mark_points && E.row < n_prows) {
      const MgPoint Q = pts[E.row];                    // (the bad bit may be changing under this read; the rule does not look at it)
      bool b;
      if (mgn_point_rule(Q.flags, Q.src_mkf, Q.src_cam, live[E.row], P.max_kfs, victim, E.cam, &b)) {
        const int old = atomicOr(&pts[E.row].flags, MCP_GP_BAD);
        if (!(old & MCP_GP_BAD)) { pts[E.row].pending = 1; marked = true; src = by_src[E.row] != 0; }
      }
    }
  }
  const unsigned long long mv = __ballot(mine), mm = __ballot(marked), ms = __ballot(marked && src);
  if ((threadIdx.x & 63) == 0) {
    if (mv) atomicAdd(&cnt[0], __popcll(mv));
    if (mm) { atomicAdd(&cnt[1], __popcll(mm)); atomicAdd(&cnt[2], __popcll(mm) - __popcll(ms)); }
    if (ms) atomicAdd(&cnt[3], __popcll(ms));
  }
  __syncthreads();
  if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&cc->n_victim_meas + threadIdx.x, cnt[threadIdx.x]);
}
static_assert(offsetof(MgnCull, n_by_source) == offsetof(MgnCull, n_victim_meas) + 3*sizeof(int), "k_mgn_mark adds its four counters as one array");
#endif  // __HIPCC__ && !MGN_HOST_ONLY

}  // namespace mcp
