// map_graph_cull.h -- outliers and bad points on the device (include/mcp_img.h mcp_map_cull_*): MapMakerServerBase::HandleOutliers
// (src/MapMakerServerBase.cc:1198-1238) and the point half of MapMaker::HandleBadEntities -- MarkDanglersAsBad, MarkOutliersAsBad
// (src/MapMakerClientBase.cc:73-108), Map::MoveBadPointsToTrash (src/Map.cc:93-116) -- over the map graph's store and point columns and the
// table's count and usable columns, gfx950.
//
// The conventions are map_graph_kernels.h's: every count is an integer and every atomic adds or maximises an integer (LDS or global); the
// report is compacted by index (per-workgroup counts, then mg_rank's ballot scatter), so nothing depends on the order workgroups are
// dispatched in; no workgroup waits for another; 256-thread workgroups.  The two rules are host / device bodies that the host twins
// (map_graph_cull_host.cpp) walk under the host compiler: integer comparisons and one product in double, so the bytes are the same.
// This header compiles with a plain C++ compiler; the kernels appear under hipcc, unless MGC_HOST_ONLY is defined.
//
// mcp_map_cull_outliers is three launches on the table's stream:
//   k_mg_edges_count  store pass: the good count of every row (map_graph_kernels.h)
//   k_mgc_match       store pass: a live entry whose key is among the sorted keys (binary search) leaves its store index with that key's
//                     list index
//   k_mgc_judge       one thread per key in (row, list index) order; the thread at the head of a row's run walks the run: the row's flags and
//                     good count in registers, a verdict per entry, the deaths, the row's mark; the tally by LDS then global integer atomics
// The boundaries are the grid-wide facts: every match and every good count must be there before a row is judged.  Rows are independent of each
// other (a key names one row, a store entry one key), so the only serial part is the walk within a row.
// mcp_map_cull_sweep is three launches:
//   k_mg_edges_count  as above
//   k_mgc_sweep_rows  row pass: the two rules, the row's flags, the table's usable byte, the report mark, the pending mark cleared, the counts
//   k_mgc_sweep_emit  row blocks: the reported rows ranked into the pinned view; store blocks: the live entries of bad rows die
// Here the row marks must be complete before a store entry is judged, and every workgroup's count before a row is ranked.
#pragma once
#include <cstdint>
#include <cstddef>
#include "../../include/mcp_img.h"

#if defined(__HIPCC__) && !defined(MGC_HOST_ONLY)
#define MGC_HD __host__ __device__
#else
#define MGC_HD
#endif

namespace mcp {

MGC_HD inline bool mgc_mkf_ok(int flags) { return (flags & MCP_MKF_PRESENT) && !(flags & MCP_MKF_BAD); }
// the store's key of a measurement (map_graph_kernels.h mg_key)
MGC_HD inline unsigned long long mgc_key(int mkf, int cam, int row) { return ((unsigned long long)(unsigned)(mkf*MCP_MAX_FRAME_CAMS + cam) << 32) | (unsigned)row; }
// a row never written reads (no source, bad, not fixed) -- k_mg_points_fill -- which mcp_map_graph_update_points refuses to write
MGC_HD inline bool mgc_row_written(int src_mkf, int flags) { return src_mkf >= 0 || (flags & MCP_GP_FIXED); }

// a row while its outliers are walked
struct MgcRow { int flags, good; };

// HandleOutliers' loop body for one outlier (MapMakerServerBase.cc:1204-1236).  found: a live entry has the key, its row is written, its slot
// present; entry_mkf_ok: that MKF is present and not bad (its entries count as good).  *dies: the entry is erased.
MGC_HD inline int mgc_judge(MgcRow& S, bool found, int source, bool entry_mkf_ok, int bad_good_count, bool* dies) {
  *dies = false;
  if (!found) return MCP_CULL_MISSING;
  if (S.flags & MCP_GP_FIXED) return MCP_CULL_FIXED;                                               // :1210-1214
  if (S.good <= bad_good_count || source == MCP_SRC_ROOT) { S.flags |= MCP_GP_BAD; return MCP_CULL_POINT_BAD; }      // :1216-1220
  if (S.flags & MCP_GP_BAD) return MCP_CULL_ALREADY_BAD;                                           // :1221
  *dies = true;                                                                                    // :1229-1230
  if (entry_mkf_ok) --S.good;
  return (source == MCP_SRC_TRACKER || source == MCP_SRC_EPIPOLAR) ? MCP_CULL_RETRY : MCP_CULL_NEVER_RETRY;      // :1224-1227
}

// MarkDanglersAsBad, then MarkOutliersAsBad, for a row: 0 stays, 1 a dangler, 2 a tracker outlier (MapMakerClientBase.cc:73-108)
MGC_HD inline int mgc_sweep_rule(int flags, int good, int inlier, int outlier, int danglers_on, int min_outliers, double multiplier) {
  if (flags & (MCP_GP_BAD | MCP_GP_FIXED)) return 0;
  if (danglers_on && good < 2) return 1;
  if (outlier > min_outliers && (double)outlier > (double)inlier*multiplier) return 2;
  return 0;
}

// what the launches leave for the host: the six verdict counters, the distinct fixed rows, the rows marked; the sweep's five counters
struct MgcCtl { int verdicts[6]; int fixed_rows, rows_marked; int danglers, tracker, reported, bad_rows, erased; int pad_[3]; };
struct MgcRun { int row, idx; };                       // a key's row and its place in the caller's list, sorted by (row, idx)

#if defined(__HIPCC__) && !defined(MGC_HOST_ONLY)
constexpr int MGC_BLOCK = MG_BLOCK;
static_assert(offsetof(MgPoint, pending) == 12 && sizeof(MgPoint) == 16, "the pending mark is the fourth word of a row's graph column");

__global__ void __launch_bounds__(MGC_BLOCK)
k_mgc_match(const MgMeas* __restrict__ store, int n_store, const unsigned long long* __restrict__ keys, const int* __restrict__ key_idx, int n,
            int* __restrict__ match /* n, -1 before */) {
  const int i = blockIdx.x*MGC_BLOCK + threadIdx.x;
  if (i >= n_store) return;
  const MgMeas E = store[i];
  if (!E.alive || E.mkf < 0 || E.mkf >= MG_MAX_MKFS || E.cam < 0 || E.cam >= MCP_MAX_FRAME_CAMS) return;
  const unsigned long long k = mgc_key(E.mkf, E.cam, E.row);
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < k) lo = mid + 1; else hi = mid; }
  if (lo < n && keys[lo] == k) atomicMax(&match[key_idx[lo]], i);      // (of several live entries with one key -- the caller's error -- the last)
}

__global__ void __launch_bounds__(MGC_BLOCK)
k_mgc_judge(int n, const MgcRun* __restrict__ runs, const int* __restrict__ match, MgMeas* __restrict__ store, const MgMkf* __restrict__ slots,
            MgPoint* __restrict__ pts, int n_prows, int n_rows, const int* __restrict__ good, int bad_good_count, uint8_t* __restrict__ verdict,
            MgcCtl* __restrict__ ctl /* zeroed */) {
  __shared__ int cnt[8];                               // the six verdicts | rows with a FIXED verdict | rows marked
  if (threadIdx.x < 8) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int j = blockIdx.x*MGC_BLOCK + threadIdx.x;
  if (j < n && (j == 0 || runs[j - 1].row != runs[j].row)) {      // the head of a row's run walks it
    const int row = runs[j].row;
    bool row_ok = row >= 0 && row < n_rows && row < n_prows;
    MgcRow S; S.flags = 0; S.good = 0;
    int was = 0;
    if (row_ok) {
      const MgPoint P = pts[row];
      row_ok = mgc_row_written(P.src_mkf, P.flags);
      S.flags = was = P.flags; S.good = good[row];
    }
    bool any_fixed = false;
    for (int q = j; q < n && runs[q].row == row; ++q) {
      const int idx = runs[q].idx, at = match[idx];
      bool found = row_ok && at >= 0, ok = false, dies;
      int source = 0;
      if (found) {
        const int mkf = store[at].mkf, f = slots[mkf].flags;       // (k_mgc_match leaves only entries whose MKF is a slot)
        found = (f & MCP_MKF_PRESENT) != 0; ok = mgc_mkf_ok(f); source = store[at].source;
      }
      const int v = mgc_judge(S, found, source, ok, bad_good_count, &dies);
      if (dies) store[at].alive = 0;
      verdict[idx] = (uint8_t)v;
      atomicAdd(&cnt[v], 1);
      any_fixed = any_fixed || v == MCP_CULL_FIXED;
    }
    if (row_ok && !(was & MCP_GP_BAD) && (S.flags & MCP_GP_BAD)) { pts[row].flags = S.flags; pts[row].pending = 1; atomicAdd(&cnt[7], 1); }
    if (any_fixed) atomicAdd(&cnt[6], 1);
  }
  __syncthreads();
  if (threadIdx.x < 8 && cnt[threadIdx.x]) atomicAdd(&ctl->verdicts[threadIdx.x], cnt[threadIdx.x]);      // (verdicts[6], [7]: fixed_rows, rows_marked)
}
static_assert(offsetof(MgcCtl, fixed_rows) == 6*sizeof(int) && offsetof(MgcCtl, rows_marked) == 7*sizeof(int), "k_mgc_judge adds its eight counters as one array");

struct MgcSweep { int min_outliers, danglers_on; double multiplier; };

__global__ void __launch_bounds__(MGC_BLOCK)
k_mgc_sweep_rows(MgcSweep Q, MgPoint* __restrict__ pts, int n_prows, int n_rows, const int* __restrict__ good, const int* __restrict__ counts /* (inlier, outlier) */,
                 PvsPoint* __restrict__ table, uint8_t* __restrict__ rep, int* __restrict__ blk_cnt, MgcCtl* __restrict__ ctl /* zeroed */) {
  __shared__ int cnt[4];                               // danglers | tracker outliers | reported | bad rows
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x*MGC_BLOCK + threadIdx.x;
  int rule = 0;
  bool bad = false, report = false;
  if (i < n_rows) {
    if (i < n_prows) {
      const MgPoint P = pts[i];
      rule = mgc_sweep_rule(P.flags, good[i], counts[2*(size_t)i], counts[2*(size_t)i + 1], Q.danglers_on, Q.min_outliers, Q.multiplier);
      bad = rule || (P.flags & MCP_GP_BAD);
      report = rule || ((P.flags & MCP_GP_BAD) && P.pending);
      if (rule) pts[i].flags = P.flags | MCP_GP_BAD;
      if (P.pending) pts[i].pending = 0;                     // (rep carries the mark to the report)
    } else bad = true;                                 // (no graph column yet: never written)
    if (bad) table[i].usable = 0;
    rep[i] = report ? 1 : 0;
  }
  const unsigned long long m1 = __ballot(rule == 1), m2 = __ballot(rule == 2), mr = __ballot(report), mb = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    if (m1) atomicAdd(&cnt[0], __popcll(m1)); if (m2) atomicAdd(&cnt[1], __popcll(m2)); if (mr) atomicAdd(&cnt[2], __popcll(mr)); if (mb) atomicAdd(&cnt[3], __popcll(mb));
  }
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt[2];
  if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&ctl->danglers + threadIdx.x, cnt[threadIdx.x]);
}
static_assert(offsetof(MgcCtl, bad_rows) == offsetof(MgcCtl, danglers) + 3*sizeof(int), "k_mgc_sweep_rows adds its four counters as one array");

// row blocks [0, nblk_rows): the reported rows, ascending, into the pinned view; store blocks after them: the live entries of bad rows die
__global__ void __launch_bounds__(MGC_BLOCK)
k_mgc_sweep_emit(int n_rows, int n_prows, int nblk_rows, const uint8_t* __restrict__ rep, const int* __restrict__ blk_cnt, int* __restrict__ out_rows /* pinned */, int cap,
                 MgMeas* __restrict__ store, int n_store, const MgPoint* __restrict__ pts, MgcCtl* __restrict__ ctl) {
  if ((int)blockIdx.x < nblk_rows) {
    const int i = blockIdx.x*MGC_BLOCK + threadIdx.x;
    const bool keep = i < n_rows && rep[i];
    const int at = mg_rank(keep, blk_cnt, nblk_rows, blockIdx.x, nullptr);
    if (keep && at >= 0 && at < cap) out_rows[at] = i;
    return;
  }
  const int i = (blockIdx.x - nblk_rows)*MGC_BLOCK + threadIdx.x;
  bool dies = false;
  if (i < n_store) {
    const int row = store[i].row;
    if (store[i].alive && row >= 0 && row < n_rows) dies = row >= n_prows || (pts[row].flags & MCP_GP_BAD);
    if (dies) store[i].alive = 0;
  }
  const unsigned long long m = __ballot(dies);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl->erased, __popcll(m));
}
#endif  // __HIPCC__

// ---- the host's statement of the two calls (plain arrays, in place) ----------------------------------------------------------------------------
struct MgcHostMap {
  int n_slots; const int* mkf_flags; int n_rows, n_prows; const int* src_mkf; int* pflags; uint8_t* pending;
  int n_store; const int* ms_mkf; const int* ms_cam; const int* ms_row; const int* ms_source; uint8_t* ms_alive;
};
MGC_HD inline int mgc_host_mkf_flags(const MgcHostMap& M, int mkf) { return (mkf >= 0 && mkf < M.n_slots) ? M.mkf_flags[mkf] : 0; }
// does a store entry count at all (map_graph_kernels.h mg_edge_live)
MGC_HD inline bool mgc_edge_live(int alive, int mkf, int row, int n_rows) { return alive && row >= 0 && row < n_rows && mkf >= 0 && mkf < MCP_MAP_MAX_MKFS; }

}  // namespace mcp
