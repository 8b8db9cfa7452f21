// map_graph_lists.h -- the keyframe-major lists of BundleAdjusterMulti::AdjustAndUpdate / MultiKeyFrame::RefreshSceneDepthRobust built on the
// device from the map graph's measurement store (src/KeyFrame.cc:549-570 and 851-869), gfx950.
//
// A call names n_mkfs distinct present MKF slots; keyframe j = i * ncam + c is (slots[i], camera index c).  List j holds, in ASCENDING STORE
// INDEX, the store entries that are alive, of MKF slots[i] and camera c, whose keyframe is active, whose row is a row of the table and whose
// graph column is not MCP_GP_BAD (a row never written reads as bad).  seg_rows is the row, seg_w = inlier / (inlier + outlier) of the table's
// count column (k_tr_scatter's expression, track_record_kernels.h, with the sum formed in double).
//
// ORDER.  The reference walks a std::map keyed by MapPoint pointers, so its order is a pointer order.  Store order is the order fixed here, and
// it is part of the summation contract of mcp_scene_depth_robust (include/mcp_img.h): k_wb_scene_depth adds the entries of a list in list
// position, so the same store gives the same bits of mean and sigma on every run and for every grid size.
//
// This is a stable counting sort by a key only the device can evaluate.  The store is cut into nb contiguous chunks, one workgroup each (nb is
// bounded on the host: MGL_MAX_BLOCKS, so the nb x n_kf count table is sized before the first enqueue):
//   k_mgl_count    chunk pass: the key of every entry (-1: in no list) and its row go to a (key, row) column; every kept entry adds 1 to its key's
//                  cell in the workgroup's OWN row of the table (integer atomics, order-free)
//   k_mgl_scan     one workgroup: every key's column becomes its exclusive prefix over the chunks, the keys' totals become seg_start
//   k_mgl_scatter  chunk pass: a workgroup walks its chunk again in tiles of MGL_BLOCK entries in ascending order; an entry's position is
//                  seg_start[key] + (cell of its key in the workgroup's own row: the entries of the chunks and tiles before) + (the equal keys
//                  before it in the tile, counted in LDS).  Behind a barrier that every read of a cell has returned before (s_waitcnt
//                  vmcnt(0), then the barrier), the last entry of a key in the tile moves the cell on with a plain store; every wavefront
//                  drains its stores the same way before the barrier between two tiles, so the next tile's read of the cell, by the same
//                  workgroup through the same L1, sees it.  No LDS atomics: a rank taken from one would depend on the order the lanes
//                  arrive in.
// No workgroup waits for another, no trip count depends on another workgroup, every cell is written by one workgroup only: the lists are the
// same bytes for every nb and every run.
//
// The predicate, the key and the weight are host / device bodies: mgl_host_lists walks them under the host compiler (no HIP needed: this header
// compiles with a plain C++ compiler; the kernels appear under hipcc, unless MGL_HOST_ONLY is defined) and gives the device's bytes -- integer
// comparisons, and one IEEE division of two exactly converted ints.
#pragma once
#include <cstdint>
#include <cstddef>
#include "../../include/mcp_img.h"

#if defined(__HIPCC__) && !defined(MGL_HOST_ONLY)
#define MGL_HD __host__ __device__
#else
#define MGL_HD
#endif

namespace mcp {

constexpr int MGL_BLOCK = 256;            // threads of a workgroup = entries of a tile
constexpr int MGL_MAX_BLOCKS = 64;        // chunks at the most; the default takes one tile per chunk until the store is longer than that
constexpr int MGL_MAX_KF = MCP_MAP_MAX_MKFS*MCP_MAX_FRAME_CAMS;

MGL_HD inline int mgl_default_blocks(int n_store) {
  const int tiles = (n_store + MGL_BLOCK - 1)/MGL_BLOCK;
  return tiles < 1 ? 1 : (tiles > MGL_MAX_BLOCKS ? MGL_MAX_BLOCKS : tiles);
}
// entries per chunk (the last chunk may be shorter, or empty)
MGL_HD inline int mgl_chunk_len(int n_store, int nb) { return (n_store + nb - 1)/nb; }
MGL_HD inline int mgl_chunk_first(int b, int chunk, int n_store) { const long long f = (long long)b*chunk; return f < n_store ? (int)f : n_store; }
constexpr int MGL_MAX_STORE = 0x7fff0000;  // (a tile past the last entry still counts in an int)

// does the entry name a keyframe of the rig and a row of the table at all
MGL_HD inline bool mgl_entry_ok(int alive, int mkf, int cam, int row, int ncam, int n_rows) {
  return alive && mkf >= 0 && mkf < MCP_MAP_MAX_MKFS && cam >= 0 && cam < ncam && row >= 0 && row < n_rows;
}
// the list of an entry that passed mgl_entry_ok; pos: the index of its MKF among the call's slots (-1: not named), active: mbActive of its
// keyframe, pflags: the graph column of its row.  -1: in no list
MGL_HD inline int mgl_key(int pos, int cam, int ncam, int active, int pflags) {
  return (pos < 0 || !active || (pflags & MCP_GP_BAD)) ? -1 : pos*ncam + cam;
}
// (the sum is formed in double: the bits of k_tr_scatter's (double)inlier / (double)(inlier + outlier) wherever that int sum does not overflow)
MGL_HD inline double mgl_weight(int inlier, int outlier) { return (double)inlier/((double)inlier + (double)outlier); }

// the lists from host arrays.  act: n_slots x ncam; pflags: n_prows graph columns (rows from n_prows on read as bad); inlier / outlier: n_rows;
// slots: n_mkfs distinct slots below n_slots (the caller has checked them).  seg_start: n_kf + 1; seg_rows / seg_w: cap entries.  Returns the
// total, or -1 when it does not fit (then only seg_start is written).
struct MglHostIn {
  int ncam, n_slots; const uint8_t* act;
  int n_rows, n_prows; const int* pflags; const int* inlier; const int* outlier;
  int n_store; const int* ms_mkf; const int* ms_cam; const int* ms_row; const uint8_t* ms_alive;
  int n_mkfs; const int* slots;
};
inline int mgl_host_key(const MglHostIn& I, const int* pos_of, int e) {
  const int mkf = I.ms_mkf[e], cam = I.ms_cam[e], row = I.ms_row[e];
  if (!mgl_entry_ok(I.ms_alive[e], mkf, cam, row, I.ncam, I.n_rows)) return -1;
  const int pos = mkf < I.n_slots ? pos_of[mkf] : -1;
  return mgl_key(pos, cam, I.ncam, pos >= 0 ? I.act[(size_t)mkf*I.ncam + cam] : 0, row < I.n_prows ? I.pflags[row] : MCP_GP_BAD);
}
inline int mgl_host_lists(const MglHostIn& I, int* pos_of /* n_slots, scratch */, int* fill /* n_kf, scratch */, int* seg_start, int cap, int* seg_rows, double* seg_w) {
  const int n_kf = I.n_mkfs*I.ncam;
  for (int k = 0; k < I.n_slots; ++k) pos_of[k] = -1;
  for (int i = 0; i < I.n_mkfs; ++i) pos_of[I.slots[i]] = i;
  for (int j = 0; j <= n_kf; ++j) seg_start[j] = 0;
  for (int e = 0; e < I.n_store; ++e) { const int k = mgl_host_key(I, pos_of, e); if (k >= 0) ++seg_start[k + 1]; }
  for (int j = 0; j < n_kf; ++j) { seg_start[j + 1] += seg_start[j]; fill[j] = seg_start[j]; }
  if (seg_start[n_kf] > cap) return -1;
  for (int e = 0; e < I.n_store; ++e) {
    const int k = mgl_host_key(I, pos_of, e);
    if (k < 0) continue;
    const int at = fill[k]++, row = I.ms_row[e];
    seg_rows[at] = row; seg_w[at] = mgl_weight(I.inlier[row], I.outlier[row]);
  }
  return seg_start[n_kf];
}

}  // namespace mcp

#if defined(__HIPCC__) && !defined(MGL_HOST_ONLY)
#include "map_graph_kernels.h"

namespace mcp {

// chunk pass 1.  pos_of: MCP_MAP_MAX_MKFS entries; pts covers n_rows rows (mcp_map_graph::grow_points); table: nb x n_kf, zeroed
__global__ void __launch_bounds__(MGL_BLOCK)
k_mgl_count(const MgMeas* __restrict__ store, int n_store, int chunk, int ncam, int n_kf, int n_rows, const int* __restrict__ pos_of, const MgMkf* __restrict__ slots,
            const MgPoint* __restrict__ pts, int2* __restrict__ key_row /* n_store */, int* __restrict__ table) {
  const int first = mgl_chunk_first(blockIdx.x, chunk, n_store), last = mgl_chunk_first(blockIdx.x + 1, chunk, n_store);
  int* mine = table + (size_t)blockIdx.x*n_kf;
  for (int e = first + threadIdx.x; e < last; e += MGL_BLOCK) {
    const MgMeas E = store[e];
    int key = -1;
    if (mgl_entry_ok(E.alive, E.mkf, E.cam, E.row, ncam, n_rows)) {
      const int pos = pos_of[E.mkf];
      key = mgl_key(pos, E.cam, ncam, pos >= 0 ? slots[E.mkf].active[E.cam] : 0, pts[E.row].flags);
    }
    key_row[e] = make_int2(key, E.row);
    if (key >= 0) atomicAdd(&mine[key], 1);                                      // key < n_mkfs * ncam = n_kf
  }
}

// one workgroup: table[b][j] becomes the kept entries of key j in the chunks before b, seg_start the exclusive scan of the keys' totals
__global__ void __launch_bounds__(MGL_BLOCK)
k_mgl_scan(int nb, int n_kf, int* __restrict__ table, int* __restrict__ seg_start /* n_kf + 1 */) {
  __shared__ int wtot[MGL_BLOCK/64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int carry = 0;                                                                 // (uniform)
  for (int j0 = 0; j0 < n_kf; j0 += MGL_BLOCK) {
    const int j = j0 + t;
    int s = 0;
    if (j < n_kf) for (int b = 0; b < nb; ++b) { int* cell = table + (size_t)b*n_kf + j; const int v = *cell; *cell = s; s += v; }
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    __syncthreads();                                                             // (the last round's reads of wtot are over)
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int all = 0;
    for (int w = 0; w < MGL_BLOCK/64; ++w) { if (w < wave) incl += wtot[w]; all += wtot[w]; }
    if (j < n_kf) seg_start[j] = carry + incl - s;
    carry += all;
  }
  if (t == 0) seg_start[n_kf] = carry;
}

// chunk pass 2.  cnt: the table's (inlier, outlier) column.  Every position is below seg_start[n_kf] <= n_store, the size of seg_rows / seg_w
__global__ void __launch_bounds__(MGL_BLOCK)
k_mgl_scatter(const int2* __restrict__ key_row, int n_store, int chunk, int n_kf, int* __restrict__ table, const int* __restrict__ seg_start, const int* __restrict__ cnt,
              int* __restrict__ seg_rows, double* __restrict__ seg_w) {
  __shared__ int4 keys4[MGL_BLOCK/4];
  int* keys = reinterpret_cast<int*>(keys4);
  const int first = mgl_chunk_first(blockIdx.x, chunk, n_store), last = mgl_chunk_first(blockIdx.x + 1, chunk, n_store), t = threadIdx.x;
  int* mine = table + (size_t)blockIdx.x*n_kf;
  for (int e0 = first; e0 < last; e0 += MGL_BLOCK) {                             // (uniform: every thread passes every barrier)
    const int e = e0 + t;
    int2 kr = make_int2(-1, 0);
    if (e < last) kr = key_row[e];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             // the tile before: its stores to `mine` have left this wavefront,
    __syncthreads();                                                             // ... and every wavefront is past its reads of keys
    keys[t] = kr.x;
    __syncthreads();
    int before = 0, base = 0; bool later = false;
    if (kr.x >= 0) {
#pragma unroll 4
      for (int q = 0; q < MGL_BLOCK/4; ++q) {
        const int4 v = keys4[q];
        const int i = 4*q;
        before += (v.x == kr.x && i < t) + (v.y == kr.x && i + 1 < t) + (v.z == kr.x && i + 2 < t) + (v.w == kr.x && i + 3 < t);
        later = later || (v.x == kr.x && i > t) || (v.y == kr.x && i + 1 > t) || (v.z == kr.x && i + 2 > t) || (v.w == kr.x && i + 3 > t);
      }
      base = mine[kr.x];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             // every read of a cell has returned ...
    __syncthreads();                                                             // ... before the last entry of its key moves it on
    if (kr.x < 0) continue;
    const int at = seg_start[kr.x] + base + before;
    const int2 io = *reinterpret_cast<const int2*>(cnt + 2*(size_t)kr.y);
    seg_rows[at] = kr.y;
    seg_w[at] = mgl_weight(io.x, io.y);
    if (!later) mine[kr.x] = base + before + 1;
  }
}

// CamFromWorld_j = cfb[c] * bfw(slots[i]), j = i * ncam + c (MultiKeyFrame::RefreshSceneDepthRobust at the graph's own poses)
__global__ void __launch_bounds__(MGL_BLOCK)
k_mgl_cfw(MgRig rig, int n_kf, const int* __restrict__ call_slots, const MgMkf* __restrict__ slots, double* __restrict__ T /* n_kf x 12 */, double* __restrict__ T_host /* pinned, or null */) {
  const int j = blockIdx.x*MGL_BLOCK + threadIdx.x;
  if (j >= n_kf) return;
  const int i = j/rig.ncam, c = j - i*rig.ncam;
  Se3 B, W;
  mg_se3_of12(slots[call_slots[i]].bfw, B);
  se3_compose(rig.cfb[c], B, W);
  for (int k = 0; k < 12; ++k) { const double x = k < 9 ? W.R[k] : W.t[k - 9]; T[12*(size_t)j + k] = x; if (T_host) T_host[12*(size_t)j + k] = x; }
}

// the solver's current pose of MKF i (12 doubles, bit for bit) becomes MgMkf::bfw of slots[i]
__global__ void __launch_bounds__(MGL_BLOCK)
k_mgl_pose_store(int n_mkfs, const int* __restrict__ call_slots, const int* __restrict__ pose_idx, const double* __restrict__ pose_T, MgMkf* __restrict__ slots,
                 double* __restrict__ bfw_host /* pinned n_mkfs x 12, or null */) {
  const int k = blockIdx.x*MGL_BLOCK + threadIdx.x;
  if (k >= n_mkfs*12) return;
  const int i = k/12, a = k - 12*i;
  const double x = pose_T[12*(size_t)pose_idx[i] + a];
  slots[call_slots[i]].bfw[a] = x;
  if (bfw_host) bfw_host[k] = x;
}

// mean -> MgMkf::depth[c] of every keyframe that was refreshed to a finite positive mean; all others keep their bytes
__global__ void __launch_bounds__(MGL_BLOCK)
k_mgl_depth_store(int n_kf, int ncam, const int* __restrict__ call_slots, const mcp_scene_depth* __restrict__ sd /* pinned: written by k_wb_scene_depth */, MgMkf* __restrict__ slots) {
  const int j = blockIdx.x*MGL_BLOCK + threadIdx.x;
  if (j >= n_kf) return;
  const mcp_scene_depth S = sd[j];
  if (S.refreshed == 1 && S.mean - S.mean == 0.0 && S.mean > 0.0) { const int i = j/ncam; slots[call_slots[i]].depth[j - i*ncam] = S.mean; }
}

}  // namespace mcp
#endif  // __HIPCC__ && !MGL_HOST_ONLY
