// map_graph_collect.h -- the co-visible points of the nearest keyframe on the device (include/mcp_img.h mcp_map_collect_nearest,
// mcp_track_collect_nearest): Tracker::CollectNearestPoints with tracker_collect_all_points false (src/Tracker.cc:1785-1854) and
// MapMakerBase::ClosestKeyFrame (src/MapMakerBase.cc:115-140) over the map graph's own columns, gfx950.
//
// One collection serves every camera of a frame: a mark is a byte whose bit c belongs to frame camera c.  The conventions are
// map_graph_kernels.h's: every count is an integer, every atomic ors or adds an integer (LDS or global), nothing depends on the order
// workgroups are dispatched in, no workgroup waits for another.  The candidate rule, the distance, the order, the entry rule and the bit count
// are host / device bodies that the host twin (map_graph_collect_host.cpp) calls too; both units are built without fused multiply-add
// contraction, so the bytes are the same.  The kernels are left out where MGCL_HOST_ONLY is defined.
//
// A collection is five launches on the table's stream behind one memset of the marks (kf_mark | seed | near) and of the device's report:
//   k_mgcl_nearest  one workgroup per frame camera: CamFromWorld = cam_from_base[c] * base_from_world (the pose read from device memory, so
//                   that it may be the one an earlier kernel of the stream left), a strided scan of the (slot, cam) candidates and the LDS
//                   tree of k_mgn_select: the smallest by ascending (dist, slot, cam)
//   k_mgcl_seed     one thread per store entry: an entry of camera c's winner sets bit c of seed[row]
//   k_mgcl_kfs      one thread per store entry: seed[row] is ored into kf_mark[mkf * MCP_MAX_FRAME_CAMS + cam]
//   k_mgcl_rows     one thread per store entry: kf_mark[..] of the entry's keyframe is ored into near[row]
//   k_mgcl_counts   one workgroup: per camera the set bits of seed, kf_mark and near (integer adds), the report into the pinned block
// The boundaries are the grid-wide marks: the winners before an entry is a seed, every seed before a keyframe is marked, every keyframe before
// a row is, every row before it is counted.  Behind a device-side word (`gate`, mcp_track_frame_recover) that is zero no stage writes anything.
// Byte marks are ored through the aligned 32-bit word that holds them; the three blocks start on word boundaries and end on one.
#pragma once
#include <cstdint>
#include <cstddef>
#include "map_graph_dist.h"

namespace mcp {

// what a collection is asked: the current keyframes' CamFromBase, depth means and use bytes (cameras past ncam: not used)
struct MgclIn { Se3 cfb[MCP_MAX_FRAME_CAMS]; double depth[MCP_MAX_FRAME_CAMS]; double frac; uint8_t use[MCP_MAX_FRAME_CAMS]; };

constexpr int MGCL_KF_MARKS = MCP_MAP_MAX_MKFS*MCP_MAX_FRAME_CAMS;                       // bytes of kf_mark
__host__ __device__ inline size_t mgcl_row_bytes(int n_rows) { return ((size_t)(n_rows > 0 ? n_rows : 0) + 255) & ~(size_t)255; }      // bytes of seed and of near

// candidate (slot, cam) has the index slot * MCP_MAX_FRAME_CAMS + cam: ascending index is ascending (slot, cam)
__host__ __device__ inline bool mgcl_is_candidate(int ncam, int cam, int flags, const uint8_t* act) { return cam < ncam && (flags & MCP_MKF_PRESENT) && act[cam]; }
// the current keyframe's CamFromWorld
__host__ __device__ inline void mgcl_cur_cfw(const Se3& cfb, const double* bfw12, Se3& out) { Se3 B; mg_se3_of12(bfw12, B); se3_compose(cfb, B, out); }
// KeyFrame::Distance from the current keyframe to keyframe `cam` of an MKF
__host__ __device__ inline double mgcl_distance(const Se3& cur, double cur_depth, const MgRig& rig, const double* bfw12, const double* dep, int cam, double frac, bool* broken) {
  Se3 B, w2;
  mg_se3_of12(bfw12, B); se3_compose(rig.cfb[cam], B, w2);
  return mg_kf_distance(cur, cur_depth, w2, dep[cam], frac, broken);
}
// is (d, i) chosen before (bd, bi); bi < 0: there is nothing yet
__host__ __device__ inline bool mgcl_before(double d, int i, double bd, int bi) { return bi < 0 || d < bd || (d == bd && i < bi); }
// does a store entry count: mg_edge_live (alive, its row in the table, its MKF a slot) and a camera that indexes kf_mark
__host__ __device__ inline bool mgcl_entry_counts(int alive, int mkf, int cam, int row, int n_rows) {
  return alive && row >= 0 && row < n_rows && mkf >= 0 && mkf < MCP_MAP_MAX_MKFS && cam >= 0 && cam < MCP_MAX_FRAME_CAMS;
}
// the marks of four bytes that have bit c set
__host__ __device__ inline int mgcl_count4(unsigned word, int c) {
  const unsigned v = (word >> c) & 0x01010101u;
  return (int)((v + (v >> 8) + (v >> 16) + (v >> 24)) & 0xffu);
}
// what a report reads before any stage has written it (and, valid apart, what a camera that is not used reads)
inline void mgcl_report_clear(mcp_collect_report* r) {
  *r = mcp_collect_report();
  for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) { r->nearest_slot[c] = -1; r->nearest_cam[c] = -1; }
}

#if defined(__HIPCC__) && !defined(MGCL_HOST_ONLY)
constexpr int MGCL_BLOCK = 256, MGCL_COUNT_BLOCK = 1024;

__device__ __forceinline__ void mgcl_or_byte(uint8_t* base, size_t i, unsigned bits) {
  if ((base[i] & bits) == bits) return;                // (set already: or is idempotent, so a stale read only costs the atomic)
  atomicOr(reinterpret_cast<unsigned*>(base + (i & ~(size_t)3)), bits << (8*(unsigned)(i & 3)));
}

// one workgroup per frame camera (a grid of MCP_MAX_FRAME_CAMS: a camera that is not used reads nearest -1); rep: device, zeroed
__global__ void __launch_bounds__(MGCL_BLOCK)
k_mgcl_nearest(const int* __restrict__ gate, MgclIn In, const double* __restrict__ bfw12, MgRig rig, const MgMkf* __restrict__ slots, int n_slots,
               mcp_collect_report* __restrict__ rep) {
  __shared__ double wd[MGCL_BLOCK]; __shared__ int wi[MGCL_BLOCK];
  __shared__ int n_cand, broken;
  if (gate && *gate == 0) return;                      // (uniform over the grid)
  const int c = blockIdx.x, t = threadIdx.x;
  if (!In.use[c]) { if (t == 0) { rep->nearest_slot[c] = -1; rep->nearest_cam[c] = -1; } return; }
  if (t == 0) { n_cand = 0; broken = 0; }
  __syncthreads();
  Se3 cur;
  mgcl_cur_cfw(In.cfb[c], bfw12, cur);
  double bd = 0.0; int bi = -1, mine = 0; bool br_any = false;
  for (int idx = t; idx < n_slots*MCP_MAX_FRAME_CAMS; idx += MGCL_BLOCK) {
    const int slot = idx/MCP_MAX_FRAME_CAMS, cam = idx % MCP_MAX_FRAME_CAMS;
    const MgMkf& K = slots[slot];
    if (!mgcl_is_candidate(rig.ncam, cam, K.flags, K.active)) continue;
    bool br;
    const double d = mgcl_distance(cur, In.depth[c], rig, K.bfw, K.depth, cam, In.frac, &br);
    ++mine; br_any = br_any || br;
    if (mgcl_before(d, idx, bd, bi)) { bd = d; bi = idx; }
  }
  if (mine) atomicAdd(&n_cand, mine);
  if (br_any) atomicOr(&broken, 1);
  wd[t] = bd; wi[t] = bi;
  __syncthreads();
  for (int h = MGCL_BLOCK/2; h > 0; h >>= 1) {
    if (t < h) {
      const int o = wi[t + h];
      if (o >= 0 && mgcl_before(wd[t + h], o, wd[t], wi[t])) { wd[t] = wd[t + h]; wi[t] = o; }
    }
    __syncthreads();
  }
  if (t != 0) return;
  const int win = wi[0];
  const int status = broken ? 3 : (win < 0 ? 1 : 0);   // KeyFrame.cc:734-744; MapMakerBase.cc:138
  rep->status[c] = status; rep->n_candidates[c] = n_cand;
  rep->nearest_slot[c] = status == 0 ? win/MCP_MAX_FRAME_CAMS : -1; rep->nearest_cam[c] = status == 0 ? win % MCP_MAX_FRAME_CAMS : -1;
  rep->nearest_dist[c] = status == 0 ? wd[0] : 0.0;
}

// one thread per store entry: the rows the winners measure
__global__ void __launch_bounds__(MGCL_BLOCK)
k_mgcl_seed(const int* __restrict__ gate, const mcp_collect_report* __restrict__ rep, const MgMeas* __restrict__ store, int n_store, int n_rows, uint8_t* __restrict__ seed) {
  __shared__ int ws[MCP_MAX_FRAME_CAMS], wc[MCP_MAX_FRAME_CAMS];
  if (gate && *gate == 0) return;
  if (threadIdx.x < MCP_MAX_FRAME_CAMS) { ws[threadIdx.x] = rep->nearest_slot[threadIdx.x]; wc[threadIdx.x] = rep->nearest_cam[threadIdx.x]; }      // (-1: matches no entry that counts)
  __syncthreads();
  const int i = blockIdx.x*MGCL_BLOCK + threadIdx.x;
  if (i >= n_store) return;
  const MgMeas& E = store[i];
  const int alive = E.alive, mkf = E.mkf, cam = E.cam, row = E.row;
  if (!mgcl_entry_counts(alive, mkf, cam, row, n_rows)) return;
  unsigned bits = 0u;
#pragma unroll
  for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) bits |= (mkf == ws[c] && cam == wc[c]) ? (1u << c) : 0u;
  if (bits) mgcl_or_byte(seed, (size_t)row, bits);
}

// one thread per store entry: the keyframes that measure a seed row
__global__ void __launch_bounds__(MGCL_BLOCK)
k_mgcl_kfs(const int* __restrict__ gate, const MgMeas* __restrict__ store, int n_store, int n_rows, const uint8_t* __restrict__ seed, uint8_t* __restrict__ kf_mark) {
  if (gate && *gate == 0) return;
  const int i = blockIdx.x*MGCL_BLOCK + threadIdx.x;
  if (i >= n_store) return;
  const MgMeas& E = store[i];
  const int alive = E.alive, mkf = E.mkf, cam = E.cam, row = E.row;
  if (!mgcl_entry_counts(alive, mkf, cam, row, n_rows)) return;
  const unsigned bits = seed[row];
  if (bits) mgcl_or_byte(kf_mark, (size_t)mkf*MCP_MAX_FRAME_CAMS + cam, bits);
}

// one thread per store entry: the rows those keyframes measure
__global__ void __launch_bounds__(MGCL_BLOCK)
k_mgcl_rows(const int* __restrict__ gate, const MgMeas* __restrict__ store, int n_store, int n_rows, const uint8_t* __restrict__ kf_mark, uint8_t* __restrict__ near) {
  if (gate && *gate == 0) return;
  const int i = blockIdx.x*MGCL_BLOCK + threadIdx.x;
  if (i >= n_store) return;
  const MgMeas& E = store[i];
  const int alive = E.alive, mkf = E.mkf, cam = E.cam, row = E.row;
  if (!mgcl_entry_counts(alive, mkf, cam, row, n_rows)) return;
  const unsigned bits = kf_mark[(size_t)mkf*MCP_MAX_FRAME_CAMS + cam];
  if (bits) mgcl_or_byte(near, (size_t)row, bits);
}

// one workgroup: the set bits per camera of the three blocks, word by word (the blocks end on word boundaries and their padding is zero), and
// the finished report into the pinned block
__global__ void __launch_bounds__(MGCL_COUNT_BLOCK)
k_mgcl_counts(const int* __restrict__ gate, const uint8_t* __restrict__ kf_mark, const uint8_t* __restrict__ seed, const uint8_t* __restrict__ near, int n_rows,
              mcp_collect_report* __restrict__ rep, mcp_collect_report* __restrict__ out /* pinned host */) {
  __shared__ int cnt[3][MCP_MAX_FRAME_CAMS];
  if (gate && *gate == 0) return;
  const int t = threadIdx.x;
  if (t < 3*MCP_MAX_FRAME_CAMS) (&cnt[0][0])[t] = 0;
  __syncthreads();
  const size_t words[3] = {(size_t)MGCL_KF_MARKS/4, mgcl_row_bytes(n_rows)/4, mgcl_row_bytes(n_rows)/4};
  const unsigned* blocks[3] = {reinterpret_cast<const unsigned*>(kf_mark), reinterpret_cast<const unsigned*>(seed), reinterpret_cast<const unsigned*>(near)};
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    int mine[MCP_MAX_FRAME_CAMS];
#pragma unroll
    for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) mine[c] = 0;
    for (size_t k = t; k < words[b]; k += MGCL_COUNT_BLOCK) {
      const unsigned w = blocks[b][k];
      if (!w) continue;
#pragma unroll
      for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) mine[c] += mgcl_count4(w, c);
    }
#pragma unroll
    for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) if (mine[c]) atomicAdd(&cnt[b][c], mine[c]);
  }
  __syncthreads();
  if (t != 0) return;
  mcp_collect_report R = *rep;
  for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) { R.n_kfs[c] = cnt[0][c]; R.n_seed_rows[c] = cnt[1][c]; R.n_rows[c] = cnt[2][c]; }
  R.valid = 1;
  *out = R;
}
#endif  // __HIPCC__ && !MGCL_HOST_ONLY

}  // namespace mcp
