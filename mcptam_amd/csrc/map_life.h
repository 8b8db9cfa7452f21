// map_life.h -- how a device map begins and how it is rescaled or moved (include/mcp_img.h mcp_init_depth_map_points, mcp_map_mark_optimized,
// mcp_map_rescale, mcp_map_transform): MapMakerServerBase::AddInitDepthMapPoints (src/MapMakerServerBase.cc:499-546), the mbOptimized
// loop at the end of InitFromMultiKeyFrame (:212-215), ApplyGlobalScaleToMap (:549-574) and ApplyGlobalTransformationToMap (:577-596), gfx950.
//
// The conventions are map_graph_kernels.h's: every count is an integer, every atomic adds an integer, the one compaction ranks by index
// (per-workgroup counts, then mg_rank's ballot scatter), nothing depends on the order workgroups are dispatched in, no workgroup waits for
// another, 256-thread workgroups, one lane per item.  What a candidate becomes, what a row and an MKF become under a scale or a rigid motion and
// which rows are marked are __host__ __device__ bodies that the host twins (map_life_host.cpp, the host half of a HIP source) call too; both
// units are built without fused multiply-add contraction, so the bytes are the same.  The kernels are left out where ML_HOST_ONLY is defined.
//
// mcp_init_depth_map_points enqueues per camera c that has candidates:
//   k_sa_busy_mark, k_sa_busy_gather, k_sa_thin_busy   (stereo_append.h, unchanged) the busy list of (src_mkf, c) from the store, ThinCandidates
//   k_ml_alive_mark   one lane per candidate: the workgroup's count of survivors
//   k_ml_create       one lane per candidate: the survivor's rank (mg_rank); rank < limit makes point base[c] + rank, base[c] read from device
//                     memory where camera c - 1 left it: the record, the row's columns, the graph column, one store entry (sa_point's row)
// mcp_map_mark_optimized: k_ml_mark_optimized, one lane per row.
// mcp_map_rescale / _transform: k_ml_mkfs (one lane per slot), k_ml_points (one lane per row; the new pose of the row's source is read
// from the slots k_ml_mkfs has just written: the boundary between the two launches), then, for a rescale, the list passes and k_wb_scene_depth
// of mcp_graph_refresh_depth over every present slot.
#pragma once
#include <cstdint>
#include <cstddef>
#if defined(ML_HOST_ONLY)          // the host twin: the bodies of the two headers below without their kernels
#ifndef STEREO_HOST_ONLY
#define STEREO_HOST_ONLY
#endif
#ifndef SA_HOST_ONLY
#define SA_HOST_ONLY
#endif
#endif
#include "stereo_kernels.h"      // stereo_unproject, normalize3, stereo_pixel_vectors
#include "map_graph_dist.h"      // se3_inverse, MgRig, mg_se3_of12
#include "stereo_append.h"       // SaRow, sa_point; the busy kernels

namespace mcp {

// ---- ThinCandidates of one candidate for the host twin: k_sa_thin_busy's walk over the list with the kernels' own two rules (ir_round, --------
// ---- stereo_busy: stereo_kernels.h) ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool ml_thin_keep(int cx, int cy, int level, int n_meas, const mcp_stereo_meas* meas) {
  const double sc = (double)(1 << level);
  for (int m = 0; m < n_meas; ++m) {
    if (!(meas[m].level == level || meas[m].level == level + 1)) continue;
    if (stereo_busy(ir_round(meas[m].root_pos[0]/sc), ir_round(meas[m].root_pos[1]/sc), cx, cy)) return false;
  }
  return true;
}

// ---- one init-depth point (:514-532) -------------------------------------------------------------------------------------------------------
// CamFromWorld of keyframe (slot, cam) from the graph's own columns: k_mgl_cfw's product
__host__ __device__ inline void ml_cfw(const MgRig& rig, int cam, const double* bfw, Se3& W) {
  Se3 B;
  mg_se3_of12(bfw, B);
  se3_compose(rig.cfb[cam], B, W);
}
// candidate i = (cx, cy) at `level` of a keyframe at CamFromWorld W: the record mcp_stereo_points would hand back, target -1
__host__ __device__ inline void ml_init_point(const mcp_camera& cam, const Se3& W, int level, int i, int cx, int cy, double init_depth, mcp_stereo_point& P) {
  const int s = 1 << level;
  const double root[2] = { (cx + 0.5)*s - 0.5, (cy + 0.5)*s - 0.5 };                         // LevelZeroPos
  double ray[3], pc[3];
  stereo_unproject(cam, root[0], root[1], ray);
  for (int k = 0; k < 3; ++k) { pc[k] = ray[k]*init_depth; P.center_nc[k] = ray[k]; }       // v3UnProj (:515)
  Se3 Wi; se3_inverse(W, Wi);
  se3_apply(Wi, pc, P.world_pos);                                                            // :518
  normalize3(P.center_nc);                                                                   // :528
  stereo_unproject(cam, root[0] + s, root[1] + 0, P.one_right_nc); normalize3(P.one_right_nc);
  stereo_unproject(cam, root[0] + 0, root[1] + s, P.one_down_nc); normalize3(P.one_down_nc);
  stereo_pixel_vectors(W, P.center_nc, P.one_right_nc, P.one_down_nc, P.world_pos, P.pixel_right_w, P.pixel_down_w);
  P.candidate = i; P.target = -1; P.hypothesis = 0; P.score = 0;
  P.root_pos[0] = root[0]; P.root_pos[1] = root[1]; P.target_pos[0] = 0.0; P.target_pos[1] = 0.0;
}

// ---- the end of init: which rows become usable (:212-215) -----------------------------------------------------------------------------------
// row < n_point_rows: the graph column covers it (a row it does not cover was never written); a covered row that was never written reads as bad
__host__ __device__ inline bool ml_marks(int row, int n_point_rows, int pflags) { return row < n_point_rows && !(pflags & MCP_GP_BAD); }

// ---- a scale or a rigid motion of the whole map ---------------------------------------------------------------------------------------------
enum { ML_SCALE = 0, ML_RIGID = 1 };
struct MlXform { int kind, pad_; double scale; Se3 T, Tinv; };      // T: new_from_old, Tinv its se3_inverse (formed once, on the host)
enum { ML_ROW_NO_SOURCE = 0, ML_ROW_NO_RAYS = 1, ML_ROW_REFRESHED = 2 };

__host__ __device__ inline void ml_mkf_move(const MlXform& X, double* bfw) {
  if (X.kind == ML_SCALE) { bfw[9] *= X.scale; bfw[10] *= X.scale; bfw[11] *= X.scale; return; }      // :559
  Se3 B, O;
  mg_se3_of12(bfw, B);
  se3_compose(B, X.Tinv, O);                                                                            // :582
  for (int k = 0; k < 9; ++k) bfw[k] = O.R[k];
  for (int k = 0; k < 3; ++k) bfw[9 + k] = O.t[k];
}
__host__ __device__ inline void ml_world_move(const MlXform& X, double* w) {
  if (X.kind == ML_SCALE) { w[0] *= X.scale; w[1] *= X.scale; w[2] *= X.scale; return; }               // :553
  double o[3];
  se3_apply(X.T, w, o);                                                                                 // :593
  w[0] = o[0]; w[1] = o[1]; w[2] = o[2];
}
// does the graph column name a slot and a camera of the rig at all (whether the slot is present is the caller's look at its flags)
__host__ __device__ inline bool ml_has_source(int src_mkf, int src_cam, int ncam) { return src_mkf >= 0 && src_mkf < MCP_MAP_MAX_MKFS && src_cam >= 0 && src_cam < ncam; }
__host__ __device__ inline int ml_row_class(bool source_present, bool has_rays) { return !source_present ? ML_ROW_NO_SOURCE : (has_rays ? ML_ROW_REFRESHED : ML_ROW_NO_RAYS); }
// a row with a source: the new world position and, with rays, RefreshPixelVectors at the source keyframe's NEW pose (new_bfw: already moved)
__host__ __device__ inline void ml_row_move(const MlXform& X, const MgRig& rig, int src_cam, const double* new_bfw, bool has_rays, const double* rays, double* world,
                                            double* pr, double* pd) {
  ml_world_move(X, world);
  if (!has_rays) return;
  Se3 W;
  ml_cfw(rig, src_cam, new_bfw, W);
  stereo_pixel_vectors(W, rays, rays + 3, rays + 6, world, pr, pd);
}
__host__ __device__ inline bool ml_bit(const uint8_t* bits, int i) { return (bits[i >> 3] >> (i & 7)) & 1; }
// the motion of a call, checked (host): NULL when it is one, otherwise what is wrong with it.  The inverse is formed here, once, for both sides
inline const char* ml_xform_make(int kind, double scale, const double* new_from_old, MlXform& X) {
  X.kind = kind; X.pad_ = 0; X.scale = 1.0;
  se3_identity(X.T); se3_identity(X.Tinv);
  if (kind == ML_SCALE) {
    if (!(scale - scale == 0.0) || !(scale > 0.0)) return "scale must be finite and positive";
    X.scale = scale;
    return nullptr;
  }
  if (kind != ML_RIGID) return "unknown kind";
  if (!new_from_old) return "new_from_old is NULL";
  for (int k = 0; k < 12; ++k) if (!(new_from_old[k] - new_from_old[k] == 0.0)) return "new_from_old has a non-finite entry";
  mg_se3_of12(new_from_old, X.T);
  double RRt[9];
  mat3_mul_t(X.T.R, X.T.R, RRt);
  for (int k = 0; k < 9; ++k) {
    const double d = RRt[k] - (k % 4 == 0 ? 1.0 : 0.0);
    if (!(d <= 1e-9 && d >= -1e-9)) return "the rotation part of new_from_old is not orthonormal (max |R R^T - I| > 1e-9)";
  }
  se3_inverse(X.T, X.Tinv);
  return nullptr;
}

#if defined(__HIPCC__) && !defined(ML_HOST_ONLY)
constexpr int ML_BLOCK = MG_BLOCK;

// what the launches of one init-depth call hand to each other and to the host (device, copied to pinned memory before the wait)
struct MlInitCtl { int base[MCP_MAX_FRAME_CAMS + 1], made[MCP_MAX_FRAME_CAMS], n_busy[MCP_MAX_FRAME_CAMS], n_alive[MCP_MAX_FRAME_CAMS]; };

__global__ void __launch_bounds__(ML_BLOCK)
k_ml_alive_mark(int n_cand, const uint8_t* __restrict__ alive, int* __restrict__ blk_cnt) {
  __shared__ int cnt;
  const int i = blockIdx.x*ML_BLOCK + threadIdx.x;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const unsigned long long m = __ballot(i < n_cand && alive[i]);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt, __popcll(m));
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = cnt;
}

// where a camera's points go, and how far a write may: the blocks were grown on the host to cover every row handed in and n_rows store entries
struct MlCreate {
  mcp_camera camera; int cam, n_cand, limit, level, src_mkf, slot1, n_rows, first_store, table_rows, graph_rows, ncam_states; double init_depth;
  long long store_cap;
};
__global__ void __launch_bounds__(ML_BLOCK)
k_ml_create(MlCreate Q, MgRig rig, const MgMkf* __restrict__ slots, const mcp_int2* __restrict__ cand, const uint8_t* __restrict__ alive, const int* __restrict__ blk_cnt, int nblk,
            const int* __restrict__ n_busy /* k_sa_busy_gather's */, MlInitCtl* __restrict__ ctl, const int* __restrict__ rows, const int* __restrict__ keys,
            mcp_stereo_point* __restrict__ recs /* pinned, n_rows */, PvsPoint* __restrict__ pts, TmSrc* __restrict__ src, TmStates states, int* __restrict__ cnt,
            double* __restrict__ rays, MgPoint* __restrict__ gp, mcp_store_entry* __restrict__ store) {
  const int i = blockIdx.x*ML_BLOCK + threadIdx.x;
  const bool live = i < Q.n_cand && alive[i];
  int total = 0;
  const int at = mg_rank(live, blk_cnt, nblk, blockIdx.x, &total);
  const int base = ctl->base[Q.cam];                      // (camera c - 1's launch wrote it; this launch writes only base[c + 1])
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int made = total < Q.limit ? total : Q.limit;
    ctl->made[Q.cam] = made; ctl->n_alive[Q.cam] = total; ctl->n_busy[Q.cam] = *n_busy; ctl->base[Q.cam + 1] = base + made;
  }
  if (!live || at >= Q.limit) return;
  const long long k = (long long)base + at, st_at = (long long)Q.first_store + k;
  if (k >= Q.n_rows || st_at >= Q.store_cap) return;      // (never: n_rows >= sum min(n_cand, limit), the store was grown by n_rows)
  const int row = rows[k];
  if (row < 0 || row >= Q.table_rows || row >= Q.graph_rows) return;                                   // (never: checked and grown on the host)
  Se3 W;
  ml_cfw(rig, Q.cam, slots[Q.src_mkf].bfw, W);
  mcp_stereo_point P;
  ml_init_point(Q.camera, W, Q.level, i, cand[i].x, cand[i].y, Q.init_depth, P);
  recs[k] = P;
  SaRow R; mcp_store_entry root, unused;
  sa_point(P, row, Q.level, Q.src_mkf, Q.cam, -1, -1, R, root, unused);
  sa_write_row(R, row, keys[k], Q.slot1, Q.ncam_states, pts, src, states, cnt, rays, gp);      // the row, by the statements k_sa_append runs
  store[st_at] = root;
}

// usable = 1 on every row ml_marks names; nothing else of a row is written
__global__ void __launch_bounds__(ML_BLOCK)
k_ml_mark_optimized(int n_rows, int n_point_rows, const MgPoint* __restrict__ gp, PvsPoint* __restrict__ pts, int* __restrict__ n_marked) {
  const int r = blockIdx.x*ML_BLOCK + threadIdx.x;
  const bool hit = r < n_rows && ml_marks(r, n_point_rows, r < n_point_rows ? gp[r].flags : MCP_GP_BAD);
  if (hit) pts[r].usable = 1;
  const unsigned long long m = __ballot(hit);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_marked, __popcll(m));
}

// one lane per slot: a present MKF (a bad one too) moves
__global__ void __launch_bounds__(ML_BLOCK)
k_ml_mkfs(MlXform X, MgMkf* __restrict__ slots) {
  const int k = blockIdx.x*ML_BLOCK + threadIdx.x;
  if (k >= MG_MAX_MKFS || !(slots[k].flags & MCP_MKF_PRESENT)) return;
  double bfw[12];
  for (int a = 0; a < 12; ++a) bfw[a] = slots[k].bfw[a];
  ml_mkf_move(X, bfw);
  for (int a = 0; a < 12; ++a) slots[k].bfw[a] = bfw[a];
}

// one lane per table row (gp covers them all); counts: n_refreshed, n_no_rays, n_no_source
__global__ void __launch_bounds__(ML_BLOCK)
k_ml_points(MlXform X, MgRig rig, int n_rows, const MgMkf* __restrict__ slots /* moved */, const MgPoint* __restrict__ gp, const uint8_t* __restrict__ ray_bits,
            const double* __restrict__ rays /* null: no row has any */, PvsPoint* __restrict__ pts, int* __restrict__ counts) {
  const int r = blockIdx.x*ML_BLOCK + threadIdx.x;
  int cls = -1;
  if (r < n_rows) {
    const MgPoint G = gp[r];
    const bool source = ml_has_source(G.src_mkf, G.src_cam, rig.ncam) && (slots[G.src_mkf].flags & MCP_MKF_PRESENT);
    const bool has = rays && ml_bit(ray_bits, r);
    cls = ml_row_class(source, has);
    if (source) {
      double ry[9], bfw[12];
      for (int a = 0; a < 9; ++a) ry[a] = has ? rays[9*(size_t)r + a] : 0.0;
      for (int a = 0; a < 12; ++a) bfw[a] = slots[G.src_mkf].bfw[a];
      PvsPoint P = pts[r];
      ml_row_move(X, rig, G.src_cam, bfw, has, ry, P.world_pos, P.pixel_right_w, P.pixel_down_w);
      for (int a = 0; a < 3; ++a) { pts[r].world_pos[a] = P.world_pos[a]; if (has) { pts[r].pixel_right_w[a] = P.pixel_right_w[a]; pts[r].pixel_down_w[a] = P.pixel_down_w[a]; } }
    }
  }
  for (int q = 0; q < 3; ++q) {
    const unsigned long long m = __ballot(cls == (q == 0 ? ML_ROW_REFRESHED : q == 1 ? ML_ROW_NO_RAYS : ML_ROW_NO_SOURCE));
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counts[q], __popcll(m));
  }
}
#endif  // __HIPCC__ && !ML_HOST_ONLY

}  // namespace mcp
