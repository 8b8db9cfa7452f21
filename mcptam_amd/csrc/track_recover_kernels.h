// track_recover_kernels.h -- the relocaliser inside the one-call recovery frame (mcp_track_frame_recover, include/mcp_img.h), gfx950.
//
//   k_reloc_make    Relocaliser::AttemptRecovery's SmallBlurryImage of the current frame (src/Relocaliser.cc:63-67): one workgroup per
//                   camera, sbi_make_body into the target handle's own SBI (k_sbi_make's bits)
//   k_reloc_score   Relocaliser::ScoreKFs (:92-120): a workgroup (one wavefront) per RELOC_TILE candidates.  The candidates' templates
//                   pass through LDS in tiles of RELOC_TILE floats: the wavefront reads RELOC_TILE consecutive floats of one candidate
//                   per load, the tile's rows are RELOC_ROW = RELOC_TILE + 1 floats apart, and lane i then walks row i -- lane i's k-th
//                   read is on bank (i + k) mod 64, no two lanes of a half-wave on one bank.  The loads of tile k + 1 are issued before
//                   tile k is summed, unconditionally and with no wait between them.  Lane i adds candidate i's elements in raster order
//                   with sbi_zmssd_step, k_sbi_score's statement: the scores carry mcp_sbi_score's bits.  LDS: 16.6 KB + 2.1 KB
//   k_reloc_align   per camera: the first smallest score among the camera's candidates (an exact min over (score bits, list index)),
//                   sbi_iterate_body against the winner (k_sbi_iterate's bits), SE3fromSE2 and the product with the winner's pose on
//                   thread 0 (track_motion.h: recover_cam_pose)
//   k_reloc_pick    Tracker::AttemptRecovery (src/Tracker.cc:526-552): the first camera in order that recovered gives BaseFromWorld,
//                   which replaces the pose in the parameter block every later kernel of the submission reads; the gate word tells
//                   k_pvs_mark_gated (pvs_kernels.h) whether there is anything to track; the report goes to pinned memory
// No kernel waits on another workgroup; every loop is bounded by ncand, ncam or SBI_N.
#pragma once
#include "track_motion.h"
#include "track_motion_kernels.h"

namespace mcp {

struct RelocCand {                   // one entry of the candidate list as uploaded (120 bytes)
  const float* templ;                // null: skipped (NULL, not a live keyframe, or no SBI)
  const float* jacs;
  int cam, pad;
  double cfw[12];                    // the keyframe's CamFromWorld
};
struct RelocMakeCam { const uint8_t* img; int w, h; uint8_t* small_img; float* templ; float* jacs; };
struct RelocMakeArgs { RelocMakeCam c[MCP_MAX_FRAME_CAMS]; };
struct RelocCurArgs { const float* templ[MCP_MAX_FRAME_CAMS]; };      // the cameras' current templates (the handles' SBIs)
struct RelocCamOut {                 // what k_reloc_align leaves per camera
  double se2[6], align_score, best_zmssd, cam_pose[12];
  int best, pad;
};
constexpr int RELOC_TILE = 64, RELOC_ROW = RELOC_TILE + 1, RELOC_NT = (SBI_N + RELOC_TILE - 1)/RELOC_TILE;
constexpr double RELOC_SKIPPED = 1.7976931348623157e308;      // DBL_MAX, as k_sbi_score

__global__ void __launch_bounds__(256)
k_reloc_make(RelocMakeArgs a, const SbiTables* __restrict__ tabs) {
  __shared__ float A[SBI_N], B[SBI_N];
  __shared__ unsigned int sum4[4];
  const RelocMakeCam& C = a.c[blockIdx.x];
  sbi_make_body(C.img, C.w, C.h, tabs[blockIdx.x], C.small_img, C.templ, C.jacs, A, B, sum4);
}

__global__ void __launch_bounds__(RELOC_TILE)
k_reloc_score(int ncand, int ncam, const RelocCand* __restrict__ cands, RelocCurArgs cur, double* __restrict__ scores /* ncand */,
              double* __restrict__ h_scores /* pinned, ncand, or null */) {
  __shared__ float tile[RELOC_TILE*RELOC_ROW];
  __shared__ float curt[MCP_MAX_FRAME_CAMS*RELOC_ROW];
  typedef const __attribute__((address_space(1))) float* GlobalFloats;      // (a pointer read from memory is generic to the compiler: say that it is global)
  const int l = threadIdx.x, g = blockIdx.x*RELOC_TILE + l;
  const float* mine = nullptr; int cam = 0;
  if (g < ncand) { mine = cands[g].templ; cam = cands[g].cam; }
  // a skipped entry, or a lane past the list, reads camera 0's current template instead (always there); its sum is thrown away below
  const unsigned long long bits = (unsigned long long)(mine ? mine : cur.templ[0]);
  const int lo = (int)(unsigned int)bits, hi = (int)(unsigned int)(bits >> 32);
  float r[RELOC_TILE], rc[MCP_MAX_FRAME_CAMS];
  // the wavefront's loads of one tile: RELOC_TILE consecutive floats of each candidate (its pointer broadcast from its lane: every lane of
  // the wavefront is active here), and of each camera's current template; no branch and no wait between them.  The last tile is short: its
  // lanes past SBI_N read the last element again, and the sums stop at the tile's length
  auto load = [&](int t) {
    const int p = min(t*RELOC_TILE + l, SBI_N - 1);
#pragma unroll
    for (int j = 0; j < RELOC_TILE; ++j) {
      const unsigned long long q = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(hi, j) << 32) | (unsigned int)__builtin_amdgcn_readlane(lo, j);
      r[j] = ((GlobalFloats)q)[p];
    }
#pragma unroll
    for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) rc[c] = cur.templ[c < ncam ? c : 0][p];
  };
  load(0);
  double ssd = 0.0;
  for (int t = 0; t < RELOC_NT; ++t) {
#pragma unroll
    for (int j = 0; j < RELOC_TILE; ++j) tile[j*RELOC_ROW + l] = r[j];
#pragma unroll
    for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) curt[c*RELOC_ROW + l] = rc[c];
    __syncthreads();
    if (t + 1 < RELOC_NT) load(t + 1);
    const int len = min(RELOC_TILE, SBI_N - t*RELOC_TILE);
    const float* mt = tile + l*RELOC_ROW; const float* ct = curt + cam*RELOC_ROW;
    for (int k = 0; k < len; ++k) sbi_zmssd_step(ssd, ct[k], mt[k]);
    __syncthreads();
  }
  if (g < ncand) {
    const double s = mine ? ssd : RELOC_SKIPPED;
    scores[g] = s;
    if (h_scores) h_scores[g] = s;
  }
}

// LDS: k_frame_sbi's 42 KB and 3 KB for the argmin
__global__ void __launch_bounds__(256)
k_reloc_align(int ncand, const RelocCand* __restrict__ cands, const double* __restrict__ scores, RelocCurArgs cur, const mcp_camera* __restrict__ cams_sbi,
              int iterations, RelocCamOut* __restrict__ out /* ncam */) {
  __shared__ float Tm[SBI_N], warped[SBI_N];
  __shared__ double X[6], red[256][SBI_RED], st[8], o8[8];
  __shared__ unsigned long long kbits[256];
  __shared__ int kidx[256];
  const int t = threadIdx.x, c = blockIdx.x;
  // ScoreKFs' "first smallest": scores are >= +0, so their bit patterns order as the doubles do; a skipped entry (DBL_MAX) and a score
  // that is not below DBL_MAX never win (dSSD < mdBestScore, Relocaliser.cc:113)
  const unsigned long long none = (unsigned long long)__double_as_longlong(RELOC_SKIPPED);
  unsigned long long kb = none; int ki = 0x7fffffff;
  for (int i = t; i < ncand; i += 256) {
    if (cands[i].cam != c || !cands[i].templ) continue;
    const unsigned long long b = (unsigned long long)__double_as_longlong(scores[i]);
    if (b < kb) { kb = b; ki = i; }      // (i rises: an equal score later in the list does not replace)
  }
  kbits[t] = kb; kidx[t] = ki;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      const unsigned long long b = kbits[t + s]; const int i = kidx[t + s];
      if (b < kbits[t] || (b == kbits[t] && i < kidx[t])) { kbits[t] = b; kidx[t] = i; }
    }
    __syncthreads();
  }
  const int best = kbits[0] < none ? kidx[0] : -1;
  RelocCamOut& O = out[c];
  if (best >= 0) sbi_iterate_body(cur.templ[c], cands[best].templ, cands[best].jacs, iterations, o8, Tm, warped, X, red, st);
  __syncthreads();
  if (t == 0) {
    O.best = best; O.pad = 0;
    if (best >= 0) {
      double se2[6];
      for (int k = 0; k < 6; ++k) { se2[k] = o8[k]; O.se2[k] = se2[k]; }
      O.align_score = o8[6];
      O.best_zmssd = __longlong_as_double((long long)kbits[0]);
      double pose[12];
      recover_cam_pose(se2, cams_sbi + c, cands[best].cfw, pose);
      for (int k = 0; k < 12; ++k) O.cam_pose[k] = pose[k];
    } else {
      for (int k = 0; k < 6; ++k) O.se2[k] = 0.0;
      O.align_score = 0.0; O.best_zmssd = 0.0;
      for (int k = 0; k < 12; ++k) O.cam_pose[k] = 0.0;
    }
  }
}

__global__ void __launch_bounds__(64)
k_reloc_pick(int ncam, const RelocCamOut* __restrict__ per_cam, const double* __restrict__ cfb, double max_score, double* __restrict__ pm /* the pose slot */,
             int* __restrict__ gate, mcp_track_recover* __restrict__ out /* pinned */) {
  if (threadIdx.x != 0) return;
  int cam = -1;
  for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) {
    const bool live = c < ncam;
    out->best[c] = live ? per_cam[c].best : -1;
    out->best_zmssd[c] = live ? per_cam[c].best_zmssd : 0.0;
    out->align_score[c] = live ? per_cam[c].align_score : 0.0;
    for (int k = 0; k < 6; ++k) out->se2[c][k] = live ? per_cam[c].se2[k] : 0.0;
    for (int k = 0; k < 12; ++k) out->cam_pose[c][k] = live ? per_cam[c].cam_pose[k] : 0.0;
    if (live && cam < 0 && per_cam[c].best >= 0 && per_cam[c].align_score < max_score) cam = c;      // dScore < sdRecoveryMaxScore, Relocaliser.cc:84
  }
  double bfw[12];
  if (cam >= 0) {
    double pose[12];
    for (int k = 0; k < 12; ++k) pose[k] = per_cam[cam].cam_pose[k];
    recover_base_pose(cfb + 12*cam, pose, bfw);
    for (int k = 0; k < 12; ++k) pm[k] = bfw[k];
  } else {
    for (int k = 0; k < 12; ++k) bfw[k] = pm[k];
  }
  for (int k = 0; k < 12; ++k) out->base_from_world[k] = bfw[k];
  out->recovered = cam >= 0 ? 1 : 0; out->cam = cam;
  *gate = cam >= 0 ? 1 : 0;
}

}  // namespace mcp
