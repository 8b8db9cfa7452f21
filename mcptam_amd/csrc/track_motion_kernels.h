// track_motion_kernels.h -- the tracker's motion model inside the one-call frame (mcp_track_frame_motion, include/mcp_img.h), gfx950.
//
//   k_frame_sbi      Tracker::TrackFrameSetup's SmallBlurryImages (src/Tracker.cc:319-330) and CalcSBIRotation's alignment (:1698-1700):
//                    one workgroup per camera makes this frame's SBI from level 0 of the target (sbi_make_body: k_sbi_make's bits) and
//                    aligns it against the camera's last SBI (sbi_iterate_body: k_sbi_iterate's bits) with the template still in LDS
//   k_motion_prior   SE3fromSE2 + ln per camera (one lane each), FindAverageRotation and ApplyMotionModel on lane 0 (:1516-1536,
//                    1701-1749): the prior replaces the pose in the parameter block every later kernel of the submission reads
//   k_motion_update  UpdateMotionModel (:1539-1547) from the pose the fine iterations left in the parameter block
// The arithmetic of the last two is track_motion.h's (__host__ __device__: mcp_track_motion_prior_host / _update_host run the same
// source).  No kernel loops on data: the averaging ends after MOTION_AVG_ROUNDS rounds at the latest.
#pragma once
#include "track_motion.h"

namespace mcp {

struct SbiSet { float templ[SBI_N]; float jacs[2*SBI_N]; uint8_t small_img[SBI_N]; };      // one SmallBlurryImage: mcp_kf_get_sbi's three layouts
struct FrameSbiCam {
  const uint8_t* img; int w, h;      // level 0 of the target
  int first;                         // the camera index has no SBI yet: `last` is written too and nothing is aligned
  int align;                         // the camera takes part in CalcSBIRotation
  SbiSet* cur; SbiSet* last;
};
struct FrameSbiArgs { FrameSbiCam c[MCP_MAX_FRAME_CAMS]; };
struct MotionFirst { int v[MCP_MAX_FRAME_CAMS]; };
struct Pose12 { double v[12]; };

// LDS: A / B of the make step are Tm / warped of the alignment (9.6 KB), the reduction scratch 32 KB: 42.5 KB in all
__global__ void __launch_bounds__(256)
k_frame_sbi(FrameSbiArgs a, const SbiTables* __restrict__ tabs, int iterations, double* __restrict__ out /* ncam x 8: se2[6], score, 0 */) {
  __shared__ float A[SBI_N], B[SBI_N];
  __shared__ unsigned int sum4[4];
  __shared__ double X[6], red[256][SBI_RED], st[8];
  const int t = threadIdx.x;
  const FrameSbiCam& C = a.c[blockIdx.x];
  sbi_make_body(C.img, C.w, C.h, tabs[blockIdx.x], C.cur->small_img, C.cur->templ, C.cur->jacs, A, B, sum4);
  __syncthreads();
  double* o = out + 8*blockIdx.x;
  if (C.first) {
    // "make both this frame and last frame's SBI's the same" (:321-323): every thread copies the entries it wrote itself
    for (int i = t; i < SBI_N; i += 256) {
      C.last->small_img[i] = C.cur->small_img[i]; C.last->templ[i] = C.cur->templ[i];
      C.last->jacs[2*i] = C.cur->jacs[2*i]; C.last->jacs[2*i + 1] = C.cur->jacs[2*i + 1];
    }
  }
  if (C.align && !C.first) sbi_iterate_body(nullptr, C.last->templ, C.last->jacs, iterations, o, A, B, X, red, st);
  else if (t < 8) o[t] = (C.align && (t == 0 || t == 3)) ? 1.0 : 0.0;      // an SBI against itself: the identity, score 0; not aligned: zeros
  if (t == 7) o[7] = 0.0;
}

__global__ void __launch_bounds__(64)
k_motion_prior(int ncam, const double* __restrict__ se2s /* ncam x 8 */, MotionFirst first, const mcp_camera* __restrict__ cams_sbi, const double* __restrict__ cfb,
               double* __restrict__ pm /* the pose slot: start in, prior out */, mcp_track_motion_params p, mcp_track_motion* __restrict__ out /* pinned */) {
  __shared__ double rot[MCP_MAX_FRAME_CAMS][3];
  const int c = threadIdx.x;
  if (c < MCP_MAX_FRAME_CAMS) {
    const bool live = c < ncam;
    for (int k = 0; k < 6; ++k) out->se2[c][k] = live ? se2s[8*c + k] : 0.0;
    out->sbi_score[c] = live ? se2s[8*c + 6] : 0.0;
    out->first_frame[c] = live ? first.v[c] : 0;
    rot[c][0] = rot[c][1] = rot[c][2] = 0.0;
    if (live && motion_cam_used(p, c)) motion_cam_rotation(se2s + 8*c, cams_sbi + c, cfb + 12*c, rot[c]);
  }
  __syncthreads();
  if (c == 0) {
    double start[12], prior[12];
    for (int k = 0; k < 12; ++k) start[k] = pm[k];
    motion_prior(ncam, rot, p, start, out, prior);
    if (p.apply) for (int k = 0; k < 12; ++k) pm[k] = prior[k];
  }
}

__global__ void __launch_bounds__(64)
k_motion_update(const double* __restrict__ pm /* the refined pose */, Pose12 start, mcp_track_motion_params p, mcp_track_motion* __restrict__ out /* pinned */) {
  if (threadIdx.x != 0) return;
  double v_new[6], vel[6];
  motion_update(start.v, pm, p, v_new, vel);
  for (int k = 0; k < 6; ++k) { out->v_new[k] = v_new[k]; out->velocity[k] = vel[k]; }
}

}  // namespace mcp
