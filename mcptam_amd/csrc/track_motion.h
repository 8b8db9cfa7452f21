// track_motion.h -- the arithmetic of the tracker's motion model (src/Tracker.cc:1516-1555, 1687-1749), __host__ __device__.
//
// One source for the device (k_motion_prior / k_motion_update, track_motion_kernels.h) and for the host entries
// (mcp_sbi_se3_from_se2, mcp_track_motion_prior_host, mcp_track_motion_update_host): SmallBlurryImage::SE3fromSE2, SO3 / SE3
// logarithms, Tracker::FindAverageRotation, ApplyMotionModel's prior and UpdateMotionModel's velocity; and the relocaliser's poses
// (k_reloc_align / k_reloc_pick, track_recover_kernels.h; mcp_track_recover_pose_host).  Plain C++ in double;
// host and device differ only in their math libraries (sin, cos, asin, acos).
#pragma once
#include "ba_device.h"
#include "img_kernels.h"
#include "../../include/mcp_img.h"

namespace mcp {

constexpr int MOTION_AVG_ROUNDS = 32;        // cap of the averaging loop (the reference's while(1) has none)
constexpr double MOTION_AVG_EPS = 1e-3;      // dEpsilon, Tracker.cc:1725

// SmallBlurryImage::SE3fromSE2 (:250-310): two points, three Gauss-Newton steps on SO3
__host__ __device__ inline void sbi_se3_from_se2(const double* se2, const mcp_camera* cs, const mcp_camera* ct, double* R) {
  const double c[2] = { SBI_W/2, SBI_H/2 };
  const double off[2][2] = { { 5, 0 }, { -5, 0 } };
  double turned[2][2], orig[2][3];
  for (int i = 0; i < 2; ++i) {
    turned[i][0] = c[0] + se2[0]*off[i][0] + se2[1]*off[i][1] + se2[4];
    turned[i][1] = c[1] + se2[2]*off[i][0] + se2[3]*off[i][1] + se2[5];
    // TaylorCamera::UnProject, TaylorCamera.cc:319-347
    const double det = ct->affine[0]*ct->affine[3] - ct->affine[1]*ct->affine[2];
    const double ai[4] = { ct->affine[3]/det, -ct->affine[1]/det, -ct->affine[2]/det, ct->affine[0]/det };
    const double dx = c[0] + off[i][0] - ct->center[0], dy = c[1] + off[i][1] - ct->center[1];
    const double x = ai[0]*dx + ai[1]*dy, y = ai[2]*dx + ai[3]*dy;
    const double rho = sqrt(x*x + y*y);
    const double p[5] = { ct->params[0], 0.0, ct->params[1], ct->params[2], ct->params[3] };
    double z = p[4]; for (int q = 3; q >= 0; --q) z = z*rho + p[q];
    const double n = sqrt(x*x + y*y + z*z);
    orig[i][0] = x/n; orig[i][1] = y/n; orig[i][2] = z/n;
  }
  double so3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
  for (int it = 0; it < 3; ++it) {
    double C[9] = { 10, 0, 0, 0, 10, 0, 0, 0, 10 }, v[3] = { 0, 0, 0 };
    for (int i = 0; i < 2; ++i) {
      double cam[3]; mat3_vec(so3, orig[i], cam);
      Projection P; cam_project<true>(*cs, cam, P);
      const double err[2] = { turned[i][0] - P.u, turned[i][1] - P.v };
      double dT[3], dP[3]; cam_sphere_deriv(cam, dT, dP);
      double J[2][3];
      for (int m = 0; m < 3; ++m) {
        double mot[3] = { 0, 0, 0 };
        mot[(m + 1)%3] = -cam[(m + 2)%3]; mot[(m + 2)%3] = cam[(m + 1)%3];
        const double sm[2] = { dT[0]*mot[0] + dT[1]*mot[1] + dT[2]*mot[2], dP[0]*mot[0] + dP[1]*mot[1] + dP[2]*mot[2] };
        J[0][m] = P.D[0]*sm[0] + P.D[1]*sm[1]; J[1][m] = P.D[2]*sm[0] + P.D[3]*sm[1];
      }
      for (int r = 0; r < 2; ++r) for (int a = 0; a < 3; ++a) { v[a] += J[r][a]*err[r]; for (int b = 0; b < 3; ++b) C[3*a + b] += J[r][a]*J[r][b]; }
    }
    const double c00 = C[4]*C[8] - C[5]*C[7], c01 = C[5]*C[6] - C[3]*C[8], c02 = C[3]*C[7] - C[4]*C[6];
    const double id = 1.0/(C[0]*c00 + C[1]*c01 + C[2]*c02);
    const double Ci[9] = { c00*id, (C[2]*C[7] - C[1]*C[8])*id, (C[1]*C[5] - C[2]*C[4])*id,
                           c01*id, (C[0]*C[8] - C[2]*C[6])*id, (C[2]*C[3] - C[0]*C[5])*id,
                           c02*id, (C[1]*C[6] - C[0]*C[7])*id, (C[0]*C[4] - C[1]*C[3])*id };
    double mu[3]; mat3_vec(Ci, v, mu);
    double E[9], Rn[9]; so3_exp(mu, E); mat3_mul(E, so3, Rn);
    for (int k = 0; k < 9; ++k) so3[k] = Rn[k];
  }
  for (int k = 0; k < 9; ++k) R[k] = so3[k];
}

// TooN SO3<>::ln [3P-memory]: the antisymmetric part scaled by asin below 45 degrees, by acos up to 135 degrees; beyond, the axis comes from
// the largest column of the symmetric part (the antisymmetric part vanishes towards pi), its sign from the antisymmetric part
__host__ __device__ inline void so3_ln(const double* R, double* w) {
  const double sqrt1_2 = 0.70710678118654752440;
  const double cos_angle = (R[0] + R[4] + R[8] - 1.0)*0.5;
  w[0] = (R[7] - R[5])/2; w[1] = (R[2] - R[6])/2; w[2] = (R[3] - R[1])/2;
  const double sin_angle_abs = sqrt(w[0]*w[0] + w[1]*w[1] + w[2]*w[2]);
  if (cos_angle > sqrt1_2) {
    if (sin_angle_abs > 0) { const double f = asin(sin_angle_abs)/sin_angle_abs; w[0] *= f; w[1] *= f; w[2] *= f; }
  } else if (cos_angle > -sqrt1_2) {
    const double f = acos(cos_angle)/sin_angle_abs; w[0] *= f; w[1] *= f; w[2] *= f;
  } else {
    const double angle = 3.14159265358979323846 - asin(sin_angle_abs);
    const double d0 = R[0] - cos_angle, d1 = R[4] - cos_angle, d2 = R[8] - cos_angle;
    double r2[3];
    if (d0*d0 > d1*d1 && d0*d0 > d2*d2) { r2[0] = d0; r2[1] = (R[3] + R[1])/2; r2[2] = (R[2] + R[6])/2; }
    else if (d1*d1 > d2*d2) { r2[0] = (R[3] + R[1])/2; r2[1] = d1; r2[2] = (R[7] + R[5])/2; }
    else { r2[0] = (R[2] + R[6])/2; r2[1] = (R[7] + R[5])/2; r2[2] = d2; }
    if (r2[0]*w[0] + r2[1]*w[1] + r2[2]*w[2] < 0) { r2[0] = -r2[0]; r2[1] = -r2[1]; r2[2] = -r2[2]; }
    const double f = angle/sqrt(r2[0]*r2[0] + r2[1]*r2[1] + r2[2]*r2[2]);
    w[0] = f*r2[0]; w[1] = f*r2[1]; w[2] = f*r2[2];
  }
}

// TooN SE3<>::ln [3P-memory]: v = (t, w) with exp(v) = T; the translation is rotated back by half the angle and rescaled
__host__ __device__ inline void se3_ln(const Se3& T, double* v) {
  double rot[3]; so3_ln(T.R, rot);
  const double th2 = rot[0]*rot[0] + rot[1]*rot[1] + rot[2]*rot[2], theta = sqrt(th2);
  double shtot = 0.5;
  if (theta > 0.00001) shtot = sin(theta/2)/theta;
  const double half[3] = { rot[0]*-0.5, rot[1]*-0.5, rot[2]*-0.5 };
  double H[9], rt[3]; so3_exp(half, H); mat3_vec(H, T.t, rt);
  const double dot = T.t[0]*rot[0] + T.t[1]*rot[1] + T.t[2]*rot[2];
  const double k = theta > 0.001 ? dot*(1 - 2*shtot)/th2 : dot/24;
  for (int i = 0; i < 3; ++i) { v[i] = (rt[i] - rot[i]*k)/(2*shtot); v[3 + i] = rot[i]; }
}

__host__ __device__ inline void se3_of12_hd(const double* a, Se3& T) { for (int k = 0; k < 9; ++k) T.R[k] = a[k]; for (int k = 0; k < 3; ++k) T.t[k] = a[9 + k]; }
__host__ __device__ inline void se3_to12_hd(const Se3& T, double* a) { for (int k = 0; k < 9; ++k) a[k] = T.R[k]; for (int k = 0; k < 3; ++k) a[9 + k] = T.t[k]; }

// Tracker::FindAverageRotation (:1723-1749), the geodesic L2 mean of n >= 1 axis-angle rotations, in the order given.  One round = one
// evaluation of the mean residual r; the loop ends when r.r < eps^2 or after MOTION_AVG_ROUNDS rounds.  Returns the rounds.
__host__ __device__ inline int average_rotation(int n, const double (*rots)[3], double* mean) {
  double R[9]; so3_exp(rots[0], R);
  int rounds = 0;
  while (rounds < MOTION_AVG_ROUNDS) {
    double r[3] = { 0, 0, 0 };
    for (int i = 0; i < n; ++i) {
      double E[9], M[9], l[3]; so3_exp(rots[i], E); mat3t_mul(R, E, M); so3_ln(M, l);
      r[0] += l[0]; r[1] += l[1]; r[2] += l[2];
    }
    const double s = 1.0/n;
    r[0] *= s; r[1] *= s; r[2] *= s;
    ++rounds;
    if (r[0]*r[0] + r[1]*r[1] + r[2]*r[2] < MOTION_AVG_EPS*MOTION_AVG_EPS) break;
    double E[9]; so3_exp(r, E); mat3_mul(R, E, R);
  }
  so3_ln(R, mean);
  return rounds;
}

// does camera c take part in CalcSBIRotation (:1695)?
__host__ __device__ inline bool motion_cam_used(const mcp_track_motion_params& p, int c) { return p.apply && p.use_rotation_estimator && p.cam_good[c]; }

// CalcSBIRotation's per-camera step (:1701-1705): the SE2 as a rotation of the 40x30 camera, its logarithm carried into the base frame.
// An SE2 that is exactly the identity (a camera's first frame: its two SBIs are one) gives exactly zero.
__host__ __device__ inline void motion_cam_rotation(const double* se2, const mcp_camera* cam_sbi, const double* cfb12, double* rot) {
  if (se2[0] == 1.0 && se2[1] == 0.0 && se2[2] == 0.0 && se2[3] == 1.0 && se2[4] == 0.0 && se2[5] == 0.0) { rot[0] = rot[1] = rot[2] = 0.0; return; }
  double R[9], w[3];
  sbi_se3_from_se2(se2, cam_sbi, cam_sbi, R);
  so3_ln(R, w);
  mat3t_vec(cfb12, w, rot);                  // mse3CamFromBase.get_rotation().inverse() * v3AxisAngle_Cam
}

// ApplyMotionModel (:1516-1536) from the rotations of the cameras (cam_rot[c] is read where motion_cam_used): fills start, prior, cam_rot,
// sbi_rot, n_used and avg_rounds of *out (which may be pinned host memory: written, never read) and returns the prior in prior12.
__host__ __device__ inline void motion_prior(int ncam, const double (*cam_rot)[3], const mcp_track_motion_params& p, const double* start12, mcp_track_motion* out,
                                             double* prior12) {
  double used[MCP_MAX_FRAME_CAMS][3];
  int n_used = 0;
  for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) {
    const bool u = c < ncam && motion_cam_used(p, c);
    for (int k = 0; k < 3; ++k) { out->cam_rot[c][k] = u ? cam_rot[c][k] : 0.0; if (u) used[n_used][k] = cam_rot[c][k]; }
    if (u) ++n_used;
  }
  double mean[3] = { 0, 0, 0 };
  const int rounds = n_used > 0 ? average_rotation(n_used, used, mean) : 0;
  out->n_used = n_used; out->avg_rounds = rounds;
  for (int k = 0; k < 3; ++k) out->sbi_rot[k] = mean[k];
  for (int k = 0; k < 12; ++k) { out->start[k] = start12[k]; prior12[k] = start12[k]; }
  if (p.apply) {
    double v6[6];
    for (int k = 0; k < 6; ++k) v6[k] = p.velocity[k]*p.dt;
    if (n_used > 0) for (int k = 0; k < 3; ++k) v6[3 + k] = mean[k];
    Se3 E, S, P;
    se3_exp(v6, E); se3_of12_hd(start12, S); se3_compose(E, S, P);
    se3_to12_hd(P, prior12);
  }
  for (int k = 0; k < 12; ++k) out->prior[k] = prior12[k];
}

// UpdateMotionModel (:1539-1547): v_new = ln(refined * start^-1) / dt, velocity = 0.9 (0.5 v_new + 0.5 velocity_in); apply == 0: no motion
// model ran -- v_new zeros, the velocity as given
__host__ __device__ inline void motion_update(const double* start12, const double* refined12, const mcp_track_motion_params& p, double* v_new, double* velocity) {
  if (!p.apply) { for (int k = 0; k < 6; ++k) { v_new[k] = 0.0; velocity[k] = p.velocity[k]; } return; }
  Se3 S, Rf, Si, D;
  se3_of12_hd(start12, S); se3_of12_hd(refined12, Rf);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Si.R[3*i + j] = S.R[3*j + i];
  double rt[3]; mat3t_vec(S.R, S.t, rt);
  Si.t[0] = -rt[0]; Si.t[1] = -rt[1]; Si.t[2] = -rt[2];
  se3_compose(Rf, Si, D);
  double v[6]; se3_ln(D, v);
  for (int k = 0; k < 6; ++k) { v_new[k] = v[k]/p.dt; velocity[k] = (0.5*v_new[k] + 0.5*p.velocity[k])*0.9; }
}

// Relocaliser::AttemptRecovery's pose (src/Relocaliser.cc:80-82): mse3Best = SE3fromSE2(se2, cam, cam) * CamFromWorld of the best keyframe,
// the rotation with zero translation, both cameras the 40x30 one of the current camera (ScoreKFs looks at keyframes of that camera only).
// An SE2 that is exactly the identity gives exactly the keyframe's pose.
__host__ __device__ inline void recover_cam_pose(const double* se2, const mcp_camera* cam_sbi, const double* cfw_best12, double* cam_pose12) {
  if (se2[0] == 1.0 && se2[1] == 0.0 && se2[2] == 0.0 && se2[3] == 1.0 && se2[4] == 0.0 && se2[5] == 0.0) {
    for (int k = 0; k < 12; ++k) cam_pose12[k] = cfw_best12[k];
    return;
  }
  Se3 Rr, K, P;
  sbi_se3_from_se2(se2, cam_sbi, cam_sbi, Rr.R);
  Rr.t[0] = Rr.t[1] = Rr.t[2] = 0.0;
  se3_of12_hd(cfw_best12, K); se3_compose(Rr, K, P);
  se3_to12_hd(P, cam_pose12);
}

// Tracker::AttemptRecovery's base pose (src/Tracker.cc:538): mse3CamFromBase.inverse() * se3Best
__host__ __device__ inline void recover_base_pose(const double* cfb12, const double* cam_pose12, double* bfw12) {
  Se3 C, Ci, P, B;
  se3_of12_hd(cfb12, C); se3_of12_hd(cam_pose12, P);
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Ci.R[3*i + j] = C.R[3*j + i];
  double rt[3]; mat3t_vec(C.R, C.t, rt);
  Ci.t[0] = -rt[0]; Ci.t[1] = -rt[1]; Ci.t[2] = -rt[2];
  se3_compose(Ci, P, B);
  se3_to12_hd(B, bfw12);
}

}  // namespace mcp
