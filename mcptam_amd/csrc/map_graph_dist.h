// map_graph_dist.h -- the keyframe distances of the map graph (src/KeyFrame.cc:715-747 and 903-927) and SE3::inverse, as __host__ __device__
// bodies with no kernel next to them: map_graph_kernels.h (the select), map_graph_neigh.h (the neighbour queries) and the host twin
// map_graph_neigh_host.cpp all call these, each built without fused multiply-add contraction, so they give the same bits.
#pragma once
#include <cfloat>
#include "ba_device.h"
#include "../../include/mcp_img.h"

namespace mcp {

__host__ __device__ inline void se3_inverse(const Se3& A, Se3& B) {         // TooN SE3::inverse: (R^T, -(R^T t))
  double t[3]; mat3t_vec(A.R, A.t, t);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) B.R[3*r + c] = A.R[3*c + r];
  B.t[0] = -t[0]; B.t[1] = -t[1]; B.t[2] = -t[2];
}

struct MgRig { Se3 cfb[MCP_MAX_FRAME_CAMS]; int ncam; };

__host__ __device__ inline void mg_se3_of12(const double* a, Se3& T) {
  for (int k = 0; k < 9; ++k) T.R[k] = a[k];
  for (int k = 0; k < 3; ++k) T.t[k] = a[9 + k];
}

// KeyFrame::Distance (KeyFrame.cc:715-747) from the two CamFromWorld and mean scene depths; *broken: the value the reference stops the process on
__host__ __device__ inline double mg_kf_distance(const Se3& cfw1, double depth1, const Se3& cfw2, double depth2, double frac, bool* broken) {
  Se3 i1, i2;
  se3_inverse(cfw1, i1); se3_inverse(cfw2, i2);
  const double m1c[3] = {0.0, 0.0, depth1}, m2c[3] = {0.0, 0.0, depth2};
  double m1[3], m2[3];
  se3_apply(i1, m1c, m1); se3_apply(i2, m2c, m2);
  const double d[3] = {i2.t[0] - i1.t[0], i2.t[1] - i1.t[1], i2.t[2] - i1.t[2]};
  const double e[3] = {m2[0] - m1[0], m2[1] - m1[1], m2[2] - m1[2]};
  const double dist = sqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2]) + sqrt(e[0]*e[0] + e[1]*e[1] + e[2]*e[2])*frac;
  *broken = !(dist - dist == 0.0) || dist > 1e10;      // (!isfinite, spelled for both compilers)
  return dist;
}

// MultiKeyFrame::Distance (KeyFrame.cc:903-927): the minimum over the pairs of active keyframes; DBL_MAX when there is no such pair
__host__ __device__ inline double mg_mkf_distance(const MgRig& rig, const double* bfw_a, const uint8_t* act_a, const double* dep_a,
                                                  const double* bfw_b, const uint8_t* act_b, const double* dep_b, double frac, bool* broken) {
  Se3 A, B;
  mg_se3_of12(bfw_a, A); mg_se3_of12(bfw_b, B);
  double best = DBL_MAX;
  *broken = false;
  for (int c1 = 0; c1 < rig.ncam; ++c1) {
    if (!act_a[c1]) continue;
    Se3 w1; se3_compose(rig.cfb[c1], A, w1);
    for (int c2 = 0; c2 < rig.ncam; ++c2) {
      if (!act_b[c2]) continue;
      Se3 w2; se3_compose(rig.cfb[c2], B, w2);
      bool br;
      const double d = mg_kf_distance(w1, dep_a[c1], w2, dep_b[c2], frac, &br);
      if (br) *broken = true;
      if (d < best) best = d;
    }
  }
  return best;
}

}  // namespace mcp
