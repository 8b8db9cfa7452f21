// track_cov.h -- the arithmetic of the tracker's pose covariance (src/Tracker.cc:1498-1502, mm6PoseCovariance), __host__ __device__.
//
// One source for the device (k_pose_cov_tiles / k_pose_cov_finish, track_cov_kernels.h) and for the host entry (mcp_track_pose_cov_host):
// the pose the last iteration linearised at, a record's 21 weighted Jacobian products, the wavefront / tile order of their sums as the host
// walks it, and the finish -- WLS<6>::add_prior(100) + add_mJ twice = get_C_inv(), then TooN's SVD<6>::get_pinv() as a cyclic Jacobi
// eigen-decomposition with its condition number 1e9 [3P-memory].  Plain C++ in double; host and device differ only in their math
// libraries (sin, cos of the pose's exponential).
// DEVIATION: the reference linearises at the pose it held before the last update.  The iteration kernels overwrite that pose, so it is
// rebuilt as exp(-mu_last) * refined, which equals it to rounding.
#pragma once
#include "ba_device.h"
#include "track_motion.h"
#include "../../include/mcp_img.h"

namespace mcp {

constexpr int COV_TILE = 256;                // records per tile: one workgroup pass, four wavefronts
constexpr int COV_NPROD = 21;                // lower triangle of the 6 x 6, row-major: (0,0) (1,0) (1,1) (2,0) ...
constexpr double COV_PRIOR = 100.0;          // wls.add_prior(100), Tracker.cc:1441
constexpr double COV_JACOBI_EPS = 2.220446049250313e-16;      // 2^-52
constexpr double COV_PINV_CONDITION = 1e9;   // TooN SVD::get_pinv's default condition number [3P-memory]

// the pose the last fine iteration linearised at: exp(-mu_last) * refined
__host__ __device__ inline void cov_pose_before(const double* refined12, const double* mu_last, double* pose12) {
  double neg[6];
  for (int k = 0; k < 6; ++k) neg[k] = -mu_last[k];
  Se3 E, Rf, P;
  se3_exp(neg, E); se3_of12_hd(refined12, Rf); se3_compose(E, Rf, P);
  se3_to12_hd(P, pose12);
}

// a[0..20] = sum over r = 0, 1 of w Jr[x] Jr[y], y <= x, with Jr = sqrt_inv_noise * row r of the 2 x 6 Jacobian -- k_pose_refine's at its
// re-projecting iterations (img_kernels.h), from the camera derivatives the record holds.  A record that is not found or whose weight is
// zero gives zeros and false.
__host__ __device__ inline bool cov_record_products(const mcp_pose_point& p, double w, const double* pose, const double* cfb_all, double* a) {
  for (int k = 0; k < COV_NPROD; ++k) a[k] = 0.0;
  if (!p.found || w == 0.0) return false;
  const double* cfb = cfb_all + 12*(size_t)p.cam;
  double xb[3], xc[3];
  mat3_vec(pose, p.world_pos, xb); xb[0] += pose[9]; xb[1] += pose[10]; xb[2] += pose[11];
  mat3_vec(cfb, xb, xc); xc[0] += cfb[9]; xc[1] += cfb[10]; xc[2] += cfb[11];
  double dT[3], dP[3]; cam_sphere_deriv(xc, dT, dP);
  double J[12];
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    double mb[3], mc[3]; generator(m, xb, mb); mat3_vec(cfb, mb, mc);
    const double s0 = dT[0]*mc[0] + dT[1]*mc[1] + dT[2]*mc[2], s1 = dP[0]*mc[0] + dP[1]*mc[1] + dP[2]*mc[2];
    J[m] = p.cam_derivs[0]*s0 + p.cam_derivs[1]*s1; J[6 + m] = p.cam_derivs[2]*s0 + p.cam_derivs[3]*s1;
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    double Jr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Jr[k] = p.sqrt_inv_noise*J[6*r + k];
    int q = 0;
#pragma unroll
    for (int x = 0; x < 6; ++x)
#pragma unroll
      for (int y = 0; y <= x; ++y) { a[q] += w*Jr[x]*Jr[y]; ++q; }
  }
  return true;
}

// The tile's partial as the device forms it, walked on the host: the products of records first .. first + COV_TILE - 1 (past n: zeros), 64
// at a time through wave_reduce_scatter32's butterfly (lanes a distance 32 apart first, then 16, 8, 4, 2, 1), the four wavefront sums added
// in wavefront order.  Returns the tile's count of used records.
inline int cov_tile_host(int n, int first, const mcp_pose_point* pts, const double* weights, const double* pose, const double* cfb_all, double* part) {
  int used = 0;
  for (int k = 0; k < COV_NPROD; ++k) part[k] = 0.0;
  for (int wave = 0; wave < COV_TILE/64; ++wave) {
    double v[64][COV_NPROD];
    for (int lane = 0; lane < 64; ++lane) {
      const int i = first + 64*wave + lane;
      if (i < n) used += cov_record_products(pts[i], weights[i], pose, cfb_all, v[lane]) ? 1 : 0;
      else for (int k = 0; k < COV_NPROD; ++k) v[lane][k] = 0.0;
    }
    for (int off = 32; off > 0; off >>= 1)
      for (int lane = 0; lane < off; ++lane)
        for (int k = 0; k < COV_NPROD; ++k) v[lane][k] = v[lane][k] + v[lane + off][k];
    for (int k = 0; k < COV_NPROD; ++k) part[k] += v[0][k];
  }
  return used;
}

// info = sums + 100 I (the prior after the sum), mirrored; cov = its pseudo-inverse.  Cyclic Jacobi: (p, q) is rotated unless
// |a_pq| <= 2^-52 sqrt(a_pp a_qq); the loop ends after a sweep without a rotation, and after MCP_POSE_COV_MAX_SWEEPS sweeps whatever the
// data (out->sweeps: the sweeps that rotated).  Eigenvalue i is kept iff lambda_i 1e9 > lambda_max.  A non-finite entry of info:
// valid = -1, cov / eig / norm_fro zeros.  *out may be pinned host memory: written, never read.  The working set is the caller's (LDS on the
// device: indexed by data, it would otherwise live in scratch).
struct CovWork { double A[36], V[36], inv[6]; int ord[6]; };
__host__ __device__ inline void cov_finish(const double* sums /* 21 */, int n_used, CovWork& W, mcp_track_pose_cov_record* out) {
  double* A = W.A; double* V = W.V; double* inv = W.inv; int* ord = W.ord;
  bool finite = true;
  int q = 0;
  for (int x = 0; x < 6; ++x)
    for (int y = 0; y <= x; ++y) {
      double s = sums[q]; ++q;
      if (x == y) s += COV_PRIOR;
      A[6*x + y] = s; A[6*y + x] = s;
      // (x - x is 0 exactly for every finite x, NaN otherwise)
      if (!(s - s == 0.0)) finite = false;
    }
  for (int k = 0; k < 36; ++k) { out->info[k] = A[k]; V[k] = (k % 7 == 0) ? 1.0 : 0.0; }
  out->n_used = n_used;
  if (!finite) {
    for (int k = 0; k < 36; ++k) out->cov[k] = 0.0;
    for (int k = 0; k < 6; ++k) out->eig[k] = 0.0;
    out->norm_fro = 0.0; out->rank = 0; out->sweeps = 0; out->valid = -1;
    return;
  }
  int sweeps = 0;
  for (int s = 0; s < MCP_POSE_COV_MAX_SWEEPS; ++s) {
    bool rotated = false;
    for (int p = 0; p < 5; ++p)
      for (int r = p + 1; r < 6; ++r) {
        const double apq = A[6*p + r], app = A[7*p], aqq = A[7*r];
        if (fabs(apq) <= COV_JACOBI_EPS*sqrt(app*aqq)) continue;
        rotated = true;
        const double theta = (aqq - app)/(2.0*apq);
        const double t = (theta < 0.0 ? -1.0 : 1.0)/(fabs(theta) + sqrt(theta*theta + 1.0));
        const double c = 1.0/sqrt(t*t + 1.0), sn = t*c;
        A[7*p] = app - t*apq; A[7*r] = aqq + t*apq; A[6*p + r] = 0.0; A[6*r + p] = 0.0;
        for (int k = 0; k < 6; ++k) {
          if (k != p && k != r) {
            const double akp = A[6*k + p], akq = A[6*k + r];
            const double np = c*akp - sn*akq, nq = sn*akp + c*akq;
            A[6*k + p] = np; A[6*p + k] = np; A[6*k + r] = nq; A[6*r + k] = nq;
          }
          const double vkp = V[6*k + p], vkq = V[6*k + r];
          V[6*k + p] = c*vkp - sn*vkq; V[6*k + r] = sn*vkp + c*vkq;
        }
      }
    if (!rotated) break;
    ++sweeps;
  }
  // eigenvalues in descending order (a stable insertion sort of the indices)
  for (int i = 0; i < 6; ++i) {
    int j = i;
    while (j > 0 && A[7*ord[j - 1]] < A[7*i]) { ord[j] = ord[j - 1]; --j; }
    ord[j] = i;
  }
  const double lmax = A[7*ord[0]];
  int rank = 0;
  for (int i = 0; i < 6; ++i) {
    const double l = A[7*ord[i]];
    out->eig[i] = l;
    const bool keep = l*COV_PINV_CONDITION > lmax;
    inv[i] = keep ? 1.0/l : 0.0;
    rank += keep ? 1 : 0;
  }
  double fro = 0.0;
  for (int x = 0; x < 6; ++x)
    for (int y = 0; y <= x; ++y) {
      double s = 0.0;
      for (int i = 0; i < 6; ++i) if (inv[i] != 0.0) s += V[6*x + ord[i]]*inv[i]*V[6*y + ord[i]];
      out->cov[6*x + y] = s; out->cov[6*y + x] = s;
      fro += (x == y ? 1.0 : 2.0)*s*s;
    }
  out->norm_fro = sqrt(fro); out->rank = rank; out->sweeps = sweeps; out->valid = 1;
}

}  // namespace mcp
