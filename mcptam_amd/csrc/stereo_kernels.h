// stereo_kernels.h -- MapMakerServerBase::AddStereoMapPoints of one source keyframe and level (src/MapMakerServerBase.cc:411-496, 604-918), gfx950.
//
// mcp_stereo_points (img_api.hip) enqueues on the source keyframe's stream:
//   k_stereo_thin_meas   one thread per candidate: ThinCandidates against the source's measurements at level L / L+1 (:411-446).  They do not
//                        change during the call and the survivors only shrink, so this runs once.
//   per target j:
//     k_stereo_thin_new  (j > 0) ThinCandidates against the points target j-1 created: the earlier ones were checked before.
//     k_stereo_walk      one wavefront per candidate: the arc (:611-723), the probe MapPoint (:726-738), every hypothesis through one fresh finder
//                        (patch_item, MCP_PF_EPI_COARSE semantics, range 3) keeping the three smallest (score, index) matches and the counts,
//                        the selection (:798-825), the refinement of the kept matches on the same finder (MCP_PF_EPI_REFINE), ReprojectPoint
//                        (:123-143) and the new point (:855-887).  Hypotheses are generated inside the walk; nothing is stored per step.
//     k_stereo_commit    one workgroup: the nLimit rule (:486-493) over the candidates in order and the created points, compacted in creation
//                        order, into pinned host memory; the running count stays in device memory for the next target.
// Hand-offs are kernel boundaries on one stream; no workgroup waits for another.
// Where STEREO_HOST_ONLY is defined only the __host__ __device__ bodies appear (the camera, the arc, the pixel vectors, ReprojectPoint): a host
// twin that shares them (map_life_host.cpp) must not define the kernels of img_kernels.h a second time.
#pragma once
#include <cmath>
#ifndef STEREO_HOST_ONLY
#include "img_kernels.h"
#endif
#include "map_graph_dist.h"      // se3_inverse

namespace mcp {

#ifndef STEREO_HOST_ONLY
struct StereoSrcDev { mcp_camera cam; Se3 cfw; const uint8_t* img; int w, h, level; };
struct StereoTargetDev { DevKfView T; const uint8_t* mask0; mcp_camera cam; Se3 cfw; double opa; };
#endif

// TaylorCamera::UnProject (src/TaylorCamera.cc:319-347), the arithmetic of mcp_sbi_se3_from_se2 and the oracle
__host__ __device__ inline void stereo_unproject(const mcp_camera& c, double u, double v, double out[3]) {
  const double det = c.affine[0]*c.affine[3] - c.affine[1]*c.affine[2];
  const double ai[4] = { c.affine[3]/det, -c.affine[1]/det, -c.affine[2]/det, c.affine[0]/det };
  const double dx = u - c.center[0], dy = v - c.center[1];
  const double x = ai[0]*dx + ai[1]*dy, y = ai[2]*dx + ai[3]*dy;
  const double rho = sqrt(x*x + y*y);
  const double p[5] = { c.params[0], 0.0, c.params[1], c.params[2], c.params[3] };
  double z = p[4]; for (int q = 3; q >= 0; --q) z = z*rho + p[q];
  const double n = sqrt(x*x + y*y + z*z);
  out[0] = x/n; out[1] = y/n; out[2] = z/n;
}
__host__ __device__ inline double dot3(const double* a, const double* b) { return a[0]*b[0] + a[1]*b[1] + a[2]*b[2]; }
__host__ __device__ inline void normalize3(double* v) { const double n = sqrt(dot3(v, v)); v[0] /= n; v[1] /= n; v[2] /= n; }   // TooN normalize
__host__ __device__ inline void cross3(const double* a, const double* b, double* o) {
  const double x = a[1]*b[2] - a[2]*b[1], y = a[2]*b[0] - a[0]*b[2], z = a[0]*b[1] - a[1]*b[0]; o[0] = x; o[1] = y; o[2] = z; }
// (se3_inverse: map_graph_dist.h)

// The epipolar arc of one candidate against one target (:611-723) and the probe MapPoint's NC vectors (:726-738).
struct StereoArc {
  int n_hyp;                       // nSteps + 1 hypotheses; 0 = none (v3BetweenEndpoints guard, or a non-finite / unrepresentable step count)
  double step;                     // dAngleStep
  double start_tc[3], dir_tc[3];   // v3RayStart_TC, v3LineDirn_TC
  double rs[2], rd[2];             // v2RayStartInPlane, v2RayDirInPlane
  Se3 wft;                         // se3WorldFromTargetCam
  double root[2];                  // v2RootPos
  double center[3], right[3], down[3];   // the probe's mv3Center_NC, mv3OneRightFromCenter_NC, mv3OneDownFromCenter_NC
};
__host__ __device__ inline void stereo_arc(const mcp_camera& cs, const Se3& Ts, const Se3& Tt, double opa, int level, int cx, int cy, StereoArc& A) {
  const int s = 1 << level;
  A.root[0] = (cx + 0.5)*s - 0.5; A.root[1] = (cy + 0.5)*s - 0.5;                      // LevelZeroPos
  double ray[3]; stereo_unproject(cs, A.root[0], A.root[1], ray);                     // v3Ray_SC
  double tmp[3]; mat3t_vec(Ts.R, ray, tmp); mat3_vec(Tt.R, tmp, A.dir_tc);           // v3LineDirn_TC
  Se3 Si; se3_inverse(Ts, Si); se3_inverse(Tt, A.wft);
  double cc_tc[3], cc_sc[3]; se3_apply(Tt, Si.t, cc_tc); se3_apply(Ts, A.wft.t, cc_sc);
  const double max_epi = M_PI/3, min_epi = 0.05;
  const double sep = sqrt(dot3(cc_sc, cc_sc));
  const double src_angle = acos(dot3(cc_sc, ray)/sep);
  const double min_t = M_PI - src_angle - max_epi, max_t = M_PI - src_angle - min_epi;
  double start = sep*sin(min_t)/sin(max_epi);
  const double end = sep*sin(max_t)/sin(min_epi);
  if (start < 0.2) start = 0.2;
  double re[3];
  for (int k = 0; k < 3; ++k) { A.start_tc[k] = cc_tc[k] + start*A.dir_tc[k]; re[k] = cc_tc[k] + end*A.dir_tc[k]; }
  double a[3] = { A.start_tc[0], A.start_tc[1], A.start_tc[2] }, b[3] = { re[0], re[1], re[2] };
  normalize3(a); normalize3(b);
  const double d[3] = { a[0] - b[0], a[1] - b[1], a[2] - b[2] };
  // the probe (:726-738) -- the same for every target
  stereo_unproject(cs, A.root[0], A.root[1], A.center); normalize3(A.center);
  stereo_unproject(cs, A.root[0] + s, A.root[1] + 0, A.right); normalize3(A.right);
  stereo_unproject(cs, A.root[0] + 0, A.root[1] + s, A.down); normalize3(A.down);
  A.n_hyp = 0; A.step = 0; A.rs[0] = A.rs[1] = A.rd[0] = A.rd[1] = 0;
  if (dot3(d, d) < 0.00000001) return;
  double nrm[3]; cross3(a, b, nrm); normalize3(nrm);
  double J[3]; cross3(nrm, a, J);                                                      // v3PlaneI = a
  const double pb0 = dot3(a, b), pb1 = dot3(J, b);
  const double max_angle = acos(pb0*1 + pb1*0);
  const double q = ceil(max_angle/(opa*s*3));
  // the reference converts with (int): NaN gives INT_MIN on x86, an empty loop; a count past INT_MAX - 1 is not representable either
  if (!(q >= -2147483648.0 && q <= 2147483646.0)) return;
  const int n_steps = (int)q;
  A.step = max_angle/n_steps;
  A.n_hyp = n_steps + 1 > 0 ? n_steps + 1 : 0;
  const double rs0 = dot3(a, A.start_tc), rs1 = dot3(J, A.start_tc), re0 = dot3(a, re), re1 = dot3(J, re);
  A.rs[0] = rs0; A.rs[1] = rs1;
  A.rd[0] = re0 - rs0; A.rd[1] = re1 - rs1;
  const double rn = sqrt(A.rd[0]*A.rd[0] + A.rd[1]*A.rd[1]); A.rd[0] /= rn; A.rd[1] /= rn;
}
// hypothesis i of the arc (:704-723): world position and position in the target camera
__host__ __device__ inline void stereo_hypothesis(const StereoArc& A, int i, double world[3], double tc[3]) {
  const double ang = i*A.step;
  const double c0 = cos(ang), c1 = sin(ang);
  const double alpha = (A.rs[0]*c1 - A.rs[1]*c0)/(A.rd[1]*c0 - A.rd[0]*c1);
  for (int k = 0; k < 3; ++k) tc[k] = A.start_tc[k] + alpha*A.dir_tc[k];
  se3_apply(A.wft, tc, world);
}
// MapPoint::RefreshPixelVectors (src/MapPoint.cc:62-87) with mv3Normal_NC = (0, 0, -1) and the patch source at CamFromWorld Ts
__host__ __device__ inline void stereo_pixel_vectors(const Se3& Ts, const double* center, const double* right, const double* down, const double* world,
                                                     double pr_w[3], double pd_w[3]) {
  const double n[3] = { 0, 0, -1 };
  double pc[3]; se3_apply(Ts, world, pc);
  const double h = fabs(dot3(pc, n));
  const double rc = fabs(dot3(center, n)), rr = fabs(dot3(right, n)), rd = fabs(dot3(down, n));
  double dr[3], dd[3];
  for (int k = 0; k < 3; ++k) { const double c = center[k]*h/rc; dr[k] = right[k]*h/rr - c; dd[k] = down[k]*h/rd - c; }
  mat3t_vec(Ts.R, dr, pr_w); mat3t_vec(Ts.R, dd, pd_w);
}
// ReprojectPoint (:123-143): the right singular vector of the smallest singular value of the 4x4 A, by one-sided (Hestenes) Jacobi on A itself --
// backward stable, A^T A is never formed.  Returns the point in frame B.
__host__ __device__ inline void stereo_reproject(const Se3& AfromB, const double* vA, const double* vB, double out[3]) {
  double M[4][4], V[4][4];                      // M[row][col]
  M[0][0] = -vB[2]; M[0][1] = 0.0;    M[0][2] = vB[0]; M[0][3] = 0.0;
  M[1][0] = 0.0;    M[1][1] = -vB[2]; M[1][2] = vB[1]; M[1][3] = 0.0;
  for (int c = 0; c < 4; ++c) {
    const double p0 = c < 3 ? AfromB.R[c] : AfromB.t[0], p1 = c < 3 ? AfromB.R[3 + c] : AfromB.t[1], p2 = c < 3 ? AfromB.R[6 + c] : AfromB.t[2];
    M[2][c] = vA[0]*p2 - vA[2]*p0;
    M[3][c] = vA[1]*p2 - vA[2]*p1;
  }
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) V[r][c] = (r == c) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int r = 0; r < 4; ++r) { al += M[r][p]*M[r][p]; be += M[r][q]*M[r][q]; ga += M[r][p]*M[r][q]; }
        if (ga == 0.0 || fabs(ga) <= 1e-15*sqrt(al*be)) continue;
        rotated = true;
        const double z = (be - al)/(2*ga);
        const double t = (z >= 0 ? 1.0 : -1.0)/(fabs(z) + hypot(1.0, z));
        const double c = 1/sqrt(1 + t*t), s = c*t;
        for (int r = 0; r < 4; ++r) {
          const double mp = M[r][p], mq = M[r][q]; M[r][p] = c*mp - s*mq; M[r][q] = s*mp + c*mq;
          const double vp = V[r][p], vq = V[r][q]; V[r][p] = c*vp - s*vq; V[r][q] = s*vp + c*vq;
        }
      }
    if (!rotated) break;
  }
  int k = 0; double kn = 0;
  for (int c = 0; c < 4; ++c) { double n2 = 0; for (int r = 0; r < 4; ++r) n2 += M[r][c]*M[r][c]; if (c == 0 || n2 < kn) { kn = n2; k = c; } }
  double v4[4] = { V[0][k], V[1][k], V[2][k], V[3][k] };
  if (v4[3] == 0.0) v4[3] = 0.00001;
  out[0] = v4[0]/v4[3]; out[1] = v4[1]/v4[3]; out[2] = v4[2]/v4[3];
}

// libCVD ir_rounded: half away from zero (restated from memory of libCVD, not checked against its source here)
__host__ __device__ inline int ir_round(double v) { return (int)(v > 0.0 ? v + 0.5 : v - 0.5); }
__host__ __device__ inline bool stereo_busy(int bx, int by, int cx, int cy) {
  const long long dx = (long long)bx - cx, dy = (long long)by - cy;
  return dx*dx + dy*dy < 100;
}

#ifndef STEREO_HOST_ONLY
__device__ inline bool finite3(const double* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// ThinCandidates against the source's measurements (filtered to level L / L+1, as :422-429)
__global__ void __launch_bounds__(256)
k_stereo_thin_meas(int n_cand, const mcp_int2* __restrict__ cand, int n_meas, const mcp_stereo_meas* __restrict__ meas, int level, uint8_t* __restrict__ alive) {
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= n_cand) return;
  const double sc = (double)(1 << level);
  bool good = true;
  for (int m = 0; m < n_meas && good; ++m) {
    const mcp_stereo_meas M = meas[m];
    if (!(M.level == level || M.level == level + 1)) continue;
    if (stereo_busy(ir_round(M.root_pos[0]/sc), ir_round(M.root_pos[1]/sc), cand[i].x, cand[i].y)) good = false;
  }
  alive[i] = good ? 1 : 0;
}
// ThinCandidates before target j > 0 against the points target j-1 created (out[counts[j-1] .. counts[j]), SRC_ROOT at `level`)
__global__ void __launch_bounds__(256)
k_stereo_thin_new(int j, int n_cand, const mcp_int2* __restrict__ cand, int level, const int* __restrict__ counts, const mcp_stereo_point* out,
                  uint8_t* __restrict__ alive) {
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= n_cand || !alive[i]) return;
  const double sc = (double)(1 << level);
  const int k0 = counts[j - 1], k1 = counts[j];
  for (int k = k0; k < k1; ++k)
    if (stereo_busy(ir_round(out[k].root_pos[0]/sc), ir_round(out[k].root_pos[1]/sc), cand[i].x, cand[i].y)) { alive[i] = 0; return; }
}

// one candidate against target j, one wavefront: everything AddPointEpipolar does after the CrossCamera check
__global__ void __launch_bounds__(64)
k_stereo_walk(StereoSrcDev S, const StereoTargetDev* __restrict__ tab, int j, int n_cand, const mcp_int2* __restrict__ cand,
              const uint8_t* __restrict__ alive, mcp_stereo_point* __restrict__ res, uint8_t* __restrict__ outcome /* n_targets x n_cand */) {
  __shared__ uint8_t tmpl[64], jtmpl[64];
  __shared__ double dprod[3][36];
  __shared__ mcp_td_out rec;
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n_cand) return;
  uint8_t* oc = outcome + (size_t)j*n_cand + i;
  if (!alive[i]) { if (lane == 0) *oc = MCP_STEREO_THINNED; return; }
  const StereoTargetDev& T = tab[j];
  const int cx = cand[i].x, cy = cand[i].y;
  StereoArc A;
  stereo_arc(S.cam, S.cfw, T.cfw, T.opa, S.level, cx, cy, A);
  if (A.n_hyp == 0) { if (lane == 0) *oc = MCP_STEREO_NO_ARC; return; }
  DevTdIn P;
  P.src_img = S.img; P.src_w = S.w; P.src_h = S.h; P.center_x = cx; P.center_y = cy; P.fixed = 0;
  PfRegs F; F.valid = 0; F.key = -1; F.bad = 0; F.jvalid = 0; F.lw[0] = F.lw[1] = F.lw[2] = F.lw[3] = 0.0; F.mean = 0.0;    // `PatchFinder finder;`
  Se3 I; se3_identity(I);
  const int key = 1;                           // one MapPoint object for every hypothesis; the finder has seen no other
  // the three smallest (score, index) matches = the first three of the stable sort of :798 (ties by hypothesis index), and the counts
  int ts[3] = { 0x7fffffff, 0x7fffffff, 0x7fffffff }, ti[3] = { -1, -1, -1 }; double tx[3] = { 0, 0, 0 }, ty[3] = { 0, 0, 0 };
  int n_match = 0, n_zero = 0;
  for (int h = 0; h < A.n_hyp; ++h) {
    double tc[3];
    stereo_hypothesis(A, h, P.world_pos, tc);
    if (!finite3(P.world_pos)) continue;       // never form an image index from a non-finite value
    stereo_pixel_vectors(S.cfw, A.center, A.right, A.down, P.world_pos, P.pixel_right_w, P.pixel_down_w);
    patch_item(PF_EPI_COARSE, T.T, T.mask0, T.cam, T.cfw, I, P, key, 0.0, 0.0, F, tmpl, jtmpl, rec, 3, 0, 0, dprod, lane);
    __syncthreads();
    const int found = rec.found, sc = rec.score; const double fx = rec.found_pos[0], fy = rec.found_pos[1];
    __syncthreads();
    if (!found) continue;
    ++n_match; if (sc == 0) ++n_zero;
    int at = 3;                                // h is the largest index so far: it goes after every equal score
    for (int k = 2; k >= 0; --k) if (sc < ts[k]) at = k;
    for (int k = 2; k > at; --k) { ts[k] = ts[k - 1]; ti[k] = ti[k - 1]; tx[k] = tx[k - 1]; ty[k] = ty[k - 1]; }
    if (at < 3) { ts[at] = sc; ti[at] = h; tx[at] = fx; ty[at] = fy; }
  }
  uint8_t code = 0;
  int keep = 0;
  if (n_match == 0) code = MCP_STEREO_NO_MATCH;
  else {
    // scores are >= 0: with best > 0 every later match is above 0.9 best; with best == 0 the positive ones are
    keep = ts[0] > 0 ? n_match : 1 + (n_match - n_zero);
    if (keep > 3) code = MCP_STEREO_TOO_MANY;
    else for (int k = 1; k < keep; ++k) if (abs(ti[k] - ti[0]) > 1) code = MCP_STEREO_INDEX_FAR;
  }
  int win = -1; double sub[2] = { -1, -1 };
  if (!code) {
    for (int k = 0; k < keep && win < 0; ++k) {
      double tc[3];
      stereo_hypothesis(A, ti[k], P.world_pos, tc);
      stereo_pixel_vectors(S.cfw, A.center, A.right, A.down, P.world_pos, P.pixel_right_w, P.pixel_down_w);
      patch_item(PF_EPI_REFINE, T.T, T.mask0, T.cam, T.cfw, I, P, key, tx[k], ty[k], F, tmpl, jtmpl, rec, 3, 10, 0, dprod, lane);
      __syncthreads();
      if (rec.found) { win = k; sub[0] = rec.found_pos[0]; sub[1] = rec.found_pos[1]; }
      __syncthreads();
    }
    if (win < 0) code = MCP_STEREO_NO_SUBPIX;
  }
  if (lane == 0) *oc = code ? code : (uint8_t)MCP_STEREO_CREATED;
  if (code || lane != 0) return;
  // :855-887
  Se3 AB; se3_compose(S.cfw, A.wft, AB);
  double vA[3], vB[3], xb[3];
  stereo_unproject(S.cam, A.root[0], A.root[1], vA);
  stereo_unproject(T.cam, sub[0], sub[1], vB);
  stereo_reproject(AB, vA, vB, xb);
  mcp_stereo_point& R = res[i];
  R.candidate = i; R.target = j; R.hypothesis = ti[win]; R.score = ts[win];
  se3_apply(A.wft, xb, R.world_pos);
  R.root_pos[0] = A.root[0]; R.root_pos[1] = A.root[1]; R.target_pos[0] = sub[0]; R.target_pos[1] = sub[1];
  for (int k = 0; k < 3; ++k) { R.center_nc[k] = A.center[k]; R.one_right_nc[k] = A.right[k]; R.one_down_nc[k] = A.down[k]; }
  stereo_pixel_vectors(S.cfw, A.center, A.right, A.down, R.world_pos, R.pixel_right_w, R.pixel_down_w);
}

// nLimit (:486-493) and compaction for target j, one workgroup.  numSuccess enters as counts[j]; candidate i (surviving) is tried when it is the
// first survivor or when counts[j] + (creations of this target before i) < limit.  Created points go to out[counts[j] + rank] in candidate order.
constexpr int STEREO_COMMIT_NT = 256;
__global__ void __launch_bounds__(STEREO_COMMIT_NT)
k_stereo_commit(int j, int n_cand, int limit, const uint8_t* __restrict__ alive, uint8_t* __restrict__ outcome, const mcp_stereo_point* __restrict__ res,
                int* __restrict__ counts, mcp_stereo_point* out) {
  __shared__ int lds[STEREO_COMMIT_NT/64 + 1];
  __shared__ int first_s;
  const int base = counts[j];
  if (threadIdx.x == 0) first_s = 0x7fffffff;
  __syncthreads();
  for (int i = threadIdx.x; i < n_cand; i += STEREO_COMMIT_NT) if (alive[i]) { atomicMin(&first_s, i); break; }
  __syncthreads();
  const int first = first_s;
  uint8_t* oc = outcome + (size_t)j*n_cand;
  int before = 0, made = 0;
  for (int c0 = 0; c0 < n_cand; c0 += STEREO_COMMIT_NT) {
    const int i = c0 + threadIdx.x;
    const bool live = i < n_cand && alive[i];
    const bool ok = live && oc[i] == MCP_STEREO_CREATED;
    int tot;
    const int r = block_rank(ok, &tot, lds);
    const bool tried = live && (i == first || base + before + r < limit);
    if (live && !tried) oc[i] = MCP_STEREO_PAST_LIMIT;
    const bool keep = ok && tried;
    if (keep) out[base + before + r] = res[i];
    int kt;
    (void)block_rank(keep, &kt, lds);
    made += kt; before += tot;
  }
  if (threadIdx.x == 0) counts[j + 1] = base + made;
}

// mcp_stereo_hypotheses: count, then write, with the walk's own functions
__global__ void __launch_bounds__(256)
k_stereo_hyp_count(mcp_camera cs, Se3 Ts, Se3 Tt, double opa, int level, int n_cand, const mcp_int2* __restrict__ cand, int* __restrict__ n_hyp) {
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= n_cand) return;
  StereoArc A; stereo_arc(cs, Ts, Tt, opa, level, cand[i].x, cand[i].y, A);
  n_hyp[i] = A.n_hyp;
}
__global__ void __launch_bounds__(256)
k_stereo_hyp_fill(mcp_camera cs, Se3 Ts, Se3 Tt, double opa, int level, int n_cand, const mcp_int2* __restrict__ cand, const int* __restrict__ offsets,
                  const mcp_kf* src_handle, mcp_td_in* __restrict__ out) {
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= n_cand) return;
  StereoArc A; stereo_arc(cs, Ts, Tt, opa, level, cand[i].x, cand[i].y, A);
  for (int h = 0; h < A.n_hyp; ++h) {
    mcp_td_in& o = out[offsets[i] + h];
    double tc[3];
    stereo_hypothesis(A, h, o.world_pos, tc);
    stereo_pixel_vectors(Ts, A.center, A.right, A.down, o.world_pos, o.pixel_right_w, o.pixel_down_w);
    o.source_kf = src_handle; o.source_level = level; o.center_x = cand[i].x; o.center_y = cand[i].y; o.fixed = 0;
  }
}

#endif  // STEREO_HOST_ONLY

}  // namespace mcp
