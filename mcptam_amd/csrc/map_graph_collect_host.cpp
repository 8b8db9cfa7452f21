// mcp_map_collect_nearest_host (include/mcp_img.h): the co-visible points of the nearest keyframe (map_graph_collect.h) from host arrays.
// Host code only: the unit is compiled as the host half of a HIP source, as map_graph_neigh_host.cpp, so that the __host__ __device__ bodies
// it shares with the kernels (the candidate rule, the distance of map_graph_dist.h, the order, the entry rule, the bit count) are the very
// text the device runs, and without fused multiply-add contraction, so that they give the device's bits.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#define MGCL_HOST_ONLY
#include "map_graph_collect.h"

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int collect_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }

extern "C" int mcp_map_collect_nearest_host(const double bfw[12], const double* cur_cfb, const mcp_collect_params* p, int ncam, const double* cfb, int n_slots,
                                            const double* mkf_bfw, const int* mkf_flags, const uint8_t* act, const double* dep, int n_rows, int n_store, const int* ms_mkf,
                                            const int* ms_cam, const int* ms_row, const uint8_t* ms_alive, mcp_collect_report* rep, uint8_t* near) {
  const std::string who = "mcp_map_collect_nearest_host";
  if (!bfw || !p || !rep) return collect_fail(who + ": NULL pose, params or report");
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !cfb || n_slots < 0 || n_slots > MCP_MAP_MAX_MKFS || (n_slots > 0 && (!mkf_bfw || !mkf_flags || !act || !dep)) || n_rows < 0 ||
      n_store < 0 || (n_store > 0 && (!ms_mkf || !ms_cam || !ms_row || !ms_alive))) return collect_fail(who + ": bad arguments");
  if (!std::isfinite(p->mean_diff_fraction)) return collect_fail(who + ": mean_diff_fraction is not finite");
  for (int c = 0; c < ncam; ++c)
    if (p->active[c] && !(std::isfinite(p->depth_mean[c]) && p->depth_mean[c] > 0.0)) return collect_fail(who + ": camera " + std::to_string(c) + ": the depth mean of a used camera must be finite and positive");
  for (int k = 0; k < 12; ++k) if (!std::isfinite(bfw[k])) return collect_fail(who + ": the pose is not finite");
  for (int k = 0; cur_cfb && k < 12*ncam; ++k) if (!std::isfinite(cur_cfb[k])) return collect_fail(who + ": a CamFromBase is not finite");
  mcp::MgRig rig; std::memset(&rig, 0, sizeof rig); rig.ncam = ncam;
  for (int c = 0; c < ncam; ++c) mcp::mg_se3_of12(cfb + 12*(size_t)c, rig.cfb[c]);
  mcp_collect_report R;
  mcp::mgcl_report_clear(&R);
  // k_mgcl_nearest: ascending index, a strict improvement only, so the smallest (dist, slot, cam)
  for (int c = 0; c < ncam; ++c) {
    if (!p->active[c]) continue;
    mcp::Se3 own, cur;
    mcp::mg_se3_of12((cur_cfb ? cur_cfb : cfb) + 12*(size_t)c, own);
    mcp::mgcl_cur_cfw(own, bfw, cur);
    double bd = 0.0; int bi = -1, n_cand = 0; bool broken = false;
    for (int idx = 0; idx < n_slots*MCP_MAX_FRAME_CAMS; ++idx) {
      const int slot = idx/MCP_MAX_FRAME_CAMS, cam = idx % MCP_MAX_FRAME_CAMS;
      if (cam >= ncam || !mcp::mgcl_is_candidate(ncam, cam, mkf_flags[slot], act + (size_t)slot*ncam)) continue;
      bool br;
      const double d = mcp::mgcl_distance(cur, p->depth_mean[c], rig, mkf_bfw + 12*(size_t)slot, dep + (size_t)slot*ncam, cam, p->mean_diff_fraction, &br);
      ++n_cand; broken = broken || br;
      if (mcp::mgcl_before(d, idx, bd, bi)) { bd = d; bi = idx; }
    }
    const int status = broken ? 3 : (bi < 0 ? 1 : 0);
    R.status[c] = status; R.n_candidates[c] = n_cand;
    if (status == 0) { R.nearest_slot[c] = bi/MCP_MAX_FRAME_CAMS; R.nearest_cam[c] = bi % MCP_MAX_FRAME_CAMS; R.nearest_dist[c] = bd; }
  }
  // the three store passes over blocks laid out as the device's (zero padding up to a word boundary)
  const size_t rb = mcp::mgcl_row_bytes(n_rows);
  std::vector<uint8_t> kf_mark((size_t)mcp::MGCL_KF_MARKS, 0), seed(rb, 0), nr(rb, 0);
  auto counts = [&](int i) { return mcp::mgcl_entry_counts(ms_alive[i], ms_mkf[i], ms_cam[i], ms_row[i], n_rows); };
  for (int i = 0; i < n_store; ++i) {
    if (!counts(i)) continue;
    for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) if (ms_mkf[i] == R.nearest_slot[c] && ms_cam[i] == R.nearest_cam[c]) seed[ms_row[i]] |= (uint8_t)(1u << c);
  }
  for (int i = 0; i < n_store; ++i) if (counts(i)) kf_mark[(size_t)ms_mkf[i]*MCP_MAX_FRAME_CAMS + ms_cam[i]] |= seed[ms_row[i]];
  for (int i = 0; i < n_store; ++i) if (counts(i)) nr[ms_row[i]] |= kf_mark[(size_t)ms_mkf[i]*MCP_MAX_FRAME_CAMS + ms_cam[i]];
  const std::vector<uint8_t>* blocks[3] = {&kf_mark, &seed, &nr};
  int* out[3] = {R.n_kfs, R.n_seed_rows, R.n_rows};
  for (int b = 0; b < 3; ++b)
    for (size_t k = 0; k + 4 <= blocks[b]->size(); k += 4) {
      unsigned w; std::memcpy(&w, blocks[b]->data() + k, 4);
      if (!w) continue;
      for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) out[b][c] += mcp::mgcl_count4(w, c);
    }
  R.valid = 1;
  *rep = R;
  if (near && n_rows > 0) std::memcpy(near, nr.data(), (size_t)n_rows);
  return 0;
}
