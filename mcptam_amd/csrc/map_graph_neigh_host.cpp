// mcp_map_neighbours_host / mcp_map_mkf_cull_host (include/mcp_img.h): the closest-keyframe queries and the removal of an MKF
// (map_graph_neigh.h) from host arrays.  Host code only: the unit is compiled as the host half of a HIP source, so that the __host__
// __device__ bodies it shares with the kernels (the candidate rule, the distances of map_graph_dist.h, the order, the point rule) are the very
// text the device runs, and without fused multiply-add contraction, so that they give the device's bits.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#define MGN_HOST_ONLY
#include "map_graph_neigh.h"

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int neigh_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }

namespace {
struct HostMkfs { int ncam, n_slots; const double* bfw; const int* flags; const uint8_t* act; const double* dep; };

std::string mkfs_check(int ncam, const double* cfb, int n_slots, const double* bfw, const int* flags, const uint8_t* act, const double* dep) {
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !cfb || n_slots < 0 || n_slots > MCP_MAP_MAX_MKFS || (n_slots > 0 && (!bfw || !flags || !act || !dep))) return "bad arguments";
  return "";
}
mcp::MgRig rig_of(int ncam, const double* cfb) {
  mcp::MgRig rig; std::memset(&rig, 0, sizeof rig); rig.ncam = ncam;
  for (int c = 0; c < ncam; ++c) mcp::mg_se3_of12(cfb + 12*(size_t)c, rig.cfb[c]);
  return rig;
}

// the query over host columns: what k_mgn_dist and k_mgn_select come to.  ext_*: the external MKF (read with Q.src_slot == -1 only)
void host_query(const mcp::MgnQuery& Q, const mcp::MgRig& rig, const HostMkfs& K, const double* ext_bfw, const uint8_t* ext_act, const double* ext_dep, mcp_neigh_result& R) {
  std::memset(&R, 0, sizeof R);
  const int nc = K.ncam, n_idx = mcp::mgn_indices(Q.kind, K.n_slots);
  auto bfw = [&](int s) { return s >= 0 ? K.bfw + 12*(size_t)s : ext_bfw; };
  auto act = [&](int s) { return s >= 0 ? K.act + (size_t)s*nc : ext_act; };
  auto dep = [&](int s) { return s >= 0 ? K.dep + (size_t)s*nc : ext_dep; };
  std::vector<std::pair<double, int>> cand;
  bool broken = false;
  for (int idx = 0; idx < n_idx; ++idx) {
    int slot, cam;
    mcp::mgn_slot_cam(Q.kind, idx, &slot, &cam);
    if (slot < 0 && Q.src_slot >= 0) continue;
    if (!mcp::mgn_is_candidate(Q, nc, slot, cam, slot >= 0 ? K.flags[slot] : 0, act(slot))) continue;
    bool br;
    const double d = mcp::mgn_distance(Q, rig, bfw(Q.src_slot), act(Q.src_slot), dep(Q.src_slot), bfw(slot), act(slot), dep(slot), cam, &br);
    broken = broken || br;
    ++R.n_candidates;
    if (mcp::mgn_eligible(Q, d)) cand.emplace_back(d, idx);
  }
  if (broken) { R.status = 3; return; }
  std::sort(cand.begin(), cand.end(), [&](const std::pair<double, int>& a, const std::pair<double, int>& b) { return mcp::mgn_before(Q.order, a.first, a.second, b.first, b.second); });
  R.count = (int)std::min<size_t>(cand.size(), (size_t)Q.n_max);
  for (int r = 0; r < R.count; ++r) {
    int slot, cam;
    mcp::mgn_slot_cam(Q.kind, cand[r].second, &slot, &cam);
    mcp_neigh_item& I = R.item[r];
    I.dist = cand[r].first; I.slot = slot; I.cam = Q.kind == MCP_NB_KF ? cam : -1; I.flags = slot >= 0 ? K.flags[slot] : 0; I.n_meas = Q.want_meas ? 0 : -1;
  }
}
}  // namespace

extern "C" int mcp_map_neighbours_host(const mcp_neigh_params* p, int ncam, const double* cfb, int n_slots, const double* bfw, const int* mkf_flags, const uint8_t* act,
                                       const double* dep, int n_store, const int* ms_mkf, const int* ms_cam, const uint8_t* ms_alive, mcp_neigh_result* res) {
  const std::string who = "mcp_map_neighbours_host";
  if (!res) return neigh_fail(who + ": NULL result");
  std::string bad = mkfs_check(ncam, cfb, n_slots, bfw, mkf_flags, act, dep);
  if (bad.empty() && n_store < 0) bad = "bad arguments";
  if (bad.empty()) bad = mcp::mgn_params_check(p, ncam);
  if (bad.empty() && p->want_meas && n_store > 0 && (!ms_mkf || !ms_cam || !ms_alive)) bad = "bad arguments";
  if (bad.empty()) {
    const int s = p->src_slot;
    bad = mcp::mgn_source_check(p, s >= 0 && s < n_slots ? mkf_flags[s] : 0, s >= 0 && s < n_slots ? act + (size_t)s*ncam : p->ext_active);
  }
  if (!bad.empty()) return neigh_fail(who + ": " + bad);
  const mcp::MgnQuery Q = mcp::mgn_query(*p);
  const HostMkfs K{ncam, n_slots, bfw, mkf_flags, act, dep};
  // the external MKF as an upload makes it: bytes 0 / 1, the depth of an inactive keyframe 0
  uint8_t ea[MCP_MAX_FRAME_CAMS] = {0, 0, 0, 0, 0, 0, 0, 0}; double ed[MCP_MAX_FRAME_CAMS] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 0; c < ncam; ++c) { ea[c] = p->ext_active[c] ? 1 : 0; ed[c] = ea[c] ? p->ext_depth_mean[c] : 0.0; }
  mcp_neigh_result R;
  host_query(Q, rig_of(ncam, cfb), K, p->ext_base_from_world, ea, ed, R);
  if (Q.want_meas)
    for (int i = 0; i < n_store; ++i) {
      if (!ms_alive[i]) continue;
      for (int w = 0; w < R.count; ++w)
        if (ms_mkf[i] == R.item[w].slot && (Q.kind == MCP_NB_MKF || ms_cam[i] == R.item[w].cam)) ++R.item[w].n_meas;
    }
  *res = R;
  return 0;
}

extern "C" int mcp_map_mkf_cull_host(const mcp_mkf_cull_params* p, int ncam, const double* cfb, int n_slots, const double* bfw, int* mkf_flags, const uint8_t* act,
                                     const double* dep, int n_rows, int n_point_rows, const int* src_mkf, const int* src_cam, int* point_flags, uint8_t* pending,
                                     int n_store, const int* ms_mkf, const int* ms_cam, const int* ms_row, uint8_t* ms_alive, mcp_mkf_cull_result* res) {
  const std::string who = "mcp_map_mkf_cull_host";
  if (!p || !res) return neigh_fail(who + ": NULL params or result");
  std::string bad = mkfs_check(ncam, cfb, n_slots, bfw, mkf_flags, act, dep);
  if (bad.empty() && (n_rows < 0 || n_point_rows < 0 || n_point_rows > n_rows || n_store < 0 || (n_point_rows > 0 && (!src_mkf || !src_cam || !point_flags || !pending)) ||
                      (n_store > 0 && (!ms_mkf || !ms_cam || !ms_row || !ms_alive)))) bad = "bad arguments";
  if (!bad.empty()) return neigh_fail(who + ": " + bad);
  auto present = [&](int k) { return k >= 0 && k < n_slots && (mkf_flags[k] & MCP_MKF_PRESENT); };
  if (p->slot != -1 && !present(p->slot)) return neigh_fail(who + ": the victim (slot " + std::to_string(p->slot) + ") is not a present slot");
  if (p->slot == -1 && !present(p->furthest_from)) return neigh_fail(who + ": furthest_from (slot " + std::to_string(p->furthest_from) + ") is not a present slot");
  if (p->max_kfs < 0) return neigh_fail(who + ": a negative max_kfs");
  if (!std::isfinite(p->mean_diff_fraction)) return neigh_fail(who + ": mean_diff_fraction is not finite");
  const mcp::MgRig rig = rig_of(ncam, cfb);
  const HostMkfs K{ncam, n_slots, bfw, mkf_flags, act, dep};
  mcp::MgnQuery Q;
  Q.kind = MCP_NB_MKF; Q.region = MCP_NB_ALL; Q.src_cam = 0; Q.same_cam = 0; Q.n_max = 1; Q.want_meas = 0; Q.max_dist = HUGE_VAL; Q.frac = p->mean_diff_fraction;
  mcp_mkf_cull_result R;
  std::memset(&R, 0, sizeof R);
  R.victim = -1; R.new_fixed = -1;
  int victim = p->slot;
  mcp_neigh_result N;
  if (victim == -1) {                                  // FurthestMultiKeyFrame(furthest_from)
    Q.order = MCP_NB_FURTHEST; Q.src_slot = p->furthest_from;
    host_query(Q, rig, K, nullptr, nullptr, nullptr, N);
    if (N.status != 0) { R.status = 3; *res = R; return 0; }
    if (N.count == 0) { R.status = 1; *res = R; return 0; }
    victim = N.item[0].slot; R.victim_dist = N.item[0].dist; R.victim_dist_valid = 1;
  }
  int new_fixed = -1;
  if (mkf_flags[victim] & MCP_MKF_FIXED) {             // ClosestMultiKeyFrame(victim), :313-317
    Q.order = MCP_NB_NEAREST; Q.src_slot = victim;
    host_query(Q, rig, K, nullptr, nullptr, nullptr, N);
    if (N.status != 0) { std::memset(&R, 0, sizeof R); R.status = 3; R.victim = -1; R.new_fixed = -1; *res = R; return 0; }
    if (N.count > 0) new_fixed = N.item[0].slot;
  }
  R.victim = victim; R.new_fixed = new_fixed;
  mkf_flags[victim] |= MCP_MKF_BAD;
  if (new_fixed >= 0) mkf_flags[new_fixed] |= MCP_MKF_FIXED;
  auto live_entry = [&](int i) { return ms_alive[i] && ms_row[i] >= 0 && ms_row[i] < n_rows && ms_mkf[i] >= 0 && ms_mkf[i] < MCP_MAP_MAX_MKFS; };
  std::vector<int> live((size_t)n_rows, 0);
  std::vector<uint8_t> by_src((size_t)n_rows, 0);
  for (int i = 0; i < n_store; ++i) {
    if (!live_entry(i)) continue;
    const int r = ms_row[i];
    ++live[r];
    if (ms_mkf[i] == victim && r < n_point_rows && src_mkf[r] == victim && src_cam[r] == ms_cam[i]) by_src[r] = 1;
  }
  std::vector<int> to_mark;
  for (int i = 0; i < n_store; ++i) {
    if (!live_entry(i) || ms_mkf[i] != victim) continue;
    ++R.n_victim_meas;
    const int r = ms_row[i];
    bool b;
    if (p->mark_points && r < n_point_rows && mcp::mgn_point_rule(point_flags[r], src_mkf[r], src_cam[r], live[r], p->max_kfs, victim, ms_cam[i], &b)) to_mark.push_back(r);
  }
  for (int r : to_mark) {
    if (point_flags[r] & MCP_GP_BAD) continue;         // bad already (or marked by an earlier entry of this call)
    point_flags[r] |= MCP_GP_BAD; pending[r] = 1;
    ++R.n_rows_marked; ++(by_src[r] ? R.n_by_source : R.n_by_count);
  }
  if (p->erase) {
    for (int i = 0; i < n_store; ++i) if (ms_alive[i] && ms_mkf[i] == victim) { ms_alive[i] = 0; ++R.n_meas_erased; }
    mkf_flags[victim] &= ~MCP_MKF_PRESENT;
  }
  *res = R;
  return 0;
}
