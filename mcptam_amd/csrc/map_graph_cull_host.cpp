// mcp_map_cull_outliers_host / mcp_map_cull_sweep_host (include/mcp_img.h): HandleOutliers and the bad-point sweep (map_graph_cull.h) from host
// arrays, in place.  Host code only -- this unit sees none of HIP, so it also builds with a plain C++ compiler next to a main() of its own
// (tests/cpp/cull_host_check.cpp, which the sanitizers read).  The rules are the bodies the kernels call; the outliers are walked in the
// caller's order with the state of every row kept in the arrays, which is what the device's walk row by row comes to.
#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>
#define MGC_HOST_ONLY
#include "map_graph_cull.h"

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int cull_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }

// the good count of every row: the live entries whose MKF is present and not bad
static std::vector<int> good_counts(const mcp::MgcHostMap& M) {
  std::vector<int> good((size_t)M.n_rows, 0);
  for (int i = 0; i < M.n_store; ++i)
    if (mcp::mgc_edge_live(M.ms_alive[i], M.ms_mkf[i], M.ms_row[i], M.n_rows) && mcp::mgc_mkf_ok(mcp::mgc_host_mkf_flags(M, M.ms_mkf[i]))) ++good[M.ms_row[i]];
  return good;
}

static std::string map_check(int n_slots, const int* mkf_flags, int n_rows, int n_point_rows, const void* pflags, const void* pending, int n_store, bool store_ok) {
  if (n_slots < 0 || n_slots > MCP_MAP_MAX_MKFS || n_rows < 0 || n_point_rows < 0 || n_point_rows > n_rows || n_store < 0) return "bad arguments";
  if ((n_slots > 0 && !mkf_flags) || (n_point_rows > 0 && (!pflags || !pending)) || (n_store > 0 && !store_ok)) return "bad arguments";
  return "";
}

extern "C" int mcp_map_cull_outliers_host(int n, const int* mkf, const int* cam, const int* row, const mcp_cull_outliers_params* prm, int ncam, int n_slots, const int* mkf_flags,
                                          int n_rows, int n_point_rows, const int* src_mkf, int* point_flags, uint8_t* pending, int n_store, const int* ms_mkf, const int* ms_cam,
                                          const int* ms_row, const int* ms_source, uint8_t* ms_alive, uint8_t* verdict_out, mcp_cull_outliers_result* res) {
  const std::string who = "mcp_map_cull_outliers_host";
  if (!prm || !res) return cull_fail(who + ": NULL params or result");
  if (n < 0 || (n > 0 && (!mkf || !cam || !row)) || ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || (n_point_rows > 0 && !src_mkf)) return cull_fail(who + ": bad arguments");
  const std::string bad = map_check(n_slots, mkf_flags, n_rows, n_point_rows, point_flags, pending, n_store, ms_mkf && ms_cam && ms_row && ms_source && ms_alive);
  if (!bad.empty()) return cull_fail(who + ": " + bad);
  if (prm->bad_good_count < 0) return cull_fail(who + ": a negative bad_good_count");
  std::vector<unsigned long long> keys((size_t)n);
  for (int k = 0; k < n; ++k) {
    if (mkf[k] < 0 || mkf[k] >= MCP_MAP_MAX_MKFS) return cull_fail(who + ": key " + std::to_string(k) + " names slot " + std::to_string(mkf[k]));
    if (cam[k] < 0 || cam[k] >= ncam) return cull_fail(who + ": key " + std::to_string(k) + " names camera " + std::to_string(cam[k]));
    keys[k] = mcp::mgc_key(mkf[k], cam[k], row[k]);
  }
  std::sort(keys.begin(), keys.end());
  for (int k = 1; k < n; ++k) if (keys[k] == keys[k - 1]) return cull_fail(who + ": a key appears twice");
  const mcp::MgcHostMap M{n_slots, mkf_flags, n_rows, n_point_rows, src_mkf, point_flags, pending, n_store, ms_mkf, ms_cam, ms_row, ms_source, ms_alive};
  // the live entries by key (of several with one key, the last)
  std::vector<std::pair<unsigned long long, int>> live;
  for (int i = 0; i < n_store; ++i)
    if (ms_alive[i] && ms_mkf[i] >= 0 && ms_mkf[i] < MCP_MAP_MAX_MKFS && ms_cam[i] >= 0 && ms_cam[i] < MCP_MAX_FRAME_CAMS) live.emplace_back(mcp::mgc_key(ms_mkf[i], ms_cam[i], ms_row[i]), i);
  std::sort(live.begin(), live.end());
  std::vector<int> good = good_counts(M);
  std::vector<uint8_t> fixed_seen((size_t)n_rows, 0);
  mcp_cull_outliers_result R = {0, 0, 0, 0, 0, 0, 0, 0};
  int cnt[6] = {0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n; ++k) {
    const int r = row[k];
    const bool row_ok = r >= 0 && r < n_point_rows && mcp::mgc_row_written(src_mkf[r], point_flags[r]);
    int at = -1;
    if (row_ok) {
      auto it = std::upper_bound(live.begin(), live.end(), std::make_pair(mcp::mgc_key(mkf[k], cam[k], r), n_store));
      if (it != live.begin() && (it - 1)->first == mcp::mgc_key(mkf[k], cam[k], r)) at = (it - 1)->second;
    }
    mcp::MgcRow S; S.flags = row_ok ? point_flags[r] : 0; S.good = row_ok ? good[r] : 0;
    const int was = S.flags, f = at >= 0 ? mcp::mgc_host_mkf_flags(M, ms_mkf[at]) : 0;
    bool dies;
    const int v = mcp::mgc_judge(S, at >= 0 && ms_alive[at] && (f & MCP_MKF_PRESENT), at >= 0 ? ms_source[at] : 0, mcp::mgc_mkf_ok(f), prm->bad_good_count, &dies);
    if (dies) ms_alive[at] = 0;
    if (row_ok) {
      good[r] = S.good;
      if (!(was & MCP_GP_BAD) && (S.flags & MCP_GP_BAD)) { point_flags[r] = S.flags; pending[r] = 1; ++R.n_rows_marked; }
    }
    if (v == MCP_CULL_FIXED && !fixed_seen[r]) { fixed_seen[r] = 1; ++R.n_fixed_rows; }
    ++cnt[v];
    if (verdict_out) verdict_out[k] = (uint8_t)v;
  }
  R.n_missing = cnt[MCP_CULL_MISSING]; R.n_fixed = cnt[MCP_CULL_FIXED]; R.n_point_bad = cnt[MCP_CULL_POINT_BAD]; R.n_retry = cnt[MCP_CULL_RETRY];
  R.n_never_retry = cnt[MCP_CULL_NEVER_RETRY]; R.n_already_bad = cnt[MCP_CULL_ALREADY_BAD];
  *res = R;
  return 0;
}

extern "C" int mcp_map_cull_sweep_host(const mcp_cull_sweep_params* prm, int n_slots, const int* mkf_flags, int n_rows, int n_point_rows, int* point_flags, uint8_t* pending,
                                       const int* inlier, const int* outlier, uint8_t* usable, int n_store, const int* ms_mkf, const int* ms_row, uint8_t* ms_alive,
                                       mcp_cull_sweep_result* res, int cap_rows, int* rows_out) {
  const std::string who = "mcp_map_cull_sweep_host";
  if (!prm || !res) return cull_fail(who + ": NULL params or result");
  const std::string bad = map_check(n_slots, mkf_flags, n_rows, n_point_rows, point_flags, pending, n_store, ms_mkf && ms_row && ms_alive);
  if (!bad.empty()) return cull_fail(who + ": " + bad);
  if ((n_rows > 0 && (!inlier || !outlier || !usable)) || cap_rows < 0 || (cap_rows > 0 && !rows_out)) return cull_fail(who + ": bad arguments");
  if (prm->min_outliers < 0) return cull_fail(who + ": a negative min_outliers");
  if (!std::isfinite(prm->outlier_multiplier)) return cull_fail(who + ": outlier_multiplier is not finite");
  const mcp::MgcHostMap M{n_slots, mkf_flags, n_rows, n_point_rows, nullptr, point_flags, pending, n_store, ms_mkf, nullptr, ms_row, nullptr, ms_alive};
  int n_present = 0;
  for (int k = 0; k < n_slots; ++k) n_present += (mkf_flags[k] & MCP_MKF_PRESENT) ? 1 : 0;
  const int danglers_on = (prm->danglers && n_present >= 2) ? 1 : 0;
  const std::vector<int> good = good_counts(M);
  std::vector<uint8_t> rule((size_t)n_point_rows, 0);
  int n_reported = 0;
  for (int i = 0; i < n_point_rows; ++i) {
    rule[i] = (uint8_t)mcp::mgc_sweep_rule(point_flags[i], good[i], inlier[i], outlier[i], danglers_on, prm->min_outliers, prm->outlier_multiplier);
    if (rule[i] || ((point_flags[i] & MCP_GP_BAD) && pending[i])) ++n_reported;
  }
  if (n_reported > cap_rows) return cull_fail(who + ": " + std::to_string(n_reported) + " rows are reported, cap_rows is " + std::to_string(cap_rows));
  mcp_cull_sweep_result R = {0, 0, 0, 0, 0};
  for (int i = 0; i < n_rows; ++i) {
    bool is_bad = true;                                // (no graph column yet: never written)
    if (i < n_point_rows) {
      if (rule[i] || ((point_flags[i] & MCP_GP_BAD) && pending[i])) rows_out[R.n_reported++] = i;
      if (rule[i]) { point_flags[i] |= MCP_GP_BAD; ++(rule[i] == 1 ? R.n_danglers : R.n_tracker_outliers); }
      pending[i] = 0;
      is_bad = (point_flags[i] & MCP_GP_BAD) != 0;
    }
    if (is_bad) { usable[i] = 0; ++R.n_bad_rows; }
  }
  for (int i = 0; i < n_store; ++i) {
    const int r = ms_row[i];
    if (!ms_alive[i] || r < 0 || r >= n_rows) continue;
    if (r >= n_point_rows || (point_flags[r] & MCP_GP_BAD)) { ms_alive[i] = 0; ++R.n_meas_erased; }
  }
  *res = R;
  return R.n_reported;
}
