// mcp_parcel_commit_host (mcptam_amd/csrc/map_graph_parcel_host.cpp) under the host compiler alone: parcels at the size seams of the device
// passes (a wavefront of 64, a workgroup of 256 entries) against the rules written out here.  Built with -fsanitize=address,undefined by
// tests/test_parcel_cpu.py; every array is sized exactly, so a read or write past one is a finding.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mcp_img.h"

static std::string g_err;
void mcp_set_error(const char* s) { g_err = s; }      // (the library's lives in the solver unit)

static uint64_t rnd(uint64_t& s) { s = s*6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

static int check(int n, int n_lanes, int cross, uint64_t seed) {
  uint64_t s = seed;
  const int n_rows = 50 + n/3, n_prows = n_rows - 9;
  std::vector<int> keys(n_rows), pflags(n_prows), smkf(n_prows), scam(n_prows), lane_mkf(n_lanes), lane_cam(n_lanes);
  for (int r = 0; r < n_rows; ++r) keys[r] = 3*r + 7;
  for (int r = 0; r < n_prows; ++r) { pflags[r] = (rnd(s) % 8 == 0 ? MCP_GP_BAD : 0) | (rnd(s) % 16 == 0 ? MCP_GP_FIXED : 0); smkf[r] = (pflags[r] & MCP_GP_FIXED) ? -1 : (int)(rnd(s) % 5); scam[r] = (int)(rnd(s) % 3); }
  for (int l = 0; l < n_lanes; ++l) { lane_mkf[l] = rnd(s) % 5 == 0 ? -1 : (int)(rnd(s) % 5); lane_cam[l] = (int)(rnd(s) % 3); }
  std::vector<mcp_parcel_entry> ent(n);
  for (int i = 0; i < n; ++i) {
    mcp_parcel_entry& e = ent[i];
    e.lane = (int)(rnd(s) % n_lanes); e.row = (int)(rnd(s) % (n_rows + 4)) - (rnd(s) % 40 == 0 ? 1 : 0);      // now and then -1 or past the table
    e.key = (e.row >= 0 && e.row < n_rows && rnd(s) % 9 != 0) ? keys[e.row] : 5; e.level = (int)(rnd(s) % MCP_LEVELS);
    e.uv[0] = (double)rnd(s)/1024.0; e.uv[1] = -(double)rnd(s)/4096.0;
  }
  // the expectation
  std::vector<uint8_t> want(n);
  std::vector<mcp_store_entry> recs;
  int cnt[5] = {0, 0, 0, 0, 0};
  std::vector<int> per_lane(n_lanes, 0);
  for (int i = 0; i < n; ++i) {
    const mcp_parcel_entry& e = ent[i];
    int v = MCP_PARCEL_APPENDED;
    if (lane_mkf[e.lane] < 0) v = MCP_PARCEL_SKIPPED;
    else if (e.row < 0 || e.row >= n_rows || keys[e.row] != e.key) v = MCP_PARCEL_STALE;
    else if (e.row >= n_prows || (pflags[e.row] & MCP_GP_BAD)) v = MCP_PARCEL_BAD;
    else if (!cross && (smkf[e.row] < 0 || scam[e.row] != lane_cam[e.lane])) v = MCP_PARCEL_CROSS;
    want[i] = (uint8_t)v; ++cnt[v];
    if (v == MCP_PARCEL_APPENDED) { recs.push_back(mcp_store_entry{{e.uv[0], e.uv[1]}, lane_mkf[e.lane], lane_cam[e.lane], e.row, e.level, 3, 1}); ++per_lane[e.lane]; }
  }
  const int total = (int)recs.size();
  std::vector<uint8_t> got(n, 99);
  std::vector<mcp_store_entry> out(total);               // exactly the appended count: one record more would be a write past it
  std::vector<int> got_lane(n_lanes, -7);
  const mcp_parcel_commit_params prm{cross, 3};
  mcp_parcel_commit_result res;
  std::memset(&res, 0xff, sizeof res);
  const int rc = mcp_parcel_commit_host(n, n ? ent.data() : nullptr, n_rows, keys.data(), n_prows, pflags.data(), smkf.data(), scam.data(), n_lanes, lane_mkf.data(), lane_cam.data(), &prm, 17,
                                        n ? got.data() : nullptr, total ? out.data() : nullptr, &res, got_lane.data());
  if (rc != total) { std::printf("n %d: returned %d, expected %d (%s)\n", n, rc, total, g_err.c_str()); return 1; }
  if (res.first != 17 || res.n_appended != cnt[0] || res.n_skipped_lane != cnt[1] || res.n_stale != cnt[2] || res.n_bad != cnt[3] || res.n_cross != cnt[4] ||
      res.n_appended + res.n_skipped_lane + res.n_stale + res.n_bad + res.n_cross != n) { std::printf("n %d: counters differ\n", n); return 1; }
  if (n && std::memcmp(got.data(), want.data(), (size_t)n) != 0) { std::printf("n %d: verdicts differ\n", n); return 1; }
  if (total && std::memcmp(out.data(), recs.data(), sizeof(mcp_store_entry)*(size_t)total) != 0) { std::printf("n %d: records differ\n", n); return 1; }
  if (got_lane != per_lane) { std::printf("n %d: per-lane counts differ\n", n); return 1; }
  // an entry of a lane the tables do not have: refused, nothing written
  if (n > 0) {
    std::vector<mcp_parcel_entry> bad(ent);
    bad[n/2].lane = n_lanes;
    std::vector<uint8_t> untouched(n, 99);
    const int rc2 = mcp_parcel_commit_host(n, bad.data(), n_rows, keys.data(), n_prows, pflags.data(), smkf.data(), scam.data(), n_lanes, lane_mkf.data(), lane_cam.data(), &prm, 0,
                                           untouched.data(), nullptr, &res, nullptr);
    if (rc2 != -1 || g_err.find("names lane") == std::string::npos) { std::printf("n %d: a lane past the tables was not refused\n", n); return 1; }
    for (uint8_t v : untouched) if (v != 99) { std::printf("n %d: a refused call wrote\n", n); return 1; }
  }
  return 0;
}

int main() {
  static_assert(sizeof(mcp_parcel_entry) == 32 && sizeof(mcp_store_entry) == 40, "no padding: the records compare as bytes");
  const int sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 513, 1031, 70001};
  int bad = 0, n = 0;
  for (int m : sizes) { bad += check(m, 1 + m % 8, 1, 1000 + m); bad += check(m, 8, 0, 5 + m); bad += check(m, 3, 0, 77 + m); n += 3; }
  if (bad) return 1;
  std::printf("parcel commit host ok: %d parcels\n", n);
  return 0;
}
