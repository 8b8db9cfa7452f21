// mcp_map_collect_nearest_host (mcptam_amd/csrc/map_graph_collect_host.cpp) on its own, with exactly sized heap arrays, for a build under
// AddressSanitizer and UndefinedBehaviorSanitizer: the two-hop walk read off a four-keyframe map, a map of 257 rows whose last row is hit
// (the mask's last byte), the last byte of kf_mark (slot 4095, camera 7), entries that must not count, and a refusal that leaves its outputs.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mcp_img.h"

static std::string g_err;
void mcp_set_error(const char* s) { g_err = s; }      // (the library's, for a unit linked without it)

namespace {
struct Map {
  int ncam; std::vector<double> cfb, bfw, dep; std::vector<int> flags; std::vector<uint8_t> act;
  std::vector<int> mkf, cam, row; std::vector<uint8_t> alive;
  Map(int nc, int n_slots) : ncam(nc), cfb(12*(size_t)nc, 0.0), bfw(12*(size_t)n_slots, 0.0), dep((size_t)n_slots*nc, 2.0), flags((size_t)n_slots, 0), act((size_t)n_slots*nc, 1) {
    for (int c = 0; c < nc; ++c) cfb[12*c] = cfb[12*c + 4] = cfb[12*c + 8] = 1.0;
    for (int s = 0; s < n_slots; ++s) bfw[12*(size_t)s] = bfw[12*(size_t)s + 4] = bfw[12*(size_t)s + 8] = 1.0;
  }
  void at(int slot, double x) { flags[slot] = MCP_MKF_PRESENT; bfw[12*(size_t)slot + 9] = -x; }
  void meas(int m, int c, int r, int a = 1) { mkf.push_back(m); cam.push_back(c); row.push_back(r); alive.push_back((uint8_t)a); }
  int run(const double* pose, const mcp_collect_params& p, int n_rows, mcp_collect_report* rep, std::vector<uint8_t>& near) {
    near.assign((size_t)n_rows, 0x5a);
    return mcp_map_collect_nearest_host(pose, nullptr, &p, ncam, cfb.data(), (int)flags.size(), bfw.data(), flags.data(), act.data(), dep.data(), n_rows, (int)mkf.size(),
                                        mkf.data(), cam.data(), row.data(), alive.data(), rep, near.data());
  }
};
mcp_collect_params params(int ncam) {
  mcp_collect_params p; std::memset(&p, 0, sizeof p);
  p.mean_diff_fraction = 0.5;
  for (int c = 0; c < ncam; ++c) { p.depth_mean[c] = 2.0; p.active[c] = 1; }
  return p;
}
}  // namespace

int main() {
  int bad = 0;
  const double pose[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  mcp_collect_report rep;
  std::vector<uint8_t> near;
  {   // K0 (nearest), K1, K2, K3; p0 {K0, K1}, p1 {K1, K2}, p2 {K2, K3}, p3 {K3}; an entry past the table, one of camera 8, a dead one
    Map m(1, 4);
    for (int s = 0; s < 4; ++s) m.at(s, 5.0*s);
    m.meas(0, 0, 0); m.meas(1, 0, 0); m.meas(1, 0, 1); m.meas(2, 0, 1); m.meas(2, 0, 2); m.meas(3, 0, 2); m.meas(3, 0, 3);
    m.meas(0, 0, 4); m.meas(0, 8, 3); m.meas(0, 0, 3, 0); m.meas(-1, 0, 3); m.meas(0, 0, -1);
    if (m.run(pose, params(1), 4, &rep, near) != 0) ++bad;
    const uint8_t want[4] = {1, 1, 0, 0};
    if (std::memcmp(near.data(), want, 4) != 0) ++bad;
    if (rep.valid != 1 || rep.status[0] != 0 || rep.nearest_slot[0] != 0 || rep.nearest_cam[0] != 0 || rep.nearest_dist[0] != 0.0) ++bad;
    if (rep.n_candidates[0] != 4 || rep.n_seed_rows[0] != 1 || rep.n_kfs[0] != 2 || rep.n_rows[0] != 2 || rep.nearest_slot[1] != -1 || rep.status[7] != 0) ++bad;
    // a refusal leaves the outputs
    mcp_collect_params p = params(1); p.depth_mean[0] = 0.0;
    std::memset(&rep, 0x5a, sizeof rep);
    if (m.run(pose, p, 4, &rep, near) != -1 || g_err.find("mcp_map_collect_nearest_host") != 0 || rep.valid != 0x5a5a5a5a || near[3] != 0x5a) ++bad;
  }
  {   // 257 rows, the last one the only one in the set; no store at all; no present slot
    Map m(2, 3);
    m.at(0, 0.0); m.at(2, 9.0);
    m.meas(0, 0, 256); m.meas(0, 1, 256); m.meas(2, 0, 255);
    if (m.run(pose, params(2), 257, &rep, near) != 0 || near[256] != 3 || near[255] != 0 || rep.n_rows[0] != 1 || rep.n_rows[1] != 1 || rep.n_kfs[0] != 2) ++bad;
    Map e(2, 3);
    e.at(1, 1.0);
    if (e.run(pose, params(2), 5, &rep, near) != 0 || rep.status[0] != 0 || rep.nearest_slot[1] != 1 || rep.n_rows[0] != 0 || near[4] != 0) ++bad;
    Map none(1, 2);
    if (none.run(pose, params(1), 0, &rep, near) != 0 || rep.status[0] != 1 || rep.nearest_slot[0] != -1) ++bad;
  }
  {   // slot 4095, camera 7: the last byte of kf_mark
    Map m(8, MCP_MAP_MAX_MKFS);
    m.at(MCP_MAP_MAX_MKFS - 1, 0.0); m.at(0, 50.0);
    m.meas(MCP_MAP_MAX_MKFS - 1, 7, 2);
    for (int c = 0; c < 7; ++c) m.act[(size_t)(MCP_MAP_MAX_MKFS - 1)*8 + c] = 0;      // (the rig's cameras coincide here: camera 7 must be the slot's only keyframe to win)
    mcp_collect_params p = params(8);
    for (int c = 0; c < 7; ++c) p.active[c] = 0;
    if (m.run(pose, p, 3, &rep, near) != 0 || rep.nearest_slot[7] != MCP_MAP_MAX_MKFS - 1 || near[2] != 0x80 || near[0] != 0 || rep.n_kfs[7] != 1 || rep.n_candidates[7] != 9) ++bad;
  }
  if (bad) { std::printf("%d checks failed (%s)\n", bad, g_err.c_str()); return 1; }
  std::printf("collect host ok\n");
  return 0;
}
