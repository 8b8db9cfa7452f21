// mcp_stereo_busy_host / mcp_stereo_append_host (mcptam_amd/csrc/stereo_append_host.cpp) under the host compiler alone: stores at the workgroup
// seams of the gather (256 entries) and appends of 0, 1 and 7 points, against the rules written out here.  Built with
// -fsanitize=address,undefined by tests/test_stereo_map_cpu.py; every array is sized exactly, so a read or write past one is a finding.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mcp_img.h"

static std::string g_err;
void mcp_set_error(const char* s) { g_err = s; }      // (the library's lives in the solver unit)

static uint64_t rnd(uint64_t& s) { s = s*6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

static int check_busy(int n, int src_mkf, int src_cam, uint64_t seed) {
  uint64_t s = seed;
  std::vector<mcp_store_entry> store(n);
  std::vector<mcp_stereo_meas> want;
  for (int i = 0; i < n; ++i) {
    mcp_store_entry& e = store[i];
    const int kind = (int)(rnd(s) % 8);
    e.mkf = kind < 6 ? src_mkf : src_mkf + 1 + (int)(rnd(s) % 3);
    e.cam = (kind < 4 || kind == 6) ? src_cam : (src_cam + 1) % 4;
    e.row = i; e.level = (int)(rnd(s) % MCP_LEVELS); e.source = (int)(rnd(s) % 5); e.alive = rnd(s) % 8 != 0;
    e.uv[0] = 0.25*i - 3.0; e.uv[1] = -(double)rnd(s)/4096.0;
    if (e.alive && e.mkf == src_mkf && e.cam == src_cam) want.push_back(mcp_stereo_meas{{e.uv[0], e.uv[1]}, e.level, 0});
  }
  const int total = (int)want.size();
  const int counted = mcp_stereo_busy_host(n, n ? store.data() : nullptr, src_mkf, src_cam, 0, nullptr);
  if (counted != total) { std::printf("busy n %d: counted %d, expected %d (%s)\n", n, counted, total, g_err.c_str()); return 1; }
  std::vector<mcp_stereo_meas> got(total);               // exactly the list: one record more would be a write past it
  if (total) {
    std::memset(got.data(), 0xff, sizeof(mcp_stereo_meas)*(size_t)total);
    const int rc = mcp_stereo_busy_host(n, store.data(), src_mkf, src_cam, total, got.data());
    if (rc != total || std::memcmp(got.data(), want.data(), sizeof(mcp_stereo_meas)*(size_t)total) != 0) { std::printf("busy n %d: the list differs\n", n); return 1; }
  }
  if (total > 1) {                                       // an array one record short: refused, nothing written past it
    std::vector<mcp_stereo_meas> small(total - 1);
    if (mcp_stereo_busy_host(n, store.data(), src_mkf, src_cam, total - 1, small.data()) != -1 || g_err.find("mcp_stereo_busy_host:") != 0) {
      std::printf("busy n %d: a short array was not refused\n", n); return 1; }
  }
  return 0;
}

static int check_append(int made, int level, int first_store, uint64_t seed) {
  uint64_t s = seed;
  const int n_targets = 3;
  const int tmkf[n_targets] = {2, 9, 4095}, tcam[n_targets] = {0, 1, 0};
  std::vector<mcp_stereo_point> pts(made);
  std::vector<int> rows(made), cx(made), cy(made);
  for (int k = 0; k < made; ++k) {
    mcp_stereo_point& p = pts[k];
    std::memset(&p, 0, sizeof p);
    p.candidate = k; p.target = (int)(rnd(s) % n_targets); p.hypothesis = (int)(rnd(s) % 90); p.score = (int)(rnd(s) % 5000);
    cx[k] = (int)(rnd(s) % (640 >> level)); cy[k] = (int)(rnd(s) % (480 >> level));
    p.root_pos[0] = (cx[k] + 0.5)*(1 << level) - 0.5; p.root_pos[1] = (cy[k] + 0.5)*(1 << level) - 0.5;
    double* f[] = {p.world_pos, p.center_nc, p.one_right_nc, p.one_down_nc, p.pixel_right_w, p.pixel_down_w};
    for (double* v : f) for (int a = 0; a < 3; ++a) v[a] = ((double)rnd(s) - 1e9)/65536.0;
    p.target_pos[0] = (double)rnd(s)/4096.0; p.target_pos[1] = -0.0;
    rows[k] = (made - k)*1000003 % 2000000011;             // out of order, far apart, distinct
  }
  std::vector<double> wp(3*(size_t)made), pr(3*(size_t)made), pd(3*(size_t)made), rays(9*(size_t)made);
  std::vector<int> cxy(2*(size_t)made), gm(made), gc(made), gf(made, -7);
  std::vector<mcp_store_entry> ap(2*(size_t)made);
  const int rc = mcp_stereo_append_host(made, made ? pts.data() : nullptr, rows.data(), level, 5, 1, tmkf, tcam, first_store, wp.data(), pr.data(), pd.data(), rays.data(),
                                        cxy.data(), gm.data(), gc.data(), gf.data(), ap.data());
  if (rc != first_store + 2*made) { std::printf("append made %d: returned %d (%s)\n", made, rc, g_err.c_str()); return 1; }
  for (int k = 0; k < made; ++k) {
    const mcp_stereo_point& p = pts[k];
    bool ok = std::memcmp(&wp[3*(size_t)k], p.world_pos, 24) == 0 && std::memcmp(&pr[3*(size_t)k], p.pixel_right_w, 24) == 0 && std::memcmp(&pd[3*(size_t)k], p.pixel_down_w, 24) == 0 &&
              std::memcmp(&rays[9*(size_t)k], p.center_nc, 24) == 0 && std::memcmp(&rays[9*(size_t)k + 3], p.one_right_nc, 24) == 0 &&
              std::memcmp(&rays[9*(size_t)k + 6], p.one_down_nc, 24) == 0;
    ok = ok && cxy[2*(size_t)k] == cx[k] && cxy[2*(size_t)k + 1] == cy[k] && gm[k] == 5 && gc[k] == 1 && gf[k] == 0;
    const mcp_store_entry root{{p.root_pos[0], p.root_pos[1]}, 5, 1, rows[k], level, MCP_SRC_ROOT, 1};
    const mcp_store_entry epi{{p.target_pos[0], p.target_pos[1]}, tmkf[p.target], tcam[p.target], rows[k], level, MCP_SRC_EPIPOLAR, 1};
    ok = ok && std::memcmp(&ap[2*(size_t)k], &root, sizeof root) == 0 && std::memcmp(&ap[2*(size_t)k + 1], &epi, sizeof epi) == 0;
    if (!ok) { std::printf("append made %d level %d: point %d differs\n", made, level, k); return 1; }
  }
  if (made > 0) {                                        // a record without a target: refused, nothing written
    std::vector<mcp_stereo_point> bad(pts);
    bad[made/2].target = -1;
    std::vector<int> untouched(made, -7);
    if (mcp_stereo_append_host(made, bad.data(), rows.data(), level, 5, 1, tmkf, tcam, first_store, wp.data(), pr.data(), pd.data(), rays.data(), cxy.data(), gm.data(), gc.data(),
                               untouched.data(), ap.data()) != -1 || g_err.find("mcp_stereo_append_host:") != 0) { std::printf("append made %d: a bad target was not refused\n", made); return 1; }
    for (int v : untouched) if (v != -7) { std::printf("append made %d: a refused call wrote\n", made); return 1; }
  }
  return 0;
}

int main() {
  static_assert(sizeof(mcp_stereo_meas) == 24 && sizeof(mcp_store_entry) == 40, "no padding: the records compare as bytes");
  int bad = 0, n = 0;
  const int sizes[] = {0, 1, 255, 256, 257, 70001};
  for (int m : sizes) { bad += check_busy(m, 3, 0, 1000 + m); bad += check_busy(m, 0, 1, 5 + m); n += 2; }
  const int made[] = {0, 1, 7};
  for (int m : made) { bad += check_append(m, 0, 0, 77 + m); bad += check_append(m, 3, 4099, 9 + m); bad += check_append(m, 0, 17, 3 + m); bad += check_append(m, 3, 0, 1 + m); n += 4; }
  if (bad) return 1;
  std::printf("stereo append host ok: %d cases\n", n);
  return 0;
}
