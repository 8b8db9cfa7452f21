// mcp_graph_kf_lists_host (mcptam_amd/csrc/map_graph_lists_host.cpp) under the host compiler alone: stores at the size seams of the device
// passes (a tile of 256 entries, 64 chunks) against a stable sort written here.  Built with -fsanitize=address,undefined by
// tests/test_graph_lists_cpu.py; the output arrays are sized exactly, so a write past the lists is a finding.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mcp_img.h"

static std::string g_err;
void mcp_set_error(const char* s) { g_err = s; }      // (the library's lives in the solver unit)

static uint64_t rnd(uint64_t& s) { s = s*6364136223846793005ull + 1442695040888963407ull; return s >> 33; }

static int check(int n_store, int P, int C, int n_rows, uint64_t seed) {
  std::vector<int> flags(P, MCP_MKF_PRESENT), pflags(n_rows, 0), inl(n_rows), outl(n_rows), mkf(n_store), cam(n_store), row(n_store), slots;
  std::vector<uint8_t> act((size_t)P*C, 1), alive(n_store, 1);
  uint64_t s = seed;
  for (int r = 0; r < n_rows; ++r) { inl[r] = 1 + (int)(rnd(s) % 40); outl[r] = (int)(rnd(s) % 40); if (rnd(s) % 7 == 0) pflags[r] = MCP_GP_BAD; }
  for (int k = 0; k < P*C; ++k) if (rnd(s) % 9 == 0) act[k] = 0;
  for (int e = 0; e < n_store; ++e) {
    mkf[e] = (int)(rnd(s) % (P + 1)) - (rnd(s) % 50 == 0);          // now and then -1 or P: in no list
    cam[e] = (int)(rnd(s) % C); row[e] = (int)(rnd(s) % (n_rows + 3)) - 1; alive[e] = rnd(s) % 5 != 0;
  }
  for (int k = P - 1; k >= 0; k -= 2) slots.push_back(k);
  const int n_mkfs = (int)slots.size(), n_kf = n_mkfs*C;
  // the expectation: a stable sort of the kept entries by key
  std::vector<int> pos(P, -1);
  for (int i = 0; i < n_mkfs; ++i) pos[slots[i]] = i;
  std::vector<std::pair<int, int>> kept;
  for (int e = 0; e < n_store; ++e) {
    if (!alive[e] || mkf[e] < 0 || mkf[e] >= P || row[e] < 0 || row[e] >= n_rows) continue;
    if (pos[mkf[e]] < 0 || !act[(size_t)mkf[e]*C + cam[e]] || (pflags[row[e]] & MCP_GP_BAD)) continue;
    kept.emplace_back(pos[mkf[e]]*C + cam[e], e);
  }
  std::stable_sort(kept.begin(), kept.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
  const int total = (int)kept.size();
  std::vector<int> seg_start(n_kf + 1, -7), seg_rows(total, -7);
  std::vector<double> seg_w(total, -7.0);
  const int rc = mcp_graph_kf_lists_host(C, P, flags.data(), act.data(), n_rows, n_rows, pflags.data(), inl.data(), outl.data(), n_store, mkf.data(), cam.data(), row.data(),
                                         alive.data(), n_mkfs, slots.data(), seg_start.data(), total, total ? seg_rows.data() : nullptr, total ? seg_w.data() : nullptr);
  if (rc != total) { std::printf("n_store %d: returned %d, expected %d (%s)\n", n_store, rc, total, g_err.c_str()); return 1; }
  for (int i = 0; i < total; ++i) {
    const int e = kept[i].second;
    const double w = (double)inl[row[e]]/(double)(inl[row[e]] + outl[row[e]]);
    if (seg_rows[i] != row[e] || std::memcmp(&seg_w[i], &w, 8) != 0) { std::printf("n_store %d: entry %d differs\n", n_store, i); return 1; }
    if (i < seg_start[kept[i].first] || i >= seg_start[kept[i].first + 1]) { std::printf("n_store %d: entry %d outside its list\n", n_store, i); return 1; }
  }
  if (seg_start[0] != 0 || seg_start[n_kf] != total) { std::printf("n_store %d: seg_start ends wrong\n", n_store); return 1; }
  // one entry too few of room: refused, nothing but seg_start written
  if (total > 0) {
    std::vector<int> small_rows(total - 1, -7); std::vector<double> small_w(total - 1, -7.0);
    const int rc2 = mcp_graph_kf_lists_host(C, P, flags.data(), act.data(), n_rows, n_rows, pflags.data(), inl.data(), outl.data(), n_store, mkf.data(), cam.data(), row.data(),
                                            alive.data(), n_mkfs, slots.data(), seg_start.data(), total - 1, total > 1 ? small_rows.data() : nullptr, total > 1 ? small_w.data() : nullptr);
    if (rc2 != -1 || g_err.find("caller's arrays") == std::string::npos) { std::printf("n_store %d: a short array was not refused\n", n_store); return 1; }
    for (int v : small_rows) if (v != -7) { std::printf("n_store %d: a refused call wrote\n", n_store); return 1; }
  }
  return 0;
}

int main() {
  const int tile = 256, chunks = 64;
  const int sizes[] = {0, 1, tile - 1, tile, tile + 1, tile*chunks - 1, tile*chunks, tile*chunks + 1, 3*tile*chunks + 17};
  int bad = 0, n = 0;
  for (int m : sizes) { bad += check(m, 9, 3, 500, 1000 + m); bad += check(m, 64, 8, 97, 5 + m); n += 2; }
  if (bad) return 1;
  std::printf("kf lists host ok: %d stores\n", n);
  return 0;
}
