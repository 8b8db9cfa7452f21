// mcp_init_depth_points_host / mcp_map_mark_optimized_host / mcp_map_transform_host (mcptam_amd/csrc/map_life_host.cpp) on their own: init-depth
// calls whose limit cuts inside, at and behind a list, maps at the 256-row seams under a scale and a rigid motion, against the rules written out
// here.  Built as the host half of a HIP source (the unit shares its bodies with the kernels) with -fsanitize=address,undefined by
// tests/test_map_life_cpu.py; every array is sized exactly, so a read or write past one is a finding.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "mcp_img.h"

static std::string g_err;
void mcp_set_error(const char* s) { g_err = s; }      // (the library's lives in the solver unit)

static uint64_t rnd(uint64_t& s) { s = s*6364136223846793005ull + 1442695040888963407ull; return s >> 33; }
static double unit(uint64_t& s) { return (double)(rnd(s) % 100000)/100000.0; }                  // [0, 1)
static double nonzero(uint64_t& s) { return (0.3 + 3.0*unit(s))*((rnd(s) & 1) ? 1.0 : -1.0); }

// a rotation about a general axis (Rodrigues), row-major
static void rotation(double ax, double ay, double az, double* R) {
  const double th = std::sqrt(ax*ax + ay*ay + az*az), c = std::cos(th), s = std::sin(th), x = ax/th, y = ay/th, z = az/th;
  const double M[9] = { c + x*x*(1 - c), x*y*(1 - c) - z*s, x*z*(1 - c) + y*s, y*x*(1 - c) + z*s, c + y*y*(1 - c), y*z*(1 - c) - x*s, z*x*(1 - c) - y*s, z*y*(1 - c) + x*s, c + z*z*(1 - c) };
  std::memcpy(R, M, sizeof M);
}
static void pose(double ax, double ay, double az, double tx, double ty, double tz, double* T) { rotation(ax, ay, az, T); T[9] = tx; T[10] = ty; T[11] = tz; }
static void compose(const double* A, const double* B, double* C) {      // (Ra Rb, Ra tb + ta)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) C[3*i + j] = A[3*i]*B[j] + A[3*i + 1]*B[3 + j] + A[3*i + 2]*B[6 + j];
    C[9 + i] = A[3*i]*B[9] + A[3*i + 1]*B[10] + A[3*i + 2]*B[11] + A[9 + i];
  }
}

static mcp_camera camera(double shift) {
  mcp_camera c; std::memset(&c, 0, sizeof c);
  c.params[0] = 250.0 + shift; c.params[1] = -0.0012; c.params[2] = 1e-7; c.params[3] = -1e-10; c.params[4] = 320.0 + shift; c.params[5] = 240.0 - shift;
  c.params[6] = 1.0; c.image_size[0] = 640; c.image_size[1] = 480; c.affine[0] = 1.0; c.affine[3] = 1.0; c.center[0] = 320.0 + shift; c.center[1] = 240.0 - shift;
  return c;
}

static int fail(const char* what, int a = 0, int b = 0) { std::printf("%s (%d, %d): %s\n", what, a, b, g_err.c_str()); return 1; }

// two cameras with n0 and n1 candidates, limits l0 and l1, a busy position on top of every third candidate of camera 0 (at `level`)
static int check_init(int n0, int n1, int l0, int l1, int level, int first_store) {
  const int ncam = 2, n_cand[2] = { n0, n1 }, limit[2] = { l0, l1 };
  double cfb[24], bfw[12];
  pose(0.01, -0.02, 0.015, 0.02, -0.01, 0.03, cfb); pose(-0.3, 0.8, 0.1, 0.11, 0.02, -0.04, cfb + 12); pose(0.2, 0.1, -0.3, 0.7, -1.1, 0.4, bfw);
  const mcp_camera cams[2] = { camera(0.0), camera(3.5) };
  const int w = 640 >> level;
  std::vector<mcp_int2> cand((size_t)n0 + n1);
  for (int i = 0; i < n0 + n1; ++i) { cand[i].x = 5 + (i*11) % (w - 10); cand[i].y = 4 + ((i*11)/(w - 10))*11 % ((480 >> level) - 8); }
  std::vector<mcp_stereo_meas> busy;
  for (int i = 0; i < n0; i += 3) busy.push_back(mcp_stereo_meas{{(cand[i].x + 0.5)*(1 << level) - 0.5, (cand[i].y + 0.5)*(1 << level) - 0.5}, level + (i % 2), 0});
  if (level == 3) for (mcp_stereo_meas& b : busy) b.level = 3;
  const int n_busy[2] = { (int)busy.size(), 0 };
  std::vector<uint8_t> want_keep((size_t)n0 + n1, 1);
  int alive[2] = { 0, 0 };
  // (the expected keep is the twin's own rule re-stated: every candidate within 10 level pixels of a busy one at level / level + 1 goes)
  for (int i = 0; i < n0; ++i)
    for (const mcp_stereo_meas& b : busy) {
      if (!(b.level == level || b.level == level + 1)) continue;
      const double sc = (double)(1 << level);
      const long long bx = (long long)(b.root_pos[0]/sc + 0.5), by = (long long)(b.root_pos[1]/sc + 0.5);      // positive positions: round half up
      const long long dx = bx - cand[i].x, dy = by - cand[i].y;
      if (dx*dx + dy*dy < 100) want_keep[i] = 0;
    }
  alive[0] = 0; for (int i = 0; i < n0; ++i) alive[0] += want_keep[i];
  alive[1] = n1;
  const int made0 = alive[0] < l0 ? alive[0] : l0, made1 = alive[1] < l1 ? alive[1] : l1, made = made0 + made1;
  const int n_rows = (n0 < l0 ? n0 : l0) + (n1 < l1 ? n1 : l1);                                              // exactly what the call asks for
  std::vector<int> rows(n_rows);
  for (int k = 0; k < n_rows; ++k) rows[k] = 1000 + 7*((k*13) % (n_rows + 1)) + k % 7;
  mcp_init_depth_params prm; prm.src_mkf = 3; prm.level = level; prm.init_depth = 2.5;
  mcp_init_depth_result res;
  std::vector<uint8_t> keep((size_t)n0 + n1, 0xee);
  std::vector<mcp_stereo_point> out(n_rows);
  std::vector<double> wp(3*(size_t)n_rows), pr(3*(size_t)n_rows), pd(3*(size_t)n_rows), rays(9*(size_t)n_rows);
  std::vector<int> cxy(2*(size_t)n_rows), gm(n_rows), gc(n_rows), gf(n_rows);
  std::vector<mcp_store_entry> ap(n_rows);
  const int rc = mcp_init_depth_points_host(ncam, cfb, bfw, cams, n_cand, cand.empty() ? nullptr : cand.data(), limit, n_busy, busy.empty() ? nullptr : busy.data(), n_rows,
                                            n_rows ? rows.data() : nullptr, &prm, first_store, &res, keep.empty() ? nullptr : keep.data(), n_rows ? out.data() : nullptr,
                                            n_rows ? wp.data() : nullptr, n_rows ? pr.data() : nullptr, n_rows ? pd.data() : nullptr, n_rows ? rays.data() : nullptr,
                                            n_rows ? cxy.data() : nullptr, n_rows ? gm.data() : nullptr, n_rows ? gc.data() : nullptr, n_rows ? gf.data() : nullptr,
                                            n_rows ? ap.data() : nullptr);
  if (rc != made || res.made_total != made || res.made[0] != made0 || res.made[1] != made1 || res.n_alive[0] != alive[0] || res.n_alive[1] != alive[1] ||
      res.first_store != first_store || res.n_busy[0] != n_busy[0]) return fail("init: counts", rc, made);
  if (!keep.empty() && std::memcmp(keep.data(), want_keep.data(), keep.size()) != 0) return fail("init: keep", n0, n1);
  double W[2][12];
  compose(cfb, bfw, W[0]); compose(cfb + 12, bfw, W[1]);
  int k = 0;
  for (int c = 0; c < 2; ++c) {
    int taken = 0;
    for (int i = 0; i < n_cand[c] && taken < (c ? made1 : made0); ++i) {
      if (!want_keep[(c ? n0 : 0) + i]) continue;
      const mcp_int2 C = cand[(c ? n0 : 0) + i];
      const mcp_store_entry& e = ap[k];
      if (out[k].candidate != i || out[k].target != -1 || cxy[2*k] != C.x || cxy[2*k + 1] != C.y || gm[k] != 3 || gc[k] != c || gf[k] != 0) return fail("init: record", c, i);
      if (e.mkf != 3 || e.cam != c || e.row != rows[k] || e.level != level || e.source != MCP_SRC_ROOT || e.alive != 1 || e.uv[0] != (C.x + 0.5)*(1 << level) - 0.5 ||
          e.uv[1] != (C.y + 0.5)*(1 << level) - 0.5) return fail("init: store entry", c, i);
      double pc[3], n2 = 0.0;
      for (int a = 0; a < 3; ++a) { pc[a] = W[c][3*a]*wp[3*k] + W[c][3*a + 1]*wp[3*k + 1] + W[c][3*a + 2]*wp[3*k + 2] + W[c][9 + a]; n2 += pc[a]*pc[a]; }
      if (std::fabs(std::sqrt(n2) - 2.5) > 1e-12) return fail("init: the point is not at init_depth", c, i);
      for (int v = 0; v < 3; ++v) {
        const double* r = &rays[9*(size_t)k + 3*v];
        if (std::fabs(r[0]*r[0] + r[1]*r[1] + r[2]*r[2] - 1.0) > 1e-14) return fail("init: a ray is not a unit vector", c, i);
      }
      if (std::memcmp(&wp[3*(size_t)k], out[k].world_pos, 24) != 0 || std::memcmp(&pr[3*(size_t)k], out[k].pixel_right_w, 24) != 0) return fail("init: columns differ from the record", c, i);
      ++k; ++taken;
    }
  }
  if (k != made) return fail("init: walk", k, made);
  // one row short: refused
  if (n_rows > 0) {
    if (mcp_init_depth_points_host(ncam, cfb, bfw, cams, n_cand, cand.data(), limit, n_busy, busy.empty() ? nullptr : busy.data(), n_rows - 1, rows.data(), &prm, first_store, &res,
                                   keep.data(), out.data(), wp.data(), pr.data(), pd.data(), rays.data(), cxy.data(), gm.data(), gc.data(), gf.data(), ap.data()) != -1 ||
        g_err.find("mcp_init_depth_points_host:") != 0) return fail("init: a short row list was not refused");
  }
  return 0;
}

static int check_mark(int n_rows, int n_prows, uint64_t seed) {
  uint64_t s = seed;
  std::vector<int> flags(n_prows);
  std::vector<uint8_t> usable(n_rows), before;
  int want = 0;
  for (int r = 0; r < n_prows; ++r) { flags[r] = (int)(rnd(s) % 4); if (r < n_rows && !(flags[r] & MCP_GP_BAD)) ++want; }
  for (int r = 0; r < n_rows; ++r) usable[r] = rnd(s) % 3 == 0;
  before = usable;
  const int got = mcp_map_mark_optimized_host(n_rows, n_prows, n_prows ? flags.data() : nullptr, n_rows ? usable.data() : nullptr);
  if (got != want) return fail("mark: count", got, want);
  for (int r = 0; r < n_rows; ++r) {
    const bool hit = r < n_prows && !(flags[r] & MCP_GP_BAD);
    if (usable[r] != (hit ? 1 : before[r])) return fail("mark: a byte", r, n_rows);
  }
  return 0;
}

struct Map { std::vector<double> bfw, world, pr, pd, rays; std::vector<int> mflags, sm, sc; std::vector<uint8_t> has; };
static bool same(const Map& a, const Map& b) {
  auto eq = [](const std::vector<double>& x, const std::vector<double>& y) { return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), 8*x.size()) == 0); };
  return eq(a.bfw, b.bfw) && eq(a.world, b.world) && eq(a.pr, b.pr) && eq(a.pd, b.pd);
}
static int move(Map& m, int kind, double scale, const double* T, const double* cfb, mcp_map_transform_result* res) {
  const int n_slots = (int)m.mflags.size(), n_rows = (int)m.has.size(), n_prows = (int)m.sm.size();
  return mcp_map_transform_host(kind, scale, T, 2, cfb, n_slots, n_slots ? m.bfw.data() : nullptr, n_slots ? m.mflags.data() : nullptr, n_rows, n_prows, n_prows ? m.sm.data() : nullptr,
                                n_prows ? m.sc.data() : nullptr, n_rows ? m.has.data() : nullptr, n_rows ? m.rays.data() : nullptr, n_rows ? m.world.data() : nullptr,
                                n_rows ? m.pr.data() : nullptr, n_rows ? m.pd.data() : nullptr, res);
}
static int check_transform(int n_rows, int n_slots, int n_prows, uint64_t seed) {
  uint64_t s = seed;
  double cfb[24];
  pose(0.01, -0.02, 0.015, 0.02, -0.01, 0.03, cfb); pose(-0.3, 0.8, 0.1, 0.11, 0.02, -0.04, cfb + 12);
  Map m;
  m.bfw.resize(12*(size_t)n_slots); m.mflags.resize(n_slots);
  int present = 0;
  for (int k = 0; k < n_slots; ++k) {
    pose(nonzero(s)*0.1, nonzero(s)*0.1, nonzero(s)*0.1, nonzero(s), nonzero(s), nonzero(s), &m.bfw[12*(size_t)k]);
    m.mflags[k] = (k % 5 == 2) ? 0 : (MCP_MKF_PRESENT | (k % 7 == 3 ? MCP_MKF_BAD : 0));
    present += (m.mflags[k] & MCP_MKF_PRESENT) ? 1 : 0;
  }
  m.world.resize(3*(size_t)n_rows); m.pr.resize(3*(size_t)n_rows); m.pd.resize(3*(size_t)n_rows); m.rays.resize(9*(size_t)n_rows); m.has.resize(n_rows);
  m.sm.resize(n_prows); m.sc.resize(n_prows);
  int want_refreshed = 0, want_no_rays = 0, want_no_source = 0;
  for (int r = 0; r < n_rows; ++r) {
    for (int a = 0; a < 3; ++a) { m.world[3*(size_t)r + a] = nonzero(s); m.pr[3*(size_t)r + a] = nonzero(s)*0.01; m.pd[3*(size_t)r + a] = nonzero(s)*0.01; }
    for (int v = 0; v < 3; ++v) {
      double* q = &m.rays[9*(size_t)r + 3*v];
      q[0] = nonzero(s)*0.1; q[1] = nonzero(s)*0.1; q[2] = 1.0;
      const double n = std::sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2]); q[0] /= n; q[1] /= n; q[2] /= n;
    }
    m.has[r] = r % 11 != 4;
    bool source = false;
    if (r < n_prows) {
      m.sm[r] = r % 13 == 5 ? -1 : (n_slots ? (int)(rnd(s) % n_slots) : 0); m.sc[r] = r % 17 == 6 ? 2 : (int)(rnd(s) % 2);
      source = m.sm[r] >= 0 && m.sm[r] < n_slots && m.sc[r] < 2 && (m.mflags[m.sm[r]] & MCP_MKF_PRESENT);
    }
    if (!source) ++want_no_source; else if (m.has[r]) ++want_refreshed; else ++want_no_rays;
  }
  const Map start = m;
  mcp_map_transform_result res;
  double T[12], I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  pose(0.3, -0.5, 0.2, 1.5, -0.7, 0.9, T);
  if (move(m, 1, 1.0, T, cfb, &res) != 0) return fail("transform: refused", n_rows, n_slots);
  if (res.n_rows != n_rows || res.n_mkfs != present || res.n_refreshed != want_refreshed || res.n_no_rays != want_no_rays || res.n_no_source != want_no_source)
    return fail("transform: counters", n_rows, n_slots);
  for (int k = 0; k < n_slots; ++k)
    if (!(m.mflags[k] & MCP_MKF_PRESENT) && std::memcmp(&m.bfw[12*(size_t)k], &start.bfw[12*(size_t)k], 96) != 0) return fail("transform: an absent slot moved", k);
  const Map moved = m;
  if (move(m, 1, 1.0, I, cfb, &res) != 0 || !same(m, moved)) return fail("transform: the identity changed a bit", n_rows, n_slots);
  if (move(m, 0, 1.0, nullptr, cfb, &res) != 0 || !same(m, moved)) return fail("transform: a scale of 1 changed a bit", n_rows, n_slots);
  if (move(m, 0, 2.0, nullptr, cfb, &res) != 0 || (want_refreshed && same(m, moved))) return fail("transform: a scale of 2 changed nothing", n_rows, n_slots);
  if (move(m, 0, 0.5, nullptr, cfb, &res) != 0 || !same(m, moved)) return fail("transform: 2 then 0.5 did not return", n_rows, n_slots);
  // refusals leave the arrays alone
  double bad[12]; std::memcpy(bad, I, sizeof I); bad[1] = 1e-6;
  if (move(m, 1, 1.0, bad, cfb, &res) != -1 || g_err.find("mcp_map_transform_host:") != 0 || !same(m, moved)) return fail("transform: a skewed rotation was not refused");
  if (move(m, 0, 0.0, nullptr, cfb, &res) != -1 || move(m, 0, -1.0, nullptr, cfb, &res) != -1 || move(m, 0, NAN, nullptr, cfb, &res) != -1 || !same(m, moved))
    return fail("transform: a bad scale was not refused");
  return 0;
}

int main() {
  int bad = 0;
  const int init[][6] = { {0, 1, 5, 5, 1, 0}, {40, 7, 0, 3, 1, 17}, {30, 12, 1000, 1 << 30, 2, 0}, {600, 300, 255, 5, 0, 4099}, {600, 300, 256, 5, 0, 4099}, {600, 300, 257, 5, 0, 4099},
                          {20, 20, 20, 20, 3, 0}, {0, 0, 3, 3, 0, 0} };
  for (const auto& c : init) bad += check_init(c[0], c[1], c[2], c[3], c[4], c[5]);
  const int mark[][2] = { {0, 0}, {1, 1}, {255, 255}, {256, 200}, {257, 257}, {300, 0}, {100, 180} };
  for (const auto& c : mark) bad += check_mark(c[0], c[1], 7 + c[0]);
  const int xf[][3] = { {0, 0, 0}, {0, 4, 0}, {1, 4, 1}, {255, 4, 255}, {256, 9, 256}, {257, 9, 200}, {150, 0, 150} };
  for (const auto& c : xf) bad += check_transform(c[0], c[1], c[2], 11 + c[0]);
  if (bad) { std::printf("%d checks failed\n", bad); return 1; }
  std::printf("map life host ok\n");
  return 0;
}
