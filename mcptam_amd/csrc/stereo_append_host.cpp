// mcp_stereo_busy_host / mcp_stereo_append_host (include/mcp_img.h): the busy list and the append of mcp_stereo_map_points (stereo_append.h) from
// host arrays.  Host code only -- this unit sees none of HIP, so it also builds with a plain C++ compiler next to a main() of its own
// (tests/cpp/stereo_append_host_check.cpp, which the sanitizers read).  The bodies are the ones the kernels call.
#include <string>
#define SA_HOST_ONLY
#include "stereo_append.h"

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int append_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }

extern "C" int mcp_stereo_busy_host(int n_store, const mcp_store_entry* store, int src_mkf, int src_cam, int cap, mcp_stereo_meas* out) {
  const std::string who = "mcp_stereo_busy_host";
  if (n_store < 0 || cap < 0 || (n_store > 0 && !store) || (cap > 0 && !out)) return append_fail(who + ": bad arguments");
  const int n = mcp::sa_host_busy(n_store, store, src_mkf, src_cam, cap, cap > 0 ? out : nullptr);
  if (cap > 0 && n > cap) return append_fail(who + ": the busy list has " + std::to_string(n) + " entries, the caller's array " + std::to_string(cap));
  return n;
}

extern "C" int mcp_stereo_append_host(int made, const mcp_stereo_point* pts, const int* rows, int level, int src_mkf, int src_cam, const int* target_mkf,
                                      const int* target_cam, int first_store, double* world_pos, double* pixel_right_w, double* pixel_down_w, double* rays,
                                      int* center_xy, int* gp_src_mkf, int* gp_src_cam, int* gp_flags, mcp_store_entry* appended) {
  const std::string who = "mcp_stereo_append_host";
  if (made < 0 || first_store < 0 || level < 0 || level >= MCP_LEVELS || (long long)first_store + 2LL*made > 0x7fffffffLL) return append_fail(who + ": bad arguments");
  if (made > 0 && (!pts || !rows || !target_mkf || !target_cam || !world_pos || !pixel_right_w || !pixel_down_w || !rays || !center_xy || !gp_src_mkf || !gp_src_cam ||
                   !gp_flags || !appended)) return append_fail(who + ": a NULL array");
  for (int k = 0; k < made; ++k)
    if (pts[k].target < 0) return append_fail(who + ": record " + std::to_string(k) + " names target " + std::to_string(pts[k].target));
  for (int k = 0; k < made; ++k) {
    mcp::SaRow R;
    mcp::sa_point(pts[k], rows[k], level, src_mkf, src_cam, target_mkf[pts[k].target], target_cam[pts[k].target], R, appended[2*(size_t)k], appended[2*(size_t)k + 1]);
    for (int a = 0; a < 3; ++a) {
      world_pos[3*(size_t)k + a] = R.world_pos[a]; pixel_right_w[3*(size_t)k + a] = R.pixel_right_w[a]; pixel_down_w[3*(size_t)k + a] = R.pixel_down_w[a];
    }
    for (int a = 0; a < 9; ++a) rays[9*(size_t)k + a] = R.rays[a];
    center_xy[2*(size_t)k] = R.cx; center_xy[2*(size_t)k + 1] = R.cy;
    gp_src_mkf[k] = R.gp_src_mkf; gp_src_cam[k] = R.gp_src_cam; gp_flags[k] = R.gp_flags;
  }
  return first_store + 2*made;
}
