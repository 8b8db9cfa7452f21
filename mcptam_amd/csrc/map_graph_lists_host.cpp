// mcp_graph_kf_lists_host (include/mcp_img.h): the keyframe lists of map_graph_lists.h from host arrays.  Host code only -- this unit sees
// none of HIP, so it also builds with a plain C++ compiler next to a main() of its own (tests/cpp/kf_lists_host_check.cpp, which the
// sanitizers read).  The bodies are the ones the kernels call.
#include <string>
#include <vector>
#define MGL_HOST_ONLY
#include "map_graph_lists.h"

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int lists_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }

extern "C" int mcp_graph_kf_lists_host(int ncam, int n_slots, const int* mkf_flags, const uint8_t* kf_active, int n_rows, int n_point_rows, const int* point_flags,
                                       const int* inlier, const int* outlier, int n_store, const int* ms_mkf, const int* ms_cam, const int* ms_row,
                                       const uint8_t* ms_alive, int n_mkfs, const int* slots, int* seg_start, int cap, int* seg_rows, double* seg_w) {
  const std::string who = "mcp_graph_kf_lists_host";
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || n_slots < 0 || n_slots > MCP_MAP_MAX_MKFS || n_rows < 0 || n_point_rows < 0 || n_point_rows > n_rows || n_store < 0 || cap < 0 ||
      n_mkfs < 0 || !seg_start || (n_slots > 0 && (!mkf_flags || !kf_active)) || (n_point_rows > 0 && !point_flags) || (n_rows > 0 && (!inlier || !outlier)) ||
      (n_store > 0 && (!ms_mkf || !ms_cam || !ms_row || !ms_alive)) || (n_mkfs > 0 && !slots) || (cap > 0 && (!seg_rows || !seg_w)))
    return lists_fail(who + ": bad arguments");
  if (n_mkfs > MCP_MAP_MAX_MKFS) return lists_fail(who + ": more than MCP_MAP_MAX_MKFS MKFs");
  std::vector<int> pos_of((size_t)n_slots + 1, -1), fill((size_t)n_mkfs*ncam + 1, 0);
  for (int i = 0; i < n_mkfs; ++i) {
    const int s = slots[i];
    if (s < 0 || s >= n_slots) return lists_fail(who + ": slot " + std::to_string(s) + " is outside the MKF columns");
    if (!(mkf_flags[s] & MCP_MKF_PRESENT)) return lists_fail(who + ": MKF slot " + std::to_string(s) + " is not present");
    if (pos_of[s] >= 0) return lists_fail(who + ": slot " + std::to_string(s) + " appears twice");
    pos_of[s] = i;
  }
  for (int r = 0; r < n_rows; ++r)
    if (inlier[r] < 1 || outlier[r] < 0) return lists_fail(who + ": row " + std::to_string(r) + " has inlier < 1 or outlier < 0");      // (as mcp_map_points_set_counts refuses them)
  const mcp::MglHostIn I{ncam, n_slots, kf_active, n_rows, n_point_rows, point_flags, inlier, outlier, n_store, ms_mkf, ms_cam, ms_row, ms_alive, n_mkfs, slots};
  const int total = mcp::mgl_host_lists(I, pos_of.data(), fill.data(), seg_start, cap, seg_rows, seg_w);
  if (total < 0) return lists_fail(who + ": the lists hold " + std::to_string(seg_start[n_mkfs*ncam]) + " entries, the caller's arrays " + std::to_string(cap));
  return total;
}
