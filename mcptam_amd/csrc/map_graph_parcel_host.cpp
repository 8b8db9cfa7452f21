// mcp_parcel_commit_host (include/mcp_img.h): the commit of a measurement parcel (map_graph_parcel.h) from host arrays.  Host code only -- this
// unit sees none of HIP, so it also builds with a plain C++ compiler next to a main() of its own (tests/cpp/parcel_commit_host_check.cpp, which
// the sanitizers read).  The bodies are the ones the kernels call.
#include <string>
#define MGP_HOST_ONLY
#include "map_graph_parcel.h"

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int parcel_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }

extern "C" int mcp_parcel_commit_host(int n, const mcp_parcel_entry* entries, int n_rows, const int* keys, int n_point_rows, const int* point_flags, const int* src_mkf,
                                      const int* src_cam, int n_lanes, const int* lane_mkf, const int* lane_cam, const mcp_parcel_commit_params* params, int first,
                                      uint8_t* verdict, mcp_store_entry* appended, mcp_parcel_commit_result* res, int* lane_appended) {
  const std::string who = "mcp_parcel_commit_host";
  if (!params || !res) return parcel_fail(who + ": NULL params or result");
  if (n < 0 || n_rows < 0 || n_point_rows < 0 || n_point_rows > n_rows || n_lanes < 0 || first < 0 || (n > 0 && !entries) || (n_rows > 0 && !keys) ||
      (n_point_rows > 0 && (!point_flags || !src_mkf || !src_cam)) || (n_lanes > 0 && (!lane_mkf || !lane_cam))) return parcel_fail(who + ": bad arguments");
  for (int i = 0; i < n; ++i)
    if (entries[i].lane < 0 || entries[i].lane >= n_lanes) return parcel_fail(who + ": entry " + std::to_string(i) + " names lane " + std::to_string(entries[i].lane) + " of " + std::to_string(n_lanes));
  const mcp::MgpHostIn I{n, entries, mcp::MgpMap{n_rows, n_point_rows, keys, 1, src_mkf, src_cam, point_flags, 1}, n_lanes, lane_mkf, lane_cam, params->cross_camera, params->source};
  int counts[5];
  const int got = mcp::mgp_host_commit(I, verdict, appended, counts, lane_appended);
  res->first = first; res->n_appended = counts[MCP_PARCEL_APPENDED]; res->n_skipped_lane = counts[MCP_PARCEL_SKIPPED]; res->n_stale = counts[MCP_PARCEL_STALE];
  res->n_bad = counts[MCP_PARCEL_BAD]; res->n_cross = counts[MCP_PARCEL_CROSS];
  return got;
}
