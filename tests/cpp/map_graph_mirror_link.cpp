// include/mcptam_hip/MapGraph.hpp against the C ABI: every member is instantiated and must link against libmcptam_hip.so; without a device the
// program checks what the mirror refuses on its own (a NULL graph, a camera count outside the rig's range) and that the library's refusal of a
// NULL graph reaches the caller as an exception carrying mcp_last_error().
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include "mcptam_hip/MapGraph.hpp"

using mcptam_hip::MapGraph;

// never run: takes every member through the linker
static void instantiate(MapGraph& g) {
  std::vector<mcp_init_depth_cam> cams(1);
  std::memset(&cams[0], 0, sizeof cams[0]);
  (void)g.AddInitDepthMapPoints(0, 1, 2.0, cams, std::vector<int>(), std::vector<int>());
  (void)g.MarkOptimized();
  std::vector<mcp_scene_depth> depth;
  (void)g.ApplyGlobalScaleToMap(2.0, &depth);
  (void)g.ApplyGlobalTransformationToMap(std::array<double, 12>{{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}});
  (void)g.handle();
}

template <class F> static bool throws(F f) { try { f(); } catch (const std::exception&) { return true; } return false; }

int main(int argc, char** argv) {
  int bad = 0;
  int dummy = 0;
  mcp_map_graph* fake = reinterpret_cast<mcp_map_graph*>(&dummy);      // (never dereferenced: only the constructor's own checks run on it)
  bad += !throws([] { MapGraph g(nullptr, 2); });
  bad += !throws([&] { MapGraph g(fake, 0); });
  bad += !throws([&] { MapGraph g(fake, MCP_MAX_FRAME_CAMS + 1); });
  bad += throws([&] { MapGraph g(fake, MCP_MAX_FRAME_CAMS); });
  // the library's own refusals arrive as exceptions with its message
  mcp_map_transform_result res;
  if (mcp_map_rescale(nullptr, 2.0, &res, nullptr) != -1 || std::string(mcp_last_error()).find("mcp_map_rescale:") != 0) ++bad;
  if (mcp_map_transform(nullptr, nullptr, &res) != -1 || std::string(mcp_last_error()).find("mcp_map_transform:") != 0) ++bad;
  if (mcp_map_mark_optimized(nullptr, nullptr) != -1 || std::string(mcp_last_error()).find("mcp_map_mark_optimized:") != 0) ++bad;
  if (argc > 99) { MapGraph g(fake, 1); instantiate(g); }
  if (bad) { std::printf("%d checks failed\n", bad); return 1; }
  std::printf("map graph mirror linked%s\n", argc > 1 && !std::strcmp(argv[1], "--link-only") ? "" : " (no device part)");
  return 0;
}
