// MapGraph.hpp -- C++ host-side mirror of the map's beginning, its rescale and its re-alignment on the device-resident map graph, over the C ABI
// of mcp_img.h: MapMakerServerBase::AddInitDepthMapPoints (src/MapMakerServerBase.cc:499-546), the mbOptimized loop at the end of
// InitFromMultiKeyFrame (:212-215), ApplyGlobalScaleToMap (:549-574) and ApplyGlobalTransformationToMap (:577-596).
//
// The class does not own the graph: it wraps an mcp_map_graph* that the map owns (shim/BundleAdjusterBase_gpu.cc creates it next to the map-point
// table).  TooN types are replaced by plain arrays (SE3 = row-major R[9] + t[3] as 12 doubles), so that the header depends on the C ABI only; a
// MCPTAM tree uses the TooN-typed bodies of shim/MapMakerServerBase_gpu.cc.  There is no CPU fallback: a failed call throws with mcp_last_error().
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../mcp_img.h"

namespace mcptam_hip {

/// What one AddInitDepthMapPoints call made: the records in creation order (camera-major, then candidate order; record k took rows[k]), the
/// thinning's verdict per camera (vCandidates = vCGood) and the call's counts.
struct InitDepthPoints {
  std::vector<mcp_stereo_point> vPoints;
  std::vector<std::vector<uint8_t>> vKeep;
  mcp_init_depth_result result;
};

class MapGraph {
 public:
  /// nCams: the cameras of the graph's rig (mcp_map_graph_create's ncam)
  MapGraph(mcp_map_graph* pGraph, int nCams) : mpGraph(pGraph), mnCams(nCams) {
    if (!mpGraph || nCams < 1 || nCams > MCP_MAX_FRAME_CAMS) throw std::invalid_argument("MapGraph: NULL graph or bad camera count");
  }
  mcp_map_graph* handle() const { return mpGraph; }

  /// AddInitDepthMapPoints(mkfSrc, nLevel, nLimit, dInitDepth) for every camera of the rig in one call.  vCams[c]: the keyframe, camera, candidates
  /// and nLimit of the rig's camera c.  vRows / vKeys: free rows and their keys, at least the sum of min(n_cand, limit).
  InitDepthPoints AddInitDepthMapPoints(int nSrcMKF, int nLevel, double dInitDepth, const std::vector<mcp_init_depth_cam>& vCams, const std::vector<int>& vRows,
                                        const std::vector<int>& vKeys) {
    if (vRows.size() != vKeys.size()) throw std::invalid_argument("AddInitDepthMapPoints: rows and keys differ in length");
    InitDepthPoints out;
    size_t nTotal = 0;
    for (const mcp_init_depth_cam& c : vCams) nTotal += (size_t)(c.n_cand > 0 ? c.n_cand : 0);
    std::vector<uint8_t> vKeepAll(nTotal + 1);
    out.vPoints.resize(vRows.size() + 1);
    mcp_init_depth_params params;
    params.src_mkf = nSrcMKF; params.level = nLevel; params.init_depth = dInitDepth;
    const int nMade = mcp_init_depth_map_points(mpGraph, (int)vCams.size(), vCams.data(), (int)vRows.size(), vRows.data(), vKeys.data(), &params, &out.result,
                                                out.vPoints.data(), vKeepAll.data());
    if (nMade < 0) throw std::runtime_error(mcp_last_error());
    out.vPoints.resize((size_t)nMade);
    size_t at = 0;
    for (const mcp_init_depth_cam& c : vCams) {
      out.vKeep.emplace_back(vKeepAll.begin() + at, vKeepAll.begin() + at + c.n_cand);
      at += (size_t)c.n_cand;
    }
    return out;
  }

  /// mbOptimized = true on every point of the map (the end of InitFromMultiKeyFrame); returns how many rows became usable candidates
  int MarkOptimized() {
    int n = 0;
    check(mcp_map_mark_optimized(mpGraph, &n));
    return n;
  }

  /// ApplyGlobalScaleToMap(dScale).  vDepth (may be null): the scene depths of the present MKFs x cameras in ascending slot order.
  mcp_map_transform_result ApplyGlobalScaleToMap(double dScale, std::vector<mcp_scene_depth>* vDepth = nullptr) {
    mcp_map_transform_result res;
    std::vector<mcp_scene_depth> depth(vDepth ? (size_t)MCP_MAP_MAX_MKFS*mnCams : 0);      // (a keyframe that was left alone keeps refreshed = 0 here)
    check(mcp_map_rescale(mpGraph, dScale, &res, vDepth ? depth.data() : nullptr));
    if (vDepth) { depth.resize((size_t)res.n_mkfs*mnCams); vDepth->swap(depth); }
    return res;
  }

  /// ApplyGlobalTransformationToMap(se3NewFromOld)
  mcp_map_transform_result ApplyGlobalTransformationToMap(const std::array<double, 12>& se3NewFromOld) {
    mcp_map_transform_result res;
    check(mcp_map_transform(mpGraph, se3NewFromOld.data(), &res));
    return res;
  }

  /// Tracker::CollectNearestPoints with tracker_collect_all_points false, at the tracker's pose se3BaseFromWorld, for the cameras of params.active:
  /// the report, and (vNear non-null) one byte per table row whose bit c says that the row is a co-visible point of the map keyframe nearest to
  /// current keyframe c.  pCamFromBase: the current keyframes' (nCams x 12), or null for the rig's.
  mcp_collect_report CollectNearestPoints(const std::array<double, 12>& se3BaseFromWorld, const mcp_collect_params& params, std::vector<uint8_t>* vNear = nullptr,
                                          const double* pCamFromBase = nullptr) {
    mcp_collect_report rep;
    check(mcp_map_collect_nearest(mpGraph, se3BaseFromWorld.data(), pCamFromBase, &params, &rep, nullptr));
    if (vNear) {
      int n = 0;
      const uint8_t* p = mcp_map_collect_rows_view(mpGraph, &n);
      vNear->assign(p, p + n);
    }
    return rep;
  }

  /// The frame mode: while it is on, FindPVS and the one-call frames of pTable (the graph's table) judge only those rows.  Host-only; call it
  /// before every frame with the current keyframes' mdSceneDepthMean.  TrackCollectAllPoints switches it off again (the default).
  void TrackCollectNearestPoints(mcp_map_points* pTable, const mcp_collect_params& params) { check(mcp_track_collect_nearest(pTable, mpGraph, &params)); }
  static void TrackCollectAllPoints(mcp_map_points* pTable) { check(mcp_track_collect_nearest(pTable, nullptr, nullptr)); }
  /// The report of the last FindPVS / frame call on pTable with the mode on
  static mcp_collect_report TrackCollectLast(const mcp_map_points* pTable) {
    mcp_collect_report rep;
    check(mcp_track_collect_last(pTable, &rep));
    return rep;
  }

 private:
  static void check(int rc) { if (rc < 0) throw std::runtime_error(mcp_last_error()); }
  mcp_map_graph* mpGraph;
  int mnCams;
};

}  // namespace mcptam_hip
