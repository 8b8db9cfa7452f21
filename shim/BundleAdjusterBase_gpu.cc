// BundleAdjusterBase_gpu.cc -- BundleAdjustAll / BundleAdjustRecent and the population of BundleAdjusterMulti::BundleAdjust over the
// device-resident map graph (include/mcp_img.h: mcp_map_graph_*, mcp_map_bundle_select), and AdjustAndUpdate's write-back over the same graph
// (mcp_graph_write_back, mcp_graph_refresh_depth).
//
// Replaces src/BundleAdjusterBase.cc:141-184 (BundleAdjustAll) and :188-265 (BundleAdjustRecent) -- delete those two bodies -- and the
// population loops of src/BundleAdjusterMulti.cc:81-200, which become BundleAdjusterMulti::BundleAdjustSelected below; the solve and the
// outlier decoding behind them (:205-264) stay as they are, fed by the id vectors this file fills instead of the std::maps.
// Replaces BundleAdjusterMulti::AdjustAndUpdate (src/BundleAdjusterMulti.cc:286-334) as well: one mcp_graph_write_back.
// Header deltas:
//   include/mcptam/Map.h, class Map:          mcp_map_points* mpMapTable; mcp_map_graph* mpMapGraph;      (created with the map, destroyed --
//                                             graph first -- with it; the table is the tracker's, shim/Tracker_gpu.cc option (b))
//   include/mcptam/KeyFrame.h, MultiKeyFrame: int mnGraphSlot;     (-1 until the MKF enters the map; slots of trashed MKFs are reused)
//                                             mcp_meas_parcel* mpMeasParcel;   (the tracker's measurements of a queued MKF, GraphCommitTrackerParcel)
//   include/mcptam/KeyFrame.h, KeyFrame:      int mnCamIndex;      (index of mCamName in the rig the graph was created with)
//   include/mcptam/MapPoint.h, MapPoint:      int mnTableRow;      (shim/MapMakerServerBase_gpu.cc has it already)
//   include/mcptam/BundleAdjusterMulti.h:     std::vector<std::string> mvCamNames (the rig's camera names in graph order); std::vector<int> mvMKFBundleID,
//                                             mvCamBundleID, mvPointBundleID, mvWriteBackRows, mvWriteBackSlots; int SolveAndDecode(...): the body
//                                             of src/BundleAdjusterMulti.cc:205-264 moved into a member, reading these vectors instead of the maps;
//                                             void AdjustAndUpdate(ChainBundle&) takes the bundle alone (the sets it walked are the vectors above)
//   shim/ChainBundle.h:                       mcp_ba* Handle() { return mpHandle; }   (AdjustAndUpdate hands it to mcp_graph_write_back)
//   include/mcptam/BundleAdjusterBase.h:      virtual int BundleAdjustSelected(const mcp_bundle_select_result&, std::vector<std::pair<KeyFrame*,
//                                             MapPoint*> >& vOutliers, bool bRecent) = 0;   std::vector<MultiKeyFrame*> mvpSlotMKF;
//                                             std::vector<MapPoint*> mvpRowPoint;  (slot -> MKF, row -> point: kept by the map maker)
// The orders of the bundle are the library's (ascending slot, row, store index), not the pointer orders of the std::sets; the solver does
// not depend on them.  The deviations (tie-break by slot, the short closest list, the dropped-source rule, status 3) are listed in
// include/mcp_img.h.
#include <mcptam/BundleAdjusterBase.h>
#include <mcptam/BundleAdjusterMulti.h>
#include <mcptam/ChainBundle.h>
#include <mcptam/Map.h>
#include <mcptam/MapPoint.h>
#include <mcptam/KeyFrame.h>
#include <mcptam/LevelHelpers.h>
#include <mcp_img.h>
#include <gvars3/instances.h>
#include <ros/ros.h>

using namespace GVars3;

namespace
{
void Pose12(const TooN::SE3<>& se3, double* a)
{
  const TooN::Matrix<3> m3 = se3.get_rotation().get_matrix();
  for(int r = 0; r < 3; ++r)
    for(int c = 0; c < 3; ++c)
      a[3 * r + c] = m3(r, c);
  for(int r = 0; r < 3; ++r)
    a[9 + r] = se3.get_translation()[r];
}
TooN::SE3<> SE3From12(const double* a)
{
  TooN::Matrix<3> m3;
  for(int r = 0; r < 3; ++r)
    for(int c = 0; c < 3; ++c)
      m3(r, c) = a[3 * r + c];
  return TooN::SE3<>(TooN::SO3<>(m3), TooN::makeVector(a[9], a[10], a[11]));
}

int RunSelect(Map& map, int nMode, MultiKeyFrame* pNewest, mcp_bundle_select_result& res)
{
  mcp_bundle_select_params params;
  params.mode = nMode;
  params.newest = pNewest ? pNewest->mnGraphSlot : -1;
  params.n_recent = BundleAdjusterBase::snRecentNum;
  params.recent_min_size = BundleAdjusterBase::snRecentMinSize;
  params.min_points = BundleAdjusterBase::snMinMapPoints;
  params.mean_diff_fraction = KeyFrame::sdDistanceMeanDiffFraction;
  if(mcp_map_bundle_select(map.mpMapGraph, &params, &res) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_bundle_select: " << mcp_last_error());
    ROS_BREAK();
  }
  if(res.status == 3)   // KeyFrame::Distance's ROS_BREAK, src/KeyFrame.cc:734-744
  {
    ROS_FATAL("BundleAdjusterBase: an MKF distance is not finite or larger than 1e10");
    ROS_BREAK();
  }
  return res.status;
}
}  // namespace

// ---- where the graph is kept current (the map maker's side; each is a few lines next to the reference's own bookkeeping) -------------------
// MultiKeyFrame enters the map (MapMakerServerBase::AddMultiKeyFrameFromTopOfQueue and the two initialisers): take a free slot, then mcp_map_graph_update_mkfs with its pose, flags and the mbActive / mdSceneDepthMean of its keyframes.
// The same call when mbFixed / mbBad / mbActive change (MarkFurthestMultiKeyFrameAsBad) or the host moves a pose itself.  NOT after an adjustment
// and not after a scene-depth refresh: mcp_graph_write_back and mcp_graph_refresh_depth leave the poses and depth means they produce in the graph.
void GraphUploadMKFs(Map& map, const std::vector<MultiKeyFrame*>& vpMKFs, const std::vector<std::string>& vCamNames)
{
  const int n = (int)vpMKFs.size(), nc = (int)vCamNames.size();
  std::vector<int> vSlots(n), vFlags(n);
  std::vector<double> vPoses(12 * n), vDepth(n * nc, 0.0);
  std::vector<uint8_t> vActive(n * nc, 0);
  for(int i = 0; i < n; ++i)
  {
    MultiKeyFrame& mkf = *vpMKFs[i];
    vSlots[i] = mkf.mnGraphSlot;
    vFlags[i] = MCP_MKF_PRESENT | (mkf.mbFixed ? MCP_MKF_FIXED : 0) | (mkf.mbBad ? MCP_MKF_BAD : 0);
    Pose12(mkf.mse3BaseFromWorld, &vPoses[12 * i]);
    for(int c = 0; c < nc; ++c)
    {
      KeyFramePtrMap::iterator kf_it = mkf.mmpKeyFrames.find(vCamNames[c]);
      if(kf_it == mkf.mmpKeyFrames.end() || !kf_it->second->mbActive)
        continue;
      vActive[i * nc + c] = 1;
      vDepth[i * nc + c] = kf_it->second->mdSceneDepthMean;
    }
  }
  if(mcp_map_graph_update_mkfs(map.mpMapGraph, n, vSlots.data(), vPoses.data(), vFlags.data(), vActive.data(), vDepth.data()) != 0)
    ROS_ERROR_STREAM("mcp_map_graph_update_mkfs: " << mcp_last_error());
}

// MultiKeyFrame trashed (Map::MoveBadMultiKeyFramesToTrash): its entries die, its slot is free again
void GraphEraseMKF(Map& map, MultiKeyFrame& mkf)
{
  mcp_map_graph_erase_mkf(map.mpMapGraph, mkf.mnGraphSlot);
  mkf.mnGraphSlot = -1;
}

// MapPoint created, its source set, mbFixed / mbBad changed by the host (initialisers other than InitFromMultiKeyFrame, HandleBadPoints): the graph columns of its row.
// Not for the rows HandleOutliers / HandleBadEntities turn bad: the device marks those itself (mcp_map_cull_*) and reports them; and not for the points of
// AddStereoMapPoints / AddInitDepthMapPoints, whose rows mcp_stereo_map_points / mcp_init_depth_map_points write on the device (shim/MapMakerServerBase_gpu.cc).  Its MapPoint columns go to the table as before.
void GraphUploadPoints(Map& map, const std::vector<MapPoint*>& vpPoints)
{
  const int n = (int)vpPoints.size();
  std::vector<int> vRows(n), vSrcMKF(n), vSrcCam(n), vFlags(n);
  for(int i = 0; i < n; ++i)
  {
    MapPoint& point = *vpPoints[i];
    vRows[i] = point.mnTableRow;
    vSrcMKF[i] = point.mpPatchSourceKF ? point.mpPatchSourceKF->mpParent->mnGraphSlot : -1;
    vSrcCam[i] = point.mpPatchSourceKF ? point.mpPatchSourceKF->mnCamIndex : 0;
    vFlags[i] = (point.mbFixed ? MCP_GP_FIXED : 0) | (point.mbBad ? MCP_GP_BAD : 0);
  }
  if(mcp_map_graph_update_points(map.mpMapGraph, n, vRows.data(), vSrcMKF.data(), vSrcCam.data(), vFlags.data()) != 0)
    ROS_ERROR_STREAM("mcp_map_graph_update_points: " << mcp_last_error());
}

// KeyFrame::AddMeasurement, batched by the caller that makes many from host data (the initialisers): one append.
// MeasPtrMap guarantees one entry per (keyframe, point), which is what the store relies on.  The tracker's measurements of a new MKF,
// ReFindBatch's and the two measurements of every point AddStereoMapPoints creates do not come through here any more: they are on the device
// already (GraphCommitTrackerParcel / GraphCommitReFindParcel / mcp_stereo_map_points).
void GraphAddMeasurements(Map& map, const std::vector<std::pair<KeyFrame*, MapPoint*> >& vPairs)
{
  const int n = (int)vPairs.size();
  std::vector<int> vMKF(n), vCam(n), vRow(n), vLevel(n), vSource(n);
  std::vector<double> vUV(2 * n);
  for(int i = 0; i < n; ++i)
  {
    KeyFrame& kf = *vPairs[i].first;
    const Measurement& meas = *kf.mmpMeasurements[vPairs[i].second];
    vMKF[i] = kf.mpParent->mnGraphSlot;
    vCam[i] = kf.mnCamIndex;
    vRow[i] = vPairs[i].second->mnTableRow;
    vUV[2 * i] = meas.v2RootPos[0];
    vUV[2 * i + 1] = meas.v2RootPos[1];
    vLevel[i] = meas.nLevel;
    vSource[i] = (int)meas.eSource;
  }
  if(mcp_map_graph_add_meas(map.mpMapGraph, n, vMKF.data(), vCam.data(), vRow.data(), vUV.data(), vLevel.data(), vSource.data()) < 0)
    ROS_ERROR_STREAM("mcp_map_graph_add_meas: " << mcp_last_error());
}

// The tracker's measurements of an MKF that enters the map (MapMakerServerBase::AddMultiKeyFrameFromTopOfQueue, after GraphUploadMKFs has
// given it its slot): the parcel Tracker::RecordMeasurements filled when the MKF was made (shim/Tracker_gpu.cc) is committed as the map
// stands NOW -- the device drops the entries of points that went bad or whose row was given to another point while the MKF waited in the
// queue, which is the sweep of src/MapMaker.cc:407-418 -- instead of walking mmpMeasurements through GraphAddMeasurements.  The host's
// Measurement objects stay (the early-outs of ReFind read them); the host's sweep over them stays too, and must agree: it is checked here.
// Header delta, MultiKeyFrame: mcp_meas_parcel* mpMeasParcel (NULL until RecordMeasurements; destroyed with the MKF, before the table).
// Lane c is camera index c of the rig; a camera the MKF has no active keyframe of is withheld.
void GraphCommitTrackerParcel(Map& map, MultiKeyFrame& mkf, const std::vector<std::string>& vCamNames)
{
  if(!mkf.mpMeasParcel)
    return;
  static gvar3<int> gvnCrossCamera("CrossCamera", 1, HIDDEN|SILENT);
  const int nc = (int)vCamNames.size();
  std::vector<int> vLaneMKF(nc, -1), vLaneCam(nc), vAppended(nc, 0);
  int nHost = 0;
  for(int c = 0; c < nc; ++c)
  {
    vLaneCam[c] = c;
    KeyFramePtrMap::iterator kf_it = mkf.mmpKeyFrames.find(vCamNames[c]);
    if(kf_it == mkf.mmpKeyFrames.end() || !kf_it->second->mbActive)
      continue;
    vLaneMKF[c] = mkf.mnGraphSlot;
    nHost += (int)kf_it->second->mmpMeasurements.size();
  }
  mcp_parcel_commit_params params;
  params.cross_camera = *gvnCrossCamera;
  params.source = (int)Measurement::SRC_TRACKER;
  mcp_parcel_commit_result res;
  if(mcp_meas_parcel_commit(map.mpMapGraph, mkf.mpMeasParcel, nc, vLaneMKF.data(), vLaneCam.data(), &params, &res, vAppended.data()) != 0)
  {
    ROS_ERROR_STREAM("mcp_meas_parcel_commit: " << mcp_last_error());
    return;
  }
  if(res.n_appended != nHost)
    ROS_WARN_STREAM("GraphCommitTrackerParcel: the device appended " << res.n_appended << " measurements (" << res.n_stale << " stale, " << res.n_bad << " bad), the keyframes hold " << nHost);
  mcp_meas_parcel_destroy(mkf.mpMeasParcel);
  mkf.mpMeasParcel = NULL;
}

// The measurements of one ReFind batch (MapMakerServerBase::ReFindBatch, shim/MapMakerServerBase_gpu.cc): the FOUND pairs the call left in its
// pinned block go to the store through the map maker's own parcel, one lane per target keyframe.
void GraphCommitReFindParcel(Map& map, mcp_meas_parcel* pParcel, const std::vector<KeyFrame*>& vTargets, int nExpected)
{
  static gvar3<int> gvnCrossCamera("CrossCamera", 1, HIDDEN|SILENT);
  if(mcp_meas_parcel_from_refind(pParcel) < 0)
  {
    ROS_ERROR_STREAM("mcp_meas_parcel_from_refind: " << mcp_last_error());
    return;
  }
  const int n = (int)vTargets.size();
  std::vector<int> vLaneMKF(n), vLaneCam(n);
  for(int t = 0; t < n; ++t)
  {
    vLaneMKF[t] = vTargets[t]->mpParent->mnGraphSlot;      // (-1 while the MKF is not in the map: the lane is withheld)
    vLaneCam[t] = vTargets[t]->mnCamIndex;
  }
  mcp_parcel_commit_params params;
  params.cross_camera = *gvnCrossCamera;
  params.source = (int)Measurement::SRC_REFIND;
  mcp_parcel_commit_result res;
  if(mcp_meas_parcel_commit(map.mpMapGraph, pParcel, n, vLaneMKF.data(), vLaneCam.data(), &params, &res, NULL) != 0)
    ROS_ERROR_STREAM("mcp_meas_parcel_commit: " << mcp_last_error());
  else if(res.n_appended != nExpected)
    ROS_WARN_STREAM("GraphCommitReFindParcel: the device appended " << res.n_appended << " of " << nExpected << " measurements");
}

// KeyFrame::EraseMeasurementOfPoint (src/KeyFrame.cc:749 on) as AddMultiKeyFrameFromTopOfQueue uses it: one call for the whole list.
// (HandleOutliers, src/MapMakerServerBase.cc:1198-1238, no longer comes through here: mcp_map_cull_outliers erases on the device what it
// judges, shim/MapMakerServerBase_gpu.cc.)  mcp_map_graph_compact when the dead entries pass a share of the
// store (store indices change: nothing on this side keeps one across calls).
void GraphEraseMeasurements(Map& map, const std::vector<std::pair<KeyFrame*, MapPoint*> >& vPairs)
{
  const int n = (int)vPairs.size();
  std::vector<int> vMKF(n), vCam(n), vRow(n);
  for(int i = 0; i < n; ++i)
  {
    vMKF[i] = vPairs[i].first->mpParent->mnGraphSlot;
    vCam[i] = vPairs[i].first->mnCamIndex;
    vRow[i] = vPairs[i].second->mnTableRow;
  }
  if(mcp_map_graph_erase_meas(map.mpMapGraph, n, vMKF.data(), vCam.data(), vRow.data()) < 0)
    ROS_ERROR_STREAM("mcp_map_graph_erase_meas: " << mcp_last_error());
  int nLive = 0, nStored = 0;
  if(mcp_map_graph_num_meas(map.mpMapGraph, &nLive, &nStored) == 0 && nStored - nLive > nStored / 4)
    mcp_map_graph_compact(map.mpMapGraph);
}

// ---- the two entry points ------------------------------------------------------------------------------------------------------------------
int BundleAdjusterBase::BundleAdjustAll(std::vector<std::pair<KeyFrame*, MapPoint*> >& vOutliers)
{
  vOutliers.clear();
  mcp_bundle_select_result res;
  const int nStatus = RunSelect(mMap, MCP_BUNDLE_ALL, NULL, res);
  if(nStatus == 2)   // BundleAdjusterMulti.cc:66-70: too few points
    return 0;
  return BundleAdjustSelected(res, vOutliers, false);
}

int BundleAdjusterBase::BundleAdjustRecent(std::vector<std::pair<KeyFrame*, MapPoint*> >& vOutliers)
{
  vOutliers.clear();
  mcp_bundle_select_result res;
  const int nStatus = RunSelect(mMap, MCP_BUNDLE_RECENT, mMap.mlpMultiKeyFrames.back(), res);
  if(nStatus == 1)
  {
    ROS_INFO("BundleAdjusterBase: Map not big enough for local BA, returning");
    mbBundleConverged_Recent = true;
    return 0;
  }
  if(nStatus == 2)
    return 0;
  if(res.n_dropped_source > 0)
    ROS_WARN_STREAM("BundleAdjusterBase: " << res.n_dropped_source << " points left out, their source MKF is bad or gone");
  return BundleAdjustSelected(res, vOutliers, true);
}

// ---- the population of BundleAdjusterMulti::BundleAdjust (src/BundleAdjusterMulti.cc:81-200) from the views ----------------------------------
// mvMKFBundleID / mvCamBundleID / mvPointBundleID (bundle index -> ChainBundle id) replace mmBase_BundleID, mmCamName_BundleID and
// mmPoint_BundleID; the inverse maps the outlier decoding needs (:246-258) are mvpSlotMKF[mkfs[i].slot] and mvpRowPoint[points[i].row].
int BundleAdjusterMulti::BundleAdjustSelected(const mcp_bundle_select_result& res, std::vector<std::pair<KeyFrame*, MapPoint*> >& vOutliers, bool bRecent)
{
  int nMKFs = 0, nPoints = 0, nMeas = 0;
  const mcp_bundle_mkf* pMKFs = mcp_map_bundle_mkfs_view(mMap.mpMapGraph, &nMKFs);
  const mcp_bundle_point* pPoints = mcp_map_bundle_points_view(mMap.mpMapGraph, &nPoints);
  const mcp_bundle_meas* pMeas = mcp_map_bundle_meas_view(mMap.mpMapGraph, &nMeas);

  ChainBundle multiBundle(mmCameraModels, mbUseRobust, mbUseTukey, mbVerbose);
  mbBundleRunning = true;
  mbBundleRunningIsRecent = bRecent;

  // poses: the MKFs (adjust set, then fixed set), one fixed pose per camera of the rig, the world pose when a fixed point needs it
  mvMKFBundleID.resize(nMKFs);
  for(int i = 0; i < nMKFs; ++i)
    mvMKFBundleID[i] = multiBundle.AddPose(mvpSlotMKF[pMKFs[i].slot]->mse3BaseFromWorld, pMKFs[i].fixed != 0);
  mvCamBundleID.resize(mvCamNames.size());
  for(unsigned c = 0; c < mvCamNames.size(); ++c)
    mvCamBundleID[c] = multiBundle.AddPose(mvpSlotMKF[pMKFs[0].slot]->mmpKeyFrames[mvCamNames[c]]->mse3CamFromBase, true);
  const int nWorldID = res.has_fixed_points ? multiBundle.AddPose(TooN::SE3<>(), true) : -1;

  // points: mcp_ba_add_points over the view (x is CamFromWorld_src * mv3WorldPos already, from the rows the last write-back left)
  std::vector<double> vX(3 * nPoints);
  std::vector<int> vChains(2 * nPoints), vChainLen(nPoints);
  std::vector<unsigned char> vFixed(nPoints);
  for(int i = 0; i < nPoints; ++i)
  {
    for(int k = 0; k < 3; ++k)
      vX[3 * i + k] = pPoints[i].x[k];
    vFixed[i] = pPoints[i].fixed != 0;
    if(pPoints[i].fixed)
    {
      vChains[2 * i] = nWorldID; vChains[2 * i + 1] = 0; vChainLen[i] = 1;
    }
    else
    {
      vChains[2 * i] = mvMKFBundleID[pPoints[i].src_mkf]; vChains[2 * i + 1] = mvCamBundleID[pPoints[i].src_cam]; vChainLen[i] = 2;
    }
  }
  mvPointBundleID.resize(nPoints);
  multiBundle.AddPoints(nPoints, vX.data(), vChains.data(), 2, vChainLen.data(), vFixed.data(), mvPointBundleID.data());

  // measurements: mcp_ba_add_measurements over the view
  std::vector<int> vMeasChains(2 * nMeas), vMeasLen(nMeas, 2), vMeasPoint(nMeas), vMeasCam(nMeas);
  std::vector<double> vUV(2 * nMeas), vSigmaSq(nMeas);
  for(int j = 0; j < nMeas; ++j)
  {
    vMeasChains[2 * j] = mvMKFBundleID[pMeas[j].mkf]; vMeasChains[2 * j + 1] = mvCamBundleID[pMeas[j].cam];
    vMeasPoint[j] = mvPointBundleID[pMeas[j].point];
    vUV[2 * j] = pMeas[j].uv[0]; vUV[2 * j + 1] = pMeas[j].uv[1];
    vSigmaSq[j] = LevelScale(pMeas[j].level) * LevelScale(pMeas[j].level);
    vMeasCam[j] = pMeas[j].cam;
  }
  multiBundle.AddMeasurements(nMeas, vMeasChains.data(), 2, vMeasLen.data(), vMeasPoint.data(), vUV.data(), vSigmaSq.data(), vMeasCam.data());

  // what mcp_graph_write_back takes comes from the same views: point_ids = mvPointBundleID, rows = points[i].row, slots = mkfs[i].slot with
  // mvMKFBundleID[i] as their pose ids and mvCamBundleID as the rig's.  No list is built here: the keyframes' lists come from the graph's store.
  mvWriteBackRows.resize(nPoints);
  for(int i = 0; i < nPoints; ++i)
    mvWriteBackRows[i] = pPoints[i].row;
  mvWriteBackSlots.resize(nMKFs);
  for(int i = 0; i < nMKFs; ++i)
    mvWriteBackSlots[i] = pMKFs[i].slot;

  // from here on src/BundleAdjusterMulti.cc:205-264 as it stands, with the vectors above in place of the maps
  return SolveAndDecode(multiBundle, pMKFs, nMKFs, pPoints, nPoints, vOutliers);
}

// ---- AdjustAndUpdate (src/BundleAdjusterMulti.cc:286-334) in one call ------------------------------------------------------------------------
// The reference refreshes every keyframe's pose, every point's position and pixel vectors, and the scene depth of every keyframe of the bundle's
// MKFs.  mcp_graph_write_back does the three on the device: the points from the solver's state, the MKF poses copied into the graph, the
// keyframes' lists built from the graph's store (alive, active keyframe, row not bad; weights from the table's count column), the scene depth on
// them and the new depth means stored in the graph.  The walk over mmpMeasurements that built seg_start / seg_rows / seg_weights is gone, and so is
// GraphUploadMKFs after an adjustment.  What comes back is what the host objects mirror: poses and depth statistics.
void BundleAdjusterMulti::AdjustAndUpdate(ChainBundle& multiBundle)
{
  const int nMKFs = (int)mvWriteBackSlots.size(), nc = (int)mvCamNames.size(), nPoints = (int)mvWriteBackRows.size();
  std::vector<double> vWorld(3 * nPoints), vRight(3 * nPoints), vDown(3 * nPoints), vCamFromWorld(12 * nMKFs * nc), vBaseFromWorld(12 * nMKFs);
  std::vector<mcp_scene_depth> vDepth(nMKFs * nc);
  if(mcp_graph_write_back(multiBundle.Handle(), mMap.mpMapGraph, nPoints, mvPointBundleID.data(), mvWriteBackRows.data(), NULL, 2, NULL, vWorld.data(),
                          vRight.data(), vDown.data(), nMKFs, mvWriteBackSlots.data(), mvMKFBundleID.data(), mvCamBundleID.data(), vCamFromWorld.data(),
                          vDepth.data(), vBaseFromWorld.data()) != 0)
  {
    ROS_ERROR_STREAM("mcp_graph_write_back: " << mcp_last_error());
    return;
  }
  for(int i = 0; i < nMKFs; ++i)
  {
    MultiKeyFrame& mkf = *mvpSlotMKF[mvWriteBackSlots[i]];
    mkf.mse3BaseFromWorld = SE3From12(&vBaseFromWorld[12 * i]);
    for(int c = 0; c < nc; ++c)
    {
      KeyFramePtrMap::iterator kf_it = mkf.mmpKeyFrames.find(mvCamNames[c]);
      if(kf_it == mkf.mmpKeyFrames.end())
        continue;
      KeyFrame& kf = *kf_it->second;
      kf.mse3CamFromWorld = SE3From12(&vCamFromWorld[12 * (i * nc + c)]);
      const mcp_scene_depth& d = vDepth[i * nc + c];
      if(d.refreshed == 1)   // 0: three points or fewer, the keyframe is left alone (KeyFrame.cc:587-591)
      {
        kf.mdSceneDepthMean = d.mean;
        kf.mdSceneDepthSigma = d.sigma;
      }
      else if(d.refreshed == -1)
        ROS_BREAK();         // KeyFrame.cc:635-644
    }
  }
  for(int i = 0; i < nPoints; ++i)
  {
    MapPoint& point = *mvpRowPoint[mvWriteBackRows[i]];
    point.mv3WorldPos = TooN::makeVector(vWorld[3 * i], vWorld[3 * i + 1], vWorld[3 * i + 2]);
    point.mv3PixelRight_W = TooN::makeVector(vRight[3 * i], vRight[3 * i + 1], vRight[3 * i + 2]);
    point.mv3PixelDown_W = TooN::makeVector(vDown[3 * i], vDown[3 * i + 1], vDown[3 * i + 2]);
    point.mbOptimized = true;
  }
}

// MultiKeyFrame enters the map (src/MapMakerServerBase.cc:219, 392): MultiKeyFrame::RefreshSceneDepthRobust at its own pose, after GraphUploadMKFs
// and GraphCommitTrackerParcel (GraphAddMeasurements for an initialiser's) have put it and its measurements into the graph.  One mcp_graph_refresh_depth; the graph keeps the new means.
void GraphRefreshSceneDepth(Map& map, MultiKeyFrame& mkf, const std::vector<std::string>& vCamNames)
{
  const int nc = (int)vCamNames.size();
  std::vector<mcp_scene_depth> vDepth(nc);
  if(mcp_graph_refresh_depth(map.mpMapGraph, 1, &mkf.mnGraphSlot, vDepth.data()) != 0)
  {
    ROS_ERROR_STREAM("mcp_graph_refresh_depth: " << mcp_last_error());
    return;
  }
  for(int c = 0; c < nc; ++c)
  {
    KeyFramePtrMap::iterator kf_it = mkf.mmpKeyFrames.find(vCamNames[c]);
    if(kf_it == mkf.mmpKeyFrames.end() || vDepth[c].refreshed != 1)
      continue;
    kf_it->second->mdSceneDepthMean = vDepth[c].mean;
    kf_it->second->mdSceneDepthSigma = vDepth[c].sigma;
  }
}
