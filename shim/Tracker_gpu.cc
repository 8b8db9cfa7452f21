// Tracker_gpu.cc -- MI355X bodies of Tracker::FindPVS, Tracker::SearchForPoints and Tracker::CalcPoseUpdate, and the optional one-call
// forms of a TrackMap stage (TrackStageOnDevice) and of the whole TrackMap from the map table (TrackMapOnDevice).
//
// Replace /root/reference/src/Tracker.cc:662-723 (FindPVS), :1297-1377 (SearchForPoints) and :1379-1512 (CalcPoseUpdate): delete those
// member functions there (or fence them with #ifndef MCPTAM_HIP) and add this file to the library's sources.  The tracker keeps all of its
// control flow -- the level buckets, the 1000-patch budget, the shuffles, the coarse / fine stages, the motion model -- and
// calls these two members exactly where it did (src/Tracker.cc:841-906, 1027-1075).  The per-point inner loops (TrackerData::Project /
// CalcJacobian, PatchFinder::MakeTemplateCoarseCont / FindPatchCoarse / IterateSubPixToConvergence, the WLS accumulation) run as one
// batched device call each.  Needs KeyFrame::mpDev (shim/KeyFrame_gpu.cc) and shim/CameraExport.h.
#include <mcptam/Tracker.h>
#include <mcptam/TrackerData.h>
#include <mcptam/MapPoint.h>
#include <mcptam/KeyFrame.h>
#include <mcptam/LevelHelpers.h>
#include <mcp_img.h>
#include "CameraExport.h"
#include <TooN/SVD.h>
#include <ros/ros.h>

using namespace TooN;


namespace
{
void ToArray12(const SE3<>& se3, double a[12])
{
  const Matrix<3>& m3 = se3.get_rotation().get_matrix();
  for(int i = 0; i < 3; ++i)
  {
    for(int j = 0; j < 3; ++j)
      a[3*i + j] = m3(i, j);
    a[9 + i] = se3.get_translation()[i];
  }
}
}  // namespace

// Find points in the image: one device call for the whole vector (include/mcp_img.h, mcp_patch_sequences in MCP_PF_TRACK mode).
// PatchFinder's members that live from frame to frame -- the template cache of MakeTemplateCoarseCont (src/PatchFinder.cc:144-181)
// and the sub-pixel state -- move from TrackerData::mFinder into an mcp_pf_state per TrackerData: add
//     mcp_pf_state mFinderState;      // zero-initialised in the constructor (a PatchFinder that has seen nothing)
// to class TrackerData (include/mcptam/TrackerData.h:75, next to mFinder, which keeps CalcSearchLevelAndWarpMatrix for FindPVS).
// One sequence of one item per tracked point; the map point's address is its key, as the reference compares &point.
int Tracker::SearchForPoints(TrackerDataPtrVector& vTD, std::string cameraName, int nRange, int nSubPixIts, bool bExhaustive)
{
  if(vTD.empty())
    return 0;

  KeyFrame& kf = *mpCurrentMKF->mmpKeyFrames[cameraName];
  ROS_ASSERT(kf.mpDev);

  std::vector<mcp_pf_item> vIn(vTD.size());
  std::vector<mcp_td_out> vOut(vTD.size());
  std::vector<mcp_pf_state> vState(vTD.size());
  std::vector<int> vSeqStart(vTD.size() + 1);
  for(unsigned i = 0; i < vTD.size(); ++i)
  {
    MapPoint& point = vTD[i]->mPoint;
    vSeqStart[i] = (int)i;
    vState[i] = vTD[i]->mFinderState;
    vIn[i].point_key = (int)(reinterpret_cast<uintptr_t>(&point) >> 4);   // identity of the MapPoint object (the finder of a TrackerData only ever sees this one)
    vIn[i].target = 0;
    vIn[i].start_pos[0] = vIn[i].start_pos[1] = 0.0;
    mcp_td_in& in = vIn[i].point;
    for(int k = 0; k < 3; ++k)
    {
      in.world_pos[k] = point.mv3WorldPos[k];
      in.pixel_right_w[k] = point.mv3PixelRight_W[k];
      in.pixel_down_w[k] = point.mv3PixelDown_W[k];
    }
    ROS_ASSERT(point.mpPatchSourceKF && point.mpPatchSourceKF->mpDev);   // source pyramids stay resident on the device
    in.source_kf = point.mpPatchSourceKF->mpDev;
    in.source_level = point.mnSourceLevel;
    in.center_x = point.mirCenter.x;
    in.center_y = point.mirCenter.y;
    in.fixed = point.mbFixed ? 1 : 0;
  }

  vSeqStart[vTD.size()] = (int)vTD.size();
  mcp_camera cam = mcptam_hip::CameraExport::Make(mmCameraModels[cameraName]);
  mcp_pf_target target;
  target.kf = kf.mpDev;
  target.cam = &cam;
  ToArray12(mpCurrentMKF->mse3BaseFromWorld, target.base_from_world);
  ToArray12(kf.mse3CamFromBase, target.cam_from_base);

  if(mcp_patch_sequences(MCP_PF_TRACK, 1, &target, (int)vTD.size(), &vSeqStart[0], &vIn[0], &vState[0], nRange, nSubPixIts, bExhaustive ? 1 : 0, &vOut[0]) != 0)
  {
    ROS_FATAL_STREAM("Tracker::SearchForPoints: "<<mcp_last_error());
    ros::shutdown();
    return 0;
  }

  int nFound = 0;
  for(unsigned i = 0; i < vTD.size(); ++i)
  {
    TrackerData& td = *vTD[i];
    const mcp_td_out& out = vOut[i];
    td.mFinderState = vState[i];      // the finder's members after this frame

    // the device re-derives the projection it searches around: identical to what FindPVS left in the TrackerData
    td.mv2Image = makeVector(out.image[0], out.image[1]);
    td.mm2CamDerivs(0, 0) = out.cam_derivs[0]; td.mm2CamDerivs(0, 1) = out.cam_derivs[1];
    td.mm2CamDerivs(1, 0) = out.cam_derivs[2]; td.mm2CamDerivs(1, 1) = out.cam_derivs[3];
    for(int r = 0; r < 2; ++r)
      for(int c = 0; c < 6; ++c)
        td.mm26Jacobian(r, c) = out.jacobian[6*r + c];
    td.mnSearchLevel = out.search_level;

    if(out.template_bad)   // PatchFinder::TemplateBad(): warp rejected or source footprint outside the source level
    {
      td.mbInImage = td.mbFound = false;
      continue;
    }
    mmMeasAttemptedLevels[cameraName][out.search_level]++;

    td.mbSearched = out.searched != 0;
    td.mbFound = out.found != 0;
    td.mbDidSubPix = out.did_subpix != 0;
    if(!td.mbFound)
      continue;     // not found in the coarse stage, or the sub-pixel iterations did not converge (counters as the reference nets them)

    td.mdSqrtInvNoise = out.sqrt_inv_noise;   // 1 / LevelScale(search level)
    td.mv2Found = makeVector(out.found_pos[0], out.found_pos[1]);
    nFound++;
    mmMeasFoundLevels[cameraName][out.search_level]++;
  }
  return nFound;
}

// Pose update from the found measurements: M-estimator weights + WLS<6> with prior 100 on the device (mcp_track_pose_update_m),
// with the estimator Tracker::sMEstimatorName selects (src/Tracker.cc:1388-1401): Tukey, Cauchy or Huber.
Vector<6> Tracker::CalcPoseUpdate(std::vector<TrackerDataPtrVector>& vIterationSets, double dOverrideSigma, bool bMarkOutliers)
{
  int nEstimator = MCP_MEST_TUKEY;
  if(Tracker::sMEstimatorName == "Tukey")
    nEstimator = MCP_MEST_TUKEY;
  else if(Tracker::sMEstimatorName == "Cauchy")
    nEstimator = MCP_MEST_CAUCHY;
  else if(Tracker::sMEstimatorName == "Huber")
    nEstimator = MCP_MEST_HUBER;
  else
  {
    ROS_FATAL_STREAM("Tracker: Invalid Tracker MEstimator selected: "<<Tracker::sMEstimatorName<<", choices are [Tukey, Cauchy, Huber]");
    ros::shutdown();
    return makeVector(0, 0, 0, 0, 0, 0);
  }

  std::vector<TrackerData*> vpTD;
  for(unsigned i = 0; i < mvCurrCamNames.size(); ++i)
    for(unsigned j = 0; j < vIterationSets[i].size(); ++j)
      vpTD.push_back(vIterationSets[i][j].get());

  const int n = (int)vpTD.size();
  std::vector<uint8_t> vFound(n > 0 ? n : 1);
  std::vector<double> vFoundPos(2*n + 2), vImagePos(2*n + 2), vSqrtInvNoise(n + 1), vJac(12*n + 12), vWeights(n + 1);
  int nUsed = 0;
  for(int i = 0; i < n; ++i)
  {
    TrackerData& td = *vpTD[i];
    vFound[i] = td.mbFound ? 1 : 0;
    if(!td.mbFound)
      continue;
    ++nUsed;
    td.mv2Error_CovScaled = td.mdSqrtInvNoise * (td.mv2Found - td.mv2Image);
    vFoundPos[2*i] = td.mv2Found[0]; vFoundPos[2*i + 1] = td.mv2Found[1];
    vImagePos[2*i] = td.mv2Image[0]; vImagePos[2*i + 1] = td.mv2Image[1];
    vSqrtInvNoise[i] = td.mdSqrtInvNoise;
    for(int r = 0; r < 2; ++r)
      for(int c = 0; c < 6; ++c)
        vJac[12*i + 6*r + c] = td.mm26Jacobian(r, c);
  }
  if(nUsed == 0)
    return makeVector(0, 0, 0, 0, 0, 0);

  double adMu[6], dSigmaSquared = 0;
  if(mcp_track_pose_update_m(n, &vFound[0], &vFoundPos[0], &vImagePos[0], &vSqrtInvNoise[0], &vJac[0], dOverrideSigma, adMu, &vWeights[0], &dSigmaSquared, nEstimator) != 0)
  {
    ROS_FATAL_STREAM("Tracker::CalcPoseUpdate: "<<mcp_last_error());
    ros::shutdown();
    return makeVector(0, 0, 0, 0, 0, 0);
  }

  // inlier / outlier bookkeeping of the marking iteration (src/Tracker.cc:1448-1487) and the covariance (:1500-1502)
  mnNumInliers = 0;
  Matrix<6> m6CInv = 100.0 * Identity;      // wls.add_prior(100)
  for(int i = 0; i < n; ++i)
  {
    TrackerData& td = *vpTD[i];
    if(!td.mbFound)
    {
      if(td.mbSearched && bMarkOutliers && !IsLost())
        td.mPoint.mnMEstimatorOutlierCount++;
      continue;
    }
    const double dWeight = vWeights[i];
    if(dWeight == 0.0)
    {
      if(bMarkOutliers)
        td.mPoint.mnMEstimatorOutlierCount++;
      continue;
    }
    if(bMarkOutliers)
    {
      td.mPoint.mnMEstimatorInlierCount++;
      mnNumInliers++;
      // C^-1 += w J^T J with J = sqrt_inv_noise * Jacobian row (WLS::add_mJ twice)
      for(int r = 0; r < 2; ++r)
      {
        const Vector<6> v6 = td.mdSqrtInvNoise * td.mm26Jacobian[r];
        m6CInv += dWeight * v6.as_col() * v6.as_row();
      }
    }
  }
  if(bMarkOutliers)
    mm6PoseCovariance = TooN::SVD<6>(m6CInv).get_pinv();

  return makeVector(adMu[0], adMu[1], adMu[2], adMu[3], adMu[4], adMu[5]);
}


// ---- one TrackMap stage in one submission (optional) -----------------------------------------------------------------------------
// Tracker::TrackMap spends a stage as: SearchForPoints per camera, then ten PoseUpdateStep / PoseUpdateStepLinear iterations over all
// cameras (src/Tracker.cc:1013-1035 coarse, 1043-1075 fine).  mcp_track_frame runs that whole stage -- and, when the frame has just
// arrived, the MakeKeyFrame_Lite of every camera before it (src/Tracker.cc:303-318) -- as one device submission with one wait: the
// searches of all cameras in one launch with the persistent finders, the pose-iteration records built on the device, the ten iterations
// in one kernel.  A maintainer who wants it declares
//     Vector<6> TrackStageOnDevice(std::vector<TrackerDataPtrVector>& vIterationSets, int nRange, int nSubPixIts, bool bFineStage, bool bMakeLite);
// in Tracker.h and calls it where the stage's SearchForPoints loop + iteration loop stood, after having collected every camera's
// points to search into vIterationSets[i] (TestForCoarse / SetupFineTracking minus their SearchForPoints calls).  Results are those
// of the per-camera calls above followed by mcp_track_pose_refine_m (tests/test_img_gpu.py::
// test_track_frame_in_one_submission_equals_the_three_calls).  The outlier marking of the last fine iteration stays on the host:
// weights_last is what CalcPoseUpdate's marking branch reads.
Vector<6> Tracker::TrackStageOnDevice(std::vector<TrackerDataPtrVector>& vIterationSets, int nRange, int nSubPixIts, bool bFineStage, bool bMakeLite)
{
  const int nCams = (int)mvCurrCamNames.size();
  std::vector<mcp_kf*> vKF(nCams);
  std::vector<mcp_camera> vCams(nCams);
  std::vector<double> vCfB(12 * nCams);
  std::vector<int> vN(nCams);
  std::vector<std::vector<mcp_td_in> > vvIn(nCams);
  std::vector<std::vector<int> > vvKey(nCams);
  std::vector<std::vector<mcp_pf_state> > vvState(nCams);
  std::vector<std::vector<mcp_td_out> > vvOut(nCams);
  std::vector<const mcp_td_in*> vpIn(nCams);
  std::vector<const int*> vpKey(nCams);
  std::vector<mcp_pf_state*> vpState(nCams);
  std::vector<mcp_td_out*> vpOut(nCams);
  std::vector<const uint8_t*> vpImg(nCams);
  std::vector<int> vStride(nCams);
  int nTotal = 0;
  for(int c = 0; c < nCams; ++c)
  {
    KeyFrame& kf = *mpCurrentMKF->mmpKeyFrames[mvCurrCamNames[c]];
    ROS_ASSERT(kf.mpDev);
    vKF[c] = kf.mpDev;
    vCams[c] = mcptam_hip::CameraExport::Make(mmCameraModels[mvCurrCamNames[c]]);
    ToArray12(kf.mse3CamFromBase, &vCfB[12*c]);
    TrackerDataPtrVector& vTD = vIterationSets[c];
    vN[c] = (int)vTD.size();
    vvIn[c].resize(vTD.size()); vvKey[c].resize(vTD.size()); vvState[c].resize(vTD.size()); vvOut[c].resize(vTD.size());
    for(unsigned i = 0; i < vTD.size(); ++i)
    {
      MapPoint& point = vTD[i]->mPoint;
      mcp_td_in& in = vvIn[c][i];
      for(int k = 0; k < 3; ++k)
      {
        in.world_pos[k] = point.mv3WorldPos[k];
        in.pixel_right_w[k] = point.mv3PixelRight_W[k];
        in.pixel_down_w[k] = point.mv3PixelDown_W[k];
      }
      in.source_kf = point.mpPatchSourceKF->mpDev;
      in.source_level = point.mnSourceLevel;
      in.center_x = point.mirCenter.x;
      in.center_y = point.mirCenter.y;
      in.fixed = point.mbFixed ? 1 : 0;
      vvKey[c][i] = (int)(reinterpret_cast<uintptr_t>(&point) >> 4);
      vvState[c][i] = vTD[i]->mFinderState;
    }
    vpIn[c] = vvIn[c].empty() ? NULL : &vvIn[c][0];
    vpKey[c] = vvKey[c].empty() ? NULL : &vvKey[c][0];
    vpState[c] = vvState[c].empty() ? NULL : &vvState[c][0];
    vpOut[c] = vvOut[c].empty() ? NULL : &vvOut[c][0];
    vpImg[c] = kf.maLevels[0].image.data();                 // only read when bMakeLite (the frame the tracker was handed)
    vStride[c] = kf.maLevels[0].image.row_stride();
    nTotal += vN[c];
  }

  // coarse stage: ten full re-projections, sigma override 1.0; fine stage: re-projection at 0, 4, 9, override 16.0 (src/Tracker.cc:1027-1030,
  // 1063-1072); PoseUpdateStep / PoseUpdateStepLinear drop the override up to the fifth iteration (:800-802)
  uint8_t abNonlinear[10];
  double adOverride[10];
  for(int it = 0; it < 10; ++it)
  {
    abNonlinear[it] = (!bFineStage || it == 0 || it == 4 || it == 9) ? 1 : 0;
    adOverride[it] = it <= 5 ? 0.0 : (bFineStage ? 16.0 : 1.0);
  }
  int nEstimator = MCP_MEST_TUKEY;
  if(Tracker::sMEstimatorName == "Cauchy") nEstimator = MCP_MEST_CAUCHY;
  else if(Tracker::sMEstimatorName == "Huber") nEstimator = MCP_MEST_HUBER;

  double adBfW[12], adMu[6];
  ToArray12(mpCurrentMKF->mse3BaseFromWorld, adBfW);
  std::vector<double> vWeights(std::max(nTotal, 1));
  if(mcp_track_frame(nCams, &vKF[0], bMakeLite ? &vpImg[0] : NULL, &vStride[0], 0, NULL, &vCams[0], adBfW, &vCfB[0], &vN[0], &vpIn[0], &vpKey[0], &vpState[0],
                     nRange, nSubPixIts, 0, 10, abNonlinear, adOverride, nEstimator, &vpOut[0], NULL, adMu, &vWeights[0]) != 0)
  {
    ROS_FATAL_STREAM("Tracker::TrackStageOnDevice: "<<mcp_last_error());
    ros::shutdown();
    return Zeros;
  }

  // BaseFromWorld as the ten iterations left it, TrackerData as SearchForPoints leaves it
  Matrix<3> m3R;
  for(int i = 0; i < 3; ++i)
    for(int j = 0; j < 3; ++j)
      m3R(i, j) = adBfW[3*i + j];
  mpCurrentMKF->mse3BaseFromWorld = SE3<>(SO3<>(m3R), makeVector(adBfW[9], adBfW[10], adBfW[11]));
  int w = 0;
  for(int c = 0; c < nCams; ++c)
  {
    TrackerDataPtrVector& vTD = vIterationSets[c];
    for(unsigned i = 0; i < vTD.size(); ++i, ++w)
    {
      TrackerData& td = *vTD[i];
      const mcp_td_out& out = vvOut[c][i];
      td.mFinderState = vvState[c][i];
      td.mnSearchLevel = out.search_level;
      td.mbSearched = out.searched != 0;
      td.mbFound = out.found != 0 && !out.template_bad;
      td.mbDidSubPix = out.did_subpix != 0;
      if(out.template_bad) { td.mbInImage = false; continue; }
      if(!td.mbFound) continue;
      td.mdSqrtInvNoise = out.sqrt_inv_noise;
      td.mv2Found = makeVector(out.found_pos[0], out.found_pos[1]);
      if(bFineStage && !IsLost())        // the marking iteration's bookkeeping (src/Tracker.cc:1448-1487)
      {
        if(vWeights[w] == 0.0) td.mPoint.mnMEstimatorOutlierCount++;
        else td.mPoint.mnMEstimatorInlierCount++;
      }
    }
  }
  return makeVector(adMu[0], adMu[1], adMu[2], adMu[3], adMu[4], adMu[5]);
}

// ---- FindPVS over a device-resident map-point table (include/mcp_img.h, mcp_track_find_pvs) ------------------------------------------
// Members this needs in class Tracker (include/mcptam/Tracker.h):
//     mcp_map_points* mpMapTable;              // mcp_map_points_create(-1) in the constructor (the keyframes' device), destroyed in ~Tracker
//     std::vector<MapPoint*> mvMapTableRows;   // table row -> MapPoint
//     std::vector<mcp_pvs_entry> mvPvsOut;     // scratch of the call
//     void UploadMapTable();                   // option (a) below
//     std::vector<uint8_t> mvNearRows;         // !sbCollectAllPoints: the collected set of this frame, one byte per table row (bit c: camera c)
//     mcp_collect_params CollectParams();      // the current keyframes' depth means for the collection
// and in class PatchFinder (include/mcptam/PatchFinder.h) a setter for the two members CalcSearchLevelAndWarpMatrix leaves behind:
//     void SetSearchLevelAndWarp(int nLevel, const TooN::Matrix<2>& m2WarpInverse) { mnSearchLevel = nLevel; mm2WarpInverse = m2WarpInverse; }
//
// Keeping the table current.  Two ways, both under mMap.mMutex (the lock FindPVS already takes, src/Tracker.cc:668):
//  (a) UploadMapTable() below: every frame, before the first FindPVS, the table is cut to the map's current size (mcp_map_points_resize:
//      the map shrinks whenever Map::MoveBadPointsToTrash erases points from mlpPoints, src/Map.cc:106-107, 158-159, and rows past the
//      new size must not reach the PVS) and all points of the map go up again (mcp_map_points_set of one range, usable = !mbBad &&
//      mbOptimized); mvMapTableRows is rebuilt.  Nothing else in the system changes; the cost is one pass over the map on the host plus
//      80 B per point over PCIe (scripts/bench_pvs.py: table_full_upload_ms).
//  (b) A slot per MapPoint (an int mnTableRow in class MapPoint, assigned when the point enters the map, never reused while it lives):
//      BundleAdjusterMulti writes the new positions back (src/BundleAdjusterMulti.cc, where it copies the adjusted points into the map)
//      -> mcp_map_points_update of those rows; MapMakerBase adds a point / refreshes its pixel vectors -> update of that row; a point
//      marked mbBad or moved to the trash -> update with usable = 0 (its slot is recycled only after the trash is emptied).  Per frame
//      nothing goes up that did not change (table_update_5pct_ms).  The updates are enqueued on the table's stream, so the FindPVS that
//      follows sees them whole, whichever thread made them.
// (a) is what is written out here; (b) replaces UploadMapTable() by those calls.
void Tracker::UploadMapTable()
{
  // caller holds mMap.mMutex
  mvMapTableRows.clear();
  std::vector<double> vPos, vRight, vDown;
  std::vector<uint8_t> vUsable;
  std::vector<int> vInlier, vOutlier;
  for(MapPointPtrList::iterator point_it = mMap.mlpPoints.begin(); point_it != mMap.mlpPoints.end(); ++point_it)
  {
    MapPoint& point = *(*point_it);
    mvMapTableRows.push_back(&point);
    for(int k = 0; k < 3; ++k)
    {
      vPos.push_back(point.mv3WorldPos[k]);
      vRight.push_back(point.mv3PixelRight_W[k]);
      vDown.push_back(point.mv3PixelDown_W[k]);
    }
    vUsable.push_back((point.mbBad || !point.mbOptimized) ? 0 : 1);      // src/Tracker.cc:680
    vInlier.push_back(point.mnMEstimatorInlierCount);                    // the count column mcp_track_map_record marks and weighs with
    vOutlier.push_back(point.mnMEstimatorOutlierCount);
  }
  // rows = the map's size, also when the map has shrunk or is empty: every row of the table is then a row of mvMapTableRows
  if(mcp_map_points_resize(mpMapTable, (int)vUsable.size()) != 0 ||
     (!vUsable.empty() && (mcp_map_points_set(mpMapTable, 0, (int)vUsable.size(), &vPos[0], &vRight[0], &vDown[0], &vUsable[0]) != 0 ||
                           mcp_map_points_set_counts(mpMapTable, 0, (int)vUsable.size(), &vInlier[0], &vOutlier[0]) != 0)))
  {
    ROS_FATAL_STREAM("Tracker::UploadMapTable: "<<mcp_last_error());
    ros::shutdown();
  }
}

// tracker_collect_all_points = false (Tracker::sbCollectAllPoints, CollectNearestPoints :1797-1854): the co-visible points of the map keyframe
// nearest to each current keyframe, collected on the device from the map graph's store (include/mcp_img.h, mcp_map_collect_nearest /
// mcp_track_collect_nearest).  The depth means are the current keyframes' mdSceneDepthMean: CopySceneDepths gave them to a fresh MKF, and the
// previous frame's record refreshed them (TrackMapOnDevice, below).  The camera order is mvCurrCamNames', which is the graph's rig order.
mcp_collect_params Tracker::CollectParams()
{
  mcp_collect_params params;
  memset(&params, 0, sizeof params);
  params.mean_diff_fraction = KeyFrame::sdDistanceMeanDiffFraction;
  for(unsigned c = 0; c < mvCurrCamNames.size(); ++c)
  {
    params.depth_mean[c] = mpCurrentMKF->mmpKeyFrames[mvCurrCamNames[c]]->mdSceneDepthMean;
    params.active[c] = 1;
  }
  return params;
}

// The reference body collects the nearest points (sbCollectAllPoints: all of them, :1785-1795, or the walk above), projects each, tests the mask,
// takes the derivatives and asks the PatchFinder for the search level.  Here one device call does that for every row of the table; the
// host only walks the PVS.  A TrackerData is created for PVS points only: one the reference would create for a point outside the PVS holds
// a PatchFinder that has seen nothing and is only ever touched again by the next FindPVS, so creating it then changes nothing.
// Drop-in: one camera per call, as TrackMap calls it (:950-961); INTEGRATION.md shows the one-call form for all cameras of the frame.
void Tracker::FindPVS(std::string cameraName, TDVLevels& vPVSLevels)
{
  TaylorCamera& camera = mmCameraModels[cameraName];
  KeyFrame& kf = *(mpCurrentMKF->mmpKeyFrames[cameraName]);
  ROS_ASSERT(kf.mpDev);

  boost::mutex::scoped_lock lock(mMap.mMutex);
  if(cameraName == mvCurrCamNames[0])
  {
    UploadMapTable();                 // option (a): once per frame, before the first camera
    // This drop-in asks for one camera per call, so it cannot use the frame mode (whose frames have the rig's cameras): the set of every
    // camera is collected once per frame by the stand-alone call, and the walk over the PVS below skips the rows outside it
    // (std::vector<uint8_t> mvNearRows in class Tracker).
    mvNearRows.clear();
    if(!Tracker::sbCollectAllPoints)
    {
      double adPose[12];
      ToArray12(mpCurrentMKF->mse3BaseFromWorld, adPose);
      mcp_collect_params params = CollectParams();
      mcp_collect_report report;
      mvNearRows.resize(std::max<size_t>(mvMapTableRows.size(), 1));
      if(mcp_map_collect_nearest(mMap.mpMapGraph, adPose, NULL, &params, &report, &mvNearRows[0]) != 0)
      {
        ROS_FATAL_STREAM("Tracker::FindPVS: "<<mcp_last_error());
        ros::shutdown();
        return;
      }
    }
  }
  const int nCamIndex = (int)(std::find(mvCurrCamNames.begin(), mvCurrCamNames.end(), cameraName) - mvCurrCamNames.begin());

  mcp_camera cam = mcptam_hip::CameraExport::Make(camera);
  double adBaseFromWorld[12], adCamFromBase[12];
  ToArray12(mpCurrentMKF->mse3BaseFromWorld, adBaseFromWorld);
  ToArray12(kf.mse3CamFromBase, adCamFromBase);
  int nCap = (int)mvMapTableRows.size();
  mvPvsOut.resize(std::max(nCap, 1));
  mcp_pvs_entry* pOut = &mvPvsOut[0];
  int anCounts[MCP_LEVELS];
  mcp_kf* pTarget = kf.mpDev;
  if(mcp_track_find_pvs(mpMapTable, 1, &pTarget, &cam, adBaseFromWorld, adCamFromBase, &nCap, &pOut, anCounts) != 0)
  {
    ROS_FATAL_STREAM("Tracker::FindPVS: "<<mcp_last_error());
    ros::shutdown();
    return;
  }

  const SE3<>& se3CamFromWorld = kf.mse3CamFromWorld;      // = CamFromBase * BaseFromWorld (UpdateCamsFromWorld, :654-659)
  int k = 0;
  for(int l = 0; l < MCP_LEVELS; ++l)
  {
    for(int i = 0; i < anCounts[l]; ++i, ++k)
    {
      const mcp_pvs_entry& e = mvPvsOut[k];
      ROS_ASSERT(e.point >= 0 && e.point < (int)mvMapTableRows.size());     // the table has exactly the rows UploadMapTable wrote
      if(!mvNearRows.empty() && !((mvNearRows[e.point] >> nCamIndex) & 1))
        continue;                       // !sbCollectAllPoints: not a co-visible point of this camera's nearest keyframe
      MapPoint& point = *mvMapTableRows[e.point];
      if(!point.mmpTData.count(cameraName))
        point.mmpTData[cameraName] = new TrackerData(&point, mmSizes[cameraName]);
      boost::intrusive_ptr<TrackerData> pTData(point.mmpTData[cameraName]);

      // what Project, GetDerivsUnsafe and CalcSearchLevelAndWarpMatrix leave behind (TrackerData.h:102-130, PatchFinder.cc:69-122)
      pTData->mv3Cam = se3CamFromWorld * point.mv3WorldPos;
      pTData->mbInImage = true;
      pTData->mv2Image = makeVector(e.image[0], e.image[1]);
      pTData->mm2CamDerivs(0, 0) = e.cam_derivs[0]; pTData->mm2CamDerivs(0, 1) = e.cam_derivs[1];
      pTData->mm2CamDerivs(1, 0) = e.cam_derivs[2]; pTData->mm2CamDerivs(1, 1) = e.cam_derivs[3];
      Matrix<2> m2WarpInverse;
      m2WarpInverse(0, 0) = e.warp_inverse[0]; m2WarpInverse(0, 1) = e.warp_inverse[1];
      m2WarpInverse(1, 0) = e.warp_inverse[2]; m2WarpInverse(1, 1) = e.warp_inverse[3];
      pTData->mFinder.SetSearchLevelAndWarp(e.level, m2WarpInverse);
      pTData->mnSearchLevel = e.level;

      if(point.mnUsing > mmCameraModels.size())
      {
        ROS_FATAL_STREAM("Tracker: mnUsing greater than number of cameras, counting leak!: "<<point.mnUsing);
        ROS_BREAK();
      }
      pTData->mbSearched = false;
      pTData->mbFound = false;
      vPVSLevels[l].push_back(pTData);      // rows ascending; TrackMap random_shuffles every level next (:983)
    }
  }
}

// ---- the whole TrackMap from the table in one submission (include/mcp_img.h, mcp_track_map) --------------------------------------------
// Replaces src/Tracker.cc:938-1075 (FindPVS of every camera, the shuffles, TestForCoarse, the coarse gate and iterations,
// SetupFineTracking, the fine iterations).  Needs, in addition to the FindPVS members above, in class Tracker:
//     bool TrackMapOnDevice(...);      (its full declaration is with TrackFrameOnDevice below)
//     void UploadMapSources();
// and the patch sources of the rows: UploadMapSources() below, after UploadMapTable() (option (a); with option (b) the same call goes
// with each row update, as mcp_map_points_update_source).  Keys: the point's address >> 4, as TrackStageOnDevice uses.  Truncated to an
// int two live points can share a key, and with option (a) a row changes points whenever the map drops one; either only costs a finder
// that has seen nothing (a new key) or a template cache tested against another point's warp (a shared key).  A unique id per MapPoint
// (a counter assigned when the point enters the map) avoids the second.  The cameras go in mvCurrCamNames order every frame (the
// table keeps a finder per (row, camera index)).
// The bookkeeping TrackMap leaves behind comes from the same submission (mcp_track_map_record with want_items = 0): the level counters and
// the per-camera quality arithmetic, the inlier / outlier marks (applied to the table's count column on the device; the host repeats them
// on the MapPoints from the 8-byte notes, so that the next UploadMapTable sends the same numbers up again), the found measurements (32
// bytes each) and RefreshSceneDepth (:1085, :1180-1228) of every camera.  No 320-byte item crosses.  The host keeps mdTotalDepthMean
// and mnLostFrames, and AssessOverallTrackingQuality's heuristics on top of rec.quality[]; IsDistanceToNearestMultiKeyFrameExcessive is a
// query of the map graph (IsDistanceToNearestMultiKeyFrameExcessiveOnDevice below).
// Needs in class Tracker:   mcp_track_record mTrackRecord;   (the last frame's record, read by AssessTrackingQuality below)
// Deviations: mv3Cam of the tracked points, and with it the depths of RefreshSceneDepth, are the final pose's (the reference leaves the
// value of the last ProjectAndDerivs).  mv2Image / mm2CamDerivs of the TrackerData keep FindPVS's values of the prior pose: nothing after
// TrackMap reads them before the next frame's FindPVS overwrites them (a caller that draws the re-projections asks for want_items = 1 and
// reads mcp_track_map_view as before).
void Tracker::UploadMapSources()
{
  // caller holds mMap.mMutex; rows as UploadMapTable() wrote them
  const int n = (int)mvMapTableRows.size();
  if(n == 0)
    return;
  std::vector<int> vKeys(n), vLevels(n), vCenters(2*n);
  std::vector<mcp_kf*> vSources(n);
  std::vector<uint8_t> vFixed(n);
  for(int k = 0; k < n; ++k)
  {
    MapPoint& point = *mvMapTableRows[k];
    vKeys[k] = (int)(reinterpret_cast<uintptr_t>(&point) >> 4);
    vSources[k] = point.mpPatchSourceKF ? point.mpPatchSourceKF->mpDev : NULL;
    vLevels[k] = point.mnSourceLevel;
    vCenters[2*k] = point.mirCenter.x;
    vCenters[2*k + 1] = point.mirCenter.y;
    vFixed[k] = point.mbFixed ? 1 : 0;
  }
  if(mcp_map_points_set_source(mpMapTable, 0, n, &vKeys[0], &vSources[0], &vLevels[0], &vCenters[0], &vFixed[0]) != 0)
  {
    ROS_FATAL_STREAM("Tracker::UploadMapSources: "<<mcp_last_error());
    ros::shutdown();
  }
}

// With pMotion the same submission also runs the frame's pyramids (apImages / anStrides: one 8-bit image per camera, mvCurrCamNames order),
// the tracker's SmallBlurryImages, CalcSBIRotation and ApplyMotionModel before TrackMap and UpdateMotionModel's velocity behind it
// (mcp_track_frame_motion): see TrackFrameOnDevice below.  Without it: TrackMap alone from the pose and the pyramids as they stand.
// With pRecover (and pMotion with apply = 0) the submission starts with the relocaliser over pRecover's candidates and TrackMap runs from the pose
// it finds, or not at all (mcp_track_frame_recover): see TrackFrameRecoverOnDevice below.  Returns false when nobody recovered: nothing was
// tracked and nothing below the call is touched.
bool Tracker::TrackMapOnDevice(const mcp_track_motion_params* pMotion, const uint8_t* const* apImages, const int* anStrides, mcp_track_motion* pMotionOut,
                               const RecoverCandidates* pRecover, mcp_track_recover* pRecoverOut)
{
  const int nCams = (int)mvCurrCamNames.size();
  std::vector<mcp_kf*> vKF(nCams);
  std::vector<mcp_camera> vCams(nCams), vCamsSBI(pMotion ? nCams : 0);
  std::vector<double> vCfB(12 * nCams);
  for(int c = 0; c < nCams; ++c)
  {
    KeyFrame& kf = *mpCurrentMKF->mmpKeyFrames[mvCurrCamNames[c]];
    ROS_ASSERT(kf.mpDev);
    vKF[c] = kf.mpDev;
    vCams[c] = mcptam_hip::CameraExport::Make(mmCameraModels[mvCurrCamNames[c]]);
    if(pMotion)
      vCamsSBI[c] = mcptam_hip::CameraExport::Make(mmCameraModelsSBI[mvCurrCamNames[c]]);      // the 40x30 camera of SE3fromSE2 (:1701)
    ToArray12(kf.mse3CamFromBase, &vCfB[12*c]);
    for(int l = 0; l < LEVELS; ++l)
      mmMeasAttemptedLevels[mvCurrCamNames[c]][l] = mmMeasFoundLevels[mvCurrCamNames[c]][l] = 0;
  }

  // the heuristics of :988-1008 stay here
  mcp_track_map_params prm;
  prm.try_coarse = !(Tracker::sbDisableCoarse || mdMSDScaledVelocityMagnitude < Tracker::sdCoarseMinVelocity || Tracker::snCoarseMax == 0);
  prm.coarse_max = Tracker::snCoarseMax;
  prm.coarse_range = Tracker::snCoarseRange;
  if(mbJustRecoveredSoUseCoarse || pRecover)                // (:549-550: a recovery sets the flag before its TrackMap)
  {
    prm.try_coarse = 1;
    prm.coarse_max *= 2;
    prm.coarse_range *= 2;
    mbJustRecoveredSoUseCoarse = false;
  }
  prm.coarse_min = Tracker::snCoarseMin;
  prm.coarse_subpix_its = Tracker::snCoarseSubPixIts;
  prm.max_patches = Tracker::snMaxPatchesPerFrame;
  prm.estimator = MCP_MEST_TUKEY;
  if(Tracker::sMEstimatorName == "Cauchy") prm.estimator = MCP_MEST_CAUCHY;
  else if(Tracker::sMEstimatorName == "Huber") prm.estimator = MCP_MEST_HUBER;
  prm.seed = mnFrame;                                   // a different shuffle every frame, reproducible per frame

  double adBfW[12];
  ToArray12(mpCurrentMKF->mse3BaseFromWorld, adBfW);
  mcp_track_record_params rprm;
  rprm.lost = IsLost() ? 1 : 0;
  rprm.want_items = 0;
  rprm.min_patches = Tracker::snMinPatchesPerFrame;
  rprm.coarse_min = Tracker::snCoarseMin;
  rprm.quality_good = Tracker::sdTrackingQualityGood;
  rprm.quality_bad = Tracker::sdTrackingQualityBad;
  mcp_track_map_result res;
  {
    boost::mutex::scoped_lock lock(mMap.mMutex);
    UploadMapTable();                                   // rows and their counts
    UploadMapSources();
    mcp_track_recover_params qprm;
    qprm.reloc_blur = 2.5;                                // SmallBlurryImage's default blur, KeyFrame::MakeSBI
    qprm.reloc_iterations = 6;                            // src/Relocaliser.cc:76
    qprm.max_score = Relocaliser::sdRecoveryMaxScore;
    // tracker_collect_all_points: false walks the store in front of the PVS launch, at the pose that launch reads (host-only, every frame:
    // the depth means are this frame's)
    mcp_collect_params cprm = CollectParams();
    if(mcp_track_collect_nearest(mpMapTable, Tracker::sbCollectAllPoints ? NULL : mMap.mpMapGraph, &cprm) != 0)
    {
      ROS_FATAL_STREAM("Tracker::TrackMapOnDevice: "<<mcp_last_error());
      ros::shutdown();
      return false;
    }
    mcp_track_pose_cov_enable(mpMapTable, 1);             // mm6PoseCovariance rides in the same submission (two launches behind the fine iterations)
    const int rc = pRecover ? mcp_track_frame_recover(mpMapTable, nCams, &vKF[0], apImages, anStrides, 0, NULL, &vCams[0], &vCamsSBI[0], adBfW, &vCfB[0], &prm, &res, &rprm,
                                                      &mTrackRecord, pMotion, pMotionOut, (int)pRecover->vKF.size(), pRecover->vKF.empty() ? NULL : &pRecover->vKF[0],
                                                      pRecover->vCam.empty() ? NULL : &pRecover->vCam[0], pRecover->vPose.empty() ? NULL : &pRecover->vPose[0],
                                                      &qprm, pRecoverOut, NULL)
                   : pMotion ? mcp_track_frame_motion(mpMapTable, nCams, &vKF[0], apImages, anStrides, 0, NULL, &vCams[0], &vCamsSBI[0], adBfW, &vCfB[0], &prm, &res, &rprm,
                                                    &mTrackRecord, pMotion, pMotionOut)
                           : mcp_track_map_record(mpMapTable, nCams, &vKF[0], NULL, NULL, 0, NULL, &vCams[0], adBfW, &vCfB[0], &prm, &res, &rprm, &mTrackRecord);
    if(rc != 0)
    {
      ROS_FATAL_STREAM("Tracker::TrackMapOnDevice: "<<mcp_last_error());
      ros::shutdown();
      return false;
    }
  }
  if(pRecover && !pRecoverOut->recovered)
    return false;                                         // :496: no TrackMap, no AssessOverallTrackingQuality
  const mcp_track_record& rec = mTrackRecord;
  mbDidCoarse = res.did_coarse != 0;
  Matrix<3> m3R;
  Vector<3> v3T;
  for(int i = 0; i < 3; ++i)
  {
    for(int j = 0; j < 3; ++j)
      m3R(i, j) = adBfW[3*i + j];
    v3T[i] = adBfW[9 + i];
  }
  mpCurrentMKF->mse3BaseFromWorld = SE3<>(SO3<>(m3R), v3T);
  UpdateCamsFromWorld();

  // mvIterationSets and the MapPoint counters from the notes, mv2Found from the measurements, the level maps and the scene depth from the record
  mvIterationSets.assign(nCams, TrackerDataPtrVector());
  mnNumInliers = rec.n_inliers;
  // mm6PoseCovariance (:1498-1502) from the record the same wait brought back: SVD<6>(wls.get_C_inv()).get_pinv() of the last fine iteration.
  // valid == -1 (non-finite sums) leaves zeros, as the record documents.  GetCurrentCovarianceNorm() keeps its host factor
  // mnTotalAttempted / (double)mnNumInliers: mnTotalAttempted is what AssessTrackingQuality below left for the last camera it assessed (:1635).
  mcp_track_pose_cov_record cov;
  if(mcp_track_pose_cov_last(mpMapTable, &cov) != 0)
  {
    ROS_FATAL_STREAM("Tracker::TrackMapOnDevice: "<<mcp_last_error());
    ros::shutdown();
    return false;
  }
  ROS_ASSERT(cov.valid != 1 || cov.n_used == rec.n_inliers);
  for(int i = 0; i < 6; ++i)
    for(int j = 0; j < 6; ++j)
      mm6PoseCovariance(i, j) = cov.cov[6*i + j];
  for(int c = 0; c < nCams; ++c)
  {
    const std::string& camName = mvCurrCamNames[c];
    KeyFrame& kf = *mpCurrentMKF->mmpKeyFrames[camName];
    const SE3<>& se3CamFromWorld = kf.mse3CamFromWorld;
    for(int l = 0; l < LEVELS; ++l)
    {
      mmMeasAttemptedLevels[camName][l] = rec.attempted[c][l];      // SearchForPoints :1322, 1347, 1361
      mmMeasFoundLevels[camName][l] = rec.found[c][l];
    }
    int n = 0, nMeas = 0;
    const mcp_track_note* pNotes = mcp_track_map_notes_view(mpMapTable, c, &n);
    const mcp_track_meas* pMeas = mcp_track_map_meas_view(mpMapTable, c, &nMeas);
    mvIterationSets[c].reserve(n);
    for(int i = 0; i < n; ++i)
    {
      const mcp_track_note& note = pNotes[i];
      MapPoint& point = *mvMapTableRows[note.row];
      if(!point.mmpTData.count(camName))
        point.mmpTData[camName] = new TrackerData(&point, mmSizes[camName]);
      boost::intrusive_ptr<TrackerData> pTData(point.mmpTData[camName]);
      TrackerData& td = *pTData;
      td.mv3Cam = se3CamFromWorld * point.mv3WorldPos;
      td.mbInImage = (note.flags & MCP_TN_IN_IMAGE) != 0;
      td.mnSearchLevel = note.level == 255 ? -1 : (int)note.level;
      td.mbSearched = (note.flags & MCP_TN_SEARCHED) != 0;
      td.mbFound = (note.flags & MCP_TN_FOUND) != 0;
      td.mbDidSubPix = (note.flags & MCP_TN_DID_SUBPIX) != 0;
      if(td.mnSearchLevel >= 0)
        td.mdSqrtInvNoise = 1.0 / LevelScale(td.mnSearchLevel);
      // the marks of the last iteration (:1452-1489), as the device applied them to the table's count column
      if(MCP_TN_MARK(note.flags) == 1) point.mnMEstimatorInlierCount++;
      else if(MCP_TN_MARK(note.flags) == 2) point.mnMEstimatorOutlierCount++;
      mvIterationSets[c].push_back(pTData);
    }
    // the found items in item order: what SaveSimpleMeasurements / RecordMeasurements walk (:1157-1177, 1237-1274).  Every row was usable
    // when the call started, so there is no mbBad to filter here
    for(int k = 0; k < nMeas; ++k)
      mvIterationSets[c][pMeas[k].item]->mv2Found = makeVector(pMeas[k].found_pos[0], pMeas[k].found_pos[1]);
    // RefreshSceneDepth (:1180-1209): KeyFrame::RefreshSceneDepthRobust(vector&) of this camera ran on the device
    if(rec.depth[c].refreshed == 1)
    {
      kf.mdSceneDepthMean = rec.depth[c].mean;
      kf.mdSceneDepthSigma = rec.depth[c].sigma;
    }
    else if(rec.depth[c].refreshed < 0)                  // :635-644: the reference stops the process on a non-finite mean
    {
      ROS_FATAL_STREAM("Tracker::TrackMapOnDevice: scene depth of "<<camName<<" is not finite");
      ros::shutdown();
      return false;
    }
  }
  // the rest of RefreshSceneDepth (:1212-1226) stays on the host
  double dSumDepth = 0.0;
  int nNum = 0;
  for(KeyFramePtrMap::iterator kf_it = mpCurrentMKF->mmpKeyFrames.begin(); kf_it != mpCurrentMKF->mmpKeyFrames.end(); ++kf_it)
  {
    KeyFrame& kf = *(kf_it->second);
    if(!kf.mbActive)
      continue;
    dSumDepth += kf.mdSceneDepthMean;
    ++nNum;
  }
  ROS_ASSERT(nNum > 0);
  mpCurrentMKF->mdTotalDepthMean = dSumDepth/nNum;
  return true;
}

// ---- RecordMeasurements of a frame tracked on the device (src/Tracker.cc:1237-1274) -------------------------------------------------------
// Runs when the tracker has decided to hand the current MKF to the map maker, behind the TrackMapOnDevice of the same frame, so the
// measurement views still show that frame.  Two things happen:
//   * the Measurement objects of the keyframes, as before, from the views (camera c's found items in item order) -- the map maker's own
//     bookkeeping and the early-outs of ReFind read them;
//   * the same list goes into a measurement parcel that the MKF owns (MultiKeyFrame::mpMeasParcel), ON THE DEVICE and without a wait: the MKF
//     now waits in the map maker's queue while this tracker goes on tracking on the same table and overwrites the views.  The map maker
//     commits the parcel when the MKF enters the map (GraphCommitTrackerParcel, shim/BundleAdjusterBase_gpu.cc); what happened to the points
//     in between is judged there, on the device.
// An MKF that never reaches the map destroys its parcel with itself.
void Tracker::RecordMeasurements()
{
  static gvar3<int> gvnCrossCamera("CrossCamera", 1, HIDDEN|SILENT);
  const bool bCrossCamera = *gvnCrossCamera != 0;
  const int nCams = (int)mvCurrCamNames.size();
  for(int c = 0; c < nCams; ++c)
  {
    const std::string& camName = mvCurrCamNames[c];
    KeyFrame& kf = *mpCurrentMKF->mmpKeyFrames[camName];
    int nMeas = 0;
    const mcp_track_meas* pMeas = mcp_track_map_meas_view(mpMapTable, c, &nMeas);
    for(int k = 0; k < nMeas; ++k)
    {
      const mcp_track_meas& m = pMeas[k];
      MapPoint& point = *mvMapTableRows[m.row];
      if(point.mbBad)
        continue;
      if(!bCrossCamera && point.mpPatchSourceKF->mCamName != camName)
        continue;
      Measurement* pNew = new Measurement;
      pNew->eSource = Measurement::SRC_TRACKER;
      pNew->nLevel = m.level;
      pNew->bSubPix = m.subpix != 0;
      pNew->v2RootPos = makeVector(m.found_pos[0], m.found_pos[1]);
      kf.AddMeasurement(&point, pNew);
    }
  }
  if(!mpCurrentMKF->mpMeasParcel)
    mpCurrentMKF->mpMeasParcel = mcp_meas_parcel_create(mpMapTable);
  if(!mpCurrentMKF->mpMeasParcel || mcp_meas_parcel_from_track(mpCurrentMKF->mpMeasParcel) < 0)
  {
    ROS_FATAL_STREAM("Tracker::RecordMeasurements: "<<mcp_last_error());
    ros::shutdown();
  }
}

// ---- IsDistanceToNearestMultiKeyFrameExcessive (src/MapMakerClientBase.cc:203-211) over the map graph ------------------------------------
// Replaces the call mMapMaker.IsDistanceToNearestMultiKeyFrameExcessive(*mpCurrentMKF) in AssessOverallTrackingQuality.  The current MKF is
// not in the map: it goes with the call as the external MKF of mcp_map_neighbours (pose, mbActive and mdSceneDepthMean per camera index), and
// ClosestMultiKeyFrame over mlpMultiKeyFrames becomes one item.  The closest MKF's mdTotalDepthMean is the host's (the graph holds the
// keyframes' means).  Needs in class Tracker:   bool IsDistanceToNearestMultiKeyFrameExcessiveOnDevice();
// NeedNewMultiKeyFrame's map side is the same query (the queue side, ClosestMultiKeyFrameInQueue, stays with MapMakerClientBase).
bool Tracker::IsDistanceToNearestMultiKeyFrameExcessiveOnDevice()
{
  mcp_neigh_params params;
  std::memset(&params, 0, sizeof params);
  params.kind = MCP_NB_MKF;
  params.order = MCP_NB_NEAREST;
  params.src_slot = -1;
  params.n_max = 1;
  params.max_dist = std::numeric_limits<double>::infinity();
  params.mean_diff_fraction = KeyFrame::sdDistanceMeanDiffFraction;
  ToArray12(mpCurrentMKF->mse3BaseFromWorld, params.ext_base_from_world);
  for(unsigned c = 0; c < mvCurrCamNames.size(); ++c)
  {
    KeyFramePtrMap::iterator kf_it = mpCurrentMKF->mmpKeyFrames.find(mvCurrCamNames[c]);
    const bool bActive = kf_it != mpCurrentMKF->mmpKeyFrames.end() && kf_it->second->mbActive;
    params.ext_active[c] = bActive ? 1 : 0;
    params.ext_depth_mean[c] = bActive ? kf_it->second->mdSceneDepthMean : 0.0;
  }
  mcp_neigh_result res;
  if(mcp_map_neighbours(mMap.mpMapGraph, &params, &res) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_neighbours: " << mcp_last_error());
    ROS_BREAK();
  }
  if(res.status == 3 || res.count == 0)     // KeyFrame::Distance's ROS_BREAK; ClosestMultiKeyFrame's ROS_ASSERT on an empty map
  {
    ROS_FATAL_STREAM("IsDistanceToNearestMultiKeyFrameExcessive: no closest MKF, status " << res.status);
    ROS_BREAK();
  }
  MultiKeyFrame* pClosestMKF = mMapMaker.GraphSlotMKF(res.item[0].slot);     // (the bundle adjuster's mvpSlotMKF, behind an accessor)
  const double dDist = res.item[0].dist * (1.0 / pClosestMKF->mdTotalDepthMean);     // scale by depth
  return dDist > MapMakerClientBase::sdMaxScaledMKFDist * 3;
}

// ---- TrackFrame's tracking branch in one submission (include/mcp_img.h, mcp_track_frame_motion) ------------------------------------------
// Replaces, for a frame with a good map, src/Tracker.cc:303-330 (MakeKeyFrame_Lite and the SmallBlurryImages of every camera), :431-434
// (ApplyMotionModel, TrackMap, UpdateMotionModel) with :1516-1555 and :1687-1749 behind them.  The tracker's SBIs live in the
// map table per camera index, so mmpSBIThisFrame / mmpSBILastFrame are not kept here; Tracker::Reset calls mcp_track_motion_reset(mpMapTable).
// The caller keeps mbActive, the timing messages and everything after UpdateMotionModel (:436 on).  Needs in class Tracker:
//     struct RecoverCandidates { std::vector<mcp_kf*> vKF; std::vector<int> vCam; std::vector<double> vPose; };      // see TrackFrameRecoverOnDevice
//     bool TrackMapOnDevice(const mcp_track_motion_params* pMotion = NULL, const uint8_t* const* apImages = NULL, const int* anStrides = NULL,
//                           mcp_track_motion* pMotionOut = NULL, const RecoverCandidates* pRecover = NULL, mcp_track_recover* pRecoverOut = NULL);
//     void FrameMotionParams(ImageBWMap& imFrames, bool bApply, mcp_track_motion_params& mprm, std::vector<const uint8_t*>& vImages, std::vector<int>& vStrides);
//     void TrackFrameOnDevice(ImageBWMap& imFrames);
//     bool TrackFrameRecoverOnDevice(ImageBWMap& imFrames);
// Deviation: a process duration that is not positive is an error here (the reference divides by it).
void Tracker::FrameMotionParams(ImageBWMap& imFrames, bool bApply, mcp_track_motion_params& mprm, std::vector<const uint8_t*>& vImages, std::vector<int>& vStrides)
{
  const int nCams = (int)mvCurrCamNames.size();
  vImages.resize(nCams);
  vStrides.resize(nCams);
  std::memset(&mprm, 0, sizeof mprm);
  mprm.apply = bApply ? 1 : 0;
  mprm.use_rotation_estimator = Tracker::sbUseRotationEstimator ? 1 : 0;
  mprm.sbi_iterations = 6;                                     // :1700
  mprm.blur = Tracker::sdRotationEstimatorBlur;
  mprm.dt = mLastProcessDur.toSec();
  for(int k = 0; k < 6; ++k)
    mprm.velocity[k] = mv6BaseVelocity[k];
  for(int c = 0; c < nCams; ++c)
  {
    CVD::Image<CVD::byte>& im = imFrames[mvCurrCamNames[c]];
    vImages[c] = im.data();
    vStrides[c] = im.row_stride();
    mprm.cam_good[c] = mmTrackingQuality[mvCurrCamNames[c]] == GOOD ? 1 : 0;      // :1695
  }
}

void Tracker::TrackFrameOnDevice(ImageBWMap& imFrames)
{
  mcp_track_motion_params mprm;
  std::vector<const uint8_t*> vImages;
  std::vector<int> vStrides;
  FrameMotionParams(imFrames, true, mprm, vImages, vStrides);
  mse3StartPose = mpCurrentMKF->mse3BaseFromWorld;              // :1518
  mcp_track_motion motion;
  TrackMapOnDevice(&mprm, &vImages[0], &vStrides[0], &motion);  // pose, cameras' poses, the record's bookkeeping, mdTotalDepthMean
  for(int k = 0; k < 6; ++k)
    mv6BaseVelocity[k] = motion.velocity[k];                    // :1547
  // :1552-1554: the velocity scaled by the mean scene depth, which mixes in the depths of cameras that were not refreshed: host
  Vector<6> v6 = mv6BaseVelocity;
  v6.slice<0,3>() *= 1.0 / mpCurrentMKF->mdTotalDepthMean;
  mdMSDScaledVelocityMagnitude = sqrt(v6*v6);
}

// ---- TrackFrame's lost branch in one submission (include/mcp_img.h, mcp_track_frame_recover) ---------------------------------------------
// Replaces, for a frame with a map and a lost tracker, src/Tracker.cc:303-330 (the pyramids and the tracker's SmallBlurryImages), :496-498
// (AttemptRecovery and TrackMap) with :526-552 and src/Relocaliser.cc:61-120 behind them: the relocaliser's SBI of every camera (into the
// keyframes' device handles), ScoreKFs over every keyframe of the map that has a device handle, the alignment against the winner, SE3fromSE2 and
// the pose products, then TrackMap from the recovered pose -- or no TrackMap when no camera recovered.  The candidates' poses are read here,
// under the map lock, at every call: they change with every adjustment.  In TrackFrame:
//     if(TrackFrameRecoverOnDevice(imFrames)) { AssessOverallTrackingQuality(); ReleasePointLock(); }
// Deviation: the reference stops at the first camera that recovers; here every camera's relocaliser SBI is made and evaluated, and the first
// camera in mvCurrCamNames order that recovered is used.  mRelocaliser is not called; its mse2 / mse3Best are not kept.
bool Tracker::TrackFrameRecoverOnDevice(ImageBWMap& imFrames)
{
  mcp_track_motion_params mprm;
  std::vector<const uint8_t*> vImages;
  std::vector<int> vStrides;
  FrameMotionParams(imFrames, false, mprm, vImages, vStrides);
  RecoverCandidates cands;
  {
    boost::mutex::scoped_lock lock(mMap.mMutex);
    for(MultiKeyFramePtrList::iterator it = mMap.mlpMultiKeyFrames.begin(); it != mMap.mlpMultiKeyFrames.end(); ++it)
    {
      MultiKeyFrame& mkf = *(*it);
      for(KeyFramePtrMap::iterator jit = mkf.mmpKeyFrames.begin(); jit != mkf.mmpKeyFrames.end(); ++jit)
      {
        KeyFrame& kf = *(jit->second);
        int c = 0;
        while(c < (int)mvCurrCamNames.size() && mvCurrCamNames[c] != kf.mCamName)
          ++c;
        if(c == (int)mvCurrCamNames.size() || !kf.mpDev)         // "only look at same camera" (Relocaliser.cc:103); no device twin: skipped like a missing mpSBI
          continue;
        cands.vKF.push_back(kf.mpDev);
        cands.vCam.push_back(c);
        cands.vPose.resize(cands.vPose.size() + 12);
        ToArray12(kf.mse3CamFromWorld, &cands.vPose[cands.vPose.size() - 12]);
      }
    }
  }
  mcp_track_motion motion;
  mcp_track_recover recover;
  if(!TrackMapOnDevice(&mprm, &vImages[0], &vStrides[0], &motion, &cands, &recover))
    return false;                                               // :545-546
  // :538, :548-550.  TrackMapOnDevice has set mse3BaseFromWorld to the refined pose and called UpdateCamsFromWorld
  Matrix<3> m3R;
  Vector<3> v3T;
  for(int i = 0; i < 3; ++i)
  {
    for(int j = 0; j < 3; ++j)
      m3R(i, j) = recover.base_from_world[3*i + j];
    v3T[i] = recover.base_from_world[9 + i];
  }
  mse3StartPose = SE3<>(SO3<>(m3R), v3T);
  mv6BaseVelocity = Zeros;
  mbJustRecoveredSoUseCoarse = false;                           // the doubled caps were used by this very call
  return true;
}

// AssessTrackingQuality (:1618-1658) from the record of TrackMapOnDevice: the same arithmetic ran on the device from the same counters
// (mnTotalAttempted / mnTotalFound are kept for the caller's messages)
Tracker::TrackingQuality Tracker::AssessTrackingQuality(std::string cameraName)
{
  int c = 0;
  while(c < (int)mvCurrCamNames.size() && mvCurrCamNames[c] != cameraName)
    ++c;
  ROS_ASSERT(c < (int)mvCurrCamNames.size());
  mnTotalAttempted = mnTotalFound = 0;
  for(int l = 0; l < LEVELS; ++l)
  {
    mnTotalAttempted += mTrackRecord.attempted[c][l];
    mnTotalFound += mTrackRecord.found[c][l];
  }
  return mTrackRecord.quality[c] == 2 ? GOOD : (mTrackRecord.quality[c] == 1 ? DODGY : BAD);
}
