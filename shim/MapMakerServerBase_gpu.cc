// MapMakerServerBase_gpu.cc -- MI355X bodies of the map maker's PatchFinder callers.
//
// Replace, in /root/reference/src/MapMakerServerBase.cc:
//   * the two PatchFinder loops of AddPointEpipolar (:745-795 hypothesis search, :827-853 sub-pixel refinement) by the two helper
//     calls below (the arc construction :604-743 above them and the triangulation / MapPoint creation :855-918 below stay), and
//   * ReFind_Common (:921-1002), ReFindInSingleKeyFrame (:1005-1019), ReFindNewlyMade (:1024-1059), ReFindFromFailureQueue (:1062-1080)
//     by the bodies below.
// The reference runs ONE PatchFinder through each of these loops and PatchFinder is stateful (template cache of
// MakeTemplateCoarseCont, src/PatchFinder.cc:144-181; Jacobians / mean difference of the sub-pixel iteration), so the loops become
// SEQUENCES: one wavefront walks one finder's items in order, its members live in an mcp_pf_state.  The epipolar loops hand them to
// mcp_patch_sequences, the re-find loops to mcp_map_refind, which reads the points from the resident map-point table (include/mcp_img.h).
// The map-side bookkeeping (measurement maps, never-retry sets, failure queue) is the reference's, unchanged.
// Needs KeyFrame::mpDev (shim/KeyFrame_gpu.cc), shim/CameraExport.h, and the table with MapPoint::mnTableRow (shim/Tracker_gpu.cc: the map
// maker holds the same mcp_map_points* as mpMapTable), and in class MapMakerServerBase: mcp_meas_parcel* mpReFindParcel
// (mcp_meas_parcel_create(mpMapTable) where the table is handed over; mcp_meas_parcel_destroy before the table goes).
// AddStereoMapPoints also needs the map's row allocator -- in class Map: std::vector<int> mvFreeRows; int mnNextRow, mnNextKey -- and
// MapPoint::mnTableKey next to mnTableRow (the key the row carries for this point: parcels and the finders tell points apart by it).
// At the end of this file: HandleOutliers (:1198-1238) and MapMaker::HandleBadEntities (src/MapMaker.cc:477-492) over mcp_map_cull_outliers /
// mcp_map_cull_sweep, and MarkFurthestMultiKeyFrameAsBad (:264-318) over mcp_map_mkf_cull -- delete those three bodies too; then InitFromMultiKeyFrame
// (:146-261), AddInitDepthMapPoints (:499-546), ApplyGlobalScaleToMap (:549-574) and ApplyGlobalTransformationToMap (:577-596) over
// mcp_init_depth_map_points, mcp_map_mark_optimized, mcp_map_rescale and mcp_map_transform -- delete those four bodies as well.
#include <mcptam/MapMakerServerBase.h>
#include <mcptam/MapMaker.h>
#include <mcptam/BundleAdjusterBase.h>
#include <mcptam/MapPoint.h>
#include <mcptam/KeyFrame.h>
#include <mcptam/LevelHelpers.h>
#include <mcp_img.h>
#include "CameraExport.h"
#include <ros/ros.h>
#include <algorithm>
#include <cstring>

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

void Identity12(double a[12])
{
  for(int i = 0; i < 12; ++i)
    a[i] = 0.0;
  a[0] = a[4] = a[8] = 1.0;
}

void FillPoint(const MapPoint& point, mcp_td_in& in)
{
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

int KeyOf(const MapPoint* pPoint)   // identity of a MapPoint object (the reference compares addresses, PatchFinder.cc:148)
{
  return (int)(reinterpret_cast<uintptr_t>(pPoint) >> 4);
}
}  // namespace

void GraphCommitReFindParcel(Map& map, mcp_meas_parcel* pParcel, const std::vector<KeyFrame*>& vTargets, int nExpected);      // shim/BundleAdjusterBase_gpu.cc

// ---- AddPointEpipolar, first loop (:745-795): every hypothesised position along the epipolar arc through ONE finder, in order.
// vMapPointPositions: (world position, position in the target camera) per step, as built at :706-723; `point` is the probe MapPoint
// of :726-738.  Fills vScoresIndicesBestMatches / nBest / nBestZMSSD / v2BestMatch exactly as the loop did; `state` is the finder
// (zero-initialised by the caller = `PatchFinder finder;` at :740) and has to be passed on to EpipolarRefine.
bool MapMakerServerBase::EpipolarSearch(KeyFrame& kfTarget, TaylorCamera& cameraTarget, MapPoint& point,
                                        const std::vector<std::pair<Vector<3>, Vector<3> > >& vMapPointPositions, mcp_pf_state& state,
                                        std::vector<mcp_pf_item>& vItems,
                                        std::vector<std::tuple<int, int, Vector<2> > >& vScoresIndicesBestMatches, int& nBest, int& nBestZMSSD,
                                        Vector<2>& v2BestMatch)
{
  const int n = (int)vMapPointPositions.size();
  vItems.resize(n);
  for(int i = 0; i < n; ++i)
  {
    point.mv3WorldPos = vMapPointPositions[i].first;
    point.RefreshPixelVectors();                    // src/MapPoint.cc:62-87, per hypothesis as at :749-750
    FillPoint(point, vItems[i].point);
    vItems[i].point_key = KeyOf(&point);            // one MapPoint object for all hypotheses: the template cache sees "the same point"
    vItems[i].target = 0;
    vItems[i].start_pos[0] = vItems[i].start_pos[1] = 0.0;
  }
  mcp_camera cam = mcptam_hip::CameraExport::Make(cameraTarget);
  mcp_pf_target target;
  target.kf = kfTarget.mpDev;                       // its level-0 mask (if any) was uploaded by MakeKeyFrame_Lite: the check of :763-765
  target.cam = &cam;
  ToArray12(kfTarget.mse3CamFromWorld, target.base_from_world);
  Identity12(target.cam_from_base);
  std::vector<mcp_td_out> vOut(n > 0 ? n : 1);
  const int anSeq[2] = { 0, n };
  if(mcp_patch_sequences(MCP_PF_EPI_COARSE, 1, &target, 1, anSeq, &vItems[0], &state, 3, 0, 0, &vOut[0]) != 0)   // range 3, :779
  {
    ROS_FATAL_STREAM("MapMakerServerBase::AddPointEpipolar: "<<mcp_last_error());
    ros::shutdown();
    return false;
  }
  for(int i = 0; i < n; ++i)
  {
    if(!vOut[i].found)
      continue;
    const Vector<2> v2Match = makeVector(vOut[i].found_pos[0], vOut[i].found_pos[1]);     // finder.GetCoarsePosAsVector()
    vScoresIndicesBestMatches.push_back(std::make_tuple(vOut[i].score, i, v2Match));
    if(vOut[i].score < nBestZMSSD)
    {
      nBestZMSSD = vOut[i].score;
      nBest = i;
      v2BestMatch = v2Match;
    }
  }
  return nBest != -1;
}

// ---- AddPointEpipolar, second loop (:827-853): the one to three surviving matches, best first, on the SAME finder; the first whose
// sub-pixel iteration converges wins.
bool MapMakerServerBase::EpipolarRefine(KeyFrame& kfTarget, TaylorCamera& cameraTarget, const std::vector<mcp_pf_item>& vItems, mcp_pf_state& state,
                                        const std::vector<std::tuple<int, int, Vector<2> > >& vScoresIndicesBestMatches, Vector<2>& v2SubPixPos)
{
  const int n = (int)vScoresIndicesBestMatches.size();
  std::vector<mcp_pf_item> vRefine(n);
  for(int i = 0; i < n; ++i)
  {
    vRefine[i] = vItems[std::get<1>(vScoresIndicesBestMatches[i])];     // same point, same pixel vectors as in the first loop (:835-836)
    vRefine[i].start_pos[0] = std::get<2>(vScoresIndicesBestMatches[i])[0];   // finder.SetSubPixPos(v2CurrBestMatch), :843
    vRefine[i].start_pos[1] = std::get<2>(vScoresIndicesBestMatches[i])[1];
  }
  mcp_camera cam = mcptam_hip::CameraExport::Make(cameraTarget);
  mcp_pf_target target;
  target.kf = kfTarget.mpDev;
  target.cam = &cam;
  ToArray12(kfTarget.mse3CamFromWorld, target.base_from_world);
  Identity12(target.cam_from_base);
  std::vector<mcp_td_out> vOut(n > 0 ? n : 1);
  const int anSeq[2] = { 0, n };
  if(mcp_patch_sequences(MCP_PF_EPI_REFINE, 1, &target, 1, anSeq, &vRefine[0], &state, 3, 10, 0, &vOut[0]) != 0)
  {
    ROS_FATAL_STREAM("MapMakerServerBase::AddPointEpipolar: "<<mcp_last_error());
    ros::shutdown();
    return false;
  }
  // The reference stops at the first candidate that converges; the later ones only change the finder, which is discarded
  // (`PatchFinder finder` is a local of AddPointEpipolar), so evaluating all of them is not observable.
  for(int i = 0; i < n; ++i)
  {
    if(vOut[i].found)
    {
      v2SubPixPos = makeVector(vOut[i].found_pos[0], vOut[i].found_pos[1]);
      return true;
    }
  }
  return false;
}

// ---- ReFind_Common (:921-1002) for one keyframe and MANY points, or one point and MANY keyframes: the checks that need the map's own
// sets (:925-937) stay here; everything after them is ONE mcp_map_refind over the resident map-point table (shim/Tracker_gpu.cc keeps the
// table and gives every MapPoint its row, MapPoint::mnTableRow): per pair the device projects, makes the template from the row's patch
// source, searches and refines, and returns one verdict byte per pair and a Measurement record per found pair -- no mcp_pf_item goes up, no
// mcp_td_out comes down.  The reference's finder is `static` (:939): its cache can only hit when consecutive calls carry the same MapPoint,
// which is what ReFindNewlyMade does (a new point walked over all keyframes), so there every run of one point is one finder
// (per_row_finders = 1); ReFindInSingleKeyFrame and ReFindFromFailureQueue change the point from call to call, i.e. every pair has its own.
// mFinderStateReFind (a member, zero-initialised) carries the static finder across calls.  The table must hold the points' current
// positions and sources: the map maker updates the rows it moves (mcp_ba_write_back does it for an adjustment) and uploads the rows of
// new points (mcp_map_points_update / _update_source / _update_rays) before it re-finds them.
int MapMakerServerBase::ReFindBatch(std::vector<std::pair<KeyFrame*, MapPoint*> >& vPairs, bool bOneFinderPerPoint)
{
  // the early-outs of :925-937
  std::vector<std::pair<KeyFrame*, MapPoint*> > vWork;
  static gvar3<int> gvnCrossCamera("CrossCamera", 1, HIDDEN|SILENT);
  for(unsigned i = 0; i < vPairs.size(); ++i)
  {
    KeyFrame& kf = *vPairs[i].first;
    MapPoint& point = *vPairs[i].second;
    if(point.mMMData.spMeasurementKFs.count(&kf) || point.mMMData.spNeverRetryKFs.count(&kf))
      continue;
    if(point.mbBad || kf.mpParent->mbBad)
      continue;
    if(!*gvnCrossCamera && kf.mCamName != point.mpPatchSourceKF->mCamName)
      continue;
    vWork.push_back(vPairs[i]);
  }
  if(vWork.empty())
    return 0;

  // targets: the distinct keyframes
  std::vector<KeyFrame*> vKFs;
  std::map<KeyFrame*, int> mTargetIdx;
  for(unsigned i = 0; i < vWork.size(); ++i)
  {
    KeyFrame* pKF = vWork[i].first;
    if(mTargetIdx.count(pKF))
      continue;
    mTargetIdx[pKF] = (int)vKFs.size();
    vKFs.push_back(pKF);
  }
  std::vector<mcp_camera> vCams(vKFs.size());
  std::vector<mcp_refind_target> vTargets(vKFs.size());
  for(unsigned t = 0; t < vKFs.size(); ++t)
  {
    ROS_ASSERT(vKFs[t]->mpDev);
    vCams[t] = mcptam_hip::CameraExport::Make(mmCameraModels[vKFs[t]->mCamName]);
    vTargets[t].kf = vKFs[t]->mpDev;
    vTargets[t].cam = &vCams[t];
    ToArray12(vKFs[t]->mse3CamFromWorld, vTargets[t].cam_from_world);
  }

  // the pair list: (table row, target)
  std::vector<int> vRowTarget(2*vWork.size());
  for(unsigned i = 0; i < vWork.size(); ++i)
  {
    ROS_ASSERT(vWork[i].second->mnTableRow >= 0);
    vRowTarget[2*i] = vWork[i].second->mnTableRow;
    vRowTarget[2*i + 1] = mTargetIdx[vWork[i].first];
  }
  std::vector<uint8_t> vVerdict(vWork.size());
  mcp_refind_result res;
  if(mcp_map_refind(mpMapTable, (int)vTargets.size(), &vTargets[0], (int)vWork.size(), &vRowTarget[0], bOneFinderPerPoint ? 1 : 0, &mFinderStateReFind,
                    &vVerdict[0], (int)vWork.size(), NULL, &res) != 0)
  {
    ROS_FATAL_STREAM("MapMakerServerBase::ReFind: "<<mcp_last_error());
    ros::shutdown();
    return 0;
  }

  // the rest of ReFind_Common per pair (:941-1001): camera.Invalid() / outside the image (:945-955), TemplateBad (:960-964) and not found
  // (:967-971) are never retried; a row whose patch source is gone (it cannot happen in the reference, which keeps the image) is left alone
  for(unsigned i = 0; i < vWork.size(); ++i)
  {
    if(vVerdict[i] == MCP_REFIND_OUTSIDE || vVerdict[i] == MCP_REFIND_TEMPLATE_BAD || vVerdict[i] == MCP_REFIND_NOT_FOUND)
      vWork[i].second->mMMData.spNeverRetryKFs.insert(vWork[i].first);
  }
  int nMeas = 0;
  const mcp_refind_meas* pMeasDev = mcp_map_refind_view(mpMapTable, &nMeas);     // read in place, in ascending pair index
  for(int k = 0; k < nMeas; ++k)
  {
    const mcp_refind_meas& r = pMeasDev[k];
    KeyFrame& kf = *vWork[r.pair].first;
    MapPoint& point = *vWork[r.pair].second;
    Measurement* pMeas = new Measurement;
    pMeas->nLevel = r.level;
    pMeas->eSource = Measurement::SRC_REFIND;
    pMeas->v2RootPos = makeVector(r.root_pos[0], r.root_pos[1]);    // sub-pixel position above level 0 (kept converged or not), coarse at level 0
    pMeas->bSubPix = r.subpix != 0;
    if(kf.mmpMeasurements.count(&point))
      ROS_BREAK();
    kf.AddMeasurement(&point, pMeas);
  }
  // the same measurements into the map graph's store, from the pinned block on the device (shim/BundleAdjusterBase_gpu.cc): a parcel the map
  // maker keeps (mpReFindParcel, created next to mpMapTable, destroyed before it), one lane per target keyframe.  The Measurement objects
  // above stay: the early-outs at the top of this function read them.
  if(nMeas > 0)
    GraphCommitReFindParcel(mMap, mpReFindParcel, vKFs, nMeas);
  return nMeas;
}

bool MapMakerServerBase::ReFind_Common(KeyFrame& kf, MapPoint& point)
{
  std::vector<std::pair<KeyFrame*, MapPoint*> > vPairs(1, std::make_pair(&kf, &point));
  return ReFindBatch(vPairs, false) == 1;
}

// A general data-association update for a single keyframe (:1005-1019): all map points against one keyframe in one call
int MapMakerServerBase::ReFindInSingleKeyFrame(KeyFrame& kf)
{
  std::vector<std::pair<KeyFrame*, MapPoint*> > vPairs;
  for(MapPointPtrList::iterator it = mMap.mlpPoints.begin(); it != mMap.mlpPoints.end(); ++it)
    vPairs.push_back(std::make_pair(&kf, *it));
  return ReFindBatch(vPairs, false);
}

// New map points against every keyframe (:1024-1059): one sequence per point, so that keyframes with similar warps share its
// template as they do through the reference's static finder.  The queue is drained in chunks so that the IncomingQueueSize()
// check of the reference keeps its meaning (it is evaluated between chunks instead of between single keyframes).
void MapMakerServerBase::ReFindNewlyMade()
{
  while(!mlpNewQueue.empty() && IncomingQueueSize() == 0)
  {
    std::vector<std::pair<KeyFrame*, MapPoint*> > vPairs;
    for(int nTaken = 0; nTaken < 64 && !mlpNewQueue.empty(); ++nTaken)
    {
      MapPoint* pPointNew = mlpNewQueue.front();
      mlpNewQueue.pop_front();
      if(pPointNew->mbBad)
        continue;
      for(MultiKeyFramePtrList::iterator it = mMap.mlpMultiKeyFrames.begin(); it != mMap.mlpMultiKeyFrames.end(); ++it)
      {
        MultiKeyFrame& mkf = *(*it);
        if(mkf.mbBad)
          continue;
        for(KeyFramePtrMap::iterator jiter = mkf.mmpKeyFrames.begin(); jiter != mkf.mmpKeyFrames.end(); ++jiter)
          vPairs.push_back(std::make_pair(jiter->second, pPointNew));
      }
    }
    ReFindBatch(vPairs, true);
  }
}

// Dud measurements get a second chance (:1062-1080)
void MapMakerServerBase::ReFindFromFailureQueue()
{
  if(mlFailureQueue.size() == 0)
    return;
  mlFailureQueue.sort();
  while(!mlFailureQueue.empty() && IncomingQueueSize() == 0)
  {
    std::vector<std::pair<KeyFrame*, MapPoint*> > vPairs;
    for(int nTaken = 0; nTaken < 256 && !mlFailureQueue.empty(); ++nTaken)
    {
      vPairs.push_back(mlFailureQueue.front());
      mlFailureQueue.pop_front();
    }
    ReFindBatch(vPairs, false);
  }
}

// ---- AddStereoMapPoints (:452-496) with one mcp_stereo_map_points call per source keyframe and level: ThinCandidates before every target, the
// arc, both PatchFinder loops, the selection, ReprojectPoint and the nLimit counter run on the device in one submission, and the created points
// go straight into the map-point table, the graph's point columns and the store (include/mcp_img.h): nothing is sent up again.  The
// targets come from the map graph: mcp_map_neighbours (keyframe kind, n_max = snMaxTriangulationKFs, max_dist as :463-470) is
// ClosestKeyFramesWithinDist over the graph's poses, active bytes and depth means -- at most n_max items come back, each with its MKF's flags.
// The host keeps the mbBad / CrossCamera / sbOnlyFirstCameraGeneratesPoints skips (a skipped target neither thins nor creates; a bad MKF is a
// candidate of the query, as in the reference's walk, and is skipped here after the list is cut), and building the MapPoints and Measurements
// from the records, in the reference's creation order.
// THE ROW HAND-OFF.  Rows are the host's to assign, and the call must know them before it knows how many points it makes: the map's row
// allocator (in class Map: std::vector<int> mvFreeRows, the rows of points whose trash was emptied; int mnNextRow, the table's end; int
// mnNextKey, the counter that gives every MapPoint its key) hands out one row and key per candidate, point k takes vRows[k], and the rows that
// were not taken go back.  A row comes out of mvFreeRows only after Map::EmptyTrash, when no live store entry names it.
// BUSY POSITIONS.  The source keyframe's measurements are in the store already (the tracker's parcel was committed when the MKF entered the
// map, the points of the levels before this one were appended by this call), so mmpMeasurements is not walked: busy_from_store = 1 gathers
// them on the device.  The gather is one pass over the store; profiles/map_graph/README.md has its cost against the walk it replaces.
namespace
{
void TakeFreeRows(Map& map, int n, std::vector<int>& vRows, std::vector<int>& vKeys)
{
  vRows.resize(n);
  vKeys.resize(n);
  for(int i = 0; i < n; ++i)
  {
    if(!map.mvFreeRows.empty())
    {
      vRows[i] = map.mvFreeRows.back();
      map.mvFreeRows.pop_back();
    }
    else
      vRows[i] = map.mnNextRow++;
    vKeys[i] = map.mnNextKey++;
  }
}

// the rows vRows[nTaken ..) were not used: back they go, the first of them to be handed out first again (their keys are just skipped)
void ReturnFreeRows(Map& map, const std::vector<int>& vRows, int nTaken)
{
  for(int i = (int)vRows.size() - 1; i >= nTaken; --i)
    map.mvFreeRows.push_back(vRows[i]);
}
}  // namespace

void MapMakerServerBase::AddStereoMapPoints(MultiKeyFrame& mkfSrc, int nLevel, int nLimit, double dDistThresh, KeyFrameRegion region)
{
  static gvar3<int> gvnCrossCamera("CrossCamera", 1, HIDDEN|SILENT);
  for(KeyFramePtrMap::iterator it = mkfSrc.mmpKeyFrames.begin(); it != mkfSrc.mmpKeyFrames.end(); it++)
  {
    if(MapMakerServerBase::sbOnlyFirstCameraGeneratesPoints && it != mkfSrc.mmpKeyFrames.begin())
      break;
    KeyFrame& kfSrc = *(it->second);
    Level& level = kfSrc.maLevels[nLevel];
    const double dDistThreshUsed = dDistThresh < 0 ? 1000 : dDistThresh;
    mcp_neigh_params nbParams;
    std::memset(&nbParams, 0, sizeof nbParams);
    nbParams.kind = MCP_NB_KF;
    nbParams.region = region == KF_ONLY_SELF ? MCP_NB_ONLY_SELF : (region == KF_ONLY_OTHER ? MCP_NB_ONLY_OTHER : MCP_NB_ALL);
    nbParams.order = MCP_NB_NEAREST;
    nbParams.src_slot = mkfSrc.mnGraphSlot;      // (the source MKF entered the map, and the graph, before its points are made)
    nbParams.src_cam = kfSrc.mnCamIndex;
    nbParams.n_max = std::min((int)MapMakerServerBase::snMaxTriangulationKFs, MCP_NB_MAX);
    nbParams.max_dist = dDistThreshUsed;
    nbParams.mean_diff_fraction = KeyFrame::sdDistanceMeanDiffFraction;
    mcp_neigh_result nbRes;
    if(mcp_map_neighbours(mMap.mpMapGraph, &nbParams, &nbRes) != 0)
    {
      ROS_FATAL_STREAM("mcp_map_neighbours: " << mcp_last_error());
      ROS_BREAK();
    }
    if(nbRes.status == 3)     // KeyFrame::Distance's ROS_BREAK, src/KeyFrame.cc:734-744
    {
      ROS_FATAL("AddStereoMapPoints: a keyframe distance is not finite or larger than 1e10");
      ROS_BREAK();
    }
    std::vector<KeyFrame*> vpTargets;
    std::vector<int> vTargetMKF, vTargetCam;     // the targets as the graph names them: where the SRC_EPIPOLAR entries go
    for(int j = 0; j < nbRes.count; ++j)
    {
      const mcp_neigh_item& item = nbRes.item[j];
      if(item.flags & MCP_MKF_BAD)     // vpAll[j]->mpParent->mbBad
        continue;
      if(!*gvnCrossCamera && kfSrc.mnCamIndex != item.cam)     // AddPointEpipolar's first check: the target creates nothing
        continue;
      MultiKeyFrame* pMKF = mBundleAdjuster.mvpSlotMKF[item.slot];
      vpTargets.push_back(pMKF->mmpKeyFrames[mBundleAdjuster.mvCamNames[item.cam]]);
      vTargetMKF.push_back(item.slot);
      vTargetCam.push_back(item.cam);
    }
    TaylorCamera& cameraSrc = mmCameraModels[kfSrc.mCamName];
    const mcp_camera camSrc = mcptam_hip::CameraExport::Make(cameraSrc);
    std::vector<mcp_camera> vCams(vpTargets.size());
    std::vector<mcp_stereo_target> vTargets(vpTargets.size());
    for(unsigned j = 0; j < vpTargets.size(); ++j)
    {
      TaylorCamera& cameraTarget = mmCameraModels[vpTargets[j]->mCamName];
      vCams[j] = mcptam_hip::CameraExport::Make(cameraTarget);
      ROS_ASSERT(vpTargets[j]->mpDev);
      vTargets[j].kf = vpTargets[j]->mpDev;
      vTargets[j].cam = &vCams[j];
      ToArray12(vpTargets[j]->mse3CamFromWorld, vTargets[j].cam_from_world);
      vTargets[j].one_pixel_angle = cameraTarget.OnePixelAngle();
    }
    std::vector<mcp_int2> vCand(level.vCandidates.size());
    for(unsigned i = 0; i < vCand.size(); ++i)
    {
      vCand[i].x = level.vCandidates[i].irLevelPos.x;
      vCand[i].y = level.vCandidates[i].irLevelPos.y;
    }
    double adSrc[12];
    ToArray12(kfSrc.mse3CamFromWorld, adSrc);
    const int n = (int)vCand.size();
    std::vector<mcp_stereo_point> vOut(n + 1);
    std::vector<uint8_t> vKeep(n + 1);
    std::vector<int> vRows, vKeys;
    TakeFreeRows(mMap, n, vRows, vKeys);
    ROS_ASSERT(kfSrc.mpDev);
    mcp_stereo_map_params params;
    params.src_mkf = mkfSrc.mnGraphSlot;
    params.src_cam = kfSrc.mnCamIndex;
    params.limit = nLimit;
    params.busy_from_store = 1;
    mcp_stereo_map_result result;
    const int nMade = mcp_stereo_map_points(mMap.mpMapGraph, kfSrc.mpDev, &camSrc, adSrc, nLevel, n, n ? &vCand[0] : NULL, 0, NULL,
                                            (int)vTargets.size(), vTargets.empty() ? NULL : &vTargets[0], vTargets.empty() ? NULL : &vTargetMKF[0],
                                            vTargets.empty() ? NULL : &vTargetCam[0], n, n ? &vRows[0] : NULL, n ? &vKeys[0] : NULL, &params, &result,
                                            &vOut[0], &vKeep[0], NULL);
    if(nMade < 0)
    {
      ROS_FATAL_STREAM("MapMakerServerBase::AddStereoMapPoints: "<<mcp_last_error());
      ros::shutdown();
      return;
    }
    ReturnFreeRows(mMap, vRows, nMade);
    if((int)mBundleAdjuster.mvpRowPoint.size() < mMap.mnNextRow)
      mBundleAdjuster.mvpRowPoint.resize(mMap.mnNextRow, NULL);
    // The host objects follow the records; their rows, graph columns and store entries are on the device already, so none of them goes through
    // the table updates, GraphUploadPoints or GraphAddMeasurements.
    for(int k = 0; k < nMade; ++k)       // :862-914, in creation order
    {
      const mcp_stereo_point& r = vOut[k];
      KeyFrame& kfTarget = *vpTargets[r.target];
      MapPoint* pPointNew = new MapPoint;
      pPointNew->mnTableRow = vRows[k];
      pPointNew->mnTableKey = vKeys[k];
      mBundleAdjuster.mvpRowPoint[vRows[k]] = pPointNew;
      pPointNew->mv3WorldPos = makeVector(r.world_pos[0], r.world_pos[1], r.world_pos[2]);
      pPointNew->mpPatchSourceKF = &kfSrc;
      pPointNew->mnSourceLevel = nLevel;
      pPointNew->mv3Normal_NC = makeVector(0, 0, -1);
      pPointNew->mirCenter = level.vCandidates[r.candidate].irLevelPos;
      pPointNew->mv3Center_NC = makeVector(r.center_nc[0], r.center_nc[1], r.center_nc[2]);
      pPointNew->mv3OneRightFromCenter_NC = makeVector(r.one_right_nc[0], r.one_right_nc[1], r.one_right_nc[2]);
      pPointNew->mv3OneDownFromCenter_NC = makeVector(r.one_down_nc[0], r.one_down_nc[1], r.one_down_nc[2]);
      pPointNew->mv3PixelRight_W = makeVector(r.pixel_right_w[0], r.pixel_right_w[1], r.pixel_right_w[2]);     // RefreshPixelVectors, on the device
      pPointNew->mv3PixelDown_W = makeVector(r.pixel_down_w[0], r.pixel_down_w[1], r.pixel_down_w[2]);
      Measurement* pMeasSrc = new Measurement;
      pMeasSrc->eSource = Measurement::SRC_ROOT;
      pMeasSrc->v2RootPos = makeVector(r.root_pos[0], r.root_pos[1]);
      pMeasSrc->nLevel = nLevel;
      pMeasSrc->bSubPix = true;
      Measurement* pMeasTarget = new Measurement;
      *pMeasTarget = *pMeasSrc;
      pMeasTarget->eSource = Measurement::SRC_EPIPOLAR;
      pMeasTarget->v2RootPos = makeVector(r.target_pos[0], r.target_pos[1]);
      kfSrc.AddMeasurement(pPointNew, pMeasSrc);
      kfTarget.AddMeasurement(pPointNew, pMeasTarget);
      mMap.mlpPoints.push_back(pPointNew);
      mlpNewQueue.push_back(pPointNew);
    }
    std::vector<Candidate> vKept;                // ThinCandidates as the reference leaves it: before the last target
    for(int i = 0; i < n; ++i)
      if(vKeep[i])
        vKept.push_back(level.vCandidates[i]);
    level.vCandidates = vKept;
  }
}

// ---- HandleOutliers (:1198-1238) in ONE call on the map graph ------------------------------------------------------------------------------------
// The reference walks the outlier list and re-reads GoodMeasCount() after every erasure; mcp_map_cull_outliers does that walk on the device (the
// store knows every measurement's source and which are alive, the graph the flags) and hands back one verdict byte per outlier.  Nothing
// map-sized crosses the link: the list goes up, the verdicts come down.  The verdicts drive what only the host has: mlFailureQueue,
// spNeverRetryKFs, the Measurement objects and bTransferred / vOutliersRemoved.  The host's own walk over its MapPoint objects runs alongside
// (it costs a list walk) and must agree; a disagreement is warned about, in the manner of GraphCommitTrackerParcel, and the device's verdict is
// the one applied, because the next select reads the device's store.
void MapMakerServerBase::HandleOutliers(std::vector<std::pair<KeyFrame*, MapPoint*> >& vOutliers)
{
  const int n = (int)vOutliers.size();
  std::vector<int> vMKF(n), vCam(n), vRow(n);
  for(int i = 0; i < n; ++i)
  {
    vMKF[i] = vOutliers[i].first->mpParent->mnGraphSlot;
    vCam[i] = vOutliers[i].first->mnCamIndex;
    vRow[i] = vOutliers[i].second->mnTableRow;
  }
  mcp_cull_outliers_params params;
  params.bad_good_count = 2;
  mcp_cull_outliers_result res;
  std::vector<uint8_t> vVerdict(n);
  if(mcp_map_cull_outliers(mMap.mpMapGraph, n, vMKF.data(), vCam.data(), vRow.data(), &params, vVerdict.data(), &res) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_cull_outliers: " << mcp_last_error());   // (a repeated key or a slot out of range: the solver's list is broken)
    ROS_BREAK();
  }

  std::vector<std::pair<KeyFrame*, MapPoint*> > vOutliersRemoved;
  int nDisagree = 0;
  for(int i = 0; i < n; ++i)
  {
    KeyFrame& kf = *(vOutliers[i].first);
    MapPoint& point = *(vOutliers[i].second);
    MeasPtrMap::iterator meas_it = kf.mmpMeasurements.find(&point);
    // the host's own verdict, from its objects as they stand (the reference's tests in the reference's order)
    int nHost = MCP_CULL_ALREADY_BAD;
    if(meas_it == kf.mmpMeasurements.end())
      nHost = MCP_CULL_MISSING;
    else if(point.mbFixed)
      nHost = MCP_CULL_FIXED;
    else if(point.mMMData.GoodMeasCount() <= 2 || meas_it->second->eSource == Measurement::SRC_ROOT)
      nHost = MCP_CULL_POINT_BAD;
    else if(!point.mbBad)
      nHost = (meas_it->second->eSource == Measurement::SRC_TRACKER || meas_it->second->eSource == Measurement::SRC_EPIPOLAR) ? MCP_CULL_RETRY : MCP_CULL_NEVER_RETRY;
    if(nHost != vVerdict[i])
      ++nDisagree;

    switch(vVerdict[i])
    {
      case MCP_CULL_POINT_BAD:
        point.mbBad = true;     // (its row is bad on the device already; the sweep reports it, and HandleBadEntities moves it to the trash)
        break;
      case MCP_CULL_RETRY:
      case MCP_CULL_NEVER_RETRY:
      {
        if(meas_it == kf.mmpMeasurements.end())
          break;                // (counted as a disagreement above)
        if(vVerdict[i] == MCP_CULL_RETRY)
          mlFailureQueue.push_back(vOutliers[i]);
        else
          point.mMMData.spNeverRetryKFs.insert(&kf);
        const bool bTransferred = meas_it->second->bTransferred;
        kf.EraseMeasurementOfPoint(&point);
        point.mMMData.spMeasurementKFs.erase(&kf);
        if(bTransferred)
          vOutliersRemoved.push_back(vOutliers[i]);
        break;
      }
      default:                  // MISSING, FIXED, ALREADY_BAD: nothing changes
        break;
    }
  }
  vOutliers.swap(vOutliersRemoved);

  ROS_INFO_STREAM("======== Number of outlier fixed points: " << res.n_fixed_rows);
  if(res.n_rows_marked > 0)
    ROS_INFO_STREAM("======== Handle outlier measurements marked " << res.n_rows_marked << " points as bad");
  if(nDisagree > 0 || res.n_missing > 0)
    ROS_WARN_STREAM("HandleOutliers: the host's walk disagrees with the device on " << nDisagree << " of " << n << " outliers (" << res.n_missing << " without a live store entry)");
}

// ---- MapMaker::HandleBadEntities (src/MapMaker.cc:477-492): the point half in ONE call --------------------------------------------------------------
// MarkDanglersAsBad, MarkOutliersAsBad and Map::MoveBadPointsToTrash read GoodMeasCount() and the tracker's counts of every point: the store
// and the table's count column, both on the device.  mcp_map_cull_sweep marks the rows, erases the measurements of every bad row (whoever
// marked it), clears the table's usable byte (the tracker's next FindPVS drops the point without a table upload) and reports the rows the
// DEVICE turned bad since the last sweep; the points the host marked bad itself (mbBad set here and uploaded with GraphUploadPoints) it finds
// in its own list.  Trashed MKFs are erased from the graph first, as the reference moves them first: a bad MKF still counts as present for the
// dangler rule's "two MKFs" until then.  mcp_map_graph_compact stays where it was: after the sweep, when the dead entries pass a share.
void MapMaker::HandleBadEntities()
{
  for(MultiKeyFramePtrList::iterator it = mMap.mlpMultiKeyFrames.begin(); it != mMap.mlpMultiKeyFrames.end(); ++it)
    if((*it)->mbBad && (*it)->mnGraphSlot >= 0)
    {
      mcp_map_graph_erase_mkf(mMap.mpMapGraph, (*it)->mnGraphSlot);
      (*it)->mnGraphSlot = -1;
    }
  mMap.MoveBadMultiKeyFramesToTrash();
  mMap.MoveDeletedMultiKeyFramesToTrash();

  mcp_cull_sweep_params params;
  params.min_outliers = MapMakerClientBase::snMinOutliers;
  params.outlier_multiplier = MapMakerClientBase::sdOutlierMultiplier;
  params.danglers = 1;
  mcp_cull_sweep_result res;
  if(mcp_map_cull_sweep(mMap.mpMapGraph, &params, &res) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_cull_sweep: " << mcp_last_error());
    ROS_BREAK();
  }
  int nRows = 0;
  const int* pRows = mcp_map_cull_rows_view(mMap.mpMapGraph, &nRows);
  for(int i = 0; i < nRows; ++i)
  {
    MapPoint* pPoint = mBundleAdjuster.mvpRowPoint[pRows[i]];
    if(pPoint)
      pPoint->mbBad = true;     // (MoveBadPointsToTrash below erases its Measurement objects and moves it; its row is free for reuse after EmptyTrash)
  }
  if(res.n_tracker_outliers > 0)
    ROS_INFO_STREAM("======== Handle outlier based on tracker marked " << res.n_tracker_outliers << " points as bad");

  // the host's list must now hold exactly the device's bad rows: every mbBad point is a bad row there, and no other written row is bad
  int nHostBad = 0;
  for(MapPointPtrList::iterator it = mMap.mlpPoints.begin(); it != mMap.mlpPoints.end(); ++it)
    nHostBad += (*it)->mbBad ? 1 : 0;
  mMap.MoveBadPointsToTrash();
  mMap.MoveDeletedPointsToTrash();
  if(nHostBad < res.n_reported)
    ROS_WARN_STREAM("HandleBadEntities: the device reported " << res.n_reported << " rows, the host's list holds " << nHostBad << " bad points");

  int nLive = 0, nStored = 0;
  if(mcp_map_graph_num_meas(mMap.mpMapGraph, &nLive, &nStored) == 0 && nStored - nLive > nStored / 4)
    mcp_map_graph_compact(mMap.mpMapGraph);

  EraseBadEntitiesFromQueues();
  mMap.EmptyTrash();
}

// ---- MarkFurthestMultiKeyFrameAsBad (:264-318) in ONE call ------------------------------------------------------------------------------------------
// FurthestMultiKeyFrame, the walk over every measurement of the victim's keyframes, the point rule (:281-283) and ClosestMultiKeyFrame for the
// fixed hand-over all read what the graph holds: mcp_map_mkf_cull picks the victim, marks it MCP_MKF_BAD, marks the rows (they get the pending
// mark: the sweep of HandleBadEntities reports them, and that body sets mbBad on the MapPoints), moves MCP_MKF_FIXED and, with erase, takes the
// victim's entries and its slot out of the graph -- what HandleBadEntities' mcp_map_graph_erase_mkf did for it.  The host repeats the two flags
// on its objects; Map::MoveBadMultiKeyFramesToTrash then trashes the MKF as before.
void MapMakerServerBase::MarkFurthestMultiKeyFrameAsBad(MultiKeyFrame& mkf)
{
  mcp_mkf_cull_params params;
  params.slot = -1;
  params.furthest_from = mkf.mnGraphSlot;
  params.mark_points = 1;
  params.max_kfs = 2;
  params.erase = 1;
  params.mean_diff_fraction = KeyFrame::sdDistanceMeanDiffFraction;
  mcp_mkf_cull_result res;
  if(mcp_map_mkf_cull(mMap.mpMapGraph, &params, &res) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_mkf_cull: " << mcp_last_error());
    ROS_BREAK();
  }
  if(res.status != 0)     // 1: FurthestMultiKeyFrame's ROS_ASSERT (no other MKF at a distance > 0); 3: KeyFrame::Distance's ROS_BREAK
  {
    ROS_FATAL_STREAM("MarkFurthestMultiKeyFrameAsBad: no victim, status " << res.status);
    ROS_BREAK();
  }
  MultiKeyFrame* pFurthestMKF = mBundleAdjuster.mvpSlotMKF[res.victim];
  pFurthestMKF->mbBad = true;
  pFurthestMKF->mnGraphSlot = -1;     // (erased: HandleBadEntities has nothing left to erase for it)
  if(res.new_fixed >= 0)
    mBundleAdjuster.mvpSlotMKF[res.new_fixed]->mbFixed = true;
  ROS_INFO_STREAM("MarkFurthestMultiKeyFrameAsBad: slot " << res.victim << " at distance " << res.victim_dist << ", " << res.n_victim_meas << " measurements, "
                  << res.n_rows_marked << " points go bad (" << res.n_by_count << " by count, " << res.n_by_source << " by source)");
}

// ---- The map's beginning, its rescale and its re-alignment on the device ------------------------------------------------------------------------------
// Replace, in /root/reference/src/MapMakerServerBase.cc: InitFromMultiKeyFrame (:146-261), AddInitDepthMapPoints (:499-546), ApplyGlobalScaleToMap
// (:549-574) and ApplyGlobalTransformationToMap (:577-596) by the four bodies below.  The points of ssInitPointMode "idp" / "both" no longer go up by
// hand (mcp_map_points_update, _update_rays, _update_source, mcp_map_graph_update_points, mcp_map_graph_add_meas): mcp_init_depth_map_points makes
// them where the map lives, all cameras of the MKF in one call, with the row hand-off of AddStereoMapPoints above.  A rescale or a re-alignment
// no longer tears the table and the graph down: mcp_map_rescale / mcp_map_transform rewrite every pose, every point and its pixel vectors (and,
// for a rescale, every keyframe's scene depth) in one submission, and every row keeps its finder state.  The host's own objects follow from the
// read-backs (mcp_map_points_get, mcp_graph_get_mkfs, depth_out); they are what the reference's host code (the tracker's hand-over, the
// queues) goes on reading.
void GraphUploadMKFs(Map& map, const std::vector<MultiKeyFrame*>& vpMKFs, const std::vector<std::string>& vCamNames);      // shim/BundleAdjusterBase_gpu.cc
void GraphRefreshSceneDepth(Map& map, MultiKeyFrame& mkf, const std::vector<std::string>& vCamNames);

bool MapMakerServerBase::InitFromMultiKeyFrame(MultiKeyFrame* pMKF, bool bPutPlaneAtOrigin)
{
  ROS_INFO("MapMakerServerBase::InitFromMultiKeyFrame");
  pMKF->mbFixed = true;
  pMKF->mse3BaseFromWorld = SE3<>();
  for(KeyFramePtrMap::iterator it = pMKF->mmpKeyFrames.begin(); it != pMKF->mmpKeyFrames.end(); it++)
  {
    KeyFrame& kf = *(it->second);
    kf.mse3CamFromWorld = kf.mse3CamFromBase * pMKF->mse3BaseFromWorld;
    kf.mdSceneDepthMean = 100;
    kf.mdSceneDepthSigma = 100000;
    kf.MakeKeyFrame_Rest();
  }
  mMap.mlpMultiKeyFrames.push_back(pMKF);
  // its slot: pose, flags and the depth mean of 100 (:158) go up once; everything below reads them from the graph
  int nSlot = 0;                                  // the first free slot of mvpSlotMKF, as where an MKF enters the map from the queue
  while(nSlot < (int)mBundleAdjuster.mvpSlotMKF.size() && mBundleAdjuster.mvpSlotMKF[nSlot])
    ++nSlot;
  if(nSlot == (int)mBundleAdjuster.mvpSlotMKF.size())
    mBundleAdjuster.mvpSlotMKF.push_back(NULL);
  mBundleAdjuster.mvpSlotMKF[nSlot] = pMKF;
  pMKF->mnGraphSlot = nSlot;
  GraphUploadMKFs(mMap, std::vector<MultiKeyFrame*>(1, pMKF), mBundleAdjuster.mvCamNames);

  const int nNumCams = pMKF->mmpKeyFrames.size();
  static gvar3<int> gvnLevelZeroPoints("LevelZeroPoints", 0, HIDDEN|SILENT);
  ROS_INFO_STREAM("==== STARTING INIT POINT CREATION, MODE: "<<MapMakerServerBase::ssInitPointMode<<"  =========");
  for(int l = 3; l >= 0; --l)
  {
    if(l == 0 && *gvnLevelZeroPoints == false)
      continue;
    const int nLevelLimit = MapMakerServerBase::snMaxInitPointsLevelZero/LevelScale(l);
    int nNumPointsBefore = mMap.mlpPoints.size();
    if(MapMakerServerBase::ssInitPointMode == "stereo" || MapMakerServerBase::ssInitPointMode == "both")
      AddStereoMapPoints(*pMKF, l, nLevelLimit, std::numeric_limits<double>::max(), KF_ONLY_SELF);     // the body above: mcp_stereo_map_points
    const int nLevelPoints = mMap.mlpPoints.size() - nNumPointsBefore;
    const int nLevelPointsLeft = (nLevelLimit*nNumCams - nLevelPoints)/nNumCams;
    ROS_INFO_STREAM("Level "<<l<<" made "<<nLevelPoints<<" with stereo, "<<nLevelPointsLeft<<" points left to make with each cam");
    if(nLevelPointsLeft < 1)
      continue;
    nNumPointsBefore = mMap.mlpPoints.size();
    if(MapMakerServerBase::ssInitPointMode == "idp" || MapMakerServerBase::ssInitPointMode == "both")
      AddInitDepthMapPoints(*pMKF, l, nLevelPointsLeft, MapMakerServerBase::sdInitDepth);
    ROS_INFO_STREAM("Made "<<mMap.mlpPoints.size() - nNumPointsBefore<<" points with Init Depth");
  }
  if((int)mMap.mlpPoints.size() < MapMakerServerBase::snMinMapPoints)
  {
    ROS_ERROR_STREAM("MapMakerServerBase: Epipolar matching and init depth method didn't make enough map points: "<<mMap.mlpPoints.size()<<"  Minimum is: "<<MapMakerServerBase::snMinMapPoints);
    return false;
  }
  // :212-215 -- the tracker may track these points: usable = 1 on every row of the table that the graph knows and does not call bad
  int nMarked = 0;
  if(mcp_map_mark_optimized(mMap.mpMapGraph, &nMarked) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_mark_optimized: "<<mcp_last_error());
    ROS_BREAK();
  }
  for(MapPointPtrList::iterator point_it = mMap.mlpPoints.begin(); point_it != mMap.mlpPoints.end(); ++point_it)
    (*point_it)->mbOptimized = true;
  if(nMarked != (int)mMap.mlpPoints.size())
    ROS_WARN_STREAM("InitFromMultiKeyFrame: the device marked "<<nMarked<<" rows, the map holds "<<mMap.mlpPoints.size()<<" points");
  mBundleAdjuster.SetNotConverged();
  GraphRefreshSceneDepth(mMap, *pMKF, mBundleAdjuster.mvCamNames);     // pMKF->RefreshSceneDepthRobust() (:219): mcp_graph_refresh_depth
  ROS_INFO_STREAM("MapMakerServerBase: Made initial map with " << mMap.mlpPoints.size());
  mMap.mbGood = true;
  return true;
}

void MapMakerServerBase::AddInitDepthMapPoints(MultiKeyFrame& mkfSrc, int nLevel, int nLimit, double dInitDepth)
{
  const std::vector<std::string>& vCamNames = mBundleAdjuster.mvCamNames;
  const int nc = (int)vCamNames.size();
  std::vector<mcp_init_depth_cam> vCams(nc);
  std::vector<mcp_camera> vCamModels(nc);
  std::vector<std::vector<mcp_int2> > vvCand(nc);
  std::vector<KeyFrame*> vpKFs(nc, (KeyFrame*)NULL);
  int nTotal = 0, nNeed = 0;
  for(int c = 0; c < nc; ++c)
  {
    std::memset(&vCams[c], 0, sizeof vCams[c]);
    KeyFramePtrMap::iterator kf_it = mkfSrc.mmpKeyFrames.find(vCamNames[c]);
    if(kf_it == mkfSrc.mmpKeyFrames.end())
      continue;                                   // a camera the MKF does not have: no candidates
    KeyFrame& kfSrc = *(kf_it->second);
    vpKFs[c] = &kfSrc;
    Level& level = kfSrc.maLevels[nLevel];
    vvCand[c].resize(level.vCandidates.size());
    for(unsigned i = 0; i < vvCand[c].size(); ++i)
    {
      vvCand[c][i].x = level.vCandidates[i].irLevelPos.x;
      vvCand[c][i].y = level.vCandidates[i].irLevelPos.y;
    }
    vCamModels[c] = mcptam_hip::CameraExport::Make(mmCameraModels[kfSrc.mCamName]);
    ROS_ASSERT(kfSrc.mpDev);
    vCams[c].src = kfSrc.mpDev;
    vCams[c].cam = &vCamModels[c];
    vCams[c].n_cand = (int)vvCand[c].size();
    vCams[c].cand = vvCand[c].empty() ? NULL : &vvCand[c][0];
    vCams[c].limit = nLimit;
    nTotal += vCams[c].n_cand;
    nNeed += std::min(vCams[c].n_cand, nLimit);
  }
  std::vector<int> vRows, vKeys;
  TakeFreeRows(mMap, nNeed, vRows, vKeys);
  std::vector<mcp_stereo_point> vOut(nNeed + 1);
  std::vector<uint8_t> vKeep(nTotal + 1);
  mcp_init_depth_params params;
  params.src_mkf = mkfSrc.mnGraphSlot;
  params.level = nLevel;
  params.init_depth = dInitDepth;
  mcp_init_depth_result result;
  const int nMade = mcp_init_depth_map_points(mMap.mpMapGraph, nc, &vCams[0], nNeed, nNeed ? &vRows[0] : NULL, nNeed ? &vKeys[0] : NULL, &params, &result, &vOut[0], &vKeep[0]);
  if(nMade < 0)
  {
    ROS_FATAL_STREAM("MapMakerServerBase::AddInitDepthMapPoints: "<<mcp_last_error());
    ros::shutdown();
    return;
  }
  ReturnFreeRows(mMap, vRows, nMade);
  if((int)mBundleAdjuster.mvpRowPoint.size() < mMap.mnNextRow)
    mBundleAdjuster.mvpRowPoint.resize(mMap.mnNextRow, NULL);
  // The host objects follow the records (:517-541), camera by camera in creation order; their rows, graph columns and store entries are on the
  // device already
  int k = 0, nCandAt = 0;
  for(int c = 0; c < nc; ++c)
  {
    if(!vpKFs[c])
      continue;
    KeyFrame& kfSrc = *vpKFs[c];
    Level& level = kfSrc.maLevels[nLevel];
    std::cout<<"AddInitDepthMapPoints, processing "<<level.vCandidates.size()<<" candidates"<<std::endl;
    for(int j = 0; j < result.made[c]; ++j, ++k)
    {
      const mcp_stereo_point& r = vOut[k];
      MapPoint* pPointNew = new MapPoint;
      pPointNew->mnTableRow = vRows[k];
      pPointNew->mnTableKey = vKeys[k];
      mBundleAdjuster.mvpRowPoint[vRows[k]] = pPointNew;
      pPointNew->mv3WorldPos = makeVector(r.world_pos[0], r.world_pos[1], r.world_pos[2]);
      pPointNew->mpPatchSourceKF = &kfSrc;
      pPointNew->mbFixed = false;
      pPointNew->mnSourceLevel = nLevel;
      pPointNew->mv3Normal_NC = makeVector(0, 0, -1);
      pPointNew->mirCenter = level.vCandidates[r.candidate].irLevelPos;
      pPointNew->mv3Center_NC = makeVector(r.center_nc[0], r.center_nc[1], r.center_nc[2]);
      pPointNew->mv3OneRightFromCenter_NC = makeVector(r.one_right_nc[0], r.one_right_nc[1], r.one_right_nc[2]);
      pPointNew->mv3OneDownFromCenter_NC = makeVector(r.one_down_nc[0], r.one_down_nc[1], r.one_down_nc[2]);
      pPointNew->mv3PixelRight_W = makeVector(r.pixel_right_w[0], r.pixel_right_w[1], r.pixel_right_w[2]);     // RefreshPixelVectors, on the device
      pPointNew->mv3PixelDown_W = makeVector(r.pixel_down_w[0], r.pixel_down_w[1], r.pixel_down_w[2]);
      mMap.mlpPoints.push_back(pPointNew);
      Measurement* pMeas = new Measurement;
      pMeas->v2RootPos = makeVector(r.root_pos[0], r.root_pos[1]);
      pMeas->nLevel = nLevel;
      pMeas->eSource = Measurement::SRC_ROOT;
      kfSrc.AddMeasurement(pPointNew, pMeas);
    }
    std::vector<Candidate> vKept;                // ThinCandidates (:506) leaves vCandidates = vCGood; the created ones stay in the list
    for(unsigned i = 0; i < level.vCandidates.size(); ++i)
      if(vKeep[nCandAt + i])
        vKept.push_back(level.vCandidates[i]);
    nCandAt += (int)level.vCandidates.size();
    level.vCandidates = vKept;
  }
}

namespace
{
// the host's objects after a rescale or a re-alignment: every pose from the graph (ONE ranged read over the slots in use), every point's position
// and pixel vectors from the table (one read)
void ReadMapBack(Map& map)
{
  const int nRows = map.mnNextRow;
  std::vector<double> vWorld(3*(size_t)nRows + 3), vRight(3*(size_t)nRows + 3), vDown(3*(size_t)nRows + 3);
  if(nRows > 0 && mcp_map_points_get(map.mpMapTable, 0, nRows, &vWorld[0], &vRight[0], &vDown[0], NULL) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_points_get: "<<mcp_last_error());
    ROS_BREAK();
  }
  for(MapPointPtrList::iterator it = map.mlpPoints.begin(); it != map.mlpPoints.end(); ++it)
  {
    MapPoint& point = *(*it);
    const size_t r = 3*(size_t)point.mnTableRow;
    point.mv3WorldPos = makeVector(vWorld[r], vWorld[r + 1], vWorld[r + 2]);
    point.mv3PixelRight_W = makeVector(vRight[r], vRight[r + 1], vRight[r + 2]);
    point.mv3PixelDown_W = makeVector(vDown[r], vDown[r + 1], vDown[r + 2]);
  }
  int nTop = -1;
  for(MultiKeyFramePtrList::iterator it = map.mlpMultiKeyFrames.begin(); it != map.mlpMultiKeyFrames.end(); ++it)
    nTop = std::max(nTop, (*it)->mnGraphSlot);
  std::vector<double> vPoses(12*(size_t)(nTop + 1) + 12);
  if(nTop >= 0 && mcp_graph_get_mkfs(map.mpMapGraph, 0, nTop + 1, &vPoses[0], NULL, NULL, NULL) != 0)
  {
    ROS_FATAL_STREAM("mcp_graph_get_mkfs: "<<mcp_last_error());
    ROS_BREAK();
  }
  for(MultiKeyFramePtrList::iterator it = map.mlpMultiKeyFrames.begin(); it != map.mlpMultiKeyFrames.end(); ++it)
  {
    MultiKeyFrame& mkf = *(*it);
    if(mkf.mnGraphSlot < 0)
      continue;
    const double* adPose = &vPoses[12*(size_t)mkf.mnGraphSlot];
    Matrix<3> m3;
    for(int i = 0; i < 3; ++i)
      for(int j = 0; j < 3; ++j)
        m3(i, j) = adPose[3*i + j];
    mkf.mse3BaseFromWorld = SE3<>(SO3<>(m3), makeVector(adPose[9], adPose[10], adPose[11]));
    for(KeyFramePtrMap::iterator kf_it = mkf.mmpKeyFrames.begin(); kf_it != mkf.mmpKeyFrames.end(); ++kf_it)
      kf_it->second->mse3CamFromWorld = kf_it->second->mse3CamFromBase * mkf.mse3BaseFromWorld;
  }
}
}  // namespace

void MapMakerServerBase::ApplyGlobalScaleToMap(double dScale)
{
  const int nc = (int)mBundleAdjuster.mvCamNames.size();
  std::vector<mcp_scene_depth> vDepth((size_t)MCP_MAP_MAX_MKFS*nc);
  mcp_map_transform_result res;
  if(mcp_map_rescale(mMap.mpMapGraph, dScale, &res, &vDepth[0]) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_rescale: "<<mcp_last_error());
    ROS_BREAK();
  }
  ReadMapBack(mMap);
  // depth_out: the present slots in ascending order, cameras in graph order
  int i = 0;
  for(int nSlot = 0; nSlot < (int)mBundleAdjuster.mvpSlotMKF.size() && i < res.n_mkfs; ++nSlot)
  {
    MultiKeyFrame* pMKF = mBundleAdjuster.mvpSlotMKF[nSlot];
    if(!pMKF || pMKF->mnGraphSlot != nSlot)
      continue;
    for(int c = 0; c < nc; ++c)
    {
      KeyFramePtrMap::iterator kf_it = pMKF->mmpKeyFrames.find(mBundleAdjuster.mvCamNames[c]);
      const mcp_scene_depth& d = vDepth[(size_t)i*nc + c];
      if(kf_it == pMKF->mmpKeyFrames.end() || d.refreshed != 1)
        continue;
      kf_it->second->mdSceneDepthMean = d.mean;
      kf_it->second->mdSceneDepthSigma = d.sigma;
    }
    ++i;
  }
  if(res.n_no_source > 0 || res.n_no_rays > 0)
    ROS_WARN_STREAM("ApplyGlobalScaleToMap: "<<res.n_no_source<<" rows without a source keyframe were left alone, "<<res.n_no_rays<<" rows without patch rays kept their pixel vectors");
}

void MapMakerServerBase::ApplyGlobalTransformationToMap(SE3<> se3NewFromOld)
{
  double adNewFromOld[12];
  ToArray12(se3NewFromOld, adNewFromOld);
  mcp_map_transform_result res;
  if(mcp_map_transform(mMap.mpMapGraph, adNewFromOld, &res) != 0)
  {
    ROS_FATAL_STREAM("mcp_map_transform: "<<mcp_last_error());
    ROS_BREAK();
  }
  ReadMapBack(mMap);
}
