// KeyFrame.hpp -- C++ host-side mirror of MCPTAM's KeyFrame / Level, SmallBlurryImage, Relocaliser scoring and the per-point
// part of Tracker over the C ABI of mcp_img.h.
//
// Member names and argument meaning follow the reference classes (/root/reference/include/mcptam/KeyFrame.h:93-260,
// SmallBlurryImage.h, Relocaliser.h, MiniPatch.h, Tracker.h); CVD / TooN types are replaced by plain arrays (images: packed
// bytes, SE3 = row-major R[9] + t[3] as 12 doubles, SE2 = { R00, R01, R10, R11, tx, ty }) so that the header depends on the
// C ABI only.  A MCPTAM tree uses the CVD/TooN-typed shims of INTEGRATION.md; this is what a stand-alone C++ caller and the
// C++ link test under tests/cpp use.  There is no CPU fallback: constructors throw when no gfx950 device is usable.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../mcp_img.h"
#include "ChainBundle.hpp"

namespace mcptam_hip {

/// What MakeKeyFrame_Lite / MakeKeyFrame_Rest leave in one pyramid level (KeyFrame.h:93-150), read back from the device.
struct Level {
  int w = 0, h = 0;
  std::vector<uint8_t> image;                 // Level::image, packed
  std::vector<mcp_int2> vCorners;             // raster order
  std::vector<int> vCornerRowLUT;
  int nFastThresh = 0;
  std::vector<double> vFastFrequency;         // index = threshold, MCP_MAX_FAST_THRESH + 1 entries
  std::vector<mcp_int2> vCandidates;          // Candidate::irLevelPos
  std::vector<double> vCandidateScores;       // Candidate::dSTScore
};

class KeyFrame {
 public:
  // statics / GVars of the reference (src/KeyFrame.cc:56-63, src/System.cc:121)
  static inline bool sbAdaptiveThresh = true;
  static inline double sdCandidateThresh = 70;
  static inline double sdCandidateTopFraction = 0.8;
  static inline std::string ssCandidateType = "fast";              // "fast" | "shi"
  static inline std::string ssCandidateCriterion = "percent";      // "percent" | "thresh"

  KeyFrame(int w, int h, bool bGlareMasking = false, bool bHalfSamplePavgb = false, int device = -1) {
    mcp_kf_params p;
    p.adaptive_thresh = sbAdaptiveThresh; p.glare_masking = bGlareMasking; p.half_sample_pavgb = bHalfSamplePavgb; p.device = device;
    mpDev = mcp_kf_create(w, h, &p);
    if (!mpDev) throw std::runtime_error(std::string("KeyFrame: ") + mcp_last_error());
  }
  ~KeyFrame() { mcp_kf_destroy(mpDev); }
  KeyFrame(const KeyFrame&) = delete;
  KeyFrame& operator=(const KeyFrame&) = delete;

  /// KeyFrame::MakeKeyFrame_Lite (src/KeyFrame.cc:145-360).  masks: nullptr or MCP_LEVELS pointers (each nullptr or packed).
  void MakeKeyFrame_Lite(const uint8_t* im, int stride, const uint8_t* const* masks = nullptr) {
    if (mcp_kf_make_lite(mpDev, im, stride, masks) != 0) throw std::runtime_error(mcp_last_error());
  }
  /// KeyFrame::MakeKeyFrame_Rest, candidate part incl. the stability pruning against the stored history (:363-527)
  void MakeKeyFrame_Rest(int nNonmaxScore = 0) {
    if (mcp_kf_make_rest(mpDev, ssCandidateType == "shi", ssCandidateCriterion == "percent", sdCandidateTopFraction,
                         sdCandidateThresh, nNonmaxScore) != 0) throw std::runtime_error(mcp_last_error());
  }
  /// frames in Level::imagePrev / vCornersPrev (0..2)
  int NumPrev() { return mcp_kf_num_prev(mpDev); }

  Level GetLevel(int l) {
    Level L;
    if (mcp_kf_level_size(mpDev, l, &L.w, &L.h) != 0) throw std::out_of_range(mcp_last_error());
    L.image.resize((size_t)L.w*L.h);
    check(mcp_kf_get_image(mpDev, l, L.image.data()));
    L.vCorners.resize((size_t)std::max(0, mcp_kf_num_corners(mpDev, l)));
    if (!L.vCorners.empty()) L.vCorners.resize((size_t)mcp_kf_get_corners(mpDev, l, L.vCorners.data(), (int)L.vCorners.size()));
    L.vCornerRowLUT.resize(L.h);
    check(mcp_kf_get_row_lut(mpDev, l, L.vCornerRowLUT.data()));
    L.nFastThresh = mcp_kf_fast_thresh(mpDev, l);
    L.vFastFrequency.resize(MCP_MAX_FAST_THRESH + 1);
    check(mcp_kf_get_fast_frequency(mpDev, l, L.vFastFrequency.data()));
    const int nc = std::max(0, mcp_kf_num_candidates(mpDev, l));
    L.vCandidates.resize(nc); L.vCandidateScores.resize(nc);
    if (nc) {
      const int got = mcp_kf_get_candidates(mpDev, l, L.vCandidates.data(), L.vCandidateScores.data(), nc);
      L.vCandidates.resize(got); L.vCandidateScores.resize(got);
    }
    return L;
  }

  // ---- SmallBlurryImage (KeyFrame::MakeSBI, src/KeyFrame.cc:539-545; src/SmallBlurryImage.cc)
  void MakeSBI(double dBlur = 2.5) { check(mcp_kf_make_sbi(mpDev, dBlur)); }
  /// SmallBlurryImage::IteratePosRelToTarget: (SE2, final sum of squares)
  std::pair<std::array<double, 6>, double> IteratePosRelToTarget(KeyFrame& other, int nIterations = 10) {
    std::array<double, 6> se2{}; double score = 0;
    check(mcp_sbi_iterate(mpDev, other.mpDev, nIterations, se2.data(), &score));
    return { se2, score };
  }
  /// Tracker::CalcSBIRotation's per-camera step: this frame's SBI against the one it replaced
  std::pair<std::array<double, 6>, double> IteratePosRelToLast(int nIterations = 6) {
    std::array<double, 6> se2{}; double score = 0;
    check(mcp_sbi_iterate_last(mpDev, nIterations, se2.data(), &score));
    return { se2, score };
  }
  /// SmallBlurryImage::SE3fromSE2 (cameras already at the 40x30 size): rotation, row-major
  static std::array<double, 9> SE3fromSE2(const std::array<double, 6>& se2, const mcp_camera& camSrc, const mcp_camera& camTarget) {
    std::array<double, 9> R{};
    if (mcp_sbi_se3_from_se2(se2.data(), &camSrc, &camTarget, R.data()) != 0) throw std::runtime_error(mcp_last_error());
    return R;
  }
  /// Relocaliser::ScoreKFs: (index of the best candidate or -1, all scores)
  std::pair<int, std::vector<double> > ScoreKFs(const std::vector<KeyFrame*>& vCandidates) {
    std::vector<mcp_kf*> h; h.reserve(vCandidates.size());
    for (KeyFrame* k : vCandidates) h.push_back(k ? k->mpDev : nullptr);
    std::vector<double> scores(vCandidates.size() + 1); int best = -1;
    check(mcp_sbi_score(mpDev, (int)vCandidates.size(), h.data(), scores.data(), &best));
    scores.resize(vCandidates.size());
    return { best, scores };
  }

  // ---- MiniPatch::SampleFromImage + FindPatch, batched (src/MiniPatch.cc:34-122): patches of *this at vSrc searched in `target`
  struct PatchMatch { mcp_int2 pos; bool found; int ssd; };
  std::vector<PatchMatch> FindPatches(KeyFrame& target, int nLevel, const std::vector<mcp_int2>& vSrc, const std::vector<mcp_int2>& vStart, int nRange) {
    if (vSrc.size() != vStart.size()) throw std::invalid_argument("FindPatches: one start position per patch");
    const int n = (int)vSrc.size();
    std::vector<mcp_int2> pos(n + 1); std::vector<uint8_t> found(n + 1); std::vector<int> ssd(n + 1);
    check(mcp_minipatch_find(mpDev, target.mpDev, nLevel, n, vSrc.data(), vStart.data(), nRange, pos.data(), found.data(), ssd.data()));
    std::vector<PatchMatch> out(n);
    for (int i = 0; i < n; ++i) out[i] = { pos[i], found[i] != 0, ssd[i] };
    return out;
  }

  // ---- the per-point part of Tracker::SearchForPoints (src/Tracker.cc:1299-1377) against this (the current) frame
  std::vector<mcp_td_out> SearchForPoints(const mcp_camera& cam, const double base_from_world[12], const double cam_from_base[12],
                                          const std::vector<mcp_td_in>& vTD, int nRange, int nSubPixIts, bool bExhaustive = false) {
    std::vector<mcp_td_out> out(vTD.size() + 1);
    check(mcp_track_search(mpDev, &cam, base_from_world, cam_from_base, (int)vTD.size(), vTD.data(), nRange, nSubPixIts, bExhaustive, out.data()));
    out.resize(vTD.size());
    return out;
  }

  mcp_kf* handle() { return mpDev; }

  // ---- MapMakerServerBase::AddStereoMapPoints of this (source) KeyFrame at one level in one submission (mcp_stereo_points,
  // src/MapMakerServerBase.cc:452-496): the candidates vCandidates of the level against the ordered targets
  struct StereoTarget { KeyFrame* pKF; mcp_camera cam; std::array<double, 12> cam_from_world; double one_pixel_angle; };
  struct StereoResult {
    std::vector<mcp_stereo_point> vPoints;   // creation order (target-major, candidate ascending)
    std::vector<uint8_t> vKeep;              // vCandidates as the reference leaves it (thinned before the last target)
    std::vector<uint8_t> vOutcome;           // targets x candidates, MCP_STEREO_*
  };
  StereoResult AddStereoPoints(const mcp_camera& cam, const double cam_from_world[12], int nLevel, const std::vector<mcp_int2>& vCandidates,
                               const std::vector<mcp_stereo_meas>& vMeasurements, const std::vector<StereoTarget>& vTargets, int nLimit) {
    std::vector<mcp_stereo_target> t(vTargets.size() + 1);
    for (size_t j = 0; j < vTargets.size(); ++j) {
      t[j].kf = vTargets[j].pKF->mpDev; t[j].cam = &vTargets[j].cam; t[j].one_pixel_angle = vTargets[j].one_pixel_angle;
      for (int k = 0; k < 12; ++k) t[j].cam_from_world[k] = vTargets[j].cam_from_world[k];
    }
    const int n = (int)vCandidates.size();
    StereoResult r;
    r.vPoints.resize(n + 1); r.vKeep.resize(n + 1); r.vOutcome.resize(vTargets.size()*n + 1);
    const int made = mcp_stereo_points(mpDev, &cam, cam_from_world, nLevel, n, vCandidates.data(), (int)vMeasurements.size(), vMeasurements.data(),
                                       (int)vTargets.size(), t.data(), nLimit, n, r.vPoints.data(), r.vKeep.data(), r.vOutcome.data());
    check(made);
    r.vPoints.resize(made); r.vKeep.resize(n); r.vOutcome.resize(vTargets.size()*n);
    return r;
  }

  // ---- the cameras of a frame in one submission (the per-camera loops of Tracker::TrackFrame, src/Tracker.cc:303-318, and of
  // Tracker::TrackMap, :985-1030): results equal the per-camera calls bit for bit
  /// MakeKeyFrame_Lite on every KeyFrame of `kfs` (<= MCP_MAX_FRAME_CAMS, one device); on_device: `ims` are device pointers
  static void MakeKeyFrameLiteBatch(const std::vector<KeyFrame*>& kfs, const std::vector<const uint8_t*>& ims, const std::vector<int>& strides,
                                    bool on_device = false, const std::vector<const uint8_t* const*>* masks = nullptr) {
    std::vector<mcp_kf*> h; for (KeyFrame* k : kfs) h.push_back(k->mpDev);
    check(mcp_kf_make_lite_batch((int)h.size(), h.data(), ims.data(), strides.data(), on_device ? 1 : 0, masks ? masks->data() : nullptr));
  }
  /// SearchForPoints of every camera against its KeyFrame in one launch; cams_from_base: 12 doubles per camera
  static std::vector<std::vector<mcp_td_out>> SearchForPointsBatch(const std::vector<KeyFrame*>& kfs, const std::vector<mcp_camera>& cams,
                                                                    const double base_from_world[12], const std::vector<double>& cams_from_base,
                                                                    const std::vector<std::vector<mcp_td_in>>& vTD, int nRange, int nSubPixIts,
                                                                    bool bExhaustive = false) {
    const int nc = (int)kfs.size();
    std::vector<mcp_kf*> h; std::vector<int> n; std::vector<const mcp_td_in*> in; std::vector<mcp_td_out*> op;
    std::vector<std::vector<mcp_td_out>> out(nc);
    for (int c = 0; c < nc; ++c) { h.push_back(kfs[c]->mpDev); n.push_back((int)vTD[c].size()); in.push_back(vTD[c].data()); out[c].resize(vTD[c].size() + 1); op.push_back(out[c].data()); }
    check(mcp_track_search_batch(nc, h.data(), cams.data(), base_from_world, cams_from_base.data(), n.data(), in.data(), nRange, nSubPixIts, bExhaustive, op.data()));
    for (int c = 0; c < nc; ++c) out[c].resize(vTD[c].size());
    return out;
  }

 private:
  static void check(int rc) { if (rc < 0) throw std::runtime_error(mcp_last_error()); }
  mcp_kf* mpDev = nullptr;
};

/// The keyframes' lists of BundleAdjusterMulti::AdjustAndUpdate's last step (RefreshSceneDepthRobust, src/KeyFrame.cc:547-645) and the chains of
/// the write-back: keyframe j's CamFromWorld is the chain kf_chains[j*chain_stride .. + kf_chain_len[j]) of the bundle ({MKF id, camera id} /
/// {KF id}); its measured, non-bad points are the table rows seg_rows[seg_start[j] .. seg_start[j+1]) with their inlier ratios seg_weights.
/// src_chains (empty, or chain_stride ints per point) / src_chain_len: the chain RefreshPixelVectors uses, length 0 = the point's own chain.
struct WriteBackLists {
  int chain_stride = 2;
  std::vector<int> src_chains, src_chain_len;
  std::vector<int> kf_chains, kf_chain_len;
  std::vector<int> seg_start, seg_rows;             // seg_start: keyframes + 1 entries (or a single 0 / empty: no keyframes)
  std::vector<double> seg_weights;
};
struct WriteBackResult {
  std::vector<double> world_pos, pixel_right_w, pixel_down_w;      // 3 per point: MapPoint::mv3WorldPos, mv3PixelRight_W, mv3PixelDown_W
  std::vector<double> kf_cam_from_world;                           // 12 per keyframe: KeyFrame::mse3CamFromWorld
  std::vector<mcp_scene_depth> depth;                              // per keyframe: mdSceneDepthMean / mdSceneDepthSigma where refreshed == 1
  std::vector<double> seg_depths;
};

/// What MapMakerServerBase::ReFind_Common decided for a list of (row, target) pairs (mcp_map_refind): a verdict per pair (MCP_REFIND_*), the
/// Measurements of the FOUND pairs in ascending pair index, the counts per verdict.  bKeepInPlace: vMeas stays empty and `view` points at the
/// n_meas records in the library's pinned block, valid until the next ReFindPairs on the table.
struct ReFindResult {
  std::vector<uint8_t> verdict;
  std::vector<mcp_refind_meas> vMeas;
  const mcp_refind_meas* view = nullptr;
  int n_meas = 0;
  int counts[6] = {0, 0, 0, 0, 0, 0};
};

/// The map points Tracker::FindPVS reads (src/Tracker.cc:662-723), resident on one device: row = the caller's point index.
class MapPointTable {
 public:
  explicit MapPointTable(int device = -1) {
    mpDev = mcp_map_points_create(device);
    if (!mpDev) throw std::runtime_error(std::string("MapPointTable: ") + mcp_last_error());
  }
  ~MapPointTable() { mcp_map_points_destroy(mpDev); }
  MapPointTable(const MapPointTable&) = delete;
  MapPointTable& operator=(const MapPointTable&) = delete;

  int Rows() const { return mcp_map_points_rows(mpDev); }
  /// rows first .. first+n-1 (SoA: 3 doubles per point in each vector; usable = !mbBad && mbOptimized)
  void Set(int first, const std::vector<double>& vWorldPos, const std::vector<double>& vPixelRight, const std::vector<double>& vPixelDown,
           const std::vector<uint8_t>& vUsable) {
    const int n = (int)vUsable.size();
    sizes(n, vWorldPos, vPixelRight, vPixelDown);
    check(mcp_map_points_set(mpDev, first, n, vWorldPos.data(), vPixelRight.data(), vPixelDown.data(), vUsable.data()));
  }
  /// the size becomes nRows: rows past it are dropped (they come back unusable if the table grows again)
  void Resize(int nRows) { check(mcp_map_points_resize(mpDev, nRows)); }
  /// rows vIds (distinct) -- the points the map maker moved, flagged or added
  void Update(const std::vector<int>& vIds, const std::vector<double>& vWorldPos, const std::vector<double>& vPixelRight,
              const std::vector<double>& vPixelDown, const std::vector<uint8_t>& vUsable) {
    const int n = (int)vIds.size();
    if ((int)vUsable.size() != n) throw std::invalid_argument("MapPointTable::Update: array sizes");
    sizes(n, vWorldPos, vPixelRight, vPixelDown);
    check(mcp_map_points_update(mpDev, n, vIds.data(), vWorldPos.data(), vPixelRight.data(), vPixelDown.data(), vUsable.data()));
  }
  /// Tracker::FindPVS for every camera of a frame in one call: result[c][level] = that camera's entries of that level, rows ascending
  /// (copied out of the library's block).  vCaps empty = the table's rows per camera.
  std::vector<std::array<std::vector<mcp_pvs_entry>, MCP_LEVELS>> FindPVS(const std::vector<KeyFrame*>& vTargets, const std::vector<mcp_camera>& vCams,
                                                                         const double base_from_world[12], const std::vector<double>& vCamFromBase,
                                                                         std::vector<int> vCaps = {}) {
    const int nc = (int)vTargets.size();
    if ((int)vCams.size() != nc || (int)vCamFromBase.size() != 12*nc) throw std::invalid_argument("MapPointTable::FindPVS: array sizes");
    if (vCaps.empty()) vCaps.assign(nc, Rows());
    std::vector<mcp_kf*> h(nc);
    for (int c = 0; c < nc; ++c) h[c] = vTargets[c]->handle();
    std::vector<int> counts(nc*MCP_LEVELS);
    check(mcp_track_find_pvs(mpDev, nc, h.data(), vCams.data(), base_from_world, vCamFromBase.data(), vCaps.data(), nullptr, counts.data()));
    std::vector<std::array<std::vector<mcp_pvs_entry>, MCP_LEVELS>> out(nc);
    for (int c = 0; c < nc; ++c)
      for (int l = 0; l < MCP_LEVELS; ++l) {
        int n = 0;
        const mcp_pvs_entry* e = mcp_track_find_pvs_view(mpDev, c, l, &n);
        if (n != counts[c*MCP_LEVELS + l]) throw std::runtime_error(mcp_last_error());
        out[c][l].assign(e, e + n);
      }
    return out;
  }
  /// rows first .. first+n-1: the patch source of each MapPoint (mpPatchSourceKF, nullptr = none; mnSourceLevel; mirCenter as x, y pairs;
  /// mbFixed) and its identity key (a changed key gives the row finders that have seen nothing)
  void SetSource(int first, const std::vector<int>& vKeys, const std::vector<KeyFrame*>& vSources, const std::vector<int>& vLevels,
                 const std::vector<int>& vCenters, const std::vector<uint8_t>& vFixed) {
    std::vector<mcp_kf*> h = sources((int)vKeys.size(), vSources, vLevels, vCenters, vFixed);
    check(mcp_map_points_set_source(mpDev, first, (int)vKeys.size(), vKeys.data(), h.data(), vLevels.data(), vCenters.data(), vFixed.data()));
  }
  void UpdateSource(const std::vector<int>& vIds, const std::vector<int>& vKeys, const std::vector<KeyFrame*>& vSources, const std::vector<int>& vLevels,
                    const std::vector<int>& vCenters, const std::vector<uint8_t>& vFixed) {
    if (vIds.size() != vKeys.size()) throw std::invalid_argument("MapPointTable::UpdateSource: array sizes");
    std::vector<mcp_kf*> h = sources((int)vKeys.size(), vSources, vLevels, vCenters, vFixed);
    check(mcp_map_points_update_source(mpDev, (int)vIds.size(), vIds.data(), vKeys.data(), h.data(), vLevels.data(), vCenters.data(), vFixed.data()));
  }
  /// the persistent finders of camera nCam for rows first .. first+n-1
  std::vector<mcp_pf_state> States(int nCam, int first, int n) const {
    std::vector<mcp_pf_state> out(n);
    check(mcp_map_points_get_states(mpDev, nCam, first, n, out.data()));
    return out;
  }
  /// Tracker::TrackMap of a frame in one call (mcp_track_map): vImages empty = the pyramids are current; base_from_world in / out.
  /// Returns the items of every camera ([C, T, R], copied out of the library's block) and fills *pResult.
  std::vector<std::vector<mcp_track_map_item>> TrackMap(const std::vector<KeyFrame*>& vTargets, const std::vector<const uint8_t*>& vImages,
                                                        const std::vector<int>& vStrides, bool bImagesOnDevice, const std::vector<mcp_camera>& vCams,
                                                        double base_from_world[12], const std::vector<double>& vCamFromBase,
                                                        const mcp_track_map_params& params, mcp_track_map_result* pResult) {
    const Frame f("TrackMap", vTargets, vImages, vStrides, vCams, nullptr, vCamFromBase);
    mcp_track_map_result r;
    check(mcp_track_map(mpDev, f.nc, f.h.data(), f.imgs, f.strides, bImagesOnDevice ? 1 : 0, nullptr, vCams.data(), base_from_world, vCamFromBase.data(), &params, &r));
    if (pResult) *pResult = r;
    std::vector<std::vector<mcp_track_map_item>> out(f.nc);
    for (int c = 0; c < f.nc; ++c) {
      int n = 0;
      const mcp_track_map_item* it = mcp_track_map_view(mpDev, c, &n);
      out[c].assign(it, it + n);
    }
    return out;
  }
  /// mnMEstimatorInlierCount / mnMEstimatorOutlierCount of rows first .. first+n-1 / of rows vIds (inlier >= 1, outlier >= 0).  A row never
  /// named reads (1, 0).  A key change in SetSource leaves the counts alone: whoever puts a new point into a row sets them.
  void SetCounts(int first, const std::vector<int>& vInlier, const std::vector<int>& vOutlier) {
    if (vInlier.size() != vOutlier.size()) throw std::invalid_argument("MapPointTable::SetCounts: array sizes");
    check(mcp_map_points_set_counts(mpDev, first, (int)vInlier.size(), vInlier.data(), vOutlier.data()));
  }
  void UpdateCounts(const std::vector<int>& vIds, const std::vector<int>& vInlier, const std::vector<int>& vOutlier) {
    if (vInlier.size() != vIds.size() || vOutlier.size() != vIds.size()) throw std::invalid_argument("MapPointTable::UpdateCounts: array sizes");
    check(mcp_map_points_update_counts(mpDev, (int)vIds.size(), vIds.data(), vInlier.data(), vOutlier.data()));
  }
  void GetCounts(int first, int n, std::vector<int>& vInlier, std::vector<int>& vOutlier) const {
    vInlier.assign((size_t)n, 0); vOutlier.assign((size_t)n, 0);
    check(mcp_map_points_get_counts(mpDev, first, n, vInlier.data(), vOutlier.data()));
  }
  /// TrackMap with its bookkeeping (mcp_track_map_record): the marks go into the count column, the level counters, quality, scene depth and
  /// cam_from_world of every camera into *pRecord.  Notes (one per item) and measurements (one per found item) are read in place through
  /// Notes() / Measurements() until the next track / PVS call; with recParams.want_items the items through mcp_track_map_view as well.
  void TrackMapRecord(const std::vector<KeyFrame*>& vTargets, const std::vector<const uint8_t*>& vImages, const std::vector<int>& vStrides, bool bImagesOnDevice,
                      const std::vector<mcp_camera>& vCams, double base_from_world[12], const std::vector<double>& vCamFromBase, const mcp_track_map_params& params,
                      const mcp_track_record_params& recParams, mcp_track_map_result* pResult, mcp_track_record* pRecord) {
    const Frame f("TrackMapRecord", vTargets, vImages, vStrides, vCams, nullptr, vCamFromBase, pRecord != nullptr);
    mcp_track_map_result r;
    check(mcp_track_map_record(mpDev, f.nc, f.h.data(), f.imgs, f.strides, bImagesOnDevice ? 1 : 0, nullptr, vCams.data(), base_from_world, vCamFromBase.data(), &params, &r,
                               &recParams, pRecord));
    if (pResult) *pResult = r;
  }
  /// Tracker::TrackFrame's tracking branch (src/Tracker.cc:431-434) in one call: ApplyMotionModel with the SBI rotation estimate, TrackMap with
  /// its bookkeeping, UpdateMotionModel (mcp_track_frame_motion).  base_from_world: last frame's pose in, the refined pose out; vCamsSBI: the
  /// 40x30 cameras (mmCameraModelsSBI).  Notes(), Measurements() and the item / PVS views are TrackMapRecord's.
  void TrackFrameMotion(const std::vector<KeyFrame*>& vTargets, const std::vector<const uint8_t*>& vImages, const std::vector<int>& vStrides, bool bImagesOnDevice,
                        const std::vector<mcp_camera>& vCams, const std::vector<mcp_camera>& vCamsSBI, double base_from_world[12], const std::vector<double>& vCamFromBase,
                        const mcp_track_map_params& params, const mcp_track_record_params& recParams, const mcp_track_motion_params& motionParams,
                        mcp_track_map_result* pResult, mcp_track_record* pRecord, mcp_track_motion* pMotion) {
    const Frame f("TrackFrameMotion", vTargets, vImages, vStrides, vCams, &vCamsSBI, vCamFromBase, pRecord && pMotion);
    mcp_track_map_result r;
    check(mcp_track_frame_motion(mpDev, f.nc, f.h.data(), f.imgs, f.strides, bImagesOnDevice ? 1 : 0, nullptr, vCams.data(), vCamsSBI.data(), base_from_world, vCamFromBase.data(),
                                 &params, &r, &recParams, pRecord, &motionParams, pMotion));
    if (pResult) *pResult = r;
  }
  /// Tracker::TrackFrame's lost branch (src/Tracker.cc:493-502, 526-552; src/Relocaliser.cc:61-120) in one call: the relocaliser over the
  /// candidate keyframes, the recovered pose, TrackMap with its bookkeeping (mcp_track_frame_recover).  vCandidates: the map's keyframes
  /// (nullptr: skipped), vCandCams: each one's camera index among vTargets, vCandPoses: each one's CamFromWorld, 12 doubles per entry;
  /// motionParams.apply must be 0.  pRecover->recovered says whether TrackMap ran; pScores (nullptr: not wanted) gets one ZMSSD per entry.
  void TrackFrameRecover(const std::vector<KeyFrame*>& vTargets, const std::vector<const uint8_t*>& vImages, const std::vector<int>& vStrides, bool bImagesOnDevice,
                         const std::vector<mcp_camera>& vCams, const std::vector<mcp_camera>& vCamsSBI, double base_from_world[12], const std::vector<double>& vCamFromBase,
                         const mcp_track_map_params& params, const mcp_track_record_params& recParams, const mcp_track_motion_params& motionParams,
                         const std::vector<KeyFrame*>& vCandidates, const std::vector<int>& vCandCams, const std::vector<double>& vCandPoses,
                         const mcp_track_recover_params& recoverParams, mcp_track_map_result* pResult, mcp_track_record* pRecord, mcp_track_motion* pMotion,
                         mcp_track_recover* pRecover, std::vector<double>* pScores = nullptr) {
    const int nk = (int)vCandidates.size();
    const Frame f("TrackFrameRecover", vTargets, vImages, vStrides, vCams, &vCamsSBI, vCamFromBase,
                  (int)vCandCams.size() == nk && (int)vCandPoses.size() == 12*nk && pRecord && pMotion && pRecover);
    std::vector<mcp_kf*> hk(nk > 0 ? nk : 1);
    for (int i = 0; i < nk; ++i) hk[i] = vCandidates[i] ? vCandidates[i]->handle() : nullptr;
    if (pScores) pScores->assign(nk, 0.0);
    mcp_track_map_result r;
    check(mcp_track_frame_recover(mpDev, f.nc, f.h.data(), f.imgs, f.strides, bImagesOnDevice ? 1 : 0, nullptr, vCams.data(), vCamsSBI.data(), base_from_world, vCamFromBase.data(),
                                  &params, &r, &recParams, pRecord, &motionParams, pMotion, nk, hk.data(), nk ? vCandCams.data() : nullptr, nk ? vCandPoses.data() : nullptr,
                                  &recoverParams, pRecover, pScores && nk ? pScores->data() : nullptr));
    if (pResult) *pResult = r;
  }
  /// the two poses of a recovery on the host (mcp_track_recover_pose_host; needs no device): cam_pose = SE3fromSE2(se2) * cam_from_world_best,
  /// base_from_world = cam_from_base^-1 * cam_pose
  static void RecoverPoseHost(const double se2[6], const mcp_camera& camSBI, const double cam_from_world_best[12], const double cam_from_base[12], double cam_pose[12],
                              double base_from_world[12]) {
    check(mcp_track_recover_pose_host(se2, &camSBI, cam_from_world_best, cam_from_base, cam_pose, base_from_world));
  }
  /// Tracker::Reset: every camera index forgets its SmallBlurryImages
  void MotionReset() { check(mcp_track_motion_reset(mpDev)); }
  /// mm6PoseCovariance (src/Tracker.cc:1498-1502) from the one-call frames: with the switch on TrackMap / TrackMapRecord / TrackFrameMotion /
  /// TrackFrameRecover append its two launches behind the fine iterations; PoseCovLast hands out the record of the last such call
  void PoseCovEnable(bool bOn) { check(mcp_track_pose_cov_enable(mpDev, bOn ? 1 : 0)); }
  mcp_track_pose_cov_record PoseCovLast() const { mcp_track_pose_cov_record r; check(mcp_track_pose_cov_last(mpDev, &r)); return r; }
  /// the same two kernels on caller arrays (nMaxWorkgroups = 0: the library's choice), and the same source on the host (no device needed)
  static mcp_track_pose_cov_record PoseCov(const std::vector<mcp_pose_point>& vPts, const std::vector<double>& vWeights, const std::vector<double>& vCamFromBase,
                                           const double refined[12], const double mu_last[6], int nMaxWorkgroups = 0) {
    if (vPts.size() != vWeights.size() || vCamFromBase.size() % 12 != 0) throw std::invalid_argument("PoseCov: one weight per record, 12 doubles per camera");
    mcp_track_pose_cov_record r;
    check(mcp_track_pose_cov((int)vPts.size(), vPts.data(), vWeights.data(), (int)(vCamFromBase.size()/12), vCamFromBase.data(), refined, mu_last, nMaxWorkgroups, &r));
    return r;
  }
  static mcp_track_pose_cov_record PoseCovHost(const std::vector<mcp_pose_point>& vPts, const std::vector<double>& vWeights, const std::vector<double>& vCamFromBase,
                                               const double refined[12], const double mu_last[6]) {
    if (vPts.size() != vWeights.size() || vCamFromBase.size() % 12 != 0) throw std::invalid_argument("PoseCovHost: one weight per record, 12 doubles per camera");
    mcp_track_pose_cov_record r;
    check(mcp_track_pose_cov_host((int)vPts.size(), vPts.data(), vWeights.data(), (int)(vCamFromBase.size()/12), vCamFromBase.data(), refined, mu_last, &r));
    return r;
  }
  /// the tracker's SBI of camera index nCam (nWhich 0: this frame's, 1: last frame's): 1200 bytes, 1200 floats, 2400 floats; nullptr: not wanted
  void MotionSBI(int nCam, int nWhich, uint8_t* pSmall, float* pTemplate, float* pJacs) const { check(mcp_track_motion_get_sbi(mpDev, nCam, nWhich, pSmall, pTemplate, pJacs)); }
  /// nullptr with *pnCount == 0: the camera's list is empty -- or the last track / PVS call was no TrackMapRecord with that camera (mcp_last_error())
  const mcp_track_note* Notes(int nCam, int* pnCount) const { return mcp_track_map_notes_view(mpDev, nCam, pnCount); }
  const mcp_track_meas* Measurements(int nCam, int* pnCount) const { return mcp_track_map_meas_view(mpDev, nCam, pnCount); }
  // ---- BundleAdjusterMulti::AdjustAndUpdate (src/BundleAdjusterMulti.cc:286-334) over the table: mcp_ba_write_back
  /// patch rays (mv3Center_NC, mv3OneRightFromCenter_NC, mv3OneDownFromCenter_NC; 3 doubles per point) of rows first .. / of rows vIds
  void SetRays(int first, const std::vector<double>& vCenter, const std::vector<double>& vOneRight, const std::vector<double>& vOneDown) {
    const int n = (int)vCenter.size()/3;
    sizes(n, vCenter, vOneRight, vOneDown);
    check(mcp_map_points_set_rays(mpDev, first, n, vCenter.data(), vOneRight.data(), vOneDown.data()));
  }
  void UpdateRays(const std::vector<int>& vIds, const std::vector<double>& vCenter, const std::vector<double>& vOneRight, const std::vector<double>& vOneDown) {
    sizes((int)vIds.size(), vCenter, vOneRight, vOneDown);
    check(mcp_map_points_update_rays(mpDev, (int)vIds.size(), vIds.data(), vCenter.data(), vOneRight.data(), vOneDown.data()));
  }
  /// rows first .. first+n-1 read back
  void Get(int first, int n, std::vector<double>& vWorldPos, std::vector<double>& vPixelRight, std::vector<double>& vPixelDown, std::vector<uint8_t>& vUsable) const {
    vWorldPos.assign(3*(size_t)n, 0.0); vPixelRight.assign(3*(size_t)n, 0.0); vPixelDown.assign(3*(size_t)n, 0.0); vUsable.assign((size_t)n, 0);
    check(mcp_map_points_get(mpDev, first, n, vWorldPos.data(), vPixelRight.data(), vPixelDown.data(), vUsable.data()));
  }
  /// KeyFrame::RefreshSceneDepthRobust of keyframes with explicit poses (12 doubles each) over the table (mcp_scene_depth_robust)
  std::vector<mcp_scene_depth> SceneDepthRobust(const std::vector<double>& vCamFromWorld, const std::vector<int>& vSegStart, const std::vector<int>& vSegRows,
                                                const std::vector<double>& vSegWeights, std::vector<double>* pvDepths = nullptr) {
    const int nkf = vSegStart.empty() ? 0 : (int)vSegStart.size() - 1;
    if ((int)vCamFromWorld.size() != 12*nkf || vSegRows.size() != vSegWeights.size() || (nkf && vSegStart.back() != (int)vSegRows.size()))
      throw std::invalid_argument("MapPointTable::SceneDepthRobust: array sizes");
    std::vector<mcp_scene_depth> out((size_t)nkf);
    if (pvDepths) pvDepths->assign(vSegRows.size(), 0.0);
    check(mcp_scene_depth_robust(mpDev, nkf, vCamFromWorld.data(), vSegStart.data(), vSegRows.data(), vSegWeights.data(), out.data(),
                                 pvDepths ? pvDepths->data() : nullptr));
    return out;
  }
  /// the whole write-back of an adjustment: vPointIds[k] (bundle point id) belongs to row vRows[k]
  WriteBackResult WriteBack(ChainBundle& bundle, const std::vector<int>& vPointIds, const std::vector<int>& vRows, const WriteBackLists& lists) {
    const int n = (int)vPointIds.size(), nkf = (int)lists.kf_chain_len.size();
    if ((int)vRows.size() != n || (!lists.src_chains.empty() && ((int)lists.src_chains.size() != n*lists.chain_stride || (int)lists.src_chain_len.size() != n)) ||
        (int)lists.kf_chains.size() != nkf*lists.chain_stride || lists.seg_rows.size() != lists.seg_weights.size() ||
        (nkf && ((int)lists.seg_start.size() != nkf + 1 || lists.seg_start.back() != (int)lists.seg_rows.size())))
      throw std::invalid_argument("MapPointTable::WriteBack: array sizes");
    WriteBackResult r;
    r.world_pos.resize(3*(size_t)n + 1); r.pixel_right_w.resize(3*(size_t)n + 1); r.pixel_down_w.resize(3*(size_t)n + 1);
    r.kf_cam_from_world.resize(12*(size_t)nkf + 1); r.depth.resize((size_t)nkf + 1); r.seg_depths.resize(lists.seg_rows.size() + 1);
    check(mcp_ba_write_back(bundle.handle(), mpDev, n, vPointIds.data(), vRows.data(), lists.src_chains.empty() ? nullptr : lists.src_chains.data(),
                            lists.chain_stride, lists.src_chains.empty() ? nullptr : lists.src_chain_len.data(), r.world_pos.data(), r.pixel_right_w.data(),
                            r.pixel_down_w.data(), nkf, lists.kf_chains.data(), lists.kf_chain_len.data(), lists.seg_start.data(), lists.seg_rows.data(),
                            lists.seg_weights.data(), r.kf_cam_from_world.data(), r.depth.data(), r.seg_depths.data()));
    r.world_pos.resize(3*(size_t)n); r.pixel_right_w.resize(3*(size_t)n); r.pixel_down_w.resize(3*(size_t)n);
    r.kf_cam_from_world.resize(12*(size_t)nkf); r.depth.resize((size_t)nkf); r.seg_depths.resize(lists.seg_rows.size());
    return r;
  }
  // ---- MapMakerServerBase::ReFind_Common (src/MapMakerServerBase.cc:921-1002) over the table: mcp_map_refind
  /// vPairs: (row, target index) per pair, the pairs that survive the caller's early-outs (:925-937), processed as given.  bOneFinderPerRow:
  /// runs of one row share a finder (ReFindNewlyMade); pFinder: the map maker's static finder, in / out (nullptr: a fresh one).
  ReFindResult ReFindPairs(const std::vector<mcp_refind_target>& vTargets, const std::vector<int>& vPairs, bool bOneFinderPerRow,
                           mcp_pf_state* pFinder = nullptr, bool bKeepInPlace = false) {
    if (vPairs.size() % 2) throw std::invalid_argument("MapPointTable::ReFindPairs: array sizes");
    const int n = (int)(vPairs.size()/2);
    ReFindResult r;
    r.verdict.resize((size_t)n + 1);
    if (!bKeepInPlace) r.vMeas.resize((size_t)n + 1);
    mcp_refind_result res;
    check(mcp_map_refind(mpDev, (int)vTargets.size(), vTargets.data(), n, vPairs.data(), bOneFinderPerRow ? 1 : 0, pFinder, r.verdict.data(), n,
                         bKeepInPlace ? nullptr : r.vMeas.data(), &res));
    r.verdict.resize((size_t)n);
    r.n_meas = res.n_meas;
    for (int k = 0; k < 6; ++k) r.counts[k] = res.counts[k];
    if (bKeepInPlace) { int m = 0; r.view = mcp_map_refind_view(mpDev, &m); if (m != res.n_meas) throw std::runtime_error(mcp_last_error()); }
    else r.vMeas.resize((size_t)res.n_meas);
    return r;
  }
  mcp_map_points* Handle() const { return mpDev; }

 private:
  static void check(int rc) { if (rc < 0) throw std::runtime_error(mcp_last_error()); }
  static std::vector<mcp_kf*> sources(int n, const std::vector<KeyFrame*>& vSources, const std::vector<int>& vLevels, const std::vector<int>& vCenters,
                                      const std::vector<uint8_t>& vFixed) {
    if ((int)vSources.size() != n || (int)vLevels.size() != n || (int)vCenters.size() != 2*n || (int)vFixed.size() != n)
      throw std::invalid_argument("MapPointTable: source array sizes");
    std::vector<mcp_kf*> h(n);
    for (int k = 0; k < n; ++k) h[k] = vSources[k] ? vSources[k]->handle() : nullptr;
    return h;
  }
  // what the one-call frames share: the size checks (who: the method's name in the refusal; bOwn: the method's own conditions hold), the
  // target handles, the image and stride pointers (nullptr: the pyramids are current)
  struct Frame {
    int nc; std::vector<mcp_kf*> h; const uint8_t* const* imgs; const int* strides;
    Frame(const char* who, const std::vector<KeyFrame*>& vTargets, const std::vector<const uint8_t*>& vImages, const std::vector<int>& vStrides,
          const std::vector<mcp_camera>& vCams, const std::vector<mcp_camera>* pvCamsSBI, const std::vector<double>& vCamFromBase, bool bOwn = true)
        : nc((int)vTargets.size()), h(vTargets.size()), imgs(vImages.empty() ? nullptr : vImages.data()), strides(vImages.empty() ? nullptr : vStrides.data()) {
      if ((int)vCams.size() != nc || (pvCamsSBI && (int)pvCamsSBI->size() != nc) || (int)vCamFromBase.size() != 12*nc ||
          (!vImages.empty() && ((int)vImages.size() != nc || (int)vStrides.size() != nc)) || !bOwn)
        throw std::invalid_argument(std::string("MapPointTable::") + who + ": array sizes");
      for (int c = 0; c < nc; ++c) h[c] = vTargets[c]->handle();
    }
  };
  static void sizes(int n, const std::vector<double>& a, const std::vector<double>& b, const std::vector<double>& c) {
    if ((int)a.size() != 3*n || (int)b.size() != 3*n || (int)c.size() != 3*n) throw std::invalid_argument("MapPointTable: array sizes");
  }
  mcp_map_points* mpDev = nullptr;
};

/// Tracker::CalcPoseUpdate (src/Tracker.cc:1386-1512): mu, Tukey sigma^2; weights (0 = outlier) if asked for
inline std::pair<std::array<double, 6>, double> CalcPoseUpdate(const std::vector<uint8_t>& vFound, const std::vector<double>& vFoundPos /*2n*/,
                                                               const std::vector<double>& vImagePos /*2n*/, const std::vector<double>& vSqrtInvNoise /*n*/,
                                                               const std::vector<double>& vJacobian /*12n*/, double dOverrideSigma = -1.0,
                                                               std::vector<double>* pvWeights = nullptr) {
  const int n = (int)vFound.size();
  if ((int)vFoundPos.size() != 2*n || (int)vImagePos.size() != 2*n || (int)vSqrtInvNoise.size() != n || (int)vJacobian.size() != 12*n)
    throw std::invalid_argument("CalcPoseUpdate: array sizes");
  std::array<double, 6> mu{}; double sigma = 0;
  if (pvWeights) pvWeights->assign(n, 0.0);
  if (mcp_track_pose_update(n, vFound.data(), vFoundPos.data(), vImagePos.data(), vSqrtInvNoise.data(), vJacobian.data(), dOverrideSigma,
                            mu.data(), pvWeights ? pvWeights->data() : nullptr, &sigma) < 0) throw std::runtime_error(mcp_last_error());
  return { mu, sigma };
}

/// The ten pose iterations of Tracker::TrackMap in one launch (src/Tracker.cc:775-838, 1038-1075); base_from_world is updated
inline std::array<double, 6> TrackMapPoseIterations(std::vector<mcp_pose_point>& vPoints, const std::vector<mcp_camera>& vCams,
                                                    const std::vector<double>& vCamFromBase /*12 per camera*/, double base_from_world[12],
                                                    const std::vector<uint8_t>& vNonlinear, const std::vector<double>& vOverrideSigma,
                                                    std::vector<double>* pvWeightsLast = nullptr) {
  if (vNonlinear.size() != vOverrideSigma.size() || vCamFromBase.size() != 12*vCams.size()) throw std::invalid_argument("TrackMapPoseIterations: array sizes");
  std::array<double, 6> mu{};
  if (pvWeightsLast) pvWeightsLast->assign(vPoints.size(), 0.0);
  if (mcp_track_pose_refine((int)vPoints.size(), vPoints.data(), (int)vCams.size(), vCams.data(), vCamFromBase.data(), base_from_world,
                            (int)vNonlinear.size(), vNonlinear.data(), vOverrideSigma.data(), mu.data(),
                            pvWeightsLast ? pvWeightsLast->data() : nullptr) < 0) throw std::runtime_error(mcp_last_error());
  return mu;
}

}  // namespace mcptam_hip
