/*
 * mcp_img.h -- C ABI of the MI355X (gfx950) KeyFrame / Tracker image path.
 *
 * Second drop-in boundary of the MCPTAM back end (SURVEY.md 8(b) "Image/track seam"): the
 * inner loops of KeyFrame::MakeKeyFrame_Lite / MakeKeyFrame_Rest
 * (/root/reference/src/KeyFrame.cc:145-360, 363-450), ShiTomasi.cc, MiniPatch.cc, PatchFinder.cc
 * and the per-point part of Tracker::SearchForPoints / CalcPoseUpdate
 * (src/Tracker.cc:1299-1377, 1386-1512; include/mcptam/TrackerData.h:102-185).
 * Control flow (which points to search, shuffles, budgets) stays in the reference's Tracker /
 * MapMaker; they hand BATCHES to these entry points.
 *
 * A keyframe handle owns the 4-level pyramid, the FAST corner lists and the row look-up
 * tables ON THE DEVICE: source keyframes of map points stay resident so that template warps
 * (PatchFinder::MakeTemplateCoarseCont) gather from HBM, not over PCIe.
 * Integer results (pyramids, corner lists and order, LUTs, thresholds, ZMSSD / SSD scores,
 * coarse positions) are bit-exact against the CPU oracle; floating-point results follow the
 * reference's float/double mix.  No CPU fallback: every entry point fails (-1 / NULL, see
 * mcp_last_error()) when no gfx950 device is usable.
 */
#ifndef MCP_IMG_H
#define MCP_IMG_H

#include <stdint.h>
#include "mcp_ba.h"      /* mcp_camera, mcp_last_error */

#ifdef __cplusplus
extern "C" {
#endif

#define MCP_LEVELS 4            /* LEVELS, include/mcptam/KeyFrame.h:85 */
#define MCP_MIN_FAST_THRESH 5   /* KeyFrame.h:88 */
#define MCP_MAX_FAST_THRESH 30  /* KeyFrame.h:89 */

typedef struct mcp_kf mcp_kf;

typedef struct mcp_int2 { int x, y; } mcp_int2;

/* options of MakeKeyFrame_Lite that are statics / GVars in the reference */
typedef struct mcp_kf_params {
  int adaptive_thresh;        /* KeyFrame::sbAdaptiveThresh (default 1)                        */
  int glare_masking;          /* GVar GlareMasking (default 0, src/System.cc:121)              */
  int half_sample_pavgb;      /* 0: truncating 2x2 mean (libCVD generic halfSample);
                                 1: cascaded round-half-up averages (libCVD SSE2 byte path)    */
  int device;                 /* HIP device ordinal, -1 = current                              */
} mcp_kf_params;

/* KeyFrame + its Levels (include/mcptam/KeyFrame.h:93-150).  w,h = level-0 size. */
mcp_kf* mcp_kf_create(int w, int h, const mcp_kf_params* params);
void    mcp_kf_destroy(mcp_kf*);

/* KeyFrame::MakeKeyFrame_Lite(CVD::Image<byte>& im, bool, bool bGlareMasking)  KeyFrame.cc:145-360
 * img: level-0 image, row stride in bytes.  masks: NULL, or MCP_LEVELS pointers (each NULL or a
 * tightly packed mask of that level's size; a corner is kept only where mask == 255, :305). */
int mcp_kf_make_lite(mcp_kf*, const uint8_t* img, int stride, const uint8_t* const* masks);

/* The MakeKeyFrame_Lite loop over the cameras of a frame (Tracker::TrackFrame, src/Tracker.cc:303-318) as ONE submission:
 * uploads + three kernel launches for all levels of all cameras + one wait.  kfs: ncam distinct handles on one device that
 * share adaptive_thresh / half_sample_pavgb; imgs_on_device != 0: imgs[] are device pointers (a capture ring that already
 * lives in HBM), nothing crosses PCIe.  masks: NULL, or per camera NULL / MCP_LEVELS pointers as in mcp_kf_make_lite.
 * Results are those of ncam mcp_kf_make_lite calls, bit for bit. */
#define MCP_MAX_FRAME_CAMS 8
int mcp_kf_make_lite_batch(int ncam, mcp_kf* const* kfs, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                           const uint8_t* const* const* masks);

/* read-back of what MakeKeyFrame_Lite leaves in Level (image, vCorners, vCornerRowLUT, nFastThresh,
 * vFastFrequency) */
int mcp_kf_level_size(mcp_kf*, int level, int* w, int* h);
int mcp_kf_get_image(mcp_kf*, int level, uint8_t* out /* w*h, packed */);
int mcp_kf_num_corners(mcp_kf*, int level);
int mcp_kf_get_corners(mcp_kf*, int level, mcp_int2* out, int cap);
int mcp_kf_get_row_lut(mcp_kf*, int level, int* out /* h */);
int mcp_kf_fast_thresh(mcp_kf*, int level);
int mcp_kf_get_fast_frequency(mcp_kf*, int level, double* out /* MCP_MAX_FAST_THRESH+1 */);

/* frames held in the Level::imagePrev / vCornersPrev history (0..2, KeyFrame.h:147-148): every mcp_kf_make_lite on a handle
 * that already holds a frame pushes that frame (device-resident) before overwriting it, KeyFrame.cc:152-199 */
int mcp_kf_num_prev(mcp_kf*);

/* KeyFrame::MakeKeyFrame_Rest, candidate part                         KeyFrame.cc:363-450, 456-527
 * use_shi: ssCandidateType ("shi" = 1 / "fast" = 0); use_percent: ssCandidateCriterion;
 * top_fraction = sdCandidateTopFraction (0.8); thresh = sdCandidateThresh (70).
 * nonmax_score: score used by CVD::fast_nonmax -- 0: FAST-10 binary-search score,
 * 1: the classic ring SAD corner_score (libCVD vintage dependent).
 * When the handle holds history, the candidates are pruned by the back/forward MiniPatch stability test (:456-527). */
int mcp_kf_make_rest(mcp_kf*, int use_shi, int use_percent, double top_fraction, double thresh, int nonmax_score);
int mcp_kf_num_candidates(mcp_kf*, int level);
int mcp_kf_get_candidates(mcp_kf*, int level, mcp_int2* pos, double* score, int cap);

/* MiniPatch::SampleFromImage + FindPatch, batched                      MiniPatch.cc:34-122
 * For each i: 9x9 patch of `src` level `level` at src_pos[i], searched among the FAST corners of
 * `dst` level `level` inside +-range of dst_pos[i] (row LUT used).  out_pos / out_found per i. */
int mcp_minipatch_find(mcp_kf* src, mcp_kf* dst, int level, int n, const mcp_int2* src_pos,
                       const mcp_int2* dst_pos, int range, mcp_int2* out_pos, uint8_t* out_found, int* out_ssd);

/* The Gauss-Newton pose iterations of Tracker::TrackMap in one call (src/Tracker.cc:775-838, 1038-1075).  Per iteration i:
 * nonlinear[i] != 0 -> PoseUpdateStep (found points are re-projected unless i == 0, CalcJacobian), else PoseUpdateStepLinear
 * (LinearUpdate with the previous update); then CalcPoseUpdate with override_sigma[i] (<= 0: Tukey sigma^2 from the
 * median -- the caller applies the "no override up to iteration 5" rule) and BaseFromWorld <- exp(mu) BaseFromWorld.
 * Points of all cameras go in one array; image / cam_derivs are updated in place, weights_last (may be NULL) receives the
 * Tukey weights of the last iteration (0 = outlier, as bMarkOutliers counts them). */
typedef struct mcp_pose_point {
  double world_pos[3];
  double found_pos[2];
  double sqrt_inv_noise;
  double image[2];
  double cam_derivs[4];
  int    cam;
  int    found;
} mcp_pose_point;
int mcp_track_pose_refine(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cam_from_base /* ncam x 12 */,
                          double base_from_world[12], int n_iter, const uint8_t* nonlinear, const double* override_sigma,
                          double mu_last[6], double* weights_last);

/* The same pose iterations with the cameras spread over ranks (one camera per GPU, BASELINE config c5 / SURVEY.md 8(e)): every rank
 * passes the points of ITS camera(s) and the same BaseFromWorld; per iteration the ranks exchange the squared errors (exact global
 * Tukey median) and the 6x6 + 6 WLS accumulator through `allreduce` (SUM of doubles in place on a device buffer, the hook type of
 * mcp_ba.h; e.g. RCCL over xGMI), so that every rank applies the identical update.  cap >= the largest n of any rank.  world = 1
 * with allreduce = NULL runs the same kernels on one device. */
int mcp_track_pose_refine_sharded(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cam_from_base /* ncam x 12 */,
                                  double base_from_world[12], int n_iter, const uint8_t* nonlinear, const double* override_sigma,
                                  double mu_last[6], double* weights_last, mcp_allreduce_fn allreduce, void* user, int rank, int world, int cap);

/* ---- SmallBlurryImage / Relocaliser -------------------------------- src/SmallBlurryImage.cc:67-330, src/Relocaliser.cc:61-121
 * The 40x30 thumbnail of the frame the handle holds, its zero-mean Gaussian-blurred float template and gradient image
 * (MakeFromKF + MakeJacs) live on the device with the keyframe (KeyFrame::mpSBI).  blur = 2.5 in the reference. */
#define MCP_SBI_W 40
#define MCP_SBI_H 30
int mcp_kf_make_sbi(mcp_kf*, double blur);
int mcp_kf_get_sbi(mcp_kf*, uint8_t* small_img /*1200 or NULL*/, float* templ /*1200 or NULL*/, float* jacs /*2400 (gx,gy) or NULL*/);
/* Relocaliser::ScoreKFs: ZMSSD of cur against n candidate keyframes (NULL / SBI-less entries are skipped with a score of
 * DBL_MAX); *best = index of the first smallest score or -1. */
int mcp_sbi_score(mcp_kf* cur, int n, mcp_kf* const* cands, double* scores, int* best);
/* SmallBlurryImage::IteratePosRelToTarget (ESM): se2 = { R00, R01, R10, R11, tx, ty }, *score = final sum of squares */
int mcp_sbi_iterate(mcp_kf* cur, mcp_kf* target, int iterations, double se2[6], double* score);
/* Tracker::CalcSBIRotation's per-camera step (src/Tracker.cc:1687-1720): every mcp_kf_make_sbi keeps the SBI it replaces as
 * "last frame's"; this aligns the current one to it. */
int mcp_sbi_iterate_last(mcp_kf*, int iterations, double se2[6], double* score);
/* SmallBlurryImage::SE3fromSE2; the cameras are the 40x30 instances (TaylorCamera::SetImageSize(sirSize)) */
int mcp_sbi_se3_from_se2(const double se2[6], const mcp_camera* cam_src, const mcp_camera* cam_target, double R[9]);

/* one tracked map point as seen by Tracker::SearchForPoints */
typedef struct mcp_td_in {
  double world_pos[3];          /* MapPoint::mv3WorldPos                                   */
  double pixel_right_w[3];      /* MapPoint::mv3PixelRight_W                               */
  double pixel_down_w[3];       /* MapPoint::mv3PixelDown_W                                */
  const mcp_kf* source_kf;      /* MapPoint::mpPatchSourceKF (resident pyramid)            */
  int source_level;             /* MapPoint::mnSourceLevel                                 */
  int center_x, center_y;       /* MapPoint::mirCenter                                     */
  int fixed;                    /* MapPoint::mbFixed (exhaustive search + 10 sub-pix its)  */
} mcp_td_in;

typedef struct mcp_td_out {
  double image[2];              /* TrackerData::mv2Image (projection)                      */
  double cam_derivs[4];         /* mm2CamDerivs, row-major                                 */
  double jacobian[12];          /* mm26Jacobian 2x6 row-major (w.r.t. the BASE pose)       */
  double found_pos[2];          /* mv2Found (sub-pixel or coarse, level-0 coordinates)     */
  double sqrt_inv_noise;        /* mdSqrtInvNoise = 1 / LevelScale                         */
  double warp_inverse[4];       /* PatchFinder::mm2WarpInverse                             */
  int in_image;                 /* mbInImage                                               */
  int search_level;             /* PatchFinder::mnSearchLevel, -1 = rejected warp          */
  int template_bad;             /* PatchFinder::TemplateBad()                              */
  int searched, found, did_subpix;
  int coarse_x, coarse_y;       /* best corner at search level (irBest)                    */
  int score;                    /* nBestSSD                                                */
  uint8_t templ[64];            /* mimTemplate (8x8, row-major)                            */
} mcp_td_out;

/* TrackerData::Project + GetDerivsUnsafe + CalcJacobian, PatchFinder::CalcSearchLevelAndWarpMatrix,
 * MakeTemplateCoarseCont (with a PatchFinder that has seen nothing: the template is always made; mcp_patch_sequences carries
 * the finder's template cache from call to call), FindPatchCoarse,
 * MakeSubPixTemplate + IterateSubPixToConvergence, for n points against keyframe `target`.
 * base_from_world / cam_from_base: (R row-major 9, t 3).  range, subpix_its, exhaustive as
 * Tracker::SearchForPoints(vTD, cam, nRange, nSubPixIts, bExhaustive). */
int mcp_track_search(mcp_kf* target, const mcp_camera* cam, const double base_from_world[12],
                     const double cam_from_base[12], int n, const mcp_td_in* in, int range,
                     int subpix_its, int exhaustive, mcp_td_out* out);
/* SearchForPoints for every camera of a frame in one launch (the per-camera loops of Tracker::TrackMap, src/Tracker.cc:985-1030):
 * targets[c], cams[c], cam_from_base[12*c..], n[c] points in[c] -> out[c]; results equal ncam mcp_track_search calls. */
int mcp_track_search_batch(int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double base_from_world[12],
                           const double* cam_from_base /* ncam x 12 */, const int* n, const mcp_td_in* const* in,
                           int range, int subpix_its, int exhaustive, mcp_td_out* const* out);

/* ---- PatchFinder with its members carried from call to call ------------------------------------------------------------
 * The reference's PatchFinder is stateful (src/PatchFinder.cc:56-65): MakeTemplateCoarseCont keeps the template while it works on
 * the same MapPoint and neither column of the warp matrix has moved by more than 0.07 (:144-181; mbTemplateBad and the sums stay
 * too), MakeSubPixTemplate's Jacobians stay until it runs again (:362-390) and mdMeanDiff is only reset there.  What a search
 * returns therefore depends on what the finder saw before.  mcp_pf_state holds those members; the caller owns one per PatchFinder
 * object of the reference, zero-initialised (valid = 0) for a new one, and passes it in and out.
 * A SEQUENCE is what one finder sees, in order (one wavefront walks it); sequences run in parallel.  Modes = the finder's callers:
 *  MCP_PF_TRACK       Tracker::SearchForPoints (src/Tracker.cc:1299-1377).  One finder per TrackerData = per (point, camera), kept
 *                     over the frames: one sequence of one item per tracked point.  range / subpix_its / exhaustive as there.
 *                     (mcp_track_search* = this with finders that have seen nothing.)
 *  MCP_PF_REFIND      MapMakerServerBase::ReFind_Common (src/MapMakerServerBase.cc:921-1002): ONE static finder over all calls --
 *                     ReFindNewlyMade walks every keyframe with the same point, so templates are shared between keyframes with
 *                     similar warps (one sequence per new point, one item per keyframe).  MakeTemplateCoarse ignores the verdict
 *                     of CalcSearchLevelAndWarpMatrix; range 4 (pass it); sub-pixel iteration (8) only when the level is > 0, and
 *                     its position is kept whether or not it converged (found stays 1, did_subpix = 1).
 *  MCP_PF_EPI_COARSE  MapMakerServerBase::AddPointEpipolar, first loop (:745-795): one finder and ONE MapPoint object for all depth
 *                     hypotheses of a candidate (same point_key): one sequence per candidate, one item per hypothesis.  Hypotheses
 *                     that project outside the level-0 image / onto a zero of the target's level-0 mask are skipped; range 3.
 *  MCP_PF_EPI_REFINE  the second loop (:827-853) on the SAME finder (pass the state the coarse sequence returned): Calc +
 *                     MakeTemplateCoarseCont, SetSubPixPos(start_pos), IterateSubPixToConvergence(10); found = converged,
 *                     found_pos = the sub-pixel position.
 * mcp_td_out per item as in mcp_track_search (jacobian w.r.t. base_from_world; template_bad = the finder's flag after the item;
 * searched = FindPatchCoarse ran).  Targets must live on one device. */
#define MCP_PF_TRACK 0
#define MCP_PF_REFIND 1
#define MCP_PF_EPI_COARSE 2
#define MCP_PF_EPI_REFINE 3
typedef struct mcp_pf_state {
  int     valid;          /* mpLastTemplateMapPoint != NULL                                                       */
  int     point_key;      /* the map point the template was made for (caller's id; the reference compares &point) */
  double  last_warp[4];   /* mm2LastWarpMatrix, row-major                                                         */
  int     template_bad;   /* mbTemplateBad                                                                        */
  int     jacs_valid;     /* MakeSubPixTemplate has run (mimJacs / mm3HInv hold something)                        */
  double  mean_diff;      /* mdMeanDiff                                                                           */
  uint8_t templ[64];      /* mimTemplate                                                                          */
  uint8_t jac_templ[64];  /* the template mimJacs / mm3HInv were made from: differs from templ after a refresh that
                             hit pixels outside the source image (:165-180 skips MakeSubPixTemplate then)         */
} mcp_pf_state;
typedef struct mcp_pf_target {
  mcp_kf* kf;                   /* keyframe searched in (its level-0 mask, if it has one, serves MCP_PF_EPI_COARSE) */
  const mcp_camera* cam;
  double base_from_world[12];   /* (R row-major 9, t 3); map-maker callers pass the keyframe's CamFromWorld here ...   */
  double cam_from_base[12];     /* ... and the identity here                                                        */
} mcp_pf_target;
typedef struct mcp_pf_item {
  mcp_td_in point;
  int point_key;                /* identity of the MapPoint object                                                  */
  int target;                   /* index into targets[]                                                             */
  double start_pos[2];          /* MCP_PF_EPI_REFINE: SetSubPixPos (level-0 coordinates)                            */
} mcp_pf_item;
int mcp_patch_sequences(int mode, int n_targets, const mcp_pf_target* targets, int n_seq, const int* seq_start /* n_seq + 1 */,
                        const mcp_pf_item* items, mcp_pf_state* state /* n_seq, in/out */, int range, int subpix_its, int exhaustive,
                        mcp_td_out* out /* one per item */);

/* Tracker::CalcPoseUpdate (Tukey M-estimator, WLS<6> with prior 100)   Tracker.cc:1386-1512
 * found[i] != 0 rows contribute.  override_sigma <= 0: Tukey sigma^2 from the median.
 * mu[6] out; weights_out[n] (may be NULL) = Tukey weight per row (0 = outlier). */
int mcp_track_pose_update(int n, const uint8_t* found, const double* found_pos /*n*2*/,
                          const double* image_pos /*n*2*/, const double* sqrt_inv_noise /*n*/,
                          const double* jacobian /*n*12*/, double override_sigma, double mu[6],
                          double* weights_out, double* sigma_sq_out);
/* The same three entries with the M-estimator Tracker::CalcPoseUpdate dispatches on (Tracker::sMEstimatorName, src/Tracker.cc:1388-1401):
 * Tukey (the default; what the entries without _m use), Cauchy, Huber -- weights and sigma^2 of include/mcptam/MEstimator.h:84-204.
 * weights == 0 (the reference's outlier test, :1470) only ever happens with Tukey, as in the reference. */
#define MCP_MEST_TUKEY 0
#define MCP_MEST_CAUCHY 1
#define MCP_MEST_HUBER 2
int mcp_track_pose_update_m(int n, const uint8_t* found, const double* found_pos, const double* image_pos, const double* sqrt_inv_noise,
                            const double* jacobian, double override_sigma, double mu[6], double* weights_out, double* sigma_sq_out, int estimator);
int mcp_track_pose_refine_m(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cam_from_base, double base_from_world[12],
                            int n_iter, const uint8_t* nonlinear, const double* override_sigma, double mu_last[6], double* weights_last, int estimator);
int mcp_track_pose_refine_sharded_m(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cam_from_base, double base_from_world[12],
                                    int n_iter, const uint8_t* nonlinear, const double* override_sigma, double mu_last[6], double* weights_last,
                                    mcp_allreduce_fn allreduce, void* user, int rank, int world, int cap, int estimator);

/* ---- One stage of Tracker::TrackMap for a whole frame in ONE submission ------------------------------------------------------
 * What Tracker::TrackFrame / TrackMap do per frame and stage (src/Tracker.cc:303-318 MakeKeyFrame_Lite of every camera, :985-1030 +
 * :1299-1384 SearchForPoints per camera, :1040-1075 the ten CalcPoseUpdate iterations) as one call with one wait:
 *   imgs != NULL : mcp_kf_make_lite_batch(ncam, targets, imgs, strides, imgs_on_device, masks) first (NULL: the pyramids are current,
 *                  e.g. the fine stage after the coarse one);
 *   the search   : state == NULL: mcp_track_search_batch (finders that have seen nothing);  state != NULL: the reference's persistent
 *                  finders -- state[c][i] / point_key[c][i] belong to point i of camera c, as one single-item MCP_PF_TRACK sequence
 *                  each of mcp_patch_sequences (states updated in place);
 *   the records of the pose iterations are built from the search results on the device (world position from in[c][i], camera = c);
 *   mcp_track_pose_refine_m(total, ..., n_iter, nonlinear, override_sigma, ..., estimator) over the points of all cameras.
 * Same kernels on the same data as the separate calls: out[c] (n[c] results), pts_out (total records as the iterations left them,
 * may be NULL), base_from_world (in: the prior, out: refined), mu_last, weights_last (total, camera-major; may be NULL) are bit-identical
 * to theirs.  n_iter = 0: search only.  It saves the two host round trips between the three calls, and with a fresh frame (imgs != NULL) every
 * copy-engine operation: the small inputs ride to the device inside the pyramids' second launch, the results are written to pinned host memory
 * by the kernels that produce them and copied into the caller's arrays after the one wait (five kernels back to back on the device). */
int mcp_track_frame(int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                    const uint8_t* const* const* masks, const mcp_camera* cams, double base_from_world[12], const double* cam_from_base /* ncam x 12 */,
                    const int* n, const mcp_td_in* const* in, const int* const* point_key, mcp_pf_state* const* state,
                    int range, int subpix_its, int exhaustive, int n_iter, const uint8_t* nonlinear, const double* override_sigma, int estimator,
                    mcp_td_out* const* out, mcp_pose_point* pts_out, double mu_last[6], double* weights_last);
/* ZERO-COPY RESULTS (round 6).  The search kernel writes the TrackerData results into a pinned block of the library; with caller arrays
 * (`out` != NULL) mcp_track_frame copies them out after its one wait -- 300 bytes per point, ~25 us of the host's time per 640x480 x 4
 * frame.  A native caller that only walks the results once (Tracker::TrackMap updating its TrackerData, src/Tracker.cc:1040-1075) passes
 * out = NULL and reads them in place:
 *     const mcp_td_out* r = mcp_track_frame_view(targets[0], c, &count);      // count == n[c]
 * valid until the next mcp_track_frame / mcp_track_search_batch call whose first target is targets[0]; NULL (count 0) for a camera
 * without points, NULL + mcp_last_error() for a camera index the last frame did not have. */
const mcp_td_out* mcp_track_frame_view(const mcp_kf* first_target, int cam, int* count);

/* ---- Tracker::FindPVS over a device-resident map --------------------------------------- src/Tracker.cc:662-723, 950-961
 * A map-point table lives on one device: per row (= point index, in the caller's order) the MapPoint fields FindPVS reads --
 * mv3WorldPos, mv3PixelRight_W, mv3PixelDown_W -- and `usable` (0 = mbBad || !mbOptimized, Tracker.cc:680).  Rows that were never
 * written (a gap left by an upload past the end) are unusable.  Uploads are enqueued on the table's stream: a PVS call that follows
 * sees them, whole; the caller's arrays may be reused as soon as an upload returns. */
typedef struct mcp_map_points mcp_map_points;
mcp_map_points* mcp_map_points_create(int device /* HIP device ordinal, -1 = current */);
void mcp_map_points_destroy(mcp_map_points*);
int  mcp_map_points_rows(const mcp_map_points*);
/* rows first .. first+count-1 from SoA arrays (world_pos / pixel_right_w / pixel_down_w: count x 3, usable: count); the table grows
 * when first + count passes its size */
int  mcp_map_points_set(mcp_map_points*, int first, int count, const double* world_pos, const double* pixel_right_w,
                        const double* pixel_down_w, const uint8_t* usable);
/* the table's size becomes `rows`: rows past it are dropped (they reach no later PVS; should the table grow again they come back
 * unusable, as zero rows); a larger size appends unusable rows.  A caller that re-uploads the whole map every frame calls this with the
 * map's current size first, so that points the map has since dropped leave the table. */
int  mcp_map_points_resize(mcp_map_points*, int rows);
/* rows ids[0..count-1] (distinct; an id past the size grows the table) -- the points the map maker moved, flagged or added */
int  mcp_map_points_update(mcp_map_points*, int count, const int* ids, const double* world_pos, const double* pixel_right_w,
                           const double* pixel_down_w, const uint8_t* usable);

/* One PVS entry: what FindPVS leaves in the TrackerData and its PatchFinder (TrackerData::mv2Image, mm2CamDerivs, PatchFinder::
 * mnSearchLevel, mm2WarpInverse) -- bit-identical to mcp_track_search's image / cam_derivs / search_level / warp_inverse. */
typedef struct mcp_pvs_entry {
  int    point;                 /* table row                                 */
  int    level;                 /* search level 0..MCP_LEVELS-1              */
  double image[2];
  double cam_derivs[4];         /* row-major                                 */
  double warp_inverse[4];       /* row-major                                 */
} mcp_pvs_entry;

/* FindPVS of every camera of a frame in one call (two launches on the table's stream, one wait).  CamFromWorld = cam_from_base[c] *
 * base_from_world, (R row-major 9, t 3).  A row enters camera c's PVS when it is usable, its projection is valid and inside
 * [0, image_size] (inclusive), the level-0 mask of targets[c] -- if it has one -- is not 0 at ((int)u, (int)v), and the search level is
 * not -1.  One deviation: with a mask, a projection on u == w or v == h is dropped (the reference reads past the mask there).
 * Order: ascending row within each (camera, level) -- the reference random_shuffles every level next (Tracker.cc:983), so a fixed
 * order is as good and makes the result reproducible; the caller shuffles with its own RNG.
 * out[c] (caps[c] entries) receives camera c's list level by level (level 0 first); counts[c*MCP_LEVELS + l] = entries of
 * (c, l), always.  A camera whose PVS exceeds caps[c] gets nothing written; the call returns -1 and mcp_last_error() names it.
 * out == NULL: nothing is copied, the lists stay in the library's pinned block -- mcp_track_find_pvs_view.  Every target must be on the
 * table's device; their pyramids / masks are those of the last mcp_kf_* call. */
int mcp_track_find_pvs(mcp_map_points*, int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double base_from_world[12],
                       const double* cam_from_base /* ncam x 12 */, const int* caps, mcp_pvs_entry* const* out, int* counts /* ncam x MCP_LEVELS */);
/* zero-copy: the (cam, level) list of the last mcp_track_find_pvs on this table, valid until the next one; NULL + count 0 for an empty
 * list, NULL + mcp_last_error() for a (cam, level) the last call did not produce */
const mcp_pvs_entry* mcp_track_find_pvs_view(const mcp_map_points*, int cam, int level, int* count);

/* ---- Tracker::TrackMap of a frame from the resident table ------------------------------------------ src/Tracker.cc:938-1075
 * The shuffle of the reference (random_shuffle, :983 and :876-883) cannot be reproduced bit for bit; every layer uses this keyed one
 * instead.  "Shuffled" means ascending (key, row); for a given (seed, stage, cam) the keys of distinct rows are distinct (mcp_mix64 is a
 * bijection).  Stage 0 orders each PVS level, stage 1 the chop of the fine stage's budget. */
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MCP_HOST_DEVICE __host__ __device__      /* the library's kernels use these very definitions */
#else
#define MCP_HOST_DEVICE
#endif
static inline MCP_HOST_DEVICE uint64_t mcp_mix64(uint64_t z) { z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                                               z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static inline MCP_HOST_DEVICE uint64_t mcp_track_shuffle_key(uint64_t seed, int stage, int cam, int row) {
  return mcp_mix64(mcp_mix64(seed ^ ((uint64_t)stage << 40) ^ ((uint64_t)cam << 32)) ^ (uint32_t)row); }

/* The patch source of each row (MapPoint::mpPatchSourceKF, mnSourceLevel, mirCenter (center_xy: count x 2), mbFixed) and its identity
 * keys[k] (the point_key of that row's finders).  source_kf[k] == NULL: the row has no source.  The table keeps (handle, creation serial)
 * and resolves it at every mcp_track_map through the library's registry of live keyframes: a row whose source has been destroyed is dropped
 * from the selection (counted in mcp_track_map_result::stale), never dereferenced.  Sources must live on the table's device.  A row whose
 * key changes gets finders that have seen nothing for every camera.  Enqueued on the table's stream like mcp_map_points_set. */
int mcp_map_points_set_source(mcp_map_points*, int first, int count, const int* keys, mcp_kf* const* source_kf, const int* source_level,
                              const int* center_xy, const uint8_t* fixed);
int mcp_map_points_update_source(mcp_map_points*, int count, const int* ids, const int* keys, mcp_kf* const* source_kf, const int* source_level,
                                 const int* center_xy, const uint8_t* fixed);
/* The persistent finders (TrackerData::mFinder, one per (row, camera index of mcp_track_map)) of rows first .. first+count-1 for camera
 * `cam`; a camera no call has used yet reads as zeroed states.  Waits for the table's stream. */
int mcp_map_points_get_states(const mcp_map_points*, int cam, int first, int count, mcp_pf_state* out);

typedef struct mcp_track_map_params {
  int try_coarse, coarse_max, coarse_range, coarse_min, coarse_subpix_its;  /* after TrackMap's heuristics, doubling on recovery included (:990-1008) */
  int max_patches;                                                        /* snMaxPatchesPerFrame                                          */
  int estimator;                                                          /* MCP_MEST_*                                                    */
  unsigned long long seed;                                                /* of mcp_track_shuffle_key                                      */
} mcp_track_map_params;
typedef struct mcp_track_map_result {
  int did_coarse, coarse_found;                   /* coarse_found = sum of found && !template_bad over the coarse set; did_coarse = > coarse_min */
  int pvs_counts[MCP_MAX_FRAME_CAMS][MCP_LEVELS]; /* this frame's PVS per (camera, level), stale-source rows included                  */
  int set_sizes[MCP_MAX_FRAME_CAMS][3];           /* |C|, |T|, |R| per camera                                                          */
  int stale[MCP_MAX_FRAME_CAMS];                  /* PVS entries dropped because the row's source keyframe is missing or destroyed      */
  double mu_last[6];                              /* last update of the fine iterations                                                */
} mcp_track_map_result;
typedef struct mcp_track_map_item {
  int point;                                      /* table row                                                                          */
  int stage;                                      /* 0 = coarse set C, 1 = remaining top level T, 2 = budgeted rest R                    */
  double weight_last;                             /* M-estimator weight of the last fine iteration (0 = outlier or not found)            */
  mcp_td_out out;                                 /* the search's record (C: the coarse search's)                                       */
} mcp_track_map_item;
/* The whole TrackMap of a frame in one submission with one wait, from the table to the refined pose (base_from_world in / out):
 *   imgs != NULL: mcp_kf_make_lite_batch(ncam, targets, imgs, strides, imgs_on_device, masks) first;
 *   FindPVS (as mcp_track_find_pvs with caps = rows; mcp_track_find_pvs_view then returns this frame's lists);
 *   per camera c, with P[l] = its PVS level l without stale-source rows, S_l = P[l] in stage-0 key order:
 *     C = (try_coarse) the first min(|S_3|, coarse_max) of S_3, then the first min(|S_2|, coarse_max - |C|) of S_2, removed from them;
 *     T = the rest of S_3; R0 = the rest of S_2, then S_1, then S_0; K = max(0, max_patches - |C| - |T|);
 *     R = R0 if |R0| <= K, else the K entries of R0 with the smallest stage-1 keys, in that order;
 *   coarse search of every C (MCP_PF_TRACK finders from the table, coarse_range, coarse_subpix_its, the prior pose);
 *   did_coarse = coarse_found > coarse_min: then 10 iterations over the C records, all re-projecting, override {0 x 6, 1.0 x 4};
 *   fine search of T (range did_coarse ? 5 : 10, 8 sub-pixel iterations) and R (same range, 0) at the current pose;
 *   10 iterations over the camera-major records [C_c, T_c, R_c], re-projecting at 0, 4, 9, override {0 x 6, 16.0 x 4};
 *   the searched finders' states back into the table.
 * Results equal mcp_track_find_pvs + the selection above + mcp_patch_sequences + mcp_track_pose_refine_m composed on the host, bit for bit,
 * with one deviation: more than 1024 records in one iteration stage run in the single-workgroup kernel (mcp_track_pose_refine_m's path with
 * MCP_TRACK_REFINE_MULTI=0), since the record count is only known on the device.  Refusals (-1) happen before anything is enqueued. */
int mcp_track_map(mcp_map_points*, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                  const uint8_t* const* const* masks, const mcp_camera* cams, double base_from_world[12], const double* cam_from_base /* ncam x 12 */,
                  const mcp_track_map_params*, mcp_track_map_result* res);
/* zero-copy: camera cam's items [C, T, R] of the last mcp_track_map on this table, in the library's pinned block; valid until the next call */
const mcp_track_map_item* mcp_track_map_view(const mcp_map_points*, int cam, int* count);

/* ---- MapMakerServerBase::AddStereoMapPoints of one source keyframe and level in ONE submission ---- src/MapMakerServerBase.cc:411-496, 604-918
 * The reference loops over the targets j = 0, 1, ... (ClosestKeyFramesWithinDist, after the caller has dropped the targets it skips: mbBad parents,
 * CrossCamera, sbOnlyFirstCameraGeneratesPoints) and per target over the candidates left by ThinCandidates, calling AddPointEpipolar.  Here, per
 * target and on the device:
 *   ThinCandidates: a candidate (level position) survives when (busy - pos).mag_squared() >= 100 for every busy position -- ir_rounded(root_pos /
 *     LevelScale(level)) of every source measurement at `level` or `level + 1`, and the root positions of the points this call created so far;
 *   per surviving candidate (one wavefront each): the epipolar arc of :611-723, the probe MapPoint of :726-738, its hypotheses walked through ONE fresh
 *     finder in MCP_PF_EPI_COARSE semantics (range 3), the ambiguity rules of :798-825 as the code has them (matches in (score, hypothesis) order;
 *     nResizeTo = 1 + #{later matches with score > 0.9 best}; reject above 3 or when a kept index is more than 1 from the best), the kept matches in
 *     MCP_PF_EPI_REFINE semantics on the same finder (first to converge wins), ReprojectPoint (:123-143, one-sided Jacobi SVD) and the new point;
 *   nLimit as the reference counts it: numSuccess runs over all targets and the break only leaves the candidate loop, so once the limit is reached every
 *     later target still tries its first surviving candidate.
 * Results equal mcp_stereo_hypotheses + mcp_patch_sequences(EPI_COARSE) with fresh states + that selection + mcp_patch_sequences(EPI_REFINE) on the
 * returned states, composed on the host.  Runs on the source's stream with scratch owned by the source; targets are only read. */
typedef struct mcp_stereo_target {
  mcp_kf* kf;                   /* keyframe searched in (its level-0 mask, if any, gates hypotheses as in MCP_PF_EPI_COARSE) */
  const mcp_camera* cam;
  double cam_from_world[12];    /* KeyFrame::mse3CamFromWorld (R row-major 9, t 3)                                          */
  double one_pixel_angle;       /* TaylorCamera::OnePixelAngle() of the target camera (src/TaylorCamera.cc:194-196), > 0       */
} mcp_stereo_target;
typedef struct mcp_stereo_meas {       /* one entry of the source's mmpMeasurements                                         */
  double root_pos[2];           /* Measurement::v2RootPos                                                                 */
  int level;                    /* Measurement::nLevel                                                                    */
  int pad_;
} mcp_stereo_meas;
typedef struct mcp_stereo_point {      /* one created MapPoint with its two measurements (:855-914)                       */
  int candidate;                /* index into the caller's candidate list                                                 */
  int target;                   /* index into targets[]                                                                   */
  int hypothesis;               /* winning hypothesis (step along the arc)                                                */
  int score;                    /* its coarse ZMSSD                                                                       */
  double world_pos[3];          /* mv3WorldPos                                                                            */
  double root_pos[2];           /* SRC_ROOT measurement: LevelZeroPos of the candidate                                    */
  double target_pos[2];         /* SRC_EPIPOLAR measurement: the sub-pixel position in the target, level 0                */
  double center_nc[3], one_right_nc[3], one_down_nc[3];   /* mv3Center_NC, mv3OneRightFromCenter_NC, mv3OneDownFromCenter_NC */
  double pixel_right_w[3], pixel_down_w[3];               /* RefreshPixelVectors at world_pos                              */
} mcp_stereo_point;
/* outcome per (target, candidate) */
#define MCP_STEREO_THINNED 1      /* not in the candidate list when the target's turn came                               */
#define MCP_STEREO_NO_ARC 2       /* v3BetweenEndpoints too small, or a non-finite arc / step count                      */
#define MCP_STEREO_NO_MATCH 3     /* no hypothesis found a match                                                         */
#define MCP_STEREO_TOO_MANY 4     /* nResizeTo > 3                                                                       */
#define MCP_STEREO_INDEX_FAR 5    /* a kept match more than one hypothesis from the best                                 */
#define MCP_STEREO_NO_SUBPIX 6    /* no kept match converged                                                             */
#define MCP_STEREO_CREATED 7
#define MCP_STEREO_PAST_LIMIT 8   /* a surviving candidate the reference never tries because numSuccess reached nLimit    */
/* src / src_cam / src_cam_from_world: the source keyframe; cand: its level-`level` candidate positions (Level::vCandidates, in order); meas: its
 * measurements.  Returns the number of created points (<= n_cand <= cap), written to out in the reference's creation order (target-major, candidate
 * ascending).  keep[n_cand]: vCandidates as the reference leaves it (thinned before the last target).  outcome: NULL or n_targets x n_cand codes.
 * Refusals (-1, mcp_last_error()) happen before anything is enqueued: NULL or destroyed keyframes, keyframes without a frame, a target on another
 * device, a level outside 0..3, negative counts, a bad camera, cap < n_cand, a candidate outside the level image, a non-finite measurement, a
 * one_pixel_angle that is not positive and finite. */
int mcp_stereo_points(mcp_kf* src, const mcp_camera* src_cam, const double src_cam_from_world[12], int level, int n_cand, const mcp_int2* cand,
                      int n_meas, const mcp_stereo_meas* meas, int n_targets, const mcp_stereo_target* targets, int limit,
                      int cap, mcp_stereo_point* out, uint8_t* keep, uint8_t* outcome);
/* (mcp_stereo_map_points, at the end of this header with the map graph it writes into, is the form that also leaves the created points in the
 * map-point table, the graph's point columns and the store, without the host sending them up again) */
/* The hypotheses of mcp_stereo_points for candidates cand[0..n_cand) against one target, computed by the same device code: hypothesis h of candidate
 * i is out[offsets[i] + h] (offsets: n_cand + 1), as the mcp_td_in the finder sees (world position, pixel vectors of the probe MapPoint, source =
 * src at `level`, center = the candidate).  Returns the total; out == NULL counts only, otherwise total > cap is refused. */
int mcp_stereo_hypotheses(mcp_kf* src, const mcp_camera* src_cam, const double src_cam_from_world[12], int level, int n_cand, const mcp_int2* cand,
                          const mcp_stereo_target* target, int cap, mcp_td_in* out, int* offsets);

/* ---- BundleAdjusterMulti::AdjustAndUpdate: the write-back of an adjustment into the table ---------- src/BundleAdjusterMulti.cc:286-334
 * (the same in BundleAdjusterSingle.cc:175-215 and BundleAdjusterCalib.cc).  After a successful adjustment the reference (1) refreshes every
 * keyframe's mse3CamFromWorld, (2) sets every point's mv3WorldPos from the bundle and calls MapPoint::RefreshPixelVectors (src/MapPoint.cc:62-87),
 * (3) calls RefreshSceneDepthRobust of every keyframe (src/KeyFrame.cc:547-645).  mcp_ba_write_back does the three steps on the device, from the
 * solver's state to the table's rows, in one submission with one wait.
 *
 * RefreshPixelVectors needs the patch rays of a point -- mv3Center_NC, mv3OneRightFromCenter_NC, mv3OneDownFromCenter_NC, set once when the
 * point is created (mcp_stereo_point returns them); mv3Normal_NC is (0, 0, -1) everywhere.  They are a column of the table: */
/* rays of rows first .. first+count-1 / of rows ids[0..count-1] (count x 3 each).  Shapes, growth, the duplicate check and the stream
 * ordering are those of mcp_map_points_set / mcp_map_points_update; the other columns of the rows keep their contents.  The table remembers on
 * the host which rows have rays: a row dropped by mcp_map_points_resize, or one that came into being as a gap, has none until they are set again. */
int mcp_map_points_set_rays(mcp_map_points*, int first, int count, const double* center_nc, const double* one_right_nc, const double* one_down_nc);
int mcp_map_points_update_rays(mcp_map_points*, int count, const int* ids, const double* center_nc, const double* one_right_nc, const double* one_down_nc);
/* rows first .. first+count-1 read back (every pointer may be NULL: that column is skipped); waits for the table's stream */
int mcp_map_points_get(const mcp_map_points*, int first, int count, double* world_pos, double* pixel_right_w, double* pixel_down_w, uint8_t* usable);

typedef struct mcp_scene_depth {
  double mean, sigma;           /* mdSceneDepthMean, mdSceneDepthSigma; written only when refreshed != 0                                     */
  double median, sigma_sq;      /* dMedianDepth and the Huber sigma^2 after the clamp at 0.4; written only when refreshed != 0                */
  int n;                        /* entries of the keyframe's list                                                                            */
  int refreshed;                /* 1: refreshed;  0: n <= 3, the keyframe is left alone (:587-591);  -1: the mean is not finite (all weights
                                   0) -- the reference stops the process there (:635-644), here the caller decides                           */
} mcp_scene_depth;

/* RefreshSceneDepthRobust(vector&) of n_kf keyframes over the table, one workgroup per keyframe, one wait.  cam_from_world: n_kf x 12 (R row-major
 * 9, t 3).  seg_rows[seg_start[j] .. seg_start[j+1]) are the table rows of keyframe j's measured points that are not bad (the caller filters
 * mbBad, :558; a row may appear more than once), seg_weights their inlier ratios (:566).  Depth = norm(CamFromWorld_j * world_pos[row]) from the
 * table as it stands on its stream.  Then, exactly: n <= 3 leaves the keyframe alone; median = element [n/2] of the sorted depths; squared distances
 * from it; Huber::FindSigmaSquared (MEstimator.h:194-204, its [n/2] element and small-sample factor) clamped below at 0.4;
 * Huber::SquareRootWeight times the given weight; mean = S(w d) / S(w), sigma = sqrt(S(w d d) / S(w) - mean^2).
 * SUMMATION ORDER (fixed, part of the contract): with the list in the caller's order, thread t of 256 adds entries t, t + 256, ... in ascending
 * position; each wavefront folds its 64 partial sums by halving (lane l += lane l + 32, then 16, 8, 4, 2, 1); the four wavefront totals are added
 * 0, 1, 2, 3.  The reference adds in sorted order, so mean and sigma differ from it by rounding (<= n 2^-52 relative per sum); median and
 * sigma_sq are exact, and two calls on the same table give the same bits.
 * depth_out: NULL or n_kf entries;  seg_depths_out: NULL or seg_start[n_kf] depths in the caller's order.  A segment may be empty; n_kf == 0 is
 * allowed.  Refusals as mcp_ba_write_back's.  Threading: as mcp_map_points_update. */
int mcp_scene_depth_robust(mcp_map_points*, int n_kf, const double* cam_from_world, const int* seg_start /* n_kf + 1 */, const int* seg_rows,
                           const double* seg_weights, mcp_scene_depth* depth_out, double* seg_depths_out);

/* The write-back.  STATE READ: the solver's current device state -- after mcp_ba_compute, or after mcp_ba_prepare alone (then: the state as added).
 * No host copy of it is used.
 * POINTS: point_ids[k] is a bundle point id, rows[k] the table row it belongs to (rows distinct, every one with rays).  With Ts = the product of
 * the current poses along the point's own chain (what the solver's residual uses), world = Ts^-1 * x; for a fixed point world = x.
 * RefreshPixelVectors runs at the pose of src_chains[k * chain_stride .. + src_chain_len[k]) (pose ids as in mcp_ba_add_meas); length 0, or
 * src_chains == NULL: the point's own chain -- a fixed point lives on the world pose's chain and names its patch source's chain here.  The row
 * becomes (world, pixel_right_w, pixel_down_w, usable = 1); rows not named keep every byte.  world_pos_out / pixel_right_out / pixel_down_out
 * (all three NULL, or n_points x 3 each) receive the same bits.
 * KEYFRAMES: kf_chains[j * chain_stride .. + kf_chain_len[j]) names keyframe j's CamFromWorld as a chain of the bundle ({MKF id, camera id} for
 * BundleAdjusterMulti, {KF id} for Single); its product at the current state goes to kf_cam_from_world_out (NULL or n_kf x 12) and is the pose of
 * the scene-depth step, which is mcp_scene_depth_robust's (same kernel) and reads the table AFTER the point step of this call: points that were
 * not in the bundle contribute their current position, as in the reference.
 * ORDER AND WAITS: one event makes the table's stream wait for the solver's stream; the kernels run on the table's stream, so a mcp_track_map /
 * mcp_track_find_pvs that follows sees whole rows.  The call returns after its one wait: nothing reads the solver's device memory once it has
 * returned, the handle may be destroyed at once.  Threading: as mcp_map_points_update -- the caller serialises calls on one table, and drives the
 * solver handle from the same thread or otherwise keeps it idle during the call.
 * REFUSALS (-1, mcp_last_error(), nothing enqueued, table unchanged): NULL handles; table and solver on different devices; a handle that was
 * never prepared (or changed since); a handle with an all-reduce hook or a communicator installed (its points are sharded over ranks: out of
 * scope); an id that is not a point; a chain entry that is not a pose, or a chain longer than MCP_MAX_CHAIN (or chain_stride); a negative or
 * repeated row; a row without rays; seg_start not non-decreasing from 0; a seg_rows entry outside the table; a non-finite or negative weight; a
 * required pointer NULL with a positive count.  n_points == 0 or n_kf == 0 is allowed. */
int mcp_ba_write_back(mcp_ba*, mcp_map_points*, int n_points, const int* point_ids, const int* rows, const int* src_chains, int chain_stride,
                      const int* src_chain_len, double* world_pos_out, double* pixel_right_out, double* pixel_down_out,
                      int n_kf, const int* kf_chains, const int* kf_chain_len, const int* seg_start, const int* seg_rows, const double* seg_weights,
                      double* kf_cam_from_world_out, mcp_scene_depth* depth_out, double* seg_depths_out);
/* device time of the last completed mcp_ba_write_back / mcp_scene_depth_robust on this table, milliseconds between HIP events on the table's
 * stream: the copy of the packed inputs, the chain table + point kernel (0 for mcp_scene_depth_robust), the scene-depth kernel.  Each may be NULL. */
int mcp_map_points_last_timing(const mcp_map_points*, double* copy_ms, double* points_ms, double* depth_ms);

/* ---- TrackMap with its bookkeeping on the device ------------------------------- src/Tracker.cc:1157-1274, 1322-1361, 1452-1489, 1618-1658
 * The counts column: MapPoint::mnMEstimatorInlierCount / mnMEstimatorOutlierCount of every row, two ints.  A row whose counts were never set
 * reads (1, 0) -- the MapPoint constructor's values (include/mcptam/MapPoint.h:103-104) -- and so does a row that came into being as a gap, or
 * one that mcp_map_points_resize dropped and a later growth brought back.  Growth, the duplicate-id check and the stream ordering are those of
 * mcp_map_points_set / mcp_map_points_update; the other columns keep their contents.  inlier < 1 or outlier < 0 is refused with the column
 * untouched (the reference asserts inlier > 0; every weight inlier / (inlier + outlier) stays finite).  Only these calls and
 * mcp_track_map_record change counts: a key change in mcp_map_points_set_source does NOT reset them -- the owner of the table sets the counts
 * when it puts a new point into a row.  mcp_map_points_get_counts waits for the table's stream. */
int mcp_map_points_set_counts(mcp_map_points*, int first, int count, const int* inlier, const int* outlier);
int mcp_map_points_update_counts(mcp_map_points*, int count, const int* ids, const int* inlier, const int* outlier);
int mcp_map_points_get_counts(const mcp_map_points*, int first, int count, int* inlier, int* outlier);

typedef struct mcp_track_record_params {
  int lost;                     /* Tracker::IsLost() before this frame: != 0 -> searched-but-not-found items get no outlier mark (:1454)     */
  int want_items;               /* != 0: the items as mcp_track_map leaves them (mcp_track_map_view); 0: no 320-byte item leaves the device */
  int min_patches;              /* snMinPatchesPerFrame  } AssessTrackingQuality                                                            */
  int coarse_min;               /* snCoarseMin           }                                                                                  */
  double quality_good, quality_bad;   /* sdTrackingQualityGood / sdTrackingQualityBad                                                     */
} mcp_track_record_params;

/* 8 bytes per item, camera-major [C_c, T_c, R_c]: the order of mcp_track_map's items */
typedef struct mcp_track_note {
  int row;                      /* table row                                                                                                */
  uint8_t cam, stage;           /* camera index; 0 = C, 1 = T, 2 = R                                                                         */
  uint8_t level;                /* search_level, 255 = -1                                                                                   */
  uint8_t flags;                /* MCP_TN_*                                                                                                 */
} mcp_track_note;
#define MCP_TN_SEARCHED     0x01
#define MCP_TN_FOUND        0x02
#define MCP_TN_DID_SUBPIX   0x04
#define MCP_TN_TEMPLATE_BAD 0x08
#define MCP_TN_IN_IMAGE     0x10
#define MCP_TN_ATTEMPTED    0x20   /* !template_bad && level >= 0: the item counts in attempted[cam][level]                                */
#define MCP_TN_MARK_SHIFT   6      /* bits 6-7, the mark of this frame: 0 none, 1 inlier, 2 outlier                                         */
#define MCP_TN_MARK(flags)  (((flags) >> MCP_TN_MARK_SHIFT) & 3)

/* 32 bytes per FOUND item, in item order: what SaveSimpleMeasurements / RecordMeasurements walk (:1157-1177, 1237-1274).  Every item's row was
 * usable (!mbBad && mbOptimized) when the call started -- FindPVS admits no other -- so the list needs no mbBad filter. */
typedef struct mcp_track_meas {
  int item;                     /* index into the camera's items / notes                                                                    */
  int row, level, subpix;       /* table row, search level, did_subpix                                                                      */
  double found_pos[2];          /* TrackerData::mv2Found, level-0 coordinates                                                               */
} mcp_track_meas;

typedef struct mcp_track_record {
  int attempted[MCP_MAX_FRAME_CAMS][MCP_LEVELS], found[MCP_MAX_FRAME_CAMS][MCP_LEVELS];   /* mmMeasAttemptedLevels / mmMeasFoundLevels       */
  int quality[MCP_MAX_FRAME_CAMS];   /* 0 BAD, 1 DODGY, 2 GOOD: the arithmetic of AssessTrackingQuality (:1618-1658), in double             */
  int quality_max;                   /* the maximum over the cameras: AssessOverallTrackingQuality before its host-only heuristics           */
  int n_items[MCP_MAX_FRAME_CAMS], n_meas[MCP_MAX_FRAME_CAMS];
  int n_inliers, n_outlier_marks;    /* mnNumInliers; all outlier marks of the frame                                                        */
  double cam_from_world[MCP_MAX_FRAME_CAMS][12];   /* cam_from_base[c] * refined base_from_world: the bits the depth step used               */
  mcp_scene_depth depth[MCP_MAX_FRAME_CAMS];       /* RefreshSceneDepth (:1180-1228); refreshed == 0: all other fields 0 but n               */
} mcp_track_record;

/* mcp_track_map plus the bookkeeping Tracker::TrackMap leaves behind, in one submission with one wait.
 * POSE AND RESULT: base_from_world, res, the finders' states and the PVS views are mcp_track_map's, bit for bit; with want_items != 0 so are the
 * items.  With want_items == 0 mcp_track_map_view returns NULL and mcp_last_error() says why.
 * MARKS follow the weights of the last fine iteration (items of the coarse set keep the coarse search's record, as in mcp_track_map).  Per item:
 *   !found: an outlier mark iff searched && !lost;   found && weight_last == 0.0: an outlier mark;   found && weight_last != 0.0: an inlier mark,
 *   counted in n_inliers.
 * Every mark adds 1 to the row's count column; a row tracked by several cameras is marked once per camera (integer atomic adds: the sums do not
 * depend on the order).
 * COUNTERS: attempted[c][l] counts the items of camera c with !template_bad && search_level == l >= 0, found[c][l] those that are found as well.
 * quality[c]: with F / A the sums over the levels and LF / LA those over levels 2 and 3 -- F < min_patches: BAD; else t = (double)F / A,
 * g = LA > coarse_min ? (double)LF / LA : t;  t > quality_good: GOOD;  else g < quality_bad: BAD;  else DODGY.
 * MEASUREMENTS: camera c's found items in item order (mcp_track_map_meas_view).
 * SCENE DEPTH runs after all marks of all cameras (a kernel boundary).  Camera c's list is its found items in item order, the weights
 * (double)inlier / (double)(inlier + outlier) from the column as it then stands, the depth norm(cam_from_world[c] * world_pos[row]) with
 * cam_from_world[c] = cam_from_base[c] * base_from_world AFTER the iterations (FindPVS's product).  One deviation: the reference reads td.mv3Cam, the value of the
 * last re-projecting iteration (:1204); here every depth is taken at the final pose.  The
 * kernel is mcp_scene_depth_robust's, the lists are built on the device: its summation-order contract holds word for word; n <= 3 gives
 * refreshed = 0, a non-finite mean refreshed = -1.
 * REFUSALS: mcp_track_map's, a NULL mcp_track_record_params / mcp_track_record, a non-finite quality threshold -- before anything is enqueued,
 * with the counts column untouched. */
int mcp_track_map_record(mcp_map_points*, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                         const uint8_t* const* const* masks, const mcp_camera* cams, double base_from_world[12], const double* cam_from_base /* ncam x 12 */,
                         const mcp_track_map_params*, mcp_track_map_result* res, const mcp_track_record_params*, mcp_track_record* rec);
/* zero-copy, in the library's pinned blocks, valid until the next track / PVS call on this table: camera cam's notes (one per item) and
 * measurements (one per found item).  NULL + count 0 for an empty list; NULL + mcp_last_error() unless the last such call on the table was a
 * successful mcp_track_map_record with that camera. */
const mcp_track_note* mcp_track_map_notes_view(const mcp_map_points*, int cam, int* count);
const mcp_track_meas* mcp_track_map_meas_view(const mcp_map_points*, int cam, int* count);

/* ---- Tracker::TrackFrame's tracking branch in ONE submission ------------------------------------ src/Tracker.cc:319-330, 431-434, 1516-1555, 1687-1749
 * mcp_track_map_record with the pose it starts from made on the device: TrackFrameSetup's SmallBlurryImages (blur 0.75), CalcSBIRotation,
 * ApplyMotionModel, then TrackMap with its bookkeeping, then UpdateMotionModel -- one submission, one wait.
 * THE TRACKER'S SBIs live in the table, a `this` and a `last` one per camera index 0 .. MCP_MAX_FRAME_CAMS-1 (pass the cameras in the same
 * order every frame, as for the finders).  They are not the keyframe handles' SBIs (mcp_kf_make_sbi: KeyFrame::mpSBI, the relocaliser's) and
 * survive a change of target handles (AddNewKeyFrame).  Every call makes `this` from level 0 of the target -- after the pyramids when imgs is
 * given, as held when imgs == NULL -- the previous `this` becoming `last`; the first frame of a camera index after creation or
 * mcp_track_motion_reset (Tracker::Reset) makes `last` equal to `this` (:319-324) and reports first_frame[c] = 1: its alignment is the identity
 * (se2 = identity, score 0), its rotation exactly zero, and it counts as used.
 * USED CAMERAS: apply != 0 && use_rotation_estimator != 0 && cam_good[c] != 0.  A used camera's SBI is aligned against its `last` for
 * sbi_iterations rounds (mcp_sbi_iterate's bits), turned into a rotation with cams_sbi[c] (SE3fromSE2; the 40x30 camera, mmCameraModelsSBI),
 * its logarithm carried into the base frame by cam_from_base[c].R^-1.  The used cameras' rotations are averaged in camera order
 * (FindAverageRotation, eps 1e-3).  DEVIATION: the reference's averaging loop has no bound; here it ends after 32 evaluations of the mean
 * residual at the latest, avg_rounds reports how many ran.
 * PRIOR: v6 = velocity * dt, its rotation part replaced by the average when n_used > 0; prior = SE3::exp(v6) * base_from_world as given
 * (`start`).  apply == 0 (the frame after AttemptRecovery, :496-500): the SBIs are made and rolled, prior = start bit for bit, v_new zeros and
 * velocity returned as given.
 * EVERYTHING ELSE is mcp_track_map_record's, word for word, started from `prior`: base_from_world returns refined, res / rec / the views / the
 * finders / the count column as there.
 * VELOCITY: v_new = SE3::ln(refined * start^-1) / dt, velocity = 0.9 (0.5 v_new + 0.5 velocity_in) (UpdateMotionModel; TooN order [t; w]).
 * mdMSDScaledVelocityMagnitude stays with the caller (it needs mdTotalDepthMean).
 * REFUSALS (-1, mcp_last_error(), nothing enqueued, no SBI rolled, outputs untouched): mcp_track_map_record's; NULL motion structs; NULL
 * cams_sbi or a bad camera in it; blur <= 0; sbi_iterations < 0; a non-finite velocity; imgs == NULL with a target that holds no frame; and
 * -- DEVIATION, the reference would divide by it -- apply != 0 with dt not finite or <= 0. */
typedef struct mcp_track_motion_params {
  int apply;                    /* 0: a frame after AttemptRecovery -- SBIs made and rolled, prior = base_from_world as given, velocity returned as given */
  int use_rotation_estimator;   /* Tracker::sbUseRotationEstimator */
  int sbi_iterations;           /* 6 */
  double blur;                  /* Tracker::sdRotationEstimatorBlur, 0.75 */
  double dt;                    /* mLastProcessDur.toSec() */
  double velocity[6];           /* mv6BaseVelocity before the frame, TooN order [t; w] */
  uint8_t cam_good[MCP_MAX_FRAME_CAMS];   /* mmTrackingQuality[cam] == GOOD after the previous frame */
} mcp_track_motion_params;
typedef struct mcp_track_motion {
  double start[12], prior[12];            /* mse3StartPose; the pose TrackMap started from: the bits the PVS kernel read */
  double se2[MCP_MAX_FRAME_CAMS][6], sbi_score[MCP_MAX_FRAME_CAMS];   /* as mcp_sbi_iterate; zeros for a camera not aligned */
  double cam_rot[MCP_MAX_FRAME_CAMS][3];  /* axis-angle in the base frame, per used camera */
  double sbi_rot[3]; int n_used, avg_rounds, first_frame[MCP_MAX_FRAME_CAMS];
  double v_new[6], velocity[6];           /* UpdateMotionModel: the new mv6BaseVelocity */
} mcp_track_motion;
int mcp_track_frame_motion(mcp_map_points*, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                           const uint8_t* const* const* masks, const mcp_camera* cams, const mcp_camera* cams_sbi, double base_from_world[12],
                           const double* cam_from_base, const mcp_track_map_params*, mcp_track_map_result*, const mcp_track_record_params*,
                           mcp_track_record*, const mcp_track_motion_params*, mcp_track_motion*);
/* Tracker::Reset (:163-164): every camera index forgets its SBIs */
int mcp_track_motion_reset(mcp_map_points*);
/* camera index cam's SBI, which = 0 this, 1 last, in mcp_kf_get_sbi's layouts (NULL: not wanted); waits for the table's stream; -1 when that
 * camera index has none */
int mcp_track_motion_get_sbi(const mcp_map_points*, int cam, int which, uint8_t* small_img, float* templ, float* jacs);
/* host restatements of the two motion kernels (same source, host compiler); need no device.  _prior_host takes the alignments (se2 is read
 * for used cameras only) and fills start, prior, se2 (zeros for a camera not used), cam_rot, sbi_rot, n_used and avg_rounds of *out;
 * _update_host fills v_new and velocity.  Refusals as above where they apply, *out untouched. */
int mcp_track_motion_prior_host(int ncam, const double* se2 /*ncam x 6*/, const mcp_camera* cams_sbi, const double* cam_from_base, const double start[12],
                                const mcp_track_motion_params*, mcp_track_motion* out);
int mcp_track_motion_update_host(const double start[12], const double refined[12], const mcp_track_motion_params*, mcp_track_motion* out);

/* ---- Tracker::TrackFrame's lost branch in ONE submission ------------------------------------------ src/Tracker.cc:493-502, 526-552; src/Relocaliser.cc:61-120
 * mcp_track_frame_motion with apply = 0 whose start pose the relocaliser makes on the device: one submission on the table's stream, one wait.
 * Per camera c, in camera order: the relocaliser's SBI of the current frame is made from level 0 of targets[c] with reloc_blur INTO THE HANDLE'S
 * OWN SBI (mcp_kf_make_sbi's bytes; the earlier one becomes `last`; mcp_kf_get_sbi reads it afterwards); its ZMSSD is taken against every
 * candidate with cand_cam == c (mcp_sbi_score's bits); the winner is the first smallest in list order (strict <, Relocaliser.cc:113: an exact
 * tie goes to the lower index); the SBI is aligned against the winner for reloc_iterations rounds (mcp_sbi_iterate's bits);
 * cam_pose[c] = SE3fromSE2(se2, cams_sbi[c], cams_sbi[c]) * cand_cam_from_world[best] (the rotation with zero translation; an se2 that is
 * exactly the identity gives exactly the candidate's pose).
 * THE CANDIDATE LIST is passed per call and rides in the call's one upload.  An entry that is NULL, not a live keyframe handle, or without an
 * SBI, or that is one of this frame's targets (whose SBI this very call rewrites), is skipped: its score reads DBL_MAX (as mcp_sbi_score)
 * and it never wins.
 * THE CAMERA USED: the first c in order with best[c] >= 0 and align_score[c] < max_score (strict, Relocaliser.cc:84).  base_from_world =
 * cam_from_base[cam]^-1 * cam_pose[cam] (Tracker.cc:538) replaces the pose every later kernel reads.  DEVIATION: the reference stops at the
 * first camera that recovers and never makes the later cameras' SBIs; here every camera's SBI is made and evaluated, `cam` says which was used.
 * EVERYTHING ELSE is mcp_track_frame_motion's with apply = 0, word for word, started from that pose: the tracker's own SBIs are made and rolled,
 * TrackMap runs with its bookkeeping; motion->velocity returns zeros (mv6BaseVelocity = Zeros, :549).  The caller sets try_coarse and the
 * doubled coarse caps (mbJustRecoveredSoUseCoarse).
 * NOBODY RECOVERS (no candidate, or no alignment under max_score): the reference runs no TrackMap and neither does the device -- the PVS
 * kernel, behind a device-side word, marks every (row, camera) outside and all later launches see empty sets; still one wait.  recovered = 0,
 * cam = -1, base_from_world returns as given bit for bit, finder states and the count column are untouched, *record reads zeros,
 * motion->velocity returns as given; the tracker's SBIs have rolled and the relocaliser's are made.
 * Cameras past ncam report best = -1 and zeros.
 * REFUSALS (-1, mcp_last_error(), nothing enqueued, no SBI rolled, outputs untouched): mcp_track_frame_motion's; motion->apply != 0; NULL
 * recover structs; ncand < 0; NULL candidate arrays with ncand > 0; a cand_cam outside 0 .. ncam-1; a candidate pose that is not finite;
 * reloc_blur not positive and finite; reloc_iterations < 0; max_score not finite; a live candidate on another device than the table. */
typedef struct mcp_track_recover_params {
  double reloc_blur;       /* SmallBlurryImage's default, 2.5 */
  int    reloc_iterations; /* 6, Relocaliser.cc:76 */
  double max_score;        /* Relocaliser::sdRecoveryMaxScore, 1e5; the test is strict: score < max_score */
} mcp_track_recover_params;
typedef struct mcp_track_recover {
  int recovered, cam;                       /* cam = first camera index, in order, that recovered; -1 */
  int best[MCP_MAX_FRAME_CAMS];             /* index into the candidate list; -1: no candidate of this camera had an SBI (mpBestKF == NULL) */
  double best_zmssd[MCP_MAX_FRAME_CAMS];
  double se2[MCP_MAX_FRAME_CAMS][6], align_score[MCP_MAX_FRAME_CAMS];   /* as mcp_sbi_iterate; zeros when best < 0 */
  double cam_pose[MCP_MAX_FRAME_CAMS][12];  /* mse3Best of that camera; zeros when best < 0 */
  double base_from_world[12];               /* cam_from_base[cam]^-1 * cam_pose[cam]: the pose TrackMap started from; as given when !recovered */
} mcp_track_recover;
int mcp_track_frame_recover(mcp_map_points*, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                            const uint8_t* const* const* masks, const mcp_camera* cams, const mcp_camera* cams_sbi, double base_from_world[12],
                            const double* cam_from_base, const mcp_track_map_params*, mcp_track_map_result*, const mcp_track_record_params*,
                            mcp_track_record*, const mcp_track_motion_params*, mcp_track_motion*,
                            int ncand, mcp_kf* const* cand_kf, const int* cand_cam /* camera index 0..ncam-1 */,
                            const double* cand_cam_from_world /* ncand x 12 */, const mcp_track_recover_params*, mcp_track_recover*,
                            double* scores /* ncand or NULL */);
/* host restatement of the two poses (the source k_reloc_align / k_reloc_pick run, host compiler); needs no device.  Either output may be NULL.
 * Refusals (-1, outputs untouched): NULL se2, camera, or candidate pose; a bad camera; out_base_from_world wanted without cam_from_base; an
 * input that is not finite. */
int mcp_track_recover_pose_host(const double se2[6], const mcp_camera* cam_sbi, const double cam_from_world_best[12], const double cam_from_base[12],
                                double out_cam_pose[12], double out_base_from_world[12]);

/* ---- Tracker::CalcPoseUpdate's pose covariance (mm6PoseCovariance) ----------------------------------------------- src/Tracker.cc:1441, 1498-1502
 * info = sum over the found records with weight != 0 of w J^T J (J: the 2 x 6 Jacobian of the last fine iteration, rows scaled by
 * sqrt_inv_noise) + 100 I (WLS<6>::add_prior(100), get_C_inv()); cov = its pseudo-inverse (TooN SVD<6>::get_pinv, condition number 1e9: the
 * eigenvalue lambda_i is kept iff lambda_i 1e9 > lambda_max), by a cyclic Jacobi eigen-decomposition that ends after a sweep without a
 * rotation and after MCP_POSE_COV_MAX_SWEEPS sweeps at the latest.  Both are exactly symmetric; TooN order [t; w], row-major.
 * DEVIATION: the reference linearises at the pose it held before the last update; here that pose is rebuilt as exp(-mu_last) * refined (equal
 * to rounding) and the Jacobians are formed from the records as the last re-projection left them (world position, cam_derivs).
 * ORDER: records in tiles of 256 in record order, 64 at a time through a fixed butterfly, the four sums in order, the tiles in ascending order:
 * the bits depend neither on the grid nor on the run.  mcp_track_pose_cov_host walks the same order under the host compiler (no GPU). */
#define MCP_POSE_COV_MAX_SWEEPS 16
typedef struct mcp_track_pose_cov_record {
  int valid;       /* 1 filled; 0 no fine iterations ran (gate closed: nobody recovered); -1 non-finite sums: cov, eig and norm_fro are zeros */
  int n_used;      /* found records with weight != 0 */
  int rank, sweeps;   /* eigenvalues kept; sweeps that rotated */
  double info[36], cov[36], eig[6], norm_fro;   /* eig: of info, descending; norm_fro: of cov (GetCurrentCovarianceNorm's first factor) */
} mcp_track_pose_cov_record;
/* on != 0: mcp_track_map, mcp_track_map_record, mcp_track_frame_motion and mcp_track_frame_recover append the covariance's two launches behind
 * the fine iterations, in the same submission and behind the same wait; every other output keeps its bits.  Default off: no launch more. */
int mcp_track_pose_cov_enable(mcp_map_points*, int on);
/* the record of the last track call on the table: mcp_track_pose_cov's bits for that call's fine records, last weights, refined pose and
 * mu_last.  -1 + mcp_last_error() unless that call succeeded with the switch on. */
int mcp_track_pose_cov_last(const mcp_map_points*, mcp_track_pose_cov_record* out);
/* the same two kernels on the caller's arrays (weights: one per record); max_workgroups = 0: the library's choice */
int mcp_track_pose_cov(int n, const mcp_pose_point* pts, const double* weights, int ncam, const double* cam_from_base /* ncam x 12 */,
                       const double refined[12], const double mu_last[6], int max_workgroups, mcp_track_pose_cov_record* out);
int mcp_track_pose_cov_host(int n, const mcp_pose_point* pts, const double* weights, int ncam, const double* cam_from_base /* ncam x 12 */,
                            const double refined[12], const double mu_last[6], mcp_track_pose_cov_record* out);
/* for tests: the fine records, last weights and mu_last of the last successful track call on the table, as they stand on the device; *n
 * receives the count (more than cap: -1, nothing copied).  Waits for the table's stream. */
int mcp_debug_track_fine_records(const mcp_map_points*, int cap, mcp_pose_point* pts, double* weights, double mu_last[6], int* n);
/* for tests: which kernels computed the last pose iterations that mcp_track_pose_refine(_m) or mcp_track_frame ran on the calling thread's
 * current device.  *route: 0 k_pose_refine_regs, 1 k_pose_refine, 2 k_pose_refine_multi, 3 k_pose_refine_multi given up and redone by
 * k_pose_refine; *nwg: the workgroups of the multi launch (0 on routes 0 and 1); *gathered: 1 when its median went through LDS
 * (MCP_TRACK_REFINE_GATHER), else 0.  Host bookkeeping only.  -1 + mcp_last_error() before the first such call or after a failed one. */
int mcp_debug_last_pose_route(int* route, int* nwg, int* gathered);

/* ---- MapMakerServerBase::ReFind_Common over the table in ONE submission ---------------------------- src/MapMakerServerBase.cc:921-1080
 * ReFindInSingleKeyFrame (every point of the map against a new keyframe), ReFindNewlyMade (every new point against every keyframe) and
 * ReFindFromFailureQueue all run ReFind_Common per (keyframe, point) pair.  The caller keeps the early-outs that read its own sets (:925-937:
 * measurement and never-retry sets, mbBad, CrossCamera) and passes the pairs that survive them as (table row, target index).  Per pair and on
 * the device, from the row's columns (world position, pixel vectors, patch source, level, centre, key): the projection and the inclusive
 * in-image test (:941-956), MakeTemplateCoarse with the warp's verdict ignored, FindPatchCoarse with range 4, and above level 0
 * MakeSubPixTemplate + eight sub-pixel iterations whose position is kept converged or not (:958-987) -- MCP_PF_REFIND of mcp_patch_sequences,
 * the same device code.  The row's patch source is resolved per call through the registry of live keyframes; a stale source is never
 * dereferenced.  `usable` is NOT consulted (new points are not optimised yet when ReFindNewlyMade runs); the table's per-(row, camera)
 * tracker finders are neither read nor written.  Pairs are processed as given: duplicates are not detected.
 * FINDERS, exactly mcp_patch_sequences' sequences: per_row_finders = 0: every pair is its own sequence (ReFindInSingleKeyFrame, the failure
 * queue); per_row_finders = 1: each maximal run of consecutive pairs with the same row is one sequence that one finder walks in order
 * (ReFindNewlyMade: keyframes with similar warps share the point's template).  *finder enters the first sequence, every other sequence starts
 * from a zeroed state; on return *finder is the state of the last sequence after its last pair.  finder == NULL: a fresh one, nothing
 * returned.  A pair that fails the projection test (or has no source) does not touch a finder.  The point key is the row's key.
 * OUTPUTS: verdict[i] for every pair; meas (cap_meas entries) receives the FOUND pairs in ascending pair index, or -- meas == NULL -- they
 * stay in the library's pinned block (mcp_map_refind_view, valid until the next call on this table); res is always filled.  More than cap_meas
 * FOUND pairs: -1, verdicts and counts filled, meas untouched (mcp_track_find_pvs's rule).
 * ORDER: enqueued on the table's stream -- uploads and a write-back issued before it are seen whole -- one copy of the packed inputs, four
 * launches, one wait.  Targets must be on the table's device; their pyramids are those of the last mcp_kf_* call.  Any number of targets.
 * REFUSALS (-1, mcp_last_error(), nothing enqueued, outputs untouched): NULL table; negative counts; a NULL pointer with a positive count; a
 * NULL or destroyed target keyframe; a bad camera; a target on another device; a row or target index out of range. */
#define MCP_REFIND_FOUND        1   /* a Measurement was produced                                   */
#define MCP_REFIND_OUTSIDE      2   /* camera.Invalid() or outside [0,size] (:945-956)              */
#define MCP_REFIND_TEMPLATE_BAD 3   /* finder.TemplateBad() (:961-965)                              */
#define MCP_REFIND_NOT_FOUND    4   /* FindPatchCoarse failed (:968-973)                            */
#define MCP_REFIND_NO_SOURCE    5   /* row without a source, or its source keyframe was destroyed   */
/* 2..4 are what the reference puts into spNeverRetryKFs; 5 cannot occur there, is not a never-retry, and is counted */

typedef struct mcp_refind_target { mcp_kf* kf; const mcp_camera* cam; double cam_from_world[12]; } mcp_refind_target;
typedef struct mcp_refind_meas {
  int pair, row, target;      /* index into pairs[], and that pair                                 */
  int level, subpix, score;   /* Measurement::nLevel, bSubPix; nBestSSD                            */
  double root_pos[2];         /* v2RootPos, level-0 coordinates                                    */
} mcp_refind_meas;
typedef struct mcp_refind_result { int counts[6]; /* per verdict, [0] unused */ int n_meas; } mcp_refind_result;

int mcp_map_refind(mcp_map_points*, int n_targets, const mcp_refind_target* targets,
                   int n_pairs, const int* pairs /* n_pairs x (row, target) */, int per_row_finders,
                   mcp_pf_state* finder /* in/out, NULL = a fresh one and nothing returned */,
                   uint8_t* verdict /* n_pairs */, int cap_meas, mcp_refind_meas* meas /* NULL: stay in the pinned block */,
                   mcp_refind_result* res);
/* zero-copy: the measurements of the last mcp_map_refind on this table (also when it copied them out); NULL + count 0 when there are none,
 * NULL + mcp_last_error() when the last call was refused or ran over its cap */
const mcp_refind_meas* mcp_map_refind_view(const mcp_map_points*, int* count);

/* ---- The map graph on the device: MKFs, rig, per-point graph columns, the measurement store ------------ src/BundleAdjusterBase.cc:141-265
 * The table above holds the MapPoint columns; the graph holds the edges: which keyframe (MKF slot, camera index) measures which point (table
 * row), where and at which level -- KeyFrame::mmpMeasurements / MapPoint::mMMData.spMeasurementKFs as one store -- with the MKF poses, the rig
 * (one CamFromBase per camera index, as BundleAdjusterMulti adds one pose per camera name) and mbFixed / mbBad / the patch source per point.
 * A graph lives on its table's device and enqueues on its table's stream: a select that follows an mcp_ba_write_back or an
 * mcp_map_points_update sees whole rows.  THE TABLE MUST OUTLIVE THE GRAPH: destroying the table first is the caller's error (as a destroyed
 * mcp_kf is for the table's rows that name it, only that nothing guards this one).  Threading: as mcp_map_points_update -- the caller
 * serialises the calls on one table and its graph.  All poses: R row-major 9 then t 3, finite.
 * REFUSALS of every call below: -1 (NULL for create), mcp_last_error(), nothing enqueued, the graph unchanged. */
#define MCP_MAP_MAX_MKFS 4096
#define MCP_MKF_PRESENT 1     /* in Map::mlpMultiKeyFrames */
#define MCP_MKF_FIXED   2     /* MultiKeyFrame::mbFixed    */
#define MCP_MKF_BAD     4     /* MultiKeyFrame::mbBad      */
#define MCP_GP_FIXED    1     /* MapPoint::mbFixed         */
#define MCP_GP_BAD      2     /* MapPoint::mbBad -- not the table's `usable`, which is !mbBad && mbOptimized */
typedef struct mcp_map_graph mcp_map_graph;
mcp_map_graph* mcp_map_graph_create(mcp_map_points* table, int ncam /* 1..MCP_MAX_FRAME_CAMS */, const double* cam_from_base /* ncam x 12 */);
void mcp_map_graph_destroy(mcp_map_graph*);
/* MKF slots first .. first+count-1 (first + count <= MCP_MAP_MAX_MKFS) / the distinct slots[0..count): BaseFromWorld, flags (MCP_MKF_*),
 * mbActive and mdSceneDepthMean per camera index.  A slot never written is not present.  The depth mean of an active keyframe must be finite
 * and positive (others are stored as 0). */
int mcp_map_graph_set_mkfs(mcp_map_graph*, int first, int count, const double* base_from_world /* count x 12 */, const int* flags,
                           const uint8_t* kf_active /* count x ncam */, const double* kf_depth_mean /* count x ncam */);
int mcp_map_graph_update_mkfs(mcp_map_graph*, int count, const int* slots, const double* base_from_world, const int* flags,
                              const uint8_t* kf_active, const double* kf_depth_mean);
/* graph columns of the distinct table rows rows[0..count): the patch source (MKF slot, camera index) and MCP_GP_* flags.  A row never
 * written is bad.  src_mkf < 0 (no source) is allowed for fixed points only; a row past the table's size is refused.  A row written here
 * loses its pending mark (mcp_map_cull_sweep's report, below): the host knows what it writes. */
int mcp_map_graph_update_points(mcp_map_graph*, int count, const int* rows, const int* src_mkf, const int* src_cam, const int* flags);
/* appends measurements in the caller's order and returns the store index of the first new one.  uv: level-0 v2RootPos; source:
 * Measurement::eSource as an int, stored and returned, not interpreted.  The caller guarantees one entry per (mkf, cam, row), as MeasPtrMap
 * does: the library does not search for duplicates (mcp_map_graph_check says afterwards what the store holds).  Refused: a slot that is not
 * present, cam outside 0..ncam-1, a row outside the table, level outside 0..MCP_LEVELS-1, a non-finite uv.  Capacity grows geometrically. */
int mcp_map_graph_add_meas(mcp_map_graph*, int count, const int* mkf, const int* cam, const int* row, const double* uv /* count x 2 */,
                           const int* level, const int* source);
/* KeyFrame::EraseMeasurementOfPoint for the distinct keys (mkf, cam, row)[0..count): the matching live entries become dead (one thread per
 * entry, binary search in the sorted keys).  Returns how many died (waits for the stream); a key that matches nothing is not an error. */
int mcp_map_graph_erase_meas(mcp_map_graph*, int count, const int* mkf, const int* cam, const int* row);
/* every entry of that MKF dies, the slot is no longer present; returns how many died */
int mcp_map_graph_erase_mkf(mcp_map_graph*, int slot);
/* stable removal of the dead entries.  STORE INDICES CHANGE: the index mcp_map_graph_add_meas returned and the `store` field of a
 * measurement view taken before are void afterwards. */
int mcp_map_graph_compact(mcp_map_graph*);
/* read-backs; each waits for the stream.  alive: 1 / 0.  good_counts: MapPoint::mMMData.GoodMeasCount() (MapPoint.h:80-87) of table rows
 * first .. first+count-1: the live entries of the row whose MKF is present and not bad.  check: for tests and adapters under development
 * -- a host sort of the read-back keys; n_dup = live entries whose (mkf, cam, row) an earlier live entry has, n_dead = dead entries. */
int mcp_map_graph_num_meas(mcp_map_graph*, int* live, int* stored);
int mcp_map_graph_get_meas(mcp_map_graph*, int first, int count, int* mkf, int* cam, int* row, double* uv, int* level, int* source, uint8_t* alive);
int mcp_map_graph_good_counts(mcp_map_graph*, int first, int count, int* out);
int mcp_map_graph_check(mcp_map_graph*, int* n_dup, int* n_dead);

/* ---- BundleAdjustRecent / BundleAdjustAll and the population of BundleAdjusterMulti::BundleAdjust in ONE submission -----------------------
 * src/BundleAdjusterBase.cc:141-265, src/BundleAdjusterMulti.cc:81-200.  The call returns, in the library's pinned block, exactly the arrays
 * mcp_ba_add_pose / mcp_ba_add_points / mcp_ba_add_measurements and mcp_ba_write_back take.  Six launches on the table's stream, one wait.
 * RECENT: fewer present MKFs than recent_min_size -> status 1 (the caller sets mbBundleConverged_Recent).  MultiKeyFrame::Distance(newest, k)
 *   for every other present MKF k, bad ones included (KeyFrame.cc:715-747, 903-927: the minimum over the pairs of active keyframes of
 *   |dC| + mean_diff_fraction |dmean|, CamFromWorld = cam_from_base[c] * base_from_world, the mean-depth point (0,0,depth_mean) carried to the
 *   world; DBL_MAX without such a pair).  The n_recent smallest in ascending (distance, slot) are `closest`; the adjust set is the newest MKF
 *   plus those of them that are neither bad nor fixed.  A row is selected iff a live entry of an adjust-set MKF measures it, it is not bad and
 *   its good count is >= 2.
 * ALL: the adjust set is every present MKF that is not bad (its own FIXED flag travels); a row is selected iff it is not bad and (good >= 2 or
 *   it is fixed).
 * Good count: the live entries of the row whose MKF is present and not bad.  The FIXED SET is every present, not bad MKF outside the adjust set
 *   with a live entry on a bundle row, or that is the source of a non-fixed bundle row.  Points gate: fewer than min_points bundle rows ->
 *   status 2, empty views.
 * VIEWS (valid until the next select on the graph): MKFs: the adjust set in ascending slot, then the fixed set in ascending slot; points: in
 *   ascending row, x = CamFromWorld_src * world_pos[row] (the two products in that order) or, fixed, world_pos[row]; src_mkf is the index into
 *   the MKF view (-1 for a fixed point, with has_fixed_points telling the adapter to add the world pose, BundleAdjusterMulti.cc:147-149);
 *   measurements: the live entries whose row is in the bundle and whose MKF is present and not bad, in store order.
 * DEVIATIONS from the reference: (1) these orders -- the reference's are pointer orders of std::set / std::map, so any fixed order is as good,
 *   and this one makes two calls give the same bytes; (2) the slot, not the pointer, breaks a distance tie in `closest`; (3) fewer than n_recent
 *   other MKFs give a shorter list (the reference indexes past the vector's end, :208-214); (4) a selected non-fixed row whose source MKF is
 *   bad, absent or < 0 is DROPPED with its measurements and counted in n_dropped_source (the reference would hand AddPoint the id 0 that
 *   mmBase_BundleID[] default-inserts) -- everything that depends on the selection (fixed set, gate, views) is decided after this rule;
 *   (5) status 3 where the reference calls ROS_BREAK.
 * REFUSALS (-1, mcp_last_error(), nothing enqueued, the views of the last call still valid): NULL handles or structs; an unknown mode; RECENT
 *   with `newest` not present; n_recent outside 0..8; a negative gate; mean_diff_fraction not finite. */
#define MCP_BUNDLE_ALL 0
#define MCP_BUNDLE_RECENT 1
typedef struct mcp_bundle_select_params {
  int mode;              /* MCP_BUNDLE_ALL | MCP_BUNDLE_RECENT */
  int newest;            /* RECENT: slot of mlpMultiKeyFrames.back() */
  int n_recent;          /* snRecentNum (3) */
  int recent_min_size;   /* snRecentMinSize (8) */
  int min_points;        /* snMinMapPoints (10) */
  double mean_diff_fraction;   /* KeyFrame::sdDistanceMeanDiffFraction (0.5) */
} mcp_bundle_select_params;
typedef struct mcp_bundle_select_result {
  int status;            /* 0 selected; 1 map smaller than recent_min_size; 2 fewer than min_points;
                            3 an MKF distance not finite or > 1e10 (the reference stops the process, KeyFrame.cc:734-744) */
  int n_adjust, n_fixed, n_points, n_meas, has_fixed_points;
  int n_dropped_source;  /* selected points left out because their source MKF is bad or absent */
  int closest[8]; double closest_dist[8];   /* RECENT, status 0 or 2: NClosestMultiKeyFrames, before the bad / fixed filter; -1 past the end */
} mcp_bundle_select_result;
typedef struct mcp_bundle_mkf { int slot, fixed /* fixed in the bundle */; } mcp_bundle_mkf;
typedef struct mcp_bundle_point { double x[3]; int row, src_mkf /* index into the MKF view */, src_cam, fixed; } mcp_bundle_point;
typedef struct mcp_bundle_meas { double uv[2]; int mkf /* index into the MKF view */, cam, point /* index into the points view */, level, source,
                                 store /* store index */; } mcp_bundle_meas;
int mcp_map_bundle_select(mcp_map_graph*, const mcp_bundle_select_params*, mcp_bundle_select_result*);
/* device time of the last select's submission (first memset to last launch, between two events on the stream), in ms; -1 unless it ran */
int mcp_map_bundle_select_last_timing(const mcp_map_graph*, double* device_ms);
/* zero-copy: the views of the last mcp_map_bundle_select on the graph (n_adjust + n_fixed, n_points, n_meas entries); NULL + count 0 when empty */
const mcp_bundle_mkf*   mcp_map_bundle_mkfs_view(const mcp_map_graph*, int* count);
const mcp_bundle_point* mcp_map_bundle_points_view(const mcp_map_graph*, int* count);
const mcp_bundle_meas*  mcp_map_bundle_meas_view(const mcp_map_graph*, int* count);
/* the same selection from host arrays, with the same bodies under the host compiler: needs no device, and gives the bytes the device gives.
 * n_slots <= MCP_MAP_MAX_MKFS MKF columns as mcp_map_graph_set_mkfs takes them, the rig, n_rows point columns with world_pos (n_rows x 3), the
 * n_store store columns with their alive flags.  out_*: caller's arrays of cap_* entries; a view that does not fit is a refusal found before
 * anything is written (sizes n_slots / n_rows / n_store always fit).  Refusals as mcp_map_bundle_select's, outputs untouched. */
int mcp_map_bundle_select_host(const mcp_bundle_select_params*, int ncam, const double* cam_from_base,
                               int n_slots, const double* base_from_world, const int* mkf_flags, const uint8_t* kf_active, const double* kf_depth_mean,
                               int n_rows, const double* world_pos, const int* src_mkf, const int* src_cam, const int* point_flags,
                               int n_store, const int* ms_mkf, const int* ms_cam, const int* ms_row, const double* ms_uv, const int* ms_level,
                               const int* ms_source, const uint8_t* ms_alive, mcp_bundle_select_result* res,
                               int cap_mkfs, mcp_bundle_mkf* out_mkfs, int cap_points, mcp_bundle_point* out_points, int cap_meas, mcp_bundle_meas* out_meas);

/* ---- The keyframe lists from the store, and AdjustAndUpdate's write-back over the graph in ONE submission --- src/BundleAdjusterMulti.cc:286-334
 * mcp_ba_write_back and mcp_scene_depth_robust take the keyframe-major lists (seg_start / seg_rows / seg_weights) from the caller.  The calls
 * below build them on the device from the graph's store and the table's count column, and keep the graph's poses and scene-depth means in step
 * with what they write, so that a select -> solve -> write-back -> select cycle moves nothing list-sized over the link.
 * THE LISTS.  A call names n_mkfs <= MCP_MAP_MAX_MKFS distinct present slots; keyframe j = i * ncam + c is (slots[i], camera index c), ncam the
 *   graph's rig size.  List j holds, in ASCENDING STORE INDEX, the store entries that are alive, of MKF slots[i] and camera c, whose keyframe is
 *   active (kf_active; an inactive keyframe has an empty list: MultiKeyFrame::RefreshSceneDepthRobust, src/KeyFrame.cc:851-869), whose row is a
 *   row of the table and whose graph column is not MCP_GP_BAD (a row never written is bad) -- KeyFrame::GetPointDepthsAndWeights, :549-570.
 *   seg_rows = the row; seg_weights = inlier / (inlier + outlier) of the table's count column, the sum and the quotient in double (rows never
 *   set: (1, 0)).
 *   ORDER: the reference's order is a pointer order (std::map over MapPoint*); store order is the one fixed here, and it JOINS THE SUMMATION
 *   CONTRACT of mcp_scene_depth_robust above: the scene-depth kernel adds a list in list position, so one store gives one set of bits, whatever
 *   the grid.  mean / sigma differ from the reference's sorted-order sums within the bound stated at mcp_scene_depth_robust; nothing else is inexact.
 *   mcp_graph_compact keeps the order; entries appended later come later.
 * Threading and streams: as the graph's other calls (the table's stream; the caller serialises).  Each call below is one submission and one
 * wait, except the debug hook.  mcp_map_points_last_timing keeps its meaning for mcp_graph_refresh_depth and mcp_graph_write_back: the copy of
 * the packed inputs (the call's slots: no list), the chain table + point kernel, and -- as depth_ms -- the list launches, the pose and depth
 * stores and the scene-depth kernel. */

/* MultiKeyFrame::RefreshSceneDepthRobust of the named MKFs at the graph's own poses (an MKF that enters the map, src/MapMakerServerBase.cc:219,
 * 392): the lists, CamFromWorld_j = cam_from_base[c] * base_from_world(slots[i]), mcp_scene_depth_robust's kernel on them, and `mean` stored as
 * the graph's depth mean of every keyframe with refreshed == 1 and a finite positive mean (all others keep their bytes).  depth_out: NULL or
 * n_mkfs x ncam records; where refreshed == 0 only n and refreshed are written (as mcp_scene_depth_robust).  n_mkfs == 0 is allowed.
 * REFUSALS (-1, mcp_last_error(), nothing enqueued, graph and table unchanged): NULL graph; n_mkfs negative or > MCP_MAP_MAX_MKFS; a slot out of
 * range, not present, or repeated. */
int mcp_graph_refresh_depth(mcp_map_graph*, int n_mkfs, const int* slots, mcp_scene_depth* depth_out);

/* mcp_ba_write_back with the keyframe half taken from the graph.  POINTS: exactly mcp_ba_write_back's arguments, checks and kernels.
 * KEYFRAMES: keyframe j = i * ncam + c is the chain {mkf_pose_ids[i], cam_pose_ids[c]} of the bundle (pose ids as mcp_ba_add_pose returned
 * them).  On the table's stream, behind the one event on the solver's stream: the chain table, the points, the solver's current pose of
 * mkf_pose_ids[i] copied into the graph's base_from_world of slots[i] (12 doubles, bit for bit), the lists, the scene depth with the chain
 * products as poses (after the point step, as mcp_ba_write_back), and the depth-mean store of mcp_graph_refresh_depth.  One wait; the solver
 * handle may be destroyed at once.  A select that follows sees the new poses and depth means: no mcp_map_graph_update_mkfs is needed.
 * kf_cam_from_world_out: NULL or n_mkfs*ncam x 12; depth_out: NULL or n_mkfs*ncam; base_from_world_out: NULL or n_mkfs x 12.
 * CONTRACT, NOT CHECKED: the caller added the graph's rig as the poses cam_pose_ids (BundleAdjusterMulti adds one pose per camera from the same
 * CamFromBase).  Otherwise the select's distances go on using the graph's rig while the depths here use the solver's.
 * REFUSALS (-1, mcp_last_error(), nothing enqueued, graph and table unchanged): those of mcp_ba_write_back for the handles and the point half;
 * those of mcp_graph_refresh_depth for the slots; a pose id that is not a pose; a required pointer NULL with a positive count; a graph whose
 * table is not on the solver's device.  n_mkfs == 0 and n_points == 0 are allowed. */
int mcp_graph_write_back(mcp_ba*, mcp_map_graph*, int n_points, const int* point_ids, const int* rows, const int* src_chains, int chain_stride,
                         const int* src_chain_len, double* world_pos_out, double* pixel_right_out, double* pixel_down_out,
                         int n_mkfs, const int* slots, const int* mkf_pose_ids, const int* cam_pose_ids /* ncam */,
                         double* kf_cam_from_world_out, mcp_scene_depth* depth_out, double* base_from_world_out);

/* MKF slots first .. first+count-1 read back as mcp_map_graph_set_mkfs takes them (every pointer may be NULL: that column is skipped; the depth
 * mean of an inactive keyframe reads 0); waits for the stream */
int mcp_graph_get_mkfs(mcp_map_graph*, int first, int count, double* base_from_world, int* flags, uint8_t* kf_active, double* kf_depth_mean);

/* test hook, read-only: the list launches alone, the lists copied out.  blocks: how many chunks the store is cut into, 1..64, or 0 for the
 * grid the other calls use (the lists do not depend on it).  seg_start: n_mkfs*ncam + 1 entries; seg_rows / seg_weights: cap entries.  Returns
 * the total; a total above cap is refused after seg_start has been written.  Two waits. */
int mcp_graph_debug_kf_lists(mcp_map_graph*, int n_mkfs, const int* slots, int blocks, int* seg_start, int cap, int* seg_rows, double* seg_weights);

/* the same lists from host arrays, by the same bodies under the host compiler: needs no device and gives the device's bytes.  kf_active:
 * n_slots x ncam; point_flags: the n_point_rows <= n_rows graph columns written so far (the rows after them read as bad); inlier / outlier: the
 * count column, n_rows.  Returns the total; refused (outputs but seg_start untouched): the slots as above, a total above cap, a count
 * the table's column would refuse (inlier < 1 or outlier < 0). */
int mcp_graph_kf_lists_host(int ncam, int n_slots, const int* mkf_flags, const uint8_t* kf_active, int n_rows, int n_point_rows, const int* point_flags,
                            const int* inlier, const int* outlier, int n_store, const int* ms_mkf, const int* ms_cam, const int* ms_row,
                            const uint8_t* ms_alive, int n_mkfs, const int* slots, int* seg_start /* n_mkfs*ncam + 1 */, int cap, int* seg_rows, double* seg_weights);

/* ---- Measurement parcels: the tracker's and ReFind's measurements into the store without a host hop ---- src/Tracker.cc:1237-1274, src/MapMaker.cc:389-423
 * mcp_track_map_record / mcp_track_frame_motion / mcp_track_frame_recover and mcp_map_refind leave their measurements in pinned blocks that
 * kernels wrote.  A PARCEL takes such a list into device memory of its own -- with, per entry, the key (mcp_map_points_set_source) the entry's
 * row held at that moment, read on the device -- and keeps it while the tracker goes on rewriting the pinned blocks.  The COMMIT, whenever the
 * map maker gets to the MultiKeyFrame, appends the entries that are still good to a graph's store, judged by the map as it is THEN.
 * A parcel lives on its table's device and enqueues on its table's stream; THE TABLE MUST OUTLIVE IT (as it must a graph).  The caller
 * serialises the calls on one table, its graphs and its parcels.  A fill replaces the parcel's contents; capacity grows geometrically (a fill
 * that outgrows the block waits for the stream first, every other fill is enqueued without a wait).
 * ENTRY: lane = which of the commit's lanes the entry belongs to; row, level, uv (level-0 coordinates) as the store keeps them; key = the row's
 *   key when the parcel was filled.
 * from_track: the measurement lists of the last successful track call with bookkeeping on the table (the three named above), exactly the bytes
 *   mcp_track_map_meas_view shows: lane = camera index, cameras ascending, a camera's entries in item order, uv = found_pos.  The sets C, T, R of
 *   a camera are disjoint (the PVS lists a row once, C takes the smallest keys of levels 3 and 2, T and R only keys above those: k_tm_select),
 *   so (lane, row) is unique in the parcel.  ORDER: the count is the host's (the record's n_meas), the fill is one launch on the table's
 *   stream, which is the stream k_tr_scatter writes the pinned list on; a later track call rewrites the list by launches on the same stream,
 *   behind the fill -- stream order, no wait.  (A later call that has to REPLACE the pinned block by a larger one waits for the stream first.)
 *   Refused unless the last track / PVS call on the table was such a call.
 * from_refind: the FOUND pairs of the last mcp_map_refind on the table, in ascending pair index (mcp_map_refind_view's bytes): lane = target,
 *   uv = root_pos.  The same order argument holds.  Refused when that call was refused or ran over its cap.
 * from_host: the caller's arrays in the caller's order (a keyframe that arrives over the wire); the keys are gathered on the device.  Refused:
 *   a row outside the table, a level outside 0..MCP_LEVELS-1, a non-finite uv, a negative lane.
 * All three return the entry count.  get: the entries read back (waits); cap below the size is refused.
 * REFUSALS: -1 (NULL for create), mcp_last_error(), nothing enqueued, the parcel unchanged. */
typedef struct mcp_meas_parcel mcp_meas_parcel;
typedef struct mcp_parcel_entry { double uv[2]; int lane, row, key, level; } mcp_parcel_entry;   /* 32 B */
mcp_meas_parcel* mcp_meas_parcel_create(mcp_map_points* table);
void mcp_meas_parcel_destroy(mcp_meas_parcel*);
int  mcp_meas_parcel_from_track (mcp_meas_parcel*);
int  mcp_meas_parcel_from_refind(mcp_meas_parcel*);
int  mcp_meas_parcel_from_host  (mcp_meas_parcel*, int n, const int* lane, const int* row, const double* uv /* n x 2 */, const int* level);
int  mcp_meas_parcel_size(const mcp_meas_parcel*);
int  mcp_meas_parcel_get (const mcp_meas_parcel*, int cap, mcp_parcel_entry* out);

/* THE COMMIT.  lane_mkf[l] / lane_cam[l]: the MKF slot and camera index lane l's entries are measurements of; lane_mkf[l] < 0 withholds the lane
 * (an inactive camera, a ReFind target the caller leaves out; its lane_cam is not looked at).  Entry e gets the first verdict that applies:
 *   MCP_PARCEL_SKIPPED  lane_mkf[e.lane] < 0
 *   MCP_PARCEL_STALE    e.row is past the table's rows, or the row's key is no longer e.key: the row was recycled for another point (nothing of
 *                       the new point is read beyond its key)
 *   MCP_PARCEL_BAD      the row's graph column is MCP_GP_BAD (a row never written is bad): td.mPoint.mbBad in RecordMeasurements and the sweep
 *                       of AddMultiKeyFrameFromTopOfQueue (src/MapMaker.cc:407-418)
 *   MCP_PARCEL_CROSS    !cross_camera and the row has no source MKF or its source camera is not lane_cam[e.lane] (src/Tracker.cc:1256)
 *   MCP_PARCEL_APPENDED otherwise: the store entry {uv, lane_mkf, lane_cam, row, level, params.source, alive} goes to store index
 *                       first + (its position among the appended entries in parcel order).
 * The five counters sum to the parcel's size; lane_appended[l] (NULL, or n_lanes ints) counts the appended entries per lane.  The appended
 * bytes are those mcp_map_graph_add_meas stores for the same surviving entries in the same order; as there, the caller guarantees that no
 * (mkf, cam, row) is in the store already.  The store is grown to hold every entry of the parcel before anything is enqueued; then one copy of
 * the lane tables, two launches on the table's stream, one wait.  A committed parcel is marked: committing it again without a refill is refused.
 * An empty parcel commits with nothing enqueued.
 * REFUSALS (-1, mcp_last_error(), graph, store and parcel unchanged): NULL handles or structs; a parcel of another table; a parcel never
 * filled or committed already; n_lanes < 0 or lane tables NULL with n_lanes > 0; an entry whose lane is >= n_lanes (a host fill's largest lane
 * is known to the host and refused before anything is enqueued; a device fill's is read back with the result -- the launches then append
 * nothing); a lane_mkf >= 0 that is not a present slot, or whose lane_cam is outside the rig; a store that would pass INT_MAX. */
#define MCP_PARCEL_APPENDED 0
#define MCP_PARCEL_SKIPPED  1
#define MCP_PARCEL_STALE    2
#define MCP_PARCEL_BAD      3
#define MCP_PARCEL_CROSS    4
typedef struct mcp_parcel_commit_params { int cross_camera; /* GVar CrossCamera (1) */ int source; /* Measurement::eSource, stored as given */ } mcp_parcel_commit_params;
typedef struct mcp_parcel_commit_result { int first, n_appended, n_skipped_lane, n_stale, n_bad, n_cross; } mcp_parcel_commit_result;
typedef struct mcp_store_entry { double uv[2]; int mkf, cam, row, level, source, alive; } mcp_store_entry;   /* a store entry as the device holds it, 40 B */
int mcp_meas_parcel_commit(mcp_map_graph*, mcp_meas_parcel*, int n_lanes, const int* lane_mkf, const int* lane_cam,
                           const mcp_parcel_commit_params*, mcp_parcel_commit_result*, int* lane_appended /* n_lanes or NULL */);

/* the same verdicts from host arrays, by the same body under the host compiler: needs no device and gives the device's bytes.  keys: the
 * table's key column now, n_rows; point_flags / src_mkf / src_cam: the n_point_rows <= n_rows graph columns written so far (rows after them
 * read as bad).  verdict: NULL or n bytes; appended: NULL or room for n records (the appended ones, in order); res->first = first.  Returns
 * n_appended.  Refused (outputs untouched): negative counts, a NULL array with a positive count, an entry lane outside 0..n_lanes-1. */
int mcp_parcel_commit_host(int n, const mcp_parcel_entry* entries, int n_rows, const int* keys, int n_point_rows, const int* point_flags,
                           const int* src_mkf, const int* src_cam, int n_lanes, const int* lane_mkf, const int* lane_cam,
                           const mcp_parcel_commit_params*, int first, uint8_t* verdict, mcp_store_entry* appended,
                           mcp_parcel_commit_result* res, int* lane_appended /* n_lanes or NULL */);

/* ---- Outliers and bad points on the device ---------------- src/MapMakerServerBase.cc:1198-1238, src/MapMakerClientBase.cc:73-108, src/Map.cc:93-116
 * What the map maker does with an adjustment's outliers (MapMakerServerBase::HandleOutliers) and the point half of MapMaker::HandleBadEntities
 * (MarkDanglersAsBad, MarkOutliersAsBad, Map::MoveBadPointsToTrash), over what the graph and its table hold already: the store with `source`
 * and `alive`, the MKF flags, the point flags, the table's (inlier, outlier) column and its `usable` byte.  What comes back is outlier-sized or
 * bad-point-sized, never map-sized.  The graph's conventions hold: the table's stream, the caller serialises, every result an integer, counts
 * per workgroup and ranks by index, so nothing depends on the order workgroups are dispatched in.  Only these calls read a meaning into the
 * store's `source`: Measurement::eSource (include/mcptam/KeyFrame.h:109); every other call stores and returns it as given.
 * REFUSALS of every call below: -1 (NULL for the view), mcp_last_error(), nothing enqueued, graph, store and table unchanged, outputs untouched. */
#define MCP_SRC_TRACKER  0
#define MCP_SRC_REFIND   1
#define MCP_SRC_ROOT     2
#define MCP_SRC_TRAIL    3
#define MCP_SRC_EPIPOLAR 4

/* HandleOutliers.  keys (mkf slot, cam, row)[0..n) in the order the solver listed its outliers (mcp_ba_get_outliers, decoded by the adapter).
 * THE ORDER MATTERS: the reference re-reads GoodMeasCount() after every erasure, so entry i is judged on the state entries 0..i-1 left.  Good
 * count: mcp_map_graph_good_counts' -- the live entries of the row whose MKF is present and not bad.  Entry i gets the first verdict that applies:
 *   MCP_CULL_MISSING      no live store entry has the key; or the row is outside the table or was never written, or the slot is not present.
 *                         No effect.  (DEVIATION: the reference would dereference the NULL that kf.mmpMeasurements[&point] default-inserts.)
 *   MCP_CULL_FIXED        the row is MCP_GP_FIXED.  No effect; n_fixed_rows counts the distinct such rows (spFixedOutliers).
 *   MCP_CULL_POINT_BAD    the row's good count is <= bad_good_count, or the entry's source is MCP_SRC_ROOT -- whether or not the row is bad
 *                         already (:1216-1220).  The row's column gets MCP_GP_BAD; the entry stays alive, as in the reference: the sweep erases it.
 *   MCP_CULL_RETRY        the row is not bad and the source is MCP_SRC_TRACKER or MCP_SRC_EPIPOLAR.  The entry dies; the row's good count drops
 *                         by one iff the entry's MKF is present and not bad.  (The adapter puts the pair on mlFailureQueue.)
 *   MCP_CULL_NEVER_RETRY  the row is not bad and the source is anything else.  As RETRY.  (The adapter inserts the keyframe into spNeverRetryKFs.)
 *   MCP_CULL_ALREADY_BAD  otherwise.  No effect.
 * verdict_out: NULL or n bytes.  The six counters sum to n; n_rows_marked: the distinct rows this call turned from not bad to bad (they are
 * reported by the next sweep).  A row never written reads (no source, bad, not fixed), which mcp_map_graph_update_points refuses to write: that
 * is how it is told.  The caller guarantees one live entry per key, as for mcp_map_graph_add_meas; of several, the one stored last is judged.
 * SHAPE: one copy of the packed keys (sorted by key with their list index for the match; sorted by (row, list index) for the walk), three
 * launches on the table's stream, one wait: k_mg_edges_count (the good counts), k_mgc_match (one thread per store entry, binary search in the
 * sorted keys), k_mgc_judge (one thread per row that has outliers walks them in list order -- rows are independent, only the walk within a row
 * is serial -- and tallies).  The launch boundaries are the grid-wide facts: matches and good counts are complete before a row is judged.
 * n == 0 enqueues nothing.
 * REFUSED: NULL graph, params or result; n < 0; a NULL key array with n > 0; a negative bad_good_count; a cam outside the rig; a slot outside
 * 0..MCP_MAP_MAX_MKFS-1; a repeated key (the solver lists a measurement once). */
#define MCP_CULL_MISSING      0
#define MCP_CULL_FIXED        1
#define MCP_CULL_POINT_BAD    2
#define MCP_CULL_RETRY        3
#define MCP_CULL_NEVER_RETRY  4
#define MCP_CULL_ALREADY_BAD  5
typedef struct mcp_cull_outliers_params { int bad_good_count; /* 2: GoodMeasCount() <= 2, src/MapMakerServerBase.cc:1216 */ } mcp_cull_outliers_params;
typedef struct mcp_cull_outliers_result { int n_missing, n_fixed, n_point_bad, n_retry, n_never_retry, n_already_bad, n_fixed_rows, n_rows_marked; } mcp_cull_outliers_result;
int mcp_map_cull_outliers(mcp_map_graph*, int n, const int* mkf, const int* cam, const int* row, const mcp_cull_outliers_params*,
                          uint8_t* verdict_out /* n or NULL */, mcp_cull_outliers_result*);

/* THE SWEEP: danglers, tracker outliers, bad points to the trash.  Over every row of the table whose graph column is not bad, in this order:
 *   danglers          only if params.danglers and at least two MKF slots are present (bad ones count: the adapter has erased the trashed MKFs
 *                     with mcp_map_graph_erase_mkf before, as HandleBadEntities does first): a row that is not fixed with good count < 2 goes bad
 *   tracker outliers  a row that is not fixed with outlier > min_outliers and outlier > inlier * outlier_multiplier (the table's count column;
 *                     the product and the comparison in double, as the reference's int * double) goes bad
 * Then for every bad row, whoever marked it (a row never written is bad): its live store entries die (MapPoint::EraseAllMeasurements) and the
 * `usable` byte of its table row is cleared, so mcp_track_find_pvs drops it without a table upload.
 * REPORT: mcp_map_cull_rows_view gives, in pinned memory and ascending row, the rows THE DEVICE turned bad since the last sweep -- by
 * mcp_map_cull_outliers calls since then and by this sweep; the host moves exactly these MapPoints to the trash.  Rows the host marked bad itself
 * through mcp_map_graph_update_points it knows already: they are swept, not reported.  The graph keeps a pending mark per row for this (the
 * fourth word of the row's graph column): set by mcp_map_cull_outliers, cleared by the sweep once the report is built and by
 * mcp_map_graph_update_points for the rows it writes, so a row recycled for a new point starts clean.  A row never written is never reported.
 * The view is valid until the next sweep on the graph; NULL + count 0 when nothing is reported.
 * n_danglers + n_tracker_outliers: the rows this call marked (a row that is both counts as a dangler); n_bad_rows: every bad row of the table
 * after the marks; n_meas_erased: the entries that died.  One submission (three launches: good counts, rows, report + store) and one wait; the
 * good counts and the row marks are complete before a store entry is judged; the report is compacted by rank (mg_rank).
 * REFUSED: NULL handles or structs; a negative min_outliers; a multiplier that is not finite. */
typedef struct mcp_cull_sweep_params {
  int min_outliers;            /* MapMakerClientBase::snMinOutliers (20) */
  int danglers;                /* 1: run MarkDanglersAsBad */
  double outlier_multiplier;   /* MapMakerClientBase::sdOutlierMultiplier (1.0) */
} mcp_cull_sweep_params;
typedef struct mcp_cull_sweep_result { int n_danglers, n_tracker_outliers, n_reported, n_bad_rows, n_meas_erased; } mcp_cull_sweep_result;
int mcp_map_cull_sweep(mcp_map_graph*, const mcp_cull_sweep_params*, mcp_cull_sweep_result*);
const int* mcp_map_cull_rows_view(const mcp_map_graph*, int* count);
/* device time in ms of the last mcp_map_cull_outliers / mcp_map_cull_sweep submission on the graph (between two events on the stream, as
 * mcp_map_bundle_select_last_timing); -1 for a call that has not run (or, outliers, whose last call had n == 0).  Either pointer may be NULL. */
int mcp_map_cull_last_timing(const mcp_map_graph*, double* outliers_ms, double* sweep_ms);

/* the same two calls from host arrays, by the same bodies under the host compiler: they need no device and give the device's bytes.  MKF flags
 * as mcp_map_bundle_select_host takes them (n_slots <= MCP_MAP_MAX_MKFS); the n_point_rows <= n_rows graph columns written so far as
 * mcp_graph_kf_lists_host takes them (rows after them read as never written); the store columns with their alive flags.  IN PLACE: point_flags,
 * pending (n_point_rows bytes), ms_alive, usable (n_rows bytes).  inlier / outlier: the count column, n_rows.  rows_out: room for cap_rows rows;
 * a report that does not fit is a refusal found before anything is written (n_rows always fits).  mcp_map_cull_sweep_host returns n_reported.
 * Refusals as the device calls', plus negative counts, a NULL array with a positive count, n_point_rows > n_rows, n_slots > MCP_MAP_MAX_MKFS. */
int mcp_map_cull_outliers_host(int n, const int* mkf, const int* cam, const int* row, const mcp_cull_outliers_params*, int ncam,
                               int n_slots, const int* mkf_flags, int n_rows, int n_point_rows, const int* src_mkf, int* point_flags, uint8_t* pending,
                               int n_store, const int* ms_mkf, const int* ms_cam, const int* ms_row, const int* ms_source, uint8_t* ms_alive,
                               uint8_t* verdict_out /* n or NULL */, mcp_cull_outliers_result*);
int mcp_map_cull_sweep_host(const mcp_cull_sweep_params*, int n_slots, const int* mkf_flags, int n_rows, int n_point_rows, int* point_flags,
                            uint8_t* pending, const int* inlier, const int* outlier, uint8_t* usable, int n_store, const int* ms_mkf,
                            const int* ms_row, uint8_t* ms_alive, mcp_cull_sweep_result*, int cap_rows, int* rows_out);

/* ---- Closest-keyframe queries and the removal of an MKF on the device ---- src/MapMakerBase.cc:90-339, src/MapMakerClientBase.cc:111-226,
 *                                                                           src/MapMakerServerBase.cc:264-318, src/Map.cc:119-187
 * ONE CALL for ClosestKeyFrame, ClosestKeyFramesWithinDist, NClosestKeyFrames, ClosestMultiKeyFrame, NClosestMultiKeyFrames and
 * FurthestMultiKeyFrame over the graph's own columns (poses, active bytes, depth means, flags, the store): at most MCP_NB_MAX items come back,
 * never a map-sized array.  The graph's conventions hold: the table's stream, the caller serialises, one wait, every atomic adds or ors an
 * integer, nothing depends on the order workgroups are dispatched in.
 * SOURCE: src_slot >= 0, a present slot; or -1, the external MKF of the params (the tracker's current MKF, which is not in the map): its pose,
 *   active bytes and depth means as mcp_map_graph_set_mkfs takes one entry.  KF kind: the source keyframe is (source, src_cam).
 * CANDIDATES, MKF kind: every present slot other than src_slot, bad ones included (the reference walks mlpMultiKeyFrames); `flags` travels
 *   with an item so that the adapter can skip them after the list is cut, as AddStereoMapPoints does.
 * CANDIDATES, KF kind: every (slot, cam) of a present slot with kf_active[cam] set, other than the source keyframe itself.  MCP_NB_ONLY_SELF:
 *   the other keyframes of the source's own MKF; MCP_NB_ONLY_OTHER: every MKF but the source's; same_cam: cam == src_cam.  With src_slot == -1
 *   the own MKF is the external one: its siblings are candidates (slot -1, cam) with its pose, active bytes and depths.
 * DISTANCE: KeyFrame::Distance / MultiKeyFrame::Distance (src/KeyFrame.cc:715-747, 903-927) exactly as mcp_map_bundle_select computes them,
 *   CamFromWorld = cam_from_base[c] * base_from_world.  An MKF pair without a pair of active keyframes gives DBL_MAX: a candidate like any
 *   other, not an error.  A distance that is not finite or > 1e10 (the value the reference stops the process on) gives status 3 and count 0.
 * ORDER: MCP_NB_NEAREST ascending (dist, slot, cam), MCP_NB_FURTHEST descending dist with ties to the smaller (slot, cam), where a candidate
 *   at distance 0 is never furthest (FurthestMultiKeyFrame starts at 0 and compares with >).  Of these the ones with dist <= max_dist are
 *   kept (+inf: all), and of those the first n_max.  count may be 0: a result, not an error.  n_candidates: the candidates before max_dist.
 * n_meas (want_meas): the alive store entries whose mkf is the item's slot (MKF kind: MultiKeyFrame::NumMeasurements) or whose (mkf, cam) is
 *   the item's keyframe (KF kind: mmpMeasurements.size()); counted for the `count` winners only; -1 without want_meas; items past count: zeros.
 * DEVIATIONS: (1) the graph's only record that a keyframe exists is kf_active; inactive keyframes are deleted before an MKF enters the map
 *   (ProcessIncomingKeyFrames), so this is the reference's set.  (2) slot and cam break ties where the reference's partial_sort compares
 *   pointers.  (3) max_dist applies under MCP_NB_FURTHEST too (the reference has no such query).
 * SHAPE: k_mgn_dist (a grid over (slot, cam): one candidate per thread, its distance and candidate byte into a scratch the graph owns -- the
 *   32768 + 8 keyframes do not fit a workgroup's LDS), k_mgn_select (one workgroup, at most n_max rounds of a strided arg-min / arg-max with
 *   an LDS tree, the winner marked taken), with want_meas k_mgn_count (one thread per store entry, a ballot per winner, lane 0 adds).
 * REFUSALS (-1, mcp_last_error() starting "mcp_map_neighbours", nothing enqueued, outputs untouched): NULL graph, params or result; unknown
 *   kind / region / order; src_slot neither -1 nor a present slot; KF kind: src_cam outside the rig, or the source keyframe not active;
 *   MCP_NB_ONLY_SELF with same_cam; n_max outside 1..MCP_NB_MAX; max_dist NaN or negative; mean_diff_fraction not finite; an external pose
 *   or active depth that is not finite, an active depth that is not positive. */
#define MCP_NB_MKF 0          /* MultiKeyFrame::Distance: the minimum over the pairs of active keyframes      */
#define MCP_NB_KF  1          /* KeyFrame::Distance from keyframe (source, src_cam) to every other keyframe   */
#define MCP_NB_ALL        0   /* KeyFrameRegion (KF kind): KF_ALL, KF_ONLY_SELF, KF_ONLY_OTHER                */
#define MCP_NB_ONLY_SELF  1
#define MCP_NB_ONLY_OTHER 2
#define MCP_NB_NEAREST  0
#define MCP_NB_FURTHEST 1
#define MCP_NB_MAX 32
typedef struct mcp_neigh_params {
  int kind, region, order;
  int src_slot;                /* >= 0: a present slot; -1: the external MKF below */
  int src_cam;                 /* KF kind */
  int same_cam;                /* KF kind: only candidates with cam == src_cam (bSameCamName) */
  int n_max;                   /* 1..MCP_NB_MAX */
  int want_meas;               /* 1: fill n_meas of every item */
  double max_dist;             /* keep dist <= max_dist; +inf: no threshold */
  double mean_diff_fraction;   /* KeyFrame::sdDistanceMeanDiffFraction */
  double ext_base_from_world[12]; uint8_t ext_active[MCP_MAX_FRAME_CAMS]; double ext_depth_mean[MCP_MAX_FRAME_CAMS];
} mcp_neigh_params;
typedef struct mcp_neigh_item { double dist; int slot, cam /* -1: MKF kind */, flags /* MCP_MKF_* of the slot; 0 for slot -1 */, n_meas; } mcp_neigh_item;
typedef struct mcp_neigh_result { int status /* 0; 3 */, count, n_candidates, pad_; mcp_neigh_item item[MCP_NB_MAX]; } mcp_neigh_result;
int mcp_map_neighbours(mcp_map_graph*, const mcp_neigh_params*, mcp_neigh_result*);
/* device time in ms of the last mcp_map_neighbours submission on the graph (two events on the stream); -1 before the first that ran */
int mcp_map_neighbours_last_timing(const mcp_map_graph*, double* device_ms);
/* the same query from host arrays by the same bodies under the host compiler (no device; the device's bytes): the rig, n_slots MKF columns as
 * mcp_map_bundle_select_host takes them, the store's mkf / cam / alive columns (read with want_meas only). */
int mcp_map_neighbours_host(const mcp_neigh_params*, int ncam, const double* cam_from_base, int n_slots, const double* base_from_world,
                            const int* mkf_flags, const uint8_t* kf_active, const double* kf_depth_mean,
                            int n_store, const int* ms_mkf, const int* ms_cam, const uint8_t* ms_alive, mcp_neigh_result*);

/* THE REMOVAL OF AN MKF: MarkFurthestMultiKeyFrameAsBad (src/MapMakerServerBase.cc:264-318) and the MKF half of HandleBadEntities
 * (Map::MoveBadMultiKeyFramesToTrash / MoveDeletedMultiKeyFramesToTrash) in one submission.
 *   victim      params.slot, or with slot == -1 the MCP_NB_FURTHEST MKF from furthest_from (the query above, MKF kind, n_max 1); without one
 *               (no other MKF at a distance > 0) status is 1 and nothing changes; a broken distance: status 3 and nothing changes.
 *   the marks   the victim gets MCP_MKF_BAD.  With mark_points, a row of the written graph columns with a live entry of the victim goes bad
 *               if (a) it is not fixed and its live entries (every one, whatever its MKF's flags: spMeasurementKFs.size()) number <= max_kfs,
 *               or (b) its patch source is that very keyframe (src_mkf == victim and src_cam == the entry's cam).  Such a row gets MCP_GP_BAD
 *               and the pending mark, so the next mcp_map_cull_sweep reports it, erases its entries and clears its usable byte, as it does
 *               for the rows of mcp_map_cull_outliers.  The counts are those on entry (the reference erases nothing inside its loop), so the
 *               rule does not depend on any order.  n_rows_marked: rows turned from not bad to bad; n_by_source: those of them for which
 *               (b) holds; n_by_count: the others.  A row that was bad already counts nowhere and keeps its pending state.
 *   the fixed   if the victim is MCP_MKF_FIXED, the nearest other present MKF to it (MCP_NB_NEAREST, MKF kind, bad included, as
 *               ClosestMultiKeyFrame) gets MCP_MKF_FIXED; new_fixed names it, -1 if there is none or the victim is not fixed.  (A broken
 *               distance in that query matters only then: status 3, nothing changes.)
 *   the erase   then, with erase, the victim's live entries die and the slot leaves the map: what mcp_map_graph_erase_mkf does.
 * SHAPE: [slot == -1: k_mgn_dist, k_mgn_select] k_mgn_dist, k_mgn_select (the hand-over, its source read from the device), k_mgn_decide (one
 * thread: victim, status, the MKF flags), [mark_points: k_mgn_rows_count: the live entries per row by integer atomicAdd, the rows whose
 * source keyframe is the victim's], k_mgn_mark (one thread per store entry: atomicOr on the row's flag word, whoever sees the old value
 * without MCP_GP_BAD counts the row), [erase: k_mg_erase]; one wait.
 * REFUSALS (-1, mcp_last_error() starting "mcp_map_mkf_cull", nothing enqueued, graph and outputs untouched): NULL graph, params or result; a
 * victim or furthest_from that is not a present slot; a negative max_kfs; mean_diff_fraction not finite. */
typedef struct mcp_mkf_cull_params {
  int slot;                    /* >= 0: the victim; -1: FurthestMultiKeyFrame(furthest_from) */
  int furthest_from;           /* used when slot == -1 */
  int mark_points;             /* 1: the point rule of MarkFurthestMultiKeyFrameAsBad; 0: only trash the MKF (mbDeleted) */
  int max_kfs;                 /* 2: spMeasurementKFs.size() <= 2 */
  int erase;                   /* 1: the victim's entries die and the slot leaves the map, after the marks */
  double mean_diff_fraction;
} mcp_mkf_cull_params;
typedef struct mcp_mkf_cull_result {
  int status /* 0; 1: no victim; 3: broken distance */, victim /* -1 unless status 0 */, victim_dist_valid /* 1 when slot was -1 */; double victim_dist;
  int n_victim_meas, n_rows_marked, n_by_count, n_by_source, new_fixed, n_meas_erased;
} mcp_mkf_cull_result;
int mcp_map_mkf_cull(mcp_map_graph*, const mcp_mkf_cull_params*, mcp_mkf_cull_result*);
/* device time in ms of the last mcp_map_mkf_cull submission on the graph; -1 before the first that ran */
int mcp_map_mkf_cull_last_timing(const mcp_map_graph*, double* device_ms);
/* the same from host arrays, IN PLACE (mkf_flags, point_flags, pending, ms_alive), as mcp_map_cull_outliers_host takes them plus the MKF pose,
 * active and depth columns. */
int mcp_map_mkf_cull_host(const mcp_mkf_cull_params*, int ncam, const double* cam_from_base, int n_slots, const double* base_from_world, int* mkf_flags,
                          const uint8_t* kf_active, const double* kf_depth_mean, int n_rows, int n_point_rows, const int* src_mkf, const int* src_cam,
                          int* point_flags, uint8_t* pending, int n_store, const int* ms_mkf, const int* ms_cam, const int* ms_row, uint8_t* ms_alive,
                          mcp_mkf_cull_result*);

/* ---- The co-visible points of the nearest keyframe ---------------------------- src/Tracker.cc:1785-1854, src/MapMakerBase.cc:115-140
 * Tracker::CollectNearestPoints with tracker_collect_all_points false: the map keyframe closest to the current keyframe, every keyframe that
 * measures one of its points, every point one of those measures.  One collection serves all cameras of a frame: a mark is a byte whose bit c
 * belongs to frame camera c; bits past the camera count are never set.
 *   nearest     per used camera c: CamFromWorld = cam_from_base[c] * base_from_world; the candidates are every (slot, cam) of a present slot
 *               with kf_active[cam] set, bad MKFs included (the reference walks mlpMultiKeyFrames; the tracker's own MKF is not in the map);
 *               KeyFrame::Distance with the map keyframe's CamFromWorld from the graph's rig, its stored depth mean, depth_mean[c] and
 *               mean_diff_fraction; the winner is the smallest by ascending (dist, slot, cam).  status[c]: 0 a winner; 1 no candidate (the
 *               reference asserts; here the set is empty); 3 some candidate's distance is not finite or exceeds 1e10 (the reference stops
 *               the process; here the set is empty).  nearest_slot / nearest_cam are -1 and nearest_dist 0 unless status is 0.
 *   the walk    over the store entries that count (alive, row inside the table, MKF a slot, camera below MCP_MAX_FRAME_CAMS):
 *               seed[row] |= bit c where the entry is camera c's winner's; kf_mark[mkf, cam] |= seed[row]; near[row] |= kf_mark[mkf, cam].
 *               Two hops, not three.  n_seed_rows, n_kfs, n_rows: per camera the marks of seed, kf_mark and near with bit c.
 * SHAPE: one memset of the marks, then k_mgcl_nearest (one workgroup per camera), k_mgcl_seed, k_mgcl_kfs, k_mgcl_rows (one thread per store
 * entry each), k_mgcl_counts (one workgroup) on the table's stream; every atomic ors an integer, so two runs give the same bytes.
 * DEVIATIONS from the reference: ties go to the smaller (slot, cam), not to list order; status 1 and 3 instead of an assert and a stop; the
 * set is computed once per frame for all cameras.
 *
 * mcp_map_collect_nearest is the stand-alone call (one submission, one wait): cam_from_base NULL means the graph's rig, otherwise ncam x 12
 * (ncam the graph's); near, if given, receives one byte per table row.  mcp_map_collect_rows_view returns the same mask zero-copy from the
 * pinned block; it stays valid until the next collection on the graph (a frame's included: NULL after one of those).
 * REFUSALS (-1, mcp_last_error() starting with the entry's name, nothing enqueued, outputs and mode untouched): NULL handles or structs; a graph
 * whose table is not this table; a frame whose camera count differs from the graph's; mean_diff_fraction not finite; a used camera's depth
 * mean that is not finite or not positive; a non-finite pose or CamFromBase in the stand-alone call. */
typedef struct mcp_collect_params {
  double mean_diff_fraction;                      /* KeyFrame::sdDistanceMeanDiffFraction */
  double depth_mean[MCP_MAX_FRAME_CAMS];          /* mdSceneDepthMean of the current keyframes: finite, > 0 for every camera used */
  uint8_t active[MCP_MAX_FRAME_CAMS];             /* stand-alone call: cameras to collect for; the frame mode uses all ncam */
} mcp_collect_params;
typedef struct mcp_collect_report {
  int valid;                                      /* 1 filled; 0 the stages did not run (a recovery frame where nobody recovered) */
  int status[MCP_MAX_FRAME_CAMS];                 /* 0, 1, 3 as above; cameras not used: 0 with nearest -1 */
  int nearest_slot[MCP_MAX_FRAME_CAMS], nearest_cam[MCP_MAX_FRAME_CAMS]; int pad_; double nearest_dist[MCP_MAX_FRAME_CAMS];
  int n_candidates[MCP_MAX_FRAME_CAMS], n_seed_rows[MCP_MAX_FRAME_CAMS], n_kfs[MCP_MAX_FRAME_CAMS], n_rows[MCP_MAX_FRAME_CAMS];
} mcp_collect_report;
int mcp_map_collect_nearest(mcp_map_graph*, const double base_from_world[12], const double* cam_from_base, const mcp_collect_params*,
                            mcp_collect_report*, uint8_t* near);
const uint8_t* mcp_map_collect_rows_view(const mcp_map_graph*, int* count);
/* device time in ms of the collection launches of the last collection on the graph, stand-alone or a frame's; -1 before the first that ran */
int mcp_map_collect_last_timing(const mcp_map_graph*, double* device_ms);
/* the same from host arrays by the same bodies under the host compiler (no device; the device's bytes): the pose, the current keyframes'
 * CamFromBase (NULL: the rig's), the rig, n_slots MKF columns as mcp_map_bundle_select_host takes them, n_rows, the store's columns. */
int mcp_map_collect_nearest_host(const double base_from_world[12], const double* cur_cam_from_base, const mcp_collect_params*, int ncam,
                                 const double* cam_from_base, int n_slots, const double* mkf_base_from_world, const int* mkf_flags,
                                 const uint8_t* kf_active, const double* kf_depth_mean, int n_rows, int n_store, const int* ms_mkf,
                                 const int* ms_cam, const int* ms_row, const uint8_t* ms_alive, mcp_collect_report*, uint8_t* near);
/* THE FRAME MODE.  mcp_track_collect_nearest(table, graph, params) switches it on for the table (graph NULL: off; params then ignored):
 * host-only, nothing enqueued, cheap enough to call before every frame with fresh depth means.  While it is on, mcp_track_find_pvs,
 * mcp_track_map, mcp_track_map_record, mcp_track_frame_motion and mcp_track_frame_recover run the collection stages in front of their PVS
 * launch, on the same stream and behind the same wait, at the pose that launch reads (the given pose, k_motion_prior's, or k_reloc_pick's
 * behind the gate), with the frame's own cam_from_base for the current keyframes and the graph's rig for the map's; a row is judged for
 * camera c only if bit c of near[row] is set, in addition to its usable byte.  Every other stage of the frame is unchanged.  Default off:
 * no launch more, and the bits of before.  mcp_map_graph_destroy switches the mode off on its table if it names the graph destroyed.
 * mcp_track_collect_last gives the report of the last such call; -1 unless that call succeeded with the mode on. */
int mcp_track_collect_nearest(mcp_map_points*, mcp_map_graph*, const mcp_collect_params*);
int mcp_track_collect_last(const mcp_map_points*, mcp_collect_report*);

/* ---- AddStereoMapPoints into the map: new points and their measurements stay on the device ------- src/MapMakerServerBase.cc:452-496, 855-914
 * mcp_stereo_points (above) hands every created point back to the host, which then sends the same numbers up again through
 * mcp_map_points_update, _update_rays, _update_source, mcp_map_graph_update_points and mcp_map_graph_add_meas.  mcp_stereo_map_points is the
 * one-call form for one source keyframe and level: it creates the points exactly as mcp_stereo_points does -- candidates, targets, limit, keep,
 * outcome, the created set and its order are that call's, byte for byte -- and leaves each of them in the table's columns, the graph's point
 * columns and the store, with one host wait.  Rows are the host's to assign, so it hands in a list of free rows and their keys up front:
 * created point k (creation order) takes rows[k] and keys[k]; the host learns `made` from the one wait.
 *
 * BUSY POSITIONS.  busy_from_store = 1: ThinCandidates' measurement list is every live store entry with (mkf, cam) == (src_mkf, src_cam), as
 * {uv, level}, gathered on the device in store order (per-workgroup counts, then ranks by index: deterministic); n_busy is its length; the level
 * filter (level, level + 1) stays in the thinning; meas / n_meas must be NULL / 0.  busy_from_store = 0: the caller's meas[], n_busy = n_meas.
 *
 * APPEND.  Row rows[k] holds afterwards what the five calls above would have written for point k: world_pos / pixel_right_w / pixel_down_w
 * from the record, usable 0 (mbOptimized is false until an adjustment); the patch rays; the source src at `level`, centre = the candidate's
 * level position, fixed 0, key keys[k] -- and, as a key change does in mcp_map_points_update_source, every camera's finder state of the row
 * zeroed when the key differs from the row's; the graph columns (src_mkf, src_cam, flags 0), pending mark cleared.  It also holds the counts
 * (1, 0) of a MapPoint that has just been constructed, which a fresh row has anyway and the owner of the table sets for a recycled one.  Two
 * store entries follow, in the order of the reference's AddMeasurement calls (:901-902), t = the record's target:
 *   first_store + 2k      {root_pos,   src_mkf,       src_cam,       rows[k], level, MCP_SRC_ROOT,     alive}
 *   first_store + 2k + 1  {target_pos, target_mkf[t], target_cam[t], rows[k], level, MCP_SRC_EPIPOLAR, alive}
 * Rows rows[made .. n_rows) are untouched and stay the caller's.  out, when not NULL, receives the records as mcp_stereo_points returns them.
 * As with mcp_map_graph_add_meas, the caller guarantees that no live store entry names a row it hands in.
 *
 * SHAPE.  Before anything is enqueued the table is grown to cover the largest row, the rays column is switched on, the graph's point columns
 * are grown and the store is grown by 2 * n_rows (through the graph's grow-when-idle rule).  The whole submission goes on the TABLE's stream,
 * behind an event recorded on the source keyframe's stream (as mcp_track_map reads keyframes); the scratch is the source's, the busy list the
 * graph's.  [busy_from_store: k_sa_busy_mark, k_sa_busy_gather, k_sa_thin_busy | k_stereo_thin_meas], per target [k_stereo_thin_new,]
 * k_stereo_walk, k_stereo_commit -- mcp_stereo_points' kernels, unchanged -- then k_sa_append (one thread per created point, the record read
 * once from the pinned block) and ONE wait; a later call on the table's stream sees whole rows.  After the wait the host's mirrors follow for
 * rows[0 .. made): has_rays, the source-slot reference counts, the store's length (+ 2 * made).  Returns made.  With n_cand == 0 there is
 * nothing to thin or create: the arguments are checked, nothing is enqueued, made = 0 (and n_busy = 0 with busy_from_store: no gather ran).
 * REFUSALS (-1, mcp_last_error() starting "mcp_stereo_map_points:", nothing enqueued, table / graph / store unchanged): everything
 * mcp_stereo_points refuses; NULL graph / params / result; src on another device than the table; src_mkf or a target_mkf[t] that is not a present
 * slot; src_cam or a target_cam[t] outside the rig; n_rows < n_cand; a negative or duplicate row; NULL rows / keys with n_cand > 0; NULL
 * target_mkf / target_cam with n_targets > 0; meas given together with busy_from_store; a store that would pass INT_MAX. */
typedef struct mcp_stereo_map_params {
  int src_mkf, src_cam;        /* the source keyframe as the graph names it: MKF slot, camera index */
  int limit;                   /* nLimit, as mcp_stereo_points */
  int busy_from_store;         /* 1: ThinCandidates' measurement list is gathered from the store; 0: the caller's meas[] */
} mcp_stereo_map_params;
typedef struct mcp_stereo_map_result { int made, first_store, n_busy; } mcp_stereo_map_result;
int mcp_stereo_map_points(mcp_map_graph*, mcp_kf* src, const mcp_camera* src_cam, const double src_cam_from_world[12], int level,
                          int n_cand, const mcp_int2* cand, int n_meas, const mcp_stereo_meas* meas,
                          int n_targets, const mcp_stereo_target* targets, const int* target_mkf, const int* target_cam,
                          int n_rows, const int* rows, const int* keys,
                          const mcp_stereo_map_params*, mcp_stereo_map_result*,
                          mcp_stereo_point* out /* NULL or n_cand */, uint8_t* keep, uint8_t* outcome /* NULL or n_targets x n_cand */);
/* the two halves from host arrays, by the same bodies under the host compiler: they need no device and give the device's bytes.
 * mcp_stereo_busy_host: the busy list of a store, in store order.  cap = 0: counts only; otherwise out has room for cap records and a longer list
 * is refused.  Returns the length.
 * mcp_stereo_append_host: created points pts[0 .. made) into per-point arrays (world_pos, pixel_right_w, pixel_down_w: made x 3; rays: made x 9;
 * center_xy: made x 2; the graph columns: made) and their 2 x made store entries.  Returns first_store + 2 * made, the store's length afterwards. */
int mcp_stereo_busy_host(int n_store, const mcp_store_entry* store, int src_mkf, int src_cam, int cap, mcp_stereo_meas* out);
int mcp_stereo_append_host(int made, const mcp_stereo_point* pts, const int* rows, int level, int src_mkf, int src_cam,
                           const int* target_mkf, const int* target_cam, int first_store,
                           double* world_pos, double* pixel_right_w, double* pixel_down_w, double* rays /* made x 9 */,
                           int* center_xy, int* gp_src_mkf, int* gp_src_cam, int* gp_flags, mcp_store_entry* appended /* 2 x made */);
/* read-backs of rows first .. first+count-1 (every output pointer may be NULL: it is skipped); each waits for the table's stream, as
 * mcp_map_points_get does.  rays: count x 9 (zeros for a row without), has: the host's record of which rows have rays.  source: the row's key,
 * level, centre (count x 2), fixed byte and whether it names a source keyframe.  gp: the graph's point columns; a row they do not cover yet
 * reads as never written (-1, 0, MCP_GP_BAD). */
int mcp_map_points_get_rays(const mcp_map_points*, int first, int count, double* rays /* count x 9 */, uint8_t* has);
int mcp_map_points_get_source(const mcp_map_points*, int first, int count, int* keys, int* source_level, int* center_xy, uint8_t* fixed, uint8_t* has_source);
int mcp_map_gp_get(mcp_map_graph*, int first, int count, int* src_mkf, int* src_cam, int* flags);

/* ---- The map's beginning, its rescale and its re-alignment on the device --------------------------- src/MapMakerServerBase.cc:146-261, 499-596
 * mcp_init_depth_map_points is AddInitDepthMapPoints (:499-546) of ONE MKF at ONE level, all cameras of the rig in one call (cams[c] is the rig's
 * camera c; ncam must be the rig's): one submission on the table's stream, one host wait.  Per camera c: the busy list of (src_mkf, c) is gathered
 * from the store in store order and ThinCandidates runs against it (levels level and level + 1, squared integer distance < 100), exactly as
 * mcp_stereo_map_points does with busy_from_store = 1; keep (all cameras' candidates one after the other) is the thinning's verdict -- the
 * reference leaves vCandidates = vCGood, created ones included.  The first `limit` survivors in candidate order become points.  Per point:
 * root = LevelZeroPos(cand, level); the three patch rays UnProject(root), UnProject(root + (2^level, 0)), UnProject(root + (0, 2^level)), each
 * normalised again; world = CamFromWorld^-1 * (UnProject(root) * init_depth) with CamFromWorld = cam_from_base[c] * base_from_world(src_mkf) TAKEN
 * FROM THE GRAPH (no pose argument); RefreshPixelVectors.  Creation order is camera-major, then candidate order; point k in that order takes
 * rows[k] / keys[k] (camera c's points start at the sum of made[c'] over c' < c, which only the device knows before the wait).  Row rows[k]
 * receives what mcp_stereo_map_points writes for a stereo point: world position and pixel vectors, usable 0, counts (1, 0), rays, source =
 * cams[c].src at `level` with the candidate as centre, fixed 0, the key (every camera's finder state of the row zeroed when the key changes),
 * graph columns (src_mkf, c, flags 0, pending 0) -- and ONE store entry at first_store + k: {root, src_mkf, c, rows[k], level, MCP_SRC_ROOT,
 * alive}.  Rows rows[made_total ..) stay untouched.  out, when not NULL, receives the records (target = -1, target_pos zero).  After the wait
 * the host's mirrors follow: has_rays, the source-slot reference counts, the store's length (+ made_total).  n_busy[c] / n_alive[c]: the length
 * of camera c's busy list and its surviving candidates (0 / 0 for a camera without candidates: no gather ran).  Growth before anything is
 * enqueued, the grow-when-idle rule and the event on each source keyframe's stream are mcp_stereo_map_points'.  Returns made_total.
 * REFUSALS (-1, mcp_last_error() starting "mcp_init_depth_map_points:", nothing enqueued, nothing changed): NULL graph / cams / params / result;
 * ncam not the rig's; level outside 0..3; a negative limit or n_cand; a camera with candidates whose src is not a live keyframe handle with a
 * frame on the table's device, whose camera is bad or that has a candidate outside the level image; n_rows < sum over c of min(n_cand, limit);
 * a negative or duplicate row; NULL rows / keys with n_rows > 0; NULL keep with candidates; init_depth not finite or <= 0; src_mkf not present; a
 * store that would pass INT_MAX.  sum n_cand == 0: the arguments are checked, nothing is enqueued, 0 is returned. */
typedef struct mcp_init_depth_cam { mcp_kf* src; const mcp_camera* cam; int n_cand; const mcp_int2* cand; int limit; } mcp_init_depth_cam;
typedef struct mcp_init_depth_params { int src_mkf, level; double init_depth; } mcp_init_depth_params;
typedef struct mcp_init_depth_result { int made_total, first_store; int made[MCP_MAX_FRAME_CAMS], n_busy[MCP_MAX_FRAME_CAMS], n_alive[MCP_MAX_FRAME_CAMS]; } mcp_init_depth_result;
int mcp_init_depth_map_points(mcp_map_graph*, int ncam, const mcp_init_depth_cam* cams, int n_rows, const int* rows, const int* keys,
                              const mcp_init_depth_params*, mcp_init_depth_result*, mcp_stereo_point* out /* NULL or n_rows */, uint8_t* keep /* sum of n_cand */);
/* NAMES.  mcp_map_mark_optimized, mcp_map_rescale and mcp_map_transform take the graph, like mcp_map_bundle_select, mcp_map_cull_*, mcp_map_neighbours
 * and mcp_map_mkf_cull, and pair with their host twins mcp_map_mark_optimized_host / mcp_map_transform_host.  They do not carry the prefix
 * mcp_map_graph_: that prefix names the graph's own upkeep (create .. check), a closed set that tests/test_capi_map_graph_cpu.py counts.
 * The end of InitFromMultiKeyFrame (:212-215, mbOptimized = true on every point): usable = 1 on every table row whose graph column has been
 * written and is not MCP_GP_BAD; every other byte of every row keeps its value.  One kernel, one wait; *n_marked (may be NULL): the rows named. */
int mcp_map_mark_optimized(mcp_map_graph*, int* n_marked);
/* ApplyGlobalScaleToMap (:549-574) / ApplyGlobalTransformationToMap (:577-596) over the resident map, one submission and one wait each:
 *  1. every MCP_MKF_PRESENT slot (bad ones included): rescale multiplies the translation of base_from_world by scale (the rig's cam_from_base is
 *     not scaled, as in the reference); transform sets base_from_world = base_from_world * new_from_old^-1.
 *  2. every table row whose graph column names a present src_mkf and a camera of the rig: world *= scale, or world = new_from_old * world; then,
 *     when the row has rays (the table's host record, sent up as one bit per row), RefreshPixelVectors at the NEW pose of its source keyframe.
 *     Counted in n_refreshed, or in n_no_rays (new world position only).  A row without such a source keeps every byte: n_no_source.
 *  3. rescale only: RefreshSceneDepthRobust of every present MKF, exactly as mcp_graph_refresh_depth over all present slots in ascending order
 *     (same lists, kernel and summation contract; mean stored into the slot's depth column); depth_out as there, n present slots x ncam.
 * usable, counts, rays, sources, keys, finder states, graph columns and the store keep every byte.  n_rows: the table's; n_mkfs: present slots.
 * REFUSALS (-1, message starting with the call's name, nothing enqueued): NULL graph or result; scale not finite or <= 0; a non-finite entry of
 * new_from_old (R row-major 9, t 3); a rotation part with max |R R^T - I| > 1e-9 (a caller's mistake is rejected, nothing is re-orthogonalised).
 * An empty table and a graph without a present slot are allowed. */
typedef struct mcp_map_transform_result { int n_rows, n_refreshed, n_no_rays, n_no_source, n_mkfs; } mcp_map_transform_result;
int mcp_map_rescale(mcp_map_graph*, double scale, mcp_map_transform_result*, mcp_scene_depth* depth_out /* NULL or n present slots x ncam, ascending slot */);
int mcp_map_transform(mcp_map_graph*, const double new_from_old[12], mcp_map_transform_result*);
/* device time in ms of the last mcp_init_depth_map_points / the last mcp_map_rescale or mcp_map_transform that ran to its wait (between two events
 * around the submission on the table's stream); -1.0 before the first such call */
int mcp_map_life_last_timing(const mcp_map_graph*, double* init_depth_ms, double* move_ms);
/* The three from host arrays, by the bodies the kernels call (map_life.h) under the host compiler: no device, the device's bytes.
 * mcp_init_depth_points_host: cams / n_cand / limit / n_busy: ncam entries; cand and busy: the cameras' lists one after the other; the busy lists
 * are the caller's (mcp_stereo_busy_host).  keep: sum n_cand; out, the per-point arrays (x 3, rays x 9, center_xy x 2) and appended: n_rows
 * entries, the first made_total written.  res->n_busy is the caller's n_busy.  Returns made_total.
 * mcp_map_mark_optimized_host: usable[r] = 1 where the rule holds (point_flags: n_point_rows graph columns); returns the count.
 * mcp_map_transform_host: kind 0 (scale) or 1 (new_from_old); base_from_world (n_slots x 12), world_pos, pixel_right_w, pixel_down_w (n_rows x 3)
 * are rewritten in place; has_rays: one byte per row; rays: n_rows x 9; gp_src_mkf / gp_src_cam: n_point_rows (rows past them have no source). */
int mcp_init_depth_points_host(int ncam, const double* cam_from_base, const double src_base_from_world[12], const mcp_camera* cams, const int* n_cand,
                               const mcp_int2* cand, const int* limit, const int* n_busy, const mcp_stereo_meas* busy, int n_rows, const int* rows,
                               const mcp_init_depth_params*, int first_store, mcp_init_depth_result*, uint8_t* keep, mcp_stereo_point* out,
                               double* world_pos, double* pixel_right_w, double* pixel_down_w, double* rays, int* center_xy, int* gp_src_mkf, int* gp_src_cam,
                               int* gp_flags, mcp_store_entry* appended);
int mcp_map_mark_optimized_host(int n_rows, int n_point_rows, const int* point_flags, uint8_t* usable);
int mcp_map_transform_host(int kind, double scale, const double new_from_old[12], int ncam, const double* cam_from_base, int n_slots, double* base_from_world,
                           const int* mkf_flags, int n_rows, int n_point_rows, const int* gp_src_mkf, const int* gp_src_cam, const uint8_t* has_rays,
                           const double* rays, double* world_pos, double* pixel_right_w, double* pixel_down_w, mcp_map_transform_result*);

#ifdef __cplusplus
}
#endif
#endif
