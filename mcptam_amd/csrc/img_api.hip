// img_api.hip -- C ABI of the KeyFrame / Tracker image path (include/mcp_img.h); host side only
// marshals buffers and launches the kernels of img_kernels.h, pvs_kernels.h, track_map_kernels.h, stereo_kernels.h, write_back_kernels.h
// and refind_kernels.h.  No CPU fallback.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <limits>
#include <map>
#include <functional>
#include <memory>
#include <mutex>
#include <unordered_map>

#include "../../include/mcp_img.h"
#include "img_kernels.h"
#include "pvs_kernels.h"
#include "track_map_kernels.h"
#include "stereo_kernels.h"
#include "write_back_kernels.h"
#include "refind_kernels.h"
#include "track_record_kernels.h"
#include "track_motion_kernels.h"
#include "track_recover_kernels.h"
#include "track_cov_kernels.h"
#include "ba_bridge.h"
#include "mcp_knobs.h"
#include "ba_select.h"
#include "map_graph_kernels.h"
#include "map_graph_lists.h"
#include "map_graph_parcel.h"
#include "map_graph_cull.h"
#include "map_graph_neigh.h"
#include "map_graph_collect.h"
#include "stereo_append.h"
#include "map_life.h"

using namespace mcp;

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int img_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }
#define ICK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return img_fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

namespace {
template <class T> struct Buf {
  T* p = nullptr; size_t n = 0;
  ~Buf() { if (p) (void)hipFree(p); }
  void swap(Buf& o) { std::swap(p, o.p); std::swap(n, o.n); }
  int alloc(size_t c) { if (c == 0) c = 1; if (c <= n) return 0; if (p) (void)hipFree(p); p = nullptr; n = 0;
    if (hipMalloc((void**)&p, c*sizeof(T)) != hipSuccess) { mcp_set_error("hipMalloc failed"); return -1; } n = c; return 0; }
};
// pinned host staging that outlives the call that fills it (the uploads of an enqueue-only helper are still in flight when it returns)
template <class T> struct PinBuf {
  T* p = nullptr; size_t n = 0;
  ~PinBuf() { if (p) (void)hipHostFree(p); }
  int alloc(size_t c) { if (c == 0) c = 1; if (c <= n) return 0; if (p) (void)hipHostFree(p); p = nullptr; n = 0;
    if (hipHostMalloc((void**)&p, c*sizeof(T)) != hipSuccess) { mcp_set_error("hipHostMalloc failed"); return -1; } n = c; return 0; }
};
struct Level {
  int w = 0, h = 0, cap = 0;
  Buf<uint8_t> img, mask, tmp_a, tmp_b;
  Buf<mcp_int2> corners, cand_pos;
  Buf<uint8_t> score8;                             // FAST score per pixel at the detection threshold (0 = no corner), scratch of MakeKeyFrame_Lite
  Buf<int> lut, rowcnt, blk_cnt, score_img;
  Buf<unsigned long long> scan;                    // k_row_tables: per 4-row workgroup, (epoch << 32 | kept corners)
  Buf<double> cand_score;
  Buf<LevelInfo> info;
  bool has_mask = false;
  std::vector<mcp_int2> h_cand; std::vector<double> h_cand_score;
  // Level::imagePrev / vCornersPrev (KeyFrame.h:147-148): the last NUM_PREV frames' level image, corners, row LUT and
  // counts stay resident; [0] is the oldest.  Buffers rotate by pointer swap, nothing is copied.
  static constexpr int NUM_PREV = 2;            // Level::snNumPrev, KeyFrame.cc:71
  int nprev = 0;
  Buf<uint8_t> pimg[NUM_PREV]; Buf<mcp_int2> pcorners[NUM_PREV]; Buf<int> plut[NUM_PREV]; Buf<LevelInfo> pinfo[NUM_PREV];
  int alloc_frame() {
    const size_t npx = (size_t)w*h;
    if (img.alloc(npx) || corners.alloc(cap) || lut.alloc(h) || info.alloc(1)) return -1;
    return 0;
  }
  int push_history() {                           // circular_buffer::push_back of the frame currently held
    if (nprev == NUM_PREV) { pimg[0].swap(pimg[1]); pcorners[0].swap(pcorners[1]); plut[0].swap(plut[1]); pinfo[0].swap(pinfo[1]); --nprev; }
    pimg[nprev].swap(img); pcorners[nprev].swap(corners); plut[nprev].swap(lut); pinfo[nprev].swap(info);
    ++nprev;
    return alloc_frame();                        // the dropped frame's buffers (or fresh ones) become the current frame
  }
};
}  // namespace

struct mcp_kf {
  int device = 0; hipStream_t st = nullptr;
  unsigned long long serial = 0;    // creation serial: the map-point table keeps (handle, serial) of patch sources, never a device pointer
  mcp_kf_params prm;
  Level lev[MCP_LEVELS];
  // scratch reused across calls (no hipMalloc on the per-frame path)
  Buf<DevTdIn> td_in; Buf<mcp_td_out> td_out;
  Buf<mcp_int2> mp_a, mp_b, mp_o; Buf<uint8_t> mp_f, mp_f2; Buf<int> mp_s;
  bool has_image = false;
  LevelInfo* h_info = nullptr;      // pinned, device-visible: the kernels leave the four levels' bookkeeping here (one wait per frame)
  Buf<int> work;                    // threshold histogram + detected-corner count per level; k_row_compact leaves it zero again
  bool work_dirty = true;
  unsigned int scan_epoch = 0;        // k_row_tables: this frame's tag
  Buf<SearchCam> stab; Buf<DevTdIn> bt_in; Buf<mcp_td_out> bt_out;      // batched search: camera table + points of all cameras
  Buf<PfTargetDev> pf_tab; Buf<PfItemDev> pf_items; Buf<int> pf_seq; Buf<mcp_pf_state> pf_state;      // mcp_patch_sequences
  PinBuf<SearchCam> h_stab; PinBuf<DevTdIn> h_bt_in;                                                   // host staging of the batched search ...
  PinBuf<mcp_td_out> h_bt_out;                                                                         // ... and, for mcp_track_frame, its results: the search kernel writes them here as well
  int view_first[MCP_MAX_FRAME_CAMS + 1] = {0}; int view_ncam = 0;                                     // mcp_track_frame_view: where camera c's results of the last frame start in h_bt_out
  PinBuf<PfTargetDev> h_pf_tab; PinBuf<PfItemDev> h_pf_items; PinBuf<int> h_pf_seq; PinBuf<mcp_pf_state> h_pf_state, h_pf_state_out;      // ... and of mcp_track_frame's finder sequences (states in / out)
  hipEvent_t ev = nullptr;
  // SmallBlurryImage of the frame currently held (KeyFrame::mpSBI): thumbnail, zero-mean blurred template, gradient image
  Buf<uint8_t> sbi_small; Buf<float> sbi_templ, sbi_jacs; bool has_sbi = false;
  Buf<uint8_t> sbi_last_small; Buf<float> sbi_last_templ, sbi_last_jacs; bool has_last_sbi = false;   // the SBI made before the current one (Tracker::mmpSBILastFrame)
  Buf<const float*> sbi_ptrs; Buf<double> sbi_out;
  // mcp_stereo_points / mcp_stereo_hypotheses with this handle as the source: their scratch
  Buf<StereoTargetDev> st_tab; Buf<mcp_int2> st_cand; Buf<mcp_stereo_meas> st_meas; Buf<uint8_t> st_alive, st_outcome; Buf<mcp_stereo_point> st_res;
  Buf<int> st_counts; Buf<mcp_td_in> st_hyp; PinBuf<mcp_stereo_point> h_st_out; PinBuf<int> h_st_counts; PinBuf<uint8_t> h_st_keep, h_st_outcome;
  ~mcp_kf() { if (st) (void)hipStreamDestroy(st); if (h_info) (void)hipHostFree(h_info); if (ev) (void)hipEventDestroy(ev); }
  DevKfView view() const {
    DevKfView v;
    for (int l = 0; l < MCP_LEVELS; ++l) { v.img[l] = lev[l].img.p; v.w[l] = lev[l].w; v.h[l] = lev[l].h; v.corners[l] = lev[l].corners.p; v.lut[l] = lev[l].lut.p; v.info[l] = lev[l].info.p; }
    return v;
  }
};

// the live keyframes and their creation serials (mcp_map_points_set_source / mcp_track_map resolve a source handle here)
static std::mutex g_kf_mu;
static std::unordered_map<const mcp_kf*, unsigned long long> g_kf_live;
static unsigned long long g_kf_serial = 0;
static unsigned long long kf_live_serial(const mcp_kf* k) { std::lock_guard<std::mutex> g(g_kf_mu); auto it = g_kf_live.find(k); return it == g_kf_live.end() ? 0ull : it->second; }

// ---- what the entries below pack for the kernels, each said once ---------------------------------------------------------------------
static Se3 se3_of12(const double* a) { Se3 T; std::memcpy(T.R, a, 72); std::memcpy(T.t, a + 9, 24); return T; }
// the level-0 mask of the frame a keyframe holds, or null
static const uint8_t* mask0_of(const mcp_kf* k) { return k->lev[0].has_mask ? k->lev[0].mask.p : nullptr; }
// a target record's view, mask and camera (PfTargetDev, TmCam, StereoTargetDev: the poses that follow differ) ...
template <class Target> static void target_of(Target& D, const mcp_kf* k, const mcp_camera& cam) { D.T = k->view(); D.mask0 = mask0_of(k); D.cam = cam; }
// ... and a finder target whole
static void target_of(PfTargetDev& D, const mcp_kf* k, const mcp_camera& cam, const double* bfw, const double* cfb) {
  target_of(D, k, cam); D.bfw = se3_of12(bfw); D.cfb = se3_of12(cfb);
}
// a caller's point as the kernels read it; false, and nothing written, for a point without a resident source keyframe and level
static bool td_in_resident(const mcp_td_in& p) { return p.source_kf && p.source_level >= 0 && p.source_level < MCP_LEVELS; }
static bool td_in_dev(const mcp_td_in& p, DevTdIn& d) {
  if (!td_in_resident(p)) return false;
  std::memcpy(d.world_pos, p.world_pos, 24); std::memcpy(d.pixel_right_w, p.pixel_right_w, 24); std::memcpy(d.pixel_down_w, p.pixel_down_w, 24);
  const Level& S = p.source_kf->lev[p.source_level];
  d.src_img = S.img.p; d.src_w = S.w; d.src_h = S.h; d.center_x = p.center_x; d.center_y = p.center_y; d.fixed = p.fixed;
  return true;
}
// the inputs of a frame's search as its pack step leaves them: at most four (pinned source, device destination, bytes).  They reach the
// device as copies on the stream, or inside the pyramids' second launch (FrameBatch::up_*, 8-byte words: a source is padded to a whole word)
struct Uploads {
  const void* src[4]; void* dst[4]; size_t bytes[4]; int n = 0;
  void add(const void* s, void* d, size_t b) { src[n] = s; dst[n] = d; bytes[n] = b; ++n; }
  int copy(hipStream_t st) const { for (int r = 0; r < n; ++r) ICK(hipMemcpyAsync(dst[r], src[r], bytes[r], hipMemcpyHostToDevice, st)); return 0; }
  void ride(FrameBatch& B) const {
    for (int r = 0; r < n; ++r) { B.up_src[r] = static_cast<const unsigned long long*>(src[r]); B.up_dst[r] = static_cast<unsigned long long*>(dst[r]); B.up_n8[r] = (int)((bytes[r] + 7)/8); }
  }
};

static bool gfx950(int dev) { hipDeviceProp_t p; return hipGetDeviceProperties(&p, dev) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0; }

extern "C" {

mcp_kf* mcp_kf_create(int w, int h, const mcp_kf_params* params) {
  if (w < 64 || h < 64) { mcp_set_error("mcp_kf_create: image too small"); return nullptr; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { mcp_set_error("mcp_kf_create: no HIP device available (the HIP path has no CPU fallback)"); return nullptr; }
  mcp_kf_params p; p.adaptive_thresh = 1; p.glare_masking = 0; p.half_sample_pavgb = 0; p.device = -1;
  if (params) p = *params;
  int dev = p.device; if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev >= ndev || !gfx950(dev)) { mcp_set_error("mcp_kf_create: device is not a gfx950 (MI355X)"); return nullptr; }
  if (hipSetDevice(dev) != hipSuccess) { mcp_set_error("hipSetDevice failed"); return nullptr; }
  mcp_kf* k = new mcp_kf(); k->device = dev; k->prm = p;
  if (hipStreamCreateWithFlags(&k->st, hipStreamNonBlocking) != hipSuccess) { mcp_set_error("hipStreamCreate failed"); delete k; return nullptr; }
  if (hipEventCreateWithFlags(&k->ev, hipEventDisableTiming) != hipSuccess || hipHostMalloc((void**)&k->h_info, MCP_LEVELS*sizeof(LevelInfo)) != hipSuccess ||
      k->work.alloc(FRAME_WORK_INTS)) { mcp_set_error("mcp_kf_create: allocation failed"); delete k; return nullptr; }
  std::memset(k->h_info, 0, MCP_LEVELS*sizeof(LevelInfo));
  for (int l = 0; l < MCP_LEVELS; ++l) {
    Level& L = k->lev[l]; L.w = w >> l; L.h = h >> l; L.cap = std::max(1024, L.w*L.h/2);
    const size_t npx = (size_t)L.w*L.h; const int nblk = (L.cap + FAST_BLOCK - 1)/FAST_BLOCK + 2;
    if (L.img.alloc(npx) || L.mask.alloc(npx) || L.score8.alloc(npx) || L.rowcnt.alloc(L.h) || L.scan.alloc((L.h + 3)/4 + 1) || L.corners.alloc(L.cap) ||
        L.lut.alloc(L.h) || L.blk_cnt.alloc(nblk) || L.info.alloc(1) || L.cand_pos.alloc(L.cap) || L.cand_score.alloc(L.cap)) { delete k; return nullptr; }
    (void)hipMemset(L.info.p, 0, sizeof(LevelInfo));
    (void)hipMemset(L.scan.p, 0, ((size_t)(L.h + 3)/4 + 1)*sizeof(unsigned long long));      // (epoch 0 = never written; frames count from 1)
  }
  { std::lock_guard<std::mutex> g(g_kf_mu); k->serial = ++g_kf_serial; g_kf_live[k] = k->serial; }
  return k;
}
void mcp_kf_destroy(mcp_kf* k) {
  if (!k) return;
  { std::lock_guard<std::mutex> g(g_kf_mu); g_kf_live.erase(k); }
  (void)hipSetDevice(k->device); delete k;
}

// MakeKeyFrame_Lite of every camera of a frame in one submission (the loop of Tracker::TrackFrame, src/Tracker.cc:303-318): the
// uploads, three launches for all levels of all cameras (k_pyr_fast, k_row_count, k_row_compact) and one wait.
// (enqueue on kfs[0]->st without waiting; lite_batch_finish after the stream has been waited for)
// (ride: called after k_pyr_fast has been launched -- host work done here overlaps it -- to name up to four pinned-host -> device copies that
//  k_row_count's grid then carries in one more z-slice, FrameBatch::up_*)
using FrameRide = std::function<int(FrameBatch&)>;
static int lite_batch_enqueue(int ncam, mcp_kf* const* kfs, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                              const uint8_t* const* const* masks, const FrameRide* ride = nullptr) {
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !kfs || !imgs || !strides) return img_fail("mcp_kf_make_lite_batch: bad arguments");
  for (int c = 0; c < ncam; ++c) {
    if (!kfs[c] || !imgs[c] || kfs[c]->device != kfs[0]->device) return img_fail("mcp_kf_make_lite_batch: keyframes must live on one device");
    for (int d = 0; d < c; ++d) if (kfs[d] == kfs[c]) return img_fail("mcp_kf_make_lite_batch: a keyframe appears twice");
  }
  ICK(hipSetDevice(kfs[0]->device));
  hipStream_t st = kfs[0]->st;
  static const int fixed_t[4] = { 10, 15, 15, 10 };
  // launches are grouped by the settings a launch shares; a frame's cameras normally share all of them
  for (int c = 1; c < ncam; ++c)
    if (kfs[c]->prm.adaptive_thresh != kfs[0]->prm.adaptive_thresh || kfs[c]->prm.half_sample_pavgb != kfs[0]->prm.half_sample_pavgb)
      return img_fail("mcp_kf_make_lite_batch: the keyframes of a batch must share adaptive_thresh and half_sample_pavgb");
  FrameBatch B; std::memset(&B, 0, sizeof B);
  B.ncam = ncam; B.adaptive = kfs[0]->prm.adaptive_thresh; B.pavgb = kfs[0]->prm.half_sample_pavgb;
  for (int l = 0; l < MCP_LEVELS; ++l) B.detect_t[l] = B.adaptive ? MCP_MIN_FAST_THRESH : fixed_t[l];
  int maxtiles = 0, maxh = 0; bool glare = false;
  for (int c = 0; c < ncam; ++c) {
    mcp_kf* k = kfs[c];
    // the frame currently held moves into the history before it is overwritten, KeyFrame.cc:152-199
    if (k->has_image) for (int l = 0; l < MCP_LEVELS; ++l) if (k->lev[l].push_history()) return -1;
    k->has_image = true;
    if (k->work_dirty) { ICK(hipMemsetAsync(k->work.p, 0, FRAME_WORK_INTS*sizeof(int), st)); }
    k->work_dirty = true;                         // until k_row_compact of this frame has run to the end
    FrameCam& C = B.c[c];
    const Level& L0 = k->lev[0];
    C.w = L0.w; C.h = L0.h; C.work = k->work.p; C.host_info = k->h_info; C.epoch = ++k->scan_epoch;
    if (imgs_on_device) { C.src = imgs[c]; C.src_stride = strides[c]; }
    else { ICK(hipMemcpy2DAsync(L0.img.p, L0.w, imgs[c], strides[c], L0.w, L0.h, hipMemcpyHostToDevice, st)); C.src = L0.img.p; C.src_stride = L0.w; }
    for (int l = 0; l < MCP_LEVELS; ++l) {
      Level& L = k->lev[l];
      C.img[l] = L.img.p; C.score[l] = L.score8.p; C.corners[l] = L.corners.p; C.lut[l] = L.lut.p; C.rowcnt[l] = L.rowcnt.p; C.scan[l] = L.scan.p; C.info[l] = L.info.p; C.cap[l] = L.cap;
      const uint8_t* m = masks && masks[c] ? masks[c][l] : nullptr;
      if (m) ICK(hipMemcpyAsync(L.mask.p, m, (size_t)L.w*L.h, hipMemcpyHostToDevice, st));
      C.mask[l] = (m || k->prm.glare_masking) ? L.mask.p : nullptr;
      L.has_mask = C.mask[l] != nullptr;
    }
    glare = glare || k->prm.glare_masking;
    maxtiles = std::max(maxtiles, ((C.w + PYR_T - 1)/PYR_T)*((C.h + PYR_T - 1)/PYR_T)); maxh = std::max(maxh, C.h);
  }
  hipLaunchKernelGGL(k_pyr_fast, dim3(maxtiles, ncam), dim3(PYR_NT), 0, st, B);
  if (glare) for (int c = 0; c < ncam; ++c) {        // cv::dilate x5 of every level image, KeyFrame.cc:214-238 (needs the level images: after k_pyr_fast)
    mcp_kf* k = kfs[c];
    if (!k->prm.glare_masking) continue;
    for (int l = 0; l < MCP_LEVELS; ++l) {
      Level& L = k->lev[l];
      const size_t npx = (size_t)L.w*L.h;
      if (L.tmp_a.alloc(npx) || L.tmp_b.alloc(npx)) return -1;
      const uint8_t* internal = masks && masks[c] && masks[c][l] ? L.mask.p : nullptr;
      const uint8_t* src = L.img.p; uint8_t* a = L.tmp_a.p; uint8_t* b = L.tmp_b.p;
      for (int it = 0; it < 5; ++it) { hipLaunchKernelGGL(k_dilate5, dim3((L.w + 31)/32, (L.h + 7)/8), dim3(32, 8), 0, st, src, a, L.w, L.h); src = a; std::swap(a, b); }
      hipLaunchKernelGGL(k_glare_mask, dim3((unsigned)((npx + 255)/256)), dim3(256), 0, st, src, internal, L.mask.p, (int)npx);
    }
  }
  if (ride && (*ride)(B)) return -1;
  const int up = (B.up_n8[0] > 0 || B.up_n8[1] > 0 || B.up_n8[2] > 0 || B.up_n8[3] > 0) ? 1 : 0;
  static const bool one_launch = mcp::knobs::img_row_tables();      // (0: k_row_count + k_row_compact, the round-5 pair)
  if (one_launch) hipLaunchKernelGGL(k_row_tables, dim3((maxh + 3)/4, MCP_LEVELS, ncam + up), dim3(256), 0, st, B);
  else {
    hipLaunchKernelGGL(k_row_count, dim3((maxh + 3)/4, MCP_LEVELS, ncam + up), dim3(256), 0, st, B);
    B.up_n8[0] = B.up_n8[1] = B.up_n8[2] = B.up_n8[3] = 0;
    hipLaunchKernelGGL(k_row_compact, dim3((maxh + 3)/4, MCP_LEVELS, ncam), dim3(256), 0, st, B);
  }
  ICK(hipGetLastError());
  return 0;
}
static int lite_batch_finish(int ncam, mcp_kf* const* kfs) {
  for (int c = 0; c < ncam; ++c) {
    kfs[c]->work_dirty = false;
    for (int l = 0; l < MCP_LEVELS; ++l) if (kfs[c]->h_info[l].overflow) return img_fail("mcp_kf_make_lite: corner capacity exceeded");
  }
  return 0;
}
int mcp_kf_make_lite_batch(int ncam, mcp_kf* const* kfs, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                           const uint8_t* const* const* masks) {
  if (lite_batch_enqueue(ncam, kfs, imgs, strides, imgs_on_device, masks)) return -1;
  ICK(hipStreamSynchronize(kfs[0]->st));
  return lite_batch_finish(ncam, kfs);
}
int mcp_kf_make_lite(mcp_kf* k, const uint8_t* img, int stride, const uint8_t* const* masks) {
  mcp_kf* kfs[1] = { k }; const uint8_t* imgs[1] = { img }; const int strides[1] = { stride }; const uint8_t* const* ms[1] = { masks };
  return mcp_kf_make_lite_batch(1, kfs, imgs, strides, 0, masks ? ms : nullptr);
}

static int get_info(mcp_kf* k, int level, LevelInfo* inf) {
  if (level < 0 || level >= MCP_LEVELS) return img_fail("bad level");
  ICK(hipSetDevice(k->device));
  ICK(hipMemcpy(inf, k->lev[level].info.p, sizeof *inf, hipMemcpyDeviceToHost));
  return 0;
}
int mcp_kf_level_size(mcp_kf* k, int level, int* w, int* h) { if (level < 0 || level >= MCP_LEVELS) return img_fail("bad level"); *w = k->lev[level].w; *h = k->lev[level].h; return 0; }
int mcp_kf_get_image(mcp_kf* k, int level, uint8_t* out) {
  if (level < 0 || level >= MCP_LEVELS) return img_fail("bad level");
  ICK(hipSetDevice(k->device));
  ICK(hipMemcpy(out, k->lev[level].img.p, (size_t)k->lev[level].w*k->lev[level].h, hipMemcpyDeviceToHost)); return 0;
}
int mcp_kf_num_corners(mcp_kf* k, int level) { LevelInfo inf; if (get_info(k, level, &inf)) return -1; return inf.n_corners; }
int mcp_kf_get_corners(mcp_kf* k, int level, mcp_int2* out, int cap) {
  LevelInfo inf; if (get_info(k, level, &inf)) return -1;
  const int n = std::min(inf.n_corners, cap);
  if (n > 0) ICK(hipMemcpy(out, k->lev[level].corners.p, sizeof(mcp_int2)*(size_t)n, hipMemcpyDeviceToHost));
  return n;
}
int mcp_kf_get_row_lut(mcp_kf* k, int level, int* out) {
  if (level < 0 || level >= MCP_LEVELS) return img_fail("bad level");
  ICK(hipSetDevice(k->device));
  ICK(hipMemcpy(out, k->lev[level].lut.p, sizeof(int)*(size_t)k->lev[level].h, hipMemcpyDeviceToHost)); return 0;
}
int mcp_kf_fast_thresh(mcp_kf* k, int level) { LevelInfo inf; if (get_info(k, level, &inf)) return -1; return inf.thresh; }
int mcp_kf_get_fast_frequency(mcp_kf* k, int level, double* out) {
  LevelInfo inf; if (get_info(k, level, &inf)) return -1;
  for (int t = 0; t <= MCP_MAX_FAST_THRESH; ++t) out[t] = (double)inf.hist[t];
  return 0;
}

int mcp_kf_make_rest(mcp_kf* k, int use_shi, int use_percent, double top_fraction, double thresh, int nonmax_score) {
  ICK(hipSetDevice(k->device));
  hipStream_t st = k->st;
  for (int l = 0; l < MCP_LEVELS; ++l) {
    Level& L = k->lev[l];
    const size_t npx = (size_t)L.w*L.h;
    if (L.score_img.alloc(npx)) return -1;
    ICK(hipMemsetAsync(L.score_img.p, 0, npx*sizeof(int), st));
    const int nb = (L.cap + FAST_BLOCK - 1)/FAST_BLOCK;
    hipLaunchKernelGGL(k_nonmax_scores, dim3(nb), dim3(FAST_BLOCK), 0, st, (const uint8_t*)L.img.p, L.w, (const mcp_int2*)L.corners.p, (const LevelInfo*)L.info.p, nonmax_score, L.score_img.p);
    hipLaunchKernelGGL((k_candidates<false>), dim3(nb), dim3(FAST_BLOCK), 0, st, (const uint8_t*)L.img.p, L.w, L.h, (const mcp_int2*)L.corners.p, L.info.p, (const int*)L.score_img.p, use_shi, L.blk_cnt.p, L.cand_pos.p, L.cand_score.p);
    hipLaunchKernelGGL((k_candidates<true>), dim3(nb), dim3(FAST_BLOCK), 0, st, (const uint8_t*)L.img.p, L.w, L.h, (const mcp_int2*)L.corners.p, L.info.p, (const int*)L.score_img.p, use_shi, L.blk_cnt.p, L.cand_pos.p, L.cand_score.p);
  }
  ICK(hipStreamSynchronize(st));
  // selection of the scored candidates (a few thousand pairs): sort / threshold on the host, KeyFrame.cc:422-452
  for (int l = 0; l < MCP_LEVELS; ++l) {
    Level& L = k->lev[l];
    LevelInfo inf; ICK(hipMemcpy(&inf, L.info.p, sizeof inf, hipMemcpyDeviceToHost));
    std::vector<mcp_int2> pos(inf.n_cand); std::vector<double> sc(inf.n_cand);
    if (inf.n_cand) { ICK(hipMemcpy(pos.data(), L.cand_pos.p, sizeof(mcp_int2)*pos.size(), hipMemcpyDeviceToHost)); ICK(hipMemcpy(sc.data(), L.cand_score.p, sizeof(double)*sc.size(), hipMemcpyDeviceToHost)); }
    std::vector<int> idx(inf.n_cand); for (int i = 0; i < inf.n_cand; ++i) idx[i] = i;
    L.h_cand.clear(); L.h_cand_score.clear();
    if (use_percent) {
      std::sort(idx.begin(), idx.end(), [&](int a, int b) {           // descending (score, ImageRef) as std::sort(rbegin, rend)
        if (sc[a] != sc[b]) return sc[a] > sc[b];
        if (pos[a].y != pos[b].y) return pos[a].y > pos[b].y;
        return pos[a].x > pos[b].x; });
      const int num = (int)(inf.n_cand*top_fraction);
      for (int i = 0; i < num && i < inf.n_cand; ++i) { L.h_cand.push_back(pos[idx[i]]); L.h_cand_score.push_back(sc[idx[i]]); }
    } else {
      for (int i = 0; i < inf.n_cand; ++i) if (sc[i] > thresh) { L.h_cand.push_back(pos[i]); L.h_cand_score.push_back(sc[i]); }
    }
  }
  // stability pruning, KeyFrame.cc:456-527: every candidate is followed back to the oldest stored frame and forward again
  // to the current one (MiniPatch, search radius 10 per stored frame); it survives if it lands within sqrt(2) pixels
  for (int l = 0; l < MCP_LEVELS; ++l) {
    Level& L = k->lev[l];
    const int n = (int)L.h_cand.size();
    if (L.nprev == 0 || n == 0) continue;
    if (k->mp_a.alloc(n) || k->mp_b.alloc(n) || k->mp_o.alloc(n) || k->mp_f.alloc(n) || k->mp_f2.alloc(n) || k->mp_s.alloc(n)) return -1;
    ICK(hipMemcpyAsync(k->mp_a.p, L.h_cand.data(), sizeof(mcp_int2)*(size_t)n, hipMemcpyHostToDevice, st));
    const int range = L.nprev*10;
    hipLaunchKernelGGL(k_minipatch, dim3(n), dim3(64), 0, st, (const uint8_t*)L.img.p, L.w, L.h, (const uint8_t*)L.pimg[0].p, L.w, L.h,
                       (const mcp_int2*)L.pcorners[0].p, (const LevelInfo*)L.pinfo[0].p, (const int*)L.plut[0].p, n, (const mcp_int2*)k->mp_a.p, (const mcp_int2*)k->mp_a.p, range,
                       k->mp_o.p, k->mp_f.p, k->mp_s.p);
    hipLaunchKernelGGL(k_minipatch, dim3(n), dim3(64), 0, st, (const uint8_t*)L.pimg[0].p, L.w, L.h, (const uint8_t*)L.img.p, L.w, L.h,
                       (const mcp_int2*)L.corners.p, (const LevelInfo*)L.info.p, (const int*)L.lut.p, n, (const mcp_int2*)k->mp_o.p, (const mcp_int2*)k->mp_o.p, range,
                       k->mp_b.p, k->mp_f2.p, k->mp_s.p);
    std::vector<mcp_int2> back(n); std::vector<uint8_t> f1(n), f2(n);
    ICK(hipMemcpyAsync(back.data(), k->mp_b.p, sizeof(mcp_int2)*(size_t)n, hipMemcpyDeviceToHost, st));
    ICK(hipMemcpyAsync(f1.data(), k->mp_f.p, (size_t)n, hipMemcpyDeviceToHost, st));
    ICK(hipMemcpyAsync(f2.data(), k->mp_f2.p, (size_t)n, hipMemcpyDeviceToHost, st));
    ICK(hipStreamSynchronize(st));
    int nk = 0;
    for (int i = 0; i < n; ++i) {
      if (!f1[i] || !f2[i]) continue;
      const int dx = back[i].x - L.h_cand[i].x, dy = back[i].y - L.h_cand[i].y;
      if (dx*dx + dy*dy > 2) continue;
      L.h_cand[nk] = L.h_cand[i]; L.h_cand_score[nk] = L.h_cand_score[i]; ++nk;
    }
    L.h_cand.resize(nk); L.h_cand_score.resize(nk);
  }
  return 0;
}
int mcp_kf_num_prev(mcp_kf* k) { return k->lev[0].nprev; }
int mcp_kf_num_candidates(mcp_kf* k, int level) { if (level < 0 || level >= MCP_LEVELS) return img_fail("bad level"); return (int)k->lev[level].h_cand.size(); }
int mcp_kf_get_candidates(mcp_kf* k, int level, mcp_int2* pos, double* score, int cap) {
  if (level < 0 || level >= MCP_LEVELS) return img_fail("bad level");
  const Level& L = k->lev[level];
  const int n = std::min((int)L.h_cand.size(), cap);
  if (n) { std::memcpy(pos, L.h_cand.data(), sizeof(mcp_int2)*n); std::memcpy(score, L.h_cand_score.data(), sizeof(double)*n); }
  return n;
}

int mcp_minipatch_find(mcp_kf* src, mcp_kf* dst, int level, int n, const mcp_int2* src_pos, const mcp_int2* dst_pos, int range,
                       mcp_int2* out_pos, uint8_t* out_found, int* out_ssd) {
  if (level < 0 || level >= MCP_LEVELS || n < 0) return img_fail("mcp_minipatch_find: bad arguments");
  if (n == 0) return 0;
  ICK(hipSetDevice(dst->device));
  Buf<mcp_int2>& dsp = dst->mp_a; Buf<mcp_int2>& ddp = dst->mp_b; Buf<mcp_int2>& dop = dst->mp_o; Buf<uint8_t>& dfound = dst->mp_f; Buf<int>& dssd = dst->mp_s;
  if (dsp.alloc(n) || ddp.alloc(n) || dop.alloc(n) || dfound.alloc(n) || dssd.alloc(n)) return -1;
  ICK(hipMemcpy(dsp.p, src_pos, sizeof(mcp_int2)*(size_t)n, hipMemcpyHostToDevice));
  ICK(hipMemcpy(ddp.p, dst_pos, sizeof(mcp_int2)*(size_t)n, hipMemcpyHostToDevice));
  const Level& S = src->lev[level]; const Level& D = dst->lev[level];
  hipLaunchKernelGGL(k_minipatch, dim3(n), dim3(64), 0, dst->st, (const uint8_t*)S.img.p, S.w, S.h, (const uint8_t*)D.img.p, D.w, D.h,
                     (const mcp_int2*)D.corners.p, (const LevelInfo*)D.info.p, (const int*)D.lut.p, n, (const mcp_int2*)dsp.p, (const mcp_int2*)ddp.p, range, dop.p, dfound.p, dssd.p);
  ICK(hipStreamSynchronize(dst->st));
  ICK(hipMemcpy(out_pos, dop.p, sizeof(mcp_int2)*(size_t)n, hipMemcpyDeviceToHost));
  ICK(hipMemcpy(out_found, dfound.p, (size_t)n, hipMemcpyDeviceToHost));
  if (out_ssd) ICK(hipMemcpy(out_ssd, dssd.p, sizeof(int)*(size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// a camera the device code may index: 0 (Newton mode) .. MCP_MAX_INV inverse-polynomial coefficients (as mcp_ba_create checks)
static bool cam_ok(const mcp_camera* c) { return c && c->n_inv >= 0 && c->n_inv <= MCP_MAX_INV; }

static bool est_ok(int e) { return e >= MCP_MEST_TUKEY && e <= MCP_MEST_HUBER; }
int mcp_track_pose_refine(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cfb, double bfw[12], int n_iter,
                          const uint8_t* nonlinear, const double* override_sigma, double mu_last[6], double* weights_last) {
  return mcp_track_pose_refine_m(n, pts, ncam, cams, cfb, bfw, n_iter, nonlinear, override_sigma, mu_last, weights_last, MCP_MEST_TUKEY);
}
// device scratch of the pose iterations, reused across calls.  The small inputs travel in ONE block (bytes): [BaseFromWorld 12 d | mu 6 d |
// pad 6 d | override sigma n_iter d | CamFromBase 12 ncam d | camera models | nonlinear flags], the results [BaseFromWorld | mu] come back
// in one copy: 2 uploads + 2-3 downloads per call instead of 6 + 4.
struct RefineScratch { Buf<mcp_pose_point> dp, dp_keep; Buf<uint8_t> dblk; Buf<double> dJ, dex, de2, dw; Buf<PrmScratch> dprm; Buf<double> de2all; std::vector<uint8_t> hblk; bool last_multi = false;
                       // what the last call on this scratch ran (mcp_debug_last_pose_route): -1 none yet, 0 k_pose_refine_regs, 1 k_pose_refine,
                       // 2 k_pose_refine_multi, 3 k_pose_refine_multi given up and redone by k_pose_refine; the multi launch's workgroups and median
                       int route = -1, route_nwg = 0; bool route_gather = false;
                       // k_pose_refine_regs reads the block and leaves BaseFromWorld | mu and the weights in PINNED HOST memory: no upload of the
                       // block, no fill of the weights, no copy back (three copy-engine operations and their queue switches per frame)
                       PinBuf<uint8_t> pblk; PinBuf<double> pw; bool res_pinned = false; };
// one scratch per (thread, device): the buffers live on the device that was current when they were allocated, and a thread that serves
// keyframes on two devices must not hand one device's kernels the other's pointers
static RefineScratch& refine_scratch() {
  static thread_local std::map<int, std::unique_ptr<RefineScratch>> per_dev;
  int dev = 0; (void)hipGetDevice(&dev);
  std::unique_ptr<RefineScratch>& p = per_dev[dev];
  if (!p) p.reset(new RefineScratch());
  return *p;
}
// where the parts behind the block's 24-double head start, and its size
struct RefineBlock {
  size_t ov, cfb, cam, nl, bytes;
  RefineBlock(int n_iter, int ncam) : ov(24*sizeof(double)), cfb(ov + 8*(size_t)n_iter), cam(cfb + 96*(size_t)ncam), nl(cam + sizeof(mcp_camera)*(size_t)ncam),
                                      bytes(((nl + (size_t)n_iter + 15)/16)*16) {}
};
// k_pose_refine_regs' dynamic LDS is a function attribute, and those are per device: set on first use by this thread on `dev`; whether the
// device took it
static bool pose_regs_attr(int dev) {
  static thread_local unsigned long long set_mask = 0, ok_mask = 0;
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(set_mask & bit)) {
    set_mask |= bit;
    if (hipFuncSetAttribute((const void*)k_pose_refine_regs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PRR_DYN_LDS) == hipSuccess) ok_mask |= bit;
    else (void)hipGetLastError();
  }
  return (ok_mask & bit) != 0;
}
// The iterations enqueued on `st`: the points come from host_pts (uploaded first) or are in the scratch's dp already (host_pts == nullptr:
// mcp_track_frame packs them on the device).  BaseFromWorld | mu are left at the head of the scratch's dblk, the weights in dw; *prm_err
// receives the multi-workgroup kernel's give-up flag once the stream has been waited for.
static int refine_enqueue(int n, const mcp_pose_point* host_pts, int ncam, const mcp_camera* cams, const double* cfb, const double bfw[12], int n_iter,
                          const uint8_t* nonlinear, const double* override_sigma, int est, hipStream_t st, unsigned int* prm_err) {
  RefineScratch& rs = refine_scratch();
  const RefineBlock O(n_iter, ncam);
  const size_t blk = O.bytes;
  static const int use_regs = mcp::knobs::track_refine_regs();
  static thread_local unsigned long long regs_refused_mask = 0;      // devices that took the attribute and then refused the launch
  int cur_dev = 0; (void)hipGetDevice(&cur_dev);
  const unsigned long long dbit = 1ull << (cur_dev & 63);
  const bool regs_ok = pose_regs_attr(cur_dev) && !(regs_refused_mask & dbit);
  bool regs = use_regs && regs_ok && n <= PRR_THREADS*PRR_PPT && ncam <= PRR_CAMS;          // the points fit the register-resident kernel, the rig its LDS
  // many points: the iterations over several workgroups (k_pose_refine_multi); MCP_TRACK_REFINE_MULTI = 0 never, 1 whenever the
  // points do not fit the register-resident kernel (default), 2 always
  const int use_multi = mcp::knobs::track_refine_multi();
  const bool multi = n_iter <= PRM_MAX_ITER && ((use_multi == 2 && n >= 64) || (use_multi == 1 && !regs && n > PRR_THREADS*PRR_PPT));
  if (multi) regs = false;
  rs.last_multi = multi;
  rs.route = -1; rs.route_nwg = 0; rs.route_gather = false;
  if (rs.dp.alloc(n) || rs.dblk.alloc(blk) || rs.dw.alloc(n)) return -1;
  auto alloc_plain = [&]() { return rs.dJ.alloc(12*(size_t)n) || rs.dex.alloc(2*(size_t)n) || rs.de2.alloc(n); };
  if (!regs && alloc_plain()) return -1;
  rs.hblk.assign(blk, 0);
  std::memcpy(rs.hblk.data(), bfw, 96);
  std::memcpy(rs.hblk.data() + O.ov, override_sigma, 8*(size_t)n_iter);
  std::memcpy(rs.hblk.data() + O.cfb, cfb, 96*(size_t)ncam);
  std::memcpy(rs.hblk.data() + O.cam, cams, sizeof(mcp_camera)*(size_t)ncam);
  std::memcpy(rs.hblk.data() + O.nl, nonlinear, (size_t)n_iter);
  if (host_pts) ICK(hipMemcpyAsync(rs.dp.p, host_pts, sizeof(mcp_pose_point)*(size_t)n, hipMemcpyHostToDevice, st));
  rs.res_pinned = false;
  if (regs) {
    if (rs.pblk.alloc(blk) || rs.pw.alloc(n)) return -1;
    std::memcpy(rs.pblk.p, rs.hblk.data(), blk);
    std::memset(rs.pw.p, 0, 8*(size_t)n);                       // weights stay zero when a point was not found
    uint8_t* b = rs.pblk.p;
    double* p_bfw = reinterpret_cast<double*>(b);
    hipLaunchKernelGGL(k_pose_refine_regs, dim3(1), dim3(PRR_THREADS), PRR_DYN_LDS, st, n, rs.dp.p, reinterpret_cast<const mcp_camera*>(b + O.cam), reinterpret_cast<const double*>(b + O.cfb),
                       p_bfw, n_iter, (const uint8_t*)(b + O.nl), reinterpret_cast<const double*>(b + O.ov), p_bfw + 12, rs.pw.p, est, ncam);
    if (hipGetLastError() != hipSuccess) {       // the launch was refused (123 KB of dynamic LDS): the plain kernel does the same work from global memory
      regs = false; regs_refused_mask |= dbit;
      if (alloc_plain()) return -1;
    } else rs.res_pinned = true;
  }
  double* d_bfw = reinterpret_cast<double*>(rs.dblk.p); double* d_mu = d_bfw + 12;
  const double* d_ov = reinterpret_cast<const double*>(rs.dblk.p + O.ov); const double* d_cfb = reinterpret_cast<const double*>(rs.dblk.p + O.cfb);
  const mcp_camera* d_cam = reinterpret_cast<const mcp_camera*>(rs.dblk.p + O.cam); const uint8_t* d_nl = rs.dblk.p + O.nl;
  if (!regs) {
    ICK(hipMemcpyAsync(rs.dblk.p, rs.hblk.data(), blk, hipMemcpyHostToDevice, st));
    if (!multi) ICK(hipMemsetAsync(rs.dw.p, 0, 8*(size_t)n, st));             // weights stay zero when no point was found
  }
  *prm_err = 0;
  if (multi) {
    if (rs.dprm.alloc(1)) return -1;
    ICK(hipMemsetAsync(rs.dprm.p, 0, sizeof(PrmScratch), st));
    const int ppw = mcp::knobs::track_refine_ppw();      // points per workgroup
    const int nwg = std::max(1, std::min(PRM_MAX_WG, (n + ppw - 1)/ppw));
    // the median: per-digit global histograms (default), or -- MCP_TRACK_REFINE_GATHER=1, up to 16k points -- all squared errors through
    // every workgroup's LDS with one barrier.  Measured at 8000 points in 16 workgroups: 311 us vs 322 us per ten iterations; the
    // redundant 8000-key selection in every workgroup costs what the two extra barriers of the histogram form cost.
    const bool gather = n <= PRM_GATHER_MAX && mcp::knobs::track_refine_gather();
    size_t dyn = 0;
    if (gather) {
      if (rs.de2all.alloc(2*(size_t)n)) return -1;
      dyn = (size_t)n*sizeof(double);
      static thread_local unsigned long long prm_attr_mask = 0;
      if (!(prm_attr_mask & dbit)) { ICK(hipFuncSetAttribute((const void*)k_pose_refine_multi, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(PRM_GATHER_MAX*sizeof(double)))); prm_attr_mask |= dbit; }
    }
    // the workgroups of this launch wait for each other; should one give up (not all of them resident next to the mapper's kernels), the
    // caller redoes the iterations with the single-workgroup kernel from this copy of the points (refine_redo_single)
    if (rs.dp_keep.alloc(n)) return -1;
    ICK(hipMemcpyAsync(rs.dp_keep.p, rs.dp.p, sizeof(mcp_pose_point)*(size_t)n, hipMemcpyDeviceToDevice, st));
    // (the parameters stay in device memory -- this kernel reads the camera models inside its iterations --, the results go to pinned host memory)
    if (rs.pblk.alloc(blk) || rs.pw.alloc(n)) return -1;
    std::memset(rs.pw.p, 0, 8*(size_t)n);
    hipLaunchKernelGGL(k_pose_refine_multi, dim3(nwg), dim3(PRM_THREADS), dyn, st, n, rs.dp.p, d_cam, d_cfb, d_bfw, n_iter, d_nl, d_ov, rs.dJ.p, rs.dex.p, rs.de2.p, d_mu, rs.pw.p, est, rs.dprm.p,
                       gather ? rs.de2all.p : (double*)nullptr, reinterpret_cast<double*>(rs.pblk.p));
    ICK(hipGetLastError());
    rs.res_pinned = true;
    rs.route_nwg = nwg; rs.route_gather = gather;
    ICK(hipMemcpyAsync(prm_err, &rs.dprm.p->err, sizeof *prm_err, hipMemcpyDeviceToHost, st));
  } else if (!regs)
    hipLaunchKernelGGL(k_pose_refine, dim3(1), dim3(PR_THREADS), 0, st, n, rs.dp.p, d_cam, d_cfb, d_bfw, n_iter, d_nl, d_ov, rs.dJ.p, rs.dex.p, rs.de2.p, d_mu, rs.dw.p, est);
#ifdef MCP_PRR_PROF
  if (regs) {
    ICK(hipStreamSynchronize(st));
    unsigned long long pr[16*8 + 8]; (void)hipMemcpyFromSymbol(pr, HIP_SYMBOL(g_prr_prof), sizeof pr);
    { unsigned long long sv[8]; (void)hipMemcpyFromSymbol(sv, HIP_SYMBOL(g_selv_prof), sizeof sv);
      fprintf(stderr, "[prr prof] last vote select: votes %llu  barrier %llu  scan %llu  further steps %llu  gather+barrier %llu  rank %llu  (steps %llu, %llu keys ranked)\n",
              sv[1] - sv[0], sv[2] - sv[1], sv[3] - sv[2], sv[4] - sv[3], sv[5] - sv[4], sv[6] - sv[5], sv[7] & 0xffffffffull, sv[7] >> 32); }
    fprintf(stderr, "[prr prof] kernel: entry to first iteration %llu  iterations %llu  write-back %llu  (cycles)\n", pr[129] - pr[128], pr[130] - pr[129], pr[131] - pr[130]);
    for (int it = 0; it < n_iter && it < 16; ++it) { const unsigned long long* q = pr + 8*it;
      fprintf(stderr, "[prr prof] it %d%s: points %llu  select %llu  accumulate %llu  reduce-scatter+barrier %llu  sum+barrier %llu  solve %llu  barrier %llu  (cycles)\n", it, nonlinear[it] ? " (re-projection)" : "",
              q[1] - q[0], q[2] - q[1], q[6] - q[2], q[7] - q[6], q[3] - q[7], q[4] - q[3], q[5] - q[4]); }
  }
#endif
  ICK(hipGetLastError());
  rs.route = multi ? 2 : regs ? 0 : 1;
  return 0;
}
// BaseFromWorld | mu (18 doubles) and the last weights to the caller: copies enqueued where the results are on the device; where the kernel
// left them in pinned host memory they are taken from there once the stream has been waited for
static int refine_results_enqueue(RefineScratch& rs, int n, double* back, double* weights_last, hipStream_t st) {
  if (rs.res_pinned) return 0;
  ICK(hipMemcpyAsync(back, rs.dblk.p, 18*sizeof(double), hipMemcpyDeviceToHost, st));
  if (weights_last) ICK(hipMemcpyAsync(weights_last, rs.dw.p, 8*(size_t)n, hipMemcpyDeviceToHost, st));
  return 0;
}
static void refine_results_finish(RefineScratch& rs, int n, double* back, double* weights_last) {
  if (!rs.res_pinned) return;
  std::memcpy(back, rs.pblk.p, 18*sizeof(double));
  if (weights_last) std::memcpy(weights_last, rs.pw.p, 8*(size_t)n);
}
// the multi-workgroup iterations gave up (prm_err): the same iterations again in ONE workgroup, from the kept copy of the points and the
// parameter block still in the scratch's host image; results where refine_enqueue leaves them.  The stream has been waited for.
static int refine_redo_single(int n, int n_iter, int ncam, int est, hipStream_t st) {
  RefineScratch& rs = refine_scratch();
  if (!rs.dp_keep.p || rs.hblk.empty()) return img_fail("pose iterations: nothing kept to redo them from");
  rs.res_pinned = false;
  const RefineBlock O(n_iter, ncam);
  ICK(hipMemcpyAsync(rs.dp.p, rs.dp_keep.p, sizeof(mcp_pose_point)*(size_t)n, hipMemcpyDeviceToDevice, st));
  ICK(hipMemcpyAsync(rs.dblk.p, rs.hblk.data(), rs.hblk.size(), hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(rs.dw.p, 0, 8*(size_t)n, st));
  double* d_bfw = reinterpret_cast<double*>(rs.dblk.p); double* d_mu = d_bfw + 12;
  hipLaunchKernelGGL(k_pose_refine, dim3(1), dim3(PR_THREADS), 0, st, n, rs.dp.p, reinterpret_cast<const mcp_camera*>(rs.dblk.p + O.cam), reinterpret_cast<const double*>(rs.dblk.p + O.cfb),
                     d_bfw, n_iter, (const uint8_t*)(rs.dblk.p + O.nl), reinterpret_cast<const double*>(rs.dblk.p + O.ov), rs.dJ.p, rs.dex.p, rs.de2.p, d_mu, rs.dw.p, est);
  ICK(hipGetLastError());
  return 0;
}
// the tail of the iterations refine_enqueue put on `st`: the results' copies, the wait, the results taken from pinned memory; should a
// workgroup of the multi-workgroup kernel have given up (*prm_err; MCP_TRACK_TEST_PRM_GIVEUP forces it), the same once more after
// refine_redo_single.  `back` gets BaseFromWorld | mu; pts_back, where not null, the pose records each time.
static int refine_collect(int n, int n_iter, int ncam, int est, hipStream_t st, const unsigned int* prm_err, mcp_pose_point* pts_back, double back[18], double* weights_last) {
  RefineScratch& rs = refine_scratch();
  auto fetch = [&]() -> int {
    if (pts_back) ICK(hipMemcpyAsync(pts_back, rs.dp.p, sizeof(mcp_pose_point)*(size_t)n, hipMemcpyDeviceToHost, st));
    if (refine_results_enqueue(rs, n, back, weights_last, st)) return -1;
    ICK(hipStreamSynchronize(st));
    refine_results_finish(rs, n, back, weights_last);
    return 0;
  };
  if (fetch()) return -1;
  if (*prm_err || (rs.last_multi && mcp::knobs::track_test_prm_giveup())) {
    // a workgroup gave up waiting for the others: the frame is not lost, one workgroup redoes the iterations
    rs.route = -1;
    if (refine_redo_single(n, n_iter, ncam, est, st) || fetch()) return -1;
    rs.route = 3;
  }
  return 0;
}
int mcp_track_pose_refine_m(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cfb, double bfw[12], int n_iter,
                            const uint8_t* nonlinear, const double* override_sigma, double mu_last[6], double* weights_last, int est) {
  if (!mu_last) return img_fail("mcp_track_pose_refine: bad arguments");
  for (int k = 0; k < 6; ++k) mu_last[k] = 0;
  if (n < 0 || ncam <= 0 || n_iter < 0 || !cams || !cfb || !bfw || !est_ok(est) || (n > 0 && !pts) || (n_iter > 0 && (!nonlinear || !override_sigma)))
    return img_fail("mcp_track_pose_refine: bad arguments");
  for (int c = 0; c < ncam; ++c) if (!cam_ok(&cams[c])) return img_fail("mcp_track_pose_refine: bad camera");
  if (n == 0 || n_iter == 0) return 0;
  for (int i = 0; i < n; ++i) if (pts[i].cam < 0 || pts[i].cam >= ncam) return img_fail("mcp_track_pose_refine: camera index out of range");
  int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return img_fail("mcp_track_pose_refine: no HIP device");
  hipStream_t st = nullptr;
  unsigned int prm_err = 0;
  double back[18];
  if (refine_enqueue(n, pts, ncam, cams, cfb, bfw, n_iter, nonlinear, override_sigma, est, st, &prm_err) ||
      refine_collect(n, n_iter, ncam, est, st, &prm_err, pts, back, weights_last)) return -1;
  std::memcpy(bfw, back, 96); std::memcpy(mu_last, back + 12, 48);
  return 0;
}

int mcp_track_pose_refine_sharded(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cfb, double bfw[12], int n_iter,
                                  const uint8_t* nonlinear, const double* override_sigma, double mu_last[6], double* weights_last,
                                  mcp_allreduce_fn allreduce, void* user, int rank, int world, int cap) {
  return mcp_track_pose_refine_sharded_m(n, pts, ncam, cams, cfb, bfw, n_iter, nonlinear, override_sigma, mu_last, weights_last, allreduce, user, rank, world, cap, MCP_MEST_TUKEY);
}
int mcp_track_pose_refine_sharded_m(int n, mcp_pose_point* pts, int ncam, const mcp_camera* cams, const double* cfb, double bfw[12], int n_iter,
                                    const uint8_t* nonlinear, const double* override_sigma, double mu_last[6], double* weights_last,
                                    mcp_allreduce_fn allreduce, void* user, int rank, int world, int cap, int est) {
  if (!mu_last) return img_fail("mcp_track_pose_refine_sharded: bad arguments");
  for (int k = 0; k < 6; ++k) mu_last[k] = 0;
  if (n < 0 || ncam <= 0 || n_iter < 0 || !cams || !cfb || !bfw || world < 1 || rank < 0 || rank >= world || cap < n || cap < 1 || (world > 1 && !allreduce) ||
      !est_ok(est) || (n > 0 && !pts) || (n_iter > 0 && (!nonlinear || !override_sigma)))
    return img_fail("mcp_track_pose_refine_sharded: bad arguments");
  for (int c = 0; c < ncam; ++c) if (!cam_ok(&cams[c])) return img_fail("mcp_track_pose_refine_sharded: bad camera");
  for (int i = 0; i < n; ++i) if (pts[i].cam < 0 || pts[i].cam >= ncam) return img_fail("mcp_track_pose_refine_sharded: camera index out of range");
  int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return img_fail("mcp_track_pose_refine_sharded: no HIP device");
  if (n_iter == 0) return 0;      // (a rank without points still joins every collective below)
  struct Scratch { Buf<mcp_pose_point> dp; Buf<mcp_camera> dc; Buf<double> dcfb, dpose, dv6, dJ, dex, de2, dtab, dacc, dw; Buf<unsigned int> dcnt; };
  static thread_local Scratch rs;
  const size_t tab = (size_t)world*cap;
  if (rs.dp.alloc(std::max(n, 1)) || rs.dc.alloc(ncam) || rs.dcfb.alloc(12*(size_t)ncam) || rs.dpose.alloc(12) || rs.dv6.alloc(6) || rs.dJ.alloc(12*(size_t)std::max(n, 1)) ||
      rs.dex.alloc(2*(size_t)std::max(n, 1)) || rs.de2.alloc(std::max(n, 1)) || rs.dtab.alloc(tab + world) || rs.dacc.alloc(28) || rs.dw.alloc(std::max(n, 1)) || rs.dcnt.alloc(1)) return -1;
  hipStream_t st = nullptr;
  if (n) ICK(hipMemcpyAsync(rs.dp.p, pts, sizeof(mcp_pose_point)*(size_t)n, hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(rs.dc.p, cams, sizeof(mcp_camera)*(size_t)ncam, hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(rs.dcfb.p, cfb, 96*(size_t)ncam, hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(rs.dpose.p, bfw, 96, hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(rs.dv6.p, 0, 48, st));
  ICK(hipMemsetAsync(rs.dw.p, 0, 8*(size_t)std::max(n, 1), st));
  for (int it = 0; it < n_iter; ++it) {
    ICK(hipMemsetAsync(rs.dtab.p, 0, (tab + world)*sizeof(double), st));
    ICK(hipMemsetAsync(rs.dcnt.p, 0, sizeof(unsigned int), st));
    if (n) hipLaunchKernelGGL(k_pr_project, dim3((n + 255)/256), dim3(256), 0, st, n, rs.dp.p, (const mcp_camera*)rs.dc.p, (const double*)rs.dcfb.p,
                              (const double*)rs.dpose.p, (const double*)rs.dv6.p, it, (int)(nonlinear[it] != 0), rs.dJ.p, rs.dex.p, rs.de2.p,
                              rs.dtab.p + (size_t)rank*cap, rs.dtab.p + tab + rank, rs.dcnt.p);
    if (world > 1) { ICK(hipStreamSynchronize(st)); if (allreduce(user, rs.dtab.p, tab + world, (void*)st) != 0) return img_fail("mcp_track_pose_refine_sharded: all-reduce hook failed"); }
    hipLaunchKernelGGL(k_pr_accum, dim3(1), dim3(1024), 0, st, n, (const mcp_pose_point*)rs.dp.p, (const double*)rs.dJ.p, (const double*)rs.dex.p, (const double*)rs.de2.p,
                       (const double*)rs.dtab.p, (const double*)(rs.dtab.p + tab), world, cap, override_sigma[it], (int)(it == n_iter - 1), rs.dacc.p, rs.dw.p, est);
    if (world > 1) { ICK(hipStreamSynchronize(st)); if (allreduce(user, rs.dacc.p, 27, (void*)st) != 0) return img_fail("mcp_track_pose_refine_sharded: all-reduce hook failed"); }
    hipLaunchKernelGGL(k_pr_solve, dim3(1), dim3(64), 0, st, (const double*)rs.dacc.p, (const double*)(rs.dtab.p + tab), world, rs.dpose.p, rs.dv6.p);
  }
  if (n) ICK(hipMemcpyAsync(pts, rs.dp.p, sizeof(mcp_pose_point)*(size_t)n, hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(bfw, rs.dpose.p, 96, hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(mu_last, rs.dv6.p, 48, hipMemcpyDeviceToHost, st));
  if (weights_last && n) ICK(hipMemcpyAsync(weights_last, rs.dw.p, 8*(size_t)n, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  return 0;
}

// ---- SmallBlurryImage / Relocaliser --------------------------------------------------------------------------------
// cv::resize's 8U INTER_LINEAR taps [3P-memory]: source coordinate (d+0.5)*scale-0.5 in float, clamped, 11-bit weights
static void sbi_resize_coeffs(int src, int dst, int* idx, short* w0, short* w1) {
  const double scale = (double)src/dst;
  for (int d = 0; d < dst; ++d) {
    float f = (float)((d + 0.5)*scale - 0.5);
    int s0 = (int)floorf(f);
    f -= s0;
    if (s0 < 0) { f = 0; s0 = 0; }
    if (s0 >= src - 1) { f = 0; s0 = src - 1; }
    idx[d] = s0;
    w0[d] = (short)lrintf((1.f - f)*2048.f); w1[d] = (short)lrintf(f*2048.f);
  }
}
// the tables of one SmallBlurryImage: resize taps for a w x h source and
// CVD::convolveGaussian's taps [3P-memory]: half size ceil(3 sigma), exp(-i^2/2 sigma^2), unit sum
static void sbi_tables(int w, int h, double blur, SbiTables& tb) {
  std::memset(&tb, 0, sizeof tb);
  sbi_resize_coeffs(w, SBI_W, tb.xi, tb.xa, tb.xb);
  sbi_resize_coeffs(h, SBI_H, tb.yi, tb.ya, tb.yb);
  tb.ks = std::min(31, (int)std::ceil(3.0*blur));
  double sum = 1.0;
  for (int i = 1; i <= tb.ks; ++i) sum += 2.0*std::exp(-(double)i*i/(2.0*blur*blur));
  tb.k[0] = (float)(1.0/sum);
  for (int i = 1; i < 32; ++i) tb.k[i] = (i <= tb.ks) ? (float)(std::exp(-(double)i*i/(2.0*blur*blur))/sum) : 0.f;
}
int mcp_kf_make_sbi(mcp_kf* k, double blur) {
  if (!k->has_image) return img_fail("mcp_kf_make_sbi: the handle holds no frame");
  if (!(blur > 0)) return img_fail("mcp_kf_make_sbi: blur must be positive");
  ICK(hipSetDevice(k->device));
  if (k->has_sbi) {     // the previous SBI becomes "last frame's" (pointer swap), Tracker.cc: mmpSBILastFrame / mmpSBIThisFrame
    k->sbi_last_small.swap(k->sbi_small); k->sbi_last_templ.swap(k->sbi_templ); k->sbi_last_jacs.swap(k->sbi_jacs);
    k->has_last_sbi = true;
  }
  if (k->sbi_small.alloc(SBI_N) || k->sbi_templ.alloc(SBI_N) || k->sbi_jacs.alloc(2*SBI_N)) return -1;
  SbiTables tb;
  const Level& L = k->lev[0];
  sbi_tables(L.w, L.h, blur, tb);
  hipLaunchKernelGGL(k_sbi_make, dim3(1), dim3(256), 0, k->st, (const uint8_t*)L.img.p, L.w, L.h, tb, k->sbi_small.p, k->sbi_templ.p, k->sbi_jacs.p);
  ICK(hipStreamSynchronize(k->st));
  k->has_sbi = true;
  return 0;
}
int mcp_kf_get_sbi(mcp_kf* k, uint8_t* small_img, float* templ, float* jacs) {
  if (!k->has_sbi) return img_fail("mcp_kf_get_sbi: no SmallBlurryImage made");
  ICK(hipSetDevice(k->device));
  if (small_img) ICK(hipMemcpy(small_img, k->sbi_small.p, SBI_N, hipMemcpyDeviceToHost));
  if (templ) ICK(hipMemcpy(templ, k->sbi_templ.p, SBI_N*sizeof(float), hipMemcpyDeviceToHost));
  if (jacs) ICK(hipMemcpy(jacs, k->sbi_jacs.p, 2*SBI_N*sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}
int mcp_sbi_score(mcp_kf* cur, int n, mcp_kf* const* cands, double* scores, int* best) {
  if (!cur->has_sbi || n < 0) return img_fail("mcp_sbi_score: bad arguments");
  *best = -1;
  if (n == 0) return 0;
  ICK(hipSetDevice(cur->device));
  std::vector<const float*> ptrs(n);
  for (int i = 0; i < n; ++i) ptrs[i] = (cands[i] && cands[i]->has_sbi) ? cands[i]->sbi_templ.p : nullptr;   // "KF doesn't have small blurry image! Skipping"
  if (cur->sbi_ptrs.alloc(n) || cur->sbi_out.alloc(std::max(n, 8))) return -1;
  ICK(hipMemcpyAsync(cur->sbi_ptrs.p, ptrs.data(), sizeof(float*)*(size_t)n, hipMemcpyHostToDevice, cur->st));
  hipLaunchKernelGGL(k_sbi_score, dim3((n + 63)/64), dim3(64), 0, cur->st, (const float*)cur->sbi_templ.p, (const float* const*)cur->sbi_ptrs.p, n, cur->sbi_out.p);
  ICK(hipMemcpyAsync(scores, cur->sbi_out.p, sizeof(double)*(size_t)n, hipMemcpyDeviceToHost, cur->st));
  ICK(hipStreamSynchronize(cur->st));
  double b = std::numeric_limits<double>::max();
  for (int i = 0; i < n; ++i) if (ptrs[i] && scores[i] < b) { b = scores[i]; *best = i; }      // strict <: first smallest, Relocaliser.cc:113
  return 0;
}
int mcp_sbi_iterate(mcp_kf* cur, mcp_kf* target, int iterations, double se2[6], double* score) {
  if (!cur->has_sbi || !target->has_sbi || iterations < 0) return img_fail("mcp_sbi_iterate: both keyframes need a SmallBlurryImage with gradients");
  ICK(hipSetDevice(cur->device));
  if (cur->sbi_out.alloc(8)) return -1;
  hipLaunchKernelGGL(k_sbi_iterate, dim3(1), dim3(256), 0, cur->st, (const float*)cur->sbi_templ.p, (const float*)target->sbi_templ.p, (const float*)target->sbi_jacs.p, iterations, cur->sbi_out.p);
  double o[7];
  ICK(hipMemcpyAsync(o, cur->sbi_out.p, sizeof o, hipMemcpyDeviceToHost, cur->st));
  ICK(hipStreamSynchronize(cur->st));
  std::memcpy(se2, o, 6*sizeof(double)); *score = o[6];
  return 0;
}
// Tracker::CalcSBIRotation's alignment (Tracker.cc:1687-1720): this frame's SBI against the one made before it on this handle
int mcp_sbi_iterate_last(mcp_kf* k, int iterations, double se2[6], double* score) {
  if (!k->has_sbi || !k->has_last_sbi || iterations < 0) return img_fail("mcp_sbi_iterate_last: needs two consecutive SmallBlurryImages on the handle");
  ICK(hipSetDevice(k->device));
  if (k->sbi_out.alloc(8)) return -1;
  hipLaunchKernelGGL(k_sbi_iterate, dim3(1), dim3(256), 0, k->st, (const float*)k->sbi_templ.p, (const float*)k->sbi_last_templ.p, (const float*)k->sbi_last_jacs.p, iterations, k->sbi_out.p);
  double o[7];
  ICK(hipMemcpyAsync(o, k->sbi_out.p, sizeof o, hipMemcpyDeviceToHost, k->st));
  ICK(hipStreamSynchronize(k->st));
  std::memcpy(se2, o, 6*sizeof(double)); *score = o[6];
  return 0;
}
// SmallBlurryImage::SE3fromSE2 (:250-310): two points, three Gauss-Newton steps on SO3 -- here on the host, from the source
// k_motion_prior runs on the device (track_motion.h, __host__ __device__ like the camera functions of ba_device.h)
int mcp_sbi_se3_from_se2(const double se2[6], const mcp_camera* cs, const mcp_camera* ct, double R[9]) {
  if (!cs || !ct || cs->n_inv < 0 || cs->n_inv > MCP_MAX_INV || ct->n_inv < 0 || ct->n_inv > MCP_MAX_INV) return img_fail("mcp_sbi_se3_from_se2: bad camera");
  sbi_se3_from_se2(se2, cs, ct, R);
  return 0;
}

int mcp_track_search(mcp_kf* target, const mcp_camera* cam, const double bfw[12], const double cfb[12], int n, const mcp_td_in* in,
                     int range, int subpix_its, int exhaustive, mcp_td_out* out) {
  if (n < 0 || !target || !cam_ok(cam) || !bfw || !cfb || (n > 0 && (!in || !out))) return img_fail("mcp_track_search: bad arguments");
  if (n == 0) return 0;
  ICK(hipSetDevice(target->device));
  std::vector<DevTdIn> h(n);
  for (int i = 0; i < n; ++i) if (!td_in_dev(in[i], h[i])) return img_fail("mcp_track_search: point without a resident source keyframe");
  Buf<DevTdIn>& din = target->td_in; Buf<mcp_td_out>& dout = target->td_out;
  if (din.alloc(n) || dout.alloc(n)) return -1;
  ICK(hipMemcpyAsync(din.p, h.data(), sizeof(DevTdIn)*(size_t)n, hipMemcpyHostToDevice, target->st));
  hipLaunchKernelGGL(k_track_search, dim3(n), dim3(64), 0, target->st, target->view(), *cam, se3_of12(bfw), se3_of12(cfb), n, (const DevTdIn*)din.p, range, subpix_its, exhaustive, dout.p);
  ICK(hipMemcpyAsync(out, dout.p, sizeof(mcp_td_out)*(size_t)n, hipMemcpyDeviceToHost, target->st));
  ICK(hipStreamSynchronize(target->st));
  return 0;
}

// pack: arguments checked, the camera table and the points of all cameras written to the pinned staging (targets[0]->h_stab / h_bt_in), device
// buffers sized, the staging's way to them listed in `up`.  launch: the kernel, once something has carried the uploads.
static int search_batch_pack(int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double* cfb, const int* n, const mcp_td_in* const* in,
                             mcp_td_out* const* out, int* total_out, int* maxn_out, Uploads* up, bool view = false /* mcp_track_frame's view mode: no caller arrays */) {
  static_assert(sizeof(SearchCam) % 8 == 0 && sizeof(DevTdIn) % 8 == 0, "the frame's upload slice copies 8-byte words");
  *total_out = 0; *maxn_out = 0;
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !targets || !cams || !cfb || !n || !in || (!out && !view)) return img_fail("mcp_track_search_batch: bad arguments");
  int total = 0, maxn = 0;
  for (int c = 0; c < ncam; ++c) {
    if (!targets[c] || n[c] < 0 || !cam_ok(&cams[c]) || targets[c]->device != targets[0]->device || (n[c] > 0 && (!in[c] || (!view && !out[c])))) return img_fail("mcp_track_search_batch: bad arguments");
    total += n[c]; maxn = std::max(maxn, n[c]);
  }
  if (total == 0) return 0;
  mcp_kf* k0 = targets[0];
  ICK(hipSetDevice(k0->device));
  if (k0->h_stab.alloc(MCP_MAX_FRAME_CAMS) || k0->h_bt_in.alloc(total)) return -1;
  SearchCam* tab = k0->h_stab.p; DevTdIn* h = k0->h_bt_in.p;
  int first = 0;
  for (int c = 0; c < ncam; ++c) {
    SearchCam& S = tab[c];
    S.T = targets[c]->view(); S.cam = cams[c]; S.cfb = se3_of12(cfb + 12*c); S.n = n[c]; S.first = first;      // (no mask: this search does not read one)
    for (int i = 0; i < n[c]; ++i) if (!td_in_dev(in[c][i], h[first + i])) return img_fail("mcp_track_search_batch: point without a resident source keyframe");
    first += n[c];
  }
  if (k0->stab.alloc(MCP_MAX_FRAME_CAMS) || k0->bt_in.alloc(total) || k0->bt_out.alloc(total)) return -1;
  up->add(tab, k0->stab.p, sizeof(SearchCam)*(size_t)ncam);
  up->add(h, k0->bt_in.p, sizeof(DevTdIn)*(size_t)total);
  *total_out = total; *maxn_out = maxn;
  return 0;
}
static int search_batch_launch(int ncam, mcp_kf* k0, int maxn, const double bfw[12], int range, int subpix_its, int exhaustive, mcp_td_out* host_out, mcp_pose_point* pose_pts) {
  hipLaunchKernelGGL(k_track_search_batch, dim3(maxn, ncam), dim3(64), 0, k0->st, (const SearchCam*)k0->stab.p, se3_of12(bfw), (const DevTdIn*)k0->bt_in.p, range, subpix_its, exhaustive, k0->bt_out.p,
                     host_out, pose_pts);
  ICK(hipGetLastError());
  return 0;
}
// SearchForPoints of every camera of a frame in one launch (the per-camera loops of Tracker::TrackMap, src/Tracker.cc:985-1030, 1299-1384)
// (the launch on targets[0]->st, results left in targets[0]->bt_out in camera-major order; *total_out = points of all cameras)
static int search_batch_enqueue(int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double bfw[12], const double* cfb, const int* n,
                                const mcp_td_in* const* in, int range, int subpix_its, int exhaustive, mcp_td_out* const* out, int* total_out) {
  int total = 0, maxn = 0;
  *total_out = 0;
  if (!bfw) return img_fail("mcp_track_search_batch: bad arguments");
  Uploads up;
  if (search_batch_pack(ncam, targets, cams, cfb, n, in, out, &total, &maxn, &up)) return -1;
  if (total == 0) return 0;
  if (up.copy(targets[0]->st) || search_batch_launch(ncam, targets[0], maxn, bfw, range, subpix_its, exhaustive, nullptr, nullptr)) return -1;
  *total_out = total;
  return 0;
}
static int search_batch_copy_out(int ncam, mcp_kf* k0, const int* n, mcp_td_out* const* out, int total) {
  // one copy when the caller's per-camera result arrays are the slices of one array (they are laid out like the device buffer)
  hipStream_t st = k0->st;
  bool contiguous = true;
  { mcp_td_out* expect = nullptr;
    for (int c = 0; c < ncam; ++c) { if (!n[c]) continue; if (expect && out[c] != expect) contiguous = false; expect = out[c] + n[c]; } }
  if (contiguous) {
    int c0 = 0; while (c0 < ncam && !n[c0]) ++c0;
    ICK(hipMemcpyAsync(out[c0], k0->bt_out.p, sizeof(mcp_td_out)*(size_t)total, hipMemcpyDeviceToHost, st));
  } else {
    int first = 0;
    for (int c = 0; c < ncam; ++c) {
      if (n[c]) ICK(hipMemcpyAsync(out[c], k0->bt_out.p + first, sizeof(mcp_td_out)*(size_t)n[c], hipMemcpyDeviceToHost, st));
      first += n[c];
    }
  }
  return 0;
}
int mcp_track_search_batch(int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double bfw[12], const double* cfb, const int* n,
                           const mcp_td_in* const* in, int range, int subpix_its, int exhaustive, mcp_td_out* const* out) {
  int total = 0;
  if (search_batch_enqueue(ncam, targets, cams, bfw, cfb, n, in, range, subpix_its, exhaustive, out, &total)) return -1;
  if (total == 0) return 0;
  if (search_batch_copy_out(ncam, targets[0], n, out, total)) return -1;
  ICK(hipStreamSynchronize(targets[0]->st));
  return 0;
}

// One stage of Tracker::TrackMap for a whole frame in ONE submission (include/mcp_img.h): the launches of mcp_kf_make_lite_batch, the search
// (mcp_track_search_batch, or -- with finder states -- mcp_patch_sequences in MCP_PF_TRACK mode, one single-item sequence per point) and
// mcp_track_pose_refine_m back to back on the frame's stream, the TrackerData -> pose-point packing in between done on the device, one wait at
// the end.  Same kernels on the same data as the three calls: identical results.
static int track_sequences_pack(int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double bfw[12], const double* cfb, const int* n,
                                const mcp_td_in* const* in, const int* const* point_key, mcp_pf_state* const* state, int* total_out, Uploads* up) {
  static_assert(sizeof(PfTargetDev) % 8 == 0 && sizeof(PfItemDev) % 8 == 0 && sizeof(mcp_pf_state) % 8 == 0, "the frame's upload slice copies 8-byte words");
  *total_out = 0;
  int total = 0;
  for (int c = 0; c < ncam; ++c) {
    if (!targets[c] || n[c] < 0 || targets[c]->device != targets[0]->device || (n[c] > 0 && (!in[c] || !state[c] || !point_key[c]))) return img_fail("mcp_track_frame: bad arguments");
    total += n[c];
  }
  if (total == 0) return 0;
  mcp_kf* k0 = targets[0];
  if (k0->h_pf_tab.alloc(MCP_MAX_FRAME_CAMS) || k0->h_pf_items.alloc(total) || k0->h_pf_seq.alloc(total + 2) || k0->h_pf_state.alloc(total) || k0->h_pf_state_out.alloc(total)) return -1;
  PfTargetDev* tab = k0->h_pf_tab.p; PfItemDev* h = k0->h_pf_items.p; int* seq = k0->h_pf_seq.p; mcp_pf_state* hs = k0->h_pf_state.p;
  for (int c = 0; c < ncam; ++c) target_of(tab[c], targets[c], cams[c], bfw, cfb + 12*c);
  int first = 0;
  for (int c = 0; c < ncam; ++c) {
    for (int i = 0; i < n[c]; ++i) {
      PfItemDev& d = h[first + i];
      if (!td_in_dev(in[c][i], d.p)) return img_fail("mcp_track_frame: point without a resident source keyframe");
      d.point_key = point_key[c][i]; d.target = c; d.start_x = 0.0; d.start_y = 0.0;
    }
    if (n[c]) std::memcpy(&hs[first], state[c], sizeof(mcp_pf_state)*(size_t)n[c]);
    first += n[c];
  }
  for (int i = 0; i <= total; ++i) seq[i] = i;
  seq[total + 1] = 0;                              // (padding: the ride copies 8-byte words)
  ICK(hipSetDevice(k0->device));
  if (k0->pf_tab.alloc(MCP_MAX_FRAME_CAMS) || k0->pf_items.alloc(total) || k0->pf_seq.alloc(total + 2) || k0->pf_state.alloc(total) || k0->bt_out.alloc(total)) return -1;
  up->add(tab, k0->pf_tab.p, sizeof(PfTargetDev)*(size_t)ncam);
  up->add(h, k0->pf_items.p, sizeof(PfItemDev)*(size_t)total);
  up->add(seq, k0->pf_seq.p, sizeof(int)*(size_t)(total + 1));
  up->add(hs, k0->pf_state.p, sizeof(mcp_pf_state)*(size_t)total);
  *total_out = total;
  return 0;
}
static int track_sequences_launch(mcp_kf* k0, int total, int range, int subpix_its, int exhaustive, mcp_td_out* host_out, mcp_pf_state* host_state, mcp_pose_point* pose_pts) {
  hipLaunchKernelGGL(k_patch_sequences, dim3(total), dim3(64), 0, k0->st, (int)MCP_PF_TRACK, (const PfTargetDev*)k0->pf_tab.p, total, (const int*)k0->pf_seq.p,
                     (const PfItemDev*)k0->pf_items.p, k0->pf_state.p, range, subpix_its, exhaustive, k0->bt_out.p, host_out, host_state, pose_pts);
  ICK(hipGetLastError());
  return 0;
}
int mcp_track_frame(int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                    const uint8_t* const* const* masks, const mcp_camera* cams, double bfw[12], const double* cfb, const int* n,
                    const mcp_td_in* const* in, const int* const* point_key, mcp_pf_state* const* state, int range, int subpix_its, int exhaustive,
                    int n_iter, const uint8_t* nonlinear, const double* override_sigma, int est, mcp_td_out* const* out, mcp_pose_point* pts_out,
                    double mu_last[6], double* weights_last) {
  if (!mu_last) return img_fail("mcp_track_frame: bad arguments");
  for (int k = 0; k < 6; ++k) mu_last[k] = 0;
  const bool view = (out == nullptr);       // results stay in the library's pinned block: mcp_track_frame_view (include/mcp_img.h)
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !targets || !cams || !bfw || !cfb || !n || !in || n_iter < 0 || !est_ok(est) ||
      (n_iter > 0 && (!nonlinear || !override_sigma)) || (imgs && !strides) || (state && !point_key)) return img_fail("mcp_track_frame: bad arguments");
  for (int c = 0; c < ncam; ++c) if (!targets[c] || !cam_ok(&cams[c]) || n[c] < 0 || (n[c] > 0 && !view && !out[c])) return img_fail("mcp_track_frame: bad arguments");
  // every per-point argument is checked BEFORE the first enqueue: an input rejected later would leave launches and copies in flight
  for (int c = 0; c < ncam; ++c) {
    if (targets[c]->device != targets[0]->device || (n[c] > 0 && (!in[c] || (state && (!state[c] || !point_key[c]))))) return img_fail("mcp_track_frame: bad arguments");
    for (int i = 0; i < n[c]; ++i) if (!td_in_resident(in[c][i])) return img_fail("mcp_track_frame: point without a resident source keyframe");
  }
  mcp_kf* k0 = targets[0];
  hipStream_t st = k0->st;
  // ... and whatever fails after it waits for the stream before the stack variables the copies write to (back, prm_err) go away
  // (the map table's Drain does the same for calls that own a table; this one has only the frame's stream)
  struct DrainOnError { hipStream_t st; bool armed; int ncam; mcp_kf* const* targets; bool lite; ~DrainOnError() { if (armed) { (void)hipStreamSynchronize(st); if (lite) (void)lite_batch_finish(ncam, targets); (void)hipGetLastError(); } } };
  DrainOnError drain{st, true, ncam, targets, imgs != nullptr};
  // the search: stateless (mcp_track_search_batch's) or, with finder states, one single-item sequence per point.  Its tables and points are
  // packed on the host while the pyramids run and ride to the device in their next launch; without images they are copied on the stream
  int total = 0, maxn = 0;
  Uploads up;
  auto pack = [&]() -> int {
    return state ? track_sequences_pack(ncam, targets, cams, bfw, cfb, n, in, point_key, state, &total, &up)
                 : search_batch_pack(ncam, targets, cams, cfb, n, in, out, &total, &maxn, &up, view);
  };
  if (imgs) {
    const FrameRide ride = [&](FrameBatch& B) -> int { if (pack()) return -1; up.ride(B); return 0; };
    if (lite_batch_enqueue(ncam, targets, imgs, strides, imgs_on_device, masks, &ride)) return -1;
  }
  ICK(hipSetDevice(k0->device));
  RefineScratch& rs = refine_scratch();
  if (!imgs && pack()) return -1;
  if (total > 0) {
    // the search leaves its results (and the finders' states) in pinned host memory too and writes the pose iterations' records itself
    if (k0->h_bt_out.alloc(total) || rs.dp.alloc(total)) return -1;
    if (!imgs && up.copy(st)) return -1;
    if (state ? track_sequences_launch(k0, total, range, subpix_its, exhaustive, k0->h_bt_out.p, k0->h_pf_state_out.p, rs.dp.p)
              : search_batch_launch(ncam, k0, maxn, bfw, range, subpix_its, exhaustive, k0->h_bt_out.p, rs.dp.p)) return -1;
  }
  unsigned int prm_err = 0;
  double back[18];
  const bool iterate = total > 0 && n_iter > 0;
  if (iterate) {
    if (refine_enqueue(total, nullptr, ncam, cams, cfb, bfw, n_iter, nonlinear, override_sigma, est, st, &prm_err) ||
        refine_collect(total, n_iter, ncam, est, st, &prm_err, pts_out, back, weights_last)) return -1;
  } else {
    if (total > 0 && pts_out) ICK(hipMemcpyAsync(pts_out, rs.dp.p, sizeof(mcp_pose_point)*(size_t)total, hipMemcpyDeviceToHost, st));
    if (total > 0 && weights_last) std::memset(weights_last, 0, 8*(size_t)total);
    ICK(hipStreamSynchronize(st));
  }
  drain.armed = false;
  if (imgs && lite_batch_finish(ncam, targets)) return -1;
  // camera c's results start at view_first[c] of the pinned block (mcp_track_frame_view); copied out for a caller that brought arrays
  int first = 0;
  for (int c = 0; c < ncam; ++c) {
    k0->view_first[c] = first;
    if (n[c] && !view) std::memcpy(out[c], k0->h_bt_out.p + first, sizeof(mcp_td_out)*(size_t)n[c]);
    if (n[c] && state) std::memcpy(state[c], k0->h_pf_state_out.p + first, sizeof(mcp_pf_state)*(size_t)n[c]);
    first += n[c];
  }
  k0->view_first[ncam] = first; k0->view_ncam = ncam;
  if (iterate) { std::memcpy(bfw, back, 96); std::memcpy(mu_last, back + 12, 48); }
  return 0;
}

// the results of camera `cam` of the last mcp_track_frame on this first target, in the library's pinned block (include/mcp_img.h)
const mcp_td_out* mcp_track_frame_view(const mcp_kf* first_target, int cam, int* count) {
  if (count) *count = 0;
  if (!first_target || cam < 0 || cam >= first_target->view_ncam) { img_fail("mcp_track_frame_view: no frame's results for that camera"); return nullptr; }
  const int first = first_target->view_first[cam], m = first_target->view_first[cam + 1] - first;
  if (count) *count = m;
  return m > 0 ? first_target->h_bt_out.p + first : nullptr;
}

// PatchFinder with its members carried from call to call (include/mcp_img.h MCP_PF_*): sequences of items, one finder each
int mcp_patch_sequences(int mode, int n_targets, const mcp_pf_target* targets, int n_seq, const int* seq_start, const mcp_pf_item* items,
                        mcp_pf_state* state, int range, int subpix_its, int exhaustive, mcp_td_out* out) {
  if (mode < MCP_PF_TRACK || mode > MCP_PF_EPI_REFINE || n_targets < 1 || !targets || n_seq < 0 || !seq_start || !state) return img_fail("mcp_patch_sequences: bad arguments");
  if (n_seq == 0) return 0;
  const int total = seq_start[n_seq];
  if (seq_start[0] != 0 || total < 0 || (total > 0 && (!items || !out))) return img_fail("mcp_patch_sequences: bad sequence table");
  for (int q = 0; q < n_seq; ++q) if (seq_start[q + 1] < seq_start[q]) return img_fail("mcp_patch_sequences: bad sequence table");
  mcp_kf* k0 = targets[0].kf;
  if (!k0) return img_fail("mcp_patch_sequences: target without a keyframe");
  std::vector<PfTargetDev> tab(n_targets);
  for (int t = 0; t < n_targets; ++t) {
    const mcp_pf_target& G = targets[t];
    if (!G.kf || !cam_ok(G.cam) || G.kf->device != k0->device) return img_fail("mcp_patch_sequences: bad target");
    target_of(tab[t], G.kf, *G.cam, G.base_from_world, G.cam_from_base);
  }
  std::vector<PfItemDev> h(std::max(total, 1));
  for (int i = 0; i < total; ++i) {
    const mcp_pf_item& I = items[i]; PfItemDev& d = h[i];
    if (I.target < 0 || I.target >= n_targets) return img_fail("mcp_patch_sequences: item with a bad target index");
    if (!td_in_dev(I.point, d.p)) return img_fail("mcp_patch_sequences: point without a resident source keyframe");
    d.point_key = I.point_key; d.target = I.target; d.start_x = I.start_pos[0]; d.start_y = I.start_pos[1];
  }
  ICK(hipSetDevice(k0->device));
  hipStream_t st = k0->st;
  if (k0->pf_tab.alloc(n_targets) || k0->pf_items.alloc(std::max(total, 1)) || k0->pf_seq.alloc(n_seq + 1) || k0->pf_state.alloc(n_seq) || k0->bt_out.alloc(std::max(total, 1))) return -1;
  ICK(hipMemcpyAsync(k0->pf_tab.p, tab.data(), sizeof(PfTargetDev)*(size_t)n_targets, hipMemcpyHostToDevice, st));
  if (total) ICK(hipMemcpyAsync(k0->pf_items.p, h.data(), sizeof(PfItemDev)*(size_t)total, hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(k0->pf_seq.p, seq_start, sizeof(int)*(size_t)(n_seq + 1), hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(k0->pf_state.p, state, sizeof(mcp_pf_state)*(size_t)n_seq, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_patch_sequences, dim3(n_seq), dim3(64), 0, st, mode, (const PfTargetDev*)k0->pf_tab.p, n_seq, (const int*)k0->pf_seq.p,
                     (const PfItemDev*)k0->pf_items.p, k0->pf_state.p, range, subpix_its, exhaustive, k0->bt_out.p);
  ICK(hipGetLastError());
  if (total) ICK(hipMemcpyAsync(out, k0->bt_out.p, sizeof(mcp_td_out)*(size_t)total, hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(state, k0->pf_state.p, sizeof(mcp_pf_state)*(size_t)n_seq, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  return 0;
}

int mcp_track_pose_update(int n, const uint8_t* found, const double* fpos, const double* ipos, const double* sinv, const double* J,
                          double override_sigma, double mu[6], double* wout, double* sigma_out) {
  return mcp_track_pose_update_m(n, found, fpos, ipos, sinv, J, override_sigma, mu, wout, sigma_out, MCP_MEST_TUKEY);
}
int mcp_track_pose_update_m(int n, const uint8_t* found, const double* fpos, const double* ipos, const double* sinv, const double* J,
                          double override_sigma, double mu[6], double* wout, double* sigma_out, int est) {
  if (!est_ok(est)) return img_fail("mcp_track_pose_update: unknown M-estimator");
  for (int k = 0; k < 6; ++k) mu[k] = 0;
  if (sigma_out) *sigma_out = 0;
  if (n <= 0) return 0;
  int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return img_fail("mcp_track_pose_update: no HIP device");
  std::vector<int> slot(n, 0); int ne = 0;
  for (int i = 0; i < n; ++i) { slot[i] = ne; if (found[i]) ++ne; }
  if (wout) std::memset(wout, 0, sizeof(double)*(size_t)n);
  if (ne == 0) return 0;
  // scratch kept across calls (the tracker calls this ~20 times per frame)
  struct PoseScratch { Buf<uint8_t> dfound; Buf<double> dfp, dip, dsi, dJ, dex, de2, dsig, dmu, dw, dhist; Buf<int> dslot; Buf<SelState> dst; };
  static thread_local PoseScratch ps;
  Buf<uint8_t>& dfound = ps.dfound; Buf<double>& dfp = ps.dfp; Buf<double>& dip = ps.dip; Buf<double>& dsi = ps.dsi; Buf<double>& dJ = ps.dJ;
  Buf<double>& dex = ps.dex; Buf<double>& de2 = ps.de2; Buf<double>& dsig = ps.dsig; Buf<double>& dmu = ps.dmu; Buf<double>& dw = ps.dw;
  Buf<double>& dhist = ps.dhist; Buf<int>& dslot = ps.dslot; Buf<SelState>& dst = ps.dst;
  if (dfound.alloc(n) || dfp.alloc(2*(size_t)n) || dip.alloc(2*(size_t)n) || dsi.alloc(n) || dJ.alloc(12*(size_t)n) || dex.alloc(2*(size_t)n) ||
      de2.alloc(ne) || dsig.alloc(4) || dmu.alloc(8) || dw.alloc(n) || dhist.alloc((size_t)SEL_PASSES*SEL_BINS) || dslot.alloc(n) || dst.alloc(SEL_PASSES + 1)) return -1;
  ICK(hipMemcpy(dfound.p, found, (size_t)n, hipMemcpyHostToDevice));
  ICK(hipMemcpy(dfp.p, fpos, 16*(size_t)n, hipMemcpyHostToDevice)); ICK(hipMemcpy(dip.p, ipos, 16*(size_t)n, hipMemcpyHostToDevice));
  ICK(hipMemcpy(dsi.p, sinv, 8*(size_t)n, hipMemcpyHostToDevice)); ICK(hipMemcpy(dJ.p, J, 96*(size_t)n, hipMemcpyHostToDevice));
  ICK(hipMemcpy(dslot.p, slot.data(), sizeof(int)*(size_t)n, hipMemcpyHostToDevice));
  hipStream_t st = nullptr;
  hipLaunchKernelGGL(k_pose_errors, dim3((n + 255)/256), dim3(256), 0, st, n, (const uint8_t*)dfound.p, (const double*)dfp.p, (const double*)dip.p, (const double*)dsi.p, dex.p, de2.p, (const int*)dslot.p);
  if (!(override_sigma > 0)) {         // Tukey::FindSigmaSquared: exact median of the squared errors
    ICK(hipMemsetAsync(dhist.p, 0, (size_t)SEL_PASSES*SEL_BINS*sizeof(double), st));
    const int grid = std::max(1, std::min(256, (ne + SEL_BLOCK*4 - 1)/(SEL_BLOCK*4)));
    for (int p = 0; p < SEL_PASSES; ++p) hipLaunchKernelGGL(k_select_pass, dim3(grid), dim3(SEL_BLOCK), 0, st, p, ne, (const double*)de2.p, dhist.p, dst.p, (unsigned long long)(ne/2));
    hipLaunchKernelGGL(k_select_final, dim3(1), dim3(SEL_BLOCK), 0, st, (const double*)dhist.p, (const SelState*)dst.p, dsig.p + 1);
  }
  hipLaunchKernelGGL(k_tukey_sigma, dim3(1), dim3(64), 0, st, (const double*)(dsig.p + 1), (double)ne, override_sigma, dsig.p, est);
  hipLaunchKernelGGL(k_pose_solve, dim3(1), dim3(256), 0, st, n, (const uint8_t*)dfound.p, (const double*)dex.p, (const double*)dsi.p, (const double*)dJ.p, (const double*)dsig.p, dmu.p, dw.p, est);
  ICK(hipDeviceSynchronize());
  ICK(hipMemcpy(mu, dmu.p, 48, hipMemcpyDeviceToHost));
  if (wout) ICK(hipMemcpy(wout, dw.p, 8*(size_t)n, hipMemcpyDeviceToHost));
  if (sigma_out) ICK(hipMemcpy(sigma_out, dsig.p, 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

// ---- Tracker::FindPVS over a device-resident map-point table (include/mcp_img.h, pvs_kernels.h) ------------------------------------
static size_t tm_align(size_t x) { return (x + 15) & ~(size_t)15; }

// one column of the table: bytes per row, how a row that appears is filled, whether the column exists yet (the rays and the finders are
// created on demand); its block holds the table's capacity in rows.  The table's own code moves blocks; everything else reads row().
enum { FILL_ZERO, FILL_COUNTS /* (1, 0): 1 inlier, 0 outliers */, FILL_NONE };
struct Column {
  size_t bytes; int fill; bool on; Buf<char> block;
  Column(size_t b, int f, bool o) : bytes(b), fill(f), on(o) {}
  char* at(size_t r) const { return block.p + bytes*r; }
};
template <class T, int PER_ROW = 1> struct ColumnOf : Column {       // a row is PER_ROW elements of T
  ColumnOf(int f, bool o) : Column(sizeof(T)*PER_ROW, f, o) {}
  T* row(size_t r = 0) const { return reinterpret_cast<T*>(at(r)); }
};
struct FinderColumn : ColumnOf<mcp_pf_state> { FinderColumn() : ColumnOf(FILL_ZERO, false) {} };

struct mcp_map_points {
  int device = 0; hipStream_t st = nullptr;
  int rows = 0; size_t cap = 0;                      // cap: the rows every live column has room for
  // the columns: points | patch sources (TrackMap) | the persistent finders per (camera, row) | (inlier, outlier) counts | patch rays (9 doubles:
  // AdjustAndUpdate).  A further column is its declaration here and its name in cols (the order grow copies and fills them in): the capacity,
  // the fills and the uploads follow from that.
  ColumnOf<PvsPoint> pts{FILL_ZERO, true}; ColumnOf<TmSrc> src{FILL_ZERO, true};
  FinderColumn states[MCP_MAX_FRAME_CAMS]; int st_ncam = 0;
  ColumnOf<int, 2> cnt{FILL_COUNTS, true}; ColumnOf<double, 9> rays{FILL_NONE, false};
  std::vector<Column*> cols;                         // (pointers into this object: it is never copied)
  mcp_map_points() { cols = {&pts, &src}; for (Column& s : states) cols.push_back(&s); cols.push_back(&cnt); cols.push_back(&rays); }
  mcp_map_points(const mcp_map_points&) = delete;
  std::vector<uint8_t> has_rays;                     // (host: which rows have patch rays)
  // uploads: packed into pinned memory (records | ids), copied (and scattered from the device staging) on st; `staged` marks when the
  // staging may be refilled.  One event serialises every upload, so one pair of blocks serves all columns.
  PinBuf<char> up_in; Buf<char> up_dev;
  hipEvent_t staged = nullptr; bool stage_busy = false;
  // a measurement parcel's fill (mcp_meas_parcel_from_track / _from_refind) may still be reading tr.h_meas / rf.out: a call that has to replace
  // one of them by a larger block waits for the stream first (rewriting them is ordered behind the fill by the stream)
  bool parcel_reads = false;
  std::vector<int> sorted_ids;                       // duplicate check of the uploads by id
  // the source keyframes as (handle, serial).  Slots are reference-counted by the rows that name them (row_slot: the host's copy of each
  // row's slot1); a slot no row names is released and its index reused, so the table walked per call stays as long as the keyframes the
  // map currently uses as sources
  std::vector<std::pair<const mcp_kf*, unsigned long long>> slots; std::map<std::pair<const mcp_kf*, unsigned long long>, int> slot_of;
  std::vector<int> slot_refs, free_slots, row_slot;
  int slot_acquire(const std::pair<const mcp_kf*, unsigned long long>& id) {      // 1 + index, one more reference
    auto it = slot_of.find(id);
    int q;
    if (it != slot_of.end()) q = it->second;
    else {
      if (free_slots.empty()) { q = (int)slots.size(); slots.push_back(id); slot_refs.push_back(0); }
      else { q = free_slots.back(); free_slots.pop_back(); slots[q] = id; }
      slot_of.emplace(id, q);
    }
    ++slot_refs[q];
    return q + 1;
  }
  void slot_release(int slot1) {
    if (slot1 <= 0) return;
    const int q = slot1 - 1;
    if (--slot_refs[q] == 0) { slot_of.erase(slots[q]); slots[q] = std::make_pair((const mcp_kf*)nullptr, 0ull); free_slots.push_back(q); }
  }
  // ---- what each call owns: its scratch, its pinned results, and what its views need; invalidate(): the last call's results are gone ----
  // FindPVS: the camera table (uploaded when it changes), the passes' scratch, the pinned result block
  struct Pvs {
    PinBuf<PvsCam> h_tab; Buf<PvsCam> d_tab; std::vector<PvsCam> tab_last;
    Buf<signed char> lvl; Buf<mcp_pvs_entry> ent; Buf<int> blk_cnt;
    PinBuf<mcp_pvs_entry> h_out; PinBuf<int> h_counts;
    int ncam = 0; int first[MCP_MAX_FRAME_CAMS][MCP_LEVELS] = {}; int count[MCP_MAX_FRAME_CAMS][MCP_LEVELS] = {}; bool ok[MCP_MAX_FRAME_CAMS] = {};
    // mcp_track_map: the lists of its PVS stay in device memory (tm.pvs) until mcp_track_find_pvs_view asks for them
    bool on_device = false; int rows = 0;            // (... laid out camera by camera at c * rows: the table's size at that call)
    int reserve(int nc, int n) {                     // the scratch of the passes over n rows for nc cameras
      const size_t nb = (size_t)nc*std::max(n, 1);
      return (lvl.alloc(nb) || ent.alloc(nb) || blk_cnt.alloc((size_t)nc*((std::max(n, 1) + PVS_BLOCK - 1)/PVS_BLOCK)*MCP_LEVELS) ||
              d_tab.alloc(MCP_MAX_FRAME_CAMS) || h_tab.alloc(MCP_MAX_FRAME_CAMS)) ? -1 : 0;
    }
    void invalidate() { ncam = 0; on_device = false; }
  } pvs;
  // mcp_track_map's scratch and its pinned results
  struct Tm {
    Buf<mcp_pvs_entry> pvs; Buf<int> counts, sel; Buf<unsigned long long> k0, k1; Buf<uint8_t> live, blk; Buf<TmCtl> ctl; Buf<TmSlot> slots;
    Buf<mcp_pose_point> crec, frec; Buf<double> w, J, ex, e2; Buf<mcp_track_map_item> items;
    PinBuf<uint8_t> h_blk; PinBuf<TmSlot> h_slots; PinBuf<mcp_track_map_item> h_items; PinBuf<TmOut> h_res;
    int ncam = 0; int first[MCP_MAX_FRAME_CAMS + 1] = {}; bool items_ok = false;      // (false: the last call kept its items on the device)
    void invalidate() { ncam = 0; }
  } tm;
  // what mcp_track_map_record adds: its scratch and the pinned notes / measurements / record
  struct Tr {
    Buf<uint8_t> flags; Buf<int> tile, seg_start, seg_rows; Buf<TrAcc> acc; Buf<double> seg_w, cfw;
    PinBuf<mcp_track_note> h_notes; PinBuf<mcp_track_meas> h_meas; PinBuf<mcp_track_record> h_rec;
    bool ok = false; int ncam = 0; int meas_first[MCP_MAX_FRAME_CAMS + 1] = {};
    void invalidate() { ok = false; }
  } tr;
  // AdjustAndUpdate write-back and scene depth: the packed inputs (pinned | device) / pinned outputs of mcp_ba_write_back and mcp_scene_depth_robust
  struct Wb {
    PinBuf<char> in; Buf<char> dev; PinBuf<char> out; Buf<double> T, depth; hipEvent_t ev = nullptr;
    std::vector<int> slot, mark; int stamp = 0;      // (mark[row] == stamp: the row was named earlier in this call)
    hipEvent_t t[4] = {nullptr, nullptr, nullptr, nullptr}; bool timed = false;      // mcp_map_points_last_timing: input copy | points | scene depth
    void invalidate() { timed = false; }
  } wb;
  // mcp_track_frame_motion: the tracker's SmallBlurryImages, two sets per camera index (cur[c]: which is this frame's, the other is last
  // frame's; have[c]: the index has made one since creation / mcp_track_motion_reset), the SBI tables (uploaded when they change), the
  // alignments (se2[6], score per camera) and the pinned report
  struct Mo {
    Buf<SbiSet> sets; int cur[MCP_MAX_FRAME_CAMS] = {}; bool have[MCP_MAX_FRAME_CAMS] = {};
    Buf<SbiTables> d_tabs; PinBuf<SbiTables> h_tabs; std::vector<SbiTables> tabs_last;
    Buf<double> se2; PinBuf<mcp_track_motion> h_out;
    int reserve() { return (sets.alloc(2*MCP_MAX_FRAME_CAMS) || d_tabs.alloc(MCP_MAX_FRAME_CAMS) || h_tabs.alloc(MCP_MAX_FRAME_CAMS) || se2.alloc(8*MCP_MAX_FRAME_CAMS) || h_out.alloc(1)) ? -1 : 0; }
    void reset() { for (bool& h : have) h = false; }
  } mo;
  // mcp_track_frame_recover: the relocaliser's SBI tables (blur 2.5; uploaded when they change), the candidates' scores (device | pinned, when
  // the caller wants them), what k_reloc_align leaves per camera, the word that gates the PVS and the pinned report
  struct Rc {
    Buf<SbiTables> d_tabs; PinBuf<SbiTables> h_tabs; std::vector<SbiTables> tabs_last;
    Buf<double> scores; PinBuf<double> h_scores; Buf<RelocCamOut> cam_out; Buf<int> gate; PinBuf<mcp_track_recover> h_out;
    int reserve(int ncand, bool want_scores) {
      return (d_tabs.alloc(MCP_MAX_FRAME_CAMS) || h_tabs.alloc(MCP_MAX_FRAME_CAMS) || scores.alloc((size_t)std::max(ncand, 1)) || (want_scores && h_scores.alloc((size_t)std::max(ncand, 1))) ||
              cam_out.alloc(MCP_MAX_FRAME_CAMS) || gate.alloc(1) || h_out.alloc(1)) ? -1 : 0;
    }
  } rc;
  // mcp_track_pose_cov_enable: the tile partials and counts, the pinned record; what mcp_debug_track_fine_records needs of the last call
  struct Cv {
    Buf<double> part; Buf<int> used; PinBuf<mcp_track_pose_cov_record> h_out;
    bool on = false, ok = false, fine_ok = false; int n_fine = 0; double mu[6] = {};
    int reserve(size_t nb) { const size_t tiles = (nb + COV_TILE - 1)/COV_TILE; return (part.alloc(COV_NPROD*tiles) || used.alloc(tiles) || h_out.alloc(1)) ? -1 : 0; }
    void invalidate() { ok = false; fine_ok = false; }
  } cv;
  // mcp_track_collect_nearest: the graph whose store the frames walk in front of their PVS launch (NULL: the mode is off), the current
  // keyframes' depth means; the report of the last frame call (ok: that call succeeded with the mode on)
  struct Co {
    mcp_map_graph* g = nullptr; mcp_collect_params p = {}; mcp_collect_report last = {}; bool ok = false;
    void invalidate() { ok = false; }
  } co;
  // mcp_map_refind: the packed inputs (pinned | device), the passes' scratch, the pinned results (RfOut | verdict bytes | measurements)
  struct Rf {
    PinBuf<char> in; Buf<char> dev; Buf<uint8_t> flags, vd; Buf<int> blk, first; Buf<RfItem> items; Buf<mcp_refind_meas> cand; PinBuf<char> out;
    size_t meas_off = 0; int view = -1;              // mcp_map_refind_view: where the measurements start in out, how many (-1: none to show)
    void invalidate() { view = -1; }
  } rf;

  ~mcp_map_points() { if (st) (void)hipStreamSynchronize(st); if (st) (void)hipStreamDestroy(st); if (staged) (void)hipEventDestroy(staged); if (wb.ev) (void)hipEventDestroy(wb.ev);
    for (hipEvent_t e : wb.t) if (e) (void)hipEventDestroy(e); }
  TmStates state_ptrs() const { TmStates S; for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) S.s[c] = states[c].row(); return S; }
  int wait_staging() { if (stage_busy) { ICK(hipEventSynchronize(staged)); stage_busy = false; } return 0; }
  hipError_t sync() { const hipError_t e = hipStreamSynchronize(st); if (e == hipSuccess) { stage_busy = false; parcel_reads = false; } return e; }      // (nothing staged is in flight after it)
  // every live column (or `only` this one, about to come to life) gets a block of new_cap rows where it has less, the rows so far copied over
  int reserve(size_t new_cap, Column* only = nullptr) {
    std::vector<Buf<char>> fresh(cols.size());
    bool any = false, stale = false;
    for (size_t i = 0; i < cols.size(); ++i) {
      Column& c = *cols[i];
      if ((only ? &c != only : !c.on) || (c.block.p && c.block.n >= c.bytes*new_cap)) continue;
      if (fresh[i].alloc(c.bytes*new_cap)) return -1;
      if (c.block.p && rows) ICK(hipMemcpyAsync(fresh[i].p, c.block.p, c.bytes*(size_t)rows, hipMemcpyDeviceToDevice, st));
      any = true; stale = stale || c.block.p;
    }
    if (!any) return 0;
    if (stale) ICK(sync());                          // the old blocks are freed below, with nothing in flight on them
    for (size_t i = 0; i < cols.size(); ++i) if (fresh[i].p) cols[i]->block.swap(fresh[i]);
    return 0;
  }
  // rows [first, first + count) of a column read as a row that has just appeared does
  int fill(Column& c, size_t first, size_t count) {
    if (c.fill == FILL_ZERO) ICK(hipMemsetAsync(c.at(first), 0, c.bytes*count, st));
    if (c.fill == FILL_COUNTS) {
      hipLaunchKernelGGL(k_tr_counts_fill, dim3((unsigned)((count + 255)/256)), dim3(256), 0, st, reinterpret_cast<int*>(c.at(0)), (int)first, (int)count);
      ICK(hipGetLastError());
    }
    return 0;
  }
  // rows [rows, new_rows) appear: unusable zero rows without a source, with finders that have seen nothing, the counts of a point that has
  // just been made and no patch rays; the contents so far move to larger blocks when the capacity is passed
  int grow(int new_rows) {
    if (new_rows <= rows) return 0;
    if ((size_t)new_rows > cap) {
      const size_t bigger = std::max<size_t>({(size_t)new_rows, 2*cap, (size_t)1024});
      if (reserve(bigger)) return -1;
      cap = bigger;
    }
    for (Column* c : cols) if (c->on && fill(*c, rows, new_rows - rows)) return -1;
    row_slot.resize(new_rows, 0);
    has_rays.resize(new_rows, 0);                    // (a new row has no patch rays until mcp_map_points_set_rays / _update_rays names it)
    rows = new_rows;
    return 0;
  }
  // a column created on demand comes to life: its block, every row of it filled as a new one; it is live only once both are done
  int ensure(Column& c) {
    if (c.on) return 0;
    if (reserve(std::max<size_t>(cap, 1), &c) || fill(c, 0, c.block.n/c.bytes)) return -1;
    c.on = true;
    return 0;
  }
  // finders for cameras 0 .. ncam-1 (zeroed when new)
  int ensure_states(int ncam) {
    for (int c = st_ncam; c < ncam; ++c) if (ensure(states[c])) return -1;
    st_ncam = std::max(st_ncam, ncam);
    return 0;
  }
};

// the frame mode of the collection (mcp_track_collect_nearest; defined with the map graph below).  collect_frame_check: the refusal of a frame
// whose camera count is not the graph's; collect_frame_reserve: the graph's scratch, before the first enqueue; collect_frame_enqueue: the
// stages on the table's stream at the pose in d_bfw (device memory; NULL: host_bfw is sent there first), *near: the marks the PVS launch
// reads; collect_frame_done: the pinned report into the table once the stream has been waited for
static int collect_frame_check(const std::string& who, const mcp_map_points* m, int ncam);
static int collect_frame_reserve(mcp_map_points* m);
static int collect_frame_enqueue(mcp_map_points* m, int ncam, const double* cfb, const double* host_bfw, const double* d_bfw, const int* d_gate, const uint8_t** near);
static void collect_frame_done(mcp_map_points* m);

// ---- the uploads and read-backs of the columns -----------------------------------------------------------------------------------------
// The rows an upload names: first .. first+count-1, or (by_ids) ids[0 .. count): distinct, none negative, none without a successor.  *top is
// the table's size once they exist.  Every upload refuses in this order: its arguments (have_arrays: the caller's own pointers), the row ids,
// then the values it carries.
static int rows_check(mcp_map_points* m, const std::string& who, bool by_ids, int first, int count, const int* ids, bool have_arrays, int* top) {
  if (!m) return img_fail(who + ": NULL table");
  if (count < 0 || (by_ids ? (count > 0 && !ids) : (first < 0 || (long long)first + count > 0x7fffffffLL)) || (count > 0 && !have_arrays))
    return img_fail(who + ": bad arguments");
  *top = by_ids ? m->rows : first + count;
  if (!by_ids || count == 0) return 0;
  for (int k = 0; k < count; ++k) { if (ids[k] < 0 || ids[k] == 0x7fffffff) return img_fail(who + ": bad row id"); *top = std::max(*top, ids[k] + 1); }
  // distinct ids: checked on a sorted copy (host memory ~ count, whatever the ids' values)
  std::vector<int>& sorted = m->sorted_ids;
  sorted.assign(ids, ids + count);
  std::sort(sorted.begin(), sorted.end());
  for (int k = 1; k < count; ++k) if (sorted[k] == sorted[k - 1]) return img_fail(who + ": row " + std::to_string(sorted[k]) + " appears twice");
  return 0;
}

// One upload into a column (count > 0, the rows checked): the table grows to `top`, pack(k, record) fills record k of col.bytes in the pinned
// staging, and the packed block is copied straight to rows first .. (ids == NULL) -- or, with ids, records and ids go to the device staging
// and scatter(records, ids) launches the column's kernel.  always_scatter: the kernel takes the ranged form too (ids == NULL there).
template <class Pack, class Scatter>
static int column_upload(mcp_map_points* m, Column& col, int first, int count, const int* ids, int top, bool always_scatter, Pack pack, Scatter scatter) {
  ICK(hipSetDevice(m->device));
  if (m->wait_staging()) return -1;
  const bool via_dev = ids || always_scatter;
  const size_t rec_bytes = col.bytes*(size_t)count, o_ids = tm_align(rec_bytes), need = o_ids + (ids ? sizeof(int)*(size_t)count : 0);
  if (m->up_in.alloc(need)) return -1;
  if (via_dev) {
    if (need > m->up_dev.n) ICK(m->sync());           // the device staging is reallocated below
    if (m->up_dev.alloc(need)) return -1;
  }
  if (m->grow(top) || m->ensure(col)) return -1;
  for (int k = 0; k < count; ++k) pack(k, m->up_in.p + col.bytes*(size_t)k);
  if (ids) std::memcpy(m->up_in.p + o_ids, ids, sizeof(int)*(size_t)count);
  if (!via_dev) ICK(hipMemcpyAsync(col.at(first), m->up_in.p, rec_bytes, hipMemcpyHostToDevice, m->st));
  else {
    ICK(hipMemcpyAsync(m->up_dev.p, m->up_in.p, rec_bytes, hipMemcpyHostToDevice, m->st));
    if (ids) ICK(hipMemcpyAsync(m->up_dev.p + o_ids, m->up_in.p + o_ids, sizeof(int)*(size_t)count, hipMemcpyHostToDevice, m->st));
    scatter((const void*)m->up_dev.p, ids ? (const int*)(m->up_dev.p + o_ids) : (const int*)nullptr, dim3((unsigned)((count + 255)/256)));
    ICK(hipGetLastError());
  }
  ICK(hipEventRecord(m->staged, m->st)); m->stage_busy = true;
  return 0;
}

// rows first .. first+count-1 of a column read back (col == NULL: the caller's own arguments were bad) into `out` -- or, out == NULL, into
// `bounce`, sized only once the range has passed; a column not created yet reads as zeros
static int column_get(const mcp_map_points* mc, const std::string& who, const Column* col, int first, int count, void* out, std::vector<char>* bounce = nullptr) {
  if (!mc) return img_fail(who + ": NULL table");
  if (!col || first < 0 || count < 0 || (long long)first + count > mc->rows) return img_fail(who + ": bad arguments");
  if (count == 0) return 0;
  if (!out) { bounce->resize(col->bytes*(size_t)count); out = bounce->data(); }
  if (!col->on) { std::memset(out, 0, col->bytes*(size_t)count); return 0; }
  mcp_map_points* m = const_cast<mcp_map_points*>(mc);
  ICK(hipSetDevice(m->device));
  ICK(hipMemcpyAsync(out, col->at(first), col->bytes*(size_t)count, hipMemcpyDeviceToHost, m->st));
  ICK(m->sync());
  return 0;
}

// camera cam's stretch first[cam] .. first[cam + 1] of a pinned list that holds the cameras one after the other
template <class T> static const T* cam_view(const T* list, const int* first, int cam, int* count) {
  const int k = first[cam + 1] - first[cam];
  if (count) *count = k;
  return k > 0 ? list + first[cam] : nullptr;
}

// a small table built on the host for every call goes to the device only when it differs, byte for byte, from the last one uploaded
template <class T> static int upload_when_changed(std::vector<T>& last, PinBuf<T>& pinned, Buf<T>& dev, const std::vector<T>& now, hipStream_t st) {
  if (last.size() == now.size() && std::memcmp(last.data(), now.data(), sizeof(T)*now.size()) == 0) return 0;
  std::memcpy(pinned.p, now.data(), sizeof(T)*now.size());
  ICK(hipMemcpyAsync(dev.p, pinned.p, sizeof(T)*now.size(), hipMemcpyHostToDevice, st));
  last = now;
  return 0;
}

static int points_upload(mcp_map_points* m, const char* who, bool by_ids, int first, int count, const int* ids, const double* wp, const double* pr, const double* pd,
                         const uint8_t* us) {
  int top = 0;
  if (rows_check(m, who, by_ids, first, count, ids, wp && pr && pd && us, &top)) return -1;
  if (count == 0) return 0;
  return column_upload(m, m->pts, first, count, ids, top, false,
    [&](int k, char* rec) {
      PvsPoint& r = *reinterpret_cast<PvsPoint*>(rec);
      std::memcpy(r.world_pos, wp + 3*(size_t)k, 24); std::memcpy(r.pixel_right_w, pr + 3*(size_t)k, 24); std::memcpy(r.pixel_down_w, pd + 3*(size_t)k, 24);
      r.usable = us[k] ? 1 : 0; r.pad_ = 0;
    },
    [&](const void* recs, const int* d_ids, dim3 grid) {
      hipLaunchKernelGGL(k_map_points_scatter, grid, dim3(256), 0, m->st, m->pts.row(), count, d_ids, (const PvsPoint*)recs);
    });
}

extern "C" {

mcp_map_points* mcp_map_points_create(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { mcp_set_error("mcp_map_points_create: no HIP device available (the HIP path has no CPU fallback)"); return nullptr; }
  int dev = device; if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
  if (dev >= ndev || !gfx950(dev)) { mcp_set_error("mcp_map_points_create: device is not a gfx950 (MI355X)"); return nullptr; }
  if (hipSetDevice(dev) != hipSuccess) { mcp_set_error("hipSetDevice failed"); return nullptr; }
  mcp_map_points* m = new mcp_map_points(); m->device = dev;
  bool ok = hipStreamCreateWithFlags(&m->st, hipStreamNonBlocking) == hipSuccess && hipEventCreateWithFlags(&m->staged, hipEventDisableTiming) == hipSuccess;
  for (hipEvent_t& e : m->wb.t) ok = ok && hipEventCreate(&e) == hipSuccess;
  if (!ok || hipEventCreateWithFlags(&m->wb.ev, hipEventDisableTiming) != hipSuccess) { mcp_set_error("mcp_map_points_create: stream / event creation failed"); delete m; return nullptr; }
  return m;
}
void mcp_map_points_destroy(mcp_map_points* m) { if (m) { (void)hipSetDevice(m->device); delete m; } }
int mcp_map_points_rows(const mcp_map_points* m) { if (!m) return img_fail("mcp_map_points_rows: NULL table"); return m->rows; }

int mcp_map_points_resize(mcp_map_points* m, int rows) {
  if (!m) return img_fail("mcp_map_points_resize: NULL table");
  if (rows < 0) return img_fail("mcp_map_points_resize: bad arguments");
  if (rows <= m->rows) {                                    // the rows past the end are gone; growing again fills them afresh (grow)
    for (int r = rows; r < m->rows && r < (int)m->row_slot.size(); ++r) m->slot_release(m->row_slot[r]);
    if ((int)m->row_slot.size() > rows) m->row_slot.resize(rows);
    if ((int)m->has_rays.size() > rows) m->has_rays.resize(rows);
    m->rows = rows;
    return 0;
  }
  ICK(hipSetDevice(m->device));
  return m->grow(rows);
}

int mcp_map_points_set(mcp_map_points* m, int first, int count, const double* wp, const double* pr, const double* pd, const uint8_t* us) {
  return points_upload(m, "mcp_map_points_set", false, first, count, nullptr, wp, pr, pd, us);
}
int mcp_map_points_update(mcp_map_points* m, int count, const int* ids, const double* wp, const double* pr, const double* pd, const uint8_t* us) {
  return points_upload(m, "mcp_map_points_update", true, 0, count, ids, wp, pr, pd, us);
}

// ---- what the frame calls share (mcp_track_find_pvs, mcp_track_map, mcp_track_map_record, mcp_map_refind) -----------------------------------
static int target_on_table_device(const std::string& who, const mcp_map_points* m, int c, const mcp_kf* k) {
  if (k->device == m->device) return 0;
  return img_fail(who + ": camera " + std::to_string(c) + "'s target is on device " + std::to_string(k->device) + ", the table on device " + std::to_string(m->device));
}

// what an early return after the first enqueue leaves behind: nothing in flight on the table's stream and no error waiting in the runtime;
// (track) no camera table taken for uploaded and no items to view; (lite) the frame's pyramids finished
struct Drain {
  mcp_map_points* m; bool armed; bool track = false; int ncam = 0; mcp_kf* const* lite = nullptr;
  ~Drain() {
    if (!armed) return;
    (void)hipStreamSynchronize(m->st);
    if (lite) { (void)hipStreamSynchronize(lite[0]->st); (void)lite_batch_finish(ncam, lite); }
    if (track) { m->pvs.tab_last.clear(); m->tm.invalidate(); m->cv.invalidate(); }
    (void)hipGetLastError();
  }
};

// the source keyframes of the table as the kernels walk them: `out` (zeroed by the caller) gets the level images of every slot still alive
static void fill_slots(const mcp_map_points* m, TmSlot* out) {
  std::lock_guard<std::mutex> reg(g_kf_mu);
  for (size_t q = 0; q < m->slots.size(); ++q) {
    const mcp_kf* s = m->slots[q].first;
    auto live = s ? g_kf_live.find(s) : g_kf_live.end();
    if (live == g_kf_live.end() || live->second != m->slots[q].second) continue;     // released, destroyed, or its address reused: dead
    for (int l = 0; l < MCP_LEVELS; ++l) { out[q].img[l] = s->lev[l].img.p; out[q].w[l] = s->lev[l].w; out[q].h[l] = s->lev[l].h; }
    out[q].live = 1;
  }
}

// where the cameras' PVS lists go: camera c lists at most cap[c] = min(caps[c], n) rows (caps == NULL: n) from first[c], behind the cameras
// before it; returns the entries all lists take together
struct PvsLayout { int cap[MCP_MAX_FRAME_CAMS], first[MCP_MAX_FRAME_CAMS]; };
static size_t pvs_layout(int ncam, const int* caps, int n, PvsLayout* Y) {
  size_t room = 0;
  for (int c = 0; c < ncam; ++c) { Y->cap[c] = caps ? std::min(caps[c], n) : n; Y->first[c] = (int)room; room += (size_t)Y->cap[c]; }
  return room;
}

// FindPVS of the table's n > 0 rows, enqueued on its stream (m->pvs.reserve has been called): the lists, laid out as Y says, and the counts
// per (camera, level) go to `lists` and `counts`, pinned or device memory.  The launches' errors are the caller's to collect (and to answer
// with tab_last.clear()).
// d_bfw != NULL: the pose is read from there (12 doubles in device memory, left by an earlier kernel of the stream) instead of bfw;
// d_gate != NULL (with d_bfw): the marking pass runs behind that device-side word (k_pvs_mark_gated).
// near != NULL: the marks of a collection enqueued before this (one byte per row, bit c: camera c judges the row).
static int pvs_enqueue(mcp_map_points* m, int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double* cfb, const double* bfw, const PvsLayout& Y,
                       mcp_pvs_entry* lists, int* counts, const double* d_bfw = nullptr, const int* d_gate = nullptr, const uint8_t* near = nullptr) {
  const int n = m->rows, nblk = (n + PVS_BLOCK - 1)/PVS_BLOCK;
  std::vector<PvsCam> tab(ncam);
  for (int c = 0; c < ncam; ++c) {
    PvsCam& C = tab[c];
    std::memset(&C, 0, sizeof(PvsCam));              // (the table is compared byte-wise with the last one uploaded)
    C.cam = cams[c]; C.cfb = se3_of12(cfb + 12*c);
    C.mask0 = mask0_of(targets[c]); C.mask_w = targets[c]->lev[0].w; C.mask_h = targets[c]->lev[0].h;
    C.cap = Y.cap[c]; C.out_first = Y.first[c];
  }
  // the cameras, their CamFromBase, masks and caps rarely change from frame to frame
  mcp_map_points::Pvs& V = m->pvs;
  if (upload_when_changed(V.tab_last, V.h_tab, V.d_tab, tab, m->st)) return -1;
  if (d_bfw && d_gate) hipLaunchKernelGGL(k_pvs_mark_gated, dim3(nblk, ncam), dim3(PVS_BLOCK), 0, m->st, d_gate, (const PvsCam*)V.d_tab.p, d_bfw, m->pts.row(), n, nblk, V.lvl.p, V.ent.p, V.blk_cnt.p, near);
  else if (d_bfw) hipLaunchKernelGGL(k_pvs_mark_at, dim3(nblk, ncam), dim3(PVS_BLOCK), 0, m->st, (const PvsCam*)V.d_tab.p, d_bfw, m->pts.row(), n, nblk, V.lvl.p, V.ent.p, V.blk_cnt.p, near);
  else hipLaunchKernelGGL(k_pvs_mark, dim3(nblk, ncam), dim3(PVS_BLOCK), 0, m->st, (const PvsCam*)V.d_tab.p, se3_of12(bfw), m->pts.row(), n, nblk, V.lvl.p, V.ent.p, V.blk_cnt.p, near);
  hipLaunchKernelGGL(k_pvs_scatter, dim3(nblk, ncam), dim3(PVS_BLOCK), 0, m->st, (const PvsCam*)V.d_tab.p, n, nblk, (const signed char*)V.lvl.p,
                     (const mcp_pvs_entry*)V.ent.p, (const int*)V.blk_cnt.p, lists, counts);
  return 0;
}

int mcp_track_find_pvs(mcp_map_points* m, int ncam, mcp_kf* const* targets, const mcp_camera* cams, const double bfw[12], const double* cfb,
                       const int* caps, mcp_pvs_entry* const* out, int* counts) {
  if (!m) return img_fail("mcp_track_find_pvs: NULL table");
  m->pvs.invalidate(); m->tr.invalidate(); m->cv.invalidate(); m->co.invalidate();
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !targets || !cams || !bfw || !cfb || !caps || !counts) return img_fail("mcp_track_find_pvs: bad arguments");
  for (int c = 0; c < ncam; ++c) {
    if (!targets[c] || !cam_ok(&cams[c]) || caps[c] < 0 || (out && !out[c])) return img_fail("mcp_track_find_pvs: bad arguments for camera " + std::to_string(c));
    if (target_on_table_device("mcp_track_find_pvs", m, c, targets[c])) return -1;
  }
  const bool collect = m->co.g != nullptr;             // mcp_track_collect_nearest: the collection stages in front of the marking pass
  if (collect && collect_frame_check("mcp_track_find_pvs", m, ncam)) return -1;
  for (int k = 0; k < ncam*MCP_LEVELS; ++k) counts[k] = 0;
  ICK(hipSetDevice(m->device));
  mcp_map_points::Pvs& V = m->pvs;
  const int n = m->rows;
  if (n == 0 && !collect) {
    for (int c = 0; c < ncam; ++c) { V.ok[c] = true; for (int l = 0; l < MCP_LEVELS; ++l) { V.first[c][l] = 0; V.count[c][l] = 0; } }
    V.ncam = ncam;
    return 0;
  }
  PvsLayout Y;
  if (V.h_out.alloc(std::max<size_t>(pvs_layout(ncam, caps, n, &Y), 1)) || V.h_counts.alloc((size_t)ncam*MCP_LEVELS) || V.reserve(ncam, n)) return -1;
  if (collect && collect_frame_reserve(m)) return -1;
  const uint8_t* near = nullptr;
  Drain drain{m, collect};
  if (collect && collect_frame_enqueue(m, ncam, cfb, bfw, nullptr, nullptr, &near)) { V.tab_last.clear(); return -1; }
  if (n == 0) std::memset(V.h_counts.p, 0, sizeof(int)*(size_t)ncam*MCP_LEVELS);
  else if (pvs_enqueue(m, ncam, targets, cams, cfb, bfw, Y, V.h_out.p, V.h_counts.p, nullptr, nullptr, near)) { V.tab_last.clear(); return -1; }
  const hipError_t le = hipGetLastError();
  const hipError_t se = m->sync();
  drain.armed = false;
  if (le != hipSuccess) { V.tab_last.clear(); return img_fail(std::string("mcp_track_find_pvs: launch: ") + hipGetErrorString(le)); }
  if (se != hipSuccess) { V.tab_last.clear(); return img_fail(std::string("mcp_track_find_pvs: ") + hipGetErrorString(se)); }
  if (collect) collect_frame_done(m);
  std::memcpy(counts, V.h_counts.p, sizeof(int)*(size_t)ncam*MCP_LEVELS);
  std::string over;
  for (int c = 0; c < ncam; ++c) {
    int first = Y.first[c], all = 0;
    for (int l = 0; l < MCP_LEVELS; ++l) { V.first[c][l] = first; V.count[c][l] = counts[c*MCP_LEVELS + l]; first += counts[c*MCP_LEVELS + l]; all += counts[c*MCP_LEVELS + l]; }
    V.ok[c] = all <= caps[c];
    if (!V.ok[c]) { if (over.empty()) over = "mcp_track_find_pvs: camera " + std::to_string(c) + "'s PVS has " + std::to_string(all) + " entries, its cap is " + std::to_string(caps[c]); continue; }
    if (out && all) std::memcpy(out[c], V.h_out.p + Y.first[c], sizeof(mcp_pvs_entry)*(size_t)all);
  }
  V.ncam = ncam;
  if (!over.empty()) return img_fail(over);
  return 0;
}

const mcp_pvs_entry* mcp_track_find_pvs_view(const mcp_map_points* m, int cam, int level, int* count) {
  if (count) *count = 0;
  if (!m || cam < 0 || cam >= m->pvs.ncam || level < 0 || level >= MCP_LEVELS || !m->pvs.ok[cam]) {
    img_fail("mcp_track_find_pvs_view: the last mcp_track_find_pvs on this table produced no list for that camera / level");
    return nullptr;
  }
  if (m->pvs.on_device) {
    // the lists of the last mcp_track_map: copied to the pinned block on first demand
    mcp_map_points* w = const_cast<mcp_map_points*>(m);
    w->pvs.on_device = false;
    bool ok = hipSetDevice(w->device) == hipSuccess && w->pvs.h_out.alloc((size_t)w->pvs.ncam*std::max(w->pvs.rows, 1)) == 0;      // (the call's layout, whatever the table's size now)
    for (int c = 0; ok && c < w->pvs.ncam; ++c) {
      int all = 0; for (int l = 0; l < MCP_LEVELS; ++l) all += w->pvs.count[c][l];
      if (all) ok = hipMemcpy(w->pvs.h_out.p + w->pvs.first[c][0], w->tm.pvs.p + w->pvs.first[c][0], sizeof(mcp_pvs_entry)*(size_t)all, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) { w->pvs.ncam = 0; img_fail("mcp_track_find_pvs_view: copy of the PVS lists failed"); return nullptr; }
  }
  const int k = m->pvs.count[cam][level];
  if (count) *count = k;
  return k > 0 ? m->pvs.h_out.p + m->pvs.first[cam][level] : nullptr;
}

// ---- TrackMap from the table (include/mcp_img.h mcp_track_map, track_map_kernels.h) -------------------------------------------------
static int source_upload(mcp_map_points* m, const char* what, bool by_ids, int first, int count, const int* ids, const int* keys, mcp_kf* const* kfs,
                         const int* levels, const int* cxy, const uint8_t* fixed) {
  int top = 0;
  if (rows_check(m, what, by_ids, first, count, ids, keys && kfs && levels && cxy && fixed, &top)) return -1;
  if (count == 0) return 0;
  std::vector<unsigned long long> ser(count, 0ull);
  for (int k = 0; k < count; ++k) {
    if (!kfs[k]) continue;
    ser[k] = kf_live_serial(kfs[k]);
    if (!ser[k]) return img_fail(std::string(what) + ": entry " + std::to_string(k) + "'s source keyframe is not a live handle");
    if (kfs[k]->device != m->device) return img_fail(std::string(what) + ": entry " + std::to_string(k) + "'s source keyframe is on another device than the table");
    if (levels[k] < 0 || levels[k] >= MCP_LEVELS) return img_fail(std::string(what) + ": bad source level");
  }
  // (the kernel takes both forms: it also resets the finders of a row whose key changed)
  return column_upload(m, m->src, first, count, ids, top, true,
    [&](int k, char* rec) {
      TmSrc& r = *reinterpret_cast<TmSrc*>(rec);
      r.key = keys[k]; r.slot1 = 0; r.level = 0; r.cx = cxy[2*(size_t)k]; r.cy = cxy[2*(size_t)k + 1]; r.fixed = fixed[k] ? 1 : 0;
      if (kfs[k]) { r.slot1 = m->slot_acquire(std::make_pair((const mcp_kf*)kfs[k], ser[k])); r.level = levels[k]; }
      const int row = ids ? ids[k] : first + k;
      m->slot_release(m->row_slot[row]);                   // (after the acquire: a row that keeps its source keeps the slot)
      m->row_slot[row] = r.slot1;
    },
    [&](const void* recs, const int* d_ids, dim3 grid) {
      hipLaunchKernelGGL(k_tm_source_scatter, grid, dim3(256), 0, m->st, m->src.row(), count, ids ? 0 : first, d_ids, (const TmSrc*)recs, m->state_ptrs(), m->st_ncam);
    });
}
int mcp_map_points_set_source(mcp_map_points* m, int first, int count, const int* keys, mcp_kf* const* kfs, const int* levels, const int* cxy, const uint8_t* fixed) {
  return source_upload(m, "mcp_map_points_set_source", false, first, count, nullptr, keys, kfs, levels, cxy, fixed);
}
int mcp_map_points_update_source(mcp_map_points* m, int count, const int* ids, const int* keys, mcp_kf* const* kfs, const int* levels, const int* cxy, const uint8_t* fixed) {
  return source_upload(m, "mcp_map_points_update_source", true, 0, count, ids, keys, kfs, levels, cxy, fixed);
}
int mcp_map_points_get_states(const mcp_map_points* m, int cam, int first, int count, mcp_pf_state* out) {
  const bool ok = cam >= 0 && cam < MCP_MAX_FRAME_CAMS && (count <= 0 || out);
  return column_get(m, "mcp_map_points_get_states", m && ok ? &m->states[cam] : nullptr, first, count, out);
}

// mcp_track_map may use the register-resident pose kernel (MCP_TRACK_REFINE_REGS is read at every call here)
static bool tm_regs_ok() {
  int dev = 0; (void)hipGetDevice(&dev);
  return pose_regs_attr(dev) && mcp::knobs::track_refine_regs() != 0;
}

// what mcp_track_frame_motion adds to the frame: the 40x30 cameras, the motion model's inputs and its report
struct MotionArg { const mcp_camera* cams_sbi; const mcp_track_motion_params* p; mcp_track_motion* out; };
static bool finite6(const double* a) { for (int k = 0; k < 6; ++k) if (!std::isfinite(a[k])) return false; return true; }
// the refusals the motion model's entries share
static int motion_check(const std::string& who, int ncam, const mcp_camera* cams_sbi, const mcp_track_motion_params* p, const mcp_track_motion* out) {
  if (!p || !out) return img_fail(who + ": NULL motion parameters or motion result");
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS) return img_fail(who + ": bad camera count");
  if (!cams_sbi) return img_fail(who + ": NULL SBI cameras");
  for (int c = 0; c < ncam; ++c) if (!cam_ok(&cams_sbi[c])) return img_fail(who + ": bad SBI camera " + std::to_string(c));
  if (!(p->blur > 0) || !std::isfinite(p->blur)) return img_fail(who + ": blur must be positive");
  if (p->sbi_iterations < 0) return img_fail(who + ": negative SBI iteration count");
  if (p->apply && !(std::isfinite(p->dt) && p->dt > 0)) return img_fail(who + ": dt must be finite and positive when the motion model is applied");
  if (!finite6(p->velocity)) return img_fail(who + ": the velocity is not finite");
  return 0;
}

// what mcp_track_frame_recover adds to that: the candidate list, the relocaliser's parameters, its report and the scores
struct RecoverArg {
  int ncand; mcp_kf* const* kf; const int* cam; const double* cfw; const mcp_track_recover_params* p; mcp_track_recover* out; double* scores;
};
// its refusals behind TrackFrame::check's NULL structs; live[i]: candidate i is a live keyframe handle with an SBI that is none of the frame's targets (the others are skipped)
static int recover_check(const std::string& who, const mcp_map_points* m, int ncam, mcp_kf* const* targets, const mcp_track_motion_params* mp, const RecoverArg& rc,
                         std::vector<uint8_t>& live) {
  if (mp->apply) return img_fail(who + ": the motion model is not applied on a recovery frame (motion apply must be 0)");
  if (rc.ncand < 0) return img_fail(who + ": negative candidate count");
  if (rc.ncand > 0 && (!rc.kf || !rc.cam || !rc.cfw)) return img_fail(who + ": NULL candidate arrays");
  if (!(rc.p->reloc_blur > 0) || !std::isfinite(rc.p->reloc_blur)) return img_fail(who + ": reloc_blur must be positive");
  if (rc.p->reloc_iterations < 0) return img_fail(who + ": negative relocaliser iteration count");
  if (!std::isfinite(rc.p->max_score)) return img_fail(who + ": max_score is not finite");
  live.assign((size_t)rc.ncand, 0);
  std::lock_guard<std::mutex> g(g_kf_mu);
  for (int i = 0; i < rc.ncand; ++i) {
    if (rc.cam[i] < 0 || rc.cam[i] >= ncam) return img_fail(who + ": candidate " + std::to_string(i) + " names a camera out of range");
    for (int k = 0; k < 12; ++k) if (!std::isfinite(rc.cfw[12*(size_t)i + k])) return img_fail(who + ": candidate " + std::to_string(i) + "'s pose is not finite");
    if (!rc.kf[i] || g_kf_live.find(rc.kf[i]) == g_kf_live.end()) continue;
    if (rc.kf[i]->device != m->device) return img_fail(who + ": candidate " + std::to_string(i) + " lives on another device than the table");
    bool is_target = false;      // (a target's SBI is the one this call rewrites: it is no keyframe of the map)
    for (int c = 0; c < ncam; ++c) is_target = is_target || rc.kf[i] == targets[c];
    live[i] = (rc.kf[i]->has_sbi && !is_target) ? 1 : 0;
  }
  return 0;
}

// ---- the pose covariance of the last fine iteration (track_cov_kernels.h) -----------------------------------------------------------------
// the two launches on `st`: the record count is n, or *n_dev where given; cap bounds it (the buffers' size) and the grid.  max_wg = 0: the
// library's choice
static int pose_cov_enqueue(hipStream_t st, int n, const int* n_dev, const int* gate, size_t cap, const mcp_pose_point* pts, const double* w, const double* d_cfb,
                            const double* d_refined, const double* d_mu, int max_wg, double* part, int* used, mcp_track_pose_cov_record* h_out) {
  const size_t tiles = std::max<size_t>((cap + COV_TILE - 1)/COV_TILE, 1);
  const unsigned grid = (unsigned)std::min<size_t>(tiles, max_wg > 0 ? (size_t)max_wg : 256);
  hipLaunchKernelGGL(k_pose_cov_tiles, dim3(grid), dim3(COV_TILE), 0, st, n, n_dev, gate, (int)cap, pts, w, d_cfb, d_refined, d_mu, part, used);
  hipLaunchKernelGGL(k_pose_cov_finish, dim3(1), dim3(64), 0, st, n, n_dev, gate, (int)cap, (const double*)part, (const int*)used, h_out);
  ICK(hipGetLastError());
  return 0;
}
static int pose_cov_check(const std::string& who, int n, const mcp_pose_point* pts, const double* weights, int ncam, const double* cfb, const double* refined,
                          const double* mu_last, const mcp_track_pose_cov_record* out) {
  if (n < 0 || ncam < 1 || !cfb || !refined || !mu_last || !out || (n > 0 && (!pts || !weights))) return img_fail(who + ": bad arguments");
  for (int i = 0; i < n; ++i) if (pts[i].cam < 0 || pts[i].cam >= ncam) return img_fail(who + ": camera index out of range");
  return 0;
}
int mcp_track_pose_cov_host(int n, const mcp_pose_point* pts, const double* weights, int ncam, const double* cfb, const double refined[12], const double mu_last[6],
                            mcp_track_pose_cov_record* out) {
  if (pose_cov_check("mcp_track_pose_cov_host", n, pts, weights, ncam, cfb, refined, mu_last, out)) return -1;
  double pose[12], sums[COV_NPROD];
  cov_pose_before(refined, mu_last, pose);
  for (int k = 0; k < COV_NPROD; ++k) sums[k] = 0.0;
  int used = 0;
  for (int first = 0; first < n; first += COV_TILE) {      // the tiles in ascending order, as k_pose_cov_finish adds them
    double part[COV_NPROD];
    used += cov_tile_host(n, first, pts, weights, pose, cfb, part);
    for (int k = 0; k < COV_NPROD; ++k) sums[k] += part[k];
  }
  CovWork W;
  cov_finish(sums, used, W, out);
  return 0;
}
struct CovScratch { Buf<mcp_pose_point> pts; Buf<double> w, blk, part; Buf<int> used; PinBuf<mcp_track_pose_cov_record> h_out; };
static CovScratch& cov_scratch() {      // one per (thread, device), as refine_scratch
  static thread_local std::map<int, std::unique_ptr<CovScratch>> per_dev;
  int dev = 0; (void)hipGetDevice(&dev);
  std::unique_ptr<CovScratch>& p = per_dev[dev];
  if (!p) p.reset(new CovScratch());
  return *p;
}
int mcp_track_pose_cov(int n, const mcp_pose_point* pts, const double* weights, int ncam, const double* cfb, const double refined[12], const double mu_last[6],
                       int max_workgroups, mcp_track_pose_cov_record* out) {
  if (pose_cov_check("mcp_track_pose_cov", n, pts, weights, ncam, cfb, refined, mu_last, out)) return -1;
  if (max_workgroups < 0) return img_fail("mcp_track_pose_cov: negative max_workgroups");
  int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return img_fail("mcp_track_pose_cov: no HIP device");
  CovScratch& cs = cov_scratch();
  const size_t cap = (size_t)std::max(n, 1), tiles = (cap + COV_TILE - 1)/COV_TILE, nblk = 18 + 12*(size_t)ncam;      // (refined | mu | CamFromBase)
  if (cs.pts.alloc(cap) || cs.w.alloc(cap) || cs.blk.alloc(nblk) || cs.part.alloc(COV_NPROD*tiles) || cs.used.alloc(tiles) || cs.h_out.alloc(1)) return -1;
  std::vector<double> hb(nblk);
  std::memcpy(hb.data(), refined, 96); std::memcpy(hb.data() + 12, mu_last, 48); std::memcpy(hb.data() + 18, cfb, 96*(size_t)ncam);
  hipStream_t st = nullptr;
  ICK(hipMemcpy(cs.blk.p, hb.data(), 8*nblk, hipMemcpyHostToDevice));
  if (n > 0) {
    ICK(hipMemcpy(cs.pts.p, pts, sizeof(mcp_pose_point)*(size_t)n, hipMemcpyHostToDevice));
    ICK(hipMemcpy(cs.w.p, weights, 8*(size_t)n, hipMemcpyHostToDevice));
  }
  std::memset(cs.h_out.p, 0, sizeof(mcp_track_pose_cov_record));
  if (pose_cov_enqueue(st, n, nullptr, nullptr, cap, cs.pts.p, cs.w.p, cs.blk.p + 18, cs.blk.p, cs.blk.p + 12, max_workgroups, cs.part.p, cs.used.p, cs.h_out.p)) return -1;
  ICK(hipStreamSynchronize(st));
  *out = *cs.h_out.p;
  return 0;
}
int mcp_track_pose_cov_enable(mcp_map_points* m, int on) {
  if (!m) return img_fail("mcp_track_pose_cov_enable: NULL table");
  m->cv.on = on != 0;
  return 0;
}
int mcp_track_pose_cov_last(const mcp_map_points* m, mcp_track_pose_cov_record* out) {
  if (!m || !out) return img_fail("mcp_track_pose_cov_last: NULL table or record");
  if (!m->cv.ok) return img_fail("mcp_track_pose_cov_last: the last track call on this table did not succeed with mcp_track_pose_cov_enable on");
  *out = *m->cv.h_out.p;
  return 0;
}
int mcp_debug_track_fine_records(const mcp_map_points* mc, int cap, mcp_pose_point* pts, double* weights, double mu_last[6], int* n) {
  if (!mc || !n || !mu_last || cap < 0 || (cap > 0 && (!pts || !weights))) return img_fail("mcp_debug_track_fine_records: bad arguments");
  if (!mc->cv.fine_ok) return img_fail("mcp_debug_track_fine_records: the last track call on this table did not succeed");
  *n = mc->cv.n_fine;
  if (mc->cv.n_fine > cap) return img_fail("mcp_debug_track_fine_records: " + std::to_string(mc->cv.n_fine) + " records, room for " + std::to_string(cap));
  mcp_map_points* m = const_cast<mcp_map_points*>(mc);
  ICK(hipSetDevice(m->device));
  ICK(m->sync());
  if (m->cv.n_fine > 0) {
    ICK(hipMemcpy(pts, m->tm.frec.p, sizeof(mcp_pose_point)*(size_t)m->cv.n_fine, hipMemcpyDeviceToHost));
    ICK(hipMemcpy(weights, m->tm.w.p, 8*(size_t)m->cv.n_fine, hipMemcpyDeviceToHost));
  }
  std::memcpy(mu_last, m->cv.mu, 48);
  return 0;
}
int mcp_debug_last_pose_route(int* route, int* nwg, int* gathered) {
  if (!route || !nwg || !gathered) return img_fail("mcp_debug_last_pose_route: bad arguments");
  const RefineScratch& rs = refine_scratch();
  if (rs.route < 0) return img_fail("mcp_debug_last_pose_route: no pose iterations have succeeded on this thread and device");
  *route = rs.route; *nwg = rs.route_nwg; *gathered = rs.route_gather ? 1 : 0;
  return 0;
}

// ---- the one-call frames: mcp_track_map, mcp_track_map_record, mcp_track_frame_motion, mcp_track_frame_recover --------------------------
// the parameter block of a frame: cameras' search table | camera models | CamFromBase | BaseFromWorld + mu | override sigma x 2 | nonlinear
// flags x 2 | the SBI cameras (with a motion model) | the candidate list (on a recovery frame); at(): those places in the host's or the device's copy
struct TmBlock { TmCam* tab; mcp_camera* cams; double* cfb; double* pm; double* ov; uint8_t* nl; mcp_camera* cams_sbi; RelocCand* cand; };
struct TmBlockLayout {
  size_t o_tab, o_cam, o_cfb, o_pm, o_ov, o_nl, o_cs, o_rc, total;
  TmBlock at(uint8_t* b) const {
    return TmBlock{reinterpret_cast<TmCam*>(b + o_tab), reinterpret_cast<mcp_camera*>(b + o_cam), reinterpret_cast<double*>(b + o_cfb), reinterpret_cast<double*>(b + o_pm),
                   reinterpret_cast<double*>(b + o_ov), b + o_nl, reinterpret_cast<mcp_camera*>(b + o_cs), reinterpret_cast<RelocCand*>(b + o_rc)};
  }
};
static TmBlockLayout tm_block_layout(int ncam, bool mo, bool rc, int ncand) {
  TmBlockLayout L; const size_t cams = tm_align(sizeof(mcp_camera)*(size_t)ncam);
  L.o_tab = 0; L.o_cam = tm_align(sizeof(TmCam)*(size_t)ncam); L.o_cfb = L.o_cam + cams; L.o_pm = L.o_cfb + tm_align(96*(size_t)ncam);
  L.o_ov = L.o_pm + tm_align(18*8); L.o_nl = L.o_ov + tm_align(20*8); L.o_cs = L.o_nl + tm_align(20);
  L.o_rc = L.o_cs + (mo ? cams : 0); L.total = L.o_rc + (rc ? tm_align(sizeof(RelocCand)*(size_t)std::max(ncand, 1)) : 0);
  return L;
}

// a frame of one of the four entries and its stages in the order run() goes through them; each optional stage is entered only with its feature
struct TrackFrame {
  // what the caller gave.  record: the entry takes rp and rec (there once check() has passed); mo, rc: NULL in an entry without them
  std::string who; mcp_map_points* m; int ncam; mcp_kf* const* targets; const uint8_t* const* imgs; const int* strides; int imgs_on_device;
  const uint8_t* const* const* masks; const mcp_camera* cams; double* bfw; const double* cfb; const mcp_track_map_params* prm; mcp_track_map_result* res;
  bool record; const mcp_track_record_params* rp; mcp_track_record* rec; const MotionArg* mo; const RecoverArg* rc;
  // what the call derives once (derive(); cand_live: recover_check's; D, the device's parameter block: reserve()'s)
  hipStream_t st; int n, ncand; size_t NB, n_coarse_max, n_tile, nslot; bool coarse, regs, cov, want_items; PvsLayout Y; TmBlockLayout L; TmParams P; TmCtl* ctl;
  std::vector<uint8_t> cand_live; TmBlock D;
  // what pack() leaves for the SBI kernels
  RelocMakeArgs rma; RelocCurArgs rca; FrameSbiArgs fa; MotionFirst mfirst;

  // every refusal, in the order the entries answer; nothing is enqueued and nothing changes before all of them pass
  int check() {
    if (!m) return img_fail(who + ": NULL table");
    if (record && (!rp || !rec)) return img_fail(who + ": NULL record parameters or record");
    if (record && (!std::isfinite(rp->quality_good) || !std::isfinite(rp->quality_bad))) return img_fail(who + ": a quality threshold is not finite");
    if (mo && (!mo->p || !mo->out)) return img_fail(who + ": NULL motion parameters or motion result");
    if (rc && (!rc->p || !rc->out)) return img_fail(who + ": NULL recover parameters or recover result");
    if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !targets || !cams || !bfw || !cfb || !prm || !res || (imgs && !strides)) return img_fail(who + ": bad arguments");
    if (prm->coarse_max < 0 || prm->coarse_range < 0 || prm->coarse_min < 0 || prm->coarse_subpix_its < 0 || prm->max_patches < 0) return img_fail(who + ": negative cap, range or iteration count");
    if (!est_ok(prm->estimator)) return img_fail(who + ": unknown M-estimator");
    for (int c = 0; c < ncam; ++c) {
      if (!targets[c] || !cam_ok(&cams[c]) || (imgs && !imgs[c])) return img_fail(who + ": bad arguments for camera " + std::to_string(c));
      if (target_on_table_device(who, m, c, targets[c])) return -1;
      for (int d = 0; imgs && d < c; ++d) if (targets[d] == targets[c]) return img_fail(who + ": a keyframe appears twice in a frame with images");
      if (mo && !imgs && !targets[c]->has_image) return img_fail(who + ": camera " + std::to_string(c) + "'s target holds no frame and no images were given");
    }
    if (mo && motion_check(who, ncam, mo->cams_sbi, mo->p, mo->out)) return -1;
    if (m->co.g && collect_frame_check(who, m, ncam)) return -1;      // mcp_track_collect_nearest: the frame's cameras are the graph's
    return rc ? recover_check(who, m, ncam, targets, mo->p, *rc, cand_live) : 0;
  }
  void derive() {
    st = m->st; n = m->rows; ncand = rc ? rc->ncand : 0; nslot = std::max<size_t>(m->slots.size(), 1);
    want_items = !rp || rp->want_items != 0;
    NB = (size_t)ncam*std::max(n, 1);                                // bound of every per-item array: a camera's sets are distinct rows
    coarse = prm->try_coarse && prm->coarse_max > 0; n_coarse_max = coarse ? std::min(NB, (size_t)ncam*prm->coarse_max) : 0;
    n_tile = (NB + TR_BLOCK - 1)/TR_BLOCK; regs = tm_regs_ok();
    cov = m->cv.on;                                                  // mcp_track_pose_cov_enable: two launches behind the fine iterations
    pvs_layout(ncam, nullptr, n, &Y);                                // caps = rows: camera c's list at c * rows
    L = tm_block_layout(ncam, mo != nullptr, rc != nullptr, ncand);
    P.ncam = ncam; P.rows = n; P.try_coarse = prm->try_coarse ? 1 : 0; P.coarse_max = prm->coarse_max; P.coarse_range = prm->coarse_range;
    P.coarse_subpix_its = prm->coarse_subpix_its; P.coarse_min = prm->coarse_min; P.max_patches = prm->max_patches; P.seed = prm->seed;
  }
  // every allocation, before the first enqueue
  int reserve() {
    if (m->ensure_states(ncam)) return -1;
    if (m->tm.pvs.alloc(NB) || m->tm.counts.alloc((size_t)MCP_MAX_FRAME_CAMS*MCP_LEVELS) || m->tm.sel.alloc(NB) || m->tm.k0.alloc(NB) || m->tm.k1.alloc(NB) || m->tm.live.alloc(NB) ||
        m->tm.ctl.alloc(1) || m->tm.slots.alloc(nslot) || m->tm.h_slots.alloc(nslot) || m->tm.crec.alloc(std::max<size_t>(n_coarse_max, 1)) || m->tm.frec.alloc(NB) || m->tm.w.alloc(NB) ||
        m->tm.items.alloc(NB) || (want_items && m->tm.h_items.alloc(NB)) || m->tm.h_res.alloc(1) || m->pvs.reserve(ncam, n)) return -1;
    if ((NB > (size_t)PRR_THREADS*PRR_PPT || !regs) && (m->tm.J.alloc(12*NB) || m->tm.ex.alloc(2*NB) || m->tm.e2.alloc(NB))) return -1;
    if (m->tm.blk.alloc(L.total) || m->tm.h_blk.alloc(L.total)) return -1;
    D = L.at(m->tm.blk.p); ctl = m->tm.ctl.p;
    if (mo && m->mo.reserve()) return -1;
    if (rc && m->rc.reserve(ncand, rc->scores != nullptr)) return -1;
    for (int c = 0; rc && c < ncam; ++c) {      // both SBIs of every target handle, so that the roll in pack_recover() is a pointer swap
      mcp_kf* k = targets[c];
      if (k->sbi_small.alloc(SBI_N) || k->sbi_templ.alloc(SBI_N) || k->sbi_jacs.alloc(2*SBI_N) || k->sbi_last_small.alloc(SBI_N) || k->sbi_last_templ.alloc(SBI_N) ||
          k->sbi_last_jacs.alloc(2*SBI_N)) return -1;
    }
    if (cov && m->cv.reserve(NB)) return -1;
    if (cov) std::memset(m->cv.h_out.p, 0, sizeof(mcp_track_pose_cov_record));        // (valid = 0 unless k_pose_cov_finish runs)
    if (m->co.g && collect_frame_reserve(m)) return -1;
    if (rp) {
      if (m->parcel_reads && m->tr.h_meas.n < NB) ICK(m->sync());       // (a parcel's fill may still read the block replaced below)
      if (m->tr.h_notes.alloc(NB) || m->tr.h_meas.alloc(NB) || m->tr.h_rec.alloc(1) || m->tr.flags.alloc(NB) || m->tr.tile.alloc(n_tile) || m->tr.acc.alloc(1) ||
          m->tr.seg_start.alloc(MCP_MAX_FRAME_CAMS + 1) || m->tr.seg_rows.alloc(NB) || m->tr.seg_w.alloc(NB) || m->tr.cfw.alloc(12*MCP_MAX_FRAME_CAMS) || m->wb.depth.alloc(NB)) return -1;
      std::memset(m->tr.h_rec.p, 0, sizeof(mcp_track_record));          // (the cameras past ncam read as zeros)
    }
    return 0;
  }
  // a recovery frame's packing: the relocaliser's SBI of every camera goes into the target handle's own (mcp_kf_make_sbi's roll: the one
  // before becomes `last`), in camera order; the candidates into the block
  void pack_recover(RelocCand* cd) {
    std::memset(&rma, 0, sizeof rma); std::memset(&rca, 0, sizeof rca);
    for (int c = 0; c < ncam; ++c) {
      mcp_kf* k = targets[c];
      if (k->has_sbi) { k->sbi_last_small.swap(k->sbi_small); k->sbi_last_templ.swap(k->sbi_templ); k->sbi_last_jacs.swap(k->sbi_jacs); k->has_last_sbi = true; }
      k->has_sbi = true;
      const Level& L0 = k->lev[0];
      rma.c[c] = RelocMakeCam{L0.img.p, L0.w, L0.h, k->sbi_small.p, k->sbi_templ.p, k->sbi_jacs.p};
      rca.templ[c] = k->sbi_templ.p;
    }
    for (int i = 0; i < ncand; ++i) {
      cd[i].templ = cand_live[i] ? rc->kf[i]->sbi_templ.p : nullptr; cd[i].jacs = cand_live[i] ? rc->kf[i]->sbi_jacs.p : nullptr;
      cd[i].cam = rc->cam[i]; cd[i].pad = 0;
      std::memcpy(cd[i].cfw, rc->cfw + 12*(size_t)i, 96);
    }
  }
  // a motion frame's: this frame's SBI set of every camera index (the one before becomes last frame's)
  void pack_motion() {
    mcp_map_points::Mo& M = m->mo;
    std::memset(&fa, 0, sizeof fa); std::memset(&mfirst, 0, sizeof mfirst);
    for (int c = 0; c < ncam; ++c) {
      const Level& L0 = targets[c]->lev[0];
      mfirst.v[c] = M.have[c] ? 0 : 1;
      if (M.have[c]) M.cur[c] ^= 1;
      M.have[c] = true;
      FrameSbiCam& F = fa.c[c];
      F.img = L0.img.p; F.w = L0.w; F.h = L0.h; F.first = mfirst.v[c]; F.align = motion_cam_used(*mo->p, c) ? 1 : 0;
      F.cur = M.sets.p + 2*c + M.cur[c]; F.last = M.sets.p + 2*c + (M.cur[c] ^ 1);
    }
  }
  // the host's parameter block and the slots, with the two changes of state that go with them (the targets' SBI roll, Mo::cur / Mo::have):
  // after the pyramids' launch, which rotates the level images the tables point at, and before the uploads
  void pack() {
    std::memset(m->tm.h_blk.p, 0, L.total);
    const TmBlock H = L.at(m->tm.h_blk.p);
    for (int c = 0; c < ncam; ++c) { target_of(H.tab[c], targets[c], cams[c]); H.tab[c].cfb = se3_of12(cfb + 12*c); }
    std::memcpy(H.cams, cams, sizeof(mcp_camera)*(size_t)ncam);
    std::memcpy(H.cfb, cfb, 96*(size_t)ncam); std::memcpy(H.pm, bfw, 96);
    if (mo) std::memcpy(H.cams_sbi, mo->cams_sbi, sizeof(mcp_camera)*(size_t)ncam);
    if (rc) pack_recover(H.cand);
    for (int i = 0; i < 10; ++i) {
      H.ov[i] = i < 6 ? 0.0 : 1.0; H.nl[i] = 1;                                                 // coarse, Tracker.cc:1012-1020
      H.ov[10 + i] = i < 6 ? 0.0 : 16.0; H.nl[10 + i] = (i == 0 || i == 4 || i == 9) ? 1 : 0;   // fine, :1063-1075
    }
    std::memset(m->tm.h_slots.p, 0, sizeof(TmSlot)*nslot);
    fill_slots(m, m->tm.h_slots.p);
    if (mo) pack_motion();
  }
  // the relocaliser: every camera's SBI, the candidates' scores, the winner's alignment and pose per camera, the recovered pose into the pose
  // slot (k_motion_prior reads it as the start) and the word that gates the PVS
  int reloc_enqueue() {
    mcp_map_points::Rc& R = m->rc;
    const mcp_track_recover_params& q = *rc->p;
    std::vector<SbiTables> tabs(ncam);
    for (int c = 0; c < ncam; ++c) sbi_tables(rma.c[c].w, rma.c[c].h, q.reloc_blur, tabs[c]);
    if (upload_when_changed(R.tabs_last, R.h_tabs, R.d_tabs, tabs, st)) return -1;
    std::memset(R.h_out.p, 0, sizeof(mcp_track_recover));
    hipLaunchKernelGGL(k_reloc_make, dim3(ncam), dim3(256), 0, st, rma, (const SbiTables*)R.d_tabs.p);
    if (ncand > 0) hipLaunchKernelGGL(k_reloc_score, dim3((ncand + RELOC_TILE - 1)/RELOC_TILE), dim3(RELOC_TILE), 0, st, ncand, ncam, (const RelocCand*)D.cand, rca, R.scores.p,
                                      rc->scores ? R.h_scores.p : (double*)nullptr);
    hipLaunchKernelGGL(k_reloc_align, dim3(ncam), dim3(256), 0, st, ncand, (const RelocCand*)D.cand, (const double*)R.scores.p, rca, (const mcp_camera*)D.cams_sbi, q.reloc_iterations, R.cam_out.p);
    hipLaunchKernelGGL(k_reloc_pick, dim3(1), dim3(64), 0, st, ncam, (const RelocCamOut*)R.cam_out.p, (const double*)D.cfb, q.max_score, D.pm, R.gate.p, R.h_out.p);
    ICK(hipGetLastError());
    return 0;
  }
  // the motion model, in front of the PVS (which then reads the pose from the block): this frame's SBI of every camera, its alignment against
  // last frame's, the prior into the pose slot
  int motion_prior_enqueue() {
    mcp_map_points::Mo& M = m->mo;
    std::vector<SbiTables> tabs(ncam);
    for (int c = 0; c < ncam; ++c) sbi_tables(fa.c[c].w, fa.c[c].h, mo->p->blur, tabs[c]);
    if (upload_when_changed(M.tabs_last, M.h_tabs, M.d_tabs, tabs, st)) return -1;
    std::memset(M.h_out.p, 0, sizeof(mcp_track_motion));
    hipLaunchKernelGGL(k_frame_sbi, dim3(ncam), dim3(256), 0, st, fa, (const SbiTables*)M.d_tabs.p, mo->p->sbi_iterations, M.se2.p);
    hipLaunchKernelGGL(k_motion_prior, dim3(1), dim3(64), 0, st, ncam, (const double*)M.se2.p, mfirst, (const mcp_camera*)D.cams_sbi, (const double*)D.cfb, D.pm, *mo->p, M.h_out.p);
    ICK(hipGetLastError());
    return 0;
  }
  // FindPVS, lists and counts in device memory (on a recovery frame behind the relocaliser's gate), and the sets
  int pvs_sets_enqueue() {
    // mcp_track_collect_nearest: the collection stages at the pose in the block -- the given one, k_motion_prior's or k_reloc_pick's
    const uint8_t* near = nullptr;
    if (m->co.g && collect_frame_enqueue(m, ncam, cfb, nullptr, D.pm, rc ? m->rc.gate.p : nullptr, &near)) return -1;
    if (n > 0) {
      if (pvs_enqueue(m, ncam, targets, cams, cfb, bfw, Y, m->tm.pvs.p, m->tm.counts.p, mo ? D.pm : nullptr, rc ? m->rc.gate.p : nullptr, near)) return -1;
    } else ICK(hipMemsetAsync(m->tm.counts.p, 0, sizeof(int)*(size_t)MCP_MAX_FRAME_CAMS*MCP_LEVELS, st));
    hipLaunchKernelGGL(k_tm_select, dim3(ncam), dim3(TM_SEL_NT), 0, st, P, (const mcp_pvs_entry*)m->tm.pvs.p, (const int*)m->tm.counts.p, m->src.row(),
                       (const TmSlot*)m->tm.slots.p, m->tm.k0.p, m->tm.k1.p, m->tm.live.p, m->tm.sel.p, ctl);
    return 0;
  }
  // the searches of a round (stage 0: coarse, 1: fine) at the pose in the block
  void search_enqueue(int stage, size_t bound, unsigned max_grid) {
    hipLaunchKernelGGL(k_tm_search, dim3((unsigned)std::min<size_t>(bound, max_grid)), dim3(64), 0, st, P, stage, (const TmCam*)D.tab, (const double*)D.pm, m->pts.row(),
                       m->src.row(), (const TmSlot*)m->tm.slots.p, (const int*)m->tm.sel.p, m->state_ptrs(), ctl, m->tm.items.p, m->tm.crec.p, m->tm.frec.p, m->tm.w.p);
  }
  // its ten pose iterations over at most `bound` records
  int iterate_enqueue(int stage, size_t bound, const int* n_dev, const int* gate, mcp_pose_point* recs) {
    const double* o = D.ov + 10*stage; const uint8_t* f = D.nl + 10*stage; const mcp_camera* d_cams = D.cams; const double* d_cfb = D.cfb;
    if (regs) hipLaunchKernelGGL(k_pose_refine_regs, dim3(1), dim3(PRR_THREADS), PRR_DYN_LDS, st, 0, recs, d_cams, d_cfb, D.pm, 10, f, o, D.pm + 12, m->tm.w.p, prm->estimator, ncam, n_dev, gate);
    if (!regs || bound > (size_t)PRR_THREADS*PRR_PPT)      // (more records than the register-resident kernel holds, or no such kernel)
      hipLaunchKernelGGL(k_pose_refine, dim3(1), dim3(PR_THREADS), 0, st, 0, recs, d_cams, d_cfb, D.pm, 10, f, o, m->tm.J.p, m->tm.ex.p, m->tm.e2.p, D.pm + 12, m->tm.w.p,
                         prm->estimator, n_dev, gate, regs ? PRR_THREADS*PRR_PPT : -1);
    ICK(hipGetLastError());
    return 0;
  }
  // coarse search, the gate, the coarse iterations
  int coarse_enqueue() {
    if (coarse) search_enqueue(0, n_coarse_max, 8192);
    hipLaunchKernelGGL(k_tm_gate, dim3(1), dim3(1), 0, st, P, ctl);
    return coarse ? iterate_enqueue(0, n_coarse_max, &ctl->n_coarse, &ctl->did_coarse, m->tm.crec.p) : 0;
  }
  // fine searches at the current pose, the fine iterations over [C_c, T_c, R_c]
  int fine_enqueue() {
    search_enqueue(1, NB, 16384);
    return iterate_enqueue(1, NB, &ctl->n_fine, nullptr, m->tm.frec.p);
  }
  int cov_enqueue() {      // mm6PoseCovariance of the last fine iteration
    return pose_cov_enqueue(st, 0, &ctl->n_fine, rc ? m->rc.gate.p : nullptr, NB, m->tm.frec.p, m->tm.w.p, D.cfb, D.pm, D.pm + 12, 0, m->cv.part.p, m->cv.used.p, m->cv.h_out.p);
  }
  void motion_update_enqueue() {      // UpdateMotionModel, from the refined pose
    Pose12 start; std::memcpy(start.v, bfw, 96);
    hipLaunchKernelGGL(k_motion_update, dim3(1), dim3(64), 0, st, (const double*)D.pm, start, *mo->p, m->mo.h_out.p);
  }
  // the bookkeeping, from the items, the last weights and the refined pose where the iterations left them
  int record_enqueue() {
    TrParams Q; Q.ncam = ncam; Q.lost = rp->lost ? 1 : 0; Q.min_patches = rp->min_patches; Q.coarse_min = rp->coarse_min; Q.good = rp->quality_good; Q.bad = rp->quality_bad;
    const unsigned grid = (unsigned)std::min<size_t>(n_tile, 2048);
    ICK(hipMemsetAsync(m->tr.acc.p, 0, sizeof(TrAcc), st));
    hipLaunchKernelGGL(k_tr_mark, dim3(grid), dim3(TR_BLOCK), 0, st, Q, (const TmCtl*)ctl, (const TmCam*)D.tab, (const double*)D.pm, (const mcp_track_map_item*)m->tm.items.p, (const double*)m->tm.w.p,
                       m->cnt.row(), m->tr.h_notes.p, m->tr.flags.p, m->tr.tile.p, m->tr.acc.p, m->tr.cfw.p, &m->tr.h_rec.p->cam_from_world[0][0]);
    hipLaunchKernelGGL(k_tr_scatter, dim3(grid), dim3(TR_BLOCK), 0, st, Q, (const TmCtl*)ctl, (const mcp_track_map_item*)m->tm.items.p, (const uint8_t*)m->tr.flags.p,
                       (const int*)m->tr.tile.p, (const TrAcc*)m->tr.acc.p, m->cnt.row(), m->tr.h_meas.p, m->tr.seg_start.p, m->tr.seg_rows.p, m->tr.seg_w.p, m->tr.h_rec.p);
    hipLaunchKernelGGL(k_wb_scene_depth, dim3((unsigned)ncam), dim3(SD_BLOCK), 0, st, (const double*)m->tr.cfw.p, (const int*)nullptr, (const int*)m->tr.seg_start.p,
                       (const int*)m->tr.seg_rows.p, (const double*)m->tr.seg_w.p, m->pts.row(), m->wb.depth.p, &m->tr.h_rec.p->depth[0], (double*)nullptr);
    ICK(hipGetLastError());
    return 0;
  }
  void finish_enqueue() {      // the results into the pinned block, with the items where the caller wants them
    if (!want_items) hipLaunchKernelGGL(k_tr_finish, dim3(1), dim3(64), 0, st, P, (const TmCtl*)ctl, (const double*)D.pm, (const int*)m->tm.counts.p, m->tm.h_res.p);
    else hipLaunchKernelGGL(k_tm_finish, dim3((unsigned)std::min<size_t>((NB*(sizeof(mcp_track_map_item)/8) + 255)/256, 1024)), dim3(256), 0, st, P, (const TmCtl*)ctl, (const double*)m->tm.w.p,
                            (const mcp_track_map_item*)m->tm.items.p, m->tm.h_items.p, (const double*)D.pm, (const int*)m->tm.counts.p, m->tm.h_res.p);
  }
  // what the synchronised stream left in pinned memory, into the caller's structs and the views' bookkeeping; bfw is written last
  int collect() {
    const TmOut& R = *m->tm.h_res.p;
    std::memset(res, 0, sizeof *res);
    res->did_coarse = R.ctl.did_coarse; res->coarse_found = R.ctl.coarse_found;
    int first = 0;
    for (int c = 0; c < ncam; ++c) {
      int off = Y.first[c];
      for (int l = 0; l < MCP_LEVELS; ++l) {
        res->pvs_counts[c][l] = R.counts[c][l];
        m->pvs.first[c][l] = off; m->pvs.count[c][l] = R.counts[c][l]; off += R.counts[c][l];
      }
      m->pvs.ok[c] = true;
      for (int q = 0; q < 3; ++q) res->set_sizes[c][q] = R.ctl.sizes[c][q];
      res->stale[c] = R.ctl.stale[c];
      m->tm.first[c] = first; first += R.ctl.sizes[c][0] + R.ctl.sizes[c][1] + R.ctl.sizes[c][2];
    }
    m->tm.first[ncam] = first; m->tm.ncam = ncam; m->tm.items_ok = want_items;
    if (rp) {
      *rec = *m->tr.h_rec.p;
      m->tr.meas_first[0] = 0;
      for (int c = 0; c < ncam; ++c) m->tr.meas_first[c + 1] = m->tr.meas_first[c] + rec->n_meas[c];
      m->tr.ncam = ncam; m->tr.ok = true;
    }
    m->pvs.ncam = ncam; m->pvs.on_device = true; m->pvs.rows = n;
    std::memcpy(res->mu_last, R.mu, 48);
    m->cv.ok = cov; m->cv.fine_ok = true; m->cv.n_fine = R.ctl.n_fine; std::memcpy(m->cv.mu, R.mu, 48);
    if (m->co.g) collect_frame_done(m);
    if (mo) *mo->out = *m->mo.h_out.p;
    if (rc) {
      *rc->out = *m->rc.h_out.p;
      if (rc->scores && ncand > 0) std::memcpy(rc->scores, m->rc.h_scores.p, sizeof(double)*(size_t)ncand);
      if (rc->out->recovered) std::memset(mo->out->velocity, 0, sizeof mo->out->velocity);      // mv6BaseVelocity = Zeros, Tracker.cc:549
      else { std::memset(rec, 0, sizeof *rec); return 0; }      // no TrackMap ran: the pose as given, no bookkeeping
    }
    std::memcpy(bfw, R.pose, 96);
    return 0;
  }
  int run() {
    if (check()) return -1;
    ICK(hipSetDevice(m->device));
    // the results of the last call are gone from here on (their blocks may be reallocated and rewritten below)
    m->pvs.invalidate(); m->tm.invalidate(); m->tr.invalidate(); m->cv.invalidate(); m->co.invalidate();
    derive();
    if (reserve()) return -1;
    Drain drain{m, true, true, ncam, imgs ? targets : nullptr};
    if (imgs) {
      if (lite_batch_enqueue(ncam, targets, imgs, strides, imgs_on_device, masks)) return -1;
      ICK(hipEventRecord(targets[0]->ev, targets[0]->st));
      ICK(hipStreamWaitEvent(st, targets[0]->ev, 0));
    }
    pack();
    ICK(hipMemcpyAsync(m->tm.blk.p, m->tm.h_blk.p, L.total, hipMemcpyHostToDevice, st));
    ICK(hipMemcpyAsync(m->tm.slots.p, m->tm.h_slots.p, sizeof(TmSlot)*nslot, hipMemcpyHostToDevice, st));
    if (rc && reloc_enqueue()) return -1;
    if (mo && motion_prior_enqueue()) return -1;
    if (pvs_sets_enqueue() || coarse_enqueue() || fine_enqueue()) return -1;
    if (cov && cov_enqueue()) return -1;
    if (mo) motion_update_enqueue();
    if (rp && record_enqueue()) return -1;
    finish_enqueue();
    ICK(hipGetLastError());
    ICK(m->sync());
    drain.armed = false;
    if (imgs && lite_batch_finish(ncam, targets)) return -1;
    return collect();
  }
};

int mcp_track_map(mcp_map_points* m, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                  const uint8_t* const* const* masks, const mcp_camera* cams, double bfw[12], const double* cfb, const mcp_track_map_params* prm,
                  mcp_track_map_result* res) {
  return TrackFrame{"mcp_track_map", m, ncam, targets, imgs, strides, imgs_on_device, masks, cams, bfw, cfb, prm, res, false, nullptr, nullptr, nullptr, nullptr}.run();
}
int mcp_track_map_record(mcp_map_points* m, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                         const uint8_t* const* const* masks, const mcp_camera* cams, double bfw[12], const double* cfb, const mcp_track_map_params* prm,
                         mcp_track_map_result* res, const mcp_track_record_params* rp, mcp_track_record* rec) {
  return TrackFrame{"mcp_track_map_record", m, ncam, targets, imgs, strides, imgs_on_device, masks, cams, bfw, cfb, prm, res, true, rp, rec, nullptr, nullptr}.run();
}
int mcp_track_frame_motion(mcp_map_points* m, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                           const uint8_t* const* const* masks, const mcp_camera* cams, const mcp_camera* cams_sbi, double bfw[12], const double* cfb,
                           const mcp_track_map_params* prm, mcp_track_map_result* res, const mcp_track_record_params* rp, mcp_track_record* rec,
                           const mcp_track_motion_params* mp, mcp_track_motion* out) {
  const MotionArg mo{cams_sbi, mp, out};
  return TrackFrame{"mcp_track_frame_motion", m, ncam, targets, imgs, strides, imgs_on_device, masks, cams, bfw, cfb, prm, res, true, rp, rec, &mo, nullptr}.run();
}
int mcp_track_frame_recover(mcp_map_points* m, int ncam, mcp_kf* const* targets, const uint8_t* const* imgs, const int* strides, int imgs_on_device,
                            const uint8_t* const* const* masks, const mcp_camera* cams, const mcp_camera* cams_sbi, double bfw[12], const double* cfb,
                            const mcp_track_map_params* prm, mcp_track_map_result* res, const mcp_track_record_params* rp, mcp_track_record* rec,
                            const mcp_track_motion_params* mp, mcp_track_motion* out, int ncand, mcp_kf* const* cand_kf, const int* cand_cam,
                            const double* cand_cfw, const mcp_track_recover_params* rprm, mcp_track_recover* rout, double* scores) {
  const MotionArg mo{cams_sbi, mp, out};
  const RecoverArg rc{ncand, cand_kf, cand_cam, cand_cfw, rprm, rout, scores};
  return TrackFrame{"mcp_track_frame_recover", m, ncam, targets, imgs, strides, imgs_on_device, masks, cams, bfw, cfb, prm, res, true, rp, rec, &mo, &rc}.run();
}

int mcp_track_recover_pose_host(const double se2[6], const mcp_camera* cam_sbi, const double cfw_best[12], const double cfb[12], double out_cam_pose[12],
                                double out_bfw[12]) {
  if (!se2 || !cfw_best) return img_fail("mcp_track_recover_pose_host: NULL alignment or candidate pose");
  if (!cam_sbi || !cam_ok(cam_sbi)) return img_fail("mcp_track_recover_pose_host: NULL or bad SBI camera");
  if (out_bfw && !cfb) return img_fail("mcp_track_recover_pose_host: base_from_world wanted without CamFromBase");
  if (!finite6(se2)) return img_fail("mcp_track_recover_pose_host: the alignment is not finite");
  for (int k = 0; k < 12; ++k) if (!std::isfinite(cfw_best[k]) || (cfb && !std::isfinite(cfb[k]))) return img_fail("mcp_track_recover_pose_host: a pose is not finite");
  double pose[12];
  recover_cam_pose(se2, cam_sbi, cfw_best, pose);
  if (out_bfw) recover_base_pose(cfb, pose, out_bfw);
  if (out_cam_pose) std::memcpy(out_cam_pose, pose, sizeof pose);
  return 0;
}

int mcp_track_motion_reset(mcp_map_points* m) {
  if (!m) return img_fail("mcp_track_motion_reset: NULL table");
  m->mo.reset();
  return 0;
}

int mcp_track_motion_get_sbi(const mcp_map_points* mc, int cam, int which, uint8_t* small_img, float* templ, float* jacs) {
  if (!mc) return img_fail("mcp_track_motion_get_sbi: NULL table");
  if (cam < 0 || cam >= MCP_MAX_FRAME_CAMS || which < 0 || which > 1) return img_fail("mcp_track_motion_get_sbi: bad camera index or selector");
  if (!mc->mo.have[cam]) return img_fail("mcp_track_motion_get_sbi: camera index " + std::to_string(cam) + " has made no SmallBlurryImage since the table was created or reset");
  mcp_map_points* m = const_cast<mcp_map_points*>(mc);
  ICK(hipSetDevice(m->device));
  ICK(m->sync());
  const SbiSet* S = m->mo.sets.p + 2*cam + (m->mo.cur[cam] ^ which);
  if (small_img) ICK(hipMemcpy(small_img, S->small_img, SBI_N, hipMemcpyDeviceToHost));
  if (templ) ICK(hipMemcpy(templ, S->templ, SBI_N*sizeof(float), hipMemcpyDeviceToHost));
  if (jacs) ICK(hipMemcpy(jacs, S->jacs, 2*SBI_N*sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int mcp_track_motion_prior_host(int ncam, const double* se2, const mcp_camera* cams_sbi, const double* cfb, const double start[12],
                                const mcp_track_motion_params* p, mcp_track_motion* out) {
  if (motion_check("mcp_track_motion_prior_host", ncam, cams_sbi, p, out)) return -1;
  if (!se2 || !cfb || !start) return img_fail("mcp_track_motion_prior_host: NULL alignments, CamFromBase or start pose");
  double rot[MCP_MAX_FRAME_CAMS][3] = {};
  for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c) {
    const bool used = c < ncam && motion_cam_used(*p, c);
    for (int k = 0; k < 6; ++k) out->se2[c][k] = used ? se2[6*c + k] : 0.0;
    if (used) motion_cam_rotation(se2 + 6*c, cams_sbi + c, cfb + 12*c, rot[c]);
  }
  double prior[12];
  motion_prior(ncam, rot, *p, start, out, prior);
  return 0;
}

int mcp_track_motion_update_host(const double start[12], const double refined[12], const mcp_track_motion_params* p, mcp_track_motion* out) {
  if (!p || !out) return img_fail("mcp_track_motion_update_host: NULL motion parameters or motion result");
  if (!start || !refined) return img_fail("mcp_track_motion_update_host: NULL pose");
  if (p->apply && !(std::isfinite(p->dt) && p->dt > 0)) return img_fail("mcp_track_motion_update_host: dt must be finite and positive when the motion model is applied");
  if (!finite6(p->velocity)) return img_fail("mcp_track_motion_update_host: the velocity is not finite");
  motion_update(start, refined, *p, out->v_new, out->velocity);
  return 0;
}

const mcp_track_note* mcp_track_map_notes_view(const mcp_map_points* m, int cam, int* count) {
  if (count) *count = 0;
  if (!m || !m->tr.ok || cam < 0 || cam >= m->tr.ncam) { img_fail("mcp_track_map_notes_view: the last track / PVS call on this table was no mcp_track_map_record with that camera"); return nullptr; }
  return cam_view(m->tr.h_notes.p, m->tm.first, cam, count);
}
const mcp_track_meas* mcp_track_map_meas_view(const mcp_map_points* m, int cam, int* count) {
  if (count) *count = 0;
  if (!m || !m->tr.ok || cam < 0 || cam >= m->tr.ncam) { img_fail("mcp_track_map_meas_view: the last track / PVS call on this table was no mcp_track_map_record with that camera"); return nullptr; }
  return cam_view(m->tr.h_meas.p, m->tr.meas_first, cam, count);
}

// ---- the count column (include/mcp_img.h mcp_map_points_set_counts) --------------------------------------------------------------------
static int counts_upload(mcp_map_points* m, const std::string& who, bool by_ids, int first, int count, const int* ids, const int* inl, const int* outl) {
  int top = 0;
  if (rows_check(m, who, by_ids, first, count, ids, inl && outl, &top)) return -1;
  for (int k = 0; k < count; ++k)
    if (inl[k] < 1 || outl[k] < 0) return img_fail(who + ": entry " + std::to_string(k) + " has inlier < 1 or outlier < 0");
  if (count == 0) return 0;
  return column_upload(m, m->cnt, first, count, ids, top, false,
    [&](int k, char* rec) { int* r = reinterpret_cast<int*>(rec); r[0] = inl[k]; r[1] = outl[k]; },
    [&](const void* recs, const int* d_ids, dim3 grid) {
      hipLaunchKernelGGL(k_tr_counts_scatter, grid, dim3(256), 0, m->st, m->cnt.row(), count, d_ids, (const int*)recs);
    });
}
int mcp_map_points_set_counts(mcp_map_points* m, int first, int count, const int* inl, const int* outl) {
  return counts_upload(m, "mcp_map_points_set_counts", false, first, count, nullptr, inl, outl);
}
int mcp_map_points_update_counts(mcp_map_points* m, int count, const int* ids, const int* inl, const int* outl) {
  return counts_upload(m, "mcp_map_points_update_counts", true, 0, count, ids, inl, outl);
}
int mcp_map_points_get_counts(const mcp_map_points* m, int first, int count, int* inl, int* outl) {
  std::vector<char> bounce;
  if (column_get(m, "mcp_map_points_get_counts", m ? &m->cnt : nullptr, first, count, nullptr, &bounce)) return -1;
  const int* h = reinterpret_cast<const int*>(bounce.data());
  for (int k = 0; k < count; ++k) { if (inl) inl[k] = h[2*(size_t)k]; if (outl) outl[k] = h[2*(size_t)k + 1]; }
  return 0;
}

const mcp_track_map_item* mcp_track_map_view(const mcp_map_points* m, int cam, int* count) {
  if (count) *count = 0;
  if (!m || cam < 0 || cam >= m->tm.ncam) { img_fail("mcp_track_map_view: the last mcp_track_map on this table produced no items for that camera"); return nullptr; }
  if (!m->tm.items_ok) { img_fail("mcp_track_map_view: the last call on this table was mcp_track_map_record with want_items = 0: no item left the device"); return nullptr; }
  return cam_view(m->tm.h_items.p, m->tm.first, cam, count);
}

// ---- MapMakerServerBase::AddStereoMapPoints of one source keyframe and level (stereo_kernels.h) ----------------------------------------------------
static bool finite12(const double* a) { for (int k = 0; k < 12; ++k) if (!std::isfinite(a[k])) return false; return true; }
static bool kf_live(const mcp_kf* k) { return k && kf_live_serial(k) != 0ull; }
// the checks both entries share: source, level, candidates
static int stereo_check_source(const char* what, mcp_kf* src, const mcp_camera* src_cam, const double* src_cfw, int level, int n_cand, const mcp_int2* cand) {
  if (!kf_live(src)) return img_fail(std::string(what) + ": the source is not a live keyframe handle");
  if (!src->has_image) return img_fail(std::string(what) + ": the source holds no frame");
  if (!cam_ok(src_cam) || !src_cfw || !finite12(src_cfw)) return img_fail(std::string(what) + ": bad source camera or pose");
  if (level < 0 || level >= MCP_LEVELS) return img_fail(std::string(what) + ": level outside 0..3");
  if (n_cand < 0 || (n_cand > 0 && !cand)) return img_fail(std::string(what) + ": bad candidate list");
  const Level& L = src->lev[level];
  for (int i = 0; i < n_cand; ++i)
    if (cand[i].x < 0 || cand[i].y < 0 || cand[i].x >= L.w || cand[i].y >= L.h) return img_fail(std::string(what) + ": a candidate outside the level image");
  return 0;
}
static int stereo_target_dev(const char* what, const mcp_kf* src, const mcp_stereo_target& G, StereoTargetDev& D) {
  if (!kf_live(G.kf)) return img_fail(std::string(what) + ": a target is not a live keyframe handle");
  if (!G.kf->has_image) return img_fail(std::string(what) + ": a target holds no frame");
  if (G.kf->device != src->device) return img_fail(std::string(what) + ": a target lives on another device than the source");
  if (!cam_ok(G.cam) || !finite12(G.cam_from_world)) return img_fail(std::string(what) + ": bad target camera or pose");
  if (!(G.one_pixel_angle > 0) || !std::isfinite(G.one_pixel_angle)) return img_fail(std::string(what) + ": one_pixel_angle must be positive and finite");
  target_of(D, G.kf, *G.cam); D.cfw = se3_of12(G.cam_from_world); D.opa = G.one_pixel_angle;
  return 0;
}

int mcp_stereo_points(mcp_kf* src, const mcp_camera* src_cam, const double src_cfw[12], int level, int n_cand, const mcp_int2* cand,
                      int n_meas, const mcp_stereo_meas* meas, int n_targets, const mcp_stereo_target* targets, int limit,
                      int cap, mcp_stereo_point* out, uint8_t* keep, uint8_t* outcome) {
  static const char* W = "mcp_stereo_points";
  if (stereo_check_source(W, src, src_cam, src_cfw, level, n_cand, cand)) return -1;
  if (n_meas < 0 || (n_meas > 0 && !meas) || n_targets < 0 || (n_targets > 0 && !targets)) return img_fail("mcp_stereo_points: negative count or missing array");
  if (cap < n_cand) return img_fail("mcp_stereo_points: cap < n_cand");
  if (n_cand > 0 && (!out || !keep)) return img_fail("mcp_stereo_points: out and keep are needed");
  for (int m = 0; m < n_meas; ++m)
    if (!std::isfinite(meas[m].root_pos[0]) || !std::isfinite(meas[m].root_pos[1]) || std::fabs(meas[m].root_pos[0]) > 1e9 || std::fabs(meas[m].root_pos[1]) > 1e9)
      return img_fail("mcp_stereo_points: a measurement with a non-finite or huge root position");
  std::vector<StereoTargetDev> tab(std::max(n_targets, 1));
  for (int t = 0; t < n_targets; ++t) if (stereo_target_dev(W, src, targets[t], tab[t])) return -1;
  if (n_cand == 0) return 0;
  ICK(hipSetDevice(src->device));
  hipStream_t st = src->st;
  const size_t nto = (size_t)std::max(n_targets, 1)*n_cand;
  if (src->st_tab.alloc(std::max(n_targets, 1)) || src->st_cand.alloc(n_cand) || src->st_meas.alloc(std::max(n_meas, 1)) || src->st_alive.alloc(n_cand) ||
      src->st_outcome.alloc(nto) || src->st_res.alloc(n_cand) || src->st_counts.alloc(n_targets + 1) || src->h_st_out.alloc(n_cand) ||
      src->h_st_counts.alloc(n_targets + 1) || src->h_st_keep.alloc(n_cand) || src->h_st_outcome.alloc(nto)) return -1;
  StereoSrcDev S; S.cam = *src_cam; S.cfw = se3_of12(src_cfw);
  S.img = src->lev[level].img.p; S.w = src->lev[level].w; S.h = src->lev[level].h; S.level = level;
  if (n_targets) ICK(hipMemcpyAsync(src->st_tab.p, tab.data(), sizeof(StereoTargetDev)*(size_t)n_targets, hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(src->st_cand.p, cand, sizeof(mcp_int2)*(size_t)n_cand, hipMemcpyHostToDevice, st));
  if (n_meas) ICK(hipMemcpyAsync(src->st_meas.p, meas, sizeof(mcp_stereo_meas)*(size_t)n_meas, hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(src->st_counts.p, 0, sizeof(int)*(size_t)(n_targets + 1), st));
  const int nb = (n_cand + 255)/256;
  hipLaunchKernelGGL(k_stereo_thin_meas, dim3(nb), dim3(256), 0, st, n_cand, (const mcp_int2*)src->st_cand.p, n_meas, (const mcp_stereo_meas*)src->st_meas.p,
                     level, src->st_alive.p);
  for (int j = 0; j < n_targets; ++j) {
    if (j > 0)
      hipLaunchKernelGGL(k_stereo_thin_new, dim3(nb), dim3(256), 0, st, j, n_cand, (const mcp_int2*)src->st_cand.p, level, (const int*)src->st_counts.p,
                         (const mcp_stereo_point*)src->h_st_out.p, src->st_alive.p);
    hipLaunchKernelGGL(k_stereo_walk, dim3(n_cand), dim3(64), 0, st, S, (const StereoTargetDev*)src->st_tab.p, j, n_cand, (const mcp_int2*)src->st_cand.p,
                       (const uint8_t*)src->st_alive.p, src->st_res.p, src->st_outcome.p);
    hipLaunchKernelGGL(k_stereo_commit, dim3(1), dim3(STEREO_COMMIT_NT), 0, st, j, n_cand, limit, (const uint8_t*)src->st_alive.p, src->st_outcome.p,
                       (const mcp_stereo_point*)src->st_res.p, src->st_counts.p, src->h_st_out.p);
  }
  ICK(hipGetLastError());
  ICK(hipMemcpyAsync(src->h_st_counts.p, src->st_counts.p, sizeof(int)*(size_t)(n_targets + 1), hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(src->h_st_keep.p, src->st_alive.p, (size_t)n_cand, hipMemcpyDeviceToHost, st));
  if (outcome && n_targets) ICK(hipMemcpyAsync(src->h_st_outcome.p, src->st_outcome.p, (size_t)n_targets*n_cand, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  const int made = src->h_st_counts.p[n_targets];
  if (made < 0 || made > n_cand) return img_fail("mcp_stereo_points: inconsistent device count");
  std::memcpy(out, src->h_st_out.p, sizeof(mcp_stereo_point)*(size_t)made);
  std::memcpy(keep, src->h_st_keep.p, (size_t)n_cand);
  if (outcome && n_targets) std::memcpy(outcome, src->h_st_outcome.p, (size_t)n_targets*n_cand);
  return made;
}

int mcp_stereo_hypotheses(mcp_kf* src, const mcp_camera* src_cam, const double src_cfw[12], int level, int n_cand, const mcp_int2* cand,
                          const mcp_stereo_target* target, int cap, mcp_td_in* out, int* offsets) {
  static const char* W = "mcp_stereo_hypotheses";
  if (stereo_check_source(W, src, src_cam, src_cfw, level, n_cand, cand)) return -1;
  if (!target || !offsets || cap < 0) return img_fail("mcp_stereo_hypotheses: bad arguments");
  StereoTargetDev D;
  if (stereo_target_dev(W, src, *target, D)) return -1;
  offsets[0] = 0;
  if (n_cand == 0) return 0;
  ICK(hipSetDevice(src->device));
  hipStream_t st = src->st;
  if (src->st_cand.alloc(n_cand) || src->st_counts.alloc(n_cand + 1) || src->h_st_counts.alloc(n_cand + 1)) return -1;
  const Se3 Ts = se3_of12(src_cfw);
  const int nb = (n_cand + 255)/256;
  ICK(hipMemcpyAsync(src->st_cand.p, cand, sizeof(mcp_int2)*(size_t)n_cand, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_stereo_hyp_count, dim3(nb), dim3(256), 0, st, *src_cam, Ts, D.cfw, D.opa, level, n_cand, (const mcp_int2*)src->st_cand.p, src->st_counts.p);
  ICK(hipGetLastError());
  ICK(hipMemcpyAsync(src->h_st_counts.p, src->st_counts.p, sizeof(int)*(size_t)n_cand, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  long long total = 0;
  for (int i = 0; i < n_cand; ++i) {
    total += src->h_st_counts.p[i];
    if (total > 0x7fffffff) return img_fail("mcp_stereo_hypotheses: more than INT_MAX hypotheses");
    offsets[i + 1] = (int)total;
  }
  if (!out) return (int)total;
  if (total > cap) return img_fail("mcp_stereo_hypotheses: cap is smaller than the number of hypotheses");
  if (total == 0) return 0;
  if (src->st_hyp.alloc((size_t)total)) return -1;
  ICK(hipMemcpyAsync(src->st_counts.p, offsets, sizeof(int)*(size_t)(n_cand + 1), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_stereo_hyp_fill, dim3(nb), dim3(256), 0, st, *src_cam, Ts, D.cfw, D.opa, level, n_cand, (const mcp_int2*)src->st_cand.p,
                     (const int*)src->st_counts.p, (const mcp_kf*)src, src->st_hyp.p);
  ICK(hipGetLastError());
  ICK(hipMemcpyAsync(out, src->st_hyp.p, sizeof(mcp_td_in)*(size_t)total, hipMemcpyDeviceToHost, st));
  ICK(hipStreamSynchronize(st));
  return (int)total;
}

}  // extern "C"


// ---- AdjustAndUpdate: the write-back of an adjustment into the table (include/mcp_img.h, write_back_kernels.h) -----------------------
namespace {
size_t wb_align(size_t x) { return (x + 15) & ~(size_t)15; }

// the argument checks of the scene-depth lists (nothing is enqueued before they pass); *total = seg_start[n_kf]
int sd_check(const std::string& who, const mcp_map_points* m, int n_kf, const int* seg_start, const int* seg_rows, const double* seg_w, int* total) {
  *total = 0;
  if (n_kf < 0) return img_fail(who + ": negative keyframe count");
  if (n_kf == 0) return 0;
  if (!seg_start) return img_fail(who + ": seg_start is NULL");
  if (seg_start[0] != 0) return img_fail(who + ": seg_start does not begin at 0");
  for (int j = 0; j < n_kf; ++j) if (seg_start[j + 1] < seg_start[j]) return img_fail(who + ": seg_start decreases at keyframe " + std::to_string(j));
  const int tot = seg_start[n_kf];
  if (tot > 0 && (!seg_rows || !seg_w)) return img_fail(who + ": seg_rows / seg_weights is NULL");
  for (int i = 0; i < tot; ++i) {
    if (seg_rows[i] < 0 || seg_rows[i] >= m->rows) return img_fail(who + ": seg_rows[" + std::to_string(i) + "] = " + std::to_string(seg_rows[i]) + " is outside the table");
    if (!(seg_w[i] >= 0.0) || !std::isfinite(seg_w[i])) return img_fail(who + ": seg_weights[" + std::to_string(i) + "] is negative or not finite");
  }
  *total = tot;
  return 0;
}

// packed inputs of one call (pinned -> device in one copy) and its pinned outputs
struct WbLayout {
  size_t chains = 0, items = 0, kf_slot = 0, seg_start = 0, seg_rows = 0, seg_w = 0, poses = 0, in_bytes = 0;
  size_t T = 0, vec = 0, sd = 0, depths = 0, out_bytes = 0;
  WbLayout(int nslot, int n_points, int n_kf, int total, bool want_vec, bool want_depths, int n_pose = 0 /* explicit poses (mcp_scene_depth_robust) */) {
    size_t o = 0;
    chains = o; o = wb_align(o + sizeof(WbChain)*(size_t)nslot);
    items = o; o = wb_align(o + sizeof(WbItem)*(size_t)n_points);
    kf_slot = o; o = wb_align(o + sizeof(int)*(size_t)n_kf);
    seg_start = o; o = wb_align(o + sizeof(int)*((size_t)n_kf + 1));
    seg_rows = o; o = wb_align(o + sizeof(int)*(size_t)total);
    seg_w = o; o = wb_align(o + sizeof(double)*(size_t)total);
    poses = o; o = wb_align(o + 96*(size_t)n_pose);
    in_bytes = o;
    o = 0;
    T = o; o = wb_align(o + 96*(size_t)nslot);
    vec = o; o = wb_align(o + (want_vec ? 72*(size_t)n_points : 0));
    sd = o; o = wb_align(o + sizeof(mcp_scene_depth)*(size_t)n_kf);
    depths = o; o = wb_align(o + (want_depths ? 8*(size_t)total : 0));
    out_bytes = o;
  }
};

void sd_copy_out(int n_kf, const mcp_scene_depth* got, mcp_scene_depth* depth_out) {
  if (!depth_out) return;
  for (int j = 0; j < n_kf; ++j) {
    if (got[j].refreshed == 0) { depth_out[j].n = got[j].n; depth_out[j].refreshed = 0; }      // left alone: mean / sigma keep the caller's values
    else depth_out[j] = got[j];
  }
}

int rays_upload(mcp_map_points* m, const char* who, bool by_ids, int first, int count, const int* ids, const double* ce, const double* ri, const double* dn) {
  int top = 0;
  if (rows_check(m, who, by_ids, first, count, ids, ce && ri && dn, &top)) return -1;
  if (count == 0) return 0;
  if (column_upload(m, m->rays, first, count, ids, top, false,
    [&](int k, char* rec) {
      double* r = reinterpret_cast<double*>(rec);
      std::memcpy(r, ce + 3*(size_t)k, 24); std::memcpy(r + 3, ri + 3*(size_t)k, 24); std::memcpy(r + 6, dn + 3*(size_t)k, 24);
    },
    [&](const void* recs, const int* d_ids, dim3 grid) {
      hipLaunchKernelGGL(k_map_rays_scatter, grid, dim3(256), 0, m->st, m->rays.row(), count, d_ids, (const double*)recs);
    })) return -1;
  for (int k = 0; k < count; ++k) m->has_rays[ids ? ids[k] : first + k] = 1;
  return 0;
}

// the scene-depth launch on the table's stream, inputs already on the device
void sd_launch(mcp_map_points* m, int n_kf, const double* T, const int* slot, const char* dev_in, const WbLayout& L, char* out_pinned, bool want_depths) {
  hipLaunchKernelGGL(k_wb_scene_depth, dim3((unsigned)n_kf), dim3(SD_BLOCK), 0, m->st, T, slot, (const int*)(dev_in + L.seg_start), (const int*)(dev_in + L.seg_rows),
                     (const double*)(dev_in + L.seg_w), m->pts.row(), m->wb.depth.p, (mcp_scene_depth*)(out_pinned + L.sd),
                     want_depths ? (double*)(out_pinned + L.depths) : (double*)nullptr);
}

// what mcp_ba_write_back and mcp_graph_write_back share before anything is enqueued: the distinct pose chains of the call as slots of the
// product table (the solver's own chains by number, a chain it does not know by its pose indices) and the checked points
struct WbPlan {
  mcp_ba* h; mcp_map_points* m; const std::string& who; int chain_stride;
  std::vector<WbChain> chains; std::map<std::vector<int>, int> extra; std::vector<WbItem> items;
  WbPlan(mcp_ba* h_, mcp_map_points* m_, const std::string& who_, int stride) : h(h_), m(m_), who(who_), chain_stride(stride) { m->wb.slot.assign((size_t)ba_bridge_num_chains(h), -1); }
  int slot_of_solver(int c) {
    int& s = m->wb.slot[c];
    if (s < 0) { WbChain C; ba_bridge_chain(h, c, &C.len, C.v); s = (int)chains.size(); chains.push_back(C); }
    return s;
  }
  int slot_of_chain(const int* ids, int len, const char* what, int k) {       // -1: refused
    int v[MCP_MAX_CHAIN];
    const int c = ba_bridge_lookup_chain(h, ids, len, v);
    if (c == -2) { img_fail(who + ": " + what + " " + std::to_string(k) + " is not a chain of poses of this bundle (1.." + std::to_string(MCP_MAX_CHAIN) + " pose ids)"); return -1; }
    if (c >= 0) return slot_of_solver(c);
    std::vector<int> key(v, v + len);
    auto it = extra.find(key);
    if (it != extra.end()) return it->second;
    WbChain C; C.len = len; for (int i = 0; i < MCP_MAX_CHAIN; ++i) C.v[i] = i < len ? v[i] : 0;
    const int s = (int)chains.size(); chains.push_back(C); extra.emplace(key, s);
    return s;
  }
  int slot_of_ids(const int* ids, int len, const char* what, int k) {         // ... of a chain in an array of chain_stride ids per entry
    if (len > chain_stride) { img_fail(who + ": " + what + " " + std::to_string(k) + " is longer than chain_stride"); return -1; }
    return slot_of_chain(ids, len, what, k);
  }
  int points(int n_points, const int* point_ids, const int* rows, const int* src_chains, const int* src_chain_len) {
    items.resize((size_t)n_points);
    if (m->wb.stamp == 0x7fffffff) { m->wb.stamp = 0; std::fill(m->wb.mark.begin(), m->wb.mark.end(), 0); }
    const int stamp = ++m->wb.stamp;
    if ((int)m->wb.mark.size() < m->rows) m->wb.mark.resize((size_t)m->rows, 0);
    for (int k = 0; k < n_points; ++k) {
      int idx, fixed, c;
      if (ba_bridge_point(h, point_ids[k], &idx, &fixed, &c)) return img_fail(who + ": point_ids[" + std::to_string(k) + "] = " + std::to_string(point_ids[k]) + " is not a point of this bundle");
      const int r = rows[k];
      if (r < 0) return img_fail(who + ": rows[" + std::to_string(k) + "] is negative");
      if (r >= m->rows || !m->has_rays[r]) return img_fail(who + ": row " + std::to_string(r) + " has no patch rays (mcp_map_points_set_rays)");
      if (m->wb.mark[r] == stamp) return img_fail(who + ": row " + std::to_string(r) + " appears twice");
      m->wb.mark[r] = stamp;
      const int own = slot_of_solver(c);
      int src = own;
      if (src_chains && src_chain_len[k] != 0) {
        src = slot_of_ids(src_chains + (size_t)chain_stride*k, src_chain_len[k], "src_chains of point", k);
        if (src < 0) return -1;
      }
      items[k].pt = idx; items[k].row = r; items[k].own = own; items[k].src2_fixed = 2*src + (fixed ? 1 : 0);
    }
    return 0;
  }
};

// the chain table and the point kernel of a write-back on the table's stream (inputs on the device); vo: the pinned vectors, or null
void wb_launch_points(mcp_map_points* m, const BaDeviceState& S, int nslot, const WbChain* chains, double* T_host, int n_points, const WbItem* items, double* vo) {
  hipLaunchKernelGGL(k_wb_chains, dim3((unsigned)((nslot + 63)/64)), dim3(64), 0, m->st, nslot, chains, S.pose, m->wb.T.p, T_host);
  if (n_points)
    hipLaunchKernelGGL(k_wb_points, dim3((unsigned)((n_points + WB_BLOCK - 1)/WB_BLOCK)), dim3(WB_BLOCK), 0, m->st, n_points, items, S.point,
                       (const double*)m->wb.T.p, m->rays.row(), m->pts.row(), vo, vo ? vo + 3*(size_t)n_points : nullptr, vo ? vo + 6*(size_t)n_points : nullptr);
}
// the index of pose `id` in BaDeviceState::pose, -1 when `id` is not a pose.  (ba_bridge_lookup_chain fills its indices only for a chain the
// solver does not number; a pose that is a one-pose chain of the bundle is read from that chain.)
int wb_pose_index(const mcp_ba* h, int id) {
  int v[MCP_MAX_CHAIN] = {0};
  const int c = ba_bridge_lookup_chain(h, &id, 1, v);
  if (c == -2) return -1;
  if (c >= 0) { int len = 0; ba_bridge_chain(h, c, &len, v); }
  return v[0];
}
void wb_copy_vec(const double* vo, int n_points, double* world_out, double* right_out, double* down_out) {
  if (world_out) std::memcpy(world_out, vo, 24*(size_t)n_points);
  if (right_out) std::memcpy(right_out, vo + 3*(size_t)n_points, 24*(size_t)n_points);
  if (down_out) std::memcpy(down_out, vo + 6*(size_t)n_points, 24*(size_t)n_points);
}
}  // namespace

extern "C" {

int mcp_map_points_set_rays(mcp_map_points* m, int first, int count, const double* ce, const double* ri, const double* dn) {
  return rays_upload(m, "mcp_map_points_set_rays", false, first, count, nullptr, ce, ri, dn);
}
int mcp_map_points_update_rays(mcp_map_points* m, int count, const int* ids, const double* ce, const double* ri, const double* dn) {
  return rays_upload(m, "mcp_map_points_update_rays", true, 0, count, ids, ce, ri, dn);
}

int mcp_map_points_get(const mcp_map_points* m, int first, int count, double* wp, double* pr, double* pd, uint8_t* us) {
  std::vector<char> bounce;
  if (column_get(m, "mcp_map_points_get", m ? &m->pts : nullptr, first, count, nullptr, &bounce)) return -1;
  const PvsPoint* h = reinterpret_cast<const PvsPoint*>(bounce.data());
  for (int k = 0; k < count; ++k) {
    if (wp) std::memcpy(wp + 3*(size_t)k, h[k].world_pos, 24);
    if (pr) std::memcpy(pr + 3*(size_t)k, h[k].pixel_right_w, 24);
    if (pd) std::memcpy(pd + 3*(size_t)k, h[k].pixel_down_w, 24);
    if (us) us[k] = h[k].usable ? 1 : 0;
  }
  return 0;
}

int mcp_map_points_last_timing(const mcp_map_points* m, double* copy_ms, double* points_ms, double* depth_ms) {
  if (!m) return img_fail("mcp_map_points_last_timing: NULL table");
  if (!m->wb.timed) return img_fail("mcp_map_points_last_timing: no completed mcp_ba_write_back / mcp_scene_depth_robust on this table");
  float a = 0, b = 0, c = 0;
  ICK(hipEventElapsedTime(&a, m->wb.t[0], m->wb.t[1])); ICK(hipEventElapsedTime(&b, m->wb.t[1], m->wb.t[2])); ICK(hipEventElapsedTime(&c, m->wb.t[2], m->wb.t[3]));
  if (copy_ms) *copy_ms = a;
  if (points_ms) *points_ms = b;
  if (depth_ms) *depth_ms = c;
  return 0;
}

int mcp_scene_depth_robust(mcp_map_points* m, int n_kf, const double* cfw, const int* seg_start, const int* seg_rows, const double* seg_w,
                           mcp_scene_depth* depth_out, double* seg_depths_out) {
  const std::string who = "mcp_scene_depth_robust";
  if (!m) return img_fail(who + ": NULL table");
  int total = 0;
  if (sd_check(who, m, n_kf, seg_start, seg_rows, seg_w, &total)) return -1;
  if (n_kf == 0) return 0;
  if (!cfw) return img_fail(who + ": cam_from_world is NULL");
  ICK(hipSetDevice(m->device));
  const bool want_depths = seg_depths_out != nullptr;
  const WbLayout L(0, 0, n_kf, total, false, want_depths, n_kf);
  if (m->wb.in.alloc(L.in_bytes) || m->wb.dev.alloc(L.in_bytes) || m->wb.out.alloc(L.out_bytes) || m->wb.depth.alloc((size_t)total)) return -1;
  char* hin = m->wb.in.p;
  std::memcpy(hin + L.poses, cfw, 96*(size_t)n_kf);
  std::memcpy(hin + L.seg_start, seg_start, sizeof(int)*((size_t)n_kf + 1));
  if (total) { std::memcpy(hin + L.seg_rows, seg_rows, sizeof(int)*(size_t)total); std::memcpy(hin + L.seg_w, seg_w, 8*(size_t)total); }
  m->wb.invalidate();
  ICK(hipEventRecord(m->wb.t[0], m->st));
  ICK(hipMemcpyAsync(m->wb.dev.p, hin, L.in_bytes, hipMemcpyHostToDevice, m->st));
  ICK(hipEventRecord(m->wb.t[1], m->st)); ICK(hipEventRecord(m->wb.t[2], m->st));
  sd_launch(m, n_kf, (const double*)(m->wb.dev.p + L.poses), nullptr, m->wb.dev.p, L, m->wb.out.p, want_depths);
  const hipError_t le = hipGetLastError();
  (void)hipEventRecord(m->wb.t[3], m->st);
  ICK(m->sync());
  if (le != hipSuccess) return img_fail(who + ": launch failed: " + hipGetErrorString(le));
  m->wb.timed = true;
  sd_copy_out(n_kf, (const mcp_scene_depth*)(m->wb.out.p + L.sd), depth_out);
  if (seg_depths_out && total) std::memcpy(seg_depths_out, m->wb.out.p + L.depths, 8*(size_t)total);
  return 0;
}

int mcp_ba_write_back(mcp_ba* h, mcp_map_points* m, int n_points, const int* point_ids, const int* rows, const int* src_chains, int chain_stride,
                      const int* src_chain_len, double* world_out, double* right_out, double* down_out,
                      int n_kf, const int* kf_chains, const int* kf_chain_len, const int* seg_start, const int* seg_rows, const double* seg_w,
                      double* kf_cfw_out, mcp_scene_depth* depth_out, double* seg_depths_out) {
  const std::string who = "mcp_ba_write_back";
  if (!h) return img_fail(who + ": NULL solver handle");
  if (!m) return img_fail(who + ": NULL table");
  BaDeviceState S;
  if (ba_bridge_state(h, who.c_str(), &S)) return -1;
  if (S.device != m->device) return img_fail(who + ": the table lives on device " + std::to_string(m->device) + ", the solver on device " + std::to_string(S.device));
  if (n_points < 0) return img_fail(who + ": negative point count");
  if (n_points > 0 && (!point_ids || !rows)) return img_fail(who + ": point_ids / rows is NULL");
  if (n_points > 0 && src_chains && !src_chain_len) return img_fail(who + ": src_chain_len is NULL");
  int total = 0;
  if (sd_check(who, m, n_kf, seg_start, seg_rows, seg_w, &total)) return -1;
  if (n_kf > 0 && (!kf_chains || !kf_chain_len)) return img_fail(who + ": kf_chains / kf_chain_len is NULL");
  if (((n_points > 0 && src_chains) || n_kf > 0) && chain_stride < 1) return img_fail(who + ": chain_stride must be positive");
  WbPlan plan(h, m, who, chain_stride);
  if (plan.points(n_points, point_ids, rows, src_chains, src_chain_len)) return -1;
  std::vector<int> kf_slot((size_t)n_kf);
  for (int j = 0; j < n_kf; ++j) {
    kf_slot[j] = plan.slot_of_ids(kf_chains + (size_t)chain_stride*j, kf_chain_len[j], "kf_chains of keyframe", j);
    if (kf_slot[j] < 0) return -1;
  }
  const std::vector<WbChain>& chains = plan.chains; const std::vector<WbItem>& items = plan.items;
  if (n_points == 0 && n_kf == 0) return 0;
  // ---- every check has passed: from here on things are enqueued ----
  ICK(hipSetDevice(m->device));
  const int nslot = (int)chains.size();
  const bool want_vec = n_points > 0 && (world_out || right_out || down_out), want_depths = seg_depths_out != nullptr;
  const WbLayout L(nslot, n_points, n_kf, total, want_vec, want_depths);
  if (m->wb.in.alloc(L.in_bytes) || m->wb.dev.alloc(L.in_bytes) || m->wb.out.alloc(L.out_bytes) || m->wb.T.alloc(12*(size_t)nslot) || m->wb.depth.alloc((size_t)total)) return -1;
  char* hin = m->wb.in.p;
  std::memcpy(hin + L.chains, chains.data(), sizeof(WbChain)*(size_t)nslot);
  if (n_points) std::memcpy(hin + L.items, items.data(), sizeof(WbItem)*(size_t)n_points);
  if (n_kf) {
    std::memcpy(hin + L.kf_slot, kf_slot.data(), sizeof(int)*(size_t)n_kf);
    std::memcpy(hin + L.seg_start, seg_start, sizeof(int)*((size_t)n_kf + 1));
    if (total) { std::memcpy(hin + L.seg_rows, seg_rows, sizeof(int)*(size_t)total); std::memcpy(hin + L.seg_w, seg_w, 8*(size_t)total); }
  }
  // the table's stream waits for whatever the solver's stream still has to write of the state
  ICK(hipEventRecord(m->wb.ev, S.stream));
  ICK(hipStreamWaitEvent(m->st, m->wb.ev, 0));
  m->wb.invalidate();
  ICK(hipEventRecord(m->wb.t[0], m->st));
  ICK(hipMemcpyAsync(m->wb.dev.p, hin, L.in_bytes, hipMemcpyHostToDevice, m->st));
  ICK(hipEventRecord(m->wb.t[1], m->st));
  const char* din = m->wb.dev.p; char* hout = m->wb.out.p;
  wb_launch_points(m, S, nslot, (const WbChain*)(din + L.chains), kf_cfw_out ? (double*)(hout + L.T) : (double*)nullptr, n_points, (const WbItem*)(din + L.items),
                   want_vec ? (double*)(hout + L.vec) : (double*)nullptr);
  hipError_t le = hipGetLastError();
  (void)hipEventRecord(m->wb.t[2], m->st);
  if (n_kf) sd_launch(m, n_kf, (const double*)m->wb.T.p, (const int*)(din + L.kf_slot), din, L, hout, want_depths);
  if (le == hipSuccess) le = hipGetLastError();
  (void)hipEventRecord(m->wb.t[3], m->st);
  const hipError_t se = m->sync();                                   // the one wait: the solver's memory is not read after this
  if (le != hipSuccess) return img_fail(who + ": launch failed: " + hipGetErrorString(le));
  if (se != hipSuccess) return img_fail(who + ": " + hipGetErrorString(se));
  m->wb.timed = true;
  if (want_vec) wb_copy_vec((const double*)(hout + L.vec), n_points, world_out, right_out, down_out);
  if (n_kf) {
    if (kf_cfw_out) for (int j = 0; j < n_kf; ++j) std::memcpy(kf_cfw_out + 12*(size_t)j, hout + L.T + 96*(size_t)kf_slot[j], 96);
    sd_copy_out(n_kf, (const mcp_scene_depth*)(hout + L.sd), depth_out);
    if (seg_depths_out && total) std::memcpy(seg_depths_out, hout + L.depths, 8*(size_t)total);
  }
  return 0;
}

}  // extern "C"

// ---- ReFind_Common over the table (include/mcp_img.h mcp_map_refind, refind_kernels.h) ----------------------------------------------
extern "C" {

int mcp_map_refind(mcp_map_points* m, int n_targets, const mcp_refind_target* targets, int n_pairs, const int* pairs, int per_row_finders,
                   mcp_pf_state* finder, uint8_t* verdict, int cap_meas, mcp_refind_meas* meas, mcp_refind_result* res) {
  static_assert(sizeof(mcp_pf_state) % 8 == 0 && sizeof(RfTarget) % 8 == 0 && sizeof(TmSlot) % 8 == 0, "the packed inputs keep 8-byte alignment");
  if (!m) return img_fail("mcp_map_refind: NULL table");
  m->rf.invalidate();
  if (n_targets < 0 || n_pairs < 0 || cap_meas < 0 || !res || (n_pairs > 0 && (!pairs || !verdict || !targets || n_targets == 0)) || (n_targets > 0 && !targets))
    return img_fail("mcp_map_refind: bad arguments");
  for (int t = 0; t < n_targets; ++t) {
    const mcp_refind_target& G = targets[t];
    if (!G.kf || !kf_live(G.kf)) return img_fail("mcp_map_refind: target " + std::to_string(t) + " has no live keyframe");
    if (!cam_ok(G.cam)) return img_fail("mcp_map_refind: target " + std::to_string(t) + " has a bad camera");
    if (G.kf->device != m->device)
      return img_fail("mcp_map_refind: target " + std::to_string(t) + " is on device " + std::to_string(G.kf->device) + ", the table on device " + std::to_string(m->device));
  }
  const int rows = m->rows;
  for (int i = 0; i < n_pairs; ++i) {
    if (pairs[2*(size_t)i] < 0 || pairs[2*(size_t)i] >= rows) return img_fail("mcp_map_refind: pair " + std::to_string(i) + " names row " + std::to_string(pairs[2*(size_t)i]) + ", the table has " + std::to_string(rows));
    if (pairs[2*(size_t)i + 1] < 0 || pairs[2*(size_t)i + 1] >= n_targets) return img_fail("mcp_map_refind: pair " + std::to_string(i) + " names target " + std::to_string(pairs[2*(size_t)i + 1]) + " of " + std::to_string(n_targets));
  }
  std::memset(res, 0, sizeof *res);
  if (n_pairs == 0) { m->rf.view = 0; return 0; }
  ICK(hipSetDevice(m->device));
  const int n = n_pairs, nblk = (n + RF_BLOCK - 1)/RF_BLOCK;
  const size_t nslot = std::max<size_t>(m->slots.size(), 1);
  const int room = std::min(cap_meas, n);
  // packed inputs: control block | FOUND and TEMPLATE_BAD counts per RF_BLOCK pairs (all zero) | targets | source slots | pairs | the finder
  const size_t o_ctl = 0, o_fb = tm_align(sizeof(RfCtl)), o_tg = o_fb + tm_align(sizeof(int)*2*(size_t)nblk), o_sl = o_tg + tm_align(sizeof(RfTarget)*(size_t)n_targets);
  const size_t o_pr = o_sl + tm_align(sizeof(TmSlot)*nslot), o_st = o_pr + tm_align(8*(size_t)n), blk = o_st + tm_align(sizeof(mcp_pf_state));
  // pinned results: RfOut | verdict bytes | measurements
  const size_t r_vd = tm_align(sizeof(RfOut)), r_ms = r_vd + tm_align((size_t)n), rblk = r_ms + sizeof(mcp_refind_meas)*(size_t)std::max(room, 1);
  // everything is allocated before the first enqueue
  if (m->parcel_reads && m->rf.out.n < rblk) ICK(m->sync());            // (a parcel's fill may still read the block replaced below)
  if (m->rf.in.alloc(blk) || m->rf.dev.alloc(blk) || m->rf.out.alloc(rblk) || m->rf.flags.alloc(n) || m->rf.vd.alloc(n) || m->rf.blk.alloc(2*(size_t)nblk) ||
      m->rf.items.alloc(n) || m->rf.first.alloc(n) || m->rf.cand.alloc(n)) return -1;
  char* hb = m->rf.in.p;
  std::memset(hb, 0, o_pr);
  RfTarget* tab = reinterpret_cast<RfTarget*>(hb + o_tg);
  for (int t = 0; t < n_targets; ++t) {
    const mcp_refind_target& G = targets[t];
    tab[t].T = G.kf->view(); tab[t].cam = *G.cam;
    tab[t].cfw = se3_of12(G.cam_from_world);
  }
  fill_slots(m, reinterpret_cast<TmSlot*>(hb + o_sl));
  std::memcpy(hb + o_pr, pairs, 8*(size_t)n);
  if (finder) std::memcpy(hb + o_st, finder, sizeof(mcp_pf_state)); else std::memset(hb + o_st, 0, sizeof(mcp_pf_state));
  hipStream_t st = m->st;
  char* db = m->rf.dev.p;
  RfCtl* ctl = reinterpret_cast<RfCtl*>(db + o_ctl);
  int* found_blk = reinterpret_cast<int*>(db + o_fb); int* bad_blk = found_blk + nblk;
  const RfTarget* d_tg = reinterpret_cast<const RfTarget*>(db + o_tg);
  const TmSlot* d_sl = reinterpret_cast<const TmSlot*>(db + o_sl);
  const int* d_pr = reinterpret_cast<const int*>(db + o_pr);
  const mcp_pf_state* d_st = finder ? reinterpret_cast<const mcp_pf_state*>(db + o_st) : nullptr;
  RfOut* h_out = reinterpret_cast<RfOut*>(m->rf.out.p);
  uint8_t* h_vd = reinterpret_cast<uint8_t*>(m->rf.out.p + r_vd);
  mcp_refind_meas* h_ms = reinterpret_cast<mcp_refind_meas*>(m->rf.out.p + r_ms);
  Drain drain{m, true};
  ICK(hipMemcpyAsync(db, hb, blk, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_rf_mark, dim3(nblk), dim3(RF_BLOCK), 0, st, n, per_row_finders ? 1 : 0, d_pr, d_tg, m->pts.row(), m->src.row(), d_sl,
                     m->rf.flags.p, m->rf.vd.p, m->rf.blk.p, m->rf.first.p, ctl);
  hipLaunchKernelGGL(k_rf_scatter, dim3(nblk), dim3(RF_BLOCK), 0, st, n, nblk, (const uint8_t*)m->rf.flags.p, (const int*)m->rf.blk.p, d_pr, m->src.row(), m->rf.items.p, m->rf.first.p, ctl);
  hipLaunchKernelGGL(k_rf_walk, dim3((unsigned)std::min(n, 65536)), dim3(64), 0, st, d_tg, m->pts.row(), d_sl, (const RfItem*)m->rf.items.p, (const int*)m->rf.first.p, d_st,
                     m->rf.vd.p, m->rf.cand.p, found_blk, bad_blk, ctl, &h_out->state);
  hipLaunchKernelGGL(k_rf_commit, dim3(nblk), dim3(RF_BLOCK), 0, st, n, nblk, room, (const uint8_t*)m->rf.vd.p, (const mcp_refind_meas*)m->rf.cand.p, (const int*)found_blk,
                     (const int*)bad_blk, (const RfItem*)m->rf.items.p, (const RfCtl*)ctl, d_st, h_vd, h_ms, h_out);
  ICK(hipGetLastError());
  ICK(m->sync());
  drain.armed = false;
  for (int q = 0; q < 6; ++q) res->counts[q] = h_out->counts[q];
  res->n_meas = h_out->n_meas;
  std::memcpy(verdict, h_vd, (size_t)n);
  if (finder) *finder = h_out->state;
  if (res->n_meas > cap_meas)
    return img_fail("mcp_map_refind: " + std::to_string(res->n_meas) + " pairs were found, cap_meas is " + std::to_string(cap_meas));
  m->rf.meas_off = r_ms; m->rf.view = res->n_meas;
  if (meas && res->n_meas) std::memcpy(meas, h_ms, sizeof(mcp_refind_meas)*(size_t)res->n_meas);
  return 0;
}

const mcp_refind_meas* mcp_map_refind_view(const mcp_map_points* m, int* count) {
  if (count) *count = 0;
  if (!m || m->rf.view < 0) { img_fail("mcp_map_refind_view: the last mcp_map_refind on this table left no measurements to show"); return nullptr; }
  if (count) *count = m->rf.view;
  return m->rf.view > 0 ? reinterpret_cast<const mcp_refind_meas*>(m->rf.out.p + m->rf.meas_off) : nullptr;
}

}  // extern "C"

// ---- the map graph (include/mcp_img.h mcp_map_graph_*, mcp_map_bundle_select; map_graph_kernels.h) ---------------------------------------
// "A block that grows is replaced with nothing in flight on the old one."  Buf::alloc and PinBuf::alloc free the old block at once, so a call
// constructs one of these before its first enqueue and passes every block it needs through it.  The first block that has to grow waits for
// the table's stream (the owner's sync(): once per call, and only then); after that it and the later ones are allocated.  Whatever the call
// enqueues between two growths it reports with enqueued(), and the next growth waits again.
template <class Owner> struct Grow {
  Owner* o; bool idle = false;
  explicit Grow(Owner* owner) : o(owner) {}
  int wait() { if (!idle) { if (o->sync()) return -1; idle = true; } return 0; }
  void enqueued() { idle = false; }
  template <class B> int grow(B& b, size_t count) { return std::max<size_t>(count, 1) <= b.n ? 0 : (wait() || b.alloc(count)) ? -1 : 0; }
  // room for `need` elements by the doubling rule of the point columns, the store and a parcel's entries; the first `keep` are copied over
  template <class T> int regrow(Buf<T>& b, size_t need, size_t keep) {
    if (need <= b.n && b.p) return 0;
    const size_t bigger = std::max<size_t>({need, 2*b.n, (size_t)1024});
    if (!keep) return (b.p && wait()) ? -1 : b.alloc(bigger);
    Buf<T> fresh;
    if (fresh.alloc(bigger)) return -1;
    ICK(hipMemcpyAsync(fresh.p, b.p, sizeof(T)*keep, hipMemcpyDeviceToDevice, o->m->st));
    enqueued();
    if (wait()) return -1;                             // the old block is freed below, with nothing in flight on it
    b.swap(fresh);
    return 0;
  }
};

// a pair of events around a call's submission, created on first use; timed: the last such call ran to its wait
struct MgTimer {
  hipEvent_t ev[2] = {nullptr, nullptr}; bool timed = false;
  ~MgTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  int begin(hipStream_t st) { timed = false; for (hipEvent_t& e : ev) if (!e) ICK(hipEventCreate(&e)); ICK(hipEventRecord(ev[0], st)); return 0; }
  int end(hipStream_t st) { ICK(hipEventRecord(ev[1], st)); return 0; }
  int ms(double* out) const {                          // -1.0 when the last call did not run
    *out = -1.0;
    if (!timed) return 0;
    float f = 0.f;
    ICK(hipEventElapsedTime(&f, ev[0], ev[1]));
    *out = f;
    return 0;
  }
};

// every launch of the map graph but the list passes' (MGL_BLOCK: a tile of the list algorithm) runs workgroups of MG_BLOCK threads
static_assert(MGP_BLOCK == MG_BLOCK && MGC_BLOCK == MG_BLOCK && MGN_BLOCK == MG_BLOCK && MGCL_BLOCK == MG_BLOCK, "the map-graph kernels share one workgroup size");
static int mg_grid(long long n, int block = MG_BLOCK) { return (int)((n + block - 1)/block); }      // (empty for n == 0: the launch is skipped or n is positive)
static int mg_grid1(long long n) { return std::max(1, mg_grid(n)); }

struct mcp_map_graph {
  mcp_map_points* m = nullptr;                        // the table: its device, its stream, its rows (it must outlive the graph)
  MgRig rig;
  Buf<MgMkf> slots;                                   // MCP_MAP_MAX_MKFS slots
  // the host's copy of their flags and active bytes (what add_meas, select and a query's refusals check)
  struct Mirror {
    std::vector<int> flags = std::vector<int>(MCP_MAP_MAX_MKFS, 0);
    std::vector<uint8_t> act = std::vector<uint8_t>((size_t)MCP_MAP_MAX_MKFS*MCP_MAX_FRAME_CAMS, 0);
    bool present(int k) const { return k >= 0 && k < MCP_MAP_MAX_MKFS && (flags[k] & MCP_MKF_PRESENT); }
    int n_present() const { int n = 0; for (int f : flags) n += (f & MCP_MKF_PRESENT) ? 1 : 0; return n; }
    int top_present() const { int k = MCP_MAP_MAX_MKFS - 1; while (k >= 0 && !(flags[k] & MCP_MKF_PRESENT)) --k; return k; }      // -1: none
    int flags_of(int k) const { return flags[k]; }
    const uint8_t* active(int k) const { return &act[(size_t)k*MCP_MAX_FRAME_CAMS]; }
    void set(int k, int f, const uint8_t* a = nullptr) { flags[k] = f; if (a) std::memcpy(&act[(size_t)k*MCP_MAX_FRAME_CAMS], a, MCP_MAX_FRAME_CAMS); }      // (a null: the active bytes stay)
  } mirror;
  Buf<MgPoint> pts; int prow = 0;                     // point columns: prow rows written or filled so far
  Buf<MgMeas> store, store_alt; int n_store = 0, n_live = 0;
  Buf<MgCtl> ctl; PinBuf<MgCtl> h_ctl;
  // uploads: packed into pinned memory, copied on the table's stream; `done` marks when the staging may be refilled
  struct Stage { PinBuf<char> in; Buf<char> dev; hipEvent_t done = nullptr; bool busy = false; } up;
  std::vector<int> sorted_ids; std::vector<unsigned long long> keys;
  // scratch every call family sizes for itself: marks (a select's mkf_in | good | seen; good counts; a removal's live | by_src) and the
  // per-workgroup counts
  Buf<int> marks, blk;
  // the select: verdicts, bundle indices; the pinned views and result, what the views hold; mcp_map_bundle_select_last_timing: around the
  // last select's submission
  struct Sel {
    Buf<int> bidx, mkf_bidx; Buf<uint8_t> adjust, rows, mkeep;
    PinBuf<mcp_bundle_mkf> v_mkfs; PinBuf<mcp_bundle_point> v_points; PinBuf<mcp_bundle_meas> v_meas; PinBuf<mcp_bundle_select_result> h_res;
    int n_mkfs = 0, n_points = 0, n_meas = 0;
    MgTimer t;
  } sel;
  // the keyframe lists (map_graph_lists.h): the call's slots (pinned | device), the (key, row) column, the count table, the lists, the
  // keyframes' poses and the pinned results of mcp_graph_refresh_depth / mcp_graph_debug_kf_lists
  struct Lists { PinBuf<char> in; Buf<char> dev; Buf<int2> key_row; Buf<int> table, start, rows; Buf<double> w, cfw; PinBuf<char> out; } lists;
  // the commit of a measurement parcel (map_graph_parcel.h): verdict bytes, per-workgroup counts, the result block (MgpCtl | per-lane counts: device, pinned)
  struct Commit { Buf<uint8_t> vd; Buf<int> blk; Buf<char> dev; PinBuf<char> out; } commit;
  // outliers and bad points (map_graph_cull.h): the store index of each key, verdict and report bytes, the counters (device, pinned with the
  // verdicts behind them), the pinned report of the last sweep; the timers of mcp_map_cull_last_timing.
  // The good counts go through `marks`, the per-workgroup counts through `blk`, as a select's do.
  struct Cull {
    Buf<int> match; Buf<uint8_t> vd, rep; Buf<MgcCtl> ctl; PinBuf<char> out; PinBuf<int> rows; int nrows = 0;
    MgTimer t_outliers, t_sweep;
    std::vector<std::pair<unsigned long long, int>> keys; std::vector<MgcRun> runs;
  } cull;
  // the neighbour queries and the removal of an MKF (map_graph_neigh.h): the scratch of distances and candidate bytes, the two queries'
  // hand-offs and results (device), the external MKF, the removal's block, the pinned results; the timers of
  // mcp_map_neighbours_last_timing / mcp_map_mkf_cull_last_timing.  The live counts of a removal go through `marks`.
  struct Neigh {
    Buf<double> dist; Buf<uint8_t> cand; Buf<MgnCtl> ctl; Buf<mcp_neigh_result> res; Buf<MgMkf> ext; Buf<MgnCull> cc; PinBuf<char> out;
    MgTimer t_query, t_remove;
  } neigh;
  // the co-visible points of the nearest keyframe (map_graph_collect.h): the marks (kf_mark | seed | near), the report (device, pinned), the
  // pose where a call brings its own (pinned, device), the pinned copy of near for the stand-alone call's view (view: its rows; -1: none);
  // the timer of mcp_map_collect_last_timing
  struct Collect {
    Buf<uint8_t> marks; Buf<mcp_collect_report> rep; PinBuf<mcp_collect_report> h_rep; PinBuf<double> h_pose; Buf<double> pose; PinBuf<uint8_t> h_near;
    int view = -1; MgTimer t;
    uint8_t* kf_mark() const { return marks.p; }
    uint8_t* seed() const { return marks.p + MGCL_KF_MARKS; }
    uint8_t* near(int rows) const { return marks.p + MGCL_KF_MARKS + mgcl_row_bytes(rows); }
    static size_t bytes(int rows) { return (size_t)MGCL_KF_MARKS + 2*mgcl_row_bytes(rows); }
  } collect;
  // mcp_stereo_map_points (stereo_append.h): the source keyframe's busy list gathered from the store, its length (device, pinned).  The rows, keys
  // and target slots go up through `up`, the per-workgroup counts through `blk`.
  struct Stereo { Buf<mcp_stereo_meas> busy; Buf<int> n_busy; PinBuf<int> h_n_busy; } stereo;
  // mcp_init_depth_map_points / mcp_map_mark_optimized / _rescale / _transform (map_life.h): the candidates' survivor bytes and their per-workgroup
  // counts, the hand-off block of the cameras' launches (device, pinned), the pinned keep bytes and records; the counters (device, pinned).
  // The rows, keys and candidates -- or the rows' ray bits -- go up through `up`, the busy list through `stereo` and `blk`.
  struct Life { Buf<uint8_t> alive; Buf<int> blk; Buf<MlInitCtl> ctl; PinBuf<MlInitCtl> h_ctl; PinBuf<uint8_t> h_keep; PinBuf<mcp_stereo_point> h_out; Buf<int> cnt; PinBuf<int> h_cnt; MgTimer t_init, t_move; } life;
  using Guard = Grow<mcp_map_graph>;
  ~mcp_map_graph() {                                  // (the timers destroy their events after this wait)
    if (m && m->st) (void)hipStreamSynchronize(m->st);
    if (up.done) (void)hipEventDestroy(up.done);
  }
  int wait_staging() { if (up.busy) { ICK(hipEventSynchronize(up.done)); up.busy = false; } return 0; }
  int sync() { ICK(hipStreamSynchronize(m->st)); up.busy = false; m->stage_busy = false; m->parcel_reads = false; return 0; }
  // the one wait of a call: past it nothing is in flight, so its Drain has nothing left to do and its timer (if it has one) may be read
  int one_wait(Drain& drain, MgTimer* t = nullptr) { if (sync()) return -1; drain.armed = false; if (t) t->timed = true; return 0; }
  // pinned + device staging of `bytes`, free to fill
  int stage(Guard& G, size_t bytes) { return (wait_staging() || G.grow(up.in, bytes) || G.grow(up.dev, bytes)) ? -1 : 0; }
  int staged_now() { ICK(hipEventRecord(up.done, m->st)); up.busy = true; return 0; }
  // the point columns cover `rows` rows: the ones that appear read as never written
  int grow_points(Guard& G, int rows) {
    if (rows <= prow) return 0;
    if (G.regrow(pts, (size_t)rows, (size_t)prow)) return -1;
    hipLaunchKernelGGL(k_mg_points_fill, dim3(mg_grid(rows - prow)), dim3(MG_BLOCK), 0, m->st, pts.p, prow, rows - prow);
    ICK(hipGetLastError());
    G.enqueued();
    prow = rows;
    return 0;
  }
  int grow_store(Guard& G, size_t need) { return G.regrow(store, need, (size_t)n_store); }
  // the fixed-size scratch of the queries and the removal
  int neigh_reserve(Guard& G) {
    const size_t n_idx = (size_t)(MCP_MAP_MAX_MKFS + 1)*MCP_MAX_FRAME_CAMS;
    return (G.grow(neigh.dist, n_idx) || G.grow(neigh.cand, n_idx) || G.grow(neigh.ctl, 2) || G.grow(neigh.res, 2) || G.grow(neigh.ext, 1) || G.grow(neigh.cc, 1) ||
            G.grow(neigh.out, 2*sizeof(mcp_neigh_result) + sizeof(MgnCull))) ? -1 : 0;
  }
  int collect_reserve(Guard& G) {
    return (G.grow(collect.marks, Collect::bytes(m->rows)) || G.grow(collect.rep, 1) || G.grow(collect.h_rep, 1) || G.grow(collect.h_pose, 12) || G.grow(collect.pose, 12)) ? -1 : 0;
  }
  // the good count of every row into marks[0 .. R) (zeroed by the caller): k_mg_edges_count without a select's hand-off
  void good_counts_enqueue(int R) {
    hipLaunchKernelGGL(k_mg_edges_count, dim3(mg_grid(n_store)), dim3(MG_BLOCK), 0, m->st, (const MgCtl*)nullptr, (const MgMeas*)store.p, n_store, R, (const MgMkf*)slots.p,
                       (const uint8_t*)nullptr, marks.p, (int*)nullptr);
  }
  // `count` elements of a device block in a host vector, waited for
  template <class T> int read_back(std::vector<T>& out, const T* from, size_t count) {
    out.resize(count);
    ICK(hipMemcpyAsync(out.data(), from, sizeof(T)*count, hipMemcpyDeviceToHost, m->st));
    return sync();
  }
};

// what a measurement from host arrays must have, whichever call takes it (at: "<call>: entry <k>"): a row of the table, a pyramid level, a finite position
static int mg_entry_check(const std::string& at, int row, int R, int level, const double* uv) {
  if (row < 0 || row >= R) return img_fail(at + " names row " + std::to_string(row) + ", the table has " + std::to_string(R));
  if (level < 0 || level >= MCP_LEVELS) return img_fail(at + " has level " + std::to_string(level));
  if (!std::isfinite(uv[0]) || !std::isfinite(uv[1])) return img_fail(at + " has a non-finite position");
  return 0;
}

static int mg_distinct(std::vector<int>& sorted,const int* ids, int count, const std::string& who, const char* what) {
  sorted.assign(ids, ids + count);
  std::sort(sorted.begin(), sorted.end());
  for (int k = 1; k < count; ++k) if (sorted[k] == sorted[k - 1]) return img_fail(who + ": " + what + " " + std::to_string(sorted[k]) + " appears twice");
  return 0;
}

static int mg_mkfs_upload(mcp_map_graph* g, const std::string& who, bool by_ids, int first, int count, const int* ids, const double* bfw, const int* flags,
                          const uint8_t* act, const double* dep) {
  if (!g) return img_fail(who + ": NULL graph");
  if (count < 0 || (count > 0 && (!bfw || !flags || !act || !dep || (by_ids && !ids)))) return img_fail(who + ": bad arguments");
  if (!by_ids && (first < 0 || (long long)first + count > MCP_MAP_MAX_MKFS)) return img_fail(who + ": more than MCP_MAP_MAX_MKFS (" + std::to_string(MCP_MAP_MAX_MKFS) + ") MKF slots");
  const int nc = g->rig.ncam;
  for (int k = 0; k < count; ++k) {
    if (by_ids && (ids[k] < 0 || ids[k] >= MCP_MAP_MAX_MKFS)) return img_fail(who + ": slot " + std::to_string(ids[k]) + " is outside 0.." + std::to_string(MCP_MAP_MAX_MKFS - 1));
    if (!finite12(bfw + 12*(size_t)k)) return img_fail(who + ": entry " + std::to_string(k) + " has a non-finite pose");
    if (flags[k] & ~(MCP_MKF_PRESENT | MCP_MKF_FIXED | MCP_MKF_BAD)) return img_fail(who + ": entry " + std::to_string(k) + " has unknown flags");
    for (int c = 0; c < nc; ++c) {
      const double d = dep[(size_t)k*nc + c];
      if (act[(size_t)k*nc + c] && !(std::isfinite(d) && d > 0.0)) return img_fail(who + ": entry " + std::to_string(k) + ", camera " + std::to_string(c) + ": the depth mean of an active keyframe must be finite and positive");
    }
  }
  if (by_ids && count && mg_distinct(g->sorted_ids, ids, count, who, "slot")) return -1;
  if (count == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  const size_t o_ids = tm_align(sizeof(MgMkf)*(size_t)count), need = o_ids + sizeof(int)*(size_t)count;
  mcp_map_graph::Guard G(g);
  if (g->stage(G, need)) return -1;
  MgMkf* rec = reinterpret_cast<MgMkf*>(g->up.in.p); int* hid = reinterpret_cast<int*>(g->up.in.p + o_ids);
  std::memset(g->up.in.p, 0, o_ids);
  for (int k = 0; k < count; ++k) {
    std::memcpy(rec[k].bfw, bfw + 12*(size_t)k, 96);
    rec[k].flags = flags[k];
    for (int c = 0; c < nc; ++c) { const bool a = act[(size_t)k*nc + c] != 0; rec[k].active[c] = a ? 1 : 0; rec[k].depth[c] = a ? dep[(size_t)k*nc + c] : 0.0; }
    hid[k] = by_ids ? ids[k] : first + k;
  }
  ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, need, hipMemcpyHostToDevice, g->m->st));
  hipLaunchKernelGGL(k_mg_mkfs_scatter, dim3(mg_grid(count)), dim3(MG_BLOCK), 0, g->m->st, g->slots.p, count, (const int*)(g->up.dev.p + o_ids), (const MgMkf*)g->up.dev.p);
  ICK(hipGetLastError());
  if (g->staged_now()) return -1;
  for (int k = 0; k < count; ++k) g->mirror.set(hid[k], flags[k], rec[k].active);
  return 0;
}

// the selection on host arrays: the host's statement of the six launches (the same __host__ __device__ bodies)
namespace {
struct MgHostIn {
  int ncam; const double* cfb; int n_slots; const double* bfw; const int* mflags; const uint8_t* act; const double* dep;
  int n_rows; const double* world; const int* src_mkf; const int* src_cam; const int* pflags;
  int n_store; const int* ms_mkf; const int* ms_cam; const int* ms_row; const double* ms_uv; const int* ms_level; const int* ms_source; const uint8_t* ms_alive;
};
}
static std::string mg_params_check(const mcp_bundle_select_params* p) {
  if (!p) return "NULL params";
  if (p->mode != MCP_BUNDLE_ALL && p->mode != MCP_BUNDLE_RECENT) return "unknown mode " + std::to_string(p->mode);
  if (p->n_recent < 0 || p->n_recent > 8) return "n_recent outside 0..8";
  if (p->recent_min_size < 0 || p->min_points < 0) return "a negative gate";
  if (!std::isfinite(p->mean_diff_fraction)) return "mean_diff_fraction is not finite";
  return "";
}
static void mg_host_select(const mcp_bundle_select_params& S, const MgHostIn& I, mcp_bundle_select_result& R, std::vector<mcp_bundle_mkf>& mk,
                           std::vector<mcp_bundle_point>& pt, std::vector<mcp_bundle_meas>& ms) {
  std::memset(&R, 0, sizeof R);
  for (int k = 0; k < 8; ++k) R.closest[k] = -1;
  MgRig rig; std::memset(&rig, 0, sizeof rig); rig.ncam = I.ncam;
  for (int c = 0; c < I.ncam; ++c) mg_se3_of12(I.cfb + 12*(size_t)c, rig.cfb[c]);
  const int P = I.n_slots, nc = I.ncam;
  auto flags_of = [&](int k) { return k >= 0 && k < P ? I.mflags[k] : 0; };
  std::vector<uint8_t> adjust(P, 0);
  if (S.mode == MCP_BUNDLE_ALL) { for (int k = 0; k < P; ++k) adjust[k] = mg_mkf_ok(I.mflags[k]); }
  else {
    int n_present = 0;
    for (int k = 0; k < P; ++k) n_present += (I.mflags[k] & MCP_MKF_PRESENT) ? 1 : 0;
    if (n_present < S.recent_min_size) { R.status = 1; return; }
    std::vector<std::pair<double, int>> d;
    bool broken = false;
    const int nw = S.newest;
    for (int k = 0; k < P; ++k) {
      if (k == nw || !(I.mflags[k] & MCP_MKF_PRESENT)) continue;
      bool br;
      d.emplace_back(mg_mkf_distance(rig, I.bfw + 12*(size_t)nw, I.act + (size_t)nw*nc, I.dep + (size_t)nw*nc, I.bfw + 12*(size_t)k, I.act + (size_t)k*nc,
                                     I.dep + (size_t)k*nc, S.mean_diff_fraction, &br), k);
      broken = broken || br;
    }
    if (broken) { R.status = 3; return; }
    std::sort(d.begin(), d.end());
    adjust[nw] = 1;
    for (int r = 0; r < S.n_recent && r < (int)d.size(); ++r) {
      R.closest[r] = d[r].second; R.closest_dist[r] = d[r].first;
      const int f = I.mflags[d[r].second];
      if (!(f & MCP_MKF_BAD) && !(f & MCP_MKF_FIXED)) adjust[d[r].second] = 1;
    }
  }
  const int N = I.n_rows, M = I.n_store;
  std::vector<int> good(N, 0), seen(N, 0), bidx(N, -1), mkf_in(P, 0);
  for (int i = 0; i < M; ++i) {
    if (!mg_edge_live(I.ms_alive[i], I.ms_mkf[i], I.ms_row[i], N) || I.ms_mkf[i] >= P) continue;
    if (mg_mkf_ok(I.mflags[I.ms_mkf[i]])) ++good[I.ms_row[i]];
    if (adjust[I.ms_mkf[i]]) seen[I.ms_row[i]] = 1;
  }
  int n_points = 0;
  for (int i = 0; i < N; ++i) {
    MgPoint Q; Q.src_mkf = I.src_mkf[i]; Q.src_cam = I.src_cam[i]; Q.flags = I.pflags[i]; Q.pending = 0;
    if (!mg_row_selected(S.mode, Q.flags, good[i], seen[i])) continue;
    const bool fixed = Q.flags & MCP_GP_FIXED;
    if (!fixed && !(mg_source_in_range(Q, nc, P) && mg_mkf_ok(I.mflags[Q.src_mkf]))) { ++R.n_dropped_source; continue; }
    if (fixed) R.has_fixed_points = 1; else mkf_in[Q.src_mkf] = 1;
    bidx[i] = n_points++;
  }
  if (n_points < S.min_points) { R.status = 2; R.has_fixed_points = 0; return; }
  std::vector<uint8_t> keep(M, 0);
  for (int i = 0; i < M; ++i) {
    if (!mg_edge_live(I.ms_alive[i], I.ms_mkf[i], I.ms_row[i], N) || I.ms_mkf[i] >= P) continue;
    if (bidx[I.ms_row[i]] < 0 || !mg_mkf_ok(I.mflags[I.ms_mkf[i]])) continue;
    keep[i] = 1; mkf_in[I.ms_mkf[i]] = 1;
  }
  std::vector<int> mkf_bidx(P, -1);
  for (int k = 0; k < P; ++k) if (adjust[k]) { mkf_bidx[k] = (int)mk.size(); mk.push_back({k, (I.mflags[k] & MCP_MKF_FIXED) ? 1 : 0}); }
  R.n_adjust = (int)mk.size();
  for (int k = 0; k < P; ++k) if (!adjust[k] && mkf_in[k] && mg_mkf_ok(flags_of(k))) { mkf_bidx[k] = (int)mk.size(); mk.push_back({k, 1}); }
  R.n_fixed = (int)mk.size() - R.n_adjust;
  for (int i = 0; i < N; ++i) {
    if (bidx[i] < 0) continue;
    MgPoint Q; Q.src_mkf = I.src_mkf[i]; Q.src_cam = I.src_cam[i]; Q.flags = I.pflags[i]; Q.pending = 0;
    const bool fixed = Q.flags & MCP_GP_FIXED;
    mcp_bundle_point O;
    mg_point_x(rig, Q, I.bfw + 12*(size_t)(fixed ? 0 : Q.src_mkf), I.world + 3*(size_t)i, O.x);
    O.row = i; O.src_mkf = fixed ? -1 : mkf_bidx[Q.src_mkf]; O.src_cam = fixed ? -1 : Q.src_cam; O.fixed = fixed ? 1 : 0;
    pt.push_back(O);
  }
  for (int i = 0; i < M; ++i) {
    if (!keep[i]) continue;
    mcp_bundle_meas O;
    O.uv[0] = I.ms_uv[2*(size_t)i]; O.uv[1] = I.ms_uv[2*(size_t)i + 1]; O.mkf = mkf_bidx[I.ms_mkf[i]]; O.cam = I.ms_cam[i]; O.point = bidx[I.ms_row[i]];
    O.level = I.ms_level[i]; O.source = I.ms_source[i]; O.store = i;
    ms.push_back(O);
  }
  R.n_points = n_points; R.n_meas = (int)ms.size();
}

extern "C" {

mcp_map_graph* mcp_map_graph_create(mcp_map_points* m, int ncam, const double* cfb) {
  if (!m) { mcp_set_error("mcp_map_graph_create: NULL table"); return nullptr; }
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !cfb) { mcp_set_error("mcp_map_graph_create: ncam must be 1..MCP_MAX_FRAME_CAMS with one CamFromBase each"); return nullptr; }
  for (int c = 0; c < ncam; ++c) if (!finite12(cfb + 12*(size_t)c)) { mcp_set_error("mcp_map_graph_create: a non-finite CamFromBase"); return nullptr; }
  if (hipSetDevice(m->device) != hipSuccess) { mcp_set_error("hipSetDevice failed"); return nullptr; }
  mcp_map_graph* g = new mcp_map_graph(); g->m = m;
  std::memset(&g->rig, 0, sizeof g->rig); g->rig.ncam = ncam;
  for (int c = 0; c < ncam; ++c) mg_se3_of12(cfb + 12*(size_t)c, g->rig.cfb[c]);
  const bool ok = !g->slots.alloc(MCP_MAP_MAX_MKFS) && !g->ctl.alloc(1) && !g->h_ctl.alloc(1) && !g->sel.h_res.alloc(1) && !g->sel.adjust.alloc(MCP_MAP_MAX_MKFS) &&
                  !g->sel.mkf_bidx.alloc(MCP_MAP_MAX_MKFS) && !g->sel.v_mkfs.alloc(MCP_MAP_MAX_MKFS) && hipEventCreateWithFlags(&g->up.done, hipEventDisableTiming) == hipSuccess &&
                  hipMemsetAsync(g->slots.p, 0, sizeof(MgMkf)*(size_t)MCP_MAP_MAX_MKFS, m->st) == hipSuccess && hipMemsetAsync(g->ctl.p, 0, sizeof(MgCtl), m->st) == hipSuccess;
  if (!ok) { mcp_set_error("mcp_map_graph_create: allocation failed"); delete g; return nullptr; }
  std::memset(g->sel.h_res.p, 0, sizeof(mcp_bundle_select_result));
  return g;
}
void mcp_map_graph_destroy(mcp_map_graph* g) {
  if (!g) return;
  if (g->m->co.g == g) g->m->co.g = nullptr;           // mcp_track_collect_nearest: no later frame follows a dead pointer
  (void)hipSetDevice(g->m->device); delete g;
}

int mcp_map_graph_set_mkfs(mcp_map_graph* g, int first, int count, const double* bfw, const int* flags, const uint8_t* act, const double* dep) {
  return mg_mkfs_upload(g, "mcp_map_graph_set_mkfs", false, first, count, nullptr, bfw, flags, act, dep);
}
int mcp_map_graph_update_mkfs(mcp_map_graph* g, int count, const int* slots, const double* bfw, const int* flags, const uint8_t* act, const double* dep) {
  return mg_mkfs_upload(g, "mcp_map_graph_update_mkfs", true, 0, count, slots, bfw, flags, act, dep);
}

int mcp_map_graph_update_points(mcp_map_graph* g, int count, const int* rows, const int* src_mkf, const int* src_cam, const int* flags) {
  const std::string who = "mcp_map_graph_update_points";
  if (!g) return img_fail(who + ": NULL graph");
  if (count < 0 || (count > 0 && (!rows || !src_mkf || !src_cam || !flags))) return img_fail(who + ": bad arguments");
  const int R = g->m->rows;
  for (int k = 0; k < count; ++k) {
    if (rows[k] < 0 || rows[k] >= R) return img_fail(who + ": row " + std::to_string(rows[k]) + " is outside the table (" + std::to_string(R) + " rows)");
    if (flags[k] & ~(MCP_GP_FIXED | MCP_GP_BAD)) return img_fail(who + ": entry " + std::to_string(k) + " has unknown flags");
    if (src_mkf[k] >= MCP_MAP_MAX_MKFS) return img_fail(who + ": entry " + std::to_string(k) + " names source slot " + std::to_string(src_mkf[k]));
    if (src_mkf[k] < 0 && !(flags[k] & MCP_GP_FIXED)) return img_fail(who + ": entry " + std::to_string(k) + " has no source and is not fixed");
    if (src_mkf[k] >= 0 && (src_cam[k] < 0 || src_cam[k] >= g->rig.ncam)) return img_fail(who + ": entry " + std::to_string(k) + " names source camera " + std::to_string(src_cam[k]));
  }
  if (count && mg_distinct(g->sorted_ids, rows, count, who, "row")) return -1;
  if (count == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  const size_t o_ids = tm_align(sizeof(MgPoint)*(size_t)count), need = o_ids + sizeof(int)*(size_t)count;
  mcp_map_graph::Guard G(g);
  if (g->stage(G, need) || g->grow_points(G, R)) return -1;
  MgPoint* rec = reinterpret_cast<MgPoint*>(g->up.in.p);
  for (int k = 0; k < count; ++k) { rec[k].src_mkf = src_mkf[k] < 0 ? -1 : src_mkf[k]; rec[k].src_cam = src_mkf[k] < 0 ? 0 : src_cam[k]; rec[k].flags = flags[k]; rec[k].pending = 0; }      // (a row that is written starts without a pending mark: mcp_map_cull_*)
  std::memcpy(g->up.in.p + o_ids, rows, sizeof(int)*(size_t)count);
  ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, need, hipMemcpyHostToDevice, g->m->st));
  hipLaunchKernelGGL(k_mg_points_scatter, dim3(mg_grid(count)), dim3(MG_BLOCK), 0, g->m->st, g->pts.p, count, (const int*)(g->up.dev.p + o_ids), (const MgPoint*)g->up.dev.p);
  ICK(hipGetLastError());
  return g->staged_now();
}

int mcp_map_graph_add_meas(mcp_map_graph* g, int count, const int* mkf, const int* cam, const int* row, const double* uv, const int* level, const int* source) {
  const std::string who = "mcp_map_graph_add_meas";
  if (!g) return img_fail(who + ": NULL graph");
  if (count < 0 || (count > 0 && (!mkf || !cam || !row || !uv || !level || !source))) return img_fail(who + ": bad arguments");
  if ((long long)g->n_store + count > 0x7fffffffLL) return img_fail(who + ": the store is full");
  const int R = g->m->rows;
  for (int k = 0; k < count; ++k) {
    const std::string at = who + ": entry " + std::to_string(k);
    if (!g->mirror.present(mkf[k])) return img_fail(at + " names MKF slot " + std::to_string(mkf[k]) + ", which is not present");
    if (cam[k] < 0 || cam[k] >= g->rig.ncam) return img_fail(at + " names camera " + std::to_string(cam[k]));
    if (mg_entry_check(at, row[k], R, level[k], uv + 2*(size_t)k)) return -1;
  }
  const int first = g->n_store;
  if (count == 0) return first;
  ICK(hipSetDevice(g->m->device));
  mcp_map_graph::Guard G(g);
  if (g->stage(G, sizeof(MgMeas)*(size_t)count) || g->grow_store(G, (size_t)first + count)) return -1;
  MgMeas* rec = reinterpret_cast<MgMeas*>(g->up.in.p);
  for (int k = 0; k < count; ++k) {
    rec[k].uv[0] = uv[2*(size_t)k]; rec[k].uv[1] = uv[2*(size_t)k + 1]; rec[k].mkf = mkf[k]; rec[k].cam = cam[k]; rec[k].row = row[k];
    rec[k].level = level[k]; rec[k].source = source[k]; rec[k].alive = 1;
  }
  ICK(hipMemcpyAsync(g->store.p + first, g->up.in.p, sizeof(MgMeas)*(size_t)count, hipMemcpyHostToDevice, g->m->st));
  if (g->staged_now()) return -1;
  g->n_store += count; g->n_live += count;
  return first;
}

// the erase kernel over the store, the count of the dead read back
static int mg_erase_run(mcp_map_graph* g, const unsigned long long* d_keys, int n_keys, int slot) {
  hipStream_t st = g->m->st;
  ICK(hipMemsetAsync(&g->ctl.p->erased, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_mg_erase, dim3(mg_grid1(g->n_store)), dim3(MG_BLOCK), 0, st, g->store.p, g->n_store, d_keys, n_keys, slot, g->slots.p, g->ctl.p, (const int*)nullptr);
  ICK(hipGetLastError());
  ICK(hipMemcpyAsync(g->h_ctl.p, g->ctl.p, sizeof(MgCtl), hipMemcpyDeviceToHost, st));
  if (g->sync()) return -1;
  const int died = g->h_ctl.p->erased;
  g->n_live -= died;
  return died;
}

int mcp_map_graph_erase_meas(mcp_map_graph* g, int count, const int* mkf, const int* cam, const int* row) {
  const std::string who = "mcp_map_graph_erase_meas";
  if (!g) return img_fail(who + ": NULL graph");
  if (count < 0 || (count > 0 && (!mkf || !cam || !row))) return img_fail(who + ": bad arguments");
  std::vector<unsigned long long>& keys = g->keys;
  keys.resize(count);
  for (int k = 0; k < count; ++k) {
    if (mkf[k] < 0 || mkf[k] >= MCP_MAP_MAX_MKFS || cam[k] < 0 || cam[k] >= MCP_MAX_FRAME_CAMS || row[k] < 0) return img_fail(who + ": key " + std::to_string(k) + " is out of range");
    keys[k] = mg_key(mkf[k], cam[k], row[k]);
  }
  std::sort(keys.begin(), keys.end());
  for (int k = 1; k < count; ++k) if (keys[k] == keys[k - 1]) return img_fail(who + ": a key appears twice");
  if (count == 0 || g->n_store == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  mcp_map_graph::Guard G(g);
  if (g->stage(G, 8*(size_t)count)) return -1;
  std::memcpy(g->up.in.p, keys.data(), 8*(size_t)count);
  ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, 8*(size_t)count, hipMemcpyHostToDevice, g->m->st));
  return mg_erase_run(g, (const unsigned long long*)g->up.dev.p, count, -1);
}

int mcp_map_graph_erase_mkf(mcp_map_graph* g, int slot) {
  if (!g) return img_fail("mcp_map_graph_erase_mkf: NULL graph");
  if (slot < 0 || slot >= MCP_MAP_MAX_MKFS) return img_fail("mcp_map_graph_erase_mkf: slot " + std::to_string(slot) + " is outside 0.." + std::to_string(MCP_MAP_MAX_MKFS - 1));
  ICK(hipSetDevice(g->m->device));
  const int died = mg_erase_run(g, nullptr, 0, slot);
  if (died >= 0) g->mirror.set(slot, g->mirror.flags_of(slot) & ~MCP_MKF_PRESENT);
  return died;
}

int mcp_map_graph_compact(mcp_map_graph* g) {
  if (!g) return img_fail("mcp_map_graph_compact: NULL graph");
  if (g->n_live == g->n_store) return 0;
  ICK(hipSetDevice(g->m->device));
  const int n = g->n_store, nblk = mg_grid(n);
  mcp_map_graph::Guard G(g);
  if (G.grow(g->store_alt, g->store.n) || G.grow(g->blk, nblk)) return -1;
  hipLaunchKernelGGL(k_mg_compact_mark, dim3(nblk), dim3(MG_BLOCK), 0, g->m->st, (const MgMeas*)g->store.p, n, g->blk.p);
  hipLaunchKernelGGL(k_mg_compact_scatter, dim3(nblk), dim3(MG_BLOCK), 0, g->m->st, (const MgMeas*)g->store.p, n, nblk, (const int*)g->blk.p, g->store_alt.p, g->n_live);
  ICK(hipGetLastError());
  g->store.swap(g->store_alt);
  g->n_store = g->n_live;
  return 0;
}

int mcp_map_graph_num_meas(mcp_map_graph* g, int* live, int* stored) {
  if (!g) return img_fail("mcp_map_graph_num_meas: NULL graph");
  if (!live || !stored) return img_fail("mcp_map_graph_num_meas: bad arguments");
  ICK(hipSetDevice(g->m->device));
  if (g->sync()) return -1;
  *live = g->n_live; *stored = g->n_store;
  return 0;
}

int mcp_map_graph_get_meas(mcp_map_graph* g, int first, int count, int* mkf, int* cam, int* row, double* uv, int* level, int* source, uint8_t* alive) {
  if (!g) return img_fail("mcp_map_graph_get_meas: NULL graph");
  if (first < 0 || count < 0 || (long long)first + count > g->n_store) return img_fail("mcp_map_graph_get_meas: bad range");
  if (count == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  std::vector<MgMeas> tmp;
  if (g->read_back(tmp, g->store.p + first, (size_t)count)) return -1;
  for (int k = 0; k < count; ++k) {
    const MgMeas& E = tmp[k];
    if (mkf) mkf[k] = E.mkf; if (cam) cam[k] = E.cam; if (row) row[k] = E.row; if (uv) { uv[2*(size_t)k] = E.uv[0]; uv[2*(size_t)k + 1] = E.uv[1]; }
    if (level) level[k] = E.level; if (source) source[k] = E.source; if (alive) alive[k] = E.alive ? 1 : 0;
  }
  return 0;
}

int mcp_map_graph_good_counts(mcp_map_graph* g, int first, int count, int* out) {
  if (!g) return img_fail("mcp_map_graph_good_counts: NULL graph");
  const int R = g->m->rows;
  if (first < 0 || count < 0 || (long long)first + count > R || (count > 0 && !out)) return img_fail("mcp_map_graph_good_counts: bad arguments");
  if (count == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  mcp_map_graph::Guard G(g);
  if (G.grow(g->marks, R)) return -1;
  hipStream_t st = g->m->st;
  ICK(hipMemsetAsync(g->marks.p, 0, sizeof(int)*(size_t)R, st));
  if (g->n_store) { g->good_counts_enqueue(R); ICK(hipGetLastError()); }
  ICK(hipMemcpyAsync(out, g->marks.p + first, sizeof(int)*(size_t)count, hipMemcpyDeviceToHost, st));
  return g->sync();
}

int mcp_map_graph_check(mcp_map_graph* g, int* n_dup, int* n_dead) {
  if (!g) return img_fail("mcp_map_graph_check: NULL graph");
  if (!n_dup || !n_dead) return img_fail("mcp_map_graph_check: bad arguments");
  *n_dup = 0; *n_dead = 0;
  if (g->n_store == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  std::vector<MgMeas> tmp;
  if (g->read_back(tmp, g->store.p, (size_t)g->n_store)) return -1;
  std::vector<unsigned long long> keys;
  for (const MgMeas& E : tmp) { if (E.alive) keys.push_back(mg_key(E.mkf, E.cam, E.row)); else ++*n_dead; }
  std::sort(keys.begin(), keys.end());
  for (size_t k = 1; k < keys.size(); ++k) if (keys[k] == keys[k - 1]) ++*n_dup;
  return 0;
}

int mcp_map_bundle_select(mcp_map_graph* g, const mcp_bundle_select_params* p, mcp_bundle_select_result* res) {
  const std::string who = "mcp_map_bundle_select";
  if (!g) return img_fail(who + ": NULL graph");
  if (!res) return img_fail(who + ": NULL result");
  const std::string bad = mg_params_check(p);
  if (!bad.empty()) return img_fail(who + ": " + bad);
  if (p->mode == MCP_BUNDLE_RECENT && !g->mirror.present(p->newest)) return img_fail(who + ": the newest MKF (slot " + std::to_string(p->newest) + ") is not present");
  mcp_map_points* m = g->m;
  mcp_map_graph::Sel& s = g->sel;
  ICK(hipSetDevice(m->device));
  const int R = m->rows, M = g->n_store;
  const int nbr = mg_grid1(R), nbm = mg_grid1(M);
  const size_t n_marks = (size_t)MCP_MAP_MAX_MKFS + 2*(size_t)std::max(R, 1);
  // everything is allocated before the first enqueue (the pinned views of the last call are replaced only here, past the refusals)
  mcp_map_graph::Guard G(g);
  if (G.grow(g->marks, n_marks) || G.grow(s.bidx, R) || G.grow(s.rows, R) || G.grow(s.mkeep, M) || G.grow(g->blk, (size_t)nbr + nbm) || G.grow(s.v_points, R) || G.grow(s.v_meas, M) ||
      g->grow_points(G, R)) return -1;
  s.n_mkfs = s.n_points = s.n_meas = 0; s.t.timed = false;
  MgSelect S; S.mode = p->mode; S.newest = p->newest; S.n_recent = p->n_recent; S.recent_min_size = p->recent_min_size; S.min_points = p->min_points; S.frac = p->mean_diff_fraction;
  int* mkf_in = g->marks.p; int* good = mkf_in + MCP_MAP_MAX_MKFS; int* seen = good + std::max(R, 1);
  int* blk_rows = g->blk.p; int* blk_meas = blk_rows + nbr;
  hipStream_t st = m->st;
  const dim3 B(MG_BLOCK);
  Drain drain{m, true};
  if (s.t.begin(st)) return -1;
  ICK(hipMemsetAsync(g->marks.p, 0, sizeof(int)*n_marks, st));
  ICK(hipMemsetAsync(g->blk.p, 0, sizeof(int)*((size_t)nbr + nbm), st));
  hipLaunchKernelGGL(k_mg_closest, dim3(1), B, 0, st, S, g->rig, (const MgMkf*)g->slots.p, s.adjust.p, g->ctl.p);
  hipLaunchKernelGGL(k_mg_edges_count, dim3(nbm), B, 0, st, (const MgCtl*)g->ctl.p, (const MgMeas*)g->store.p, M, R, (const MgMkf*)g->slots.p, (const uint8_t*)s.adjust.p, good, seen);
  hipLaunchKernelGGL(k_mg_rows_mark, dim3(nbr), B, 0, st, S, g->rig.ncam, g->ctl.p, (const MgMkf*)g->slots.p, (const MgPoint*)g->pts.p, R, (const int*)good, (const int*)seen,
                     s.rows.p, mkf_in, blk_rows);
  hipLaunchKernelGGL(k_mg_rank_mark, dim3(nbr + nbm), B, 0, st, (const MgCtl*)g->ctl.p, R, nbr, (const uint8_t*)s.rows.p, (const int*)blk_rows, s.bidx.p, (const MgMeas*)g->store.p, M,
                     (const MgMkf*)g->slots.p, mkf_in, s.mkeep.p, blk_meas);
  hipLaunchKernelGGL(k_mg_mkfs, dim3(1), B, 0, st, S, g->ctl.p, (const MgMkf*)g->slots.p, (const uint8_t*)s.adjust.p, (const int*)mkf_in, (const int*)blk_rows, nbr,
                     (const int*)blk_meas, nbm, s.mkf_bidx.p, s.v_mkfs.p, s.h_res.p);
  hipLaunchKernelGGL(k_mg_emit, dim3(nbr + nbm), B, 0, st, (const MgCtl*)g->ctl.p, g->rig, (const MgMkf*)g->slots.p, (const int*)s.mkf_bidx.p, (const MgPoint*)g->pts.p,
                     (const PvsPoint*)m->pts.row(), R, nbr, (const int*)s.bidx.p, (const MgMeas*)g->store.p, M, (const uint8_t*)s.mkeep.p, (const int*)blk_meas, nbm,
                     s.v_points.p, R, s.v_meas.p, M);
  ICK(hipGetLastError());
  if (s.t.end(st) || g->one_wait(drain, &s.t)) return -1;
  *res = *s.h_res.p;
  s.n_mkfs = res->n_adjust + res->n_fixed; s.n_points = res->n_points; s.n_meas = res->n_meas;
  return 0;
}

int mcp_map_bundle_select_last_timing(const mcp_map_graph* g, double* device_ms) {
  if (!g || !device_ms) return img_fail("mcp_map_bundle_select_last_timing: bad arguments");
  if (!g->sel.t.timed) return img_fail("mcp_map_bundle_select_last_timing: the last mcp_map_bundle_select on this graph did not run");
  return g->sel.t.ms(device_ms);
}

const mcp_bundle_mkf* mcp_map_bundle_mkfs_view(const mcp_map_graph* g, int* count) {
  if (count) *count = 0;
  if (!g) { img_fail("mcp_map_bundle_mkfs_view: NULL graph"); return nullptr; }
  if (count) *count = g->sel.n_mkfs;
  return g->sel.n_mkfs > 0 ? g->sel.v_mkfs.p : nullptr;
}
const mcp_bundle_point* mcp_map_bundle_points_view(const mcp_map_graph* g, int* count) {
  if (count) *count = 0;
  if (!g) { img_fail("mcp_map_bundle_points_view: NULL graph"); return nullptr; }
  if (count) *count = g->sel.n_points;
  return g->sel.n_points > 0 ? g->sel.v_points.p : nullptr;
}
const mcp_bundle_meas* mcp_map_bundle_meas_view(const mcp_map_graph* g, int* count) {
  if (count) *count = 0;
  if (!g) { img_fail("mcp_map_bundle_meas_view: NULL graph"); return nullptr; }
  if (count) *count = g->sel.n_meas;
  return g->sel.n_meas > 0 ? g->sel.v_meas.p : nullptr;
}

int mcp_map_bundle_select_host(const mcp_bundle_select_params* p, int ncam, const double* cfb, int n_slots, const double* bfw, const int* mflags, const uint8_t* act,
                               const double* dep, int n_rows, const double* world, const int* src_mkf, const int* src_cam, const int* pflags, int n_store, const int* ms_mkf,
                               const int* ms_cam, const int* ms_row, const double* ms_uv, const int* ms_level, const int* ms_source, const uint8_t* ms_alive,
                               mcp_bundle_select_result* res, int cap_mkfs, mcp_bundle_mkf* out_mkfs, int cap_points, mcp_bundle_point* out_points, int cap_meas,
                               mcp_bundle_meas* out_meas) {
  const std::string who = "mcp_map_bundle_select_host";
  if (!res) return img_fail(who + ": NULL result");
  const std::string bad = mg_params_check(p);
  if (!bad.empty()) return img_fail(who + ": " + bad);
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !cfb || n_slots < 0 || n_slots > MCP_MAP_MAX_MKFS || n_rows < 0 || n_store < 0 || cap_mkfs < 0 || cap_points < 0 || cap_meas < 0 ||
      (n_slots > 0 && (!bfw || !mflags || !act || !dep)) || (n_rows > 0 && (!world || !src_mkf || !src_cam || !pflags)) ||
      (n_store > 0 && (!ms_mkf || !ms_cam || !ms_row || !ms_uv || !ms_level || !ms_source || !ms_alive)) || (cap_mkfs > 0 && !out_mkfs) || (cap_points > 0 && !out_points) ||
      (cap_meas > 0 && !out_meas)) return img_fail(who + ": bad arguments");
  if (p->mode == MCP_BUNDLE_RECENT && (p->newest < 0 || p->newest >= n_slots || !(mflags[p->newest] & MCP_MKF_PRESENT)))
    return img_fail(who + ": the newest MKF (slot " + std::to_string(p->newest) + ") is not present");
  MgHostIn I{ncam, cfb, n_slots, bfw, mflags, act, dep, n_rows, world, src_mkf, src_cam, pflags, n_store, ms_mkf, ms_cam, ms_row, ms_uv, ms_level, ms_source, ms_alive};
  mcp_bundle_select_result R;
  std::vector<mcp_bundle_mkf> mk; std::vector<mcp_bundle_point> pt; std::vector<mcp_bundle_meas> ms;
  mg_host_select(*p, I, R, mk, pt, ms);
  if ((int)mk.size() > cap_mkfs || (int)pt.size() > cap_points || (int)ms.size() > cap_meas) return img_fail(who + ": a view does not fit the caller's arrays");
  *res = R;
  if (!mk.empty()) std::memcpy(out_mkfs, mk.data(), sizeof(mcp_bundle_mkf)*mk.size());
  if (!pt.empty()) std::memcpy(out_points, pt.data(), sizeof(mcp_bundle_point)*pt.size());
  if (!ms.empty()) std::memcpy(out_meas, ms.data(), sizeof(mcp_bundle_meas)*ms.size());
  return 0;
}

}  // extern "C"

// ---- the keyframe lists from the store and the one-call write-back over the graph (include/mcp_img.h mcp_graph_*, map_graph_lists.h) -------
namespace {
// the call's slots: distinct, present.  pos_of (MCP_MAP_MAX_MKFS entries) receives the index of each in the call, -1 elsewhere
int mgl_slots_check(const mcp_map_graph* g, const std::string& who, int n_mkfs, const int* slots, std::vector<int>& pos_of) {
  if (n_mkfs < 0) return img_fail(who + ": negative MKF count");
  if (n_mkfs > MCP_MAP_MAX_MKFS) return img_fail(who + ": more than MCP_MAP_MAX_MKFS (" + std::to_string(MCP_MAP_MAX_MKFS) + ") MKFs");
  if (n_mkfs > 0 && !slots) return img_fail(who + ": slots is NULL");
  if (g->n_store > MGL_MAX_STORE) return img_fail(who + ": the store is too long for the list passes");
  pos_of.assign(MCP_MAP_MAX_MKFS, -1);
  for (int i = 0; i < n_mkfs; ++i) {
    const int s = slots[i];
    if (s < 0 || s >= MCP_MAP_MAX_MKFS) return img_fail(who + ": slot " + std::to_string(s) + " is outside 0.." + std::to_string(MCP_MAP_MAX_MKFS - 1));
    if (!g->mirror.present(s)) return img_fail(who + ": MKF slot " + std::to_string(s) + " is not present");
    if (pos_of[s] >= 0) return img_fail(who + ": slot " + std::to_string(s) + " appears twice");
    pos_of[s] = i;
  }
  return 0;
}
// the packed input of the list passes: slot -> index in the call | the call's slots | the solver's pose index of each (write-back only)
struct MglIn {
  size_t pos_of = 0, slots = 0, pose_idx = 0, bytes = 0;
  explicit MglIn(int n_mkfs, size_t at = 0) {
    size_t o = at;
    pos_of = o; o = wb_align(o + sizeof(int)*(size_t)MCP_MAP_MAX_MKFS);
    slots = o; o = wb_align(o + sizeof(int)*(size_t)n_mkfs);
    pose_idx = o; o = wb_align(o + sizeof(int)*(size_t)n_mkfs);
    bytes = o - at;
  }
  void fill(char* h, const std::vector<int>& pos, int n_mkfs, const int* sl, const int* pose) const {
    std::memcpy(h + pos_of, pos.data(), sizeof(int)*(size_t)MCP_MAP_MAX_MKFS);
    if (n_mkfs) std::memcpy(h + slots, sl, sizeof(int)*(size_t)n_mkfs);
    if (n_mkfs && pose) std::memcpy(h + pose_idx, pose, sizeof(int)*(size_t)n_mkfs);
  }
};
// every buffer of the list passes, sized from n_store, n_mkfs, ncam and nb before the first enqueue; the scene-depth scratch of the table with them
int mgl_reserve(mcp_map_graph::Guard& G, mcp_map_graph* g, int n_kf, int nb) {
  const size_t M = (size_t)std::max(g->n_store, 1), K = (size_t)std::max(n_kf, 1);
  mcp_map_graph::Lists& l = g->lists;
  return (G.grow(l.key_row, M) || G.grow(l.rows, M) || G.grow(l.w, M) || G.grow(l.table, K*nb) || G.grow(l.start, K + 1) || G.grow(l.cfw, 12*K) || G.grow(g->m->wb.depth, M) ||
          g->grow_points(G, g->m->rows)) ? -1 : 0;
}
// the three list launches on the table's stream (behind one memset of the count table); d_pos_of: on the device
void mgl_enqueue(mcp_map_graph* g, int n_kf, int nb, const int* d_pos_of) {
  mcp_map_points* m = g->m;
  mcp_map_graph::Lists& l = g->lists;
  const int M = g->n_store, chunk = mgl_chunk_len(M, nb);
  (void)hipMemsetAsync(l.table.p, 0, sizeof(int)*(size_t)std::max(n_kf, 1)*nb, m->st);
  hipLaunchKernelGGL(k_mgl_count, dim3(nb), dim3(MGL_BLOCK), 0, m->st, (const MgMeas*)g->store.p, M, chunk, g->rig.ncam, n_kf, m->rows, d_pos_of, (const MgMkf*)g->slots.p,
                     (const MgPoint*)g->pts.p, l.key_row.p, l.table.p);
  hipLaunchKernelGGL(k_mgl_scan, dim3(1), dim3(MGL_BLOCK), 0, m->st, nb, n_kf, l.table.p, l.start.p);
  hipLaunchKernelGGL(k_mgl_scatter, dim3(nb), dim3(MGL_BLOCK), 0, m->st, (const int2*)l.key_row.p, M, chunk, n_kf, l.table.p, (const int*)l.start.p, (const int*)m->cnt.row(), l.rows.p, l.w.p);
}
// k_wb_scene_depth over the device-built lists (T: 12 doubles per pose, slot: pose of keyframe j or null), then the depth store into the slots
void mgl_depth_enqueue(mcp_map_graph* g, int n_kf, const double* T, const int* slot, const int* d_slots, mcp_scene_depth* sd_pinned) {
  mcp_map_points* m = g->m;
  hipLaunchKernelGGL(k_wb_scene_depth, dim3((unsigned)n_kf), dim3(SD_BLOCK), 0, m->st, T, slot, (const int*)g->lists.start.p, (const int*)g->lists.rows.p, (const double*)g->lists.w.p,
                     m->pts.row(), m->wb.depth.p, sd_pinned, (double*)nullptr);
  hipLaunchKernelGGL(k_mgl_depth_store, dim3(mg_grid(n_kf, MGL_BLOCK)), dim3(MGL_BLOCK), 0, m->st, n_kf, g->rig.ncam, d_slots, (const mcp_scene_depth*)sd_pinned, g->slots.p);
}
}  // namespace

extern "C" {

int mcp_graph_get_mkfs(mcp_map_graph* g, int first, int count, double* bfw, int* flags, uint8_t* act, double* dep) {
  if (!g) return img_fail("mcp_graph_get_mkfs: NULL graph");
  if (first < 0 || count < 0 || (long long)first + count > MCP_MAP_MAX_MKFS) return img_fail("mcp_graph_get_mkfs: bad range");
  if (count == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  std::vector<MgMkf> tmp;
  if (g->read_back(tmp, g->slots.p + first, (size_t)count)) return -1;
  const int nc = g->rig.ncam;
  for (int k = 0; k < count; ++k) {
    if (bfw) std::memcpy(bfw + 12*(size_t)k, tmp[k].bfw, 96);
    if (flags) flags[k] = tmp[k].flags;
    for (int c = 0; c < nc; ++c) { if (act) act[(size_t)k*nc + c] = tmp[k].active[c]; if (dep) dep[(size_t)k*nc + c] = tmp[k].depth[c]; }
  }
  return 0;
}

int mcp_graph_debug_kf_lists(mcp_map_graph* g, int n_mkfs, const int* slots, int blocks, int* seg_start, int cap, int* seg_rows, double* seg_w) {
  const std::string who = "mcp_graph_debug_kf_lists";
  if (!g) return img_fail(who + ": NULL graph");
  if (blocks < 0 || blocks > MGL_MAX_BLOCKS) return img_fail(who + ": blocks outside 0.." + std::to_string(MGL_MAX_BLOCKS));
  if (!seg_start || cap < 0 || (cap > 0 && (!seg_rows || !seg_w))) return img_fail(who + ": bad arguments");
  std::vector<int> pos_of;
  if (mgl_slots_check(g, who, n_mkfs, slots, pos_of)) return -1;
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  const int n_kf = n_mkfs*g->rig.ncam, nb = blocks ? blocks : mgl_default_blocks(g->n_store);
  const MglIn L(n_mkfs);
  const size_t o_rows = wb_align(sizeof(int)*((size_t)n_kf + 1)), o_w = wb_align(o_rows + sizeof(int)*(size_t)std::max(g->n_store, 1));
  mcp_map_graph::Lists& l = g->lists;
  mcp_map_graph::Guard G(g);
  if (G.grow(l.in, L.bytes) || G.grow(l.dev, L.bytes) || G.grow(l.out, o_w + 8*(size_t)std::max(g->n_store, 1)) || mgl_reserve(G, g, n_kf, nb)) return -1;
  L.fill(l.in.p, pos_of, n_mkfs, slots, nullptr);
  Drain drain{m, true};
  ICK(hipMemcpyAsync(l.dev.p, l.in.p, L.bytes, hipMemcpyHostToDevice, m->st));
  mgl_enqueue(g, n_kf, nb, (const int*)(l.dev.p + L.pos_of));
  ICK(hipGetLastError());
  ICK(hipMemcpyAsync(l.out.p, l.start.p, sizeof(int)*((size_t)n_kf + 1), hipMemcpyDeviceToHost, m->st));
  if (g->sync()) return -1;
  std::memcpy(seg_start, l.out.p, sizeof(int)*((size_t)n_kf + 1));
  const int total = seg_start[n_kf];
  if (total > cap) { drain.armed = false; return img_fail(who + ": the lists hold " + std::to_string(total) + " entries, the caller's arrays " + std::to_string(cap)); }
  if (total) {
    ICK(hipMemcpyAsync(l.out.p + o_rows, l.rows.p, sizeof(int)*(size_t)total, hipMemcpyDeviceToHost, m->st));
    ICK(hipMemcpyAsync(l.out.p + o_w, l.w.p, 8*(size_t)total, hipMemcpyDeviceToHost, m->st));
    if (g->sync()) return -1;
    std::memcpy(seg_rows, l.out.p + o_rows, sizeof(int)*(size_t)total);
    std::memcpy(seg_w, l.out.p + o_w, 8*(size_t)total);
  }
  drain.armed = false;
  return total;
}

int mcp_graph_refresh_depth(mcp_map_graph* g, int n_mkfs, const int* slots, mcp_scene_depth* depth_out) {
  const std::string who = "mcp_graph_refresh_depth";
  if (!g) return img_fail(who + ": NULL graph");
  std::vector<int> pos_of;
  if (mgl_slots_check(g, who, n_mkfs, slots, pos_of)) return -1;
  if (n_mkfs == 0) return 0;
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  const int n_kf = n_mkfs*g->rig.ncam, nb = mgl_default_blocks(g->n_store);
  const MglIn L(n_mkfs);
  mcp_map_graph::Lists& l = g->lists;
  mcp_map_graph::Guard G(g);
  if (G.grow(l.in, L.bytes) || G.grow(l.dev, L.bytes) || G.grow(l.out, sizeof(mcp_scene_depth)*(size_t)n_kf) || mgl_reserve(G, g, n_kf, nb)) return -1;
  L.fill(l.in.p, pos_of, n_mkfs, slots, nullptr);
  mcp_scene_depth* sd = reinterpret_cast<mcp_scene_depth*>(l.out.p);
  const int* d_slots = (const int*)(l.dev.p + L.slots);
  Drain drain{m, true};
  m->wb.invalidate();
  ICK(hipEventRecord(m->wb.t[0], m->st));
  ICK(hipMemcpyAsync(l.dev.p, l.in.p, L.bytes, hipMemcpyHostToDevice, m->st));
  ICK(hipEventRecord(m->wb.t[1], m->st)); ICK(hipEventRecord(m->wb.t[2], m->st));
  mgl_enqueue(g, n_kf, nb, (const int*)(l.dev.p + L.pos_of));
  hipLaunchKernelGGL(k_mgl_cfw, dim3(mg_grid(n_kf, MGL_BLOCK)), dim3(MGL_BLOCK), 0, m->st, g->rig, n_kf, d_slots, (const MgMkf*)g->slots.p, l.cfw.p, (double*)nullptr);
  mgl_depth_enqueue(g, n_kf, (const double*)l.cfw.p, nullptr, d_slots, sd);
  const hipError_t le = hipGetLastError();
  (void)hipEventRecord(m->wb.t[3], m->st);
  if (g->one_wait(drain)) return -1;
  if (le != hipSuccess) return img_fail(who + ": launch failed: " + hipGetErrorString(le));
  m->wb.timed = true;
  sd_copy_out(n_kf, sd, depth_out);
  return 0;
}

int mcp_graph_write_back(mcp_ba* h, mcp_map_graph* g, int n_points, const int* point_ids, const int* rows, const int* src_chains, int chain_stride,
                         const int* src_chain_len, double* world_out, double* right_out, double* down_out,
                         int n_mkfs, const int* slots, const int* mkf_pose_ids, const int* cam_pose_ids,
                         double* kf_cfw_out, mcp_scene_depth* depth_out, double* bfw_out) {
  const std::string who = "mcp_graph_write_back";
  if (!h) return img_fail(who + ": NULL solver handle");
  if (!g) return img_fail(who + ": NULL graph");
  mcp_map_points* m = g->m;
  BaDeviceState S;
  if (ba_bridge_state(h, who.c_str(), &S)) return -1;
  if (S.device != m->device) return img_fail(who + ": the table lives on device " + std::to_string(m->device) + ", the solver on device " + std::to_string(S.device));
  if (n_points < 0) return img_fail(who + ": negative point count");
  if (n_points > 0 && (!point_ids || !rows)) return img_fail(who + ": point_ids / rows is NULL");
  if (n_points > 0 && src_chains && !src_chain_len) return img_fail(who + ": src_chain_len is NULL");
  if (n_points > 0 && src_chains && chain_stride < 1) return img_fail(who + ": chain_stride must be positive");
  std::vector<int> pos_of;
  if (mgl_slots_check(g, who, n_mkfs, slots, pos_of)) return -1;
  if (n_mkfs > 0 && (!mkf_pose_ids || !cam_pose_ids)) return img_fail(who + ": mkf_pose_ids / cam_pose_ids is NULL");
  const int nc = g->rig.ncam, n_kf = n_mkfs*nc;
  std::vector<int> pose_idx((size_t)n_mkfs), kf_slot((size_t)n_kf);
  for (int i = 0; i < n_mkfs; ++i) {
    pose_idx[i] = wb_pose_index(h, mkf_pose_ids[i]);
    if (pose_idx[i] < 0 || pose_idx[i] >= S.npose) return img_fail(who + ": mkf_pose_ids[" + std::to_string(i) + "] = " + std::to_string(mkf_pose_ids[i]) + " is not a pose of this bundle");
  }
  for (int c = 0; c < (n_mkfs ? nc : 0); ++c)
    if (wb_pose_index(h, cam_pose_ids[c]) < 0) return img_fail(who + ": cam_pose_ids[" + std::to_string(c) + "] = " + std::to_string(cam_pose_ids[c]) + " is not a pose of this bundle");
  WbPlan plan(h, m, who, chain_stride);
  if (plan.points(n_points, point_ids, rows, src_chains, src_chain_len)) return -1;
  for (int j = 0; j < n_kf; ++j) {
    const int ids[2] = {mkf_pose_ids[j/nc], cam_pose_ids[j % nc]};
    kf_slot[j] = plan.slot_of_chain(ids, 2, "the chain of keyframe", j);
    if (kf_slot[j] < 0) return -1;
  }
  if (n_points == 0 && n_mkfs == 0) return 0;
  // ---- every check has passed: from here on things are enqueued ----
  ICK(hipSetDevice(m->device));
  const int nslot = (int)plan.chains.size(), nb = mgl_default_blocks(g->n_store);
  const bool want_vec = n_points > 0 && (world_out || right_out || down_out);
  const WbLayout W(nslot, n_points, n_kf, 0, want_vec, false);                 // (its list fields stay empty: the lists are built on the device)
  const MglIn L(n_mkfs, W.in_bytes);
  const size_t in_bytes = W.in_bytes + L.bytes, o_bfw = W.out_bytes, out_bytes = o_bfw + 96*(size_t)n_mkfs;
  mcp_map_graph::Guard G(g);
  if (G.grow(m->wb.in, in_bytes) || G.grow(m->wb.dev, in_bytes) || G.grow(m->wb.out, out_bytes) || G.grow(m->wb.T, 12*(size_t)nslot) || mgl_reserve(G, g, n_kf, nb)) return -1;
  char* hin = m->wb.in.p;
  std::memcpy(hin + W.chains, plan.chains.data(), sizeof(WbChain)*(size_t)nslot);
  if (n_points) std::memcpy(hin + W.items, plan.items.data(), sizeof(WbItem)*(size_t)n_points);
  if (n_kf) std::memcpy(hin + W.kf_slot, kf_slot.data(), sizeof(int)*(size_t)n_kf);
  L.fill(hin, pos_of, n_mkfs, slots, pose_idx.data());
  Drain drain{m, true};
  // the table's stream waits for whatever the solver's stream still has to write of the state
  ICK(hipEventRecord(m->wb.ev, S.stream));
  ICK(hipStreamWaitEvent(m->st, m->wb.ev, 0));
  m->wb.invalidate();
  ICK(hipEventRecord(m->wb.t[0], m->st));
  ICK(hipMemcpyAsync(m->wb.dev.p, hin, in_bytes, hipMemcpyHostToDevice, m->st));
  ICK(hipEventRecord(m->wb.t[1], m->st));
  const char* din = m->wb.dev.p; char* hout = m->wb.out.p;
  wb_launch_points(m, S, nslot, (const WbChain*)(din + W.chains), kf_cfw_out ? (double*)(hout + W.T) : (double*)nullptr, n_points, (const WbItem*)(din + W.items),
                   want_vec ? (double*)(hout + W.vec) : (double*)nullptr);
  hipError_t le = hipGetLastError();
  (void)hipEventRecord(m->wb.t[2], m->st);
  if (n_mkfs) {
    const int* d_slots = (const int*)(din + L.slots);
    hipLaunchKernelGGL(k_mgl_pose_store, dim3(mg_grid(12*n_mkfs, MGL_BLOCK)), dim3(MGL_BLOCK), 0, m->st, n_mkfs, d_slots, (const int*)(din + L.pose_idx), S.pose,
                       g->slots.p, bfw_out ? (double*)(hout + o_bfw) : (double*)nullptr);
    mgl_enqueue(g, n_kf, nb, (const int*)(din + L.pos_of));
    mgl_depth_enqueue(g, n_kf, (const double*)m->wb.T.p, (const int*)(din + W.kf_slot), d_slots, (mcp_scene_depth*)(hout + W.sd));
  }
  if (le == hipSuccess) le = hipGetLastError();
  (void)hipEventRecord(m->wb.t[3], m->st);
  if (g->one_wait(drain)) return -1;                                  // the solver's memory is not read after this
  if (le != hipSuccess) return img_fail(who + ": launch failed: " + hipGetErrorString(le));
  m->wb.timed = true;
  if (want_vec) wb_copy_vec((const double*)(hout + W.vec), n_points, world_out, right_out, down_out);
  if (n_mkfs) {
    if (kf_cfw_out) for (int j = 0; j < n_kf; ++j) std::memcpy(kf_cfw_out + 12*(size_t)j, hout + W.T + 96*(size_t)kf_slot[j], 96);
    sd_copy_out(n_kf, (const mcp_scene_depth*)(hout + W.sd), depth_out);
    if (bfw_out) std::memcpy(bfw_out, hout + o_bfw, 96*(size_t)n_mkfs);
  }
  return 0;
}

}  // extern "C"

// ---- measurement parcels (include/mcp_img.h mcp_meas_parcel_*, map_graph_parcel.h) ---------------------------------------------------------
struct mcp_meas_parcel {
  mcp_map_points* m = nullptr;                        // the table: its device, its stream, its key column (it must outlive the parcel)
  Buf<mcp_parcel_entry> ent; int n = 0;
  Buf<int> max_lane;                                  // the largest lane of the fill, for the commit's launches (-1: none)
  int h_max_lane = -1; bool lane_known = true;        // ... on the host: known for a host fill, read back by the commit for a device fill
  bool filled = false, committed = false;
  PinBuf<mcp_parcel_entry> up_in; hipEvent_t staged = nullptr; bool stage_busy = false;      // from_host: packed here, copied on the table's stream
  ~mcp_meas_parcel() { if (m && m->st) (void)hipStreamSynchronize(m->st); if (staged) (void)hipEventDestroy(staged); }
  using Guard = Grow<mcp_meas_parcel>;
  int sync() { ICK(m->sync()); return 0; }
  // room for `need` entries, contents not kept (a fill replaces them)
  int reserve(Guard& G, size_t need) { return G.regrow(ent, need, 0); }
  int filled_now(int count, int top, bool known) {
    n = count; h_max_lane = top; lane_known = known; filled = true; committed = false;
    return count;
  }
};

extern "C" {

mcp_meas_parcel* mcp_meas_parcel_create(mcp_map_points* m) {
  if (!m) { mcp_set_error("mcp_meas_parcel_create: NULL table"); return nullptr; }
  if (hipSetDevice(m->device) != hipSuccess) { mcp_set_error("hipSetDevice failed"); return nullptr; }
  mcp_meas_parcel* p = new mcp_meas_parcel(); p->m = m;
  const bool ok = !p->max_lane.alloc(1) && hipEventCreateWithFlags(&p->staged, hipEventDisableTiming) == hipSuccess &&
                  hipMemsetAsync(p->max_lane.p, 0xff, sizeof(int), m->st) == hipSuccess;
  if (!ok) { mcp_set_error("mcp_meas_parcel_create: allocation failed"); delete p; return nullptr; }
  return p;
}
void mcp_meas_parcel_destroy(mcp_meas_parcel* p) { if (p) { (void)hipSetDevice(p->m->device); delete p; } }

int mcp_meas_parcel_from_track(mcp_meas_parcel* p) {
  const std::string who = "mcp_meas_parcel_from_track";
  if (!p) return img_fail(who + ": NULL parcel");
  mcp_map_points* m = p->m;
  if (!m->tr.ok) return img_fail(who + ": the last track / PVS call on this table was no successful mcp_track_map_record, mcp_track_frame_motion or mcp_track_frame_recover");
  const int ncam = m->tr.ncam, n = m->tr.meas_first[ncam];
  ICK(hipSetDevice(m->device));
  mcp_meas_parcel::Guard G(p);
  if (p->reserve(G, (size_t)n)) return -1;
  ICK(hipMemsetAsync(p->max_lane.p, 0xff, sizeof(int), m->st));
  if (n > 0) {
    MgpFirst F; std::memset(&F, 0, sizeof F);
    for (int c = 0; c <= ncam; ++c) F.v[c] = m->tr.meas_first[c];
    hipLaunchKernelGGL(k_mgp_from_track, dim3(mg_grid(n)), dim3(MG_BLOCK), 0, m->st, (const mcp_track_meas*)m->tr.h_meas.p, n, ncam, F,
                       (const TmSrc*)m->src.row(), m->rows, p->ent.p, p->max_lane.p);
    ICK(hipGetLastError());
    m->parcel_reads = true;
  }
  return p->filled_now(n, -1, n == 0);
}

int mcp_meas_parcel_from_refind(mcp_meas_parcel* p) {
  const std::string who = "mcp_meas_parcel_from_refind";
  if (!p) return img_fail(who + ": NULL parcel");
  mcp_map_points* m = p->m;
  if (m->rf.view < 0) return img_fail(who + ": the last mcp_map_refind on this table left no measurements to take");
  const int n = m->rf.view;
  ICK(hipSetDevice(m->device));
  mcp_meas_parcel::Guard G(p);
  if (p->reserve(G, (size_t)n)) return -1;
  ICK(hipMemsetAsync(p->max_lane.p, 0xff, sizeof(int), m->st));
  if (n > 0) {
    hipLaunchKernelGGL(k_mgp_from_refind, dim3(mg_grid(n)), dim3(MG_BLOCK), 0, m->st, reinterpret_cast<const mcp_refind_meas*>(m->rf.out.p + m->rf.meas_off), n,
                       (const TmSrc*)m->src.row(), m->rows, p->ent.p, p->max_lane.p);
    ICK(hipGetLastError());
    m->parcel_reads = true;
  }
  return p->filled_now(n, -1, n == 0);
}

int mcp_meas_parcel_from_host(mcp_meas_parcel* p, int n, const int* lane, const int* row, const double* uv, const int* level) {
  const std::string who = "mcp_meas_parcel_from_host";
  if (!p) return img_fail(who + ": NULL parcel");
  if (n < 0 || (n > 0 && (!lane || !row || !uv || !level))) return img_fail(who + ": bad arguments");
  mcp_map_points* m = p->m;
  const int R = m->rows;
  int top = -1;
  for (int k = 0; k < n; ++k) {
    const std::string at = who + ": entry " + std::to_string(k);
    if (lane[k] < 0) return img_fail(at + " names lane " + std::to_string(lane[k]));
    if (mg_entry_check(at, row[k], R, level[k], uv + 2*(size_t)k)) return -1;
    top = std::max(top, lane[k]);
  }
  ICK(hipSetDevice(m->device));
  if (p->stage_busy) { ICK(hipEventSynchronize(p->staged)); p->stage_busy = false; }
  mcp_meas_parcel::Guard G(p);
  if (G.grow(p->up_in, (size_t)n) || p->reserve(G, (size_t)n)) return -1;
  ICK(hipMemsetAsync(p->max_lane.p, 0xff, sizeof(int), m->st));
  if (n > 0) {
    mcp_parcel_entry* rec = p->up_in.p;
    for (int k = 0; k < n; ++k) { rec[k].uv[0] = uv[2*(size_t)k]; rec[k].uv[1] = uv[2*(size_t)k + 1]; rec[k].lane = lane[k]; rec[k].row = row[k]; rec[k].key = 0; rec[k].level = level[k]; }
    ICK(hipMemcpyAsync(p->ent.p, rec, sizeof(mcp_parcel_entry)*(size_t)n, hipMemcpyHostToDevice, m->st));
    hipLaunchKernelGGL(k_mgp_keys, dim3(mg_grid(n)), dim3(MG_BLOCK), 0, m->st, p->ent.p, n, (const TmSrc*)m->src.row(), R);
    ICK(hipGetLastError());
    ICK(hipEventRecord(p->staged, m->st)); p->stage_busy = true;
  }
  return p->filled_now(n, top, true);
}

int mcp_meas_parcel_size(const mcp_meas_parcel* p) {
  if (!p) return img_fail("mcp_meas_parcel_size: NULL parcel");
  return p->n;
}

int mcp_meas_parcel_get(const mcp_meas_parcel* p, int cap, mcp_parcel_entry* out) {
  if (!p) return img_fail("mcp_meas_parcel_get: NULL parcel");
  if (cap < p->n || (p->n > 0 && !out)) return img_fail("mcp_meas_parcel_get: the parcel holds " + std::to_string(p->n) + " entries, the caller's array " + std::to_string(cap));
  mcp_map_points* m = p->m;
  ICK(hipSetDevice(m->device));
  if (p->n > 0) ICK(hipMemcpyAsync(out, p->ent.p, sizeof(mcp_parcel_entry)*(size_t)p->n, hipMemcpyDeviceToHost, m->st));
  ICK(m->sync());
  return p->n;
}

int mcp_meas_parcel_commit(mcp_map_graph* g, mcp_meas_parcel* p, int n_lanes, const int* lane_mkf, const int* lane_cam, const mcp_parcel_commit_params* prm,
                           mcp_parcel_commit_result* res, int* lane_appended) {
  const std::string who = "mcp_meas_parcel_commit";
  if (!g) return img_fail(who + ": NULL graph");
  if (!p) return img_fail(who + ": NULL parcel");
  if (!prm || !res) return img_fail(who + ": NULL params or result");
  if (p->m != g->m) return img_fail(who + ": the parcel belongs to another table than the graph");
  if (!p->filled) return img_fail(who + ": the parcel was never filled");
  if (p->committed) return img_fail(who + ": the parcel was committed already; a second commit without a refill would duplicate every entry");
  if (n_lanes < 0 || (n_lanes > 0 && (!lane_mkf || !lane_cam))) return img_fail(who + ": bad lane tables");
  for (int l = 0; l < n_lanes; ++l) {
    if (lane_mkf[l] < 0) continue;
    if (!g->mirror.present(lane_mkf[l])) return img_fail(who + ": lane " + std::to_string(l) + " names MKF slot " + std::to_string(lane_mkf[l]) + ", which is not present");
    if (lane_cam[l] < 0 || lane_cam[l] >= g->rig.ncam) return img_fail(who + ": lane " + std::to_string(l) + " names camera " + std::to_string(lane_cam[l]));
  }
  const int n = p->n, first = g->n_store;
  if (p->lane_known && p->h_max_lane >= n_lanes) return img_fail(who + ": the parcel holds an entry of lane " + std::to_string(p->h_max_lane) + ", the call has " + std::to_string(n_lanes) + " lanes");
  if ((long long)first + n > 0x7fffffffLL) return img_fail(who + ": the store is full");
  if (n == 0) {
    std::memset(res, 0, sizeof *res); res->first = first;
    for (int l = 0; lane_appended && l < n_lanes; ++l) lane_appended[l] = 0;
    p->committed = true;
    return 0;
  }
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  const int R = m->rows, nblk = mg_grid(n);
  // staging: lane_mkf | lane_cam up; MgpCtl | lane_appended down.  Everything is allocated before the first enqueue.
  const size_t o_cam = tm_align(sizeof(int)*(size_t)std::max(n_lanes, 1)), up = 2*o_cam, o_lanes = tm_align(sizeof(MgpCtl)), down = o_lanes + sizeof(int)*(size_t)std::max(n_lanes, 1);
  mcp_map_graph::Commit& c = g->commit;
  mcp_map_graph::Guard G(g);
  if (G.grow(c.vd, n) || G.grow(c.blk, nblk) || G.grow(c.dev, down) || G.grow(c.out, down) || g->stage(G, up) || g->grow_store(G, (size_t)first + n) || g->grow_points(G, R)) return -1;
  std::memset(g->up.in.p, 0, up);
  if (n_lanes) { std::memcpy(g->up.in.p, lane_mkf, sizeof(int)*(size_t)n_lanes); std::memcpy(g->up.in.p + o_cam, lane_cam, sizeof(int)*(size_t)n_lanes); }
  hipStream_t st = m->st;
  MgpCommit Q; Q.n = n; Q.n_lanes = n_lanes; Q.cross_camera = prm->cross_camera ? 1 : 0; Q.source = prm->source; Q.first = first; Q.cap = (long long)g->store.n;
  const int* d_mkf = (const int*)g->up.dev.p; const int* d_cam = (const int*)(g->up.dev.p + o_cam);
  MgpCtl* d_ctl = reinterpret_cast<MgpCtl*>(c.dev.p); int* d_lanes = reinterpret_cast<int*>(c.dev.p + o_lanes);
  const dim3 B(MG_BLOCK);
  Drain drain{m, true};
  ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, up, hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(c.dev.p, 0, down, st));
  hipLaunchKernelGGL(k_mgp_judge, dim3(nblk), B, 0, st, Q, (const mcp_parcel_entry*)p->ent.p, d_mkf, d_cam, (const TmSrc*)m->src.row(), R, (const MgPoint*)g->pts.p, g->prow,
                     (const int*)p->max_lane.p, c.vd.p, c.blk.p, d_ctl, d_lanes);
  hipLaunchKernelGGL(k_mgp_append, dim3(nblk), B, 0, st, Q, (const mcp_parcel_entry*)p->ent.p, d_mkf, d_cam, (const uint8_t*)c.vd.p, (const int*)c.blk.p, nblk,
                     (const int*)p->max_lane.p, reinterpret_cast<mcp_store_entry*>(g->store.p));
  ICK(hipGetLastError());
  ICK(hipMemcpyAsync(c.out.p, c.dev.p, down, hipMemcpyDeviceToHost, st));
  if (g->one_wait(drain)) return -1;
  const MgpCtl& C = *reinterpret_cast<const MgpCtl*>(c.out.p);
  p->h_max_lane = C.max_lane; p->lane_known = true;
  if (C.refused) return img_fail(who + ": the parcel holds an entry of lane " + std::to_string(C.max_lane) + ", the call has " + std::to_string(n_lanes) + " lanes");
  res->first = first; res->n_appended = C.counts[MCP_PARCEL_APPENDED]; res->n_skipped_lane = C.counts[MCP_PARCEL_SKIPPED]; res->n_stale = C.counts[MCP_PARCEL_STALE];
  res->n_bad = C.counts[MCP_PARCEL_BAD]; res->n_cross = C.counts[MCP_PARCEL_CROSS];
  if (lane_appended && n_lanes) std::memcpy(lane_appended, c.out.p + o_lanes, sizeof(int)*(size_t)n_lanes);
  g->n_store += res->n_appended; g->n_live += res->n_appended;
  p->committed = true;
  return 0;
}

}  // extern "C"

// ---- outliers and bad points on the device (include/mcp_img.h mcp_map_cull_*; map_graph_cull.h) ---------------------------------------------
extern "C" {

int mcp_map_cull_outliers(mcp_map_graph* g, int n, const int* mkf, const int* cam, const int* row, const mcp_cull_outliers_params* prm, uint8_t* verdict_out,
                          mcp_cull_outliers_result* res) {
  const std::string who = "mcp_map_cull_outliers";
  if (!g) return img_fail(who + ": NULL graph");
  if (!prm || !res) return img_fail(who + ": NULL params or result");
  if (n < 0 || (n > 0 && (!mkf || !cam || !row))) return img_fail(who + ": bad arguments");
  if (prm->bad_good_count < 0) return img_fail(who + ": a negative bad_good_count");
  mcp_map_graph::Cull& c = g->cull;
  std::vector<std::pair<unsigned long long, int>>& keys = c.keys;
  std::vector<MgcRun>& runs = c.runs;
  keys.resize(n); runs.resize(n);
  for (int k = 0; k < n; ++k) {
    if (mkf[k] < 0 || mkf[k] >= MCP_MAP_MAX_MKFS) return img_fail(who + ": key " + std::to_string(k) + " names slot " + std::to_string(mkf[k]) + ", outside 0.." + std::to_string(MCP_MAP_MAX_MKFS - 1));
    if (cam[k] < 0 || cam[k] >= g->rig.ncam) return img_fail(who + ": key " + std::to_string(k) + " names camera " + std::to_string(cam[k]) + ", the rig has " + std::to_string(g->rig.ncam));
    keys[k] = std::make_pair(mgc_key(mkf[k], cam[k], row[k]), k);
    runs[k].row = row[k]; runs[k].idx = k;
  }
  std::sort(keys.begin(), keys.end());
  for (int k = 1; k < n; ++k) if (keys[k].first == keys[k - 1].first) return img_fail(who + ": a key appears twice (list entries " + std::to_string(keys[k - 1].second) + " and " + std::to_string(keys[k].second) + ")");
  if (n == 0) { std::memset(res, 0, sizeof *res); c.t_outliers.timed = false; return 0; }
  std::sort(runs.begin(), runs.end(), [](const MgcRun& a, const MgcRun& b) { return a.row != b.row ? a.row < b.row : a.idx < b.idx; });
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  const int R = m->rows, M = g->n_store;
  // staging: sorted keys | their list indices | the runs up; MgcCtl | verdict bytes down.  Everything is allocated before the first enqueue.
  const size_t o_idx = tm_align(8*(size_t)n), o_runs = o_idx + tm_align(sizeof(int)*(size_t)n), up = o_runs + sizeof(MgcRun)*(size_t)n, o_vd = tm_align(sizeof(MgcCtl)), down = o_vd + (size_t)n;
  mcp_map_graph::Guard G(g);
  if (G.grow(c.ctl, 1) || G.grow(g->marks, R) || G.grow(c.match, n) || G.grow(c.vd, n) || G.grow(c.out, down) || g->stage(G, up) || g->grow_points(G, R)) return -1;
  unsigned long long* hk = reinterpret_cast<unsigned long long*>(g->up.in.p); int* hi = reinterpret_cast<int*>(g->up.in.p + o_idx);
  for (int k = 0; k < n; ++k) { hk[k] = keys[k].first; hi[k] = keys[k].second; }
  std::memcpy(g->up.in.p + o_runs, runs.data(), sizeof(MgcRun)*(size_t)n);
  hipStream_t st = m->st;
  const dim3 B(MG_BLOCK);
  Drain drain{m, true};
  if (c.t_outliers.begin(st)) return -1;
  ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, up, hipMemcpyHostToDevice, st));
  if (R) ICK(hipMemsetAsync(g->marks.p, 0, sizeof(int)*(size_t)R, st));
  ICK(hipMemsetAsync(c.match.p, 0xff, sizeof(int)*(size_t)n, st));
  ICK(hipMemsetAsync(c.ctl.p, 0, sizeof(MgcCtl), st));
  if (M) {
    g->good_counts_enqueue(R);
    hipLaunchKernelGGL(k_mgc_match, dim3(mg_grid(M)), B, 0, st, (const MgMeas*)g->store.p, M, (const unsigned long long*)g->up.dev.p, (const int*)(g->up.dev.p + o_idx), n, c.match.p);
  }
  hipLaunchKernelGGL(k_mgc_judge, dim3(mg_grid(n)), B, 0, st, n, (const MgcRun*)(g->up.dev.p + o_runs), (const int*)c.match.p, g->store.p, (const MgMkf*)g->slots.p, g->pts.p, g->prow, R,
                     (const int*)g->marks.p, prm->bad_good_count, c.vd.p, c.ctl.p);
  ICK(hipGetLastError());
  if (c.t_outliers.end(st)) return -1;
  ICK(hipMemcpyAsync(c.out.p, c.ctl.p, sizeof(MgcCtl), hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(c.out.p + o_vd, c.vd.p, (size_t)n, hipMemcpyDeviceToHost, st));
  if (g->one_wait(drain, &c.t_outliers)) return -1;
  const MgcCtl& C = *reinterpret_cast<const MgcCtl*>(c.out.p);
  res->n_missing = C.verdicts[MCP_CULL_MISSING]; res->n_fixed = C.verdicts[MCP_CULL_FIXED]; res->n_point_bad = C.verdicts[MCP_CULL_POINT_BAD]; res->n_retry = C.verdicts[MCP_CULL_RETRY];
  res->n_never_retry = C.verdicts[MCP_CULL_NEVER_RETRY]; res->n_already_bad = C.verdicts[MCP_CULL_ALREADY_BAD]; res->n_fixed_rows = C.fixed_rows; res->n_rows_marked = C.rows_marked;
  g->n_live -= res->n_retry + res->n_never_retry;
  if (verdict_out) std::memcpy(verdict_out, c.out.p + o_vd, (size_t)n);
  return 0;
}

int mcp_map_cull_sweep(mcp_map_graph* g, const mcp_cull_sweep_params* prm, mcp_cull_sweep_result* res) {
  const std::string who = "mcp_map_cull_sweep";
  if (!g) return img_fail(who + ": NULL graph");
  if (!prm || !res) return img_fail(who + ": NULL params or result");
  if (prm->min_outliers < 0) return img_fail(who + ": a negative min_outliers");
  if (!std::isfinite(prm->outlier_multiplier)) return img_fail(who + ": outlier_multiplier is not finite");
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  const int R = m->rows, M = g->n_store;
  const int nbr = mg_grid1(R), nbm = mg_grid(M);
  mcp_map_graph::Cull& c = g->cull;
  mcp_map_graph::Guard G(g);
  if (G.grow(c.ctl, 1) || G.grow(g->marks, R) || G.grow(c.rep, R) || G.grow(g->blk, nbr) || G.grow(c.out, sizeof(MgcCtl)) || G.grow(c.rows, R) || g->grow_points(G, R)) return -1;
  MgcSweep Q; Q.min_outliers = prm->min_outliers; Q.danglers_on = (prm->danglers && g->mirror.n_present() >= 2) ? 1 : 0; Q.multiplier = prm->outlier_multiplier;
  hipStream_t st = m->st;
  const dim3 B(MG_BLOCK);
  c.nrows = 0;
  Drain drain{m, true};
  if (c.t_sweep.begin(st)) return -1;
  if (R) ICK(hipMemsetAsync(g->marks.p, 0, sizeof(int)*(size_t)R, st));
  ICK(hipMemsetAsync(c.ctl.p, 0, sizeof(MgcCtl), st));
  if (M) g->good_counts_enqueue(R);
  hipLaunchKernelGGL(k_mgc_sweep_rows, dim3(nbr), B, 0, st, Q, g->pts.p, g->prow, R, (const int*)g->marks.p, (const int*)m->cnt.row(), m->pts.row(), c.rep.p, g->blk.p, c.ctl.p);
  hipLaunchKernelGGL(k_mgc_sweep_emit, dim3(nbr + nbm), B, 0, st, R, g->prow, nbr, (const uint8_t*)c.rep.p, (const int*)g->blk.p, c.rows.p, R, g->store.p, M, (const MgPoint*)g->pts.p, c.ctl.p);
  ICK(hipGetLastError());
  if (c.t_sweep.end(st)) return -1;
  ICK(hipMemcpyAsync(c.out.p, c.ctl.p, sizeof(MgcCtl), hipMemcpyDeviceToHost, st));
  if (g->one_wait(drain, &c.t_sweep)) return -1;
  const MgcCtl& C = *reinterpret_cast<const MgcCtl*>(c.out.p);
  res->n_danglers = C.danglers; res->n_tracker_outliers = C.tracker; res->n_reported = C.reported; res->n_bad_rows = C.bad_rows; res->n_meas_erased = C.erased;
  g->n_live -= C.erased; c.nrows = C.reported;
  return 0;
}

const int* mcp_map_cull_rows_view(const mcp_map_graph* g, int* count) {
  if (count) *count = 0;
  if (!g) { img_fail("mcp_map_cull_rows_view: NULL graph"); return nullptr; }
  if (count) *count = g->cull.nrows;
  return g->cull.nrows > 0 ? g->cull.rows.p : nullptr;
}

int mcp_map_cull_last_timing(const mcp_map_graph* g, double* outliers_ms, double* sweep_ms) {
  if (!g) return img_fail("mcp_map_cull_last_timing: NULL graph");
  return ((outliers_ms && g->cull.t_outliers.ms(outliers_ms)) || (sweep_ms && g->cull.t_sweep.ms(sweep_ms))) ? -1 : 0;
}

}  // extern "C"

// ---- the neighbour queries and the removal of an MKF (include/mcp_img.h mcp_map_neighbours, mcp_map_mkf_cull; map_graph_neigh.h) -------------
namespace {
// the two launches of one query on the table's stream, into entry q of the graph's hand-offs and results (zeroed here).  src_from: see k_mgn_dist
int mgn_enqueue(mcp_map_graph* g, const MgnQuery& Q, int q, const int* src_from) {
  hipStream_t st = g->m->st;
  mcp_map_graph::Neigh& nb = g->neigh;
  ICK(hipMemsetAsync(nb.ctl.p + q, 0, sizeof(MgnCtl), st));
  ICK(hipMemsetAsync(nb.res.p + q, 0, sizeof(mcp_neigh_result), st));
  const int n_idx = mgn_indices(Q.kind, g->mirror.top_present() + 1);      // the slots up to the last present one: nothing above them is a candidate
  hipLaunchKernelGGL(k_mgn_dist, dim3(mg_grid(n_idx)), dim3(MG_BLOCK), 0, st, Q, n_idx, g->rig, (const MgMkf*)g->slots.p, (const MgMkf*)nb.ext.p, src_from, nb.dist.p, nb.cand.p, nb.ctl.p + q);
  hipLaunchKernelGGL(k_mgn_select, dim3(1), dim3(MG_BLOCK), 0, st, Q, n_idx, (const MgMkf*)g->slots.p, (const double*)nb.dist.p, (const uint8_t*)nb.cand.p, nb.ctl.p + q, nb.res.p + q);
  ICK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" {

int mcp_map_neighbours(mcp_map_graph* g, const mcp_neigh_params* p, mcp_neigh_result* res) {
  const std::string who = "mcp_map_neighbours";
  if (!g) return img_fail(who + ": NULL graph");
  if (!res) return img_fail(who + ": NULL result");
  std::string bad = mgn_params_check(p, g->rig.ncam);
  if (bad.empty()) bad = mgn_source_check(p, p->src_slot >= 0 ? g->mirror.flags_of(p->src_slot) : 0, p->src_slot >= 0 ? g->mirror.active(p->src_slot) : nullptr);
  if (!bad.empty()) return img_fail(who + ": " + bad);
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  const MgnQuery Q = mgn_query(*p);
  const bool ext = p->src_slot < 0;
  mcp_map_graph::Neigh& nb = g->neigh;
  mcp_map_graph::Guard G(g);
  if (g->neigh_reserve(G) || (ext && g->stage(G, sizeof(MgMkf)))) return -1;
  if (ext) {
    MgMkf* rec = reinterpret_cast<MgMkf*>(g->up.in.p);
    std::memset(rec, 0, sizeof(MgMkf));
    std::memcpy(rec->bfw, p->ext_base_from_world, 96);
    for (int c = 0; c < g->rig.ncam; ++c) { const bool a = p->ext_active[c] != 0; rec->active[c] = a ? 1 : 0; rec->depth[c] = a ? p->ext_depth_mean[c] : 0.0; }
  }
  hipStream_t st = m->st;
  Drain drain{m, true};
  if (nb.t_query.begin(st)) return -1;
  if (ext) { ICK(hipMemcpyAsync(nb.ext.p, g->up.in.p, sizeof(MgMkf), hipMemcpyHostToDevice, st)); if (g->staged_now()) return -1; }
  if (mgn_enqueue(g, Q, 0, nullptr)) return -1;
  if (Q.want_meas && g->n_store) {
    hipLaunchKernelGGL(k_mgn_count, dim3(mg_grid(g->n_store)), dim3(MG_BLOCK), 0, st, Q.kind, (const MgMeas*)g->store.p, g->n_store, nb.res.p);
    ICK(hipGetLastError());
  }
  if (nb.t_query.end(st)) return -1;
  ICK(hipMemcpyAsync(nb.out.p, nb.res.p, sizeof(mcp_neigh_result), hipMemcpyDeviceToHost, st));
  if (g->one_wait(drain, &nb.t_query)) return -1;
  std::memcpy(res, nb.out.p, sizeof(mcp_neigh_result));
  return 0;
}

int mcp_map_neighbours_last_timing(const mcp_map_graph* g, double* device_ms) {
  if (!g || !device_ms) return img_fail("mcp_map_neighbours_last_timing: bad arguments");
  return g->neigh.t_query.ms(device_ms);
}

}  // extern "C"

// ---- the co-visible points of the nearest keyframe (include/mcp_img.h mcp_map_collect_nearest, mcp_track_collect_nearest; map_graph_collect.h) ----
// what both routes refuse in the parameters; ncam: the cameras looked at, use: which of them (NULL: all)
static std::string mgcl_params_check(const mcp_collect_params* p, int ncam, const uint8_t* use) {
  if (!p) return "NULL params";
  if (!std::isfinite(p->mean_diff_fraction)) return "mean_diff_fraction is not finite";
  for (int c = 0; c < ncam; ++c)
    if ((!use || use[c]) && !(std::isfinite(p->depth_mean[c]) && p->depth_mean[c] > 0.0)) return "camera " + std::to_string(c) + ": the depth mean of a used camera must be finite and positive";
  return "";
}
// the memset and the five launches on the table's stream between the timer's events (the graph's scratch reserved, h_rep cleared by the
// caller).  d_bfw: the pose in device memory; gate: NULL, or the device-side word behind which the stages run
static int mgcl_enqueue(mcp_map_graph* g, const MgclIn& In, const double* d_bfw, const int* gate) {
  hipStream_t st = g->m->st;
  mcp_map_graph::Collect& C = g->collect;
  const int R = g->m->rows, M = g->n_store;
  const dim3 GM(mg_grid(M)), B(MG_BLOCK);
  if (C.t.begin(st)) return -1;
  ICK(hipMemsetAsync(C.marks.p, 0, mcp_map_graph::Collect::bytes(R), st));
  ICK(hipMemsetAsync(C.rep.p, 0, sizeof(mcp_collect_report), st));
  hipLaunchKernelGGL(k_mgcl_nearest, dim3(MCP_MAX_FRAME_CAMS), B, 0, st, gate, In, d_bfw, g->rig, (const MgMkf*)g->slots.p, g->mirror.top_present() + 1, C.rep.p);
  if (M) {
    hipLaunchKernelGGL(k_mgcl_seed, GM, B, 0, st, gate, (const mcp_collect_report*)C.rep.p, (const MgMeas*)g->store.p, M, R, C.seed());
    hipLaunchKernelGGL(k_mgcl_kfs, GM, B, 0, st, gate, (const MgMeas*)g->store.p, M, R, (const uint8_t*)C.seed(), C.kf_mark());
    hipLaunchKernelGGL(k_mgcl_rows, GM, B, 0, st, gate, (const MgMeas*)g->store.p, M, R, (const uint8_t*)C.kf_mark(), C.near(R));
  }
  hipLaunchKernelGGL(k_mgcl_counts, dim3(1), dim3(MGCL_COUNT_BLOCK), 0, st, gate, (const uint8_t*)C.kf_mark(), (const uint8_t*)C.seed(), (const uint8_t*)C.near(R), R, C.rep.p, C.h_rep.p);
  ICK(hipGetLastError());
  return C.t.end(st);
}

static int collect_frame_check(const std::string& who, const mcp_map_points* m, int ncam) {
  if (ncam == m->co.g->rig.ncam) return 0;
  return img_fail(who + ": mcp_track_collect_nearest is on and the frame has " + std::to_string(ncam) + " cameras, the graph " + std::to_string(m->co.g->rig.ncam));
}
static int collect_frame_reserve(mcp_map_points* m) {
  mcp_map_graph::Guard G(m->co.g);
  return m->co.g->collect_reserve(G);
}
static int collect_frame_enqueue(mcp_map_points* m, int ncam, const double* cfb, const double* host_bfw, const double* d_bfw, const int* d_gate, const uint8_t** near) {
  mcp_map_graph* g = m->co.g;
  mcp_map_graph::Collect& C = g->collect;
  MgclIn In; std::memset(&In, 0, sizeof In);
  In.frac = m->co.p.mean_diff_fraction;
  for (int c = 0; c < ncam; ++c) { In.cfb[c] = se3_of12(cfb + 12*c); In.depth[c] = m->co.p.depth_mean[c]; In.use[c] = 1; }
  C.view = -1;
  mgcl_report_clear(C.h_rep.p);                        // (valid = 0 unless k_mgcl_counts runs)
  if (!d_bfw) {
    std::memcpy(C.h_pose.p, host_bfw, 96);
    ICK(hipMemcpyAsync(C.pose.p, C.h_pose.p, 96, hipMemcpyHostToDevice, m->st));
    d_bfw = C.pose.p;
  }
  if (mgcl_enqueue(g, In, d_bfw, d_gate)) return -1;
  *near = C.near(m->rows);
  return 0;
}
static void collect_frame_done(mcp_map_points* m) {
  m->co.g->collect.t.timed = true;
  m->co.last = *m->co.g->collect.h_rep.p; m->co.ok = true;
}

extern "C" {

int mcp_map_collect_nearest(mcp_map_graph* g, const double bfw[12], const double* cfb, const mcp_collect_params* p, mcp_collect_report* rep, uint8_t* near) {
  const std::string who = "mcp_map_collect_nearest";
  if (!g) return img_fail(who + ": NULL graph");
  if (!bfw || !rep) return img_fail(who + ": NULL pose or report");
  const int nc = g->rig.ncam;
  std::string bad = mgcl_params_check(p, nc, p ? p->active : nullptr);
  if (bad.empty() && !finite12(bfw)) bad = "the pose is not finite";
  for (int c = 0; bad.empty() && cfb && c < nc; ++c) if (!finite12(cfb + 12*(size_t)c)) bad = "a CamFromBase is not finite";
  if (!bad.empty()) return img_fail(who + ": " + bad);
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  mcp_map_graph::Collect& C = g->collect;
  const int R = m->rows;
  mcp_map_graph::Guard G(g);
  if (g->collect_reserve(G) || G.grow(C.h_near, (size_t)R)) return -1;
  MgclIn In; std::memset(&In, 0, sizeof In);
  In.frac = p->mean_diff_fraction;
  for (int c = 0; c < nc; ++c) { In.cfb[c] = cfb ? se3_of12(cfb + 12*c) : g->rig.cfb[c]; In.depth[c] = p->depth_mean[c]; In.use[c] = p->active[c] ? 1 : 0; }
  C.view = -1;
  mgcl_report_clear(C.h_rep.p);
  std::memcpy(C.h_pose.p, bfw, 96);
  hipStream_t st = m->st;
  Drain drain{m, true};
  ICK(hipMemcpyAsync(C.pose.p, C.h_pose.p, 96, hipMemcpyHostToDevice, st));
  if (mgcl_enqueue(g, In, C.pose.p, nullptr)) return -1;
  if (R) ICK(hipMemcpyAsync(C.h_near.p, C.near(R), (size_t)R, hipMemcpyDeviceToHost, st));
  if (g->one_wait(drain, &C.t)) return -1;
  *rep = *C.h_rep.p;
  if (near && R) std::memcpy(near, C.h_near.p, (size_t)R);
  C.view = R;
  return 0;
}

const uint8_t* mcp_map_collect_rows_view(const mcp_map_graph* g, int* count) {
  if (count) *count = 0;
  if (!g || g->collect.view < 0) { img_fail("mcp_map_collect_rows_view: the last collection on this graph was no mcp_map_collect_nearest that succeeded"); return nullptr; }
  if (count) *count = g->collect.view;
  return g->collect.view > 0 ? g->collect.h_near.p : nullptr;
}

int mcp_map_collect_last_timing(const mcp_map_graph* g, double* device_ms) {
  if (!g || !device_ms) return img_fail("mcp_map_collect_last_timing: bad arguments");
  return g->collect.t.ms(device_ms);
}

int mcp_track_collect_nearest(mcp_map_points* m, mcp_map_graph* g, const mcp_collect_params* p) {
  const std::string who = "mcp_track_collect_nearest";
  if (!m) return img_fail(who + ": NULL table");
  if (!g) { m->co.g = nullptr; return 0; }
  if (g->m != m) return img_fail(who + ": the graph's table is not this table");
  const std::string bad = mgcl_params_check(p, g->rig.ncam, nullptr);
  if (!bad.empty()) return img_fail(who + ": " + bad);
  m->co.g = g; m->co.p = *p;
  return 0;
}

int mcp_track_collect_last(const mcp_map_points* m, mcp_collect_report* out) {
  if (!m || !out) return img_fail("mcp_track_collect_last: NULL table or report");
  if (!m->co.ok) return img_fail("mcp_track_collect_last: the last track / PVS call on this table did not succeed with mcp_track_collect_nearest on");
  *out = m->co.last;
  return 0;
}

int mcp_map_mkf_cull(mcp_map_graph* g, const mcp_mkf_cull_params* p, mcp_mkf_cull_result* res) {
  const std::string who = "mcp_map_mkf_cull";
  if (!g) return img_fail(who + ": NULL graph");
  if (!p || !res) return img_fail(who + ": NULL params or result");
  mcp_map_graph::Mirror& mir = g->mirror;
  if (p->slot != -1 && !mir.present(p->slot)) return img_fail(who + ": the victim (slot " + std::to_string(p->slot) + ") is not a present slot");
  if (p->slot == -1 && !mir.present(p->furthest_from)) return img_fail(who + ": furthest_from (slot " + std::to_string(p->furthest_from) + ") is not a present slot");
  if (p->max_kfs < 0) return img_fail(who + ": a negative max_kfs");
  if (!std::isfinite(p->mean_diff_fraction)) return img_fail(who + ": mean_diff_fraction is not finite");
  mcp_map_points* m = g->m;
  ICK(hipSetDevice(m->device));
  const int R = m->rows, M = g->n_store;
  const size_t n_marks = 2*(size_t)std::max(R, 1);
  mcp_map_graph::Neigh& nb = g->neigh;
  mcp_map_graph::Guard G(g);
  if (g->neigh_reserve(G) || G.grow(g->marks, n_marks) || g->grow_points(G, R)) return -1;
  MgnQuery Q;
  Q.kind = MCP_NB_MKF; Q.region = MCP_NB_ALL; Q.src_cam = 0; Q.same_cam = 0; Q.n_max = 1; Q.want_meas = 0; Q.max_dist = HUGE_VAL; Q.frac = p->mean_diff_fraction;
  MgnCullIn P; P.slot = p->slot; P.mark_points = p->mark_points ? 1 : 0; P.max_kfs = p->max_kfs; P.erase = p->erase ? 1 : 0;
  int* live = g->marks.p; int* by_src = live + std::max(R, 1);
  hipStream_t st = m->st;
  const dim3 B(MG_BLOCK), GM(mg_grid1(M));
  Drain drain{m, true};
  if (nb.t_remove.begin(st)) return -1;
  ICK(hipMemsetAsync(nb.cc.p, 0, sizeof(MgnCull), st));
  ICK(hipMemsetAsync(&g->ctl.p->erased, 0, sizeof(int), st));
  const mcp_neigh_result* far = nullptr;
  if (p->slot == -1) {                                 // FurthestMultiKeyFrame(furthest_from)
    Q.order = MCP_NB_FURTHEST; Q.src_slot = p->furthest_from;
    if (mgn_enqueue(g, Q, 0, nullptr)) return -1;
    far = nb.res.p;
  }
  Q.order = MCP_NB_NEAREST; Q.src_slot = p->slot;      // ClosestMultiKeyFrame(victim): used if the victim is fixed
  if (mgn_enqueue(g, Q, 1, far ? &nb.ctl.p->first_slot : nullptr)) return -1;
  hipLaunchKernelGGL(k_mgn_decide, dim3(1), dim3(64), 0, st, P, far, (const mcp_neigh_result*)(nb.res.p + 1), g->slots.p, nb.cc.p);
  if (P.mark_points && M) {
    ICK(hipMemsetAsync(g->marks.p, 0, sizeof(int)*n_marks, st));
    hipLaunchKernelGGL(k_mgn_rows_count, GM, B, 0, st, (const MgnCull*)nb.cc.p, (const MgMeas*)g->store.p, M, R, g->prow, (const MgPoint*)g->pts.p, live, by_src);
  }
  if (M) hipLaunchKernelGGL(k_mgn_mark, GM, B, 0, st, P, nb.cc.p, (const MgMeas*)g->store.p, M, R, g->prow, g->pts.p, (const int*)live, (const int*)by_src);
  if (P.erase) hipLaunchKernelGGL(k_mg_erase, GM, B, 0, st, g->store.p, M, (const unsigned long long*)nullptr, 0, -1, g->slots.p, g->ctl.p, (const int*)&nb.cc.p->victim);
  ICK(hipGetLastError());
  if (nb.t_remove.end(st)) return -1;
  ICK(hipMemcpyAsync(nb.out.p, nb.cc.p, sizeof(MgnCull), hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(g->h_ctl.p, g->ctl.p, sizeof(MgCtl), hipMemcpyDeviceToHost, st));
  if (g->one_wait(drain, &nb.t_remove)) return -1;
  const MgnCull& C = *reinterpret_cast<const MgnCull*>(nb.out.p);
  std::memset(res, 0, sizeof *res);
  res->status = C.status; res->victim = C.victim; res->victim_dist_valid = C.dist_valid; res->victim_dist = C.dist; res->new_fixed = C.new_fixed;
  if (C.status == 0) {
    res->n_victim_meas = C.n_victim_meas; res->n_rows_marked = C.n_rows_marked; res->n_by_count = C.n_by_count; res->n_by_source = C.n_by_source;
    res->n_meas_erased = P.erase ? g->h_ctl.p->erased : 0;
    g->n_live -= res->n_meas_erased;
    if (C.new_fixed >= 0) mir.set(C.new_fixed, mir.flags_of(C.new_fixed) | MCP_MKF_FIXED);
    mir.set(C.victim, (mir.flags_of(C.victim) | MCP_MKF_BAD) & (P.erase ? ~MCP_MKF_PRESENT : ~0));
  }
  return 0;
}

int mcp_map_mkf_cull_last_timing(const mcp_map_graph* g, double* device_ms) {
  if (!g || !device_ms) return img_fail("mcp_map_mkf_cull_last_timing: bad arguments");
  return g->neigh.t_remove.ms(device_ms);
}

}  // extern "C"

// ---- AddStereoMapPoints into the map (include/mcp_img.h mcp_stereo_map_points; stereo_kernels.h, stereo_append.h) ----------------------------
namespace {
// one reference on the source keyframe's slot for the length of the call: the rows' own references are taken after the wait, once `made` is known
struct SlotHold { mcp_map_points* m; int slot1; ~SlotHold() { m->slot_release(slot1); } };
}  // namespace

extern "C" {

int mcp_stereo_map_points(mcp_map_graph* g, mcp_kf* src, const mcp_camera* src_cam, const double src_cfw[12], int level, int n_cand, const mcp_int2* cand,
                          int n_meas, const mcp_stereo_meas* meas, int n_targets, const mcp_stereo_target* targets, const int* target_mkf, const int* target_cam,
                          int n_rows, const int* rows, const int* keys, const mcp_stereo_map_params* prm, mcp_stereo_map_result* res,
                          mcp_stereo_point* out, uint8_t* keep, uint8_t* outcome) {
  static const char* W = "mcp_stereo_map_points";
  const std::string who = W;
  if (!g) return img_fail(who + ": NULL graph");
  if (!prm || !res) return img_fail(who + ": NULL params or result");
  if (stereo_check_source(W, src, src_cam, src_cfw, level, n_cand, cand)) return -1;
  if (n_meas < 0 || (n_meas > 0 && !meas) || n_targets < 0 || (n_targets > 0 && (!targets || !target_mkf || !target_cam))) return img_fail(who + ": negative count or missing array");
  const bool from_store = prm->busy_from_store != 0;
  if (from_store && (meas || n_meas)) return img_fail(who + ": meas given together with busy_from_store");
  if (n_cand > 0 && !keep) return img_fail(who + ": keep is needed");
  for (int k = 0; k < n_meas; ++k)
    if (!std::isfinite(meas[k].root_pos[0]) || !std::isfinite(meas[k].root_pos[1]) || std::fabs(meas[k].root_pos[0]) > 1e9 || std::fabs(meas[k].root_pos[1]) > 1e9)
      return img_fail(who + ": a measurement with a non-finite or huge root position");
  mcp_map_points* m = g->m;
  if (src->device != m->device) return img_fail(who + ": the source is on device " + std::to_string(src->device) + ", the table on device " + std::to_string(m->device));
  if (!g->mirror.present(prm->src_mkf)) return img_fail(who + ": the source names MKF slot " + std::to_string(prm->src_mkf) + ", which is not present");
  if (prm->src_cam < 0 || prm->src_cam >= g->rig.ncam) return img_fail(who + ": the source names camera " + std::to_string(prm->src_cam));
  std::vector<StereoTargetDev> tab(std::max(n_targets, 1));
  for (int t = 0; t < n_targets; ++t) {
    if (stereo_target_dev(W, src, targets[t], tab[t])) return -1;
    if (!g->mirror.present(target_mkf[t])) return img_fail(who + ": target " + std::to_string(t) + " names MKF slot " + std::to_string(target_mkf[t]) + ", which is not present");
    if (target_cam[t] < 0 || target_cam[t] >= g->rig.ncam) return img_fail(who + ": target " + std::to_string(t) + " names camera " + std::to_string(target_cam[t]));
  }
  if (n_rows < n_cand) return img_fail(who + ": n_rows < n_cand");
  if (n_rows > 0 && (!rows || !keys)) return img_fail(who + ": rows and keys are needed");
  int top = m->rows;
  for (int k = 0; k < n_rows; ++k) { if (rows[k] < 0 || rows[k] == 0x7fffffff) return img_fail(who + ": bad row id"); top = std::max(top, rows[k] + 1); }
  if (n_rows && mg_distinct(g->sorted_ids, rows, n_rows, who, "row")) return -1;
  const int first = g->n_store;
  if ((long long)first + 2LL*n_rows > 0x7fffffffLL) return img_fail(who + ": the store is full");
  res->made = 0; res->first_store = first; res->n_busy = from_store ? 0 : n_meas;
  if (n_cand == 0) return 0;                           // (nothing to thin, nothing to create: nothing is enqueued)

  ICK(hipSetDevice(m->device));
  const size_t nto = (size_t)std::max(n_targets, 1)*n_cand;
  if (src->st_tab.alloc(std::max(n_targets, 1)) || src->st_cand.alloc(n_cand) || src->st_meas.alloc(std::max(n_meas, 1)) || src->st_alive.alloc(n_cand) ||
      src->st_outcome.alloc(nto) || src->st_res.alloc(n_cand) || src->st_counts.alloc(n_targets + 1) || src->h_st_out.alloc(n_cand) ||
      src->h_st_counts.alloc(n_targets + 1) || src->h_st_keep.alloc(n_cand) || src->h_st_outcome.alloc(nto)) return -1;
  // the table's columns, then the graph's blocks; each grows with nothing in flight on the block it replaces
  if (m->grow(top) || m->ensure(m->rays)) return -1;
  const int n_store = first, nblk = mg_grid(n_store);
  const size_t o_keys = tm_align(sizeof(int)*(size_t)n_rows), o_tmkf = 2*o_keys, o_tcam = o_tmkf + tm_align(sizeof(int)*(size_t)std::max(n_targets, 1)),
               up = o_tcam + tm_align(sizeof(int)*(size_t)std::max(n_targets, 1));
  mcp_map_graph::Stereo& sg = g->stereo;
  mcp_map_graph::Guard G(g);
  if (g->stage(G, up) || G.grow(sg.n_busy, 1) || G.grow(sg.h_n_busy, 1) || (from_store && (G.grow(sg.busy, n_store) || G.grow(g->blk, nblk))) ||
      g->grow_points(G, m->rows) || g->grow_store(G, (size_t)first + 2*(size_t)n_rows)) return -1;
  std::memset(g->up.in.p, 0, up);
  std::memcpy(g->up.in.p, rows, sizeof(int)*(size_t)n_rows); std::memcpy(g->up.in.p + o_keys, keys, sizeof(int)*(size_t)n_rows);
  if (n_targets) { std::memcpy(g->up.in.p + o_tmkf, target_mkf, sizeof(int)*(size_t)n_targets); std::memcpy(g->up.in.p + o_tcam, target_cam, sizeof(int)*(size_t)n_targets); }
  SlotHold hold{m, m->slot_acquire(std::make_pair((const mcp_kf*)src, kf_live_serial(src)))};

  StereoSrcDev S; S.cam = *src_cam; S.cfw = se3_of12(src_cfw);
  S.img = src->lev[level].img.p; S.w = src->lev[level].w; S.h = src->lev[level].h; S.level = level;
  hipStream_t st = m->st;
  Drain drain{m, true};
  // the table's stream waits for whatever the source's stream still has to write of its frame
  ICK(hipEventRecord(src->ev, src->st));
  ICK(hipStreamWaitEvent(st, src->ev, 0));
  ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, up, hipMemcpyHostToDevice, st));
  if (n_targets) ICK(hipMemcpyAsync(src->st_tab.p, tab.data(), sizeof(StereoTargetDev)*(size_t)n_targets, hipMemcpyHostToDevice, st));
  ICK(hipMemcpyAsync(src->st_cand.p, cand, sizeof(mcp_int2)*(size_t)n_cand, hipMemcpyHostToDevice, st));
  if (n_meas) ICK(hipMemcpyAsync(src->st_meas.p, meas, sizeof(mcp_stereo_meas)*(size_t)n_meas, hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(src->st_counts.p, 0, sizeof(int)*(size_t)(n_targets + 1), st));
  const int nb = (n_cand + 255)/256;
  if (from_store) {
    const mcp_store_entry* store = reinterpret_cast<const mcp_store_entry*>(g->store.p);
    if (n_store) hipLaunchKernelGGL(k_sa_busy_mark, dim3(nblk), dim3(SA_BLOCK), 0, st, store, n_store, prm->src_mkf, prm->src_cam, g->blk.p);
    hipLaunchKernelGGL(k_sa_busy_gather, dim3(mg_grid1(n_store)), dim3(SA_BLOCK), 0, st, store, n_store, nblk, (const int*)g->blk.p, prm->src_mkf, prm->src_cam, sg.busy.p,
                       n_store, sg.n_busy.p);
    hipLaunchKernelGGL(k_sa_thin_busy, dim3(nb), dim3(256), 0, st, n_cand, (const mcp_int2*)src->st_cand.p, (const int*)sg.n_busy.p, n_store, (const mcp_stereo_meas*)sg.busy.p,
                       level, src->st_alive.p);
    ICK(hipMemcpyAsync(sg.h_n_busy.p, sg.n_busy.p, sizeof(int), hipMemcpyDeviceToHost, st));
  } else
    hipLaunchKernelGGL(k_stereo_thin_meas, dim3(nb), dim3(256), 0, st, n_cand, (const mcp_int2*)src->st_cand.p, n_meas, (const mcp_stereo_meas*)src->st_meas.p,
                       level, src->st_alive.p);
  for (int j = 0; j < n_targets; ++j) {
    if (j > 0)
      hipLaunchKernelGGL(k_stereo_thin_new, dim3(nb), dim3(256), 0, st, j, n_cand, (const mcp_int2*)src->st_cand.p, level, (const int*)src->st_counts.p,
                         (const mcp_stereo_point*)src->h_st_out.p, src->st_alive.p);
    hipLaunchKernelGGL(k_stereo_walk, dim3(n_cand), dim3(64), 0, st, S, (const StereoTargetDev*)src->st_tab.p, j, n_cand, (const mcp_int2*)src->st_cand.p,
                       (const uint8_t*)src->st_alive.p, src->st_res.p, src->st_outcome.p);
    hipLaunchKernelGGL(k_stereo_commit, dim3(1), dim3(STEREO_COMMIT_NT), 0, st, j, n_cand, prm->limit, (const uint8_t*)src->st_alive.p, src->st_outcome.p,
                       (const mcp_stereo_point*)src->st_res.p, src->st_counts.p, src->h_st_out.p);
  }
  if (n_targets) {
    SaAppend Q; Q.n_targets = n_targets; Q.n_rows = n_rows; Q.level = level; Q.src_mkf = prm->src_mkf; Q.src_cam = prm->src_cam; Q.slot1 = hold.slot1; Q.first_store = first;
    Q.table_rows = m->rows; Q.graph_rows = g->prow; Q.ncam_states = m->st_ncam; Q.store_cap = (long long)g->store.n;
    const char* d = g->up.dev.p;
    hipLaunchKernelGGL(k_sa_append, dim3(mg_grid(n_cand)), dim3(SA_BLOCK), 0, st, Q, (const int*)src->st_counts.p, (const mcp_stereo_point*)src->h_st_out.p, (const int*)d,
                       (const int*)(d + o_keys), (const int*)(d + o_tmkf), (const int*)(d + o_tcam), m->pts.row(), m->src.row(), m->state_ptrs(), m->cnt.row(), m->rays.row(),
                       g->pts.p, reinterpret_cast<mcp_store_entry*>(g->store.p));
  }
  ICK(hipGetLastError());
  if (g->staged_now()) return -1;
  ICK(hipMemcpyAsync(src->h_st_counts.p, src->st_counts.p, sizeof(int)*(size_t)(n_targets + 1), hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(src->h_st_keep.p, src->st_alive.p, (size_t)n_cand, hipMemcpyDeviceToHost, st));
  if (outcome && n_targets) ICK(hipMemcpyAsync(src->h_st_outcome.p, src->st_outcome.p, (size_t)n_targets*n_cand, hipMemcpyDeviceToHost, st));
  if (g->one_wait(drain)) return -1;
  const int made = src->h_st_counts.p[n_targets];
  if (made < 0 || made > n_cand) return img_fail(who + ": inconsistent device count");
  if (out) std::memcpy(out, src->h_st_out.p, sizeof(mcp_stereo_point)*(size_t)made);
  std::memcpy(keep, src->h_st_keep.p, (size_t)n_cand);
  if (outcome && n_targets) std::memcpy(outcome, src->h_st_outcome.p, (size_t)n_targets*n_cand);
  // the host's mirrors of the rows that were taken
  const std::pair<const mcp_kf*, unsigned long long> id = m->slots[hold.slot1 - 1];
  for (int k = 0; k < made; ++k) {
    const int row = rows[k];
    m->has_rays[row] = 1;
    const int s1 = m->slot_acquire(id);                  // (before the release: a row that keeps its source keeps the slot)
    m->slot_release(m->row_slot[row]);
    m->row_slot[row] = s1;
  }
  g->n_store += 2*made; g->n_live += 2*made;
  res->made = made; res->n_busy = from_store ? *sg.h_n_busy.p : n_meas;
  return made;
}

int mcp_map_points_get_rays(const mcp_map_points* m, int first, int count, double* rays, uint8_t* has) {
  std::vector<char> bounce;                              // (rays == NULL: the read still waits for the stream)
  if (column_get(m, "mcp_map_points_get_rays", m ? &m->rays : nullptr, first, count, rays, &bounce)) return -1;
  for (int k = 0; k < count; ++k) {                      // (the column is created without a fill: a row that was never given rays reads as zeros)
    const uint8_t h = m->has_rays[(size_t)first + k];
    if (has) has[k] = h;
    if (rays && !h) std::memset(rays + 9*(size_t)k, 0, 72);
  }
  return 0;
}

int mcp_map_points_get_source(const mcp_map_points* m, int first, int count, int* keys, int* source_level, int* center_xy, uint8_t* fixed, uint8_t* has_source) {
  std::vector<char> bounce;
  if (column_get(m, "mcp_map_points_get_source", m ? &m->src : nullptr, first, count, nullptr, &bounce)) return -1;
  const TmSrc* h = reinterpret_cast<const TmSrc*>(bounce.data());
  for (int k = 0; k < count; ++k) {
    if (keys) keys[k] = h[k].key; if (source_level) source_level[k] = h[k].level;
    if (center_xy) { center_xy[2*(size_t)k] = h[k].cx; center_xy[2*(size_t)k + 1] = h[k].cy; }
    if (fixed) fixed[k] = h[k].fixed ? 1 : 0; if (has_source) has_source[k] = h[k].slot1 ? 1 : 0;
  }
  return 0;
}

int mcp_map_gp_get(mcp_map_graph* g, int first, int count, int* src_mkf, int* src_cam, int* flags) {
  if (!g) return img_fail("mcp_map_gp_get: NULL graph");
  if (first < 0 || count < 0 || (long long)first + count > g->m->rows) return img_fail("mcp_map_gp_get: bad range");
  if (count == 0) return 0;
  ICK(hipSetDevice(g->m->device));
  const int covered = std::max(0, std::min(count, g->prow - first));
  std::vector<MgPoint> tmp;
  if (covered > 0 ? g->read_back(tmp, (const MgPoint*)(g->pts.p + first), (size_t)covered) : g->sync()) return -1;
  for (int k = 0; k < count; ++k) {
    MgPoint P; P.src_mkf = -1; P.src_cam = 0; P.flags = MCP_GP_BAD; P.pending = 0;      // (k_mg_points_fill's row)
    if (k < covered) P = tmp[k];
    if (src_mkf) src_mkf[k] = P.src_mkf; if (src_cam) src_cam[k] = P.src_cam; if (flags) flags[k] = P.flags;
  }
  return 0;
}

}  // extern "C"

// ---- the map's beginning, its rescale and its re-alignment (include/mcp_img.h mcp_init_depth_map_points, mcp_map_mark_optimized, ----
// ---- mcp_map_rescale, mcp_map_transform; map_life.h) ------------------------------------------------------------------------------
namespace {
// one reference on every source keyframe's slot for the length of the call, as SlotHold (slot_release ignores 0)
struct SlotHolds { mcp_map_points* m; int slot1[MCP_MAX_FRAME_CAMS]; ~SlotHolds() { for (int s : slot1) m->slot_release(s); } };

// a rescale or a rigid motion of the whole map: the MKFs, the rows, and (a rescale with a present slot) the scene depths
int life_move(mcp_map_graph* g, const std::string& who, const MlXform& X, mcp_map_transform_result* res, mcp_scene_depth* depth_out) {
  mcp_map_points* m = g->m;
  std::memset(res, 0, sizeof *res);
  res->n_rows = m->rows;
  std::vector<int> slots;
  for (int k = 0; k < MCP_MAP_MAX_MKFS; ++k) if (g->mirror.present(k)) slots.push_back(k);
  const int n_mkfs = (int)slots.size(), R = m->rows;
  res->n_mkfs = n_mkfs;
  if (R == 0 && n_mkfs == 0) return 0;
  const bool depth = X.kind == ML_SCALE && n_mkfs > 0;
  std::vector<int> pos_of;
  if (depth && mgl_slots_check(g, who, n_mkfs, slots.data(), pos_of)) return -1;
  ICK(hipSetDevice(m->device));
  const int n_kf = n_mkfs*g->rig.ncam, nb = mgl_default_blocks(g->n_store);
  const size_t bits = ((size_t)R + 7)/8;
  const MglIn L(n_mkfs);
  mcp_map_graph::Lists& l = g->lists;
  mcp_map_graph::Life& lf = g->life;
  mcp_map_graph::Guard G(g);
  if (g->stage(G, std::max<size_t>(bits, 1)) || G.grow(lf.cnt, 4) || G.grow(lf.h_cnt, 4)) return -1;
  if (depth ? (G.grow(l.in, L.bytes) || G.grow(l.dev, L.bytes) || G.grow(l.out, sizeof(mcp_scene_depth)*(size_t)n_kf) || mgl_reserve(G, g, n_kf, nb)) : g->grow_points(G, R)) return -1;
  std::memset(g->up.in.p, 0, std::max<size_t>(bits, 1));
  const bool any_rays = m->rays.on;
  for (int r = 0; r < R; ++r) if (any_rays && m->has_rays[r]) g->up.in.p[r >> 3] |= (char)(1 << (r & 7));
  hipStream_t st = m->st;
  Drain drain{m, true};
  if (lf.t_move.begin(st)) return -1;
  if (bits) ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, bits, hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(lf.cnt.p, 0, sizeof(int)*4, st));
  hipLaunchKernelGGL(k_ml_mkfs, dim3(mg_grid(MG_MAX_MKFS)), dim3(ML_BLOCK), 0, st, X, g->slots.p);
  if (R) hipLaunchKernelGGL(k_ml_points, dim3(mg_grid(R)), dim3(ML_BLOCK), 0, st, X, g->rig, R, (const MgMkf*)g->slots.p, (const MgPoint*)g->pts.p, (const uint8_t*)g->up.dev.p,
                            any_rays ? (const double*)m->rays.row() : (const double*)nullptr, m->pts.row(), lf.cnt.p);
  ICK(hipGetLastError());
  if (g->staged_now()) return -1;
  mcp_scene_depth* sd = nullptr;
  if (depth) {                                         // mcp_graph_refresh_depth's submission over every present slot, at the moved state
    L.fill(l.in.p, pos_of, n_mkfs, slots.data(), nullptr);
    sd = reinterpret_cast<mcp_scene_depth*>(l.out.p);
    const int* d_slots = (const int*)(l.dev.p + L.slots);
    m->wb.invalidate();
    ICK(hipMemcpyAsync(l.dev.p, l.in.p, L.bytes, hipMemcpyHostToDevice, st));
    mgl_enqueue(g, n_kf, nb, (const int*)(l.dev.p + L.pos_of));
    hipLaunchKernelGGL(k_mgl_cfw, dim3(mg_grid(n_kf, MGL_BLOCK)), dim3(MGL_BLOCK), 0, st, g->rig, n_kf, d_slots, (const MgMkf*)g->slots.p, l.cfw.p, (double*)nullptr);
    mgl_depth_enqueue(g, n_kf, (const double*)l.cfw.p, nullptr, d_slots, sd);
    ICK(hipGetLastError());
  }
  ICK(hipMemcpyAsync(lf.h_cnt.p, lf.cnt.p, sizeof(int)*4, hipMemcpyDeviceToHost, st));
  if (lf.t_move.end(st) || g->one_wait(drain, &lf.t_move)) return -1;
  res->n_refreshed = lf.h_cnt.p[0]; res->n_no_rays = lf.h_cnt.p[1]; res->n_no_source = lf.h_cnt.p[2];
  if (depth) sd_copy_out(n_kf, sd, depth_out);
  return 0;
}
}  // namespace

extern "C" {

int mcp_init_depth_map_points(mcp_map_graph* g, int ncam, const mcp_init_depth_cam* cams, int n_rows, const int* rows, const int* keys, const mcp_init_depth_params* prm,
                              mcp_init_depth_result* res, mcp_stereo_point* out, uint8_t* keep) {
  static const char* W = "mcp_init_depth_map_points";
  const std::string who = W;
  static const double eye12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  if (!g) return img_fail(who + ": NULL graph");
  if (!prm || !res) return img_fail(who + ": NULL params or result");
  mcp_map_points* m = g->m;
  if (ncam != g->rig.ncam) return img_fail(who + ": ncam is " + std::to_string(ncam) + ", the rig has " + std::to_string(g->rig.ncam) + " cameras");
  if (!cams) return img_fail(who + ": NULL cams");
  if (prm->level < 0 || prm->level >= MCP_LEVELS) return img_fail(who + ": level outside 0..3");
  if (!std::isfinite(prm->init_depth) || !(prm->init_depth > 0.0)) return img_fail(who + ": init_depth must be finite and positive");
  if (!g->mirror.present(prm->src_mkf)) return img_fail(who + ": the source names MKF slot " + std::to_string(prm->src_mkf) + ", which is not present");
  long long total = 0, need = 0;
  for (int c = 0; c < ncam; ++c) {
    const mcp_init_depth_cam& C = cams[c];
    if (C.n_cand < 0 || C.limit < 0) return img_fail(who + ": camera " + std::to_string(c) + " has a negative limit or n_cand");
    total += C.n_cand; need += std::min(C.n_cand, C.limit);
    if (C.n_cand == 0) continue;
    if (stereo_check_source(W, C.src, C.cam, eye12, prm->level, C.n_cand, C.cand)) return -1;
    if (C.src->device != m->device) return img_fail(who + ": camera " + std::to_string(c) + "'s source is on device " + std::to_string(C.src->device) + ", the table on device " + std::to_string(m->device));
  }
  if (total > 0x7fffffffLL) return img_fail(who + ": too many candidates");
  if (n_rows < 0 || n_rows < need) return img_fail(who + ": n_rows < the sum of min(n_cand, limit)");
  if (n_rows > 0 && (!rows || !keys)) return img_fail(who + ": rows and keys are needed");
  if (total > 0 && !keep) return img_fail(who + ": keep is needed");
  int top = m->rows;
  for (int k = 0; k < n_rows; ++k) { if (rows[k] < 0 || rows[k] == 0x7fffffff) return img_fail(who + ": bad row id"); top = std::max(top, rows[k] + 1); }
  if (n_rows && mg_distinct(g->sorted_ids, rows, n_rows, who, "row")) return -1;
  const int first = g->n_store;
  if ((long long)first + n_rows > 0x7fffffffLL) return img_fail(who + ": the store is full");
  std::memset(res, 0, sizeof *res);
  res->first_store = first;
  if (total == 0) return 0;                            // (nothing to thin, nothing to create: nothing is enqueued)

  ICK(hipSetDevice(m->device));
  // the table's columns, then the graph's blocks; each grows with nothing in flight on the block it replaces
  if (m->grow(top) || m->ensure(m->rays)) return -1;
  const int n_store = first, nblk = mg_grid(n_store), n_total = (int)total;
  int nb_max = 1;
  for (int c = 0; c < ncam; ++c) nb_max = std::max(nb_max, mg_grid(cams[c].n_cand));
  const size_t o_keys = tm_align(sizeof(int)*(size_t)n_rows), o_cand = 2*o_keys, up = o_cand + tm_align(sizeof(mcp_int2)*(size_t)n_total);
  mcp_map_graph::Stereo& sg = g->stereo;
  mcp_map_graph::Life& lf = g->life;
  mcp_map_graph::Guard G(g);
  if (g->stage(G, up) || G.grow(sg.n_busy, 1) || G.grow(sg.busy, n_store) || G.grow(g->blk, nblk) || G.grow(lf.alive, n_total) || G.grow(lf.blk, nb_max) || G.grow(lf.ctl, 1) ||
      G.grow(lf.h_ctl, 1) || G.grow(lf.h_keep, n_total) || G.grow(lf.h_out, n_rows) || g->grow_points(G, m->rows) || g->grow_store(G, (size_t)first + (size_t)n_rows)) return -1;
  std::memset(g->up.in.p, 0, up);
  if (n_rows) { std::memcpy(g->up.in.p, rows, sizeof(int)*(size_t)n_rows); std::memcpy(g->up.in.p + o_keys, keys, sizeof(int)*(size_t)n_rows); }
  {
    size_t at = 0;
    for (int c = 0; c < ncam; ++c) { if (cams[c].n_cand) std::memcpy(g->up.in.p + o_cand + sizeof(mcp_int2)*at, cams[c].cand, sizeof(mcp_int2)*(size_t)cams[c].n_cand); at += (size_t)cams[c].n_cand; }
  }
  SlotHolds hold; hold.m = m;
  for (int c = 0; c < MCP_MAX_FRAME_CAMS; ++c)
    hold.slot1[c] = (c < ncam && cams[c].n_cand) ? m->slot_acquire(std::make_pair((const mcp_kf*)cams[c].src, kf_live_serial(cams[c].src))) : 0;

  hipStream_t st = m->st;
  Drain drain{m, true};
  // the table's stream waits for whatever each source's stream still has to write of its frame
  for (int c = 0; c < ncam; ++c) {
    if (!cams[c].n_cand) continue;
    ICK(hipEventRecord(cams[c].src->ev, cams[c].src->st));
    ICK(hipStreamWaitEvent(st, cams[c].src->ev, 0));
  }
  if (lf.t_init.begin(st)) return -1;
  ICK(hipMemcpyAsync(g->up.dev.p, g->up.in.p, up, hipMemcpyHostToDevice, st));
  ICK(hipMemsetAsync(lf.ctl.p, 0, sizeof(MlInitCtl), st));
  const char* d = g->up.dev.p;
  const mcp_store_entry* store = reinterpret_cast<const mcp_store_entry*>(g->store.p);
  size_t at = 0;
  for (int c = 0; c < ncam; ++c) {
    const int n_cand = cams[c].n_cand, nb = mg_grid(n_cand);
    const mcp_int2* d_cand = reinterpret_cast<const mcp_int2*>(d + o_cand) + at;
    uint8_t* d_alive = lf.alive.p + at;
    if (n_cand) {
      if (n_store) hipLaunchKernelGGL(k_sa_busy_mark, dim3(nblk), dim3(SA_BLOCK), 0, st, store, n_store, prm->src_mkf, c, g->blk.p);
      hipLaunchKernelGGL(k_sa_busy_gather, dim3(mg_grid1(n_store)), dim3(SA_BLOCK), 0, st, store, n_store, nblk, (const int*)g->blk.p, prm->src_mkf, c, sg.busy.p, n_store, sg.n_busy.p);
      hipLaunchKernelGGL(k_sa_thin_busy, dim3(nb), dim3(256), 0, st, n_cand, d_cand, (const int*)sg.n_busy.p, n_store, (const mcp_stereo_meas*)sg.busy.p, prm->level, d_alive);
      hipLaunchKernelGGL(k_ml_alive_mark, dim3(nb), dim3(ML_BLOCK), 0, st, n_cand, (const uint8_t*)d_alive, lf.blk.p);
    } else
      ICK(hipMemsetAsync(sg.n_busy.p, 0, sizeof(int), st));      // (no gather ran: the camera reports an empty busy list)
    MlCreate Q; std::memset(&Q, 0, sizeof Q);
    if (n_cand) Q.camera = *cams[c].cam;
    Q.cam = c; Q.n_cand = n_cand; Q.limit = cams[c].limit; Q.level = prm->level; Q.src_mkf = prm->src_mkf; Q.slot1 = hold.slot1[c]; Q.n_rows = n_rows; Q.first_store = first;
    Q.table_rows = m->rows; Q.graph_rows = g->prow; Q.ncam_states = m->st_ncam; Q.init_depth = prm->init_depth; Q.store_cap = (long long)g->store.n;
    hipLaunchKernelGGL(k_ml_create, dim3(mg_grid1(n_cand)), dim3(ML_BLOCK), 0, st, Q, g->rig, (const MgMkf*)g->slots.p, d_cand, (const uint8_t*)d_alive, (const int*)lf.blk.p, nb,
                       (const int*)sg.n_busy.p, lf.ctl.p, (const int*)d, (const int*)(d + o_keys), lf.h_out.p, m->pts.row(), m->src.row(), m->state_ptrs(), m->cnt.row(),
                       m->rays.row(), g->pts.p, reinterpret_cast<mcp_store_entry*>(g->store.p));
    at += (size_t)n_cand;
  }
  ICK(hipGetLastError());
  if (g->staged_now()) return -1;
  ICK(hipMemcpyAsync(lf.h_ctl.p, lf.ctl.p, sizeof(MlInitCtl), hipMemcpyDeviceToHost, st));
  ICK(hipMemcpyAsync(lf.h_keep.p, lf.alive.p, (size_t)n_total, hipMemcpyDeviceToHost, st));
  if (lf.t_init.end(st) || g->one_wait(drain, &lf.t_init)) return -1;
  const MlInitCtl& C = *lf.h_ctl.p;
  int made_total = 0;
  for (int c = 0; c < ncam; ++c) {
    if (C.made[c] < 0 || C.made[c] > std::min(cams[c].n_cand, cams[c].limit) || C.base[c] != made_total) return img_fail(who + ": inconsistent device count");
    made_total += C.made[c];
    res->made[c] = C.made[c]; res->n_busy[c] = C.n_busy[c]; res->n_alive[c] = C.n_alive[c];
  }
  if (made_total > n_rows) return img_fail(who + ": inconsistent device count");
  if (out && made_total) std::memcpy(out, lf.h_out.p, sizeof(mcp_stereo_point)*(size_t)made_total);
  std::memcpy(keep, lf.h_keep.p, (size_t)n_total);
  // the host's mirrors of the rows that were taken
  int k = 0;
  for (int c = 0; c < ncam; ++c) {
    if (!C.made[c]) continue;
    const std::pair<const mcp_kf*, unsigned long long> id = m->slots[hold.slot1[c] - 1];
    for (int j = 0; j < C.made[c]; ++j, ++k) {
      const int row = rows[k];
      m->has_rays[row] = 1;
      const int s1 = m->slot_acquire(id);                // (before the release: a row that keeps its source keeps the slot)
      m->slot_release(m->row_slot[row]);
      m->row_slot[row] = s1;
    }
  }
  g->n_store += made_total; g->n_live += made_total;
  res->made_total = made_total;
  return made_total;
}

int mcp_map_life_last_timing(const mcp_map_graph* g, double* init_depth_ms, double* move_ms) {
  if (!g || !init_depth_ms || !move_ms) return img_fail("mcp_map_life_last_timing: bad arguments");
  ICK(hipSetDevice(g->m->device));
  return (g->life.t_init.ms(init_depth_ms) || g->life.t_move.ms(move_ms)) ? -1 : 0;
}

int mcp_map_mark_optimized(mcp_map_graph* g, int* n_marked) {
  const std::string who = "mcp_map_mark_optimized";
  if (!g) return img_fail(who + ": NULL graph");
  mcp_map_points* m = g->m;
  if (n_marked) *n_marked = 0;
  if (m->rows == 0) return 0;
  ICK(hipSetDevice(m->device));
  mcp_map_graph::Life& lf = g->life;
  mcp_map_graph::Guard G(g);
  if (G.grow(lf.cnt, 4) || G.grow(lf.h_cnt, 4)) return -1;
  Drain drain{m, true};
  ICK(hipMemsetAsync(lf.cnt.p, 0, sizeof(int)*4, m->st));
  hipLaunchKernelGGL(k_ml_mark_optimized, dim3(mg_grid(m->rows)), dim3(ML_BLOCK), 0, m->st, m->rows, std::min(g->prow, m->rows), (const MgPoint*)g->pts.p, m->pts.row(), lf.cnt.p);
  ICK(hipGetLastError());
  ICK(hipMemcpyAsync(lf.h_cnt.p, lf.cnt.p, sizeof(int), hipMemcpyDeviceToHost, m->st));
  if (g->one_wait(drain)) return -1;
  if (n_marked) *n_marked = lf.h_cnt.p[0];
  return 0;
}

int mcp_map_rescale(mcp_map_graph* g, double scale, mcp_map_transform_result* res, mcp_scene_depth* depth_out) {
  const std::string who = "mcp_map_rescale";
  if (!g) return img_fail(who + ": NULL graph");
  if (!res) return img_fail(who + ": NULL result");
  MlXform X;
  if (const char* why = ml_xform_make(ML_SCALE, scale, nullptr, X)) return img_fail(who + ": " + why);
  return life_move(g, who, X, res, depth_out);
}

int mcp_map_transform(mcp_map_graph* g, const double new_from_old[12], mcp_map_transform_result* res) {
  const std::string who = "mcp_map_transform";
  if (!g) return img_fail(who + ": NULL graph");
  if (!res) return img_fail(who + ": NULL result");
  MlXform X;
  if (const char* why = ml_xform_make(ML_RIGID, 1.0, new_from_old, X)) return img_fail(who + ": " + why);
  return life_move(g, who, X, res, nullptr);
}

}  // extern "C"
