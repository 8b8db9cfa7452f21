// mcp_init_depth_points_host / mcp_map_mark_optimized_host / mcp_map_transform_host (include/mcp_img.h): the first points of a map, the end of
// its initialisation and its rescale / re-alignment (map_life.h) from host arrays.  Host code only: the unit is compiled as the host half of a
// HIP source, so that the __host__ __device__ bodies it shares with the kernels (the unprojection, the pixel vectors, the pose products) are
// the very text the device runs, and without fused multiply-add contraction, so that they give the device's bits.
#include <cmath>
#include <cstring>
#include <string>
#define ML_HOST_ONLY
#include "map_life.h"

extern void mcp_set_error(const char* s);     // ba_solver.hip
static int life_fail(const std::string& s) { mcp_set_error(s.c_str()); return -1; }

static mcp::MgRig life_rig(int ncam, const double* cfb) {
  mcp::MgRig rig; std::memset(&rig, 0, sizeof rig); rig.ncam = ncam;
  for (int c = 0; c < ncam; ++c) mcp::mg_se3_of12(cfb + 12*(size_t)c, rig.cfb[c]);
  return rig;
}

extern "C" int mcp_init_depth_points_host(int ncam, const double* cam_from_base, const double src_bfw[12], const mcp_camera* cams, const int* n_cand, const mcp_int2* cand,
                                          const int* limit, const int* n_busy, const mcp_stereo_meas* busy, int n_rows, const int* rows,
                                          const mcp_init_depth_params* prm, int first_store, mcp_init_depth_result* res, uint8_t* keep, mcp_stereo_point* out,
                                          double* world_pos, double* pixel_right_w, double* pixel_down_w, double* rays, int* center_xy, int* gp_src_mkf, int* gp_src_cam,
                                          int* gp_flags, mcp_store_entry* appended) {
  const std::string who = "mcp_init_depth_points_host";
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !cam_from_base || !src_bfw || !cams || !n_cand || !limit || !n_busy || !prm || !res || n_rows < 0 || first_store < 0)
    return life_fail(who + ": bad arguments");
  if (prm->level < 0 || prm->level >= MCP_LEVELS) return life_fail(who + ": level outside 0..3");
  if (!(prm->init_depth - prm->init_depth == 0.0) || !(prm->init_depth > 0.0)) return life_fail(who + ": init_depth must be finite and positive");
  long long total_cand = 0, total_busy = 0, need = 0;
  for (int c = 0; c < ncam; ++c) {
    if (n_cand[c] < 0 || limit[c] < 0 || n_busy[c] < 0) return life_fail(who + ": a negative count");
    total_cand += n_cand[c]; total_busy += n_busy[c]; need += n_cand[c] < limit[c] ? n_cand[c] : limit[c];
  }
  if (n_rows < need) return life_fail(who + ": n_rows < the points the call may make");
  if ((total_cand > 0 && (!cand || !keep)) || (total_busy > 0 && !busy)) return life_fail(who + ": a NULL array");
  if (n_rows > 0 && (!rows || !out || !world_pos || !pixel_right_w || !pixel_down_w || !rays || !center_xy || !gp_src_mkf || !gp_src_cam || !gp_flags || !appended))
    return life_fail(who + ": a NULL array");
  if ((long long)first_store + n_rows > 0x7fffffffLL) return life_fail(who + ": the store is full");
  const mcp::MgRig rig = life_rig(ncam, cam_from_base);
  std::memset(res, 0, sizeof *res);
  res->first_store = first_store;
  int k = 0;
  size_t c0 = 0, b0 = 0;
  for (int c = 0; c < ncam; ++c) {
    mcp::Se3 W;
    mcp::ml_cfw(rig, c, src_bfw, W);
    int alive = 0, made = 0;
    for (int i = 0; i < n_cand[c]; ++i) {
      const mcp_int2 C = cand[c0 + i];
      const bool good = mcp::ml_thin_keep(C.x, C.y, prm->level, n_busy[c], busy + b0);
      keep[c0 + i] = good ? 1 : 0;
      if (!good) continue;
      if (alive++ >= limit[c]) continue;
      mcp_stereo_point& P = out[k];
      mcp::ml_init_point(cams[c], W, prm->level, i, C.x, C.y, prm->init_depth, P);
      mcp::SaRow R; mcp_store_entry unused;
      mcp::sa_point(P, rows[k], prm->level, prm->src_mkf, c, -1, -1, R, appended[k], unused);
      for (int a = 0; a < 3; ++a) {
        world_pos[3*(size_t)k + a] = R.world_pos[a]; pixel_right_w[3*(size_t)k + a] = R.pixel_right_w[a]; pixel_down_w[3*(size_t)k + a] = R.pixel_down_w[a];
      }
      for (int a = 0; a < 9; ++a) rays[9*(size_t)k + a] = R.rays[a];
      center_xy[2*(size_t)k] = R.cx; center_xy[2*(size_t)k + 1] = R.cy;
      gp_src_mkf[k] = R.gp_src_mkf; gp_src_cam[k] = R.gp_src_cam; gp_flags[k] = R.gp_flags;
      ++k; ++made;
    }
    res->made[c] = made; res->n_alive[c] = alive; res->n_busy[c] = n_busy[c];
    c0 += (size_t)n_cand[c]; b0 += (size_t)n_busy[c];
  }
  res->made_total = k;
  return k;
}

extern "C" int mcp_map_mark_optimized_host(int n_rows, int n_point_rows, const int* point_flags, uint8_t* usable) {
  const std::string who = "mcp_map_mark_optimized_host";
  if (n_rows < 0 || n_point_rows < 0 || (n_point_rows > 0 && !point_flags) || (n_rows > 0 && !usable)) return life_fail(who + ": bad arguments");
  int n = 0;
  for (int r = 0; r < n_rows; ++r)
    if (mcp::ml_marks(r, n_point_rows, r < n_point_rows ? point_flags[r] : MCP_GP_BAD)) { usable[r] = 1; ++n; }
  return n;
}

extern "C" int mcp_map_transform_host(int kind, double scale, const double new_from_old[12], int ncam, const double* cam_from_base, int n_slots, double* bfw,
                                      const int* mkf_flags, int n_rows, int n_point_rows, const int* gp_src_mkf, const int* gp_src_cam, const uint8_t* has_rays,
                                      const double* rays, double* world_pos, double* pixel_right_w, double* pixel_down_w, mcp_map_transform_result* res) {
  const std::string who = "mcp_map_transform_host";
  if (ncam < 1 || ncam > MCP_MAX_FRAME_CAMS || !cam_from_base || n_slots < 0 || n_slots > MCP_MAP_MAX_MKFS || (n_slots > 0 && (!bfw || !mkf_flags)) || n_rows < 0 ||
      n_point_rows < 0 || (n_point_rows > 0 && (!gp_src_mkf || !gp_src_cam)) || (n_rows > 0 && (!has_rays || !rays || !world_pos || !pixel_right_w || !pixel_down_w)) || !res)
    return life_fail(who + ": bad arguments");
  mcp::MlXform X;
  if (const char* why = mcp::ml_xform_make(kind, scale, new_from_old, X)) return life_fail(who + ": " + why);
  const mcp::MgRig rig = life_rig(ncam, cam_from_base);
  std::memset(res, 0, sizeof *res);
  res->n_rows = n_rows;
  for (int s = 0; s < n_slots; ++s) {
    if (!(mkf_flags[s] & MCP_MKF_PRESENT)) continue;
    mcp::ml_mkf_move(X, bfw + 12*(size_t)s);
    ++res->n_mkfs;
  }
  for (int r = 0; r < n_rows; ++r) {
    const int sm = r < n_point_rows ? gp_src_mkf[r] : -1, sc = r < n_point_rows ? gp_src_cam[r] : 0;
    const bool source = mcp::ml_has_source(sm, sc, ncam) && sm < n_slots && (mkf_flags[sm] & MCP_MKF_PRESENT);
    const bool has = has_rays[r] != 0;
    const int cls = mcp::ml_row_class(source, has);
    if (cls == mcp::ML_ROW_REFRESHED) ++res->n_refreshed; else if (cls == mcp::ML_ROW_NO_RAYS) ++res->n_no_rays; else ++res->n_no_source;
    if (!source) continue;
    mcp::ml_row_move(X, rig, sc, bfw + 12*(size_t)sm, has, rays + 9*(size_t)r, world_pos + 3*(size_t)r, pixel_right_w + 3*(size_t)r, pixel_down_w + 3*(size_t)r);
  }
  return 0;
}
