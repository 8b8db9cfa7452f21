// refind_kernels.h -- MapMakerServerBase::ReFind_Common over the resident map-point table (src/MapMakerServerBase.cc:921-1002), gfx950.
//
// mcp_map_refind (img_api.hip) enqueues on the table's stream, after ONE copy of the packed inputs (control block and per-workgroup
// counters as zeros | targets | source slots | pairs | the finder's state):
//   k_rf_mark      one thread per pair: the projection of :941-956 through track_project -- the function patch_item runs, so the walk
//                  cannot disagree -- and the row's source slot.  OUTSIDE and NO_SOURCE are final here.  Leaves a flag byte per pair
//                  (survivor, head of a sequence) and the two counts of its workgroup.
//   k_rf_scatter   the survivors in pair order, each as one record (pair, row, target, number of its sequence, the row's patch source): the
//                  counts of the workgroups before its own, ballot ranks inside (k_pvs_scatter's scheme); and per sequence its first survivor.
//   k_rf_walk      one wavefront per sequence that has survivors: grid-stride over the sequence count, which only the device knows; the
//                  wavefront starts at its sequence's first survivor and walks the sequence in order with the finder's members in
//                  registers and its two templates in LDS (patch_item, PF_REFIND, unchanged; its record stays in LDS), the next
//                  survivor's record fetched one item ahead.  Verdict and a measurement candidate per pair, FOUND / TEMPLATE_BAD counted
//                  per RF_BLOCK pairs; the sequence of the last pair leaves the finder's state in pinned memory.
//   k_rf_commit    verdict bytes, the FOUND candidates compacted in pair order, the counts and (when no wavefront walked the last
//                  sequence) the finder's state into pinned host memory.
// Hand-offs are kernel boundaries on one stream; no workgroup waits for another.  Atomics only add integers: the same bytes on every run.
#pragma once
#include "img_kernels.h"
#include "pvs_kernels.h"
#include "track_map_kernels.h"

namespace mcp {

struct RfTarget { DevKfView T; mcp_camera cam; Se3 cfw; };
struct RfCtl { int counts[6]; int n_surv, n_seq; };                      // zeroed by the input copy
struct RfOut { int counts[6]; int n_meas, pad_; mcp_pf_state state; };   // pinned: what the host reads after the wait
constexpr int RF_BLOCK = 256;
constexpr int RF_SURV = 1, RF_HEAD = 2, RF_NONE = 0x7fffffff;
struct RfItem { int pair, row, tgt, seq; TmSrc s; };                      // a survivor, in pair order: its pair, the number of its sequence, its row's patch source

__device__ __forceinline__ void rf_identity(Se3& I) {
#pragma unroll
  for (int k = 0; k < 9; ++k) I.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
  I.t[0] = I.t[1] = I.t[2] = 0.0;
}

__global__ void __launch_bounds__(RF_BLOCK)
k_rf_mark(int n, int per_row, const int* __restrict__ pairs, const RfTarget* __restrict__ tg, const PvsPoint* __restrict__ pts, const TmSrc* __restrict__ src,
          const TmSlot* __restrict__ slots, uint8_t* __restrict__ flags, uint8_t* __restrict__ vd, int* __restrict__ blk_cnt /* nblk x 2 */, int* __restrict__ first /* n */,
          RfCtl* __restrict__ ctl) {
  __shared__ int cnt[4];                                          // survivors, heads, OUTSIDE, NO_SOURCE
  const int t = threadIdx.x, i = blockIdx.x*RF_BLOCK + t;
  if (t < 4) cnt[t] = 0;
  __syncthreads();
  if (i < n) {
    const int row = pairs[2*(size_t)i], tgt = pairs[2*(size_t)i + 1];
    const bool head = i == 0 || !per_row || pairs[2*(size_t)(i - 1)] != row;
    const TmSrc& R = src[row];
    int v = 0;
    if (!(R.slot1 > 0 && slots[R.slot1 - 1].live)) v = MCP_REFIND_NO_SOURCE;
    else {
      const RfTarget& G = tg[tgt];
      Se3 I, cfw; double xc[3]; Projection pr;
      rf_identity(I);                                             // (the map maker's callers: BaseFromWorld = the keyframe's CamFromWorld, CamFromBase = identity)
      if (!track_project(G.cam, G.cfw, I, pts[row].world_pos, cfw, xc, pr)) v = MCP_REFIND_OUTSIDE;
    }
    flags[i] = (uint8_t)((v == 0 ? RF_SURV : 0) | (head ? RF_HEAD : 0));
    vd[i] = (uint8_t)v;
    first[i] = RF_NONE;                                           // (k_rf_scatter: the first survivor of sequence i, if there is such a sequence)
    if (v == 0) atomicAdd(&cnt[0], 1);
    if (head) atomicAdd(&cnt[1], 1);
    if (v == MCP_REFIND_OUTSIDE) atomicAdd(&cnt[2], 1);
    if (v == MCP_REFIND_NO_SOURCE) atomicAdd(&cnt[3], 1);
  }
  __syncthreads();
  if (t == 0) {
    blk_cnt[2*(size_t)blockIdx.x] = cnt[0]; blk_cnt[2*(size_t)blockIdx.x + 1] = cnt[1];
    if (cnt[2]) atomicAdd(&ctl->counts[MCP_REFIND_OUTSIDE], cnt[2]);
    if (cnt[3]) atomicAdd(&ctl->counts[MCP_REFIND_NO_SOURCE], cnt[3]);
  }
}

__global__ void __launch_bounds__(RF_BLOCK)
k_rf_scatter(int n, int nblk, const uint8_t* __restrict__ flags, const int* __restrict__ blk_cnt, const int* __restrict__ pairs, const TmSrc* __restrict__ src,
             RfItem* __restrict__ items, int* __restrict__ first, RfCtl* __restrict__ ctl) {
  constexpr int NW = RF_BLOCK/64;
  __shared__ int before[2], total[2], wcnt[NW][2];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < 2) { before[t] = 0; total[t] = 0; }
  __syncthreads();
  int mb[2] = {0, 0}, mt[2] = {0, 0};
  for (int j = t; j < nblk; j += RF_BLOCK) {
#pragma unroll
    for (int q = 0; q < 2; ++q) { const int v = blk_cnt[2*(size_t)j + q]; mt[q] += v; if (j < b) mb[q] += v; }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) { if (mt[q]) atomicAdd(&total[q], mt[q]); if (mb[q]) atomicAdd(&before[q], mb[q]); }
  const int i = b*RF_BLOCK + t;
  const int f = i < n ? (int)flags[i] : 0;
  const unsigned long long ms = __ballot((f & RF_SURV) != 0), mh = __ballot((f & RF_HEAD) != 0);
  const unsigned long long below = (1ull << lane) - 1ull, upto = below | (1ull << lane);
  const int srank = __popcll(ms & below), hincl = __popcll(mh & upto);
  if (lane == 0) { wcnt[wave][0] = __popcll(ms); wcnt[wave][1] = __popcll(mh); }
  __syncthreads();
  if (b == 0 && t == 0) { ctl->n_surv = total[0]; ctl->n_seq = total[1]; }
  if (!(f & RF_SURV)) return;
  int ks = before[0] + srank, kh = before[1] + hincl - 1;           // (the first pair is a head: kh >= 0)
  for (int w = 0; w < wave; ++w) { ks += wcnt[w][0]; kh += wcnt[w][1]; }
  RfItem& It = items[ks];                                             // ks < total[0] <= n
  It.pair = i; It.row = pairs[2*(size_t)i]; It.tgt = pairs[2*(size_t)i + 1]; It.seq = kh; It.s = src[It.row];
  // the sequence's first survivor: a minimum of integers, the same in any order.  A survivor whose predecessor in the wavefront belongs to the
  // same sequence (no head between them) cannot be it and stays away from the address
  const unsigned long long prev = ms & below;
  bool candidate = true;
  if (prev) { const int pl = 63 - __clzll((long long)prev); candidate = (mh & upto & ~((2ull << pl) - 1ull)) != 0ull; }
  if (candidate) atomicMin(&first[kh], ks);
}

__global__ void __launch_bounds__(64)
k_rf_walk(const RfTarget* __restrict__ tg, const PvsPoint* __restrict__ pts, const TmSlot* __restrict__ slots, const RfItem* __restrict__ items, const int* __restrict__ first,
          const mcp_pf_state* __restrict__ in_state /* the static finder, or null */, uint8_t* __restrict__ vd, mcp_refind_meas* __restrict__ cand /* per pair */,
          int* __restrict__ found_blk, int* __restrict__ bad_blk /* FOUND / TEMPLATE_BAD pairs per RF_BLOCK pairs, zeroed */,
          RfCtl* __restrict__ ctl, mcp_pf_state* __restrict__ out_state /* pinned host */) {
  __shared__ uint8_t tmpl[64], jtmpl[64];
  __shared__ double dprod[3][36];
  __shared__ mcp_td_out O;                                            // patch_item's record: only a few of its fields leave the workgroup
  const int lane = threadIdx.x;
  const int ns = ctl->n_surv, nseq = ctl->n_seq, last_seq = nseq - 1;
  Se3 I; rf_identity(I);
  for (int sq = blockIdx.x; sq < nseq; sq += gridDim.x) {
    const int k = first[sq];
    if (k == RF_NONE) continue;                                       // a sequence without survivors: its finder stays as it is
    RfItem cur = items[k];
    PfRegs S;
    if (sq == 0 && in_state) {                                        // the static finder enters the first sequence ...
      const mcp_pf_state& G = *in_state;
      S.valid = G.valid; S.key = G.point_key; S.bad = G.template_bad; S.jvalid = G.jacs_valid; S.mean = G.mean_diff;
      S.lw[0] = G.last_warp[0]; S.lw[1] = G.last_warp[1]; S.lw[2] = G.last_warp[2]; S.lw[3] = G.last_warp[3];
      tmpl[lane] = G.templ[lane]; jtmpl[lane] = G.jac_templ[lane];
    } else {                                                          // ... every other one starts from a finder that has seen nothing
      S.valid = 0; S.key = 0; S.bad = 0; S.jvalid = 0; S.mean = 0.0; S.lw[0] = S.lw[1] = S.lw[2] = S.lw[3] = 0.0;
      tmpl[lane] = 0; jtmpl[lane] = 0;
    }
    __syncthreads();
    for (int q = k; ; ++q) {
      // the next survivor's record is fetched (whether or not it belongs to this sequence) while this one is searched: one independent
      // load, nothing of the next item waits on the critical path
      const RfItem nxt = items[min(q + 1, ns - 1)];
      const int i = cur.pair;
      const TmSrc& R = cur.s;
      const PvsPoint& Pt = pts[cur.row];
      const TmSlot& Sl = slots[R.slot1 - 1];                          // (a survivor's source is live)
      const RfTarget& G = tg[cur.tgt];
      DevTdIn D;
#pragma unroll
      for (int a = 0; a < 3; ++a) { D.world_pos[a] = Pt.world_pos[a]; D.pixel_right_w[a] = Pt.pixel_right_w[a]; D.pixel_down_w[a] = Pt.pixel_down_w[a]; }
      D.src_img = Sl.img[R.level]; D.src_w = Sl.w[R.level]; D.src_h = Sl.h[R.level]; D.center_x = R.cx; D.center_y = R.cy; D.fixed = R.fixed;
      patch_item(PF_REFIND, G.T, nullptr, G.cam, G.cfw, I, D, R.key, 0.0, 0.0, S, tmpl, jtmpl, O, 4, 8, 0, dprod, lane);      // range 4, :968
      if (lane == 0) {                                                // (lane 0 wrote the fields it reads here)
        int v;
        if (!O.in_image) { v = MCP_REFIND_OUTSIDE; atomicAdd(&ctl->counts[MCP_REFIND_OUTSIDE], 1); }      // (cannot happen: k_rf_mark ran the same projection)
        else if (O.template_bad) { v = MCP_REFIND_TEMPLATE_BAD; atomicAdd(&bad_blk[i/RF_BLOCK], 1); }
        else if (!O.found) v = MCP_REFIND_NOT_FOUND;
        else {
          v = MCP_REFIND_FOUND;
          mcp_refind_meas& M = cand[i];
          M.pair = i; M.row = cur.row; M.target = cur.tgt; M.level = O.search_level; M.subpix = O.did_subpix; M.score = O.score;
          M.root_pos[0] = O.found_pos[0]; M.root_pos[1] = O.found_pos[1];
          atomicAdd(&found_blk[i/RF_BLOCK], 1);                       // (spread over the pair list: no address takes more than RF_BLOCK of them)
        }
        vd[i] = (uint8_t)v;
      }
      __syncthreads();
      if (q + 1 >= ns || nxt.seq != sq) break;
      cur = nxt;
    }
    if (sq == last_seq) {                                             // ... and the finder leaves with the last one
      mcp_pf_state& H = *out_state;
      H.templ[lane] = tmpl[lane]; H.jac_templ[lane] = jtmpl[lane];
      if (lane == 0) {
        H.valid = S.valid; H.point_key = S.key; H.template_bad = S.bad; H.jacs_valid = S.jvalid; H.mean_diff = S.mean;
        H.last_warp[0] = S.lw[0]; H.last_warp[1] = S.lw[1]; H.last_warp[2] = S.lw[2]; H.last_warp[3] = S.lw[3];
      }
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(RF_BLOCK)
k_rf_commit(int n, int nblk, int cap, const uint8_t* __restrict__ vd, const mcp_refind_meas* __restrict__ cand, const int* __restrict__ found_blk,
            const int* __restrict__ bad_blk, const RfItem* __restrict__ items, const RfCtl* __restrict__ ctl, const mcp_pf_state* __restrict__ in_state,
            uint8_t* __restrict__ h_vd, mcp_refind_meas* __restrict__ h_meas, RfOut* __restrict__ h_out) {
  constexpr int NW = RF_BLOCK/64;
  __shared__ int before, total, bad, wcnt[NW];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t == 0) { before = 0; total = 0; bad = 0; }
  __syncthreads();
  int mb = 0, mt = 0, mbad = 0;
  for (int j = t; j < nblk; j += RF_BLOCK) { const int v = found_blk[j]; mt += v; if (j < b) mb += v; if (b == 0) mbad += bad_blk[j]; }
  if (mb) atomicAdd(&before, mb);
  if (mt) atomicAdd(&total, mt);
  if (mbad) atomicAdd(&bad, mbad);
  const int i = b*RF_BLOCK + t;
  const int v = i < n ? (int)vd[i] : 0;
  if (i < n) h_vd[i] = (uint8_t)v;
  const unsigned long long m = __ballot(v == MCP_REFIND_FOUND);
  const int rank = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  const int all = total;
  if (b == 0) {
    const int ns = ctl->n_surv, nseq = ctl->n_seq;
    if (t == 0) {
      // the walk counts FOUND and TEMPLATE_BAD per RF_BLOCK pairs; what is left of the survivors was not found
      const int extra_out = ctl->counts[MCP_REFIND_OUTSIDE];          // (k_rf_mark's count + the walk's, which is 0)
      h_out->counts[0] = 0; h_out->counts[MCP_REFIND_FOUND] = all; h_out->counts[MCP_REFIND_OUTSIDE] = extra_out;
      h_out->counts[MCP_REFIND_TEMPLATE_BAD] = bad; h_out->counts[MCP_REFIND_NO_SOURCE] = ctl->counts[MCP_REFIND_NO_SOURCE];
      h_out->counts[MCP_REFIND_NOT_FOUND] = n - all - bad - extra_out - ctl->counts[MCP_REFIND_NO_SOURCE];
      h_out->n_meas = all; h_out->pad_ = 0;
    }
    if (ns == 0 || items[ns - 1].seq != nseq - 1) {                   // nothing of the last sequence was searched: its finder is as it started
      const bool carry = nseq == 1 && in_state;
      unsigned long long* o = reinterpret_cast<unsigned long long*>(&h_out->state);
      const unsigned long long* s = reinterpret_cast<const unsigned long long*>(in_state);
      if (t < (int)(sizeof(mcp_pf_state)/8)) o[t] = carry ? s[t] : 0ull;
    }
  }
  if (v != MCP_REFIND_FOUND || all > cap) return;                    // over the cap: no measurement is written (the host reports it)
  int off = before + rank;
  for (int w = 0; w < wave; ++w) off += wcnt[w];
  h_meas[off] = cand[i];                                              // off < all <= cap
}

}  // namespace mcp
