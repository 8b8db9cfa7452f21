// Unit check of the building blocks of mcptam_amd/csrc/ba_select.h against std::sort: block_find_rank, sel_find_bin, lds_find_bin and
// lds_radix_select in kernels of their own, and the full six-pass chain k_select_pass x 6 + k_select_final (which the solver reaches
// only behind a multi-rank table overflow) on grids of 1, 2 and 1024 workgroups.
// Build: hipcc --offload-arch=gfx950 -O2 -munsafe-fp-atomics -I mcptam_amd/csrc tests/cpp/ba_select_check.hip -o ba_select_check ;
// prints one line per mismatch and "ok <cases>" at the end.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "ba_select.h"
using namespace mcp;
typedef unsigned long long u64;

constexpr int MAXN = 70000, MAXK = 2*1024 + 8;

template <int NT> __global__ void __launch_bounds__(NT) k_bfr(const u64* loc, const u64* ks, int nk, int* t_out, u64* e_out) {
  __shared__ u64 lds[NT/64 + 2];
  for (int i = 0; i < nk; ++i) {                       // (call after call on the same LDS words, as the passes of a select make them)
    int t; u64 e;
    block_find_rank<NT>(loc[threadIdx.x], ks[i], t, e, lds);
    if (threadIdx.x == 0) { t_out[i] = t; e_out[i] = e; }
  }
}
__global__ void __launch_bounds__(SEL_BLOCK) k_sfb(const double* hist, int nbins, const u64* ks, int nk, int* b_out, u64* k_out) {
  __shared__ u64 lds[SEL_BLOCK + 2];
  for (int i = 0; i < nk; ++i) {
    int b; u64 kin;
    sel_find_bin(hist, nbins, ks[i], b, kin, lds);
    if (threadIdx.x == 0) { b_out[i] = b; k_out[i] = kin; }
  }
}
template <int NT> __global__ void __launch_bounds__(NT) k_lfb(const unsigned int* ghist, const u64* ks, int nk, int* b_out, u64* k_out, unsigned int* c_out) {
  __shared__ unsigned int hist[SEL_BINS];
  __shared__ u64 sc[NT/64 + 3];
  for (int i = threadIdx.x; i < SEL_BINS; i += NT) hist[i] = ghist[i];
  __syncthreads();
  for (int i = 0; i < nk; ++i) {
    int b; u64 kin; unsigned int inb;
    lds_find_bin<NT>(hist, ks[i], b, kin, inb, sc);
    if (threadIdx.x == 0) { b_out[i] = b; k_out[i] = kin; c_out[i] = inb; }
  }
}
// keyfn as k_select_small's slot mode has it: entries whose `live` byte is 0 are rejected
template <int NT> __global__ void __launch_bounds__(NT) k_lrs(int m, const double* x, const unsigned char* live, u64 k, int pass0, u64 prefix0, u64* out) {
  __shared__ unsigned int hist[SEL_BINS];
  __shared__ u64 sc[NT/64 + 3];
  __shared__ u64 st[2];
  for (int rep = 0; rep < 2; ++rep) {
    const u64 r = lds_radix_select<NT>(m, k, pass0, prefix0, [&](int i, u64& key) {
      if (!live[i]) return false;
      key = (u64)__double_as_longlong(fabs(x[i]));
      return true; }, hist, sc, st);
    if (threadIdx.x == 0) out[rep] = r;
  }
}

static u64 key_of(double v) { const double a = std::fabs(v); u64 b; std::memcpy(&b, &a, 8); return b; }
static int fails = 0, cases = 0;
static bool dev_ok(const char* where) {
  const hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) { printf("device error after %s: %s\n", where, hipGetErrorString(e)); return false; }
  return true;
}

// the populations: lognormal, sixty binades, all equal, zeros below the rank, a cluster 1 + j 2^-52 (distinct / equal in all 64 bits) of
// `cl` values around the middle, the middle on a boundary of a coarse bin / the 22-bit prefix / the last 9-bit digit (last key of one
// side or first key of the other), denormals
constexpr int NKIND = 14;
static std::vector<double> population(int kind, int n, int cl, std::mt19937_64& g) {
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  std::vector<double> x(n);
  const int rank = n/2;
  auto around = [&](auto mid) {            // `c` cluster values with the rank inside, small values below, large ones above
    const int c = std::min(cl, n), below = std::min(std::max(rank - c/2, 0), n - c);
    for (int i = 0; i < n; ++i) x[i] = i < below ? 1e-3 + 0.4*U(g) : (i < below + c ? mid(i - below) : 4.0 + 900.0*U(g));
  };
  auto boundary = [&](double hi, bool last) {
    const double lo = std::nextafter(hi, 0.0), ulp = hi - lo;
    const int nlo = last ? std::min(rank + 1, n) : rank;
    for (int i = 0; i < n; ++i) {
      const bool low = i < nlo; const int j = low ? i : i - nlo;
      if (j < 3) x[i] = low ? lo : hi;
      else if (j % 4 == 0) x[i] = low ? lo - ulp*(double)(g()%1000) : hi + ulp*(double)(g()%1000);
      else x[i] = low ? lo*(1.0 - 0.45*U(g)) : hi*(1.0 + 0.9*U(g));
    }
  };
  switch (kind) {
    case 0: for (auto& v : x) v = std::exp(2.0*N(g))*(U(g) < 0.1 ? -1.0 : 1.0); break;
    case 1: for (auto& v : x) v = std::exp2(60.0*U(g) - 30.0); break;
    case 2: for (auto& v : x) v = 1.2345; break;
    case 3: for (int i = 0; i < n; ++i) x[i] = i <= rank ? ((i & 1) ? -0.0 : 0.0) : std::exp(N(g)); break;
    case 4: around([&](int j) { return 1.0 + j*std::exp2(-52.0); }); break;
    case 5: around([&](int) { return 1.0 + std::exp2(-30.0); }); break;
    case 6: boundary(2.0, true); break;
    case 7: boundary(2.0, false); break;
    case 8: boundary(1.0 + std::exp2(-10.0), true); break;
    case 9: boundary(1.0 + std::exp2(-10.0), false); break;
    case 10: boundary(1.0 + 512*std::exp2(-52.0), true); break;
    case 11: boundary(1.0 + 512*std::exp2(-52.0), false); break;
    case 12: for (auto& v : x) { const u64 b = 1 + g()%((1ull << 52) - 1); std::memcpy(&v, &b, 8); } break;
    default: for (int i = 0; i < n; ++i) x[i] = i < rank ? 0.0 : (i == rank ? 1.0 : INFINITY); break;
  }
  std::shuffle(x.begin(), x.end(), g);
  return x;
}

int main() {
  std::mt19937_64 g(20261019);
  u64 *d_loc, *d_ks, *d_e, *d_out; int* d_t; unsigned int *d_uh, *d_c; double *d_hist, *d_x, *d_med; unsigned char* d_live; SelState* d_state;
  if (hipMalloc(&d_loc, 8*1024) || hipMalloc(&d_ks, 8*MAXK) || hipMalloc(&d_e, 8*MAXK) || hipMalloc(&d_out, 8*4) || hipMalloc(&d_t, 4*MAXK) ||
      hipMalloc(&d_uh, 4*SEL_BINS) || hipMalloc(&d_c, 4*MAXK) || hipMalloc(&d_hist, 8*SEL_PASSES*SEL_BINS) || hipMalloc(&d_x, 8*MAXN) ||
      hipMalloc(&d_med, 8) || hipMalloc(&d_live, MAXN) || hipMalloc(&d_state, sizeof(SelState)*(SEL_PASSES + 1)) != hipSuccess) { printf("no device memory\n"); return 2; }

  // ---- block_find_rank<256>, <1024>: k on every thread boundary, beyond the total, all mass in one thread, zero-count threads around the hit
  for (int NT : {256, 1024})
    for (int pat = 0; pat < 6; ++pat) {
      std::vector<u64> loc(NT, 0);
      for (int t = 0; t < NT; ++t)
        switch (pat) {
          case 0: loc[t] = 1; break;
          case 1: loc[t] = (g()%4 == 0) ? g()%6 : 0; break;
          case 2: loc[t] = t == 0 ? 70000 : 0; break;
          case 3: loc[t] = t == NT - 1 ? 70000 : 0; break;
          case 4: loc[t] = (t == 63 || t == 64 || t == 200 || t == NT - 2) ? 7 : 0; break;            // hits next to a wavefront seam, zeros all round
          default: loc[t] = 1ull + g()%(1ull << 40); break;                                          // counts beyond 32 bits
        }
      u64 total = 0; std::vector<u64> excl(NT), ks;
      for (int t = 0; t < NT; ++t) { excl[t] = total; total += loc[t]; }
      for (int t = 0; t < NT; ++t) if (loc[t]) { ks.push_back(excl[t]); ks.push_back(excl[t] + loc[t] - 1); }
      ks.push_back(total); ks.push_back(total + 5); ks.push_back(~0ull);
      if (total == 0) continue;
      const int nk = (int)ks.size();
      (void)hipMemcpy(d_loc, loc.data(), 8*NT, hipMemcpyHostToDevice); (void)hipMemcpy(d_ks, ks.data(), 8*nk, hipMemcpyHostToDevice);
      if (NT == 256) hipLaunchKernelGGL(k_bfr<256>, dim3(1), dim3(256), 0, 0, d_loc, d_ks, nk, d_t, d_e);
      else hipLaunchKernelGGL(k_bfr<1024>, dim3(1), dim3(1024), 0, 0, d_loc, d_ks, nk, d_t, d_e);
      if (!dev_ok("block_find_rank")) return 2;
      std::vector<int> tt(nk); std::vector<u64> ee(nk);
      (void)hipMemcpy(tt.data(), d_t, 4*nk, hipMemcpyDeviceToHost); (void)hipMemcpy(ee.data(), d_e, 8*nk, hipMemcpyDeviceToHost);
      for (int i = 0; i < nk; ++i) {
        int want = NT - 1;                                     // k >= total: clamped to the last thread
        if (ks[i] < total) for (int t = 0; t < NT; ++t) if (excl[t] <= ks[i] && ks[i] < excl[t] + loc[t]) { want = t; break; }
        ++cases;
        if (tt[i] != want || ee[i] != excl[want]) { ++fails; printf("block_find_rank<%d> pattern %d k %llu: thread %d excl %llu, want %d %llu\n", NT, pat, ks[i], tt[i], ee[i], want, excl[want]); }
      }
    }

  // ---- sel_find_bin (2048 and 512 bins of doubles), lds_find_bin<256>, <1024> (2048 bins in LDS): the same shapes
  for (int pat = 0; pat < 6; ++pat)
    for (int nbins : {SEL_BINS, 512}) {
      std::vector<unsigned int> h(SEL_BINS, 0);
      for (int b = 0; b < nbins; ++b)
        switch (pat) {
          case 0: h[b] = 1; break;
          case 1: h[b] = (g()%5 == 0) ? (unsigned int)(g()%40) : 0; break;
          case 2: h[b] = b == 0 ? 70000 : 0; break;
          case 3: h[b] = b == nbins - 1 ? 70000 : 0; break;
          case 4: h[b] = (b == 7 || b == 8 || b == 15 || b == 16 || b == 511 || b == nbins - 2) ? 3 : 0; break;      // around the seams of a thread's span (8 and 2 bins)
          default: h[b] = (unsigned int)(g()%1000); break;
        }
      u64 total = 0; std::vector<u64> excl(nbins), ks;
      for (int b = 0; b < nbins; ++b) { excl[b] = total; total += h[b]; }
      for (int b = 0; b < nbins; ++b) if (h[b]) { ks.push_back(excl[b]); ks.push_back(excl[b] + h[b] - 1); }
      if (ks.empty()) continue;
      if ((int)ks.size() > MAXK) ks.resize(MAXK);
      const int nk = (int)ks.size();
      std::vector<double> hd(SEL_BINS); for (int b = 0; b < SEL_BINS; ++b) hd[b] = (double)h[b];
      (void)hipMemcpy(d_hist, hd.data(), 8*SEL_BINS, hipMemcpyHostToDevice); (void)hipMemcpy(d_uh, h.data(), 4*SEL_BINS, hipMemcpyHostToDevice);
      (void)hipMemcpy(d_ks, ks.data(), 8*nk, hipMemcpyHostToDevice);
      for (int which = 0; which < 3; ++which) {
        if (which > 0 && nbins != SEL_BINS) continue;          // (the LDS histogram always has SEL_BINS counters)
        if (which == 0) hipLaunchKernelGGL(k_sfb, dim3(1), dim3(SEL_BLOCK), 0, 0, d_hist, nbins, d_ks, nk, d_t, d_e);
        else if (which == 1) hipLaunchKernelGGL(k_lfb<256>, dim3(1), dim3(256), 0, 0, d_uh, d_ks, nk, d_t, d_e, d_c);
        else hipLaunchKernelGGL(k_lfb<1024>, dim3(1), dim3(1024), 0, 0, d_uh, d_ks, nk, d_t, d_e, d_c);
        if (!dev_ok("find_bin")) return 2;
        std::vector<int> bb(nk); std::vector<u64> kk(nk); std::vector<unsigned int> cc(nk);
        (void)hipMemcpy(bb.data(), d_t, 4*nk, hipMemcpyDeviceToHost); (void)hipMemcpy(kk.data(), d_e, 8*nk, hipMemcpyDeviceToHost);
        if (which) (void)hipMemcpy(cc.data(), d_c, 4*nk, hipMemcpyDeviceToHost);
        for (int i = 0; i < nk; ++i) {
          int want = 0; while (!(excl[want] <= ks[i] && ks[i] < excl[want] + h[want])) ++want;
          ++cases;
          if (bb[i] != want || kk[i] != ks[i] - excl[want] || (which && cc[i] != h[want])) {
            ++fails; printf("%s pattern %d bins %d k %llu: bin %d rank %llu count %u, want %d %llu %u\n", which == 0 ? "sel_find_bin" : (which == 1 ? "lds_find_bin<256>" : "lds_find_bin<1024>"),
                            pat, nbins, ks[i], bb[i], kk[i], which ? cc[i] : h[want], want, ks[i] - excl[want], h[want]);
          }
        }
      }
    }

  // ---- lds_radix_select<256>, <1024> from pass0 = 0, 1, 2 (the bits above fixed to the answer's), m = 1, 2, 65, 4097 and 70000, with and
  //      without rejected entries, clusters of 64 / 65 / m values
  for (int m : {1, 2, 65, 4097, MAXN})
    for (int kind = 0; kind < NKIND; ++kind)
      for (int cl : {65, 4097})
        for (int gaps = 0; gaps < 2; ++gaps) {
          if (cl != 65 && kind != 4 && kind != 5) continue;
          if (m == MAXN && (kind % 3 != 1 || gaps)) continue;           // (the long one: a few kinds only)
          const std::vector<double> x = population(kind, m, cl, g);
          std::vector<unsigned char> live(m, 1);
          if (gaps) for (int i = 0; i < m; ++i) if (g()%5 == 0) live[i] = 0;
          std::vector<u64> all;
          for (int i = 0; i < m; ++i) if (live[i]) all.push_back(key_of(x[i]));
          if (all.empty()) continue;
          std::sort(all.begin(), all.end());
          (void)hipMemcpy(d_x, x.data(), 8*(size_t)m, hipMemcpyHostToDevice); (void)hipMemcpy(d_live, live.data(), m, hipMemcpyHostToDevice);
          for (int pass0 = 0; pass0 < 3; ++pass0)
            for (int sel = 0; sel < 3; ++sel) {
              const u64 target = all[sel == 0 ? all.size()/2 : (sel == 1 ? 0 : all.size() - 1)];
              const u64 himask = pass0 == 0 ? 0ull : (~0ull << sel_shift(pass0 - 1)), prefix0 = target & himask;
              std::vector<u64> in; for (u64 k : all) if ((k & himask) == prefix0) in.push_back(k);
              for (u64 k : {(u64)(in.size()/2), (u64)0, (u64)in.size() - 1}) {
                for (int NT : {256, 1024}) {
                  if (NT == 256) hipLaunchKernelGGL(k_lrs<256>, dim3(1), dim3(256), 0, 0, m, d_x, d_live, k, pass0, prefix0, d_out);
                  else hipLaunchKernelGGL(k_lrs<1024>, dim3(1), dim3(1024), 0, 0, m, d_x, d_live, k, pass0, prefix0, d_out);
                  if (!dev_ok("lds_radix_select")) return 2;
                  u64 out[2]; (void)hipMemcpy(out, d_out, 16, hipMemcpyDeviceToHost);
                  ++cases;
                  if (out[0] != in[k] || out[1] != in[k]) { ++fails; printf("lds_radix_select<%d> m %d kind %d cluster %d gaps %d pass0 %d k %llu of %zu: got %016llx %016llx want %016llx\n", NT, m, kind, cl, gaps, pass0, k, in.size(), out[0], out[1], in[k]); }
                }
                if (in.size() == 1) break;
              }
            }
        }

  // ---- the full chain: k_select_pass x 6 + k_select_final on grids of 1, 2 and 1024 workgroups, n = 1, 257, 70000
  for (int n : {1, 257, MAXN})
    for (int kind = 0; kind < NKIND; ++kind)
      for (int cl : {65, 4097, 65537}) {
        if (cl != 65 && (kind != 4 && kind != 5)) continue;
        if (cl > n && cl != 65) continue;
        const std::vector<double> x = population(kind, n, cl, g);
        std::vector<u64> all(n); for (int i = 0; i < n; ++i) all[i] = key_of(x[i]);
        std::sort(all.begin(), all.end());
        (void)hipMemcpy(d_x, x.data(), 8*(size_t)n, hipMemcpyHostToDevice);
        for (int grid : {1, 2, 1024})
          for (u64 k : {(u64)(n/2), (u64)0, (u64)(n - 1)}) {
            (void)hipMemset(d_hist, 0, 8*SEL_PASSES*SEL_BINS);
            for (int p = 0; p < SEL_PASSES; ++p) hipLaunchKernelGGL(k_select_pass, dim3(grid), dim3(SEL_BLOCK), 0, 0, p, n, (const double*)d_x, d_hist, d_state, k);
            hipLaunchKernelGGL(k_select_final, dim3(1), dim3(SEL_BLOCK), 0, 0, (const double*)d_hist, (const SelState*)d_state, d_med);
            if (!dev_ok("k_select_pass x 6 + k_select_final")) return 2;
            double md; (void)hipMemcpy(&md, d_med, 8, hipMemcpyDeviceToHost);
            u64 got; std::memcpy(&got, &md, 8);
            ++cases;
            if (got != all[k]) { ++fails; printf("six-pass chain n %d kind %d cluster %d grid %d k %llu: got %016llx want %016llx\n", n, kind, cl, grid, k, got, all[k]); }
            if (n == 1) break;
          }
      }

  if (!dev_ok("the end")) return 2;
  if (!fails) printf("ok %d\n", cases); else printf("FAILED: %d of %d\n", fails, cases);
  return fails ? 1 : 0;
}
