// Unit check of tm_emit (mcptam_amd/csrc/track_map_kernels.h): the k smallest keys of a candidate set, ascending, by radix select and
// bitonic sort in chunks of TM_SORT -- with crafted keys, against std::sort on (key, index).
// Build: hipcc --offload-arch=gfx950 -O2 -ffp-contract=off -I mcptam_amd/csrc -I include tests/cpp/tm_select_check.hip -o tm_select_check ;
// prints "ok <cases>" or the failing cases.
//
// A case = a set of distinct candidate keys, a layout that places them among the entries (dead entries, entries outside [a, b)), a
// filter (has_lo, the excl window, Ks != K0) and k.  The expectation restates TmCand::in on the host, sorts the candidates as
// (key, index) pairs and takes the first k; compared are out[0..k), the returned key and 64 sentinel words after out[k).
//
// The digit passes: a population "depth d" shares its top d bits, so the passes at shift > 56 - d see one bucket.  Its crafted variants
// put three buckets (m1, m2, the rest) into the digit at shift 56 - d: k = m1 + m2 leaves through the exact-bucket exit at that digit,
// k = m1 + m2 - 1 finds one key more than needed there and goes on to the digits below.  At depth 56 the crafted digit is the last one
// and distinct keys have it to themselves, so every k < n passes seven digits whose bucket holds more than is needed and ends at
// shift == 0; "one more" is k = n - 1, "exact" is k = n (the bucket of the first pass holds exactly what is needed).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>
#include "track_map_kernels.h"
using namespace mcp;
typedef unsigned long long u64;

constexpr int NMAX = 16384, TAIL = 64;
constexpr int SENT = (int)0xEEEEEEEE;

__global__ void __launch_bounds__(TM_SEL_NT) k_emit(TmCand cd, int k, const u64* K0, const u64* Ks, const uint8_t* live, const mcp_pvs_entry* E, int* out, u64* last) {
  __shared__ TmSelLds S;
  const u64 r = tm_emit(cd, k, K0, Ks, live, E, out, S);
  if (threadIdx.x == 0) *last = r;
}

static std::mt19937_64 g(20240229);

// n distinct keys: `top` in the bits above `free_bits`, random below
static std::vector<u64> shared_top(int n, u64 top, int free_bits) {
  std::set<u64> s;
  const u64 mask = free_bits >= 64 ? ~0ull : ((1ull << free_bits) - 1ull);
  while ((int)s.size() < n) s.insert((top & ~mask) | (g() & mask));
  std::vector<u64> v(s.begin(), s.end());
  std::shuffle(v.begin(), v.end(), g);
  return v;
}

// depth d with the digit at shift 56 - d holding buckets of m1, m2 and rest keys (digits 0x11, 0x5a, 0xc3)
static std::vector<u64> crafted(int d, int m1, int m2, int rest) {
  const int shift = 56 - d;
  const u64 top = d ? (0xA5C3F00F5A3C0FF0ull & (~0ull << (64 - d))) : 0ull;
  std::vector<u64> v;
  const int m[3] = {m1, m2, rest}; const u64 dig[3] = {0x11, 0x5a, 0xc3};
  for (int q = 0; q < 3; ++q) {
    std::vector<u64> part = shared_top(m[q], top | (dig[q] << shift), shift);
    v.insert(v.end(), part.begin(), part.end());
  }
  std::shuffle(v.begin(), v.end(), g);
  return v;
}

struct Dev { u64 *K0, *Ks, *last; uint8_t* live; mcp_pvs_entry* E; int* out; };
static Dev D;
static std::vector<int> point;                      // E[i].point
static int cases = 0, bad = 0;
static bool dead_device = false;

struct Layout { const char* name; int a; bool thirds; int tail; };       // entries before a and after b are junk, every third entry dead
struct Filter { const char* name; bool has_lo, excl, two_keys; };

// one population under one layout and one filter, at every k of `ks` (values above the candidate count are dropped; count - 1 and count
// are added when `ends`)
static void run(const std::string& pop, const std::vector<u64>& keys, const Layout& L, const Filter& F, std::vector<int> ks, bool ends) {
  if (dead_device) return;
  const int nk = (int)keys.size();
  std::vector<u64> K0, Ks; std::vector<uint8_t> live;
  for (int i = 0; i < L.a; ++i) { K0.push_back(g() >> 8); live.push_back(1); }                 // small keys outside [a, b): tempting
  const int a = L.a;
  for (int j = 0; j < nk; ++j) {
    if (L.thirds && (K0.size() - a) % 3 == 2) { K0.push_back(g() >> 8); live.push_back(0); }
    K0.push_back(keys[j]); live.push_back(1);
  }
  const int b = (int)K0.size();
  for (int i = 0; i < L.tail; ++i) { K0.push_back(g() >> 8); live.push_back(1); }
  const int n = (int)K0.size();
  if (n > NMAX) { printf("harness: %s too long\n", pop.c_str()); ++bad; return; }
  Ks = K0;
  if (F.two_keys) {                                                       // select on other keys than the exclusion reads: a permutation of the population
    std::vector<u64> other = keys; std::shuffle(other.begin(), other.end(), g);
    for (int i = a, j = 0; i < b; ++i) if (live[i]) Ks[i] = other[j++]; else Ks[i] = g();
  }
  TmCand cd{a, b, 0, 0, false, 0ull, false, 0ull};
  auto sorted_of = [&](const std::vector<u64>& K, int lo_i, int hi_i) { std::vector<u64> s; for (int i = lo_i; i < hi_i; ++i) if (live[i]) s.push_back(K[i]); std::sort(s.begin(), s.end()); return s; };
  u64 next_kept = 0; bool want_next = false;
  if (F.excl) {
    cd.excl = true; cd.e2a = a + (b - a)/5; cd.e2b = a + (3*(b - a))/5;
    std::vector<u64> s = sorted_of(K0, cd.e2a, cd.e2b);
    if (s.size() < 3) { printf("harness: %s/%s/%s: window too small\n", pop.c_str(), L.name, F.name); ++bad; return; }
    cd.thr2 = s[s.size()/2]; next_kept = s[s.size()/2 + 1]; want_next = true;
  }
  if (F.has_lo) {
    std::vector<u64> s = sorted_of(Ks, a, b);
    cd.has_lo = true; cd.lo = s[s.size()/7];
  }
  // the expectation: TmCand::in restated
  std::vector<std::pair<u64, int>> cand;
  bool thr2_seen = false, lo_seen = false, next_in = false, next_below_lo = false;      // the bounds are keys of live entries they apply to
  for (int i = a; i < b; ++i) {
    if (!live[i]) continue;
    thr2_seen |= cd.excl && i >= cd.e2a && i < cd.e2b && K0[i] == cd.thr2;
    lo_seen |= cd.has_lo && Ks[i] == cd.lo;
    if (cd.excl && i >= cd.e2a && i < cd.e2b && K0[i] <= cd.thr2) continue;
    if (cd.has_lo && !(Ks[i] > cd.lo)) { next_below_lo |= F.excl && i >= cd.e2a && i < cd.e2b && K0[i] == next_kept; continue; }
    cand.push_back({Ks[i], i});
    if (F.excl && i >= cd.e2a && i < cd.e2b) next_in |= K0[i] == next_kept;
  }
  std::sort(cand.begin(), cand.end());
  for (size_t i = 1; i < cand.size(); ++i) if (cand[i].first == cand[i - 1].first) { printf("harness: %s: keys not distinct\n", pop.c_str()); ++bad; return; }
  // the filters do what they are named for, on the expectation alone
  if ((F.excl && !thr2_seen) || (F.has_lo && !lo_seen)) { printf("harness: %s/%s/%s: a bound is not a present key\n", pop.c_str(), L.name, F.name); ++bad; return; }
  if (want_next && !next_in && !next_below_lo) { printf("harness: %s/%s/%s: the key after thr2 is not a candidate\n", pop.c_str(), L.name, F.name); ++bad; return; }
  const int nc = (int)cand.size();
  if (ends) { ks.push_back(nc - 1); ks.push_back(nc); }
  std::sort(ks.begin(), ks.end()); ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
  bool uploaded = false;
  for (int k : ks) {
    if (k < 1 || k > nc) continue;
    if (!uploaded) {
      hipError_t e = hipMemcpy(D.K0, K0.data(), 8*(size_t)n, hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipMemcpy(D.Ks, Ks.data(), 8*(size_t)n, hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipMemcpy(D.live, live.data(), (size_t)n, hipMemcpyHostToDevice);
      if (e != hipSuccess) { printf("HIP error (upload): %s\n", hipGetErrorString(e)); dead_device = true; return; }
      uploaded = true;
    }
    (void)hipMemsetAsync(D.out, 0xEE, 4*(size_t)(k + TAIL), 0);
    hipLaunchKernelGGL(k_emit, dim3(1), dim3(TM_SEL_NT), 0, 0, cd, k, D.K0, D.Ks, D.live, D.E, D.out, D.last);
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { printf("HIP error in %s/%s/%s k %d: %s\n", pop.c_str(), L.name, F.name, k, hipGetErrorString(e)); dead_device = true; return; }
    std::vector<int> out(k + TAIL); u64 last = 0;
    (void)hipMemcpy(out.data(), D.out, 4*(size_t)(k + TAIL), hipMemcpyDeviceToHost);
    (void)hipMemcpy(&last, D.last, 8, hipMemcpyDeviceToHost);
    ++cases;
    int first_bad = -1;
    for (int r = 0; r < k && first_bad < 0; ++r) if (out[r] != point[cand[r].second]) first_bad = r;
    for (int r = k; r < k + TAIL && first_bad < 0; ++r) if (out[r] != SENT) first_bad = r;
    if (first_bad >= 0 || last != cand[k - 1].first) {
      ++bad;
      if (first_bad >= 0) printf("WRONG: %s/%s/%s k %d of %d: out[%d] = %d, want %d\n", pop.c_str(), L.name, F.name, k, nc, first_bad, out[first_bad],
                                 first_bad < k ? point[cand[first_bad].second] : SENT);
      else printf("WRONG: %s/%s/%s k %d of %d: last %016llx, want %016llx\n", pop.c_str(), L.name, F.name, k, nc, last, cand[k - 1].first);
    }
  }
}

int main() {
  if (hipMalloc(&D.K0, 8*NMAX) != hipSuccess || hipMalloc(&D.Ks, 8*NMAX) != hipSuccess || hipMalloc(&D.live, NMAX) != hipSuccess ||
      hipMalloc(&D.E, sizeof(mcp_pvs_entry)*NMAX) != hipSuccess || hipMalloc(&D.out, 4*(NMAX + TAIL)) != hipSuccess || hipMalloc(&D.last, 8) != hipSuccess) {
    printf("device error: allocation\n"); return 2;
  }
  // E[i].point: a permutation of the entries without a fixed point (7 i + 3 mod 2^14 is odd where i is even and the other way round)
  point.resize(NMAX);
  std::vector<mcp_pvs_entry> E(NMAX);
  std::memset(E.data(), 0, sizeof(mcp_pvs_entry)*NMAX);
  std::vector<char> seen(NMAX, 0);
  for (int i = 0; i < NMAX; ++i) {
    point[i] = (7*i + 3) % NMAX; E[i].point = point[i];
    if (point[i] == i || seen[point[i]]) { printf("harness: E is not a permutation without fixed points\n"); return 2; }
    seen[point[i]] = 1;
  }
  if (hipMemcpy(D.E, E.data(), sizeof(mcp_pvs_entry)*NMAX, hipMemcpyHostToDevice) != hipSuccess) { printf("device error: upload\n"); return 2; }

  const std::vector<int> KS = {1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097};
  const Layout layouts[] = {{"plain", 0, false, 0}, {"thirds", 0, true, 0}, {"window", 37, false, 91}, {"window_thirds", 1029, true, 5}};
  const Filter filters[] = {{"none", false, false, false}, {"has_lo", true, false, false}, {"excl", false, true, false},
                            {"excl_lo", true, true, false}, {"chop", false, true, true}, {"chop_lo", true, true, true}};
  const int N = 6007;                                                 // candidates of the large populations (b - a = 6007: no multiple of 1024)

  // every population, every layout, every filter, every k
  std::vector<std::pair<std::string, std::vector<u64>>> pops;
  pops.push_back({"uniform", shared_top(N, 0ull, 64)});
  for (int d = 8; d <= 56; d += 8) {
    const int n = d == 56 ? 200 : N;
    pops.push_back({"depth" + std::to_string(d), shared_top(n, 0x3C96A55A0FF0C369ull, 64 - d)});
  }
  { std::vector<u64> v; std::vector<int> tops(256); for (int i = 0; i < 256; ++i) tops[i] = i; std::shuffle(tops.begin(), tops.end(), g);
    for (int i = 0; i < 201; ++i) v.push_back(((u64)tops[i] << 56) | 0x00C3A55A0FF0963Cull);
    pops.push_back({"top_byte_only", v}); }
  { std::vector<u64> v = shared_top(997, 0ull, 64); v[5] = 0ull; v[500] = ~0ull;          // 0 and ~0 as real keys; 997 candidates: no power of two
    std::set<u64> s(v.begin(), v.end()); if (s.size() != v.size()) { printf("harness: zero_ones not distinct\n"); return 2; }
    pops.push_back({"zero_and_ones", v}); }
  for (const auto& p : pops)
    for (const Layout& L : layouts)
      for (const Filter& F : filters) run(p.first, p.second, L, F, KS, true);

  // the crafted digit: exact bucket and one more, at every depth and at the top digit (depth 0), plain and under the layouts; k above
  // TM_SORT as well (the digit is then met in the second or third chunk, under the has_lo the first chunks left)
  struct M { int m1, m2, rest; };
  const M wide[] = {{300, 500, 1200}, {2048, 1000, 1500}, {1, 1, 300}, {2500, 1597, 700}};
  const M narrow[] = {{100, 200, 150}, {256, 255, 30}, {1, 1, 100}, {63, 65, 256}};       // depth 48: 256 keys to a bucket at the most
  for (int d = 0; d <= 48; d += 8)
    for (const M& m : d == 48 ? narrow : wide) {
      const std::vector<u64> v = crafted(d, m.m1, m.m2, m.rest);
      const std::string nm = "crafted" + std::to_string(d) + "_" + std::to_string(m.m1) + "_" + std::to_string(m.m2);
      for (const Layout& L : layouts) run(nm, v, L, filters[0], {m.m1, m.m1 + 1, m.m1 + m.m2 - 1, m.m1 + m.m2, m.m1 + m.m2 + 1}, true);
    }
  { const std::vector<u64> v = shared_top(256, 0x3C96A55A0FF0C369ull, 8);                 // depth 56, all 256 last bytes
    for (const Layout& L : layouts) run("depth56_full", v, L, filters[0], {1, 2, 63, 64, 65, 128, 254}, true); }

  if (dead_device) { printf("FAILED: stopped at a HIP error after %d cases\n", cases); return 2; }
  if (hipDeviceSynchronize() != hipSuccess) { printf("device error\n"); return 2; }
  if (!bad) printf("ok %d\n", cases); else printf("FAILED: %d wrong of %d\n", bad, cases);
  return bad ? 1 : 0;
}
