// Every reader of mcptam_amd/csrc/mcp_knobs.h against a literal table: what the library made of each MCP_* variable when the
// reads were still written out where they were used -- `e ? atoi(e) != 0 : dflt`, `if (e) x = atoi(e)`, getenv(...) != nullptr
// and their clamps.  Host only, its own main; built with the sanitizers by tests/test_knobs_cpu.py.
//
// Each knob is probed unset and set to "", "0", "1", "2", "-3", "abc" (atoi and atof make 0 of "" and "abc"), then at the
// boundaries of its clamp or oddity.  A probe reduces a reader to one number; the table holds the seven numbers expected.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "mcp_knobs.h"

namespace k = mcp::knobs;

static int g_bad = 0, g_checks = 0;
static const char* const VALUES[7] = {nullptr, "", "0", "1", "2", "-3", "abc"};

static void put(const char* name, const char* v) { if (v) setenv(name, v, 1); else unsetenv(name); }
static void expect(const char* name, const char* v, double got, double want) {
  ++g_checks;
  if (got == want) return;
  ++g_bad;
  std::fprintf(stderr, "%s=%s: got %.17g, expected %.17g\n", name, v ? (*v ? v : "\"\"") : "(unset)", got, want);
}
// the probe at one value (and the variable unset again behind it)
static void at(const char* name, const char* v, const std::function<double()>& probe, double want) {
  put(name, v); expect(name, v, probe(), want); unsetenv(name);
}

struct Row { const char* name; std::function<double()> probe; double want[7]; };

// the seven expected numbers of the plain idioms
#define FLAG_T {1, 0, 0, 1, 1, 1, 0}          /* e ? atoi(e) != 0 : true, also written !(e && atoi(e) == 0) */
#define FLAG_F {0, 0, 0, 1, 1, 1, 0}          /* e ? atoi(e) != 0 : false */
#define PRESENT {0, 1, 1, 1, 1, 1, 1}         /* getenv(name) != nullptr: "0" and "" count as set */
#define INT_OR(d) {d, 0, 0, 1, 2, -3, 0}      /* e ? atoi(e) : d, also written if (e) x = atoi(e) over x = d */
#define CLAMP1(d) {d, 1, 1, 1, 2, 1, 1}       /* e ? max(1, atoi(e)) : d */

template <class F> static std::function<double()> handle(F f) { return [f] { k::HandleKnobs h; return (double)f(h); }; }
template <class F> static std::function<double()> build(F f) { return [f] { k::PrepareKnobs p; p.read_build(); return (double)f(p); }; }
template <class F> static std::function<double()> chains(F f) { return [f] { k::PrepareKnobs p; p.read_chains(); return (double)f(p); }; }
template <class F> static std::function<double()> call(F f) { return [f] { k::PrepareKnobs p; p.read_call(); return (double)f(p); }; }
template <class F> static std::function<double()> pool(F f) { return [f] { k::DevCacheKnobs d; return (double)f(d); }; }
template <class F> static std::function<double()> persist(F f) { return [f] { k::CholPersistKnobs c; return (double)f(c); }; }

int main() {
  const std::vector<Row> rows = {
    // ---- the handle's knobs: the field initialisers of the handle and the block in mcp_ba_create
    {"MCP_BA_POINT_ORDER", handle([](const k::HandleKnobs& h) { return h.point_order_refine; }), FLAG_T},
    {"MCP_BA_GROUP_LMAX13", handle([](const k::HandleKnobs& h) { return h.group_lmax13; }), FLAG_T},
    {"MCP_BA_SCHUR4", handle([](const k::HandleKnobs& h) { return h.sch4_on; }), FLAG_T},
    {"MCP_BA_LIN_PIPE", handle([](const k::HandleKnobs& h) { return h.lin_pipe; }), FLAG_T},
    {"MCP_BA_STREAM_POOL", handle([](const k::HandleKnobs& h) { return h.stream_pool; }), FLAG_T},
    {"MCP_BA_OVERLAP", handle([](const k::HandleKnobs& h) { return h.overlap_spec; }), INT_OR(1)},
    {"MCP_BA_OVERLAP", handle([](const k::HandleKnobs& h) { return h.overlap_auto; }), {1, 0, 0, 0, 0, 0, 0}},      // being set clears overlap_auto
    {"MCP_BA_MAILBOX", handle([](const k::HandleKnobs& h) { return h.use_mailbox; }), INT_OR(1)},
    {"MCP_BA_MAIN_SYS", handle([](const k::HandleKnobs& h) { return h.main_sys; }), INT_OR(1)},
    {"MCP_BA_EVT", handle([](const k::HandleKnobs& h) { return h.evt_debug; }), INT_OR(0)},
    {"MCP_BA_SPEC_TRIALS", handle([](const k::HandleKnobs& h) { return h.spec_trials; }), INT_OR(2)},
    {"MCP_BA_HEAD_AHEAD", handle([](const k::HandleKnobs& h) { return h.large_head_ahead; }), INT_OR(0)},
    {"MCP_BA_NEAR_MISS", handle([](const k::HandleKnobs& h) { return h.near_miss_on; }), INT_OR(1)},
    {"MCP_BA_FORCE_MULTI", handle([](const k::HandleKnobs& h) { return h.force_multi; }), INT_OR(0)},
    {"MCP_BA_TEST_FAIL_TRIAL", handle([](const k::HandleKnobs& h) { return h.test_fail_trial; }), INT_OR(0)},
    {"MCP_BA_SPEC_DELAY", handle([](const k::HandleKnobs& h) { return h.spec_delay; }), INT_OR(0)},
    {"MCP_BA_SMALL", handle([](const k::HandleKnobs& h) { return h.small_on; }), INT_OR(1)},
    {"MCP_BA_SELECT_RIDE", handle([](const k::HandleKnobs& h) { return h.sel_ride; }), INT_OR(1)},
    {"MCP_BA_TIMEOUT_MS", handle([](const k::HandleKnobs& h) { return h.timeout_ms; }), {60000, 60000, 60000, 1, 2, 60000, 60000}},      // values <= 0 are ignored
    // ---- Prepare(): what the builders, the structure key and the launch choices read
    {"MCP_BA_PREPARE_LEGACY", build([](const k::PrepareKnobs& p) { return p.legacy; }), PRESENT},
    {"MCP_BA_ASM_LONG", build([](const k::PrepareKnobs& p) { return p.asm_long.set ? 1 + (p.asm_long.v != 0) : 0; }), {0, 1, 1, 2, 2, 2, 1}},      // unset, 0, non-zero
    {"MCP_BA_ASM_PAIR", build([](const k::PrepareKnobs& p) { return p.asm_pair; }), FLAG_T},
    {"MCP_BA_SCHUR4_ORDER", build([](const k::PrepareKnobs& p) { return p.schur4_order; }), FLAG_T},
    {"MCP_BA_SMALL_POINTS", build([](const k::PrepareKnobs& p) { return p.small_points; }), INT_OR(16384)},
    {"MCP_BA_TEST_CHOL_CUT", build([](const k::PrepareKnobs& p) { return p.chol_cut.set ? 1000 + p.chol_cut.v : 0; }), {0, 1000, 1000, 1001, 1002, 997, 1000}},
    {"MCP_BA_TEST_CHOL_ATOMIC", build([](const k::PrepareKnobs& p) { return p.chol_atomic; }), PRESENT},
    {"MCP_BA_CHOL_CHAINS", chains([](const k::PrepareKnobs& p) { return p.dissect_on; }), {1, 1, 1, 0, 1, 1, 1}},      // on unless exactly 1
    {"MCP_BA_CHOL_ARCS", chains([](const k::PrepareKnobs& p) { return p.chain_arcs; }), INT_OR(6)},
    {"MCP_BA_SPECULATE", call([](const k::PrepareKnobs& p) { return p.speculate; }), INT_OR(3)},
    {"MCP_BA_SPECULATE_ADAPT", call([](const k::PrepareKnobs& p) { return p.spec_adapt; }), INT_OR(1)},
    {"MCP_BA_LIN_JOIN", call([](const k::PrepareKnobs& p) { return p.lin_join_full; }), INT_OR(0)},
    {"MCP_BA_TRIAL_FUSE", call([](const k::PrepareKnobs& p) { return p.trial_fuse; }), INT_OR(1)},
    {"MCP_BA_HEAD_LARGE", call([](const k::PrepareKnobs& p) { return p.head_large_on; }), INT_OR(0)},
    {"MCP_BA_GRAPH", call([](const k::PrepareKnobs& p) { return p.use_graph; }), INT_OR(0)},
    {"MCP_BA_SELECT_CAP", call([](const k::PrepareKnobs& p) { return p.sel_cap; }), CLAMP1(4096)},
    // ---- read where they are used, or once per process / device at that place
    {"MCP_BA_TRACE", [] { return k::trace_level() >= 1; }, PRESENT},                          // the laps of Prepare(): "0" still counts as set
    {"MCP_BA_TRACE", [] { return k::trace_level() >= 2; }, {0, 0, 0, 0, 1, 0, 0}},
    {"MCP_BA_TRACE", [] { return k::trace_level() >= 3; }, {0, 0, 0, 0, 0, 0, 0}},
    {"MCP_BA_HOST_THREADS", [] { return k::host_threads(8); }, {8, 1, 1, 1, 2, 1, 1}},          // default 16, clamped to 1 .. usable cores
    {"MCP_BA_HOST_NUMA", [] { return k::host_numa(); }, FLAG_T},
    {"MCP_BA_PREP_PAR_MIN", [] { return k::prep_par_min(); }, INT_OR(32768)},
    {"MCP_BA_PREP_CHUNKS", [] { return k::prep_chunks(); }, CLAMP1(8)},
    {"MCP_BA_SELECT_GRID", [] { return k::select_grid(); }, CLAMP1(1024)},
    {"MCP_BA_STREAM_CALIBRATE", [] { return k::stream_calibrate(); }, FLAG_T},
    {"MCP_BA_SPEC_CUS", [] { return k::spec_cus(); }, INT_OR(0)},
    {"MCP_BA_STRUCT_CACHE_MB", [] { return (double)(k::struct_cache_bytes() >> 20); }, {512, 0, 0, 1, 2, 0, 0}},      // clamps at 0
    {"MCP_BA_STRUCT_CACHE", [] { return (double)(k::struct_cache_bytes() >> 20); }, {512, 0, 0, 512, 512, 512, 0}},
    {"MCP_DEV_CACHE_POISON", pool([](const k::DevCacheKnobs& d) { return d.poison; }), FLAG_F},
    {"MCP_DEV_CACHE_POISON_CLASS", pool([](const k::DevCacheKnobs& d) { return d.poison_cls; }), INT_OR(-1)},
    {"MCP_DEV_CACHE_POISON_NTH", pool([](const k::DevCacheKnobs& d) { return d.poison_nth; }), INT_OR(0)},
    {"MCP_DEV_CACHE_LOG", pool([](const k::DevCacheKnobs& d) { return d.log; }), FLAG_F},
    {"MCP_DEV_CACHE_MB", pool([](const k::DevCacheKnobs& d) { return d.enabled; }), {1, 0, 0, 1, 1, 0, 0}},           // <= 0 disables the cache
    {"MCP_DEV_CACHE_MB", pool([](const k::DevCacheKnobs& d) { return d.enabled ? (double)(d.budget >> 20) : -1.0; }), {2048, -1, -1, 1, 2, -1, -1}},
    {"MCP_BA_LIN_QUAD", [] { return k::lin_quad(); }, FLAG_T},
    {"MCP_BA_TEST_REFUSE_LAUNCH", [] { return k::test_refuse_launch(); }, PRESENT},
    {"MCP_BA_DEBUG_POISON_RED", [] { int q = 0; long lo = 0, hi = 0; return k::debug_poison_red(&q, &lo, &hi); }, {0, 0, 0, 0, 0, 0, 0}},      // not "q,lo,hi"
    {"MCP_CHOL_TEST_BAND", [] { int bw = 50; return k::chol_test_band(&bw) ? (double)bw : 50.5; }, {50.5, 0, 0, 1, 2, -3, 0}},
    {"MCP_BA_CHOL_PERSIST", [] { return k::chol_persist(); }, FLAG_T},
    {"MCP_BA_CHOL_FUSE1", [] { return k::chol_fuse1(); }, FLAG_T},
    {"MCP_BA_CHOL_CAPACITY", [] { return k::chol_capacity(77); }, INT_OR(77)},
    {"MCP_BA_CHOL_DEADLINE_MS", [] { return k::chol_deadline_ms(); }, {20, 0.01, 0.01, 1, 2, 0.01, 0.01}},            // clamps to >= 0.01
    {"MCP_BA_CHOL_WORKERS", persist([](const k::CholPersistKnobs& c) { return c.workers; }), {0, 0, 0, 1, 2, 0, 0}},  // counts only when > 0 ...
    {"MCP_BA_CHOL_WORKERS", persist([](const k::CholPersistKnobs& c) { return c.spread; }), {1, 0, 0, 0, 0, 0, 0}},   // ... its mere presence switches SPREAD off
    {"MCP_BA_CHOL_SPREAD", persist([](const k::CholPersistKnobs& c) { return c.spread; }), FLAG_T},
    {"MCP_BA_CHOL_BACK_CHAINS", persist([](const k::CholPersistKnobs& c) { return c.back_chains; }), FLAG_T},
    {"MCP_BA_TEST_PERSIST_FAIL", persist([](const k::CholPersistKnobs& c) { return c.test_fail_launch; }), INT_OR(-1)},
    {"MCP_IMG_ROW_TABLES", [] { return k::img_row_tables(); }, FLAG_T},
    {"MCP_TRACK_REFINE_REGS", [] { return k::track_refine_regs(); }, INT_OR(1)},               // (both sites: the value as a truth value)
    {"MCP_TRACK_REFINE_MULTI", [] { return k::track_refine_multi(); }, INT_OR(1)},
    {"MCP_TRACK_REFINE_PPW", [] { return k::track_refine_ppw(); }, {512, 512, 512, 1, 2, 512, 512}},                  // <= 0 means 512
    {"MCP_TRACK_REFINE_GATHER", [] { return k::track_refine_gather(); }, FLAG_F},
    {"MCP_TRACK_TEST_PRM_GIVEUP", [] { return k::track_test_prm_giveup(); }, PRESENT},
  };
  for (const Row& r : rows) unsetenv(r.name);
  for (const Row& r : rows) for (int i = 0; i < 7; ++i) at(r.name, VALUES[i], r.probe, r.want[i]);

  // ---- boundaries of the clamps and oddities
  at("MCP_BA_TRACE", "3", [] { return k::trace_level() >= 3; }, 1);
  at("MCP_BA_TRACE", "3", [] { return k::trace_level() >= 2; }, 1);
  at("MCP_BA_TRACE", "7", [] { return k::trace_level() >= 3; }, 1);
  at("MCP_BA_TIMEOUT_MS", "0.5", handle([](const k::HandleKnobs& h) { return h.timeout_ms; }), 0.5);
  at("MCP_BA_TIMEOUT_MS", "1e3", handle([](const k::HandleKnobs& h) { return h.timeout_ms; }), 1000);
  at("MCP_BA_TIMEOUT_MS", "-0.5", handle([](const k::HandleKnobs& h) { return h.timeout_ms; }), 60000);
  at("MCP_BA_HOST_THREADS", nullptr, [] { return k::host_threads(64); }, 16);
  at("MCP_BA_HOST_THREADS", "100", [] { return k::host_threads(64); }, 64);
  at("MCP_BA_HOST_THREADS", "64", [] { return k::host_threads(64); }, 64);
  at("MCP_BA_HOST_THREADS", "4", [] { return k::host_threads(4); }, 4);
  at("MCP_BA_HOST_THREADS", "5", [] { return k::host_threads(1); }, 1);
  at("MCP_BA_CHOL_DEADLINE_MS", "0.01", [] { return k::chol_deadline_ms(); }, 0.01);
  at("MCP_BA_CHOL_DEADLINE_MS", "0.005", [] { return k::chol_deadline_ms(); }, 0.01);
  at("MCP_BA_CHOL_DEADLINE_MS", "0.5", [] { return k::chol_deadline_ms(); }, 0.5);
  at("MCP_BA_SELECT_CAP", "4097", call([](const k::PrepareKnobs& p) { return p.sel_cap; }), 4097);
  at("MCP_BA_STRUCT_CACHE_MB", "-1", [] { return (double)k::struct_cache_bytes(); }, 0);
  at("MCP_BA_STRUCT_CACHE_MB", "64", [] { return (double)(k::struct_cache_bytes() >> 20); }, 64);
  setenv("MCP_BA_STRUCT_CACHE", "0", 1);                     // ... overrides the budget
  at("MCP_BA_STRUCT_CACHE_MB", "64", [] { return (double)k::struct_cache_bytes(); }, 0);
  unsetenv("MCP_BA_STRUCT_CACHE");
  at("MCP_DEV_CACHE_MB", "-1", pool([](const k::DevCacheKnobs& d) { return d.enabled; }), 0);
  at("MCP_DEV_CACHE_MB", "4096", pool([](const k::DevCacheKnobs& d) { return (double)d.budget; }), 4096.0*1048576.0);
  at("MCP_TRACK_REFINE_PPW", "1024", [] { return k::track_refine_ppw(); }, 1024);
  setenv("MCP_BA_CHOL_WORKERS", "-3", 1);                    // WORKERS does not count, and still switches SPREAD=1 off
  at("MCP_BA_CHOL_SPREAD", "1", persist([](const k::CholPersistKnobs& c) { return c.spread || c.workers; }), 0);
  unsetenv("MCP_BA_CHOL_WORKERS");
  at("MCP_BA_CHOL_WORKERS", "126", persist([](const k::CholPersistKnobs& c) { return c.workers; }), 126);
  {
    int q = 0; long lo = 0, hi = 0;
    at("MCP_BA_DEBUG_POISON_RED", "1,2,3", [&] { return k::debug_poison_red(&q, &lo, &hi) ? 100.0*q + 10.0*lo + hi : -1.0; }, 123);
    at("MCP_BA_DEBUG_POISON_RED", "1,2", [&] { return (double)k::debug_poison_red(&q, &lo, &hi); }, 0);
    at("MCP_BA_DEBUG_POISON_RED", "-1,5,900000000000", [&] { return k::debug_poison_red(&q, &lo, &hi) && q == -1 && lo == 5 && hi == 900000000000L; }, 1);      // (the caller checks the ranges)
  }

  // ---- absent does not mean default: the LM driver's knobs keep what an earlier Prepare() of the handle read
  {
    k::PrepareKnobs p;
    setenv("MCP_BA_SPECULATE", "0", 1); setenv("MCP_BA_SELECT_CAP", "-5", 1); setenv("MCP_BA_GRAPH", "1", 1);
    p.read_call();
    unsetenv("MCP_BA_SPECULATE"); unsetenv("MCP_BA_SELECT_CAP"); unsetenv("MCP_BA_GRAPH");
    p.read_build(); p.read_chains(); p.read_call();
    expect("MCP_BA_SPECULATE", "(0, then unset)", p.speculate, 0);
    expect("MCP_BA_SELECT_CAP", "(-5, then unset)", p.sel_cap, 1);
    expect("MCP_BA_GRAPH", "(1, then unset)", p.use_graph, 1);
    expect("MCP_BA_TRIAL_FUSE", "(never set)", p.trial_fuse, 1);
  }
  // ---- the serial builder's Prepare() skips the two reads of the chains: read_build() alone leaves them alone
  {
    k::PrepareKnobs p;
    setenv("MCP_BA_CHOL_CHAINS", "1", 1); setenv("MCP_BA_CHOL_ARCS", "3", 1);
    p.read_build(); p.read_call();
    expect("MCP_BA_CHOL_CHAINS", "(1, not read)", p.dissect_on, 1);
    expect("MCP_BA_CHOL_ARCS", "(3, not read)", p.chain_arcs, 6);
    p.read_chains();
    expect("MCP_BA_CHOL_CHAINS", "1", p.dissect_on, 0);
    expect("MCP_BA_CHOL_ARCS", "3", p.chain_arcs, 3);
    unsetenv("MCP_BA_CHOL_CHAINS"); unsetenv("MCP_BA_CHOL_ARCS");
    p.read_build();                                           // ... and a Prepare() of the serial builder behind a threaded one
    expect("MCP_BA_CHOL_ARCS", "(kept)", p.chain_arcs, 3);
  }
  // ---- the flags word of the structure key, as cache_lookup put it together: grouping limit | 32 point order | 64 schur4 | 128 schur4
  // order | points per group << 8 | (ASM_LONG: 0 unset, 1 "0", 2 non-zero) << 16 | (arcs & 7) << 18 unless one chain, ^ (cut & 0xff) << 21
  {
    struct Case { const char* name; const char* value; int want; };
    const Case cases[] = {
      {nullptr, nullptr, 13 + 32 + 64 + 128 + (64 << 8) + (6 << 18)},
      {"MCP_BA_ASM_LONG", "0", 13 + 32 + 64 + 128 + (64 << 8) + (1 << 16) + (6 << 18)},
      {"MCP_BA_ASM_LONG", "5", 13 + 32 + 64 + 128 + (64 << 8) + (2 << 16) + (6 << 18)},
      {"MCP_BA_SCHUR4_ORDER", "0", 13 + 32 + 64 + (64 << 8) + (6 << 18)},
      {"MCP_BA_SCHUR4", "0", 13 + 32 + 128 + (64 << 8) + (6 << 18)},
      {"MCP_BA_POINT_ORDER", "0", 13 + 64 + 128 + (64 << 8) + (6 << 18)},
      {"MCP_BA_CHOL_CHAINS", "1", 13 + 32 + 64 + 128 + (64 << 8)},
      {"MCP_BA_CHOL_ARCS", "3", 13 + 32 + 64 + 128 + (64 << 8) + (3 << 18)},
      {"MCP_BA_CHOL_ARCS", "9", 13 + 32 + 64 + 128 + (64 << 8) + (1 << 18)},
      {"MCP_BA_TEST_CHOL_CUT", "2", 13 + 32 + 64 + 128 + (64 << 8) + (6 << 18) + (2 << 21)},
      {"MCP_BA_TEST_CHOL_CUT", "0", 13 + 32 + 64 + 128 + (64 << 8) + (6 << 18)},
      {"MCP_BA_ASM_PAIR", "0", 13 + 32 + 64 + 128 + (64 << 8) + (6 << 18)},      // (not a structure knob: the task table is built either way)
    };
    for (const Case& c : cases) {
      if (c.name) setenv(c.name, c.value, 1);
      k::HandleKnobs h; k::PrepareKnobs p; p.read_build(); p.read_chains();
      expect(c.name ? c.name : "(flags, nothing set)", c.value, p.structure_flags(h, 13, 64), c.want);
      if (c.name) unsetenv(c.name);
    }
    k::HandleKnobs h; k::PrepareKnobs p; p.read_build(); p.read_chains();
    expect("(flags, groups of 16 closed at 16 poses)", nullptr, p.structure_flags(h, 16, 16), 16 + 32 + 64 + 128 + (16 << 8) + (6 << 18));
  }
  if (g_bad) { std::fprintf(stderr, "%d of %d checks failed\n", g_bad, g_checks); return 1; }
  std::printf("knobs ok: %d checks\n", g_checks);
  return 0;
}
