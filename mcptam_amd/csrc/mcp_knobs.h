// mcp_knobs.h -- every MCP_* environment switch of the library: its name, default, parse and clamp, each exactly once.
//
// Host only (no HIP header: the host compiler takes this file alone, tests/cpp/knobs_check.cpp does).  The callers decide WHEN a
// knob is read -- INTEGRATION.md 7 lists the moment of every knob in its "read at" column, tests/test_knob_moments_gpu.py pins them:
//   process      the reader is called from the initialiser of a function-local static (or of a process-wide singleton)
//   device       ... from the first use of a device (cp_device(), solver_streams())
//   handle       a HandleKnobs is made, when mcp_ba_create makes the handle
//   Prepare      PrepareKnobs::read_build / read_chains / read_call, at every Prepare() of a handle
//   every call   the reader is called where the value is used
// A reader has no state of its own: called twice it reads the environment twice.  The knob structs read in their member initialisers.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace mcp {
namespace knobs {

// ---- the parse idioms (an unparsable or empty value is 0, as atoi / atof have it)
inline const char* text(const char* name) { return std::getenv(name); }
inline bool present(const char* name) { return text(name) != nullptr; }                                                  // set at all: "0" and "" count
inline bool flag(const char* name, bool dflt) { const char* e = text(name); return e ? std::atoi(e) != 0 : dflt; }
inline int int_or(const char* name, int dflt) { const char* e = text(name); return e ? std::atoi(e) : dflt; }           // (absent keeps `dflt`: x = int_or(name, x))
struct Opt { bool set; int v; };                                                                                         // present, and its number
inline Opt opt_int(const char* name) { const char* e = text(name); return Opt{e != nullptr, e ? std::atoi(e) : 0}; }
inline long long_or(const char* name, long dflt) { const char* e = text(name); return e ? std::atol(e) : dflt; }
inline double double_or(const char* name, double dflt) { const char* e = text(name); return e ? std::atof(e) : dflt; }

// ---- diagnostics
// MCP_BA_TRACE: 0 = absent; 1 = set (to anything, "0" included): the phases of Prepare() and the bulk entries on stderr; 2: also the
// phases at the end of Compute(); 3: also, per LM iteration, when each trial's result reached the host
inline int trace_level() { const char* e = text("MCP_BA_TRACE"); return e ? std::max(1, std::atoi(e)) : 0; }

// ---- the host side of Prepare() (process)
// worker threads of the structure build (default: up to 16 of the cores this process may use; measured on a 256-thread host, cold
// Prepare() of the metric map: see profiles/r06/README.md)
inline int host_threads(int usable_cores) { return std::min(std::max(int_or("MCP_BA_HOST_THREADS", 16), 1), usable_cores); }
inline bool host_numa() { return flag("MCP_BA_HOST_NUMA", true); }                       // 0: the workers stay unpinned (read when the pool is made)
inline int prep_par_min() { return int_or("MCP_BA_PREP_PAR_MIN", 32768); }              // measurements from which the structure is built on the worker pool
inline int prep_chunks() { return std::max(1, int_or("MCP_BA_PREP_CHUNKS", 8)); }      // chunks per worker thread of the slot phase

// ---- streams of a device (device, first use) and of a handle
inline bool stream_calibrate() { return flag("MCP_BA_STREAM_CALIBRATE", true); }
inline int spec_cus() { return int_or("MCP_BA_SPEC_CUS", 0); }                          // (experiment) the side streams on the first n compute units

// ---- structure cache (process): bytes it may hold; MCP_BA_STRUCT_CACHE=0 switches it off whatever the budget says
inline size_t struct_cache_bytes() { return flag("MCP_BA_STRUCT_CACHE", true) ? (size_t)std::max(0L, long_or("MCP_BA_STRUCT_CACHE_MB", 512)) << 20 : 0; }

// ---- process-wide cache of device blocks (ba_pool.h; process).  Test aids: MCP_DEV_CACHE_POISON=1 hands every block out filled with
// 0xFF -- NaNs, index -1 -- so that a read of something never written shows instead of passing on whatever the block held;
// _POISON_CLASS=c: only size class c, the others zero-filled (to find which buffer it is); _POISON_NTH=n: only the n-th block handed
// out; MCP_DEV_CACHE_LOG=1 lists the classes handed out
struct DevCacheKnobs {
  bool poison = flag("MCP_DEV_CACHE_POISON", false), log = flag("MCP_DEV_CACHE_LOG", false);
  int poison_cls = int_or("MCP_DEV_CACHE_POISON_CLASS", -1), poison_nth = int_or("MCP_DEV_CACHE_POISON_NTH", 0);
  long mb = long_or("MCP_DEV_CACHE_MB", 2048);      // per device; <= 0: no caching
  bool enabled = mb > 0; size_t budget = enabled ? (size_t)mb << 20 : 0;
};

// ---- kernels of the solver
inline bool lin_quad() { return flag("MCP_BA_LIN_QUAD", true); }                         // (process) 0: quarter-size groups through the one-lane-per-point kernel
inline bool test_refuse_launch() { return present("MCP_BA_TEST_REFUSE_LAUNCH"); }       // (every call) test hook: the linearisation asks for more LDS than a compute unit has
inline int select_grid() { return std::max(1, int_or("MCP_BA_SELECT_GRID", 1024)); }   // (process) workgroups at most of the median's histogram passes
// (every Prepare()) test aid, "q,lo,hi": doubles [lo, hi) of system q of the reduced-system buffer; false: absent or not three numbers
inline bool debug_poison_red(int* q, long* lo, long* hi) { const char* e = text("MCP_BA_DEBUG_POISON_RED"); return e && std::sscanf(e, "%d,%ld,%ld", q, lo, hi) == 3; }
// (builds with -DMCP_CHOL_PROF only) the dense-solve hook takes a banded + bordered tile pattern of that band width
inline bool chol_test_band(int* bw) { const char* e = text("MCP_CHOL_TEST_BAND"); if (e) *bw = std::atoi(e); return e != nullptr; }

// ---- factorisation of the reduced system (ba_chol.h, ba_chol2.h)
inline bool chol_persist() { return flag("MCP_BA_CHOL_PERSIST", true); }                // (Prepare: when the plan is built) the one-launch factorisation
inline bool chol_fuse1() { return flag("MCP_BA_CHOL_FUSE1", true); }                    // (handle: when a CholPlan is made) the single-tile system in one launch
// (device) test hook: pretend the device is a partition of that many workgroup slots; the wall-clock bound of every spin
inline int chol_capacity(int measured) { return int_or("MCP_BA_CHOL_CAPACITY", measured); }
inline double chol_deadline_ms() { const char* e = text("MCP_BA_CHOL_DEADLINE_MS"); return e ? std::max(0.01, std::atof(e)) : 20.0; }
// (Prepare: when the one-launch plan is built)
struct CholPersistKnobs {
  Opt workers_env = opt_int("MCP_BA_CHOL_WORKERS");
  int workers = std::max(0, workers_env.v);                                   // workers per system; 0 (absent, or a value <= 0): the plan's own count
  bool spread = flag("MCP_BA_CHOL_SPREAD", true) && !workers_env.set;          // a batch's workgroups spread over the device; the mere presence of WORKERS switches it off
  bool back_chains = flag("MCP_BA_CHOL_BACK_CHAINS", true);                   // the back-substitution on a workgroup per chain
  int test_fail_launch = int_or("MCP_BA_TEST_PERSIST_FAIL", -1);              // =k: the k-th one-launch factorisation times out; -1 = none
};

// ---- image and tracker side (img_api.hip)
inline bool img_row_tables() { return flag("MCP_IMG_ROW_TABLES", true); }               // (process) 0: k_row_count + k_row_compact, the round-5 pair
// the register-resident pose kernel: mcp_track_pose_refine reads it once per process, mcp_track_map at every call
inline int track_refine_regs() { return int_or("MCP_TRACK_REFINE_REGS", 1); }
// (every call) the iterations over several workgroups: 0 never, 1 whenever the points do not fit the register-resident kernel, 2 always
inline int track_refine_multi() { return int_or("MCP_TRACK_REFINE_MULTI", 1); }
// (every call) points per workgroup (measured at 8000 points: 128: 407 us, 256: 337, 512: 311, 1024: 322)
inline int track_refine_ppw() { const int v = int_or("MCP_TRACK_REFINE_PPW", 0); return v > 0 ? v : 512; }
inline bool track_refine_gather() { return flag("MCP_TRACK_REFINE_GATHER", false); }    // (every call) the median through every workgroup's LDS
inline bool track_test_prm_giveup() { return present("MCP_TRACK_TEST_PRM_GIVEUP"); }    // (every call) test hook: the multi-workgroup iterations give up

// ---- the knobs of a solver handle, read when one is made (mcp_ba_create makes it with the handle): name and default on the member's line
struct HandleKnobs {
  bool point_order_refine = flag("MCP_BA_POINT_ORDER", true);     // MCP_BA_POINT_ORDER: secondary point order (refine_point_order)
  bool group_lmax13 = flag("MCP_BA_GROUP_LMAX13", true); // MCP_BA_GROUP_LMAX13: groups are closed at 13 poses (what k_schur4 holds), 0: at 16
  // round 5 (ba_schur4.h): all systems of a batch in one Schur workgroup.  Groups are closed at S4_LMAX poses (a single point
  // that sees more keeps its group beyond that: then no group of the map takes the new kernel)
  bool sch4_on = flag("MCP_BA_SCHUR4", true); // MCP_BA_SCHUR4
  bool lin_pipe = flag("MCP_BA_LIN_PIPE", true); // MCP_BA_LIN_PIPE: k_linearize_pipe, 0: the plain loop (k_linearize_group)
  bool stream_pool = flag("MCP_BA_STREAM_POOL", true); // MCP_BA_STREAM_POOL=0: private streams per handle instead of the device's pool
  // MCP_BA_OVERLAP: 0 = one stream, 1 = the speculative systems together on a second stream, 2 = system 1 on the second and
  // systems 2.. on a third stream, so that the system the SECOND trial needs is ready as early as the first one's.  While the knob
  // is absent (overlap_auto) a one-rank handle with a one-launch factorisation keeps the batch on the main stream.
  Opt overlap_env = opt_int("MCP_BA_OVERLAP");
  int overlap_spec = overlap_env.set ? overlap_env.v : 1; bool overlap_auto = !overlap_env.set;
  int main_sys = int_or("MCP_BA_MAIN_SYS", 1); // MCP_BA_MAIN_SYS: systems of a split batch that stay on the main stream
  int use_mailbox = int_or("MCP_BA_MAILBOX", 1); // MCP_BA_MAILBOX=0: device-to-host copy + stream wait per trial
  int evt_debug = int_or("MCP_BA_EVT", 0); // MCP_BA_EVT=1: device time stamps (timing events) of the phases of every iteration on both streams, printed to stderr
  // MCP_BA_SPEC_TRIALS: 0 = trials strictly in sequence; 1 = one trial ahead on the stream that solved it; 2 (default since round 6)
  // = the steps of ALL speculatively solved systems are applied and evaluated as soon as their solutions exist, each on its own
  // stream (lane[q].st_tr, behind the speculative chain's event).  Round 3 measured 819 / 835 it/s (1) vs 733 / 743 (2) -- three trial
  // evaluations at once took the compute units from the trial the host was waiting for; with a trial's step in one launch and the
  // evaluation at 17 us the balance has turned: 1518 / 1519 / 1610 (1) vs 1543 / 1538 / 1629 (2), pairs within one run.
  int spec_trials = int_or("MCP_BA_SPEC_TRIALS", 2);
  // MCP_BA_HEAD_AHEAD, maps beyond the small-bundle limit (round 6; ba_head.h): EVERY trial of an iteration -- the one on
  // the main stream and the ones evaluated ahead on the second -- counts the digit histograms of its |chi2| while it evaluates them
  // and is followed by ONE kernel that finishes the median and writes the sigma block of the iteration its acceptance would start,
  // each trial into its own scratch and its own sigma / start block: slot [parity of the iteration][q].  The accepted trial's blocks
  // become the current ones (sig_idx, start_blk); the others are never looked at.
  // MEASURED (profiles/r06/README.md): with the heads on, a one-trial iteration reaches its linearisation 11 us after it starts (65 without)
  // and every iteration finds its sigma^2 ready -- but the two extra launches + events per trial on the host and the heads' kernels
  // beside the trials' cost more than that saves on the metric map: 1290-1335 it/s with them, 1335-1385 without, same box and run.
  // So the default is OFF; =1 switches every trial's head on, =2 only the main stream's.  Bit-identical either way.
  int large_head_ahead = int_or("MCP_BA_HEAD_AHEAD", 0);
  int near_miss_on = int_or("MCP_BA_NEAR_MISS", 1); // MCP_BA_NEAR_MISS=0: a map that lost measurements is built cold
  // MCP_BA_FORCE_MULTI=1: a one-rank communicator / hook is driven through the whole multi-rank machine (packed tiles, per-lane
  // collectives, riding histograms) -- sums over one rank are exact, so the result must equal the plain single-rank solve bit for
  // bit; the GPU suite uses it to run the two-lane RCCL path on the one device a test box has
  int force_multi = int_or("MCP_BA_FORCE_MULTI", 0);
  int test_fail_trial = int_or("MCP_BA_TEST_FAIL_TRIAL", 0); // MCP_BA_TEST_FAIL_TRIAL=k: the k-th trial of the handle's life is treated as a failed factorisation
  int spec_delay = int_or("MCP_BA_SPEC_DELAY", 0); // MCP_BA_SPEC_DELAY=1: the speculative systems' Schur complements start only when the trial's own is through
  int small_on = int_or("MCP_BA_SMALL", 1); // MCP_BA_SMALL=0: a small bundle runs the same launches as a large one (ba_small.h)
  int sel_ride = int_or("MCP_BA_SELECT_RIDE", 1); // MCP_BA_SELECT_RIDE=0: the median never uses the histograms that rode on the trial's all-reduce
  // every host-side wait of the solve is bounded (MCP_BA_TIMEOUT_MS, default 60 s; a value <= 0 is ignored): a rank that dies inside a
  // collective leaves the others waiting on a kernel that never ends, which must surface as MCP_ERR_RUNTIME with the place, not as a hang
  double timeout_env = double_or("MCP_BA_TIMEOUT_MS", 0.0), timeout_ms = timeout_env > 0 ? timeout_env : 60000.0;
};

// ---- the knobs of one Prepare() of a handle, three groups with three rules for an absent knob.  The block lives in the handle.
// (1) What the builders, the structure key and the launch choices of THIS Prepare() go by: read_build(), at the head of every
// Prepare(), makes the group anew -- absent = the default on the member's line; one read each, so that the three cannot disagree.
struct BuildKnobs {
  bool legacy = present("MCP_BA_PREPARE_LEGACY");           // (set to anything) the serial reference builder
  Opt asm_long = opt_int("MCP_BA_ASM_LONG");                // absent: chosen from the staged lists; 0 never, else k_assemble_long whenever there are pose pairs
  bool asm_pair = flag("MCP_BA_ASM_PAIR", true);            // 0: k_assemble_tiles where k_assemble would run
  bool schur4_order = flag("MCP_BA_SCHUR4_ORDER", true);    // 0: the groups of k_schur4 in index order, not heaviest first
  int small_points = int_or("MCP_BA_SMALL_POINTS", 16384);  // maps of at most that many points get quarter-size groups (0: the large-map layout for every map)
  Opt chol_cut = opt_int("MCP_BA_TEST_CHOL_CUT");           // =k (tests): the cut between the chains moved k tiles into the first one
  bool chol_atomic = present("MCP_BA_TEST_CHOL_ATOMIC");    // (tests, set to anything) the per-point observer sets taken with atomics
};
struct PrepareKnobs : BuildKnobs {
  void read_build() { static_cast<BuildKnobs&>(*this) = BuildKnobs(); }
  // (2) read_chains(), by the threaded builder only (a Prepare() of the serial one leaves them as they were): absent = the default
  int dissect_on = 1, chain_arcs = 6;
  void read_chains() {
    dissect_on = int_or("MCP_BA_CHOL_CHAINS", 0) != 1;      // on unless exactly 1 (= one chain, the poses in add order)
    chain_arcs = int_or("MCP_BA_CHOL_ARCS", 6);             // the cut has that many arcs at most (2 ... 6)
  }
  // (3) read_call(), the LM driver's knobs, read once the structure stands (a test sets them between two handles): absent = what the
  // handle had -- the default written here, or what an earlier Prepare() of the handle read
  int speculate = 3, spec_adapt = 1, lin_join_full = 0, trial_fuse = 1, head_large_on = 0, use_graph = 0, sel_cap = 4096;
  void read_call() {
    speculate = int_or("MCP_BA_SPECULATE", speculate);      // speculative systems per solve at most; 0 turns them off
    // Small bundles (ba_small.h) speculate only while trials are being rejected: a BundleAdjustRecent window accepts every first trial, and the
    // three systems solved beside it were 16 launches per iteration for nobody (compute 1.09 -> 1.01 ms without them).  A rejection arms the
    // speculation for the re-solve that follows and the next iterations; MCP_BA_SPECULATE_ADAPT=0: always, as large bundles do.
    spec_adapt = int_or("MCP_BA_SPECULATE_ADAPT", spec_adapt);
    lin_join_full = int_or("MCP_BA_LIN_JOIN", lin_join_full);      // 1: linearize() waits for everything the speculative stream has in flight (round 2's behaviour)
    trial_fuse = int_or("MCP_BA_TRIAL_FUSE", trial_fuse);          // 0: the step of a trial as separate kernels, not k_trial_apply with several chain workgroups
    // the head of an iteration of a large map in one launch (ba_headl.h, MCP_BA_HEAD_LARGE=1).  Default off:
    // measured equal to the six launches at the metric size (1611 / 1603 vs 1606 / 1611 it/s) -- 39 us alone on the device against ~50, but its 64
    // fat workgroups wait for room beside the trials evaluated ahead on the other stream, which six small launches slip past
    head_large_on = int_or("MCP_BA_HEAD_LARGE", head_large_on);
    use_graph = int_or("MCP_BA_GRAPH", use_graph);                 // 1: replay the factorisation chain from a captured hipGraph (a capture that fails clears it)
    sel_cap = std::max(1, int_or("MCP_BA_SELECT_CAP", sel_cap));   // candidates per rank slot of the multi-rank median's gather table
  }
  // The `flags` word of the structure cache's key: every switch that decides what Prepare() builds, beside the topology.  `grp_lmax`
  // and `grp_pts` are what the handle makes of group_lmax13 and small_points (the kernels' constants).  A NEW STRUCTURE KNOB GOES IN HERE.
  int structure_flags(const HandleKnobs& h, int grp_lmax, int grp_pts) const {
    int f = grp_lmax | (h.point_order_refine ? 32 : 0) | (h.sch4_on ? 64 : 0) | (schur4_order ? 128 : 0) | (grp_pts << 8) |
            ((asm_long.set ? 1 + (asm_long.v != 0) : 0) << 16) | (dissect_on ? (chain_arcs & 7) << 18 : 0);
    if (chol_cut.set) f ^= (unsigned)(chol_cut.v & 0xff) << 21;
    return f;
  }
};

}  // namespace knobs
}  // namespace mcp
