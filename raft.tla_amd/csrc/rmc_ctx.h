// rmc_ctx.h — the host-side context behind the C ABI: rmc_api.cpp (create, run,
// trace, expand, simulate), rmc_spill.cpp, rmc_ckpt.cpp, rmc_wide.cpp, rmc_dist.cpp,
// rmc_dist_comm.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rmc.h"
#include "rmc_codec.h"
#include "rmc_internal.h"
#include "rmc_plan.h"

// Sharded mode (rmc_shard): this ctx is one rank of a BFS whose fingerprint
// space is partitioned over `world` GPUs.  The exchange runs
// over RCCL (one communicator per ctx, on the ctx stream) or over a
// caller-supplied host transport (rmc_transport, e.g. gloo in tests).
struct DistState {
    int on = 0;
    int rank = 0, world = 1;
    int rccl = 0;                   // 1: RCCL communicator, 0: host transport
    ncclComm_t comm = nullptr;
    rmc_transport host{};
    hipStream_t xs = nullptr;       // exchange stream: every collective, owner insert, phase 2
    // Outbox sets, double-buffered: the expansion of round k + 1 (ctx stream)
    // fills one set while round k's exchange (xs) drains the other.
    struct Set {
        rmc::u64* key_out = nullptr;             // [world][kcap] 12-B keys per owner {k lo, k hi, s32}
        rmc::u64* tick_out = nullptr;            // [world][kcap] tickets (parent | lane << 56)
        unsigned long long* ocount = nullptr;    // [world] keys written per owner, [world]: pool records
        rmc::u32* pool = nullptr;                // remote-successor pool (phase-2 records, flush_pool)
        rmc::u64* cx = nullptr;                  // device count row: [2W + 1] sent, [2W] received
        rmc::u64* h_cx = nullptr;                // pinned copy of cx
        hipEvent_t ev_exp = nullptr;             // expansion (or drain) of this set's round done
        hipEvent_t ev_free = nullptr;            // the round's exchange no longer reads the set
        hipEvent_t k0 = nullptr, k1 = nullptr;   // expansion kernel time
        hipEvent_t x0 = nullptr, x1 = nullptr;   // exchange time (xs) of the round
        int timed = 0, xtimed = 0;
    } set[2];
    hipEvent_t ev_cnt = nullptr, ev_acc = nullptr, ev_c = nullptr, ev_x = nullptr;
    hipEvent_t ev_h = nullptr;      // host waits on xs (under the deadline)
    // single buffers (used on xs only, rounds in order)
    rmc::u64* key_in = nullptr;     // keys received (12-B {k, s32} records), blocks by source
    uint8_t* rep_out = nullptr;     // replies to the keys received (same layout)
    uint8_t* rep_in = nullptr;      // replies to the keys sent, [world][kcap]
    rmc::u32* st_in = nullptr;      // accepted states received, blocks by source
    unsigned long long* sa = nullptr;  // [2W]: states to send per owner (scount), states to receive per source
    rmc::u64* h_sa = nullptr;       // pinned copy of sa
    rmc::u64 in_cap = 0;            // keys / states receivable per round (all sources)
    void* ag_dev = nullptr;         // RCCL all-gathers of small rows: device staging,
    rmc::u64 ag_cap = 0;            // (world + 1) x ag_cap bytes, allocated once per shard
    std::vector<uint8_t> stage_send, stage_recv;  // host transport staging
    rmc::u64 sent_slots = 0;
    rmc::u64 pool_cap = 0;          // records per pool (one pool per outbox set)
    int debug = 0;                  // RMC_DIST_DEBUG: one stderr line per round
    int table_grown = 0;            // rmc_shard doubled the fingerprint set once (send markers)
    int split = 2;                  // RMC_DIST_SPLIT: rounds a large level is cut into at least (1 at world 1)
    int overlap = 1;                // RMC_DIST_OVERLAP=0: the next expansion waits for the exchange
    double fill = 0.5;              // RMC_DIST_FILL: expected fill of the fullest outbox a round aims at
                                    // (> 1 forces parking: a test hook)
    // replicated levels: a level of at most rep_max states in total is gathered
    // whole (k_pack_rep records) into rep_buf on every rank and expanded there
    rmc::u64 rep_max = 0;
    rmc::u32* rep_send = nullptr;   // this rank's records of the level
    rmc::u32* rep_buf = nullptr;    // every rank's, in rank order
    rmc::u64 rep_levels = 0;        // replicated levels of the last run
    // deadlines (RMC_DIST_TIMEOUT_S) and where the loop is, for error messages
    double timeout_s = 300.0;
    int nonblocking = 0;            // the RCCL communicator is non-blocking
    int aborted = 0;                // a deadline aborted the communicator: the ctx is unusable
    int abort_pending = 0;          // ... and the abort has not returned: device buffers are leaked, not freed
    int lvl = 0, rnd = 0;
    const char* phase = "";
    int stall_rank = -1, stall_level = 2;  // test hook (RMC_DIST_STALL_*)
    double stall_s = 0;
    // statistics of the last run
    rmc::u64 keys_sent = 0, states_sent = 0, chunks = 0, parked = 0;
    double xfer_seconds = 0;        // device time of the exchange rounds (xs), overlapped or not
    double wait_seconds = 0;        // host wall time blocked on count read-backs and level ends
};

// Frontier spill (RMC_FLAG_SPILL): the device holds the fingerprint set and
// the window of states [base, base + win) — the frontier being expanded and the
// level being built.  Below base only the trace links survive, in host memory:
// parent index + action lane per state (9 B, TLC's trace file), and a
// counterexample re-derives those states by replaying the lanes from Init.
// B.store / B.parent / B.act are biased by -base, so kernels keep indexing
// states by their global index.
struct SpillState {
    int on = 0;
    // device links (default when they fit): the trace links of every state stay in
    // HBM (9 B per state, B.parent / B.act indexed by global index, never rebased)
    // and a spill only shifts the window's states, footprints and classes — no
    // PCIe traffic; otherwise (RMC_SPILL_HOST_LINKS=1, or no room) they move to
    // the host as below
    int dev_links = 0;
    rmc::u64 base = 0;          // first device-resident global index
    rmc::u64 win = 0;           // device window (states)
    rmc::u64 total_cap = 0;     // all states (fingerprint-set sizing)
    rmc::u32* store = nullptr;  // the real device allocations
    rmc::u64* parent = nullptr;
    uint8_t* act = nullptr;
    rmc::u64* foot = nullptr;
    uint8_t* cls = nullptr;
    rmc::u64* h_parent = nullptr;  // host, [total_cap], reserved address space,
    uint8_t* h_act = nullptr;      // pages touched as levels spill
    size_t h_bytes = 0;
    rmc::u64 faulted = 0;          // links [0, faulted) have backed pages
    std::thread ahead;             // backs the next window's pages during expansion
    // verification + spill (RMC_FLAG_VERIFY_STATES): a host copy of every state that
    // leaves the device window ([0, hcopied) copied), against which the hits on
    // spilled owners are checked (B.hbuf, k_verify_host); reserved like the links
    rmc::u32* h_state = nullptr;
    size_t hs_bytes = 0;
    rmc::u64 hcopied = 0;
    rmc::u32* h_ostage = nullptr;  // pinned / device staging of the owners of one batch of hits
    rmc::u32* d_ostage = nullptr;
    rmc::u64 ostage_cap = 0;       // states per batch
    rmc::u64 host_hits = 0;        // hits checked against host copies in the last run
};

struct rmc_ctx {
    rmc_config cfg{};
    rmc::Shape sh{};
    const rmc::ShapeKernels* k = nullptr;  // the launchers of shape (sh.S, sh.K), resolved at create
    rmc::Params P{};
    rmc::PermTable PT{};
    int NW = 0;  // 32-bit words per packed state
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // bracket each level's expansion launches
    rmc::DevBufs B{};
    rmc::Counters* h_ctr = nullptr;  // pinned
    rmc::u32* d_staged = nullptr;
    rmc::u64 table_slots = 0;
    // the epoch the set's current entries carry (raft_packed.h c_set_ep): 0 = untagged
    // (cleared to 0 by the last run, or unknown), 1..255 = tagged; the next plain
    // single-GPU run takes the next epoch without clearing the set (rmc_run_bfs)
    rmc::u32 set_epoch = 0;
    rmc::u64 walked = 0;  // (state, lane) slots of the lane walk in the last run (RMC_WALK_STATS)
    // action coverage (RMC_FLAG_COVERAGE; rmc_cover.h): the device tallies, generated[COV_ROWS]
    // then distinct[COV_ROWS], allocated only with the flag (not part of Counters, whose size
    // the sharded count rows fix), and the last completed run's copy (rmc_get_coverage)
    unsigned long long* d_cov = nullptr;
    rmc_coverage cov{};
    int cov_valid = 0;
    // continue past violations (RMC_FLAG_CONTINUE; rmc_viol.h): the device tallies (VIOL_WORDS
    // words: first, each, least index), allocated only with the flag, the last completed run's
    // result (rmc_get_violations) and its least indices (rmc_trace_violation)
    unsigned long long* d_viol = nullptr;
    rmc_violations viol{};
    rmc::u64 viol_least[RMC_INV_COUNT] = {};
    int viol_valid = 0;
    // model-defined invariants (rmc_set_predicates; rmc_pred.h, rmc_pred.cpp): the ctx's copy of the
    // program and its names, the program in device memory and the pass's word (min over the states
    // a predicate fails on of index << 8 | predicate << 1 | error), all allocated by
    // rmc_set_predicates only; whether the violation reported is an evaluation error
    rmc_predicates* preds = nullptr;
    rmc::pred::Program* d_prog = nullptr;
    unsigned long long* d_pword = nullptr;
    int pred_error = 0;
    // action properties (rmc_set_actions; rmc_act.cpp, rmc_dev_act.h): the ctx's copy of the program and
    // its names, the program in device memory and the pass's word (min over the failing transitions
    // of source << 16 | lane << 8 | property << 1 | error), all allocated by rmc_set_actions only; and
    // the last run's reported transition (act_hit: rmc_action_violation, and rmc_trace's last state)
    rmc_predicates* acts = nullptr;
    rmc::pred::Program* d_aprog = nullptr;
    rmc::Params* d_apar = nullptr;  // the run's Params in device memory (act_begin)
    unsigned long long* d_aword = nullptr;
    int act_hit = 0, act_prop = 0, act_lane = 0, act_error = 0;
    rmc::u64 act_src = 0;
    // model-defined constraints (rmc_set_constraints; rmc_cons.cpp, rmc_dev_cons.h): the ctx's copy of
    // the residuals' program and names, the program in device memory, the pass's word (min over the
    // states a residual's evaluation failed on), its scratch for launches of up to cons_cap new states
    // — all allocated by rmc_set_constraints and the passes only — the Params its expansion launches
    // run with (no fused invariant check, no commuting-diamond skipping), and 1 + the residual whose
    // evaluation stopped the last run
    rmc_predicates* cons = nullptr;
    rmc::pred::Program* d_cprog = nullptr;
    unsigned long long* d_cword = nullptr;
    rmc::ConsBufs CB{};
    rmc::u64 cons_cap = 0;
    rmc::Params PE{};
    int cons_error = 0;
    rmc::u64 cons_passes = 0, cons_removed = 0;  // the last run's passes and the states they removed
    // state graph export (rmc_graph.cpp): a completed rmc_run_bfs whose store, links and set the
    // calls may read; its fingerprint salt (rmc_set_seed may change cfg.seed after it); and whether
    // B.sidx maps every stored state's set slot to its index — a verification run leaves it so, any
    // other ctx builds it at its first graph call (one k_publish pass); every rmc_run_bfs resets both
    int run_done = 0;
    int run_cons = 0;  // ... and it ran with constraints: its set holds keys of removed states, which no stored state owns
    int graph_idx = 0;
    rmc::u64 run_seed = 0;
    rmc_result res{};
    std::string err;
    std::vector<rmc::u64> level_start;  // level d (1-based) = [level_start[d-1], level_start[d])
    int have_target = 0;                // a violation / deadlock state to trace
    int stop = 0;                       // ... that ends the search (RMC_FLAG_CONTINUE: a deadlock only)
    rmc::u64 target_idx = 0;            // sharded: global ref (rank << 48 | index)
    DistState dist;
    SpillState spill;
    // recovery (rmc_recover): the next rmc_run_bfs continues from this level
    int resume = 0;
    int resume_depth = 0;
    // the wide layout (raft_wide.h): bounds beyond the packed capacity
    int wide = 0;
    rmc::wide::WModel WM{};
    rmc::wide::WideBufs WB{};
    rmc::wide::WState* w_staged = nullptr;
};

#define HIPCHK(c, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return rmc_host::fail((c), e_ == hipErrorOutOfMemory ? RMC_E_NOMEM : RMC_E_HIP,           \
                                  std::string(#expr) + ": " + hipGetErrorString(e_));                \
    } while (0)

namespace rmc_host {
// TLC's "calculated (optimistic)" collision estimate D * (G - D) / 2^b for the
// fingerprint bits b the set compares: 64 of k plus the bits of the second sum
// folded in under the slot mask, min(32, log2 slots) (raft_packed.h Fp).
inline double fp_collision_estimate(double D, double G, rmc::u64 slots, bool tagged = false) {
    int lb = 0;
    while (lb < 32 && (2ull << lb) <= slots) ++lb;
    // a tagged set compares 56 + lb bits (the top 8 hold the run's epoch)
    return D * (G - D) / 18446744073709551616.0 / (double)(1ull << lb) * (tagged ? 256.0 : 1.0);
}
int fail(rmc_ctx* c, int code, const std::string& msg);
int kcap_for(int max_msgs);
int validate(const rmc_config* c, std::string* why);
void fill_params(rmc_ctx* c);
int reset_counters(rmc_ctx* c, bool keep_count);
int read_counters(rmc_ctx* c);
// The set of a fresh run, single-GPU or sharded: the next set epoch or a cleared
// set (rmc_plan.h next_set_epoch under RMC_SET_EPOCH; tagged: the run's kernels
// can tell epochs apart), verification's slot -> state map cleared, the salt set.
int begin_set(rmc_ctx* c, bool tagged);
// Init (raft.tla:125-129), the one initial state: encoded, staged and seeded (k_seed).
int seed_init(rmc_ctx* c);
// Action coverage, both layouts: the tallies zeroed at the start of a run, and
// copied out at its end (the stream is idle after it).
inline bool cover_on(const rmc_ctx* c) { return (c->cfg.flags & RMC_FLAG_COVERAGE) != 0; }
int cover_begin(rmc_ctx* c);
int cover_end(rmc_ctx* c);
// Continue past violations, both layouts: the tallies cleared at the start of a
// run (the least indices to ~0), and at its end copied out and turned into
// rmc_violations (depth[r]: the level of level_start that holds the least index).
inline bool continue_on(const rmc_ctx* c) { return (c->cfg.flags & RMC_FLAG_CONTINUE) != 0; }
int viol_begin(rmc_ctx* c);
int viol_end(rmc_ctx* c);
// Model-defined invariants, both layouts: the word cleared at the start of a run; the pass
// over the states a launch (or the seed) added, [nlo, nhi); and at a level's end (after
// scan_target) the word read back and merged with the fused check's target: the least
// index wins, at equal index the built-in invariant.
inline bool pred_on(const rmc_ctx* c) { return c->preds != nullptr; }
int pred_begin(rmc_ctx* c);
int pred_pass(rmc_ctx* c, rmc::u64 nlo, rmc::u64 nhi);
int pred_scan(rmc_ctx* c, int depth);
void pred_free(rmc_ctx* c);
// Model-defined constraints (packed layout, resident store): at the start of a run the word
// cleared and PE set; the pass over the states a launch (or the seed) added, [nlo, nhi) — filter,
// in-place compaction, Counters read back (count = nlo + kept), then the built-in invariants over
// the kept states (launched, not waited for); at a level's end (after scan_target and
// pred_scan) the word read back: an evaluation error stops the search, the target the least kept
// state of the level [level_lo, count) on which a residual's evaluation fails.
inline bool cons_on(const rmc_ctx* c) { return c->cons != nullptr; }
// Action properties (packed layout, single GPU): the word cleared at the start of a run; the pass
// over a launch's parents [lo, hi), still resident; at a level's end (after the invariants' scans)
// the word read back: it is the target only when no invariant is violated in the level.  act_tail:
// the reported transition's successor, recomputed on the host from the stored source `src` (NW
// words) through the lane code.
inline bool act_on(const rmc_ctx* c) { return c->acts != nullptr; }
int act_begin(rmc_ctx* c);
int act_pass(rmc_ctx* c, rmc::u64 lo, rmc::u64 hi);
int act_scan(rmc_ctx* c);
void act_free(rmc_ctx* c);
int act_successor(rmc_ctx* c, const rmc::u32* src, int lane, rmc::u32* out);
// The Params of the seed and expansion launches.
inline const rmc::Params& expand_params(const rmc_ctx* c) { return c->cons ? c->PE : c->P; }
int cons_begin(rmc_ctx* c);
int cons_pass(rmc_ctx* c, rmc::u64 nlo, rmc::u64 nhi);
int cons_scan(rmc_ctx* c, int depth, rmc::u64 level_lo);
int cons_end(rmc_ctx* c);  // RMC_CONS_STATS: one stderr line of the run's passes, states removed and moved
void cons_free(rmc_ctx* c);
int pred_eval_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, uint8_t* d_out);  // rmc_wide.cpp
// After the seed launch's read_counters, on either layout: level 1 is the states
// it stored, and an invariant Init violates is the target.  Returns the depth.
int seed_done(rmc_ctx* c);
// What the level epilogue of the two layouts differs in.
struct LevelText {
    const char* no_owner;    // RMC_E_HIP message of Counters.overflow & 8
    const char* tie_full;    // RMC_E_CAPACITY message of Counters.overflow & 16 (nullptr: no tie buffer)
    const char* store_noun;  // "state store full (capacity N <noun>)"
    rmc::u64* walked;        // accumulates Counters.walked (nullptr: not counted)
};
// The error a level's counters report (Counters.table_full / overflow), 0 if
// none; rank: the sharded rank the row came from, named in the message (-1: a
// single GPU).  Bit 16 is the single-GPU tie buffer's, bit 2 the sharded parking buffer's.
int level_error(rmc_ctx* c, const rmc::Counters& k, int depth, const LevelText& text, int rank);
// The violation, else deadlock (RMC_FLAG_CHECK_DEADLOCK), the counter rows of n
// ranks report, as the target to trace (target_idx = rank << 48 | index; the
// lowest rank's wins); nothing if a target is already known.  Either one stops
// the search (c->stop) — under RMC_FLAG_CONTINUE only the deadlock does: the
// first violation is recorded once, stays the target, and the search goes on.
void scan_target(rmc_ctx* c, const rmc::Counters* rows, int n, int depth);
// The end of a level's launches (hi: the states before it), from the closing
// event to the progress callback: kernel time, the Counters.overflow errors,
// the result's totals, level_start / depth, the violation or deadlock target.
// *more = 0 when the search ends here: no new states, or the callback stopped it.
int end_level(rmc_ctx* c, rmc::u64 hi, int* depth, rmc_progress_fn cb, void* user,
              std::chrono::steady_clock::time_point t0, const LevelText& text, int* more);
// RMC_E_CAPACITY: a spilled search whose window of `win` states has no room for
// one more launch (ring_room, rmc_plan.h) beside a set of slot_bytes per slot
int window_too_small(rmc_ctx* c, rmc::u64 win, rmc::u64 slot_bytes);
// RMC_E_CAPACITY message for an unbounded field a successor took past the
// packed capacity (Counters.overflow bits 8-11), "" if none
std::string capacity_message(const rmc_ctx* c, rmc::u32 overflow, int depth);
// sharded mode (rmc_dist.cpp)
int run_bfs_sharded(rmc_ctx* c, rmc_progress_fn cb, void* user);
int trace_sharded(rmc_ctx* c, rmc_state_view* states, int32_t* families, int32_t* instances, size_t cap,
                  size_t* len);
void free_dist(rmc_ctx* c);
// frontier spill (rmc_spill.cpp)
rmc::u64 max_new_per_state(const rmc_ctx* c);  // what the window's launches are sized by
void spill_rebase(rmc_ctx* c, rmc::u64 base);
int spill_reserve(rmc_ctx* c);
void spill_prefault_ahead(rmc_ctx* c, rmc::u64 f1);  // back the link pages [faulted, f1) on X.ahead
int spill_to(rmc_ctx* c, rmc::u64 a, rmc::u64 count);
void spill_free(rmc_ctx* c);
int verify_spill_reserve(rmc_ctx* c);
int verify_copy_out(rmc_ctx* c, rmc::u64 upto);
int verify_host_hits(rmc_ctx* c, rmc::u64 n);
int read_link(rmc_ctx* c, rmc::u64 idx, rmc::u64* parent, uint8_t* act);
// the wide layout (rmc_wide.cpp)
bool wide_wanted(const rmc_config& g);
size_t wide_record_bytes(const rmc_config& g);  // the BFS store's record: compact or full
int validate_wide(const rmc_config* c, std::string* why);
int create_wide(rmc_ctx* c);
void destroy_wide(rmc_ctx* c);
int run_bfs_wide(rmc_ctx* c, rmc_progress_fn cb, void* user);
int trace_wide(rmc_ctx* c, rmc::u64 target, rmc_state_view* states, int32_t* families, int32_t* instances, size_t cap,
               size_t* len);
int expand_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, rmc_succ_view* out, size_t cap, size_t* n_out);
int keys_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, uint64_t* keys, const uint32_t* ref, uint8_t* same);
int check_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, uint32_t mask, int32_t* violated);
int sim_wide(rmc_ctx* c, const rmc_sim_config* sc, rmc_sim_result* out, rmc::i64 rec_beh,
             std::vector<rmc_state_view>* rec);
void fill_wide_model(rmc_ctx* c);
inline SmokeShape smoke_shape(const rmc_config& g, bool wide) {  // what SmokeInit draws for (rmc_codec.h)
    return {g.n_servers, g.n_values, wide, wide ? rmc::wide::KW : kcap_for(g.max_msgs)};
}

// A per-call allocation of n T's (hipMalloc; Pinned: hipHostMalloc), freed at scope exit.
template <class T, bool Pinned = false>
class DevScratch {
    void* p_ = nullptr;

public:
    DevScratch() = default;
    DevScratch(DevScratch&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    ~DevScratch() { (void)(Pinned ? hipHostFree(p_) : hipFree(p_)); }  // (a null pointer is no error)
    hipError_t alloc(size_t n) {  // once per object
        return Pinned ? hipHostMalloc(&p_, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p_, n * sizeof(T));
    }
    T* get() const { return (T*)p_; }
};

// Simulation, both layouts: the counters start clear, `go` launches the walks on
// c->st between ev0 and ev1, and *h is what they counted.
template <class F>
int sim_timed(rmc_ctx* c, rmc::SimCounters* d_out, rmc::SimCounters* h, float* ms, F go) {
    *h = rmc::SimCounters{};
    h->viol = ~0ull;
    HIPCHK(c, hipMemcpy(d_out, h, sizeof *h, hipMemcpyHostToDevice));
    HIPCHK(c, hipEventRecord(c->ev0, c->st));
    HIPCHK(c, go());
    HIPCHK(c, hipEventRecord(c->ev1, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    HIPCHK(c, hipMemcpy(h, d_out, sizeof *h, hipMemcpyDeviceToHost));
    return 0;
}
inline void fill_sim_result(rmc_sim_result* out, const rmc::SimCounters& h, rmc::u64 behaviours, rmc::u64 n_init,
                            float ms, std::chrono::steady_clock::time_point t0) {
    memset(out, 0, sizeof *out);
    out->behaviours = behaviours;
    out->steps = h.steps;
    out->init_states = n_init;
    out->truncated = h.truncated;
    out->deadlocked = h.deadlocked;
    if (h.viol != ~0ull) {
        out->violated_inv = 1 << (int)((h.viol >> 40) & 15);
        out->violation_depth = (int32_t)(h.viol >> 44);
        out->violation_behaviour = h.viol & ((1ull << 40) - 1);
    }
    out->kernel_seconds = 1e-3 * ms;
    out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The counterexample's parent links from `target` back to an initial state, then
// reversed: read_one(idx, &parent, &act) reads one link.
template <class F>
int walk_links(rmc_ctx* c, rmc::u64 target, F read_one, std::vector<rmc::u64>* chain, std::vector<uint8_t>* acts) {
    for (rmc::u64 idx = target;;) {
        rmc::u64 p = 0;
        uint8_t a = 0;
        if (int rc = read_one(idx, &p, &a)) return rc;
        chain->push_back(idx);
        acts->push_back(a);
        if (p == ~0ull || chain->size() > 100000) break;
        idx = p;
    }
    std::reverse(chain->begin(), chain->end());
    std::reverse(acts->begin(), acts->end());
    return 0;
}
inline void fill_step(int32_t* families, int32_t* instances, size_t q, int family, uint8_t act) {
    if (families) families[q] = family;
    if (instances) instances[q] = act == 255 ? -1 : act;
}
}  // namespace rmc_host
