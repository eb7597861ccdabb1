// rmc_internal.h — structures shared by the host engine and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raft_packed.h"
#include "raft_wide.h"

namespace rmc {
namespace pred {
struct Program;  // rmc_pred.h: a compiled set of model-defined invariants
}

// Device-side counters of one BFS level (zeroed/reset by the host per level).
struct Counters {
    u64 count;      // next free index of the state store (= distinct so far)
    u64 generated;  // successors generated in this launch
    u64 viol;       // min over violating new states of (index << 4 | invariant), ~0 = none
    u64 deadlock;   // min index of a state with no enabled lane, ~0 = none
    u32 overflow;   // state store full
    u32 table_full; // fingerprint set full
    u64 probes;     // fingerprint-set probes issued by k_expand
    // full-state verification mode (RMC_FLAG_VERIFY_STATES)
    u64 collisions; // fingerprint hits whose stored state differs from the successor
    u64 vchecked;   // fingerprint hits compared state against state
    u64 vcount;     // deferred hits in vbuf (stored twin not yet published)
    u64 nties;      // SYMMETRY: successors with tied signatures deferred to k_ties
    u64 novf;       // sharded: keys that did not fit their owner's outbox (parked in B.ovf)
    u64 wnext;      // dynamic work units: the next (window, wave slot) of the launch (zeroed by k_window_order)
    u64 walked;     // (state, lane) slots the lane walk visited (RMC_WALK_STATS: lane efficiency = generated / walked)
    u64 hcount;     // verification + spill: hits in hbuf whose stored owner has left the device window
};

struct DevBufs {
    u32* store;      // packed states, (2S + K) words each; levels are contiguous ranges
    u64* parent;     // parent index per state (~0 for initial states)
    uint8_t* act;    // lane that produced the state (255 for initial states)
    u64* foot;       // messages the producing lane acted on / added (make_foot; 0 = unknown)
    uint8_t* cls;    // window-sort class of each state (state_class_fine; a layout hint)
    uint16_t* word;  // presorted windows (k_window_order): the launch's window positions in class order
    u64* table;      // fingerprint set, power-of-two slots, 0 = empty
    u64 tmask;       // slots - 1
    u64 cap;         // state store capacity
    // ring window (RMC_FLAG_SPILL with the trace links in HBM): store / foot / cls hold
    // state i at slot i & wmask, the last wmask + 1 states; ~0 (resident, host-link
    // spill, sharded): slot = index.  parent / act are indexed by the index itself.
    u64 wmask;
    Counters* ctr;
    // sharded mode (rank/world > 1 GPU processes; single mode: rank 0, world 1)
    u32 rank, world;
    u32 owner_mode;            // 0: by fingerprint, 1: by server 0 word, 2: by servers 0+1 words (default), 3: all words
    u64 ref_tag;               // (rank << 48): parent refs are global (rank, index)
    u64* sent;                 // lossy cache of fingerprints already shipped to their owner
    u64 smask;                 // sent-cache slots - 1
    // two-phase exchange: phase 1 keys, phase 2 accepted states
    u64* key_out;              // [world][kcap] 12-B keys for each owner: the raw fingerprint {k lo, k hi, s32}
    u64* tick_out;             // [world][kcap] local tickets: parent index | lane << 56, or POOL_TICK | pool index
    u64 kcap;                  // keys per destination and chunk
    unsigned long long* ocount;  // [world] keys written per destination
    u32* st_out;               // [world][scap][NW + 4] accepted states for each owner (+ ref, footprint)
    u64 scap;                  // state records per destination and round (= kcap)
    unsigned long long* scount;  // [world] state records written per destination
    // keys whose owner's outbox was full: {k, s32 | flags << 32, parent index | dest << 48 |
    // lane << 56}, sent in later exchange rounds of the same level (never dropped);
    // flag OVF_UNKEYED: a successor the expansion could not put in the pool, keyed by k_route_fix
    u64* ovf;
    u64 ovf_cap;               // records in ovf
    // remote-successor pool (the sharded expansion's default flush, flush_pool):
    // every new successor owned by another rank, materialised once as its
    // phase-2 record {state, global parent ref | lane << 40, footprint}; k_route
    // then keys it and fills the owners' outboxes with tickets POOL_TICK | index
    u32* pool;
    u64 pool_cap;              // records in pool
    unsigned long long* npool; // records written (may exceed pool_cap: the rest were parked)
    // replicated levels (small levels of a sharded search): the whole level's
    // records, gathered from every rank (RepRec: state, global ref, footprint, lane | class)
    const u32* rep;
    // full-state verification mode: store index of the state owning each
    // fingerprint-set slot (~0 = not yet published; published between launches
    // by k_publish) and the deferred hits {parent index, slot | lane << 56}.  The state graph calls
    // (rmc_graph.cpp) allocate and publish sidx on a ctx without the mode too, after a run
    u64* sidx;
    u64* vbuf;
    u64 vcap;                  // records in vbuf
    // verification + spill: owners with a store index below vlo are no longer on
    // the device (spilled; their host copies are compared after the launch): such
    // hits go to hbuf as {parent index, owner index | lane << 56}
    u64 vlo;
    u64* hbuf;
    u64 hcap;                  // records in hbuf
    // SYMMETRY: successors whose server signatures tie, {parent index | lane << 56},
    // canonicalised by k_ties after each expansion launch
    u64* ties;
    u64 tie_cap;
    // per launch (rmc_plan.h): the store index no flush may reach — cap, and on the ring
    // never past live_lo + window (the overflow bit instead of a live slot overwritten) —
    // and the reserve of a dynamic-unit launch's admission: once the count is above
    // lim - admit_reserve no further unit is claimed (0: no admission, lim is the only bound)
    u64 lim;
    u32 admit_reserve;
};

// The constraint pass's scratch of one launch's n new states (rmc_dev_cons.h; allocated by
// rmc_set_constraints' ctx only, grown to the largest launch): a keep byte per state, the kept
// count of each tile of 256 and their exclusive scan (off[tiles]: the kept states in all), and
// the head's holes in rank order (at most n / 2).
struct ConsBufs {
    uint8_t* keep;
    u32* cnt;
    u64* off;
    u64* dst;
};

struct PermTable {
    u32 code[120];  // every server permutation (old id -> new id), 3 bits per id, S <= 5
    int np;         // S!
};

struct Shape {
    int S, K;
    bool sym;
    bool verify;  // full-state verification (single GPU)
};

// One edge of the state graph (k_graph_edges): rmc.h's rmc_edge, field for field.
struct GraphEdge {
    u64 src, dst;  // store indices; dst ~0: the set does not hold the successor's key (an error)
    int family, instance;
};

// Simulation counters (k_simulate).
typedef int64_t i64;
struct SimCounters {
    u64 steps, truncated, deadlocked;
    u64 viol;  // min over violations of (depth << 44 | invariant << 40 | behaviour), ~0 = none
};

// The launchers of one packed shape (S servers, K bag slots), on buffers B and stream st, each
// named after its kernel.  sym / verify are Shape's; expand_rep and route (the plain search only)
// and ties (SYMMETRY only) go by P.symmetry, which fill_params sets from Shape.  A launch over no
// work items launches nothing and succeeds.
struct ShapeKernels {
    using Expand = hipError_t(bool sym, bool verify, const Params& P, const PermTable& PT, const DevBufs& B, u64 lo,
                              u64 hi, hipStream_t st);
    using Range = hipError_t(bool sym, const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi,
                             hipStream_t st);
    Expand *expand, *expand_dist;  // over store[lo, hi): single GPU / sharded (outbox and pool in B)
    // The plain single-GPU search's launch (k_expand_sort, dynamic units) over nf states: its
    // blocks, the tiles of its windows and units, and the entries a wave's list holds — what
    // the ring's admission reserve is made of (rmc_plan.h admit_reserve).
    struct AdmitShape {
        u64 grid;
        u32 wt, ut, list_cap;
    };
    AdmitShape (*admit_shape)(u64 nf);
    // ... re-launched over the same [lo, hi) after it stopped on admission (B.admit_reserve): from
    // the Counters.wnext it left, on the presorted positions it left in B.word
    hipError_t (*expand_resume)(const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi, hipStream_t st);
    hipError_t (*expand_rep)(const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi, hipStream_t st);
    hipError_t (*route)(const Params& P, const DevBufs& B, hipStream_t st);  // k_route_fix, then k_route
    hipError_t (*ties)(const Params& P, const PermTable& PT, const DevBufs& B, hipStream_t st);
    hipError_t (*seed)(bool sym, const Params& P, const PermTable& PT, const DevBufs& B, const u32* staged, u64 n,
                       hipStream_t st);
    hipError_t (*list)(bool sym, const Params& P, const PermTable& PT, const u32* in, u64 n, u32* out, u64 cap,
                       unsigned long long* count, hipStream_t st);
    Range *publish, *rehash;  // over store[lo, hi)
    hipError_t (*verify)(bool sym, const Params& P, const PermTable& PT, const DevBufs& B, u64 n_hits, hipStream_t st);
    hipError_t (*verify_host)(bool sym, const Params& P, const PermTable& PT, const DevBufs& B,
                              const u32* staged_owners, u64 n_hits, u64 hbuf_off, hipStream_t st);
    hipError_t (*materialize_remote)(const Params& P, const DevBufs& B, const uint8_t* reply, u64 keys_per_dest,
                                     u64 window_off, hipStream_t st);
    hipError_t (*store_remote)(const Params& P, const DevBufs& B, const u32* recs, u64 n, hipStream_t st);
    hipError_t (*compare_remote)(bool sym, const Params& P, const PermTable& PT, const DevBufs& B, const u32* recs,
                                 u64 n, hipStream_t st);
    hipError_t (*pack_rep)(const DevBufs& B, u64 lo, u64 hi, u32* out, hipStream_t st);
    hipError_t (*simulate)(const Params& P, const u32* inits, u64 n_init, u64 n_beh, int depth, u64 seed, int mode,
                           SimCounters* out, i64 rec_beh, u32* rec, hipStream_t st);
    // parents [lo, hi) and the states their launch added, [nlo, nhi), into cov (k_cover, rmc_dev_tools.h)
    hipError_t (*cover)(const Params& P, const DevBufs& B, u64 lo, u64 hi, u64 nlo, u64 nhi, u64 n_init,
                        unsigned long long* cov, hipStream_t st);
    // the states a launch added, [nlo, nhi), into the violation tallies (k_violations, rmc_dev_tools.h;
    // viol: VIOL_WORDS words, rmc_viol.h)
    hipError_t (*violations)(const Params& P, const DevBufs& B, u64 nlo, u64 nhi, unsigned long long* viol,
                             hipStream_t st);
    hipError_t (*check)(const Params& P, const u32* in, u64 n, int* out, hipStream_t st);
    // model-defined invariants (k_pred, k_pred_eval, rmc_dev_pred.h; prog: the program in device memory):
    // the states a launch added, [nlo, nhi), into word = min (index << 8 | predicate << 1 | error) over
    // the states on which a predicate does not hold; out[t * n_pred + p] = predicate p's verdict on in[t]
    hipError_t (*pred)(const pred::Program* prog, const DevBufs& B, u64 nlo, u64 nhi, unsigned long long* word,
                       hipStream_t st);
    hipError_t (*pred_eval)(const pred::Program* prog, const u32* in, u64 n, uint8_t* out, hipStream_t st);
    // action properties (k_act, k_act_eval, rmc_dev_act.h): the transitions out of a launch's parents
    // [lo, hi) that are edges of the state graph, into word = min (source << 16 | lane << 8 |
    // property << 1 | error) over those a property does not hold on; out[t * n_pred + p] = property
    // p's verdict on the pair in[t] (the current state's words, then the next state's).  P: the
    // model's parameters in device memory (the kernel keeps them in LDS)
    hipError_t (*act)(const pred::Program* prog, const Params* P, const DevBufs& B, u64 lo, u64 hi,
                      unsigned long long* word, hipStream_t st);
    hipError_t (*act_eval)(const pred::Program* prog, const u32* in, u64 n, uint8_t* out, hipStream_t st);
    // model-defined constraints (rmc_dev_cons.h; prog: the residuals' program in device memory): the
    // states a launch added, [nlo, nhi), filtered and compacted in place — afterwards [nlo, nlo + kept)
    // holds the kept states with their links and Counters.count = nlo + kept; word = min (index << 8 |
    // residual << 1 | 1) over the states a residual's evaluation failed on (their index before the
    // move), word[1] += the states moved.  cons_inv: the built-in invariants of P.inv_mask on the kept states [lo, hi), into
    // Counters.viol as the fused check writes it
    hipError_t (*cons)(const pred::Program* prog, const DevBufs& B, u64 nlo, u64 nhi, const ConsBufs& C,
                       unsigned long long* word, hipStream_t st);
    hipError_t (*cons_inv)(const Params& P, const DevBufs& B, u64 lo, u64 hi, hipStream_t st);
    // keys[t] = the key of in[t] (P.fp_mask applied); ref != nullptr: same[t] = in[t] compares equal to
    // the record in[ref[t]] (k_keys, rmc_dev_tools.h)
    hipError_t (*keys)(bool sym, const Params& P, const PermTable& PT, const u32* in, u64 n, u64* keys,
                       const u32* ref, unsigned char* same, hipStream_t st);
    hipError_t (*set_salt)(u64 salt, u64 epoch, hipStream_t st);  // epoch << 56; returns after the copies
    // the state graph (rmc_dev_graph.h; B.sidx published for every stored state): cnt[i - lo] = the
    // edges out of stored state i of [lo, hi); those edges at out[off[i - lo] ..] (off: the exclusive
    // scan of cnt, launch_graph_scan), err: min (src << 8 | lane) of an edge without its key in the
    // set; index[t] = the store index of the stored state with staged state in[t]'s key, or ~0
    hipError_t (*graph_count)(const Params& P, const DevBufs& B, u64 lo, u64 hi, u32* cnt, hipStream_t st);
    hipError_t (*graph_edges)(bool sym, const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi,
                              const u64* off, GraphEdge* out, u64 cap, unsigned long long* err, hipStream_t st);
    hipError_t (*graph_find)(bool sym, const Params& P, const PermTable& PT, const DevBufs& B, const u32* in, u64 n,
                             u64* index, hipStream_t st);
};
// The table of shape (S, K), defined by its object (rmc_kernels_shape.hip), and its lookup:
// nullptr for a shape that is not built.  The tables are filled when the library loads: not
// for use from another object's static initialiser.
#define RMC_SHAPE_TABLE(SS, KK) kShapeKernels_##SS##_##KK
const ShapeKernels* shape_kernels(int S, int K);

// Sharded mode, phase 1 owner side: insert n received keys (12-B {k lo, k hi, s32}
// records), reply[t] = new;
// keys [src_off[p], src_off[p + 1]) came from rank p, acc[p] += keys of p that were new.
constexpr int kMaxWorld = 64;
struct SrcOff {
    u64 o[kMaxWorld + 1];
};
hipError_t launch_owner_insert(const DevBufs& B, const u64* keys, uint8_t* reply, u64 n, const SrcOff& so,
                               unsigned long long* acc, hipStream_t st);
// Sharded mode: the exchange-count row of one round, one block of kRowWords u64
// per rank p: [0] keys for p (min(ocount[p], kcap), 0 for p = rank), [1] flags
// (bit 0: this rank has more to send: host_more, or parked keys beyond
// ovf_done; bit 1: its parking buffer overflowed; bit 2: it sends keys this
// round), [2..] this rank's Counters (so a round after which nothing changes
// them ends the level without a counter all-gather); out[kRowWords * W] = novf.
constexpr int kRowWords = 2 + (int)(sizeof(Counters) / 8);
static_assert(sizeof(Counters) % 8 == 0, "Counters travel as u64 words");
// mirror (a world of one): the row's blocks also written there (its received half).
hipError_t launch_pack_counts(const DevBufs& B, u64 host_more, u64 ovf_done, u64* out, hipStream_t st,
                              u64* mirror = nullptr);
// States per single-GPU expansion launch at most (B.word holds one launch's
// presorted window positions: min(2^kMaxLaunchLog2, the store's states) entries);
// a launch of the sharded search (rmc_dist.cpp round_states) at most 2^kMaxDistLaunchLog2.
constexpr int kMaxLaunchLog2 = 28;
constexpr int kMaxDistLaunchLog2 = 25;
// Presorted windows: k_window_order over the launch [lo, hi) for an expansion
// grid of `grid` blocks and windows of at most wt_max tiles (B.word).
hipError_t launch_window_order(const DevBufs& B, u64 lo, u64 hi, u64 grid, u64 wt_max, hipStream_t st);
// One round of resident blocks of kernel k (256 threads) on this device (rmc_kernels_common.hip).
u64 resident_grid(const void* k);
// The slot of state index i in the store / foot / cls arrays (DevBufs.wmask).
__host__ __device__ __forceinline__ u64 wslot(const DevBufs& B, u64 i) { return i & B.wmask; }
// Sharded mode: move parked keys ovf[a, a + n) into the (emptied) outbox; n <= kcap.
hipError_t launch_drain(const DevBufs& B, u64 a, u64 n, hipStream_t st);
// Outbox ticket of a pool record (bit 48: a parent ticket's index is < 2^48 and
// its lane sits at bits 56-63).
constexpr u64 POOL_TICK = 1ull << 48;

// Fingerprint salt for the kernels of shape k on this device (0 = default
// hash); returns after the copy (the staging value lives on the caller's stack).
// the fingerprint salt of rmc_config.seed and the set epoch of the run (raft_packed.h
// c_set_ep: 0 = an untagged set, cleared before the run)
hipError_t set_fp_salt(const ShapeKernels& k, u64 seed, u32 set_epoch, hipStream_t st);

// Sets bytes [p, p + bytes) to `byte` (the fingerprint set's clear; RMC_FILL=0: hipMemsetAsync).
hipError_t launch_fill(void* p, u64 bytes, uint8_t byte, hipStream_t st);
// off[0 .. n] = the exclusive scan of cnt[0 .. n) (off[n]: the total), one block.
hipError_t launch_graph_scan(const u32* cnt, u64 n, u64* off, hipStream_t st);
// Random-probe microbenchmark over table[mask + 1] (mode 0 loads, 1 CAS).
hipError_t launch_probe_bench(u64* table, u64 mask, u64 threads, u32 iters, int mode, u64* sink, hipStream_t st);

// ---- the wide layout (raft_wide.h, rmc_wide.hip) ------------------------------------
namespace wide {
struct WideBufs {
    void* store;      // wide records (WState, WStateC or WStateD); levels are contiguous ranges
    int compact;      // the store's record: 0 WState, 1 the compact WStateC, 2 the depth-sized WStateD
    u64* parent;      // parent index per state (~0 for initial states)
    uint8_t* act;     // lane that produced the state (255 for initial states)
    u64* table;       // fingerprint set (wfp keys), power-of-two slots
    u64 tmask, cap;
    Counters* ctr;
    u64 salt;         // fingerprint salt (rmc_config.seed)
    // ring window (RMC_FLAG_SPILL): the store holds state i at slot i % window, the
    // last `window` records (any size, no power of two); parent / act stay indexed
    // by the state's index and cap stays "all states".  0: no ring, slot = index.
    u64 window;
    int work;         // ring: the record the expansion works on (>= the store's; same numbering)
    int unstored;     // ring, per launch: the level being built is never expanded (max_depth):
                      // its states get index, links and the invariant check, no record
    // full-state verification (RMC_FLAG_VERIFY_STATES; resident store only): the
    // store index of the state owning each set slot (~0: none yet), written by the
    // inserting lane itself, and the hits of a launch on owners found in the same
    // launch {parent index, slot | lane << 48}, compared by k_wverify after it (a
    // lane needs 9 bits, a slot index is below 2^34).  The tallies are Counters'
    // collisions / vchecked / vcount.  verify = 0: none of these is read.
    int verify;
    u64* sidx;
    u64* vbuf;
    u64 vcap;         // records in vbuf
    u64 vbase;        // per launch: Counters.count when it began (owners at or above it are deferred)
    u64 fp_mask;      // fingerprint bits kept (~0 = all; rmc_set_fp_bits)
    int sym;          // RMC_FLAG_SYMMETRY: the set holds canonical orbit keys (wcanon), verification
                      // compares orbits (wsame_orbit); the records stored are the states found
};
// One successor listed by k_wlist (rmc_expand on the wide layout).
struct WSucc {
    u64 parent;
    int lane, code, in_model, pad;
    u64 fp;
    WState state;
};
hipError_t launch_wseed(const WModel& M, const WideBufs& B, const void* staged, u64 n, hipStream_t st);  // staged: B's work record (ring) / store record
hipError_t launch_wexpand(const WModel& M, const WideBufs& B, u64 lo, u64 hi, hipStream_t st);
hipError_t launch_wverify(const WModel& M, const WideBufs& B, u64 n, hipStream_t st);  // the n deferred hits in B.vbuf
// ShapeKernels::cover on the wide records (k_wcover)
hipError_t launch_wcover(const WModel& M, const WideBufs& B, u64 lo, u64 hi, u64 nlo, u64 nhi, u64 n_init,
                         unsigned long long* cov, hipStream_t st);
// ShapeKernels::violations on the wide records (k_wviolations; the resident store only)
hipError_t launch_wviolations(const WModel& M, const WideBufs& B, u64 nlo, u64 nhi, unsigned long long* viol,
                              hipStream_t st);
// sym: WSucc.fp is the canonical key under SYMMETRY (wcanon), else wfp
hipError_t launch_wlist(const WModel& M, const WState* in, u64 n, WSucc* out, u64 cap, unsigned long long* count,
                        u64 salt, int sym, hipStream_t st);
// rmc_state_keys on a wide ctx under SYMMETRY (k_wkeys): keys[t] as the search inserts it (wcanon),
// same[t] (ref given) by its verification's comparison of in[t] with in[ref[t]] (wsame_orbit)
hipError_t launch_wkeys(const WModel& M, const WState* in, u64 n, u64* keys, const u32* ref, unsigned char* same,
                        u64 salt, hipStream_t st);
hipError_t launch_wsimulate(const WModel& M, const WState* inits, u64 n_init, u64 n_beh, int depth, u64 seed, int mode,
                            SimCounters* out, i64 rec_beh, WState* rec, hipStream_t st);
// ShapeKernels::pred on the wide records (k_wpred; the resident store only), and ::pred_eval on
// staged records of the store's kind (k_wpred_eval; compact: WideBufs.compact's numbering)
hipError_t launch_wpred(const pred::Program* prog, const WModel& M, const WideBufs& B, u64 nlo, u64 nhi,
                        unsigned long long* word, hipStream_t st);
hipError_t launch_wpred_eval(const pred::Program* prog, const WModel& M, int compact, const void* in, u64 n,
                             uint8_t* out, hipStream_t st);
// rmc_check_states on the wide layout: out[t] = the invariant result of M.inv_mask on in[t], by
// wcheck_invariants with one thread per state (wave = 0: the BFS's and k_wsimulate's check), or by
// w_check_invariants_wave with one wave per state on a copy in LDS (k_wsimulate_w's)
hipError_t launch_wcheck(const WModel& M, const WState* in, u64 n, int* out, int wave, hipStream_t st);
}  // namespace wide

}  // namespace rmc
