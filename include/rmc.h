/*
 * rmc.h — C ABI of librmc.so, the MI355X-native breadth-first model checker
 * for raft.tla (the hot path of TLC's `tlc2.TLC -config MCraft.cfg MCraft.tla`).
 *
 * The reference path has no FFI of its own: it sits behind TLC's CLI and file
 * formats.  Each entry point below replaces one piece of that
 * path; the reference interface it replaces is cited next to it.  A Java
 * driver binds these through Panama FFM; the C++ CLI
 * (`bin/rmc-tlc`) and the Python ctypes harness (tests, bench) bind the same
 * symbols.
 *
 * Conventions: plain C types only; return 0 on success and a negative code
 * otherwise (RMC_E_*); the message is available from rmc_last_error(ctx).
 * No C++ exception crosses the ABI.  A ctx owns all device memory; output
 * buffers are caller-owned.  Calls on one ctx are not reentrant.
 */
#ifndef RMC_H_
#define RMC_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMC_ABI_VERSION 16 /* 6: rmc_result.spill_links_on_device (round 5); 7: .verified_spilled, 8: rmc_config.set_bytes and
                              rmc_result.set_slots (round 6); 9: RMC_FLAG_COVERAGE, rmc_coverage, rmc_get_coverage,
                              rmc_coverage_action (round 8); 10: rmc_check_states; 11: rmc_state_keys; 12: RMC_FLAG_CONTINUE,
                              rmc_violations, rmc_get_violations, rmc_trace_violation; 13: RMC_FLAG_SYMMETRY on the wide
                              layout (depth-bounded runs), rmc_state_keys on a wide ctx under it; 14: the state
                              graph: rmc_get_levels, rmc_read_states, rmc_find_states, rmc_graph_edges; 15: model-defined
                              invariants: RMC_FRONT_PREDICATES, rmc_predicates_from_files, rmc_set_predicates,
                              rmc_eval_predicates, rmc_predicate_error, RMC_INV_USER0; 16: model-defined
                              constraints: RMC_FRONT_CONSTRAINTS, rmc_constraints_from_files, rmc_set_constraints,
                              rmc_constraint_error; additive, still 16: action properties: RMC_FRONT_ACTIONS,
                              rmc_actions_from_files, rmc_set_actions, rmc_eval_actions, rmc_action_violation,
                              RMC_ACT_USER0, RMC_MAX_ACTION_PROPS */

/* Capacity of the packed encoding (DESIGN.md "Packed state"): the layout the
 * BFS kernels run on when every bound fits it. */
#define RMC_MAX_SERVERS 5
#define RMC_MAX_VALUES 2
#define RMC_MAX_LOG 3      /* MaxLogLen bound <= 3 */
#define RMC_MAX_MSGS 8     /* |DOMAIN messages| bound <= 8 */
#define RMC_MAX_TERM 14    /* MaxTerm bound <= 14 */
#define RMC_MAX_DUP 3      /* per-message count bound <= 3 */
/* Capacity of the wide encoding (DESIGN.md "Wide state"): a model with any
 * bound beyond the packed capacity — or a field no CONSTRAINT bounds, under a
 * depth bound or in simulation — runs on it (single GPU; RMC_FLAG_SYMMETRY
 * keeps one state per orbit of Permutations(Server): the set holds canonical
 * orbit keys, the records and traces are the states found, with the resident
 * store and with the ring, for runs under a depth bound — max_depth > 0; a model
 * whose CONSTRAINT exceeds the packed capacity searched to fixpoint under
 * SYMMETRY is RMC_E_INVAL — with RMC_FLAG_VERIFY_STATES, RMC_FLAG_COVERAGE and
 * RMC_FLAG_CONTINUE; RMC_FLAG_SPILL keeps its records in a ring window;
 * RMC_FLAG_VERIFY_STATES
 * compares every fingerprint hit with the resident stored state, so the two
 * flags together are RMC_E_INVAL: at the depths that need the ring — depth 15
 * of MCraft.cfg as shipped, 2.24 G states, 2^33 set slots — the slot-to-state
 * array of 8 B per slot no longer fits beside the set and the frontier; such a
 * run is cross-checked by a second fingerprint salt, rmc_config.seed).  A
 * CONSTRAINT bound must stay below the wide capacity; an unbounded field is
 * given the capacity itself, and a successor beyond it stops the search with
 * RMC_E_CAPACITY naming the field. */
#define RMC_WIDE_MAX_TERM 255
#define RMC_WIDE_MAX_LOG 32
#define RMC_WIDE_MAX_MSGS 64
#define RMC_WIDE_MAX_DUP 255
/* Sizes of the decoded state view (rmc_state_view): the wide capacity. */
#define RMC_VIEW_LOG 32
#define RMC_VIEW_MSGS 64

/* Error codes. */
#define RMC_OK 0
#define RMC_E_INVAL (-22)      /* config validation failed (TLC: semantic error) */
#define RMC_E_NOMEM (-12)      /* device allocation failed */
#define RMC_E_HIP (-5)         /* HIP runtime error */
#define RMC_E_CAPACITY (-28)   /* fingerprint set full, or state store full without RMC_FLAG_SPILL */
#define RMC_E_NOGPU (-19)      /* no usable gfx950 device */
#define RMC_E_PARSE (-74)      /* .cfg / .tla front-end could not recognise the model */
#define RMC_E_STATE (-71)      /* call out of order (e.g. rmc_trace before a violation) */
#define RMC_E_IO (-61)         /* checkpoint file missing, unreadable or of another model */

/* rmc_config.flags */
#define RMC_FLAG_SYMMETRY (1u << 0)        /* SYMMETRY Permutations(Server); both       */
                                           /* layouts (rmc_shard: the packed one; the   */
                                           /* wide one under max_depth > 0)             */
#define RMC_FLAG_CHECK_DEADLOCK (1u << 1)  /* CHECK_DEADLOCK TRUE (TLC default)         */
#define RMC_FLAG_BUG_QUORUM (1u << 2)      /* BecomeLeader guard raft.tla:197 weakened  */
                                           /* to votesGranted[i] /= {} (config 5)       */
#define RMC_FLAG_VERIFY_STATES (1u << 3)   /* full-state verification: every fingerprint */
                                           /* hit is compared with the stored state;    */
                                           /* differences = collisions (no TLC analog;  */
                                           /* single GPU).  Both layouts; on the wide   */
                                           /* one without RMC_FLAG_SPILL only (8 B more */
                                           /* per set slot, every state resident).      */
                                           /* With RMC_FLAG_SYMMETRY the comparison is  */
                                           /* "some permutation of the successor is the */
                                           /* stored state" (both layouts)              */
#define RMC_FLAG_SPILL (1u << 4)           /* frontier spill (TLC's states/ directory): */
                                           /* expanded levels leave the device window   */
                                           /* when it fills, so a model whose states    */
                                           /* outgrow HBM completes while its           */
                                           /* fingerprints fit.  Their trace links      */
                                           /* (parent, lane: 9 B) stay in HBM when they */
                                           /* fit (else they move to host memory).      */
                                           /* state_capacity then sizes the fingerprint */
                                           /* set and links (all states), device_window */
                                           /* the resident states.  Single GPU.  With   */
                                           /* RMC_FLAG_VERIFY_STATES every state leaving */
                                           /* the window keeps a host copy, and hits on  */
                                           /* it are compared with that copy (round 6;   */
                                           /* no checkpoint / recover then).  On the    */
                                           /* wide layout: a ring of exactly             */
                                           /* device_window records, the links always in */
                                           /* HBM; a run bounded by max_depth does not   */
                                           /* store its last level (never expanded), so  */
                                           /* its record is sized one level shallower;   */
                                           /* traces are replayed from Init; not with    */
                                           /* RMC_FLAG_VERIFY_STATES (RMC_E_INVAL)       */
/* A model without a CONSTRAINT on some field (MCraft.cfg as shipped) runs only
 * under a depth bound (max_depth > 0, TLC -depth).  The front-end then gives
 * each unbounded field the wide capacity (RMC_WIDE_MAX_TERM, RMC_WIDE_MAX_LOG,
 * RMC_WIDE_MAX_MSGS, RMC_WIDE_MAX_DUP) and sets its bit here; the search stops
 * with RMC_E_CAPACITY, naming the field, the first time a successor needs more
 * than the capacity (it is never silently filtered as out of the model). */
#define RMC_FLAG_UNBOUNDED_TERM (1u << 5)  /* no CONSTRAINT on currentTerm[i]            */
#define RMC_FLAG_UNBOUNDED_LOG (1u << 6)   /* no CONSTRAINT on Len(log[i])               */
#define RMC_FLAG_UNBOUNDED_MSGS (1u << 7)  /* no CONSTRAINT on Cardinality(DOMAIN messages) */
#define RMC_FLAG_UNBOUNDED_DUP (1u << 8)   /* no CONSTRAINT on messages[m]               */
#define RMC_UNBOUNDED_ANY (RMC_FLAG_UNBOUNDED_TERM | RMC_FLAG_UNBOUNDED_LOG | RMC_FLAG_UNBOUNDED_MSGS | \
                           RMC_FLAG_UNBOUNDED_DUP)
#define RMC_FLAG_COVERAGE (1u << 9)        /* action coverage (TLC -coverage): per-action  */
                                           /* generated / distinct counts of the BFS, read */
                                           /* with rmc_get_coverage.  Single GPU, both     */
                                           /* layouts, with RMC_FLAG_SYMMETRY on both; no  */
                                           /* checkpoint / recover; ignored by             */
                                           /* rmc_simulate                                 */
/* (bit 10 is not assigned: rmc_create refuses it as an unknown flag bit) */
#define RMC_FLAG_CONTINUE (1u << 11)       /* continue past violations (TLC -continue): a  */
                                           /* violated invariant does not stop rmc_run_bfs; */
                                           /* violating states are stored and expanded, and */
                                           /* counted per invariant (rmc_get_violations).   */
                                           /* Single GPU; the wide layout without           */
                                           /* RMC_FLAG_SPILL only; with RMC_FLAG_SYMMETRY   */
                                           /* on both layouts; no checkpoint / recover;     */
                                           /* ignored by rmc_simulate                       */

/* rmc_config.invariants — the INVARIANT names the engine knows (fused checks).
 * TypeOK on the packed layout: the search (rmc_run_bfs, rmc_simulate) evaluates
 * every conjunct a packed state can violate except two, which it takes by
 * induction from Init (or from SmokeInit's draws): the entry values inside
 * messages, m.mentries of an AppendEntriesRequest (raft.tla:456) and m.mlog of a
 * RequestVoteResponse (:465), in Seq([term : Nat, value : Value]).  A message's
 * entries are copied from a log (raft.tla:183, :259), a log's entries come from
 * ClientRequest (v \in Value) or from a message (:330), and the logs' values are
 * checked, so no state reached from Init violates them.  (nextIndex >= 1 holds
 * by construction of the packed word: it is stored minus one.)  rmc_check_states,
 * whose states come from the caller, evaluates the complete predicate, these two
 * conjuncts included; the wide layout evaluates it everywhere. */
#define RMC_INV_TYPEOK (1u << 0)           /* raft.tla:482-492                          */
#define RMC_INV_ONE_LEADER (1u << 1)       /* ElectionSafety restated (raft.tla:1124)   */
#define RMC_INV_LOG_MATCHING (1u << 2)     /* raft.tla:1132-1136                        */
#define RMC_INV_MESSAGES (1u << 3)         /* MessagesInv raft.tla:941-946 (:910 fixed)  */
#define RMC_INV_LEADER_VOTES (1u << 4)     /* LeaderVotesQuorum raft.tla:1033-1037       */
#define RMC_INV_CAND_TERM (1u << 5)        /* CandidateTermNotInLog raft.tla:1041-1047   */
/* The IsPrefix invariants (raft.tla:1143-1180), restated in specs/MCraftBounded.tla
 * with IsPrefix defined and Committed(i) = the first min(commitIndex[i], Len(log[i]))
 * entries of log[i] (raft.tla's SubSeq is out of range when commitIndex > Len). */
#define RMC_INV_VOTES_GRANTED (1u << 6)    /* VotesGrantedInv raft.tla:1145-1153         */
#define RMC_INV_QUORUM_LOG (1u << 7)       /* QuorumLogInv raft.tla:1157-1161            */
#define RMC_INV_MORE_UP_TO_DATE (1u << 8)  /* MoreUpToDateCorrect raft.tla:1167-1172     */
#define RMC_INV_LEADER_COMPLETE (1u << 9)  /* LeaderCompleteness raft.tla:1176-1180      */

/* A bounded model: constants of the MC module + the CONSTRAINT bounds.
 * Replaces the CONSTANTS / CONSTRAINT / INVARIANT / SYMMETRY / CHECK_DEADLOCK
 * sections of a TLC .cfg (MCraft.cfg:1-39, Smokeraft.cfg:43-48). */
typedef struct rmc_config {
    int32_t n_servers;        /* |Server|  (MCraft.tla:20-21: {r1,r2,r3})        */
    int32_t n_values;         /* |Value|   (MCraft.tla:15-16: {v1,v2})           */
    int32_t max_term;         /* CONSTRAINT \A i: currentTerm[i] <= max_term      */
    int32_t max_log_len;      /* CONSTRAINT \A i: Len(log[i]) <= max_log_len      */
    int32_t max_msgs;         /* CONSTRAINT Cardinality(DOMAIN messages) <= ..    */
    int32_t max_dup;          /* CONSTRAINT \A m: messages[m] <= max_dup          */
    uint32_t flags;           /* RMC_FLAG_*                                       */
    uint32_t invariants;      /* RMC_INV_*                                        */
    int32_t device;           /* HIP device ordinal                               */
    int32_t max_depth;        /* 0 = unbounded; else stop after this many levels  */
    uint64_t state_capacity;  /* distinct states this GPU may store; 0 = auto     */
    uint64_t seed;            /* BFS: fingerprint salt (0 = default hash; two runs */
                              /* with different salts and equal counts rule out   */
                              /* fingerprint collisions); simulation: RNG seed     */
    uint64_t device_window;   /* RMC_FLAG_SPILL: states resident on the device    */
                              /* (frontier + the level being built); 0 = auto     */
    uint64_t set_bytes;       /* the fingerprint set's size (TLC -fpmem), rounded */
                              /* down to a power of two of 8-B slots; it holds at */
                              /* most half as many states (a capacity error past  */
                              /* that).  With state_capacity given it is an upper */
                              /* bound, halved until the store fits beside it.    */
                              /* 0 = auto: 2 slots per state of state_capacity    */
                              /* (auto: for the largest store the device holds)   */
} rmc_config;

/* End-of-run summary.  Replaces TLC's stdout summary lines:
 * "N states generated, M distinct states found, Q states left on queue." and
 * "The depth of the complete state graph search is D." */
typedef struct rmc_result {
    uint64_t generated;        /* init states + every successor of every expanded state */
    uint64_t distinct;         /* distinct (canonical) states found                     */
    uint64_t left_on_queue;    /* frontier states not expanded at stop                  */
    int32_t depth;             /* BFS levels (init = level 1)                           */
    int32_t violated_inv;      /* RMC_INV_* bit of the violated invariant, or 0         */
    int32_t violation_depth;   /* level of the violating state, or 0                    */
    int32_t deadlock;          /* 1 if a state without successors was found             */
    double collision_probability; /* fingerprint collision estimate (TLC prints one too) */
    double seconds;            /* wall time of rmc_run_bfs                              */
    double expand_kernel_seconds; /* device time of the expansion kernels, HIP events on */
                                  /* the ctx stream (sum over levels)                    */
    uint64_t expand_launches;  /* expansion kernel launches (levels are split in chunks) */
    uint64_t probes;           /* fingerprint-set probes (successors that reached the set) */
    uint64_t collisions;       /* RMC_FLAG_VERIFY_STATES: fingerprint hits whose stored state */
                               /* differs (0 = the counts are exact, not probabilistic)   */
    uint64_t verified;         /* RMC_FLAG_VERIFY_STATES: hits compared state by state    */
                               /* (wide layout: every probe is a new state or a compared  */
                               /* hit, verified == probes - (distinct - 1); with           */
                               /* RMC_FLAG_SYMMETRY too, orbit by orbit)                   */
    /* sharded mode (rmc_shard): this rank's exchange */
    uint64_t keys_sent;        /* phase-1 keys sent to other owners                        */
    uint64_t states_sent;      /* phase-2 accepted states shipped                          */
    uint64_t chunks;           /* exchange rounds (frontier chunks and drains of parked keys) */
    double exchange_seconds;   /* device time of the exchange rounds (exchange stream),    */
                               /* overlapped with the next round's expansion or not        */
    uint64_t stored_here;      /* distinct states this rank stores                         */
    /* RMC_FLAG_SPILL */
    uint64_t spilled;          /* states that left the device window (all spills of the run) */
    uint64_t spills;           /* spill events; with the links in HBM (a ring window whose  */
                               /* slots are reused, nothing copied) the passes of the ring  */
    double spill_seconds;      /* wall time of the spills (device-to-host + window shift;   */
                               /* 0 for the ring)                                           */
    /* sharded mode, continued */
    uint64_t parked;           /* keys parked because an owner's outbox was full; sent in   */
                               /* further rounds of the same level (never dropped)          */
    double exchange_wait_seconds; /* host wall time blocked on count read-backs and level ends */
    /* RMC_FLAG_SPILL, continued */
    int32_t spill_links_on_device; /* 1: the trace links (parent, lane) of spilled states stayed */
                                   /* in HBM and the window was a ring; 0: links on the host   */
    int32_t pad2;
    /* RMC_FLAG_VERIFY_STATES with RMC_FLAG_SPILL */
    uint64_t verified_spilled; /* hits (of `verified`) whose stored state had left the device */
                               /* window, compared with its host copy                       */
    uint64_t set_slots;        /* 8-B slots of the fingerprint set this run used (set_bytes) */
} rmc_result;

/* Per-level progress (TLC prints "Progress(D) ... states generated ..."). */
typedef struct rmc_level_stats {
    int32_t level;             /* level just completed (its successors were generated)  */
    int32_t pad;
    uint64_t generated;        /* cumulative generated                                  */
    uint64_t distinct;         /* cumulative distinct                                   */
    uint64_t new_states;       /* distinct states found at level+1                      */
    double seconds;            /* wall time since rmc_run_bfs started                   */
} rmc_level_stats;

/* Return non-zero to stop the search early. */
typedef int (*rmc_progress_fn)(const rmc_level_stats* stats, void* user);

/* A decoded state in neutral form, for traces and tests.  Field meanings are
 * the TLA+ variables of raft.tla:31-67; Nil = -1; roles 0/1/2 =
 * Follower/Candidate/Leader; mtype 0..3 = RequestVoteRequest,
 * RequestVoteResponse, AppendEntriesRequest, AppendEntriesResponse.
 * Fields that do not apply to a message type are 0. */
typedef struct rmc_entry { int32_t term, value; } rmc_entry;
typedef struct rmc_msg_view {
    int32_t mtype, mterm, msource, mdest;
    int32_t mlastLogTerm, mlastLogIndex;                      /* RequestVoteRequest    */
    int32_t mvoteGranted, mlog_len;                           /* RequestVoteResponse   */
    rmc_entry mlog[RMC_VIEW_LOG];
    int32_t mprevLogIndex, mprevLogTerm, mentries_len;        /* AppendEntriesRequest  */
    rmc_entry mentries[1];
    int32_t mcommitIndex;
    int32_t msuccess, mmatchIndex;                            /* AppendEntriesResponse */
    int32_t count;                                            /* bag multiplicity >= 1 */
} rmc_msg_view;
typedef struct rmc_state_view {
    int32_t n_servers, n_msgs;
    int32_t currentTerm[RMC_MAX_SERVERS];
    int32_t state[RMC_MAX_SERVERS];
    int32_t votedFor[RMC_MAX_SERVERS];
    int32_t commitIndex[RMC_MAX_SERVERS];
    int32_t log_len[RMC_MAX_SERVERS];
    rmc_entry log[RMC_MAX_SERVERS][RMC_VIEW_LOG];
    uint32_t votesResponded[RMC_MAX_SERVERS];   /* bitmask over server ids */
    uint32_t votesGranted[RMC_MAX_SERVERS];
    int32_t nextIndex[RMC_MAX_SERVERS][RMC_MAX_SERVERS];
    int32_t matchIndex[RMC_MAX_SERVERS][RMC_MAX_SERVERS];
    rmc_msg_view msgs[RMC_VIEW_MSGS];
} rmc_state_view;

/* One successor produced by rmc_expand (differential tests). */
typedef struct rmc_succ_view {
    uint64_t parent;           /* index into the input array                       */
    int32_t family;            /* 0..9 = Restart .. DropMessage (raft.tla:421-430)  */
    int32_t instance;          /* lane id within the state (DESIGN.md lane table)   */
    int32_t in_constraint;     /* 1 if the successor satisfies the CONSTRAINT       */
    int32_t pad;
    uint64_t fingerprint;
    rmc_state_view state;      /* valid when in_constraint                          */
} rmc_succ_view;

typedef struct rmc_ctx rmc_ctx;

/* ---- lifecycle ----------------------------------------------------------
 * rmc_create replaces TLC's model setup: cfg binding, ASSUME checks
 * (raft.tla:494-503, trivially true for model values), and FPSet/queue
 * allocation.  It validates the config and allocates the device state store,
 * fingerprint table and parent array on `cfg->device`. */
int rmc_create(const rmc_config* cfg, rmc_ctx** out);
void rmc_destroy(rmc_ctx* ctx);
const char* rmc_last_error(const rmc_ctx* ctx);   /* never NULL */
const char* rmc_version(void);                    /* "rmc <abi> gfx950 ..."           */

/* ---- breadth-first search ----------------------------------------------
 * Replaces TLC's BFS worker loop (ModelChecker: dequeue, getNextStates over
 * Next raft.tla:421-430, CONSTRAINT filter, FP64 + FPSet.put, invariant check,
 * enqueue).  Blocks until fixpoint, first violation, deadlock (when checked),
 * max_depth, or the callback asks to stop (RMC_FLAG_CONTINUE: not at a violation). */
int rmc_run_bfs(rmc_ctx* ctx, rmc_progress_fn cb, void* user);
/* Changes rmc_config.seed (fingerprint salt) for the next run on this ctx. */
int rmc_set_seed(rmc_ctx* ctx, uint64_t seed);
int rmc_get_result(const rmc_ctx* ctx, rmc_result* out);
/* Test hook of the verification mode: keep only the low `bits` fingerprint
 * bits (1..64), so collisions happen and must be reported.  Needs
 * RMC_FLAG_VERIFY_STATES. */
int rmc_set_fp_bits(rmc_ctx* ctx, int32_t bits);

/* ---- action coverage (TLC -coverage) ---------------------------------------
 * With RMC_FLAG_COVERAGE the BFS tallies, for every action of Next, how many
 * successors it generated and how many of the stored states it produced: TLC's
 * per-action "distinct:generated" statistics.  The rows, in this fixed order:
 * Init; the seven server families Restart, Timeout, RequestVote, BecomeLeader,
 * ClientRequest, AdvanceCommitIndex, AppendEntries; the five disjuncts of
 * Receive (raft.tla:393-403), which TLC treats as separate actions: UpdateTerm
 * (the message's term is newer than its receiver's) and Receive:<mtype> for
 * the four message types; DuplicateMessage; DropMessage.
 *  - generated[a]: every enabled lane of action a over every expanded state,
 *    the notion of rmc_result.generated (stuttering and out-of-CONSTRAINT
 *    successors count).  Deterministic.
 *  - distinct[a]: the stored states whose producing lane is of action a.  A
 *    state reached by two actions in the same launch is credited to the lane
 *    that won the set insert (TLC with several workers does the same), so a
 *    distinct[a] may differ between runs, between the number of new states
 *    only a reaches and the number a reaches at all.
 *  - row Init: the initial states generated and stored.
 * Whenever rmc_run_bfs returns 0 (fixpoint, max_depth, a callback stop, a
 * violation, a deadlock) the generated[] sum to rmc_result.generated and the
 * distinct[] to rmc_result.distinct.  Every rmc_run_bfs starts from zero
 * tallies.  The counting is a pass of its own after each expansion launch (the
 * expansion kernels are unchanged); without the flag nothing is allocated,
 * launched or read back for it.
 * rmc_get_coverage: RMC_E_STATE on a ctx without the flag or before a run.
 * rmc_coverage_action: the name of a row, for rows 1..14 the key
 * rmc_action_location accepts ("Init" for row 0); NULL out of range.
 * rmc_shard on a ctx with the flag is RMC_E_INVAL, rmc_checkpoint and
 * rmc_recover RMC_E_STATE (the tallies are of whole runs and are not written). */
#define RMC_COV_ACTIONS 15
typedef struct rmc_coverage {
    uint64_t generated[RMC_COV_ACTIONS];
    uint64_t distinct[RMC_COV_ACTIONS];
} rmc_coverage;
int rmc_get_coverage(const rmc_ctx* ctx, rmc_coverage* out);
const char* rmc_coverage_action(int32_t row);

/* ---- continue past violations (TLC -continue) --------------------------------
 * With RMC_FLAG_CONTINUE a violated invariant does not stop rmc_run_bfs: the
 * violating states are stored and expanded like any other, and the run ends at
 * fixpoint, at max_depth, on a callback stop, or on a deadlock (handled as
 * without the flag).  rmc_result's generated, distinct, depth, left_on_queue and
 * the level callbacks are those of the same model with no violated invariant in
 * its mask; violated_inv and violation_depth are what the run without the flag
 * reports — the first level with a violation and its least index — and
 * rmc_trace traces to that state.
 * rmc_get_violations: the tallies over every stored state, all deterministic
 * (the set of stored states is; under SYMMETRY the predicates are
 * permutation-invariant, so whichever member of an orbit is stored counts the
 * same).  RMC_E_STATE on a ctx without the flag or before a run; every
 * rmc_run_bfs starts from zero tallies.
 * rmc_trace_violation: rmc_trace to the least-index stored state that violates
 * `inv_bit` — one RMC_INV_* bit of the ctx's mask — checked alone: *len is
 * depth[r] and the last state violates that invariant (which state it is may
 * differ between runs; its depth does not).  RMC_E_STATE when each[r] == 0,
 * RMC_E_INVAL for a bit outside the mask.
 * The counting is a pass of its own after each expansion launch (the expansion
 * kernels are unchanged); without the flag nothing is allocated, launched or
 * read back for it.  Packed layout: resident, RMC_FLAG_SPILL (both windows),
 * SYMMETRY, RMC_FLAG_VERIFY_STATES, RMC_FLAG_COVERAGE.  Wide layout: resident
 * only (SYMMETRY, RMC_FLAG_VERIFY_STATES and RMC_FLAG_COVERAGE included) — with
 * RMC_FLAG_SPILL rmc_create is RMC_E_INVAL (the ring does not store
 * the last level of a max_depth run, so no pass can read it).  rmc_shard on a
 * ctx with the flag is RMC_E_INVAL, rmc_checkpoint and rmc_recover RMC_E_STATE
 * (the tallies are of whole runs and are not written). */
#define RMC_INV_COUNT 10
typedef struct rmc_violations {
    uint64_t states;                /* stored states violating at least one invariant of the mask */
    uint64_t first[RMC_INV_COUNT];  /* ... whose first violated invariant (lowest bit; the notion of
                                       rmc_result.violated_inv / rmc_check_states) is bit r: sums to states */
    uint64_t each[RMC_INV_COUNT];   /* ... that violate invariant r checked alone (each[r] >= first[r]) */
    int32_t  depth[RMC_INV_COUNT];  /* level of the shallowest state violating r alone; 0 = none */
} rmc_violations;
int rmc_get_violations(const rmc_ctx* ctx, rmc_violations* out);
int rmc_trace_violation(rmc_ctx* ctx, uint32_t inv_bit, rmc_state_view* states, int32_t* families,
                        int32_t* instances, size_t cap, size_t* len);

/* Counterexample: the states from an initial state to the violating (or
 * deadlocked) state, in order, with the action family and lane of the step
 * into each state (-1 for the initial state).  Replaces TLC's trace
 * reconstruction from the states/ trace file ("State 1: ... State d").
 * *len receives the trace length even if it exceeds cap. */
int rmc_trace(rmc_ctx* ctx, rmc_state_view* states, int32_t* families, int32_t* instances,
              size_t cap, size_t* len);

/* ---- checkpoint / recovery (TLC -checkpoint / -recover) ----------------------
 * rmc_checkpoint: after rmc_run_bfs stopped at a level boundary (max_depth or
 * the progress callback), write the stored levels (states, parent refs, lanes),
 * the level table and the counters to `path`.  rmc_recover: on a ctx of the
 * same model (constants, bounds, flags, seed; capacity >= the checkpoint's
 * states), load them and rebuild the fingerprint set from the states; the next
 * rmc_run_bfs continues from the first unexpanded level, with cumulative
 * counts.  A sharded ctx (rmc_shard) writes and reads its own part,
 * <path>.rank<r>; every rank of the same world calls them, and the recovered
 * ctxs must be sharded the same way (rank, world) before rmc_recover. */
int rmc_checkpoint(rmc_ctx* ctx, const char* path);
int rmc_recover(rmc_ctx* ctx, const char* path);

/* ---- codec and successor enumeration (tests, Java driver printing) -------
 * rmc_state_bytes: bytes of one stored state for this config (packed, or the
 * wide layout's BFS store record: 336 B depth-sized, 904 B compact or 5,080 B;
 * with RMC_FLAG_SPILL and max_depth the record of the last stored level).
 * rmc_expand: run the SAME device successor code as the BFS on n caller
 * states (no dedup) and return every enabled lane's successor.  *n_out
 * receives the number of successors even if it exceeds cap.  Under
 * RMC_FLAG_SYMMETRY rmc_succ_view.fingerprint is the canonical key of the
 * successor's orbit (both layouts), the state returned is the successor itself. */
size_t rmc_state_bytes(const rmc_config* cfg);
int rmc_expand(rmc_ctx* ctx, const rmc_state_view* states, size_t n, rmc_succ_view* out,
               size_t cap, size_t* n_out);
/* Test hook: evaluate the SAME device invariant code as the BFS / simulator on n
 * caller states.  invariants = RMC_INV_* mask for this call (0 = the ctx's own).
 * violated[t] = 0, or the RMC_INV_* bit of the first violated invariant of state
 * t (the notion of rmc_result.violated_inv: the lowest bit of the mask that
 * fails).  The states need not be reachable, nor within the CONSTRAINT; a view
 * the layout's encoder refuses, a mask bit above RMC_INV_LEADER_COMPLETE or a
 * NULL array with n > 0 is RMC_E_INVAL with the reason; n = 0 launches nothing.
 * On the wide layout RMC_WSIM (read at each call) picks the check as it picks
 * the simulation kernel: 1 (default) the one-wave-per-state check, 0 the
 * one-thread-per-state check the BFS uses. */
int rmc_check_states(rmc_ctx* ctx, const rmc_state_view* states, size_t n, uint32_t invariants,
                     int32_t* violated);
/* Test hook: keys[t] = the 64-bit key (Fp.k) the search would insert for state t:
 * state_fp, under RMC_FLAG_SYMMETRY canon_state — the same device function k_seed,
 * k_rehash and k_publish call; on a wide ctx under RMC_FLAG_SYMMETRY wcanon, as
 * k_wseed and k_wexpand insert it.  ref != NULL: same[t] = 1 iff verification's
 * comparison (same_state; under SYMMETRY same_orbit, on a wide ctx wsame_orbit)
 * finds state t equal to the stored form of state ref[t] (ref[t] < n).
 * RMC_E_INVAL on a wide ctx without RMC_FLAG_SYMMETRY (as before ABI 13), for a
 * view the encoder refuses, a NULL array with n > 0, or ref[t] >= n; n = 0
 * launches nothing. */
int rmc_state_keys(rmc_ctx* ctx, const rmc_state_view* states, size_t n, uint64_t* keys,
                   const uint32_t* ref, uint8_t* same);

/* ---- state graph export (TLC -dump FILE, -dump dot,actionlabels FILE) -----------
 * After a completed rmc_run_bfs the ctx holds the whole state graph in HBM: the
 * stored states in level order, and the fingerprint set that tells which stored
 * state a successor is.  These calls read it.  Packed layout, single GPU,
 * resident store; with RMC_FLAG_SYMMETRY (the nodes are the stored orbit
 * representatives), RMC_FLAG_VERIFY_STATES, RMC_FLAG_COVERAGE, RMC_FLAG_CONTINUE.
 *
 * rmc_get_levels (both layouts): starts[l] = the store index of the first state
 * of level l + 1, the last entry = rmc_result.distinct; *n receives the number
 * of entries (depth + 1) even if it exceeds cap.
 * rmc_read_states: the stored states [first, first + n) decoded, and (keys !=
 * NULL) the 64-bit key the search inserted for each: rmc_state_keys' notion,
 * state_fp, canon_state under RMC_FLAG_SYMMETRY.
 * rmc_find_states: index[t] = the store index of the stored state that holds
 * caller state t's key, or RMC_NO_STATE.  Under RMC_FLAG_SYMMETRY any member of
 * an orbit finds the stored representative.
 * rmc_graph_edges: every edge out of the stored states [lo, hi).
 *  - A source has edges only if the run expanded it: the indices below
 *    distinct - left_on_queue.  The states of an unexpanded last level (max_depth,
 *    a callback stop) have none, as in TLC's dump of a stopped run.
 *  - An expanded source yields one edge per enabled lane whose successor
 *    satisfies the CONSTRAINT; stuttering lanes included (dst = the source
 *    itself; under SYMMETRY the stored representative of its orbit, which is the
 *    source); two lanes that reach the same state give two edges.
 *  - family and instance are rmc_succ_view's.
 *  - dst = the index of the stored state that holds the successor's key, looked
 *    up exactly as the search computes it (rmc_set_fp_bits, the salt of
 *    rmc_config.seed and the set's epoch tag all apply; under SYMMETRY the
 *    canonical key).  An edge whose key the set does not hold is an engine
 *    error: RMC_E_HIP naming the source index and the lane, never dropped.
 *  - Order: ascending src, then ascending instance, the same at every call.
 *  - *n_out receives the number of edges even if it exceeds cap; a range of any
 *    size is served in internal chunks; lo == hi launches nothing.
 * The lookup is a slot -> store index array of 8 B per fingerprint-set slot: a
 * ctx with RMC_FLAG_VERIFY_STATES has it; any other ctx allocates it at its first
 * rmc_find_states / rmc_graph_edges (RMC_E_NOMEM if it does not fit beside the
 * store and the set: give rmc_config.state_capacity or set_bytes) and fills it
 * with one pass over the stored states; rmc_destroy frees it; the next
 * rmc_run_bfs invalidates it.
 * Refusals (each with a message): a NULL ctx, or a NULL array with n > 0 (cap >
 * 0), is RMC_E_INVAL; a range beyond rmc_result.distinct and a view the encoder
 * refuses are RMC_E_INVAL; RMC_E_STATE: before a completed rmc_run_bfs; after
 * rmc_recover and before the next run; on a sharded ctx (rmc_shard); on a ctx
 * created with RMC_FLAG_SPILL (the states must be resident); on a wide ctx, for
 * all but rmc_get_levels; and rmc_graph_edges after a run that stopped at a
 * violation or a deadlock (which states it expanded is then not a level
 * boundary: search with RMC_FLAG_CONTINUE; the other three calls still work). */
#define RMC_NO_STATE UINT64_MAX
typedef struct rmc_edge {
    uint64_t src, dst;         /* store indices                                    */
    int32_t family, instance;  /* rmc_succ_view's                                  */
} rmc_edge;                    /* 24 B */
int rmc_get_levels(const rmc_ctx* ctx, uint64_t* starts, size_t cap, size_t* n);
int rmc_read_states(rmc_ctx* ctx, uint64_t first, size_t n, rmc_state_view* states, uint64_t* keys);
int rmc_find_states(rmc_ctx* ctx, const rmc_state_view* states, size_t n, uint64_t* index);
int rmc_graph_edges(rmc_ctx* ctx, uint64_t lo, uint64_t hi, rmc_edge* out, size_t cap, size_t* n_out);

/* ---- simulation (TLC -simulate; Smokeraft.cfg, config 4) ---------------------
 * Replaces TLC's Simulator: random behaviours, each from a random initial state
 * and then a uniformly random enabled successor per step, invariants checked on
 * every state.  smoke_k > 0 draws the initial states like SmokeInit
 * (Smokeraft.tla:64-76: one RandomSubset(k, .) per variable, k^9 states, over
 * SmokeNat = 0..smoke_nat, SmokeInt = -1..1, BoundedSeq(.,3)/(.,1) logs);
 * smoke_k = 0 starts from Init.  TLC's StopAfter (a 1-s budget,
 * Smokeraft.tla:88-92) is replaced by an explicit behaviour count.  Walks stay
 * within the config's bounds (max_term, max_log_len, max_msgs, max_dup: the
 * model's CONSTRAINT, or the packed capacity when it has none — the front-end
 * fills them in): RMC_SIM_WITHIN_CAPACITY draws each step uniformly among the
 * enabled successors within them (so behaviours run to `depth`);
 * RMC_SIM_TRUNCATE draws among all enabled successors and a draw beyond them
 * ends that behaviour (counted in `truncated`). */
#define RMC_SIM_WITHIN_CAPACITY 0
#define RMC_SIM_TRUNCATE 1
/* TLC's draw (its simulator's action choice, restated): Next's actions — each
 * instance of Restart .. AppendEntries (\E over the constant Server/Value sets
 * expands into one action each; the sets are the model's, so ClientRequest has
 * n_servers * n_values actions), Receive, DuplicateMessage and DropMessage
 * (\E m \in DOMAIN messages ranges over the state) one action each — are
 * visited from a uniformly random index with a random prime stride (primes
 * above the action count, so every action is visited); the first one with a
 * successor is taken and one of its successors drawn uniformly.  Not uniform
 * over the enabled actions: an action after a run of disabled ones is likelier.
 * Beyond the bounds it ends the behaviour like RMC_SIM_TRUNCATE.  Wide layout
 * only (rmc_simulate refuses it on the packed one). */
#define RMC_SIM_TLC 2
typedef struct rmc_sim_config {
    uint64_t behaviours;       /* random behaviours to run                        */
    int32_t depth;             /* states per behaviour (TLC -depth, default 100)  */
    int32_t smoke_k;           /* SmokeInit RandomSubset size k; 0 = Init         */
    int32_t smoke_nat;         /* SmokeNat = 0..smoke_nat (default 2)             */
    int32_t mode;              /* RMC_SIM_WITHIN_CAPACITY (0) or RMC_SIM_TRUNCATE */
    uint64_t seed;             /* RNG seed for the SmokeInit draws and the walks  */
} rmc_sim_config;
typedef struct rmc_sim_result {
    uint64_t behaviours, steps, init_states, truncated, deadlocked;
    int32_t violated_inv;      /* RMC_INV_* bit of the first violation, or 0      */
    int32_t violation_depth;   /* its state index in the behaviour (1 = initial)  */
    uint64_t violation_behaviour;
    double seconds;            /* wall time incl. the SmokeInit draw              */
    double kernel_seconds;     /* device time of the walks (HIP events)           */
} rmc_sim_result;
int rmc_simulate(rmc_ctx* ctx, const rmc_sim_config* sc, rmc_sim_result* out);
/* The initial states rmc_simulate draws for sc (SmokeInit, sc->smoke_k >= 1):
 * host-only, no device needed.  *n receives k^9 even if it exceeds cap. */
int rmc_smoke_init(const rmc_config* cfg, const rmc_sim_config* sc, rmc_state_view* states,
                   size_t cap, size_t* n);
/* Re-runs behaviour `behaviour` of the same rmc_sim_config and returns its states. */
int rmc_sim_replay(rmc_ctx* ctx, const rmc_sim_config* sc, uint64_t behaviour, rmc_state_view* states,
                   size_t cap, size_t* len);

/* ---- sharded BFS over several GPUs (one process or thread per GPU) ---------
 * Replaces TLC's distributed mode (TLCServer/TLCWorker with a partitioned
 * FPSet).  rmc_shard turns a ctx into rank `rank`
 * of `world`; rmc_run_bfs, rmc_get_result and rmc_trace then become
 * collectives that every rank calls, and return the GLOBAL result on every
 * rank.  A state is owned by the rank given by a hash of its servers 0 and 1
 * words (RMC_OWNER=2, default; 1: server 0 only; 0: by fingerprint, always
 * under SYMMETRY); each rank stores and expands the states it owns.
 * A level is expanded in rounds; each round's exchange is fingerprint-first
 * (two phases):
 *   1. a successor owned elsewhere (and not in this rank's lossy sent-cache)
 *      sends only its 8-byte key; the owner inserts the keys it receives
 *      into its fingerprint set and answers new / seen (1 byte per key);
 *   2. for the keys answered "new" the sender re-derives the successor and
 *      ships the state and its global parent ref ((rank << 48) | index, lane
 *      in bits 40-47); the owner stores it for the next level.
 * Rounds are pipelined: the next round's expansion runs while this round's
 * exchange is on the wire (two outbox sets, an exchange stream).  Per round
 * the host reads back two small count rows; one all-gather of the device
 * counters per level combines the level statistics.  A key whose owner's
 * outbox is full is parked and sent in a further round of the same level.
 * Replicated levels: a level of at most RMC_DIST_REP states (default 2^20) is
 * gathered whole on every rank (one all-gather of state records) and every
 * rank expands all of it, probing and storing only the successors it owns —
 * no key or state exchange for the small levels at either end of the search.
 * Deadlines: every collective and the communicator set-up run under
 * RMC_DIST_TIMEOUT_S (default 300 s; the RCCL communicator is non-blocking and
 * aborted on expiry, host-transport callbacks are expected to honour it too):
 * a stalled rank makes every other rank's rmc_run_bfs return RMC_E_HIP naming
 * the level, round and phase.
 * Transport: RCCL over xGMI (rccl_id = an id from rmc_rccl_unique_id on rank
 * 0, given to every rank; host = NULL), or a caller-supplied host transport
 * (rccl_id = NULL) whose callbacks move host buffers: alltoallv sends
 * send_bytes[d] bytes to rank d (blocks back to back in `send`) and receives
 * recv_bytes[s] from rank s (back to back in `recv`); allgather gathers
 * `bytes` from every rank into recv (rank order).  They return 0 on success.
 * keys_per_dest bounds the keys one round sends to one owner (0 = auto);
 * sent_cache_slots sizes the sent-cache (0 = auto).  Full-state verification
 * (RMC_FLAG_VERIFY_STATES) ships every remote successor and compares the ones
 * the owner had seen; checkpoints are per rank; RMC_FLAG_SPILL is single-GPU. */
typedef struct rmc_transport {
    void* user;
    int (*alltoallv)(void* user, const void* send, const uint64_t* send_bytes, void* recv,
                     const uint64_t* recv_bytes);
    int (*allgather)(void* user, const void* send, uint64_t bytes, void* recv);
} rmc_transport;
int rmc_rccl_unique_id(uint8_t id[128]);
int rmc_shard(rmc_ctx* ctx, int32_t rank, int32_t world, const uint8_t* rccl_id,
              const rmc_transport* host, uint64_t keys_per_dest, uint64_t sent_cache_slots);

/* ---- roofline microbenchmark -----------------------------------------------
 * Random 8-byte accesses into a table of table_bytes on `device`, 8 in flight
 * per thread, the access pattern of the fingerprint set: mode 0 = loads,
 * mode 1 = CAS.  *per_second receives accesses/s (device time, HIP events).
 * This is R_max of SURVEY.md §8d (no TLC analog). */
int rmc_probe_bench(int device, uint64_t table_bytes, uint64_t accesses, int mode, double* per_second);

/* ---- front-end -----------------------------------------------------------
 * Replaces TLC's SANY + cfg reading for this spec: reads a TLC model (root
 * .tla module, the modules it EXTENDS next to it, its .cfg, and raft.tla) and
 * fills *cfg — or refuses it, naming the construct the engine does not
 * compile.  The engine compiles lemmy/raft.tla:1-505 and nothing else, so:
 *  - raft.tla is read (raft_path, else $RMC_RAFT_TLA, else next to the
 *    model) and every top-level unit of its module body must match the
 *    compiled-in text (comments and whitespace normalised).  The one edit
 *    recognised is config 5's weakened quorum guard in BecomeLeader
 *    (raft.tla:197 `votesGranted[i] /= {}`), which sets RMC_FLAG_BUG_QUORUM.
 *    With no raft.tla on disk the call fails unless options has
 *    RMC_FRONT_BUILTIN_RAFT (then the compiled-in text is used, and said so);
 *  - CONSTANTS: model values, `X <- Def`, `Name = n`; Server and Value must
 *    be set literals of distinct model values;
 *  - CONSTRAINT(S): split into top-level conjuncts (bulleted or infix, through
 *    definition references); every conjunct must be one of
 *    `\A i \in Server : currentTerm[i] <= N /\ Len(log[i]) <= N`,
 *    `Cardinality(DOMAIN messages) <= N`, `\A m \in DOMAIN messages :
 *    messages[m] <= N` (<, =<, \leq too); anything else is refused (or, under
 *    RMC_FRONT_CONSTRAINTS, a residual: "model-defined constraints" below);
 *  - INVARIANT(S): TypeOK, or a name from RMC_INV_* whose definition (with the
 *    model definitions it uses) is the compiled-in restatement;
 *  - `BecomeLeader <- Def`: Def must be the compiled-in bug variant;
 *  - SYMMETRY: exactly Permutations(Server) (or of Server's set definition);
 *  - simulation (RMC_FRONT_SIMULATE, TLC -simulate): `Init <- SmokeInit` must
 *    be Smokeraft's sampler (k and SmokeNat are read as its parameters); a
 *    CONSTRAINT that only reads TLCGet/TLCSet is a run budget, replaced by
 *    sim->behaviours; bounds the cfg does not give are the packed capacity.
 *  - an unconstrained field is refused unless options has
 *    RMC_FRONT_DEPTH_BOUNDED (see RMC_FLAG_UNBOUNDED_TERM).
 * On success `info` receives the provenance notes (which raft.tla was
 * verified, which overrides were recognised), on failure the error. */
#define RMC_FRONT_BUILTIN_RAFT (1u << 0)
#define RMC_FRONT_SIMULATE (1u << 1)
/* RMC_FRONT_DEPTH_BOUNDED: the caller bounds the depth (TLC -depth), so a model
 * whose CONSTRAINT leaves fields unbounded — or that has none, as MCraft.cfg
 * as shipped (MCraft.cfg:1-39) — is accepted with the RMC_FLAG_UNBOUNDED_*
 * bits set (rmc_create then requires max_depth > 0). */
#define RMC_FRONT_DEPTH_BOUNDED (1u << 2)
/* RMC_FRONT_PREDICATES: an INVARIANT whose name is not one of the compiled-in ten is
 * accepted (not put in rmc_config.invariants): the caller promises to compile it with
 * rmc_predicates_from_files and hand it to the ctx with rmc_set_predicates.  The ten
 * known names keep their digest rule. */
#define RMC_FRONT_PREDICATES (1u << 3)
int rmc_model_from_files(const char* cfg_path, const char* tla_path, const char* raft_path,
                         uint32_t options, rmc_config* cfg, rmc_sim_config* sim,
                         char* info, size_t info_cap);
/* ---- model-defined invariants ------------------------------------------------------
 * A state predicate the model defines and its .cfg names under INVARIANT, other than
 * the ten compiled-in ones, is compiled by the front-end to a small bytecode program
 * and evaluated by a pass of its own on every state the BFS stores (after the seed and
 * after each expansion launch; the expansion kernels and the fused check are unchanged;
 * without predicates nothing is allocated, launched or read back for them).
 *
 * The language (DESIGN.md "Model-defined invariants" has the grammar): a typed subset
 * of TLA+ over raft.tla's variables in which every value is a 32-bit integer —
 * Booleans, naturals, servers (Nil = -1), roles, message types, sets of servers.
 * Atoms: integers, TRUE, FALSE, Nil, Follower, Candidate, Leader, the four message
 * types, the cfg's integer constants, server model values, Server, Quorum (to the right
 * of \in or as a quantifier's domain).  State reads: currentTerm[e], state[e],
 * votedFor[e], commitIndex[e], votesResponded[e], votesGranted[e], nextIndex[e][e],
 * matchIndex[e][e], Len(log[e]), LastTerm(log[e]), log[e][n].term, log[e][n].value,
 * messages[m], and the scalar fields of a bound message m.  Operators: /\ \/ ~ => <=>
 * (infix and as bulleted lists), = /= # < <= =< \leq > >= \geq, + -, IF THEN ELSE, \in,
 * \notin, {a, b}, {x \in D : P}, \cup \cap \ \subseteq, Cardinality.  Quantifiers \A \E
 * over Server, a server-set expression, Quorum, a..b, DOMAIN log[e], DOMAIN messages.
 * The model's own operator definitions are expanded in place (no recursion).  Everything
 * else is refused when compiled, with the construct, its line and column.
 * Evaluation is left to right with short circuit, as in TLC; a read outside a domain is
 * an evaluation error, as in TLC.  A verdict is 0 (holds), 1 (violated), 2 (error).
 *
 * rmc_predicates_from_files: rmc_model_from_files' arguments (options without
 * RMC_FRONT_PREDICATES too); compiles exactly the INVARIANTs rmc_model_from_files would
 * accept only under RMC_FRONT_PREDICATES, in cfg order, at most RMC_MAX_PREDICATES (1024
 * code words, stack depth 16, 8 bound names: more is refused with the count).  A model
 * with none gives a program of count 0.  RMC_E_PARSE with the message in err.
 * rmc_set_predicates copies the program into the ctx (NULL, or a program of count 0,
 * removes it).  rmc_run_bfs then reports a violated predicate p like a built-in
 * invariant: violated_inv = RMC_INV_USER0 << p, violation_depth, rmc_trace; the level is
 * finished first, the least store index wins over the fused check's and the pass's, at
 * equal index the built-in; rmc_predicate_error tells a violation from an evaluation
 * error.  Counts of a run whose predicates hold equal the run without them.
 * Single GPU; packed layout resident and with RMC_FLAG_SPILL; wide layout resident; with
 * RMC_FLAG_SYMMETRY, RMC_FLAG_VERIFY_STATES, RMC_FLAG_COVERAGE.  RMC_E_INVAL: a ctx with
 * RMC_FLAG_CONTINUE (its tallies have ten rows), a sharded ctx (and rmc_shard after
 * predicates are set), a wide ctx with RMC_FLAG_SPILL (the unstored last level), under
 * RMC_FLAG_SYMMETRY a predicate that names a server model value, a program compiled
 * for another n_servers.  With predicates set rmc_simulate, rmc_checkpoint and
 * rmc_recover are RMC_E_STATE.
 * rmc_eval_predicates (test hook): the same device interpreter on n caller states,
 * verdicts[t * count + p] for every predicate, none skipped. */
#define RMC_MAX_PREDICATES 8
#define RMC_INV_USER0 (1u << 16)      /* predicate p is bit 16 + p of rmc_result.violated_inv */
typedef struct rmc_predicates rmc_predicates;
int rmc_predicates_from_files(const char* cfg_path, const char* tla_path, const char* raft_path,
                              uint32_t options, rmc_predicates** out, char* err, size_t err_cap);
void rmc_predicates_free(rmc_predicates* p);
int rmc_predicates_count(const rmc_predicates* p);
const char* rmc_predicates_name(const rmc_predicates* p, int index);
int rmc_set_predicates(rmc_ctx* ctx, const rmc_predicates* p);
int rmc_eval_predicates(rmc_ctx* ctx, const rmc_state_view* states, size_t n, uint8_t* verdicts);
int rmc_predicate_error(const rmc_ctx* ctx);  /* 1 if the reported violation is an evaluation error */

/* ---- model-defined constraints -----------------------------------------------------
 * RMC_FRONT_CONSTRAINTS: a top-level conjunct of a CONSTRAINT that is none of the four
 * bounds is not refused but recorded as a *residual* (a note line names each one): the
 * caller promises to compile the residuals with rmc_constraints_from_files and hand them
 * to the ctx with rmc_set_constraints.  The recognised bounds stay bounds (they size the
 * packed layout and run inside the expansion kernel), and a model must still bound all
 * four fields.  Without the option every refusal stays as it is.
 *
 * A residual is a state predicate in the language of the model-defined invariants above,
 * compiled to the same program format with the same limits and the same refusals with
 * line and column.  The residuals of all CONSTRAINT names, in order, are one program;
 * residual r carries the name of the CONSTRAINT of the .cfg it came from.
 *
 * Semantics (TLC's): a successor that fails a residual counts in rmc_result.generated
 * and nowhere else: it is not stored, not counted in distinct, not expanded, not left on
 * the queue and never reported by an invariant, built-in or model-defined; its
 * fingerprint stays in the set, so later copies are dropped as duplicates.  A level
 * whose states are all filtered adds nothing to depth.  An initial state that fails
 * gives distinct 0, generated 1, depth 0.  The filter is a pass of its own after the
 * seed and after every expansion launch (the expansion kernels are unchanged; they run
 * with the fused invariant check off and without commuting-diamond skipping, and the
 * built-in invariants are checked by a pass over the kept states); without constraints
 * nothing is allocated, launched or read back for them.
 * An evaluation error in a residual (verdict 2) keeps the state and stops the search at
 * the end of its level: rmc_run_bfs returns 0, rmc_constraint_error is 1 + the
 * residual's index (0: none) and rmc_trace leads to the state.
 *
 * rmc_constraints_from_files: rmc_model_from_files' arguments; the residuals as an
 * rmc_predicates (rmc_predicates_count / _name / _free apply); count 0: the model has
 * none.  rmc_set_constraints copies the program into the ctx (NULL or count 0 removes
 * it).  Single GPU, packed layout, resident store.  RMC_E_INVAL, each named with its
 * reason: RMC_FLAG_VERIFY_STATES (a removed state's set slot never gets an owner),
 * RMC_FLAG_CONTINUE, RMC_FLAG_COVERAGE, RMC_FLAG_SPILL, a wide ctx, a sharded ctx (and
 * rmc_shard after constraints are set), under RMC_FLAG_SYMMETRY a residual that names a
 * server model value, a program compiled for another n_servers; RMC_E_STATE on a ctx
 * with a checkpoint loaded (rmc_recover rebuilt its set from the stored states).  With
 * constraints set rmc_simulate, rmc_checkpoint and rmc_recover are RMC_E_STATE, and after
 * a run with constraints rmc_graph_edges and rmc_find_states are (that run's set holds
 * keys without a stored state, whether or not the constraints are still set);
 * rmc_get_levels and rmc_read_states show the kept states only. */
#define RMC_FRONT_CONSTRAINTS (1u << 4)
int rmc_constraints_from_files(const char* cfg_path, const char* tla_path, const char* raft_path,
                               uint32_t options, rmc_predicates** out, char* err, size_t err_cap);
int rmc_set_constraints(rmc_ctx* ctx, const rmc_predicates* p);
int rmc_constraint_error(const rmc_ctx* ctx);  /* 1 + the residual whose evaluation failed, 0: none */

/* ---- action properties ------------------------------------------------------------------
 * RMC_FRONT_ACTIONS: a PROPERTY / PROPERTIES name whose definition is [][A]_vars (the
 * subscript exactly raft.tla's vars) is accepted: a safety property of every transition,
 * as TLC checks it, with no liveness machinery.  Without the option every PROPERTY stays
 * refused; every other temporal form (<>, ~>, WF_, SF_, []P of a state predicate, a
 * conjunction of temporal formulas) is refused by name with or without it.
 *
 * A is an expression of the predicate language above plus primes: a primed variable
 * wherever a state read is accepted (currentTerm'[i], Len(log'[i]), log'[i][n].term,
 * DOMAIN messages', messages'[m], ...), and a primed parenthesised expression or use of a
 * definition of the model ((e)', Name', Name(args)'), which primes every variable read
 * inside; a prime inside a primed expression is refused.  A bound message belongs to the
 * bag it was bound in (\A m \in DOMAIN messages' binds slots of the successor's bag); using
 * it to index the other state's bag is refused.  UNCHANGED, ENABLED, \cdot, EXCEPT and
 * sequence or record equality (log' = log) are refused by name.  At most
 * RMC_MAX_ACTION_PROPS properties, sharing the predicates' code, stack and bound-name limits.
 *
 * rmc_actions_from_files: rmc_model_from_files' arguments; the action properties in cfg
 * order as an rmc_predicates (rmc_predicates_count / _name / _free apply); count 0: none.
 * rmc_set_actions copies the program into the ctx (NULL or count 0 removes it).
 * rmc_run_bfs then evaluates every property, after each expansion launch, on every
 * transition (s, t) of the launch's parents that the state graph counts as an edge: the
 * lane is enabled and t satisfies the CONSTRAINT's bounds (stuttering ones included).
 * [A]_vars is A \/ UNCHANGED vars: "violated" on a transition with t = s is "holds"; an
 * evaluation error stays an error.  The level is finished first; an invariant (built-in
 * or model-defined) violated in the same level is reported as without properties;
 * otherwise the least (source index, lane, property): violated_inv = RMC_ACT_USER0 << p,
 * violation_depth = the source's level + 1 (the trace's length), rmc_trace = the path to
 * the source plus the successor (recomputed from the stored source) as the last state
 * under its family and lane, rmc_action_violation the details.  Counts of a run whose
 * properties hold equal the run without them; without properties nothing is allocated,
 * launched or read back.  Single GPU, packed layout; with RMC_FLAG_SPILL, SYMMETRY (stored
 * representatives to raw successors), VERIFY_STATES, COVERAGE and model-defined invariants.
 * RMC_E_INVAL: a wide ctx, a sharded ctx (and rmc_shard afterwards), RMC_FLAG_CONTINUE,
 * constraints set (in either order), under SYMMETRY a property that names a server model
 * value, a program compiled for another n_servers.  With properties set rmc_simulate,
 * rmc_checkpoint and rmc_recover are RMC_E_STATE.
 * rmc_eval_actions (test hook): the same device interpreter on n caller pairs (cur[t],
 * next[t]), verdicts[t * count + p] for every property with the stutter rule applied.
 * rmc_action_violation: RMC_E_STATE when the last run reported no action property. */
#define RMC_FRONT_ACTIONS (1u << 5)
#define RMC_MAX_ACTION_PROPS 4
#define RMC_ACT_USER0 (1u << 24) /* property p is bit 24 + p of rmc_result.violated_inv */
int rmc_actions_from_files(const char* cfg_path, const char* tla_path, const char* raft_path,
                           uint32_t options, rmc_predicates** out, char* err, size_t err_cap);
int rmc_set_actions(rmc_ctx* ctx, const rmc_predicates* p);
int rmc_eval_actions(rmc_ctx* ctx, const rmc_state_view* cur, const rmc_state_view* next, size_t n,
                     uint8_t* verdicts);
int rmc_action_violation(const rmc_ctx* ctx, int32_t* property, uint64_t* src_index, int32_t* family,
                         int32_t* instance, int32_t* is_error);

/* rmc_model_from_files for BFS / simulation models with raft_path = NULL and
 * RMC_FRONT_BUILTIN_RAFT taken from the environment (RMC_BUILTIN_RAFT=1).
 * `tla_path` may be NULL (the module next to cfg_path with the same stem). */
int rmc_config_from_files(const char* cfg_path, const char* tla_path, rmc_config* cfg,
                          char* err, size_t err_cap);
int rmc_sim_config_from_files(const char* cfg_path, const char* tla_path, rmc_config* cfg,
                              rmc_sim_config* sim, char* err, size_t err_cap);
/* TLC's location of an action of Next in raft.tla, as its counterexample
 * headers print it (`State k: <Action line L1, col C1 to line L2, col C2 of
 * module raft>`): the body of the action's definition.  `action` is a family
 * name of rmc.h's lane table, "UpdateTerm", or "Receive:<mtype>" for the
 * Receive disjunct of that message type (raft.tla:393-403); "Init" gives the
 * initial predicate's body (raft.tla:125-129).  out4 = L1, C1, L2, C2. */
int rmc_action_location(const char* action, int32_t* out4);

#ifdef __cplusplus
}
#endif
#endif /* RMC_H_ */
