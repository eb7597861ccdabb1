// rmc_wide.cpp — host side of the wide layout (raft_wide.h, rmc_wide.hip):
// the BFS level loop, the counterexample walk, the successor listing and the
// random walks (the codec of the wide record is rmc_codec.cpp).  A
// ctx is wide when some bound of its config exceeds the packed capacity
// (rmc.h RMC_WIDE_MAX_*), e.g. the unbounded fields of MCraft.cfg as shipped
// under a depth bound, or Smokeraft's walks; RMC_FORCE_WIDE=1 forces it on a
// packed-size model (tests compare the two layouts on the same model).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "rmc_ctx.h"
#include "rmc_wide_plan.h"

using namespace rmc;
using namespace rmc::wide;

namespace rmc_host {

bool wide_wanted(const rmc_config& g) {
    if (const char* e = getenv("RMC_FORCE_WIDE"))
        if (atoi(e)) return true;
    return g.max_term > RMC_MAX_TERM || g.max_log_len > RMC_MAX_LOG || g.max_msgs > RMC_MAX_MSGS ||
           g.max_dup > RMC_MAX_DUP;
}

int validate_wide(const rmc_config* c, std::string* why) {
    auto bad = [&](const char* s) { *why = s; return RMC_E_INVAL; };
    static_assert(wide::LW == RMC_WIDE_MAX_LOG && wide::KW == RMC_WIDE_MAX_MSGS && wide::TMAX == RMC_WIDE_MAX_TERM &&
                      wide::CMAX == RMC_WIDE_MAX_DUP && RMC_VIEW_LOG >= wide::LW && RMC_VIEW_MSGS >= wide::KW,
                  "the wide layout's capacity is rmc.h's RMC_WIDE_MAX_*");
    if (c->max_term < 1 || c->max_term > RMC_WIDE_MAX_TERM) return bad("max_term must be 1..255 (wide layout)");
    if (c->max_log_len < 0 || c->max_log_len > RMC_WIDE_MAX_LOG) return bad("max_log_len must be 0..32 (wide layout)");
    if (c->max_msgs < 0 || c->max_msgs > RMC_WIDE_MAX_MSGS) return bad("max_msgs must be 0..64 (wide layout)");
    if (c->max_dup < 1 || c->max_dup > RMC_WIDE_MAX_DUP) return bad("max_dup must be 1..255 (wide layout)");
    // SYMMETRY on this layout: runs under a depth bound (the reference's MCraft.cfg as
    // shipped under -depth, what it was built for) and RMC_FORCE_WIDE runs; a model whose
    // CONSTRAINT exceeds the packed capacity searched to fixpoint stays refused, as before
    if ((c->flags & RMC_FLAG_SYMMETRY) && c->max_depth <= 0 &&
        (c->max_term > RMC_MAX_TERM || c->max_log_len > RMC_MAX_LOG || c->max_msgs > RMC_MAX_MSGS ||
         c->max_dup > RMC_MAX_DUP))
        return bad("the wide layout (bounds beyond the packed capacity) supports SYMMETRY only under a depth "
                   "bound (max_depth > 0)");
    // verification compares a hit with its owner's resident record, found through 8 B
    // more per set slot; at the depths that need the ring that array no longer fits
    // beside the set and the window (DESIGN.md "Wide state")
    if ((c->flags & RMC_FLAG_VERIFY_STATES) && (c->flags & RMC_FLAG_SPILL))
        return bad("the wide layout (bounds beyond the packed capacity) supports RMC_FLAG_VERIFY_STATES only "
                   "without RMC_FLAG_SPILL: verification needs every state resident");
    // the ring does not store the last level of a max_depth run, so no pass can read it
    if ((c->flags & RMC_FLAG_CONTINUE) && (c->flags & RMC_FLAG_SPILL))
        return bad("the wide layout (bounds beyond the packed capacity) supports RMC_FLAG_CONTINUE only "
                   "without RMC_FLAG_SPILL: the violation pass reads every stored state, and the ring "
                   "stores no record of a depth-bounded run's last level");
    return 0;
}

void fill_wide_model(rmc_ctx* c) {
    const rmc_config& g = c->cfg;
    WModel& M = c->WM;
    M.S = g.n_servers;
    M.V = g.n_values;
    M.max_term = g.max_term;
    M.max_log = g.max_log_len;
    M.max_msgs = g.max_msgs;
    M.max_dup = g.max_dup;
    M.unbounded = (int)((g.flags >> 5) & 15u);
    M.bug_quorum = (g.flags & RMC_FLAG_BUG_QUORUM) ? 1 : 0;
    M.inv_mask = (int)g.invariants;
    M.L.init(M.S);
}

// The BFS store's record (WideBufs.compact): the smallest that no state of the
// run can outgrow — each field either bounded by a CONSTRAINT within the record
// (a successor beyond it is out of the model anyway) or unbounded in a run of
// few enough levels.  2: the depth-sized WStateD (4 entries, 12 messages; after
// n steps a log holds at most n - 9 entries, n - 5 under the weakened quorum,
// and the bag at most n - 1 messages: raft_wide.h), 1: the compact WStateC (16,
// 16; one step adds at most one entry and one message), 0: the full WState.
// RMC_WIDE_COMPACT=0/1/2 overrides (A/B, tests).
static int record_for(const rmc_config& g, int steps) {
    const bool blog = (g.flags & RMC_FLAG_UNBOUNDED_LOG) == 0, bmsg = (g.flags & RMC_FLAG_UNBOUNDED_MSGS) == 0;
    const int lead = (g.flags & RMC_FLAG_BUG_QUORUM) ? 5 : 9;  // steps before a first log entry can exist
    if (((blog && g.max_log_len <= LWD) || steps - lead <= LWD) && ((bmsg && g.max_msgs <= KWD) || steps - 1 <= KWD))
        return 2;
    const bool logs = (blog && g.max_log_len <= LWC) || steps <= LWC;
    const bool msgs = (bmsg && g.max_msgs <= KWC) || steps <= KWC;
    return logs && msgs ? 1 : 0;
}
// With RMC_FLAG_SPILL (the ring window) a depth-bounded run never stores its
// last level — it is never expanded — so the stored states are at most
// max_depth - 2 steps from Init, one step fewer than above, and the expansion
// works on a second, possibly larger record (WideBufs.work) that holds the
// last level's states, max_depth - 1 steps: MCraft.cfg as shipped at depth 15
// stores 336-B records and builds level 15 in 904-B ones.  RMC_WIDE_WORK=0/1/2
// overrides the work record (never smaller than the store's).
static int wide_compact(const rmc_config& g) {
    if (const char* e = getenv("RMC_WIDE_COMPACT")) return std::max(0, std::min(2, atoi(e)));
    const bool ring = (g.flags & RMC_FLAG_SPILL) != 0;
    return record_for(g, g.max_depth > 0 ? g.max_depth - (ring ? 2 : 1) : 1 << 30);
}
static int wide_work(const rmc_config& g, int store) {
    if (!(g.flags & RMC_FLAG_SPILL)) return store;
    int w = record_for(g, g.max_depth > 0 ? g.max_depth - 1 : 1 << 30);
    if (const char* e = getenv("RMC_WIDE_WORK")) w = std::max(0, std::min(2, atoi(e)));
    return std::min(w, store);  // (0 is the largest record)
}
// Calls f with a null pointer to the record of a kind (WideBufs.compact / .work),
// the idiom of rmc_wide.hip's w_dispatch.
template <class F>
static auto with_record(int kind, F f) {
    return kind == 2 ? f((WStateD*)nullptr) : kind == 1 ? f((WStateC*)nullptr) : f((WState*)nullptr);
}
static size_t record_bytes(int kind) {
    return with_record(kind, [](auto* r) { return sizeof *r; });
}
size_t wide_record_bytes(const rmc_config& g) { return record_bytes(wide_compact(g)); }

// The most new states one state's expansion can yield (rmc_plan.h
// new_states_bound, the guards of raft.tla's Next) with the wide bag: Receive,
// Duplicate and Drop per message of a bag in the model and in the work record.
static u64 wide_bag(const rmc_config& g, int work) {  // messages of a stored state at most
    const u64 kw = work == 2 ? KWD : work == 1 ? KWC : KW;
    return std::min<u64>((u64)g.max_msgs, kw);
}
static u64 wide_new_per_state(const rmc_config& g, int work) {
    return new_states_bound((u64)g.n_servers, (u64)g.n_values, wide_bag(g, work));
}

// ---- context ----------------------------------------------------------------------
// Records of the deferred-hit buffer of full-state verification (WideBufs.vbuf): the
// packed layout's default; RMC_WIDE_VCAP=<records> overrides (A/B, tests: a small
// buffer makes many launches per level).
static u64 wide_vcap() {
    u64 v = 1ull << 26;
    if (const char* e = getenv("RMC_WIDE_VCAP")) v = strtoull(e, nullptr, 10);
    return std::max<u64>(std::min<u64>(v, 1ull << 32), 1024);  // (a state has at most WLANES_MAX = 272 lanes)
}

int create_wide(rmc_ctx* c) {
    fill_wide_model(c);
    const int compact = wide_compact(c->cfg);
    const u64 rec = record_bytes(compact);
    const bool ring = (c->cfg.flags & RMC_FLAG_SPILL) != 0;
    const bool verify = (c->cfg.flags & RMC_FLAG_VERIFY_STATES) != 0;
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    // the division of the budget: rmc_wide_plan.h (host arithmetic, tested without a device)
    WidePlanIn in{};
    in.budget = (u64)((double)fr * 0.80);
    in.rec = rec;
    in.state_capacity = c->cfg.state_capacity;
    in.set_slots = set_slots_of(c->cfg.set_bytes);  // rmc_config.set_bytes (TLC -fpmem)
    in.device_window = c->cfg.device_window;
    in.ring = ring;
    in.verify = verify;
    in.vcap = verify ? wide_vcap() : 0;
    const WidePlan plan = wide_plan(in);
    if (plan.cap_exceeds_set) {
        c->err = "state_capacity exceeds what a set of set_bytes " + std::to_string(c->cfg.set_bytes) + " holds";
        return RMC_E_INVAL;
    }
    const u64 cap = plan.cap, slots = plan.slots, win = plan.window;
    c->table_slots = slots;
    WideBufs& B = c->WB;
    B = WideBufs{};
    B.cap = cap;
    B.tmask = slots - 1;
    B.compact = compact;
    B.work = wide_work(c->cfg, compact);
    B.window = ring ? win : 0;
    B.verify = verify ? 1 : 0;
    B.vcap = in.vcap;
    B.fp_mask = ~0ull;
    B.sym = (c->cfg.flags & RMC_FLAG_SYMMETRY) ? 1 : 0;
    if (hipMalloc(&B.store, win * rec) != hipSuccess || hipMalloc(&B.parent, cap * 8) != hipSuccess ||
        hipMalloc(&B.act, cap) != hipSuccess || hipMalloc(&B.table, slots * 8) != hipSuccess ||
        hipMalloc(&B.ctr, sizeof(Counters)) != hipSuccess || hipMalloc(&c->w_staged, sizeof(WState)) != hipSuccess ||
        // verification: slot -> store index (8 B per slot) + the deferred hits (16 B each)
        (verify && (hipMalloc(&B.sidx, slots * 8) != hipSuccess || hipMalloc(&B.vbuf, B.vcap * 16) != hipSuccess)))
        return fail(c, RMC_E_NOMEM, "device allocation failed (wide layout, capacity " + std::to_string(cap) +
                                        " states" + (ring ? ", window " + std::to_string(win) + " records" : "") +
                                        (verify ? ", verification: " + std::to_string(slots) + " slot owners and " +
                                                      std::to_string(B.vcap) + " deferred hits"
                                                : "") +
                                        ")");
    c->B.ctr = B.ctr;  // reset_counters / read_counters work on it
    c->B.cap = cap;
    return 0;
}

void destroy_wide(rmc_ctx* c) {
    WideBufs& B = c->WB;
    (void)hipFree(B.store);
    (void)hipFree(B.parent);
    (void)hipFree(B.act);
    (void)hipFree(B.table);
    (void)hipFree(B.ctr);
    (void)hipFree(B.sidx);
    (void)hipFree(B.vbuf);
    (void)hipFree(c->w_staged);
    B = WideBufs{};
    c->B.ctr = nullptr;
    c->w_staged = nullptr;
}

static u64 wide_salt(u64 seed) { return seed ? (mix64(seed) & ((1ull << 59) - 1)) : 0ull; }

// ---- BFS (TLC's worker loop on the wide layout) ----------------------------------------
int run_bfs_wide(rmc_ctx* c, rmc_progress_fn cb, void* user) {
    const auto t0 = std::chrono::steady_clock::now();
    if (c->resume) return fail(c, RMC_E_STATE, "recover: not supported on the wide layout");
    WideBufs B = c->WB;
    B.salt = wide_salt(c->cfg.seed);
    c->have_target = 0;
    c->stop = 0;
    c->viol_valid = 0;
    c->res = rmc_result{};
    c->res.set_slots = c->table_slots;
    c->res.spill_links_on_device = B.window ? 1 : 0;
    c->level_start.clear();
    HIPCHK(c, launch_fill(B.table, c->table_slots * 8, 0, c->st));
    if (B.verify) {  // no slot has an owner yet
        HIPCHK(c, launch_fill(B.sidx, c->table_slots * 8, 0xFF, c->st));
        B.fp_mask = c->P.fp_mask;  // rmc_set_fp_bits
        B.vbase = 0;
    }
    c->h_ctr->count = 0;
    if (int rc = reset_counters(c, false)) return rc;
    const bool cover = cover_on(c);
    if (cover)
        if (int rc = cover_begin(c)) return rc;
    const bool cont = continue_on(c);  // (validate_wide refuses it with the ring)
    if (cont)
        if (int rc = viol_begin(c)) return rc;
    const bool preds = pred_on(c);  // (rmc_set_predicates refuses the ring)
    if (preds)
        if (int rc = pred_begin(c)) return rc;
    // Init in the record the seed kernel reads: the work record (= the store's without the ring)
    HIPCHK(c, with_record(B.window ? B.work : B.compact, [&](auto* r) {
        std::remove_pointer_t<decltype(r)> init;
        winit(c->WM, init);
        const hipError_t e = hipMemcpyAsync(c->w_staged, &init, sizeof init, hipMemcpyHostToDevice, c->st);
        return e != hipSuccess ? e : hipStreamSynchronize(c->st);  // (init lives on this stack frame)
    }));
    HIPCHK(c, launch_wseed(c->WM, B, c->w_staged, 1, c->st));
    if (int rc = read_counters(c)) return rc;
    int depth = seed_done(c);
    if (cover)  // row Init: the one initial state generated, and what the seed stored
        HIPCHK(c, launch_wcover(c->WM, B, 0, 0, 0, c->h_ctr->count, 1, c->d_cov, c->st));
    if (cont)  // the seed's states
        HIPCHK(c, launch_wviolations(c->WM, B, 0, c->h_ctr->count, c->d_viol, c->st));
    if (preds) {  // the seed's states: a predicate Init fails is the target, at depth 1
        if (int rc = pred_pass(c, 0, c->h_ctr->count)) return rc;
        if (int rc = pred_scan(c, 1)) return rc;
    }
    const u64 CHUNK = 1ull << 22;
    const u64 bound = wide_new_per_state(c->cfg, B.work);
    u64 records = c->h_ctr->count;  // ring: records written so far
    // verification: a launch defers at most one hit per lane of its states — the
    // lanes of families 0-6 and three per message of a bag in the model and in the
    // work record — so one of at most vcap / lanes states cannot overflow vbuf
    const u64 vlanes = (u64)c->WM.L.off[7] + 3 * wide_bag(c->cfg, B.work);
    const u64 chunk = B.verify ? std::max<u64>(1, std::min(CHUNK, B.vcap / vlanes)) : CHUNK;
    const LevelText text = {"verification: a fingerprint hit has no stored owner", nullptr, "wide states", nullptr};
    for (int more = 1; more && !c->stop;) {
        const u64 lo = c->level_start[(size_t)depth - 1], hi = c->level_start[(size_t)depth];
        if (lo == hi) break;
        if (c->cfg.max_depth > 0 && depth >= c->cfg.max_depth) {
            c->res.left_on_queue = hi - lo;
            break;
        }
        if (int rc = reset_counters(c, true)) return rc;
        HIPCHK(c, hipEventRecord(c->ev0, c->st));
        // the ring: a level no later one expands (max_depth) is not stored, and its
        // launches need no room
        B.unstored = B.window && c->cfg.max_depth > 0 && depth == c->cfg.max_depth - 1;
        for (u64 a = lo, b = 0; a < hi; a = b) {
            b = std::min(hi, a + chunk);
            if (B.window && !B.unstored) {
                // a launch overwrites no live record (rmc_plan.h ring_room)
                const u64 want = std::min(b - a, ring_room(c->h_ctr->count, a, B.window) / bound);
                if (want == 0) return window_too_small(c, B.window, 8);
                b = a + want;
            }
            B.vbase = c->h_ctr->count;  // (verification, coverage: read back after every launch)
            const u64 cov_before = c->h_ctr->count;
            HIPCHK(c, launch_wexpand(c->WM, B, a, b, c->st));
            c->res.expand_launches += 1;
            if (B.verify) {
                // the launch's hits on owners of the same launch, now that they are stored
                if (int rc = read_counters(c)) return rc;
                if (c->h_ctr->overflow || c->h_ctr->table_full) break;
                if (c->h_ctr->vcount > B.vcap)
                    return fail(c, RMC_E_HIP, "verification: " + std::to_string(b - a) + " states deferred " +
                                                  std::to_string(c->h_ctr->vcount) + " hits, bound " +
                                                  std::to_string(vlanes) + " each");
                HIPCHK(c, launch_wverify(c->WM, B, c->h_ctr->vcount, c->st));
                HIPCHK(c, hipMemsetAsync(&B.ctr->vcount, 0, 8, c->st));
                c->h_ctr->vcount = 0;
            }
            if (B.window) {
                const u64 before = c->h_ctr->count;
                if (int rc = read_counters(c)) return rc;
                if (c->h_ctr->overflow || c->h_ctr->table_full) break;
                // the room above rests on the bound: checked, not trusted
                if (c->h_ctr->count - before > (b - a) * bound)
                    return fail(c, RMC_E_HIP, "ring bound exceeded: " + std::to_string(b - a) + " states yielded " +
                                                  std::to_string(c->h_ctr->count - before) + " new states, bound " +
                                                  std::to_string(bound) + " each");
                if (!B.unstored) records = c->h_ctr->count;
                c->res.spilled = records > B.window ? records - B.window : 0;
                c->res.spills = records / B.window;  // passes of the ring
            }
            if (cover || cont || preds) {
                // the coverage pass of this launch: the ring still holds its parents [a, b)
                // (its room is relative to a), and the states it added, [count before, count
                // after), have their links even on the unstored last level; the violation
                // pass reads those states' records (the resident store only)
                if (!B.verify && !B.window) {  // (those paths have read the counters)
                    if (int rc = read_counters(c)) return rc;
                    if (c->h_ctr->overflow || c->h_ctr->table_full) break;
                }
                if (cover)
                    HIPCHK(c, launch_wcover(c->WM, B, a, b, cov_before, c->h_ctr->count, 0, c->d_cov, c->st));
                if (cont) HIPCHK(c, launch_wviolations(c->WM, B, cov_before, c->h_ctr->count, c->d_viol, c->st));
                if (preds)  // (the predicate pass: those states' records too)
                    if (int rc = pred_pass(c, cov_before, c->h_ctr->count)) return rc;
            }
        }
        if (int rc = end_level(c, hi, &depth, cb, user, t0, text, &more)) return rc;
    }
    c->res.distinct = c->level_start.back();
    c->res.depth = depth;
    c->res.stored_here = c->res.distinct;
    if (cover)
        if (int rc = cover_end(c)) return rc;
    if (cont)
        if (int rc = viol_end(c)) return rc;
    const double Dd = (double)c->res.distinct, G = (double)c->res.generated;
    c->res.collision_probability = fp_collision_estimate(Dd, G, (c->WB.tmask + 1));
    c->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int trace_wide(rmc_ctx* c, u64 target, rmc_state_view* states, int32_t* families, int32_t* instances, size_t cap,
               size_t* len) {
    std::vector<u64> chain;
    std::vector<uint8_t> acts;
    auto read_one = [c](u64 idx, u64* p, uint8_t* a) {
        HIPCHK(c, hipMemcpy(p, c->WB.parent + idx, 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(a, c->WB.act + idx, 1, hipMemcpyDeviceToHost));
        return 0;
    };
    if (int rc = walk_links(c, target, read_one, &chain, &acts)) return rc;
    *len = chain.size();
    const int S = c->WM.S;
    if (c->WB.window) {
        // the ring: a state of the chain may be overwritten, or of the unstored last
        // level — every state is re-derived from Init by its lane, on full records
        // (a bag lane is a slot of the parent's canonical bag, the same in every record)
        WState s, t;
        winit(c->WM, s);
        for (size_t q = 0; q < chain.size() && q < cap; ++q) {
            if (q) {
                if (wlane(c->WM, s, (int)acts[q], &t) != W_ON)
                    return fail(c, RMC_E_HIP, "trace replay: lane " + std::to_string((int)acts[q]) + " of state " +
                                                  std::to_string(chain[q - 1]) + " gives no successor");
                wcopy_state(s, t);
            }
            if (states) decode_wide(S, s, &states[q]);
            fill_step(families, instances, q, wide_family(c->WM, acts[q]), acts[q]);
        }
        return 0;
    }
    for (size_t q = 0; q < chain.size() && q < cap; ++q) {
        HIPCHK(c, with_record(c->WB.compact, [&](auto* r) {
            std::remove_pointer_t<decltype(r)> s;
            const hipError_t e =
                hipMemcpy(&s, static_cast<decltype(r)>(c->WB.store) + chain[q], sizeof s, hipMemcpyDeviceToHost);
            if (e == hipSuccess && states) decode_wide(S, s, &states[q]);
            return e;
        }));
        fill_step(families, instances, q, wide_family(c->WM, acts[q]), acts[q]);
    }
    return 0;
}

int expand_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, rmc_succ_view* out, size_t cap, size_t* n_out) {
    std::vector<WState> in(n);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_wide(c->WM.S, states[t], &in[t], &why))
            return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    const u64 lanes = (u64)c->WM.L.off[10];
    const u64 rcap = std::max<u64>(1, std::min<u64>((u64)cap, n * lanes));
    DevScratch<WState> d_in;
    DevScratch<WSucc> d_out;
    DevScratch<unsigned long long> d_cnt;
    HIPCHK(c, d_in.alloc(n));
    HIPCHK(c, d_out.alloc(rcap));
    HIPCHK(c, d_cnt.alloc(1));
    HIPCHK(c, hipMemcpy(d_in.get(), in.data(), n * sizeof(WState), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(d_cnt.get(), 0, 8));
    HIPCHK(c, launch_wlist(c->WM, d_in.get(), (u64)n, d_out.get(), rcap, d_cnt.get(), wide_salt(c->cfg.seed),
                           c->WB.sym, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    unsigned long long cnt = 0;
    HIPCHK(c, hipMemcpy(&cnt, d_cnt.get(), 8, hipMemcpyDeviceToHost));
    const u64 got = std::min<u64>(cnt, rcap);
    std::vector<WSucc> recs(got);
    if (got) HIPCHK(c, hipMemcpy(recs.data(), d_out.get(), got * sizeof(WSucc), hipMemcpyDeviceToHost));
    std::sort(recs.begin(), recs.end(), [](const WSucc& a, const WSucc& b) {
        return a.parent != b.parent ? a.parent < b.parent : a.lane < b.lane;
    });
    for (u64 q = 0; q < got && q < cap; ++q) {
        rmc_succ_view& s = out[q];
        memset(&s, 0, sizeof s);
        s.parent = recs[q].parent;
        s.instance = recs[q].lane;
        s.family = wide_family(c->WM, recs[q].lane);
        s.in_constraint = recs[q].in_model;
        s.fingerprint = recs[q].fp;
        if (s.in_constraint) decode_wide(c->WM.S, recs[q].state, &s.state);
    }
    *n_out = (size_t)cnt;
    return 0;
}

// rmc_state_keys on a wide ctx under SYMMETRY: the views as full records through k_wkeys.
int keys_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, uint64_t* keys, const uint32_t* ref, uint8_t* same) {
    std::vector<WState> in(n);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_wide(c->WM.S, states[t], &in[t], &why))
            return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    DevScratch<WState> d_in;
    DevScratch<u32> d_ref;
    DevScratch<u64> d_keys;
    DevScratch<unsigned char> d_same;
    HIPCHK(c, d_in.alloc(n));
    HIPCHK(c, d_keys.alloc(n));
    HIPCHK(c, hipMemcpy(d_in.get(), in.data(), n * sizeof(WState), hipMemcpyHostToDevice));
    if (ref) {
        HIPCHK(c, d_ref.alloc(n));
        HIPCHK(c, d_same.alloc(n));
        HIPCHK(c, hipMemcpy(d_ref.get(), ref, n * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(c, launch_wkeys(c->WM, d_in.get(), (u64)n, d_keys.get(), ref ? d_ref.get() : nullptr,
                           ref ? d_same.get() : nullptr, wide_salt(c->cfg.seed), c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(keys, d_keys.get(), n * 8, hipMemcpyDeviceToHost));
    if (ref) HIPCHK(c, hipMemcpy(same, d_same.get(), n, hipMemcpyDeviceToHost));
    return 0;
}

// rmc_check_states on the wide layout.  RMC_WSIM (read per call) picks the check as it
// picks the simulator's kernel: 1 (default) the wave's, 0 the thread's.
int check_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, uint32_t mask, int32_t* violated) {
    std::vector<WState> in(n);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_wide(c->WM.S, states[t], &in[t], &why))
            return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    const char* e = getenv("RMC_WSIM");
    const int wave = e ? atoi(e) : 1;
    WModel M = c->WM;
    M.inv_mask = (int)mask;
    DevScratch<WState> d_in;
    DevScratch<int> d_out;
    HIPCHK(c, d_in.alloc(n));
    HIPCHK(c, d_out.alloc(n));
    HIPCHK(c, hipMemcpy(d_in.get(), in.data(), n * sizeof(WState), hipMemcpyHostToDevice));
    HIPCHK(c, launch_wcheck(M, d_in.get(), (u64)n, d_out.get(), wave, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    std::vector<int> v(n);
    HIPCHK(c, hipMemcpy(v.data(), d_out.get(), n * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < n; ++t) violated[t] = v[t] ? 1 << (v[t] - 1) : 0;
    return 0;
}

// rmc_eval_predicates on the wide layout: the views as records of the store's kind (the
// interpreter reads the record the BFS pass reads), through k_wpred_eval into d_out.
int pred_eval_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, uint8_t* d_out) {
    return with_record(c->WB.compact, [&](auto* r) -> int {
        typedef std::remove_pointer_t<decltype(r)> Rec;
        std::vector<Rec> in(n);
        std::string why;
        for (size_t t = 0; t < n; ++t) {
            WState s;
            if (encode_wide(c->WM.S, states[t], &s, &why))
                return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
            if (wnarrow_bits<Rec>(s))
                return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": beyond the ctx's store record (" +
                                                std::to_string(Rec::kLW) + " log entries, " + std::to_string(Rec::kKW) +
                                                " messages)");
            wconvert(in[t], s);
        }
        DevScratch<Rec> d_in;
        HIPCHK(c, d_in.alloc(n));
        HIPCHK(c, hipMemcpy(d_in.get(), in.data(), n * sizeof(Rec), hipMemcpyHostToDevice));
        HIPCHK(c, launch_wpred_eval(c->d_prog, c->WM, c->WB.compact, d_in.get(), (u64)n, d_out, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        return 0;
    });
}

int sim_wide(rmc_ctx* c, const rmc_sim_config* sc, rmc_sim_result* out, i64 rec_beh, std::vector<rmc_state_view>* rec) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<WState> inits;
    std::string why;
    if (sc->smoke_k > 0) {
        std::vector<rmc_state_view> views;
        if (int rc = smoke_views(smoke_shape(c->cfg, true), *sc, &views, &why)) return fail(c, rc, why);
        inits.resize(views.size());
        for (size_t q = 0; q < views.size(); ++q)
            if (int rc = encode_wide(c->WM.S, views[q], &inits[q], &why)) return fail(c, rc, why);
    } else {
        inits.resize(1);
        winit(c->WM, inits[0]);
    }
    const u64 n_init = inits.size();
    DevScratch<WState> d_init, d_rec;
    DevScratch<SimCounters> d_out;
    HIPCHK(c, d_init.alloc(n_init));
    HIPCHK(c, d_out.alloc(1));
    if (rec) HIPCHK(c, d_rec.alloc((size_t)sc->depth));
    HIPCHK(c, hipMemcpy(d_init.get(), inits.data(), n_init * sizeof(WState), hipMemcpyHostToDevice));
    SimCounters h;
    float ms = 0.f;
    if (int rc = sim_timed(c, d_out.get(), &h, &ms, [&] {
            return launch_wsimulate(c->WM, d_init.get(), n_init, sc->behaviours, sc->depth, sc->seed, sc->mode,
                                    d_out.get(), rec_beh, d_rec.get(), c->st);
        }))
        return rc;
    if (rec) {
        std::vector<WState> ws((size_t)(h.steps + 1));
        HIPCHK(c, hipMemcpy(ws.data(), d_rec.get(), ws.size() * sizeof(WState), hipMemcpyDeviceToHost));
        rec->resize(ws.size());
        for (size_t q = 0; q < ws.size(); ++q) decode_wide(c->WM.S, ws[q], &(*rec)[q]);
    }
    fill_sim_result(out, h, rec ? 1 : sc->behaviours, n_init, ms, t0);
    return 0;
}

}  // namespace rmc_host

