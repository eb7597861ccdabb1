// rmc_wide.cpp — host side of the wide layout (raft_wide.h, rmc_wide.hip):
// the codec between rmc_state_view and the wide record, the BFS level loop,
// the counterexample walk, the successor listing and the random walks.  A
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
    if (c->flags & RMC_FLAG_SYMMETRY)
        return bad("the wide layout (bounds beyond the packed capacity) supports no SYMMETRY");
    // verification compares a hit with its owner's resident record, found through 8 B
    // more per set slot; at the depths that need the ring that array no longer fits
    // beside the set and the window (DESIGN.md "Wide state")
    if ((c->flags & RMC_FLAG_VERIFY_STATES) && (c->flags & RMC_FLAG_SPILL))
        return bad("the wide layout (bounds beyond the packed capacity) supports RMC_FLAG_VERIFY_STATES only "
                   "without RMC_FLAG_SPILL: verification needs every state resident");
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

int wide_family(const rmc_ctx* c, int lane) { return lane == 255 ? -1 : c->WM.L.family(lane); }

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

// ---- codec ----------------------------------------------------------------------
int encode_wide(const rmc_ctx* c, const rmc_state_view& v, WState* out, std::string* why) {
    const int S = c->WM.S;
    auto bad = [&](const std::string& s) { *why = s; return RMC_E_INVAL; };
    WState& s = *out;
    wzero(&s, (int)sizeof s);
    if (v.n_servers != S) return bad("view n_servers differs from config");
    if (v.n_msgs < 0 || v.n_msgs > KW) return bad("too many messages for the wide bag");
    auto byte = [](int x, int lo, int hi) { return x >= lo && x <= hi; };
    for (int i = 0; i < S; ++i) {
        if (!byte(v.currentTerm[i], 0, TMAX)) return bad("currentTerm out of the wide range");
        if (!byte(v.state[i], 0, 2)) return bad("state out of range");
        if (v.votedFor[i] < -1 || v.votedFor[i] >= S) return bad("votedFor out of range");
        if (!byte(v.commitIndex[i], 0, 255)) return bad("commitIndex out of range");
        if (!byte(v.log_len[i], 0, LW)) return bad("log length out of the wide range");
        if ((v.votesResponded[i] | v.votesGranted[i]) >> S) return bad("vote set out of range");
        s.ct[i] = (uint8_t)v.currentTerm[i];
        s.st[i] = (uint8_t)v.state[i];
        s.vf[i] = v.votedFor[i] < 0 ? NIL : (uint8_t)v.votedFor[i];
        s.ci[i] = (uint8_t)v.commitIndex[i];
        s.len[i] = (uint8_t)v.log_len[i];
        s.vR[i] = (uint8_t)v.votesResponded[i];
        s.vG[i] = (uint8_t)v.votesGranted[i];
        for (int x = 0; x < v.log_len[i]; ++x) {
            if (!byte(v.log[i][x].term, 0, TMAX) || !byte(v.log[i][x].value, 0, 1)) return bad("log entry out of range");
            s.log[i][x].term = (uint8_t)v.log[i][x].term;
            s.log[i][x].value = (uint8_t)v.log[i][x].value;
        }
        for (int j = 0; j < S; ++j) {
            if (!byte(v.nextIndex[i][j], 1, 255) || !byte(v.matchIndex[i][j], 0, 255)) return bad("index out of range");
            s.ni[i][j] = (uint8_t)v.nextIndex[i][j];
            s.mi[i][j] = (uint8_t)v.matchIndex[i][j];
        }
    }
    for (int q = 0; q < v.n_msgs; ++q) {
        const rmc_msg_view& m = v.msgs[q];
        if (!byte(m.mtype, 0, 3)) return bad("mtype out of range");
        if (!byte(m.msource, 0, S - 1) || !byte(m.mdest, 0, S - 1)) return bad("message endpoint out of range");
        if (!byte(m.mterm, 0, TMAX)) return bad("mterm out of the wide range");
        if (!byte(m.count, 1, CMAX)) return bad("message count out of the wide range");
        WMsg w;
        wmsg_zero(w);
        w.type = (uint8_t)m.mtype;
        w.term = (uint8_t)m.mterm;
        w.src = (uint8_t)m.msource;
        w.dst = (uint8_t)m.mdest;
        switch (m.mtype) {
            case RVQ:
                if (!byte(m.mlastLogTerm, 0, TMAX) || !byte(m.mlastLogIndex, 0, 255))
                    return bad("RequestVoteRequest field out of range");
                w.b = (uint8_t)m.mlastLogTerm;
                w.c = (uint8_t)m.mlastLogIndex;
                break;
            case RVP:
                if (!byte(m.mlog_len, 0, LW)) return bad("mlog too long");
                w.a = (int8_t)(m.mvoteGranted != 0);
                w.n = (uint8_t)m.mlog_len;
                for (int x = 0; x < m.mlog_len; ++x) {
                    if (!byte(m.mlog[x].term, 0, TMAX) || !byte(m.mlog[x].value, 0, 1)) return bad("mlog entry out of range");
                    w.e[x].term = (uint8_t)m.mlog[x].term;
                    w.e[x].value = (uint8_t)m.mlog[x].value;
                }
                break;
            case AEQ:
                if (!byte(m.mprevLogIndex, -1, 127) || !byte(m.mprevLogTerm, 0, 255) || !byte(m.mentries_len, 0, 1) ||
                    !byte(m.mcommitIndex, 0, 255))
                    return bad("AppendEntriesRequest field out of range");
                w.a = (int8_t)m.mprevLogIndex;
                w.b = (uint8_t)m.mprevLogTerm;
                w.c = (uint8_t)m.mcommitIndex;
                w.n = (uint8_t)m.mentries_len;
                if (m.mentries_len) {
                    if (!byte(m.mentries[0].term, 0, TMAX) || !byte(m.mentries[0].value, 0, 1))
                        return bad("mentries entry out of range");
                    w.e[0].term = (uint8_t)m.mentries[0].term;
                    w.e[0].value = (uint8_t)m.mentries[0].value;
                }
                break;
            default:
                if (!byte(m.mmatchIndex, 0, 255)) return bad("mmatchIndex out of range");
                w.a = (int8_t)(m.msuccess != 0);
                w.b = (uint8_t)m.mmatchIndex;
        }
        for (int k = 0; k < s.nmsg; ++k)
            if (wmsg_cmp(s.msg[k], w) == 0) return bad("duplicate message in bag view");
        // insert sorted (the canonical order)
        int k = 0;
        while (k < s.nmsg && wmsg_cmp(s.msg[k], w) < 0) ++k;
        for (int r = s.nmsg; r > k; --r) {
            s.msg[r] = s.msg[r - 1];
            s.cnt[r] = s.cnt[r - 1];
        }
        s.msg[k] = w;
        s.cnt[k] = (uint8_t)m.count;
        s.nmsg += 1;
    }
    return 0;
}

template <class St>
void decode_wide(const rmc_ctx* c, const St& s, rmc_state_view* v) {
    const int S = c->WM.S;
    memset(v, 0, sizeof *v);
    v->n_servers = S;
    for (int i = 0; i < S; ++i) {
        v->currentTerm[i] = s.ct[i];
        v->state[i] = s.st[i];
        v->votedFor[i] = s.vf[i] == NIL ? -1 : s.vf[i];
        v->commitIndex[i] = s.ci[i];
        v->log_len[i] = s.len[i];
        for (int x = 0; x < s.len[i]; ++x) {
            v->log[i][x].term = s.log[i][x].term;
            v->log[i][x].value = s.log[i][x].value;
        }
        v->votesResponded[i] = s.vR[i];
        v->votesGranted[i] = s.vG[i];
        for (int j = 0; j < S; ++j) {
            v->nextIndex[i][j] = s.ni[i][j];
            v->matchIndex[i][j] = s.mi[i][j];
        }
    }
    v->n_msgs = s.nmsg;
    for (int q = 0; q < s.nmsg; ++q) {
        const auto& w = s.msg[q];
        rmc_msg_view& m = v->msgs[q];
        m.mtype = w.type;
        m.mterm = w.term;
        m.msource = w.src;
        m.mdest = w.dst;
        m.count = s.cnt[q];
        switch (w.type) {
            case RVQ: m.mlastLogTerm = w.b; m.mlastLogIndex = w.c; break;
            case RVP:
                m.mvoteGranted = w.a;
                m.mlog_len = w.n;
                for (int x = 0; x < w.n; ++x) { m.mlog[x].term = w.e[x].term; m.mlog[x].value = w.e[x].value; }
                break;
            case AEQ:
                m.mprevLogIndex = w.a;
                m.mprevLogTerm = w.b;
                m.mcommitIndex = w.c;
                m.mentries_len = w.n;
                if (w.n) { m.mentries[0].term = w.e[0].term; m.mentries[0].value = w.e[0].value; }
                break;
            default: m.msuccess = w.a; m.mmatchIndex = w.b;
        }
    }
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
    const u64 CHUNK = 1ull << 22;
    const u64 bound = wide_new_per_state(c->cfg, B.work);
    u64 records = c->h_ctr->count;  // ring: records written so far
    // verification: a launch defers at most one hit per lane of its states — the
    // lanes of families 0-6 and three per message of a bag in the model and in the
    // work record — so one of at most vcap / lanes states cannot overflow vbuf
    const u64 vlanes = (u64)c->WM.L.off[7] + 3 * wide_bag(c->cfg, B.work);
    const u64 chunk = B.verify ? std::max<u64>(1, std::min(CHUNK, B.vcap / vlanes)) : CHUNK;
    const LevelText text = {"verification: a fingerprint hit has no stored owner", nullptr, "wide states", nullptr};
    for (int more = 1; more && !c->have_target;) {
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
            B.vbase = c->h_ctr->count;  // (verification: read back after every launch)
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
        }
        if (int rc = end_level(c, hi, &depth, cb, user, t0, text, &more)) return rc;
    }
    c->res.distinct = c->level_start.back();
    c->res.depth = depth;
    c->res.stored_here = c->res.distinct;
    const double Dd = (double)c->res.distinct, G = (double)c->res.generated;
    c->res.collision_probability = fp_collision_estimate(Dd, G, (c->WB.tmask + 1));
    c->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

int trace_wide(rmc_ctx* c, rmc_state_view* states, int32_t* families, int32_t* instances, size_t cap, size_t* len) {
    std::vector<u64> chain;
    std::vector<uint8_t> acts;
    u64 idx = c->target_idx;
    for (;;) {
        u64 p = 0;
        uint8_t a = 0;
        HIPCHK(c, hipMemcpy(&p, c->WB.parent + idx, 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&a, c->WB.act + idx, 1, hipMemcpyDeviceToHost));
        chain.push_back(idx);
        acts.push_back(a);
        if (p == ~0ull || chain.size() > 100000) break;
        idx = p;
    }
    std::reverse(chain.begin(), chain.end());
    std::reverse(acts.begin(), acts.end());
    *len = chain.size();
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
            if (states) decode_wide(c, s, &states[q]);
            if (families) families[q] = wide_family(c, acts[q]);
            if (instances) instances[q] = acts[q] == 255 ? -1 : acts[q];
        }
        return 0;
    }
    for (size_t q = 0; q < chain.size() && q < cap; ++q) {
        HIPCHK(c, with_record(c->WB.compact, [&](auto* r) {
            std::remove_pointer_t<decltype(r)> s;
            const hipError_t e =
                hipMemcpy(&s, static_cast<decltype(r)>(c->WB.store) + chain[q], sizeof s, hipMemcpyDeviceToHost);
            if (e == hipSuccess && states) decode_wide(c, s, &states[q]);
            return e;
        }));
        if (families) families[q] = wide_family(c, acts[q]);
        if (instances) instances[q] = acts[q] == 255 ? -1 : acts[q];
    }
    return 0;
}

int expand_wide(rmc_ctx* c, const rmc_state_view* states, size_t n, rmc_succ_view* out, size_t cap, size_t* n_out) {
    std::vector<WState> in(n);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_wide(c, states[t], &in[t], &why)) return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    const u64 lanes = (u64)c->WM.L.off[10];
    const u64 rcap = std::max<u64>(1, std::min<u64>((u64)cap, n * lanes));
    WState* d_in = nullptr;
    WSucc* d_out = nullptr;
    unsigned long long* d_cnt = nullptr;
    HIPCHK(c, hipMalloc(&d_in, n * sizeof(WState)));
    HIPCHK(c, hipMalloc(&d_out, rcap * sizeof(WSucc)));
    HIPCHK(c, hipMalloc(&d_cnt, 8));
    HIPCHK(c, hipMemcpy(d_in, in.data(), n * sizeof(WState), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(d_cnt, 0, 8));
    HIPCHK(c, launch_wlist(c->WM, d_in, (u64)n, d_out, rcap, d_cnt, wide_salt(c->cfg.seed), c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    unsigned long long cnt = 0;
    HIPCHK(c, hipMemcpy(&cnt, d_cnt, 8, hipMemcpyDeviceToHost));
    const u64 got = std::min<u64>(cnt, rcap);
    std::vector<WSucc> recs(got);
    if (got) HIPCHK(c, hipMemcpy(recs.data(), d_out, got * sizeof(WSucc), hipMemcpyDeviceToHost));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_cnt);
    std::sort(recs.begin(), recs.end(), [](const WSucc& a, const WSucc& b) {
        return a.parent != b.parent ? a.parent < b.parent : a.lane < b.lane;
    });
    for (u64 q = 0; q < got && q < cap; ++q) {
        rmc_succ_view& s = out[q];
        memset(&s, 0, sizeof s);
        s.parent = recs[q].parent;
        s.instance = recs[q].lane;
        s.family = wide_family(c, recs[q].lane);
        s.in_constraint = recs[q].in_model;
        s.fingerprint = recs[q].fp;
        if (s.in_constraint) decode_wide(c, recs[q].state, &s.state);
    }
    *n_out = (size_t)cnt;
    return 0;
}

int smoke_views(const rmc_ctx* c, const rmc_sim_config& sc, std::vector<rmc_state_view>* views, std::string* why);

int sim_wide(rmc_ctx* c, const rmc_sim_config* sc, rmc_sim_result* out, i64 rec_beh, std::vector<rmc_state_view>* rec) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<WState> inits;
    std::string why;
    if (sc->smoke_k > 0) {
        std::vector<rmc_state_view> views;
        if (int rc = smoke_views(c, *sc, &views, &why)) return fail(c, rc, why);
        inits.resize(views.size());
        for (size_t q = 0; q < views.size(); ++q)
            if (int rc = encode_wide(c, views[q], &inits[q], &why)) return fail(c, rc, why);
    } else {
        inits.resize(1);
        winit(c->WM, inits[0]);
    }
    const u64 n_init = inits.size();
    WState *d_init = nullptr, *d_rec = nullptr;
    SimCounters* d_out = nullptr;
    HIPCHK(c, hipMalloc(&d_init, n_init * sizeof(WState)));
    HIPCHK(c, hipMalloc(&d_out, sizeof(SimCounters)));
    if (rec) HIPCHK(c, hipMalloc(&d_rec, (size_t)sc->depth * sizeof(WState)));
    SimCounters h{};
    h.viol = ~0ull;
    HIPCHK(c, hipMemcpy(d_init, inits.data(), n_init * sizeof(WState), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_out, &h, sizeof h, hipMemcpyHostToDevice));
    HIPCHK(c, hipEventRecord(c->ev0, c->st));
    HIPCHK(c, launch_wsimulate(c->WM, d_init, n_init, sc->behaviours, sc->depth, sc->seed, sc->mode, d_out, rec_beh,
                               d_rec, c->st));
    HIPCHK(c, hipEventRecord(c->ev1, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    HIPCHK(c, hipMemcpy(&h, d_out, sizeof h, hipMemcpyDeviceToHost));
    if (rec) {
        std::vector<WState> ws((size_t)(h.steps + 1));
        HIPCHK(c, hipMemcpy(ws.data(), d_rec, ws.size() * sizeof(WState), hipMemcpyDeviceToHost));
        rec->resize(ws.size());
        for (size_t q = 0; q < ws.size(); ++q) decode_wide(c, ws[q], &(*rec)[q]);
    }
    (void)hipFree(d_init);
    (void)hipFree(d_out);
    (void)hipFree(d_rec);
    memset(out, 0, sizeof *out);
    out->behaviours = rec ? 1 : sc->behaviours;
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
    return 0;
}

}  // namespace rmc_host
