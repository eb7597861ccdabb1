// rmc_dist.cpp — sharded BFS over several GPUs behind the C ABI (rmc_shard).
//
// One ctx per GPU, each a rank of a state-space partition (SURVEY.md §8e;
// replaces TLC's distributed mode).  A small level is REPLICATED: every rank
// gathers the whole frontier, expands it and keeps the successors it owns.
// Any other level every rank expands the frontier it owns in ROUNDS; a round's
// exchange is two-phase, fingerprint first:
//   expansion  k_expand_dist stores the new successors this rank owns and puts
//            every new one owned elsewhere, materialised once as its phase-2
//            record, in the round's pool (the pool flush; a send marker in the
//            fingerprint set keeps a successor from being pooled twice);
//            k_route keys the pool's records and fills the owners' key
//            outboxes with tickets naming them.  (SYMMETRY and verification:
//            k_expand<DIST> fills the outboxes itself with tickets (parent,
//            lane), SYMMETRY behind a lossy sent-cache.)
//   count row  a count all-to-all tells every rank what it receives;
//   phase 1  keys all-to-all; the owner inserts them (k_owner_insert), answers
//            new/seen with 1 byte per key and counts per source the states it
//            will receive; replies all-to-all (the reverse of the key exchange);
//   phase 2  k_materialize_remote copies the accepted successors' pool records
//            (or re-derives them from their tickets) into per-owner state
//            outboxes, counting them; states all-to-all; the owner stores them
//            (k_store_remote).
// The arithmetic of a round — the count row's layout, the byte blocks of the
// three all-to-alls, the round's size — is rmc_dist_plan.h (host-tested); the
// collectives and the deadlines on them are rmc_dist_comm.cpp.
// Pipelining: two outbox sets.  The ctx stream expands round k + 1 into one
// set while the exchange stream (xs) runs round k's exchange on the other, so
// the host's two count read-backs per round wait while the GPU expands.  A
// level ends with one all-gather of the device counters.  Keys that do not
// fit an outbox are parked (B.ovf) and sent in later rounds of the same level:
// an outbox overflow costs a round, never the run.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "rmc_dist_comm.h"
#include "rmc_dist_plan.h"

using namespace rmc;
using namespace rmc_host;

namespace {

// Bytes per phase-1 key record: the raw fingerprint (k, s32) as three u32
// {k lo, k hi, s32} (raft_packed.h Fp, put_key; the owner derives its own
// table value and slot).
constexpr u64 KEYB = 12;
static_assert(kPlanMaxWorld == kMaxWorld, "rmc_dist_plan.h sizes its per-peer arrays by kMaxWorld");

// The layout of this world's count rows, with the library's Counters in each block.
CountRow row_layout(const rmc_ctx* c) { return CountRow{(u64)kRowWords, (u64)c->dist.world}; }

float elapsed_ms(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

// One sharded search: what it carries from level to level, and the rounds of
// the exchanged level in progress.
struct Run {
    rmc_progress_fn cb = nullptr;
    void* user = nullptr;
    double t0 = 0;
    std::vector<Counters> rows;  // every rank's counters at the last level end
    bool rows_final = false;     // the level's last count row carried every rank's final counters
    std::vector<u64> fsz;           // every rank's frontier size (replicated levels need them all)
    std::vector<u64> count_before;  // every rank's store count when the current level began
    u64 total_prev = 0, generated = 0, probes = 0;
    int depth = 0;
    int any_cb = 0;   // some rank passed a progress callback (the per-level stop vote runs only then)
    // Round sizing: rho = most keys one round sends one owner, per expanded
    // state, from the previous rounds (rmc_dist_plan.h round_states, next_rho)
    double rho = 1.0;
    u64 vpub = 0;     // verification: states [0, vpub) are published (slot -> index)
    bool rep_timed = false;  // a replicated level's launch awaits its timing (read after the level end)
    // ---- the exchanged level in progress
    u64 hi = 0, cursor = 0;             // the frontier's end; its states below cursor are expanded
    u64 ovf_known = 0, ovf_done = 0;    // keys parked this level, as the last count row told; drained
    u64 split_cap = 0;
    u64 round_states[2] = {0, 0};  // states expanded by the round held in each set
    int round_kind[2] = {0, 0};    // 0 empty, 1 expansion, 2 drain
};

// c->B with the outboxes, tickets, counts and pool of outbox set S: what the
// kernels of a round run on (the expansion, k_route, k_drain, k_pack_counts,
// k_materialize_remote).  Of these fields k_pack_counts reads only ocount, and
// k_materialize_remote neither npool nor pool_cap: each gets a superset of
// what it reads.  (A replicated level's overlay is another: B.rep, no set.)
DevBufs set_bufs(const rmc_ctx* c, const DistState::Set& S) {
    DevBufs B = c->B;
    B.key_out = S.key_out;
    B.tick_out = S.tick_out;
    B.ocount = S.ocount;
    B.pool = S.pool;  // tickets POOL_TICK | index name this set's pool records
    B.npool = S.ocount + c->dist.world;
    B.pool_cap = c->dist.pool_cap;
    return B;
}

// Level end: the all-gathered device counters; errors stop every rank alike.
int level_end(rmc_ctx* c, Run& R) {
    DistState& D = c->dist;
    D.phase = "level end (counter all-gather)";
    if (!R.rows_final) {
        if (int rc = allgather_counters(c, R.rows.data())) return rc;
    }
    R.rows_final = false;
    *c->h_ctr = R.rows[(size_t)D.rank];
    const LevelText text = {"verification: a fingerprint without a published state", nullptr, "", nullptr};
    for (int r = 0; r < D.world; ++r)
        if (int rc = level_error(c, R.rows[(size_t)r], D.lvl, text, r)) return rc;
    return 0;
}

// The start of a search: the statistics cleared, the set begun and Init seeded
// (rmc_recover instead restored this rank's levels, parents and set — every rank
// of the checkpoint's world, each from its own part), the first level end, and
// every rank's frontier size.
int start(rmc_ctx* c, Run& R) {
    DistState& D = c->dist;
    const int W = D.world;
    D.lvl = 0;
    D.rnd = 0;
    D.phase = "start";
    const bool resume = c->resume != 0;
    c->resume = 0;
    const rmc_result saved = c->res;
    c->res = rmc_result{};
    c->res.set_slots = c->table_slots;
    if (!resume) c->level_start.clear();
    c->have_target = 0;
    c->stop = 0;
    D.keys_sent = D.states_sent = D.chunks = D.parked = 0;
    D.xfer_seconds = D.wait_seconds = 0;
    D.rep_levels = 0;
    if (c->B.sent) HIPCHK(c, launch_fill(c->B.sent, D.sent_slots * 8, 0, c->st));
    // Set epochs as on one GPU.  The send-marker kernels re-derive every remote
    // key from its materialised successor, never from a set value; SYMMETRY and
    // verification (the lossy sent-cache kernel recovers raw keys from set
    // values) keep an untagged set.
    const bool verify = c->sh.verify;
    if (!resume) {
        if (int rc = begin_set(c, !verify && !c->sh.sym)) return rc;
    } else {
        HIPCHK(c, set_fp_salt(*c->k, c->cfg.seed, c->set_epoch, c->st));
        c->h_ctr->count = c->level_start.back();
    }
    if (int rc = reset_counters(c, resume)) return rc;
    if (!resume)  // Init is stored by its owner only
        if (int rc = seed_init(c)) return rc;
    R.rows.resize((size_t)W);
    if (int rc = level_end(c, R)) return rc;
    if (!resume) {
        c->level_start.push_back(0);
        c->level_start.push_back(c->h_ctr->count);
    }
    if (verify && !resume && c->h_ctr->count)  // slot -> store index of the initial state(s)
        HIPCHK(c, c->k->publish(c->sh.sym, c->P, c->PT, c->B, 0, c->h_ctr->count, c->st));
    R.count_before.resize((size_t)W);
    for (int r = 0; r < W; ++r) {
        R.total_prev += R.rows[(size_t)r].count;
        R.count_before[(size_t)r] = R.rows[(size_t)r].count;
    }
    if (resume && R.total_prev != saved.distinct)
        return fail(c, RMC_E_IO, "recover: the ranks' parts hold " + std::to_string(R.total_prev) +
                                     " states, the checkpoint " + std::to_string(saved.distinct));
    if (!resume) scan_target(c, R.rows.data(), W, 1);  // Init's violation check (level 1)
    D.phase = "start (frontier sizes)";
    const u64 mine[2] = {c->level_start.back() - c->level_start[c->level_start.size() - 2], R.cb ? 1ull : 0ull};
    std::vector<u64> all(2 * (size_t)W);
    if (int rc = allgather(c, mine, sizeof mine, all.data())) return rc;
    R.fsz.resize((size_t)W);
    for (int r = 0; r < W; ++r) {
        R.fsz[(size_t)r] = all[2 * (size_t)r];
        R.any_cb |= all[2 * (size_t)r + 1] ? 1 : 0;
    }
    R.generated = resume ? saved.generated : 1;
    R.probes = resume ? saved.probes : 0;
    R.depth = resume ? c->resume_depth : 1;
    R.vpub = c->h_ctr->count;
    return 0;
}

// A replicated level: every rank gathers the whole frontier (ftot states),
// expands all of it and keeps the successors it owns; no key or state
// exchange, one all-gather of the level's records.
int replicated_level(rmc_ctx* c, Run& R, u64 lo, u64 hi, u64 ftot) {
    DistState& D = c->dist;
    const u64 RBR = (u64)(c->NW + 6) * 4;  // the level's record (RepRec)
    D.phase = "replicated level (frontier all-gather)";
    if (hi > lo) HIPCHK(c, c->k->pack_rep(c->B, lo, hi, D.rep_send, c->st));
    HIPCHK(c, hipEventRecord(D.ev_c, c->st));
    HIPCHK(c, hipStreamWaitEvent(D.xs, D.ev_c, 0));
    if (int rc = gather_level(c, R.fsz, RBR)) return rc;
    HIPCHK(c, hipEventRecord(D.ev_x, D.xs));
    HIPCHK(c, hipStreamWaitEvent(c->st, D.ev_x, 0));
    D.phase = "replicated level (expansion)";
    DevBufs Bb = c->B;
    Bb.rep = D.rep_buf;
    // one launch (rep_max <= 2^24 records); timed by events read after the level end
    HIPCHK(c, hipEventRecord(D.set[0].k0, c->st));
    HIPCHK(c, c->k->expand_rep(c->P, c->PT, Bb, 0, ftot, c->st));
    HIPCHK(c, hipEventRecord(D.set[0].k1, c->st));
    R.rep_timed = ftot != 0;
    c->res.expand_launches += 1;
    D.rep_levels += 1;
    D.chunks += 1;
    return 0;
}

// Enqueue, on the ctx stream, the expansion (or the drain of parked keys) of
// round k into set k & 1, once that set's last exchange has let go of it.
int enqueue_round(rmc_ctx* c, Run& R, u64 k) {
    DistState& D = c->dist;
    const int W = D.world, b = (int)(k & 1);
    const bool verify = c->sh.verify;
    DistState::Set& S = D.set[b];
    HIPCHK(c, hipStreamWaitEvent(c->st, S.ev_free, 0));
    HIPCHK(c, hipMemsetAsync(S.ocount, 0, 8 * (u64)(W + 1), c->st));
    const DevBufs Bb = set_bufs(c, S);
    R.round_states[b] = 0;
    R.round_kind[b] = 0;
    S.timed = 0;
    if (R.ovf_done < R.ovf_known) {
        const u64 n = std::min((u64)c->B.kcap, R.ovf_known - R.ovf_done);
        HIPCHK(c, launch_drain(Bb, R.ovf_done, n, c->st));
        R.ovf_done += n;
        R.round_kind[b] = 2;
    } else if (R.cursor < R.hi) {
        const u64 n = round_states(R.hi - R.cursor, c->B.kcap, D.fill, R.rho, R.split_cap, 1ull << kMaxDistLaunchLog2);
        HIPCHK(c, hipEventRecord(S.k0, c->st));
        HIPCHK(c, c->k->expand_dist(c->sh.sym, c->sh.verify, c->P, c->PT, Bb, R.cursor, R.cursor + n, c->st));
        // the pool flush's remote successors: keyed and routed to the outboxes
        if (W > 1 && !verify && !c->sh.sym)
            HIPCHK(c, c->k->route(c->P, Bb, c->st));
        HIPCHK(c, hipEventRecord(S.k1, c->st));
        S.timed = 1;
        c->res.expand_launches += 1;
        R.cursor += n;
        R.round_states[b] = n;
        R.round_kind[b] = 1;
    }
    if (verify) {  // publish this round's local states, then check the hits deferred to them
        if (int rc = read_counters(c)) return rc;
        const u64 c1 = c->h_ctr->count;
        if (c1 > R.vpub)
            HIPCHK(c, c->k->publish(c->sh.sym, c->P, c->PT, c->B, R.vpub, c1, c->st));
        R.vpub = c1;
        if (c->h_ctr->vcount) {
            HIPCHK(c, c->k->verify(c->sh.sym, c->P, c->PT, c->B, c->h_ctr->vcount, c->st));
            HIPCHK(c, hipMemsetAsync(&c->B.ctr->vcount, 0, 8, c->st));
        }
    }
    HIPCHK(c, hipEventRecord(S.ev_exp, c->st));
    return 0;
}

// The count row of the round held in set S, after its expansion: packed,
// exchanged and on its way to the pinned host row; D.ev_cnt follows it.
int count_row(rmc_ctx* c, DistState::Set& S, bool host_more, u64 ovf_done) {
    DistState& D = c->dist;
    const CountRow L = row_layout(c);
    D.phase = "count all-to-all";
    const DevBufs Bb = set_bufs(c, S);
    if (D.world == 1) {
        // a world of one: the row is its own all-to-all; the pack kernel writes
        // it (both halves) straight into the pinned host row, on the ctx stream
        // right after the expansion: no stream hop, collective or copy
        HIPCHK(c, hipEventRecord(S.x0, c->st));
        HIPCHK(c, launch_pack_counts(Bb, host_more ? 1ull : 0ull, ovf_done, S.h_cx, c->st, S.h_cx + L.recv(0)));
        HIPCHK(c, hipEventRecord(D.ev_cnt, c->st));
        return 0;
    }
    HIPCHK(c, hipStreamWaitEvent(D.xs, S.ev_exp, 0));
    HIPCHK(c, hipEventRecord(S.x0, D.xs));
    HIPCHK(c, launch_pack_counts(Bb, host_more ? 1ull : 0ull, ovf_done, S.cx, D.xs));
    if (int rc = a2a_u64(c, S.cx, S.cx + L.recv(0), L.words)) return rc;
    HIPCHK(c, hipMemcpyAsync(S.h_cx, S.cx, L.len() * 8, hipMemcpyDeviceToHost, D.xs));
    HIPCHK(c, hipEventRecord(D.ev_cnt, D.xs));
    return 0;
}

// The level's last round, idle on this rank: when no rank sent keys in it,
// nothing changes a counter after its count row, so the rows carry every
// rank's final counters — no level-end all-gather.
void take_final_rows(rmc_ctx* c, Run& R, const u64* cx, const RoundPlan& rp) {
    if (rp.global_sends || c->sh.verify) return;
    const CountRow L = row_layout(c);
    for (int p = 0; p < c->dist.world; ++p) memcpy(&R.rows[(size_t)p], cx + L.recv(p) + kRowCounters, sizeof(Counters));
    R.rows_final = true;
}

// Phase 1 of the round held in set S, on xs: keys to their owners, the owners'
// replies back, the accepted successors into the state outboxes; then the
// set's keys and tickets are consumed, and D.h_sa holds the phase-2 sizes.
int phase1(rmc_ctx* c, DistState::Set& S, const RoundPlan& rp) {
    DistState& D = c->dist;
    const int W = D.world;
    D.phase = "phase 1 (keys to owners)";
    HIPCHK(c, hipMemsetAsync(D.sa, 0, 16 * (u64)W, D.xs));
    const PeerBlocks& K = rp.keys;
    if (int rc = a2a(c, S.key_out, K.soff, K.scnt, D.key_in, K.roff, K.rcnt)) return rc;
    SrcOff so{};
    for (int p = 0; p < W; ++p) so.o[p] = rp.replies.soff[p];  // the keys from p, in records
    so.o[W] = rp.tot_in;
    HIPCHK(c, launch_owner_insert(c->B, D.key_in, D.rep_out, rp.tot_in, so, D.sa + W, D.xs));
    D.phase = "phase 1 (replies)";
    const PeerBlocks& Y = rp.replies;
    if (int rc = a2a(c, D.rep_out, Y.soff, Y.scnt, D.rep_in, Y.roff, Y.rcnt)) return rc;
    if (rp.mx) HIPCHK(c, c->k->materialize_remote(c->P, set_bufs(c, S), D.rep_in, rp.mx, 0, D.xs));
    HIPCHK(c, hipEventRecord(S.ev_free, D.xs));  // the set's keys and tickets are consumed
    HIPCHK(c, hipMemcpyAsync(D.h_sa, D.sa, 16 * (u64)W, hipMemcpyDeviceToHost, D.xs));
    HIPCHK(c, hipEventRecord(D.ev_acc, D.xs));
    return xwait(c, D.ev_acc);
}

// Phase 2, on xs: the accepted states to their owners, stored there (cx: the round's count row).
int phase2(rmc_ctx* c, Run& R, const u64* cx) {
    DistState& D = c->dist;
    const u64 RB = (u64)(c->NW + 4) * 4;  // state record: packed state, global parent ref, footprint
    const bool verify = c->sh.verify;
    D.phase = "phase 2 (states to owners)";
    const StatePlan sp = state_blocks(D.h_sa, cx, row_layout(c), D.rank, c->B.kcap, RB, verify);
    if (sp.over) return fail(c, RMC_E_HIP, "phase 2: more accepted states than keys sent");
    D.states_sent += sp.states_sent;
    const u64 tot_st = sp.tot_st;
    if (tot_st > (u64)D.world * c->B.kcap) return fail(c, RMC_E_CAPACITY, "phase-2 inbox full at " + where(c));
    const PeerBlocks& T = sp.states;
    if (int rc = a2a(c, c->B.st_out, T.soff, T.scnt, D.st_in, T.roff, T.rcnt)) return rc;
    if (tot_st) HIPCHK(c, c->k->store_remote(c->P, c->B, D.st_in, tot_st, D.xs));
    if (verify && tot_st) {  // publish the received new states, then compare the seen ones
        HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
        if (int rc = xwait(c, D.ev_h)) return rc;
        if (int rc = read_counters(c)) return rc;
        const u64 c2 = c->h_ctr->count;
        if (c2 > R.vpub)
            HIPCHK(c, c->k->publish(c->sh.sym, c->P, c->PT, c->B, R.vpub, c2, D.xs));
        R.vpub = c2;
        HIPCHK(c, c->k->compare_remote(c->sh.sym, c->P, c->PT, c->B, D.st_in, tot_st, D.xs));
        HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
        if (int rc = xwait(c, D.ev_h)) return rc;
    }
    return 0;
}

// What the host does with round k's count row once it has arrived: the parked
// keys known, the statistics, rho.  Fails alike on every rank when a rank's
// parking buffer or this rank's inbox is full.
int read_row(rmc_ctx* c, Run& R, u64 k, const RoundPlan& rp) {
    DistState& D = c->dist;
    const int b = (int)(k & 1);
    DistState::Set& S = D.set[b];
    if (rp.park_full >= 0)
        return fail(c, RMC_E_CAPACITY, "exchange parking buffer full on rank " + std::to_string(rp.park_full) +
                                           " (raise keys_per_dest) at " + where(c));
    D.parked += rp.newly_parked;
    R.ovf_known = std::max(R.ovf_known, rp.novf);
    D.keys_sent += rp.keys_sent;
    if (S.timed) {
        c->res.expand_kernel_seconds += 1e-3 * elapsed_ms(S.k0, S.k1);
        S.timed = 0;
    }
    if (D.set[b ^ 1].xtimed) {  // the previous round is complete on xs (stream order)
        D.xfer_seconds += 1e-3 * elapsed_ms(D.set[b ^ 1].x0, D.set[b ^ 1].x1);
        D.set[b ^ 1].xtimed = 0;
    }
    if (R.round_kind[b] == 1 && R.round_states[b]) R.rho = next_rho(R.rho, rp.mx, rp.newly_parked, R.round_states[b]);
    if (D.debug)
        fprintf(stderr, "[rmc rank %d] level %d round %llu kind %d states %llu: most keys to one owner %llu "
                        "(cap %llu), parked %llu/%llu, in %llu, rho %.3f, more %d\n",
                D.rank, R.depth, (unsigned long long)k, R.round_kind[b], (unsigned long long)R.round_states[b],
                (unsigned long long)rp.mx, (unsigned long long)c->B.kcap, (unsigned long long)R.ovf_done,
                (unsigned long long)R.ovf_known, (unsigned long long)rp.tot_in, R.rho, (int)rp.global_more);
    if (rp.tot_in > D.in_cap) return fail(c, RMC_E_CAPACITY, "phase-1 inbox full at " + where(c));
    return 0;
}

// An exchanged level: the frontier [lo, hi) this rank owns in rounds, until
// no rank has more to send.  Round k lives in set k & 1; its expansion is
// queued while round k - 1 is exchanged.
int exchanged_level(rmc_ctx* c, Run& R, u64 lo, u64 hi) {
    DistState& D = c->dist;
    const int W = D.world;
    const bool verify = c->sh.verify;
    const CountRow L = row_layout(c);
    R.hi = hi;
    R.cursor = lo;
    R.ovf_known = R.ovf_done = 0;
    R.split_cap = split_cap(hi - lo, D.split);
    R.round_states[0] = R.round_states[1] = 0;
    R.round_kind[0] = R.round_kind[1] = 0;
    if (int rc = enqueue_round(c, R, 0)) return rc;
    for (u64 k = 0;; ++k) {
        DistState::Set& S = D.set[k & 1];
        D.rnd = (int)k;
        const bool host_more = R.cursor < R.hi || R.ovf_done < R.ovf_known;
        if (int rc = count_row(c, S, host_more, R.ovf_done)) return rc;
        // the next round's expansion is queued before waiting, so the GPU
        // expands while the counts travel (not in RMC_DIST_OVERLAP=0 runs)
        bool next_queued = false;
        if (D.overlap && host_more) {
            if (int rc = enqueue_round(c, R, k + 1)) return rc;
            next_queued = true;
        }
        if (int rc = xwait(c, D.ev_cnt)) return rc;
        const u64* cx = S.h_cx;
        const RoundPlan rp = decode_round(cx, L, c->B.kcap, c->B.ovf_cap, R.ovf_known, KEYB);
        if (int rc = read_row(c, R, k, rp)) return rc;
        if (rp.global_more && !next_queued) {
            if (int rc = enqueue_round(c, R, k + 1)) return rc;
        }
        // nothing crosses this rank this round (always so at one rank): no
        // phase 1 or 2 and no second read-back.  RCCL point-to-point groups
        // pair ranks, so the others go on without this one; the host
        // transport's all-to-all is a collective of every rank, so there
        // only a world of one skips.
        const bool idle = !verify && (D.rccl || W == 1) && rp.tot_in == 0 && rp.mx == 0;
        hipStream_t over = D.xs;  // where the round ends
        if (idle) {
            over = W == 1 ? c->st : D.xs;  // where the count row ran
            HIPCHK(c, hipEventRecord(S.ev_free, over));
            if (!rp.global_more) take_final_rows(c, R, cx, rp);
        } else {
            if (int rc = phase1(c, S, rp)) return rc;
            if (int rc = phase2(c, R, cx)) return rc;
        }
        HIPCHK(c, hipEventRecord(S.x1, over));
        S.xtimed = 1;
        D.chunks += 1;
        if (!rp.global_more) break;
    }
    // expansion of the next level reads what xs stored: the ctx stream waits for it
    HIPCHK(c, hipEventRecord(D.ev_x, D.xs));
    HIPCHK(c, hipStreamWaitEvent(c->st, D.ev_x, 0));
    return 0;
}

// After the level end: the timings, the totals over every rank, the next
// level's frontier sizes, the target, and the progress vote.  *more = false when
// the search ends here: no new states, or rank 0's callback stopped it.
int level_totals(rmc_ctx* c, Run& R, bool* more) {
    DistState& D = c->dist;
    const int W = D.world;
    *more = false;
    if (R.rep_timed) {  // a replicated level's launch (complete: the counters were gathered after it)
        c->res.expand_kernel_seconds += 1e-3 * elapsed_ms(D.set[0].k0, D.set[0].k1);
        R.rep_timed = false;
    }
    for (auto& S : D.set)  // exchange device time of the level's last round
        if (S.xtimed) {
            D.xfer_seconds += 1e-3 * elapsed_ms(S.x0, S.x1);
            S.xtimed = 0;
        }
    u64 tot = 0;
    for (int r = 0; r < W; ++r) {
        const Counters& k = R.rows[(size_t)r];
        tot += k.count;
        R.generated += k.generated;
        R.probes += k.probes;
        c->res.collisions += k.collisions;
        c->res.verified += k.vchecked;
        // the next level's frontier on every rank: the states it stored in this one
        R.fsz[(size_t)r] = k.count - R.count_before[(size_t)r];
        R.count_before[(size_t)r] = k.count;
    }
    const u64 nnew = tot - R.total_prev;
    R.total_prev = tot;
    c->level_start.push_back(c->h_ctr->count);
    if (nnew) ++R.depth;
    scan_target(c, R.rows.data(), W, R.depth);
    if (R.any_cb) {  // progress: the same collective on every rank; all stop when rank 0's callback asks to
        rmc_level_stats ls{};
        ls.level = nnew ? R.depth - 1 : R.depth;
        ls.generated = R.generated;
        ls.distinct = tot;
        ls.new_states = nnew;
        ls.seconds = now_s() - R.t0;
        const int stop = (R.cb && R.cb(&ls, R.user)) ? 1 : 0;
        std::vector<int> votes((size_t)W);
        D.phase = "progress vote";
        if (int rc = allgather(c, &stop, sizeof stop, votes.data())) return rc;
        if (votes[0]) {
            c->res.left_on_queue = nnew;
            return 0;
        }
    }
    *more = nnew != 0;
    return 0;
}

void summary(rmc_ctx* c, const Run& R) {
    DistState& D = c->dist;
    c->res.generated = R.generated;
    c->res.distinct = R.total_prev;
    c->res.depth = R.depth;
    c->res.probes = R.probes;
    c->res.stored_here = c->level_start.back();
    c->res.keys_sent = D.keys_sent;
    c->res.states_sent = D.states_sent;
    c->res.chunks = D.chunks;
    c->res.exchange_seconds = D.xfer_seconds;
    c->res.exchange_wait_seconds = D.wait_seconds;
    c->res.parked = D.parked;
    c->res.collision_probability =
        fp_collision_estimate((double)R.total_prev, (double)R.generated, c->table_slots, c->set_epoch != 0);
    c->res.seconds = now_s() - R.t0;
    D.phase = "done";
}

}  // namespace

namespace rmc_host {

void free_dist(rmc_ctx* c) {
    DistState& D = c->dist;
    if (D.abort_pending) {  // RCCL kernels may still wait on these buffers: leave them to the process exit
        D = DistState{};
        D.aborted = 1;
        D.abort_pending = 1;
        return;
    }
    if (D.xs) (void)hipStreamSynchronize(D.xs);
    (void)hipFree(c->B.sent);
    (void)hipFree(c->B.ovf);
    for (auto& S : D.set) {
        (void)hipFree(S.key_out);
        (void)hipFree(S.tick_out);
        (void)hipFree(S.ocount);
        (void)hipFree(S.pool);
        (void)hipFree(S.cx);
        if (S.h_cx) (void)hipHostFree(S.h_cx);
        for (hipEvent_t e : {S.ev_exp, S.ev_free, S.k0, S.k1, S.x0, S.x1})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : {D.ev_cnt, D.ev_acc, D.ev_c, D.ev_x, D.ev_h})
        if (e) (void)hipEventDestroy(e);
    (void)hipFree(D.rep_send);
    (void)hipFree(D.rep_buf);
    (void)hipFree(D.key_in);
    (void)hipFree(D.rep_out);
    (void)hipFree(D.rep_in);
    (void)hipFree(D.st_in);
    (void)hipFree(c->B.st_out);
    (void)hipFree(D.sa);
    if (D.h_sa) (void)hipHostFree(D.h_sa);
    (void)hipFree(D.ag_dev);
    comm_close(c);
    if (D.xs) (void)hipStreamDestroy(D.xs);
    // every sharded field back to its default: only the set's doubling outlives a re-shard
    const int grown = D.table_grown;
    D = DistState{};
    D.table_grown = grown;
    c->B.sent = nullptr; c->B.key_out = nullptr; c->B.tick_out = nullptr; c->B.ocount = nullptr;
    c->B.st_out = nullptr; c->B.scount = nullptr; c->B.ovf = nullptr; c->B.ovf_cap = 0;
}

// The loop of the protocol above: per level, a replicated level or rounds of
// expansion and exchange, then the level end every rank reaches alike.
int run_bfs_sharded(rmc_ctx* c, rmc_progress_fn cb, void* user) {
    DistState& D = c->dist;
    Run R;
    R.cb = cb;
    R.user = user;
    R.t0 = now_s();
    if (D.aborted) return fail(c, RMC_E_STATE, "sharded search: the communicator was aborted by an earlier deadline");
    if (int rc = start(c, R)) return rc;
    // Replicated levels: the plain kernel (every shape), models with a
    // CONSTRAINT on every field (the capacity pass reads the store)
    // (a world of one has nothing to gather: its levels run as plain rounds)
    const bool rep_ok = D.world > 1 && !c->sh.verify && !c->sh.sym && !c->P.unbounded && D.rep_max > 0;
    for (bool more = true; more && !c->stop;) {
        const u64 lo = c->level_start[(size_t)R.depth - 1], hi = c->level_start[(size_t)R.depth];
        D.lvl = R.depth;
        D.rnd = 0;
        u64 ftot = 0;
        for (u64 x : R.fsz) ftot += x;
        if (c->cfg.max_depth > 0 && R.depth >= c->cfg.max_depth) {
            c->res.left_on_queue = ftot;
            break;
        }
        if (D.stall_rank == D.rank && D.stall_level == R.depth) {  // test hook: this rank stops answering
            fprintf(stderr, "[rmc rank %d] RMC_DIST_STALL_RANK: stalling %.1f s at level %d\n", D.rank, D.stall_s,
                    R.depth);
            std::this_thread::sleep_for(std::chrono::duration<double>(D.stall_s));
        }
        if (int rc = reset_counters(c, true)) return rc;
        if (int rc = rep_ok && ftot <= D.rep_max ? replicated_level(c, R, lo, hi, ftot) : exchanged_level(c, R, lo, hi))
            return rc;
        if (int rc = level_end(c, R)) return rc;
        if (int rc = level_totals(c, R, &more)) return rc;
    }
    summary(c, R);
    return 0;
}

// Counterexample across ranks (TLC's distributed trace reconstruction): each
// step the rank holding the current state contributes {state, parent ref,
// lane} to an all-gather; the parent ref names the next rank.
int trace_sharded(rmc_ctx* c, rmc_state_view* states, int32_t* families, int32_t* instances, size_t cap,
                  size_t* len) {
    DistState& D = c->dist;
    const int W = D.world;
    const u64 RB = 8 * 2 + (u64)c->NW * 4;  // has | act, parent ref, state
    std::vector<uint8_t> mine(RB), all(RB * (u64)W);
    std::vector<std::vector<u32>> chain_states;
    std::vector<int> chain_act;
    u64 ref = c->target_idx;
    for (int guard = 0; guard < 100000; ++guard) {
        const int owner = (int)(ref >> 48);
        const u64 idx = ref & ((1ull << 48) - 1);
        std::fill(mine.begin(), mine.end(), 0);
        if (owner == D.rank) {
            u64 head[2] = {1, 0};
            uint8_t a = 0;
            HIPCHK(c, hipMemcpy(&head[1], c->B.parent + idx, 8, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(&a, c->B.act + idx, 1, hipMemcpyDeviceToHost));
            head[0] = 1 | ((u64)a << 8);
            memcpy(mine.data(), head, 16);
            HIPCHK(c, hipMemcpy(mine.data() + 16, c->B.store + idx * (u64)c->NW, (u64)c->NW * 4, hipMemcpyDeviceToHost));
        }
        if (int rc = allgather(c, mine.data(), RB, all.data())) return rc;
        const uint8_t* rec = all.data() + (u64)owner * RB;
        u64 head[2];
        memcpy(head, rec, 16);
        if (!(head[0] & 1)) return fail(c, RMC_E_HIP, "trace: rank " + std::to_string(owner) + " holds no state " +
                                                          std::to_string(idx));
        std::vector<u32> st((size_t)c->NW);
        memcpy(st.data(), rec + 16, (u64)c->NW * 4);
        chain_states.push_back(st);
        chain_act.push_back((int)((head[0] >> 8) & 0xFF));
        if (head[1] == ~0ull) break;
        ref = head[1];
    }
    std::reverse(chain_states.begin(), chain_states.end());
    std::reverse(chain_act.begin(), chain_act.end());
    *len = chain_states.size();
    for (size_t q = 0; q < chain_states.size() && q < cap; ++q) {
        if (states) decode_state(c->sh.S, c->sh.K, chain_states[q].data(), &states[q]);
        fill_step(families, instances, q, family_of(c->P, chain_act[q]), chain_act[q]);
    }
    return 0;
}

}  // namespace rmc_host

extern "C" {

int rmc_shard(rmc_ctx* c, int32_t rank, int32_t world, const uint8_t* rccl_id, const rmc_transport* host,
              uint64_t keys_per_dest, uint64_t sent_cache_slots) {
    if (!c || world < 1 || world > kMaxWorld || rank < 0 || rank >= world) return RMC_E_INVAL;
    if (!rccl_id && !(host && host->alltoallv && host->allgather))
        return fail(c, RMC_E_INVAL, "rmc_shard needs an RCCL id or a host transport");
    if (pred_on(c))
        return fail(c, RMC_E_INVAL, "rmc_shard: model-defined invariants are single-GPU (rmc_set_predicates(ctx, NULL) "
                                    "removes them)");
    if (cons_on(c))
        return fail(c, RMC_E_INVAL, "rmc_shard: model-defined constraints are single-GPU (rmc_set_constraints(ctx, NULL) "
                                    "removes them)");
    if (act_on(c))
        return fail(c, RMC_E_INVAL, "rmc_shard: action properties are single-GPU (rmc_set_actions(ctx, NULL) removes "
                                    "them)");
    if (c->cfg.flags & RMC_FLAG_COVERAGE)
        return fail(c, RMC_E_INVAL, "sharded mode does not support RMC_FLAG_COVERAGE (coverage is single GPU)");
    if (c->cfg.flags & RMC_FLAG_CONTINUE)
        return fail(c, RMC_E_INVAL, "sharded mode does not support RMC_FLAG_CONTINUE (the violation tallies are "
                                    "single GPU)");
    if (c->spill.on) return fail(c, RMC_E_INVAL, "sharded mode does not support RMC_FLAG_SPILL");
    if (c->wide) return fail(c, RMC_E_INVAL, "sharded mode runs the packed layout only (bounds within its capacity)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    free_dist(c);
    DistState& D = c->dist;
    D.rank = rank;
    D.world = world;
    D.rccl = rccl_id != nullptr;
    if (host) D.host = *host;
    const u64 W = (u64)world;
    // keys one round may send one owner: 2^26 keys over all owners by default
    // (2^25 at 2 ranks, 2^23 at 8), which bounds the outboxes and inboxes
    const u64 kcap = keys_per_dest ? keys_per_dest : std::min<u64>(1ull << 25, std::max<u64>(1ull << 20, (1ull << 26) / W));
    u64 slots = 1;
    while (slots < std::max<u64>(sent_cache_slots ? sent_cache_slots : (1ull << 27), 1024)) slots <<= 1;
    const u64 RB = (u64)(c->NW + 4) * 4;
    D.sent_slots = slots;
    D.in_cap = W * kcap;
    // (RMC_DIST_XPRIO=1: the exchange stream at the highest priority, A/B)
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    const char* xp = getenv("RMC_DIST_XPRIO");
    bool ok = hipStreamCreateWithPriority(&D.xs, hipStreamNonBlocking, (xp && atoi(xp)) ? prio_hi : prio_lo) ==
              hipSuccess;
    // full-state verification ships every remote successor: no sent-cache
    // (the default kernel keeps send markers in the fingerprint set instead)
    if (!c->sh.verify && c->sh.sym) ok = ok && hipMalloc(&c->B.sent, slots * 8) == hipSuccess;
    const u64 ovf_cap = std::max<u64>(W * kcap, 1ull << 20);  // parked keys per level: >= a round's worth
    ok = ok && hipMalloc(&c->B.ovf, ovf_cap * 24) == hipSuccess;  // {k, s32 | flags, ticket}
    // the pool flush's remote successors of one round: as many as the round's
    // outboxes hold (a fuller pool parks tickets); none leave a world of one
    D.pool_cap = world > 1 ? W * kcap : 64;
    for (auto& S : D.set) {
        ok = ok && hipMalloc(&S.key_out, W * kcap * KEYB) == hipSuccess && hipMalloc(&S.tick_out, W * kcap * 8) == hipSuccess &&
             hipMalloc(&S.ocount, 8 * (W + 1)) == hipSuccess && hipMalloc(&S.cx, 8 * row_layout(c).len()) == hipSuccess &&
             hipMalloc(&S.pool, D.pool_cap * RB) == hipSuccess &&
             hipHostMalloc(&S.h_cx, 8 * row_layout(c).len(), hipHostMallocDefault) == hipSuccess;
        for (hipEvent_t* e : {&S.ev_exp, &S.ev_free})
            ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
        for (hipEvent_t* e : {&S.k0, &S.k1, &S.x0, &S.x1}) ok = ok && hipEventCreate(e) == hipSuccess;
    }
    for (hipEvent_t* e : {&D.ev_cnt, &D.ev_acc, &D.ev_c, &D.ev_x, &D.ev_h})
        ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    // replicated levels: levels of at most rep_max states in total are gathered
    // whole on every rank (RMC_DIST_REP states; 0 turns them off)
    D.rep_max = 1ull << 20;
    if (const char* e = getenv("RMC_DIST_REP")) D.rep_max = std::min<u64>((u64)atoll(e), 1ull << 24);
    if (D.rep_max) {
        const u64 rbr = (u64)(c->NW + 6) * 4;
        ok = ok && hipMalloc(&D.rep_send, D.rep_max * rbr) == hipSuccess &&
             hipMalloc(&D.rep_buf, D.rep_max * rbr) == hipSuccess;
    }
    ok = ok && hipMalloc(&D.key_in, W * kcap * KEYB) == hipSuccess && hipMalloc(&D.rep_out, W * kcap) == hipSuccess &&
         hipMalloc(&D.rep_in, W * kcap) == hipSuccess && hipMalloc(&c->B.st_out, W * kcap * RB) == hipSuccess &&
         hipMalloc(&D.st_in, W * kcap * RB) == hipSuccess && hipMalloc(&D.sa, 16 * W) == hipSuccess &&
         hipHostMalloc(&D.h_sa, 16 * W, hipHostMallocDefault) == hipSuccess &&
         hipMalloc(&D.ag_dev, 4096 * (W + 1)) == hipSuccess;
    if (!ok) {
        free_dist(c);
        return fail(c, RMC_E_NOMEM, "sharded-mode buffers do not fit (lower keys_per_dest / sent_cache_slots)");
    }
    // send markers share the fingerprint set with this rank's states: twice the
    // slots keeps the load of linear probing near the single-GPU one (when
    // HBM allows; otherwise the set stays as rmc_create sized it)
    // (only with 8 GiB to spare after the larger set is allocated: the kernels'
    // scratch, RCCL and other ranks sharing the device allocate after this)
    size_t mfree = 0, mtot = 0;
    (void)hipMemGetInfo(&mfree, &mtot);
    if (world > 1 && !c->sh.verify && !c->sh.sym && !D.table_grown && mfree >= c->table_slots * 16 + (8ull << 30)) {
        u64* t2 = nullptr;
        if (hipMalloc(&t2, c->table_slots * 16) == hipSuccess) {
            (void)hipFree(c->B.table);
            c->B.table = t2;
            c->table_slots *= 2;
            c->B.tmask = c->table_slots - 1;
            c->set_epoch = 0;  // a new, uncleared set: the next run clears it
            D.table_grown = 1;
        }
    }
    D.ag_cap = 4096;
    D.debug = getenv("RMC_DIST_DEBUG") != nullptr;
    // rounds per large level: 4 at world > 1 (round 6; 2 before), so each round's
    // exchange overlaps the next round's expansion and only the last quarter of a
    // level's exchange is exposed; 1 at world 1, where no round exchanges anything
    // (283.4-283.7 vs 289.8-294.0 ms for 2 on the one-rank bench,
    // profiles/r04/ab/dist_split_r04u.txt)
    D.split = world > 1 ? 4 : 1;
    if (const char* s = getenv("RMC_DIST_SPLIT")) D.split = std::max(1, std::min(64, atoi(s)));
    if (const char* s = getenv("RMC_DIST_OVERLAP")) D.overlap = atoi(s) != 0;
    if (c->sh.verify) D.overlap = 0;  // rounds in order: each publishes its states before the next compares
    if (const char* s = getenv("RMC_DIST_FILL")) D.fill = std::max(0.01, std::min(64.0, atof(s)));
    c->B.smask = slots - 1;
    c->B.kcap = kcap;
    c->B.scap = kcap;
    c->B.scount = D.sa;
    c->B.ovf_cap = ovf_cap;
    c->B.rank = (u32)rank;
    c->B.world = (u32)world;
    c->B.ref_tag = (u64)rank << 48;
    const char* om = getenv("RMC_OWNER");  // partition: 0 fingerprint, 1 server-0 word, 2 servers 0+1
    c->B.owner_mode = om ? (u32)std::min(3, std::max(0, atoi(om))) : 2u;
    // SYMMETRY: the states of one orbit must meet at one owner, so the owner is
    // a function of the canonical fingerprint (server words differ across the orbit)
    if (c->sh.sym) c->B.owner_mode = 0;
    D.timeout_s = 300.0;
    if (const char* e = getenv("RMC_DIST_TIMEOUT_S")) D.timeout_s = std::max(0.1, atof(e));
    // test hook: rank RMC_DIST_STALL_RANK sleeps RMC_DIST_STALL_S (default twice
    // the deadline) before level RMC_DIST_STALL_LEVEL (default 2)
    D.stall_rank = -1;
    if (const char* e = getenv("RMC_DIST_STALL_RANK")) D.stall_rank = atoi(e);
    D.stall_level = 2;
    if (const char* e = getenv("RMC_DIST_STALL_LEVEL")) D.stall_level = atoi(e);
    D.stall_s = 2 * D.timeout_s;
    if (const char* e = getenv("RMC_DIST_STALL_S")) D.stall_s = atof(e);
    D.lvl = 0;
    D.rnd = 0;
    D.phase = "communicator init";
    if (D.rccl)
        if (int rc = comm_init(c, rccl_id)) {
            const std::string msg = c->err;
            free_dist(c);
            c->err = msg;
            return rc;
        }
    D.on = 1;
    return 0;
}

}  // extern "C"
