// rmc_dist_plan.h — the arithmetic of one exchange round of the sharded BFS
// (rmc_dist.cpp): the layout of the count row, what a rank sends to and receives
// from every peer in the three all-to-alls, and how many states a round expands.
// Host arithmetic only (no HIP, no getenv, not rmc_ctx.h), so a host test plays
// every rank of a world and checks that the ranks' plans agree
// (tests/native/dist_plan_check.cpp).  The Counters layout is rmc_internal.h's,
// which pulls in HIP: the row's block width and the record sizes are arguments.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rmc_host {

constexpr int kPlanMaxWorld = 64;  // = rmc::kMaxWorld (rmc_dist.cpp asserts it)

// The count row of a round (k_pack_counts): a block of `words` u64 for every
// rank p, what this rank sends p; one word, the keys this rank has parked so far
// this level; then the block every rank p sent this rank.  A block is {keys for
// the peer, flags, the sender's Counters}.
struct CountRow {
    uint64_t words;  // kRowWords
    uint64_t W;      // world
    uint64_t sent(int p) const { return words * (uint64_t)p; }  // word offsets into the row
    uint64_t novf() const { return words * W; }
    uint64_t recv(int p) const { return words * W + 1 + words * (uint64_t)p; }
    uint64_t len() const { return 2 * words * W + 1; }
};
enum : uint64_t { kRowKeys = 0, kRowFlags = 1, kRowCounters = 2 };  // words of a block
enum : uint64_t {
    kFlagMore = 1,      // the rank has more to send this level (frontier left, or parked keys)
    kFlagParkFull = 2,  // its parking buffer overflowed: every rank reads every row and fails alike
    kFlagSends = 4,     // it sends keys to some peer this round
};

// One all-to-all: block p of the send buffer is [soff[p], soff[p] + scnt[p]) for
// rank p, block p of the receive buffer [roff[p], roff[p] + rcnt[p]) from rank p (bytes).
struct PeerBlocks {
    uint64_t soff[kPlanMaxWorld], scnt[kPlanMaxWorld], roff[kPlanMaxWorld], rcnt[kPlanMaxWorld];
};

// What the host reads off a round's count row.
struct RoundPlan {
    bool global_more;   // some rank has more to send this level
    bool global_sends;  // some rank sends keys this round
    int park_full;      // the first rank whose parking buffer is full, -1: none
    uint64_t mx;        // most keys this rank sends one owner
    uint64_t keys_sent, tot_in;  // keys this rank sends / receives
    uint64_t novf;      // keys parked so far this level, never past the buffer
    uint64_t newly_parked;
    PeerBlocks keys;     // phase 1: key_out [W][kcap] -> key_in, packed in rank order (key_bytes each)
    PeerBlocks replies;  // the reverse exchange, 1 byte per key: rep_out (as key_in) -> rep_in [W][kcap]
};
inline RoundPlan decode_round(const uint64_t* cx, CountRow L, uint64_t kcap, uint64_t ovf_cap, uint64_t ovf_known,
                              uint64_t key_bytes) {
    RoundPlan r{};
    r.park_full = -1;
    r.novf = std::min(cx[L.novf()], ovf_cap);  // never drain past the buffer
    r.newly_parked = r.novf - std::min(r.novf, ovf_known);
    for (int p = 0; p < (int)L.W; ++p) {
        const uint64_t out = cx[L.sent(p) + kRowKeys], in = cx[L.recv(p) + kRowKeys], fl = cx[L.recv(p) + kRowFlags];
        if ((fl & kFlagParkFull) && r.park_full < 0) r.park_full = p;
        r.global_more |= (fl & kFlagMore) != 0;
        r.global_sends |= (fl & kFlagSends) != 0;
        r.keys.scnt[p] = out * key_bytes;
        r.keys.soff[p] = (uint64_t)p * kcap * key_bytes;
        r.keys.rcnt[p] = in * key_bytes;
        r.keys.roff[p] = r.tot_in * key_bytes;
        // block p of rep_out (the keys from p) back to p; from p into rep_in + p * kcap
        r.replies.scnt[p] = in;
        r.replies.soff[p] = r.tot_in;
        r.replies.rcnt[p] = out;
        r.replies.roff[p] = (uint64_t)p * kcap;
        r.tot_in += in;
        r.mx = std::max(r.mx, out);
        r.keys_sent += out;
    }
    return r;
}

// Phase 2, from the accept counts sa = {[W] states to send per owner, [W] states
// to receive per source} (k_materialize_remote, k_owner_insert): st_out
// [W][kcap] -> st_in, packed in rank order (state_bytes each).  Verification
// ships every key's state, the seen ones to be compared.
struct StatePlan {
    PeerBlocks states;
    uint64_t tot_st;       // state records this rank receives
    uint64_t states_sent;
    bool over;             // more accepted states for a peer than the keys it was sent
};
inline StatePlan state_blocks(const uint64_t* sa, const uint64_t* cx, CountRow L, int me, uint64_t kcap,
                              uint64_t state_bytes, bool verify) {
    StatePlan s{};
    for (int p = 0; p < (int)L.W; ++p) {
        const uint64_t ns = sa[p], nr = verify ? cx[L.recv(p) + kRowKeys] : sa[L.W + (uint64_t)p];
        if (p != me && ns > kcap) s.over = true;
        s.states.soff[p] = (uint64_t)p * kcap * state_bytes;
        s.states.scnt[p] = p == me ? 0 : ns * state_bytes;
        s.states.rcnt[p] = p == me ? 0 : nr * state_bytes;
        s.states.roff[p] = s.tot_st * state_bytes;
        s.tot_st += p == me ? 0 : nr;
        if (p != me) s.states_sent += ns;
    }
    return s;
}

// ---- round sizing -----------------------------------------------------------------
// A large level takes at least `split` rounds, so one round's count exchange
// and read-back overlap the next round's expansion.
inline uint64_t split_cap(uint64_t frontier, int split) {
    return frontier >= (1ull << 21) ? (frontier + (uint64_t)split - 1) / (uint64_t)split : frontier;
}
// States of the next round, `rest` of the level left.  rho = most keys one round
// sends one owner, per expanded state: a round aims at an outbox `fill` full (what
// does not fit is parked, not lost).  The rest goes in equal rounds of at most
// that size — not full rounds and a small remainder: a small round idles most of
// the grid.
inline uint64_t round_states(uint64_t rest, uint64_t kcap, double fill, double rho, uint64_t split_cap,
                             uint64_t max_launch) {
    const uint64_t target = (uint64_t)(fill * (double)kcap / std::max(rho, 0.02));
    const uint64_t cap = std::max<uint64_t>(1, std::min<uint64_t>({max_launch, target, split_cap}));
    const uint64_t nr = (rest + cap - 1) / cap;
    return (rest + nr - 1) / nr;
}
// rho after an expansion round of `states` (> 0): the keys per state of its fullest
// owner, parked ones included; an old peak decays by half a round (rho varies along
// a frontier: states received from other ranks are appended after the local ones).
inline double next_rho(double rho, uint64_t mx, uint64_t newly_parked, uint64_t states) {
    return std::max(0.5 * rho, (double)(mx + newly_parked) / (double)states);
}

}  // namespace rmc_host
