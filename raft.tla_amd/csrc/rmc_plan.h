// rmc_plan.h — how a packed ctx divides its HBM budget (rmc_create, rmc_api.cpp):
// states, fingerprint-set slots, spill window, where the trace links live; and
// the launch sizing of the ring window, shared with the wide layout; and the set
// epoch a run takes (single-GPU and sharded, tests/native/dist_plan_check.cpp).  Host
// arithmetic only (no HIP, no getenv), so a host test can check it
// (tests/native/packed_plan_check.cpp against tests/golden/packed_plan_cases.txt).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace rmc_host {

// rmc_config.set_bytes -> fingerprint-set slots: the largest power of two of
// 8-B slots within the bytes (at least 1024), 0 when the set is sized automatically
inline uint64_t set_slots_of(uint64_t bytes) {
    if (bytes == 0) return 0;
    uint64_t sl = 1024;
    while ((sl << 1) * 8 <= bytes) sl <<= 1;
    return sl;
}

// The set epoch of a run (raft_packed.h c_set_ep).  A run on a ctx whose set holds
// the tagged entries of an earlier run takes the next epoch and clears nothing:
// their slots read as empty.  The first run of a ctx, every ep_max-th one and a
// run that cannot tag its set (tagged = false: verification, whose slot -> state
// map is cleared anyway; sharded SYMMETRY, whose sent-cache kernel recovers raw
// keys from set values) clear the set.  ep_max is RMC_SET_EPOCH (255; 0: every
// run clears).  Epoch 0 is an untagged set.
struct SetEpoch {
    uint32_t epoch;  // the epoch to run with
    bool clear;      // clear the set first
};
inline SetEpoch next_set_epoch(uint32_t current, uint32_t ep_max, bool tagged) {
    if (ep_max > 0 && tagged && current >= 1 && current < ep_max) return {current + 1, false};
    return {ep_max > 0 && tagged ? 1u : 0u, true};
}

struct PackedPlanIn {
    uint64_t budget;          // bytes the ctx may take (a share of the free HBM)
    uint64_t state_words;     // NW: 32-bit words per packed state
    uint64_t state_capacity;  // rmc_config.state_capacity (0: sized from the budget)
    uint64_t set_slots;       // slots of rmc_config.set_bytes (0: sized from the capacity)
    uint64_t device_window;   // rmc_config.device_window (spill only; 0: what the rest leaves)
    bool spill;               // RMC_FLAG_SPILL
    bool verify;              // RMC_FLAG_VERIFY_STATES
    bool host_links;          // RMC_SPILL_HOST_LINKS=1: never keep the trace links in HBM
};
struct PackedPlan {
    uint64_t cap;        // all states (fingerprint-set sizing; the store's without spill)
    uint64_t slots;      // fingerprint-set slots, a power of two >= 2 cap
    uint64_t window;     // states resident on the device (= cap without spill)
    uint64_t link_cap;   // trace links on the device: cap with dev_links, else the window
    uint64_t set_slots;  // in.set_slots after the halving below (0: none given)
    bool dev_links;      // the links of every state stay in HBM and the window is a ring
    bool cap_exceeds_set;  // state_capacity beyond the set_slots / 2 states the given set holds
                           // (RMC_E_INVAL): only set_slots is planned
};

constexpr uint64_t kLinkBytes = 9;                     // trace link per state: parent index + action lane
constexpr uint64_t kVerifyHitReserve = 2ull << 30;     // verify + spill: the two hit buffers (vbuf, hbuf), 1 GiB each
inline uint64_t slot_bytes(bool verify) { return verify ? 16 : 8; }  // key (+ the slot's owner index)
inline uint64_t window_bytes_per_state(uint64_t state_words) { return state_words * 4 + 8 + 1; }  // state, footprint, class

// Bytes of a ctx planned this way: the allocations rmc_create sizes from the
// plan (window, links, set) and the reserve the plan makes for the hit buffers.
// Not in it, as they were never budgeted: the counters, the launch's presort
// words (B.word: 2 B per state of the largest launch, min(2^28, the window) states, so up
// to 512 MiB where it was 64 MiB), staging, the SYMMETRY tie buffer — and the one 1-GiB
// hit buffer of a resident verifying ctx, which only the spilled plan reserves; it comes out of
// the share of free HBM the budget leaves.
inline uint64_t packed_plan_bytes(const PackedPlanIn& in, const PackedPlan& p) {
    return p.window * window_bytes_per_state(in.state_words) + p.link_cap * kLinkBytes + p.slots * slot_bytes(in.verify) +
           (in.verify && in.spill ? kVerifyHitReserve : 0);
}

inline PackedPlan packed_plan(const PackedPlanIn& in) {
    PackedPlan p{};
    const uint64_t wbytes = window_bytes_per_state(in.state_words), per_state = wbytes + kLinkBytes;
    const uint64_t sb = slot_bytes(in.verify), budget = in.budget;
    // the window a spilled search asks for: verification keeps a smaller ring (its
    // set is twice the size), an eighth of the states
    auto need_win = [&](uint64_t cap) { return in.device_window ? in.device_window : cap / (in.verify ? 8 : 4); };
    uint64_t cap = in.state_capacity, set_slots = in.set_slots;
    if (set_slots && cap) {
        // set_bytes is an upper bound: halved (down to load 1/2) until the store fits
        // beside it — the states, or spilling the device trace links and the window
        const uint64_t store = in.spill ? cap * kLinkBytes + need_win(cap) * wbytes : cap * per_state;
        while (set_slots > 1024 && set_slots / 2 >= 2 * cap && set_slots * sb + store > budget) set_slots >>= 1;
    }
    p.set_slots = set_slots;
    if (set_slots && cap > set_slots / 2) {
        p.cap_exceeds_set = true;
        return p;
    }
    if (cap == 0 && set_slots) {
        // the given set holds set_slots / 2 states; the store fills what the set leaves
        cap = set_slots / 2;
        if (!in.spill) cap = std::min<uint64_t>(cap, (budget - std::min<uint64_t>(budget, set_slots * sb)) / per_state);
    } else if (cap == 0) {
        // table <= 4 slots per state after pow2 rounding (+ as many sidx words when verifying);
        // spilling: the largest set of at most half the budget, two slots per state
        if (in.spill) {
            // (8 B * (2 sl) <= budget / 2; verification: the set and its slot -> index
            // map, 16 B per slot, <= 2/3 of the budget — the loops charge twice that
            // per slot because the final sl is twice the last one that passed)
            uint64_t sl = 1ull << 20;
            while (in.verify ? sl * 32 <= budget / 3 * 2 : sl * 16 <= budget / 2) sl <<= 1;
            cap = sl / 2;
        } else {
            cap = budget / (per_state + 4 * sb);
        }
        cap = std::min<uint64_t>(cap, 1ull << 36);  // (only a derived capacity is clamped)
    }
    cap = std::max<uint64_t>(cap, 1024);
    uint64_t slots = 1;
    while (slots < 2 * cap) slots <<= 1;
    if (set_slots) slots = std::max(slots, set_slots);
    // spilling: the trace links of every state stay on the device when that leaves
    // a window of at least need_win states; otherwise, or with host_links, they
    // move to the host with the spilled levels
    uint64_t win = cap;
    if (in.spill) {
        const uint64_t fixed = slots * sb + (in.verify ? kVerifyHitReserve : 0);
        const uint64_t rest = budget - std::min<uint64_t>(budget, fixed), links = cap * kLinkBytes;
        p.dev_links = !in.host_links && rest > links && (rest - links) / wbytes >= need_win(cap);
        win = in.device_window;
        if (win == 0) win = p.dev_links ? (rest - links) / wbytes : rest / per_state;
        win = std::max<uint64_t>(std::min<uint64_t>(win, cap), 1024);
        if (p.dev_links) {
            // the window is a ring of a power of two states (DevBufs.wmask): a
            // given window rounds up (past cap, even), librmc's own sizing down
            uint64_t p2 = 1024;
            while (p2 < win) p2 <<= 1;
            win = (in.device_window || p2 == win) ? p2 : p2 >> 1;
        }
    }
    p.cap = cap;
    p.slots = slots;
    p.window = win;
    p.link_cap = p.dev_links ? cap : win;
    return p;
}

// ---- launch sizing of the ring window ---------------------------------------------
// The most new states one state's expansion can yield: every lane yields at most
// one, and the guards of raft.tla's Next (raft.tla:421-430) enable per server i at
// most Restart + Timeout (a Follower, :136,146), Restart + Timeout + S x RequestVote +
// BecomeLeader (a Candidate, :157-158,195-196) or Restart + V x ClientRequest +
// AdvanceCommitIndex + (S - 1) x AppendEntries (a Leader, :171-173,206-207,219-220),
// plus Receive, Duplicate and Drop per message of the bag.
inline uint64_t new_states_bound(uint64_t S, uint64_t V, uint64_t bag) {
    return S * std::max<uint64_t>(std::max<uint64_t>(2, S + 3), S + V + 1) + 3 * bag;
}
// ... of the packed layout: never more than its lanes
inline uint64_t packed_new_states_bound(uint64_t lanes, uint64_t S, uint64_t V, uint64_t K) {
    return std::min(lanes, new_states_bound(S, V, K));
}
// The ring holds [a, count) live — the rest of the frontier and the level being
// built — so a launch of n states, each yielding at most `bound` new ones,
// overwrites no live state when count + n * bound <= a + win: the states' room.
inline uint64_t ring_room(uint64_t count, uint64_t a, uint64_t win) { return count - a < win ? a + win - count : 0; }

// ---- device-side admission of a ring launch -----------------------------------------
// A launch of the dynamic-unit kernel (rmc_units.h) need not be sized by the bound: no
// unit is claimed once the count is above the stop, live_lo + win - reserve,
// where live_lo is the oldest state the launch still reads and the reserve is what the
// launch's waves can add after the count has passed the stop.  The flushes see the count
// (their allocation returns it); the claims do not read it.  Take the first flush that
// takes the count above the stop.  From it on every flush raises the stop bit of the
// work counter (rmc_units.h kStopBit) before its wave's next claim — both are atomics of
// one lane on one word — so after its first flush from then on a wave claims nothing:
// it adds what its list carried, at most list_cap entries, and the new states of the
// unit it is in, at most unit_states * bound.  So the count never passes stop +
// reserve = live_lo + win, and no state at or above live_lo is overwritten.

// Tiles per window of a presorted launch of nf states on `grid` blocks (expand_body's
// and k_window_order's wt): wt_max, fewer when every block would not get a full window.
inline uint64_t launch_window_tiles(uint64_t nf, uint64_t grid, uint64_t wt_max) {
    const uint64_t per_block = (nf + grid * 256 - 1) / (grid * 256);
    return per_block < wt_max ? (per_block ? per_block : 1) : wt_max;
}
// States of the launch's unit: a wave's 64 positions of at most unit_tiles of a window's wt tiles.
inline uint64_t unit_states(uint64_t wt, uint64_t unit_tiles) { return std::min(wt, unit_tiles) * 64; }
// `waves`: the launch's, and never more than the units it has left to claim (a re-launch
// near the end of its range: a wave without a unit adds nothing, its list starts empty).
inline uint64_t admit_reserve(uint64_t waves, uint64_t units_left, uint64_t unit_states, uint64_t bound,
                              uint64_t list_cap) {
    return std::min(waves, units_left) * (unit_states * bound + list_cap);
}
// No reserve is needed where the store's capacity ends before the ring wraps onto live_lo:
// the store limit alone (a capacity error) keeps every live state.
inline bool admit_needs_reserve(uint64_t cap, uint64_t live_lo, uint64_t win) { return cap > live_lo + win; }
// The count above which no unit is claimed, under the launch's store limit `lim`
// (launch_store_limit below: live_lo + win on the ring); 0: the reserve alone exceeds it.
// The device holds the reserve in 32 bits (DevBufs.admit_reserve) and compares
// count + reserve > lim.
inline uint64_t admit_stop(uint64_t lim, uint64_t reserve) { return lim > reserve ? lim - reserve : 0; }
constexpr uint64_t kAdmitReserveMax = 0xFFFFFFFFull;
// The reserve fits: the launch starts below its stop, so its first claims get units.  (The
// condition under which the device stops claiming, negated: count > admit_stop stops.)
inline bool admit_fits(uint64_t count, uint64_t stop) { return stop > count; }
// A launch over [lo, lo + nf) that stopped with wnext units claimed (rmc_units.h
// units_claimed; each one finished): the first state of the first window not fully claimed — units
// are claimed window-major, groups_x4 = 4 * unit_groups(wt, ut) per window — which the
// re-launch takes as its live_lo.
inline uint64_t admit_live_lo(uint64_t lo, uint64_t nf, uint64_t wnext, uint64_t wt, uint64_t groups_x4) {
    return lo + std::min(nf, wnext / groups_x4 * 256 * wt);
}
// The store index no flush may reach in a launch: the capacity, and on the ring live_lo + win.
inline uint64_t launch_store_limit(uint64_t cap, bool ring, uint64_t live_lo, uint64_t win) {
    return ring ? std::min(cap, live_lo + win) : cap;
}

}  // namespace rmc_host
