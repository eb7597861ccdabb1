// rmc_wide_plan.h — how a wide ctx divides its HBM budget (create_wide,
// rmc_wide.cpp): states, fingerprint-set slots, ring window.  Host arithmetic
// only (no HIP), so a host test can check it (tests/native/wide_plan_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>

#include "rmc_plan.h"  // set_slots_of: WidePlanIn.set_slots from rmc_config.set_bytes

namespace rmc_host {

struct WidePlanIn {
    uint64_t budget;          // bytes the ctx may take (a share of the free HBM)
    uint64_t rec;             // bytes of the store's record (5,080, 904 or 336)
    uint64_t state_capacity;  // rmc_config.state_capacity (0: sized from the budget)
    uint64_t set_slots;       // slots of rmc_config.set_bytes (0: sized from the capacity)
    uint64_t device_window;   // rmc_config.device_window (ring only; 0: what the rest leaves)
    bool ring;                // RMC_FLAG_SPILL
    bool verify;              // RMC_FLAG_VERIFY_STATES (resident only): a second 8 B per slot
    uint64_t vcap;            // (the slot's owner, WideBufs.sidx) and vcap 16-B deferred hits
};
struct WidePlan {
    uint64_t cap;     // states (records without the ring, links always)
    uint64_t slots;   // fingerprint-set slots, a power of two >= 2 cap
    uint64_t window;  // records of the ring (= cap without it)
    bool cap_exceeds_set;  // state_capacity beyond what a set of set_bytes holds (RMC_E_INVAL)
};

// Bytes of a ctx planned this way (what create_wide allocates, bar the counters).
inline uint64_t wide_plan_bytes(const WidePlanIn& in, const WidePlan& p) {
    return p.window * in.rec + p.cap * 9 + p.slots * (in.verify ? 16 : 8) + (in.verify ? in.vcap * 16 : 0);
}

inline WidePlan wide_plan(const WidePlanIn& in) {
    WidePlan p{};
    const uint64_t rec = in.rec, per_state = rec + 8 + 1;
    const uint64_t slot_b = in.verify ? 16 : 8;  // key (+ owner index)
    // verification's deferred-hit buffer comes off the top
    const uint64_t budget = in.budget - std::min<uint64_t>(in.budget, in.verify ? in.vcap * 16 : 0);
    uint64_t set_slots = in.set_slots, cap = in.state_capacity;
    if (in.ring && set_slots && cap) {
        // as on the packed layout, set_bytes is an upper bound: halved (down to load
        // 1/2) until the links of every state and the window fit beside the set
        const uint64_t need_win = in.device_window ? in.device_window : cap / 4;
        while (set_slots > 1024 && set_slots / 2 >= 2 * cap && set_slots * 8 + cap * 9 + need_win * rec > budget)
            set_slots >>= 1;
    }
    if (set_slots && cap > set_slots / 2) {
        p.cap_exceeds_set = true;
        return p;
    }
    if (cap == 0 && in.ring) {
        // state_capacity sizes the set and the links only: what the given set holds,
        // else the largest set of at most half the budget, two slots per state
        uint64_t sl = 1ull << 20;
        while (sl * 16 <= budget / 2) sl <<= 1;
        cap = set_slots ? set_slots / 2 : sl / 2;
    } else if (cap == 0) {
        // the set takes 2 to 4 slots per state (the next power of two): 4 budgeted
        cap = set_slots ? std::min<uint64_t>(set_slots / 2, (budget - std::min<uint64_t>(budget, set_slots * slot_b)) / per_state)
                        : budget / (per_state + 4 * slot_b);
    }
    cap = std::max<uint64_t>(std::min<uint64_t>(cap, 1ull << 33), 1024);
    uint64_t slots = 1;
    while (slots < 2 * cap) slots <<= 1;
    if (set_slots) slots = std::max(slots, set_slots);
    // the ring window: device_window records exactly (no rounding to a power of
    // two: at 336 B to 5 KB a record, the round-up could cost tens of GB), or what
    // the budget leaves after the set and the links, at most every state
    uint64_t win = cap;
    if (in.ring) {
        const uint64_t fixed = slots * 8 + cap * 9;
        win = in.device_window ? in.device_window : (budget - std::min<uint64_t>(budget, fixed)) / rec;
        win = std::max<uint64_t>(std::min<uint64_t>(win, cap), 1024);
    }
    p.cap = cap;
    p.slots = slots;
    p.window = win;
    return p;
}

}  // namespace rmc_host
