// Host check of the packed ctx's HBM division (rmc_plan.h packed_plan, the
// arithmetic of rmc_create) and of the ring window's launch bound.
//  1. every line of the case file (tests/golden/packed_plan_cases.txt: recorded
//     from rmc_create's sizing before it became packed_plan) is recomputed and
//     must match exactly.  A line is
//       NW verify spill host_links budget state_capacity set_slots device_window
//       cap slots window link_cap dev_links cap_exceeds_set set_slots'
//     (set_slots': the given set after its halving, what the "exceeds" message quotes)
//  2. invariants of every plan that is not cap_exceeds_set
//  3. specs/MCraftBenchXL.cfg's shape on a 288-GB device: spill, everything derived
//  4. new_states_bound
// Build: g++ -O2 -std=c++17 -I raft.tla_amd/csrc packed_plan_check.cpp
// Run:   ./a.out tests/golden/packed_plan_cases.txt   (prints "ok ..." or the first failure)
#include <cstdio>

#include "rmc_plan.h"

using namespace rmc_host;
typedef unsigned long long ull;

static bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

static void show(const char* tag, const PackedPlanIn& in, const PackedPlan& p) {
    printf("%s NW %llu verify %d spill %d host_links %d budget %llu capacity %llu set %llu window %llu -> cap %llu slots "
           "%llu window %llu link_cap %llu dev_links %d exceeds %d set' %llu, %llu bytes\n",
           tag, (ull)in.state_words, in.verify, in.spill, in.host_links, (ull)in.budget, (ull)in.state_capacity,
           (ull)in.set_slots, (ull)in.device_window, (ull)p.cap, (ull)p.slots, (ull)p.window, (ull)p.link_cap,
           p.dev_links, p.cap_exceeds_set, (ull)p.set_slots, (ull)packed_plan_bytes(in, p));
}

int main(int argc, char** argv) {
    if (argc < 2) return printf("usage: packed_plan_check <case file>\n"), 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return printf("FAIL cannot open %s\n", argv[1]), 1;
    int cases = 0, exempt = 0, may_exempt = 0, exceeds = 0;
    for (;;) {
        ull v[15];
        int n = 0;
        while (n < 15 && fscanf(f, "%llu", &v[n]) == 1) ++n;
        if (n == 0) break;
        if (n != 15) return printf("FAIL case %d: %d fields\n", cases + 1, n), 1;
        ++cases;
        PackedPlanIn in{};
        in.state_words = v[0];
        in.verify = v[1] != 0;
        in.spill = v[2] != 0;
        in.host_links = v[3] != 0;
        in.budget = v[4];
        in.state_capacity = v[5];
        in.set_slots = v[6];
        in.device_window = v[7];
        const PackedPlan p = packed_plan(in);
        const bool same = p.cap_exceeds_set == (v[13] != 0) && p.set_slots == v[14] &&
                          (p.cap_exceeds_set || (p.cap == v[8] && p.slots == v[9] && p.window == v[10] &&
                                                 p.link_cap == v[11] && p.dev_links == (v[12] != 0)));
        if (!same) {
            show("FAIL mismatch:", in, p);
            return printf("  recorded: cap %llu slots %llu window %llu link_cap %llu dev_links %llu exceeds %llu set' %llu\n",
                          v[8], v[9], v[10], v[11], v[12], v[13], v[14]), 1;
        }
        const bool given = in.state_capacity || in.set_slots || in.device_window;
        if (given || in.budget == 2000000000ull) ++may_exempt;
        if (p.cap_exceeds_set) {
            ++exceeds;
            continue;
        }
        const char* bad = nullptr;
        if (!pow2(p.slots) || p.slots < 2 * p.cap) bad = "slots not a power of two >= 2 cap";
        else if (p.window > p.cap) bad = "window > cap";
        else if (p.dev_links && (!pow2(p.window) || p.link_cap != p.cap)) bad = "device links without a power-of-two ring";
        else if (!p.dev_links && p.link_cap != p.window) bad = "link_cap differs from the window";
        else if (packed_plan_bytes(in, p) > in.budget) {
            // a given value is honoured and the allocation left to fail; so are the floors
            if (given || p.cap == 1024 || p.window == 1024) ++exempt;
            else bad = "plan beyond its budget";
        }
        if (bad) return show("FAIL", in, p), printf("  %s\n", bad), 1;
    }
    fclose(f);
    if (cases != 648) return printf("FAIL %d cases, 648 expected\n", cases), 1;
    if (exempt > may_exempt) return printf("FAIL %d plans exempt from the budget, at most %d may be\n", exempt, may_exempt), 1;

    // MCraftBenchXL (S = 3, K = 4: 10 words) on a 288-GB device
    PackedPlanIn xl{};
    xl.budget = (uint64_t)(0.80 * 288e9);
    xl.state_words = 10;
    xl.spill = true;
    const PackedPlan x = packed_plan(xl);
    show("XL:", xl, x);
    if (x.cap_exceeds_set || !x.dev_links || !pow2(x.window) || x.slots < 2 * x.cap || !pow2(x.slots) ||
        x.link_cap != x.cap || packed_plan_bytes(xl, x) > xl.budget)
        return printf("FAIL the XL plan\n"), 1;

    // rmc_config.set_bytes -> slots: the largest power of two within the bytes, at least 1024
    if (set_slots_of(0) != 0 || set_slots_of(1) != 1024 || set_slots_of(8ull << 20) != 1ull << 20 ||
        set_slots_of((8ull << 20) - 1) != 1ull << 19)
        return printf("FAIL set_slots_of\n"), 1;
    // the guard-derived bound on one state's new states
    if (new_states_bound(3, 2, 4) != 30 || new_states_bound(5, 1, 8) != 64) return printf("FAIL new_states_bound\n"), 1;
    for (uint64_t S = 2; S <= 5; ++S)
        for (uint64_t V = 1; V <= 2; ++V)
            for (uint64_t K : {4ull, 8ull}) {
                const uint64_t lanes = 4 * S + 2 * S * S + S * 2 + 3 * K;  // Lanes<S, K> (raft_packed.h, VMAX = 2)
                const uint64_t b = packed_new_states_bound(lanes, S, V, K);
                if (b > lanes || b > new_states_bound(S, V, K)) return printf("FAIL packed bound S %llu\n", (ull)S), 1;
                if (packed_new_states_bound(7, S, V, K) != 7) return printf("FAIL bound above the lanes\n"), 1;
            }
    if (ring_room(100, 40, 64) != 4 || ring_room(104, 40, 64) != 0 || ring_room(200, 40, 64) != 0)
        return printf("FAIL ring_room\n"), 1;
    printf("ok %d cases (%d beyond a given set, %d of at most %d exempt from the budget)\n", cases, exceeds, exempt,
           may_exempt);
    return 0;
}
