// Host check of the wide ctx's HBM division (rmc_wide_plan.h wide_plan, the
// arithmetic of create_wide): under full-state verification the set's second
// 8 B per slot and the deferred-hit buffer are part of the plan, and with
// state_capacity = 0 on a 288-GB device the 499,414,539 states of MCraft.cfg as
// shipped at depth 14 (336-B records) still fit resident.
// Build: g++ -O2 -std=c++17 -I raft.tla_amd/csrc wide_plan_check.cpp
// Run:   ./a.out   (prints "ok ..." or the first failure)
#include <cstdio>

#include "rmc_wide_plan.h"

using namespace rmc_host;

static int bad(const char* what, const WidePlan& p) {
    printf("FAIL %s: cap %llu slots %llu window %llu\n", what, (unsigned long long)p.cap, (unsigned long long)p.slots,
           (unsigned long long)p.window);
    return 1;
}

int main() {
    const uint64_t D14 = 499414539ull;            // profiles/r06/wide/mcraft_shipped_d14_depthrec.jsonl
    const uint64_t free_hbm = 288ull * 1000000000ull;  // no more than a 288-GB device reports free
    WidePlanIn in{};
    in.budget = (uint64_t)((double)free_hbm * 0.80);
    in.rec = 336;
    in.verify = true;
    in.vcap = 1ull << 26;
    const WidePlan v = wide_plan(in);
    if (v.cap_exceeds_set || v.cap < D14) return bad("depth 14 does not fit resident under verification", v);
    if (v.slots < 2 * v.cap || (v.slots & (v.slots - 1))) return bad("set below two slots per state", v);
    if (v.window != v.cap) return bad("resident plan with a window", v);
    if (wide_plan_bytes(in, v) > in.budget) return bad("plan beyond its budget", v);
    // without the flag: today's division, 32 B of set per state budgeted
    WidePlanIn pl = in;
    pl.verify = false;
    pl.vcap = 0;
    const WidePlan p = wide_plan(pl);
    if (p.cap != in.budget / (336 + 9 + 32)) return bad("plain capacity changed", p);
    if (p.cap <= v.cap) return bad("verification costs nothing?", p);
    if (wide_plan_bytes(pl, p) > pl.budget) return bad("plain plan beyond its budget", p);
    // every record, given and derived capacities, small and large budgets: within the budget
    const uint64_t recs[3] = {336, 904, 5080};
    for (uint64_t rec : recs)
        for (uint64_t gb : {1ull, 8ull, 64ull, 192ull, 288ull})
            for (int verify = 0; verify < 2; ++verify) {
                WidePlanIn q{};
                q.budget = gb * 800000000ull;
                q.rec = rec;
                q.verify = verify != 0;
                q.vcap = verify ? 1ull << 20 : 0;
                const WidePlan r = wide_plan(q);
                if (r.slots < 2 * r.cap || wide_plan_bytes(q, r) > q.budget) return bad("derived plan", r);
            }
    // a set given by set_bytes: capacity from what it leaves, never more than half its slots
    WidePlanIn s = in;
    s.set_slots = 1ull << 31;
    const WidePlan g = wide_plan(s);
    if (g.slots != s.set_slots || g.cap > g.slots / 2 || wide_plan_bytes(s, g) > s.budget) return bad("given set", g);
    s.state_capacity = (1ull << 30) + 1;
    if (!wide_plan(s).cap_exceeds_set) return bad("capacity beyond the given set accepted", g);
    printf("ok depth-14 verified plan: %llu states, %llu slots, %.1f GB of a %.1f GB budget\n",
           (unsigned long long)v.cap, (unsigned long long)v.slots, wide_plan_bytes(in, v) / 1e9, in.budget / 1e9);
    return 0;
}
