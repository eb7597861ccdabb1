// rmc_viol.h — continue past violations (RMC_FLAG_CONTINUE, TLC -continue): how a
// stored state is classified for rmc_violations, and the layout of the device
// tallies.  Host and device: the violation kernels (k_violations, k_wviolations)
// and the host check (tests/native/viol_check.cpp) call the same functions.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "raft_packed.h"
#include "raft_wide.h"

namespace rmc {

// The invariants of rmc.h (RMC_INV_COUNT), and the device tallies of one run, u64
// words: first[r], each[r], then least[r], the least index of a stored state that
// violates invariant r alone (~0: none).
constexpr int VIOL_INVS = 10;
constexpr int VIOL_FIRST = 0, VIOL_EACH = VIOL_INVS, VIOL_LEAST = 2 * VIOL_INVS, VIOL_WORDS = 3 * VIOL_INVS;

// One state against the mask: first = 0, or 1 + the index of the lowest bit of the
// mask that fails (the BFS's check, the notion of rmc_result.violated_inv); each =
// the bits of the mask that fail when checked alone.  The bits below `first` hold
// (it is the lowest that fails) and bit first - 1 fails, so only the bits above it
// are evaluated again, and a state that violates nothing costs the BFS's check.
struct ViolClass {
    int first;
    u32 each;
};

// Packed layout.  first: check_invariants<S, K>, the variant store_new calls.  A
// remaining bit alone (never TypeOK, the lowest) is what that function evaluates
// under a mask of that bit: check_named_invariants (out of line on the device).
template <int S, int K>
RMC_HD ViolClass classify_violations(const u64 (&w)[S], const u32 (&m)[K], const Params& P) {
    ViolClass c;
    c.first = check_invariants<S, K>(w, m, P);
    c.each = 0;
    if (!c.first) return c;
    c.each = 1u << (c.first - 1);
    const u32 rest = (u32)P.inv_mask & ~((2u << (c.first - 1)) - 1u);  // (bit 0 is below every other)
    if (!rest) return c;
    PackedState<S, K> s;
    for (int i = 0; i < S; ++i) s.w[i] = w[i];
    for (int q = 0; q < K; ++q) s.m[q] = m[q];
    for (int r = c.first; r < VIOL_INVS; ++r)
        if (((rest >> r) & 1u) && check_named_invariants<S, K>(s, 1 << r)) c.each |= 1u << r;
    return c;
}

namespace wide {
// Wide layout: wcheck_invariants, the check w_store runs, under the mask and
// under each remaining bit of it alone.
template <class St>
RMC_HD ViolClass wclassify_violations(const WModel& M, const St& s) {
    ViolClass c;
    c.first = wcheck_invariants(M, s);
    c.each = 0;
    if (!c.first) return c;
    c.each = 1u << (c.first - 1);
    const u32 rest = (u32)M.inv_mask & ~((2u << (c.first - 1)) - 1u);
    WModel M1 = M;
    for (int r = c.first; r < VIOL_INVS; ++r) {
        if (!((rest >> r) & 1u)) continue;
        M1.inv_mask = 1 << r;
        if (wcheck_invariants(M1, s)) c.each |= 1u << r;
    }
    return c;
}
}  // namespace wide

}  // namespace rmc
