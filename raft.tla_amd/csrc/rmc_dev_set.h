// rmc_dev_set.h — the fingerprint set's device side (packed layout): the wave-aggregated
// reservation and the open-addressing insert of every inserting kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "raft_packed.h"

namespace rmc {

__device__ __forceinline__ u64 bcast64(u64 v, int src) {
    const u32 lo = (u32)__builtin_amdgcn_readlane((int)(u32)v, src);
    const u32 hi = (u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// Wave-aggregated reservation: the lanes with `want` set take consecutive
// indices from *ctr with ONE atomic (by the first of them); returns this
// lane's index (meaningful only where `want`).  Must be reached by every lane
// of the wave (it contains a ballot).  expand_body, commit_new and k_route keep
// the same steps written out: there the call shifts the kernels' register
// allocation (k_expand_sym +5 instructions, k_ties a spill), and those kernels
// are pinned to their measured code.
__device__ __forceinline__ u64 wave_reserve(bool want, unsigned long long* ctr) {
    const u64 bal = __ballot(want);
    if (bal == 0) return 0;
    const int me = (int)__lane_id();
    const int leader = __ffsll((long long)bal) - 1;
    u64 base = 0;
    if (me == leader) base = atomicAdd(ctr, (unsigned long long)__popcll(bal));
    base = bcast64(base, leader);
    return base + (u64)__popcll(bal & ((1ull << me) - 1ull));
}

// Open-addressing insert of a non-zero 64-bit value v whose probe sequence
// starts at slot s0, linear probing.
// Returns 1 if this lane inserted the key, 0 if it was present (or the table
// is full, flagged in *full).  Plain probe loads may be stale only in the
// EMPTY direction (slots go 0 -> key once); the CAS (agent scope, executed at
// the memory side) settles every race.
__device__ __forceinline__ int fp_insert(u64* __restrict__ table, u64 mask, u64 s0, u64 key, u32* full) {
    u64 s = s0;
    for (u64 n = 0; n <= mask; ++n) {
        const u64 cur = table[s];
        if (cur == key) return 0;
        if (fp_empty(cur)) {  // 0, or another epoch's entry (a tagged set)
            const u64 prev = atomicCAS((unsigned long long*)&table[s], (unsigned long long)cur, (unsigned long long)key);
            if (prev == cur) return 1;
            if (prev == key) return 0;
        }
        s = (s + 1) & mask;
    }
    atomicOr(full, 1u);
    return 0;
}

// fp_insert that also reports the slot holding the key (verification mode).
__device__ __forceinline__ int fp_insert_at(u64* __restrict__ table, u64 mask, u64 s0, u64 key, u32* full, u64* at) {
    u64 s = s0;
    for (u64 n = 0; n <= mask; ++n) {
        const u64 cur = table[s];
        if (cur == key) { *at = s; return 0; }
        if (fp_empty(cur)) {
            const u64 prev = atomicCAS((unsigned long long*)&table[s], (unsigned long long)cur, (unsigned long long)key);
            if (prev == cur) { *at = s; return 1; }
            if (prev == key) { *at = s; return 0; }
        }
        s = (s + 1) & mask;
    }
    atomicOr(full, 1u);
    *at = ~0ull;
    return 0;
}

// Same protocol, given the already-loaded content `cur` of the first slot s0.
__device__ __forceinline__ int fp_resolve(u64* __restrict__ table, u64 mask, u64 s0, u64 key, u64 cur, u32* full) {
    if (cur == key) return 0;
    if (fp_empty(cur)) {
        const u64 prev = atomicCAS((unsigned long long*)&table[s0], (unsigned long long)cur, (unsigned long long)key);
        if (prev == cur) return 1;
        if (prev == key) return 0;
    }
    return fp_insert(table, mask, s0, key, full);  // rare: continue linear probing
}
// Insert fingerprint h (raft_packed.h Fp) into the table.
__device__ __forceinline__ int fp_insert_fp(u64* __restrict__ table, u64 mask, const Fp& h, u32* full) {
    const TKey t = tkey(h, mask);
    return fp_insert(table, mask, t.s0, t.v, full);
}
// (fp_weaken, the rmc_set_fp_bits hook: raft_packed.h, shared with rmc_wide.hip)

}  // namespace rmc
