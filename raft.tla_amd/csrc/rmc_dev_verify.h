// rmc_dev_verify.h — full-state verification of fingerprint hits (RMC_FLAG_VERIFY_STATES):
// the state / orbit comparisons and the kernels k_publish, k_verify, k_verify_host.
#pragma once
#include <hip/hip_runtime.h>

#include "raft_packed.h"
#include "rmc_dev_state.h"
#include "rmc_internal.h"

namespace rmc {

// ---- full-state verification (RMC_FLAG_VERIFY_STATES) ---------------------------
// TLC trusts its 64-bit fingerprints; this mode checks them.  Every successor
// whose fingerprint is already in the set is compared, field for field, with
// the stored state that owns that fingerprint.  A difference is a fingerprint
// collision (a distinct state the search would silently drop) and is counted.
// The slot -> store-index map (sidx) is published between launches
// (k_publish), so a hit on a state of a completed launch is checked inline
// and a hit on a state found in the same launch is deferred to k_verify.
template <int S, int K>
__device__ __forceinline__ bool same_state(const u64 (&w)[S], const u32 (&m)[K], const u32* __restrict__ st) {
    u64 w2[S];
    u32 m2[K];
    load_state<S, K>(st, w2, m2);
    bool eq = true;
#pragma unroll
    for (int i = 0; i < S; ++i) eq &= w[i] == w2[i];
#pragma unroll
    for (int q = 0; q < K; ++q) eq &= m[q] == m2[q];
    return eq;
}

// SYMMETRY: the successor and the stored state are the same orbit iff some
// server permutation maps one onto the other (bag re-sorted after permuting).
template <int S, int K>
__device__ __noinline__ bool same_orbit(const PackedState<S, K> a, const u32* __restrict__ st, const PermTable& PT) {
    u64 w2[S];
    u32 m2[K];
    load_state<S, K>(st, w2, m2);
    for (int p = 0; p < PT.np; ++p) {
        const u32 c = PT.code[p];
        u64 wp[S];
        u32 mp[K];
#pragma unroll
        for (int t = 0; t < S; ++t) {
            u64 v = 0;
#pragma unroll
            for (int i = 0; i < S; ++i) v |= pe(c, (u32)i) == (u32)t ? perm_word<S>(a.w[i], c) : 0ull;
            wp[t] = v;
        }
#pragma unroll
        for (int q = 0; q < K; ++q) mp[q] = perm_slot(a.m[q], c);
#pragma unroll
        for (int r = 0; r < K; ++r) {
#pragma unroll
            for (int q = (r & 1); q + 1 < K; q += 2) {
                const u32 x = mp[q], y = mp[q + 1];
                mp[q] = x > y ? x : y;
                mp[q + 1] = x > y ? y : x;
            }
        }
        bool eq = true;
#pragma unroll
        for (int i = 0; i < S; ++i) eq &= wp[i] == w2[i];
#pragma unroll
        for (int q = 0; q < K; ++q) eq &= mp[q] == m2[q];
        if (eq) return true;
    }
    return false;
}

// Check one fingerprint hit: 0 = the stored state equals the successor,
// 1 = it differs (a collision), 2 = the owner is not published yet (defer),
// 3 = no slot (table full, flagged by the insert).  Counting and deferral are
// aggregated by the caller (one atomic per wave, not per hit).
template <int S, int K, bool SYM>
__device__ __forceinline__ int verify_hit(const u64 (&w)[S], const u32 (&m)[K], int lane, u64 slot, const Params& P,
                                       const PermTable& PT, const DevBufs& B) {
    constexpr int NW = 2 * S + K;
    if (slot == ~0ull) return 3;
    const u64 ix = B.sidx[slot];
    if (ix == ~0ull) return 2;  // owner found in this launch: check after it
    if (ix < B.vlo) return 4;   // owner spilled: checked against its host copy after the launch
    Delta d;
    lane_delta<S, K>(w, m, lane, P, d);
    PackedState<S, K> o;
    materialise<S, K>(w, m, d, o.w, o.m);
    const u32* st = B.store + wslot(B, ix) * (u64)NW;
    if constexpr (SYM) return same_orbit<S, K>(o, st, PT) ? 0 : 1;
    return same_state<S, K>(o.w, o.m, st) ? 0 : 1;
}

__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += (u64)(u32)__shfl_xor((int)(u32)v, off) | ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), off) << 32);
    return v;
}

template <int S, int K, bool SYM>
__device__ __forceinline__ TKey verify_key(const u64 (&w)[S], const u32 (&m)[K], const Params& P, const PermTable& PT,
                                           u64 tmask) {
    return tkey(fp_weaken(SYM ? canon_state<S, K>(w, m, PT.code, PT.np) : state_fp<S, K>(w, m), P.fp_mask), tmask);
}

// sidx[slot of state i's fingerprint] = i for the stored states [lo, hi).
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_publish(const Params P, const PermTable PT, const DevBufs B, u64 lo, u64 hi) {
    constexpr int NW = 2 * S + K;
    for (u64 i = lo + (u64)blockIdx.x * 256ull + threadIdx.x; i < hi; i += (u64)gridDim.x * 256ull) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, i) * (u64)NW, w, m);
        const TKey key = verify_key<S, K, SYM>(w, m, P, PT, B.tmask);
        u64 s = key.s0;
        u64 n = 0;
        while (B.table[s] != key.v && n <= B.tmask) { s = (s + 1) & B.tmask; ++n; }
        if (n > B.tmask) atomicOr(&B.ctr->overflow, 8u);  // a stored state without its key
        else B.sidx[s] = i;
    }
}

// The deferred hits of the last launch, now that their owners are published.
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_verify(const Params P, const PermTable PT, const DevBufs B, u64 n) {
    constexpr int NW = 2 * S + K;
    u64 vchk = 0, vcol = 0;
    for (u64 q = (u64)blockIdx.x * 256ull + threadIdx.x; q < n; q += (u64)gridDim.x * 256ull) {
        const u64 parent = B.vbuf[2 * q], sl = B.vbuf[2 * q + 1];
        const u64 slot = sl & ((1ull << 56) - 1);
        const int lane = (int)(sl >> 56);
        PackedState<S, K> o;
        derive_succ<S, K>(B.store + wslot(B, parent) * (u64)NW, lane, P, o.w, o.m);
        const u64 ix = B.sidx[slot];
        if (ix == ~0ull) {
            atomicOr(&B.ctr->overflow, 8u);
            continue;
        }
        ++vchk;
        const u32* st = B.store + wslot(B, ix) * (u64)NW;  // found in this launch: in the window
        bool same;
        if constexpr (SYM) same = same_orbit<S, K>(o, st, PT);
        else same = same_state<S, K>(o.w, o.m, st);
        vcol += same ? 0u : 1u;
    }
    vchk = wave_sum64(vchk);
    vcol = wave_sum64(vcol);
    if (__lane_id() == 0 && vchk) atomicAdd((unsigned long long*)&B.ctr->vchecked, (unsigned long long)vchk);
    if (__lane_id() == 0 && vcol) atomicAdd((unsigned long long*)&B.ctr->collisions, (unsigned long long)vcol);
}

// Verification + spill: the hits hbuf[off, off + n) whose owners had left the
// device window, against the owners' host copies staged at `owners` (one
// record each, in hbuf order).  The parents are the launch's frontier states,
// still in the window (the ring never overwrites a launch's own frontier).
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_verify_host(const Params P, const PermTable PT, const DevBufs B,
                                                     const u32* owners, u64 n, u64 off) {
    constexpr int NW = 2 * S + K;
    u64 vchk = 0, vcol = 0;
    for (u64 q = (u64)blockIdx.x * 256ull + threadIdx.x; q < n; q += (u64)gridDim.x * 256ull) {
        const u64 parent = B.hbuf[2 * (off + q)];
        const int lane = (int)(B.hbuf[2 * (off + q) + 1] >> 56);
        PackedState<S, K> o;
        derive_succ<S, K>(B.store + wslot(B, parent) * (u64)NW, lane, P, o.w, o.m);
        const u32* st = owners + q * (u64)NW;
        bool same;
        if constexpr (SYM) same = same_orbit<S, K>(o, st, PT);
        else same = same_state<S, K>(o.w, o.m, st);
        ++vchk;
        vcol += same ? 0u : 1u;
    }
    vchk = wave_sum64(vchk);
    vcol = wave_sum64(vcol);
    if (__lane_id() == 0 && vchk) atomicAdd((unsigned long long*)&B.ctr->vchecked, (unsigned long long)vchk);
    if (__lane_id() == 0 && vcol) atomicAdd((unsigned long long*)&B.ctr->collisions, (unsigned long long)vcol);
}

}  // namespace rmc
