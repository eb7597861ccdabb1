// rmc_dev_state.h — packed state records on the device: load / store, the successor
// re-derivation, the commit of new states (store slot, trace link, footprint, class, fused
// invariant check), the per-wave new-state list's flush and the wave reductions.
#pragma once
#include <hip/hip_runtime.h>

#include "raft_packed.h"
#include "rmc_dev_set.h"
#include "rmc_internal.h"
#include "rmc_units.h"

namespace rmc {

template <int S, int K>
__device__ __forceinline__ void load_state(const u32* __restrict__ base, u64 (&w)[S], u32 (&m)[K]) {
    const u64* ws = reinterpret_cast<const u64*>(base);
#pragma unroll
    for (int i = 0; i < S; ++i) w[i] = ws[i];
    // Records are 8-byte aligned (2S + K words, K even), so the bag is read
    // as 8-byte pairs: a 16-byte load would be misaligned for odd S.
    if constexpr (K % 2 == 0) {
        const uint2* ms = reinterpret_cast<const uint2*>(base + 2 * S);
#pragma unroll
        for (int q = 0; q < K / 2; ++q) {
            const uint2 v = ms[q];
            m[2 * q] = v.x; m[2 * q + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int q = 0; q < K; ++q) m[q] = base[2 * S + q];
    }
}

template <int S, int K>
__device__ __forceinline__ void store_state(u32* __restrict__ base, const u64 (&w)[S], const u32 (&m)[K]) {
    u64* ws = reinterpret_cast<u64*>(base);
#pragma unroll
    for (int i = 0; i < S; ++i) ws[i] = w[i];
#pragma unroll
    for (int q = 0; q < K; ++q) base[2 * S + q] = m[q];
}

// Successor re-derivation: the kernels keep (parent, lane) for a successor and
// run the lane's code again where they need the successor itself (same code,
// deterministic): load the parent record, the lane's delta, materialise.
// Used by the kernels outside the expansion launch.  The flushes of the
// expansion kernels and k_materialize_remote, which also need the footprint
// (through the lane's descriptor in the sorted kernels), keep the steps written
// out: through a helper their register allocation changes (spill counts, an
// instruction or two), and those kernels are pinned to their measured code.
template <int S, int K>
__device__ __forceinline__ void derive_succ(const u32* parent, int lane, const Params& P, u64 (&wo)[S],
                                            u32 (&mo)[K]) {
    u64 w[S];
    u32 m[K];
    load_state<S, K>(parent, w, m);
    Delta d;
    lane_delta<S, K>(w, m, lane, P, d);
    materialise<S, K>(w, m, d, wo, mo);
}

// Store one new state at index ni: the packed state, its trace link (global
// parent ref, lane), the footprint of its discovering lane (commuting
// diamonds; only shapes whose kernels skip diamonds keep them), its
// window-sort class (B.cls: a layout hint, read 1 B per state by the next
// level's window sort) and the fused invariant check.
template <int S, int K>
__device__ __forceinline__ void store_new(const Params& P, const DevBufs& B, u64 ni, const u64 (&wo)[S],
                                          const u32 (&mo)[K], u64 parent, int lane, u64 foot) {
    const u64 sl = wslot(B, ni);  // the ring window's slot (= ni unless spilling with links in HBM)
    store_state<S, K>(B.store + sl * (u64)(2 * S + K), wo, mo);
    B.parent[ni] = parent;
    B.act[ni] = (uint8_t)lane;
    B.foot[sl] = foot;
    B.cls[sl] = (uint8_t)state_class_fine<S, K>(wo, mo);
    const int v = check_invariants<S, K>(wo, mo, P);
    if (v) atomicMin((unsigned long long*)&B.ctr->viol, (unsigned long long)((ni << 4) | (u64)(v - 1)));
}

// Wave-aggregated allocation of store slots for the lanes with is_new set,
// then materialise + store + parent + invariants.  Must be reached by every
// lane of the wave (it contains a ballot).
template <int S, int K>
__device__ __forceinline__ void commit_new(int is_new, const u64 (&w)[S], const u32 (&m)[K], const Delta& d,
                                           const Params& P, const DevBufs& B, u64 parent_idx, int lane) {
    const u64 bal = __ballot(is_new);
    if (bal == 0) return;
    const int me = (int)__lane_id();
    const int leader = __ffsll((long long)bal) - 1;
    u64 base = 0;
    if (me == leader) base = atomicAdd((unsigned long long*)&B.ctr->count, (unsigned long long)__popcll(bal));
    base = bcast64(base, leader);
    if (!is_new) return;
    const u64 ni = base + (u64)__popcll(bal & ((1ull << me) - 1ull));
    if (ni >= B.lim) {
        atomicOr(&B.ctr->overflow, 1u);
        return;
    }
    u64 wo[S];
    u32 mo[K];
    materialise<S, K>(w, m, d, wo, mo);
    // initial states and deferred SYMMETRY ties: no diamond skipping from them
    store_new<S, K>(P, B, ni, wo, mo, parent_idx, lane, 0ull);
}

// Per-wave list of new states, kept in LDS until a flush materialises them.
constexpr int WCAP = 512;

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Replicated levels (sharded mode): one record per frontier state of the
// whole level, gathered from every rank — the packed state, its global ref
// (rank << 48 | index), its footprint and lane | class << 8 (k_pack_rep).
template <int S, int K>
struct RepRec {
    static constexpr int NW = 2 * S + K;
    static constexpr int REF = NW, FOOT = NW + 2, ACT = NW + 4;
    static constexpr int RR = NW + 6;  // words per record (8-byte aligned: NW is even)
};

// Materialise the wave's n listed new states: ONE global allocation atomic per
// flush, then each lane re-derives one listed successor from its parent
// (same lane_delta code, deterministic), stores it, its parent pointer and
// lane, and runs the fused invariant checks.  Convergent: the whole wave
// runs it together, so the rare new-state path does not serialise the
// per-lane expansion loop.  REP: the parents are replicated-level records
// (B.rep), their refs global.
template <int S, int K, bool REP = false, bool ADMIT = false>
__device__ __forceinline__ void flush_new(const Params& P, const DevBufs& B, u64 lo, const u32* l_rel,
                                          const uint8_t* l_lane, u32 n) {
    constexpr int NW = 2 * S + K;
    typedef RepRec<S, K> RR;
    wave_sync_lds();
    const int me = (int)__lane_id();
    u64 base = 0;
    if (me == 0) {
        base = atomicAdd((unsigned long long*)&B.ctr->count, (unsigned long long)n);
        // ADMIT: the count is past the launch's admission stop — no further unit is claimed
        // (expand_body).  Lane 0 issues this before its wave's next claim, on the same word.
        if constexpr (ADMIT)
            if (base + n + B.admit_reserve > B.lim)
                atomicOr((unsigned long long*)&B.ctr->wnext, (unsigned long long)rmc_units::kStopBit);
    }
    base = bcast64(base, 0);
    for (u32 e = (u32)me; e < n; e += 64) {
        const u64 rel = l_rel[e];
        const int lane = l_lane[e];
        const u64 ni = base + e;
        if (ni >= B.lim) {  // the launch's limit: the capacity, on the ring the live window's end
            atomicOr(&B.ctr->overflow, 1u);
            continue;
        }
        u64 w[S];
        u32 m[K];
        const u32* pr = REP ? B.rep + (lo + rel) * (u64)RR::RR : B.store + wslot(B, lo + rel) * (u64)NW;
        load_state<S, K>(pr, w, m);
        Delta d;
        const u32 desc = P.ldesc[lane];  // the lane's descriptor: no family-offset compares
        lane_delta_desc<S, K>(w, m, desc, P, d);
        const u64 foot = make_foot_desc<S, K>(m, desc, d);
        u64 wo[S];
        u32 mo[K];
        materialise<S, K>(w, m, d, wo, mo);
        const u64 parent = REP ? ((u64)pr[RR::REF] | ((u64)pr[RR::REF + 1] << 32)) : B.ref_tag | (lo + rel);
        store_new<S, K>(P, B, ni, wo, mo, parent, lane, foot);
    }
    wave_sync_lds();
}

__device__ __forceinline__ u64 wave_or64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v |= (u64)(u32)__shfl_xor((int)(u32)v, off) | ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), off) << 32);
    // the same on every lane: make it a scalar so the lane dispatch stays scalar branches
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
    const u32 hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32));
    return ((u64)hi << 32) | lo;
}

// The OR over the wave's live states of lane_superset (raft_packed.h), built
// from one ballot per predicate instead of a shuffle reduction of the 64-bit
// masks: each bit of the mask is an OR of role / slot-occupancy predicates, so
// "some state of the wave has it" is a ballot.  Scalar result (SGPRs).
template <int S, int K>
__device__ __forceinline__ LaneMask lane_superset_wave(const u64 (&w)[S], const u32 (&m)[K], int V, bool live) {
    typedef Lanes<S, K> L;
    static_assert(L::N <= 128, "lane mask holds < 128 lanes");
    constexpr int O1 = L::off(1), O2 = L::off(2), O3 = L::off(3), O4 = L::off(4), O5 = L::off(5), O6 = L::off(6),
                  O7 = L::off(7), O8 = L::off(8), O9 = L::off(9);
    constexpr u64 SM = (1ull << S) - 1;
    LaneMask mk{0ull, 0ull};
    if (!__ballot(live)) return mk;
    mk.lo = SM;  // Restart(i): always enabled
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const u32 st = w_st(w[i]);
        if (__ballot(live && st != LEADER)) mk.put(1ull, O1 + i);
        if (__ballot(live && st == CANDIDATE)) { mk.put(SM, O2 + i * S); mk.put(1ull, O3 + i); }
        if (__ballot(live && st == LEADER)) {
            mk.put((1ull << V) - 1, O4 + i * VMAX);
            mk.put(1ull, O5 + i);
            mk.put(SM, O6 + i * S);
        }
    }
#pragma unroll
    for (int q = 0; q < K; ++q)
        if (__ballot(live && m[q] != 0u)) { mk.put(1ull, O7 + q); mk.put(1ull, O8 + q); mk.put(1ull, O9 + q); }
    return mk;
}

}  // namespace rmc
