// rmc_dev_cons.h — model-defined constraints on the packed layout (DESIGN.md "Model-defined
// constraints"; the index arithmetic: rmc_cons_plan.h).  After the seed and after each
// expansion launch, over the states it added, [nlo, nhi):
//  k_cons       : k_pred's structure (the program in LDS, a column of working memory per
//                 thread, the state read in place through PackedAcc) over tiles of 256
//                 states: one keep byte per state — every residual holds, or one's
//                 evaluation is an error (such a state stays, and is recorded in the word
//                 as k_pred records it) — and the kept count of each tile, by a wave
//                 ballot and popcount per 64 states.
//  (the exclusive scan of the tile counts: k_graph_scan, launch_graph_scan)
//  k_cons_holes : every position of the head [nlo, nlo + kept) that leaves writes itself
//                 into dst[its rank among them].
//  k_cons_move  : every state of the tail [nlo + kept, nhi) that stays moves — packed
//                 words, parent, lane, footprint, class — to dst[its rank from the end];
//                 Counters.count = nlo + kept; word[1] += the states moved.
//  k_cons_inv   : the built-in invariants (check_invariants, the fused check's and
//                 k_violations') on the kept states, the least index << 4 | invariant into
//                 Counters.viol: with constraints the expansion runs with its mask off, so
//                 no removed state is ever reported.
// Sources and destinations of the move are disjoint, so it runs in place; plain vector
// loads and stores only.
#pragma once
#include "rmc_cons_plan.h"
#include "rmc_dev_pred.h"
#include "rmc_dev_state.h"
#include "rmc_internal.h"

namespace rmc {

static_assert(cons::kConsTile == kPredThreads, "a block of k_cons is one tile");

// A position's kept rank inside its tile (every thread of the block calls it; s_w: 4 words).
__device__ __forceinline__ u32 cons_tile_rank(bool keep, u32* s_w) {
    const u64 ballot = __ballot(keep ? 1 : 0);
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    __syncthreads();  // (the last tile's readers are done with s_w)
    if (lane == 0) s_w[wave] = (u32)__popcll(ballot);
    __syncthreads();
    u32 before = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) before += q < wave ? s_w[q] : 0u;
    return before + cons::lane_rank(ballot, lane);
}

template <int S, int K>
__global__ __launch_bounds__(kPredThreads) void k_cons(const pred::Program* prog, const DevBufs B, u64 nlo, u64 nhi,
                                                       ConsBufs C, unsigned long long* word) {
    constexpr int NW = 2 * S + K;
    __shared__ PredLds L;
    __shared__ u32 s_w[4];
    pred_load(L, prog);
    const int n_pred = prog->n_pred;
    int* mem = L.mem + threadIdx.x;
    u64 err = ~0ull;
    nhi = nhi < B.cap ? nhi : B.cap;  // (a launch that overflowed the store is an error: the pass is not run)
    const u64 n = nhi > nlo ? nhi - nlo : 0, nt = cons::tiles(n);
    for (u64 tile = blockIdx.x; tile < nt; tile += gridDim.x) {
        const u64 p = tile * cons::kConsTile + threadIdx.x, i = nlo + p;
        bool keep = false;
        if (p < n) {
            const pred::PackedAcc<S, K> a{B.store + wslot(B, i) * (u64)NW};
            const int f = pred::first_failing<kPredThreads>(L.entry, n_pred, L.code, a, mem);
            const bool error = f && ((f - 1) & 1);
            keep = f == 0 || error;
            if (error && err == ~0ull) err = (i << 8) | (u64)(f - 1);
            C.keep[p] = keep ? 1 : 0;
        }
        const u64 ballot = __ballot(keep ? 1 : 0);
        __syncthreads();
        if ((threadIdx.x & 63u) == 0) s_w[threadIdx.x >> 6] = (u32)__popcll(ballot);
        __syncthreads();
        if (threadIdx.x == 0) C.cnt[tile] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
    err = pred_wave_min(err);
    if (__lane_id() == 0 && err != ~0ull) atomicMin(word, (unsigned long long)err);
}

template <int S, int K>
__global__ __launch_bounds__(256) void k_cons_holes(u64 n, ConsBufs C) {
    __shared__ u32 s_w[4];
    const u64 nt = cons::tiles(n), kept = C.off[nt];
    const u64 head_tiles = cons::tiles(kept);  // the tiles with a position below kept
    for (u64 tile = blockIdx.x; tile < head_tiles; tile += gridDim.x) {
        const u64 p = tile * cons::kConsTile + threadIdx.x;
        const bool live = p < n, keep = live && C.keep[p];
        const u64 kr = cons::kept_rank(C.off[tile], cons_tile_rank(keep, s_w));
        if (live && cons::is_hole(p, kept, keep)) C.dst[cons::hole_rank(p, kr)] = p;
    }
}

template <int S, int K>
__global__ __launch_bounds__(256) void k_cons_move(const DevBufs B, u64 nlo, u64 n, ConsBufs C,
                                                   unsigned long long* moved) {
    constexpr int NW = 2 * S + K;
    static_assert(NW % 2 == 0, "a packed state is copied as 64-bit pairs");
    __shared__ u32 s_w[4];
    const u64 nt = cons::tiles(n), kept = C.off[nt];
    u64 n_moved = 0;  // (lane 0 of each wave: the run's statistic, RMC_CONS_STATS)
    for (u64 tile = kept / cons::kConsTile + blockIdx.x; tile < nt; tile += gridDim.x) {
        const u64 p = tile * cons::kConsTile + threadIdx.x;
        const bool live = p < n, keep = live && C.keep[p];
        const u64 kr = cons::kept_rank(C.off[tile], cons_tile_rank(keep, s_w));
        const bool mover = live && cons::is_mover(p, kept, keep);
        const u64 movers = __ballot(mover ? 1 : 0);
        if (__lane_id() == 0 && movers) n_moved += (u64)__popcll(movers);
        if (!mover) continue;
        const u64 from = nlo + p, to = nlo + C.dst[cons::mover_rank(kept, kr)];
        const uint2* src = reinterpret_cast<const uint2*>(B.store + wslot(B, from) * (u64)NW);
        uint2* dst = reinterpret_cast<uint2*>(B.store + wslot(B, to) * (u64)NW);
#pragma unroll
        for (int q = 0; q < NW / 2; ++q) dst[q] = src[q];
        B.parent[to] = B.parent[from];
        B.act[to] = B.act[from];
        B.foot[wslot(B, to)] = B.foot[wslot(B, from)];
        B.cls[wslot(B, to)] = B.cls[wslot(B, from)];
    }
    if (n_moved) atomicAdd(moved, (unsigned long long)n_moved);
    if (blockIdx.x == 0 && threadIdx.x == 0) B.ctr->count = nlo + kept;
}

template <int S, int K>
__global__ __launch_bounds__(256) void k_cons_inv(const Params P, const DevBufs B, u64 lo, u64 hi) {
    constexpr int NW = 2 * S + K;
    u64 best = ~0ull;
    for (u64 i = lo + (u64)blockIdx.x * 256ull + threadIdx.x; i < hi; i += (u64)gridDim.x * 256ull) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, i) * (u64)NW, w, m);
        const int v = check_invariants<S, K>(w, m, P);
        if (v) {  // (ascending i per thread: the first is this thread's least)
            best = (i << 4) | (u64)(v - 1);
            break;
        }
    }
    best = pred_wave_min(best);
    if (__lane_id() == 0 && best != ~0ull) atomicMin((unsigned long long*)&B.ctr->viol, (unsigned long long)best);
}

}  // namespace rmc
