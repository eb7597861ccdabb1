// rmc_dev_act.h — action properties on the packed layout (PROPERTY [][A]_vars; rmc_pred.h: the
// program format and the two-state interpreter; DESIGN.md "Action properties").
//  k_act      : the BFS pass over the parents [lo, hi) of one expansion launch, one thread per
//               parent read through wslot.  It walks every lane (k_graph_count's walk: no diamond
//               skipping, no footprints) and checks a transition exactly when k_graph_count
//               counts it as an edge: the lane is enabled and the successor satisfies the
//               CONSTRAINT's bounds (delta_in_model: delta_fp's verdict without its fingerprint).
//               So a successor outside the CONSTRAINT, which may not fit the packed shape, is
//               never materialised or read.  Every property in order on each such transition,
//               the least (source << 16 | lane << 8 | property << 1 | error) into one word.
//  k_act_eval : the same interpreter on staged caller pairs (current, next), every property's
//               verdict per pair (rmc_eval_actions), the stutter rule applied.
// The successor is materialised in registers (every index a constant) and placed in the thread's
// LDS column — 2 S + K rows beside the interpreter's 32 working rows, the same [row * 256 + t]
// layout: no barrier, no bank conflict — where the next-state accessor reads it; the current
// state is read in place through PackedAcc.  No dynamically indexed private array, no scratch.
// [A]_vars = A \/ UNCHANGED vars: "violated" on a transition whose successor equals the parent word
// for word is "holds"; an evaluation error stays an error.
#pragma once
#include "rmc_dev_pred.h"
#include "rmc_dev_state.h"

namespace rmc {

// par: the block's copy of the model's parameters.  The lane code reads them between two runs of
// the interpreter; as a kernel argument they sit in SGPRs across it (11 lane offsets, the bounds),
// which the interpreter's divergent control flow needs for its masks: 14-22 SGPR spills on every
// shape.  Read from LDS they are short-lived VGPRs and nothing spills.
template <int S, int K>
struct ActLds {
    PredLds p;
    u32 nxt[(2 * S + K) * kPredThreads];
    Params par;
};

// The word of a failing transition; lanes < 128 (rmc_launch_shape.h), properties < 4.
__device__ __forceinline__ u64 act_word(u64 src, int lane, int prop, int verdict) {
    return (src << 16) | ((u64)lane << 8) | ((u64)prop << 1) | (verdict == 2 ? 1ull : 0ull);
}

template <int S, int K>
__global__ __launch_bounds__(kPredThreads) void k_act(const pred::Program* prog, const Params* params,
                                                      const DevBufs B, u64 lo, u64 hi, unsigned long long* word) {
    constexpr int NW = 2 * S + K;
    static_assert(sizeof(Params) % 4 == 0, "Params is copied word by word");
    __shared__ ActLds<S, K> L;
    for (int q = (int)threadIdx.x; q < (int)(sizeof(Params) / 4); q += kPredThreads)
        reinterpret_cast<u32*>(&L.par)[q] = reinterpret_cast<const u32*>(params)[q];
    pred_load(L.p, prog);  // (its barrier covers the copy above)
    const Params& P = L.par;
    const int n_pred = prog->n_pred;
    int* mem = L.p.mem + threadIdx.x;
    u32* col = L.nxt + threadIdx.x;
    const pred::PackedAcc<S, K, kPredThreads> nx{col};
    const int nl = __builtin_amdgcn_readfirstlane(P.off[10]);  // (wave-uniform: the lane loop is scalar)
    u64 best = ~0ull;
    // The walk's loop-long values live in vector registers (an empty asm with a "v" constraint):
    // wave-uniform, they would hold ten SGPRs across the interpreter, whose divergent control flow
    // needs those for its execution masks — the difference between a few SGPR spills and none.
    u64 end = hi, step = (u64)gridDim.x * kPredThreads, wmask = B.wmask;
    const u32* store = B.store;
    asm volatile("" : "+v"(end), "+v"(step), "+v"(wmask), "+v"(store));
    for (u64 i = lo + (u64)blockIdx.x * kPredThreads + threadIdx.x; i < end && best == ~0ull; i += step) {
        const u32* rec = store + (i & wmask) * (u64)NW;  // (wslot)
        const pred::PackedAcc<S, K> cur{rec};
        u64 w[S];
        u32 m[K];
        load_state<S, K>(rec, w, m);
#pragma unroll 1
        for (int lane = 0; lane < nl && best == ~0ull; ++lane) {
            // the lane's descriptor, made wave-uniform again (an LDS read is a vector value): the
            // family dispatch is scalar branches, which save no execution masks
            const u32 desc = (u32)__builtin_amdgcn_readfirstlane((int)P.ldesc[lane]);
            Delta d;
            lane_delta_desc<S, K>(w, m, desc, P, d);
            if (!d.en || !delta_in_model<S, K>(m, d, P)) continue;
            u64 wo[S];
            u32 mo[K];
            materialise<S, K>(w, m, d, wo, mo);
            bool same = true;
#pragma unroll
            for (int q = 0; q < S; ++q) {
                col[(2 * q) * kPredThreads] = (u32)wo[q];
                col[(2 * q + 1) * kPredThreads] = (u32)(wo[q] >> 32);
                same = same && wo[q] == w[q];
            }
#pragma unroll
            for (int q = 0; q < K; ++q) {
                col[(2 * S + q) * kPredThreads] = mo[q];
                same = same && mo[q] == m[q];
            }
            for (int p = 0; p < n_pred; ++p) {
                int v = pred::run2<kPredThreads, true>(L.p.code, L.p.entry[p], cur, nx, mem);
                if (v == 1 && same) v = 0;
                if (v) {  // (ascending i, lane, p per thread: the first is this thread's least)
                    best = act_word(i, lane, p, v);
                    break;
                }
            }
        }
    }
    best = pred_wave_min(best);
    if (__lane_id() == 0 && best != ~0ull) atomicMin(word, (unsigned long long)best);
}

// in: n pairs, the current state's NW words, then the next state's.
template <int S, int K>
__global__ __launch_bounds__(kPredThreads) void k_act_eval(const pred::Program* prog, const u32* in, u64 n,
                                                           uint8_t* out) {
    constexpr int NW = 2 * S + K;
    __shared__ PredLds L;
    pred_load(L, prog);
    const int n_pred = prog->n_pred;
    const u64 t = (u64)blockIdx.x * kPredThreads + threadIdx.x;
    if (t >= n) return;
    const u32* rec = in + t * (u64)(2 * NW);
    const pred::PackedAcc<S, K> cur{rec}, nx{rec + NW};
    bool same = true;
#pragma unroll
    for (int q = 0; q < NW; ++q) same = same && rec[q] == rec[NW + q];
    for (int p = 0; p < n_pred; ++p) {
        int v = pred::run2<kPredThreads, true>(L.code, L.entry[p], cur, nx, L.mem + threadIdx.x);
        if (v == 1 && same) v = 0;
        out[t * (u64)n_pred + p] = (uint8_t)v;
    }
}

}  // namespace rmc
