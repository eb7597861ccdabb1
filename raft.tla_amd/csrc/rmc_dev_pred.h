// rmc_dev_pred.h — model-defined invariants on the packed layout (rmc_pred.h: the
// program format and the interpreter; DESIGN.md "Model-defined invariants").
//  k_pred      : the BFS pass over the states one expansion launch (or the seed) added,
//                [nlo, nhi), as k_violations walks them: every predicate in order on each
//                state, the least (index << 8 | predicate << 1 | error) into one word.
//  k_pred_eval : the same interpreter on staged caller states, every predicate's verdict
//                per state (rmc_eval_predicates).
// Threads diverge — short circuit and data-dependent domains give each its own pc — so
// the program sits in LDS, loaded once per block, and each thread's evaluation stack and
// bound names are a column of an LDS array (row r of thread t at [r * 256 + t]: a wave's
// accesses to one row fall in 64 consecutive words, no bank conflict, and no thread
// reads another's column, so no barrier after the load).  The state is read in place
// through PackedAcc: no dynamically indexed private array, no scratch.
#pragma once
#include "rmc_internal.h"
#include "rmc_pred.h"

namespace rmc {

constexpr int kPredThreads = 256;

struct PredLds {
    u32 code[pred::PRED_CODE];
    int entry[pred::PRED_MAX];
    int mem[pred::PRED_ROWS * kPredThreads];
};

// The block's copy of the program (every thread of the block calls it).
__device__ __forceinline__ void pred_load(PredLds& L, const pred::Program* prog) {
    const int n_code = prog->n_code;
    for (int q = (int)threadIdx.x; q < n_code; q += kPredThreads) L.code[q] = prog->code[q];
    if (threadIdx.x < pred::PRED_MAX) L.entry[threadIdx.x] = prog->entry[threadIdx.x];
    __syncthreads();
}

__device__ __forceinline__ u64 pred_wave_min(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = (u64)(u32)__shfl_xor((int)(u32)v, off) | ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), off) << 32);
        v = o < v ? o : v;
    }
    return v;
}

template <int S, int K>
__global__ __launch_bounds__(kPredThreads) void k_pred(const pred::Program* prog, const DevBufs B, u64 nlo, u64 nhi,
                                                       unsigned long long* word) {
    constexpr int NW = 2 * S + K;
    __shared__ PredLds L;
    pred_load(L, prog);
    const int n_pred = prog->n_pred;
    int* mem = L.mem + threadIdx.x;
    u64 best = ~0ull;
    nhi = nhi < B.cap ? nhi : B.cap;  // (a launch that overflowed the store is an error: the word is not read)
    for (u64 i = nlo + (u64)blockIdx.x * kPredThreads + threadIdx.x; i < nhi; i += (u64)gridDim.x * kPredThreads) {
        const pred::PackedAcc<S, K> a{B.store + wslot(B, i) * (u64)NW};
        const int f = pred::first_failing<kPredThreads>(L.entry, n_pred, L.code, a, mem);
        if (f) {  // (ascending i per thread: the first is this thread's least)
            best = (i << 8) | (u64)(f - 1);
            break;
        }
    }
    best = pred_wave_min(best);
    if (__lane_id() == 0 && best != ~0ull) atomicMin(word, (unsigned long long)best);
}

template <int S, int K>
__global__ __launch_bounds__(kPredThreads) void k_pred_eval(const pred::Program* prog, const u32* in, u64 n,
                                                            uint8_t* out) {
    constexpr int NW = 2 * S + K;
    __shared__ PredLds L;
    pred_load(L, prog);
    const int n_pred = prog->n_pred;
    const u64 t = (u64)blockIdx.x * kPredThreads + threadIdx.x;
    if (t >= n) return;
    const pred::PackedAcc<S, K> a{in + t * (u64)NW};
    for (int p = 0; p < n_pred; ++p)
        out[t * (u64)n_pred + p] = (uint8_t)pred::run<kPredThreads>(L.code, L.entry[p], a, L.mem + threadIdx.x);
}

}  // namespace rmc
