// rmc_dev_tools.h — the kernels beside the expansion (DESIGN.md "Kernels").
//
//  k_seed   : inserts initial states (Init raft.tla:125-129) the way k_expand
//             inserts successors.
//  k_list   : the same lane code with every enabled successor written out
//             (no dedup) — the differential-test entry point (rmc_expand).
//  k_cover  : action coverage (RMC_FLAG_COVERAGE, TLC -coverage): a pass beside
//             each expansion launch that tallies the enabled lanes of its
//             parents and the producing lanes of its new states per action.
//  k_violations : continue past violations (RMC_FLAG_CONTINUE, TLC -continue): a
//             pass over the states each launch added that tallies, per
//             invariant, the stored states violating it.
//
// and k_rehash (recovery), k_pack_rep (replicated levels), k_check (rmc_check_states),
// k_keys (rmc_state_keys), k_simulate (TLC -simulate).
#pragma once
#include <hip/hip_runtime.h>

#include "raft_packed.h"
#include "rmc_cover.h"
#include "rmc_dev_set.h"
#include "rmc_dev_sharded.h"
#include "rmc_dev_state.h"
#include "rmc_dev_verify.h"
#include "rmc_internal.h"
#include "rmc_viol.h"

namespace rmc {

// Insert n staged initial states (packed) into the set and the store.
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_seed(const Params P, const PermTable PT, const DevBufs B, const u32* staged,
                                              u64 n) {
    constexpr int NW = 2 * S + K;
    const u64 t = (u64)blockIdx.x * 256ull + threadIdx.x;
    const bool live = t < n;
    u64 w[S];
    u32 m[K];
    if (live) {
        load_state<S, K>(staged + t * (u64)NW, w, m);
    } else {
#pragma unroll
        for (int i = 0; i < S; ++i) w[i] = 0;
#pragma unroll
        for (int q = 0; q < K; ++q) m[q] = 0;
    }
    int is_new = 0;
    if (live) {
        // fp_weaken: a no-op unless a verification test weakens the fingerprint
        const Fp key = fp_weaken(SYM ? canon_state<S, K>(w, m, PT.code, PT.np) : state_fp<S, K>(w, m), P.fp_mask);
        // sharded mode: only the owner of an initial state stores it
        if (owner_state<S>(key.k, w, B) == B.rank) is_new = fp_insert_fp(B.table, B.tmask, key, &B.ctr->table_full);
    }
    Delta d;  // identity delta: the state itself
    d.srv = -1; d.rm = -1; d.has_add = 0; d.add = 0; d.en = 1; d.w_new = 0;
    commit_new<S, K>(is_new, w, m, d, P, B, ~0ull, 255);
}

// Recovery (rmc_recover): re-insert the keys of the stored states [lo, hi)
// into an empty fingerprint set — the set is rebuilt, not checkpointed.
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_rehash(const Params P, const PermTable PT, const DevBufs B, u64 lo, u64 hi) {
    constexpr int NW = 2 * S + K;
    for (u64 i = lo + (u64)blockIdx.x * 256ull + threadIdx.x; i < hi; i += (u64)gridDim.x * 256ull) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, i) * (u64)NW, w, m);
        const Fp key = fp_weaken(SYM ? canon_state<S, K>(w, m, PT.code, PT.np) : state_fp<S, K>(w, m), P.fp_mask);
        if (!fp_insert_fp(B.table, B.tmask, key, &B.ctr->table_full)) atomicOr(&B.ctr->overflow, 8u);  // duplicate
    }
}

// Replicated level (sharded mode): this rank's frontier states [lo, hi) as
// records for the level's all-gather (RepRec: state, global ref, footprint,
// lane | class << 8).
template <int S, int K>
__global__ __launch_bounds__(256) void k_pack_rep(const DevBufs B, u64 lo, u64 hi, u32* out) {
    constexpr int NW = 2 * S + K;
    typedef RepRec<S, K> RR;
    for (u64 i = lo + (u64)blockIdx.x * 256ull + threadIdx.x; i < hi; i += (u64)gridDim.x * 256ull) {
        u32* r = out + (i - lo) * (u64)RR::RR;
        const uint2* src = reinterpret_cast<const uint2*>(B.store + i * (u64)NW);
        uint2* dst = reinterpret_cast<uint2*>(r);
#pragma unroll
        for (int q = 0; q < NW / 2; ++q) dst[q] = src[q];
        const u64 ref = B.ref_tag | i;
        const u64 f = B.foot[i];
        r[RR::REF] = (u32)ref;
        r[RR::REF + 1] = (u32)(ref >> 32);
        r[RR::FOOT] = (u32)f;
        r[RR::FOOT + 1] = (u32)(f >> 32);
        r[RR::ACT] = (u32)B.act[i] | ((u32)B.cls[i] << 8);
        r[RR::ACT + 1] = 0;
    }
}

// Every enabled lane of n given states, written out without dedup.
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_list(const Params P, const PermTable PT, const u32* in, u64 n, u32* out,
                                              u64 cap, unsigned long long* count) {
    constexpr int NW = 2 * S + K;
    constexpr int RW = 6 + NW;  // record: parent(2) lane(1) flags(1) fp(2) + state
    const u64 t = (u64)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n) return;
    u64 w[S];
    u32 m[K];
    load_state<S, K>(in + t * (u64)NW, w, m);
    const Fp h0 = state_fp<S, K>(w, m);
    u64 sbase[S];
#pragma unroll
    for (int i = 0; i < S; ++i) sbase[i] = sig_base<S>(w[i], (u32)i);
    const int nl = P.off[10];  // == Lanes<S,K>::N; runtime on purpose (see lane_delta)
#pragma unroll 1
    for (int lane = 0; lane < nl; ++lane) {
        Delta d;
        lane_delta<S, K>(w, m, lane, P, d);
        if (!d.en) continue;
        Fp h{0, 0};
        const int in_model = delta_fp<S, K>(w, m, h0, d, P, &h);
        if (in_model) {
            if constexpr (SYM) h = canon_delta<S, K>(w, m, sbase, d, PT.code, PT.np);
        }
        const u64 o = atomicAdd(count, 1ull);
        if (o >= cap) continue;
        u32* r = out + o * (u64)RW;
        r[0] = (u32)t; r[1] = (u32)(t >> 32); r[2] = (u32)lane; r[3] = (u32)in_model;
        r[4] = (u32)h.k; r[5] = (u32)(h.k >> 32);
        u64 wo[S];
        u32 mo[K];
        if (in_model) {
            materialise<S, K>(w, m, d, wo, mo);
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i) wo[i] = 0;
#pragma unroll
            for (int q = 0; q < K; ++q) mo[q] = 0;
        }
#pragma unroll
        for (int i = 0; i < S; ++i) { r[6 + 2 * i] = (u32)wo[i]; r[7 + 2 * i] = (u32)(wo[i] >> 32); }
#pragma unroll
        for (int q = 0; q < K; ++q) r[6 + 2 * S + q] = mo[q];
    }
}

// The invariants of n given states, one thread per state (rmc_check_states): the
// expansion kernels' and k_simulate's check_invariants and nothing else, with the
// complete TypeOK (raft_packed.h msg_entries_ok: the states are the caller's).
template <int S, int K>
__global__ __launch_bounds__(256) void k_check(const Params P, const u32* in, u64 n, int* out) {
    constexpr int NW = 2 * S + K;
    const u64 t = (u64)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n) return;
    u64 w[S];
    u32 m[K];
    load_state<S, K>(in + t * (u64)NW, w, m);
    out[t] = check_invariants<S, K, true>(w, m, P);
}

// The keys of n given states, one thread per state (rmc_state_keys): the key k_seed,
// k_rehash and k_publish compute for a stored state (state_fp, under SYMMETRY
// canon_state; fp_weaken as there), and with ref the comparison of verification
// (same_state, under SYMMETRY same_orbit) of state t against the record of state
// ref[t] of the same array.  No set and no store is touched.
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_keys(const PermTable PT, u64 fp_mask, const u32* in, u64 n, u64* keys,
                                              const u32* ref, unsigned char* same) {
    constexpr int NW = 2 * S + K;
    const u64 t = (u64)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n) return;
    PackedState<S, K> s;
    load_state<S, K>(in + t * (u64)NW, s.w, s.m);
    keys[t] = fp_weaken(SYM ? canon_state<S, K>(s.w, s.m, PT.code, PT.np) : state_fp<S, K>(s.w, s.m), fp_mask).k;
    if (ref) {
        const u32* st = in + (u64)ref[t] * (u64)NW;  // ref[t] < n: checked by the caller
        bool eq;
        if constexpr (SYM) eq = same_orbit<S, K>(s, st, PT);
        else eq = same_state<S, K>(s.w, s.m, st);
        same[t] = eq ? 1 : 0;
    }
}

// ---- action coverage (RMC_FLAG_COVERAGE, TLC -coverage; rmc_cover.h) ------------------
// A pass of its own beside one expansion launch (the expansion kernels do not
// change): `generated` over the launch's parents [lo, hi) — the lane walk of
// k_list, every enabled lane tallied in its action's row — and `distinct` over
// the states the launch added, [nlo, nhi): the row of each one's producing
// lane (B.act), classified for a Receive lane from its parent's record, which
// is still resident (the parent is of [lo, hi)).  n_init: initial states to
// add to row Init's generated (the seed step).  Per-thread counts in registers
// (every index a compile-time constant), a wave sum, one LDS add per wave and
// row, one global atomic per block and non-zero row.
__device__ __forceinline__ u32 wave_sum32(u32 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (u32)__shfl_xor((int)v, off);
    return v;
}

template <int S, int K>
__global__ __launch_bounds__(256) void k_cover(const Params P, const DevBufs B, u64 lo, u64 hi, u64 nlo, u64 nhi,
                                               u64 n_init, unsigned long long* cov) {
    constexpr int NW = 2 * S + K;
    __shared__ u32 s_row[2 * COV_ROWS];
    if (threadIdx.x < 2 * COV_ROWS) s_row[threadIdx.x] = 0;
    __syncthreads();
    u32 g[COV_ROWS], n[COV_ROWS];
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) g[r] = n[r] = 0;
    const u64 t0 = (u64)blockIdx.x * 256ull + threadIdx.x, step = (u64)gridDim.x * 256ull;
    for (u64 i = lo + t0; i < hi; i += step) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, i) * (u64)NW, w, m);
        // one family at a time: its row is one value (Receive: per message), and
        // the lane code is inlined once (lane_delta: a runtime lane, wave-uniform here)
#pragma unroll 1
        for (int f = 0; f < 10; ++f) {
            u32 on = 0;
#pragma unroll 1
            for (int lane = P.off[f]; lane < P.off[f + 1]; ++lane) {
                Delta d;
                lane_delta<S, K>(w, m, lane, P, d);
                if (!d.en) continue;
                if (f == 7) {
                    const int row = cover_row<S, K>(P, w, m, lane);
#pragma unroll
                    for (int r = COV_UPDATE_TERM; r < COV_DUPLICATE; ++r) g[r] += row == r ? 1u : 0u;
                } else {
                    ++on;
                }
            }
            const int frow = f == 7 ? -1 : cover_family_row(f);
#pragma unroll
            for (int r = 0; r < COV_ROWS; ++r) g[r] += frow == r ? on : 0u;  // (g's indices stay constants)
        }
    }
    nhi = nhi < B.cap ? nhi : B.cap;  // (a launch that overflowed the store is an error: its tallies are not read)
    for (u64 i = nlo + t0; i < nhi; i += step) {
        const int lane = (int)B.act[i];
        int row = COV_INIT;  // 255: an initial state
        if (lane != 255) {
            if (lane >= P.off[10]) continue;
            const int f = lane_family(P, lane);
            row = f == 7 ? -1 : cover_family_row(f);
            if (f == 7) {
                const u64 p = B.parent[i];
                if (p < lo || p >= hi) continue;  // not of this launch: left out, and the sums show it
                u64 w[S];
                u32 m[K];
                load_state<S, K>(B.store + wslot(B, p) * (u64)NW, w, m);
                row = cover_row<S, K>(P, w, m, lane);
            }
        }
#pragma unroll
        for (int r = 0; r < COV_ROWS; ++r) n[r] += row == r ? 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) {
        const u32 gs = wave_sum32(g[r]), ns = wave_sum32(n[r]);
        if (__lane_id() == 0 && gs) atomicAdd(&s_row[r], gs);
        if (__lane_id() == 0 && ns) atomicAdd(&s_row[COV_ROWS + r], ns);
    }
    __syncthreads();
    if (threadIdx.x < 2 * COV_ROWS) {
        u64 v = s_row[threadIdx.x];
        if (threadIdx.x == COV_INIT && blockIdx.x == 0) v += n_init;
        if (v) atomicAdd(&cov[threadIdx.x], (unsigned long long)v);
    }
}

// ---- continue past violations (RMC_FLAG_CONTINUE, TLC -continue; rmc_viol.h) ---------
// A pass of its own over the states one launch (or the seed) added, [nlo, nhi),
// which every allowed path still holds (the store; the linear window, which moves
// only expanded states and before a launch; the ring, whose room keeps a launch's
// new states inside it): each state is loaded through wslot and classified by
// classify_violations — the BFS's own check for `first`, each remaining bit of
// the mask alone for `each`.  Reduced like k_cover: per-thread counts in registers
// (every index a compile-time constant), a wave sum, one LDS add per wave and
// row, one global atomic per block and non-zero row; the least index per
// invariant through a wave min and one atomicMin per wave that has one.
__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = (u64)(u32)__shfl_xor((int)(u32)v, off) | ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), off) << 32);
        v = o < v ? o : v;
    }
    return v;
}

template <int S, int K>
__global__ __launch_bounds__(256) void k_violations(const Params P, const DevBufs B, u64 nlo, u64 nhi,
                                                    unsigned long long* viol) {
    constexpr int NW = 2 * S + K;
    __shared__ u32 s_row[2 * VIOL_INVS];
    if (threadIdx.x < 2 * VIOL_INVS) s_row[threadIdx.x] = 0;
    __syncthreads();
    u32 nf[VIOL_INVS], ne[VIOL_INVS];
    u64 least[VIOL_INVS];
#pragma unroll
    for (int r = 0; r < VIOL_INVS; ++r) {
        nf[r] = ne[r] = 0;
        least[r] = ~0ull;
    }
    nhi = nhi < B.cap ? nhi : B.cap;  // (a launch that overflowed the store is an error: its tallies are not read)
    for (u64 i = nlo + (u64)blockIdx.x * 256ull + threadIdx.x; i < nhi; i += (u64)gridDim.x * 256ull) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, i) * (u64)NW, w, m);
        const ViolClass c = classify_violations<S, K>(w, m, P);
        if (!c.first) continue;
#pragma unroll
        for (int r = 0; r < VIOL_INVS; ++r) {
            const bool alone = ((c.each >> r) & 1u) != 0;
            nf[r] += c.first == r + 1 ? 1u : 0u;
            ne[r] += alone ? 1u : 0u;
            least[r] = alone && i < least[r] ? i : least[r];
        }
    }
#pragma unroll
    for (int r = 0; r < VIOL_INVS; ++r) {
        const u32 fs = wave_sum32(nf[r]), es = wave_sum32(ne[r]);
        if (!es) continue;  // (wave-uniform; first[r] <= each[r])
        const u64 lm = wave_min64(least[r]);
        if (__lane_id() == 0) {
            if (fs) atomicAdd(&s_row[VIOL_FIRST + r], fs);
            atomicAdd(&s_row[VIOL_EACH + r], es);
            atomicMin(&viol[VIOL_LEAST + r], (unsigned long long)lm);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * VIOL_INVS) {
        const u32 v = s_row[threadIdx.x];
        if (v) atomicAdd(&viol[threadIdx.x], (unsigned long long)v);
    }
}

// ---- simulation (TLC -simulate; Smokeraft.cfg) -------------
// One thread per behaviour: a random initial state from `inits`, then up to
// depth-1 steps, each choosing uniformly (one reservoir pass over the lanes)
// among the enabled successors — mode 0: those within the packed capacity
// (term <= 15, Len(log) <= 3, <= K messages, count <= 3; P carries these
// bounds), mode 1: all of them, a chosen successor beyond the capacity ending
// the behaviour as "truncated".  No candidate ends it as "deadlocked"
// (Smokeraft.cfg:48 turns deadlock checking off).  Invariants are checked on
// every state.
// rec_beh >= 0: that behaviour also writes its states to rec (replay).
__device__ __forceinline__ u64 sim_rand(u64& x) {  // splitmix64 stream
    x += 0x9E3779B97F4A7C15ull;
    return mix64(x);
}

template <int S, int K>
__global__ __launch_bounds__(256) void k_simulate(const Params P, const u32* inits, u64 n_init, u64 n_beh, int depth,
                                                  u64 seed, int mode, SimCounters* out, i64 rec_beh, u32* rec) {
    constexpr int NW = 2 * S + K;
    u64 steps = 0, trunc = 0, dead = 0;
    for (u64 t = (u64)blockIdx.x * 256ull + threadIdx.x; t < n_beh; t += (u64)gridDim.x * 256ull) {
        if (rec_beh >= 0 && (i64)t != rec_beh) continue;  // replay of one behaviour
        u64 rs = mix64(seed ^ (t * 0xD1B54A32D192ED03ull));
        u64 w[S];
        u32 m[K];
        load_state<S, K>(inits + (sim_rand(rs) % n_init) * (u64)NW, w, m);
        const bool record = (i64)t == rec_beh;
        if (record) store_state<S, K>(rec, w, m);
        int v = check_invariants<S, K>(w, m, P);
        if (v) atomicMin((unsigned long long*)&out->viol, (unsigned long long)((1ull << 44) | ((u64)(v - 1) << 40) | t));
        for (int dd = 2; dd <= depth && !v; ++dd) {
            u32 cnt = 0;
            int pick = -1;
            for (int lane = 0; lane < P.off[10]; ++lane) {
                Delta d;
                lane_delta<S, K>(w, m, lane, P, d);
                if (!d.en) continue;
                Fp hh;
                if (mode == 0 && !delta_fp<S, K>(w, m, Fp{0, 0}, d, P, &hh)) continue;  // beyond the capacity
                ++cnt;
                if (sim_rand(rs) % cnt == 0) pick = lane;  // reservoir: uniform over enabled lanes
            }
            if (cnt == 0) {
                ++dead;
                break;
            }
            Delta d;
            lane_delta<S, K>(w, m, pick, P, d);
            Fp hh;
            if (!delta_fp<S, K>(w, m, Fp{0, 0}, d, P, &hh)) {
                ++trunc;
                break;
            }
            u64 wo[S];
            u32 mo[K];
            materialise<S, K>(w, m, d, wo, mo);
#pragma unroll
            for (int i = 0; i < S; ++i) w[i] = wo[i];
#pragma unroll
            for (int q = 0; q < K; ++q) m[q] = mo[q];
            ++steps;
            if (record) store_state<S, K>(rec + (u64)(dd - 1) * NW, w, m);
            v = check_invariants<S, K>(w, m, P);
            if (v)
                atomicMin((unsigned long long*)&out->viol,
                          (unsigned long long)(((u64)dd << 44) | ((u64)(v - 1) << 40) | t));
        }
    }
    atomicAdd((unsigned long long*)&out->steps, (unsigned long long)steps);
    if (trunc) atomicAdd((unsigned long long*)&out->truncated, (unsigned long long)trunc);
    if (dead) atomicAdd((unsigned long long*)&out->deadlocked, (unsigned long long)dead);
}

}  // namespace rmc
