// rmc_dev_graph.h — the state graph of a finished search (rmc_graph.cpp; DESIGN.md "State graph"):
//
//  k_graph_count : the edges out of each stored state of [lo, hi): its enabled lanes whose
//                  successor satisfies the CONSTRAINT (stuttering lanes included).
//  k_graph_edges : the same every-lane walk (k_list's, k_cover's: no diamond skipping, no
//                  footprints, which omit lanes), each such lane's key looked up in the set and
//                  written as (src, dst, family, lane) at the place the scan of the counts gives
//                  it: ascending src, then ascending lane, whatever the launch's schedule.
//  k_graph_find  : the lookup alone on staged states (rmc_find_states): the key as k_keys
//                  computes it, then the probe.
//
// The lookup goes key -> set slot -> store index through verification's slot -> index array
// (DevBufs.sidx, filled by k_publish).  It reads the set only: a slot that is empty — or, in a
// tagged set, of another run's epoch (fp_empty) — ends the probe sequence as it does for the
// inserts, so the entries of earlier runs on the ctx are never found.
#pragma once
#include <hip/hip_runtime.h>

#include "raft_packed.h"
#include "rmc_dev_set.h"
#include "rmc_dev_state.h"
#include "rmc_internal.h"

namespace rmc {

// The slot that holds table value `key`, whose probe sequence starts at s0 (content `cur`,
// already loaded), or ~0: not in the set.
__device__ __forceinline__ u64 fp_find(const u64* __restrict__ table, u64 mask, u64 s0, u64 key, u64 cur) {
    u64 s = s0;
    for (u64 n = 0; n <= mask; ++n) {
        if (cur == key) return s;
        if (fp_empty(cur)) return ~0ull;
        s = (s + 1) & mask;
        cur = table[s];
    }
    return ~0ull;
}

template <int S, int K>
__global__ __launch_bounds__(256) void k_graph_count(const Params P, const DevBufs B, u64 lo, u64 hi, u32* cnt) {
    constexpr int NW = 2 * S + K;
    const int nl = P.off[10];  // runtime on purpose (see lane_delta)
    for (u64 i = lo + (u64)blockIdx.x * 256ull + threadIdx.x; i < hi; i += (u64)gridDim.x * 256ull) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, i) * (u64)NW, w, m);
        u32 n = 0;
#pragma unroll 1
        for (int lane = 0; lane < nl; ++lane) {
            Delta d;
            lane_delta<S, K>(w, m, lane, P, d);
            if (!d.en) continue;
            Fp h;
            n += delta_fp<S, K>(w, m, Fp{0, 0}, d, P, &h) ? 1u : 0u;
        }
        cnt[i - lo] = n;
    }
}

// off[i - lo]: the first record of state i in out (the exclusive scan of k_graph_count's counts).
// err: min over the edges whose key the set does not hold of (src << 8 | lane); ~0 = none.
template <int S, int K, bool SYM, int BATCH>
__global__ __launch_bounds__(256) void k_graph_edges(const Params P, const PermTable PT, const DevBufs B, u64 lo,
                                                     u64 hi, const u64* __restrict__ off, GraphEdge* out, u64 cap,
                                                     unsigned long long* err) {
    constexpr int NW = 2 * S + K;
    // a batch's table values and first slots, parked per thread (a column each: no barrier)
    __shared__ u64 s_key[BATCH][256];
    __shared__ u64 s_slot[BATCH][256];
    const int nl = P.off[10];
    for (u64 i = lo + (u64)blockIdx.x * 256ull + threadIdx.x; i < hi; i += (u64)gridDim.x * 256ull) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, i) * (u64)NW, w, m);
        const Fp h0 = state_fp<S, K>(w, m);
        u64 sbase[SYM ? S : 1];
        if constexpr (SYM) {
#pragma unroll
            for (int q = 0; q < S; ++q) sbase[q] = sig_base<S>(w[q], (u32)q);
        }
        u64 o = off[i - lo];
        for (int lane0 = 0; lane0 < nl; lane0 += BATCH) {
            // (a) the keys of BATCH lanes (0: no edge); one copy of the lane code
#pragma unroll 1
            for (int b = 0; b < BATCH; ++b) {
                const int lane = lane0 + b;
                u64 key = 0, slot0 = 0;
                if (lane < nl) {
                    Delta d;
                    lane_delta<S, K>(w, m, lane, P, d);
                    Fp h{0, 0};
                    if (d.en && delta_fp<S, K>(w, m, h0, d, P, &h)) {
                        // SYMMETRY: the canonical key, ties resolved here (as k_list does)
                        if constexpr (SYM) h = canon_delta<S, K>(w, m, sbase, d, PT.code, PT.np);
                        const TKey t = tkey(fp_weaken(h, P.fp_mask), B.tmask);
                        key = t.v;  // never 0 (fp_norm)
                        slot0 = t.s0;
                    }
                }
                s_key[b][threadIdx.x] = key;
                s_slot[b][threadIdx.x] = slot0;
            }
            // (b) BATCH independent first-slot probes in flight at once
            u64 key[BATCH], cur[BATCH];
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                key[b] = s_key[b][threadIdx.x];
                cur[b] = key[b] ? B.table[s_slot[b][threadIdx.x]] : 0ull;
            }
            // (c) resolve and write, in lane order
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                if (!key[b]) continue;
                const int lane = lane0 + b;
                const u64 s = fp_find(B.table, B.tmask, s_slot[b][threadIdx.x], key[b], cur[b]);
                const u64 dst = s == ~0ull ? ~0ull : B.sidx[s];
                if (dst == ~0ull) atomicMin(err, (unsigned long long)((i << 8) | (u64)lane));
                if (o < cap) {
                    GraphEdge e;
                    e.src = i;
                    e.dst = dst;
                    e.family = lane_family(P, lane);
                    e.instance = lane;
                    out[o] = e;
                }
                ++o;
            }
        }
    }
}

template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_graph_find(const Params P, const PermTable PT, const DevBufs B, const u32* in,
                                                    u64 n, u64* index) {
    constexpr int NW = 2 * S + K;
    const u64 t = (u64)blockIdx.x * 256ull + threadIdx.x;
    if (t >= n) return;
    u64 w[S];
    u32 m[K];
    load_state<S, K>(in + t * (u64)NW, w, m);
    const TKey key =
        tkey(fp_weaken(SYM ? canon_state<S, K>(w, m, PT.code, PT.np) : state_fp<S, K>(w, m), P.fp_mask), B.tmask);
    const u64 s = fp_find(B.table, B.tmask, key.s0, key.v, B.table[key.s0]);
    index[t] = s == ~0ull ? ~0ull : B.sidx[s];
}

}  // namespace rmc
