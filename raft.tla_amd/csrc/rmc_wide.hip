// rmc_wide.hip — gfx950 kernels of the wide layout (raft_wide.h): the BFS,
// the successor listing and the random walks of models whose fields outgrow
// the packed layout (MCraft.cfg as shipped under a depth bound, Smokeraft's
// unbounded depth-100 walks).  One thread per state or behaviour; each lane
// materialises its successor (5,080 bytes, private memory), the fingerprint
// hashes the whole canonical record, and new states are inserted into the
// same kind of open-addressing HBM set as the packed kernels use.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "raft_wide.h"
#include "rmc_cover.h"
#include "rmc_dev_pred.h"
#include "rmc_internal.h"
#include "rmc_viol.h"

namespace rmc {
namespace wide {

// 1: h was inserted, 0: it was there (or the table is full).  *at = the slot that
// holds it (~0: table full) — full-state verification finds the owner by it.
__device__ __forceinline__ int w_insert(u64* __restrict__ table, u64 mask, const Fp& h, u32* full, u64* at) {
    const TKey t = tkey(h, mask);
    const u64 key = t.v;
    u64 s = t.s0;
    for (u64 n = 0; n <= mask; ++n) {
        const u64 cur = table[s];
        *at = s;
        if (cur == key) return 0;
        if (cur == 0) {
            const u64 prev = atomicCAS((unsigned long long*)&table[s], 0ull, (unsigned long long)key);
            if (prev == 0) return 1;
            if (prev == key) return 0;
        }
        s = (s + 1) & mask;
    }
    *at = ~0ull;
    atomicOr(full, 1u);
    return 0;
}

__device__ __forceinline__ u64 w_wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v += (u64)(u32)__shfl_xor((int)(u32)v, off) | ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), off) << 32);
    return v;
}
__device__ __forceinline__ u64 w_bcast(u64 v, int src) {
    return (u64)(u32)__shfl((int)(u32)v, src) | ((u64)(u32)__shfl((int)(u32)(v >> 32), src) << 32);
}

// The slot of state i's record: its index, or in the ring window i % window
// (any size; one 64-bit remainder per 336-B to 5-KB record copy).
template <bool Ring>
__device__ __forceinline__ u64 w_slot(const WideBufs& B, u64 i) {
    return Ring ? i % B.window : i;
}

// Store a new state (index allocated by the caller) with its trace link and the
// fused invariant check on the caller's private copy.  Ring: t is narrowed into
// the store's record — one it does not fit is never cut short: the fields come
// back as Counters.overflow field bits and nothing is written — and a state of
// a level that is never expanded (B.unstored) gets no record at all.
template <class Store, bool Ring, class Work>
__device__ __forceinline__ u32 w_store(const WModel& M, const WideBufs& B, u64 ni, const Work& t, u64 parent,
                                       int lane) {
    u32 bad = 0;
    if (!Ring) {
        wcopy_state(static_cast<Work*>(B.store)[ni], t);
    } else if (!B.unstored) {
        bad = (u32)wnarrow_bits<Store>(t);
        if (!bad) wconvert(static_cast<Store*>(B.store)[w_slot<Ring>(B, ni)], t);
    }
    B.parent[ni] = parent;
    B.act[ni] = (uint8_t)lane;
    const int v = wcheck_invariants(M, t);
    if (v) atomicMin((unsigned long long*)&B.ctr->viol, (unsigned long long)((ni << 4) | (u64)(v - 1)));
    return bad;
}

// Init (raft.tla:125-129) or SmokeInit's states: n staged records (of the work type).
// Verify (RMC_FLAG_VERIFY_STATES): the key is weakened as the expansion's and
// the new state becomes its slot's owner.  Sym (RMC_FLAG_SYMMETRY): the key is the
// canonical key of the state's orbit (wcanon); the record stored is the state given.
template <class Store, class Work, bool Ring, bool Verify, bool Sym>
__global__ __launch_bounds__(256) void k_wseed(const WModel M, const WideBufs B, const Work* staged, u64 n) {
    static_assert(Ring || sizeof(Store) == sizeof(Work), "without the ring the store holds the work record");
    static_assert(!(Ring && Verify), "verification compares with resident records");
    for (u64 t = (u64)blockIdx.x * 256ull + threadIdx.x; t < n; t += (u64)gridDim.x * 256ull) {
        Fp h;
        if constexpr (Sym) h = wcanon(staged[t], B.salt, M.S);
        else h = wfp(staged[t], B.salt, M.S);
        if constexpr (Verify) h = fp_weaken(h, B.fp_mask);
        u64 slot;
        if (!w_insert(B.table, B.tmask, h, &B.ctr->table_full, &slot)) continue;
        const u64 ni = atomicAdd((unsigned long long*)&B.ctr->count, 1ull);
        if (ni >= B.cap) {
            atomicOr(&B.ctr->overflow, 1u);
            continue;
        }
        const u32 bad = w_store<Store, Ring>(M, B, ni, staged[t], ~0ull, 255);
        if constexpr (Verify) B.sidx[slot] = ni;
        if (bad) atomicOr(&B.ctr->overflow, bad << 8);
    }
}

// One BFS level: every lane of every frontier state [lo, hi).  Successors
// outside the CONSTRAINT count as generated and are dropped; a successor the
// layout cannot hold in a field no CONSTRAINT bounds stops the search
// (Counters.overflow bits 8-11, the field).  Round 6: the parent's fingerprint
// once per state and each successor's from it (wfp_delta: the components the
// lane changed), the bag families walked only over the state's messages, and
// stuttering successors (the parent's fingerprint) not probed.
// Ring (RMC_FLAG_SPILL): the frontier state is read from its ring slot and
// widened into a Work record; lanes, CONSTRAINT and fingerprints run on Work
// (wfp does not depend on the record's capacity), and a stored successor is
// narrowed into a Store record (w_store).
// Verify (RMC_FLAG_VERIFY_STATES, resident store): the inserting lane records
// itself as its slot's owner (B.sidx: it knows the slot and the index, and the
// end of the launch publishes the write), and a lane whose key is already in
// the set compares its private successor with the owner's record — at once
// when the owner was stored by an earlier launch (index below B.vbase: the
// record is complete), else through B.vbuf and k_wverify after this launch (the
// owner's record may be half written: it is never read here).  A successor
// that differs from its key's owner is a collision: counted and dropped, as
// TLC would drop it.  The key that reaches the set is weakened by B.fp_mask
// (rmc_set_fp_bits), and the stutter shortcut — taken on the full fingerprint —
// is confirmed on the states, so every probe is either a new state or a
// compared hit: verified = probes - (distinct - 1).
// Sym (RMC_FLAG_SYMMETRY): the key of a successor is its orbit's canonical key,
// computed on the materialised successor t from the parent's signature bases
// (wcanon_succ: the one server the lane wrote gets a new base) — no permuted
// record, no third Work.  The record stored is the successor found.  The
// stutter shortcut compares canonical keys: a successor in its parent's orbit
// is already stored; with Verify that is confirmed by wsame_orbit, and both
// compare sites decide "some permutation of the successor is the owner".  The
// non-symmetric instantiations are what they were.
template <class Store, class Work, bool Ring, bool Verify, bool Sym>
__global__ __launch_bounds__(256) void k_wexpand(const WModel M, const WideBufs B, u64 lo, u64 hi) {
    static_assert(Ring || sizeof(Store) == sizeof(Work), "without the ring the store holds the work record");
    static_assert(Store::kLW <= Work::kLW && Store::kKW <= Work::kKW, "the work record holds every stored state");
    static_assert(!(Ring && Verify), "verification compares with resident records");
    u64 gen = 0, probes = 0, vchk = 0, vcol = 0;
    u32 bad = 0;
    const int o7 = M.L.off[7];
    for (u64 i = lo + (u64)blockIdx.x * 256ull + threadIdx.x; i < hi; i += (u64)gridDim.x * 256ull) {
        Work s, t;
        wconvert(s, static_cast<const Store*>(B.store)[w_slot<Ring>(B, i)]);
        Fp h0;
        u64 base0[Sym ? WS : 1];
        if constexpr (Sym) {
            wsig_bases(s, M.S, base0);
            h0 = wcanon_based(s, base0, M.S, B.salt);
        } else {
            h0 = wfp(s, B.salt, M.S);
        }
        u32 g = 0;
        // lanes of families 0-6, then the three bag families over slots [0, nmsg)
        const int nb = s.nmsg, nl = o7 + 3 * nb;
        for (int q = 0; q < nl; ++q) {
            const int lane = q < o7 ? q : M.L.off[7 + (q - o7) / nb] + (q - o7) % nb;
            WDelta dl;
            const int r = wlane(M, s, lane, &t, false, &dl);
            if (r == W_OFF) continue;
            ++g;
            if (r != W_ON) {  // beyond the layout: an error for a field no CONSTRAINT bounds,
                bad |= (u32)(woverflow_bits(r) & M.unbounded);  // else beyond its bound (filtered)
                continue;
            }
            if (!win_model(M, t)) continue;
            Fp h;
            if constexpr (Sym) h = wcanon_succ(t, base0, dl.srv, B.salt, M.S);
            else h = wfp_delta(s, t, h0, dl, B.salt);
            // a stutter (without Verify: or a full-fingerprint twin of the parent); Sym: in the parent's orbit
            if constexpr (Sym) {
                if (h.k == h0.k && h.s == h0.s && (!Verify || wsame_orbit(s, t, M.S))) continue;
            } else {
                if (h.k == h0.k && h.s == h0.s && (!Verify || wsame(s, t, M.S))) continue;
            }
            ++probes;
            u64 slot;
            if (!w_insert(B.table, B.tmask, Verify ? fp_weaken(h, B.fp_mask) : h, &B.ctr->table_full, &slot)) {
                if constexpr (Verify) {
                    if (slot == ~0ull) continue;  // table full (flagged by the insert)
                    const u64 ix = B.sidx[slot];
                    if (ix != ~0ull && ix < B.vbase) {
                        ++vchk;
                        if constexpr (Sym) vcol += wsame_orbit(static_cast<const Store*>(B.store)[ix], t, M.S) ? 0u : 1u;
                        else vcol += wsame(static_cast<const Store*>(B.store)[ix], t, M.S) ? 0u : 1u;
                        continue;
                    }
                    // the owner is of this launch: deferred, one vcount bump for the lanes here together
                    const u64 bal = __ballot(1);
                    const int leader = __ffsll((long long)bal) - 1, me = (int)__lane_id();
                    u64 q0 = 0;
                    if (me == leader) q0 = atomicAdd((unsigned long long*)&B.ctr->vcount, (unsigned long long)__popcll(bal));
                    const u64 q = w_bcast(q0, leader) + (u64)__popcll(bal & ((1ull << me) - 1ull));
                    if (q < B.vcap) {
                        B.vbuf[2 * q] = i;
                        B.vbuf[2 * q + 1] = slot | ((u64)lane << 48);
                    } else {
                        atomicOr(&B.ctr->overflow, 4u);
                    }
                }
                continue;
            }
            const u64 ni = atomicAdd((unsigned long long*)&B.ctr->count, 1ull);
            if (ni >= B.cap) {
                atomicOr(&B.ctr->overflow, 1u);
                continue;
            }
            bad |= w_store<Store, Ring>(M, B, ni, t, i, lane);
            if constexpr (Verify) B.sidx[slot] = ni;
        }
        if (g == 0) atomicMin((unsigned long long*)&B.ctr->deadlock, (unsigned long long)i);
        gen += g;
    }
    gen = w_wave_sum(gen);
    probes = w_wave_sum(probes);
    if (__lane_id() == 0 && gen) atomicAdd((unsigned long long*)&B.ctr->generated, (unsigned long long)gen);
    if (__lane_id() == 0 && probes) atomicAdd((unsigned long long*)&B.ctr->probes, (unsigned long long)probes);
    if (bad) atomicOr(&B.ctr->overflow, bad << 8);
    if constexpr (Verify) {
        vchk = w_wave_sum(vchk);
        vcol = w_wave_sum(vcol);
        if (__lane_id() == 0 && vchk) atomicAdd((unsigned long long*)&B.ctr->vchecked, (unsigned long long)vchk);
        if (__lane_id() == 0 && vcol) atomicAdd((unsigned long long*)&B.ctr->collisions, (unsigned long long)vcol);
    }
}

// The deferred hits of the last expansion launch (B.vbuf[0, n)), now that the
// launch is over and every owner's record and B.sidx entry are written: the
// successor is re-derived from its parent's record by its lane and compared
// with the owner's.  A hit without an owner (or a record out of range) is
// Counters.overflow bit 3, an internal error.
template <class St, bool Sym>
__global__ __launch_bounds__(256) void k_wverify(const WModel M, const WideBufs B, u64 n) {
    u64 vchk = 0, vcol = 0;
    const St* store = static_cast<const St*>(B.store);
    for (u64 q = (u64)blockIdx.x * 256ull + threadIdx.x; q < n; q += (u64)gridDim.x * 256ull) {
        const u64 parent = B.vbuf[2 * q], sl = B.vbuf[2 * q + 1];
        const u64 slot = sl & ((1ull << 48) - 1ull);
        const int lane = (int)(sl >> 48);
        const u64 ix = parent < B.cap && slot <= B.tmask ? B.sidx[slot] : ~0ull;
        St t;
        if (ix >= B.cap || wlane(M, store[parent], lane, &t) != W_ON) {
            atomicOr(&B.ctr->overflow, 8u);
            continue;
        }
        ++vchk;
        if constexpr (Sym) vcol += wsame_orbit(store[ix], t, M.S) ? 0u : 1u;
        else vcol += wsame(store[ix], t, M.S) ? 0u : 1u;
    }
    vchk = w_wave_sum(vchk);
    vcol = w_wave_sum(vcol);
    if (__lane_id() == 0 && vchk) atomicAdd((unsigned long long*)&B.ctr->vchecked, (unsigned long long)vchk);
    if (__lane_id() == 0 && vcol) atomicAdd((unsigned long long*)&B.ctr->collisions, (unsigned long long)vcol);
}

// Action coverage (RMC_FLAG_COVERAGE; rmc_cover.h, the packed k_cover's twin): a
// pass of its own beside one expansion launch over [lo, hi).  `generated`: the
// expansion's lane walk — families 0-6, then the bag families over the state's
// messages — with only the guards evaluated on the stored record (wlane without
// a successor: anything but W_OFF counts, as in k_wexpand).  `distinct`: the
// states the launch added, [nlo, nhi), by the row of their producing lane; a
// Receive lane reads its parent's record, which the ring still holds (ring_room
// is relative to lo), and a state of the unstored last level has its links.
__device__ __forceinline__ u32 w_wave_sum32(u32 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (u32)__shfl_xor((int)v, off);
    return v;
}

template <class Store, bool Ring>
__global__ __launch_bounds__(256) void k_wcover(const WModel M, const WideBufs B, u64 lo, u64 hi, u64 nlo, u64 nhi,
                                                u64 n_init, unsigned long long* cov) {
    __shared__ u32 s_row[2 * COV_ROWS];
    if (threadIdx.x < 2 * COV_ROWS) s_row[threadIdx.x] = 0;
    __syncthreads();
    u32 g[COV_ROWS], n[COV_ROWS];
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) g[r] = n[r] = 0;
    const Store* store = static_cast<const Store*>(B.store);
    const u64 t0 = (u64)blockIdx.x * 256ull + threadIdx.x, step = (u64)gridDim.x * 256ull;
    for (u64 i = lo + t0; i < hi; i += step) {
        const Store& s = store[w_slot<Ring>(B, i)];
        const int nb = s.nmsg;
#pragma unroll 1
        for (int f = 0; f < 10; ++f) {  // one family at a time: its row is one value (Receive: per message)
            u32 on = 0;
            const int l0 = M.L.off[f], l1 = f < 7 ? M.L.off[f + 1] : l0 + nb;
#pragma unroll 1
            for (int lane = l0; lane < l1; ++lane) {
                if (wlane(M, s, lane, nullptr) == W_OFF) continue;
                if (f == 7) {
                    const int row = wcover_row(M, s, lane);
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
            const int f = M.L.family(lane);
            row = f == 7 ? -1 : cover_family_row(f);
            if (f == 7) {
                const u64 p = B.parent[i];
                if (p < lo || p >= hi) continue;  // not of this launch: left out, and the sums show it
                const Store& s = store[w_slot<Ring>(B, p)];
                if (lane - M.L.off[7] >= (int)s.nmsg) continue;
                row = wcover_row(M, s, lane);
            }
        }
#pragma unroll
        for (int r = 0; r < COV_ROWS; ++r) n[r] += row == r ? 1u : 0u;
    }
#pragma unroll
    for (int r = 0; r < COV_ROWS; ++r) {
        const u32 gs = w_wave_sum32(g[r]), ns = w_wave_sum32(n[r]);
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

// Continue past violations (RMC_FLAG_CONTINUE; rmc_viol.h, the packed k_violations'
// twin): a pass over the states one launch (or the seed) added, [nlo, nhi), on
// the store's record in place — the resident store only (rmc_create refuses the
// ring: it does not store the last level of a depth-bounded run).  Classified by
// wclassify_violations, reduced as there.
__device__ __forceinline__ u64 w_wave_min(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = (u64)(u32)__shfl_xor((int)(u32)v, off) | ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), off) << 32);
        v = o < v ? o : v;
    }
    return v;
}

template <class Store>
__global__ __launch_bounds__(256) void k_wviolations(const WModel M, const WideBufs B, u64 nlo, u64 nhi,
                                                     unsigned long long* viol) {
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
    const Store* store = static_cast<const Store*>(B.store);
    nhi = nhi < B.cap ? nhi : B.cap;  // (a launch that overflowed the store is an error: its tallies are not read)
    for (u64 i = nlo + (u64)blockIdx.x * 256ull + threadIdx.x; i < nhi; i += (u64)gridDim.x * 256ull) {
        const ViolClass c = wclassify_violations(M, store[i]);
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
        const u32 fs = w_wave_sum32(nf[r]), es = w_wave_sum32(ne[r]);
        if (!es) continue;  // (wave-uniform; first[r] <= each[r])
        const u64 lm = w_wave_min(least[r]);
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

// Model-defined invariants (rmc_pred.h, rmc_dev_pred.h: the packed k_pred's and k_pred_eval's
// twins): the BFS pass over the states one launch (or the seed) added, [nlo, nhi), on the
// store's record in place — the resident store only — and the same interpreter on staged
// records of the store's kind.  The program in LDS, each thread's stack and bound names an
// LDS column, as there.
template <class Store>
__global__ __launch_bounds__(kPredThreads) void k_wpred(const pred::Program* prog, const WModel M, const WideBufs B,
                                                        u64 nlo, u64 nhi, unsigned long long* word) {
    __shared__ PredLds L;
    pred_load(L, prog);
    const int n_pred = prog->n_pred;
    const Store* store = static_cast<const Store*>(B.store);
    u64 best = ~0ull;
    nhi = nhi < B.cap ? nhi : B.cap;  // (a launch that overflowed the store is an error: the word is not read)
    for (u64 i = nlo + (u64)blockIdx.x * kPredThreads + threadIdx.x; i < nhi; i += (u64)gridDim.x * kPredThreads) {
        const pred::WideAcc<Store> a{store + i, M.S};
        const int f = pred::first_failing<kPredThreads>(L.entry, n_pred, L.code, a, L.mem + threadIdx.x);
        if (f) {
            best = (i << 8) | (u64)(f - 1);
            break;
        }
    }
    best = pred_wave_min(best);
    if (__lane_id() == 0 && best != ~0ull) atomicMin(word, (unsigned long long)best);
}

template <class Store>
__global__ __launch_bounds__(kPredThreads) void k_wpred_eval(const pred::Program* prog, const WModel M,
                                                             const Store* in, u64 n, uint8_t* out) {
    __shared__ PredLds L;
    pred_load(L, prog);
    const int n_pred = prog->n_pred;
    const u64 t = (u64)blockIdx.x * kPredThreads + threadIdx.x;
    if (t >= n) return;
    const pred::WideAcc<Store> a{in + t, M.S};
    for (int p = 0; p < n_pred; ++p)
        out[t * (u64)n_pred + p] = (uint8_t)pred::run<kPredThreads>(L.code, L.entry[p], a, L.mem + threadIdx.x);
}

// Every enabled lane of n given states, without dedup (rmc_expand).  Sym: the
// fingerprint listed is the successor's canonical key, as k_wexpand would insert it.
template <bool Sym>
__global__ __launch_bounds__(64) void k_wlist(const WModel M, const WState* in, u64 n, WSucc* out, u64 cap,
                                             unsigned long long* count, u64 salt) {
    const u64 p = (u64)blockIdx.x * 64ull + threadIdx.x;
    if (p >= n) return;
    WState t;
    for (int lane = 0; lane < M.L.off[10]; ++lane) {
        const int r = wlane(M, in[p], lane, &t);
        if (r == W_OFF) continue;
        const u64 o = atomicAdd(count, 1ull);
        if (o >= cap) continue;
        WSucc& w = out[o];
        w.parent = p;
        w.lane = lane;
        w.code = r;
        const int inm = r == W_ON && win_model(M, t);
        w.in_model = inm;
        w.fp = !inm ? 0ull : Sym ? wcanon(t, salt, M.S).k : wfp(t, salt, M.S).k;
        if (inm) wcopy_state(w.state, t);
        else wzero(&w.state, (int)sizeof(WState));
    }
}
// The keys of n given states under SYMMETRY, one thread per state (rmc_state_keys on
// a wide ctx; the packed twin is k_keys): the key k_wseed and k_wexpand insert for
// the state (wcanon), and with ref whether their verification's comparison
// (wsame_orbit) finds state t equal to state ref[t].
__global__ __launch_bounds__(64) void k_wkeys(const WModel M, const WState* in, u64 n, u64* keys, const u32* ref,
                                             unsigned char* same, u64 salt) {
    const u64 p = (u64)blockIdx.x * 64ull + threadIdx.x;
    if (p >= n) return;
    keys[p] = wcanon(in[p], salt, M.S).k;
    if (ref) same[p] = wsame_orbit(in[p], in[ref[p]], M.S) ? 1 : 0;  // (ref[p] < n: checked by the host)
}

// ---- one wave on one record in LDS (k_wsimulate_w) ----------------------------------
// Every lane of the wave calls these with the same arguments; lane q handles
// message q (KW = 64 = the wave), so a bag search is one compare per lane and a
// ballot, and an insert / removal moves every later message at once.
__device__ __forceinline__ void w_wsync() {  // the wave's LDS writes seen by the whole wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
static_assert(KW <= 64, "WaveBag: one message per lane of the wave");
struct WaveBag {
    // slot of m in the sorted bag (-1: absent); *pos = the messages below m
    static __device__ int find(const WState& s, const WMsg& m, int* pos) {
        const int ln = (int)__lane_id();
        const int n = s.nmsg;
        const int c = ln < n ? wmsg_cmp(s.msg[ln], m) : 1;
        const u64 eq = __ballot(c == 0), lt = __ballot(c < 0);
        *pos = (int)__popcll(lt);
        return eq ? (int)__builtin_ctzll(eq) : -1;
    }
    static __device__ int fits(const WState& s, const WMsg& m) {
        int pos;
        const int k = find(s, m, &pos);
        if (k >= 0) return s.cnt[k] >= CMAX ? W_DUP : W_ON;
        return s.nmsg >= KW ? W_MSGS : W_ON;
    }
    static __device__ int reply_fits(const WState& s, const WMsg& r, int x) {
        int pos;
        const int k = find(s, r, &pos);
        if (k >= 0) return s.cnt[k] >= CMAX ? W_DUP : W_ON;
        return (s.nmsg >= KW && s.cnt[x] > 1) ? W_MSGS : W_ON;
    }
    static __device__ int add(WState& s, const WMsg& m) {  // wbag_add
        const int ln = (int)__lane_id();
        w_wsync();
        int k;
        const int e = find(s, m, &k);
        const int n = s.nmsg;
        if (e >= 0) {
            const int c = s.cnt[e];
            if (c >= CMAX) return W_DUP;
            w_wsync();
            if (ln == 0) s.cnt[e] = (uint8_t)(c + 1);
            w_wsync();
            return W_ON;
        }
        if (n >= KW) return W_MSGS;
        const bool mv = ln >= k && ln < n;  // messages k .. n-1 move up one slot
        WMsg mine;
        uint8_t c = 0;
        if (mv) {
            mine = s.msg[ln];
            c = s.cnt[ln];
        }
        w_wsync();
        if (mv) {
            s.msg[ln + 1] = mine;
            s.cnt[ln + 1] = c;
        }
        if (ln == 0) {
            s.msg[k] = m;
            s.cnt[k] = 1;
            s.nmsg = (uint8_t)(n + 1);
        }
        w_wsync();
        return W_ON;
    }
    static __device__ void remove_at(WState& s, int k) {  // wbag_remove_at
        const int ln = (int)__lane_id();
        w_wsync();
        const int c = s.cnt[k], n = s.nmsg;
        if (c > 1) {
            w_wsync();
            if (ln == 0) s.cnt[k] = (uint8_t)(c - 1);
            w_wsync();
            return;
        }
        const bool mv = ln > k && ln < n;  // messages k+1 .. n-1 move down one slot
        WMsg mine;
        uint8_t cm = 0;
        if (mv) {
            mine = s.msg[ln];
            cm = s.cnt[ln];
        }
        w_wsync();
        if (mv) {
            s.msg[ln - 1] = mine;
            s.cnt[ln - 1] = cm;
        }
        if (ln == n - 1) {  // the freed last slot (also written by no mover: n - 1 > ln - 1)
            wmsg_zero(s.msg[n - 1]);
            s.cnt[n - 1] = 0;
        }
        if (ln == 0) s.nmsg = (uint8_t)(n - 1);
        w_wsync();
    }
};

// win_model with lane q checking message q's count.
__device__ __forceinline__ int w_in_model_wave(const WModel& M, const WState& t) {
    const int ln = (int)__lane_id();
    bool bad = ln < t.nmsg && t.cnt[ln] > M.max_dup;
    if (ln < M.S) bad = bad || t.ct[ln] > M.max_term || t.len[ln] > M.max_log;
    if (ln == 0) bad = bad || t.nmsg > M.max_msgs;
    return __ballot(bad) == 0;
}

// TypeOK (raft.tla:482-492, wtype_ok) with lane i checking server i and lane q
// message q.
__device__ __forceinline__ int w_type_ok_wave(const WModel& M, const WState& s) {
    const int ln = (int)__lane_id();
    bool bad = false;
    if (ln < M.S) {
        const int i = ln;
        bad = s.st[i] > LEADER || (s.vf[i] != NIL && s.vf[i] >= M.S) || ((s.vR[i] | s.vG[i]) >> M.S) != 0;
        for (int j = 0; j < M.S; ++j) bad = bad || s.ni[i][j] < 1;
        for (int x = 0; x < s.len[i]; ++x) bad = bad || s.log[i][x].value >= M.V;
    }
    if (ln < s.nmsg) {
        const WMsg& m = s.msg[ln];
        bad = bad || s.cnt[ln] < 1 || m.src >= M.S || m.dst >= M.S;
        for (int x = 0; x < m.n; ++x) bad = bad || m.e[x].value >= M.V;
    }
    return __ballot(bad) == 0;
}

// wcheck_invariants for the whole wave (every lane gets the result): TypeOK
// lane-parallel, the other named invariants on lane 0 in wcheck_invariants'
// order.
__device__ __forceinline__ int w_check_invariants_wave(const WModel& M, const WState& s) {
    if ((M.inv_mask & 1) && !w_type_ok_wave(M, s)) return 1;
    if (!(M.inv_mask & ~1)) return 0;
    WModel M2 = M;
    M2.inv_mask &= ~1;
    const int v = __lane_id() == 0 ? wcheck_invariants(M2, s) : 0;
    return __shfl(v, 0);
}

// Random behaviours (TLC -simulate): one thread per behaviour, from one of the
// n_init staged initial states, up to depth - 1 steps.  mode 0: uniform over
// the enabled successors within the bounds (rejection: an out-of-bounds draw
// is excluded and the draw repeated; uniform_draw); 1: uniform over every enabled successor,
// one beyond the bounds ends the behaviour (truncated); 2: TLC's draw
// (tlc_draw: random start, random prime stride, the first enabled action, a
// uniform successor of it); beyond the bounds it is truncated like mode 1.
__global__ __launch_bounds__(64) void k_wsimulate(const WModel M, const WState* inits, u64 n_init, u64 n_beh, int depth,
                                                 u64 seed, int mode, SimCounters* out, i64 rec_beh, WState* rec) {
    u64 steps = 0, trunc = 0, dead = 0;
    const int nl = M.L.off[10];
    for (u64 b = (u64)blockIdx.x * 64ull + threadIdx.x; b < n_beh; b += (u64)gridDim.x * 64ull) {
        if (rec_beh >= 0 && (i64)b != rec_beh) continue;
        u64 rs = mix64(seed ^ (b * 0xD1B54A32D192ED03ull));
        // two records used in turn (the successor becomes the current state by
        // swapping the roles, not by a 5-KB copy)
        WState buf[2];
        int cur = 0;
        wcopy_state(buf[0], inits[w_rand(rs) % n_init]);
        const bool record = (i64)b == rec_beh;
        if (record) wcopy_state(rec[0], buf[cur]);
        int v = wcheck_invariants(M, buf[cur]);
        if (v) atomicMin((unsigned long long*)&out->viol, (unsigned long long)((1ull << 44) | ((u64)(v - 1) << 40) | b));
        u64 excl[WLMASK] = {};  // mode 0: lanes whose successor left the bounds this step
        for (int dd = 2; dd <= depth && !v;) {
            u64 en[WLMASK] = {};
            for (int lane = 0; lane < nl; ++lane)
                if (wlane(M, buf[cur], lane, nullptr) != W_OFF) en[lane >> 6] |= 1ull << (lane & 63);
            const int pick = mode == 2 ? tlc_draw<WLMASK>(en, M.L, M.V, rs)  // TLC's draw
                                       : uniform_draw<WLMASK>(en, excl, rs);
            if (pick < 0) {
                u64 any = 0;
                for (int q = 0; q < WLMASK; ++q) any |= excl[q];
                if (any) ++trunc;  // mode 0: every enabled successor leaves the bounds
                else ++dead;
                break;
            }
            const int r = wlane(M, buf[cur], pick, &buf[cur ^ 1]);
            if (r != W_ON || !win_model(M, buf[cur ^ 1])) {
                if (mode == 0) {  // exclude it and draw again (a lane whose successor overflows too)
                    excl[pick >> 6] |= 1ull << (pick & 63);
                    continue;
                }
                ++trunc;
                break;
            }
            cur ^= 1;
            for (int q = 0; q < WLMASK; ++q) excl[q] = 0;
            ++steps;
            if (record) wcopy_state(rec[dd - 1], buf[cur]);
            v = wcheck_invariants(M, buf[cur]);
            if (v)
                atomicMin((unsigned long long*)&out->viol, (unsigned long long)(((u64)dd << 44) | ((u64)(v - 1) << 40) | b));
            ++dd;
        }
    }
    atomicAdd((unsigned long long*)&out->steps, (unsigned long long)steps);
    if (trunc) atomicAdd((unsigned long long*)&out->truncated, (unsigned long long)trunc);
    if (dead) atomicAdd((unsigned long long*)&out->deadlocked, (unsigned long long)dead);
}

// The same walks, one WAVE per behaviour (RMC_WSIM=1, the default): the two
// 5-KB records live in LDS instead of one lane's private memory, the 64 lanes
// evaluate the action guards in parallel (a ballot per 64 lanes of the lane
// table), copy the record together, apply the drawn action together (the
// scalar fields by every lane alike, the bag one message per lane: WaveBag)
// and check TypeOK and the CONSTRAINT one server / message per lane.  The
// draws are the thread kernel's (the same random stream per behaviour), so
// both give the same behaviours.
constexpr int WSIM_WAVES = 4;  // behaviours per 256-thread block (2 x 5,080 B of LDS each)
__global__ __launch_bounds__(64 * WSIM_WAVES) __attribute__((amdgpu_waves_per_eu(4))) void k_wsimulate_w(const WModel M, const WState* inits, u64 n_init,
                                                                u64 n_beh, int depth, u64 seed, int mode,
                                                                SimCounters* out, i64 rec_beh, WState* rec,
                                                                int inplace) {
    __shared__ WState s_buf[WSIM_WAVES][2];
    const int wv = (int)(threadIdx.x >> 6), ln = (int)(threadIdx.x & 63);
    u64 steps = 0, trunc = 0, dead = 0;  // lane 0's tallies
    const int nl = M.L.off[10];
    constexpr int NC = (WLANES_MAX + 63) / 64;  // 64-lane chunks of the lane table
    auto copy = [&](WState& d, const WState& s) {  // the whole wave, 8 bytes a lane at a time
        u64* x = reinterpret_cast<u64*>(&d);
        const u64* y = reinterpret_cast<const u64*>(&s);
        for (int k = ln; k < WWORDS; k += 64) x[k] = y[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    for (u64 b = (u64)blockIdx.x * WSIM_WAVES + wv; b < n_beh; b += (u64)gridDim.x * WSIM_WAVES) {  // wave-uniform
        if (rec_beh >= 0 && (i64)b != rec_beh) continue;
        u64 rs = mix64(seed ^ (b * 0xD1B54A32D192ED03ull));  // every lane: the same stream
        int cur = 0;
        copy(s_buf[wv][0], inits[w_rand(rs) % n_init]);
        const bool record = (i64)b == rec_beh;
        if (record && ln == 0) wcopy_state(rec[0], s_buf[wv][0]);
        int v = w_check_invariants_wave(M, s_buf[wv][0]);
        if (v && ln == 0)
            atomicMin((unsigned long long*)&out->viol, (unsigned long long)((1ull << 44) | ((u64)(v - 1) << 40) | b));
        u64 excl[WLMASK] = {};  // mode 0: lanes whose successor left the bounds this step (uniform)
        for (int dd = 2; dd <= depth && !v;) {
            const WState& s = s_buf[wv][cur];
            // guards in parallel: en[c] bit l = lane 64 c + l enabled (wave-uniform masks)
            u64 en[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int lane = 64 * c + ln;
                const bool on = lane < nl && wlane(M, s, lane, nullptr) != W_OFF;
                en[c] = __ballot(on);
            }
            static_assert(NC == WLMASK, "one mask word per 64 lanes");
            const int pick = mode == 2 ? tlc_draw<NC>(en, M.L, M.V, rs)  // k_wsimulate's draws exactly
                                       : uniform_draw<NC>(en, excl, rs);
            if (pick < 0) {
                u64 any = 0;
                for (int q = 0; q < WLMASK; ++q) any |= excl[q];
                if (any) ++trunc;
                else ++dead;
                break;
            }
            // mode 0 may redraw from s: the successor goes to the other record.
            // Otherwise a failed draw ends the behaviour, so the successor is
            // written over s in place (wlane reads every field of s before it
            // writes it) and the 5-KB copy is skipped.
            const bool inp = inplace && mode != 0;
            WState& t = s_buf[wv][inp ? cur : cur ^ 1];
            if (!inp) copy(t, s);
            const int r = wlane<WaveBag>(M, s, pick, &t, true);  // every lane: the same r
            w_wsync();
            if (r != W_ON || !w_in_model_wave(M, t)) {
                if (mode == 0) {
                    excl[pick >> 6] |= 1ull << (pick & 63);
                    continue;
                }
                ++trunc;
                break;
            }
            if (!inp) cur ^= 1;
            for (int q = 0; q < WLMASK; ++q) excl[q] = 0;
            ++steps;
            if (record && ln == 0) wcopy_state(rec[dd - 1], t);
            v = w_check_invariants_wave(M, t);
            if (v && ln == 0)
                atomicMin((unsigned long long*)&out->viol, (unsigned long long)(((u64)dd << 44) | ((u64)(v - 1) << 40) | b));
            ++dd;
        }
    }
    if (ln == 0) {
        atomicAdd((unsigned long long*)&out->steps, (unsigned long long)steps);
        if (trunc) atomicAdd((unsigned long long*)&out->truncated, (unsigned long long)trunc);
        if (dead) atomicAdd((unsigned long long*)&out->deadlocked, (unsigned long long)dead);
    }
}

// The invariants of n given states (rmc_check_states): one thread per state with
// the BFS's and k_wsimulate's wcheck_invariants, or one wave per state on a copy
// in LDS with k_wsimulate_w's w_check_invariants_wave.  They call those and
// nothing else.
__global__ __launch_bounds__(64) void k_wcheck(const WModel M, const WState* in, u64 n, int* out) {
    const u64 p = (u64)blockIdx.x * 64ull + threadIdx.x;
    if (p >= n) return;
    out[p] = wcheck_invariants(M, in[p]);
}
__global__ __launch_bounds__(64 * WSIM_WAVES) void k_wcheck_w(const WModel M, const WState* in, u64 n, int* out) {
    __shared__ WState s_buf[WSIM_WAVES];
    const int wv = (int)(threadIdx.x >> 6), ln = (int)(threadIdx.x & 63);
    for (u64 p = (u64)blockIdx.x * WSIM_WAVES + wv; p < n; p += (u64)gridDim.x * WSIM_WAVES) {  // wave-uniform
        u64* x = reinterpret_cast<u64*>(&s_buf[wv]);
        const u64* y = reinterpret_cast<const u64*>(&in[p]);
        for (int k = ln; k < WWORDS; k += 64) x[k] = y[k];
        w_wsync();
        const int v = w_check_invariants_wave(M, s_buf[wv]);
        if (ln == 0) out[p] = v;
        w_wsync();  // every lane has read the record before the next state overwrites it
    }
}

// ---- host launchers ---------------------------------------------------------------
static unsigned grid_for(u64 n, u64 threads, u64 maxg) {
    const u64 b = (n + threads - 1) / threads;
    return (unsigned)(b < maxg ? (b ? b : 1) : maxg);
}

// The record pairs <store, work> of a ctx (WideBufs.compact / .work: 0 WState,
// 1 WStateC, 2 WStateD): without the ring the store's record on both sides
// (the three kernels of round 6), with it every pair whose work record is no
// smaller than the store's.
template <class F>
static bool w_dispatch(const WideBufs& B, F f) {
    if (!B.window) {
        if (B.compact == 2) f((WStateD*)nullptr, (WStateD*)nullptr, std::false_type{});
        else if (B.compact) f((WStateC*)nullptr, (WStateC*)nullptr, std::false_type{});
        else f((WState*)nullptr, (WState*)nullptr, std::false_type{});
        return true;
    }
    const int p = B.compact * 3 + B.work;
    switch (p) {
        case 2 * 3 + 2: f((WStateD*)nullptr, (WStateD*)nullptr, std::true_type{}); return true;
        case 2 * 3 + 1: f((WStateD*)nullptr, (WStateC*)nullptr, std::true_type{}); return true;
        case 2 * 3 + 0: f((WStateD*)nullptr, (WState*)nullptr, std::true_type{}); return true;
        case 1 * 3 + 1: f((WStateC*)nullptr, (WStateC*)nullptr, std::true_type{}); return true;
        case 1 * 3 + 0: f((WStateC*)nullptr, (WState*)nullptr, std::true_type{}); return true;
        case 0: f((WState*)nullptr, (WState*)nullptr, std::true_type{}); return true;
    }
    return false;  // a work record smaller than the store's: no such kernel
}

// B.sym (RMC_FLAG_SYMMETRY): the instantiation with the canonical key.
template <class F>
static void w_sym(const WideBufs& B, F f) {
    if (B.sym) f(std::true_type{});
    else f(std::false_type{});
}

// (B.verify: the Verify kernels, which exist for the resident store only)
hipError_t launch_wseed(const WModel& M, const WideBufs& B, const void* staged, u64 n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (B.verify && B.window) return hipErrorInvalidValue;
    const bool ok = w_dispatch(B, [&](auto* sp, auto* wp, auto ring) {
        typedef std::remove_pointer_t<decltype(sp)> Store;
        typedef std::remove_pointer_t<decltype(wp)> Work;
        constexpr bool Ring = decltype(ring)::value;
        const dim3 grid(grid_for(n, 256, 1024));
        w_sym(B, [&](auto sym) {
            constexpr bool Sym = decltype(sym)::value;
            if constexpr (!Ring) {
                if (B.verify) {
                    hipLaunchKernelGGL((k_wseed<Store, Work, false, true, Sym>), grid, dim3(256), 0, st, M, B,
                                       static_cast<const Work*>(staged), n);
                    return;
                }
            }
            hipLaunchKernelGGL((k_wseed<Store, Work, Ring, false, Sym>), grid, dim3(256), 0, st, M, B,
                               static_cast<const Work*>(staged), n);
        });
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
hipError_t launch_wexpand(const WModel& M, const WideBufs& B, u64 lo, u64 hi, hipStream_t st) {
    if (hi <= lo) return hipSuccess;
    if (B.verify && B.window) return hipErrorInvalidValue;
    const bool ok = w_dispatch(B, [&](auto* sp, auto* wp, auto ring) {
        typedef std::remove_pointer_t<decltype(sp)> Store;
        typedef std::remove_pointer_t<decltype(wp)> Work;
        constexpr bool Ring = decltype(ring)::value;
        const dim3 grid(grid_for(hi - lo, 256, 4096));
        w_sym(B, [&](auto sym) {
            constexpr bool Sym = decltype(sym)::value;
            if constexpr (!Ring) {
                if (B.verify) {
                    hipLaunchKernelGGL((k_wexpand<Store, Work, false, true, Sym>), grid, dim3(256), 0, st, M, B, lo, hi);
                    return;
                }
            }
            hipLaunchKernelGGL((k_wexpand<Store, Work, Ring, false, Sym>), grid, dim3(256), 0, st, M, B, lo, hi);
        });
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
hipError_t launch_wverify(const WModel& M, const WideBufs& B, u64 n, hipStream_t st) {
    if (!n) return hipSuccess;
    if (!B.verify || B.window || n > B.vcap) return hipErrorInvalidValue;
    const dim3 grid(grid_for(n, 256, 4096));
    w_sym(B, [&](auto sym) {
        constexpr bool Sym = decltype(sym)::value;
        if (B.compact == 2) hipLaunchKernelGGL((k_wverify<WStateD, Sym>), grid, dim3(256), 0, st, M, B, n);
        else if (B.compact) hipLaunchKernelGGL((k_wverify<WStateC, Sym>), grid, dim3(256), 0, st, M, B, n);
        else hipLaunchKernelGGL((k_wverify<WState, Sym>), grid, dim3(256), 0, st, M, B, n);
    });
    return hipGetLastError();
}
hipError_t launch_wcover(const WModel& M, const WideBufs& B, u64 lo, u64 hi, u64 nlo, u64 nhi, u64 n_init,
                         unsigned long long* cov, hipStream_t st) {
    const u64 np = hi > lo ? hi - lo : 0, nn = nhi > nlo ? nhi - nlo : 0;
    const dim3 grid(grid_for(np > nn ? np : nn, 256, 4096));
    // the store's record on both sides: the guards read it in place (no work record)
    const bool ok = w_dispatch(B, [&](auto* sp, auto*, auto ring) {
        typedef std::remove_pointer_t<decltype(sp)> Store;
        constexpr bool Ring = decltype(ring)::value;
        hipLaunchKernelGGL((k_wcover<Store, Ring>), grid, dim3(256), 0, st, M, B, lo, hi, nlo, nhi, n_init, cov);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}
hipError_t launch_wviolations(const WModel& M, const WideBufs& B, u64 nlo, u64 nhi, unsigned long long* viol,
                              hipStream_t st) {
    if (nhi <= nlo) return hipSuccess;
    if (B.window) return hipErrorInvalidValue;  // the resident store only
    const dim3 grid(grid_for(nhi - nlo, 256, 4096));
    if (B.compact == 2) hipLaunchKernelGGL(k_wviolations<WStateD>, grid, dim3(256), 0, st, M, B, nlo, nhi, viol);
    else if (B.compact) hipLaunchKernelGGL(k_wviolations<WStateC>, grid, dim3(256), 0, st, M, B, nlo, nhi, viol);
    else hipLaunchKernelGGL(k_wviolations<WState>, grid, dim3(256), 0, st, M, B, nlo, nhi, viol);
    return hipGetLastError();
}
hipError_t launch_wpred(const pred::Program* prog, const WModel& M, const WideBufs& B, u64 nlo, u64 nhi,
                        unsigned long long* word, hipStream_t st) {
    if (nhi <= nlo) return hipSuccess;
    if (B.window) return hipErrorInvalidValue;  // the resident store only
    const dim3 grid(grid_for(nhi - nlo, kPredThreads, 4096)), block(kPredThreads);
    if (B.compact == 2) hipLaunchKernelGGL(k_wpred<WStateD>, grid, block, 0, st, prog, M, B, nlo, nhi, word);
    else if (B.compact) hipLaunchKernelGGL(k_wpred<WStateC>, grid, block, 0, st, prog, M, B, nlo, nhi, word);
    else hipLaunchKernelGGL(k_wpred<WState>, grid, block, 0, st, prog, M, B, nlo, nhi, word);
    return hipGetLastError();
}
hipError_t launch_wpred_eval(const pred::Program* prog, const WModel& M, int compact, const void* in, u64 n,
                             uint8_t* out, hipStream_t st) {
    if (!n) return hipSuccess;
    const dim3 grid(grid_for(n, kPredThreads, 1u << 22)), block(kPredThreads);
    if (compact == 2)
        hipLaunchKernelGGL(k_wpred_eval<WStateD>, grid, block, 0, st, prog, M, static_cast<const WStateD*>(in), n, out);
    else if (compact)
        hipLaunchKernelGGL(k_wpred_eval<WStateC>, grid, block, 0, st, prog, M, static_cast<const WStateC*>(in), n, out);
    else
        hipLaunchKernelGGL(k_wpred_eval<WState>, grid, block, 0, st, prog, M, static_cast<const WState*>(in), n, out);
    return hipGetLastError();
}
hipError_t launch_wlist(const WModel& M, const WState* in, u64 n, WSucc* out, u64 cap, unsigned long long* count,
                        u64 salt, int sym, hipStream_t st) {
    if (!n) return hipSuccess;
    const dim3 grid(grid_for(n, 64, 1u << 20));
    if (sym) hipLaunchKernelGGL(k_wlist<true>, grid, dim3(64), 0, st, M, in, n, out, cap, count, salt);
    else hipLaunchKernelGGL(k_wlist<false>, grid, dim3(64), 0, st, M, in, n, out, cap, count, salt);
    return hipGetLastError();
}
hipError_t launch_wkeys(const WModel& M, const WState* in, u64 n, u64* keys, const u32* ref, unsigned char* same,
                        u64 salt, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_wkeys, dim3(grid_for(n, 64, 1u << 20)), dim3(64), 0, st, M, in, n, keys, ref, same, salt);
    return hipGetLastError();
}
hipError_t launch_wsimulate(const WModel& M, const WState* inits, u64 n_init, u64 n_beh, int depth, u64 seed, int mode,
                            SimCounters* out, i64 rec_beh, WState* rec, hipStream_t st) {
    static const int wave = [] {  // RMC_WSIM=0: one thread per behaviour (k_wsimulate, A/B)
        const char* e = getenv("RMC_WSIM");
        return e ? atoi(e) : 1;
    }();
    static const int inplace = [] {  // RMC_WSIM_INPLACE=0: every successor to the other record (A/B)
        const char* e = getenv("RMC_WSIM_INPLACE");
        return e ? atoi(e) : 1;
    }();
    if (wave)
        hipLaunchKernelGGL(k_wsimulate_w, dim3(grid_for(n_beh, WSIM_WAVES, 8192)), dim3(64 * WSIM_WAVES), 0, st, M,
                           inits, n_init, n_beh, depth, seed, mode, out, rec_beh, rec, inplace);
    else
        hipLaunchKernelGGL(k_wsimulate, dim3(grid_for(n_beh, 64, 16384)), dim3(64), 0, st, M, inits, n_init, n_beh,
                           depth, seed, mode, out, rec_beh, rec);
    return hipGetLastError();
}
hipError_t launch_wcheck(const WModel& M, const WState* in, u64 n, int* out, int wave, hipStream_t st) {
    if (!n) return hipSuccess;
    if (wave)
        hipLaunchKernelGGL(k_wcheck_w, dim3(grid_for(n, WSIM_WAVES, 8192)), dim3(64 * WSIM_WAVES), 0, st, M, in, n, out);
    else
        hipLaunchKernelGGL(k_wcheck, dim3(grid_for(n, 64, 1u << 20)), dim3(64), 0, st, M, in, n, out);
    return hipGetLastError();
}

}  // namespace wide
}  // namespace rmc
