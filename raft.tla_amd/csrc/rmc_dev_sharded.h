// rmc_dev_sharded.h — the sharded search's device side: owner ranks, the expansion's sharded
// flushes (flush_dist, flush_pool), the pool's routing (k_route, k_route_fix), the owner-side
// kernels of the two-phase exchange (k_materialize_remote, k_store_remote, k_compare_remote)
// and SYMMETRY's k_ties.  The outboxes themselves: rmc_dev_outbox.h.
#pragma once
#include <hip/hip_runtime.h>

#include "raft_packed.h"
#include "rmc_dev_outbox.h"
#include "rmc_dev_set.h"
#include "rmc_dev_state.h"
#include "rmc_dev_verify.h"
#include "rmc_internal.h"

namespace rmc {

// Owner rank of a state in sharded mode.  Mode 0: by fingerprint.  Mode 1: by
// server 0's word — a successor that does not touch server 0 (bag-only
// actions, actions of the other servers) stays on its parent's rank, so far
// fewer successors cross GPUs; balance relies on server 0's many word values.
// Mode 2 (default): by the words of servers 0 and 1 (more distinct values:
// better balance, successors of two servers cross).  The word hash is the
// fingerprint's own component mix hS(w, i): the expansion kernel has the
// parent's mixes and the new word's mix at hand, so routing a successor costs
// no extra mix64 (and no extra registers) in its lane loop.
// Number of server words the owner hashes: mode 1 one, 2 two, 3 all S.
template <int S>
__device__ __forceinline__ int owner_words(const DevBufs& B) {
    return B.owner_mode >= 3 ? S : (int)B.owner_mode;
}
template <int S>
__device__ __forceinline__ u32 owner_state(u64 key, const u64 (&w)[S], const DevBufs& B) {
    if (B.owner_mode == 0) return owner_of(key, B.world);
    const int nw = owner_words<S>(B);
    u64 h = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) h += i < nw ? hS(w[i], (u32)i) : 0ull;
    return owner_of(h, B.world);
}
// Owner of a successor from the parent's words (kernels without the parent's mixes).
template <int S>
__device__ __forceinline__ u32 owner_succ_w(u64 key, const Delta& d, const u64 (&w)[S], const DevBufs& B) {
    if (B.owner_mode == 0) return owner_of(key, B.world);
    if (d.srv < 0 || d.srv >= owner_words<S>(B)) return B.rank;
    u64 ws[S];
#pragma unroll
    for (int i = 0; i < S; ++i) ws[i] = i == d.srv ? d.w_new : w[i];
    return owner_state<S>(key, ws, B);
}
// Owner of a successor from the parent's word mixes (pm.hw) and the new word's
// mix hn (delta_fp_pre): a lane that leaves the hashed words alone keeps its
// parent's owner `powner` — this rank in the sharded kernel (a state is
// expanded by its owner), the record's rank in a replicated level.
template <int S, int K>
__device__ __forceinline__ u32 owner_succ(u64 key, const Delta& d, const ParentMix<S, K>& pm, u64 hn,
                                          const DevBufs& B, u32 powner) {
    if (B.world == 1) return 0;
    if (B.owner_mode == 0) return owner_of(key, B.world);
    const int nw = owner_words<S>(B);
    if (d.srv < 0 || d.srv >= nw) return powner;
    u64 h = 0;
#pragma unroll
    for (int i = 0; i < S; ++i) h += i < nw ? (i == d.srv ? hn : pm.hw[i]) : 0ull;
    return owner_of(h, B.world);
}

template <int S, int K>
__device__ __forceinline__ Fp fp_of_materialised(const u64 (&w)[S], const u32 (&m)[K], const Params& P) {
    return state_fp<S, K>(w, m);  // = the incremental key: the fp is order-free
}

// Sharded mode, phase 1 (fingerprint first): the listed
// successors carry their owner rank.  Owned ones were inserted into the local
// set at probe time and are stored as in flush_new; for the others only the
// key travels: it goes to the owner's key outbox, with a local ticket (parent
// index | lane << 56) kept here so that, if the owner answers "new", phase 2
// re-derives the successor and ships the state.  Slots are reserved with one
// atomic per destination per flush.
template <int S, int K>
__device__ __forceinline__ void flush_dist(const Params& P, const DevBufs& B, u64 lo, const u32* l_rel,
                                           const uint8_t* l_lane, const uint8_t* l_dest, const u64* l_key,
                                           const u32* l_ks, u32 n) {
    constexpr int NW = 2 * S + K;
    wave_sync_lds();
    const int me = (int)__lane_id();
    const u64 lt = (1ull << me) - 1ull;
    // Reserve every destination's slots for the whole list with ONE atomic per
    // destination: lane dd (world <= 64) counts destination dd's entries, adds
    // them to dd's counter, then hands out consecutive slots round by round.
    u64 mine = 0;  // lane dd: entries for destination dd, then its next slot
    for (u32 e0 = 0; e0 < n; e0 += 64) {
        const u32 e = e0 + (u32)me;
        const u32 dest = e < n ? l_dest[e] : 0xFFu;
        for (u32 dd = 0; dd < B.world; ++dd) {
            const u64 bal = __ballot(dest == dd);
            if ((u32)me == dd) mine += (u64)__popcll(bal);
        }
    }
    if ((u32)me < B.world && mine) {
        unsigned long long* ctr = (u32)me == B.rank ? (unsigned long long*)&B.ctr->count : &B.ocount[me];
        mine = atomicAdd(ctr, (unsigned long long)mine);
    }
    for (u32 e0 = 0; e0 < n; e0 += 64) {  // wave-uniform rounds
        const u32 e = e0 + (u32)me;
        const bool valid = e < n;
        const u32 dest = valid ? l_dest[e] : 0xFFu;
        u64 slot = ~0ull;
        for (u32 dd = 0; dd < B.world; ++dd) {
            const u64 bal = __ballot(dest == dd);
            if (!bal) continue;
            const u64 base = bcast64(mine, (int)dd);
            if (dest == dd) slot = base + (u64)__popcll(bal & lt);
            if ((u32)me == dd) mine += (u64)__popcll(bal);
        }
        if (!valid) continue;
        const u64 rel = l_rel[e];
        const int lane = l_lane[e];
        if (dest != B.rank) {  // the key to its owner, the ticket stays here
            if (slot >= B.kcap) {
                // the owner's outbox is full: park the key with its ticket; a later
                // exchange round of this level sends it (the sent-cache entry
                // written at probe time stays right: the key IS sent)
                // (the list holds the local table value: the raw k is v ^ (s32 & tmask))
                park_key(B, l_key[e] ^ ((u64)l_ks[e] & B.tmask), l_ks[e],
                         (lo + rel) | ((u64)dest << 48) | ((u64)lane << 56));
                continue;
            }
            put_key(B, dest, slot, l_key[e] ^ ((u64)l_ks[e] & B.tmask), l_ks[e], (lo + rel) | ((u64)lane << 56));
            continue;
        }
        if (slot >= B.cap) {
            atomicOr(&B.ctr->overflow, 1u);
            continue;
        }
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + (lo + rel) * (u64)NW, w, m);
        Delta d;
        lane_delta<S, K>(w, m, lane, P, d);
        u64 wo[S];
        u32 mo[K];
        materialise<S, K>(w, m, d, wo, mo);
        store_new<S, K>(P, B, slot, wo, mo, B.ref_tag | (lo + rel), lane, make_foot<S, K>(m, lane, d, P));
    }
    wave_sync_lds();
}

// Sharded mode with send markers (MARK): the local fingerprint set doubles as
// the record of keys already sent — a successor owned elsewhere is CAS-inserted
// into it like a local one, so the probe loop is the single-GPU loop (no owner
// computed per probe) and a remote key is shipped at most once per rank.  The
// list carries only (rel, lane).  The pool flush: flush_new with the owner decided per listed successor from its materialised words — a lane that
// leaves the hashed words alone keeps its parent's owner, this rank — and two
// reservation atomics per 64 entries, one for the local store, one for the
// remote-successor pool (B.pool).  A remote successor is written there once, as
// its phase-2 record; keying it, the per-destination slots and parking are left
// to k_route after the launch.  So the flush carries no per-destination
// bookkeeping, no second pass over the list and no re-hash of the successor,
// and the sharded kernel keeps the single-GPU kernel's registers.  A pool that
// is full parks the successor's ticket with key 0 (k_route keys it).
template <int S, int K>
__device__ __forceinline__ void flush_pool(const Params& P, const DevBufs& B, u64 lo, const u32* l_rel,
                                           const uint8_t* l_lane, uint8_t* l_own, u32 n) {
    constexpr int NW = 2 * S + K, RW = NW + 4;
    wave_sync_lds();
    const int me = (int)__lane_id();
    const u64 lt = (1ull << me) - 1ull;
    // pass 1 (more than one rank): which listed successors this rank owns (LDS
    // byte per entry): only lanes that change a hashed server word can leave
    u32 nown = n;  // wave-uniform
    if (B.world > 1) {
        nown = 0;
        for (u32 e0 = 0; e0 < n; e0 += 64) {
            const u32 e = e0 + (u32)me;
            bool own = true;
            if (e < n) {
                const int lane = l_lane[e];
                Delta d;
                u64 w[S];
                u32 m[K];
                load_state<S, K>(B.store + (lo + l_rel[e]) * (u64)NW, w, m);
                lane_delta_desc<S, K>(w, m, P.ldesc[lane], P, d);
                if (B.owner_mode == 0) {
                    u64 wo[S];
                    u32 mo[K];
                    materialise<S, K>(w, m, d, wo, mo);
                    own = owner_of(fp_of_materialised<S, K>(wo, mo, P).k, B.world) == B.rank;
                } else if (d.srv >= 0 && d.srv < owner_words<S>(B)) {
                    own = owner_succ_w<S>(0ull, d, w, B) == B.rank;
                }
                l_own[e] = own ? 1 : 0;
            }
            nown += (u32)__popcll(__ballot(e < n && own));
        }
        wave_sync_lds();
    }
    u64 base_l = 0, base_r = 0;
    if (me == 0 && nown) base_l = atomicAdd((unsigned long long*)&B.ctr->count, (unsigned long long)nown);
    if (me == 0 && n > nown) base_r = atomicAdd(B.npool, (unsigned long long)(n - nown));
    base_l = bcast64(base_l, 0);
    base_r = bcast64(base_r, 0);
    for (u32 e0 = 0; e0 < n; e0 += 64) {  // wave-uniform rounds
        const u32 e = e0 + (u32)me;
        const bool valid = e < n;
        const bool own = valid && (B.world == 1 || l_own[e]);
        const u64 bl = __ballot(own), br = __ballot(valid && !own);
        const u64 ql = base_l + (u64)__popcll(bl & lt), qr = base_r + (u64)__popcll(br & lt);
        base_l += (u64)__popcll(bl);
        base_r += (u64)__popcll(br);
        if (!valid) continue;
        const u64 rel = l_rel[e];
        const int lane = l_lane[e];
        if (own && ql >= B.cap) {
            atomicOr(&B.ctr->overflow, 1u);
            continue;
        }
        if (!own && qr >= B.pool_cap) {  // pool full: park the ticket, k_route_fix keys it
            park_key(B, 0ull, OVF_UNKEYED, (lo + rel) | ((u64)lane << 56));
            continue;
        }
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + (lo + rel) * (u64)NW, w, m);
        Delta d;
        const u32 desc = P.ldesc[lane];
        lane_delta_desc<S, K>(w, m, desc, P, d);
        const u64 foot = make_foot_desc<S, K>(m, desc, d);
        u64 wo[S];
        u32 mo[K];
        materialise<S, K>(w, m, d, wo, mo);
        const u64 parent = B.ref_tag | (lo + rel);
        if (own) {
            store_new<S, K>(P, B, ql, wo, mo, parent, lane, foot);
            continue;
        }
        u32* r = B.pool + qr * (u64)RW;
        store_state<S, K>(r, wo, mo);
        const u64 ref = parent | ((u64)lane << 40);
        r[NW] = (u32)ref;
        r[NW + 1] = (u32)(ref >> 32);
        r[NW + 2] = (u32)foot;
        r[NW + 3] = (u32)(foot >> 32);
    }
    wave_sync_lds();
}

// Sharded mode, after a pool-flush expansion (k_expand_dist<POOL>): every pool
// record [0, npool) gets its key (the state's fingerprint: order-free, so equal
// to the incremental probe key) and owner and goes to that owner's outbox as
// POOL_TICK | index, one reservation atomic per destination present in a wave;
// what does not fit is parked as a parent ticket (the pool is reused by the
// round after next, the parent store is not).
template <int S, int K>
__global__ __launch_bounds__(256) void k_route(const Params P, const DevBufs B) {
    constexpr int NW = 2 * S + K, RW = NW + 4;
    const int me = (int)__lane_id();
    const u64 lt = (1ull << me) - 1ull;
    const u64 np = *B.npool < B.pool_cap ? *B.npool : B.pool_cap;
    for (u64 t0 = (u64)blockIdx.x * 256ull; t0 < np; t0 += (u64)gridDim.x * 256ull) {  // wave-uniform
        const u64 t = t0 + threadIdx.x;
        const bool live = t < np;
        Fp key{0, 0};
        u64 ref = 0;
        u32 dest = 0xFFFFFFFFu;
        if (live) {
            const u32* r = B.pool + t * (u64)RW;
            u64 w[S];
            u32 m[K];
            load_state<S, K>(r, w, m);
            key = fp_of_materialised<S, K>(w, m, P);
            dest = owner_state<S>(key.k, w, B);
            ref = (u64)r[NW] | ((u64)r[NW + 1] << 32);
        }
        u64 slot = ~0ull;
        u64 pending = __ballot(live);
        while (pending) {  // wave-uniform: one atomic per destination present
            const int l = __ffsll((long long)pending) - 1;
            const u32 dd = (u32)__builtin_amdgcn_readlane((int)dest, l);
            const u64 bal = __ballot(dest == dd);
            u64 base = 0;
            if (me == l) base = atomicAdd(&B.ocount[dd], (unsigned long long)__popcll(bal));
            base = bcast64(base, l);
            if (dest == dd) slot = base + (u64)__popcll(bal & lt);
            pending &= ~bal;
        }
        if (!live) continue;
        if (slot < B.kcap) {
            put_key(B, dest, slot, key.k, (u32)key.s, POOL_TICK | t);
            continue;
        }
        // the owner's outbox is full: park it with its parent ticket (a later round sends it)
        park_key(B, key.k, (u32)key.s,
                 (ref & ((1ull << 40) - 1)) | ((u64)dest << 48) | (((ref >> 40) & 0xFFull) << 56));
    }
}
// Before k_route: the tickets the expansion itself parked (pool full) are
// OVF_UNKEYED until keyed here (k_route's own parked records carry theirs).
template <int S, int K>
__global__ __launch_bounds__(256) void k_route_fix(const Params P, const DevBufs B) {
    constexpr int NW = 2 * S + K;
    const u64 nov = B.ctr->novf < B.ovf_cap ? B.ctr->novf : B.ovf_cap;
    for (u64 q = (u64)blockIdx.x * 256ull + threadIdx.x; q < nov; q += (u64)gridDim.x * 256ull) {
        if (!(B.ovf[3 * q + 1] & OVF_UNKEYED)) continue;
        const u64 tk = B.ovf[3 * q + 2];
        const u64 pidx = tk & ((1ull << 48) - 1);
        const int lane = (int)(tk >> 56);
        u64 wo[S];
        u32 mo[K];
        derive_succ<S, K>(B.store + pidx * (u64)NW, lane, P, wo, mo);
        const Fp key = fp_of_materialised<S, K>(wo, mo, P);
        B.ovf[3 * q] = key.k;
        B.ovf[3 * q + 2] = pidx | ((u64)owner_state<S>(key.k, wo, B) << 48) | ((u64)lane << 56);
        B.ovf[3 * q + 1] = (u32)key.s;
    }
}

// Sharded mode, phase 2, sender side: for every key an owner accepted
// (reply[d * kcap + i] = 1), re-derive the successor from its ticket and put
// the record {state, global parent ref | lane << 40} into owner d's state
// outbox.  Grid over (destination, key index).
// Full-state verification (B.sidx set): every key is shipped, the ones the
// owner had seen flagged REF_SEEN (parent-ref word), so the owner compares them with its state.
template <int S, int K>
__global__ __launch_bounds__(256) void k_materialize_remote(const Params P, const DevBufs B, const uint8_t* reply,
                                                            u64 per_dest, u64 i0) {
    constexpr int NW = 2 * S + K, RW = NW + 4;  // state, parent ref, footprint
    const u64 total = per_dest * B.world;  // window [i0, i0 + per_dest) of every destination's keys
    for (u64 t = (u64)blockIdx.x * 256ull + threadIdx.x; t < total; t += (u64)gridDim.x * 256ull) {
        const u32 d = (u32)(t / per_dest);
        const u64 i = i0 + (t - (u64)d * per_dest);
        const u64 sent = B.ocount[d] < B.kcap ? B.ocount[d] : B.kcap;  // beyond kcap: parked, not sent
        if (d == B.rank || i >= sent) continue;
        const bool seen = !reply[(u64)d * B.kcap + i];
        if (seen && !B.sidx) continue;
        const u64 tick = B.tick_out[(u64)d * B.kcap + i];
        const u64 pidx = tick & ((1ull << 48) - 1);
        const int lane = (int)(tick >> 56);
        const u64 slot = atomicAdd((unsigned long long*)&B.scount[d], 1ull);
        if (slot >= B.scap) {
            atomicOr(&B.ctr->overflow, 2u);
            continue;
        }
        if (tick & POOL_TICK) {  // a pool record is already the phase-2 record (never REF_SEEN: no verification)
            const uint2* src = reinterpret_cast<const uint2*>(B.pool + pidx * (u64)RW);
            uint2* dst = reinterpret_cast<uint2*>(B.st_out + ((u64)d * B.scap + slot) * (u64)RW);
#pragma unroll
            for (int q = 0; q < RW / 2; ++q) dst[q] = src[q];
            continue;
        }
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + pidx * (u64)NW, w, m);
        Delta dl;
        lane_delta<S, K>(w, m, lane, P, dl);
        u64 wo[S];
        u32 mo[K];
        materialise<S, K>(w, m, dl, wo, mo);
        u32* r = B.st_out + ((u64)d * B.scap + slot) * (u64)RW;
        store_state<S, K>(r, wo, mo);
        const u64 ref = B.ref_tag | ((u64)lane << 40) | pidx | (seen ? REF_SEEN : 0ull);
        r[NW] = (u32)ref;
        r[NW + 1] = (u32)(ref >> 32);
        const u64 ft = make_foot<S, K>(m, lane, dl, P);
        r[NW + 2] = (u32)ft;
        r[NW + 3] = (u32)(ft >> 32);
    }
}

// Sharded mode, phase 2, owner side: store the n accepted states received (their
// keys are already in this rank's set since phase 1): one allocation atomic per
// wave, parent ref and lane from the record, fused invariants.
template <int S, int K>
__global__ __launch_bounds__(256) void k_store_remote(const Params P, const DevBufs B, const u32* inbox, u64 n) {
    constexpr int NW = 2 * S + K, RW = NW + 4;  // state, parent ref, footprint
    for (u64 t0 = (u64)blockIdx.x * 256ull; t0 < n; t0 += (u64)gridDim.x * 256ull) {
        const u64 t = t0 + threadIdx.x;
        // verification mode also receives the states the owner had seen (compared by k_compare_remote)
        const bool live = t < n && !(inbox[t * (u64)RW + NW + 1] & (u32)(REF_SEEN >> 32));
        const u64 ni = wave_reserve(live, (unsigned long long*)&B.ctr->count);
        if (!live) continue;
        if (ni >= B.cap) {
            atomicOr(&B.ctr->overflow, 1u);
            continue;
        }
        const u32* r = inbox + t * (u64)RW;
        u64 w[S];
        u32 m[K];
        load_state<S, K>(r, w, m);
        const u64 ref = (u64)r[NW] | ((u64)r[NW + 1] << 32);
        store_new<S, K>(P, B, ni, w, m, ref & ~((0xFFull << 40) | REF_SEEN), (int)((ref >> 40) & 0xFFu),
                        (u64)r[NW + 2] | ((u64)r[NW + 3] << 32));
    }
}

// Sharded full-state verification, owner side: every received record the
// owner had already seen (REF_SEEN) is compared with the stored state that
// owns its fingerprint's slot (published by k_publish before this runs); a
// difference is a fingerprint collision.
template <int S, int K, bool SYM>
__global__ __launch_bounds__(256) void k_compare_remote(const Params P, const PermTable PT, const DevBufs B,
                                                        const u32* inbox, u64 n) {
    constexpr int NW = 2 * S + K, RW = NW + 4;
    u64 vchk = 0, vcol = 0;
    for (u64 t = (u64)blockIdx.x * 256ull + threadIdx.x; t < n; t += (u64)gridDim.x * 256ull) {
        const u32* r = inbox + t * (u64)RW;
        if (!(r[NW + 1] & (u32)(REF_SEEN >> 32))) continue;
        PackedState<S, K> o;
        load_state<S, K>(r, o.w, o.m);
        const TKey key = verify_key<S, K, SYM>(o.w, o.m, P, PT, B.tmask);
        u64 s = key.s0, k = 0;
        while (B.table[s] != key.v && k <= B.tmask) { s = (s + 1) & B.tmask; ++k; }
        const u64 ix = k > B.tmask ? ~0ull : B.sidx[s];
        if (ix == ~0ull) {
            atomicOr(&B.ctr->overflow, 8u);  // a seen key without a published owner
            continue;
        }
        ++vchk;
        bool same;
        if constexpr (SYM) same = same_orbit<S, K>(o, B.store + ix * (u64)NW, PT);
        else same = same_state<S, K>(o.w, o.m, B.store + ix * (u64)NW);
        vcol += same ? 0u : 1u;
    }
    vchk = wave_sum64(vchk);
    vcol = wave_sum64(vcol);
    if (__lane_id() == 0 && vchk) atomicAdd((unsigned long long*)&B.ctr->vchecked, (unsigned long long)vchk);
    if (__lane_id() == 0 && vcol) atomicAdd((unsigned long long*)&B.ctr->collisions, (unsigned long long)vcol);
}

// SYMMETRY, single GPU: the successors k_expand_sym deferred because their
// server signatures tie.  Each is re-derived from its parent, canonicalised
// over every order of the tied servers, inserted, and committed if new.
template <int S, int K>
__global__ __launch_bounds__(256) void k_ties(const Params P, const PermTable PT, const DevBufs B) {
    constexpr int NW = 2 * S + K;
    const u64 n = B.ctr->nties < B.tie_cap ? B.ctr->nties : B.tie_cap;
    u64 pr = 0;
    for (u64 t0 = (u64)blockIdx.x * 256ull; t0 < n; t0 += (u64)gridDim.x * 256ull) {  // wave-uniform
        const u64 t = t0 + threadIdx.x;
        const bool live = t < n;
        u64 w[S];
        u32 m[K];
        u64 pidx = 0;
        int lane = 0;
        Delta d;
        int is_new = 0;
        if (live) {
            const u64 rec = B.ties[t];
            pidx = rec & ((1ull << 56) - 1);
            lane = (int)(rec >> 56);
            load_state<S, K>(B.store + wslot(B, pidx) * (u64)NW, w, m);
            lane_delta<S, K>(w, m, lane, P, d);
            u64 base[S];
#pragma unroll
            for (int i = 0; i < S; ++i) base[i] = sig_base<S>(w[i], (u32)i);
            is_new = fp_insert_fp(B.table, B.tmask, canon_delta<S, K>(w, m, base, d, PT.code, PT.np),
                                  &B.ctr->table_full);
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i) w[i] = 0;
#pragma unroll
            for (int q = 0; q < K; ++q) m[q] = 0;
            d.srv = -1; d.rm = -1; d.has_add = 0; d.add = 0; d.en = 0; d.w_new = 0;
        }
        pr += (u64)__popcll(__ballot(live));
        commit_new<S, K>(is_new, w, m, d, P, B, B.ref_tag | pidx, lane);
    }
    if (__lane_id() == 0 && pr) atomicAdd((unsigned long long*)&B.ctr->probes, (unsigned long long)pr);
}

}  // namespace rmc
