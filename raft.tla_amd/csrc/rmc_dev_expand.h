// rmc_dev_expand.h — the expansion kernels of the raft.tla BFS (DESIGN.md "Kernels").
//
//  k_expand : one lane per frontier state; loops over the state's action lanes
//             (Next raft.tla:421-430) in wave-uniform order, computes each
//             successor as a delta + incremental fingerprint, filters the
//             CONSTRAINT and stuttering successors, probes/CAS-inserts the
//             fingerprint into the HBM open-addressing set, and for the lanes
//             that won: wave-aggregated slot allocation, materialise, store,
//             parent pointer, fused invariant check.  Replaces TLC's worker
//             loop body (getNextStates + FPSet.put + invariant check).
//
// expand_body is the one body; the named configs below (ExpandEveryLane, ExpandSort,
// ExpandSym, ExpandDist) and their __global__ wrappers are the kernels built from it.
#pragma once
#include <hip/hip_runtime.h>

#include "raft_packed.h"
#include "rmc_dev_set.h"
#include "rmc_dev_sharded.h"
#include "rmc_dev_state.h"
#include "rmc_dev_verify.h"
#include "rmc_internal.h"
#include "rmc_units.h"

namespace rmc {

// Grid-stride over 256-state tiles of the frontier [lo, hi).  Lanes are
// processed BATCH at a time so BATCH fingerprint probes per thread are in
// flight together (the kernel is bound by probe latency, not bandwidth).
// SORT: the lane-superset walk — each block takes windows of WTILES tiles and
//   walks their states in class order (a counting sort in LDS over the 1-byte
//   classes B.cls), so its waves hold states of one kind and walk only the
//   lanes some state of the wave can enable (lane_superset, a scalar).
// DIST: sharded mode — successors owned by another rank go to that owner's
//   key outbox: with MARK (the default) after a CAS into the local set (send
//   markers: a lossless sent-cache), else through the lossy sent-cache B.sent
//   (SYMMETRY and verification).
// DIA: commuting-diamond successors are not probed (raft_packed.h "commuting
//   diamonds"; P.diamond = 0 turns it off at run time).
// PIPE: a probe's load is issued as soon as its key is known, so the loads
//   overlap the lane code of the batch's later lanes (266-272 vs 271-279 ms
//   per bench BFS, profiles/r03/ab/probe_issue_r03pipe*.jsonl).
// REP: a replicated level of the sharded search — [lo, hi) indexes the whole
//   level's records in B.rep (gathered from every rank); every rank expands
//   all of them and probes, stores and counts only the successors it owns.
// POOL: the sharded kernel whose flush pools the remote successors (flush_pool).
// POOL and REP are the send-marker kernels (MARK); a DIST kernel that is neither
// goes through the lossy sent-cache (SENTC, flush_dist).
//
// The configuration of one expansion kernel, read by name in expand_body; each
// kernel below states what it changes next to its definition.
struct ExpandDefaults {
    static constexpr bool SYM = false;      // SYMMETRY: canonical fingerprints, ties deferred to k_ties
    static constexpr int BATCH = 8;         // probes in flight per thread
    static constexpr bool DIST = false;     // sharded mode
    static constexpr bool VERIFY = false;   // full-state verification of fingerprint hits
    static constexpr bool PRE = false;      // the parent's mixes computed once per state (parent_mix)
    static constexpr bool SORT = false;     // the lane-superset walk over class-sorted windows
    static constexpr bool DIA = false;      // commuting-diamond skipping
    static constexpr int WTILES = 8;        // tiles per window (SORT)
    static constexpr int PIPE = 0;          // probe loads issued during the lane code
    static constexpr bool REP = false;      // a replicated level (B.rep)
    static constexpr bool PRESORT = false;  // windows sorted before the launch (k_window_order, B.word)
    static constexpr int DYN = 0;           // dynamic per-wave work units
    static constexpr int UNIT_TILES = 16;   // DYN: tiles per unit (rmc_units.h; 16: a wave's quarter of a whole window)
    static constexpr bool POOL = false;     // the pool flush
};

// The materialising flush of a wave's list, by the kernel's configuration.
template <int S, int K, class C>
__device__ __forceinline__ void flush_list(const Params& P, const DevBufs& B, u64 lo, const u32* l_rel,
                                           const uint8_t* l_lane, uint8_t* l_dest, const u64* l_key, const u32* l_ks,
                                           u32 n) {
    if constexpr (C::REP) flush_new<S, K, true>(P, B, lo, l_rel, l_lane, n);
    else if constexpr (C::POOL) flush_pool<S, K>(P, B, lo, l_rel, l_lane, l_dest, n);
    else if constexpr (C::DIST) flush_dist<S, K>(P, B, lo, l_rel, l_lane, l_dest, l_key, l_ks, n);
    else flush_new<S, K, false, C::DYN != 0>(P, B, lo, l_rel, l_lane, n);  // dynamic units: admission
}

template <int S, int K, class C>
__device__ __forceinline__ void expand_body(const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi) {
    constexpr bool SYM = C::SYM, DIST = C::DIST, VERIFY = C::VERIFY, PRE = C::PRE, SORT = C::SORT, DIA = C::DIA,
                   REP = C::REP, PRESORT = C::PRESORT, POOL = C::POOL;
    constexpr int BATCH = C::BATCH, WTILES = C::WTILES, PIPE = C::PIPE, DYN = C::DYN, UT = C::UNIT_TILES;
    constexpr bool MARK = POOL || REP;  // send markers in the local set
    static_assert(!MARK || (DIST && !VERIFY && !SYM), "send markers: the plain sharded kernel only");
    static_assert(!POOL || !REP, "the pool flush: not on a replicated level");
    constexpr bool SENTC = DIST && !MARK;  // the lossy sent-cache + (key, dest) list entries
    static_assert(!SENTC || !PRE, "the sent-cache kernels: every lane, no parent mixes");
    static_assert(!DIA || (!SYM && !VERIFY && SORT), "diamond skipping: the sorted plain kernels");
    static_assert(!SORT || !VERIFY, "SORT: not with verification");
    static_assert(!SORT || BATCH * 7 <= 64, "SORT packs a batch's lanes 7 bits each into one u64");
    static_assert(PIPE == 0 || (!SYM && !VERIFY && !SENTC), "PIPE: the plain and marker kernels");
    static_assert(!REP || (SORT && PRE), "replicated levels: the plain sharded kernel");
    // PRESORT: the windows were counting-sorted by class before the launch
    // (k_window_order writes each window's positions in class order to B.word),
    // so the kernel carries no sort: no LDS bins, scan or block barriers
    static_assert(!PRESORT || (SORT && !REP), "presorted windows: the sorted kernels");
    constexpr bool INSORT = SORT && !PRESORT;
    // DYN: each wave takes its next unit of work — one wave's quarter of a
    // tile group of a presorted window (its 64 lanes of UT tiles; rmc_units.h)
    // — from a launch-wide counter, instead of the block's fixed share of
    // windows: the waves end together however unequal the units' costs and
    // whatever the window count, and the launch drains over one unit's time,
    // which is why the unit is shorter than a window
    static_assert(DYN == 0 || PRESORT, "dynamic units: presorted windows");
    static_assert(UT >= 1 && UT <= 16 && (UT & (UT - 1)) == 0, "unit tiles: a power of two, at most 16");
    // (the marker kernel measured no gain from PIPE at one rank: 308.7-309.7 vs 307.4-308.7 ms)
    constexpr int NW = 2 * S + K;
    typedef RepRec<S, K> RR;
    constexpr int FW = REP ? RR::RR : NW;  // words per frontier record
    const u32* const fr = REP ? B.rep : B.store;
    constexpr bool TIEDEFER = SYM && !DIST && !VERIFY;
    constexpr bool LISTOWN = SENTC;  // list entries carry their owner (MARK: found at flush time)
    constexpr int WT = SORT ? WTILES : 1;   // tiles per window
    __shared__ uint16_t s_ord[INSORT ? 256 * WT : 1];  // window positions in class order
    __shared__ uint8_t s_wcls[INSORT ? 256 * WT : 1];  // class of each window position
    constexpr int NBIN = 256;                           // roles x message-count classes
    __shared__ u32 s_wbin[INSORT ? NBIN : 1];           // class counters / cursors
    // Sharded mode keeps per-probe owners in LDS too; a shorter list keeps the
    // block under 160 KB / 6 so it runs at the same 6 waves/SIMD as the
    // single-GPU kernel (VGPR-bound there).
    constexpr int LCAP = SENTC ? 256 : MARK ? WCAP - 64 : WCAP;  // MARK: the owner byte per entry
    __shared__ u32 s_rel[4][LCAP];
    __shared__ uint8_t s_lane[4][LCAP];
    constexpr bool LDEST = SENTC || MARK;
    __shared__ uint8_t s_dest[LDEST ? 4 : 1][LDEST ? LCAP : 1];  // owner per listed successor
    __shared__ u64 s_lkey[SENTC ? 4 : 1][SENTC ? LCAP : 1];  // sharded: the key of each listed successor
    __shared__ u32 s_lks[SENTC ? 4 : 1][SENTC ? LCAP : 1];   // ... and its s32 (fp_norm)
    __shared__ u64 s_key[BATCH][256];  // per lane of the batch: the probe's table value (0 = no probe)
    __shared__ u32 s_ks[BATCH][256];   // ... and its s32, which recovers its slot (fp_slot)
    __shared__ uint8_t s_own[LISTOWN ? BATCH : 1][LISTOWN ? 256 : 1];  // owner rank per probe
    const int wv = (int)(threadIdx.x >> 6);
    const int me = (int)__lane_id();
    const u64 lt_mask = (1ull << me) - 1ull;
    u32* l_rel = s_rel[wv];
    uint8_t* l_lane = s_lane[wv];
    uint8_t* l_dest = s_dest[LDEST ? wv : 0];
    u64* l_key = s_lkey[SENTC ? wv : 0];
    u32* l_ks = s_lks[SENTC ? wv : 0];
    u32 n = 0;  // wave-uniform list length
    u32 gen = 0;  // generated lanes of this thread's states (< 2^32 per launch)
    u64 vchk = 0, vcol = 0;  // verification: hits compared, collisions
    u64 pr = 0;  // probes issued by the whole wave (wave-uniform)
    u32 walked = 0;  // (live state, lane) slots this thread's waves visited for it
    const u64 nf = hi - lo;
    const int nl = P.off[10];  // == Lanes<S,K>::N; runtime on purpose (see lane_delta)
    // tiles per window, fewer when the launch has too few states to give every
    // block a full window (small levels would idle most blocks)
    u64 wt = WT;
    if constexpr (SORT) {
        const u64 per_block = (nf + (u64)gridDim.x * 256ull - 1) / ((u64)gridDim.x * 256ull);
        wt = per_block < (u64)WT ? (per_block ? per_block : 1ull) : (u64)WT;
    }
    u32 q64 = (u32)threadIdx.x & ~63u;  // this thread's window slot base (DYN: the unit's)
    constexpr bool GROUPS = DYN != 0 && UT < WT;  // units of part of a window's tiles
    // GROUPS: the unit's first tile as a quarter tile of the window (tile * 4 +
    // quarter, a step of 4 per tile: the quarter rides in the loop counter, not
    // in q64) and the tile after its last; the walk's bound is wn cut to that
    // tile, so the unit adds no scalar held over the walk
    int wk0 = 0;
    u32 tile1 = 0;
    u64 win = DYN ? 0ull : (u64)blockIdx.x * 256ull * wt;
    for (;; win += (u64)gridDim.x * 256ull * wt) {  // block-uniform (DYN: wave-uniform)
    if constexpr (DYN != 0) {
        // admission (rmc_plan.h): a flush that takes the count within B.admit_reserve of
        // B.lim raises rmc_units::kStopBit in the work counter (flush_new), and a claim that
        // returns it names no unit (it decodes to win >= nf below), so the wave leaves as at the launch's
        // end; a claimed unit is always finished.  The wave takes its count back — the low
        // half stays the units claimed, the high half counts the waves that left — so the
        // host re-launches from exactly there.  Nothing is read on the claim path: a
        // device-scope load of the count before every claim measured +43 % on MCraftBench
        // (profiles/r16/level_launch/claim_variants.txt)
        u32 unit = 0;
        if (me == 0) {
            unit = (u32)atomicAdd((unsigned long long*)&B.ctr->wnext, 1ull);
            if (unit & rmc_units::kStopBit) atomicAdd((unsigned long long*)&B.ctr->wnext, 0xFFFFFFFFull);
        }
        if constexpr (GROUPS) {
            // decoded by lane 0 before the broadcast: the division's temporaries are
            // vector registers, free between two units, not scalars held over the walk
            const rmc_units::Unit un =
                rmc_units::unit_decode(unit, (u32)wt, (u32)UT, rmc_units::unit_groups((u32)wt, (u32)UT));
            win = bcast64(un.win, 0);
            const u32 pk = (u32)__builtin_amdgcn_readlane(
                (int)(un.quarter | (un.tile0 << 2) | ((un.tile0 + un.ntiles) << 8)), 0);
            wk0 = (int)(pk & 255u);
            tile1 = pk >> 8;
        } else {
            unit = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)unit, 0));
            const rmc_units::Unit un = rmc_units::unit_decode(unit, (u32)wt, (u32)UT, 1u);
            win = un.win;
            q64 = un.quarter * 64u;
        }
    }
    if (win >= nf) break;
    u32 wn = 0;  // SORT: states in this window
    if constexpr (SORT) wn = (u32)((nf - win) < 256ull * wt ? (nf - win) : 256ull * wt);
    if constexpr (GROUPS) wn = wn < tile1 * 256u ? wn : tile1 * 256u;  // ... up to the unit's last tile
    if constexpr (INSORT) {
        __syncthreads();  // the previous window's s_ord is consumed
        if (threadIdx.x < NBIN) s_wbin[threadIdx.x] = 0;
        __syncthreads();
        for (int k = 0; k < (int)wt; ++k) {
            const u32 p = (u32)k * 256u + threadIdx.x;
            if (p < wn) {
                // the stored 1-byte class (B.cls / the record's class byte), not the state
                const u32 c = REP ? (fr[(lo + win + p) * (u64)FW + RR::ACT] >> 8) & 0xFFu
                                  : (u32)B.cls[wslot(B, lo + win + p)];
                s_wcls[p] = (uint8_t)c;
                atomicAdd(&s_wbin[c], 1u);
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {  // exclusive scan of the counters (wave 0; NBIN / 64 per lane)
            constexpr int PER = NBIN / 64;
            u32 v[PER], tot = 0;
#pragma unroll
            for (int q = 0; q < PER; ++q) { v[q] = s_wbin[threadIdx.x * PER + q]; tot += v[q]; }
            u32 incl = tot;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const u32 t = (u32)__shfl_up((int)incl, off);
                if ((int)threadIdx.x >= off) incl += t;
            }
            u32 ex = incl - tot;
#pragma unroll
            for (int q = 0; q < PER; ++q) { s_wbin[threadIdx.x * PER + q] = ex; ex += v[q]; }
        }
        __syncthreads();
        for (int k = 0; k < (int)wt; ++k) {
            const u32 p = (u32)k * 256u + threadIdx.x;
            if (p < wn) s_ord[atomicAdd(&s_wbin[s_wcls[p]], 1u)] = (uint16_t)p;
        }
        __syncthreads();
    }
    for (int wk = GROUPS ? wk0 : 0; GROUPS ? ((u32)wk & ~3u) * 64u < wn : wk < (int)wt; wk += GROUPS ? 4 : 1) {
        u64 rel;
        bool live;
        if constexpr (SORT) {
            const u32 p = GROUPS ? (u32)wk * 64u + (u32)me : (u32)wk * 256u + q64 + (u32)me;
            live = p < wn;
            if constexpr (PRESORT) rel = win + (live ? (u32)B.word[win + p] : 0u);
            else rel = win + (live ? s_ord[p] : 0u);
        } else {
            rel = win + threadIdx.x;
            live = rel < nf;
        }
        u64 w[S];
        u32 m[K];
        const u32* rec = fr + (REP ? lo + rel : wslot(B, lo + rel)) * (u64)FW;
        if (live) {
            load_state<S, K>(rec, w, m);
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i) w[i] = 0;
#pragma unroll
            for (int q = 0; q < K; ++q) m[q] = 0;
        }
        // REP: the record's rank; only this rank's own states count as generated
        // (every rank expands every state) and as deadlocks
        u32 powner = B.rank;
        bool mine = true;
        if constexpr (REP) {
            powner = live ? (rec[RR::REF + 1] >> 16) & 0xFFu : B.rank;
            mine = powner == B.rank;
        }
        ParentMix<S, K> pmx;
        Fp h0;
        if constexpr (PRE) {
            parent_mix<S, K>(w, m, pmx);
            h0 = pmx.h0;
        } else {
            h0 = state_fp<S, K>(w, m);
        }
        // SYMMETRY: the parent's signature bases (reused by every lane)
        u64 sbase[SYM ? S : 1];
        if constexpr (SYM) {
#pragma unroll
            for (int i = 0; i < S; ++i) sbase[i] = sig_base<S>(w[i], (u32)i);
        }
        Diamond dm;  // DIA: how this state was discovered (lane + footprint), once per state
        if constexpr (DIA) {
            const bool on = live && P.diamond;
            int act = 255;
            u64 foot = 0;
            if (on) {
                if constexpr (REP) {
                    act = (int)(rec[RR::ACT] & 0xFFu);
                    foot = (u64)rec[RR::FOOT] | ((u64)rec[RR::FOOT + 1] << 32);
                } else {
                    act = (int)B.act[lo + rel];
                    foot = B.foot[wslot(B, lo + rel)];
                }
            }
            diamond_of<S, K>(m, act, foot, P, dm);
        }
        u32 g = 0;
        // SORT: the lanes some state of this wave can enable (wave-uniform, scalar;
        // wm_hi: lanes 64-127, shapes of more than 64 lanes only)
        constexpr bool WIDE_MASK = Lanes<S, K>::N > 64;
        u64 wm = 0, wm_hi = 0;
        if constexpr (SORT) {
            const LaneMask lm = lane_superset_wave<S, K>(w, m, P.V, live);
            wm = lm.lo;
            if constexpr (WIDE_MASK) wm_hi = lm.hi;
        }
#ifdef RMC_WALK_STATS_BUILD
        walked += live ? (u32)(SORT ? __popcll(wm) + __popcll(wm_hi) : nl) : 0u;  // per thread (a VGPR)
#endif
        for (int lane0 = 0; SORT ? ((wm | wm_hi) != 0) : (lane0 < nl); lane0 += BATCH) {  // wave-uniform (pr: probes)
            u64 lp = 0;  // SORT: this batch's lanes, 7 bits each (127 = none), a scalar
            if constexpr (SORT) {
#pragma unroll
                for (int b = 0; b < BATCH; ++b) {
                    u64 ln;
                    if constexpr (WIDE_MASK) {
                        ln = wm ? (u64)__builtin_ctzll(wm) : wm_hi ? 64ull + (u64)__builtin_ctzll(wm_hi) : 127ull;
                        if (wm) wm &= wm - 1;
                        else wm_hi &= wm_hi - 1;
                    } else {
                        ln = wm ? (u64)__builtin_ctzll(wm) : 127ull;
                        wm &= wm - 1;
                    }
                    lp |= ln << (7 * b);
                }
            }
            u64 cur_p[PIPE ? BATCH : 1];  // PIPE: the probes issued during (a)
            // (a) deltas + fingerprints of BATCH lanes; keys parked in LDS (0 = no probe).
            // Rolled under SYMMETRY: one copy of the canonicalisation in flight.
            // (Rolling the plain kernel too, one copy of the lane code instead of
            // 8, measured no difference: instruction-cache misses are ~1e-5.)
#ifndef RMC_LANE_UNROLL
#define RMC_LANE_UNROLL BATCH
#endif
            constexpr int UNROLL = SYM ? 1 : RMC_LANE_UNROLL;
#pragma unroll UNROLL
            for (int b = 0; b < BATCH; ++b) {
                const int lane = SORT ? (int)((lp >> (7 * b)) & 127u) : lane0 + b;
                u64 key = 0, slot0 = 0;  // the probe's table value (0: none) and first slot
                u32 ks = 0;
                int tied = 0;  // SYMMETRY: signatures tie, deferred to k_ties
                if (lane < nl) {
                    Delta d;
                    if constexpr (SORT) lane_delta_desc<S, K>(w, m, P.ldesc[SORT ? lane : 0], P, d);  // scalar descriptor
                    else lane_delta<S, K>(w, m, lane, P, d);
                    const int en = d.en && live;
                    g += (u32)(en && mine);
                    Fp h{0, 0};
                    u64 hwn = 0;  // REP: the mix of the changed server word (owner routing)
                    int in_model = 0;
                    if constexpr (SYM) {
                        // a stutter (successor = parent: no bag change, no word change) is never probed
                        const bool stutter = d.rm < 0 && !d.has_add && (d.srv < 0 || d.w_new == selw<S>(w, d.srv));
                        if (en && !stutter && delta_in_model<S, K>(m, d, P)) {
                            in_model = 1;
                            if constexpr (TIEDEFER) {  // tied signatures: k_ties canonicalises it after this launch
                                h = canon_delta<S, K, true>(w, m, sbase, d, PT.code, PT.np, &tied);
                                if (tied) in_model = 0;
                            } else {
                                h = canon_delta<S, K>(w, m, sbase, d, PT.code, PT.np);
                            }
                        }
                    } else if (en) {
                        int nmb = 0;
                        if constexpr (PRE)
                            in_model = delta_fp_pre<S, K>(w, m, pmx, d, P, &h, DIA ? &nmb : nullptr,
                                                          REP ? &hwn : nullptr);
                        else in_model = delta_fp<S, K>(w, m, h0, d, P, &h, DIA ? &nmb : nullptr);
                        if constexpr (DIA)
                            if (in_model && h.k != h0.k && diamond_skip_desc<S, K>(m, lane, P.ldesc[lane], d, nmb, dm))
                                in_model = 0;
                    }
                    if (in_model && (SYM || h.k != h0.k)) {  // (a stutter has the parent's k)
                        if constexpr (VERIFY) h = fp_weaken(h, P.fp_mask);
                        ks = fp_norm(h.k, (u32)h.s, B.tmask);
                        key = fp_v(h.k, ks, B.tmask);
                        slot0 = h.k & B.tmask;
                        if constexpr (REP) {  // a replicated level: only the owner probes
                            if (owner_succ<S, K>(h.k, d, pmx, hwn, B, powner) != B.rank) key = 0;
                        } else if constexpr (SENTC) {
                            // no parent mixes: the successor's hashed words when it changes one
                            s_own[b][threadIdx.x] = (uint8_t)(
                                B.world == 1 ? 0u
                                : B.owner_mode == 0 ? owner_of(h.k, B.world)
                                : owner_succ_w<S>(h.k, d, w, B));
                        }
                    }
                }
                s_key[b][threadIdx.x] = key;
                s_ks[b][threadIdx.x] = ks;
                if constexpr (PIPE != 0) cur_p[b] = key ? B.table[slot0] : 0ull;
                if constexpr (TIEDEFER) {  // one queue atomic per wave and lane, not per tied successor
                    const u64 bal = __ballot(tied);
                    if (bal) {
                        const int leader = __ffsll((long long)bal) - 1;
                        u64 q0 = 0;
                        if (me == leader) q0 = atomicAdd((unsigned long long*)&B.ctr->nties, (unsigned long long)__popcll(bal));
                        q0 = bcast64(q0, leader);
                        if (tied) {
                            const u64 q = q0 + (u64)__popcll(bal & lt_mask);
                            if (q < B.tie_cap) B.ties[q] = (lo + rel) | ((u64)lane << 56);
                            else atomicOr(&B.ctr->overflow, 16u);
                        }
                    }
                }
            }
            // (b) BATCH independent first-slot probes in flight at once
            u64 key[BATCH], cur[BATCH];
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                key[b] = s_key[b][threadIdx.x];
                if constexpr (SENTC) {
                    const bool remote = key[b] && s_own[b][threadIdx.x] != B.rank;
                    // no sent-cache in verification mode (B.sent null): every remote successor is shipped
                    cur[b] = !key[b] ? 0ull
                           : remote ? (B.sent ? B.sent[(key[b] >> 8) & B.smask] : 0ull)
                                    : B.table[fp_slot(key[b], s_ks[b][threadIdx.x], B.tmask)];
                } else if constexpr (PIPE != 0) {
                    cur[b] = cur_p[PIPE ? b : 0];
                } else {
                    cur[b] = key[b] ? B.table[fp_slot(key[b], s_ks[b][threadIdx.x], B.tmask)] : 0ull;
                }
            }
#pragma unroll
            for (int b = 0; b < BATCH; ++b) pr += (u64)__popcll(__ballot(key[b] != 0));  // wave-uniform
            // (c) resolve: hit -> duplicate; empty -> CAS; mismatch -> slow path
            u32 newbits = 0, slowbits = 0;
            u32 hitbits = 0;  // verification: probes that found their key (slot parked in s_key)
#pragma unroll
            for (int b = 0; b < BATCH; ++b) {
                if (!key[b]) continue;
                if (cur[b] == key[b]) {
                    if constexpr (VERIFY) {
                        hitbits |= 1u << b;
                        s_key[b][threadIdx.x] = fp_slot(key[b], s_ks[b][threadIdx.x], B.tmask);  // the key's slot
                    }
                    continue;
                }
                if constexpr (SENTC) {
                    if (s_own[b][threadIdx.x] != B.rank) {  // not sent before (lossy cache): ship it
                        if (B.sent) B.sent[(key[b] >> 8) & B.smask] = key[b];
                        newbits |= 1u << b;
                        continue;
                    }
                }
                if (fp_empty(cur[b])) {  // 0, or another epoch's entry: CAS it away
                    const u64 sl0 = fp_slot(key[b], s_ks[b][threadIdx.x], B.tmask);
                    const u64 prev = atomicCAS((unsigned long long*)&B.table[sl0], (unsigned long long)cur[b],
                                               (unsigned long long)key[b]);
                    if (prev == cur[b]) newbits |= 1u << b;
                    else if (prev != key[b]) slowbits |= 1u << b;
                    else if constexpr (VERIFY) {
                        hitbits |= 1u << b;
                        s_key[b][threadIdx.x] = sl0;
                    }
                } else {
                    slowbits |= 1u << b;
                }
            }
            while (slowbits) {  // rare: linear probing past an occupied first slot
                const int b = __builtin_ctz(slowbits);
                slowbits &= slowbits - 1;
                const u64 kv = s_key[b][threadIdx.x], sl0 = fp_slot(kv, s_ks[b][threadIdx.x], B.tmask);
                if constexpr (VERIFY) {
                    u64 at = 0;
                    if (fp_insert_at(B.table, B.tmask, sl0, kv, &B.ctr->table_full, &at)) {
                        newbits |= 1u << b;
                    } else {
                        hitbits |= 1u << b;
                        s_key[b][threadIdx.x] = at;  // the slot that holds the key
                    }
                } else if (fp_insert(B.table, B.tmask, sl0, kv, &B.ctr->table_full)) {
                    newbits |= 1u << b;
                }
            }
            if constexpr (VERIFY) {
                // compare each hit with the stored owner of its slot (parked in s_key)
                u32 defbits = 0, hostbits = 0;
                for (int b = 0; b < BATCH; ++b) {  // rolled: one inlined copy of the check
                    if (!((hitbits >> b) & 1u)) continue;
                    const int r = verify_hit<S, K, SYM>(w, m, lane0 + b, s_key[b][threadIdx.x], P, PT, B);
                    vchk += (u64)(r <= 1);
                    vcol += (u64)(r == 1);
                    defbits |= (u32)(r == 2) << b;
                    hostbits |= (u32)(r == 4) << b;
                }
                // owners that left the device window (spill): checked on their host
                // copies after the launch (k_verify_host)
                for (int b = 0; b < BATCH; ++b) {
                    const bool hd = (hostbits >> b) & 1u;
                    const u64 bal = __ballot(hd);
                    if (!bal) continue;
                    const int leader = __ffsll((long long)bal) - 1;
                    u64 q0 = 0;
                    if (me == leader) q0 = atomicAdd((unsigned long long*)&B.ctr->hcount, (unsigned long long)__popcll(bal));
                    q0 = bcast64(q0, leader);
                    if (hd) {
                        const u64 q = q0 + (u64)__popcll(bal & lt_mask);
                        if (q < B.hcap) {
                            B.hbuf[2 * q] = lo + rel;
                            B.hbuf[2 * q + 1] = B.sidx[s_key[b][threadIdx.x]] | ((u64)(lane0 + b) << 56);
                        } else {
                            atomicOr(&B.ctr->overflow, 4u);
                        }
                    }
                }
                // defer hits on owners not yet published (one atomic per wave and probe batch)
                for (int b = 0; b < BATCH; ++b) {
                    const bool def = (defbits >> b) & 1u;
                    const u64 bal = __ballot(def);
                    if (!bal) continue;
                    const int leader = __ffsll((long long)bal) - 1;
                    u64 q0 = 0;
                    if (me == leader) q0 = atomicAdd((unsigned long long*)&B.ctr->vcount, (unsigned long long)__popcll(bal));
                    q0 = bcast64(q0, leader);
                    if (def) {
                        const u64 q = q0 + (u64)__popcll(bal & lt_mask);
                        if (q < B.vcap) {
                            B.vbuf[2 * q] = lo + rel;
                            B.vbuf[2 * q + 1] = s_key[b][threadIdx.x] | ((u64)(lane0 + b) << 56);
                        } else {
                            atomicOr(&B.ctr->overflow, 4u);
                        }
                    }
                }
            }
            // (d) list the winners (wave-aggregated, no global atomics)
            for (int b = 0; b < BATCH; ++b) {
                const int is_new = (newbits >> b) & 1u;
                const u64 bal = __ballot(is_new);
                if (bal) {
                    if (is_new) {
                        const u32 pos = n + (u32)__popcll(bal & lt_mask);
                        l_rel[pos] = (u32)rel;
                        l_lane[pos] = (uint8_t)(SORT ? (int)((lp >> (7 * b)) & 127u) : lane0 + b);
                        if constexpr (SENTC) {
                            l_dest[pos] = s_own[b][threadIdx.x];
                            l_key[pos] = key[b];
                            l_ks[pos] = s_ks[b][threadIdx.x];
                        }
                    }
                    n += (u32)__popcll(bal);
                    if (n > (u32)(LCAP - 64)) {
                        flush_list<S, K, C>(P, B, lo, l_rel, l_lane, l_dest, l_key, l_ks, n);
                        n = 0;
                    }
                }
            }
        }
        if (live && mine && g == 0) {  // deadlock: the state's index on its own rank
            const u64 ix = REP ? (((u64)rec[RR::REF] | ((u64)rec[RR::REF + 1] << 32)) & ((1ull << 48) - 1)) : lo + rel;
            atomicMin((unsigned long long*)&B.ctr->deadlock, (unsigned long long)ix);
        }
        gen += g;
    }
    }
    if (n) flush_list<S, K, C>(P, B, lo, l_rel, l_lane, l_dest, l_key, l_ks, n);
    // wave reductions of the generated and probe counts, one atomic each per wave
    u64 gs = (u64)gen;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        gs += (u64)(u32)__shfl_xor((int)(u32)gs, off) | ((u64)(u32)__shfl_xor((int)(u32)(gs >> 32), off) << 32);
    if (me == 0 && gs) atomicAdd((unsigned long long*)&B.ctr->generated, (unsigned long long)gs);
    if (me == 0 && pr) atomicAdd((unsigned long long*)&B.ctr->probes, (unsigned long long)pr);
    const u64 wk_sum = wave_sum64((u64)walked);
    if (me == 0 && wk_sum) atomicAdd((unsigned long long*)&B.ctr->walked, (unsigned long long)wk_sum);
    if constexpr (VERIFY) {
        vchk = wave_sum64(vchk);
        vcol = wave_sum64(vcol);
        if (me == 0 && vchk) atomicAdd((unsigned long long*)&B.ctr->vchecked, (unsigned long long)vchk);
        if (me == 0 && vcol) atomicAdd((unsigned long long*)&B.ctr->collisions, (unsigned long long)vcol);
    }
}

// Depth-bounded unconstrained models (Params.unbounded): a successor that takes
// an unbounded field past the packed capacity stops the search with
// RMC_E_CAPACITY naming the field.  A separate pass over the launch's states,
// run only for such models, so the expansion kernels carry no code for it
// (in their lane loop it cost 8 % of the S = 5 kernel's instructions).
template <int S, int K>
__global__ __launch_bounds__(256) void k_capacity_check(const Params P, const DevBufs B, u64 lo, u64 hi) {
    constexpr int NW = 2 * S + K;
    const int nl = P.off[10];
    u32 bad = 0;
    for (u64 t = lo + (u64)blockIdx.x * 256 + threadIdx.x; t < hi; t += (u64)gridDim.x * 256) {
        u64 w[S];
        u32 m[K];
        load_state<S, K>(B.store + wslot(B, t) * (u64)NW, w, m);
        for (int lane = 0; lane < nl; ++lane) {
            Delta d;
            lane_delta<S, K>(w, m, lane, P, d);
            if (d.en) bad |= (u32)capacity_exceeded<S, K>(m, d, P);  // 0 for in-model successors
        }
    }
    if (bad) atomicOr(&B.ctr->overflow, bad << 8);
}

// Every lane of every state: full-state verification (single GPU and sharded)
// and the sharded SYMMETRY search (the lossy sent-cache).
template <bool SYM_, int BATCH_, bool DIST_, bool VERIFY_>
struct ExpandEveryLane : ExpandDefaults {
    static constexpr bool SYM = SYM_, DIST = DIST_, VERIFY = VERIFY_;
    static constexpr int BATCH = BATCH_;
};
template <int S, int K, bool SYM, int BATCH, bool DIST, bool VERIFY = false>
__global__ __launch_bounds__(256) void k_expand(const Params P, const PermTable PT, const DevBufs B, u64 lo, u64 hi) {
    static_assert(DIST || VERIFY, "the single-GPU searches have their own kernels (k_expand_sort, k_expand_sym)");
    expand_body<S, K, ExpandEveryLane<SYM, BATCH, DIST, VERIFY>>(P, PT, B, lo, hi);
}

// The single-GPU expansion kernel: the lane-superset walk over windows of 16
// tiles presorted by class (k_window_order), commuting-diamond skipping, the
// parent's mixes recomputed per lane, dynamic per-wave work units, WPE
// waves/SIMD; PI: probe loads issued during the lane code (K = 8 shapes would
// spill 10-13 VGPRs).
template <int BATCH_, int PI>
struct ExpandSort : ExpandDefaults {
    static constexpr bool SORT = true, PRESORT = true, DIA = true;
    static constexpr int BATCH = BATCH_, WTILES = 16, PIPE = PI, DYN = 1;
    // tiles per unit: 8 measured best of 16, 8, 4, 2 on MCraftBenchXL (profiles/r09/units/);
    // -DRMC_UNIT_TILES=... builds the other rungs of the ladder for an A/B
#ifndef RMC_UNIT_TILES
#define RMC_UNIT_TILES 8
#endif
    static constexpr int UNIT_TILES = RMC_UNIT_TILES;
};
template <int S, int K, int BATCH, int PI, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void k_expand_sort(
    const Params P, const PermTable PT, const DevBufs B, u64 lo, u64 hi) {
    expand_body<S, K, ExpandSort<BATCH, PI>>(P, PT, B, lo, hi);
}

// SYMMETRY expansion: each lane fingerprints its successor under the
// permutation that sorts the servers by signature, all S! only on ties
// (deferred to k_ties).  The lane-superset walk over windows of 16 tiles
// presorted by k_window_order, so the block carries no LDS sort (35 instead of
// 48 KB: the 96-bit keys' s_ks array had cut the in-kernel sort's block to 3
// per CU, i.e. 3 waves/SIMD); with 6 probes in flight (BATCH) the block takes
// 28.7 KB and the kernel runs at 5 waves (the shapes that fit 96 VGPRs).
template <int BATCH_>
struct ExpandSym : ExpandDefaults {
    static constexpr bool SYM = true, SORT = true, PRESORT = true;
    static constexpr int BATCH = BATCH_, WTILES = 16;
};
template <int S, int K, int BATCH, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void
k_expand_sym(const Params P, const PermTable PT, const DevBufs B, u64 lo, u64 hi) {
    expand_body<S, K, ExpandSym<BATCH>>(P, PT, B, lo, hi);
}

// The sharded expansion: send markers in the local set, diamond skipping and
// the lane-superset walk, in two forms.
// The pool flush (flush_pool) at the single-GPU kernel's shape: presorted
// windows of 16 tiles, early probe loads (K <= 4), the parent's mixes
// recomputed per lane.
// REP: a replicated level (the whole level's records in B.rep): windows of 8
// tiles sorted in LDS by the kernel, the parent's mixes held (the owner of
// every probe is computed from them), 4 waves/SIMD.
template <int K, int BATCH_, bool REP_>
struct ExpandDist : ExpandDefaults {
    static constexpr bool DIST = true, SORT = true, DIA = true;
    static constexpr bool REP = REP_, POOL = !REP_, PRE = REP_, PRESORT = !REP_;
    static constexpr int BATCH = BATCH_, WTILES = REP_ ? 8 : 16, PIPE = !REP_ && K <= 4 ? 1 : 0;
};
template <int S, int K, int BATCH, bool REP, int WPE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE))) void k_expand_dist(
    const Params P, const PermTable PT, const DevBufs B, u64 lo, u64 hi) {
    expand_body<S, K, ExpandDist<K, BATCH, REP>>(P, PT, B, lo, hi);
}

}  // namespace rmc
