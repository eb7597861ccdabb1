// rmc_kernels_common.hip — the packed layout's shape-free kernels and their launchers (the
// sharded exchange's owner insert, count row and drain; the window order; the set's fill;
// the probe microbenchmark), the lookup of a shape's launchers and the common half of
// set_fp_salt.  The kernels of a shape are in its own object (rmc_kernels_shape.hip).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <map>
#include <mutex>

#include "raft_packed.h"
#include "rmc_dev_outbox.h"
#include "rmc_dev_set.h"
#include "rmc_internal.h"
#include "rmc_plan.h"

namespace rmc {

// Sharded mode, phase 1, owner side: insert the keys other ranks sent;
// reply[t] = 1 if key t was new here (its sender then ships the state), and
// acc[p] counts the new keys of source p — the states p will send in phase 2,
// so the receive sizes need no second count exchange.  Keys arrive grouped by
// source, so a wave mostly adds to one counter (one atomic per source present).
__global__ __launch_bounds__(256) void k_owner_insert(const DevBufs B, const u32* keys, uint8_t* reply, u64 n,
                                                      const SrcOff so, unsigned long long* acc) {
    u64 pr = 0;
    const int me = (int)__lane_id();
    for (u64 t0 = (u64)blockIdx.x * 256ull; t0 < n; t0 += (u64)gridDim.x * 256ull) {
        const u64 t = t0 + threadIdx.x;
        u32 src = 0xFFFFFFFFu;
        if (t < n) {
            const u32* kr = keys + 3 * t;  // {k lo, k hi, s32}
            const int isnew = fp_insert_fp(B.table, B.tmask, Fp{(u64)kr[0] | ((u64)kr[1] << 32), kr[2]},
                                           &B.ctr->table_full);
            reply[t] = (uint8_t)isnew;
            if (isnew) {
                u32 p = 0;
                while (p + 1 < B.world && so.o[p + 1] <= t) ++p;
                src = p;
            }
        }
        pr += (u64)__popcll(__ballot(t < n));
        u64 pending = __ballot(src != 0xFFFFFFFFu);
        while (pending) {  // wave-uniform
            const int l = __ffsll((long long)pending) - 1;
            const u32 s = (u32)__builtin_amdgcn_readlane((int)src, l);
            const u64 bal = __ballot(src == s);
            if (me == l) atomicAdd(&acc[s], (unsigned long long)__popcll(bal));
            pending &= ~bal;
        }
    }
    if (me == 0 && pr) atomicAdd((unsigned long long*)&B.ctr->probes, (unsigned long long)pr);
}

// Presorted windows (k_expand_sort<PS>): the frontier [lo, lo + nf) cut into
// the windows the expansion kernel will take (256 * wt states, wt from the
// launch size and the expansion grid exactly as the kernel computes it), each
// counting-sorted by the states' 1-byte classes: word[win + i] = the i-th
// position of window win in class order.
// The lanes of the wave holding the same 8-bit class as this one (one ballot
// per class bit; inactive lanes never match).
__device__ __forceinline__ u64 match_class8(u32 c, bool act) {
    u64 peers = __ballot(act);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const u64 on = __ballot(act && ((c >> b) & 1u));
        peers &= ((c >> b) & 1u) ? on : ~on;
    }
    return peers;
}

// The class counters take one LDS atomic per class present in a wave's 64
// positions (match_class8), not one per position: a window's states fall in a
// few classes, and same-address LDS atomics serialise (0.91 bank conflicts per
// LDS access with per-position atomics, round 4's PMC profile).
// Round 6: every class byte of the thread's window positions is loaded up front
// (16 independent loads, one memory latency per window instead of one per
// 256-position round), each position's peers (match_class8) are found once and
// kept for the scatter pass, and the grid is one round of resident blocks of
// this kernel rather than of the expansion kernel.
__global__ __launch_bounds__(256) void k_window_order(const uint8_t* cls, u64 wmask, u64 lo, u64 nf, u64 wt,
                                                      uint16_t* word, unsigned long long* wnext) {
    __shared__ u32 bins[256];
    const u32 tid = threadIdx.x;
    const u64 lt = (1ull << __lane_id()) - 1ull;
    if (blockIdx.x == 0 && tid == 0) *wnext = 0;  // the next expansion launch's dynamic work counter
    for (u64 win = (u64)blockIdx.x * 256ull * wt; win < nf; win += (u64)gridDim.x * 256ull * wt) {
        const u32 wn = (u32)((nf - win) < 256ull * wt ? (nf - win) : 256ull * wt);
        u32 cv[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const u32 p = (u32)k * 256u + tid;
            cv[k] = p < wn ? (u32)cls[(lo + win + p) & wmask] : 0u;
        }
        __syncthreads();
        bins[tid] = 0;
        __syncthreads();
        // pass 1: one counter atomic per class present in a wave's 64 positions; each
        // position keeps class | rank among its peers << 8 | their leader << 14 | their number << 20
#pragma unroll
        for (int k = 0; k < 16; ++k) {  // block-uniform rounds
            if ((u32)k * 256u >= wn) break;
            const bool act = (u32)k * 256u + tid < wn;
            const u32 c = cv[k];
            const u64 peers = match_class8(c, act);
            const u32 rank = (u32)__popcll(peers & lt), cnt = (u32)__popcll(peers);
            if (act && rank == 0) atomicAdd(&bins[c], cnt);
            const u32 leader = peers ? (u32)(__ffsll((long long)peers) - 1) : 0u;
            cv[k] = c | (rank << 8) | (leader << 14) | (cnt << 20);
        }
        __syncthreads();
        if (tid < 64) {  // exclusive scan of the 256 counters: 4 per lane, then across the wave
            u32 v[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) { v[q] = bins[tid * 4 + q]; tot += v[q]; }
            u32 incl = tot;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const u32 t = (u32)__shfl_up((int)incl, off);
                if ((int)tid >= off) incl += t;
            }
            u32 ex = incl - tot;
#pragma unroll
            for (int q = 0; q < 4; ++q) { bins[tid * 4 + q] = ex; ex += v[q]; }
        }
        __syncthreads();
        // pass 2: the leader of each class group reserves its group's positions
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if ((u32)k * 256u >= wn) break;
            const u32 p = (u32)k * 256u + tid;
            const bool act = p < wn;
            const u32 v = cv[k], c = v & 0xFFu, rank = (v >> 8) & 63u, leader = (v >> 14) & 63u, cnt = v >> 20;
            u32 base = 0;
            if (act && rank == 0) base = atomicAdd(&bins[c], cnt);
            base = (u32)__shfl((int)base, (int)leader);
            if (act) word[win + base + rank] = (uint16_t)p;
        }
    }
}

hipError_t launch_window_order(const DevBufs& B, u64 lo, u64 hi, u64 grid, u64 wt_max, hipStream_t st) {
    const u64 nf = hi - lo;
    if (nf == 0) return hipSuccess;
    if (wt_max > 16 || nf > (1ull << kMaxLaunchLog2)) return hipErrorInvalidValue;
    // the expansion kernel's window size for this launch (expand_body: per_block)
    const u64 wt = rmc_host::launch_window_tiles(nf, grid, wt_max);
    const u64 nwin = (nf + 256ull * wt - 1) / (256ull * wt);
    // its own grid: one round of its resident blocks (RMC_WORDER_GRID=0: the expansion's, round 5)
    static const u64 og = [] {
        const char* e = getenv("RMC_WORDER_GRID");
        return e ? (u64)atoll(e) : (u64)1;
    }();
    const u64 g2 = og == 0 ? grid : og == 1 ? resident_grid(reinterpret_cast<const void*>(&k_window_order)) : og;
    hipLaunchKernelGGL(k_window_order, dim3((unsigned)(nwin < g2 ? nwin : g2)), dim3(256), 0, st, B.cls, B.wmask, lo, nf,
                       wt, B.word, (unsigned long long*)&B.ctr->wnext);
    return hipGetLastError();
}

// Sharded mode: the count row of one exchange round (launch_pack_counts): a
// block of kRowWords u64 per peer — keys for it, flags, this rank's counters —
// then novf.
__global__ void k_pack_counts(const DevBufs B, u64 host_more, u64 ovf_done, u64* out, u64* mirror) {
    const u32 p = threadIdx.x;
    const u64 novf = B.ctr->novf;
    bool sends = false;
    for (u32 q = 0; q < B.world; ++q) sends |= q != B.rank && B.ocount[q] != 0;
    // bit 0: more to send this level; bit 1: the parking buffer overflowed (every
    // rank reads every row and fails alike); bit 2: keys to some peer this round
    const u64 flags = host_more | (novf > ovf_done ? 1ull : 0ull) | (novf > B.ovf_cap ? 2ull : 0ull) |
                      (sends ? 4ull : 0ull);
    if (p < B.world) {
        u64* r = out + (u64)p * kRowWords;
        const u64 c = B.ocount[p];
        r[0] = p == B.rank ? 0ull : (c < B.kcap ? c : B.kcap);
        r[1] = flags;
        const u64* k = reinterpret_cast<const u64*>(B.ctr);
        for (int i = 0; i < kRowWords - 2; ++i) r[2 + i] = k[i];
        if (mirror)
            for (int i = 0; i < kRowWords; ++i) mirror[(u64)p * kRowWords + i] = r[i];
    }
    if (p == 0) out[(u64)kRowWords * B.world] = novf;
    if (mirror) __threadfence_system();  // the row is in pinned host memory: visible before the event
}

// Sharded mode: parked keys ovf[a, a + n) back into the outbox (n <= kcap, so
// no destination can overflow; ocount was zeroed for this round).
__global__ __launch_bounds__(256) void k_drain(const DevBufs B, u64 a, u64 n) {
    for (u64 t = (u64)blockIdx.x * 256ull + threadIdx.x; t < n; t += (u64)gridDim.x * 256ull) {
        const u64* r = B.ovf + 3 * (a + t);
        const u64 k = r[0], sf = r[1], tk = r[2];
        const u32 dest = (u32)((tk >> 48) & 0xFFu);
        const u64 slot = atomicAdd(&B.ocount[dest], 1ull);
        if (slot >= B.kcap) {  // cannot happen for n <= kcap; never write past the outbox
            atomicOr(&B.ctr->overflow, 2u);
            continue;
        }
        put_key(B, dest, slot, k, (u32)sf, (tk & ((1ull << 48) - 1)) | (tk & (0xFFull << 56)));
    }
}

// Probe-rate microbenchmark (the roofline ceiling for k_expand): every thread
// issues `iters` rounds of BATCH independent random 8-byte accesses into a
// table of `mask + 1` slots — plain loads (mode 0) or CAS (mode 1) — the
// access pattern of the fingerprint set, with no successor computation.
template <int BATCH>
__global__ __launch_bounds__(256) void k_probe_bench(u64* table, u64 mask, u32 iters, int mode, u64* sink) {
    const u64 t = (u64)blockIdx.x * 256ull + threadIdx.x;
    u64 acc = 0;
    for (u32 it = 0; it < iters; ++it) {
        u64 v[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            const u64 key = mix64(t * 0x9E3779B97F4A7C15ull + (u64)it * BATCH + b) | 1ull;
            if (mode == 0) v[b] = table[key & mask];
            else v[b] = atomicCAS((unsigned long long*)&table[key & mask], 0ull, (unsigned long long)key);
        }
#pragma unroll
        for (int b = 0; b < BATCH; ++b) acc ^= v[b];
    }
    if (acc == 0x5A5A5A5A5A5A5A5Aull) sink[0] = acc;  // keeps the loads live
}

hipError_t launch_owner_insert(const DevBufs& B, const u64* keys, uint8_t* reply, u64 n, const SrcOff& so,
                               unsigned long long* acc, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const u64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_owner_insert, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, B,
                       reinterpret_cast<const u32*>(keys), reply, n, so, acc);
    return hipGetLastError();
}

hipError_t launch_pack_counts(const DevBufs& B, u64 host_more, u64 ovf_done, u64* out, hipStream_t st, u64* mirror) {
    if (B.world > (u32)kMaxWorld) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pack_counts, dim3(1), dim3(64), 0, st, B, host_more, ovf_done, out, mirror);
    return hipGetLastError();
}

hipError_t launch_drain(const DevBufs& B, u64 a, u64 n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const u64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_drain, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, B, a, n);
    return hipGetLastError();
}

// Clears the fingerprint set (or writes the verification slot map's 0xFF) at
// the start of a run: 16-B nontemporal stores, each thread four per round,
// consecutive across the block, the rounds strided over a fixed grid.  The
// run-start clear of the 69-GB XL set is 1.5 % of its BFS (verdict r05).
typedef u32 v4u __attribute__((ext_vector_type(4)));
template <bool NT>
__global__ void __launch_bounds__(256) k_fill(v4u* p, u64 n16, u32 pat) {
    const v4u x = {pat, pat, pat, pat};
    const u64 stride = (u64)gridDim.x * 1024ull;
    for (u64 i = (u64)blockIdx.x * 1024ull + threadIdx.x; i < n16; i += stride) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u64 q = i + (u64)j * 256ull;
            if (q < n16) {
                if constexpr (NT) __builtin_nontemporal_store(x, p + q);
                else p[q] = x;
            }
        }
    }
}

hipError_t launch_fill(void* p, u64 bytes, uint8_t byte, hipStream_t st) {
    static const int mode = [] {  // RMC_FILL=0: hipMemsetAsync (the A/B baseline), 1 nontemporal, 2 plain stores
        const char* e = getenv("RMC_FILL");
        return e ? atoi(e) : 1;
    }();
    const u64 n16 = mode ? bytes / 16 : 0;
    if (n16) {
        const u64 blocks = (n16 + 1023) / 1024;
        const u32 pat = 0x01010101u * byte;
        const dim3 g((unsigned)(blocks < 4096 ? blocks : 4096));
        if (mode == 1) hipLaunchKernelGGL(k_fill<true>, g, dim3(256), 0, st, static_cast<v4u*>(p), n16, pat);
        else hipLaunchKernelGGL(k_fill<false>, g, dim3(256), 0, st, static_cast<v4u*>(p), n16, pat);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (bytes > n16 * 16) return hipMemsetAsync(static_cast<char*>(p) + n16 * 16, byte, bytes - n16 * 16, st);
    return hipSuccess;
}

hipError_t launch_probe_bench(u64* table, u64 mask, u64 threads, u32 iters, int mode, u64* sink, hipStream_t st) {
    hipLaunchKernelGGL((k_probe_bench<8>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, table, mask,
                       iters, mode, sink);
    return hipGetLastError();
}

// The exclusive scan of the per-state edge counts of one chunk of the graph walk (at most
// a few hundred thousand states): one block, each thread sums a contiguous part, the parts'
// sums are scanned in LDS, and each thread writes its part's offsets.  off has n + 1 entries.
__global__ __launch_bounds__(1024) void k_graph_scan(const u32* __restrict__ cnt, u64 n, u64* __restrict__ off) {
    __shared__ u64 s_sum[1024];
    const u64 per = (n + 1023) / 1024;
    const u64 a = threadIdx.x * per < n ? threadIdx.x * per : n, b = a + per < n ? a + per : n;
    u64 s = 0;
    for (u64 q = a; q < b; ++q) s += cnt[q];
    s_sum[threadIdx.x] = s;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        const u64 v = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0ull;
        __syncthreads();
        s_sum[threadIdx.x] += v;
        __syncthreads();
    }
    u64 base = s_sum[threadIdx.x] - s;
    for (u64 q = a; q < b; ++q) {
        off[q] = base;
        base += cnt[q];
    }
    if (threadIdx.x == 1023) off[n] = s_sum[1023];
}

hipError_t launch_graph_scan(const u32* cnt, u64 n, u64* off, hipStream_t st) {
    hipLaunchKernelGGL(k_graph_scan, dim3(1), dim3(1024), 0, st, cnt, n, off);
    return hipGetLastError();
}

// One round of resident blocks of kernel `k` on this device (blocks per CU at
// its register / LDS occupancy x CUs), cached per kernel and device: 1024 for
// the 4-wave sorted kernels, 1280 for the 5-wave every-lane kernel (a fixed
// 1024 left a fifth of the CUs' slots idle on S = 5: 0.339 s vs 0.289 s).
u64 resident_grid(const void* k) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, u64> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    auto it = cache.find({k, dev});
    if (it != cache.end()) return it->second;
    int nb = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, 256, 0) != hipSuccess || nb <= 0) nb = 4;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    const u64 v = (u64)nb * (u64)cus;
    cache[{k, dev}] = v;
    return v;
}

// ---- the shapes built: one object each (rmc_kernels_shape.hip; the Makefile's SHAPES) ----
#define RMC_SHAPES(X) X(2, 4) X(2, 8) X(3, 4) X(3, 8) X(4, 4) X(4, 8) X(5, 4) X(5, 8)
const ShapeKernels* shape_kernels(int S, int K) {
#define RMC_SHAPE_CASE(SS, KK)                                   \
    {                                                            \
        extern const ShapeKernels RMC_SHAPE_TABLE(SS, KK);       \
        if (S == SS && K == KK) return &RMC_SHAPE_TABLE(SS, KK); \
    }
    RMC_SHAPES(RMC_SHAPE_CASE)
#undef RMC_SHAPE_CASE
    return nullptr;
}

hipError_t set_fp_salt(const ShapeKernels& k, u64 seed, u32 set_epoch, hipStream_t st) {
    const u64 salt = seed ? (mix64(seed) & ((1ull << 59) - 1)) : 0ull;
    if (set_epoch > 255) return hipErrorInvalidValue;
    const u64 ep = (u64)set_epoch << 56;
    // the common object's kernels insert too (k_owner_insert: sharded keys received)
    {
        const u64 h_ep = ep;
        const hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_set_ep), &h_ep, sizeof h_ep, 0, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    // only the ctx's shape object runs its kernels (the call waits for both copies)
    return k.set_salt(salt, ep, st);
}

}  // namespace rmc
