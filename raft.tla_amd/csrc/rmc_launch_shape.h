// rmc_launch_shape.h — the host launchers of one packed shape (S servers, K bag slots) and the
// shape's table of them (rmc_internal.h ShapeKernels, which names and explains their arguments).
#pragma once
#include <cstdlib>

#include "rmc_dev_act.h"
#include "rmc_dev_cons.h"
#include "rmc_dev_expand.h"
#include "rmc_dev_graph.h"
#include "rmc_dev_pred.h"
#include "rmc_dev_sharded.h"
#include "rmc_dev_tools.h"
#include "rmc_dev_verify.h"
#include "rmc_internal.h"
#include "rmc_plan.h"

namespace rmc {

template <int S, int K>
static hipError_t launch_sim_t(const Params& P, const u32* inits, u64 n_init, u64 n_beh, int depth, u64 seed,
                               int mode, SimCounters* out, i64 rec_beh, u32* rec, hipStream_t st) {
    const u64 blocks = (n_beh + 255) / 256;
    const u64 g = blocks < 4096 ? blocks : 4096;
    hipLaunchKernelGGL((k_simulate<S, K>), dim3((unsigned)g), dim3(256), 0, st, P, inits, n_init, n_beh, depth, seed,
                       mode, out, rec_beh, rec);
    return hipGetLastError();
}

// The coverage pass of one expansion launch (or of the seed step: no parents).
template <int S, int K>
static hipError_t launch_cover_t(const Params& P, const DevBufs& B, u64 lo, u64 hi, u64 nlo, u64 nhi, u64 n_init,
                                 unsigned long long* cov, hipStream_t st) {
    const u64 np = hi > lo ? hi - lo : 0, nn = nhi > nlo ? nhi - nlo : 0;
    const u64 blocks = ((np > nn ? np : nn) + 255) / 256;
    const u64 g = blocks < 1 ? 1 : blocks < 2048 ? blocks : 2048;  // grid-stride over both ranges
    hipLaunchKernelGGL((k_cover<S, K>), dim3((unsigned)g), dim3(256), 0, st, P, B, lo, hi, nlo, nhi, n_init, cov);
    return hipGetLastError();
}

// The violation pass of one expansion launch (or of the seed step) over the states it added.
template <int S, int K>
static hipError_t launch_violations_t(const Params& P, const DevBufs& B, u64 nlo, u64 nhi, unsigned long long* viol,
                                      hipStream_t st) {
    if (nhi <= nlo) return hipSuccess;
    const u64 blocks = (nhi - nlo + 255) / 256;
    hipLaunchKernelGGL((k_violations<S, K>), dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, P, B,
                       nlo, nhi, viol);
    return hipGetLastError();
}

// The predicate pass of one expansion launch (or of the seed step) over the states it added.
template <int S, int K>
static hipError_t launch_pred_t(const pred::Program* prog, const DevBufs& B, u64 nlo, u64 nhi,
                                unsigned long long* word, hipStream_t st) {
    if (nhi <= nlo) return hipSuccess;
    const u64 blocks = (nhi - nlo + kPredThreads - 1) / kPredThreads;
    hipLaunchKernelGGL((k_pred<S, K>), dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kPredThreads), 0, st, prog,
                       B, nlo, nhi, word);
    return hipGetLastError();
}

// The constraint pass of one expansion launch (or of the seed step) over the states it added:
// the filter, the scan of its tile counts, the holes, the move.
template <int S, int K>
static hipError_t launch_cons_t(const pred::Program* prog, const DevBufs& B, u64 nlo, u64 nhi, const ConsBufs& C,
                                unsigned long long* word, hipStream_t st) {
    if (nhi <= nlo) return hipSuccess;
    const u64 n = nhi - nlo, nt = cons::tiles(n);
    const unsigned grid = (unsigned)(nt < 2048 ? nt : 2048);
    hipLaunchKernelGGL((k_cons<S, K>), dim3(grid), dim3(kPredThreads), 0, st, prog, B, nlo, nhi, C, word);
    if (hipError_t e = launch_graph_scan(C.cnt, nt, C.off, st)) return e;
    hipLaunchKernelGGL((k_cons_holes<S, K>), dim3(grid), dim3(256), 0, st, n, C);
    hipLaunchKernelGGL((k_cons_move<S, K>), dim3(grid), dim3(256), 0, st, B, nlo, n, C, word + 1);
    return hipGetLastError();
}

template <int S, int K>
static hipError_t launch_cons_inv_t(const Params& P, const DevBufs& B, u64 lo, u64 hi, hipStream_t st) {
    if (hi <= lo) return hipSuccess;
    const u64 blocks = (hi - lo + 255) / 256;
    hipLaunchKernelGGL((k_cons_inv<S, K>), dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, st, P, B, lo,
                       hi);
    return hipGetLastError();
}

template <int S, int K>
static hipError_t launch_pred_eval_t(const pred::Program* prog, const u32* in, u64 n, uint8_t* out, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL((k_pred_eval<S, K>), dim3((unsigned)((n + kPredThreads - 1) / kPredThreads)), dim3(kPredThreads),
                       0, st, prog, in, n, out);
    return hipGetLastError();
}

// The action-property pass of one expansion launch over its parents [lo, hi).
template <int S, int K>
static hipError_t launch_act_t(const pred::Program* prog, const Params* P, const DevBufs& B, u64 lo, u64 hi,
                               unsigned long long* word, hipStream_t st) {
    if (hi <= lo) return hipSuccess;
    const u64 blocks = (hi - lo + kPredThreads - 1) / kPredThreads;
    hipLaunchKernelGGL((k_act<S, K>), dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(kPredThreads), 0, st, prog,
                       P, B, lo, hi, word);
    return hipGetLastError();
}

template <int S, int K>
static hipError_t launch_act_eval_t(const pred::Program* prog, const u32* in, u64 n, uint8_t* out, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL((k_act_eval<S, K>), dim3((unsigned)((n + kPredThreads - 1) / kPredThreads)), dim3(kPredThreads),
                       0, st, prog, in, n, out);
    return hipGetLastError();
}

template <int S, int K>
static hipError_t launch_check_t(const Params& P, const u32* in, u64 n, int* out, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL((k_check<S, K>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, in, n, out);
    return hipGetLastError();
}

template <int S, int K>
static hipError_t launch_keys_t(bool sym, const Params& P, const PermTable& PT, const u32* in, u64 n, u64* keys,
                                const u32* ref, unsigned char* same, hipStream_t st) {
    if (!n) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (sym) hipLaunchKernelGGL((k_keys<S, K, true>), grid, dim3(256), 0, st, PT, P.fp_mask, in, n, keys, ref, same);
    else hipLaunchKernelGGL((k_keys<S, K, false>), grid, dim3(256), 0, st, PT, P.fp_mask, in, n, keys, ref, same);
    return hipGetLastError();
}

// Blocks of the expansion kernels (RMC_EXPAND_GRID for A/B runs, from 1 block; default
// 1024 = the resident blocks at 4 waves/SIMD: 4 per CU x 256 CUs, so a launch
// is one block round and every window sorts more tiles; 309.7 vs 315.6 ms per
// MCraftBench BFS against 2048, profiles/r03/ab/).  The other grid-stride
// kernels run 2048 blocks.
static u64 expand_grid_env() {
    static u64 v = [] {
        const char* e = getenv("RMC_EXPAND_GRID");
        const long long x = e ? atoll(e) : 0;
        return x >= 1 && x <= (1 << 20) ? (u64)x : (u64)0;
    }();
    return v;
}

// Probes in flight per thread of the every-lane kernels: 8 (measured best of
// 4/8/16 on MI355X).  The presorted plain kernels keep 5 (80 VGPRs: 6
// waves/SIMD), the SYMMETRY kernel 6 where it then fits 5 waves.  The variants
// measured and rejected in rounds 2-6 (the mixes held, windows sorted in LDS,
// fixed shares, 4-8 probes at 4-6 waves, prefetching, 64-B store records, the
// flush doing the routing) are in git history; their numbers are in DESIGN.md
// §Kernels.
constexpr int kBatch = 8;

// kernel(args...) over n work items, on at most max_blocks blocks of 256 threads: kStrided for
// the grid-stride kernels, kPerBlock for the kernels of one thread per item.
constexpr u64 kStrided = 2048, kPerBlock = 0x7fffffffull;
template <class... KA, class... A>
static hipError_t launch_n(void (*kernel)(KA...), u64 n, u64 max_blocks, hipStream_t st, const A&... args) {
    if (n == 0) return hipSuccess;
    const u64 blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < max_blocks ? blocks : max_blocks)), dim3(256), 0, st, args...);
    return hipGetLastError();
}

// One expansion launch over [lo, hi): `kernel` on RMC_EXPAND_GRID blocks (not kFixedGrid), else
// on `dflt` blocks (0: one round of the kernel's resident blocks).  kPresorted: after
// k_window_order over the same launch and grid.  kCapacity: then a depth-bounded unconstrained
// model's capacity pass.  kResume: a presorted launch that stopped on admission, launched
// again: no k_window_order (B.word and Counters.wnext are as it left them) and no second
// capacity pass.
enum : unsigned { kPresorted = 1, kFixedGrid = 2, kCapacity = 4, kResume = 8 };
template <class Kernel>
static u64 expansion_grid(Kernel kernel, unsigned how, u64 dflt, u64 nf) {
    const u64 blocks = (nf + 255) / 256;
    const u64 want = expand_grid_env() && !(how & kFixedGrid) ? expand_grid_env()
                     : dflt                                   ? dflt
                                                              : resident_grid(reinterpret_cast<const void*>(kernel));
    return blocks < want ? blocks : want;
}
template <int S, int K, class Kernel>
static hipError_t expansion(Kernel kernel, unsigned how, u64 dflt, const Params& P, const PermTable& PT,
                            const DevBufs& B, u64 lo, u64 hi, hipStream_t st) {
    if (hi == lo) return hipSuccess;
    const u64 blocks = (hi - lo + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const u64 eg = expansion_grid(kernel, how, dflt, hi - lo);
    if ((how & kPresorted) && !(how & kResume))
        if (hipError_t e = launch_window_order(B, lo, hi, eg, 16, st)) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)eg), dim3(256), 0, st, P, PT, B, lo, hi);
    if ((how & kCapacity) && !(how & kResume) && P.unbounded)
        hipLaunchKernelGGL((k_capacity_check<S, K>), dim3((unsigned)(blocks < kStrided ? blocks : kStrided)), dim3(256),
                           0, st, P, B, lo, hi);
    return hipGetLastError();
}

// The plain single-GPU kernel: 5 probes, 6 waves/SIMD (80 VGPRs).  S >= 4 (68 / 92 lanes): 5
// waves (96 VGPRs, 16 B of scratch) beat 6 waves with 48 B of spills: MCraft5 -depth 20 206 vs
// 245-246 ms (4 probes at 6 waves 247-248 ms), profiles/r06/ab/s5_waves.txt
template <int S, int K>
static constexpr auto sort_kernel() {
    return &k_expand_sort<S, K, 5, K <= 4 ? 1 : 0, S >= 4 ? 5 : 6>;
}
template <int S, int K>
static ShapeKernels::AdmitShape admit_shape_t(u64 nf) {
    typedef ExpandSort<5, K <= 4 ? 1 : 0> C;
    static_assert(C::DYN != 0 && C::PRESORT, "admission: the dynamic-unit kernel");
    ShapeKernels::AdmitShape a{};
    a.grid = nf ? expansion_grid(sort_kernel<S, K>(), kPresorted, 0, nf) : 0;
    a.wt = a.grid ? (u32)rmc_host::launch_window_tiles(nf, a.grid, (u64)C::WTILES) : 0;
    a.ut = (u32)C::UNIT_TILES;
    a.list_cap = (u32)WCAP;
    return a;
}

template <int S, int K>
static hipError_t launch_expand(bool sym, bool verify, const Params& P, const PermTable& PT, const DevBufs& B, u64 lo,
                                u64 hi, hipStream_t st) {
    // every kernel of this object walks lanes through the 128-bit LaneMask and
    // the lane descriptors; a wider shape needs its own walk
    static_assert(Lanes<S, K>::N <= 128, "a shape's lanes must fit the 128-bit lane mask");
    constexpr unsigned C = kCapacity;
    // SYMMETRY keeps 2048 blocks: 79.7 vs 81.5 ms on the MCraftBench bounds
    if (sym && verify)
        return expansion<S, K>(&k_expand<S, K, true, kBatch, false, true>, kFixedGrid | C, 2048, P, PT, B, lo, hi, st);
    if (sym) {
        // 6 probes in flight, 5 waves/SIMD: the shapes that fit 96 VGPRs without spills
        if constexpr (S <= 3 && K == 4)
            return expansion<S, K>(&k_expand_sym<S, K, 6, 5>, kPresorted | C, 2048, P, PT, B, lo, hi, st);
        else
            return expansion<S, K>(&k_expand_sym<S, K, kBatch, 1>, kPresorted | C, 2048, P, PT, B, lo, hi, st);
    }
    if (verify) return expansion<S, K>(&k_expand<S, K, false, kBatch, false, true>, C, 0, P, PT, B, lo, hi, st);
    return expansion<S, K>(sort_kernel<S, K>(), kPresorted | C, 0, P, PT, B, lo, hi, st);
}

template <int S, int K>
static hipError_t launch_expand_dist(bool sym, bool verify, const Params& P, const PermTable& PT, const DevBufs& B,
                                     u64 lo, u64 hi, hipStream_t st) {
    constexpr unsigned C = kCapacity;
    if (verify)  // sharded full-state verification: every lane, hits compared
        return sym ? expansion<S, K>(&k_expand<S, K, true, kBatch, true, true>, C, 0, P, PT, B, lo, hi, st)
                   : expansion<S, K>(&k_expand<S, K, false, kBatch, true, true>, C, 0, P, PT, B, lo, hi, st);
    // SYMMETRY: the lossy sent-cache
    if (sym) return expansion<S, K>(&k_expand<S, K, true, kBatch, true>, C, 0, P, PT, B, lo, hi, st);
    // the pool flush at the single-GPU kernel's shape.  S >= 4: 5 waves/SIMD (96
    // VGPRs) instead of 6 with 96 B of spills: MCraft5 to depth 20 on one sharded
    // rank 0.322 vs 0.568 s (profiles/r06/ab/s5_dist_waves.txt)
    return expansion<S, K>(&k_expand_dist<S, K, 5, false, S >= 4 ? 5 : 6>, kPresorted | C, 0, P, PT, B, lo, hi, st);
}

// The edges out of the stored states [lo, hi) (k_graph_edges): kBatch probes in flight per
// thread, as the every-lane expansion kernels keep.
template <int S, int K>
static hipError_t launch_graph_edges_t(bool sym, const Params& P, const PermTable& PT, const DevBufs& B, u64 lo,
                                       u64 hi, const u64* off, GraphEdge* out, u64 cap, unsigned long long* err,
                                       hipStream_t st) {
    return launch_n(sym ? k_graph_edges<S, K, true, kBatch> : k_graph_edges<S, K, false, kBatch>, hi - lo, kStrided,
                    st, P, PT, B, lo, hi, off, out, cap, err);
}

// The salt and the set epoch of this object's kernels (raft_packed.h c_fp_salt, c_set_ep).
static hipError_t set_object_salt(u64 salt, u64 epoch, hipStream_t st) {
    // staged on this call's stack and waited for: concurrent callers (one host
    // thread per GPU in rmc-tlc -gpus N) share no staging buffer
    const u64 h_salt = salt, h_ep = epoch;
    hipError_t e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_fp_salt), &h_salt, sizeof h_salt, 0, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyToSymbolAsync(HIP_SYMBOL(c_set_ep), &h_ep, sizeof h_ep, 0, hipMemcpyHostToDevice, st);
    return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// The shape's table.  Not constexpr: a const object with a constant initialiser is emitted
// into the device code too, where these host functions do not exist.
template <int S, int K>
static ShapeKernels shape_table() {
    ShapeKernels k{};
    k.expand = launch_expand<S, K>;
    k.expand_dist = launch_expand_dist<S, K>;
    k.admit_shape = admit_shape_t<S, K>;
    k.expand_resume = [](const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi, hipStream_t st) {
        if (P.symmetry) return hipErrorInvalidValue;  // the plain search only
        return expansion<S, K>(sort_kernel<S, K>(), kPresorted | kResume, 0, P, PT, B, lo, hi, st);
    };
    k.expand_rep = [](const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi, hipStream_t st) {
        if (hi != lo && P.symmetry) return hipErrorInvalidValue;  // the plain search only
        return expansion<S, K>(&k_expand_dist<S, K, kBatch, true, 4>, 0, 0, P, PT, B, lo, hi, st);
    };
    k.route = [](const Params& P, const DevBufs& B, hipStream_t st) {
        if (P.symmetry) return hipErrorInvalidValue;  // the plain search only
        hipLaunchKernelGGL((k_route_fix<S, K>), dim3(256), dim3(256), 0, st, P, B);
        hipLaunchKernelGGL((k_route<S, K>), dim3(1024), dim3(256), 0, st, P, B);
        return hipGetLastError();
    };
    k.ties = [](const Params& P, const PermTable& PT, const DevBufs& B, hipStream_t st) {
        if (P.symmetry) hipLaunchKernelGGL((k_ties<S, K>), dim3(1024), dim3(256), 0, st, P, PT, B);
        return hipGetLastError();
    };
    k.seed = [](bool sym, const Params& P, const PermTable& PT, const DevBufs& B, const u32* staged, u64 n,
                hipStream_t st) {
        return launch_n(sym ? k_seed<S, K, true> : k_seed<S, K, false>, n, kPerBlock, st, P, PT, B, staged, n);
    };
    k.list = [](bool sym, const Params& P, const PermTable& PT, const u32* in, u64 n, u32* out, u64 cap,
                unsigned long long* count, hipStream_t st) {
        return launch_n(sym ? k_list<S, K, true> : k_list<S, K, false>, n, kPerBlock, st, P, PT, in, n, out, cap,
                        count);
    };
    k.publish = [](bool sym, const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi, hipStream_t st) {
        return launch_n(sym ? k_publish<S, K, true> : k_publish<S, K, false>, hi - lo, kStrided, st, P, PT, B, lo, hi);
    };
    k.rehash = [](bool sym, const Params& P, const PermTable& PT, const DevBufs& B, u64 lo, u64 hi, hipStream_t st) {
        return launch_n(sym ? k_rehash<S, K, true> : k_rehash<S, K, false>, hi - lo, kStrided, st, P, PT, B, lo, hi);
    };
    k.verify = [](bool sym, const Params& P, const PermTable& PT, const DevBufs& B, u64 n_hits, hipStream_t st) {
        return launch_n(sym ? k_verify<S, K, true> : k_verify<S, K, false>, n_hits, kStrided, st, P, PT, B, n_hits);
    };
    k.verify_host = [](bool sym, const Params& P, const PermTable& PT, const DevBufs& B, const u32* staged_owners,
                       u64 n_hits, u64 hbuf_off, hipStream_t st) {
        return launch_n(sym ? k_verify_host<S, K, true> : k_verify_host<S, K, false>, n_hits, kStrided, st, P, PT, B,
                        staged_owners, n_hits, hbuf_off);
    };
    k.materialize_remote = [](const Params& P, const DevBufs& B, const uint8_t* reply, u64 keys_per_dest,
                              u64 window_off, hipStream_t st) {
        return launch_n(k_materialize_remote<S, K>, keys_per_dest * (u64)B.world, kStrided, st, P, B, reply,
                        keys_per_dest, window_off);
    };
    k.store_remote = [](const Params& P, const DevBufs& B, const u32* recs, u64 n, hipStream_t st) {
        return launch_n(k_store_remote<S, K>, n, kStrided, st, P, B, recs, n);
    };
    k.compare_remote = [](bool sym, const Params& P, const PermTable& PT, const DevBufs& B, const u32* recs, u64 n,
                          hipStream_t st) {
        return launch_n(sym ? k_compare_remote<S, K, true> : k_compare_remote<S, K, false>, n, kStrided, st, P, PT, B,
                        recs, n);
    };
    k.pack_rep = [](const DevBufs& B, u64 lo, u64 hi, u32* out, hipStream_t st) {
        return launch_n(k_pack_rep<S, K>, hi - lo, kStrided, st, B, lo, hi, out);
    };
    k.simulate = launch_sim_t<S, K>;
    k.cover = launch_cover_t<S, K>;
    k.violations = launch_violations_t<S, K>;
    k.check = launch_check_t<S, K>;
    k.pred = launch_pred_t<S, K>;
    k.pred_eval = launch_pred_eval_t<S, K>;
    k.act = launch_act_t<S, K>;
    k.act_eval = launch_act_eval_t<S, K>;
    k.cons = launch_cons_t<S, K>;
    k.cons_inv = launch_cons_inv_t<S, K>;
    k.keys = launch_keys_t<S, K>;
    k.set_salt = set_object_salt;
    k.graph_count = [](const Params& P, const DevBufs& B, u64 lo, u64 hi, u32* cnt, hipStream_t st) {
        return launch_n(k_graph_count<S, K>, hi - lo, kStrided, st, P, B, lo, hi, cnt);
    };
    k.graph_edges = launch_graph_edges_t<S, K>;
    k.graph_find = [](bool sym, const Params& P, const PermTable& PT, const DevBufs& B, const u32* in, u64 n,
                      u64* index, hipStream_t st) {
        return launch_n(sym ? k_graph_find<S, K, true> : k_graph_find<S, K, false>, n, kPerBlock, st, P, PT, B, in, n,
                        index);
    };
    return k;
}

}  // namespace rmc
