// rmc_spill.cpp — frontier spill (RMC_FLAG_SPILL) of the packed layout: the window
// rebase, the host trace links, and the host mirror of full-state verification.
#include <sys/mman.h>

#include <algorithm>
#include <cstring>

#include "rmc_ctx.h"

using namespace rmc;

namespace rmc_host {

int window_too_small(rmc_ctx* c, u64 win, u64 slot_bytes) {
    return fail(c, RMC_E_CAPACITY,
                "spill: the device window (" + std::to_string(win) +
                    " states) cannot hold the frontier and the level being built; raise "
                    "rmc_config.device_window, or give the fingerprint set less HBM "
                    "(rmc_config.set_bytes, rmc-tlc -fpmem: its " +
                    std::to_string(c->table_slots) + " slots take " +
                    std::to_string((c->table_slots * slot_bytes) >> 30) + " GiB) so the window gets more");
}

// The most new states one state's expansion can yield (rmc_plan.h
// new_states_bound, never more than the lanes).  The spill window sizes its
// launches by this bound (RMC_LANE_BOUND=0: every lane, the round-5 bound).
u64 max_new_per_state(const rmc_ctx* c) {
    const u64 lanes = (u64)c->P.off[10];
    static const bool all_lanes = [] {
        const char* e = getenv("RMC_LANE_BOUND");
        return e && atoi(e) == 0;
    }();
    if (all_lanes) return lanes;
    return packed_new_states_bound(lanes, (u64)c->sh.S, (u64)c->P.V, (u64)(c->P.off[8] - c->P.off[7]));
}

// ---- frontier spill (RMC_FLAG_SPILL) ---------------------------------------------
// TLC keeps its state queue in the states/ directory and a trace file of
// (parent, action) records from which it re-derives counterexample states
// (SURVEY.md §8f rank 4).  Here the fingerprint set and the state window stay
// in HBM; spilled states keep only their trace links in host memory.  Kernels
// index states by their global index through device pointers biased by -base.
void spill_rebase(rmc_ctx* c, u64 base) {
    SpillState& X = c->spill;
    X.base = base;
    if (X.dev_links) {  // the ring window (DevBufs.wmask): nothing moves, base = the oldest resident state
        c->B.store = X.store;
        c->B.parent = X.parent;
        c->B.act = X.act;
        c->B.foot = X.foot;
        c->B.cls = X.cls;
        c->B.cap = c->B.lim = X.total_cap;
        return;
    }
    const uintptr_t nw = (uintptr_t)c->NW;
    c->B.store = (u32*)((uintptr_t)X.store - (uintptr_t)base * nw * 4);
    const u64 lb = X.dev_links ? 0 : base;  // device links: indexed by global index, never rebased
    c->B.parent = (u64*)((uintptr_t)X.parent - (uintptr_t)lb * 8);
    c->B.act = (uint8_t*)((uintptr_t)X.act - (uintptr_t)lb);
    c->B.foot = (u64*)((uintptr_t)X.foot - (uintptr_t)base * 8);
    c->B.cls = (uint8_t*)((uintptr_t)X.cls - (uintptr_t)base);
    // device links hold total_cap states: no store index may pass it
    c->B.cap = X.dev_links ? std::min(base + X.win, X.total_cap) : base + X.win;
    c->B.lim = c->B.cap;
}

// Address space for the trace links of every state the set can hold; pages
// are only backed once a spill touches them.
int spill_reserve(rmc_ctx* c) {
    SpillState& X = c->spill;
    X.h_bytes = (size_t)X.total_cap * 9;
    void* m = mmap(nullptr, X.h_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) {
        X.h_bytes = 0;
        return fail(c, RMC_E_NOMEM, "spill: cannot reserve host address space for the trace links");
    }
    (void)madvise(m, X.h_bytes, MADV_HUGEPAGE);  // 2 MiB faults: fewer, cheaper first touches
    X.h_parent = (u64*)m;
    X.h_act = (uint8_t*)m + (size_t)X.total_cap * 8;
    X.faulted = 0;
    return 0;
}

void spill_free(rmc_ctx* c) {
    if (c->spill.ahead.joinable()) c->spill.ahead.join();
    if (c->spill.h_bytes) munmap(c->spill.h_parent, c->spill.h_bytes);
    c->spill.h_parent = nullptr;
    c->spill.h_act = nullptr;
    c->spill.h_bytes = 0;
}

// Touch fresh host pages from several threads: a device-to-host copy into
// untouched pageable memory runs at page-fault speed (~13 GB/s measured),
// into touched memory at ~48 GB/s (profiles/r02/host_link_rates.jsonl).
static void prefault(void* p, size_t n) {
    const int T = (int)std::min<size_t>(8, std::max<size_t>(1, n >> 26));
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([=] {  // one store per 4 KiB page backs it (fresh pages read as zero)
            volatile char* q = (volatile char*)p;
            for (size_t o = n * t / T, hi = n * (t + 1) / T; o < hi; o += 4096) q[o] = 0;
        });
    for (auto& x : th) x.join();
}

void spill_prefault_ahead(rmc_ctx* c, u64 f1) {
    SpillState& X = c->spill;
    if (f1 <= X.faulted) return;
    const u64 f0 = X.faulted;
    X.faulted = f1;
    X.ahead = std::thread([&X, f0, f1] {
        prefault(X.h_parent + f0, (f1 - f0) * 8);
        prefault(X.h_act + f0, f1 - f0);
    });
}

// Move the trace links of the device-resident states [base, a) to the host
// and shift [a, count) to the start of the window.  (With the links in HBM the
// window is a ring and nothing ever moves: see the launch loop.)
int spill_to(rmc_ctx* c, u64 a, u64 count) {
    SpillState& X = c->spill;
    const u64 n = a - X.base;
    if (!n) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    const u64 W = (u64)c->NW * 4;
    u64* hp = X.h_parent + X.base;
    uint8_t* ha = X.h_act + X.base;
    if (X.ahead.joinable()) X.ahead.join();
    if (a > X.faulted) {  // what the background touch did not reach
        const u64 f0 = std::max(X.faulted, X.base);
        prefault(X.h_parent + f0, (a - f0) * 8);
        prefault(X.h_act + f0, a - f0);
        X.faulted = a;
    }
    HIPCHK(c, hipMemcpyAsync(hp, X.parent, n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(ha, X.act, n, hipMemcpyDeviceToHost, c->st));
    if (X.h_state) {  // verification: the states too (the window's first n are [base, a))
        HIPCHK(c, hipMemcpyAsync(X.h_state + X.base * (u64)c->NW, X.store, n * W, hipMemcpyDeviceToHost, c->st));
        X.hcopied = a;
    }
    // shift in pieces of at most n states: no piece overlaps its own destination,
    // and stream order keeps every source read before a later piece overwrites it
    const u64 m = count - a;
    for (u64 off = 0; off < m; off += n) {
        const u64 k = std::min(n, m - off);
        HIPCHK(c, hipMemcpyAsync((char*)X.store + off * W, (char*)X.store + (n + off) * W, k * W,
                                 hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(X.parent + off, X.parent + n + off, k * 8, hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(X.act + off, X.act + n + off, k, hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(X.foot + off, X.foot + n + off, k * 8, hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(X.cls + off, X.cls + n + off, k, hipMemcpyDeviceToDevice, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    spill_rebase(c, a);
    // the next spill takes at most a window's worth: back those pages while the
    // device expands
    spill_prefault_ahead(c, std::min(X.total_cap, a + X.win));
    c->res.spilled += n;
    c->res.spills += 1;
    c->res.spill_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// ---- verification + spill --------------------------------------------------------
// Full-state verification compares every fingerprint hit with the stored state
// that owns the slot.  A spilled search overwrites (ring) or drops (shifted
// window) the device copies of old states, so each state is copied to a host
// mirror before its device copy goes, and a hit on such an owner is parked by
// the expansion kernel (B.hbuf) and compared after the launch with the owner's
// host copy (k_verify_host).  Most duplicates are of recent states, so few hits
// take that path.
int verify_spill_reserve(rmc_ctx* c) {
    SpillState& X = c->spill;
    X.hs_bytes = (size_t)X.total_cap * (size_t)c->NW * 4;
    void* m = mmap(nullptr, X.hs_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (m == MAP_FAILED) {
        X.hs_bytes = 0;
        return fail(c, RMC_E_NOMEM, "verification + spill: cannot reserve host address space for the states");
    }
    (void)madvise(m, X.hs_bytes, MADV_HUGEPAGE);
    X.h_state = (u32*)m;
    X.ostage_cap = 1ull << 22;
    c->B.hcap = 1ull << 26;
    if (hipHostMalloc(&X.h_ostage, X.ostage_cap * (u64)c->NW * 4, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&X.d_ostage, X.ostage_cap * (u64)c->NW * 4) != hipSuccess ||
        hipMalloc(&c->B.hbuf, c->B.hcap * 16) != hipSuccess)
        return fail(c, RMC_E_NOMEM, "verification + spill: staging allocation failed");
    return 0;
}

// Ring window: copy the states [hcopied, upto) — all below the launch's frontier,
// so final, and not yet overwritten — to the host mirror (up to two pieces).
int verify_copy_out(rmc_ctx* c, u64 upto) {
    SpillState& X = c->spill;
    const u64 W = (u64)c->NW * 4;
    while (X.hcopied < upto) {
        const u64 i = X.hcopied, sl = i & c->B.wmask;
        const u64 n = std::min(upto - i, X.win - sl);
        HIPCHK(c, hipMemcpyAsync((char*)X.h_state + i * W, (char*)X.store + sl * W, n * W, hipMemcpyDeviceToHost,
                                 c->st));
        X.hcopied = i + n;
    }
    return 0;
}

// The n hits the last launch parked in B.hbuf {parent, owner index | lane << 56}:
// stage the owners' host copies (batches of ostage_cap) and compare on the device.
int verify_host_hits(rmc_ctx* c, u64 n) {
    SpillState& X = c->spill;
    if (n > c->B.hcap) return fail(c, RMC_E_CAPACITY, "verification buffer full");
    std::vector<u64> rec(2 * n);
    HIPCHK(c, hipMemcpyAsync(rec.data(), c->B.hbuf, n * 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    const u64 NW = (u64)c->NW;
    for (u64 off = 0; off < n; off += X.ostage_cap) {
        const u64 m = std::min(X.ostage_cap, n - off);
        for (u64 q = 0; q < m; ++q) {
            const u64 ix = rec[2 * (off + q) + 1] & ((1ull << 56) - 1);
            if (ix >= X.hcopied)
                return fail(c, RMC_E_HIP, "verification: a spilled owner (index " + std::to_string(ix) +
                                              ") has no host copy");
            memcpy(X.h_ostage + q * NW, X.h_state + ix * NW, NW * 4);
        }
        HIPCHK(c, hipMemcpyAsync(X.d_ostage, X.h_ostage, m * NW * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, c->k->verify_host(c->sh.sym, c->P, c->PT, c->B, X.d_ostage, m, off, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));  // the pinned stage is refilled next
    }
    HIPCHK(c, hipMemsetAsync(&c->B.ctr->hcount, 0, 8, c->st));
    c->h_ctr->hcount = 0;
    X.host_hits += n;
    return 0;
}

// The trace link (parent index, action lane) of any stored state.
int read_link(rmc_ctx* c, u64 idx, u64* parent, uint8_t* act) {
    if (c->spill.on && !c->spill.dev_links && idx < c->spill.base) {
        *parent = c->spill.h_parent[idx];
        *act = c->spill.h_act[idx];
        return 0;
    }
    HIPCHK(c, hipMemcpy(parent, c->B.parent + idx, 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(act, c->B.act + idx, 1, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace rmc_host
