// rmc_dist_comm.cpp — the transport of the sharded BFS (rmc_dist_comm.h): RCCL
// over xGMI (one non-blocking communicator per ctx) or a caller-supplied host
// transport (gloo in the tests, where several ranks share one GPU; every
// collective is then a synchronous host round trip).  Every wait on another
// rank is under a deadline.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>

#include "rmc_dist_comm.h"

using namespace rmc;

namespace rmc_host {

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- deadlines ---------------------------------------------------------------------
// Every wait of the sharded loop on other ranks has a deadline
// (RMC_DIST_TIMEOUT_S, default 300 s): a collective that has not completed in
// time aborts the RCCL communicator (ncclCommAbort also ends the kernels
// waiting inside it) and fails the call on this rank, naming the level, the
// round and the phase, instead of hanging until an outer time limit.  The
// communicator is non-blocking (ncclConfig_t.blocking = 0), so connection
// set-up inside a group call is polled under the same deadline.  A host
// transport applies its own deadline inside its callbacks (rmc.h).
std::string where(const rmc_ctx* c) {
    const DistState& D = c->dist;
    return "rank " + std::to_string(D.rank) + " of " + std::to_string(D.world) + ", level " +
           std::to_string(D.lvl) + ", round " + std::to_string(D.rnd) + ", phase " + D.phase;
}

// ncclCommAbort of a communicator whose peers never connected can itself wait
// on them (the bootstrap of an unfinished init): it runs on a helper thread,
// waited for at most kAbortWait s; past that the call returns and the helper
// is left to the process exit (after a deadline the caller ends the process,
// rmc.h).  Returns whether the abort completed.
static constexpr double kAbortWait = 10.0;
static bool abort_bounded(ncclComm_t comm) {
    auto done = std::make_shared<std::atomic<int>>(0);
    std::thread([comm, done] {
        (void)ncclCommAbort(comm);
        done->store(1);
    }).detach();
    const double t0 = now_s();
    while (!done->load() && now_s() - t0 < kAbortWait) std::this_thread::sleep_for(std::chrono::milliseconds(2));
    return done->load() != 0;
}

// pending: the caller left a communicator it could not abort (communicator init).
static int deadline_fail(rmc_ctx* c, const char* what, int pending = 0) {
    DistState& D = c->dist;
    D.aborted = 1;
    bool aborted = !pending;
    if (D.rccl && D.comm) {
        aborted = abort_bounded(D.comm);
        D.comm = nullptr;
    }
    if (D.rccl) D.abort_pending = aborted ? 0 : 1;
    char t[32];
    snprintf(t, sizeof t, "%g", D.timeout_s);
    return fail(c, RMC_E_HIP, std::string("sharded search: ") + what + " did not complete within the " + t +
                                  " s deadline (RMC_DIST_TIMEOUT_S) at " + where(c) +
                                  (!D.rccl ? "" : aborted ? "; the RCCL communicator was aborted"
                                                          : "; the RCCL communicator's abort is still pending "
                                                            "(end the process)"));
}

// Wait for an event of the exchange path under the deadline: spin first (a
// round's read-back is on the critical path), then back off.
int xwait(rmc_ctx* c, hipEvent_t ev) {
    DistState& D = c->dist;
    const double t0 = now_s();
    for (u64 spin = 0;; ++spin) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady)
            return fail(c, RMC_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e) + " at " + where(c));
        if ((spin & 63) == 0) {
            const double dt = now_s() - t0;
            if (dt > D.timeout_s) return deadline_fail(c, "a wait on the exchange");
            // a level's expansion takes up to tens of ms: poll without sleeping for
            // the first 100 ms (a 20-us sleep wakes 50-80 us late, once per wait),
            // then gently (a stalled peer)
            if (dt > 0.1) std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
    D.wait_seconds += now_s() - t0;
    return 0;
}

// The result of an RCCL call on the non-blocking communicator: ncclInProgress
// is polled (ncclCommGetAsyncError) until the call is enqueued, under the deadline.
static int nccl_done(rmc_ctx* c, ncclResult_t r, const char* what) {
    DistState& D = c->dist;
    if (r == ncclInProgress || (r == ncclSuccess && D.nonblocking)) {
        const double t0 = now_s();
        for (u64 spin = 0;; ++spin) {
            if (!D.comm) return fail(c, RMC_E_HIP, std::string(what) + ": no communicator at " + where(c));
            if (ncclCommGetAsyncError(D.comm, &r) != ncclSuccess) break;
            if (r != ncclInProgress) break;
            if ((spin & 63) == 0 && now_s() - t0 > D.timeout_s) return deadline_fail(c, what);
            if (spin > 4096) std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    }
    if (r != ncclSuccess) return fail(c, RMC_E_HIP, std::string(what) + ": " + ncclGetErrorString(r) + " at " + where(c));
    return 0;
}

#define NCCLCHK(c, expr)                                              \
    do {                                                              \
        if (int rc_ = nccl_done((c), (expr), #expr)) return rc_;      \
    } while (0)

// The host transport's callbacks return non-zero on failure, their own
// deadline included (rmc.h): the call fails naming where; a callback that
// failed after the deadline had passed is reported as the deadline.
static int host_fail(rmc_ctx* c, const char* what, double t0) {
    const DistState& D = c->dist;
    if (now_s() - t0 >= 0.9 * D.timeout_s) {
        char t[32];
        snprintf(t, sizeof t, "%g", D.timeout_s);
        return fail(c, RMC_E_HIP, std::string("sharded search: the host transport's ") + what +
                                      " did not complete within the " + t + " s deadline (RMC_DIST_TIMEOUT_S) at " +
                                      where(c));
    }
    return fail(c, RMC_E_HIP, std::string("host transport ") + what + " failed at " + where(c));
}

// All-to-all of per-peer byte blocks living on the device, on the exchange
// stream: block p of the send side is sbuf + soff[p] (scnt[p] bytes) for rank
// p; block p of the receive side lands at rbuf + roff[p] (rcnt[p] bytes) from
// rank p.
int a2a(rmc_ctx* c, const void* sbuf, const u64* soff, const u64* scnt, void* rbuf, const u64* roff, const u64* rcnt) {
    DistState& D = c->dist;
    const int W = D.world;
    if (D.rccl) {
        bool any = false;
        for (int p = 0; p < W; ++p) any |= scnt[p] || rcnt[p];
        if (!any) return 0;
        NCCLCHK(c, ncclGroupStart());
        for (int p = 0; p < W; ++p) {
            if (scnt[p]) {
                const ncclResult_t r = ncclSend((const char*)sbuf + soff[p], scnt[p], ncclUint8, p, D.comm, D.xs);
                if (r != ncclSuccess && r != ncclInProgress) {
                    (void)ncclGroupEnd();
                    return nccl_done(c, r, "ncclSend");
                }
            }
            if (rcnt[p]) {
                const ncclResult_t r = ncclRecv((char*)rbuf + roff[p], rcnt[p], ncclUint8, p, D.comm, D.xs);
                if (r != ncclSuccess && r != ncclInProgress) {
                    (void)ncclGroupEnd();
                    return nccl_done(c, r, "ncclRecv");
                }
            }
        }
        NCCLCHK(c, ncclGroupEnd());
        return 0;
    }
    u64 st = 0, rt = 0;
    for (int p = 0; p < W; ++p) { st += scnt[p]; rt += rcnt[p]; }
    D.stage_send.resize(std::max<u64>(st, 1));
    D.stage_recv.resize(std::max<u64>(rt, 1));
    u64 o = 0;
    for (int p = 0; p < W; ++p) {
        if (scnt[p])
            HIPCHK(c, hipMemcpyAsync(D.stage_send.data() + o, (const char*)sbuf + soff[p], scnt[p], hipMemcpyDeviceToHost,
                                     D.xs));
        o += scnt[p];
    }
    HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
    if (int rc = xwait(c, D.ev_h)) return rc;
    const double th = now_s();
    if (D.host.alltoallv(D.host.user, D.stage_send.data(), scnt, D.stage_recv.data(), rcnt))
        return host_fail(c, "alltoallv", th);
    o = 0;
    for (int p = 0; p < W; ++p) {
        if (rcnt[p])
            HIPCHK(c, hipMemcpyAsync((char*)rbuf + roff[p], D.stage_recv.data() + o, rcnt[p], hipMemcpyHostToDevice, D.xs));
        o += rcnt[p];
    }
    HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
    return xwait(c, D.ev_h);
}

// All-to-all of `per` u64 per peer between device buffers (the count rows).
int a2a_u64(rmc_ctx* c, const u64* send, u64* recv, u64 per) {
    DistState& D = c->dist;
    if (D.world == 1) {  // a world of one: the row to itself, no collective
        HIPCHK(c, hipMemcpyAsync(recv, send, per * 8, hipMemcpyDeviceToDevice, D.xs));
        return 0;
    }
    if (D.rccl) {
        NCCLCHK(c, ncclAllToAll(send, recv, per, ncclUint64, D.comm, D.xs));
        return 0;
    }
    std::vector<u64> off((size_t)D.world), cnt((size_t)D.world, per * 8);
    for (int p = 0; p < D.world; ++p) off[(size_t)p] = (u64)p * per * 8;
    return a2a(c, send, off.data(), cnt.data(), recv, off.data(), cnt.data());
}

// All-gather of `bytes` host bytes per rank into all (world * bytes, rank order).
int allgather(rmc_ctx* c, const void* mine, u64 bytes, void* all) {
    DistState& D = c->dist;
    if (!D.rccl) {
        const double th = now_s();
        if (D.host.allgather(D.host.user, mine, bytes, all)) return host_fail(c, "allgather", th);
        return 0;
    }
    const bool big = bytes > D.ag_cap;  // rows are small: the staging buffer is allocated once
    void* d_buf = D.ag_dev;
    if (big) HIPCHK(c, hipMallocAsync(&d_buf, bytes * (u64)(D.world + 1), D.xs));
    char* d_in = (char*)d_buf + bytes * (u64)D.world;
    HIPCHK(c, hipMemcpyAsync(d_in, mine, bytes, hipMemcpyHostToDevice, D.xs));
    NCCLCHK(c, ncclAllGather(d_in, d_buf, bytes, ncclUint8, D.comm, D.xs));
    HIPCHK(c, hipMemcpyAsync(all, d_buf, bytes * (u64)D.world, hipMemcpyDeviceToHost, D.xs));
    if (big) HIPCHK(c, hipFreeAsync(d_buf, D.xs));
    HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
    return xwait(c, D.ev_h);
}

// All-gather of this rank's device counters (the level statistics), after
// every kernel of the level on both streams.
int allgather_counters(rmc_ctx* c, Counters* rows) {
    DistState& D = c->dist;
    HIPCHK(c, hipEventRecord(D.ev_c, c->st));
    HIPCHK(c, hipStreamWaitEvent(D.xs, D.ev_c, 0));
    const u64 bytes = sizeof(Counters);
    if (D.rccl) {
        NCCLCHK(c, ncclAllGather(c->B.ctr, D.ag_dev, bytes, ncclUint8, D.comm, D.xs));
        HIPCHK(c, hipMemcpyAsync(rows, D.ag_dev, bytes * (u64)D.world, hipMemcpyDeviceToHost, D.xs));
        HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
        return xwait(c, D.ev_h);
    }
    Counters mine;
    HIPCHK(c, hipMemcpyAsync(&mine, c->B.ctr, bytes, hipMemcpyDeviceToHost, D.xs));
    HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
    if (int rc = xwait(c, D.ev_h)) return rc;
    const double th = now_s();
    if (D.host.allgather(D.host.user, &mine, bytes, rows)) return host_fail(c, "allgather", th);
    return 0;
}

// Replicated level: every rank's records (n[p] of them, rb bytes each) into
// D.rep_buf, contiguous in rank order; this rank's own block is copied locally.
int gather_level(rmc_ctx* c, const std::vector<u64>& n, u64 rb) {
    DistState& D = c->dist;
    const int W = D.world, me = D.rank;
    std::vector<u64> off((size_t)W + 1, 0);
    for (int p = 0; p < W; ++p) off[(size_t)p + 1] = off[(size_t)p] + n[(size_t)p];
    char* dst = (char*)D.rep_buf;
    if (n[(size_t)me])
        HIPCHK(c, hipMemcpyAsync(dst + off[(size_t)me] * rb, D.rep_send, n[(size_t)me] * rb, hipMemcpyDeviceToDevice,
                                 D.xs));
    if (W == 1) return 0;
    if (D.rccl) {
        bool any = false;
        for (int p = 0; p < W; ++p) any |= p != me && (n[(size_t)p] || n[(size_t)me]);
        if (!any) return 0;
        NCCLCHK(c, ncclGroupStart());
        for (int p = 0; p < W; ++p) {
            if (p == me) continue;
            ncclResult_t r = ncclSuccess;
            if (n[(size_t)me]) r = ncclSend(D.rep_send, n[(size_t)me] * rb, ncclUint8, p, D.comm, D.xs);
            if ((r == ncclSuccess || r == ncclInProgress) && n[(size_t)p])
                r = ncclRecv(dst + off[(size_t)p] * rb, n[(size_t)p] * rb, ncclUint8, p, D.comm, D.xs);
            if (r != ncclSuccess && r != ncclInProgress) {
                (void)ncclGroupEnd();
                return nccl_done(c, r, "ncclSend/ncclRecv (level all-gather)");
            }
        }
        NCCLCHK(c, ncclGroupEnd());
        return 0;
    }
    // host transport: this rank's block to every peer (the block repeated per destination)
    const u64 mine = n[(size_t)me] * rb;
    std::vector<u64> scnt((size_t)W), rcnt((size_t)W);
    for (int p = 0; p < W; ++p) {
        scnt[(size_t)p] = p == me ? 0 : mine;
        rcnt[(size_t)p] = p == me ? 0 : n[(size_t)p] * rb;
    }
    D.stage_send.resize(std::max<u64>(mine * (u64)(W - 1), 1));
    D.stage_recv.resize(std::max<u64>((off[(size_t)W] - n[(size_t)me]) * rb, 1));
    if (mine) HIPCHK(c, hipMemcpyAsync(D.stage_send.data(), D.rep_send, mine, hipMemcpyDeviceToHost, D.xs));
    HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
    if (int rc = xwait(c, D.ev_h)) return rc;
    for (int q = 1; q < W - 1; ++q) memcpy(D.stage_send.data() + (u64)q * mine, D.stage_send.data(), mine);
    const double th = now_s();
    if (D.host.alltoallv(D.host.user, D.stage_send.data(), scnt.data(), D.stage_recv.data(), rcnt.data()))
        return host_fail(c, "alltoallv (level all-gather)", th);
    u64 o = 0;
    for (int p = 0; p < W; ++p) {
        if (rcnt[(size_t)p])
            HIPCHK(c, hipMemcpyAsync(dst + off[(size_t)p] * rb, D.stage_recv.data() + o, rcnt[(size_t)p],
                                     hipMemcpyHostToDevice, D.xs));
        o += rcnt[(size_t)p];
    }
    HIPCHK(c, hipEventRecord(D.ev_h, D.xs));
    return xwait(c, D.ev_h);
}

// The communicator of this rank (D.rank of D.world) from the id every rank
// shares.  On failure the caller frees the sharded state (free_dist).
int comm_init(rmc_ctx* c, const uint8_t* rccl_id) {
    DistState& D = c->dist;
    const int rank = D.rank, world = D.world;
    ncclUniqueId u;
    memcpy(&u, rccl_id, sizeof u);
    // non-blocking (RMC_DIST_NCCL_BLOCKING=1: the blocking mode, A/B): every
    // call is polled under the deadline, connection set-up included
    D.nonblocking = 1;
    if (const char* e = getenv("RMC_DIST_NCCL_BLOCKING")) D.nonblocking = atoi(e) ? 0 : 1;
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = D.nonblocking ? 0 : 1;
    // The whole set-up — the init call and, on the non-blocking communicator,
    // its completion — runs on a helper thread (on this ctx's device) that
    // lives until it is complete (RCCL's group state of a call is the calling
    // thread's), waited for here under the deadline: the call does not
    // promise to return at once for every bootstrap state (a peer that never
    // connects).  On expiry the helper, which owns the communicator, aborts it
    // itself once it leaves its poll loop (no other thread frees it while the
    // helper may still be polling it); this thread waits for that, bounded
    // (kAbortWait), and a call that never returns is left to the process exit.
    struct Init {
        std::atomic<int> done{0}, quit{0}, aborted{0};
        std::atomic<ncclComm_t> comm{nullptr};
        ncclResult_t r = ncclSuccess;
    };
    auto in = std::make_shared<Init>();
    const int dev = c->cfg.device;
    const bool nb = D.nonblocking != 0;
    std::thread([in, world, u, rank, cfg, dev, nb]() mutable {
        (void)hipSetDevice(dev);
        ncclComm_t cm = nullptr;
        ncclResult_t r = ncclCommInitRankConfig(&cm, world, u, rank, &cfg);
        in->comm.store(cm);
        while (nb && r == ncclInProgress && cm && !in->quit.load()) {
            ncclResult_t a = ncclSuccess;
            if (ncclCommGetAsyncError(cm, &a) != ncclSuccess) break;
            r = a;
            if (r == ncclInProgress) std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        if (in->quit.load() && cm) {  // the waiting thread gave up: the owner aborts
            (void)ncclCommAbort(cm);
            in->aborted.store(1);
        }
        in->r = r;
        in->done.store(1);
    }).detach();
    const double t_init = now_s();
    while (!in->done.load()) {
        if (now_s() - t_init > D.timeout_s) {
            in->quit.store(1);
            const double t_q = now_s();
            while (!in->done.load() && now_s() - t_q < kAbortWait)
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
            const bool returned = in->comm.load() != nullptr;
            bool aborted = in->aborted.load() != 0;
            if (in->done.load() && !aborted && returned) {
                // the helper completed the init just before it saw quit: it has
                // left the communicator, so it is aborted here
                aborted = abort_bounded(in->comm.load());
            }
            D.comm = nullptr;  // never touched again by this thread
            return deadline_fail(c,
                                 returned ? "ncclCommInitRankConfig (waiting for every rank)"
                                          : "ncclCommInitRankConfig (the call has not returned)",
                                 !returned || aborted ? 0 : 1);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    D.comm = in->comm.load();
    ncclResult_t r = in->r;
    if (r != ncclSuccess && r != ncclInProgress) {
        if (D.comm) (void)abort_bounded(D.comm);
        D.comm = nullptr;
        return fail(c, RMC_E_HIP, std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r));
    }
    return nccl_done(c, r, "ncclCommInitRankConfig (waiting for every rank)");
}

void comm_close(rmc_ctx* c) {
    DistState& D = c->dist;
    if (D.comm) {  // finalize (polled and bounded on a non-blocking communicator), then destroy
        ncclResult_t r = ncclCommFinalize(D.comm);
        const double t0 = now_s();
        while (r == ncclInProgress && now_s() - t0 < 10.0) {
            if (ncclCommGetAsyncError(D.comm, &r) != ncclSuccess) break;
            if (r == ncclInProgress) std::this_thread::sleep_for(std::chrono::microseconds(50));
        }
        if (r == ncclSuccess) (void)ncclCommDestroy(D.comm);
        else (void)ncclCommAbort(D.comm);
    }
    D.comm = nullptr;
}

}  // namespace rmc_host

extern "C" int rmc_rccl_unique_id(uint8_t id[128]) {
    if (!id) return RMC_E_INVAL;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return RMC_E_HIP;
    static_assert(sizeof u == 128, "ncclUniqueId is 128 bytes");
    memcpy(id, &u, 128);
    return 0;
}
