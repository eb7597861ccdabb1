// rmc_dist_comm.h — the transport under the sharded BFS (rmc_dist.cpp): the
// collectives of the exchange stream D.xs over RCCL or the host transport, and
// the waits on other ranks, each under the deadline (RMC_DIST_TIMEOUT_S): a wait
// that expires aborts the RCCL communicator and fails the call on this rank,
// naming where the loop was (DistState lvl / rnd / phase).
#pragma once
#include "rmc_ctx.h"

namespace rmc_host {

double now_s();
std::string where(const rmc_ctx* c);  // "rank r of W, level l, round k, phase ..."
// Wait for an event of the exchange path (adds to D.wait_seconds).
int xwait(rmc_ctx* c, hipEvent_t ev);
// All-to-all of per-peer byte blocks on the device: block p of the send side is
// sbuf + soff[p] (scnt[p] bytes) for rank p; block p of the receive side lands
// at rbuf + roff[p] (rcnt[p] bytes) from rank p.
int a2a(rmc_ctx* c, const void* sbuf, const rmc::u64* soff, const rmc::u64* scnt, void* rbuf, const rmc::u64* roff,
        const rmc::u64* rcnt);
// All-to-all of `per` u64 per peer between device buffers (the count rows).
int a2a_u64(rmc_ctx* c, const rmc::u64* send, rmc::u64* recv, rmc::u64 per);
// All-gather of `bytes` host bytes per rank into all (world * bytes, rank order).
int allgather(rmc_ctx* c, const void* mine, rmc::u64 bytes, void* all);
// All-gather of this rank's device counters, after every kernel on both streams.
int allgather_counters(rmc_ctx* c, rmc::Counters* rows);
// Replicated level: every rank's records (n[p] of them, rb bytes each) from
// D.rep_send into D.rep_buf, contiguous in rank order.
int gather_level(rmc_ctx* c, const std::vector<rmc::u64>& n, rmc::u64 rb);
// The RCCL communicator: set-up under the deadline (on failure the caller frees
// the sharded state), and finalize-then-destroy.
int comm_init(rmc_ctx* c, const uint8_t* rccl_id);
void comm_close(rmc_ctx* c);

}  // namespace rmc_host
