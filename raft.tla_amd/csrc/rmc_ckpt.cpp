// rmc_ckpt.cpp — checkpoint / recovery (TLC -checkpoint / -recover).
// File: header, level boundaries, then the stored states, parent refs and lanes
// of levels 1..depth.  The fingerprint set is not written: rmc_recover rebuilds
// it from the states (k_rehash), one pass over the store.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "rmc_ctx.h"

using namespace rmc;
using namespace rmc_host;

namespace {
// The header embeds the ABI structs rmc_config and rmc_result, so its size is
// written too and must match: a struct that grows changes kCkptVersion.
constexpr uint32_t kCkptVersion = 5;  // 3: rmc_result with parked / exchange_wait_seconds; 4: the set holds
                                      // k ^ s values (raft_packed.h Fp), rmc_result with spill_links_on_device;
                                      // 5: rmc_config.set_bytes, rmc_result.verified_spilled
struct CkptHeader {
    char magic[8];
    uint32_t version, nw;
    uint32_t header_bytes, pad_;
    rmc_config cfg;
    uint64_t count, nlevels;
    int32_t depth;
    int32_t shard;   // sharded checkpoint: rank | world << 16 (0: single GPU)
    rmc_result res;
    uint64_t first;  // states are written from this index on (0: all; else the frontier)
    uint64_t slots;  // fingerprint-set slots dumped after the states (first > 0), else 0
};
const char kCkptMagic[8] = {'R', 'M', 'C', 'C', 'K', 'P', 'T', '1'};

bool same_model(const rmc_config& a, const rmc_config& b) {
    return a.n_servers == b.n_servers && a.n_values == b.n_values && a.max_term == b.max_term &&
           a.max_log_len == b.max_log_len && a.max_msgs == b.max_msgs && a.max_dup == b.max_dup &&
           ((a.flags ^ b.flags) & ~RMC_FLAG_SPILL) == 0 && a.invariants == b.invariants && a.seed == b.seed;
}

// Copy n bytes between a device buffer and a file through a pinned bounce buffer.
int move_file(rmc_ctx* c, FILE* f, void* dev, u64 n, bool to_file) {
    const u64 B = 64ull << 20;
    DevScratch<char, true> h;
    HIPCHK(c, h.alloc(B));
    int rc = 0;
    for (u64 off = 0; off < n && !rc; off += B) {
        const u64 k = std::min(B, n - off);
        char* d = (char*)dev + off;
        if (to_file) {
            if (hipMemcpy(h.get(), d, k, hipMemcpyDeviceToHost) != hipSuccess) rc = RMC_E_HIP;
            else if (fwrite(h.get(), 1, k, f) != k) rc = fail(c, RMC_E_IO, "checkpoint write failed");
        } else {
            if (fread(h.get(), 1, k, f) != k) rc = fail(c, RMC_E_IO, "checkpoint file truncated");
            else if (hipMemcpy(d, h.get(), k, hipMemcpyHostToDevice) != hipSuccess) rc = RMC_E_HIP;
        }
    }
    if (rc == RMC_E_HIP) return fail(c, rc, "checkpoint copy failed");
    return rc;
}

// The checkpoint file of this ctx's part: <path> on one GPU, <path>.rank<r>
// for rank r of a sharded search.
std::string shard_path(const rmc_ctx* c, const char* path) {
    if (!c->dist.on || c->dist.world <= 1) return path;
    return std::string(path) + ".rank" + std::to_string(c->dist.rank);
}
}  // namespace

extern "C" {

// Layout: header, level table, parent[0, count), act[0, count), store[first,
// count), then — when the states below `first` have spilled and no longer
// exist — the fingerprint set itself (TLC checkpoints its FPSet too).
int rmc_checkpoint(rmc_ctx* c, const char* path) {
    if (!c || !path) return RMC_E_INVAL;
    if (c->wide) return fail(c, RMC_E_STATE, "checkpoint / recover: not supported on the wide layout");
    if (pred_on(c))
        return fail(c, RMC_E_STATE, "checkpoint: not supported with model-defined invariants set (rmc_set_predicates)");
    if (cons_on(c))
        return fail(c, RMC_E_STATE, "checkpoint: not supported with model-defined constraints set (rmc_set_constraints)");
    if (act_on(c))
        return fail(c, RMC_E_STATE, "checkpoint: not supported with action properties set (rmc_set_actions)");
    if (c->cfg.flags & RMC_FLAG_COVERAGE)
        return fail(c, RMC_E_STATE, "checkpoint: not supported with RMC_FLAG_COVERAGE (the tallies are of whole "
                                    "runs and are not written)");
    if (c->cfg.flags & RMC_FLAG_CONTINUE)
        return fail(c, RMC_E_STATE, "checkpoint: not supported with RMC_FLAG_CONTINUE (the violation tallies are of "
                                    "whole runs and are not written)");
    if (c->level_start.size() < 2 || c->have_target)
        return fail(c, RMC_E_STATE, "checkpoint: needs a BFS stopped at a level boundary without a violation");
    if (c->res.left_on_queue == 0) return fail(c, RMC_E_STATE, "checkpoint: the search is complete");
    if (c->spill.on && c->sh.verify)
        return fail(c, RMC_E_STATE, "checkpoint: not supported with RMC_FLAG_VERIFY_STATES and RMC_FLAG_SPILL "
                                    "(the host copies of the spilled states are not written)");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->st));
    // a sharded search: every rank writes its own part, <path>.rank<r> (collective
    // only in the sense that every rank calls it; the global counts ride in res)
    const std::string file = shard_path(c, path);
    FILE* f = fopen(file.c_str(), "wb");
    if (!f) return fail(c, RMC_E_IO, "checkpoint: cannot create " + file);
    CkptHeader h{};
    h.shard = c->dist.on ? (c->dist.rank | (c->dist.world << 16)) : 0;
    memcpy(h.magic, kCkptMagic, 8);
    h.version = kCkptVersion;
    h.header_bytes = (uint32_t)sizeof(CkptHeader);
    h.nw = (uint32_t)c->NW;
    h.cfg = c->cfg;
    h.count = c->level_start.back();
    h.nlevels = c->level_start.size();
    h.depth = c->res.depth;
    h.res = c->res;
    const u64 base = c->spill.on ? c->spill.base : 0;
    h.first = base ? c->level_start[h.nlevels - 2] : 0;  // >= base at a level boundary
    h.slots = base ? c->table_slots : 0;
    h.pad_ = h.slots ? c->set_epoch : 0;  // the dumped set's epoch tag (0: untagged)
    int rc = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(c->level_start.data(), 8, h.nlevels, f) == h.nlevels
                 ? 0 : fail(c, RMC_E_IO, "checkpoint write failed");
    auto put = [&](const void* p, u64 n) {
        if (!rc && n && fwrite(p, 1, n, f) != n) rc = fail(c, RMC_E_IO, "checkpoint write failed");
    };
    const u64 lb = c->spill.dev_links ? 0 : base;  // links below lb are on the host
    const u64 nd = h.count - lb;
    if (lb) put(c->spill.h_parent, lb * 8);
    if (!rc) rc = move_file(c, f, c->B.parent + lb, nd * 8, true);
    if (lb) put(c->spill.h_act, lb);
    if (!rc) rc = move_file(c, f, c->B.act + lb, nd, true);
    for (u64 i = h.first; !rc && i < h.count;) {  // the ring window: in up to two pieces
        const u64 sl = wslot(c->B, i), n = std::min(h.count - i, c->B.wmask == ~0ull ? h.count - i : c->spill.win - sl);
        rc = move_file(c, f, c->B.store + sl * (u64)c->NW, n * (u64)c->NW * 4, true);
        i += n;
    }
    if (!rc && h.slots) rc = move_file(c, f, c->B.table, h.slots * 8, true);
    if (fclose(f) != 0 && !rc) rc = fail(c, RMC_E_IO, "checkpoint close failed");
    return rc;
}

int rmc_recover(rmc_ctx* c, const char* path) {
    if (!c || !path) return RMC_E_INVAL;
    if (c->wide) return fail(c, RMC_E_STATE, "checkpoint / recover: not supported on the wide layout");
    if (pred_on(c))
        return fail(c, RMC_E_STATE, "recover: not supported with model-defined invariants set (rmc_set_predicates)");
    if (cons_on(c))
        return fail(c, RMC_E_STATE, "recover: not supported with model-defined constraints set (rmc_set_constraints): "
                                    "recovery rebuilds the set from the stored states, without the removed ones' keys");
    if (act_on(c))
        return fail(c, RMC_E_STATE, "recover: not supported with action properties set (rmc_set_actions): the levels "
                                    "before the checkpoint were expanded without them");
    if (c->cfg.flags & RMC_FLAG_COVERAGE)
        return fail(c, RMC_E_STATE, "recover: not supported with RMC_FLAG_COVERAGE (the tallies are of whole runs)");
    if (c->cfg.flags & RMC_FLAG_CONTINUE)
        return fail(c, RMC_E_STATE, "recover: not supported with RMC_FLAG_CONTINUE (the violation tallies are of "
                                    "whole runs)");
    if (c->spill.on && c->sh.verify)
        return fail(c, RMC_E_STATE, "recover: not supported with RMC_FLAG_VERIFY_STATES and RMC_FLAG_SPILL");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const std::string file = shard_path(c, path);
    FILE* f = fopen(file.c_str(), "rb");
    if (!f) return fail(c, RMC_E_IO, "recover: cannot open " + file);
    CkptHeader h{};
    int rc = 0;
    std::vector<u64> ls;
    // the fixed prefix first (magic, version): an older version is refused by
    // name before its differently laid-out remainder is interpreted
    const size_t pre = offsetof(CkptHeader, header_bytes);
    if (fread(&h, pre, 1, f) != 1 || memcmp(h.magic, kCkptMagic, 8) != 0)
        rc = fail(c, RMC_E_IO, "recover: not an rmc checkpoint");
    else if (h.version != kCkptVersion)
        rc = fail(c, RMC_E_IO, "recover: checkpoint format version " + std::to_string(h.version) +
                                   " (this build reads version " + std::to_string(kCkptVersion) +
                                   "); recreate the checkpoint with this build");
    else if (fread((char*)&h + pre, sizeof h - pre, 1, f) != 1 || h.header_bytes != (uint32_t)sizeof(CkptHeader))
        rc = fail(c, RMC_E_IO, "recover: checkpoint header truncated or of another layout");
    else if (h.shard != (c->dist.on ? (c->dist.rank | (c->dist.world << 16)) : 0))
        rc = fail(c, RMC_E_INVAL, "recover: the checkpoint is of another shard layout (rank / world), or of a "
                                  "single-GPU run recovered on a sharded ctx or the reverse");
    else if (h.nw != (uint32_t)c->NW || !same_model(h.cfg, c->cfg))
        rc = fail(c, RMC_E_INVAL, "recover: the checkpoint is of another model (constants, bounds, flags or seed)");
    else if (h.first && (!c->spill.on || h.slots != c->table_slots))
        rc = fail(c, RMC_E_INVAL, "recover: a spilled checkpoint holds the fingerprint set, not the spilled "
                                  "states; recover it with RMC_FLAG_SPILL and the same state_capacity");
    else {
        ls.resize(h.nlevels);
        if (h.nlevels < 2 || fread(ls.data(), 8, h.nlevels, f) != h.nlevels || ls.back() != h.count ||
            h.first > h.count)
            rc = fail(c, RMC_E_IO, "recover: corrupt level table");
    }
    // states [0, s) keep only their trace links, on the host (spill mode, when
    // they do not all fit the window); [s, count) — at least the frontier — go
    // to the device
    u64 s = 0;
    if (!rc) {
        s = h.first ? h.first : (c->spill.on && h.count > c->spill.win) ? ls[ls.size() - 2] : 0;
        const u64 room = c->spill.on ? c->spill.win : c->B.cap;
        if (h.count - s > room || (c->spill.on && h.count > c->spill.total_cap))
            rc = fail(c, RMC_E_CAPACITY, "recover: the checkpoint holds more states than this ctx's capacity");
        if (!rc && !h.first && s && h.count - s >= room)  // no room left to stream the rehash through
            rc = fail(c, RMC_E_CAPACITY, "recover: the frontier fills the device window");
    }
    if (rc) {
        fclose(f);
        return rc;
    }
    if (c->spill.on) {
        if (c->spill.ahead.joinable()) c->spill.ahead.join();  // it may be touching [0, s)
        spill_rebase(c, 0);
        if (!c->spill.dev_links) c->spill.faulted = std::max(c->spill.faulted, s);  // fread backs the links it writes
    }
    const u64 NW = (u64)c->NW, W = NW * 4;
    u32* dstore = c->spill.on ? c->spill.store : c->B.store;
    u64* dparent = c->spill.on ? c->spill.parent : c->B.parent;
    uint8_t* dact = c->spill.on ? c->spill.act : c->B.act;
    auto get = [&](void* p, u64 n) {
        if (!rc && n && fread(p, 1, n, f) != n) rc = fail(c, RMC_E_IO, "checkpoint file truncated");
    };
    HIPCHK(c, launch_fill(c->B.table, c->table_slots * 8, 0, c->st));
    if (c->sh.verify) HIPCHK(c, launch_fill(c->B.sidx, c->table_slots * 8, 0xFF, c->st));
    // footprints are not checkpointed: the recovered frontier is expanded without
    // diamond skipping (FOOT_VALID clear), the levels after it with
    HIPCHK(c, hipMemsetAsync(c->spill.on ? c->spill.foot : c->B.foot, 0,
                             (c->spill.on ? c->spill.win : c->B.cap) * 8, c->st));
    // a dumped set keeps its entries' epoch tag (header pad_); states rehashed
    // below go into an untagged set
    c->set_epoch = h.slots ? std::min<u32>(h.pad_, 255u) : 0u;
    HIPCHK(c, set_fp_salt(*c->k, c->cfg.seed, c->set_epoch, c->st));
    if (int r2 = reset_counters(c, false)) return r2;
    const u64 ls0 = c->spill.dev_links ? 0 : s;  // links below ls0 go to the host
    if (ls0) get(c->spill.h_parent, ls0 * 8);
    if (!rc) rc = move_file(c, f, dparent, (h.count - ls0) * 8, false);
    if (ls0) get(c->spill.h_act, ls0);
    if (!rc) rc = move_file(c, f, dact, h.count - ls0, false);
    if (!h.first && s && !rc) {
        // no set in the file: rehash the states below s through the free part
        // of the window (the frontier is loaded after them, at its start)
        const u64 piece = c->spill.win - (h.count - s);
        u32* area = dstore + (h.count - s) * NW;
        for (u64 p = 0; p < s && !rc; p += piece) {
            const u64 k = std::min(piece, s - p);
            rc = move_file(c, f, area, k * W, false);
            DevBufs T = c->B;
            T.store = (u32*)((uintptr_t)area - (uintptr_t)(p * W));
            T.wmask = ~0ull;  // indexed through the biased pointer, not the ring
            if (!rc) HIPCHK(c, c->k->rehash(c->sh.sym, c->P, c->PT, T, p, p + k, c->st));
            if (!rc) HIPCHK(c, hipStreamSynchronize(c->st));
        }
    }
    if (c->spill.on && c->spill.dev_links) {  // the ring window: state i at slot i & wmask
        const u64 win = c->spill.win;
        for (u64 i = s; !rc && i < h.count;) {
            const u64 sl = i & (win - 1), n = std::min(h.count - i, win - sl);
            rc = move_file(c, f, dstore + sl * NW, n * W, false);
            i += n;
        }
    } else if (!rc) {
        rc = move_file(c, f, dstore, (h.count - s) * W, false);
    }
    if (!rc && h.slots) rc = move_file(c, f, c->B.table, h.slots * 8, false);
    fclose(f);
    if (rc) return rc;
    if (s) spill_rebase(c, s);
    if (!h.slots) HIPCHK(c, c->k->rehash(c->sh.sym, c->P, c->PT, c->B, s, h.count, c->st));
    if (c->sh.verify) HIPCHK(c, c->k->publish(c->sh.sym, c->P, c->PT, c->B, 0, h.count, c->st));
    if (int r2 = read_counters(c)) return r2;
    if (c->h_ctr->table_full) return fail(c, RMC_E_CAPACITY, "recover: fingerprint set full");
    if (c->h_ctr->overflow) return fail(c, RMC_E_IO, "recover: the checkpoint holds duplicate states");
    c->level_start = ls;
    c->res = h.res;
    c->resume = 1;
    c->resume_depth = h.depth;
    return 0;
}

}  // extern "C"
