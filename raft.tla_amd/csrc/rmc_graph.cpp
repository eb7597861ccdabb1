// rmc_graph.cpp — the state graph of a finished search (rmc.h "state graph export"; DESIGN.md
// "State graph"): rmc_get_levels, rmc_read_states, rmc_find_states, rmc_graph_edges.
//
// Packed layout, single GPU, resident store.  The calls read what the last completed
// rmc_run_bfs left in HBM — the store, the level table, the fingerprint set — through a
// key -> store index lookup: verification's slot -> index array (DevBufs.sidx), which a
// verification run has filled and any other ctx fills at its first graph call with one
// k_publish pass over every stored state (8 B per set slot, freed by rmc_destroy; the next
// rmc_run_bfs invalidates it).  Ranges of any size are served in chunks through per-call
// scratch buffers.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rmc_ctx.h"

using namespace rmc;
using namespace rmc_host;

static_assert(sizeof(rmc_edge) == 24 && sizeof(GraphEdge) == sizeof(rmc_edge), "GraphEdge is rmc_edge");
static_assert(RMC_NO_STATE == ~0ull, "the kernels write ~0 for no state");

namespace {

// States per chunk: of the reads and lookups (staging buffers), and of the edge walk (its
// counts, offsets and — at most 128 lanes a state — edge records).
// RMC_GRAPH_CHUNK (read per call: tests vary it) caps both, so that small models cross chunk
// boundaries too.
constexpr u64 kStateChunk = 1ull << 16, kEdgeChunk = 1ull << 18;
u64 chunk_states(u64 dflt) {
    const char* e = getenv("RMC_GRAPH_CHUNK");
    const long long v = e ? atoll(e) : 0;
    return v >= 1 && (u64)v < dflt ? (u64)v : dflt;
}

// What every call but rmc_get_levels requires of the ctx; `who` names the call.
int graph_ready(rmc_ctx* c, const char* who, bool levels_only) {
    const std::string w = std::string(who) + ": ";
    if (c->dist.on) return fail(c, RMC_E_STATE, w + "a sharded ctx (rmc_shard) holds a part of the graph only");
    if (c->resume)
        return fail(c, RMC_E_STATE, w + "rmc_recover loaded a checkpoint: call rmc_run_bfs before reading the graph");
    if (!c->run_done) return fail(c, RMC_E_STATE, w + "no completed rmc_run_bfs to report");
    if (c->cfg.flags & RMC_FLAG_SPILL)
        return fail(c, RMC_E_STATE, w + "the ctx was created with RMC_FLAG_SPILL: the states must be resident");
    if (c->wide && !levels_only)
        return fail(c, RMC_E_STATE, w + "the packed layout only (this model runs on the wide layout)");
    return 0;
}

// The run's salt and set epoch in the shape's kernels (another ctx of the shape may have set
// its own since), and B.sidx published for every stored state.
int graph_index(rmc_ctx* c, const char* who) {
    HIPCHK(c, set_fp_salt(*c->k, c->run_seed, c->set_epoch, c->st));
    if (c->graph_idx) return 0;
    if (!c->B.sidx && hipMalloc(&c->B.sidx, c->table_slots * 8) != hipSuccess) {
        c->B.sidx = nullptr;
        (void)hipGetLastError();
        return fail(c, RMC_E_NOMEM, std::string(who) + ": device allocation failed (the slot -> state index, " +
                                        std::to_string(c->table_slots * 8) + " bytes: 8 per set slot)");
    }
    HIPCHK(c, launch_fill(c->B.sidx, c->table_slots * 8, 0xFF, c->st));
    HIPCHK(c, hipMemsetAsync(&c->B.ctr->overflow, 0, 4, c->st));
    HIPCHK(c, c->k->publish(c->sh.sym, c->P, c->PT, c->B, 0, c->res.distinct, c->st));
    if (int rc = read_counters(c)) return rc;
    if (c->h_ctr->overflow & 8u)
        return fail(c, RMC_E_HIP, std::string(who) + ": a stored state has no fingerprint slot (index build)");
    c->graph_idx = 1;
    return 0;
}

int encode_all(rmc_ctx* c, const rmc_state_view* states, size_t n, std::vector<u32>* packed) {
    packed->assign(n * (size_t)c->NW, 0u);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_view(c->sh.S, c->sh.K, states[t], packed->data() + t * c->NW, &why))
            return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    return 0;
}

}  // namespace

extern "C" {

int rmc_get_levels(const rmc_ctx* ctx, uint64_t* starts, size_t cap, size_t* n) {
    if (!ctx) return RMC_E_INVAL;
    rmc_ctx* c = const_cast<rmc_ctx*>(ctx);  // (only the message is written)
    if (!n || (cap && !starts)) return fail(c, RMC_E_INVAL, "rmc_get_levels: n or starts is NULL");
    if (int rc = graph_ready(c, "rmc_get_levels", true)) return rc;
    *n = c->level_start.size();
    for (size_t l = 0; l < *n && l < cap; ++l) starts[l] = c->level_start[l];
    return 0;
}

int rmc_read_states(rmc_ctx* c, uint64_t first, size_t n, rmc_state_view* states, uint64_t* keys) {
    if (!c) return RMC_E_INVAL;
    if (n && !states) return fail(c, RMC_E_INVAL, "rmc_read_states: states is NULL");
    if (int rc = graph_ready(c, "rmc_read_states", false)) return rc;
    if (first > c->res.distinct || n > c->res.distinct - first)
        return fail(c, RMC_E_INVAL, "rmc_read_states: [" + std::to_string(first) + ", " + std::to_string(first) + " + " +
                                        std::to_string(n) + ") is beyond the " + std::to_string(c->res.distinct) +
                                        " stored states");
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (keys) HIPCHK(c, set_fp_salt(*c->k, c->run_seed, c->set_epoch, c->st));
    const u64 NW = (u64)c->NW, chunk = std::min<u64>(n, chunk_states(kStateChunk));
    std::vector<u32> recs(chunk * NW);
    DevScratch<u64> d_keys;
    if (keys) HIPCHK(c, d_keys.alloc(chunk));
    for (u64 a = 0; a < n; a += chunk) {
        const u64 m = std::min<u64>(chunk, n - a);
        const u32* src = c->B.store + (first + a) * NW;  // resident: slot = index
        HIPCHK(c, hipMemcpyAsync(recs.data(), src, m * NW * 4, hipMemcpyDeviceToHost, c->st));
        if (keys) {  // the stored records are k_keys' input as they lie
            HIPCHK(c, c->k->keys(c->sh.sym, c->P, c->PT, src, m, d_keys.get(), nullptr, nullptr, c->st));
            HIPCHK(c, hipMemcpyAsync(keys + a, d_keys.get(), m * 8, hipMemcpyDeviceToHost, c->st));
        }
        HIPCHK(c, hipStreamSynchronize(c->st));
        for (u64 t = 0; t < m; ++t) decode_state(c->sh.S, c->sh.K, recs.data() + t * NW, &states[a + t]);
    }
    return 0;
}

int rmc_find_states(rmc_ctx* c, const rmc_state_view* states, size_t n, uint64_t* index) {
    if (!c) return RMC_E_INVAL;
    if (n && (!states || !index)) return fail(c, RMC_E_INVAL, "rmc_find_states: states or index is NULL");
    if (int rc = graph_ready(c, "rmc_find_states", false)) return rc;
    if (c->run_cons)
        return fail(c, RMC_E_STATE, "rmc_find_states: the run had model-defined constraints set (rmc_set_constraints): its set "
                                    "holds the keys of removed states, which no stored state owns");
    if (n == 0) return 0;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const u64 NW = (u64)c->NW, chunk = std::min<u64>(n, chunk_states(kStateChunk));
    std::vector<u32> packed;  // (a view the encoder refuses is refused before anything is launched)
    if (int rc = encode_all(c, states, n, &packed)) return rc;
    if (int rc = graph_index(c, "rmc_find_states")) return rc;
    DevScratch<u32> d_in;
    DevScratch<u64> d_ix;
    HIPCHK(c, d_in.alloc(chunk * NW));
    HIPCHK(c, d_ix.alloc(chunk));
    for (u64 a = 0; a < n; a += chunk) {
        const u64 m = std::min<u64>(chunk, n - a);
        HIPCHK(c, hipMemcpyAsync(d_in.get(), packed.data() + a * NW, m * NW * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, c->k->graph_find(c->sh.sym, c->P, c->PT, c->B, d_in.get(), m, d_ix.get(), c->st));
        HIPCHK(c, hipMemcpyAsync(index + a, d_ix.get(), m * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    return 0;
}

int rmc_graph_edges(rmc_ctx* c, uint64_t lo, uint64_t hi, rmc_edge* out, size_t cap, size_t* n_out) {
    if (!c) return RMC_E_INVAL;
    if (!n_out || (cap && !out)) return fail(c, RMC_E_INVAL, "rmc_graph_edges: n_out or out is NULL");
    *n_out = 0;
    if (int rc = graph_ready(c, "rmc_graph_edges", false)) return rc;
    if (c->run_cons)
        return fail(c, RMC_E_STATE, "rmc_graph_edges: the run had model-defined constraints set (rmc_set_constraints): its set "
                                    "holds the keys of removed states, which no stored state owns");
    if (c->stop)
        return fail(c, RMC_E_STATE,
                    "rmc_graph_edges: the run stopped at a violation or a deadlock, so which states it expanded is "
                    "not a level boundary (run with RMC_FLAG_CONTINUE, or without the invariant)");
    if (lo > hi || hi > c->res.distinct)
        return fail(c, RMC_E_INVAL, "rmc_graph_edges: [" + std::to_string(lo) + ", " + std::to_string(hi) +
                                        ") is beyond the " + std::to_string(c->res.distinct) + " stored states");
    if (lo == hi) return 0;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (int rc = graph_index(c, "rmc_graph_edges")) return rc;
    // the states the run expanded: every level but an unexpanded last one
    const u64 expanded = c->res.distinct - c->res.left_on_queue;
    hi = std::min<u64>(hi, expanded);
    if (lo >= hi) return 0;
    const u64 chunk = std::min<u64>(hi - lo, chunk_states(kEdgeChunk));
    DevScratch<u32> d_cnt;
    DevScratch<u64> d_off;
    DevScratch<unsigned long long> d_err;
    HIPCHK(c, d_cnt.alloc(chunk));
    HIPCHK(c, d_off.alloc(chunk + 1));
    HIPCHK(c, d_err.alloc(1));
    HIPCHK(c, hipMemsetAsync(d_err.get(), 0xFF, 8, c->st));
    GraphEdge* d_out = nullptr;  // grown to the largest chunk's edges
    u64 out_cap = 0, total = 0;
    int rc = 0;
    auto step = [&](u64 a, u64 b) -> int {
        HIPCHK(c, c->k->graph_count(c->P, c->B, a, b, d_cnt.get(), c->st));
        HIPCHK(c, launch_graph_scan(d_cnt.get(), b - a, d_off.get(), c->st));
        u64 ne = 0;
        HIPCHK(c, hipMemcpyAsync(&ne, d_off.get() + (b - a), 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (ne > out_cap) {
            (void)hipFree(d_out);
            d_out = nullptr;
            out_cap = 0;
            HIPCHK(c, hipMalloc(&d_out, ne * sizeof(GraphEdge)));
            out_cap = ne;
        }
        if (ne) {
            HIPCHK(c, c->k->graph_edges(c->sh.sym, c->P, c->PT, c->B, a, b, d_off.get(), d_out, ne, d_err.get(), c->st));
            unsigned long long bad = 0;
            HIPCHK(c, hipMemcpyAsync(&bad, d_err.get(), 8, hipMemcpyDeviceToHost, c->st));
            const u64 room = total < cap ? std::min<u64>(ne, cap - total) : 0;
            if (room)
                HIPCHK(c, hipMemcpyAsync(out + total, d_out, room * sizeof(GraphEdge), hipMemcpyDeviceToHost, c->st));
            HIPCHK(c, hipStreamSynchronize(c->st));
            if (bad != ~0ull)
                return fail(c, RMC_E_HIP, "rmc_graph_edges: the fingerprint set does not hold the successor of stored state " +
                                              std::to_string(bad >> 8) + " through lane " + std::to_string(bad & 255) +
                                              " (a successor of an expanded state within the CONSTRAINT)");
        }
        total += ne;
        return 0;
    };
    for (u64 a = lo; a < hi && !rc; a += chunk) rc = step(a, std::min<u64>(hi, a + chunk));
    (void)hipFree(d_out);
    if (rc) return rc;
    *n_out = (size_t)total;
    return 0;
}

}  // extern "C"
