// Host check of model-defined constraints, no GPU.
//   cons_check plan
//     The in-place compaction of the constraint pass (rmc_cons_plan.h, the arithmetic
//     rmc_dev_cons.h's kernels run), played on the host phase by phase as the kernels run it:
//     tile counts by ballots of 64, their exclusive scan, the head's holes into dst by rank,
//     the tail's movers to dst by rank from the end.  Keep patterns all-kept, none-kept,
//     alternating, only the tail removed, only the head removed and random, at sizes 1, 63,
//     64, 65, 255, 256, 257 and 10,000: afterwards [0, kept) must hold exactly the kept
//     states, each once and with its own links, no source of a move may be a destination,
//     and at most (removed) states move.  Prints "ok <cases>".
//   cons_check verdicts <cfg> <tla> <views.bin> <S> <verdicts.out>
//     The residuals of the model's CONSTRAINTs compiled by the front-end
//     (rmc_constraints_from_files) and evaluated by the interpreter of rmc_pred.h through
//     ViewAcc on raw rmc_state_view records: verdict[t * count + r].  Prints "residual <r>
//     <name>" per residual and "ok <evaluations>"; a refused model prints "refused:
//     <message>" and exits 3.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc -I include cons_check.cpp
//            raft.tla_amd/csrc/rmc_front.cpp raft.tla_amd/csrc/rmc_codec.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rmc_cons_plan.h"
#include "rmc_pred.h"

using namespace rmc;

namespace {

struct Rec {
    uint64_t state, parent;
    uint8_t act, cls;
    uint64_t foot;
};
Rec rec_of(uint64_t id) { return {id * 3 + 1, id * 7 + 2, (uint8_t)(id % 251), (uint8_t)(id % 13), id * 11 + 5}; }
bool same(const Rec& a, const Rec& b) {
    return a.state == b.state && a.parent == b.parent && a.act == b.act && a.cls == b.cls && a.foot == b.foot;
}

// one wave's ballot of keep over positions [base, base + 64) (beyond n: 0)
uint64_t ballot(const std::vector<uint8_t>& keep, uint64_t base) {
    uint64_t b = 0;
    for (int l = 0; l < 64; ++l)
        if (base + l < keep.size() && keep[base + l]) b |= 1ull << l;
    return b;
}
// kept_rank of position p as a thread of its tile computes it (cons_tile_rank)
uint64_t kept_rank_of(const std::vector<uint8_t>& keep, const std::vector<uint64_t>& off, uint64_t p) {
    const uint64_t tile = p / cons::kConsTile, in = p % cons::kConsTile;
    const int wave = (int)(in / 64), lane = (int)(in % 64);
    uint32_t before = 0;
    for (int q = 0; q < wave; ++q) before += (uint32_t)__builtin_popcountll(ballot(keep, tile * cons::kConsTile + 64 * q));
    return cons::kept_rank(off[tile], before + cons::lane_rank(ballot(keep, tile * cons::kConsTile + 64 * wave), lane));
}

int one(const char* pattern, const std::vector<uint8_t>& keep) {
    const uint64_t n = keep.size(), nt = cons::tiles(n);
    std::vector<Rec> a(n);
    for (uint64_t p = 0; p < n; ++p) a[p] = rec_of(p);
    // k_cons: tile counts; the scan
    std::vector<uint32_t> cnt(nt);
    for (uint64_t t = 0; t < nt; ++t)
        for (int w = 0; w < 4; ++w) cnt[t] += (uint32_t)__builtin_popcountll(ballot(keep, t * cons::kConsTile + 64 * w));
    std::vector<uint64_t> off(nt + 1, 0);
    for (uint64_t t = 0; t < nt; ++t) off[t + 1] = off[t] + cnt[t];
    const uint64_t kept = off[nt], removed = n - kept;
    // k_cons_holes
    const uint64_t room = n / 2 + 1, none = ~0ull;
    std::vector<uint64_t> dst(room, none);
    for (uint64_t p = 0; p < cons::tiles(kept) * cons::kConsTile && p < n; ++p) {
        if (!cons::is_hole(p, kept, keep[p] != 0)) continue;
        const uint64_t h = cons::hole_rank(p, kept_rank_of(keep, off, p));
        if (h >= room || dst[h] != none) { printf("FAIL %s n=%llu: hole rank %llu of %llu\n", pattern, (unsigned long long)n, (unsigned long long)h, (unsigned long long)p); return 1; }
        dst[h] = p;
    }
    // k_cons_move (every mover reads its source before any destination is read: they are disjoint)
    uint64_t moved = 0;
    std::vector<uint8_t> written(n, 0);
    for (uint64_t p = (kept / cons::kConsTile) * cons::kConsTile; p < n; ++p) {
        if (!cons::is_mover(p, kept, keep[p] != 0)) continue;
        const uint64_t j = cons::mover_rank(kept, kept_rank_of(keep, off, p));
        if (j >= room || dst[j] == none) { printf("FAIL %s n=%llu: mover rank %llu of %llu\n", pattern, (unsigned long long)n, (unsigned long long)j, (unsigned long long)p); return 1; }
        const uint64_t to = dst[j];
        if (to >= kept || keep[to] || written[to]) { printf("FAIL %s n=%llu: %llu -> %llu is no free hole of the head\n", pattern, (unsigned long long)n, (unsigned long long)p, (unsigned long long)to); return 1; }
        a[to] = a[p];
        written[to] = 1;
        ++moved;
    }
    if (moved > removed || moved > kept) { printf("FAIL %s n=%llu: %llu moved, %llu removed\n", pattern, (unsigned long long)n, (unsigned long long)moved, (unsigned long long)removed); return 1; }
    // [0, kept): a permutation of the kept states, links intact
    std::vector<uint8_t> seen(n, 0);
    for (uint64_t p = 0; p < kept; ++p) {
        const uint64_t id = (a[p].state - 1) / 3;
        if (id >= n || !keep[id] || seen[id] || !same(a[p], rec_of(id))) {
            printf("FAIL %s n=%llu: position %llu holds no kept state with its links\n", pattern, (unsigned long long)n, (unsigned long long)p);
            return 1;
        }
        seen[id] = 1;
    }
    return 0;
}

int plan() {
    const uint64_t sizes[] = {1, 63, 64, 65, 255, 256, 257, 10000};
    int cases = 0;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (uint64_t n : sizes) {
        std::vector<uint8_t> k(n);
        auto run = [&](const char* name) { ++cases; return one(name, k); };
        std::fill(k.begin(), k.end(), 1);
        if (run("all kept")) return 1;
        std::fill(k.begin(), k.end(), 0);
        if (run("none kept")) return 1;
        for (uint64_t p = 0; p < n; ++p) k[p] = p & 1;
        if (run("alternating (odd kept)")) return 1;
        for (uint64_t p = 0; p < n; ++p) k[p] = !(p & 1);
        if (run("alternating (even kept)")) return 1;
        for (uint64_t p = 0; p < n; ++p) k[p] = p < n - n / 3;
        if (run("only the tail removed")) return 1;
        for (uint64_t p = 0; p < n; ++p) k[p] = p >= n / 3;
        if (run("only the head removed")) return 1;
        for (int dens = 1; dens <= 9; dens += 4)
            for (int rep = 0; rep < 4; ++rep) {
                for (uint64_t p = 0; p < n; ++p) {
                    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                    k[p] = (int)(x % 10) < dens;
                }
                if (run("random")) return 1;
            }
    }
    printf("ok %d\n", cases);
    return 0;
}

int verdicts(char** argv) {
    using namespace rmc::pred;
    rmc_predicates* P = nullptr;
    char err[2048] = "";
    if (rmc_constraints_from_files(argv[2], argv[3], nullptr, RMC_FRONT_BUILTIN_RAFT, &P, err, sizeof err)) {
        printf("refused: %s\n", err);
        return 3;
    }
    const Program& g = P->prog;
    for (int r = 0; r < rmc_predicates_count(P); ++r) printf("residual %d %s\n", r, rmc_predicates_name(P, r));
    printf("code %d words, names a server: %d\n", g.n_code, P->names_server);
    std::vector<rmc_state_view> views;
    if (strcmp(argv[4], "-") != 0) {
        FILE* f = fopen(argv[4], "rb");
        if (!f) { printf("FAIL cannot read %s\n", argv[4]); return 1; }
        rmc_state_view v;
        while (fread(&v, sizeof v, 1, f) == 1) views.push_back(v);
        fclose(f);
        if (views.empty() || atoi(argv[5]) != g.n_servers) { printf("FAIL no views, or S differs from the model's %d\n", g.n_servers); return 1; }
    }
    std::vector<uint8_t> out(views.size() * (size_t)g.n_pred);
    for (size_t t = 0; t < views.size(); ++t) {
        int mem[PRED_ROWS];
        for (int r = 0; r < g.n_pred; ++r) out[t * g.n_pred + r] = (uint8_t)run<1>(g.code, g.entry[r], ViewAcc{&views[t]}, mem);
    }
    if (strcmp(argv[6], "-") != 0) {
        FILE* f = fopen(argv[6], "wb");
        if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { printf("FAIL cannot write %s\n", argv[6]); return 1; }
        fclose(f);
    }
    rmc_predicates_free(P);
    printf("ok %zu\n", out.size());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && strcmp(argv[1], "plan") == 0) return plan();
    if (argc == 7 && strcmp(argv[1], "verdicts") == 0) return verdicts(argv);
    printf("usage: cons_check plan | cons_check verdicts <cfg> <tla> <views.bin | -> <S> <verdicts.out | ->\n");
    return 2;
}
