// Host check of the action-coverage classifiers (raft.tla_amd/csrc/rmc_cover.h:
// cover_row on the packed layout, wcover_row on the wide one — the functions
// the coverage kernels k_cover / k_wcover call).  A BFS to fixpoint (or to
// max_levels) on the host with the packed lane code, and again with the wide
// lane code, each lane walk the one its kernel does; every enabled lane is
// tallied in its action's row.  Two independent lane implementations must give
// the same rows, and the caller compares them with the oracle's
// (tests/golden/coverage_tiny2.json).  Also checked on every lane of every
// state: the wide guard-only evaluation (wlane without a successor, what
// k_wcover runs) is W_OFF exactly when the full evaluation is.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc cover_check.cpp
// Run:   ./a.out S V MaxTerm MaxLogLen MaxMsgs MaxDup max_levels   (S = 2 or 3, MaxMsgs <= 4)
// Prints one JSON line; exit status 1 when the layouts disagree.
#include <cstdio>
#include <cstdlib>
#include <unordered_set>
#include <vector>

#include "rmc_cover.h"

using namespace rmc;

struct Tally {
    u64 gen[COV_ROWS] = {};
    u64 distinct = 0, generated = 0, guard_mismatch = 0;
    int depth = 0;
};

template <int S, int K>
static Tally packed_bfs(int V, int mt, int ml, int mm, int md, int max_levels) {
    Params P{};
    P.V = V; P.max_term = mt; P.max_log = ml; P.max_msgs = mm; P.max_dup = md;
    for (int f = 0; f <= 10; ++f) P.off[f] = Lanes<S, K>::off(f);
    fill_lane_desc(P, S);
    Tally o;
    std::vector<u64> W;
    std::vector<u32> M;
    std::unordered_set<u64> seen;
    u64 w0[S];
    u32 m0[K];
    for (int i = 0; i < S; ++i) w0[i] = 1ull | ((u64)NILV << VF_SH);
    for (int q = 0; q < K; ++q) m0[q] = 0;
    seen.insert(state_fp<S, K>(w0, m0).k);
    W.insert(W.end(), w0, w0 + S);
    M.insert(M.end(), m0, m0 + K);
    o.gen[COV_INIT] = 1;
    u64 lo = 0, hi = 1;
    for (o.depth = 1; (max_levels == 0 || o.depth < max_levels) && lo < hi;) {
        for (u64 t = lo; t < hi; ++t) {
            u64 w[S];
            u32 m[K];
            for (int i = 0; i < S; ++i) w[i] = W[t * S + i];
            for (int q = 0; q < K; ++q) m[q] = M[t * K + q];
            const Fp h0 = state_fp<S, K>(w, m);
            for (int lane = 0; lane < P.off[10]; ++lane) {
                Delta d;
                lane_delta<S, K>(w, m, lane, P, d);
                if (!d.en) continue;
                ++o.gen[cover_row<S, K>(P, w, m, lane)];
                Fp h{0, 0};
                if (!delta_fp<S, K>(w, m, h0, d, P, &h)) continue;
                if (!seen.insert(h.k).second) continue;
                u64 wo[S];
                u32 mo[K];
                materialise<S, K>(w, m, d, wo, mo);
                W.insert(W.end(), wo, wo + S);
                M.insert(M.end(), mo, mo + K);
            }
        }
        lo = hi;
        hi = W.size() / S;
        if (hi > lo) ++o.depth;
    }
    o.distinct = W.size() / S;
    for (int r = 0; r < COV_ROWS; ++r) o.generated += o.gen[r];
    return o;
}

template <class St>
static Tally wide_bfs(int S, int V, int mt, int ml, int mm, int md, int max_levels) {
    using namespace rmc::wide;
    WModel M{};
    M.S = S; M.V = V; M.max_term = mt; M.max_log = ml; M.max_msgs = mm; M.max_dup = md;
    M.inv_mask = 0;
    M.L.init(S);
    Tally o;
    std::vector<St> store(1);
    std::unordered_set<u64> seen;
    winit(M, store[0]);
    seen.insert(wfp(store[0], 0, S).k);
    o.gen[COV_INIT] = 1;
    u64 lo = 0, hi = 1;
    for (o.depth = 1; (max_levels == 0 || o.depth < max_levels) && lo < hi;) {
        for (u64 q = lo; q < hi; ++q) {
            const St s = store[q];
            const int nb = s.nmsg;
            // k_wcover's walk: families 0-6, then the bag families over the state's messages
            for (int f = 0; f < 10; ++f) {
                const int l0 = M.L.off[f], l1 = f < 7 ? M.L.off[f + 1] : l0 + nb;
                for (int lane = l0; lane < l1; ++lane) {
                    St t;
                    const int r = wlane(M, s, lane, &t);
                    if ((wlane(M, s, lane, nullptr) == W_OFF) != (r == W_OFF)) ++o.guard_mismatch;
                    if (r == W_OFF) continue;
                    ++o.gen[wcover_row(M, s, lane)];
                    if (r != W_ON || !win_model(M, t)) continue;
                    if (!seen.insert(wfp(t, 0, S).k).second) continue;
                    store.push_back(t);
                }
            }
            // a bag lane beyond the state's messages is never enabled (the walk skips them)
            for (int f = 7; f < 10; ++f)
                if (nb < St::kKW && wlane(M, s, M.L.off[f] + nb, nullptr) != W_OFF) ++o.guard_mismatch;
        }
        lo = hi;
        hi = store.size();
        if (hi > lo) ++o.depth;
    }
    o.distinct = store.size();
    for (int r = 0; r < COV_ROWS; ++r) o.generated += o.gen[r];
    return o;
}

static void print_tally(const char* name, const Tally& t) {
    printf("\"%s\": {\"distinct\": %llu, \"generated\": %llu, \"depth\": %d, \"gen\": [", name,
           (unsigned long long)t.distinct, (unsigned long long)t.generated, t.depth);
    for (int r = 0; r < COV_ROWS; ++r) printf("%s%llu", r ? ", " : "", (unsigned long long)t.gen[r]);
    printf("]}");
}

int main(int argc, char** argv) {
    if (argc < 8) {
        fprintf(stderr, "usage: %s S V MaxTerm MaxLogLen MaxMsgs MaxDup max_levels\n", argv[0]);
        return 2;
    }
    const int S = atoi(argv[1]), V = atoi(argv[2]), mt = atoi(argv[3]), ml = atoi(argv[4]), mm = atoi(argv[5]),
              md = atoi(argv[6]), lv = atoi(argv[7]);
    if ((S != 2 && S != 3) || mm > 4 || ml > 3 || mt > 14 || md > 3) {
        fprintf(stderr, "S must be 2 or 3 and the bounds within the packed K = 4 shape\n");
        return 2;
    }
    const Tally p = S == 2 ? packed_bfs<2, 4>(V, mt, ml, mm, md, lv) : packed_bfs<3, 4>(V, mt, ml, mm, md, lv);
    // the 336-B record holds 4 log entries and 12 messages: every state of these bounds
    const Tally w = wide_bfs<wide::WStateD>(S, V, mt, ml, mm, md, lv);
    bool same = p.distinct == w.distinct && p.generated == w.generated && p.depth == w.depth;
    for (int r = 0; r < COV_ROWS; ++r) same = same && p.gen[r] == w.gen[r];
    printf("{");
    print_tally("packed", p);
    printf(", ");
    print_tally("wide", w);
    printf(", \"same\": %s, \"guard_mismatches\": %llu}\n", same ? "true" : "false",
           (unsigned long long)w.guard_mismatch);
    return same && !w.guard_mismatch ? 0 : 1;
}
