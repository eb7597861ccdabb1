// Host check of the violation classifiers (raft.tla_amd/csrc/rmc_viol.h:
// classify_violations on the packed layout, wclassify_violations on the wide one —
// the functions the kernels k_violations / k_wviolations call).  A BFS that does
// not stop at a violation, to fixpoint (or to max_levels), on the host with the
// packed lane code and again with the wide lane code; every stored state — the
// seed's and the last, unexpanded level's too — is classified under `mask` and
// tallied as rmc_violations is: first[r], each[r], depth[r].  Two independent
// lane and predicate implementations must agree, and the caller compares them
// with the oracle's (tests/golden/continue_cases.json).  Also checked on every
// state: `first` is the lowest bit of `each`, and `each` is the mask's bits that
// fail under a mask of that bit alone.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc viol_check.cpp
// Run:   ./a.out S V MaxTerm MaxLogLen MaxMsgs MaxDup bug max_levels mask   (S = 2 or 3, MaxMsgs <= 4)
// Prints one JSON line; exit status 1 when the layouts disagree or a state is misclassified.
#include <cstdio>
#include <cstdlib>
#include <unordered_set>
#include <vector>

#include "rmc_viol.h"

using namespace rmc;

struct Tally {
    u64 first[VIOL_INVS] = {}, each[VIOL_INVS] = {};
    int inv_depth[VIOL_INVS] = {};
    u64 states = 0, distinct = 0, generated = 1, misclassified = 0;
    int depth = 0;
    // alone: the bits of the mask that fail when checked on their own, computed by the caller
    void add(const ViolClass& c, u32 alone, int level) {
        const int low = alone ? __builtin_ctz(alone) + 1 : 0;
        if (c.each != alone || c.first != low) ++misclassified;
        if (!c.first) return;
        ++states;
        ++first[c.first - 1];
        for (int r = 0; r < VIOL_INVS; ++r)
            if ((c.each >> r) & 1u) {
                ++each[r];
                if (!inv_depth[r]) inv_depth[r] = level;
            }
    }
};

template <int S, int K>
static Tally packed_bfs(int V, int mt, int ml, int mm, int md, int bug, int max_levels, int mask) {
    Params P{};
    P.V = V; P.max_term = mt; P.max_log = ml; P.max_msgs = mm; P.max_dup = md;
    P.bug_quorum = bug;
    P.inv_mask = mask;
    for (int f = 0; f <= 10; ++f) P.off[f] = Lanes<S, K>::off(f);
    fill_lane_desc(P, S);
    Tally o;
    std::vector<u64> W;
    std::vector<u32> M;
    std::unordered_set<u64> seen;
    auto classify = [&](const u64(&w)[S], const u32(&m)[K], int level) {
        u32 alone = 0;
        Params Q = P;
        for (int r = 0; r < VIOL_INVS; ++r) {
            Q.inv_mask = mask & (1 << r);
            if (Q.inv_mask && check_invariants<S, K>(w, m, Q)) alone |= 1u << r;
        }
        o.add(classify_violations<S, K>(w, m, P), alone, level);
    };
    u64 w0[S];
    u32 m0[K];
    for (int i = 0; i < S; ++i) w0[i] = 1ull | ((u64)NILV << VF_SH);
    for (int q = 0; q < K; ++q) m0[q] = 0;
    seen.insert(state_fp<S, K>(w0, m0).k);
    W.insert(W.end(), w0, w0 + S);
    M.insert(M.end(), m0, m0 + K);
    classify(w0, m0, 1);
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
                ++o.generated;
                Fp h{0, 0};
                if (!delta_fp<S, K>(w, m, h0, d, P, &h)) continue;
                if (!seen.insert(h.k).second) continue;
                u64 wo[S];
                u32 mo[K];
                materialise<S, K>(w, m, d, wo, mo);
                W.insert(W.end(), wo, wo + S);
                M.insert(M.end(), mo, mo + K);
                classify(wo, mo, o.depth + 1);
            }
        }
        lo = hi;
        hi = W.size() / S;
        if (hi > lo) ++o.depth;
    }
    o.distinct = W.size() / S;
    return o;
}

template <class St>
static Tally wide_bfs(int S, int V, int mt, int ml, int mm, int md, int bug, int max_levels, int mask) {
    using namespace rmc::wide;
    WModel M{};
    M.S = S; M.V = V; M.max_term = mt; M.max_log = ml; M.max_msgs = mm; M.max_dup = md;
    M.bug_quorum = bug;
    M.inv_mask = mask;
    M.L.init(S);
    Tally o;
    auto classify = [&](const St& s, int level) {
        u32 alone = 0;
        WModel Q = M;
        for (int r = 0; r < VIOL_INVS; ++r) {
            Q.inv_mask = mask & (1 << r);
            if (Q.inv_mask && wcheck_invariants(Q, s)) alone |= 1u << r;
        }
        o.add(wclassify_violations(M, s), alone, level);
    };
    std::vector<St> store(1);
    std::unordered_set<u64> seen;
    winit(M, store[0]);
    seen.insert(wfp(store[0], 0, S).k);
    classify(store[0], 1);
    u64 lo = 0, hi = 1;
    for (o.depth = 1; (max_levels == 0 || o.depth < max_levels) && lo < hi;) {
        for (u64 q = lo; q < hi; ++q) {
            const St s = store[q];
            for (int f = 0; f < 10; ++f) {
                const int l0 = M.L.off[f], l1 = f < 7 ? M.L.off[f + 1] : l0 + s.nmsg;
                for (int lane = l0; lane < l1; ++lane) {
                    St t;
                    const int r = wlane(M, s, lane, &t);
                    if (r == W_OFF) continue;
                    ++o.generated;
                    if (r != W_ON || !win_model(M, t)) continue;
                    if (!seen.insert(wfp(t, 0, S).k).second) continue;
                    store.push_back(t);
                    classify(t, o.depth + 1);
                }
            }
        }
        lo = hi;
        hi = store.size();
        if (hi > lo) ++o.depth;
    }
    o.distinct = store.size();
    return o;
}

static void print_row(const char* key, const u64* v) {
    printf("\"%s\": [", key);
    for (int r = 0; r < VIOL_INVS; ++r) printf("%s%llu", r ? ", " : "", (unsigned long long)v[r]);
    printf("]");
}

static void print_tally(const char* name, const Tally& t) {
    printf("\"%s\": {\"distinct\": %llu, \"generated\": %llu, \"depth\": %d, \"states\": %llu, \"misclassified\": %llu, ",
           name, (unsigned long long)t.distinct, (unsigned long long)t.generated, t.depth, (unsigned long long)t.states,
           (unsigned long long)t.misclassified);
    print_row("first", t.first);
    printf(", ");
    print_row("each", t.each);
    printf(", \"inv_depth\": [");
    for (int r = 0; r < VIOL_INVS; ++r) printf("%s%d", r ? ", " : "", t.inv_depth[r]);
    printf("]}");
}

int main(int argc, char** argv) {
    if (argc < 10) {
        fprintf(stderr, "usage: %s S V MaxTerm MaxLogLen MaxMsgs MaxDup bug max_levels mask\n", argv[0]);
        return 2;
    }
    const int S = atoi(argv[1]), V = atoi(argv[2]), mt = atoi(argv[3]), ml = atoi(argv[4]), mm = atoi(argv[5]),
              md = atoi(argv[6]), bug = atoi(argv[7]), lv = atoi(argv[8]), mask = atoi(argv[9]);
    if ((S != 2 && S != 3) || mm > 4 || ml > 3 || mt > 14 || md > 3 || (mask & ~1023)) {
        fprintf(stderr, "S must be 2 or 3, the bounds within the packed K = 4 shape, the mask of RMC_INV_* bits\n");
        return 2;
    }
    const Tally p = S == 2 ? packed_bfs<2, 4>(V, mt, ml, mm, md, bug, lv, mask)
                           : packed_bfs<3, 4>(V, mt, ml, mm, md, bug, lv, mask);
    // the 336-B record holds 4 log entries and 12 messages: every state of these bounds
    const Tally w = wide_bfs<wide::WStateD>(S, V, mt, ml, mm, md, bug, lv, mask);
    bool same = p.distinct == w.distinct && p.generated == w.generated && p.depth == w.depth && p.states == w.states;
    for (int r = 0; r < VIOL_INVS; ++r)
        same = same && p.first[r] == w.first[r] && p.each[r] == w.each[r] && p.inv_depth[r] == w.inv_depth[r];
    printf("{");
    print_tally("packed", p);
    printf(", ");
    print_tally("wide", w);
    printf(", \"same\": %s}\n", same ? "true" : "false");
    return same && !p.misclassified && !w.misclassified ? 0 : 1;
}
