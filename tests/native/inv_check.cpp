// Host check of the invariant predicates of both layouts against the oracle's
// verdicts, no GPU: the states arrive as raw rmc_state_view records with the
// oracle's mask of violated invariants per state (tests/test_invariants_native.py
// writes both), are encoded with encode_view / encode_wide, and go through the
// host compilation of the kernels' own check_invariants<S, K> (raft_packed.h) and
// wcheck_invariants (raft_wide.h) on the full and, where the state fits, the
// compact record.  Per state and layout: with each single RMC_INV_* bit as the
// mask the result is non-zero exactly when the oracle has that bit, with all ten
// bits it names the oracle's lowest violated bit, and the single-bit results
// agree with the full-mask one.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc -I include inv_check.cpp raft.tla_amd/csrc/rmc_codec.cpp
// Run:   ./a.out <views.bin> <verdicts.bin> <S> <V> <K: 4, 8, or 0 = beyond the packed capacity>
//        (prints "shape ... <states>" per instantiation and "ok <checks>", or the first failure)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rmc_codec.h"

using namespace rmc;
using namespace rmc::wide;
using namespace rmc_host;

static const char* kInv[10] = {"TypeOK", "OneLeaderPerTerm", "LogMatching", "MessagesInv", "LeaderVotesQuorum",
                               "CandidateTermNotInLog", "VotesGrantedInv", "QuorumLogInv", "MoreUpToDateCorrect",
                               "LeaderCompleteness"};

// check(mask) = 0, or 1 + the index of the first violated invariant of the mask
template <class F>
static int compare(const char* what, size_t t, u32 oracle, F check, u64* checks) {
    int first = 0;
    for (int b = 0; b < 10; ++b) {
        const int r = check(1 << b);
        const bool want = (oracle >> b) & 1u;
        if ((r != 0) != want || (r != 0 && r != b + 1)) {
            printf("FAIL %s state %zu: %s alone gives %d, the oracle says %s\n", what, t, kInv[b], r,
                   want ? "violated" : "holds");
            return 1;
        }
        if (r && !first) first = r;
        ++*checks;
    }
    const int all = check(1023);
    const int want = oracle ? __builtin_ctz(oracle) + 1 : 0;
    if (all != want || all != first) {
        printf("FAIL %s state %zu: all ten give %d, the oracle's first violated is %d, the single bits' %d\n", what, t,
               all, want, first);
        return 1;
    }
    ++*checks;
    return 0;
}

template <int S, int K>
static int packed(const std::vector<rmc_state_view>& views, const std::vector<u32>& oracle, int V, u64* checks) {
    Params P{};
    P.V = V;
    for (size_t t = 0; t < views.size(); ++t) {
        u32 p[2 * S + K];
        std::string why;
        if (encode_view(S, K, views[t], p, &why)) { printf("FAIL packed S=%d K=%d state %zu: %s\n", S, K, t, why.c_str()); return 1; }
        u64 w[S];
        u32 m[K];
        for (int i = 0; i < S; ++i) w[i] = (u64)p[2 * i] | ((u64)p[2 * i + 1] << 32);
        for (int q = 0; q < K; ++q) m[q] = p[2 * S + q];
        char what[64];
        snprintf(what, sizeof what, "packed S=%d K=%d V=%d", S, K, V);
        if (compare(what, t, oracle[t], [&](int mask) { P.inv_mask = mask; return check_invariants<S, K, true>(w, m, P); }, checks))
            return 1;
        // the BFS's form (TypeOK without the message entries' values) names the same invariant of the other nine
        P.inv_mask = 1022;
        if (check_invariants<S, K>(w, m, P) != check_invariants<S, K, true>(w, m, P)) {
            printf("FAIL %s state %zu: the two forms of check_invariants differ on the named invariants\n", what, t);
            return 1;
        }
        P.inv_mask = 1;
        if (check_invariants<S, K>(w, m, P) && !check_invariants<S, K, true>(w, m, P)) {
            printf("FAIL %s state %zu: type_ok alone refuses what the complete TypeOK accepts\n", what, t);
            return 1;
        }
    }
    printf("shape packed S=%d K=%d V=%d %zu\n", S, K, V, views.size());
    return 0;
}

static int wide_records(const std::vector<rmc_state_view>& views, const std::vector<u32>& oracle, int S, int V, u64* checks) {
    WModel M{};
    M.S = S;
    M.V = V;
    M.max_term = TMAX;
    M.max_log = LW;
    M.max_msgs = KW;
    M.max_dup = CMAX;
    M.L.init(S);
    size_t compact = 0;
    for (size_t t = 0; t < views.size(); ++t) {
        WState s;
        std::string why;
        if (encode_wide(S, views[t], &s, &why)) { printf("FAIL wide S=%d state %zu: %s\n", S, t, why.c_str()); return 1; }
        char what[64];
        snprintf(what, sizeof what, "wide full S=%d V=%d", S, V);
        if (compare(what, t, oracle[t], [&](int mask) { M.inv_mask = mask; return wcheck_invariants(M, s); }, checks)) return 1;
        if (wnarrow_bits<WStateC>(s)) continue;
        WStateC c;
        wconvert(c, s);
        snprintf(what, sizeof what, "wide compact S=%d V=%d", S, V);
        if (compare(what, t, oracle[t], [&](int mask) { M.inv_mask = mask; return wcheck_invariants(M, c); }, checks)) return 1;
        ++compact;
    }
    printf("shape wide full S=%d V=%d %zu\n", S, V, views.size());
    printf("shape wide compact S=%d V=%d %zu\n", S, V, compact);
    return 0;
}

template <class T>
static bool read_all(const char* path, std::vector<T>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % (long)sizeof(T)) { fclose(f); return false; }
    out->resize((size_t)bytes / sizeof(T));
    const size_t got = out->empty() ? 0 : fread(out->data(), sizeof(T), out->size(), f);
    fclose(f);
    return got == out->size();
}

int main(int argc, char** argv) {
    if (argc != 6) { printf("usage: inv_check <views.bin> <verdicts.bin> <S> <V> <K>\n"); return 2; }
    std::vector<rmc_state_view> views;
    std::vector<u32> oracle;
    if (!read_all(argv[1], &views) || !read_all(argv[2], &oracle) || views.size() != oracle.size() || views.empty()) {
        printf("FAIL the view file is not whole rmc_state_view records (%zu B each), one verdict each\n", sizeof(rmc_state_view));
        return 1;
    }
    const int S = atoi(argv[3]), V = atoi(argv[4]), K = atoi(argv[5]);
    u64 checks = 0;
    int rc = 0;
    switch (K ? S * 10 + K : 0) {
        case 0: break;
        case 24: rc = packed<2, 4>(views, oracle, V, &checks); break;
        case 28: rc = packed<2, 8>(views, oracle, V, &checks); break;
        case 34: rc = packed<3, 4>(views, oracle, V, &checks); break;
        case 38: rc = packed<3, 8>(views, oracle, V, &checks); break;
        case 44: rc = packed<4, 4>(views, oracle, V, &checks); break;
        case 48: rc = packed<4, 8>(views, oracle, V, &checks); break;
        case 54: rc = packed<5, 4>(views, oracle, V, &checks); break;
        case 58: rc = packed<5, 8>(views, oracle, V, &checks); break;
        default: printf("FAIL no packed shape S=%d K=%d\n", S, K); return 1;
    }
    if (rc || wide_records(views, oracle, S, V, &checks)) return 1;
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
