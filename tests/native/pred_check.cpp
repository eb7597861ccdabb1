// Host check of model-defined invariants, no GPU: the front-end compiles the INVARIANTs
// of a model that are none of the ten compiled-in ones (rmc_predicates_from_files), and
// the interpreter of rmc_pred.h evaluates every one of them on raw rmc_state_view records
// (tests/test_predicates_native.py writes them) through each of its state accessors: the
// view itself, the packed words of the model's shape, and the full, compact and
// depth-sized wide records where the state fits them.  The accessors must agree state by
// state; the verdicts of the view accessor are written out for the test to compare with
// the oracle's twins.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc -I include pred_check.cpp
//            raft.tla_amd/csrc/rmc_front.cpp raft.tla_amd/csrc/rmc_codec.cpp
// Run:   ./a.out <cfg> <tla> <views.bin | -> <S> <K: 4, 8, or 0 = beyond the packed capacity> <verdicts.out | ->
//        Prints "predicate <p> <name>" per compiled predicate, "shape ... <states>" per
//        accessor and "ok <evaluations>"; a refused model prints "refused: <message>" and
//        exits 3; a disagreement prints FAIL and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rmc_codec.h"
#include "rmc_pred.h"

using namespace rmc;
using namespace rmc::pred;
using namespace rmc::wide;
using namespace rmc_host;

template <class Acc>
static void eval_all(const Program& g, const Acc& a, uint8_t* out) {
    int mem[PRED_ROWS];
    for (int p = 0; p < g.n_pred; ++p) out[p] = (uint8_t)run<1>(g.code, g.entry[p], a, mem);
}

static int differ(const char* what, size_t t, const Program& g, const uint8_t* want, const uint8_t* got) {
    for (int p = 0; p < g.n_pred; ++p)
        if (want[p] != got[p]) {
            printf("FAIL %s state %zu predicate %d: %d, the view gives %d\n", what, t, p, got[p], want[p]);
            return 1;
        }
    return 0;
}

template <int S, int K>
static int packed(const Program& g, const std::vector<rmc_state_view>& views, const std::vector<uint8_t>& want,
                  unsigned long long* evals) {
    char what[64];
    snprintf(what, sizeof what, "packed S=%d K=%d", S, K);
    for (size_t t = 0; t < views.size(); ++t) {
        u32 p[2 * S + K];
        std::string why;
        if (encode_view(S, K, views[t], p, &why)) { printf("FAIL %s state %zu: %s\n", what, t, why.c_str()); return 1; }
        uint8_t got[PRED_MAX];
        eval_all(g, PackedAcc<S, K>{p}, got);
        if (differ(what, t, g, &want[t * g.n_pred], got)) return 1;
        *evals += g.n_pred;
    }
    printf("shape %s %zu\n", what, views.size());
    return 0;
}

template <class Rec>
static int narrow(const char* what, const Program& g, const WState& s, size_t t, const uint8_t* want, size_t* n,
                  unsigned long long* evals) {
    if (wnarrow_bits<Rec>(s)) return 0;
    Rec c;
    wconvert(c, s);
    uint8_t got[PRED_MAX];
    eval_all(g, WideAcc<Rec>{&c, g.n_servers}, got);
    if (differ(what, t, g, want, got)) return 1;
    ++*n;
    *evals += g.n_pred;
    return 0;
}

static int wide_records(const Program& g, const std::vector<rmc_state_view>& views, const std::vector<uint8_t>& want,
                        unsigned long long* evals) {
    size_t full = 0, compact = 0, depth = 0;
    for (size_t t = 0; t < views.size(); ++t) {
        WState s;
        std::string why;
        if (encode_wide(g.n_servers, views[t], &s, &why)) { printf("FAIL wide state %zu: %s\n", t, why.c_str()); return 1; }
        const uint8_t* w = &want[t * g.n_pred];
        if (narrow<WState>("wide full", g, s, t, w, &full, evals) ||
            narrow<WStateC>("wide compact", g, s, t, w, &compact, evals) ||
            narrow<WStateD>("wide depth-sized", g, s, t, w, &depth, evals))
            return 1;
    }
    printf("shape wide full %zu\nshape wide compact %zu\nshape wide depth-sized %zu\n", full, compact, depth);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        printf("usage: pred_check <cfg> <tla> <views.bin | -> <S> <K> <verdicts.out | ->\n");
        return 2;
    }
    rmc_predicates* P = nullptr;
    char err[2048] = "";
    const int rc = rmc_predicates_from_files(argv[1], argv[2], nullptr, RMC_FRONT_BUILTIN_RAFT, &P, err, sizeof err);
    if (rc) {
        printf("refused: %s\n", err);
        return 3;
    }
    const Program& g = P->prog;
    for (int p = 0; p < rmc_predicates_count(P); ++p) printf("predicate %d %s\n", p, rmc_predicates_name(P, p));
    printf("code %d words, names a server: %d\n", g.n_code, P->names_server);
    if (strcmp(argv[3], "-") == 0) {
        rmc_predicates_free(P);
        return 0;
    }
    std::vector<rmc_state_view> views;
    {
        FILE* f = fopen(argv[3], "rb");
        if (!f) { printf("FAIL cannot read %s\n", argv[3]); return 1; }
        rmc_state_view v;
        while (fread(&v, sizeof v, 1, f) == 1) views.push_back(v);
        fclose(f);
    }
    const int S = atoi(argv[4]), K = atoi(argv[5]);
    if (views.empty() || S != g.n_servers) { printf("FAIL no views, or S differs from the model's %d\n", g.n_servers); return 1; }
    std::vector<uint8_t> want(views.size() * (size_t)g.n_pred);
    unsigned long long evals = 0;
    for (size_t t = 0; t < views.size(); ++t) {
        eval_all(g, ViewAcc{&views[t]}, &want[t * g.n_pred]);
        evals += g.n_pred;
    }
    printf("shape view %zu\n", views.size());
    int bad = 0;
    switch (K ? S * 10 + K : 0) {
        case 0: break;
        case 24: bad = packed<2, 4>(g, views, want, &evals); break;
        case 28: bad = packed<2, 8>(g, views, want, &evals); break;
        case 34: bad = packed<3, 4>(g, views, want, &evals); break;
        case 38: bad = packed<3, 8>(g, views, want, &evals); break;
        case 44: bad = packed<4, 4>(g, views, want, &evals); break;
        case 48: bad = packed<4, 8>(g, views, want, &evals); break;
        case 54: bad = packed<5, 4>(g, views, want, &evals); break;
        case 58: bad = packed<5, 8>(g, views, want, &evals); break;
        default: printf("FAIL no packed shape S=%d K=%d\n", S, K); return 1;
    }
    if (bad || wide_records(g, views, want, &evals)) return 1;
    if (strcmp(argv[6], "-") != 0) {
        FILE* f = fopen(argv[6], "wb");
        if (!f || fwrite(want.data(), 1, want.size(), f) != want.size()) { printf("FAIL cannot write %s\n", argv[6]); return 1; }
        fclose(f);
    }
    rmc_predicates_free(P);
    printf("ok %llu\n", evals);
    return 0;
}
