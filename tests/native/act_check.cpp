// Host check of action properties, no GPU: the front-end compiles the PROPERTY names of a model
// that are of the form [][A]_vars (rmc_actions_from_files), and the two-state interpreter of
// rmc_pred.h evaluates every one of them on raw pairs of rmc_state_view records (current, next;
// tests/test_actions_native.py writes them) through two pairs of accessors: ViewAcc on both
// views — the reference — and, as the device pass does, PackedAcc on the packed words of the
// current state in place with the strided column accessor on the next state's words laid out as
// a thread's LDS column (stride 256).  The stutter rule is applied (violated on next = current is
// holds).  The two must agree pair by pair; the verdicts are written out for the test to compare
// with the oracle's twins.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc -I include act_check.cpp
//            raft.tla_amd/csrc/rmc_front.cpp raft.tla_amd/csrc/rmc_codec.cpp
// Run:   ./a.out <cfg> <tla> <pairs.bin | -> <S> <K: 4 or 8> <verdicts.out | -> [options]
//        options: the front-end options (default RMC_FRONT_BUILTIN_RAFT | RMC_FRONT_ACTIONS); with
//        a value without RMC_FRONT_ACTIONS the model goes through rmc_model_from_files instead.
//        Prints "property <p> <name>" per compiled property and "ok <evaluations>"; a refused
//        model prints "refused: <message>" and exits 3; a disagreement prints FAIL and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rmc_codec.h"
#include "rmc_pred.h"

using namespace rmc;
using namespace rmc::pred;
using namespace rmc_host;

constexpr int kColumn = 256;  // the device block's threads: the stride of a thread's LDS column

template <class A, class B>
static void eval_pair(const Program& g, const A& cur, const B& nxt, bool same, uint8_t* out) {
    int mem[PRED_ROWS];
    for (int p = 0; p < g.n_pred; ++p) {
        int v = run2<1, true>(g.code, g.entry[p], cur, nxt, mem);
        if (v == 1 && same) v = 0;
        out[p] = (uint8_t)v;
    }
}

template <int S, int K>
static int packed(const Program& g, const std::vector<rmc_state_view>& views, const std::vector<uint8_t>& want,
                  unsigned long long* evals) {
    constexpr int NW = 2 * S + K;
    std::vector<u32> column((size_t)NW * kColumn);
    for (size_t t = 0; t + 1 < views.size(); t += 2) {
        u32 cur[NW], nxt[NW];
        std::string why;
        if (encode_view(S, K, views[t], cur, &why) || encode_view(S, K, views[t + 1], nxt, &why)) {
            printf("FAIL packed S=%d K=%d pair %zu: %s\n", S, K, t / 2, why.c_str());
            return 1;
        }
        const int lane = (int)((t / 2) % kColumn);  // every column of the block in turn
        bool same = true;
        for (int q = 0; q < NW; ++q) {
            column[(size_t)q * kColumn + lane] = nxt[q];
            same = same && nxt[q] == cur[q];
        }
        uint8_t got[PRED_MAX];
        eval_pair(g, PackedAcc<S, K>{cur}, PackedAcc<S, K, kColumn>{column.data() + lane}, same, got);
        for (int p = 0; p < g.n_pred; ++p)
            if (got[p] != want[(t / 2) * g.n_pred + p]) {
                printf("FAIL packed S=%d K=%d pair %zu property %d: %d, the views give %d\n", S, K, t / 2, p, got[p],
                       want[(t / 2) * g.n_pred + p]);
                return 1;
            }
        *evals += g.n_pred;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 7 && argc != 8) {
        printf("usage: act_check <cfg> <tla> <pairs.bin | -> <S> <K> <verdicts.out | -> [options]\n");
        return 2;
    }
    const uint32_t options = argc == 8 ? (uint32_t)strtoul(argv[7], nullptr, 0) : (RMC_FRONT_BUILTIN_RAFT | RMC_FRONT_ACTIONS);
    char err[2048] = "";
    if (!(options & RMC_FRONT_ACTIONS)) {
        rmc_config cfg;
        if (rmc_model_from_files(argv[1], argv[2], nullptr, options, &cfg, nullptr, err, sizeof err)) {
            printf("refused: %s\n", err);
            return 3;
        }
        printf("accepted\n");
        return 0;
    }
    rmc_predicates* P = nullptr;
    if (rmc_actions_from_files(argv[1], argv[2], nullptr, options, &P, err, sizeof err)) {
        printf("refused: %s\n", err);
        return 3;
    }
    {
        rmc_config cfg;
        char info[4096] = "";
        if (rmc_model_from_files(argv[1], argv[2], nullptr, options, &cfg, nullptr, info, sizeof info)) {
            printf("FAIL rmc_model_from_files refuses what rmc_actions_from_files accepts: %s\n", info);
            return 1;
        }
        printf("%s\n", info);
    }
    const Program& g = P->prog;
    for (int p = 0; p < rmc_predicates_count(P); ++p) printf("property %d %s\n", p, rmc_predicates_name(P, p));
    int primed = 0;
    for (int q = 0; q < g.n_code; ++q) primed += (g.code[q] & OP_PRIMED) ? 1 : 0;
    printf("code %d words, %d primed reads, names a server: %d\n", g.n_code, primed, P->names_server);
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
    if (views.empty() || views.size() % 2 || S != g.n_servers) {
        printf("FAIL no pairs, or S differs from the model's %d\n", g.n_servers);
        return 1;
    }
    const size_t n = views.size() / 2;
    std::vector<uint8_t> want(n * (size_t)g.n_pred);
    unsigned long long evals = 0;
    for (size_t t = 0; t < n; ++t) {
        const bool same = memcmp(&views[2 * t], &views[2 * t + 1], sizeof(rmc_state_view)) == 0;
        eval_pair(g, ViewAcc{&views[2 * t]}, ViewAcc{&views[2 * t + 1]}, same, &want[t * g.n_pred]);
        evals += g.n_pred;
    }
    int bad = 0;
    switch (S * 10 + K) {
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
    if (bad) return 1;
    if (strcmp(argv[6], "-") != 0) {
        FILE* f = fopen(argv[6], "wb");
        if (!f || fwrite(want.data(), 1, want.size(), f) != want.size()) { printf("FAIL cannot write %s\n", argv[6]); return 1; }
        fclose(f);
    }
    rmc_predicates_free(P);
    printf("ok %llu\n", evals);
    return 0;
}
