// Host check of the codecs between rmc_state_view and the two state layouts
// (rmc_codec.h) against the kernels' own states: random walks from Init with
// the kernels' lane code (the walks of lane_mask_check.cpp and
// wide_same_check.cpp); every visited state must survive decode -> encode
// unchanged, and encode_view must refuse, with a reason, a view whose bounded
// field is one step past its packed range.
// Build: g++ -O2 -std=c++17 -I raft.tla_amd/csrc -I include codec_check.cpp raft.tla_amd/csrc/rmc_codec.cpp
// Run:   ./a.out <walks> <depth> <wide walks> <wide depth> <seed>
//        (prints "shape ... <states>" per shape and "ok <states checked>", or the first failure)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rmc_codec.h"

using namespace rmc;
using namespace rmc::wide;
using namespace rmc_host;

static u64 rng(u64& x) {
    x += 0x9E3779B97F4A7C15ull;
    return mix64(x);
}

// perturbation kinds seen refused at least once over the whole run
enum Kind {
    P_TERM, P_STATE, P_VOTED, P_COMMIT, P_LOGLEN, P_ENT_TERM, P_ENT_VALUE, P_VOTESET, P_NEXT, P_MATCH, P_MTYPE,
    P_ENDPOINT, P_MTERM, P_COUNT, P_RVQ, P_RVP, P_AEQ, P_AEP, P_DUP, P_KINDS
};
static const char* kKindName[P_KINDS] = {
    "currentTerm", "state", "votedFor", "commitIndex", "log length", "log entry term", "log entry value", "vote set",
    "nextIndex", "matchIndex", "mtype", "message endpoint", "mterm", "count", "RequestVoteRequest fields",
    "RequestVoteResponse fields", "AppendEntriesRequest fields", "AppendEntriesResponse fields", "duplicate message"};
static u64 g_refused[P_KINDS];

// The view v with one field changed must be refused with a reason.
template <class F>
static int refused(int S, int K, const rmc_state_view& v, Kind kind, F change) {
    rmc_state_view b = v;
    change(b);
    u32 out[2 * 5 + 8];
    std::string why;
    if (encode_view(S, K, b, out, &why) != RMC_E_INVAL || why.empty()) {
        printf("FAIL S=%d K=%d: a view with %s out of range was not refused (%s)\n", S, K, kKindName[kind], why.c_str());
        return 1;
    }
    ++g_refused[kind];
    return 0;
}

static int perturb(int S, int K, const rmc_state_view& v) {
#define BAD(kind, stmt) \
    if (refused(S, K, v, kind, [&](rmc_state_view& b) { stmt; })) return 1
    const int i = S - 1;
    BAD(P_TERM, b.currentTerm[i] = 16);
    BAD(P_TERM, b.currentTerm[i] = -1);
    BAD(P_STATE, b.state[i] = 3);
    BAD(P_VOTED, b.votedFor[i] = S);
    BAD(P_VOTED, b.votedFor[i] = -2);
    BAD(P_COMMIT, b.commitIndex[i] = 4);
    BAD(P_LOGLEN, b.log_len[i] = LOG_CAP + 1);
    for (int s = 0; s < S; ++s)
        if (v.log_len[s] > 0) {
            BAD(P_ENT_TERM, b.log[s][v.log_len[s] - 1].term = 16);
            BAD(P_ENT_VALUE, b.log[s][0].value = 2);
        }
    BAD(P_VOTESET, b.votesResponded[i] |= 1u << S);
    BAD(P_VOTESET, b.votesGranted[0] |= 1u << S);
    BAD(P_NEXT, b.nextIndex[i][0] = 5);
    BAD(P_NEXT, b.nextIndex[0][i] = 0);
    BAD(P_MATCH, b.matchIndex[i][0] = 4);
    for (int q = 0; q < v.n_msgs; ++q) {
        BAD(P_MTYPE, b.msgs[q].mtype = 4);
        BAD(P_ENDPOINT, b.msgs[q].msource = S);
        BAD(P_ENDPOINT, b.msgs[q].mdest = -1);
        BAD(P_MTERM, b.msgs[q].mterm = 16);
        BAD(P_COUNT, b.msgs[q].count = 4);
        BAD(P_COUNT, b.msgs[q].count = 0);
        switch (v.msgs[q].mtype) {
            case RVQ:
                BAD(P_RVQ, b.msgs[q].mlastLogTerm = 16);
                BAD(P_RVQ, b.msgs[q].mlastLogIndex = 4);
                break;
            case RVP:
                BAD(P_RVP, b.msgs[q].mlog_len = 4);
                if (v.msgs[q].mlog_len) BAD(P_RVP, b.msgs[q].mlog[0].term = 16);
                break;
            case AEQ:
                BAD(P_AEQ, b.msgs[q].mprevLogIndex = 4);
                BAD(P_AEQ, b.msgs[q].mprevLogTerm = 16);
                BAD(P_AEQ, b.msgs[q].mentries_len = 2);
                BAD(P_AEQ, b.msgs[q].mcommitIndex = 4);
                if (v.msgs[q].mentries_len) BAD(P_AEQ, b.msgs[q].mentries[0].value = 2);
                break;
            default: BAD(P_AEP, b.msgs[q].mmatchIndex = 4);
        }
    }
    if (v.n_msgs > 0 && v.n_msgs < K)  // the same message twice, whatever its count
        BAD(P_DUP, (b.msgs[b.n_msgs] = b.msgs[0], b.msgs[b.n_msgs].count = 1, b.n_msgs += 1));
#undef BAD
    return 0;
}

template <int S, int K>
static int packed(u64 walks, int depth, u64 seed, int V, u64* total) {
    Params P{};
    P.V = V; P.max_term = 6; P.max_log = 3; P.max_msgs = K; P.max_dup = 3;
    for (int f = 0; f <= 10; ++f) P.off[f] = Lanes<S, K>::off(f);
    const int nl = Lanes<S, K>::N, NW = 2 * S + K;
    u64 x = seed, checked = 0;
    for (u64 wk = 0; wk < walks; ++wk) {
        u64 w[S];
        u32 m[K];
        for (int i = 0; i < S; ++i) w[i] = 1ull | ((u64)NILV << VF_SH);
        for (int q = 0; q < K; ++q) m[q] = 0;
        for (int dd = 0; dd < depth; ++dd) {
            u32 p[NW], back[NW];
            int bag = 0;
            for (int i = 0; i < S; ++i) { p[2 * i] = (u32)w[i]; p[2 * i + 1] = (u32)(w[i] >> 32); }
            for (int q = 0; q < K; ++q) { p[2 * S + q] = m[q]; bag += m[q] != 0; }
            rmc_state_view v;
            decode_state(S, K, p, &v);
            std::string why;
            if (v.n_msgs != bag) { printf("FAIL S=%d K=%d walk %llu step %d: n_msgs %d, %d bag slots used\n", S, K, (unsigned long long)wk, dd, v.n_msgs, bag); return 1; }
            if (encode_view(S, K, v, back, &why)) { printf("FAIL S=%d K=%d walk %llu step %d: a decoded state is refused: %s\n", S, K, (unsigned long long)wk, dd, why.c_str()); return 1; }
            for (int q = 0; q < NW; ++q)
                if (back[q] != p[q]) { printf("FAIL S=%d K=%d V=%d walk %llu step %d: word %d is %08x, was %08x\n", S, K, V, (unsigned long long)wk, dd, q, back[q], p[q]); return 1; }
            for (int q = 1; q < K; ++q)
                if (back[2 * S + q] > back[2 * S + q - 1]) { printf("FAIL S=%d K=%d: the encoded bag is not sorted descending\n", S, K); return 1; }
            ++checked;
            if ((checked & 15) == 0 && perturb(S, K, v)) return 1;
            int cand[128], nc = 0;
            for (int lane = 0; lane < nl; ++lane) {
                Delta d;
                lane_delta<S, K>(w, m, lane, P, d);
                if (d.en && delta_in_model<S, K>(m, d, P)) cand[nc++] = lane;
            }
            if (!nc) break;
            Delta d;
            lane_delta<S, K>(w, m, cand[rng(x) % (u64)nc], P, d);
            u64 wo[S];
            u32 mo[K];
            materialise<S, K>(w, m, d, wo, mo);
            for (int i = 0; i < S; ++i) w[i] = wo[i];
            for (int q = 0; q < K; ++q) m[q] = mo[q];
        }
    }
    printf("shape packed S=%d K=%d V=%d %llu\n", S, K, V, (unsigned long long)checked);
    *total += checked;
    return 0;
}

// A narrower record of s, where it holds s, decodes to the view of s itself.
template <class N>
static int narrow(int S, const WState& s, const rmc_state_view& v, u64* narrowed) {
    if (wnarrow_bits<N>(s)) return 0;
    N n;
    wconvert(n, s);
    rmc_state_view vn;
    decode_wide(S, n, &vn);
    if (memcmp(&vn, &v, sizeof v) != 0) { printf("FAIL wide S=%d: a %zu-byte record decodes to another view\n", S, sizeof(N)); return 1; }
    ++*narrowed;
    return 0;
}

static int wide_walks(int S, int walks, int depth, u64 seed, u64* total) {
    WModel M{};  // specs/MCraft.cfg as shipped: |Value| = 2, no CONSTRAINT bounds any field
    M.S = S;
    M.V = 2;
    M.max_term = TMAX;
    M.max_log = LW;
    M.max_msgs = KW;
    M.max_dup = CMAX;
    M.unbounded = 15;
    M.L.init(M.S);
    u64 x = seed, checked = 0, narrowed = 0;
    for (int wk = 0; wk < walks; ++wk) {
        WState s, t, back;
        winit(M, s);
        for (int step = 0; step < depth; ++step) {
            rmc_state_view v;
            decode_wide(S, s, &v);
            std::string why;
            if (encode_wide(S, v, &back, &why)) { printf("FAIL wide S=%d walk %d step %d: a decoded state is refused: %s\n", S, wk, step, why.c_str()); return 1; }
            if (!wsame(back, s) || !wsame(s, back)) { printf("FAIL wide S=%d walk %d step %d: encode(decode(s)) differs from s\n", S, wk, step); return 1; }
            if (narrow<WStateC>(S, s, v, &narrowed) || narrow<WStateD>(S, s, v, &narrowed)) return 1;
            ++checked;
            int on[WLANES_MAX], n_on = 0;
            for (int lane = 0; lane < M.L.off[10]; ++lane)
                if (wlane(M, s, lane, &t) == W_ON) on[n_on++] = lane;
            if (!n_on) break;
            if (wlane(M, s, on[w_rand(x) % (u64)n_on], &t) != W_ON) { printf("FAIL wide: lane not repeatable\n"); return 1; }
            wcopy_state(s, t);
        }
    }
    if (!narrowed) { printf("FAIL wide S=%d: no state fitted a narrower record\n", S); return 1; }
    printf("shape wide S=%d %llu\n", S, (unsigned long long)checked);
    *total += checked;
    return 0;
}

int main(int argc, char** argv) {
    const u64 walks = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1500;
    const int depth = argc > 2 ? atoi(argv[2]) : 60;
    const int wwalks = argc > 3 ? atoi(argv[3]) : 300;
    const int wdepth = argc > 4 ? atoi(argv[4]) : 14;
    const u64 seed = argc > 5 ? strtoull(argv[5], nullptr, 10) : 1;
    u64 n = 0;
    for (int V = 1; V <= 2; ++V)
        if (packed<2, 4>(walks, depth, seed, V, &n) || packed<2, 8>(walks, depth, seed + 1, V, &n) ||
            packed<3, 4>(walks, depth, seed + 2, V, &n) || packed<3, 8>(walks, depth, seed + 3, V, &n) ||
            packed<4, 4>(walks, depth, seed + 4, V, &n) || packed<4, 8>(walks, depth, seed + 5, V, &n) ||
            packed<5, 4>(walks, depth, seed + 6, V, &n) || packed<5, 8>(walks, depth, seed + 7, V, &n))
            return 1;
    for (int k = 0; k < P_KINDS; ++k)
        if (!g_refused[k]) { printf("FAIL no walk reached a view to perturb in %s\n", kKindName[k]); return 1; }
    for (int S : {2, 3, 5})
        if (wide_walks(S, wwalks, wdepth, seed + 8 + (u64)S, &n)) return 1;
    printf("ok %llu\n", (unsigned long long)n);
    return 0;
}
