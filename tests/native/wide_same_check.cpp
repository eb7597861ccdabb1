// Host check of the wide layout's state equality (raft_wide.h wsame, the
// comparison of full-state verification): random walks from Init with the
// kernels' own lane code on the full record; every visited state that a
// narrower record holds (wnarrow_bits) is converted into it (wconvert) and
// must equal its original, in both argument orders; then the original is
// changed in one semantic field at a time — a term, a role, votedFor,
// commitIndex, a log entry's term or value, a log length, a vote bit, a
// nextIndex / matchIndex cell, each field of a message, a message count, one
// message removed — and every such change must make the two differ.
// Build: g++ -O2 -std=c++17 -I raft.tla_amd/csrc wide_same_check.cpp
// Run:   ./a.out <walks> <depth> <seed>   (prints "ok <checked>" or the first failure)
#include <cstdio>
#include <cstdlib>

#include "raft_wide.h"

using namespace rmc;
using namespace rmc::wide;

static long g_checked = 0;
static int g_walk = 0, g_step = 0;

static int fail(const char* rec, const char* what, int a = -1, int b = -1) {
    printf("FAIL walk %d step %d, %s record: %s [%d][%d]\n", g_walk, g_step, rec, what, a, b);
    return 1;
}

// One mutation of a copy of w must differ from n (in both argument orders).
template <class N, class F>
static int differs(const N& n, const WState& w, const char* rec, const char* what, int a, int b, F mutate) {
    WState m;
    wcopy_state(m, w);
    mutate(m);
    ++g_checked;
    if (wsame(n, m) || wsame(m, n)) return fail(rec, what, a, b);
    return 0;
}

template <class N>
static int check(const WModel& M, const WState& w, const char* rec) {
    if (wnarrow_bits<N>(w)) return 0;  // the record cannot hold this state
    N n;
    wconvert(n, w);
    ++g_checked;
    if (!wsame(n, w) || !wsame(w, n) || !wsame(n, n) || !wsame(w, w)) return fail(rec, "a converted state differs");
    if (!wsame(n, w, M.S) || !wsame(w, n, M.S)) return fail(rec, "a converted state differs over S servers");
#define DIFF(what, a, b, stmt) \
    if (differs(n, w, rec, what, a, b, [&](WState& m) { stmt; })) return 1
    for (int i = 0; i < M.S; ++i) {
        DIFF("currentTerm", i, -1, m.ct[i] += 1);
        DIFF("state", i, -1, m.st[i] = (uint8_t)((m.st[i] + 1) % 3));
        DIFF("votedFor", i, -1, m.vf[i] = m.vf[i] == NIL ? 0 : NIL);
        DIFF("commitIndex", i, -1, m.ci[i] += 1);
        for (int j = 0; j < M.S; ++j) {
            DIFF("votesResponded", i, j, m.vR[i] ^= (uint8_t)(1u << j));
            DIFF("votesGranted", i, j, m.vG[i] ^= (uint8_t)(1u << j));
            DIFF("nextIndex", i, j, m.ni[i][j] += 1);
            DIFF("matchIndex", i, j, m.mi[i][j] += 1);
        }
        for (int x = 0; x < w.len[i]; ++x) {
            DIFF("log term", i, x, m.log[i][x].term += 1);
            DIFF("log value", i, x, m.log[i][x].value ^= 1);
        }
        if (w.len[i] > 0) DIFF("Len(log) - 1", i, -1, (m.len[i] -= 1, m.log[i][m.len[i]] = WEnt{0, 0}));
        if (w.len[i] < LW) DIFF("Len(log) + 1", i, -1, (m.log[i][m.len[i]] = WEnt{1, 0}, m.len[i] += 1));
    }
    for (int q = 0; q < w.nmsg; ++q) {
        DIFF("mtype", q, -1, m.msg[q].type = (uint8_t)((m.msg[q].type + 1) & 3));
        DIFF("mterm", q, -1, m.msg[q].term += 1);
        DIFF("msource", q, -1, m.msg[q].src = (uint8_t)((m.msg[q].src + 1) % M.S));
        DIFF("mdest", q, -1, m.msg[q].dst = (uint8_t)((m.msg[q].dst + 1) % M.S));
        DIFF("message field a", q, -1, m.msg[q].a += 1);
        DIFF("message field b", q, -1, m.msg[q].b += 1);
        DIFF("message field c", q, -1, m.msg[q].c += 1);
        DIFF("message entries + 1", q, -1, (m.msg[q].e[m.msg[q].n] = WEnt{1, 0}, m.msg[q].n += 1));
        for (int x = 0; x < w.msg[q].n; ++x) {
            DIFF("message entry term", q, x, m.msg[q].e[x].term += 1);
            DIFF("message entry value", q, x, m.msg[q].e[x].value ^= 1);
        }
        DIFF("message count", q, -1, m.cnt[q] += 1);
        DIFF("message removed", q, -1, (m.cnt[q] = 1, wbag_remove_at(m, q)));
    }
    if (w.nmsg < KW) DIFF("message added", w.nmsg, -1, (m.msg[m.nmsg].type = RVQ, m.cnt[m.nmsg] = 1, m.nmsg += 1));
#undef DIFF
    return 0;
}

int main(int argc, char** argv) {
    const int walks = argc > 1 ? atoi(argv[1]) : 300;
    const int depth = argc > 2 ? atoi(argv[2]) : 14;
    u64 x = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1;
    WModel M{};
    M.S = 3;
    M.V = 2;
    M.max_term = TMAX;
    M.max_log = LW;
    M.max_msgs = KW;
    M.max_dup = CMAX;
    M.unbounded = 15;
    M.L.init(M.S);
    long narrow_c = 0, narrow_d = 0;
    for (g_walk = 0; g_walk < walks; ++g_walk) {
        WState s, t;
        winit(M, s);
        for (g_step = 0; g_step < depth; ++g_step) {
            if (check<WStateC>(M, s, "compact")) return 1;
            if (check<WStateD>(M, s, "depth-sized")) return 1;
            if (check<WState>(M, s, "full")) return 1;
            narrow_c += !wnarrow_bits<WStateC>(s);
            narrow_d += !wnarrow_bits<WStateD>(s);
            // a uniformly drawn enabled lane whose successor the full record holds
            int on[WLANES_MAX], n_on = 0;
            for (int lane = 0; lane < M.L.off[10]; ++lane)
                if (wlane(M, s, lane, &t) == W_ON) on[n_on++] = lane;
            if (!n_on) break;
            if (wlane(M, s, on[w_rand(x) % (u64)n_on], &t) != W_ON) return fail("full", "lane not repeatable");
            wcopy_state(s, t);
        }
    }
    if (!narrow_c || !narrow_d) {
        printf("FAIL no state fitted a narrower record\n");
        return 1;
    }
    printf("ok %ld\n", g_checked);
    return 0;
}
