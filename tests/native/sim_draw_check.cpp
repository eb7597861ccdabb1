// Host print-out of the wide simulators' draws (raft_wide.h w_rand, uniform_draw,
// tlc_draw) for tests/test_sim_rules.py, which asserts that the Python
// restatement (tests/sim_rules.py) returns the same picks and leaves the stream
// in the same position.  For (S, V) in {(2,1), (3,1), (3,2), (5,2)}: random sets
// of enabled lanes (ClientRequest lanes with v >= V never enabled, message
// families up to a random bag size), random sets of excluded lanes, a stream
// position, then the real draws.
// Build: g++ -O2 -std=c++17 -I raft.tla_amd/csrc sim_draw_check.cpp
// Run:   ./a.out <cases per (S, V)> <seed>
// Lines: "stream <seed> <behaviour> <draw> x4"
//        "uni <S> <V> <rs> <en words> <excl words> <pick> <rs after>"
//        "tlc <S> <V> <rs> <en words> <pick> <rs after>"        (hex but S, V, pick)
#include <cstdio>
#include <cstdlib>

#include "raft_wide.h"

using namespace rmc;
using namespace rmc::wide;

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    u64 x = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    constexpr int NC = WLMASK;
    for (int t = 0; t < 16; ++t) {
        const u64 seed = t < 2 ? (u64)t : w_rand(x), b = t < 4 ? (u64)t : w_rand(x) >> (t * 4);
        u64 rs = mix64(seed ^ (b * 0xD1B54A32D192ED03ull));
        printf("stream %llx %llx", (unsigned long long)seed, (unsigned long long)b);
        for (int d = 0; d < 4; ++d) printf(" %llx", (unsigned long long)w_rand(rs));
        printf("\n");
    }
    const int sv[4][2] = {{2, 1}, {3, 1}, {3, 2}, {5, 2}};
    for (const auto& m : sv) {
        const int S = m[0], V = m[1];
        WLanes L;
        L.init(S);
        const int nl = L.off[10], o4 = L.off[4], o5 = L.off[5], o7 = L.off[7], o8 = L.off[8], o9 = L.off[9];
        for (int t = 0; t < cases; ++t) {
            u64 en[NC] = {}, excl[NC] = {};
            const u64 dens = w_rand(x) % 5, xdens = w_rand(x) % 4;  // dens 0: few lanes, now and then none
            const int nmsg = (int)(w_rand(x) % 12);
            for (int lane = 0; lane < nl; ++lane) {
                if (lane >= o7 && (lane - (lane < o8 ? o7 : lane < o9 ? o8 : o9)) >= nmsg) continue;
                if (lane >= o4 && lane < o5 && (lane - o4) % VMAX >= V) continue;
                if (w_rand(x) % 8 < 2 * dens) en[lane >> 6] |= 1ull << (lane & 63);
                if (w_rand(x) % 4 < xdens) excl[lane >> 6] |= 1ull << (lane & 63);
            }
            if (t % 7 == 3)  // every enabled lane excluded
                for (int c = 0; c < NC; ++c) excl[c] |= en[c];
            u64 rs = w_rand(x);
            printf("uni %d %d %llx", S, V, (unsigned long long)rs);
            for (int c = 0; c < NC; ++c) printf(" %llx", (unsigned long long)en[c]);
            for (int c = 0; c < NC; ++c) printf(" %llx", (unsigned long long)excl[c]);
            int pick = uniform_draw<NC>(en, excl, rs);
            printf(" %d %llx\n", pick, (unsigned long long)rs);
            rs = w_rand(x);
            printf("tlc %d %d %llx", S, V, (unsigned long long)rs);
            for (int c = 0; c < NC; ++c) printf(" %llx", (unsigned long long)en[c]);
            pick = tlc_draw<NC>(en, L, V, rs);
            printf(" %d %llx\n", pick, (unsigned long long)rs);
        }
    }
    return 0;
}
