// Host check of the wide layout's SYMMETRY code (raft_wide.h: wcomp_srv_perm,
// wcomp_msg_perm, wfp_perm, wsig_base, wsignatures, wsig_rank, wcanon_ties, wcanon,
// wcanon_succ, wsame_perm, wsame_orbit), no GPU.
//
// The states arrive as raw rmc_state_view records with the oracle's orbit number per
// state (tests/test_wide_symmetry_native.py writes both) and are encoded with
// encode_wide.  Checked:
//   * wcanon's key (k and s) is equal exactly when the orbit numbers are equal, over
//     all pairs of the file (and k alone separates the orbits too);
//   * wsame_orbit(a, b) is the oracle's orbit equality over all pairs, and the same
//     with a narrowed into the compact and the depth-sized record where it fits;
//   * the key does not depend on the record type (full, compact, depth-sized);
//   * wfp_perm under the identity is wfp;
//   * for every lane of every state with a successor the full record holds:
//     wcanon_succ(successor, the parent's signature bases, WDelta.srv) is wcanon of the
//     successor (the expansion kernel's path), and a successor that wsame finds equal to
//     its parent has its parent's key.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc -I include wide_canon_check.cpp raft.tla_amd/csrc/rmc_codec.cpp
// Run:   ./a.out <views.bin> <orbits.bin> <S> <V>
//        (prints "shape wide S=.. <states> tied .. successors .. tied .. orbits .. narrow .. .." and
//        "ok <checks>", or the first failure)
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rmc_codec.h"

using namespace rmc;
using namespace rmc::wide;
using namespace rmc_host;

typedef std::pair<u64, u32> Key;
static Key key_of(const Fp& h) { return Key(h.k, h.s); }

template <class St>
static bool ties_of(const St& s, int S) {
    u64 base[WS];
    wsig_bases(s, S, base);
    WSig sg;
    wsignatures(s, base, S, sg);
    u32 lo, tc;
    return wsig_rank(sg, S, &lo, &tc);
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
    if (argc != 5) {
        printf("usage: wide_canon_check <views.bin> <orbits.bin> <S> <V>\n");
        return 2;
    }
    std::vector<rmc_state_view> views;
    std::vector<u32> orbit;
    if (!read_all(argv[1], &views) || !read_all(argv[2], &orbit) || views.size() != orbit.size() || views.empty()) {
        printf("FAIL the view file is not whole rmc_state_view records (%zu B each), one orbit number each\n", sizeof(rmc_state_view));
        return 1;
    }
    WModel M{};
    M.S = atoi(argv[3]);
    M.V = atoi(argv[4]);
    M.max_term = TMAX;
    M.max_log = LW;
    M.max_msgs = KW;
    M.max_dup = CMAX;
    M.unbounded = 15;
    M.L.init(M.S);
    const int S = M.S;
    if (S < 2 || S > WS) { printf("FAIL no wide shape S=%d\n", S); return 1; }
    const u64 salt = 0;
    const size_t n = views.size();
    std::vector<WState> st(n);
    std::vector<Key> keys(n);
    u64 checks = 0, tied = 0, succ = 0, succ_tied = 0, narrow_c = 0, narrow_d = 0;
    for (size_t t = 0; t < n; ++t) {
        std::string why;
        if (encode_wide(S, views[t], &st[t], &why)) { printf("FAIL wide S=%d state %zu: %s\n", S, t, why.c_str()); return 1; }
        const WState& s = st[t];
        const Fp key = wcanon(s, salt, S);
        keys[t] = key_of(key);
        tied += ties_of(s, S) ? 1 : 0;
        u32 id = 0;
        for (int i = 0; i < S; ++i) id |= (u32)i << (3 * i);
        if (key_of(wfp_perm(s, id, S, salt)) != key_of(wfp(s, salt, S))) {
            printf("FAIL wide S=%d state %zu: wfp_perm under the identity is not wfp\n", S, t);
            return 1;
        }
        ++checks;
        // the narrower records: the same key, the same orbit
        if (!wnarrow_bits<WStateC>(s)) {
            WStateC c;
            wconvert(c, s);
            if (key_of(wcanon(c, salt, S)) != keys[t] || !wsame_orbit(c, s, S) || !wsame_orbit(s, c, S)) {
                printf("FAIL wide S=%d state %zu: the compact record has another key or orbit\n", S, t);
                return 1;
            }
            ++narrow_c;
            ++checks;
        }
        if (!wnarrow_bits<WStateD>(s)) {
            WStateD d;
            wconvert(d, s);
            if (key_of(wcanon(d, salt, S)) != keys[t] || !wsame_orbit(d, s, S) || !wsame_orbit(s, d, S)) {
                printf("FAIL wide S=%d state %zu: the depth-sized record has another key or orbit\n", S, t);
                return 1;
            }
            ++narrow_d;
            ++checks;
        }
        // the expansion's path, lane by lane
        u64 base0[WS];
        wsig_bases(s, S, base0);
        WState u;
        for (int lane = 0; lane < M.L.off[10]; ++lane) {
            WDelta dl;
            if (wlane(M, s, lane, &u, false, &dl) != W_ON) continue;
            const Fp want = wcanon(u, salt, S), got = wcanon_succ(u, base0, dl.srv, salt, S);
            if (key_of(got) != key_of(want)) {
                printf("FAIL wide S=%d state %zu lane %d: wcanon_succ %016llx:%08x, wcanon of the successor %016llx:%08x\n", S, t,
                       lane, (unsigned long long)got.k, got.s, (unsigned long long)want.k, want.s);
                return 1;
            }
            if (wsame(s, u, S) && key_of(want) != keys[t]) {
                printf("FAIL wide S=%d state %zu lane %d: a stuttering successor has another key\n", S, t, lane);
                return 1;
            }
            if ((key_of(want) == keys[t]) != wsame_orbit(s, u, S)) {
                printf("FAIL wide S=%d state %zu lane %d: the successor's key equals its parent's %s wsame_orbit\n", S, t, lane,
                       key_of(want) == keys[t] ? "without" : "against");
                return 1;
            }
            ++succ;
            succ_tied += ties_of(u, S) ? 1 : 0;
            checks += 3;
        }
    }
    // all pairs: equal key <=> equal orbit, through the two maps
    std::map<u32, size_t> first_of_orbit;
    std::map<Key, size_t> first_of_key;
    std::map<u64, size_t> first_of_k;
    for (size_t t = 0; t < n; ++t) {
        const size_t a = first_of_orbit.emplace(orbit[t], t).first->second;
        if (keys[a] != keys[t]) {
            printf("FAIL wide S=%d: states %zu and %zu are one orbit (%u) with keys %016llx:%08x and %016llx:%08x (an orbit split)\n",
                   S, a, t, orbit[t], (unsigned long long)keys[a].first, keys[a].second, (unsigned long long)keys[t].first,
                   keys[t].second);
            return 1;
        }
        const size_t b = first_of_key.emplace(keys[t], t).first->second;
        const size_t c = first_of_k.emplace(keys[t].first, t).first->second;
        if (orbit[b] != orbit[t] || orbit[c] != orbit[t]) {
            const size_t o = orbit[b] != orbit[t] ? b : c;
            printf("FAIL wide S=%d: states %zu and %zu of orbits %u and %u share the key %016llx (two orbits merged)\n", S, o, t,
                   orbit[o], orbit[t], (unsigned long long)keys[t].first);
            return 1;
        }
        checks += n;
    }
    // all pairs: wsame_orbit is the oracle's orbit equality
    for (size_t a = 0; a < n; ++a)
        for (size_t b = 0; b < n; ++b) {
            const bool got = wsame_orbit(st[a], st[b], S), want = orbit[a] == orbit[b];
            if (got != want) {
                printf("FAIL wide S=%d: wsame_orbit(%zu, %zu) is %d, the oracle's orbits %u and %u\n", S, a, b, (int)got, orbit[a],
                       orbit[b]);
                return 1;
            }
            ++checks;
        }
    printf("shape wide S=%d %zu tied %llu successors %llu tied %llu orbits %zu narrow %llu %llu\n", S, n, (unsigned long long)tied,
           (unsigned long long)succ, (unsigned long long)succ_tied, first_of_orbit.size(), (unsigned long long)narrow_c,
           (unsigned long long)narrow_d);
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
