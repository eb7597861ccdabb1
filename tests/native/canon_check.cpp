// Host check of the SYMMETRY canonical keys (raft_packed.h: perm_word, perm_slot,
// sig_base, signatures, sig_rank, canon_ties, canon_sorted, canon_state, canon_delta),
// no GPU.
//
// File mode: the states arrive as raw rmc_state_view records with the oracle's orbit
// number per state (tests/test_symmetry_native.py writes both) and are encoded with
// encode_view.  canon_state's key (k and s) must be equal exactly when the orbit numbers
// are equal, over all pairs of the file.  And for every enabled lane of every state
// whose successor is in the model: canon_delta(parent, delta) is canon_state of the
// materialised successor; canon_delta<.., NOTIE> reports a tie exactly when sig_rank of
// the materialised successor does, and else returns the same key.
//
// Generated mode: per shape random packed states, half of them tie-heavy (servers built
// alike up to the ids they name); every state is permuted by every server permutation,
// written on the decoded fields (bits / setbits, not perm_word / perm_slot), and every
// image must have the state's key; and on a quarter of the states every bit of every field
// that is no server id is flipped in turn, which must change the key.
// Build: g++ -O2 -std=c++17 -fno-strict-aliasing -I raft.tla_amd/csrc -I include canon_check.cpp raft.tla_amd/csrc/rmc_codec.cpp
// Run:   ./a.out <views.bin> <orbits.bin> <S> <V> <K> <MaxTerm> <MaxLog> <MaxMsgs> <MaxDup>
//        ./a.out gen [<states per shape> [<states per S = 5 shape>]]
//        (prints "shape packed S=.. K=.. <states> ..." per shape and "ok <checks>", or the first failure)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "rmc_codec.h"

using namespace rmc;
using namespace rmc_host;

struct Perms {
    u32 code[120];
    int np;
};
static Perms perms_of(int S) {  // lexicographic, the identity first (rmc_api.cpp fill_params)
    Perms pt{};
    int a[5] = {0, 1, 2, 3, 4};
    do {
        u32 c = 0;
        for (int i = 0; i < S; ++i) c |= (u32)a[i] << (3 * i);
        pt.code[pt.np++] = c;
    } while (std::next_permutation(a, a + S));
    return pt;
}

template <int S, int K>
static bool ties_of(const u64 (&w)[S], const u32 (&m)[K]) {
    u64 base[S];
    for (int i = 0; i < S; ++i) base[i] = sig_base<S>(w[i], (u32)i);
    Sig<S> sg;
    signatures<S, K>(base, m, sg);
    u32 lo, tc;
    return sig_rank<S>(sg, &lo, &tc);
}

static void show(const char* what, int S, int K, const u64* w, const u32* m) {
    printf("  %s:", what);
    for (int i = 0; i < S; ++i) printf(" %016llx", (unsigned long long)w[i]);
    printf(" |");
    for (int q = 0; q < K; ++q) printf(" %08x", m[q]);
    printf("\n");
}

// ---- file mode ------------------------------------------------------------------------
template <int S, int K>
static int from_file(const std::vector<rmc_state_view>& views, const std::vector<u32>& orbit, const Params& P0,
                     u64* checks) {
    Params P = P0;
    for (int f = 0; f <= 10; ++f) P.off[f] = Lanes<S, K>::off(f);
    fill_lane_desc(P, S);
    const Perms pt = perms_of(S);
    typedef std::pair<u64, u32> Key;
    std::vector<Key> keys(views.size());
    u64 succ = 0, succ_tied = 0, tied = 0;
    for (size_t t = 0; t < views.size(); ++t) {
        u32 p[2 * S + K];
        std::string why;
        if (encode_view(S, K, views[t], p, &why)) { printf("FAIL packed S=%d K=%d state %zu: %s\n", S, K, t, why.c_str()); return 1; }
        u64 w[S];
        u32 m[K];
        for (int i = 0; i < S; ++i) w[i] = (u64)p[2 * i] | ((u64)p[2 * i + 1] << 32);
        for (int q = 0; q < K; ++q) m[q] = p[2 * S + q];
        const Fp key = canon_state<S, K>(w, m, pt.code, pt.np);
        keys[t] = Key(key.k, key.s);
        tied += ties_of<S, K>(w, m) ? 1 : 0;
        // the incremental path against the materialised successor, lane by lane
        const Fp h0 = state_fp<S, K>(w, m);
        u64 base[S];
        for (int i = 0; i < S; ++i) base[i] = sig_base<S>(w[i], (u32)i);
        for (int lane = 0; lane < Lanes<S, K>::N; ++lane) {
            Delta d;
            lane_delta<S, K>(w, m, lane, P, d);
            Fp h;
            if (!d.en || !delta_fp<S, K>(w, m, h0, d, P, &h)) continue;
            u64 wo[S];
            u32 mo[K];
            materialise<S, K>(w, m, d, wo, mo);
            const Fp want = canon_state<S, K>(wo, mo, pt.code, pt.np);
            const Fp got = canon_delta<S, K>(w, m, base, d, pt.code, pt.np);
            if (got.k != want.k || got.s != want.s) {
                printf("FAIL packed S=%d K=%d state %zu lane %d: canon_delta %016llx:%08x, canon_state of the successor %016llx:%08x\n",
                       S, K, t, lane, (unsigned long long)got.k, got.s, (unsigned long long)want.k, want.s);
                show("parent", S, K, w, m);
                show("successor", S, K, wo, mo);
                return 1;
            }
            int flag = 0;
            const Fp nt = canon_delta<S, K, true>(w, m, base, d, pt.code, pt.np, &flag);
            const bool tie = ties_of<S, K>(wo, mo);
            if ((flag != 0) != tie) {
                printf("FAIL packed S=%d K=%d state %zu lane %d: canon_delta<NOTIE> says %s, sig_rank of the successor %s\n", S, K,
                       t, lane, flag ? "tied" : "not tied", tie ? "ties" : "does not tie");
                show("parent", S, K, w, m);
                return 1;
            }
            if (!tie && (nt.k != want.k || nt.s != want.s)) {
                printf("FAIL packed S=%d K=%d state %zu lane %d: canon_delta<NOTIE> %016llx:%08x without a tie, canon_state %016llx:%08x\n",
                       S, K, t, lane, (unsigned long long)nt.k, nt.s, (unsigned long long)want.k, want.s);
                show("parent", S, K, w, m);
                return 1;
            }
            ++succ;
            succ_tied += tie ? 1 : 0;
            *checks += 3;
        }
    }
    // all pairs: equal key <=> equal orbit, through the two maps (and k alone separates the orbits too)
    std::map<u32, size_t> first_of_orbit;
    std::map<Key, size_t> first_of_key;
    std::map<u64, size_t> first_of_k;
    for (size_t t = 0; t < views.size(); ++t) {
        const size_t a = first_of_orbit.emplace(orbit[t], t).first->second;
        if (keys[a] != keys[t]) {
            printf("FAIL packed S=%d K=%d: states %zu and %zu are one orbit (%u) with keys %016llx:%08x and %016llx:%08x (an orbit split)\n",
                   S, K, a, t, orbit[t], (unsigned long long)keys[a].first, keys[a].second, (unsigned long long)keys[t].first,
                   keys[t].second);
            return 1;
        }
        const size_t b = first_of_key.emplace(keys[t], t).first->second;
        const size_t c = first_of_k.emplace(keys[t].first, t).first->second;
        if (orbit[b] != orbit[t] || orbit[c] != orbit[t]) {
            const size_t o = orbit[b] != orbit[t] ? b : c;
            printf("FAIL packed S=%d K=%d: states %zu and %zu of orbits %u and %u share the key %016llx (two orbits merged)\n", S, K,
                   o, t, orbit[o], orbit[t], (unsigned long long)keys[t].first);
            return 1;
        }
        *checks += views.size();  // the pairs (., t) this decides
    }
    printf("shape packed S=%d K=%d %zu tied %llu successors %llu tied %llu orbits %zu\n", S, K, views.size(),
           (unsigned long long)tied, (unsigned long long)succ, (unsigned long long)succ_tied, first_of_orbit.size());
    return 0;
}

// ---- generated mode -------------------------------------------------------------------
static u64 rnd(u64& x) {
    x += 0x9E3779B97F4A7C15ull;
    return mix64(x);
}
static u32 below(u64& x, u32 n) { return (u32)(rnd(x) % n); }

// p: old id -> new id.  Field by field on the decoded word, not perm_word.
template <int S>
static u64 permuted_word(u64 w, const int* p) {
    u64 r = 0;
    r = setbits(r, CT_SH, 4, w_ct(w));
    r = setbits(r, ST_SH, 2, w_st(w));
    r = setbits(r, VF_SH, 3, w_vf(w) == NILV ? NILV : (u32)p[w_vf(w)]);
    r = setbits(r, CI_SH, 2, w_ci(w));
    r = setbits(r, LEN_SH, 2, w_len(w));
    for (u32 x = 0; x < (u32)LOG_CAP; ++x) r = setbits(r, LOG_SH + ENT_W * (int)x, ENT_W, w_ent(w, x));
    for (int j = 0; j < S; ++j) {
        r = setbits(r, SL<S>::VR + p[j], 1, (w_vr<S>(w) >> j) & 1u);
        r = setbits(r, SL<S>::VG + p[j], 1, (w_vg<S>(w) >> j) & 1u);
        r = setbits(r, SL<S>::NI + 2 * p[j], 2, w_ni<S>(w, (u32)j) - 1u);
        r = setbits(r, SL<S>::MI + 2 * p[j], 2, w_mi<S>(w, (u32)j));
    }
    return r;
}
static u32 permuted_slot(u32 sl, const int* p) {
    if (!sl) return 0;
    u64 r = sl;
    r = setbits(r, 2, 3, (u32)p[m_src(sl)]);
    r = setbits(r, 5, 3, (u32)p[m_dst(sl)]);
    return (u32)r;
}

template <int S>
static u64 word_of(u32 ct, u32 st, u32 vf, u32 ci, u32 len, const u32* ent, u32 vr, u32 vg, const u32* ni1, const u32* mi) {
    u64 w = 0;
    w = setbits(w, CT_SH, 4, ct);
    w = setbits(w, ST_SH, 2, st);
    w = setbits(w, VF_SH, 3, vf);
    w = setbits(w, CI_SH, 2, ci);
    w = setbits(w, LEN_SH, 2, len);
    for (u32 x = 0; x < len; ++x) w = setbits(w, LOG_SH + ENT_W * (int)x, ENT_W, ent[x]);
    w = setbits(w, SL<S>::VR, S, vr);
    w = setbits(w, SL<S>::VG, S, vg);
    for (int j = 0; j < S; ++j) {
        w = setbits(w, SL<S>::NI + 2 * j, 2, ni1[j]);
        w = setbits(w, SL<S>::MI + 2 * j, 2, mi[j]);
    }
    return w;
}

template <int K>
static bool put_msg(u32 (&m)[K], int* n, u32 msg, u32 cnt) {  // false: the bag has it already, or is full
    if (*n >= K) return false;
    for (int q = 0; q < *n; ++q)
        if ((m[q] & MSG_MASK) == msg) return false;
    m[(*n)++] = msg | (cnt << 30);
    return true;
}
// type, term and the 18 body bits of a message (every body bit pattern: the key must not care)
static u32 msg_rest(u64& x) { return below(x, 4) | (below(x, 15) << 8) | (below(x, 1u << 18) << 12); }

template <int S, int K>
static void uniform_state(u64& x, u64 (&w)[S], u32 (&m)[K]) {
    for (int i = 0; i < S; ++i) {
        u32 ent[3], ni1[S], mi[S];
        for (int e = 0; e < 3; ++e) ent[e] = below(x, 32);
        for (int j = 0; j < S; ++j) { ni1[j] = below(x, 4); mi[j] = below(x, 4); }
        const u32 vf = below(x, S + 1), ct = below(x, 15), st = below(x, 3), ci = below(x, 4), len = below(x, 4);
        const u32 vr = below(x, 1u << S), vg = below(x, 1u << S);
        w[i] = word_of<S>(ct, st, vf == (u32)S ? NILV : vf, ci, len, ent, vr, vg, ni1, mi);
    }
    for (int q = 0; q < K; ++q) m[q] = 0;
    int n = 0;
    for (u32 want = below(x, K + 1), tries = 0; n < (int)want && tries < 64; ++tries)
        put_msg<K>(m, &n, msg_rest(x) | (below(x, S) << 2) | (below(x, S) << 5), 1 + below(x, 3));
}

// Servers in 1-3 classes; a class shares what a permutation leaves alone, every member
// draws for itself the ids it names.
template <int S, int K>
static void tied_state(u64& x, u64 (&w)[S], u32 (&m)[K]) {
    const int ncls = 1 + (int)below(x, S < 3 ? S : 3);
    int cls[S];
    for (int i = 0; i < S; ++i) cls[i] = (int)below(x, ncls);
    struct Kind { u32 ct, st, vfk, ci, len, ent[3], self_vr, self_vg, n_vr, n_vg, own_ni, own_mi, pni[S], pmi[S]; } kind[3];
    for (int c = 0; c < ncls; ++c) {
        Kind& k = kind[c];
        k.ct = below(x, 15); k.st = below(x, 3); k.vfk = below(x, 3); k.ci = below(x, 4); k.len = below(x, 4);
        for (int e = 0; e < 3; ++e) k.ent[e] = below(x, 32);
        k.self_vr = below(x, 2); k.self_vg = below(x, 2); k.n_vr = below(x, S); k.n_vg = below(x, S);
        k.own_ni = below(x, 4); k.own_mi = below(x, 4);
        for (int j = 0; j < S - 1; ++j) { k.pni[j] = below(x, 4); k.pmi[j] = below(x, 4); }
    }
    for (int i = 0; i < S; ++i) {
        const Kind& k = kind[cls[i]];
        int peers[S] = {};
        int np = 0;
        for (int j = 0; j < S; ++j)
            if (j != i) peers[np++] = j;
        auto shuffle = [&] { for (int a = np - 1; a > 0; --a) std::swap(peers[a], peers[below(x, a + 1)]); };
        shuffle();
        const u32 vf = k.vfk == 0 ? NILV : k.vfk == 1 ? (u32)i : (u32)peers[0];
        shuffle();
        u32 vr = k.self_vr << i, vg = k.self_vg << i;
        for (u32 a = 0; a < k.n_vr; ++a) vr |= 1u << peers[a];
        shuffle();
        for (u32 a = 0; a < k.n_vg; ++a) vg |= 1u << peers[a];
        shuffle();
        u32 ni1[S], mi[S];
        ni1[i] = k.own_ni; mi[i] = k.own_mi;
        for (int a = 0; a < np; ++a) { ni1[peers[a]] = k.pni[a]; mi[peers[a]] = k.pmi[a]; }
        w[i] = word_of<S>(k.ct, k.st, vf, k.ci, k.len, k.ent, vr, vg, ni1, mi);
    }
    for (int q = 0; q < K; ++q) m[q] = 0;
    int n = 0;
    for (u32 tmpl = below(x, 4); tmpl > 0; --tmpl) {
        const int c = (int)below(x, ncls);
        int size = 0;
        for (int i = 0; i < S; ++i) size += cls[i] == c;
        if (n + size > K) break;
        const u32 rest = msg_rest(x), cnt = 1 + below(x, 3), sends = below(x, 2);
        for (int i = 0; i < S; ++i) {
            if (cls[i] != c) continue;
            for (int tries = 0; tries < 8; ++tries) {
                const int j = (i + 1 + (int)below(x, S - 1)) % S;  // a peer
                if (put_msg<K>(m, &n, rest | ((u32)(sends ? i : j) << 2) | ((u32)(sends ? j : i) << 5), cnt)) break;
            }
        }
    }
}

template <int K>
static void sort_bag(u32 (&m)[K]) { std::sort(m, m + K, [](u32 a, u32 b) { return a > b; }); }

template <int S, int K>
static int generated(u64 n_states, u64 seed, u64* checks) {
    const Perms pt = perms_of(S);
    u64 x = seed, tied[2] = {0, 0};
    for (u64 t = 0; t < n_states; ++t) {
        const int heavy = (int)(t & 1);
        u64 w[S];
        u32 m[K];
        if (heavy) tied_state<S, K>(x, w, m);
        else uniform_state<S, K>(x, w, m);
        sort_bag<K>(m);
        tied[heavy] += ties_of<S, K>(w, m) ? 1 : 0;
        const Fp key = canon_state<S, K>(w, m, pt.code, pt.np);
        int p[5] = {0, 1, 2, 3, 4};
        do {
            u64 wp[S];
            u32 mp[K];
            for (int i = 0; i < S; ++i) wp[p[i]] = permuted_word<S>(w[i], p);
            for (int q = 0; q < K; ++q) mp[q] = permuted_slot(m[q], p);
            sort_bag<K>(mp);
            const Fp img = canon_state<S, K>(wp, mp, pt.code, pt.np);
            if (img.k != key.k || img.s != key.s) {
                printf("FAIL packed S=%d K=%d %s state %llu: key %016llx:%08x, its image under (", S, K,
                       heavy ? "tie-heavy" : "uniform", (unsigned long long)t, (unsigned long long)key.k, key.s);
                for (int i = 0; i < S; ++i) printf("%d", p[i]);
                printf(") has %016llx:%08x\n", (unsigned long long)img.k, img.s);
                show("state", S, K, w, m);
                show("image", S, K, wp, mp);
                return 1;
            }
            ++*checks;
        } while (std::next_permutation(p, p + S));
        // Every field counts (a quarter of the states): one bit of one server's term, role,
        // commitIndex, log entries (below Len), vote sets or index pairs flipped, or one bit of
        // one message's type, term, body or count, changes what a permutation cannot change of
        // that server (of the message's sender) and of no other, so the state leaves its orbit
        // and its key must change.  (votedFor and the messages' servers are ids: left alone.)
        if ((t & 7) > 1) continue;
        for (int i = 0; i < S; ++i) {
            for (int b = 0; b < SL<S>::END; ++b) {
                if (b >= VF_SH && b < CI_SH) continue;
                if (b >= LEN_SH && b < LOG_SH) continue;  // (Len: it decides which entry bits are part of the state)
                if (b >= LOG_SH && b < VR_SH && (u32)((b - LOG_SH) / ENT_W) >= w_len(w[i])) continue;
                u64 w2[S];
                for (int j = 0; j < S; ++j) w2[j] = w[j];
                w2[i] ^= 1ull << b;
                const Fp other = canon_state<S, K>(w2, m, pt.code, pt.np);
                if (other.k == key.k) {
                    printf("FAIL packed S=%d K=%d %s state %llu: bit %d of server %d flipped and the key is still %016llx\n", S, K,
                           heavy ? "tie-heavy" : "uniform", (unsigned long long)t, b, i, (unsigned long long)key.k);
                    show("state", S, K, w, m);
                    return 1;
                }
                ++*checks;
            }
        }
        for (int q = 0; q < K; ++q) {
            if (!m[q]) continue;
            for (int b = 0; b < 32; ++b) {
                if (b >= 2 && b < 8) continue;
                u32 m2[K];
                for (int r = 0; r < K; ++r) m2[r] = m[r];
                m2[q] ^= 1u << b;
                bool valid = m_cnt(m2[q]) >= 1;
                for (int r = 0; r < K; ++r) valid &= r == q || !m[r] || (m[r] & MSG_MASK) != (m2[q] & MSG_MASK);
                if (!valid) continue;
                sort_bag<K>(m2);
                const Fp other = canon_state<S, K>(w, m2, pt.code, pt.np);
                if (other.k == key.k) {
                    printf("FAIL packed S=%d K=%d %s state %llu: bit %d of slot %d flipped and the key is still %016llx\n", S, K,
                           heavy ? "tie-heavy" : "uniform", (unsigned long long)t, b, q, (unsigned long long)key.k);
                    show("state", S, K, w, m);
                    return 1;
                }
                ++*checks;
            }
        }
    }
    printf("shape packed S=%d K=%d %llu tied %llu of %llu tie-heavy, %llu of %llu uniform\n", S, K,
           (unsigned long long)n_states, (unsigned long long)tied[1], (unsigned long long)(n_states / 2),
           (unsigned long long)tied[0], (unsigned long long)(n_states - n_states / 2));
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
    u64 checks = 0;
    if (argc >= 2 && !strcmp(argv[1], "gen")) {
        const u64 n = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20000, n5 = argc > 3 ? strtoull(argv[3], nullptr, 10) : 2000;
        if (generated<2, 4>(n, 1, &checks) || generated<2, 8>(n, 2, &checks) || generated<3, 4>(n, 3, &checks) ||
            generated<3, 8>(n, 4, &checks) || generated<4, 4>(n, 5, &checks) || generated<4, 8>(n, 6, &checks) ||
            generated<5, 4>(n5, 7, &checks) || generated<5, 8>(n5, 8, &checks))
            return 1;
        printf("ok %llu\n", (unsigned long long)checks);
        return 0;
    }
    if (argc != 10) {
        printf("usage: canon_check <views.bin> <orbits.bin> <S> <V> <K> <MaxTerm> <MaxLog> <MaxMsgs> <MaxDup> | canon_check gen [n [n5]]\n");
        return 2;
    }
    std::vector<rmc_state_view> views;
    std::vector<u32> orbit;
    if (!read_all(argv[1], &views) || !read_all(argv[2], &orbit) || views.size() != orbit.size() || views.empty()) {
        printf("FAIL the view file is not whole rmc_state_view records (%zu B each), one orbit number each\n", sizeof(rmc_state_view));
        return 1;
    }
    const int S = atoi(argv[3]), K = atoi(argv[5]);
    Params P{};
    P.V = atoi(argv[4]); P.max_term = atoi(argv[6]); P.max_log = atoi(argv[7]); P.max_msgs = atoi(argv[8]); P.max_dup = atoi(argv[9]);
    P.symmetry = 1;
    P.fp_mask = ~0ull;
    int rc = 0;
    switch (S * 10 + K) {
        case 24: rc = from_file<2, 4>(views, orbit, P, &checks); break;
        case 28: rc = from_file<2, 8>(views, orbit, P, &checks); break;
        case 34: rc = from_file<3, 4>(views, orbit, P, &checks); break;
        case 38: rc = from_file<3, 8>(views, orbit, P, &checks); break;
        case 44: rc = from_file<4, 4>(views, orbit, P, &checks); break;
        case 48: rc = from_file<4, 8>(views, orbit, P, &checks); break;
        case 54: rc = from_file<5, 4>(views, orbit, P, &checks); break;
        case 58: rc = from_file<5, 8>(views, orbit, P, &checks); break;
        default: printf("FAIL no packed shape S=%d K=%d\n", S, K); return 1;
    }
    if (rc) return 1;
    printf("ok %llu\n", (unsigned long long)checks);
    return 0;
}
