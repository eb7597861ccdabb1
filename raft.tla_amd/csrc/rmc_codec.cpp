// rmc_codec.cpp — rmc_state_view <-> packed words / wide records, and the
// SmokeInit sampler (rmc_codec.h): host arithmetic only.
#include "rmc_codec.h"

#include <algorithm>
#include <random>

using namespace rmc;
using namespace rmc::wide;

namespace rmc_host {

int family_of(const Params& P, int lane) {
    if (lane == 255) return -1;
    for (int f = 0; f < 10; ++f)
        if (lane < P.off[f + 1]) return f;
    return -1;
}

// ---- the packed codec --------------------------------------------------------------
int encode_view(int S, int K, const rmc_state_view& v, u32* out, std::string* why) {
    const int VR = VR_SH, VG = VR_SH + S, NI = VR_SH + 2 * S, MI = VR_SH + 4 * S;
    auto bad = [&](const std::string& s) { *why = s; return RMC_E_INVAL; };
    if (v.n_servers != S) return bad("view n_servers differs from config");
    if (v.n_msgs < 0 || v.n_msgs > K) return bad("too many messages for the packed bag");
    for (int i = 0; i < S; ++i) {
        const int len = v.log_len[i];
        if (v.currentTerm[i] < 0 || v.currentTerm[i] > 15) return bad("currentTerm out of packed range");
        if (v.state[i] < 0 || v.state[i] > 2) return bad("state out of range");
        if (v.votedFor[i] < -1 || v.votedFor[i] >= S) return bad("votedFor out of range");
        if (v.commitIndex[i] < 0 || v.commitIndex[i] > 3) return bad("commitIndex out of packed range");
        if (len < 0 || len > LOG_CAP) return bad("log length out of packed range");
        u64 w = (u64)v.currentTerm[i] | ((u64)v.state[i] << ST_SH) |
                ((u64)(v.votedFor[i] < 0 ? NILV : (u32)v.votedFor[i]) << VF_SH) | ((u64)v.commitIndex[i] << CI_SH) |
                ((u64)len << LEN_SH);
        for (int x = 0; x < len; ++x) {
            const rmc_entry e = v.log[i][x];
            if (e.term < 0 || e.term > 15 || e.value < 0 || e.value > 1) return bad("log entry out of range");
            w |= (u64)(e.term | (e.value << 4)) << (LOG_SH + ENT_W * x);
        }
        if ((v.votesResponded[i] | v.votesGranted[i]) >> S) return bad("vote set out of range");
        w |= (u64)v.votesResponded[i] << VR;
        w |= (u64)v.votesGranted[i] << VG;
        for (int j = 0; j < S; ++j) {
            if (v.nextIndex[i][j] < 1 || v.nextIndex[i][j] > 4) return bad("nextIndex out of packed range");
            if (v.matchIndex[i][j] < 0 || v.matchIndex[i][j] > 3) return bad("matchIndex out of packed range");
            w |= (u64)(v.nextIndex[i][j] - 1) << (NI + 2 * j);
            w |= (u64)v.matchIndex[i][j] << (MI + 2 * j);
        }
        out[2 * i] = (u32)w;
        out[2 * i + 1] = (u32)(w >> 32);
    }
    std::vector<u32> slots;
    for (int q = 0; q < v.n_msgs; ++q) {
        const rmc_msg_view& m = v.msgs[q];
        if (m.mtype < 0 || m.mtype > 3) return bad("mtype out of range");
        if (m.msource < 0 || m.msource >= S || m.mdest < 0 || m.mdest >= S) return bad("message endpoint out of range");
        if (m.mterm < 0 || m.mterm > 15) return bad("mterm out of packed range");
        if (m.count < 1 || m.count > 3) return bad("message count out of packed range");
        u32 s = m_hdr((u32)m.mtype, (u32)m.msource, (u32)m.mdest, (u32)m.mterm);
        switch (m.mtype) {
            case RVQ:
                if (m.mlastLogTerm < 0 || m.mlastLogTerm > 15 || m.mlastLogIndex < 0 || m.mlastLogIndex > 3)
                    return bad("RequestVoteRequest field out of packed range");
                s |= ((u32)m.mlastLogTerm << 12) | ((u32)m.mlastLogIndex << 16);
                break;
            case RVP: {
                if (m.mlog_len < 0 || m.mlog_len > 3) return bad("mlog too long");
                u32 lg = (u32)m.mlog_len;
                for (int x = 0; x < m.mlog_len; ++x) {
                    if (m.mlog[x].term < 0 || m.mlog[x].term > 15 || m.mlog[x].value < 0 || m.mlog[x].value > 1)
                        return bad("mlog entry out of range");
                    lg |= (u32)(m.mlog[x].term | (m.mlog[x].value << 4)) << (2 + ENT_W * x);
                }
                s |= ((u32)(m.mvoteGranted != 0) << 12) | (lg << 13);
                break;
            }
            case AEQ: {
                if (m.mprevLogIndex < -1 || m.mprevLogIndex > 3 || m.mprevLogTerm < 0 || m.mprevLogTerm > 15 ||
                    m.mentries_len < 0 || m.mentries_len > 1 || m.mcommitIndex < 0 || m.mcommitIndex > 3)
                    return bad("AppendEntriesRequest field out of packed range");
                u32 e = 0;
                if (m.mentries_len) {
                    if (m.mentries[0].term < 0 || m.mentries[0].term > 15 || m.mentries[0].value < 0 ||
                        m.mentries[0].value > 1)
                        return bad("mentries entry out of range");
                    e = (u32)(m.mentries[0].term | (m.mentries[0].value << 4));
                }
                s |= ((u32)(m.mprevLogIndex + 1) << 12) | ((u32)m.mprevLogTerm << 15) |
                     ((u32)m.mentries_len << 19) | (e << 20) | ((u32)m.mcommitIndex << 25);
                break;
            }
            default:
                if (m.mmatchIndex < 0 || m.mmatchIndex > 3) return bad("mmatchIndex out of packed range");
                s |= ((u32)(m.msuccess != 0) << 12) | ((u32)m.mmatchIndex << 13);
        }
        for (u32 o : slots)
            if ((o & MSG_MASK) == s) return bad("duplicate message in bag view");
        slots.push_back(s | ((u32)m.count << 30));
    }
    std::sort(slots.begin(), slots.end(), [](u32 a, u32 b) { return a > b; });
    for (int q = 0; q < K; ++q) out[2 * S + q] = q < (int)slots.size() ? slots[q] : 0u;
    return 0;
}

void decode_state(int S, int K, const u32* in, rmc_state_view* v) {
    const int VR = VR_SH, VG = VR_SH + S, NI = VR_SH + 2 * S, MI = VR_SH + 4 * S;
    memset(v, 0, sizeof *v);
    v->n_servers = S;
    for (int i = 0; i < S; ++i) {
        const u64 w = (u64)in[2 * i] | ((u64)in[2 * i + 1] << 32);
        v->currentTerm[i] = (int)w_ct(w);
        v->state[i] = (int)w_st(w);
        v->votedFor[i] = w_vf(w) == NILV ? -1 : (int)w_vf(w);
        v->commitIndex[i] = (int)w_ci(w);
        v->log_len[i] = (int)w_len(w);
        for (u32 x = 0; x < w_len(w); ++x) {
            v->log[i][x].term = (int)(w_ent(w, x) & 15u);
            v->log[i][x].value = (int)(w_ent(w, x) >> 4);
        }
        v->votesResponded[i] = bits(w, VR, S);
        v->votesGranted[i] = bits(w, VG, S);
        for (int j = 0; j < S; ++j) {
            v->nextIndex[i][j] = (int)bits(w, NI + 2 * j, 2) + 1;
            v->matchIndex[i][j] = (int)bits(w, MI + 2 * j, 2);
        }
    }
    int n = 0;
    for (int q = 0; q < K; ++q) {
        const u32 s = in[2 * S + q];
        if (!s) continue;
        rmc_msg_view& m = v->msgs[n++];
        m.mtype = (int)m_type(s);
        m.msource = (int)m_src(s);
        m.mdest = (int)m_dst(s);
        m.mterm = (int)m_term(s);
        m.count = (int)m_cnt(s);
        switch (m.mtype) {
            case RVQ:
                m.mlastLogTerm = (int)((s >> 12) & 15u);
                m.mlastLogIndex = (int)((s >> 16) & 3u);
                break;
            case RVP: {
                m.mvoteGranted = (int)((s >> 12) & 1u);
                const u32 lg = (s >> 13) & 0x1FFFFu;
                m.mlog_len = (int)(lg & 3u);
                for (int x = 0; x < m.mlog_len; ++x) {
                    const u32 e = (lg >> (2 + ENT_W * x)) & 31u;
                    m.mlog[x].term = (int)(e & 15u);
                    m.mlog[x].value = (int)(e >> 4);
                }
                break;
            }
            case AEQ: {
                m.mprevLogIndex = (int)((s >> 12) & 7u) - 1;
                m.mprevLogTerm = (int)((s >> 15) & 15u);
                m.mentries_len = (int)((s >> 19) & 1u);
                const u32 e = (s >> 20) & 31u;
                if (m.mentries_len) {
                    m.mentries[0].term = (int)(e & 15u);
                    m.mentries[0].value = (int)(e >> 4);
                }
                m.mcommitIndex = (int)((s >> 25) & 3u);
                break;
            }
            default:
                m.msuccess = (int)((s >> 12) & 1u);
                m.mmatchIndex = (int)((s >> 13) & 3u);
        }
    }
    v->n_msgs = n;
}

void init_view(const rmc_config& g, rmc_state_view* v) {  // Init raft.tla:113-129
    memset(v, 0, sizeof *v);
    v->n_servers = g.n_servers;
    for (int i = 0; i < g.n_servers; ++i) {
        v->currentTerm[i] = 1;
        v->state[i] = 0;
        v->votedFor[i] = -1;
        for (int j = 0; j < g.n_servers; ++j) v->nextIndex[i][j] = 1;
    }
}

// ---- the wide codec ----------------------------------------------------------------
int wide_family(const WModel& M, int lane) { return lane == 255 ? -1 : M.L.family(lane); }

int encode_wide(int S, const rmc_state_view& v, WState* out, std::string* why) {
    auto bad = [&](const std::string& s) { *why = s; return RMC_E_INVAL; };
    WState& s = *out;
    wzero(&s, (int)sizeof s);
    if (v.n_servers != S) return bad("view n_servers differs from config");
    if (v.n_msgs < 0 || v.n_msgs > KW) return bad("too many messages for the wide bag");
    auto byte = [](int x, int lo, int hi) { return x >= lo && x <= hi; };
    for (int i = 0; i < S; ++i) {
        if (!byte(v.currentTerm[i], 0, TMAX)) return bad("currentTerm out of the wide range");
        if (!byte(v.state[i], 0, 2)) return bad("state out of range");
        if (v.votedFor[i] < -1 || v.votedFor[i] >= S) return bad("votedFor out of range");
        if (!byte(v.commitIndex[i], 0, 255)) return bad("commitIndex out of range");
        if (!byte(v.log_len[i], 0, LW)) return bad("log length out of the wide range");
        if ((v.votesResponded[i] | v.votesGranted[i]) >> S) return bad("vote set out of range");
        s.ct[i] = (uint8_t)v.currentTerm[i];
        s.st[i] = (uint8_t)v.state[i];
        s.vf[i] = v.votedFor[i] < 0 ? NIL : (uint8_t)v.votedFor[i];
        s.ci[i] = (uint8_t)v.commitIndex[i];
        s.len[i] = (uint8_t)v.log_len[i];
        s.vR[i] = (uint8_t)v.votesResponded[i];
        s.vG[i] = (uint8_t)v.votesGranted[i];
        for (int x = 0; x < v.log_len[i]; ++x) {
            if (!byte(v.log[i][x].term, 0, TMAX) || !byte(v.log[i][x].value, 0, 1)) return bad("log entry out of range");
            s.log[i][x].term = (uint8_t)v.log[i][x].term;
            s.log[i][x].value = (uint8_t)v.log[i][x].value;
        }
        for (int j = 0; j < S; ++j) {
            if (!byte(v.nextIndex[i][j], 1, 255) || !byte(v.matchIndex[i][j], 0, 255)) return bad("index out of range");
            s.ni[i][j] = (uint8_t)v.nextIndex[i][j];
            s.mi[i][j] = (uint8_t)v.matchIndex[i][j];
        }
    }
    for (int q = 0; q < v.n_msgs; ++q) {
        const rmc_msg_view& m = v.msgs[q];
        if (!byte(m.mtype, 0, 3)) return bad("mtype out of range");
        if (!byte(m.msource, 0, S - 1) || !byte(m.mdest, 0, S - 1)) return bad("message endpoint out of range");
        if (!byte(m.mterm, 0, TMAX)) return bad("mterm out of the wide range");
        if (!byte(m.count, 1, CMAX)) return bad("message count out of the wide range");
        WMsg w;
        wmsg_zero(w);
        w.type = (uint8_t)m.mtype;
        w.term = (uint8_t)m.mterm;
        w.src = (uint8_t)m.msource;
        w.dst = (uint8_t)m.mdest;
        switch (m.mtype) {
            case RVQ:
                if (!byte(m.mlastLogTerm, 0, TMAX) || !byte(m.mlastLogIndex, 0, 255))
                    return bad("RequestVoteRequest field out of range");
                w.b = (uint8_t)m.mlastLogTerm;
                w.c = (uint8_t)m.mlastLogIndex;
                break;
            case RVP:
                if (!byte(m.mlog_len, 0, LW)) return bad("mlog too long");
                w.a = (int8_t)(m.mvoteGranted != 0);
                w.n = (uint8_t)m.mlog_len;
                for (int x = 0; x < m.mlog_len; ++x) {
                    if (!byte(m.mlog[x].term, 0, TMAX) || !byte(m.mlog[x].value, 0, 1)) return bad("mlog entry out of range");
                    w.e[x].term = (uint8_t)m.mlog[x].term;
                    w.e[x].value = (uint8_t)m.mlog[x].value;
                }
                break;
            case AEQ:
                if (!byte(m.mprevLogIndex, -1, 127) || !byte(m.mprevLogTerm, 0, 255) || !byte(m.mentries_len, 0, 1) ||
                    !byte(m.mcommitIndex, 0, 255))
                    return bad("AppendEntriesRequest field out of range");
                w.a = (int8_t)m.mprevLogIndex;
                w.b = (uint8_t)m.mprevLogTerm;
                w.c = (uint8_t)m.mcommitIndex;
                w.n = (uint8_t)m.mentries_len;
                if (m.mentries_len) {
                    if (!byte(m.mentries[0].term, 0, TMAX) || !byte(m.mentries[0].value, 0, 1))
                        return bad("mentries entry out of range");
                    w.e[0].term = (uint8_t)m.mentries[0].term;
                    w.e[0].value = (uint8_t)m.mentries[0].value;
                }
                break;
            default:
                if (!byte(m.mmatchIndex, 0, 255)) return bad("mmatchIndex out of range");
                w.a = (int8_t)(m.msuccess != 0);
                w.b = (uint8_t)m.mmatchIndex;
        }
        for (int k = 0; k < s.nmsg; ++k)
            if (wmsg_cmp(s.msg[k], w) == 0) return bad("duplicate message in bag view");
        // insert sorted (the canonical order)
        int k = 0;
        while (k < s.nmsg && wmsg_cmp(s.msg[k], w) < 0) ++k;
        for (int r = s.nmsg; r > k; --r) {
            s.msg[r] = s.msg[r - 1];
            s.cnt[r] = s.cnt[r - 1];
        }
        s.msg[k] = w;
        s.cnt[k] = (uint8_t)m.count;
        s.nmsg += 1;
    }
    return 0;
}

// ---- simulation: SmokeInit sampler (Smokeraft.tla:4-76) ----------------------------
namespace {

// RandomSubset(k, X): k distinct random elements of X, X given by a sampler.
template <class T, class F>
std::vector<T> random_subset(int k, F draw, std::mt19937_64& g) {
    std::vector<T> out;
    for (int guard = 0; (int)out.size() < k && guard < 100000; ++guard) {
        T x = draw(g);
        if (std::find(out.begin(), out.end(), x) == out.end()) out.push_back(x);
    }
    return out;
}

struct SmokeDomains {
    int S, V, nat;
    int uni(std::mt19937_64& g, int lo, int hi) const {  // uniform in lo..hi
        return lo + (int)(g() % (u64)(hi - lo + 1));
    }
    // BoundedSeq([term : SmokeNat, value : Value], n) (Smokeraft.tla:4-6): uniform over
    // the whole set of sequences of length 0..n; encoded as (len, e0, e1, ...).
    std::vector<int> seq(std::mt19937_64& g, int n) const {
        const u64 E = (u64)(nat + 1) * (u64)V;
        u64 total = 0, p = 1;
        for (int m = 0; m <= n; ++m, p *= E) total += p;
        u64 r = g() % total;
        int len = 0;
        p = 1;
        while (r >= p) { r -= p; p *= E; ++len; }
        std::vector<int> s{len};
        for (int x = 0; x < len; ++x) {
            const u64 e = r % E;
            r /= E;
            s.push_back((int)(e / (u64)V));  // term
            s.push_back((int)(e % (u64)V));  // value
        }
        return s;
    }
};

// One message of SmokeMessageType (Smokeraft.tla:24-62) as a canonical int vector.
std::vector<int> smoke_msg(const SmokeDomains& D, int type, std::mt19937_64& g) {
    std::vector<int> v{type, D.uni(g, 0, D.nat), D.uni(g, 0, D.S - 1), D.uni(g, 0, D.S - 1)};
    if (type == RVQ) { v.push_back(D.uni(g, 0, D.nat)); v.push_back(D.uni(g, 0, D.nat)); }
    if (type == AEQ) {
        v.push_back(D.uni(g, -1, 1));              // mprevLogIndex \in SmokeInt
        v.push_back(D.uni(g, 0, D.nat));           // mprevLogTerm
        const auto e = D.seq(g, 1);                // mentries \in SmokeSeq(...)
        v.insert(v.end(), e.begin(), e.end());
        v.push_back(D.uni(g, 0, D.nat));           // mcommitIndex
    }
    if (type == RVP) {
        v.push_back(D.uni(g, 0, 1));               // mvoteGranted \in BOOLEAN
        const auto e = D.seq(g, 1);                // mlog \in SmokeSeq(...)
        v.insert(v.end(), e.begin(), e.end());
    }
    if (type == AEP) { v.push_back(D.uni(g, 0, 1)); v.push_back(D.uni(g, 0, D.nat)); }
    return v;
}

void msg_to_view(const std::vector<int>& v, rmc_msg_view* m) {
    memset(m, 0, sizeof *m);
    m->mtype = v[0];
    m->mterm = v[1];
    m->msource = v[2];
    m->mdest = v[3];
    m->count = 1;
    size_t p = 4;
    auto seq = [&](rmc_entry* out, int32_t* len) {
        *len = v[p++];
        for (int x = 0; x < *len; ++x) { out[x].term = v[p++]; out[x].value = v[p++]; }
    };
    if (v[0] == RVQ) { m->mlastLogTerm = v[p++]; m->mlastLogIndex = v[p++]; }
    if (v[0] == AEQ) { m->mprevLogIndex = v[p++]; m->mprevLogTerm = v[p++]; seq(m->mentries, &m->mentries_len); m->mcommitIndex = v[p++]; }
    if (v[0] == RVP) { m->mvoteGranted = v[p++]; seq(m->mlog, &m->mlog_len); }
    if (v[0] == AEP) { m->msuccess = v[p++]; m->mmatchIndex = v[p++]; }
}

}  // namespace

// SmokeInit (Smokeraft.tla:64-76): k choices for each of the 9 per-server
// variables, all k^9 combinations, each with the same bag of k messages drawn as
// [RandomSubset(k, SmokeMessageType) -> {1}].
int smoke_views(const SmokeShape& m, const rmc_sim_config& sc, std::vector<rmc_state_view>* views, std::string* why) {
    const int S = m.n_servers, k = sc.smoke_k;
    SmokeDomains D{S, m.n_values, sc.smoke_nat > 0 ? sc.smoke_nat : 2};
    if (D.nat > 3 && !m.wide) { *why = "smoke_nat > 3 exceeds the packed index range"; return RMC_E_INVAL; }
    if (D.nat > 100) { *why = "smoke_nat > 100"; return RMC_E_INVAL; }
    if (k > m.bag) { *why = "smoke_k messages exceed the bag capacity (set MaxMsgs >= k)"; return RMC_E_INVAL; }
    std::mt19937_64 g(sc.seed ^ 0x5350AC3ull);
    using V = std::vector<int>;
    auto fn = [&](auto elem) { return [&, elem](std::mt19937_64& gg) { V v; for (int i = 0; i < S; ++i) { auto e = elem(gg); v.insert(v.end(), e.begin(), e.end()); } return v; }; };
    auto one = [&](int lo, int hi) { return [&D, lo, hi](std::mt19937_64& gg) { return V{D.uni(gg, lo, hi)}; }; };
    const auto ct = random_subset<V>(k, fn(one(0, D.nat)), g);                               // :67
    const auto st = random_subset<V>(k, fn(one(0, 2)), g);                                   // :68
    const auto vf = random_subset<V>(k, fn(one(-1, S - 1)), g);                              // :69 (Nil = -1)
    const auto lg = random_subset<V>(k, fn([&](std::mt19937_64& gg) { return D.seq(gg, 3); }), g);  // :70
    const auto ci = random_subset<V>(k, fn(one(0, D.nat)), g);                               // :71
    const auto vr = random_subset<V>(k, fn(one(0, (1 << S) - 1)), g);                        // :72
    const auto vg = random_subset<V>(k, fn(one(0, (1 << S) - 1)), g);                        // :73
    auto row = [&](int lo, int hi) { return [&, lo, hi](std::mt19937_64& gg) { V v; for (int j = 0; j < S; ++j) v.push_back(D.uni(gg, lo, hi)); return v; }; };
    const auto ni = random_subset<V>(k, fn(row(1, D.nat)), g);                               // :74
    const auto mi = random_subset<V>(k, fn(row(0, D.nat)), g);                               // :75
    std::vector<V> mtype_union;                                                              // :58-62
    for (int t : {RVQ, AEQ, RVP, AEP}) {
        auto part = random_subset<V>(k, [&, t](std::mt19937_64& gg) { return smoke_msg(D, t, gg); }, g);
        mtype_union.insert(mtype_union.end(), part.begin(), part.end());
    }
    const auto msgs = random_subset<V>(k, [&](std::mt19937_64& gg) { return mtype_union[gg() % mtype_union.size()]; }, g);  // :76
    for (const auto* vec : {&ct, &st, &vf, &lg, &ci, &vr, &vg, &ni, &mi})
        if ((int)vec->size() != k) { *why = "RandomSubset could not draw k distinct elements"; return RMC_E_INVAL; }
    u64 n = 1;
    for (int x = 0; x < 9; ++x) n *= (u64)k;
    views->assign(n, rmc_state_view{});
    for (u64 idx = 0; idx < n; ++idx) {
        int dg[9];
        u64 r = idx;
        for (int x = 0; x < 9; ++x) { dg[x] = (int)(r % (u64)k); r /= (u64)k; }
        rmc_state_view v;
        memset(&v, 0, sizeof v);
        v.n_servers = S;
        size_t lp = 0;
        for (int i = 0; i < S; ++i) {
            v.currentTerm[i] = ct[dg[0]][i];
            v.state[i] = st[dg[1]][i];
            v.votedFor[i] = vf[dg[2]][i];
            v.commitIndex[i] = ci[dg[4]][i];
            v.votesResponded[i] = (uint32_t)vr[dg[5]][i];
            v.votesGranted[i] = (uint32_t)vg[dg[6]][i];
            for (int j = 0; j < S; ++j) {
                v.nextIndex[i][j] = ni[dg[7]][i * S + j];
                v.matchIndex[i][j] = mi[dg[8]][i * S + j];
            }
        }
        const V& L = lg[dg[3]];
        for (int i = 0; i < S; ++i) {
            v.log_len[i] = L[lp++];
            for (int x = 0; x < v.log_len[i]; ++x) { v.log[i][x].term = L[lp++]; v.log[i][x].value = L[lp++]; }
        }
        v.n_msgs = (int)msgs.size();
        for (size_t q = 0; q < msgs.size(); ++q) msg_to_view(msgs[q], &v.msgs[q]);
        (*views)[idx] = v;
    }
    return 0;
}

int smoke_init(const SmokeShape& m, const rmc_sim_config& sc, std::vector<u32>* packed, std::string* why) {
    std::vector<rmc_state_view> views;
    if (int rc = smoke_views(m, sc, &views, why)) return rc;
    const u64 NW = (u64)(2 * m.n_servers + m.bag);
    packed->assign(views.size() * NW, 0u);
    for (size_t q = 0; q < views.size(); ++q)
        if (int rc = encode_view(m.n_servers, m.bag, views[q], packed->data() + q * NW, why)) return rc;
    return 0;
}

}  // namespace rmc_host
