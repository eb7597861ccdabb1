// rmc_codec.h — the codecs between rmc_state_view (include/rmc.h) and the two
// state layouts (raft_packed.h words, raft_wide.h records), and the SmokeInit
// sampler.  Host arithmetic only: no HIP, no ctx; compiled into librmc.so and,
// with plain g++, by tests/native/codec_check.cpp.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rmc.h"
#include "raft_packed.h"
#include "raft_wide.h"

namespace rmc_host {
// ---- the packed layout: S servers, K bag slots, 2S + K words ----------------------
int family_of(const rmc::Params& P, int lane);
int encode_view(int S, int K, const rmc_state_view& v, rmc::u32* out, std::string* why);
void decode_state(int S, int K, const rmc::u32* in, rmc_state_view* v);
void init_view(const rmc_config& g, rmc_state_view* v);

// ---- the wide layout ----------------------------------------------------------------
int wide_family(const rmc::wide::WModel& M, int lane);
int encode_wide(int S, const rmc_state_view& v, rmc::wide::WState* out, std::string* why);

template <class St>  // WState, WStateC or WStateD
void decode_wide(int S, const St& s, rmc_state_view* v) {
    using namespace rmc;
    using namespace rmc::wide;
    memset(v, 0, sizeof *v);
    v->n_servers = S;
    for (int i = 0; i < S; ++i) {
        v->currentTerm[i] = s.ct[i];
        v->state[i] = s.st[i];
        v->votedFor[i] = s.vf[i] == NIL ? -1 : s.vf[i];
        v->commitIndex[i] = s.ci[i];
        v->log_len[i] = s.len[i];
        for (int x = 0; x < s.len[i]; ++x) {
            v->log[i][x].term = s.log[i][x].term;
            v->log[i][x].value = s.log[i][x].value;
        }
        v->votesResponded[i] = s.vR[i];
        v->votesGranted[i] = s.vG[i];
        for (int j = 0; j < S; ++j) {
            v->nextIndex[i][j] = s.ni[i][j];
            v->matchIndex[i][j] = s.mi[i][j];
        }
    }
    v->n_msgs = s.nmsg;
    for (int q = 0; q < s.nmsg; ++q) {
        const auto& w = s.msg[q];
        rmc_msg_view& m = v->msgs[q];
        m.mtype = w.type;
        m.mterm = w.term;
        m.msource = w.src;
        m.mdest = w.dst;
        m.count = s.cnt[q];
        switch (w.type) {
            case RVQ: m.mlastLogTerm = w.b; m.mlastLogIndex = w.c; break;
            case RVP:
                m.mvoteGranted = w.a;
                m.mlog_len = w.n;
                for (int x = 0; x < w.n; ++x) { m.mlog[x].term = w.e[x].term; m.mlog[x].value = w.e[x].value; }
                break;
            case AEQ:
                m.mprevLogIndex = w.a;
                m.mprevLogTerm = w.b;
                m.mcommitIndex = w.c;
                m.mentries_len = w.n;
                if (w.n) { m.mentries[0].term = w.e[0].term; m.mentries[0].value = w.e[0].value; }
                break;
            default: m.msuccess = w.a; m.mmatchIndex = w.b;
        }
    }
}

// ---- SmokeInit (Smokeraft.tla:64-76) ------------------------------------------------
// What the sampler needs of a model: its constants, its layout and the bag's slots.
struct SmokeShape {
    int n_servers, n_values;
    bool wide;
    int bag;
};
// SmokeInit as k^9 views, in RandomSubset product order.
int smoke_views(const SmokeShape& m, const rmc_sim_config& sc, std::vector<rmc_state_view>* views, std::string* why);
// The same, as packed states of 2S + K words (K = m.bag).
int smoke_init(const SmokeShape& m, const rmc_sim_config& sc, std::vector<rmc::u32>* packed, std::string* why);
}  // namespace rmc_host
