// rmc_act.cpp — action properties, host side (rmc.h "action properties"; the program and its
// two-state interpreter: rmc_pred.h; the compiler: rmc_front.cpp; the kernels: rmc_dev_act.h).
// rmc_set_actions gives a ctx its program — the only place anything is allocated for them — and
// rmc_run_bfs then runs the pass over the parents of every expansion launch (act_pass, beside
// the coverage pass, which reads the same resident parents) and reads its word at each level's
// end (act_scan, after the invariants' scans: an invariant violated in the level wins).
// rmc_eval_actions runs the same interpreter on caller pairs.
#include <cstring>
#include <string>
#include <vector>

#include "rmc_ctx.h"
#include "rmc_pred.h"

using namespace rmc;

namespace rmc_host {

void act_free(rmc_ctx* c) {
    delete c->acts;
    c->acts = nullptr;
    (void)hipFree(c->d_aprog);
    (void)hipFree(c->d_aword);
    (void)hipFree(c->d_apar);
    c->d_apar = nullptr;
    c->d_aprog = nullptr;
    c->d_aword = nullptr;
}

int act_begin(rmc_ctx* c) {
    HIPCHK(c, hipMemsetAsync(c->d_aword, 0xFF, 8, c->st));
    HIPCHK(c, hipMemcpyAsync(c->d_apar, &c->P, sizeof(Params), hipMemcpyHostToDevice, c->st));  // (c->P outlives the copy)
    return 0;
}

int act_pass(rmc_ctx* c, u64 lo, u64 hi) {
    HIPCHK(c, c->k->act(c->d_aprog, c->d_apar, c->B, lo, hi, c->d_aword, c->st));
    return 0;
}

int act_scan(rmc_ctx* c) {
    unsigned long long w = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&w, c->d_aword, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (w == ~0ull) return 0;
    // an invariant (built-in or model-defined) violated in the same level is reported as it is
    // without properties; a deadlock yields, as it does to an invariant
    if (c->have_target && c->res.violated_inv != 0) return 0;
    const u64 src = w >> 16;
    int level = 1;  // the source's: level d (1-based) = [level_start[d-1], level_start[d])
    while ((size_t)level + 1 < c->level_start.size() && c->level_start[(size_t)level] <= src) ++level;
    c->act_hit = 1;
    c->act_src = src;
    c->act_lane = (int)((w >> 8) & 255u);
    c->act_prop = (int)((w >> 1) & 127u);
    c->act_error = (int)(w & 1u);
    c->res.violated_inv = (int32_t)(RMC_ACT_USER0 << c->act_prop);
    c->res.violation_depth = level + 1;  // the trace's length: the path to the source, and the successor
    c->res.deadlock = 0;
    c->have_target = 1;
    c->stop = 1;
    c->target_idx = src;
    return 0;
}

namespace {
template <int S, int K>
void successor_t(const Params& P, const u32* src, int lane, u32* out) {
    u64 w[S], wo[S];
    u32 m[K], mo[K];
    for (int i = 0; i < S; ++i) w[i] = (u64)src[2 * i] | ((u64)src[2 * i + 1] << 32);
    for (int q = 0; q < K; ++q) m[q] = src[2 * S + q];
    Delta d;
    lane_delta<S, K>(w, m, lane, P, d);
    materialise<S, K>(w, m, d, wo, mo);
    for (int i = 0; i < S; ++i) {
        out[2 * i] = (u32)wo[i];
        out[2 * i + 1] = (u32)(wo[i] >> 32);
    }
    for (int q = 0; q < K; ++q) out[2 * S + q] = mo[q];
}
}  // namespace

int act_successor(rmc_ctx* c, const u32* src, int lane, u32* out) {
    const int S = c->sh.S, K = c->sh.K;
    if (lane < 0 || lane >= c->P.off[10]) return fail(c, RMC_E_STATE, "action property: the recorded lane is out of range");
#define RMC_ACT_SHAPE(SS, KK) \
    if (S == SS && K == KK) return successor_t<SS, KK>(c->P, src, lane, out), 0
    RMC_ACT_SHAPE(2, 4); RMC_ACT_SHAPE(2, 8); RMC_ACT_SHAPE(3, 4); RMC_ACT_SHAPE(3, 8);
    RMC_ACT_SHAPE(4, 4); RMC_ACT_SHAPE(4, 8); RMC_ACT_SHAPE(5, 4); RMC_ACT_SHAPE(5, 8);
#undef RMC_ACT_SHAPE
    return fail(c, RMC_E_STATE, "action property: no packed shape for this ctx");
}

}  // namespace rmc_host

using namespace rmc_host;

extern "C" {

int rmc_set_actions(rmc_ctx* c, const rmc_predicates* p) {
    if (!c) return RMC_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->st) HIPCHK(c, hipStreamSynchronize(c->st));
    if (!p || p->prog.n_pred == 0) {
        act_free(c);
        return 0;
    }
    const pred::Program& g = p->prog;
    if (!p->actions || g.n_pred < 0 || g.n_pred > RMC_MAX_ACTION_PROPS || g.n_code < 1 || g.n_code > pred::PRED_CODE)
        return fail(c, RMC_E_INVAL, "rmc_set_actions: not a program of rmc_actions_from_files");
    if (c->wide)
        return fail(c, RMC_E_INVAL, "rmc_set_actions: action properties run on the packed layout (this model's bounds "
                                    "need the wide layout)");
    if (c->dist.on) return fail(c, RMC_E_INVAL, "rmc_set_actions: action properties are single-GPU (the ctx is sharded)");
    if (continue_on(c))
        return fail(c, RMC_E_INVAL, "rmc_set_actions: a ctx with RMC_FLAG_CONTINUE tallies the ten compiled-in "
                                    "invariants only (it has no tally of transitions)");
    if (cons_on(c))
        return fail(c, RMC_E_INVAL, "rmc_set_actions: model-defined constraints are set (rmc_set_constraints): the pass "
                                    "checks the transitions the bounds admit, before a residual removes any");
    if ((c->cfg.flags & RMC_FLAG_SYMMETRY) && p->names_server)
        return fail(c, RMC_E_INVAL, "rmc_set_actions: a property names a server model value, so it is not invariant "
                                    "under SYMMETRY Permutations(Server)");
    if (g.n_servers != c->cfg.n_servers)
        return fail(c, RMC_E_INVAL, "rmc_set_actions: the program was compiled for " + std::to_string(g.n_servers) +
                                        " servers, the ctx has " + std::to_string(c->cfg.n_servers));
    if (!c->d_aprog && hipMalloc(&c->d_aprog, sizeof(pred::Program)) != hipSuccess)
        return fail(c, RMC_E_NOMEM, "device allocation failed (action property program)");
    if (!c->d_aword && hipMalloc(&c->d_aword, 8) != hipSuccess)
        return fail(c, RMC_E_NOMEM, "device allocation failed (action property result word)");
    if (!c->d_apar && hipMalloc(&c->d_apar, sizeof(Params)) != hipSuccess)
        return fail(c, RMC_E_NOMEM, "device allocation failed (action property parameters)");
    HIPCHK(c, hipMemcpy(c->d_aprog, &g, sizeof g, hipMemcpyHostToDevice));
    if (!c->acts) c->acts = new rmc_predicates();
    *c->acts = *p;
    return 0;
}

int rmc_action_violation(const rmc_ctx* c, int32_t* property, uint64_t* src_index, int32_t* family, int32_t* instance,
                         int32_t* is_error) {
    if (!c) return RMC_E_INVAL;
    if (!c->act_hit)
        return fail(const_cast<rmc_ctx*>(c), RMC_E_STATE, "rmc_action_violation: the last run reported no action property");
    if (property) *property = c->act_prop;
    if (src_index) *src_index = c->act_src;
    if (family) *family = family_of(c->P, c->act_lane);
    if (instance) *instance = c->act_lane;
    if (is_error) *is_error = c->act_error;
    return 0;
}

int rmc_eval_actions(rmc_ctx* c, const rmc_state_view* cur, const rmc_state_view* next, size_t n, uint8_t* verdicts) {
    if (!c) return RMC_E_INVAL;
    if (!act_on(c)) return fail(c, RMC_E_STATE, "rmc_eval_actions: no action properties set (rmc_set_actions)");
    if (n && (!cur || !next || !verdicts)) return fail(c, RMC_E_INVAL, "rmc_eval_actions: cur, next or verdicts is NULL");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n == 0) return 0;
    const size_t np = (size_t)c->acts->prog.n_pred;
    const int NW = c->NW;
    std::vector<u32> packed(n * 2 * (size_t)NW);
    std::string why;
    for (size_t t = 0; t < n; ++t) {
        if (encode_view(c->sh.S, c->sh.K, cur[t], packed.data() + t * 2 * NW, &why))
            return fail(c, RMC_E_INVAL, "pair " + std::to_string(t) + ", current state: " + why);
        if (encode_view(c->sh.S, c->sh.K, next[t], packed.data() + t * 2 * NW + NW, &why))
            return fail(c, RMC_E_INVAL, "pair " + std::to_string(t) + ", next state: " + why);
    }
    DevScratch<uint8_t> d_out;
    DevScratch<u32> d_in;
    HIPCHK(c, d_out.alloc(n * np));
    HIPCHK(c, d_in.alloc(packed.size()));
    HIPCHK(c, hipMemcpy(d_in.get(), packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, c->k->act_eval(c->d_aprog, d_in.get(), (u64)n, d_out.get(), c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(verdicts, d_out.get(), n * np, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
