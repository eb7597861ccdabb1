// rmc_pred.cpp — model-defined invariants, host side (rmc.h "model-defined invariants";
// the program and its interpreter: rmc_pred.h; the compiler: rmc_front.cpp; the kernels:
// rmc_dev_pred.h, rmc_wide.hip).  rmc_set_predicates gives a ctx its program — the only
// place anything is allocated for them — and rmc_run_bfs then runs the pass over the
// seed's states and after every expansion launch (pred_pass, beside the coverage and
// violation passes) and merges its word with the fused check's at each level's end
// (pred_scan).  rmc_eval_predicates runs the same interpreter on caller states.
#include <cstring>
#include <string>
#include <vector>

#include "rmc_ctx.h"
#include "rmc_pred.h"

using namespace rmc;

namespace rmc_host {

void pred_free(rmc_ctx* c) {
    delete c->preds;
    c->preds = nullptr;
    (void)hipFree(c->d_prog);
    (void)hipFree(c->d_pword);
    c->d_prog = nullptr;
    c->d_pword = nullptr;
}

int pred_begin(rmc_ctx* c) {
    c->pred_error = 0;
    HIPCHK(c, hipMemsetAsync(c->d_pword, 0xFF, 8, c->st));
    return 0;
}

int pred_pass(rmc_ctx* c, u64 nlo, u64 nhi) {
    if (c->wide) HIPCHK(c, wide::launch_wpred(c->d_prog, c->WM, c->WB, nlo, nhi, c->d_pword, c->st));
    else HIPCHK(c, c->k->pred(c->d_prog, c->B, nlo, nhi, c->d_pword, c->st));
    return 0;
}

int pred_scan(rmc_ctx* c, int depth) {
    unsigned long long w = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&w, c->d_pword, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (w == ~0ull) return 0;
    const u64 idx = w >> 8;
    // the least index wins; at equal index the built-in does (the lower bit).  A deadlock
    // found in the same level yields, as it does to a built-in violation
    const bool builtin = c->have_target && c->res.violated_inv != 0;
    if (builtin && (c->target_idx & ((1ull << 48) - 1)) <= idx) return 0;
    c->res.violated_inv = (int32_t)(RMC_INV_USER0 << ((w >> 1) & 127u));
    c->res.violation_depth = depth;
    c->res.deadlock = 0;
    c->pred_error = (int)(w & 1u);
    c->have_target = 1;
    c->stop = 1;
    c->target_idx = idx;
    return 0;
}

}  // namespace rmc_host

using namespace rmc_host;

extern "C" {

int rmc_set_predicates(rmc_ctx* c, const rmc_predicates* p) {
    if (!c) return RMC_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->st) HIPCHK(c, hipStreamSynchronize(c->st));
    if (!p || p->prog.n_pred == 0) {
        pred_free(c);
        return 0;
    }
    const pred::Program& g = p->prog;
    if (p->actions || g.n_pred < 0 || g.n_pred > pred::PRED_MAX || g.n_code < 1 || g.n_code > pred::PRED_CODE)
        return fail(c, RMC_E_INVAL, "rmc_set_predicates: not a program of rmc_predicates_from_files");
    if (continue_on(c))
        return fail(c, RMC_E_INVAL, "rmc_set_predicates: a ctx with RMC_FLAG_CONTINUE counts the ten compiled-in "
                                    "invariants only (its tallies have ten rows)");
    if (c->dist.on) return fail(c, RMC_E_INVAL, "rmc_set_predicates: model-defined invariants are single-GPU (the ctx is sharded)");
    if (c->wide && (c->cfg.flags & RMC_FLAG_SPILL))
        return fail(c, RMC_E_INVAL, "rmc_set_predicates: the wide layout with RMC_FLAG_SPILL stores no record of a "
                                    "depth-bounded run's last level, so no pass can read it");
    if ((c->cfg.flags & RMC_FLAG_SYMMETRY) && p->names_server)
        return fail(c, RMC_E_INVAL, "rmc_set_predicates: a predicate names a server model value, so it is not "
                                    "invariant under SYMMETRY Permutations(Server)");
    if (g.n_servers != c->cfg.n_servers)
        return fail(c, RMC_E_INVAL, "rmc_set_predicates: the program was compiled for " + std::to_string(g.n_servers) +
                                        " servers, the ctx has " + std::to_string(c->cfg.n_servers));
    if (!c->d_prog && hipMalloc(&c->d_prog, sizeof(pred::Program)) != hipSuccess)
        return fail(c, RMC_E_NOMEM, "device allocation failed (predicate program)");
    if (!c->d_pword && hipMalloc(&c->d_pword, 8) != hipSuccess)
        return fail(c, RMC_E_NOMEM, "device allocation failed (predicate result word)");
    HIPCHK(c, hipMemcpy(c->d_prog, &g, sizeof g, hipMemcpyHostToDevice));
    if (!c->preds) c->preds = new rmc_predicates();
    *c->preds = *p;
    return 0;
}

int rmc_predicate_error(const rmc_ctx* c) {
    return c && c->res.violated_inv >= (int32_t)RMC_INV_USER0 && c->res.violated_inv < (int32_t)RMC_ACT_USER0 ? c->pred_error
                                                                                                             : 0;
}

int rmc_eval_predicates(rmc_ctx* c, const rmc_state_view* states, size_t n, uint8_t* verdicts) {
    if (!c) return RMC_E_INVAL;
    if (!pred_on(c)) return fail(c, RMC_E_STATE, "rmc_eval_predicates: no predicates set (rmc_set_predicates)");
    if (n && (!states || !verdicts)) return fail(c, RMC_E_INVAL, "rmc_eval_predicates: states or verdicts is NULL");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n == 0) return 0;
    const size_t np = (size_t)c->preds->prog.n_pred;
    DevScratch<uint8_t> d_out;
    HIPCHK(c, d_out.alloc(n * np));
    if (c->wide) {
        if (int rc = pred_eval_wide(c, states, n, d_out.get())) return rc;
    } else {
        const int NW = c->NW;
        std::vector<u32> packed(n * (size_t)NW);
        std::string why;
        for (size_t t = 0; t < n; ++t)
            if (encode_view(c->sh.S, c->sh.K, states[t], packed.data() + t * NW, &why))
                return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
        DevScratch<u32> d_in;
        HIPCHK(c, d_in.alloc(packed.size()));
        HIPCHK(c, hipMemcpy(d_in.get(), packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(c, c->k->pred_eval(c->d_prog, d_in.get(), (u64)n, d_out.get(), c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    HIPCHK(c, hipMemcpy(verdicts, d_out.get(), n * np, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
