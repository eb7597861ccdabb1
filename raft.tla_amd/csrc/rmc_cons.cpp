// rmc_cons.cpp — model-defined constraints, host side (rmc.h "model-defined constraints";
// the program and its interpreter: rmc_pred.h; the compiler: rmc_front.cpp; the kernels:
// rmc_dev_cons.h; the compaction's arithmetic: rmc_cons_plan.h).  rmc_set_constraints gives a
// ctx the residuals' program — nothing is allocated for them anywhere else but in the pass's
// scratch, which grows to the largest launch — and rmc_run_bfs then runs the pass over the
// seed's states and after every expansion launch, before anything else reads the states the
// launch added (cons_pass), and reads the error word at each level's end (cons_scan).
#include <cstdio>
#include <cstdlib>
#include <string>

#include "rmc_cons_plan.h"
#include "rmc_ctx.h"
#include "rmc_pred.h"

using namespace rmc;

namespace rmc_host {

static void cons_free_scratch(rmc_ctx* c) {
    (void)hipFree(c->CB.keep);
    (void)hipFree(c->CB.cnt);
    (void)hipFree(c->CB.off);
    (void)hipFree(c->CB.dst);
    c->CB = ConsBufs{};
    c->cons_cap = 0;
}

void cons_free(rmc_ctx* c) {
    delete c->cons;
    c->cons = nullptr;
    (void)hipFree(c->d_cprog);
    (void)hipFree(c->d_cword);
    c->d_cprog = nullptr;
    c->d_cword = nullptr;
    cons_free_scratch(c);
}

int cons_begin(rmc_ctx* c) {
    c->cons_error = 0;
    c->PE = c->P;
    c->PE.inv_mask = 0;  // checked on the kept states (k_cons_inv)
    c->PE.diamond = 0;   // a skipped successor relies on a sibling that a residual may remove
    c->cons_passes = c->cons_removed = 0;
    HIPCHK(c, hipMemsetAsync(c->d_cword, 0xFF, 8, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_cword + 1, 0, 8, c->st));  // the states moved
    return 0;
}

int cons_end(rmc_ctx* c) {
    if (!getenv("RMC_CONS_STATS")) return 0;
    unsigned long long moved = 0;
    HIPCHK(c, hipMemcpyAsync(&moved, c->d_cword + 1, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    fprintf(stderr, "[rmc] constraint pass: %llu passes, %llu states removed, %llu states moved\n",
            (unsigned long long)c->cons_passes, (unsigned long long)c->cons_removed, moved);
    return 0;
}

// The scratch of a launch of n new states.
static int cons_reserve(rmc_ctx* c, u64 n) {
    if (n <= c->cons_cap) return 0;
    HIPCHK(c, hipStreamSynchronize(c->st));
    cons_free_scratch(c);
    const u64 cap = std::max<u64>(std::max<u64>(n, 1ull << 16), std::min<u64>(2 * n, c->B.cap));
    const u64 nt = cons::tiles(cap);
    if (hipMalloc(&c->CB.keep, cap) != hipSuccess || hipMalloc(&c->CB.cnt, nt * 4) != hipSuccess ||
        hipMalloc(&c->CB.off, (nt + 1) * 8) != hipSuccess || hipMalloc(&c->CB.dst, (cap / 2 + 1) * 8) != hipSuccess) {
        cons_free_scratch(c);
        (void)hipGetLastError();
        return fail(c, RMC_E_NOMEM, "device allocation failed (constraint pass scratch for a launch of " +
                                        std::to_string(n) + " new states)");
    }
    c->cons_cap = cap;
    return 0;
}

int cons_pass(rmc_ctx* c, u64 nlo, u64 nhi) {
    if (nhi <= nlo) return 0;
    if (int rc = cons_reserve(c, nhi - nlo)) return rc;
    HIPCHK(c, c->k->cons(c->d_cprog, c->B, nlo, nhi, c->CB, c->d_cword, c->st));
    if (int rc = read_counters(c)) return rc;  // count = nlo + kept
    c->cons_passes += 1;
    c->cons_removed += nhi - c->h_ctr->count;
    if (c->cfg.invariants) HIPCHK(c, c->k->cons_inv(c->P, c->B, nlo, c->h_ctr->count, c->st));
    return 0;
}

int cons_scan(rmc_ctx* c, int depth, u64 level_lo) {
    unsigned long long w = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&w, c->d_cword, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (w == ~0ull) return 0;
    // the word's index is from before its launch's compaction: the state is found again among
    // the level's kept states, on which no residual is false (k_pred records what does not hold)
    HIPCHK(c, hipMemsetAsync(c->d_cword, 0xFF, 8, c->st));
    HIPCHK(c, c->k->pred(c->d_cprog, c->B, level_lo, c->h_ctr->count, c->d_cword, c->st));
    HIPCHK(c, hipMemcpyAsync(&w, c->d_cword, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (w == ~0ull) return fail(c, RMC_E_HIP, "constraint pass: the state a residual failed to evaluate on was not kept");
    const u64 idx = w >> 8;
    // a violation or deadlock at a lower or equal index was met first
    if (c->have_target && (c->target_idx & ((1ull << 48) - 1)) <= idx) return 0;
    c->res.violated_inv = 0;
    c->res.violation_depth = depth;
    c->res.deadlock = 0;
    c->pred_error = 0;
    c->cons_error = 1 + (int)((w >> 1) & 127u);
    c->have_target = 1;
    c->stop = 1;
    c->target_idx = idx;
    return 0;
}

}  // namespace rmc_host

using namespace rmc_host;

extern "C" {

int rmc_set_constraints(rmc_ctx* c, const rmc_predicates* p) {
    if (!c) return RMC_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->st) HIPCHK(c, hipStreamSynchronize(c->st));
    if (!p || p->prog.n_pred == 0) {
        cons_free(c);
        return 0;
    }
    const pred::Program& g = p->prog;
    if (g.n_pred < 0 || g.n_pred > pred::PRED_MAX || g.n_code < 1 || g.n_code > pred::PRED_CODE)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: not a program of rmc_constraints_from_files");
    if (c->resume)
        return fail(c, RMC_E_STATE, "rmc_set_constraints: rmc_recover loaded a checkpoint: its set was rebuilt from the "
                                    "stored states, without the keys of states a constraint removed");
    const uint32_t f = c->cfg.flags;
    if (f & RMC_FLAG_VERIFY_STATES)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: a ctx with RMC_FLAG_VERIFY_STATES gives every set slot the "
                                    "stored state that owns it, and the slot of a state the constraint removes never "
                                    "gets an owner");
    if (f & RMC_FLAG_CONTINUE)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: a ctx with RMC_FLAG_CONTINUE tallies violations where a "
                                    "launch stores its states, before the constraint removes any");
    if (f & RMC_FLAG_COVERAGE)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: a ctx with RMC_FLAG_COVERAGE tallies distinct states per "
                                    "action from the states a launch stores, before the constraint removes any");
    if (f & RMC_FLAG_SPILL)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: a ctx with RMC_FLAG_SPILL sizes its launches by the states "
                                    "they may store; the constraint pass compacts a resident store only");
    if (c->wide)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: model-defined constraints run on the packed layout (this "
                                    "model's bounds need the wide layout)");
    if (c->dist.on) return fail(c, RMC_E_INVAL, "rmc_set_constraints: model-defined constraints are single-GPU (the ctx is sharded)");
    if (act_on(c))
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: action properties are set (rmc_set_actions): their pass checks "
                                    "the transitions the bounds admit, before a residual removes any");
    if ((f & RMC_FLAG_SYMMETRY) && p->names_server)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: a residual names a server model value, so it is not "
                                    "invariant under SYMMETRY Permutations(Server)");
    if (g.n_servers != c->cfg.n_servers)
        return fail(c, RMC_E_INVAL, "rmc_set_constraints: the program was compiled for " + std::to_string(g.n_servers) +
                                        " servers, the ctx has " + std::to_string(c->cfg.n_servers));
    if (!c->d_cprog && hipMalloc(&c->d_cprog, sizeof(pred::Program)) != hipSuccess)
        return fail(c, RMC_E_NOMEM, "device allocation failed (constraint program)");
    if (!c->d_cword && hipMalloc(&c->d_cword, 16) != hipSuccess)  // the error word, the states moved
        return fail(c, RMC_E_NOMEM, "device allocation failed (constraint error word)");
    HIPCHK(c, hipMemcpy(c->d_cprog, &g, sizeof g, hipMemcpyHostToDevice));
    if (!c->cons) c->cons = new rmc_predicates();
    *c->cons = *p;
    c->cons_error = 0;
    return 0;
}

int rmc_constraint_error(const rmc_ctx* c) { return c && c->cons ? c->cons_error : 0; }

}  // extern "C"
