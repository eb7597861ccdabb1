// rmc_api.cpp — the C ABI of librmc.so (include/rmc.h): context, BFS driver,
// traces, simulation, and the differential-test entry point.  (The codecs are
// rmc_codec.cpp, the frontier spill rmc_spill.cpp, checkpoints rmc_ckpt.cpp.)
//
// Host side of the hot path: one HIP stream per context, one kernel launch
// (plus one 40-byte counter read-back) per BFS level.  The level loop
// replaces TLC's ModelChecker.runTLC / Worker loop.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <sys/mman.h>

#include "rmc_cover.h"
#include "rmc_ctx.h"
#include "rmc_units.h"
#include "rmc_viol.h"

using namespace rmc;

static const char* kVersion = "rmc 2 (raft.tla BFS, gfx950 HIP, packed-delta lanes, HBM fp set, RCCL sharding)";

namespace rmc_host {

int fail(rmc_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

int kcap_for(int max_msgs) { return max_msgs <= 4 ? 4 : 8; }

int validate(const rmc_config* c, std::string* why) {
    auto bad = [&](const char* s) { *why = s; return RMC_E_INVAL; };
    if (c->n_servers < 2 || c->n_servers > RMC_MAX_SERVERS) return bad("n_servers must be 2..5");
    if (c->n_values < 1 || c->n_values > RMC_MAX_VALUES) return bad("n_values must be 1..2");
    if (c->invariants & ~1023u) return bad("unknown invariant bit");
    if (c->flags & ~(1023u | RMC_FLAG_CONTINUE)) return bad("unknown flag bit");  // (bit 10 is not assigned)
    if ((c->flags & RMC_UNBOUNDED_ANY) && c->max_depth <= 0)
        return bad("a model with unbounded fields (RMC_FLAG_UNBOUNDED_*) needs max_depth > 0 (TLC -depth)");
    if (wide_wanted(*c)) return validate_wide(c, why);  // bounds beyond the packed capacity
    if (c->max_term < 1 || c->max_term > RMC_MAX_TERM) return bad("max_term must be 1..14");
    if (c->max_log_len < 0 || c->max_log_len > RMC_MAX_LOG) return bad("max_log_len must be 0..3");
    if (c->max_msgs < 0 || c->max_msgs > RMC_MAX_MSGS) return bad("max_msgs must be 0..8");
    if (c->max_dup < 1 || c->max_dup > RMC_MAX_DUP) return bad("max_dup must be 1..3");
    return 0;
}

void fill_params(rmc_ctx* c) {
    const rmc_config& g = c->cfg;
    c->wide = wide_wanted(g) ? 1 : 0;
    if (c->wide) fill_wide_model(c);
    c->sh.S = g.n_servers;
    c->sh.K = kcap_for(g.max_msgs);
    c->sh.sym = (g.flags & RMC_FLAG_SYMMETRY) != 0;
    c->sh.verify = (g.flags & RMC_FLAG_VERIFY_STATES) != 0;
    c->k = shape_kernels(c->sh.S, c->sh.K);
    c->NW = 2 * c->sh.S + c->sh.K;
    Params& P = c->P;
    P.V = g.n_values;
    P.max_term = g.max_term;
    P.max_log = g.max_log_len;
    P.max_msgs = g.max_msgs;
    P.max_dup = g.max_dup;
    P.bug_quorum = (g.flags & RMC_FLAG_BUG_QUORUM) ? 1 : 0;
    P.inv_mask = (int)g.invariants;
    P.symmetry = c->sh.sym ? 1 : 0;
    P.fp_mask = ~0ull;
    P.unbounded = (int)((g.flags >> 5) & 15u);  // RMC_FLAG_UNBOUNDED_TERM .. _DUP
    {  // commuting-diamond probe elimination (not under SYMMETRY; RMC_DIAMOND=0 turns it off)
        const char* e = getenv("RMC_DIAMOND");
        P.diamond = (!c->sh.sym && !(e && e[0] == '0')) ? 1 : 0;
    }
    const int S = c->sh.S, K = c->sh.K;
    const int sizes[10] = {S, S, S * S, S, S * VMAX, S, S * S, K, K, K};  // = Lanes<S,K>
    P.off[0] = 0;
    for (int f = 0; f < 10; ++f) P.off[f + 1] = P.off[f] + sizes[f];
    fill_lane_desc(P, S);
    // permutations of 0..S-1 in lexicographic order (identity first), 3 bits per id
    memset(&c->PT, 0, sizeof c->PT);
    {
        int a[5] = {0, 1, 2, 3, 4};
        int n = 0;
        do {
            u32 code = 0;
            for (int i = 0; i < S; ++i) code |= (u32)a[i] << (3 * i);
            c->PT.code[n] = code;
            ++n;
        } while (std::next_permutation(a, a + S));
        c->PT.np = n;
    }
}

int reset_counters(rmc_ctx* c, bool keep_count) {
    Counters h{};
    h.count = keep_count ? c->h_ctr->count : 0;
    h.viol = ~0ull;
    h.deadlock = ~0ull;
    *c->h_ctr = h;
    HIPCHK(c, hipMemcpyAsync(c->B.ctr, c->h_ctr, sizeof(Counters), hipMemcpyHostToDevice, c->st));
    return 0;
}

std::string capacity_message(const rmc_ctx* c, u32 overflow, int depth) {
    const u32 f = (overflow >> 8) & 15u;
    if (!f) return "";
    std::string what;
    if (f & 1) what += std::string(what.empty() ? "" : ", ") + "currentTerm > " + std::to_string(c->cfg.max_term);
    if (f & 2) what += std::string(what.empty() ? "" : ", ") + "Len(log) > " + std::to_string(c->cfg.max_log_len);
    if (f & 4) what += std::string(what.empty() ? "" : ", ") + "Cardinality(DOMAIN messages) > " +
                       std::to_string(c->cfg.max_msgs);
    if (f & 8) what += std::string(what.empty() ? "" : ", ") + "messages[m] > " + std::to_string(c->cfg.max_dup);
    return "a successor of a level-" + std::to_string(depth) + " state needs " + what + ": beyond the " +
           (c->wide ? "wide" : "packed") +
           " layout's capacity of a field no CONSTRAINT bounds (lower the depth bound or add a CONSTRAINT)";
}

int read_counters(rmc_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(c->h_ctr, c->B.ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return 0;
}

int begin_set(rmc_ctx* c, bool tagged) {
    const char* epe = getenv("RMC_SET_EPOCH");  // (read per run: tests vary it)
    const u32 ep_max = epe ? (u32)std::min(255, std::max(0, atoi(epe))) : 255u;
    const SetEpoch e = next_set_epoch(c->set_epoch, ep_max, tagged);
    if (e.clear) HIPCHK(c, launch_fill(c->B.table, c->table_slots * 8, 0, c->st));
    c->set_epoch = e.epoch;
    if (c->sh.verify) HIPCHK(c, launch_fill(c->B.sidx, c->table_slots * 8, 0xFF, c->st));
    HIPCHK(c, set_fp_salt(*c->k, c->cfg.seed, c->set_epoch, c->st));
    return 0;
}

int seed_init(rmc_ctx* c) {
    rmc_state_view iv;
    init_view(c->cfg, &iv);
    std::vector<u32> packed((size_t)c->NW);
    std::string why;
    if (encode_view(c->sh.S, c->sh.K, iv, packed.data(), &why)) return fail(c, RMC_E_INVAL, why);
    HIPCHK(c, hipMemcpyAsync(c->d_staged, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, c->k->seed(c->sh.sym, expand_params(c), c->PT, c->B, c->d_staged, 1, c->st));
    return 0;
}

static_assert(COV_ROWS == RMC_COV_ACTIONS, "rmc_cover.h's rows are rmc.h's");

int cover_begin(rmc_ctx* c) {
    c->cov_valid = 0;
    HIPCHK(c, hipMemsetAsync(c->d_cov, 0, sizeof(rmc_coverage), c->st));
    return 0;
}

int cover_end(rmc_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(&c->cov, c->d_cov, sizeof(rmc_coverage), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    c->cov_valid = 1;
    return 0;
}

static_assert(VIOL_INVS == RMC_INV_COUNT, "rmc_viol.h's invariants are rmc.h's");

int viol_begin(rmc_ctx* c) {
    c->viol_valid = 0;
    HIPCHK(c, hipMemsetAsync(c->d_viol, 0, VIOL_LEAST * 8, c->st));
    HIPCHK(c, hipMemsetAsync(c->d_viol + VIOL_LEAST, 0xFF, VIOL_INVS * 8, c->st));
    return 0;
}

int viol_end(rmc_ctx* c) {
    unsigned long long h[VIOL_WORDS];
    HIPCHK(c, hipMemcpyAsync(h, c->d_viol, sizeof h, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    rmc_violations& v = c->viol;
    v = rmc_violations{};
    for (int r = 0; r < VIOL_INVS; ++r) {
        v.first[r] = h[VIOL_FIRST + r];
        v.each[r] = h[VIOL_EACH + r];
        v.states += v.first[r];
        const u64 least = h[VIOL_LEAST + r];
        c->viol_least[r] = least;
        if (least == ~0ull) continue;
        // level d = [level_start[d - 1], level_start[d])
        const auto it = std::upper_bound(c->level_start.begin(), c->level_start.end(), least);
        v.depth[r] = (int32_t)(it - c->level_start.begin());
    }
    c->viol_valid = 1;
    return 0;
}

int level_error(rmc_ctx* c, const Counters& k, int depth, const LevelText& text, int rank) {
    const std::string on = rank < 0 ? "" : " on rank " + std::to_string(rank);
    if (k.table_full) return fail(c, RMC_E_CAPACITY, "fingerprint set full" + on);
    if (k.overflow >> 8) return fail(c, RMC_E_CAPACITY, capacity_message(c, k.overflow, depth));
    if (k.overflow & 4u) return fail(c, RMC_E_CAPACITY, "verification buffer full" + on);
    if (text.tie_full && (k.overflow & 16u)) return fail(c, RMC_E_CAPACITY, text.tie_full);
    if (k.overflow & 8u) return fail(c, RMC_E_HIP, text.no_owner + on);
    if (rank >= 0 && (k.overflow & 2u))
        return fail(c, RMC_E_CAPACITY, "exchange parking buffer full" + on + " (raise keys_per_dest)");
    if (k.overflow && rank >= 0)
        return fail(c, RMC_E_CAPACITY, "state store full" + on + " (raise rmc_config.state_capacity)");
    if (k.overflow)
        return fail(c, RMC_E_CAPACITY, "state store full (capacity " + std::to_string(c->B.cap) + " " + text.store_noun +
                                           "); raise rmc_config.state_capacity");
    return 0;
}

void scan_target(rmc_ctx* c, const Counters* rows, int n, int depth) {
    for (int r = 0; r < n && !c->have_target; ++r)  // the lowest rank's least violating index
        if (rows[r].viol != ~0ull) {
            c->res.violated_inv = 1 << (int)(rows[r].viol & 15);
            c->res.violation_depth = depth;
            c->have_target = 1;
            c->stop = continue_on(c) ? 0 : 1;
            c->target_idx = ((u64)r << 48) | (rows[r].viol >> 4);
        }
    if (c->cfg.flags & RMC_FLAG_CHECK_DEADLOCK)
        for (int r = 0; r < n && !c->stop; ++r)
            if (rows[r].deadlock != ~0ull) {
                c->res.deadlock = 1;
                c->stop = 1;
                if (!c->have_target) {  // (RMC_FLAG_CONTINUE: a violation recorded before stays the target)
                    c->have_target = 1;
                    c->target_idx = ((u64)r << 48) | rows[r].deadlock;
                }
            }
}

int seed_done(rmc_ctx* c) {
    c->res.generated = 1;
    c->level_start.push_back(0);
    c->level_start.push_back(c->h_ctr->count);
    scan_target(c, c->h_ctr, 1, 1);  // (a seed launch finds no deadlock: Counters.deadlock stays ~0)
    return c->h_ctr->count ? 1 : 0;
}

int end_level(rmc_ctx* c, u64 hi, int* depth, rmc_progress_fn cb, void* user,
              std::chrono::steady_clock::time_point t0, const LevelText& text, int* more) {
    *more = 0;
    HIPCHK(c, hipEventRecord(c->ev1, c->st));
    if (int rc = read_counters(c)) return rc;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->res.expand_kernel_seconds += 1e-3 * ms;
    const Counters& k = *c->h_ctr;
    if (int rc = level_error(c, k, *depth, text, -1)) return rc;
    c->res.collisions += k.collisions;
    c->res.verified += k.vchecked;
    c->res.generated += k.generated;
    c->res.probes += k.probes;
    if (text.walked) *text.walked += k.walked;
    const u64 nnew = k.count - hi;
    if (nnew) {
        ++*depth;
        c->level_start.push_back(k.count);
    }
    c->res.distinct = k.count;
    scan_target(c, &k, 1, *depth);
    if (pred_on(c))
        if (int rc = pred_scan(c, *depth)) return rc;
    if (cons_on(c))  // (the level's kept states: [hi, count))
        if (int rc = cons_scan(c, *depth, hi)) return rc;
    if (act_on(c))  // (last: an invariant violated in the level wins)
        if (int rc = act_scan(c)) return rc;
    if (cb) {
        rmc_level_stats ls{};
        ls.level = nnew ? *depth - 1 : *depth;
        ls.generated = c->res.generated;
        ls.distinct = k.count;
        ls.new_states = nnew;
        ls.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (cb(&ls, user)) {
            c->res.left_on_queue = nnew;
            return 0;
        }
    }
    *more = nnew != 0;
    return 0;
}

}  // namespace rmc_host

using namespace rmc_host;

extern "C" {

const char* rmc_version(void) { return kVersion; }

const char* rmc_last_error(const rmc_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

size_t rmc_state_bytes(const rmc_config* cfg) {
    if (!cfg) return 0;
    if (wide_wanted(*cfg)) return wide_record_bytes(*cfg);
    return (size_t)(2 * cfg->n_servers + kcap_for(cfg->max_msgs)) * 4u;
}

int rmc_create(const rmc_config* cfg, rmc_ctx** out) {
    if (!cfg || !out) return RMC_E_INVAL;
    *out = nullptr;
    std::string why;
    if (int rc = validate(cfg, &why)) {
        fprintf(stderr, "rmc_create: %s\n", why.c_str());
        return rc;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device || cfg->device < 0) {
        fprintf(stderr, "rmc_create: no HIP device %d\n", cfg->device);
        return RMC_E_NOGPU;
    }
    rmc_ctx* c = new rmc_ctx();
    c->cfg = *cfg;
    fill_params(c);
    auto bail = [&](int rc) {
        fprintf(stderr, "rmc_create: %s\n", c->err.c_str());
        rmc_destroy(c);
        return rc;
    };
    if (!c->k) { c->err = "no kernels built for this shape"; return bail(RMC_E_INVAL); }
    if (hipSetDevice(cfg->device) != hipSuccess) { c->err = "hipSetDevice failed"; return bail(RMC_E_NOGPU); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) { c->err = "hipGetDeviceProperties failed"; return bail(RMC_E_NOGPU); }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        c->err = std::string("device is ") + prop.gcnArchName + ", librmc is built for gfx950 only";
        return bail(RMC_E_NOGPU);
    }
    if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
        c->err = "stream/event creation failed";
        return bail(RMC_E_HIP);
    }
    if (hipHostMalloc(&c->h_ctr, sizeof(Counters), hipHostMallocDefault) != hipSuccess) {
        c->err = "pinned allocation failed";
        return bail(RMC_E_NOMEM);
    }
    memset(c->h_ctr, 0, sizeof(Counters));
    if (cover_on(c) && hipMalloc(&c->d_cov, sizeof(rmc_coverage)) != hipSuccess) {
        c->err = "device allocation failed (coverage tallies)";
        return bail(RMC_E_NOMEM);
    }
    if (continue_on(c) && hipMalloc(&c->d_viol, VIOL_WORDS * 8) != hipSuccess) {
        c->err = "device allocation failed (violation tallies)";
        return bail(RMC_E_NOMEM);
    }
    if (c->wide) {  // bounds beyond the packed capacity: the wide layout (rmc_wide.cpp)
        if (int rc = create_wide(c)) return bail(rc);
        *out = c;
        return 0;
    }

    // ---- capacity: state store + parents + lanes + fingerprint set (load <= 0.5):
    // the division of the budget is rmc_plan.h (host arithmetic, tested without a device)
    const char* hl = getenv("RMC_SPILL_HOST_LINKS");
    size_t fr = 0, tot = 0;
    (void)hipMemGetInfo(&fr, &tot);
    PackedPlanIn in{};
    in.budget = (u64)((double)fr * 0.80);
    in.state_words = (u64)c->NW;
    in.state_capacity = cfg->state_capacity;
    in.set_slots = set_slots_of(cfg->set_bytes);  // rmc_config.set_bytes (TLC -fpmem)
    in.device_window = cfg->device_window;
    in.spill = (cfg->flags & RMC_FLAG_SPILL) != 0;
    in.verify = c->sh.verify;
    in.host_links = hl && atoi(hl);
    const PackedPlan plan = packed_plan(in);
    if (plan.cap_exceeds_set) {
        c->err = "state_capacity " + std::to_string(cfg->state_capacity) + " exceeds what a set of set_bytes " +
                 std::to_string(cfg->set_bytes) + " holds (" + std::to_string(plan.set_slots / 2) + " states)";
        return bail(RMC_E_INVAL);
    }
    const bool spill = in.spill, dev_links = plan.dev_links;
    const u64 cap = plan.cap, slots = plan.slots, win = plan.window, link_cap = plan.link_cap;
    c->table_slots = slots;
    c->B.cap = win;
    c->B.lim = win;  // (set again by every launch of rmc_run_bfs)
    c->B.admit_reserve = 0;
    c->B.tmask = slots - 1;
    c->B.wmask = dev_links ? win - 1 : ~0ull;
    if (hipMalloc(&c->B.store, win * (u64)c->NW * 4) != hipSuccess ||
        hipMalloc(&c->B.parent, link_cap * 8) != hipSuccess || hipMalloc(&c->B.act, link_cap) != hipSuccess ||
        hipMalloc(&c->B.foot, win * 8) != hipSuccess || hipMalloc(&c->B.cls, win) != hipSuccess ||
        hipMalloc(&c->B.table, slots * 8) != hipSuccess || hipMalloc(&c->B.ctr, sizeof(Counters)) != hipSuccess ||
        hipMalloc(&c->B.word, std::min<u64>(1ull << kMaxLaunchLog2, win) * 2) != hipSuccess ||  // presorted windows of one launch
        hipMalloc(&c->d_staged, (size_t)c->NW * 4 * 64) != hipSuccess) {
        c->err = "device allocation failed (capacity " + std::to_string(win) + " states)";
        return bail(RMC_E_NOMEM);
    }
    c->spill.on = spill ? 1 : 0;
    c->spill.dev_links = dev_links ? 1 : 0;
    c->spill.win = win;
    c->spill.total_cap = cap;
    c->spill.store = c->B.store;
    c->spill.parent = c->B.parent;
    c->spill.act = c->B.act;
    c->spill.foot = c->B.foot;
    c->spill.cls = c->B.cls;
    // classes are a layout hint (any value is a valid class): zero them once so
    // recovered or never-written states sort deterministically
    if (hipMemset(c->B.cls, 0, win) != hipSuccess) {
        c->err = "hipMemset failed";
        return bail(RMC_E_HIP);
    }
    if (spill && !dev_links && spill_reserve(c)) return bail(RMC_E_NOMEM);
    if (c->sh.sym) {  // successors with tied signatures, canonicalised by k_ties after each launch
        // a lane defers at most one tied successor, so launches of at most
        // tie_cap / lanes states cannot overflow it (run_bfs sizes them so):
        // room for full 2^24-state launches (6.4 GB for S = 3, K = 4; smaller
        // launches cost ~6 % on the MCraftBench bounds), halved until it fits
        c->B.tie_cap = (u64)c->P.off[10] << 24;
        while (hipMalloc(&c->B.ties, c->B.tie_cap * 8) != hipSuccess) {
            c->B.ties = nullptr;
            c->B.tie_cap >>= 1;
            if (c->B.tie_cap < (1ull << 20)) break;
        }
        if (!c->B.ties) {
            c->err = "device allocation failed (symmetry tie buffer)";
            return bail(RMC_E_NOMEM);
        }
    }
    if (c->sh.verify) {  // slot -> store index (8 B per slot) + deferred-hit buffer (16 B per record)
        c->B.vcap = 1ull << 26;
        if (hipMalloc(&c->B.sidx, slots * 8) != hipSuccess || hipMalloc(&c->B.vbuf, c->B.vcap * 16) != hipSuccess) {
            c->err = "device allocation failed (verification buffers)";
            return bail(RMC_E_NOMEM);
        }
        if (spill && verify_spill_reserve(c)) return bail(RMC_E_NOMEM);
    }
    c->B.rank = 0;
    c->B.world = 1;
    c->B.ref_tag = 0;
    *out = c;
    return 0;
}

void rmc_destroy(rmc_ctx* c) {
    if (!c) return;
    if (c->st) (void)hipStreamSynchronize(c->st);
    if (c->wide) destroy_wide(c);
    spill_free(c);
    // the unbiased allocations (B.* may be rebased by a spill)
    (void)hipFree(c->spill.store ? c->spill.store : c->B.store);
    (void)hipFree(c->spill.parent ? c->spill.parent : c->B.parent);
    (void)hipFree(c->spill.act ? c->spill.act : c->B.act);
    (void)hipFree(c->spill.foot ? c->spill.foot : c->B.foot);
    (void)hipFree(c->spill.cls ? c->spill.cls : c->B.cls);
    (void)hipFree(c->B.table);
    (void)hipFree(c->B.ctr);
    (void)hipFree(c->B.word);
    (void)hipFree(c->d_staged);
    free_dist(c);
    (void)hipFree(c->B.sidx);
    (void)hipFree(c->B.vbuf);
    (void)hipFree(c->B.hbuf);
    (void)hipFree(c->spill.d_ostage);
    if (c->spill.h_ostage) (void)hipHostFree(c->spill.h_ostage);
    if (c->spill.hs_bytes) munmap(c->spill.h_state, c->spill.hs_bytes);
    (void)hipFree(c->B.ties);
    (void)hipFree(c->d_cov);
    (void)hipFree(c->d_viol);
    pred_free(c);
    cons_free(c);
    act_free(c);
    if (c->h_ctr) (void)hipHostFree(c->h_ctr);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->st) (void)hipStreamDestroy(c->st);
    delete c;
}

// A fresh run (no rmc_recover before it): clear the result, the set and the
// counters, and seed Init.  *depth: the level the loop starts from.
static int start_run(rmc_ctx* c, int* depth) {
    c->res = rmc_result{};
    c->res.set_slots = c->table_slots;
    c->res.spill_links_on_device = c->spill.on && c->spill.dev_links;
    c->walked = 0;
    c->level_start.clear();
    if (c->spill.on) {
        spill_rebase(c, 0);
        SpillState& X = c->spill;  // back the first spill's pages meanwhile
        if (!X.dev_links && !X.ahead.joinable()) spill_prefault_ahead(c, std::min(X.total_cap, X.win));
    }
    // the set epoch: the next one, or a cleared set (rmc_plan.h next_set_epoch)
    if (int rc = begin_set(c, !c->sh.verify)) return rc;
    if (int rc = reset_counters(c, false)) return rc;
    if (cover_on(c))
        if (int rc = cover_begin(c)) return rc;
    if (continue_on(c))
        if (int rc = viol_begin(c)) return rc;
    if (pred_on(c))
        if (int rc = pred_begin(c)) return rc;
    if (cons_on(c))
        if (int rc = cons_begin(c)) return rc;
    if (act_on(c))
        if (int rc = act_begin(c)) return rc;
    c->B.vlo = 0;
    c->spill.hcopied = 0;
    c->spill.host_hits = 0;

    // ---- Init (raft.tla:125-129): one initial state
    if (int rc = seed_init(c)) return rc;
    if (int rc = read_counters(c)) return rc;
    if (cons_on(c)) {  // an initial state that fails the constraint is generated and dropped: depth 0
        if (int rc = cons_pass(c, 0, c->h_ctr->count)) return rc;
        if (int rc = read_counters(c)) return rc;  // (the built-in invariants of the kept states)
    }
    *depth = seed_done(c);
    if (c->sh.verify) HIPCHK(c, c->k->publish(c->sh.sym, c->P, c->PT, c->B, 0, c->h_ctr->count, c->st));
    if (cover_on(c))  // row Init: the one initial state generated, and what the seed stored
        HIPCHK(c, c->k->cover(c->P, c->B, 0, 0, 0, c->h_ctr->count, 1, c->d_cov, c->st));
    if (continue_on(c))  // the seed's states
        HIPCHK(c, c->k->violations(c->P, c->B, 0, c->h_ctr->count, c->d_viol, c->st));
    if (pred_on(c)) {  // the seed's states: a predicate Init fails is the target, at depth 1
        if (int rc = pred_pass(c, 0, c->h_ctr->count)) return rc;
        if (int rc = pred_scan(c, 1)) return rc;
    }
    if (cons_on(c))
        if (int rc = cons_scan(c, 1, 0)) return rc;
    return 0;
}

int rmc_run_bfs(rmc_ctx* c, rmc_progress_fn cb, void* user) {
    if (!c) return RMC_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the state graph calls (rmc_graph.cpp) read a completed run only: its index is built on demand
    c->run_done = 0;
    c->run_cons = cons_on(c) ? 1 : 0;
    c->act_hit = 0;
    c->graph_idx = 0;
    c->run_seed = c->cfg.seed;
    if (c->wide || c->dist.on) {
        const int rc = c->wide ? run_bfs_wide(c, cb, user) : run_bfs_sharded(c, cb, user);
        c->run_done = rc == 0;
        return rc;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const bool resume = c->resume != 0;  // rmc_recover restored store, set and counters
    c->resume = 0;
    c->have_target = 0;
    c->stop = 0;
    c->cov_valid = 0;
    c->viol_valid = 0;
    const bool cover = cover_on(c);  // (rmc_recover refuses the flags: never a resumed run)
    const bool cont = continue_on(c);
    const bool preds = pred_on(c);  // (rmc_recover refuses a ctx with predicates too)
    const bool cons = cons_on(c);   // (and one with constraints)
    const bool acts = act_on(c);    // (and one with action properties; never with cons: rmc_set_actions)
    int depth = 0;
    if (resume) {
        c->res.left_on_queue = 0;
        c->res.seconds = 0;
        HIPCHK(c, set_fp_salt(*c->k, c->cfg.seed, c->set_epoch, c->st));
        c->h_ctr->count = c->level_start.back();
        if (int rc = reset_counters(c, true)) return rc;
        depth = c->resume_depth;
    } else if (int rc = start_run(c, &depth)) {
        return rc;
    }
    // states per expansion launch: at most 2^kMaxLaunchLog2 (B.word holds one launch's
    // presorted positions), so a level is one launch, or beyond that cut into EQUAL
    // launches: no launch is a small remainder that leaves most of the resident grid idle
    // (RMC_LAUNCH_LOG2: a smaller cap, A/B)
    static const u64 CHUNK = [] {
        const char* e = getenv("RMC_LAUNCH_LOG2");
        const int l = e ? std::max(16, std::min(kMaxLaunchLog2, atoi(e))) : kMaxLaunchLog2;
        return 1ull << l;
    }();
    const LevelText text = {"verification: a stored state has no fingerprint slot", "symmetry tie buffer full", "states",
                            &c->walked};
    for (int more = depth > 0; more && !c->stop;) {  // (depth 0: the constraint dropped the initial state)
        const u64 lo = c->level_start[depth - 1], hi = c->level_start[depth];
        if (lo == hi) break;  // fixpoint
        if (c->cfg.max_depth > 0 && depth >= c->cfg.max_depth) {
            c->res.left_on_queue = hi - lo;
            break;
        }
        if (int rc = reset_counters(c, true)) return rc;
        HIPCHK(c, hipEventRecord(c->ev0, c->st));
        // verification mode: smaller launches, each followed by publishing its
        // new states (k_publish) and checking its deferred hits (k_verify)
        // SYMMETRY: every lane of a launch could defer a tied successor, so a
        // launch holds at most tie_cap / lanes states (5.6 M for S = 3, K = 4):
        // the tie buffer cannot overflow whatever the model's tie rate
        const u64 sym_chunk = c->sh.sym ? std::max<u64>(1, std::min<u64>(CHUNK, c->B.tie_cap / (u64)c->P.off[10])) : CHUNK;
        const u64 chunk = c->sh.verify ? (1ull << 20) : c->sh.sym ? sym_chunk : CHUNK;
        const u64 nlaunch = (hi - lo + chunk - 1) / chunk;
        const u64 even = (hi - lo + nlaunch - 1) / nlaunch;  // <= chunk
        for (u64 a = lo, b = 0; a < hi; a = b) {
            b = std::min(hi, a + even);
            // the ring's device-side admission (rmc_plan.h): a launch the bound would cut is
            // launched whole when its reserve fits, and launched again from where it stopped
            const bool ring = c->spill.on && c->spill.dev_links;
            bool admit = false, abort_level = false;
            u64 live_lo = a, reserve = 0, units = 0;
            ShapeKernels::AdmitShape as{};
            if (c->spill.on) {
                // a state yields at most `bound` new states; verification parks
                // every hit of a launch on a spilled owner in hbuf
                const u64 bound = max_new_per_state(c), count = c->h_ctr->count;
                u64 want = b - a;
                if (c->sh.verify) want = std::min(want, c->B.hcap / bound);
                if (c->spill.dev_links) {
                    // the ring window: nothing is ever moved (rmc_plan.h ring_room)
                    const u64 win = c->spill.win;
                    want = std::min(want, ring_room(count, a, win) / bound);
                    if (want < b - a && !c->sh.verify && !c->sh.sym) {  // (the dynamic-unit kernel's searches)
                        as = c->k->admit_shape(b - a);
                        units = rmc_units::units_total(b - a, as.wt, as.ut);
                        reserve = admit_needs_reserve(c->B.cap, a, win)
                                      ? admit_reserve(as.grid * 4, units, unit_states(as.wt, as.ut), bound, as.list_cap)
                                      : 0;
                        admit = reserve <= kAdmitReserveMax &&
                                admit_fits(count, admit_stop(launch_store_limit(c->B.cap, true, a, win), reserve));
                    }
                    if (c->sh.verify && want) {
                        // the launch may overwrite the ring slots of states below
                        // count + n * bound - win (<= a): copy them to the host first, and
                        // send hits on them to hbuf
                        const u64 top = count + want * bound;
                        const u64 vlo = top > win ? top - win : 0;
                        if (int rc = verify_copy_out(c, vlo)) return rc;
                        c->B.vlo = vlo;
                    }
                } else {
                    // the linear window: a launch of n states stays inside it when
                    // n * bound <= its room.  Launches shrink as the window fills;
                    // below 2^20 states the expanded states [base, a) move to the
                    // host first — once they are at least 1/8 of what the move
                    // shifts down (or nothing fits)
                    const u64 fit = (c->B.cap - count) / bound, old = a - c->spill.base;
                    const bool due = fit < std::min<u64>(b - a, 1ull << 20) && old && (old * 8 >= count - a || fit == 0);
                    if (due)
                        if (int rc = spill_to(c, a, count)) return rc;
                    want = std::min(want, (c->B.cap - count) / bound);
                    if (c->sh.verify) c->B.vlo = c->spill.base;  // [0, base) were copied to the host by spill_to
                }
                // the reserve does not fit (or no admission in this search): sized by the bound
                if (!admit) {
                    if (want == 0) return window_too_small(c, c->spill.win, slot_bytes(c->sh.verify));
                    b = a + want;
                }
            }
            for (bool resumed = false;; resumed = true) {
                c->B.lim = launch_store_limit(c->B.cap, ring, live_lo, c->spill.win);
                c->B.admit_reserve = admit ? (u32)reserve : 0u;
                // coverage reads Counters.count back after every launch, so it is current here
                const u64 cov_before = c->h_ctr->count;
                if (resumed) {
                    HIPCHK(c, c->k->expand_resume(expand_params(c), c->PT, c->B, a, b, c->st));
                } else {
                    HIPCHK(c, c->k->expand(c->sh.sym, c->sh.verify, expand_params(c), c->PT, c->B, a, b, c->st));
                }
                c->res.expand_launches += 1;
                if (c->sh.sym && !c->sh.verify) {
                    HIPCHK(c, c->k->ties(expand_params(c), c->PT, c->B, c->st));
                    HIPCHK(c, hipMemsetAsync(&c->B.ctr->nties, 0, 8, c->st));
                }
                if (c->sh.verify) {
                    const u64 before = c->h_ctr->count;
                    if (int rc = read_counters(c)) return rc;
                    if (c->h_ctr->overflow) { abort_level = true; break; }
                    HIPCHK(c, c->k->publish(c->sh.sym, c->P, c->PT, c->B, before, c->h_ctr->count, c->st));
                    HIPCHK(c, c->k->verify(c->sh.sym, c->P, c->PT, c->B, c->h_ctr->vcount, c->st));
                    HIPCHK(c, hipMemsetAsync(&c->B.ctr->vcount, 0, 8, c->st));
                    c->h_ctr->vcount = 0;
                    if (c->h_ctr->hcount)  // hits on spilled owners: against their host copies
                        if (int rc = verify_host_hits(c, c->h_ctr->hcount)) return rc;
                }
                if (c->spill.on) {
                    if (int rc = read_counters(c)) return rc;
                    if (c->h_ctr->overflow || c->h_ctr->table_full) { abort_level = true; break; }
                    if (c->h_ctr->count > c->spill.total_cap)
                        return fail(c, RMC_E_CAPACITY, "spill: more states than rmc_config.state_capacity (" +
                                                           std::to_string(c->spill.total_cap) + ")");
                    if (c->spill.dev_links) {  // the ring: states below count - win are overwritten
                        const u64 cnt = c->h_ctr->count, win = c->spill.win;
                        c->spill.base = cnt > win ? cnt - win : 0;
                        c->res.spilled = c->spill.base;
                        c->res.spills = cnt / win;  // passes of the ring
                    }
                }
                if (cover || cont || preds || cons || acts) {
                    // the coverage pass of this launch: its parents [a, b) are still resident
                    // (the store; the linear window, which moves only [base, a) and before the
                    // launch; the ring, whose room is relative to a: a launch stopped on
                    // admission tallies all its parents here, its re-launches none), and the
                    // states it added are [count before, count after) — after k_ties, Publish / Verify.  The
                    // violation pass and the predicate pass read those states: resident too
                    // (ring_room keeps a launch's new states inside the window)
                    if (!c->sh.verify && !c->spill.on) {  // (those paths have read the counters)
                        if (int rc = read_counters(c)) return rc;
                        if (c->h_ctr->overflow || c->h_ctr->table_full) { abort_level = true; break; }
                    }
                    // the constraint pass first: whatever follows reads the kept states only (it
                    // reads the counters back: count = the kept states' end)
                    if (cons)
                        if (int rc = cons_pass(c, cov_before, c->h_ctr->count)) return rc;
                    if (cover)
                        HIPCHK(c, c->k->cover(c->P, c->B, resumed ? b : a, b, cov_before, c->h_ctr->count, 0, c->d_cov,
                                              c->st));
                    if (cont) HIPCHK(c, c->k->violations(c->P, c->B, cov_before, c->h_ctr->count, c->d_viol, c->st));
                    if (preds)
                        if (int rc = pred_pass(c, cov_before, c->h_ctr->count)) return rc;
                    // the action properties: the launch's parents, as coverage walks them (a
                    // launch stopped on admission checks all its parents here, its re-launches none)
                    if (acts)
                        if (int rc = act_pass(c, resumed ? b : a, b)) return rc;
                }
                // a launch that stopped on admission left units unclaimed (every claimed one is
                // finished): again over [a, b), live from the first window not fully claimed
                const u64 claimed = rmc_units::units_claimed(c->h_ctr->wnext);
                if (!admit || claimed >= units) break;
                live_lo = admit_live_lo(a, b - a, claimed, as.wt, 4ull * rmc_units::unit_groups(as.wt, as.ut));
                reserve = admit_needs_reserve(c->B.cap, live_lo, c->spill.win)
                              ? admit_reserve(as.grid * 4, units - claimed, unit_states(as.wt, as.ut),
                                              max_new_per_state(c), as.list_cap)
                              : 0;
                if (!admit_fits(c->h_ctr->count,
                                admit_stop(launch_store_limit(c->B.cap, true, live_lo, c->spill.win), reserve)))
                    return window_too_small(c, c->spill.win, slot_bytes(c->sh.verify));
                // the work counter without its stop bit and the count of the waves that left
                c->h_ctr->wnext = claimed;
                HIPCHK(c, hipMemcpyAsync(&c->B.ctr->wnext, &c->h_ctr->wnext, 8, hipMemcpyHostToDevice, c->st));
            }
            if (abort_level) break;
        }
        if (int rc = end_level(c, hi, &depth, cb, user, t0, text, &more)) return rc;
    }
    c->res.distinct = c->level_start.back();
    c->res.depth = depth;
    c->res.verified_spilled = c->spill.host_hits;
    if (cover)
        if (int rc = cover_end(c)) return rc;
    if (cont)
        if (int rc = viol_end(c)) return rc;
    if (cons)
        if (int rc = cons_end(c)) return rc;
    const double D = (double)c->res.distinct, G = (double)c->res.generated;
    // TLC's "calculated (optimistic)" fingerprint-collision estimate
    c->res.collision_probability = fp_collision_estimate(D, G, c->table_slots, c->set_epoch != 0);
    c->res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    // lane efficiency of the walk: enabled lanes / visited slots (the kernels count
    // the slots only when built with -DRMC_WALK_STATS_BUILD: a register in the hot loop)
    if (getenv("RMC_WALK_STATS"))
        fprintf(stderr, "[rmc] lane walk: %llu slots visited, %llu generated, %llu probes: efficiency %.4f\n",
                (unsigned long long)c->walked, (unsigned long long)c->res.generated,
                (unsigned long long)c->res.probes, c->walked ? G / (double)c->walked : 0.0);
    c->run_done = 1;
    c->graph_idx = c->sh.verify ? 1 : 0;  // verification published every stored state (k_publish)
    return 0;
}

int rmc_set_seed(rmc_ctx* c, uint64_t seed) {
    if (!c) return RMC_E_INVAL;
    c->cfg.seed = seed;
    return 0;
}

int rmc_set_fp_bits(rmc_ctx* c, int32_t bits) {
    if (!c || bits < 1 || bits > 64) return RMC_E_INVAL;
    if (!c->sh.verify) return fail(c, RMC_E_INVAL, "rmc_set_fp_bits needs RMC_FLAG_VERIFY_STATES");
    c->P.fp_mask = bits == 64 ? ~0ull : ((1ull << bits) - 1);
    return 0;
}

int rmc_get_coverage(const rmc_ctx* c, rmc_coverage* out) {
    if (!c || !out) return RMC_E_INVAL;
    rmc_ctx* m = const_cast<rmc_ctx*>(c);  // (only the message is written)
    if (!cover_on(c)) return fail(m, RMC_E_STATE, "rmc_get_coverage: the ctx was created without RMC_FLAG_COVERAGE");
    if (!c->cov_valid) return fail(m, RMC_E_STATE, "rmc_get_coverage: no completed rmc_run_bfs to report");
    *out = c->cov;
    return 0;
}

const char* rmc_coverage_action(int32_t row) {
    static const char* const kRows[RMC_COV_ACTIONS] = {
        "Init", "Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest", "AdvanceCommitIndex",
        "AppendEntries", "UpdateTerm", "Receive:RequestVoteRequest", "Receive:RequestVoteResponse",
        "Receive:AppendEntriesRequest", "Receive:AppendEntriesResponse", "DuplicateMessage", "DropMessage"};
    return row >= 0 && row < RMC_COV_ACTIONS ? kRows[row] : nullptr;
}

int rmc_get_violations(const rmc_ctx* c, rmc_violations* out) {
    if (!c || !out) return RMC_E_INVAL;
    rmc_ctx* m = const_cast<rmc_ctx*>(c);  // (only the message is written)
    if (!continue_on(c)) return fail(m, RMC_E_STATE, "rmc_get_violations: the ctx was created without RMC_FLAG_CONTINUE");
    if (!c->viol_valid) return fail(m, RMC_E_STATE, "rmc_get_violations: no completed rmc_run_bfs to report");
    *out = c->viol;
    return 0;
}

int rmc_get_result(const rmc_ctx* c, rmc_result* out) {
    if (!c || !out) return RMC_E_INVAL;
    *out = c->res;
    return 0;
}

}  // extern "C"

// The counterexample to the single-GPU state `target`: parent links back to Init,
// then the states.  States whose store was spilled are re-derived by replaying the
// recorded lanes from the last state still known (Init at worst) with the listing
// kernel — the stored successor of a parent through a lane is exactly what it lists.
static int trace_to(rmc_ctx* c, u64 target, rmc_state_view* states, int32_t* families, int32_t* instances, size_t cap,
                    size_t* len, std::vector<u32>* last = nullptr) {
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->wide) return trace_wide(c, target, states, families, instances, cap, len);
    std::vector<u64> chain;
    std::vector<uint8_t> acts;
    if (int rc = walk_links(c, target, [c](u64 i, u64* p, uint8_t* a) { return read_link(c, i, p, a); }, &chain, &acts))
        return rc;
    *len = chain.size();
    const u64 NW = (u64)c->NW, RW = 6 + NW, lanes = (u64)c->P.off[10];
    std::vector<u32> cur(NW);
    DevScratch<u32> d_in, d_out;  // replay buffers, allocated by the first replayed state
    DevScratch<unsigned long long> d_cnt;
    for (size_t q = 0; q < chain.size(); ++q) {
        if (!c->spill.on || chain[q] >= c->spill.base) {
            HIPCHK(c, hipMemcpy(cur.data(), c->B.store + wslot(c->B, chain[q]) * NW, NW * 4, hipMemcpyDeviceToHost));
        } else if (q == 0) {  // Init (raft.tla:125-129), the one initial state
            rmc_state_view iv;
            init_view(c->cfg, &iv);
            std::string why;
            if (encode_view(c->sh.S, c->sh.K, iv, cur.data(), &why)) return fail(c, RMC_E_INVAL, why);
        } else {  // replay lane acts[q] from the previous state on the device
            if (!d_in.get() && (d_in.alloc(NW) != hipSuccess || d_out.alloc(lanes * RW) != hipSuccess ||
                                d_cnt.alloc(1) != hipSuccess))
                return fail(c, RMC_E_NOMEM, "trace: replay buffers");
            std::vector<u32> recs(lanes * RW);
            unsigned long long n = 0;
            if (hipMemcpy(d_in.get(), cur.data(), NW * 4, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemset(d_cnt.get(), 0, 8) != hipSuccess ||
                c->k->list(c->sh.sym, c->P, c->PT, d_in.get(), 1, d_out.get(), lanes, d_cnt.get(), c->st) != hipSuccess ||
                hipStreamSynchronize(c->st) != hipSuccess ||
                hipMemcpy(&n, d_cnt.get(), 8, hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(recs.data(), d_out.get(), std::min<u64>(n, lanes) * RW * 4, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(c, RMC_E_HIP, "trace: replay launch failed");
            bool found = false;
            for (u64 r = 0; r < std::min<u64>(n, lanes) && !found; ++r) {
                const u32* rec = &recs[r * RW];
                found = rec[2] == acts[q] && rec[3];
                if (found) memcpy(cur.data(), rec + 6, NW * 4);
            }
            if (!found) return fail(c, RMC_E_STATE, "trace: a recorded lane is not enabled on replay");
        }
        if (q < cap) {
            if (states) decode_state(c->sh.S, c->sh.K, cur.data(), &states[q]);
            fill_step(families, instances, q, family_of(c->P, acts[q]), acts[q]);
        }
    }
    if (last) *last = cur;  // the target's packed words
    return 0;
}

extern "C" {

int rmc_trace(rmc_ctx* c, rmc_state_view* states, int32_t* families, int32_t* instances, size_t cap, size_t* len) {
    if (!c || !len) return RMC_E_INVAL;
    if (!c->have_target) return fail(c, RMC_E_STATE, "no violation or deadlock to trace");
    if (c->dist.on && !c->wide) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        return trace_sharded(c, states, families, instances, cap, len);
    }
    if (c->act_hit) {
        // an action property: the path to the source, then the violating transition's successor,
        // recomputed from the stored source through the lane code
        std::vector<u32> src, nxt((size_t)c->NW);
        if (int rc = trace_to(c, c->target_idx, states, families, instances, cap, len, &src)) return rc;
        if (int rc = act_successor(c, src.data(), c->act_lane, nxt.data())) return rc;
        const size_t q = (*len)++;
        if (q < cap) {
            if (states) decode_state(c->sh.S, c->sh.K, nxt.data(), &states[q]);
            fill_step(families, instances, q, family_of(c->P, c->act_lane), (uint8_t)c->act_lane);
        }
        return 0;
    }
    return trace_to(c, c->target_idx, states, families, instances, cap, len);
}

int rmc_trace_violation(rmc_ctx* c, uint32_t inv_bit, rmc_state_view* states, int32_t* families, int32_t* instances,
                        size_t cap, size_t* len) {
    if (!c || !len) return RMC_E_INVAL;
    if (!continue_on(c))
        return fail(c, RMC_E_STATE, "rmc_trace_violation: the ctx was created without RMC_FLAG_CONTINUE");
    if (!inv_bit || (inv_bit & (inv_bit - 1)) || !(inv_bit & c->cfg.invariants))
        return fail(c, RMC_E_INVAL, "rmc_trace_violation: inv_bit must be one RMC_INV_* bit of the ctx's invariants");
    if (!c->viol_valid) return fail(c, RMC_E_STATE, "rmc_trace_violation: no completed rmc_run_bfs to report");
    const int r = __builtin_ctz(inv_bit);
    if (!c->viol.each[r]) return fail(c, RMC_E_STATE, "rmc_trace_violation: no stored state violates this invariant");
    return trace_to(c, c->viol_least[r], states, families, instances, cap, len);
}

}  // extern "C"

// ---- simulation: random walks from Init or SmokeInit (rmc_codec.cpp) -----------
namespace {

int run_sim(rmc_ctx* c, const rmc_sim_config* sc, rmc_sim_result* out, i64 rec_beh, std::vector<u32>* rec,
            std::vector<rmc_state_view>* wrec = nullptr) {
    if (!c || !sc || !out || sc->behaviours == 0 || sc->depth < 1 ||
        (sc->mode != RMC_SIM_WITHIN_CAPACITY && sc->mode != RMC_SIM_TRUNCATE && sc->mode != RMC_SIM_TLC))
        return RMC_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (pred_on(c))
        return fail(c, RMC_E_STATE, "simulation does not evaluate model-defined invariants (rmc_set_predicates(ctx, NULL) "
                                    "removes them)");
    if (cons_on(c))
        return fail(c, RMC_E_STATE, "simulation does not evaluate model-defined constraints (rmc_set_constraints(ctx, "
                                    "NULL) removes them)");
    if (act_on(c))
        return fail(c, RMC_E_STATE, "simulation does not evaluate action properties (rmc_set_actions(ctx, NULL) removes "
                                    "them)");
    if (c->wide) return sim_wide(c, sc, out, rec_beh, wrec);
    if (sc->mode == RMC_SIM_TLC)
        return fail(c, RMC_E_INVAL, "RMC_SIM_TLC draws on the wide layout only (bounds beyond the packed capacity)");
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<u32> inits;
    std::string why;
    if (sc->smoke_k > 0) {
        if (int rc = smoke_init(smoke_shape(c->cfg, false), *sc, &inits, &why)) return fail(c, rc, why);
    } else {
        rmc_state_view iv;
        init_view(c->cfg, &iv);
        inits.assign((size_t)c->NW, 0u);
        if (int rc = encode_view(c->sh.S, c->sh.K, iv, inits.data(), &why)) return fail(c, rc, why);
    }
    const u64 n_init = inits.size() / (u64)c->NW;
    // The model's bounds, as TLC's simulator respects a state CONSTRAINT; a
    // simulation model without one gets the packed capacity from the front-end
    // (rmc_model_from_files with RMC_FRONT_SIMULATE), so walks never exceed
    // what a state can hold.
    Params P = c->P;
    P.max_msgs = std::min(P.max_msgs, c->sh.K);
    DevScratch<u32> d_init, d_rec;
    DevScratch<SimCounters> d_out;
    HIPCHK(c, d_init.alloc(inits.size()));
    HIPCHK(c, d_out.alloc(1));
    if (rec) HIPCHK(c, d_rec.alloc((size_t)sc->depth * c->NW));
    HIPCHK(c, hipMemcpy(d_init.get(), inits.data(), inits.size() * 4, hipMemcpyHostToDevice));
    SimCounters h;
    float ms = 0.f;
    if (int rc = sim_timed(c, d_out.get(), &h, &ms, [&] {
            return c->k->simulate(P, d_init.get(), n_init, sc->behaviours, sc->depth, sc->seed, sc->mode, d_out.get(),
                              rec_beh, d_rec.get(), c->st);
        }))
        return rc;
    if (rec) {
        rec->assign((size_t)(h.steps + 1) * c->NW, 0u);
        HIPCHK(c, hipMemcpy(rec->data(), d_rec.get(), rec->size() * 4, hipMemcpyDeviceToHost));
    }
    fill_sim_result(out, h, rec ? 1 : sc->behaviours, n_init, ms, t0);
    return 0;
}

}  // namespace

extern "C" {

int rmc_simulate(rmc_ctx* c, const rmc_sim_config* sc, rmc_sim_result* out) { return run_sim(c, sc, out, -1, nullptr); }

int rmc_smoke_init(const rmc_config* cfg, const rmc_sim_config* sc, rmc_state_view* states, size_t cap, size_t* n) {
    if (!cfg || !sc || !n || sc->smoke_k < 1) return RMC_E_INVAL;
    std::string why;
    if (validate(cfg, &why)) return RMC_E_INVAL;
    const SmokeShape m = smoke_shape(*cfg, wide_wanted(*cfg));
    if (m.wide) {
        std::vector<rmc_state_view> views;
        if (smoke_views(m, *sc, &views, &why)) return RMC_E_INVAL;
        *n = views.size();
        for (size_t q = 0; q < *n && q < cap && states; ++q) states[q] = views[q];
        return 0;
    }
    std::vector<u32> packed;
    if (smoke_init(m, *sc, &packed, &why)) return RMC_E_INVAL;
    const size_t NW = (size_t)(2 * m.n_servers + m.bag);
    *n = packed.size() / NW;
    for (size_t q = 0; q < *n && q < cap && states; ++q)
        decode_state(m.n_servers, m.bag, packed.data() + q * NW, &states[q]);
    return 0;
}

int rmc_sim_replay(rmc_ctx* c, const rmc_sim_config* sc, uint64_t behaviour, rmc_state_view* states, size_t cap,
                   size_t* len) {
    if (!c || !sc || !len || behaviour >= sc->behaviours) return RMC_E_INVAL;
    rmc_sim_result r;
    std::vector<u32> rec;
    if (c->wide) {
        std::vector<rmc_state_view> wrec;
        if (int rc = run_sim(c, sc, &r, (i64)behaviour, nullptr, &wrec)) return rc;
        *len = wrec.size();
        for (size_t q = 0; q < *len && q < cap; ++q) states[q] = wrec[q];
        return 0;
    }
    if (int rc = run_sim(c, sc, &r, (i64)behaviour, &rec)) return rc;
    *len = rec.size() / (size_t)c->NW;
    for (size_t q = 0; q < *len && q < cap; ++q) decode_state(c->sh.S, c->sh.K, rec.data() + q * c->NW, &states[q]);
    return 0;
}

int rmc_probe_bench(int device, uint64_t table_bytes, uint64_t accesses, int mode, double* per_second) {
    if (!per_second || table_bytes < 4096 || accesses == 0 || (mode != 0 && mode != 1)) return RMC_E_INVAL;
    if (hipSetDevice(device) != hipSuccess) return RMC_E_NOGPU;
    u64 slots = 1;
    while (slots * 2 * 8 <= table_bytes) slots <<= 1;
    DevScratch<u64> table, sink;
    const u64 threads = 256ull * 2048;                       // 8 blocks of 256 per CU
    const u32 iters = (u32)std::max<u64>(1, accesses / (threads * 8));
    float ms = 0.f;
    if (table.alloc(slots) != hipSuccess || sink.alloc(1) != hipSuccess) return RMC_E_NOMEM;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool ok =
        hipStreamCreate(&st) == hipSuccess && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess &&
        hipMemsetAsync(table.get(), 0, slots * 8, st) == hipSuccess &&
        // warm-up launch (page mapping, clocks), then the timed one
        launch_probe_bench(table.get(), slots - 1, threads, 1, mode, sink.get(), st) == hipSuccess &&
        hipEventRecord(e0, st) == hipSuccess &&
        launch_probe_bench(table.get(), slots - 1, threads, iters, mode, sink.get(), st) == hipSuccess &&
        hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
        hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (st) (void)hipStreamDestroy(st);
    if (!ok) return RMC_E_HIP;
    *per_second = (double)threads * 8.0 * iters / (1e-3 * ms);
    return 0;
}

int rmc_expand(rmc_ctx* c, const rmc_state_view* states, size_t n, rmc_succ_view* out, size_t cap, size_t* n_out) {
    if (!c || (!states && n) || !n_out) return RMC_E_INVAL;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    *n_out = 0;
    if (n == 0) return 0;
    if (c->wide) return expand_wide(c, states, n, out, cap, n_out);
    const int NW = c->NW, RW = 6 + NW;
    std::vector<u32> packed(n * (size_t)NW);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_view(c->sh.S, c->sh.K, states[t], packed.data() + t * NW, &why))
            return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    const u64 lanes = (u64)c->P.off[10];
    const u64 rcap = std::max<u64>(1, std::min<u64>((u64)cap, n * lanes));
    DevScratch<u32> d_in, d_out;
    DevScratch<unsigned long long> d_cnt;
    HIPCHK(c, d_in.alloc(packed.size()));
    HIPCHK(c, d_out.alloc(rcap * (u64)RW));
    HIPCHK(c, d_cnt.alloc(1));
    HIPCHK(c, hipMemcpy(d_in.get(), packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(d_cnt.get(), 0, 8));
    HIPCHK(c, c->k->list(c->sh.sym, c->P, c->PT, d_in.get(), (u64)n, d_out.get(), rcap, d_cnt.get(), c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    unsigned long long cnt = 0;
    HIPCHK(c, hipMemcpy(&cnt, d_cnt.get(), 8, hipMemcpyDeviceToHost));
    const u64 got = std::min<u64>(cnt, rcap);
    std::vector<u32> recs(got * (u64)RW);
    if (got) HIPCHK(c, hipMemcpy(recs.data(), d_out.get(), recs.size() * 4, hipMemcpyDeviceToHost));
    // deterministic order: (parent, lane)
    std::vector<u64> order(got);
    for (u64 q = 0; q < got; ++q) order[q] = q;
    std::sort(order.begin(), order.end(), [&](u64 a, u64 b) {
        const u32* ra = &recs[a * RW];
        const u32* rb = &recs[b * RW];
        const u64 pa = (u64)ra[0] | ((u64)ra[1] << 32), pb = (u64)rb[0] | ((u64)rb[1] << 32);
        return pa != pb ? pa < pb : ra[2] < rb[2];
    });
    for (u64 q = 0; q < got && q < cap; ++q) {
        const u32* r = &recs[order[q] * RW];
        rmc_succ_view& s = out[q];
        memset(&s, 0, sizeof s);
        s.parent = (u64)r[0] | ((u64)r[1] << 32);
        s.instance = (int)r[2];
        s.family = family_of(c->P, (int)r[2]);
        s.in_constraint = (int)r[3];
        s.fingerprint = (u64)r[4] | ((u64)r[5] << 32);
        if (s.in_constraint) decode_state(c->sh.S, c->sh.K, r + 6, &s.state);
    }
    *n_out = (size_t)cnt;
    return 0;
}

int rmc_check_states(rmc_ctx* c, const rmc_state_view* states, size_t n, uint32_t invariants, int32_t* violated) {
    if (!c) return RMC_E_INVAL;
    if (n && (!states || !violated)) return fail(c, RMC_E_INVAL, "rmc_check_states: states or violated is NULL");
    if (invariants & ~1023u) return fail(c, RMC_E_INVAL, "rmc_check_states: unknown invariant bit");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n == 0) return 0;
    const uint32_t mask = invariants ? invariants : c->cfg.invariants;
    if (c->wide) return check_wide(c, states, n, mask, violated);
    const int NW = c->NW;
    std::vector<u32> packed(n * (size_t)NW);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_view(c->sh.S, c->sh.K, states[t], packed.data() + t * NW, &why))
            return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    Params P = c->P;
    P.inv_mask = (int)mask;
    DevScratch<u32> d_in;
    DevScratch<int> d_out;
    HIPCHK(c, d_in.alloc(packed.size()));
    HIPCHK(c, d_out.alloc(n));
    HIPCHK(c, hipMemcpy(d_in.get(), packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, c->k->check(P, d_in.get(), (u64)n, d_out.get(), c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    std::vector<int> v(n);
    HIPCHK(c, hipMemcpy(v.data(), d_out.get(), n * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < n; ++t) violated[t] = v[t] ? 1 << (v[t] - 1) : 0;
    return 0;
}

int rmc_state_keys(rmc_ctx* c, const rmc_state_view* states, size_t n, uint64_t* keys, const uint32_t* ref,
                   uint8_t* same) {
    if (!c) return RMC_E_INVAL;
    // a wide ctx: under SYMMETRY (the canonical keys this hook exists for); without it the
    // refusal of ABI 11 stands
    if (c->wide && !c->WB.sym)
        return fail(c, RMC_E_INVAL, "rmc_state_keys: the packed layout only, or a wide ctx under RMC_FLAG_SYMMETRY");
    if (n && (!states || !keys || (ref && !same)))
        return fail(c, RMC_E_INVAL, "rmc_state_keys: states, keys or same is NULL");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (n == 0) return 0;
    for (size_t t = 0; ref && t < n; ++t)
        if (ref[t] >= n) return fail(c, RMC_E_INVAL, "rmc_state_keys: ref[" + std::to_string(t) + "] is not below n");
    if (c->wide) return keys_wide(c, states, n, keys, ref, same);
    const int NW = c->NW;
    std::vector<u32> packed(n * (size_t)NW);
    std::string why;
    for (size_t t = 0; t < n; ++t)
        if (encode_view(c->sh.S, c->sh.K, states[t], packed.data() + t * NW, &why))
            return fail(c, RMC_E_INVAL, "state " + std::to_string(t) + ": " + why);
    DevScratch<u32> d_in, d_ref;
    DevScratch<u64> d_keys;
    DevScratch<unsigned char> d_same;
    HIPCHK(c, d_in.alloc(packed.size()));
    HIPCHK(c, d_keys.alloc(n));
    HIPCHK(c, hipMemcpy(d_in.get(), packed.data(), packed.size() * 4, hipMemcpyHostToDevice));
    if (ref) {
        HIPCHK(c, d_ref.alloc(n));
        HIPCHK(c, d_same.alloc(n));
        HIPCHK(c, hipMemcpy(d_ref.get(), ref, n * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(c, c->k->keys(c->sh.sym, c->P, c->PT, d_in.get(), (u64)n, d_keys.get(), ref ? d_ref.get() : nullptr,
                         ref ? d_same.get() : nullptr, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, hipMemcpy(keys, d_keys.get(), n * 8, hipMemcpyDeviceToHost));
    if (ref) HIPCHK(c, hipMemcpy(same, d_same.get(), n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
