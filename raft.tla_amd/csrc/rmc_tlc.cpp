// rmc_tlc.cpp — `rmc-tlc`, a drop-in for `java tlc2.TLC` on raft.tla models.
//
// Same command line shape as TLC (`[-workers N] [-config X.cfg] [-depth N]
// [-deadlock] X.tla`) and the same summary lines, so scripts that grep TLC's
// output ("states generated", "distinct states found", "depth of the complete
// state graph", "Error: Invariant ... is violated", "State N:") keep working.
// It is the host side above the C ABI (include/rmc.h); Java users bind the
// same symbols through Panama.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "../../include/rmc.h"
#include "rmc_dump.h"

namespace {

const char* kFamilies[10] = {"Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest",
                             "AdvanceCommitIndex", "AppendEntries", "Receive", "DuplicateMessage", "DropMessage"};
const char* kRoles[3] = {"Follower", "Candidate", "Leader"};
const char* kMtypes[4] = {"RequestVoteRequest", "RequestVoteResponse", "AppendEntriesRequest",
                          "AppendEntriesResponse"};

std::string srv(int i) { return "r" + std::to_string(i + 1); }
std::string val(int v) { return "v" + std::to_string(v + 1); }

std::string seq(const rmc_entry* e, int n) {
    if (n == 0) return "<<>>";
    std::string s = "<<";
    for (int x = 0; x < n; ++x) {
        if (x) s += ", ";
        s += "[term |-> " + std::to_string(e[x].term) + ", value |-> " + val(e[x].value) + "]";
    }
    return s + ">>";
}

template <class F>
std::string fn(int S, F f) {  // (r1 :> f(0) @@ r2 :> f(1) ...)
    std::string s = "(";
    for (int i = 0; i < S; ++i) {
        if (i) s += " @@ ";
        s += srv(i) + " :> " + f(i);
    }
    return s + ")";
}

std::string set_of(uint32_t m, int S) {
    std::string s = "{";
    bool first = true;
    for (int i = 0; i < S; ++i)
        if (m >> i & 1) { s += (first ? "" : ", ") + srv(i); first = false; }
    return s + "}";
}

std::string msg(const rmc_msg_view& m) {
    std::string s = "[mtype |-> " + std::string(kMtypes[m.mtype]) + ", mterm |-> " + std::to_string(m.mterm);
    switch (m.mtype) {
        case 0: s += ", mlastLogTerm |-> " + std::to_string(m.mlastLogTerm) + ", mlastLogIndex |-> " +
                     std::to_string(m.mlastLogIndex); break;
        case 1: s += std::string(", mvoteGranted |-> ") + (m.mvoteGranted ? "TRUE" : "FALSE") + ", mlog |-> " +
                     seq(m.mlog, m.mlog_len); break;
        case 2: s += ", mprevLogIndex |-> " + std::to_string(m.mprevLogIndex) + ", mprevLogTerm |-> " +
                     std::to_string(m.mprevLogTerm) + ", mentries |-> " + seq(m.mentries, m.mentries_len) +
                     ", mcommitIndex |-> " + std::to_string(m.mcommitIndex); break;
        default: s += std::string(", msuccess |-> ") + (m.msuccess ? "TRUE" : "FALSE") + ", mmatchIndex |-> " +
                      std::to_string(m.mmatchIndex);
    }
    return s + ", msource |-> " + srv(m.msource) + ", mdest |-> " + srv(m.mdest) + "]";
}

// The state as TLC prints it: one "/\ var = value" line per variable.
std::string state_text(const rmc_state_view& v) {
    std::string out;
    auto line = [&](const char* var, const std::string& value) { out += std::string("/\\ ") + var + " = " + value + "\n"; };
    const int S = v.n_servers;
    std::string bag = v.n_msgs ? "(" : "<<>>";
    for (int q = 0; q < v.n_msgs; ++q) {
        if (q) bag += " @@ ";
        bag += msg(v.msgs[q]) + " :> " + std::to_string(v.msgs[q].count);
    }
    if (v.n_msgs) bag += ")";
    line("messages", bag);
    line("currentTerm", fn(S, [&](int i) { return std::to_string(v.currentTerm[i]); }));
    line("state", fn(S, [&](int i) { return std::string(kRoles[v.state[i]]); }));
    line("votedFor", fn(S, [&](int i) { return v.votedFor[i] < 0 ? std::string("Nil") : srv(v.votedFor[i]); }));
    line("log", fn(S, [&](int i) { return seq(v.log[i], v.log_len[i]); }));
    line("commitIndex", fn(S, [&](int i) { return std::to_string(v.commitIndex[i]); }));
    line("votesResponded", fn(S, [&](int i) { return set_of(v.votesResponded[i], S); }));
    line("votesGranted", fn(S, [&](int i) { return set_of(v.votesGranted[i], S); }));
    line("nextIndex", fn(S, [&](int i) { return fn(S, [&](int j) { return std::to_string(v.nextIndex[i][j]); }); }));
    line("matchIndex", fn(S, [&](int i) { return fn(S, [&](int j) { return std::to_string(v.matchIndex[i][j]); }); }));
    return out;
}

void print_state(const rmc_state_view& v) { fputs(state_text(v).c_str(), stdout); }

const char* inv_name(int bit) {
    switch (bit) {
        case RMC_INV_TYPEOK: return "TypeOK";
        case RMC_INV_ONE_LEADER: return "OneLeaderPerTerm";
        case RMC_INV_LOG_MATCHING: return "LogMatching";
        case RMC_INV_MESSAGES: return "MessagesInv";
        case RMC_INV_LEADER_VOTES: return "LeaderVotesQuorum";
        case RMC_INV_CAND_TERM: return "CandidateTermNotInLog";
        case RMC_INV_VOTES_GRANTED: return "VotesGrantedInv";
        case RMC_INV_QUORUM_LOG: return "QuorumLogInv";
        case RMC_INV_MORE_UP_TO_DATE: return "MoreUpToDateCorrect";
        case RMC_INV_LEADER_COMPLETE: return "LeaderCompleteness";
    }
    return "?";
}

// TLC's header of a behaviour step: the action of Next that produced the
// state and its location in raft.tla (the body of the action's definition;
// for Receive, the disjunct of raft.tla:393-403 that fired: UpdateTerm when
// the message's term is newer, else the one for its mtype).
std::string g_override_header;  // an override's action location (front-end notes), e.g. BugBecomeLeader

// `<shown line L1, col C1 to line L2, col C2 of module raft>` for an action key
// of rmc_action_location, `<shown>` when it has no location.
std::string action_header(const std::string& action, const std::string& shown) {
    if (action == "BecomeLeader" && !g_override_header.empty()) return g_override_header;
    int32_t loc[4];
    if (rmc_action_location(action.c_str(), loc) != 0) return "<" + shown + ">";
    char buf[256];
    snprintf(buf, sizeof buf, "<%s line %d, col %d to line %d, col %d of module raft>", shown.c_str(), loc[0], loc[1],
             loc[2], loc[3]);
    return buf;
}

std::string step_header(int family, int instance, const rmc_state_view& parent) {
    std::string action = kFamilies[family], shown = action;
    if (family == 7) {
        const int S = parent.n_servers;
        const int q = instance - (6 * S + 2 * S * S);  // Receive lanes start after the server families
        if (q >= 0 && q < parent.n_msgs) {
            const rmc_msg_view& m = parent.msgs[q];
            if (m.mterm > parent.currentTerm[m.mdest]) action = shown = "UpdateTerm";
            else action = std::string("Receive:") + kMtypes[m.mtype];
        }
    }
    return action_header(action, shown);
}

// TLC -coverage: one line per action of Next (and Init), `<header>: distinct:generated`,
// the headers those of the trace printer (a Receive disjunct is shown as Receive).
void print_coverage(const rmc_coverage& cv) {
    printf("The coverage statistics :\n");
    for (int row = 0; row < RMC_COV_ACTIONS; ++row) {
        const std::string action = rmc_coverage_action(row);
        const std::string shown = action.compare(0, 8, "Receive:") == 0 ? "Receive" : action;
        printf("%s: %llu:%llu\n", action_header(action, shown).c_str(), (unsigned long long)cv.distinct[row],
               (unsigned long long)cv.generated[row]);
    }
    printf("End of statistics.\n");
}

// -dump: the graph of the finished search, read back from the ctx (rmc.h "state graph export")
// and written by rmc_dump.h's writers.  Returns 0, or 1 after printing the error.
int write_dump(rmc_ctx* ctx, const std::string& file, bool dot, bool labels) {
    auto bad = [&](const char* what) {
        printf("Error: -dump: %s: %s\n", what, rmc_last_error(ctx));
        return 1;
    };
    size_t nl = 0;
    if (rmc_get_levels(ctx, nullptr, 0, &nl)) return bad("rmc_get_levels");
    std::vector<uint64_t> starts(nl);
    if (rmc_get_levels(ctx, starts.data(), nl, &nl)) return bad("rmc_get_levels");
    const uint64_t distinct = nl ? starts[nl - 1] : 0;
    std::vector<rmc_dump::Node> nodes(distinct);
    {
        const uint64_t chunk = 1024;
        std::vector<rmc_state_view> st((size_t)std::min<uint64_t>(chunk, distinct));
        std::vector<uint64_t> keys(st.size());
        size_t level = 1;  // level L = [starts[L - 1], starts[L])
        for (uint64_t a = 0; a < distinct; a += chunk) {
            const size_t m = (size_t)std::min<uint64_t>(chunk, distinct - a);
            if (rmc_read_states(ctx, a, m, st.data(), keys.data())) return bad("rmc_read_states");
            for (size_t t = 0; t < m; ++t) {
                while (a + t >= starts[level]) ++level;
                nodes[a + t] = rmc_dump::Node{keys[t], (int)level, state_text(st[t])};
            }
        }
    }
    std::vector<rmc_dump::Edge> edges;
    if (dot) {
        std::vector<rmc_edge> buf(1u << 20);
        const uint64_t chunk = 1u << 16;
        for (uint64_t a = 0; a < distinct; a += chunk) {
            const uint64_t b = std::min<uint64_t>(distinct, a + chunk);
            size_t n = 0;
            if (rmc_graph_edges(ctx, a, b, buf.data(), buf.size(), &n)) return bad("rmc_graph_edges");
            if (n > buf.size()) {
                buf.resize(n);
                if (rmc_graph_edges(ctx, a, b, buf.data(), buf.size(), &n)) return bad("rmc_graph_edges");
            }
            for (size_t q = 0; q < n; ++q) edges.push_back(rmc_dump::Edge{buf[q].src, buf[q].dst, buf[q].family, buf[q].instance});
        }
    }
    FILE* f = fopen(file.c_str(), "w");
    if (!f) {
        printf("Error: -dump: cannot write %s\n", file.c_str());
        return 1;
    }
    const bool ok = dot ? rmc_dump::write_dot(f, nodes, edges, kFamilies, 10, labels) : rmc_dump::write_states(f, nodes);
    if (fclose(f) != 0 || !ok) {
        printf("Error: -dump: writing %s failed\n", file.c_str());
        return 1;
    }
    if (dot) printf("State graph written to %s (%zu states, %zu transitions).\n", file.c_str(), nodes.size(), edges.size());
    else printf("States written to %s (%zu states).\n", file.c_str(), nodes.size());
    return 0;
}

int progress(const rmc_level_stats* s, void*) {
    printf("Progress(%d) at %.2fs: %llu states generated, %llu distinct states found, %llu states left on queue.\n",
           s->level + 1, s->seconds, (unsigned long long)s->generated, (unsigned long long)s->distinct,
           (unsigned long long)s->new_states);
    fflush(stdout);
    return 0;
}

int usage() {
    fprintf(stderr,
            "usage: rmc-tlc [-config X.cfg] [-depth N] [-deadlock] [-device D] [-capacity N] [-workers N]\n"
            "               [-verify] [-fpseed S] [-checkpoint F] [-recover F] [-simulate [num=N]] [-seed S]\n"
            "               [-raft raft.tla] [-builtin-raft] [-gpus N] [-nospill] [-window N] [-fpmem B]\n"
            "               [-coverage [minutes]] [-continue] [-dump [dot[,actionlabels]] FILE] X.tla\n"
            "  -dump FILE     write every distinct state found to FILE (TLC -dump)\n"
            "  -dump dot[,actionlabels] FILE  write the state graph to FILE in GraphViz dot format: a node per\n"
            "             state (its id the state's fingerprint), an edge per transition, labelled with its\n"
            "             action under actionlabels; colorize and snapshot are not supported.  FILE is\n"
            "             written as named (no extension is added).  Implies -nospill, and -capacity 2^26\n"
            "             unless given (the graph's state index takes 8 B per fingerprint-set slot);\n"
            "             single GPU, packed layout; not with -gpus N > 1, -simulate or -recover.  The\n"
            "             edges need a search that did not stop at a violation: use -continue\n"
            "  -continue      search past invariant violations (TLC -continue): violating states are kept\n"
            "             and expanded; after the search every violated invariant is reported with the\n"
            "             trace to its first state and the number of states that violate it (single\n"
            "             GPU; not with -checkpoint, -recover or -simulate; a wide-layout run then\n"
            "             keeps every state on the device, as under -nospill)\n"
            "  -coverage [M]  per-action statistics (TLC -coverage): for every action of Next the states it\n"
            "             generated and the distinct states it found; M, TLC's reporting interval in\n"
            "             minutes, is accepted and ignored (single GPU; not with -checkpoint, -recover\n"
            "             or -simulate)\n"
            "  -gpus N        shard the search over N GPUs (one ctx and RCCL rank per GPU)\n"
            "  -raft F        the raft.tla to verify against the compiled-in spec (default: next to X.tla)\n"
            "  -builtin-raft  no raft.tla on disk: check the compiled-in lemmy/raft.tla (said in the output)\n"
            "  -depth N   stop after N BFS levels (level N is left on the queue)\n"
            "  -verify    full-state verification: compare every fingerprint hit with the stored state\n"
            "             and report the collisions (both layouts; a wide-layout run then keeps every\n"
            "             state on the device, as under -nospill)\n"
            "  -nospill   keep every state on the device (stop with a capacity error when it fills);\n"
            "             by default expanded levels leave the device window (single GPU; their trace\n"
            "             links stay in HBM, or move to pinned host memory).  Runs on the wide layout\n"
            "             (-depth runs of models with unbounded fields, SYMMETRY Permutations(Server)\n"
            "             included) spill too, unless -verify\n"
            "  -window N  states kept on the device when spilling (default: what the set leaves;\n"
            "             the wide layout keeps exactly N records, the packed one rounds up to 2^k)\n"
            "  -fpseed S  fingerprint salt (TLC -fp: another member of the fingerprint family)\n"
            "  -fpmem B   bytes of HBM for the fingerprint set (TLC -fpmem; suffix K/M/G; it holds\n"
            "             B / 16 states, \"fingerprint set full\" past that); default: sized for the\n"
            "             largest store the device holds\n"
            "  -checkpoint F  write the search to F when it stops at -depth (TLC -checkpoint)\n"
            "  -recover F     continue the search saved in F (TLC -recover)\n"
            "  -simulate  random simulation (TLC -simulate; num=N behaviours, default 2^20;\n"
            "             -depth = states per behaviour, default 100; -seed = RNG seed)\n");
    return 2;
}

// TLC -simulate: random behaviours with the invariants checked on every state
// (Smokeraft.cfg:43-48 through rmc_sim_config_from_files).
int run_simulation(const std::string& cfg, const std::string& tla, const std::string& raft, uint32_t fopts, int device,
                   int depth, unsigned long long num, unsigned long long seed) {
    rmc_config c;
    rmc_sim_config sc;
    char info[2048];
    int rc = rmc_model_from_files(cfg.c_str(), tla.c_str(), raft.empty() ? nullptr : raft.c_str(),
                                  fopts | RMC_FRONT_SIMULATE, &c, &sc, info, sizeof info);
    if (rc) { printf("Error: %s\n", info); return 1; }
    if (info[0]) printf("%s\n", info);
    c.device = device;
    c.state_capacity = 1 << 12;  // no state store needed for walks
    if (depth > 0) sc.depth = depth;
    if (num > 0) sc.behaviours = num;
    sc.seed = seed;
    // a model that bounds no field (Smokeraft.cfg) walks on the wide layout with
    // TLC's draw (an action, then a successor); a bounded one within its bounds
    const bool wide = rmc_state_bytes(&c) > 64 * 4;
    if (wide) sc.mode = RMC_SIM_TLC;
    printf("Running Random Simulation with seed %llu: %llu behaviours of up to %d states, %s.\n",
           (unsigned long long)seed, (unsigned long long)sc.behaviours, sc.depth,
           sc.smoke_k ? "initial states from SmokeInit" : "initial state from Init");
    rmc_ctx* ctx = nullptr;
    rc = rmc_create(&c, &ctx);
    if (rc) { printf("Error: rmc_create failed (%d)\n", rc); return 1; }
    rmc_sim_result r;
    rc = rmc_simulate(ctx, &sc, &r);
    if (rc) { printf("Error: %s\n", rmc_last_error(ctx)); rmc_destroy(ctx); return 1; }
    if (sc.smoke_k) printf("SmokeInit: %llu initial states (k = %d).\n", (unsigned long long)r.init_states, sc.smoke_k);
    int exitcode = 0;
    if (r.violated_inv) {
        printf("Error: Invariant %s is violated.\n", inv_name(r.violated_inv));
        printf("Error: The behavior up to this point is:\n");
        std::vector<rmc_state_view> st((size_t)sc.depth);
        size_t len = 0;
        rmc_sim_replay(ctx, &sc, r.violation_behaviour, st.data(), st.size(), &len);
        for (size_t k = 0; k < len && k < st.size(); ++k) {
            printf("State %zu:\n", k + 1);
            print_state(st[k]);
            printf("\n");
        }
        exitcode = 12;
    } else {
        printf("No error has been found in %llu behaviours.\n", (unsigned long long)r.behaviours);
    }
    printf("%llu states generated (%llu steps), %llu behaviours truncated at the %s layout's capacity, "
           "%llu deadlocked (no successor within the capacity).\n",
           (unsigned long long)(r.steps + r.behaviours), (unsigned long long)r.steps,
           (unsigned long long)r.truncated, wide ? "wide" : "packed", (unsigned long long)r.deadlocked);
    printf("Finished in %.0fms (%.3g behaviours/s, %.3g steps/s on the device)\n", r.seconds * 1e3,
           r.behaviours / (r.kernel_seconds > 0 ? r.kernel_seconds : 1), r.steps / (r.kernel_seconds > 0 ? r.kernel_seconds : 1));
    rmc_destroy(ctx);
    return exitcode;
}

}  // namespace

int main(int argc, char** argv) {
    std::string cfg, tla;
    int depth = 0, device = 0, nodeadlock = 0, verify = 0;
    unsigned long long fpseed = 0, seed = 0, num = 0;
    int simulate = 0, gpus = 1;
    std::string ckpt, recover, raft;
    uint32_t fopts = 0;
    unsigned long long capacity = 0, window = 0, fpmem = 0;
    int nospill = 0, coverage = 0, cont = 0;
    std::string dump;  // -dump's FILE
    int dump_dot = 0, dump_labels = 0;
    for (int a = 1; a < argc; ++a) {
        std::string s = argv[a];
        auto next = [&]() -> const char* { return a + 1 < argc ? argv[++a] : nullptr; };
        if (s == "-config") { const char* v = next(); if (!v) return usage(); cfg = v; }
        else if (s == "-depth") { const char* v = next(); if (!v) return usage(); depth = atoi(v); }
        else if (s == "-deadlock") nodeadlock = 1;  // TLC: -deadlock turns deadlock checking OFF
        else if (s == "-device") { const char* v = next(); if (!v) return usage(); device = atoi(v); }
        else if (s == "-capacity") { const char* v = next(); if (!v) return usage(); capacity = strtoull(v, nullptr, 10); }
        else if (s == "-workers") { if (!next()) return usage(); }  // accepted for compatibility
        else if (s == "-gpus") { const char* v = next(); if (!v) return usage(); gpus = atoi(v); }
        else if (s == "-verify") verify = 1;
        else if (s == "-nospill") nospill = 1;
        else if (s == "-continue") cont = 1;
        else if (s == "-dump") {  // TLC: -dump FILE, or -dump dot[,option...] FILE
            const char* v = next();
            if (!v) return usage();
            std::string f = v;
            if (f == "dot" || f.compare(0, 4, "dot,") == 0) {
                dump_dot = 1;
                for (size_t p = 3; p < f.size();) {
                    const size_t e = f.find(',', p + 1);
                    const std::string opt = f.substr(p + 1, e == std::string::npos ? e : e - p - 1);
                    if (opt == "actionlabels") dump_labels = 1;
                    else if (opt == "colorize" || opt == "snapshot") {
                        fprintf(stderr, "-dump dot: the option %s is not supported (actionlabels is)\n", opt.c_str());
                        return usage();
                    } else {
                        fprintf(stderr, "-dump dot: unknown option %s\n", opt.c_str());
                        return usage();
                    }
                    p = e == std::string::npos ? f.size() : e;
                }
                v = next();
                if (!v) return usage();
                f = v;
            }
            dump = f;
        }
        else if (s == "-coverage") {  // TLC's optional interval in minutes: a number, not the model
            coverage = 1;
            if (a + 1 < argc && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '9' &&
                strspn(argv[a + 1], "0123456789") == strlen(argv[a + 1]))
                ++a;
        }
        else if (s == "-fpmem") {
            const char* v = next();
            if (!v) return usage();
            char* e = nullptr;
            fpmem = strtoull(v, &e, 10);
            if (e && (*e == 'K' || *e == 'k')) fpmem <<= 10;
            else if (e && (*e == 'M' || *e == 'm')) fpmem <<= 20;
            else if (e && (*e == 'G' || *e == 'g')) fpmem <<= 30;
            else if (e && *e) return usage();
        }
        else if (s == "-window") { const char* v = next(); if (!v) return usage(); window = strtoull(v, nullptr, 10); }
        else if (s == "-raft") { const char* v = next(); if (!v) return usage(); raft = v; }
        else if (s == "-builtin-raft") fopts |= RMC_FRONT_BUILTIN_RAFT;
        else if (s == "-checkpoint") { const char* v = next(); if (!v) return usage(); ckpt = v; }
        else if (s == "-recover") { const char* v = next(); if (!v) return usage(); recover = v; }
        else if (s == "-simulate") {
            simulate = 1;
            if (a + 1 < argc && strncmp(argv[a + 1], "num=", 4) == 0) num = strtoull(argv[++a] + 4, nullptr, 10);
        }
        else if (s == "-seed") { const char* v = next(); if (!v) return usage(); seed = strtoull(v, nullptr, 0); }
        else if (s == "-fpseed" || s == "-fp") { const char* v = next(); if (!v) return usage(); fpseed = strtoull(v, nullptr, 0); }
        else if (s[0] == '-') { fprintf(stderr, "unsupported option %s\n", s.c_str()); return usage(); }
        else tla = s;
    }
    if (tla.empty()) return usage();
    if (coverage && (gpus > 1 || !ckpt.empty() || !recover.empty() || simulate)) {
        fprintf(stderr, "-coverage counts whole single-GPU searches: not with %s\n",
                gpus > 1 ? "-gpus N > 1" : !ckpt.empty() ? "-checkpoint" : !recover.empty() ? "-recover" : "-simulate");
        return usage();
    }
    if (cont && (gpus > 1 || !ckpt.empty() || !recover.empty() || simulate)) {
        fprintf(stderr, "-continue counts whole single-GPU searches: not with %s\n",
                gpus > 1 ? "-gpus N > 1" : !ckpt.empty() ? "-checkpoint" : !recover.empty() ? "-recover" : "-simulate");
        return usage();
    }
    if (!dump.empty() && (gpus > 1 || simulate || !recover.empty())) {
        fprintf(stderr, "-dump writes the graph of one whole single-GPU search: not with %s\n",
                gpus > 1 ? "-gpus N > 1" : simulate ? "-simulate" : "-recover");
        return usage();
    }
    if (!dump.empty()) nospill = 1;  // the graph is read from the resident store
    if (cfg.empty()) cfg = (tla.size() > 4 && tla.substr(tla.size() - 4) == ".tla" ? tla.substr(0, tla.size() - 4) : tla) + ".cfg";
    printf("rmc-tlc: %s\n", rmc_version());
    if (const char* b = getenv("RMC_BUILTIN_RAFT")) if (b[0] == '1') fopts |= RMC_FRONT_BUILTIN_RAFT;
    // INVARIANTs of the model's own (none of the ten compiled-in ones) are compiled to the
    // predicate interpreter's bytecode and checked by a pass of the single-GPU search
    fopts |= RMC_FRONT_PREDICATES;
    // CONSTRAINT conjuncts that are none of the four bounds (residuals) are compiled the same way
    // and filter what the single-GPU search stores, in a pass after each of its launches
    fopts |= RMC_FRONT_CONSTRAINTS;
    // a PROPERTY of the form [][A]_vars is an action property: compiled the same way, with primes,
    // and checked on every transition by a pass of the single-GPU search
    fopts |= RMC_FRONT_ACTIONS;
    if (depth > 0 && !simulate) fopts |= RMC_FRONT_DEPTH_BOUNDED;
    rmc_predicates* preds = nullptr;
    {
        char perr[2048];
        if (rmc_predicates_from_files(cfg.c_str(), tla.c_str(), raft.empty() ? nullptr : raft.c_str(),
                                      fopts | (simulate ? RMC_FRONT_SIMULATE : 0u), &preds, perr, sizeof perr)) {
            printf("Error: %s\n", perr);
            return 1;
        }
    }
    // (a model with residuals is refused by its constraint first)
    rmc_predicates* cons = nullptr;
    {
        char cerr[2048];
        if (rmc_constraints_from_files(cfg.c_str(), tla.c_str(), raft.empty() ? nullptr : raft.c_str(),
                                       fopts | (simulate ? RMC_FRONT_SIMULATE : 0u), &cons, cerr, sizeof cerr)) {
            printf("Error: %s\n", cerr);
            rmc_predicates_free(preds);
            return 1;
        }
    }
    rmc_predicates* acts = nullptr;
    {
        char aerr[2048];
        if (rmc_actions_from_files(cfg.c_str(), tla.c_str(), raft.empty() ? nullptr : raft.c_str(),
                                   fopts | (simulate ? RMC_FRONT_SIMULATE : 0u), &acts, aerr, sizeof aerr)) {
            printf("Error: %s\n", aerr);
            rmc_predicates_free(preds);
            rmc_predicates_free(cons);
            return 1;
        }
    }
    const int nacts = rmc_predicates_count(acts);
    if (nacts && (cont || gpus > 1 || simulate || !ckpt.empty() || !recover.empty() || rmc_predicates_count(cons))) {
        printf("Error: PROPERTY %s is an action property, checked by the single-GPU search's pass over every "
               "transition: not with %s\n", rmc_predicates_name(acts, 0),
               cont ? "-continue" : gpus > 1 ? "-gpus N > 1" : simulate ? "-simulate" : !ckpt.empty() ? "-checkpoint"
               : !recover.empty() ? "-recover" : "a CONSTRAINT conjunct that is no bound");
        rmc_predicates_free(preds);
        rmc_predicates_free(cons);
        rmc_predicates_free(acts);
        return 1;
    }
    const int ncons = rmc_predicates_count(cons);
    if (ncons && (verify || cont || coverage || !dump.empty() || gpus > 1 || simulate || !ckpt.empty() || !recover.empty())) {
        printf("Error: CONSTRAINT %s has a conjunct that is no bound and is filtered by the single-GPU search's "
               "constraint pass: not with %s\n", rmc_predicates_name(cons, 0),
               verify ? "-verify" : cont ? "-continue" : coverage ? "-coverage" : !dump.empty() ? "-dump"
               : gpus > 1 ? "-gpus N > 1" : simulate ? "-simulate" : !ckpt.empty() ? "-checkpoint" : "-recover");
        rmc_predicates_free(preds);
        rmc_predicates_free(cons);
        return 1;
    }
    const int npred = rmc_predicates_count(preds);
    if (npred && (cont || gpus > 1 || simulate || !ckpt.empty() || !recover.empty())) {
        printf("Error: INVARIANT %s is defined by the model and checked by the single-GPU search's predicate pass: "
               "not with %s\n", rmc_predicates_name(preds, 0),
               cont ? "-continue" : gpus > 1 ? "-gpus N > 1" : simulate ? "-simulate" : !ckpt.empty() ? "-checkpoint"
                                                                                                     : "-recover");
        rmc_predicates_free(preds);
        rmc_predicates_free(cons);
        return 1;
    }
    if (simulate) return run_simulation(cfg, tla, raft, fopts, device, depth, num, seed);
    rmc_config c;
    char info[2048];
    // -depth N: a model that leaves fields unbounded (MCraft.cfg as shipped) runs level by level
    if (depth > 0) fopts |= RMC_FRONT_DEPTH_BOUNDED;
    int rc = rmc_model_from_files(cfg.c_str(), tla.c_str(), raft.empty() ? nullptr : raft.c_str(), fopts, &c, nullptr,
                                  info, sizeof info);
    if (rc) { printf("Error: %s\n", info); return 1; }
    if (info[0]) printf("%s\n", info);
    if (const char* a = strstr(info, "BecomeLeader <- "))
        if (const char* b = strstr(a, "; action <"))
            if (const char* e = strchr(b, '>')) g_override_header.assign(b + 9, e + 1);
    c.device = device;
    c.max_depth = depth;
    c.state_capacity = capacity;
    if (nodeadlock) c.flags &= ~RMC_FLAG_CHECK_DEADLOCK;
    if (verify) c.flags |= RMC_FLAG_VERIFY_STATES;
    if (coverage) c.flags |= RMC_FLAG_COVERAGE;
    if (cont) c.flags |= RMC_FLAG_CONTINUE;
    // like TLC's states/ directory, expanded levels leave the device when it fills
    // (single GPU; under -verify the spilled states keep a host copy for the
    // comparisons, and checkpoints of such runs stay resident).  The wide layout of
    // -depth runs of unbounded models spills too, through a ring window of its
    // records with the trace links in HBM — not under -verify, which on the wide
    // layout compares with resident records only (it refuses the two flags together),
    // nor under -continue, whose pass reads every stored state's record
    const bool wide = rmc_state_bytes(&c) > 64 * 4;  // (a packed state is at most 18 words)
    if (!dump.empty() && wide) {
        printf("Error: -dump reads the graph of the packed layout: this model runs on the wide layout (bounds "
               "beyond the packed capacity, or fields no CONSTRAINT bounds)\n");
        return 1;
    }
    // the graph's slot -> state index takes as much HBM as the set: not beside an auto-sized one
    if (!dump.empty() && !capacity && !fpmem) c.state_capacity = 1ull << 26;
    // (nor with model-defined invariants, whose pass reads them too)
    if (!nospill && !(verify && (!ckpt.empty() || !recover.empty())) && gpus == 1 &&
        !(wide && (verify || cont || npred)) && !ncons)
        c.flags |= RMC_FLAG_SPILL;
    else if (ncons && !nospill)
        printf("Note: the constraint pass compacts a resident store: expanded levels do not leave the device "
               "(-capacity sizes the store).\n");
    c.device_window = window;
    c.set_bytes = fpmem;
    c.seed = fpseed;
    printf("Model: %d servers, %d values, CONSTRAINT MaxTerm=%d MaxLogLen=%d MaxMsgs=%d MaxDup=%d%s%s\n",
           c.n_servers, c.n_values, c.max_term, c.max_log_len, c.max_msgs, c.max_dup,
           (c.flags & RMC_FLAG_SYMMETRY) ? ", SYMMETRY Permutations(Server)" : "",
           (c.flags & RMC_FLAG_BUG_QUORUM) ? ", BecomeLeader quorum guard weakened" : "");
    if (c.invariants & (RMC_INV_VOTES_GRANTED | RMC_INV_QUORUM_LOG | RMC_INV_MORE_UP_TO_DATE | RMC_INV_LEADER_COMPLETE))
        printf("Note: Committed(i) is read as the first min(commitIndex[i], Len(log[i])) entries; raft.tla:896's "
               "SubSeq(log[i], 1, commitIndex[i]) is out of range when commitIndex[i] > Len(log[i]), which TLC "
               "would report as an evaluation error (specs/MCraftBounded.tla).\n");
    rmc_ctx* ctx = nullptr;
    rc = rmc_create(&c, &ctx);
    if (rc) { printf("Error: rmc_create failed (%d)\n", rc); return 1; }
    if (npred) {
        if (rmc_set_predicates(ctx, preds)) {
            printf("Error: %s\n", rmc_last_error(ctx));
            rmc_destroy(ctx);
            return 1;
        }
        printf("Compiled model-defined invariants:");
        for (int p = 0; p < npred; ++p) printf("%s %s", p ? "," : "", rmc_predicates_name(preds, p));
        printf("\n");
    }
    if (nacts) {
        if (rmc_set_actions(ctx, acts)) {
            printf("Error: %s\n", rmc_last_error(ctx));
            rmc_destroy(ctx);
            return 1;
        }
        printf("Compiled action properties:");
        for (int p = 0; p < nacts; ++p) printf("%s %s", p ? "," : "", rmc_predicates_name(acts, p));
        printf("\n");
    }
    if (ncons) {
        if (rmc_set_constraints(ctx, cons)) {
            printf("Error: %s\n", rmc_last_error(ctx));
            rmc_destroy(ctx);
            return 1;
        }
        printf("Compiled %d residual constraint conjunct%s of:", ncons, ncons == 1 ? "" : "s");
        for (int p = 0; p < ncons; ++p) printf("%s %s", p ? "," : "", rmc_predicates_name(cons, p));
        printf("\n");
    }
    // -gpus N: one ctx per GPU (devices device..device+N-1), each a rank of the
    // sharded search on librmc's RCCL communicator, each driven by its own
    // thread through every collective (the BFS and the trace walk).  All
    // contexts are created before any communicator exists, and a rank that
    // fails later ends the process (stdout flushed, exit code 1) instead of
    // leaving the other ranks blocked in a collective.
    std::vector<rmc_state_view> tr_st;
    std::vector<int32_t> tr_fam, tr_inst;
    rmc_result r{};
    if (gpus > 1) {
        // -verify, -checkpoint and -recover work per rank: every rank compares
        // its own hits and writes / reads its own part, <F>.rank<r>
        std::vector<rmc_ctx*> ctxs((size_t)gpus, nullptr);
        ctxs[0] = ctx;
        for (int k = 1; k < gpus; ++k) {
            rmc_config cr = c;
            cr.device = device + k;
            if (rmc_create(&cr, &ctxs[(size_t)k])) {
                printf("Error: rank %d: rmc_create on device %d failed\n", k, cr.device);
                for (rmc_ctx* x : ctxs) rmc_destroy(x);
                return 1;
            }
        }
        uint8_t id[128];
        if (rmc_rccl_unique_id(id)) { printf("Error: rmc_rccl_unique_id failed\n"); return 1; }
        printf("Sharded over %d GPUs (librmc two-phase exchange over RCCL).\n", gpus);
        if (!recover.empty()) printf("Recovering from checkpoint %s.rank0..%d...\n", recover.c_str(), gpus - 1);
        else printf("Computing initial states...\n");
        fflush(stdout);
        std::atomic<int> done{0}, failed{-1};
        std::vector<std::string> errs((size_t)gpus);
        std::vector<std::thread> ranks;
        for (int k = 0; k < gpus; ++k) {
            ranks.emplace_back([&, k]() {
                rmc_ctx* h = ctxs[(size_t)k];
                auto bad = [&](const char* what) {
                    errs[(size_t)k] = std::string(what) + ": " + rmc_last_error(h);
                    int none = -1;
                    failed.compare_exchange_strong(none, k);
                };
                if (rmc_shard(h, k, gpus, id, nullptr, 0, 0)) { bad("rmc_shard"); return; }
                if (!recover.empty() && rmc_recover(h, recover.c_str())) { bad("rmc_recover"); return; }
                if (rmc_run_bfs(h, k == 0 ? progress : nullptr, nullptr)) { bad("rmc_run_bfs"); return; }
                rmc_result rr;
                rmc_get_result(h, &rr);
                if (!ckpt.empty() && rr.left_on_queue > 0 && !rr.violated_inv && !rr.deadlock &&
                    rmc_checkpoint(h, ckpt.c_str())) { bad("rmc_checkpoint"); return; }
                if (rr.violated_inv || rr.deadlock) {  // the trace walk is collective: every rank calls it
                    size_t n = 0;
                    if (rmc_trace(h, nullptr, nullptr, nullptr, 0, &n)) { bad("rmc_trace"); return; }
                    std::vector<rmc_state_view> st(n);
                    std::vector<int32_t> f(n), in(n);
                    if (rmc_trace(h, st.data(), f.data(), in.data(), n, &n)) { bad("rmc_trace"); return; }
                    if (k == 0) { tr_st.swap(st); tr_fam.swap(f); tr_inst.swap(in); }
                }
                done.fetch_add(1);
            });
        }
        while (done.load() < gpus && failed.load() < 0) std::this_thread::sleep_for(std::chrono::milliseconds(20));
        if (failed.load() >= 0) {
            printf("Error: rank %d: %s\n", failed.load(), errs[(size_t)failed.load()].c_str());
            fflush(stdout);
            fflush(stderr);
            _exit(1);  // the other ranks may be blocked in a collective of the failed one
        }
        for (auto& t : ranks) t.join();
        rmc_get_result(ctx, &r);
        for (int k = 1; k < gpus; ++k) rmc_destroy(ctxs[(size_t)k]);
    } else {
        if (!recover.empty()) {
            rc = rmc_recover(ctx, recover.c_str());
            if (rc) { printf("Error: %s\n", rmc_last_error(ctx)); rmc_destroy(ctx); return 1; }
            printf("Recovering from checkpoint %s...\n", recover.c_str());
        } else {
            printf("Computing initial states...\n");
        }
        rc = rmc_run_bfs(ctx, progress, nullptr);
        if (rc) { printf("Error: %s\n", rmc_last_error(ctx)); rmc_destroy(ctx); return 1; }
        rmc_get_result(ctx, &r);
        if ((r.violated_inv && !cont) || r.deadlock || rmc_constraint_error(ctx)) {  // (-continue: rmc_trace_violation's)
            size_t len = 0;
            rmc_trace(ctx, nullptr, nullptr, nullptr, 0, &len);
            tr_st.resize(len);
            tr_fam.resize(len);
            tr_inst.resize(len);
            rmc_trace(ctx, tr_st.data(), tr_fam.data(), tr_inst.data(), len, &len);
        }
    }
    int exitcode = 0;
    auto print_behaviour = [&]() {
        printf("Error: The behavior up to this point is:\n");
        for (size_t k = 0; k < tr_st.size(); ++k) {
            if (tr_fam[k] < 0 || k == 0) printf("State %zu: <Initial predicate>\n", k + 1);
            else printf("State %zu: %s\n", k + 1, step_header(tr_fam[k], tr_inst[k], tr_st[k - 1]).c_str());
            print_state(tr_st[k]);
            printf("\n");
        }
    };
    rmc_violations vs{};
    if (cont && rmc_get_violations(ctx, &vs)) {
        printf("Error: %s\n", rmc_last_error(ctx));
        rmc_destroy(ctx);
        return 1;
    }
    if (cont && (vs.states || r.deadlock)) {
        // TLC -continue: every violated invariant, in mask order, with the trace to its first state
        const bool dead_only = r.deadlock && !r.violated_inv;  // (its trace was fetched above)
        std::vector<rmc_state_view> dl_st;
        std::vector<int32_t> dl_fam, dl_inst;
        if (dead_only) { dl_st.swap(tr_st); dl_fam.swap(tr_fam); dl_inst.swap(tr_inst); }
        for (int q = 0; q < RMC_INV_COUNT; ++q) {
            if (!vs.each[q]) continue;
            printf("Error: Invariant %s is violated.\n", inv_name(1 << q));
            size_t len = 0;
            if (rmc_trace_violation(ctx, 1u << q, nullptr, nullptr, nullptr, 0, &len)) {
                printf("Error: %s\n", rmc_last_error(ctx));
                continue;
            }
            tr_st.resize(len);
            tr_fam.resize(len);
            tr_inst.resize(len);
            if (rmc_trace_violation(ctx, 1u << q, tr_st.data(), tr_fam.data(), tr_inst.data(), len, &len)) {
                printf("Error: %s\n", rmc_last_error(ctx));
                continue;
            }
            print_behaviour();
        }
        if (r.deadlock) {
            printf("Error: Deadlock reached.\n");
            if (dead_only) {
                tr_st.swap(dl_st); tr_fam.swap(dl_fam); tr_inst.swap(dl_inst);
                print_behaviour();
            }
        }
        exitcode = 12;
    } else if (const int ce = gpus == 1 ? rmc_constraint_error(ctx) : 0) {
        const char* name = rmc_predicates_name(cons, ce - 1);
        printf("Error: Evaluating constraint %s failed.\n", name ? name : "?");
        printf("  (residual %d: a read outside its domain — log[i][n] beyond Len(log[i]), a server index that is "
               "Nil, or a field of another message type)\n", ce - 1);
        print_behaviour();
        exitcode = 12;
    } else if (r.violated_inv || r.deadlock) {
        if ((uint32_t)r.violated_inv >= RMC_ACT_USER0) {  // an action property: bit 24 + p
            int32_t prop = 0, is_err = 0;
            rmc_action_violation(ctx, &prop, nullptr, nullptr, nullptr, &is_err);
            const char* name = rmc_predicates_name(acts, prop);
            if (is_err)
                printf("Error: Evaluating action property %s failed: a read outside its domain (log[i][n] beyond "
                       "Len(log[i]), a server index that is Nil, or a field of another message type).\n",
                       name ? name : "?");
            else
                printf("Error: Action property %s is violated.\n", name ? name : "?");
        } else if ((uint32_t)r.violated_inv >= RMC_INV_USER0) {  // a model-defined invariant: bit 16 + p
            const char* name = rmc_predicates_name(preds, __builtin_ctz((uint32_t)r.violated_inv) - 16);
            if (rmc_predicate_error(ctx))
                printf("Error: Evaluating invariant %s failed: a read outside its domain (log[i][n] beyond "
                       "Len(log[i]), a server index that is Nil, or a field of another message type).\n",
                       name ? name : "?");
            else
                printf("Error: Invariant %s is violated.\n", name ? name : "?");
        } else if (r.violated_inv) printf("Error: Invariant %s is violated.\n", inv_name(r.violated_inv));
        else printf("Error: Deadlock reached.\n");
        print_behaviour();
        exitcode = 12;
    } else {
        printf("Model checking completed. No error has been found.\n");
        printf("  Estimates of the probability that TLC did not check all reachable states\n"
               "  because two distinct states had the same fingerprint:\n"
               "  calculated (optimistic):  val = %.1E\n", r.collision_probability);
    }
    if (verify) {
        printf("Full-state verification: %llu fingerprint hits compared state by state, %llu collisions.\n",
               (unsigned long long)r.verified, (unsigned long long)r.collisions);
        if (r.verified_spilled)
            printf("  (%llu of the hits were on states that had left the device window: compared with "
                   "their host copies)\n", (unsigned long long)r.verified_spilled);
    }
    if (cont) {
        // a line of our own (not TLC's): per violated invariant the stored states that violate it
        // checked alone, those it is the first violated invariant of, and its shallowest level
        printf("Violations (-continue): %llu states violate an invariant.", (unsigned long long)vs.states);
        for (int q = 0; q < RMC_INV_COUNT; ++q)
            if (vs.each[q])
                printf(" %s: each %llu, first %llu, depth %d.", inv_name(1 << q), (unsigned long long)vs.each[q],
                       (unsigned long long)vs.first[q], vs.depth[q]);
        printf("\n");
    }
    if (coverage) {
        rmc_coverage cv;
        if (rmc_get_coverage(ctx, &cv)) printf("Error: %s\n", rmc_last_error(ctx));
        else print_coverage(cv);
    }
    printf("%llu states generated, %llu distinct states found, %llu states left on queue.\n",
           (unsigned long long)r.generated, (unsigned long long)r.distinct, (unsigned long long)r.left_on_queue);
    printf("The depth of the complete state graph search is %d.\n", r.depth);
    if (r.spills)
        printf("Spilled %llu expanded states out of the device window in %llu spills (%.2fs; trace links kept in %s).\n",
               (unsigned long long)r.spilled, (unsigned long long)r.spills, r.spill_seconds,
               r.spill_links_on_device ? "HBM" : "host memory");
    if (gpus > 1)
        printf("Exchange (rank 0): %llu rounds, %llu keys and %llu states sent, %llu keys parked, "
               "%.1fms of exchange on the device, %.1fms waited on the host.\n",
               (unsigned long long)r.chunks, (unsigned long long)r.keys_sent, (unsigned long long)r.states_sent,
               (unsigned long long)r.parked, r.exchange_seconds * 1e3, r.exchange_wait_seconds * 1e3);
    if (!ckpt.empty() && r.left_on_queue > 0 && !r.violated_inv && !r.deadlock) {
        if (gpus > 1) printf("Checkpoint written to %s.rank0..%d (%llu states on the queue).\n", ckpt.c_str(), gpus - 1,
                             (unsigned long long)r.left_on_queue);
        else if (rmc_checkpoint(ctx, ckpt.c_str())) printf("Error: %s\n", rmc_last_error(ctx));
        else printf("Checkpoint written to %s (%llu states on the queue).\n", ckpt.c_str(),
                    (unsigned long long)r.left_on_queue);
    }
    if (!dump.empty() && write_dump(ctx, dump, dump_dot != 0, dump_labels != 0) && !exitcode) exitcode = 1;
    if (recover.empty())
        printf("Finished in %.0fms (%.0f distinct states/s)\n", r.seconds * 1e3, r.distinct / (r.seconds > 0 ? r.seconds : 1));
    else
        printf("Finished in %.0fms after recovery (counts include the checkpointed levels)\n", r.seconds * 1e3);
    rmc_destroy(ctx);
    rmc_predicates_free(preds);
    rmc_predicates_free(cons);
    rmc_predicates_free(acts);
    return exitcode;
}
