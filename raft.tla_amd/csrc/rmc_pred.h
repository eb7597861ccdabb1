// rmc_pred.h — model-defined invariants (DESIGN.md "Model-defined invariants"): the
// bytecode a state predicate of the model's own is compiled to (rmc_front.cpp), and the
// one interpreter that evaluates it, on the host and on gfx950.
//
// Every value is a 32-bit integer: a Boolean, a natural, a server index (Nil = -1), a
// role, a message type, a set of servers as a bit mask (bit 31: Nil, so {i, Nil} is a
// set), a bag slot.  A program is a
// stack machine's code: conditional jumps give /\ \/ => IF their short circuit, loop
// instructions walk a quantifier's or a comprehension's domain.  A read outside a domain
// (log[i][n] beyond Len(log[i]), a server index that is Nil, a field of another message
// type) is an evaluation error, as in TLC: verdict 2.
//
// Programs come from the compiler only and the interpreter validates nothing: the
// compiler proves the stack depth (<= PRED_STACK), the bound names (<= PRED_BOUND), the
// code size (<= PRED_CODE words in all) and that every jump stays inside its predicate.
//
// The interpreter is templated over a state accessor (PackedAcc<S, K>: the packed words
// in place; WideAcc<Rec>: a wide record in place; ViewAcc: rmc_state_view) and over the
// stride of its working memory, PRED_ROWS words per evaluation: the device kernels keep
// it in LDS columns (stride = the block's threads; each thread its own column, so no
// barrier and no bank conflict), the host in a local array (stride 1).
//
// An action property (PROPERTY [][A]_vars) is a program over two states: run2 takes a
// current and a next accessor, and a read flagged OP_PRIMED reads the next one.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "../../include/rmc.h"
#include "raft_packed.h"
#include "raft_wide.h"

namespace rmc {
namespace pred {

constexpr int PRED_MAX = RMC_MAX_PREDICATES;  // predicates per program
constexpr int PRED_CODE = 1024;               // code words, all predicates together
constexpr int PRED_STACK = 16;                // evaluation stack depth
constexpr int PRED_BOUND = 8;                 // bound names in scope at once
constexpr int PRED_ROWS = PRED_STACK + 2 * PRED_BOUND;  // stack, then (value, loop state) per bound name

// A compiled set of predicates.  entry[p]: the first code word of predicate p, which ends
// in HALT with its Boolean on the stack.
struct Program {
    int n_servers;  // the model it was compiled for (Server's model values are indices)
    int n_pred;
    int n_code;
    int pad;
    int entry[PRED_MAX];
    u32 code[PRED_CODE];
};

// An instruction: the operation in bits 0-7, a signed 24-bit argument above.  Jumps hold
// the target's code index; the loop instructions hold (target << 3 | bound name).
enum Op : u32 {
    OP_HALT = 0,
    OP_PUSH,    // arg
    OP_LOAD,    // the value of bound name arg
    OP_POP,
    OP_JMP,     // arg
    OP_JF,      // pop; jump if 0
    OP_JT,      // pop; jump if not 0
    OP_AND_SC,  // top == 0: jump (the 0 stays); else pop
    OP_OR_SC,   // top != 0: jump (it stays); else pop
    OP_NOT,
    OP_ADD, OP_SUB, OP_MIN, OP_MAX,
    OP_EQ, OP_NE, OP_LT, OP_LE, OP_GT, OP_GE,
    OP_OR, OP_AND, OP_ANDN,  // sets: \cup, \cap, a \ b
    OP_SUBSET,   // a \subseteq b
    OP_IN,       // pop set, element: element \in set (Nil is in no set)
    OP_INRANGE,  // pop hi, lo, x: lo <= x <= hi
    OP_CARD,     // Cardinality of a set
    OP_BIT,      // {x}: 1 << x (a server index)
    OP_ISQUORUM, // 2 * Cardinality(set) > |Server|
    // state reads (the index or indices popped; an index outside its domain: error)
    OP_TERM, OP_ROLE, OP_VOTED, OP_COMMIT, OP_VRESP, OP_VGRANT, OP_LEN, OP_LASTTERM,
    OP_NEXT, OP_MATCH,       // pop j, i
    OP_LOGTERM, OP_LOGVAL,   // pop n, i: log[i][n], n in 1..Len(log[i])
    OP_NMSG,                 // |DOMAIN messages| (a bound message is a bag slot 0..n-1)
    OP_MSGCNT,               // pop slot: messages[m]
    OP_MSGF,                 // pop slot: field arg of the message (MsgField)
    // loops over bound name r = arg & 7, exit target = arg >> 3
    OP_ITER_RANGE,   // pop hi, lo
    OP_ITER_SET,     // pop the set
    OP_ITER_QUORUM,  // the quorums of Server, as masks in ascending order
    OP_NEXT_RANGE, OP_NEXT_SET, OP_NEXT_QUORUM,  // the next element into r, or jump
};

enum MsgField : int {
    F_MTYPE = 0, F_MTERM, F_MSOURCE, F_MDEST,
    F_MLASTLOGTERM, F_MLASTLOGINDEX,                // RequestVoteRequest
    F_MVOTEGRANTED,                                 // RequestVoteResponse
    F_MPREVLOGINDEX, F_MPREVLOGTERM, F_MCOMMITINDEX,  // AppendEntriesRequest
    F_MSUCCESS, F_MMATCHINDEX,                      // AppendEntriesResponse
    F_COUNT
};
// the message type a field belongs to (-1: every type has it)
RMC_HD int field_type(int f) {
    return f < F_MLASTLOGTERM ? -1 : f < F_MVOTEGRANTED ? (int)RVQ : f < F_MPREVLOGINDEX ? (int)RVP
           : f < F_MSUCCESS ? (int)AEQ : (int)AEP;
}

// An action property's read of the next state: the state-read operation with this bit (bit 7 of
// the operation byte; the operations stay below 128).  Programs without primes hold none.
constexpr u32 OP_PRIMED = 128u;

constexpr u32 ins(Op op, int arg = 0) { return (u32)op | ((u32)arg << 8); }
RMC_HD u32 ins_op(u32 w) { return w & 255u; }
RMC_HD int ins_arg(u32 w) { return (int)w >> 8; }

// ---- state accessors: every read an int ----------------------------------------------
// The packed state in place: (2 S + K) 32-bit words (raft_packed.h), read where they lie
// (the store, a staged array), so no thread holds a dynamically indexed copy.
// STRIDE: the distance between its words (1: a record; a block's threads: a thread's LDS column,
// rmc_dev_act.h).
template <int S, int K, int STRIDE = 1>
struct PackedAcc {
    const u32* r;
    RMC_HD u64 w(int i) const { return (u64)r[(2 * i) * STRIDE] | ((u64)r[(2 * i + 1) * STRIDE] << 32); }
    RMC_HD u32 m(int q) const { return r[(2 * S + q) * STRIDE]; }
    RMC_HD int servers() const { return S; }
    RMC_HD int term(int i) const { return (int)w_ct(w(i)); }
    RMC_HD int role(int i) const { return (int)w_st(w(i)); }
    RMC_HD int voted(int i) const { const u32 v = w_vf(w(i)); return v == NILV ? -1 : (int)v; }
    RMC_HD int commit(int i) const { return (int)w_ci(w(i)); }
    RMC_HD int vresp(int i) const { return (int)w_vr<S>(w(i)); }
    RMC_HD int vgrant(int i) const { return (int)w_vg<S>(w(i)); }
    RMC_HD int len(int i) const { return (int)w_len(w(i)); }
    RMC_HD int log_term(int i, int x) const { return (int)ent_term(w_ent(w(i), (u32)x)); }  // x 0-based
    RMC_HD int log_val(int i, int x) const { return (int)(w_ent(w(i), (u32)x) >> 4); }
    RMC_HD int next(int i, int j) const { return (int)w_ni<S>(w(i), (u32)j); }
    RMC_HD int match(int i, int j) const { return (int)w_mi<S>(w(i), (u32)j); }
    RMC_HD int nmsg() const {  // a canonical bag: the live slots first
        int n = 0;
        for (int q = 0; q < K; ++q) n += m(q) ? 1 : 0;
        return n;
    }
    RMC_HD int msg_cnt(int q) const { return (int)m_cnt(m(q)); }
    RMC_HD int msg_field(int q, int f) const {
        const u32 s = m(q);
        switch (f) {
            case F_MTYPE: return (int)m_type(s);
            case F_MTERM: return (int)m_term(s);
            case F_MSOURCE: return (int)m_src(s);
            case F_MDEST: return (int)m_dst(s);
            case F_MLASTLOGTERM: return (int)((s >> 12) & 15u);
            case F_MLASTLOGINDEX: return (int)((s >> 16) & 3u);
            case F_MVOTEGRANTED: return (int)((s >> 12) & 1u);
            case F_MPREVLOGINDEX: return (int)((s >> 12) & 7u) - 1;
            case F_MPREVLOGTERM: return (int)((s >> 15) & 15u);
            case F_MCOMMITINDEX: return (int)((s >> 25) & 3u);
            case F_MSUCCESS: return (int)((s >> 12) & 1u);
            default: return (int)((s >> 13) & 3u);  // F_MMATCHINDEX
        }
    }
};

// A wide record in place (raft_wide.h WStateT, any of the three).
template <class Rec>
struct WideAcc {
    const Rec* s;
    int S;
    RMC_HD int servers() const { return S; }
    RMC_HD int term(int i) const { return s->ct[i]; }
    RMC_HD int role(int i) const { return s->st[i]; }
    RMC_HD int voted(int i) const { return s->vf[i] == wide::NIL ? -1 : (int)s->vf[i]; }
    RMC_HD int commit(int i) const { return s->ci[i]; }
    RMC_HD int vresp(int i) const { return s->vR[i]; }
    RMC_HD int vgrant(int i) const { return s->vG[i]; }
    RMC_HD int len(int i) const { return s->len[i]; }
    RMC_HD int log_term(int i, int x) const { return s->log[i][x].term; }
    RMC_HD int log_val(int i, int x) const { return s->log[i][x].value; }
    RMC_HD int next(int i, int j) const { return s->ni[i][j]; }
    RMC_HD int match(int i, int j) const { return s->mi[i][j]; }
    RMC_HD int nmsg() const { return s->nmsg; }
    RMC_HD int msg_cnt(int q) const { return s->cnt[q]; }
    RMC_HD int msg_field(int q, int f) const {
        const typename Rec::Msg& m = s->msg[q];
        switch (f) {
            case F_MTYPE: return m.type;
            case F_MTERM: return m.term;
            case F_MSOURCE: return m.src;
            case F_MDEST: return m.dst;
            case F_MLASTLOGTERM: return m.b;
            case F_MLASTLOGINDEX: return m.c;
            case F_MVOTEGRANTED: return m.a;
            case F_MPREVLOGINDEX: return m.a;
            case F_MPREVLOGTERM: return m.b;
            case F_MCOMMITINDEX: return m.c;
            case F_MSUCCESS: return m.a;
            default: return m.b;  // F_MMATCHINDEX
        }
    }
};

// The decoded view (rmc.h): the host's reference evaluation.
struct ViewAcc {
    const rmc_state_view* v;
    RMC_HD int servers() const { return v->n_servers; }
    RMC_HD int term(int i) const { return v->currentTerm[i]; }
    RMC_HD int role(int i) const { return v->state[i]; }
    RMC_HD int voted(int i) const { return v->votedFor[i]; }
    RMC_HD int commit(int i) const { return v->commitIndex[i]; }
    RMC_HD int vresp(int i) const { return (int)v->votesResponded[i]; }
    RMC_HD int vgrant(int i) const { return (int)v->votesGranted[i]; }
    RMC_HD int len(int i) const { return v->log_len[i]; }
    RMC_HD int log_term(int i, int x) const { return v->log[i][x].term; }
    RMC_HD int log_val(int i, int x) const { return v->log[i][x].value; }
    RMC_HD int next(int i, int j) const { return v->nextIndex[i][j]; }
    RMC_HD int match(int i, int j) const { return v->matchIndex[i][j]; }
    RMC_HD int nmsg() const { return v->n_msgs; }
    RMC_HD int msg_cnt(int q) const { return v->msgs[q].count; }
    RMC_HD int msg_field(int q, int f) const {
        const rmc_msg_view& m = v->msgs[q];
        switch (f) {
            case F_MTYPE: return m.mtype;
            case F_MTERM: return m.mterm;
            case F_MSOURCE: return m.msource;
            case F_MDEST: return m.mdest;
            case F_MLASTLOGTERM: return m.mlastLogTerm;
            case F_MLASTLOGINDEX: return m.mlastLogIndex;
            case F_MVOTEGRANTED: return m.mvoteGranted;
            case F_MPREVLOGINDEX: return m.mprevLogIndex;
            case F_MPREVLOGTERM: return m.mprevLogTerm;
            case F_MCOMMITINDEX: return m.mcommitIndex;
            case F_MSUCCESS: return m.msuccess;
            default: return m.mmatchIndex;
        }
    }
};

// ---- the interpreter --------------------------------------------------------------------
// One predicate from code[pc] on: 0 it holds, 1 it is violated, 2 an evaluation error.
// mem: PRED_ROWS words at stride STRIDE (row k at mem[k * STRIDE]).
// PRIMED (action properties, DESIGN.md "Action properties"): a state read whose operation carries
// OP_PRIMED reads the next state `n`; without PRIMED the code holds no such operation and `n` is not
// looked at (the one-state entry point below passes the current state twice).
template <int STRIDE, bool PRIMED, class Acc, class AccN>
RMC_HD int run2(const u32* code, int pc, const Acc& a, const AccN& n, int* mem) {
#define PR_STK(k) mem[(k) * STRIDE]
#define PR_VAL(r) mem[(PRED_STACK + 2 * (r)) * STRIDE]
#define PR_AUX(r) mem[(PRED_STACK + 2 * (r) + 1) * STRIDE]
    const int S = a.servers();
    int sp = 0;  // the next free stack row
    for (;;) {
        const u32 w = code[pc++];
        const int arg = ins_arg(w);
        const bool pr = PRIMED && (w & OP_PRIMED) != 0;
#define PR_RD(call) (PRIMED && pr ? n.call : a.call)
        const u32 op = PRIMED ? (w & (OP_PRIMED - 1u)) : ins_op(w);
        switch (op) {
            case OP_HALT: return PR_STK(sp - 1) ? 0 : 1;
            case OP_PUSH: PR_STK(sp++) = arg; break;
            case OP_LOAD: PR_STK(sp++) = PR_VAL(arg); break;
            case OP_POP: --sp; break;
            case OP_JMP: pc = arg; break;
            case OP_JF: if (!PR_STK(--sp)) pc = arg; break;
            case OP_JT: if (PR_STK(--sp)) pc = arg; break;
            case OP_AND_SC: if (!PR_STK(sp - 1)) pc = arg; else --sp; break;
            case OP_OR_SC: if (PR_STK(sp - 1)) pc = arg; else --sp; break;
            case OP_NOT: PR_STK(sp - 1) = !PR_STK(sp - 1); break;
#define PR_BIN(expr)                                  \
    {                                                 \
        const int y = PR_STK(--sp), x = PR_STK(sp - 1); \
        PR_STK(sp - 1) = (expr);                      \
    }                                                 \
    break
            case OP_ADD: PR_BIN(x + y);
            case OP_SUB: PR_BIN(x - y);
            case OP_MIN: PR_BIN(x < y ? x : y);
            case OP_MAX: PR_BIN(x > y ? x : y);
            case OP_EQ: PR_BIN(x == y);
            case OP_NE: PR_BIN(x != y);
            case OP_LT: PR_BIN(x < y);
            case OP_LE: PR_BIN(x <= y);
            case OP_GT: PR_BIN(x > y);
            case OP_GE: PR_BIN(x >= y);
            case OP_OR: PR_BIN(x | y);
            case OP_AND: PR_BIN(x & y);
            case OP_ANDN: PR_BIN(x & ~y);
            case OP_SUBSET: PR_BIN((x & ~y) == 0);
            case OP_IN: PR_BIN(x >= -1 && x < 31 && (((unsigned)y >> (x & 31)) & 1u));  // (Nil = -1: bit 31)
#undef PR_BIN
            case OP_INRANGE: {
                const int hi = PR_STK(--sp), lo = PR_STK(--sp), x = PR_STK(sp - 1);
                PR_STK(sp - 1) = lo <= x && x <= hi;
                break;
            }
            case OP_CARD: PR_STK(sp - 1) = __builtin_popcount((unsigned)PR_STK(sp - 1)); break;
            case OP_BIT: {
                const int x = PR_STK(sp - 1);
                if (x < -1 || x >= S) return 2;
                PR_STK(sp - 1) = (int)(1u << (x & 31));  // (Nil = -1: bit 31)
                break;
            }
            case OP_ISQUORUM: {  // a subset of Server (Nil is no server) of more than half of it
                const unsigned x = (unsigned)PR_STK(sp - 1);
                PR_STK(sp - 1) = !(x >> S) && 2 * __builtin_popcount(x) > S;
                break;
            }
#define PR_SRV(read)                      \
    {                                     \
        const int i = PR_STK(sp - 1);     \
        if (i < 0 || i >= S) return 2;    \
        PR_STK(sp - 1) = (read);          \
    }                                     \
    break
            case OP_TERM: PR_SRV(PR_RD(term(i)));
            case OP_ROLE: PR_SRV(PR_RD(role(i)));
            case OP_VOTED: PR_SRV(PR_RD(voted(i)));
            case OP_COMMIT: PR_SRV(PR_RD(commit(i)));
            case OP_VRESP: PR_SRV(PR_RD(vresp(i)));
            case OP_VGRANT: PR_SRV(PR_RD(vgrant(i)));
            case OP_LEN: PR_SRV(PR_RD(len(i)));
            case OP_LASTTERM: PR_SRV(PR_RD(len(i)) ? PR_RD(log_term(i, PR_RD(len(i)) - 1)) : 0);
#undef PR_SRV
            case OP_NEXT:
            case OP_MATCH: {
                const int j = PR_STK(--sp), i = PR_STK(sp - 1);
                if (i < 0 || i >= S || j < 0 || j >= S) return 2;
                PR_STK(sp - 1) = op == OP_NEXT ? PR_RD(next(i, j)) : PR_RD(match(i, j));
                break;
            }
            case OP_LOGTERM:
            case OP_LOGVAL: {
                const int k = PR_STK(--sp), i = PR_STK(sp - 1);
                if (i < 0 || i >= S) return 2;
                if (k < 1 || k > PR_RD(len(i))) return 2;
                PR_STK(sp - 1) = op == OP_LOGTERM ? PR_RD(log_term(i, k - 1)) : PR_RD(log_val(i, k - 1));
                break;
            }
            case OP_NMSG: PR_STK(sp++) = PR_RD(nmsg()); break;
            case OP_MSGCNT: {
                const int q = PR_STK(sp - 1);
                if (q < 0 || q >= PR_RD(nmsg())) return 2;
                PR_STK(sp - 1) = PR_RD(msg_cnt(q));
                break;
            }
            case OP_MSGF: {
                const int q = PR_STK(sp - 1);
                if (q < 0 || q >= PR_RD(nmsg())) return 2;
                const int ft = field_type(arg);
                if (ft >= 0 && PR_RD(msg_field(q, F_MTYPE)) != ft) return 2;
                PR_STK(sp - 1) = PR_RD(msg_field(q, arg));
                break;
            }
            case OP_ITER_RANGE: {
                const int hi = PR_STK(--sp), lo = PR_STK(--sp);
                PR_VAL(arg & 7) = lo - 1;
                PR_AUX(arg & 7) = hi;
                break;
            }
            case OP_ITER_SET:
                PR_AUX(arg & 7) = PR_STK(--sp);
                break;
            case OP_ITER_QUORUM:
                PR_VAL(arg & 7) = 0;
                PR_AUX(arg & 7) = (1 << S) - 1;
                break;
            case OP_NEXT_RANGE: {
                const int v = PR_VAL(arg & 7) + 1;
                if (v > PR_AUX(arg & 7)) pc = arg >> 3;
                else PR_VAL(arg & 7) = v;
                break;
            }
            case OP_NEXT_SET: {
                const unsigned rem = (unsigned)PR_AUX(arg & 7);
                if (!rem) {
                    pc = arg >> 3;
                } else {
                    const int e = __builtin_ctz(rem);
                    PR_VAL(arg & 7) = e == 31 ? -1 : e;
                    PR_AUX(arg & 7) = (int)(rem & (rem - 1));
                }
                break;
            }
            case OP_NEXT_QUORUM: {
                int v = PR_VAL(arg & 7) + 1;
                const int end = PR_AUX(arg & 7);
                while (v <= end && 2 * __builtin_popcount((unsigned)v) <= S) ++v;
                if (v > end) pc = arg >> 3;
                else PR_VAL(arg & 7) = v;
                break;
            }
            default: return 2;  // (no such instruction: the compiler emits none)
        }
    }
#undef PR_STK
#undef PR_VAL
#undef PR_AUX
#undef PR_RD
}

// One state predicate (an INVARIANT, a CONSTRAINT's residual): no primed reads.
template <int STRIDE, class Acc>
RMC_HD int run(const u32* code, int pc, const Acc& a, int* mem) {
    return run2<STRIDE, false>(code, pc, a, a, mem);
}

// Every predicate in order: 0 if all hold, else 1 + (p << 1 | error) of the first that
// does not (the BFS pass's word per state).
template <int STRIDE, class Acc>
RMC_HD int first_failing(const int* entry, int n_pred, const u32* code, const Acc& a, int* mem) {
    for (int p = 0; p < n_pred; ++p) {
        const int v = run<STRIDE>(code, entry[p], a, mem);
        if (v) return 1 + ((p << 1) | (v == 2 ? 1 : 0));
    }
    return 0;
}

}  // namespace pred
}  // namespace rmc

// The opaque handle of rmc.h: a program, the names of its predicates, and whether one of
// them names a server model value (then it is not invariant under Permutations(Server)).
struct rmc_predicates {
    rmc::pred::Program prog;
    char name[RMC_MAX_PREDICATES][64];
    int names_server;
    int actions;  // action properties (rmc_actions_from_files): two-state programs, for rmc_set_actions only
};
