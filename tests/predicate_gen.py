"""Generated predicates for the predicate VM (test_predicate_gen_native.py on the host,
test_predicate_gen.py on the GPU): a typed AST of the predicate language of DESIGN.md
("Model-defined invariants -> The language", plus the grammar delta of "Action properties"),
a seeded generator of well-typed expressions, two printers to TLA+ text (fully parenthesised
on one line; minimal parentheses by TLA+'s precedence levels with bulleted junction lists),
and an evaluator over oracle.raft_spec states, or pairs of them, written from the rules of
DESIGN.md and the header of rmc_pred.h.  Nothing is read from the engine.
Test infrastructure only.

The AST is nested tuples, the first element the kind:
  ("num", n) ("const", name) ("srv", k) ("true",) ("false",) ("nil",) ("role", name) ("mtype", name)
  ("var", name)                          a bound name or a definition's parameter
  ("not", e) ("bin", op, a, b)           op as it is spelled: /\\ \\/ => <=> \\equiv = /= # < <= =< \\leq > >=
                                         \\geq \\subseteq \\cup \\cap \\ + -
  ("in", op, e, rhs)                     op \\in or \\notin; rhs a domain (no messages, no meet)
  ("if", c, a, b)
  ("q", "\\A" | "\\E", ((names, dom), ...), body)
  domains: ("d_set", set) ("d_quorum",) ("d_range", a, b) ("d_cap", a, b, c, d) ("d_log", logref)
           ("d_msgs", primed)
  ("server_set",) ("setlit", (e, ...)) ("setcomp", x, set, P)
  ("card", set) ("cardmsgs", primed) ("len", logref) ("lastterm", logref)
  ("logterm", logref, n) ("logval", logref, n);  logref: ("log", e, primed) or ("var", parameter)
  ("sv", variable, e, primed) ("sv2", variable, e, e, primed) ("msgcnt", m, primed) ("mf", m, field)
  ("ref", Name) ("call", Name, (args...)) ("prime", e)
"""
import functools
import random

from oracle import raft_spec as R

HOLDS, VIOLATED, ERROR = 0, 1, 2
NIL = -1

# the cfg constants of predicate_cases.write_model's defaults (the text names them; the evaluator knows them)
CONSTS = {"MaxTerm": 2, "MaxLogLen": 1, "MaxMsgs": 2, "MaxDup": 1}
ROLES = ("Follower", "Candidate", "Leader")
MTYPES = (R.RVQ, R.RVP, R.AEQ, R.AEP)
# field -> (type, the message type that has it or None)
FIELDS = {"mtype": ("T", None), "mterm": ("I", None), "msource": ("S", None), "mdest": ("S", None),
          "mlastLogTerm": ("I", R.RVQ), "mlastLogIndex": ("I", R.RVQ), "mvoteGranted": ("B", R.RVP),
          "mprevLogIndex": ("I", R.AEQ), "mprevLogTerm": ("I", R.AEQ), "mcommitIndex": ("I", R.AEQ),
          "msuccess": ("B", R.AEP), "mmatchIndex": ("I", R.AEP)}
SV = {"currentTerm": "I", "state": "R", "votedFor": "S", "commitIndex": "I", "votesResponded": "SET",
      "votesGranted": "SET"}
REL = ("<", "<=", "=<", "\\leq", ">", ">=", "\\geq")
JUNCTION = ("/\\", "\\/")


# ---- the evaluator -----------------------------------------------------------------------------
class EvalError(Exception):
    """A read outside a domain.  src: "log" (a position outside DOMAIN log[i]), "nil" (a variable
    indexed by Nil), "field" (a field the message's type does not have), "elem" ({e}, e no server)."""

    def __init__(self, src):
        Exception.__init__(self, src)
        self.src = src


class _St:
    """A state as the evaluator reads it: votedFor as an index (Nil = -1), the bag as a list of
    (fields, count) in an order of the evaluator's own."""
    __slots__ = ("s", "voted", "msgs")

    def __init__(self, s):
        self.s = s
        self.voted = tuple(NIL if v == R.NIL else v for v in s.votedFor)
        self.msgs = [(dict(m), c) for m, c in sorted(s.messages, key=repr)]


class _X:
    __slots__ = ("cur", "nxt", "S", "regs", "od", "masked", "probe", "nil_iter", "nil_card", "quorum_iter")

    def __init__(self, S, cur, nxt):
        self.S, self.cur, self.nxt = S, cur, nxt
        self.regs = [None] * 64
        self.od = False        # a message quantifier saw both an error and a deciding value
        self.masked = set()    # constructs whose unevaluated part would have been an error
        self.probe = 0
        self.nil_iter = self.nil_card = self.quorum_iter = False


def _probe(X, tag, thunk):
    """Would the part that short circuit left out have been an error?  (Statistics only.)"""
    if X.probe:
        return
    X.probe += 1
    od = X.od
    try:
        thunk()
    except EvalError:
        X.masked.add(tag)
    finally:
        X.probe -= 1
        X.od = od


def _enum_set(X, v):
    out = sorted(e for e in v if e != NIL)
    if NIL in v:
        out.append(NIL)  # Nil last
        if not X.probe:
            X.nil_iter = True
    return out


def _quorums(S):
    out = []
    for mask in range(1 << S):
        q = frozenset(j for j in range(S) if mask >> j & 1)
        if 2 * len(q) > S:
            out.append(q)
    return out


_QUORUMS = {S: _quorums(S) for S in range(1, 6)}


class Compiler:
    """AST -> Python closures f(X).  Definitions are expanded where they are referred to: a
    parameter stands for its argument, read in the caller's scope (so a bound name of the caller
    that the definition binds again is the caller's), and primed wherever the use is primed."""

    def __init__(self, defs):
        self.defs = defs  # name -> (params, body)

    def comp(self, n, env, pr, ns):
        """env: name -> ("reg", slot, primed bag or None) | ("param", arg, env of the call).
        pr: inside a primed expression.  ns: the next free register."""
        k = n[0]
        c = self.comp
        if k == "num":
            v = n[1]
            return lambda X: v
        if k == "const":
            v = CONSTS[n[1]]
            return lambda X: v
        if k == "srv":
            v = n[1]
            return lambda X: v
        if k in ("true", "false"):
            v = k == "true"
            return lambda X: v
        if k == "nil":
            return lambda X: NIL
        if k in ("role", "mtype"):
            v = n[1]
            return lambda X: v
        if k == "server_set":
            return lambda X: frozenset(range(X.S))
        if k == "var":
            b = env[n[1]]
            if b[0] == "reg":
                slot = b[1]
                return lambda X: X.regs[slot]
            return c(b[1], b[2], pr, ns)
        if k == "not":
            a = c(n[1], env, pr, ns)
            return lambda X: not a(X)
        if k == "if":
            cc, a, b = (c(x, env, pr, ns) for x in n[1:])

            def f_if(X):
                if cc(X):
                    _probe(X, "IF", lambda: b(X))
                    return a(X)
                _probe(X, "IF", lambda: a(X))
                return b(X)
            return f_if
        if k == "bin":
            return self.comp_bin(n, env, pr, ns)
        if k == "in":
            f = self.comp_in(n, env, pr, ns)
            if n[1] == "\\notin":
                return lambda X: not f(X)
            return f
        if k == "q":
            return self.comp_quant(n[1] == "\\A", [(nm, d) for names, d in n[2] for nm in names], n[3], env, pr, ns)
        if k == "setlit":
            es = [c(e, env, pr, ns) for e in n[1]]

            def f_setlit(X):
                out = set()
                for e in es:
                    v = e(X)
                    if not (v == NIL or 0 <= v < X.S):
                        raise EvalError("elem")
                    out.add(v)
                return frozenset(out)
            return f_setlit
        if k == "setcomp":
            dom = c(n[2], env, pr, ns)
            inner = dict(env)
            inner[n[1]] = ("reg", ns, None)
            body = c(n[3], inner, pr, ns + 1)

            def f_setcomp(X):
                out = []
                for e in _enum_set(X, dom(X)):
                    X.regs[ns] = e
                    if body(X):
                        out.append(e)
                return frozenset(out)
            return f_setcomp
        if k == "card":
            a = c(n[1], env, pr, ns)

            def f_card(X):
                v = a(X)
                if NIL in v and not X.probe:
                    X.nil_card = True
                return len(v)  # Nil counts
            return f_card
        if k == "cardmsgs":
            nx = pr or n[1]
            return lambda X: len((X.nxt if nx else X.cur).msgs)
        if k in ("len", "lastterm", "logterm", "logval"):
            return self.comp_log(n, env, pr, ns)
        if k == "sv":
            nx = pr or n[3]
            name = n[1]
            e = c(n[2], env, pr, ns)
            if name == "votedFor":
                def f_voted(X):
                    i = e(X)
                    if i < 0:
                        raise EvalError("nil")
                    return (X.nxt if nx else X.cur).voted[i]
                return f_voted

            def f_sv(X):
                i = e(X)
                if i < 0:
                    raise EvalError("nil")
                return getattr((X.nxt if nx else X.cur).s, name)[i]
            return f_sv
        if k == "sv2":
            nx = pr or n[4]
            name = n[1]
            e1, e2 = c(n[2], env, pr, ns), c(n[3], env, pr, ns)

            def f_sv2(X):
                i, j = e1(X), e2(X)
                if i < 0 or j < 0:
                    raise EvalError("nil")
                return getattr((X.nxt if nx else X.cur).s, name)[i][j]
            return f_sv2
        if k == "msgcnt":
            m = c(n[1], env, pr, ns)
            return lambda X: m(X)[1]
        if k == "mf":
            m = c(n[1], env, pr, ns)
            field = n[2]

            def f_mf(X):
                rec = m(X)[0]
                if field not in rec:
                    raise EvalError("field")
                return rec[field]
            return f_mf
        if k in ("ref", "call"):
            params, body = self.defs[n[1]]
            args = n[2] if k == "call" else ()
            assert len(params) == len(args)
            inner = {p: ("param", a, env) for p, a in zip(params, args)}
            return c(body, inner, pr, ns)
        if k == "prime":
            assert not pr
            return c(n[1], env, True, ns)
        raise AssertionError(k)

    def comp_bin(self, n, env, pr, ns):
        op = n[1]
        a, b = self.comp(n[2], env, pr, ns), self.comp(n[3], env, pr, ns)
        if op == "/\\":
            def f_and(X):
                if not a(X):
                    _probe(X, "/\\", lambda: b(X))
                    return False
                return b(X)
            return f_and
        if op == "\\/":
            def f_or(X):
                if a(X):
                    _probe(X, "\\/", lambda: b(X))
                    return True
                return b(X)
            return f_or
        if op == "=>":
            def f_imp(X):
                if not a(X):
                    _probe(X, "=>", lambda: b(X))
                    return True
                return b(X)
            return f_imp
        if op in ("<=>", "\\equiv", "="):
            return lambda X: a(X) == b(X)
        if op in ("/=", "#"):
            return lambda X: a(X) != b(X)
        if op == "<":
            return lambda X: a(X) < b(X)
        if op in ("<=", "=<", "\\leq"):
            return lambda X: a(X) <= b(X)
        if op == ">":
            return lambda X: a(X) > b(X)
        if op in (">=", "\\geq"):
            return lambda X: a(X) >= b(X)
        if op == "+":
            return lambda X: a(X) + b(X)
        if op == "-":
            return lambda X: a(X) - b(X)
        if op == "\\cup":
            return lambda X: a(X) | b(X)
        if op == "\\cap":
            return lambda X: a(X) & b(X)
        if op == "\\":
            return lambda X: a(X) - b(X)
        if op == "\\subseteq":
            return lambda X: a(X) <= b(X)
        raise AssertionError(op)

    def logref(self, n, env, pr, ns):
        """log[e] or a parameter that stands for it -> (closure of the server index, primed)."""
        while n[0] == "var":
            b = env[n[1]]
            assert b[0] == "param"
            n, env = b[1], b[2]
        assert n[0] == "log"
        return self.comp(n[1], env, pr, ns), pr or n[2]

    def comp_log(self, n, env, pr, ns):
        k = n[0]
        e, nx = self.logref(n[1], env, pr, ns)
        if k in ("len", "lastterm"):
            def f_len(X):
                i = e(X)
                if i < 0:
                    raise EvalError("nil")
                lg = (X.nxt if nx else X.cur).s.log[i]
                if k == "len":
                    return len(lg)
                return R.rget(lg[-1], "term") if lg else 0
            return f_len
        pos = self.comp(n[2], env, pr, ns)
        field = "term" if k == "logterm" else "value"

        def f_entry(X):
            i = e(X)
            p = pos(X)
            if i < 0:
                raise EvalError("nil")
            lg = (X.nxt if nx else X.cur).s.log[i]
            if not 1 <= p <= len(lg):
                raise EvalError("log")
            return R.rget(lg[p - 1], field)
        return f_entry

    def comp_in(self, n, env, pr, ns):
        lhs = self.comp(n[2], env, pr, ns)
        d, denv = n[3], env
        while d[0] == "d_set" and d[1][0] == "var" and denv[d[1][1]][0] == "param":
            b = denv[d[1][1]]
            d, denv = ("d_set", b[1]) if b[1][0] not in ("d_quorum", "d_range", "d_log") else b[1], b[2]
        if d[0] == "d_quorum":
            def f_isq(X):
                v = lhs(X)
                return NIL not in v and 2 * len(v) > X.S  # a set that holds Nil is no quorum
            return f_isq
        if d[0] == "d_range":
            a, b = self.comp(d[1], denv, pr, ns), self.comp(d[2], denv, pr, ns)

            def f_inrange(X):
                v, lo, hi = lhs(X), a(X), b(X)
                return lo <= v <= hi
            return f_inrange
        if d[0] == "d_log":
            e, nx = self.logref(d[1], denv, pr, ns)

            def f_indom(X):
                v = lhs(X)
                i = e(X)
                if i < 0:
                    raise EvalError("nil")
                return 1 <= v <= len((X.nxt if nx else X.cur).s.log[i])
            return f_indom
        s = self.comp(d[1], denv, pr, ns)
        return lambda X: lhs(X) in s(X)  # Nil \in {.., Nil} is TRUE

    def domain(self, d, env, pr, ns):
        """-> (closure giving the elements in order, kind), kind "msgs0" / "msgs1" for the two bags."""
        if d[0] == "d_set" and d[1][0] == "var" and env[d[1][1]][0] == "param":
            b = env[d[1][1]]
            if b[1][0].startswith("d_"):
                return self.domain(b[1], b[2], pr, ns)
            return self.domain(("d_set", b[1]), b[2], pr, ns)
        if d[0] == "d_quorum":
            def f_quorums(X):
                if not X.probe:
                    X.quorum_iter = True
                return _QUORUMS[X.S]
            return f_quorums, "set"
        if d[0] == "d_range":
            a, b = self.comp(d[1], env, pr, ns), self.comp(d[2], env, pr, ns)

            def f_range(X):
                lo, hi = a(X), b(X)
                return range(lo, hi + 1)
            return f_range, "int"
        if d[0] == "d_cap":
            a, b, cc, dd = (self.comp(x, env, pr, ns) for x in d[1:])

            def f_cap(X):
                lo1, hi1, lo2, hi2 = a(X), b(X), cc(X), dd(X)
                return range(max(lo1, lo2), min(hi1, hi2) + 1)
            return f_cap, "int"
        if d[0] == "d_log":
            e, nx = self.logref(d[1], env, pr, ns)

            def f_dlog(X):
                i = e(X)
                if i < 0:
                    raise EvalError("nil")
                return range(1, len((X.nxt if nx else X.cur).s.log[i]) + 1)
            return f_dlog, "int"
        if d[0] == "d_msgs":
            nx = pr or d[1]
            return (lambda X: (X.nxt if nx else X.cur).msgs), "msgs"
        s = self.comp(d[1], env, pr, ns)
        return (lambda X: _enum_set(X, s(X))), "server"

    def comp_quant(self, all_, binds, body, env, pr, ns):
        if not binds:
            return self.comp(body, env, pr, ns)
        (name, d), rest = binds[0], binds[1:]
        dom, kind = self.domain(d, env, pr, ns)
        inner = dict(env)
        inner[name] = ("reg", ns, None)
        sub = self.comp_quant(all_, rest, body, inner, pr, ns + 1)
        tag = "\\A" if all_ else "\\E"
        if kind == "msgs":
            def f_qmsgs(X):
                # the bag's order is the engine's own: every element is evaluated
                err, decided = None, False
                for el in dom(X):
                    X.regs[ns] = el
                    try:
                        if bool(sub(X)) != all_:
                            decided = True
                    except EvalError as e:
                        err = err or e
                if err and decided:
                    X.od = True
                    return not all_
                if err:
                    raise err
                return not all_ if decided else all_
            return f_qmsgs

        def f_quant(X):
            els = list(dom(X))
            for t, el in enumerate(els):
                X.regs[ns] = el
                if bool(sub(X)) != all_:  # \A stops at the first FALSE, \E at the first TRUE
                    def remaining():
                        for el2 in els[t + 1:]:
                            X.regs[ns] = el2
                            sub(X)
                    _probe(X, tag, remaining)
                    return not all_
            return all_
        return f_quant


class Evaluated:
    """One evaluation: the verdict and what the non-vacuity tests count."""
    __slots__ = ("verdict", "raw", "order_dependent", "error_source", "masked", "nil_iter", "nil_card", "quorum_iter")


def evaluate(fn, n_servers, s, t=None):
    """fn: a compiled predicate.  s: an oracle state; t: its successor (action mode: the stutter
    rule of [A]_vars applies: violated on t = s is holds; an error stays an error)."""
    X = _X(n_servers, _St(s), _St(t) if t is not None else None)
    out = Evaluated()
    out.error_source = None
    try:
        out.verdict = HOLDS if fn(X) else VIOLATED
    except EvalError as e:
        out.verdict = ERROR
        out.error_source = e.src
    out.raw = out.verdict  # before the stutter rule
    if t is not None and out.verdict == VIOLATED and s == t:
        out.verdict = HOLDS
    out.order_dependent = X.od
    out.masked = frozenset(X.masked)
    out.nil_iter, out.nil_card, out.quorum_iter = X.nil_iter, X.nil_card, X.quorum_iter
    return out


def compile_predicate(defs, body):
    return Compiler(defs).comp(body, {}, False, 0)


# ---- printer (a): fully parenthesised, one line --------------------------------------------------
def _srv_name(k):
    return "r%d" % (k + 1)


def _pr(flag):
    return "'" if flag else ""


def text_full(n):
    k = n[0]
    f = text_full
    if k == "num":
        return str(n[1])
    if k == "const":
        return n[1]
    if k == "srv":
        return _srv_name(n[1])
    if k in ("true", "false"):
        return k.upper()
    if k == "nil":
        return "Nil"
    if k in ("role", "mtype", "var", "ref"):
        return n[1]
    if k == "server_set":
        return "Server"
    if k == "not":
        return "(~%s)" % f(n[1])
    if k == "bin":
        return "(%s %s %s)" % (f(n[2]), n[1], f(n[3]))
    if k == "in":
        return "(%s %s %s)" % (f(n[2]), n[1], _dom_full(n[3]))
    if k == "if":
        return "(IF %s THEN %s ELSE %s)" % (f(n[1]), f(n[2]), f(n[3]))
    if k == "q":
        return "(%s %s : %s)" % (n[1], ", ".join("%s \\in %s" % (", ".join(names), _dom_full(d)) for names, d in n[2]),
                                 f(n[3]))
    if k == "setlit":
        return "{%s}" % ", ".join(f(e) for e in n[1])
    if k == "setcomp":
        return "{%s \\in %s : %s}" % (n[1], f(n[2]), f(n[3]))
    if k == "card":
        return "Cardinality(%s)" % f(n[1])
    if k == "cardmsgs":
        return "Cardinality(DOMAIN messages%s)" % _pr(n[1])
    if k == "log":
        return "log%s[%s]" % (_pr(n[2]), f(n[1]))
    if k == "len":
        return "Len(%s)" % f(n[1])
    if k == "lastterm":
        return "LastTerm(%s)" % f(n[1])
    if k in ("logterm", "logval"):
        return "%s[%s].%s" % (f(n[1]), f(n[2]), "term" if k == "logterm" else "value")
    if k == "sv":
        return "%s%s[%s]" % (n[1], _pr(n[3]), f(n[2]))
    if k == "sv2":
        return "%s%s[%s][%s]" % (n[1], _pr(n[4]), f(n[2]), f(n[3]))
    if k == "msgcnt":
        return "messages%s[%s]" % (_pr(n[2]), f(n[1]))
    if k == "mf":
        return "%s.%s" % (f(n[1]), n[2])
    if k == "call":
        return "%s(%s)" % (n[1], ", ".join(f(a) for a in n[2]))
    if k == "prime":
        return f(n[1]) + "'" if n[1][0] in ("ref", "call") else "(%s)'" % f(n[1])
    raise AssertionError(k)


def _dom_full(d):
    f = text_full
    if d[0] == "d_set":
        return f(d[1])
    if d[0] == "d_quorum":
        return "Quorum"
    if d[0] == "d_range":
        return "(%s..%s)" % (f(d[1]), f(d[2]))
    if d[0] == "d_cap":
        return "((%s..%s) \\cap (%s..%s))" % tuple(f(x) for x in d[1:])
    if d[0] == "d_log":
        return "DOMAIN %s" % f(d[1])
    if d[0] == "d_msgs":
        return "DOMAIN messages%s" % _pr(d[1])
    raise AssertionError(d[0])


# ---- printer (b): minimal parentheses, bulleted junction lists ------------------------------------
# TLA+'s precedence levels: => 1, <=> 2, /\ and \/ 3, ~ 4, relations, \in and \subseteq 5, the set
# operators 8, .. 9, + 10, - 11; application, . and ' above all.  Different operators of one level
# are parenthesised (SANY demands it); a quantifier or IF is parenthesised unless it ends its
# expression; a chain of two or more /\ or \/ is a column-aligned bulleted list.
LEVEL = {"=>": 1, "<=>": 2, "\\equiv": 2, "/\\": 3, "\\/": 3, "\\subseteq": 5, "\\cup": 8, "\\cap": 8, "\\": 8,
         "+": 10, "-": 11, "=": 5, "/=": 5, "#": 5}
LEVEL.update({op: 5 for op in REL})
ASSOC = ("/\\", "\\/", "\\cup", "\\cap", "+")   # a op (b op c) = (a op b) op c, so no parentheses either side
LEFT = ("-",)                                   # left-associative: a - b - c is (a - b) - c
TOP = 20


def _level(n):
    k = n[0]
    if k == "bin":
        return LEVEL[n[1]]
    if k == "not":
        return 4
    if k == "in":
        return 5
    if k in ("if", "q"):
        return 0
    return TOP


def _chain(n, op):
    """The items of a chain of one junction, in evaluation order."""
    if n[0] == "bin" and n[1] == op:
        return _chain(n[2], op) + _chain(n[3], op)
    return [n]


def _is_list(n):
    return n[0] == "bin" and n[1] in JUNCTION and len(_chain(n, n[1])) >= 3


def _end(col, lines):
    """The column after a text whose first line began at col (later lines are whole lines)."""
    return col + len(lines[0]) if len(lines) == 1 else len(lines[-1])


def _cat(col, lines, s):
    return lines[:-1] + [lines[-1] + s]


def _join(col, a, b):
    """b's first line goes on a's last."""
    return a[:-1] + [a[-1] + b[0]] + b[1:]


class Layout:
    def seq(self, col, parts):
        """parts: strings and functions (col, ) -> lines, laid out one after another."""
        lines = [""]
        for p in parts:
            if isinstance(p, str):
                lines = _cat(col, lines, p)
            else:
                lines = _join(col, lines, p(_end(col, lines)))
        return lines

    def child(self, n, need, tail, same_ok=None):
        """n as an operand that must bind at least as tightly as `need`; same_ok: the operator
        that may stand at exactly that level without parentheses."""
        lv = _level(n)
        if same_ok == "any":  # a set expression as a whole operand: one set operator stands bare
            same_ok, need = None, (7 if lv == 8 else 8)
        if n[0] in ("if", "q"):
            bare = tail
        elif _is_list(n):
            bare = tail and need <= 3 and same_ok is None
        elif lv > need:
            bare = True
        elif lv == need:
            bare = n[0] == "bin" and n[1] == same_ok
        else:
            bare = False
        if bare:
            return lambda col: self.expr(n, col, tail)
        return lambda col: self.seq(col, ["(", lambda c: self.expr(n, c, True), ")"])

    def expr(self, n, col, tail):
        k = n[0]
        if k == "bin":
            op = n[1]
            if op in JUNCTION:
                items = _chain(n, op)
                if len(items) >= 3:
                    lines = []
                    for t, it in enumerate(items):
                        sub = self.expr(it, col + 3, True)
                        lines.append((" " * col if t else "") + op + " " + sub[0])
                        lines.extend(sub[1:])
                    return lines
            lv = LEVEL[op]
            if op in ("=>", "<=>", "\\equiv") and _is_list(n[2]):
                # the list ends at a token left of its bullets: no parentheses
                left = self.expr(n[2], col + 3, True)
                right = self.seq(col + len(op) + 1, [self.child(n[3], lv + 1, tail)])
                return ["   " + left[0]] + left[1:] + [" " * col + op + " " + right[0]] + right[1:]
            a = self.child(n[2], lv, False, op if op in ASSOC or op in LEFT else None)
            b = self.child(n[3], lv, tail, op if op in ASSOC else None)
            return self.seq(col, [a, " " + op + " ", b])
        if k == "not":
            return self.seq(col, ["~", self.child(n[1], 4, tail, None) if n[1][0] != "not" else
                                  (lambda c: self.seq(c, [" ", self.child(n[1], 4, tail)]))])
        if k == "in":
            return self.seq(col, [self.child(n[2], 6, False), " " + n[1] + " ", lambda c: self.dom(n[3], c, tail)])
        if k == "if":
            cc = self.expr(n[1], col + 3, True)
            a = self.expr(n[2], col + 5, True)
            b = self.expr(n[3], col + 5, tail)
            if len(cc) == len(a) == len(b) == 1:
                return ["IF %s THEN %s ELSE %s" % (cc[0], a[0], b[0])]
            pad = " " * col
            return ["IF " + cc[0]] + cc[1:] + [pad + "THEN " + a[0]] + a[1:] + [pad + "ELSE " + b[0]] + b[1:]
        if k == "q":
            parts = [n[1] + " "]
            for t, (names, d) in enumerate(n[2]):
                parts += [(", " if t else "") + ", ".join(names) + " \\in ", lambda c, d=d: self.dom(d, c, False)]
            parts += [" : ", lambda c: self.expr(n[3], c, True)]
            return self.seq(col, parts)
        if k == "setlit":
            parts = ["{"]
            for t, e in enumerate(n[1]):
                parts += [", " if t else "", self.child(e, 0, t == len(n[1]) - 1)]
            return self.seq(col, parts + ["}"])
        if k == "setcomp":
            return self.seq(col, ["{" + n[1] + " \\in ", self.child(n[2], 8, False, "any"), " : ",
                                  lambda c: self.expr(n[3], c, True), "}"])
        if k == "card":
            return self.seq(col, ["Cardinality(", lambda c: self.expr(n[1], c, True), ")"])
        if k == "log":
            return self.seq(col, ["log" + _pr(n[2]) + "[", lambda c: self.expr(n[1], c, True), "]"])
        if k in ("len", "lastterm"):
            return self.seq(col, ["Len(" if k == "len" else "LastTerm(", lambda c: self.expr(n[1], c, True), ")"])
        if k in ("logterm", "logval"):
            return self.seq(col, [lambda c: self.expr(n[1], c, True), "[", lambda c: self.expr(n[2], c, True),
                                  "].term" if k == "logterm" else "].value"])
        if k == "sv":
            return self.seq(col, [n[1] + _pr(n[3]) + "[", lambda c: self.expr(n[2], c, True), "]"])
        if k == "sv2":
            return self.seq(col, [n[1] + _pr(n[4]) + "[", lambda c: self.expr(n[2], c, True), "][",
                                  lambda c: self.expr(n[3], c, True), "]"])
        if k == "msgcnt":
            return self.seq(col, ["messages" + _pr(n[2]) + "[", lambda c: self.expr(n[1], c, True), "]"])
        if k == "mf":
            return self.seq(col, [lambda c: self.expr(n[1], c, True), "." + n[2]])
        if k == "call":
            parts = [n[1] + "("]
            for t, a in enumerate(n[2]):
                parts += [", " if t else "", self.child(a, 0, t == len(n[2]) - 1)]
            return self.seq(col, parts + [")"])
        if k == "prime":
            if n[1][0] in ("ref", "call"):
                return self.seq(col, [lambda c: self.expr(n[1], c, True), "'"])
            return self.seq(col, ["(", lambda c: self.expr(n[1], c, True), ")'"])
        return [text_full(n)]

    def dom(self, d, col, tail):
        if d[0] == "d_set":
            return self.seq(col, [self.child(d[1], 8, tail, "any")])
        if d[0] == "d_range":
            return self.seq(col, [self.child(d[1], 10, False), "..", self.child(d[2], 10, tail)])
        if d[0] == "d_cap":
            a, b, cc, dd = (self.child(x, 10, False) for x in d[1:])
            return self.seq(col, ["(", a, "..", b, ") \\cap (", cc, "..", dd, ")"])
        if d[0] == "d_log":
            return self.seq(col, ["DOMAIN ", lambda c: self.expr(d[1], c, True)])
        return [_dom_full(d)]


def text_min(n, col=0):
    """Printer (b): the lines of n, the first beginning at column col."""
    return Layout().expr(n, col, True)


def definition_text(name, params, body, minimal, action=False):
    head = name + ("(%s)" % ", ".join(params) if params else "") + " =="
    if action:
        head += " [][" if not minimal else " [][\n   "
        tail = "]_vars" if not minimal else "\n    ]_vars"
    else:
        head, tail = head + ("\n   " if minimal else ""), ""
    if not minimal:
        return head + " " + text_full(body) + tail
    lines = text_min(body, 4)
    return head + " " + "\n".join(lines) + tail


# ---- the generator -----------------------------------------------------------------------------
BOUND_NAMES = ("i", "j", "k", "n", "p", "q", "u", "w")
MAX_COST = 2000          # the product of the domain sizes of the open loops, roughly


class Gen:
    """A seeded generator of well-typed expressions.  scope: [(name, kind, info)] with kind "S" (a
    server), "I" (an integer; info: the log reference it is a position of, or None), "Q" (a set:
    a quorum, or a set parameter), "M" (a message; info: its bag is the successor's), "L" (a
    parameter that stands for log[i])."""

    def __init__(self, rng, helpers, action=False, closed=False):
        self.r = rng
        self.helpers = helpers     # name -> (params, kinds, type, body)
        self.action = action
        self.scope = []
        self.primed = False
        self.cost = 1
        self.mtype_known = {}      # message name -> the type a guard established
        self.safe = []             # server expressions a guard showed to be no Nil
        self.names_server = False
        self.in_msg_body = 0
        self.in_arg = 0            # inside an argument of a definition
        self.closed = closed       # no server model values (the SYMMETRY tests need predicates without)
        self.max_bind = 5          # bound names of this definition alone (those of the definitions it calls add)

    # -- helpers of the generator itself
    def pick(self, xs):
        return xs[self.r.randrange(len(xs))]

    def chance(self, p):
        return self.r.random() < p

    def vars_of(self, kind):
        return [(nm, info) for nm, kd, info in self.scope if kd == kind]

    def fresh(self):
        used = {nm for nm, _k, _i in self.scope}
        return next(nm for nm in BOUND_NAMES if nm not in used)

    def can_bind(self, k=1):
        return sum(1 for nm, _kd, _i in self.scope if nm in BOUND_NAMES) + k <= self.max_bind

    def pp(self):
        """Whether a state read is written primed (action mode, outside a primed expression)."""
        return self.action and not self.primed and self.chance(0.4)

    # -- servers
    def server(self, d, safe=False):
        vs = self.vars_of("S")
        ms = self.vars_of("M")
        strict = self.in_msg_body > 0   # under a message quantifier no evaluation may be an error (see msg_pred)
        if strict:
            vs = [v for v in vs if v[1] == "clean"]
        c = []
        if vs:
            c += ["var"] * 6
        if ms:
            c += ["mf"] * 2
        if self.safe and not (strict and (self.action or self.primed)):
            c += ["safe"] * 3
        if not self.closed:
            c += ["srv"]
        if not safe and not strict and d > 0 and (vs or ms):
            c += ["voted", "voted", "if"]
        if not c:
            if self.closed and strict:
                return ("mf", ("var", ms[0][0]), "msource")
            self.names_server = True
            return ("srv", self.r.randrange(2))
        k = self.pick(c)
        if k == "var":
            return ("var", self.pick(vs)[0])
        if k == "mf":
            return ("mf", ("var", self.pick(ms)[0]), self.pick(("msource", "mdest")))
        if k == "safe":
            return self.pick(self.safe)
        if k == "srv":
            self.names_server = True
            return ("srv", self.r.randrange(2))
        if k == "voted":
            return ("sv", "votedFor", self.server(d - 1, True), self.pp())
        return ("if", self.boolean(d - 1), self.server(d - 1, True), self.server_or_nil(d - 1))

    def server_or_nil(self, d):
        return ("nil",) if self.chance(0.3) else self.server(d)

    def logref(self, d):
        ls = self.vars_of("L")
        if ls and self.chance(0.5):
            return ("var", self.pick(ls)[0])
        return ("log", self.server(d - 1, self.in_msg_body > 0 or self.chance(0.9)), self.pp())

    # -- integers
    def integer(self, d):
        c = ["num", "num", "const"]
        ivs = self.vars_of("I")
        ms = self.vars_of("M")
        if ivs:
            c += ["var"] * 3
        if d > 0:
            c += ["term", "term", "commit", "len", "len", "lastterm", "card", "cardmsgs", "add", "sub", "next", "match",
                  "entry", "if"]
            if self.action:
                c += ["cardmsgs", "cardmsgs"]
            if ms:
                c += ["msgcnt", "mfield", "mfield", "mfield"] * (4 if self.mtype_known else 1)
            c += ["call"] * (2 if any(h[2] == "I" for h in self.helpers.values()) else 0)
        k = self.pick(c)
        if k == "num":
            return ("num", self.pick((0, 1, 1, 2, 2, 3, 4, -1, -2)))
        if k == "const":
            return ("const", self.pick(sorted(CONSTS)))
        if k == "var":
            return ("var", self.pick(ivs)[0])
        if k == "term":
            return ("sv", "currentTerm", self.server(d - 1), self.pp())
        if k == "commit":
            return ("sv", "commitIndex", self.server(d - 1), self.pp())
        if k == "len":
            return ("len", self.logref(d))
        if k == "lastterm":
            return ("lastterm", self.logref(d))
        if k == "card":
            if self.chance(0.4):  # a set that holds Nil: Cardinality counts it
                return ("card", ("bin", "\\cup", self.set(d - 1), ("setlit", (("nil",), self.server(0, True)))))
            return ("card", self.set(d - 1))
        if k == "cardmsgs":
            return ("cardmsgs", self.pp())
        if k in ("add", "sub"):
            return ("bin", "+" if k == "add" else "-", self.integer(d - 1), self.integer(d - 1))
        if k in ("next", "match"):
            return ("sv2", "nextIndex" if k == "next" else "matchIndex", self.server(d - 1), self.server(d - 1), self.pp())
        if k == "entry":
            return self.entry(d, "logterm")
        if k == "if":
            return ("if", self.boolean(d - 1), self.integer(d - 1), self.integer(d - 1))
        if k == "msgcnt":
            # messages[m] reads the bag m was bound in: inside a primed expression only the successor's
            ok = [(nm, bool(bag)) for nm, bag in ms if bag or not self.primed]
            if not ok:
                return ("cardmsgs", self.pp())
            nm, bag = self.pick(ok)
            return ("msgcnt", ("var", nm), bag and not self.primed)
        if k == "mfield":
            return self.msg_field("I", d)
        if k == "call":
            return self.call("I", d)
        raise AssertionError(k)

    def entry(self, d, kind):
        """log[e][n].term / .value: mostly at a position bound in that log's domain."""
        pos = [(nm, info) for nm, info in self.vars_of("I") if info is not None and info[1] == self.primed]
        if pos and (self.in_msg_body or self.chance(0.85)):
            nm, (ref, _ctx) = self.pick(pos)
            return (kind, ref, ("var", nm))
        ref = self.logref(d)
        if self.in_msg_body:
            return ("lastterm", ref) if kind == "logterm" else ("len", ref)
        p = self.pick([("num", 1), ("num", 1), ("num", 2), ("len", ref), ("len", ref),
                       ("sv", "commitIndex", self.server(0, True), False)])
        return (kind, ref, p)

    def msg_field(self, ty, d):
        ms = self.vars_of("M")
        nm = self.pick(ms)[0]
        known = self.mtype_known.get(nm)
        common = [f for f, (t, own) in FIELDS.items() if t == ty and own is None]
        typed = [f for f, (t, own) in FIELDS.items() if t == ty and own is not None and own == known]
        wild = [f for f, (t, own) in FIELDS.items() if t == ty and own is not None]
        if typed and self.chance(0.8):
            return ("mf", ("var", nm), self.pick(typed))
        if wild and not common and self.in_msg_body:
            return ("true",) if ty == "B" else ("num", 1)
        if wild and not self.in_msg_body and (not common or self.chance(0.06)):
            return ("mf", ("var", nm), self.pick(wild))
        return ("mf", ("var", nm), self.pick(common))

    # -- roles, message types
    def role(self, d):
        if d > 0 and self.chance(0.15):
            return ("if", self.boolean(d - 1), self.role(d - 1), self.role(0))
        if d > 0 and self.chance(0.6):
            return ("sv", "state", self.server(d - 1), self.pp())
        return ("role", self.pick(ROLES))

    def mtype(self, d):
        ms = self.vars_of("M")
        if d > 0 and self.chance(0.3):
            return ("if", self.boolean(d - 1), self.mtype(d - 1), self.mtype(0))
        if ms and self.chance(0.7):
            return ("mf", ("var", self.pick(ms)[0]), "mtype")
        return ("mtype", self.pick(MTYPES))

    # -- sets
    def set(self, d):
        c = ["Server", "Server", "empty", "lit"]
        qs = self.vars_of("Q")
        if qs:
            c += ["var"] * 3
        if d > 0:
            c += ["vresp", "vgrant", "vgrant", "lit", "cup", "cap", "minus", "comp", "if"]
            c += ["call"] * (2 if any(h[2] == "SET" for h in self.helpers.values()) else 0)
        k = self.pick(c)
        if k == "Server":
            return ("server_set",)
        if k == "empty":
            return ("setlit", ())
        if k == "lit":
            return ("setlit", tuple(self.server_or_nil(d - 1) for _ in range(self.r.randint(1, 3))))
        if k == "var":
            return ("var", self.pick(qs)[0])
        if k in ("vresp", "vgrant"):
            return ("sv", "votesResponded" if k == "vresp" else "votesGranted", self.server(d - 1), self.pp())
        if k in ("cup", "cap", "minus"):
            return ("bin", {"cup": "\\cup", "cap": "\\cap", "minus": "\\"}[k], self.set(d - 1), self.set(d - 1))
        if k == "comp":
            if not self.can_bind() or self.cost * 4 > MAX_COST:
                return ("server_set",)
            dom = ("server_set",) if self.in_msg_body else self.set(d - 1)
            nm = self.fresh()
            self.scope.append((nm, "S", "clean" if dom == ("server_set",) else None))
            self.cost *= 4
            body = self.boolean(d - 1)
            self.cost //= 4
            self.scope.pop()
            return ("setcomp", nm, dom, body)
        if k == "if":
            return ("if", self.boolean(d - 1), self.set(d - 1), self.set(d - 1))
        return self.call("SET", d)

    # -- definitions
    def call(self, ty, d):
        names = [nm for nm, h in sorted(self.helpers.items()) if h[2] == ty and
                 not (self.in_msg_body and may_err(h[3], self.helpers))]
        # an argument that refers to the definition it is passed to, F(F(x)), is refused by the compiler as
        # "recursive" (it expands arguments inside the body): no definition is called inside an argument
        if self.in_arg or self.cost * 16 > MAX_COST:
            names = []
        if not names:
            return {"I": ("num", 1), "SET": ("server_set",), "B": ("true",)}[ty]
        nm = self.pick(names)
        params, kinds, _ty, _body = self.helpers[nm]
        args = []
        self.in_arg += 1
        for kd in kinds:
            if kd == "S":
                args.append(self.server(min(d - 1, 1)))
            elif kd == "I":
                args.append(self.integer(min(d - 1, 1)))
            elif kd == "SET":
                args.append(self.set(min(d - 1, 1)))
            else:
                args.append(("log", self.server(0, self.chance(0.9)), False) if not self.vars_of("L") or self.chance(0.7)
                            else ("var", self.pick(self.vars_of("L"))[0]))
        self.in_arg -= 1
        if len(kinds) == 2 and kinds[0] == kinds[1] == "S" and len(self.vars_of("S")) >= 2 and self.chance(0.7):
            vs = [v for v, _ in self.vars_of("S")]
            a = self.r.randrange(len(vs) - 1)
            args = [("var", vs[a + 1]), ("var", vs[a])]  # the later bound name first
        n = ("call", nm, tuple(args)) if params else ("ref", nm)
        if self.action and not self.primed and self.chance(0.35) and self.primable(n) and \
                not (self.in_msg_body and any(x[0] in ("logterm", "logval") for x in walk(n))):
            return ("prime", n)
        return n

    def primable(self, n):
        """n' is in the language: no prime inside, and no messages[m] (m keeps the bag it was bound in)."""
        flag = {"sv": 3, "sv2": 4, "log": 2, "cardmsgs": 1, "d_msgs": 1}
        return not any(x[0] in ("prime", "msgcnt") or (x[0] in flag and x[flag[x[0]]]) for x in walk(n))

    # -- Booleans
    def boolean(self, d):
        if d <= 0:
            return self.atom_bool(0)
        c = ["and", "and", "or", "or", "imp", "imp", "iff", "not", "rel", "rel", "rel", "eq", "eq", "eq", "in", "in",
             "subset", "if", "quant", "quant", "quant", "atom", "err", "junction", "guardnil"]
        if self.vars_of("M"):
            c += ["guardmsg"] * 6
        if any(h[2] == "B" for h in self.helpers.values()):
            c += ["call"] * 5
        if self.action and not self.primed:
            c += ["prime"] * 3
        k = self.pick(c)
        if k == "err" and self.in_msg_body:
            k = "rel"
        if k in ("and", "or"):
            return ("bin", "/\\" if k == "and" else "\\/", self.boolean(d - 1), self.boolean(d - 1))
        if k == "junction":
            op = self.pick(JUNCTION)
            out = self.boolean(d - 1)
            for _ in range(self.r.randint(2, 3)):
                out = ("bin", op, out, self.boolean(d - 1))
            return out
        if k == "imp":
            return ("bin", "=>", self.boolean(d - 1), self.boolean(d - 1))
        if k == "iff":
            return ("bin", self.pick(("<=>", "\\equiv")), self.boolean(d - 1), self.boolean(d - 1))
        if k == "not":
            return ("not", self.boolean(d - 1))
        if k == "rel":
            return ("bin", self.pick(REL), self.integer(d - 1), self.integer(d - 1))
        if k == "eq":
            op = self.pick(("=", "=", "/=", "#"))
            ty = self.pick(("I", "I", "S", "S", "R", "R", "T", "SET", "B", "V") + ("T", "T") * bool(self.vars_of("M")))
            if ty == "I":
                return ("bin", op, self.integer(d - 1), self.integer(d - 1))
            if ty == "S":
                return ("bin", op, self.server(d - 1), self.server_or_nil(d - 1))
            if ty == "R":
                return ("bin", op, self.role(d - 1), self.role(d - 1))
            if ty == "T":
                return ("bin", op, self.mtype(d - 1), self.mtype(d - 1))
            if ty == "SET":
                return ("bin", op, self.set(d - 1), self.set(d - 1))
            if ty == "B":
                return ("bin", op, self.boolean(d - 1), self.boolean(d - 1))
            a, b = self.entry(d, "logval"), self.entry(d, "logval")
            if a[0] != "logval" or b[0] != "logval":
                return ("bin", op, self.integer(d - 1), self.integer(d - 1))
            return ("bin", op, a, b)
        if k == "in":
            op = self.pick(("\\in", "\\in", "\\notin"))
            w = self.pick(("set", "set", "quorum", "range", "dlog"))
            if w == "set":
                return ("in", op, self.server_or_nil(d - 1), ("d_set", self.set(d - 1)))
            if w == "quorum":
                return ("in", op, self.set(d - 1), ("d_quorum",))
            if w == "range":
                return ("in", op, self.integer(d - 1), ("d_range", self.integer(d - 2), self.integer(d - 2)))
            return ("in", op, self.integer(d - 1), ("d_log", self.logref(d)))
        if k == "subset":
            return ("bin", "\\subseteq", self.set(d - 1), self.set(d - 1))
        if k == "if":
            return ("if", self.boolean(d - 1), self.boolean(d - 1), self.boolean(d - 1))
        if k == "quant":
            return self.quant(d)
        if k == "err":
            return self.error_prone(d)
        if k == "guardnil":
            e = ("sv", "votedFor", self.server(0, True), False)
            if e[2][0] == "srv" or self.primed or (self.in_msg_body and self.action):
                return self.atom_bool(d)
            self.safe.append(e)
            body = self.boolean(d - 1)
            self.safe.pop()
            guard = ("bin", self.pick(("/=", "#")), e, ("nil",))
            return self.guarded(guard, body)
        if k == "guardmsg":
            nm = self.pick(self.vars_of("M"))[0]
            if nm in self.mtype_known:
                return self.atom_bool(d)
            ty = self.pick(MTYPES)
            self.mtype_known[nm] = ty
            body = self.boolean(d - 1)
            del self.mtype_known[nm]
            return self.guarded(("bin", "=", ("mf", ("var", nm), "mtype"), ("mtype", ty)), body)
        if k == "call":
            return self.call("B", d)
        if k == "prime":
            self.primed = True
            body = self.boolean(d - 1)
            self.primed = False
            return ("prime", body)
        return self.atom_bool(d)

    def msg_pred(self, d):
        """A quantifier over a bag whose body reads the fields of one message type behind a guard."""
        nm = self.fresh()
        bag = self.pp()
        self.scope.append((nm, "M", bag))
        self.cost *= 40
        self.in_msg_body += 1
        ty = self.pick(MTYPES)
        self.mtype_known[nm] = ty
        own = [f for f, (_t, o) in FIELDS.items() if o == ty]
        self.r.shuffle(own)
        inner = None
        for f in own[:2]:
            e = ("mf", ("var", nm), f)
            e = e if FIELDS[f][0] == "B" else ("bin", self.pick(REL), e, self.integer(1))
            inner = e if inner is None else ("bin", self.pick(JUNCTION), inner, e)
        body = ("bin", self.pick(JUNCTION), inner, self.boolean(d - 2))
        del self.mtype_known[nm]
        body = self.guarded(("bin", "=", ("mf", ("var", nm), "mtype"), ("mtype", ty)), body)
        if self.chance(0.5):
            body = ("bin", self.pick(("/\\", "\\/", "=>")), self.boolean(d - 2), body)
        self.in_msg_body -= 1
        self.cost //= 40
        self.scope.pop()
        return ("q", self.pick(("\\A", "\\E")), (((nm,), ("d_msgs", bag)),), body)

    def guarded(self, guard, body):
        w = self.r.randrange(3)
        if w == 0:
            return ("bin", "=>", guard, body)
        if w == 1:
            return ("bin", "/\\", guard, body)
        return ("if", guard, body, self.pick((("true",), ("false",))))

    def atom_bool(self, d):
        ms = self.vars_of("M")
        if ms and self.chance(0.3):
            return self.msg_field("B", d)
        w = self.r.randrange(6)
        if w == 0:
            return self.pick((("true",), ("true",), ("false",)))
        if w == 1:
            return ("bin", self.pick(("=", "/=", "#")), self.role(1), ("role", self.pick(ROLES)))
        if w == 2:
            return ("bin", self.pick(REL), self.integer(1), self.integer(0))
        if w == 3:
            return ("in", self.pick(("\\in", "\\notin")), self.server_or_nil(1), ("d_set", self.set(1)))
        if w == 4:
            return ("bin", self.pick(("=", "/=")), self.server(1), self.server_or_nil(1))
        return ("bin", self.pick(REL), self.integer(1), self.integer(1))

    def error_prone(self, d):
        """A Boolean whose evaluation is an error on some states: the three sources, unguarded."""
        w = self.r.randrange(3)
        ms = self.vars_of("M")
        if w == 0:
            ref = ("log", self.server(0, True), self.pp())
            return ("bin", self.pick(REL), ("logterm", ref, self.pick((("num", 1), ("num", 2), ("len", ref)))),
                    self.integer(1))
        if w == 1:
            i = self.server(0, True)
            return ("bin", self.pick(REL), ("sv", "currentTerm", ("sv", "votedFor", i, self.pp()), self.pp()), self.integer(1))
        # a field of one message type read on every message: an error if the bag holds another type, and
        # TRUE otherwise, so no element decides and the bag's order does not matter
        f = self.pick([f for f, (t, own) in FIELDS.items() if own is not None])
        if not self.can_bind() or self.cost * 40 > MAX_COST:
            return self.atom_bool(0)
        nm = self.fresh()
        bag = self.pp()
        e = ("mf", ("var", nm), f)
        body = ("bin", "\\/", e, ("true",)) if FIELDS[f][0] == "B" else ("bin", self.pick((">=", "\\geq")), e, ("num", -1))
        return ("q", "\\A", (((nm,), ("d_msgs", bag)),), body)

    def quant(self, d):
        q = self.pick(("\\A", "\\A", "\\E"))
        groups, pushed, cost0 = [], 0, self.cost
        shape = self.pick(("one", "one", "one", "two", "three", "dep", "dep", "twogroups"))
        plan = {"one": [1], "two": [2], "three": [3], "dep": [1, 1], "twogroups": [self.r.randint(1, 2), 1]}[shape]
        for g, count in enumerate(plan):
            if not self.can_bind(count):
                break
            dom, kind, info, cost = self.domain(d, dependent=(shape == "dep" and g == 1))
            if self.cost * cost ** count > MAX_COST:
                if kind == "M" or not groups:
                    dom, kind, info, cost = ("d_range", ("num", 1), ("num", 2)), "I", None, 2
                    if self.cost * cost ** count > MAX_COST:
                        break
                else:
                    break
            names = []
            for _ in range(count):
                nm = self.fresh()
                self.scope.append((nm, kind, info))
                pushed += 1
                names.append(nm)
                self.cost *= cost
            groups.append((tuple(names), dom))
        if not groups:
            return self.atom_bool(d)
        msg = any(dm[0] == "d_msgs" for _n, dm in groups)
        self.in_msg_body += msg
        body = self.boolean(d - 1)
        self.in_msg_body -= msg
        del self.scope[len(self.scope) - pushed:]
        self.cost = cost0
        return ("q", q, tuple(groups), body)

    def domain(self, d, dependent=False):
        """-> (domain, the bound name's kind, its info, a size estimate)."""
        svs = self.vars_of("S")
        if dependent and svs:
            last = ("var", svs[-1][0])
            w = self.r.randrange(4)
            if w <= 1:
                ref = ("log", last, self.pp())
                return ("d_log", ref), "I", (ref, self.primed), 2
            if w == 2:
                return ("d_set", ("sv", self.pick(("votesGranted", "votesResponded")), last, self.pp())), "S", "clean", 3
            return ("d_set", ("bin", "\\", ("server_set",), ("setlit", (last,)))), "S", "clean", 4
        c = ["Server"] * 5 + ["set", "quorum", "range", "cap", "dlog", "dlog", "msgs", "msgs", "msgs", "nilset"]
        if self.vars_of("Q"):
            c += ["qvar"] * 2
        k = self.pick(c)
        if self.in_msg_body and k in ("set", "nilset"):
            k = "Server"
        if k == "Server":
            return ("d_set", ("server_set",)), "S", "clean", 4
        if k == "set":
            return ("d_set", self.set(d - 1)), "S", None, 3
        if k == "nilset":
            return ("d_set", ("bin", "\\cup", self.set(1), ("setlit", (("nil",),)))), "S", None, 4
        if k == "qvar":
            qv = self.pick(self.vars_of("Q"))
            return ("d_set", ("var", qv[0])), "S", qv[1], 3
        if k == "quorum":
            return ("d_quorum",), "Q", "clean", 8
        if k == "range":
            return ("d_range", self.integer(1), self.integer(1)), "I", None, 3
        if k == "cap":
            return ("d_cap", self.integer(0), self.integer(1), self.integer(0), self.integer(1)), "I", None, 3
        if k == "dlog":
            ref = ("log", self.server(0, True), self.pp()) if not self.vars_of("L") or self.chance(0.6) else \
                ("var", self.pick(self.vars_of("L"))[0])
            return ("d_log", ref), "I", (ref, self.primed), 2
        bag = self.primed or self.pp()
        return ("d_msgs", bag and not self.primed), "M", bag, 40


def may_err(n, helpers, seen=()):
    """Could evaluating n be an error?  (Syntactic and on the safe side: the bodies of message
    quantifiers call only definitions for which this is False.)"""
    for x in walk(n):
        if x[0] in ("logterm", "logval", "nil", "if") or (x[0] == "sv" and x[1] == "votedFor"):
            return True
        if x[0] == "mf" and FIELDS[x[2]][1] is not None:
            return True
        if x[0] in ("q", "setcomp") and any(d[0] == "d_set" and d[1] != ("server_set",)
                                            for d in ([dm for _n, dm in x[2]] if x[0] == "q" else [("d_set", x[2])])):
            return True
        if x[0] in ("ref", "call") and (x[1] in seen or may_err(helpers[x[1]][3], helpers, seen + (x[1],))):
            return True
    return False


def children(n):
    k = n[0]
    if k in ("not", "d_set", "card", "len", "lastterm", "log", "msgcnt", "mf", "prime", "d_log"):
        return [n[1]]
    if k in ("bin", "in"):
        return [n[2], n[3]]
    if k in ("if", "d_range", "d_cap", "logterm", "logval"):
        return list(n[1:])
    if k == "q":
        return [d for _names, d in n[2]] + [n[3]]
    if k == "setlit":
        return list(n[1])
    if k == "setcomp":
        return [n[2], n[3]]
    if k == "sv":
        return [n[2]]
    if k == "sv2":
        return [n[2], n[3]]
    if k == "call":
        return list(n[2])
    return []


def walk(n):
    """Every node of an AST (domains and log references included; definitions are not entered)."""
    yield n
    for x in children(n):
        for y in walk(x):
            yield y


# ---- grammar productions: what a predicate exercises ----------------------------------------------
BIN_OPS = ("/\\", "\\/", "=>", "<=>", "\\equiv", "=", "/=", "#", "\\subseteq", "\\cup", "\\cap", "\\", "+", "-") + REL
PRODUCTIONS = tuple(
    ["op:" + op for op in BIN_OPS] + ["op:~", "op:\\in", "op:\\notin", "in:set", "in:quorum", "in:range", "in:dlog",
                                      "set:{}", "set:{e}", "set:{Nil}", "set:comp", "set:Server", "card", "cardmsgs",
                                      "len", "lastterm", "logterm", "logval", "sv2:nextIndex", "sv2:matchIndex", "msgcnt"] +
    ["sv:" + v for v in SV] + ["mf:" + f for f in FIELDS] + ["if:" + t for t in ("B", "I", "S", "R", "T", "SET")] +
    ["q:1", "q:2", "q:3", "q:groups2", "q:dependent", "dom:set", "dom:quorum", "dom:range", "dom:cap", "dom:log",
     "dom:msgs", "const", "srv", "num:negative", "call:0", "call:1", "call:2", "call:swapped", "call:capture",
     "call:via", "param:log", "param:set"])
ACTION_PRODUCTIONS = ("prime:variable", "prime:expr", "prime:Name", "prime:Name(args)", "dom:msgs'", "msgcnt'",
                      "dom:log'", "cardmsgs'")


def _binders(n, defs, seen=()):
    """The names a definition's body binds, those of the definitions it refers to included."""
    out = set()
    for x in walk(n):
        if x[0] == "q":
            out |= {nm for names, _d in x[2] for nm in names}
        elif x[0] == "setcomp":
            out.add(x[1])
        elif x[0] in ("ref", "call") and x[1] not in seen:
            out |= _binders(defs[x[1]][3], defs, seen + (x[1],))
    return out


def productions(n, defs, env=None, out=None):
    """The productions of PRODUCTIONS / ACTION_PRODUCTIONS that n uses, definitions entered.
    defs: name -> (params, kinds, type, body).  env: name -> (kind, order of binding)."""
    env = {} if env is None else env
    out = set() if out is None else out
    k = n[0]

    def ty(x):
        kk = x[0]
        if kk in ("num", "const", "card", "cardmsgs", "len", "lastterm", "logterm", "sv2", "msgcnt"):
            return "I"
        if kk in ("srv", "nil"):
            return "S"
        if kk in ("true", "false", "not", "in", "q", "prime"):
            return "B"
        if kk == "role":
            return "R"
        if kk == "mtype":
            return "T"
        if kk in ("server_set", "setlit", "setcomp"):
            return "SET"
        if kk == "bin":
            return "I" if x[1] in "+-" else "SET" if x[1] in ("\\cup", "\\cap", "\\") else "B"
        if kk == "sv":
            return SV[x[1]]
        if kk == "mf":
            return FIELDS[x[2]][0]
        if kk == "if":
            return ty(x[2])
        if kk == "var":
            return {"Q": "SET", "M": "M", "L": "L"}.get(env[x[1]][0], env[x[1]][0])
        if kk in ("ref", "call"):
            return defs[x[1]][2]
        raise AssertionError(kk)

    def sub(x, e=env):
        productions(x, defs, e, out)

    def bind(e, names, kind):
        e = dict(e)
        for nm in names:
            e[nm] = (kind, len(e))
        return e

    def dom(d, e):
        """-> the kind of the name bound in d; the domain's own productions."""
        if d[0] == "d_set":
            sub(d[1], e)
            out.add("dom:set")
            return "S"
        if d[0] == "d_quorum":
            out.add("dom:quorum")
            return "Q"
        if d[0] in ("d_range", "d_cap"):
            for x in d[1:]:
                sub(x, e)
            out.add("dom:range" if d[0] == "d_range" else "dom:cap")
            return "I"
        if d[0] == "d_log":
            sub(d[1], e)
            out.add("dom:log")
            if d[1][0] == "log" and d[1][2]:
                out.add("dom:log'")
            return "I"
        out.add("dom:msgs")
        if d[1]:
            out.add("dom:msgs'")
        return "M"

    if k == "bin":
        out.add("op:" + n[1])
        sub(n[2]), sub(n[3])
    elif k == "not":
        out.add("op:~")
        sub(n[1])
    elif k == "in":
        out.add("op:" + n[1])
        out.add({"d_set": "in:set", "d_quorum": "in:quorum", "d_range": "in:range", "d_log": "in:dlog"}[n[3][0]])
        sub(n[2])
        for x in n[3][1:]:
            sub(x)
    elif k == "if":
        out.add("if:" + ty(n))
        sub(n[1]), sub(n[2]), sub(n[3])
    elif k == "q":
        e = env
        out.add("q:%d" % max(len(names) for names, _d in n[2]))
        if len(n[2]) >= 2:
            out.add("q:groups2")
            first = set(n[2][0][0])
            if any(x[0] == "var" and x[1] in first for _names, d in n[2][1:] for x in walk(d)):
                out.add("q:dependent")
        for names, d in n[2]:
            e = bind(e, names, dom(d, e))
        sub(n[3], e)
    elif k == "setlit":
        out.add("set:{}" if not n[1] else "set:{e}")
        if any(x == ("nil",) for x in n[1]):
            out.add("set:{Nil}")
        for x in n[1]:
            sub(x)
    elif k == "setcomp":
        out.add("set:comp")
        sub(n[2])
        sub(n[3], bind(env, [n[1]], "S"))
    elif k == "server_set":
        out.add("set:Server")
    elif k in ("card", "len", "lastterm", "logterm", "logval"):
        out.add(k)
        for x in n[1:]:
            sub(x)
    elif k == "log":
        if n[2]:
            out.add("prime:variable")
        sub(n[1])
    elif k == "cardmsgs":
        out.add("cardmsgs")
        if n[1]:
            out.add("cardmsgs'")
    elif k == "sv":
        out.add("sv:" + n[1])
        if n[3]:
            out.add("prime:variable")
        sub(n[2])
    elif k == "sv2":
        out.add("sv2:" + n[1])
        if n[4]:
            out.add("prime:variable")
        sub(n[2]), sub(n[3])
    elif k == "msgcnt":
        out.add("msgcnt")
        if n[2]:
            out.add("msgcnt'")
    elif k == "mf":
        out.add("mf:" + n[2])
    elif k == "const":
        out.add("const")
    elif k == "srv":
        out.add("srv")
    elif k == "num" and n[1] < 0:
        out.add("num:negative")
    elif k in ("ref", "call"):
        params, kinds, _t, body = defs[n[1]]
        args = n[2] if k == "call" else ()
        out.add("call:%d" % len(args))
        if "L" in kinds:
            out.add("param:log")
        if "SET" in kinds:
            out.add("param:set")
        if any(x[0] in ("ref", "call") for x in walk(body)):
            out.add("call:via")
        vs = [a[1] for a in args if a[0] == "var" and a[1] in env]
        if len(args) == 2 and len(vs) == 2 and env[vs[0]][1] > env[vs[1]][1]:
            out.add("call:swapped")
        if set(vs) & _binders(body, defs):
            out.add("call:capture")
        for a in args:
            sub(a)
        kind = {"S": "S", "I": "I", "SET": "Q", "L": "L"}
        productions(body, defs, {p: (kind[kd], t) for t, (p, kd) in enumerate(zip(params, kinds))}, out)
    elif k == "prime":
        out.add({"ref": "prime:Name", "call": "prime:Name(args)"}.get(n[1][0], "prime:expr"))
        sub(n[1])
    return out


def names_server(n, defs):
    return "srv" in productions(n, defs)


def reads_state(n, defs):
    return any(p.split(":")[0] in ("sv", "sv2", "mf", "msgcnt", "cardmsgs", "len", "lastterm", "logterm", "logval",
                                   "dom") and p not in ("dom:set", "dom:range", "dom:cap", "dom:quorum")
               for p in productions(n, defs))


# ---- programs: definitions and predicates, as text ----------------------------------------------
class Program:
    """helpers: name -> (params, kinds, type, body); preds: [(name, body)]; action: [][A]_vars."""

    def __init__(self, helpers, preds, action):
        self.helpers, self.preds, self.action = helpers, preds, action
        self.names = tuple(nm for nm, _b in preds)
        self.defs = {nm: (h[0], h[3]) for nm, h in helpers.items()}

    def definitions(self, minimal):
        out = [definition_text(nm, h[0], h[3], minimal) for nm, h in sorted(self.helpers.items())]
        out += [definition_text(nm, (), b, minimal, self.action) for nm, b in self.preds]
        return "\n\n".join(out)

    @functools.lru_cache(maxsize=None)
    def compiled(self):
        return tuple(compile_predicate(self.defs, b) for _nm, b in self.preds)

    def productions(self, p):
        return productions(self.preds[p][1], self.helpers)

    def verdicts(self, n_servers, states):
        """Per state (or pair, for an action program): a tuple of Evaluated, one per predicate."""
        fns = self.compiled()
        if self.action:
            return [tuple(evaluate(f, n_servers, s, t) for f in fns) for s, t in states]
        return [tuple(evaluate(f, n_servers, s) for f in fns) for s in states]


PARAM_KINDS_1 = (("S",), ("S",), ("L",), ("SET",), ("I",))
PARAM_KINDS_2 = (("S", "S"), ("S", "S"), ("S", "S"), ("S", "I"), ("L", "I"), ("SET", "S"), ("L", "S"))
SCOPE_KIND = {"S": "S", "I": "I", "SET": "Q", "L": "L"}


def make_helpers(rng, tag):
    """Two or three definitions: one without parameters, one with one, one with two that may refer
    to the others.  Their bodies bind names from `i` on, as the predicates that call them do."""
    helpers = {}
    for kinds in ((), PARAM_KINDS_1[rng.randrange(len(PARAM_KINDS_1))], PARAM_KINDS_2[rng.randrange(len(PARAM_KINDS_2))]):
        if len(kinds) == 0 and rng.random() < 0.3:
            continue
        g = Gen(rng, dict(helpers) if len(kinds) == 2 else {})
        g.max_bind = 1
        params = ("x", "y")[:len(kinds)]
        g.scope = [(p, SCOPE_KIND[kd], None) for p, kd in zip(params, kinds)]
        ty = g.pick(("B", "B", "B", "I", "SET"))
        for _ in range(50):
            body = g.quant(3) if ty == "B" and (not kinds or g.chance(0.6)) else \
                {"B": g.boolean, "I": g.integer, "SET": g.set}[ty](3)
            if len(kinds) == 2 and ty == "B" and g.chance(0.6):  # through another definition
                t2 = g.pick([h[2] for h in helpers.values()])
                other = g.call(t2, 2)
                body = ("bin", g.pick(("/\\", "\\/", "=>")), body, other if t2 == "B" else ("bin", "=", other, other))
            used = {x[1] for x in walk(body) if x[0] == "var"}
            if set(params) <= used and (ty != "B" or body[0] != "true"):
                break
        helpers["H%s%s" % (tag, "abc"[len(kinds)])] = (params, kinds, ty, body)
    return helpers


def deep_sum(k):
    """\\A i \\in Server : currentTerm[i] <= 1 - (1 - (... - Len(log[i]))): k operands on the right,
    nested to the right, so the evaluation stack holds 1 + k values at its deepest."""
    e = ("len", ("log", ("var", "i"), False))
    for _ in range(k - 1):
        e = ("bin", "-", ("num", 1), e)
    return ("q", "\\A", ((("i",), ("d_set", ("server_set",))),), ("bin", "<=", ("sv", "currentTerm", ("var", "i"), False), e))


def deep_scope(k):
    """k bound names in scope at once, each domain a singleton (or empty) built from the name before."""
    names = (BOUND_NAMES + ("z",))[:k]
    body = ("bin", "=", ("var", names[0]), ("var", names[-1]))
    for t in range(k - 1, 0, -1):
        prev = ("var", names[t - 1])
        d = ("d_set", ("setlit", (prev,))) if t % 2 else \
            ("d_set", ("bin", "\\", ("setlit", (prev, ("nil",))), ("setlit", (("nil",),))))
        body = ("q", "\\A" if t % 3 else "\\E", (((names[t],), d),), body) if t % 4 else \
            ("bin", "=", ("card", ("setcomp", names[t], d[1], body)), ("num", 1))
    return ("q", "\\A", (((names[0],), ("d_set", ("server_set",))),), body)


N_INV_PROGRAMS, N_ACT_PROGRAMS = 16, 16
INV_SEED, ACT_SEED = 41000, 52000


def _sample_states():
    from tests import invariant_cases as IC
    out = []
    for name in ("fuzz0", "edge1", "fuzz2"):
        m, _ = IC.CASES[name]
        st = IC.states(name)
        out.append((m.n_servers, st[:25] + st[IC.N_PER_FAMILY:IC.N_PER_FAMILY + 25]))
    return out


def _sample_pairs():
    from tests import action_cases as AC
    from tests import invariant_cases as IC
    out = []
    for name, K in (("fuzz0", 4), ("edge1", 8), ("fuzz2", 4)):
        ps = AC.pairs(name, K)
        out.append((IC.CASES[name][0].n_servers, ps[::max(1, len(ps) // 60)]))
    return out


def _varies(fn, samples, action):
    """Two verdicts over the sample, and seldom dependent on the bag's order."""
    seen, od, n = set(), 0, 0
    for S, items in samples:
        for it in items:
            ev = evaluate(fn, S, *it) if action else evaluate(fn, S, it)
            seen.add(ev.verdict)
            od += ev.order_dependent
            n += 1
    return len(seen) >= 2 and od * 50 <= n


@functools.lru_cache(maxsize=None)
def pool(kind):
    """The pool from its fixed seeds: kind "inv", 16 programs of 8 invariants; "act", 16 programs of
    4 action properties.  For each place twelve candidates are generated; they are tried in the order of
    how many productions they add that fewer than four predicates have so far, and the first one
    that shows two verdicts on a small sample is taken."""
    action = kind == "act"
    samples = _sample_pairs() if action else _sample_states()
    count = {}
    programs = []
    for p in range(N_ACT_PROGRAMS if action else N_INV_PROGRAMS):
        rng = random.Random((ACT_SEED if action else INV_SEED) + p)
        tag = "%s%d" % ("A" if action else "I", p)
        helpers = make_helpers(rng, tag)
        defs = {nm: (h[0], h[3]) for nm, h in helpers.items()}
        preds = []
        fixed = {}
        if not action and p == 0:  # the limits, met exactly: stack depth 16, 8 names in scope
            fixed = {0: deep_sum(15), 1: deep_scope(8)}
        for q in range(4 if action else 8):
            name = "G%s_%d" % (tag, q)
            body = fixed.get(q)
            for _round in range(60):
                if body is not None:
                    break
                cands = []
                for _c in range(12):
                    g = Gen(random.Random(rng.random()), helpers, action=action, closed=(q % 4 == 3))
                    b = g.msg_pred(4) if q % 4 in (1, 2) and g.chance(0.7) else g.quant(4) if g.chance(0.8) else g.boolean(4)
                    if g.closed and names_server(b, helpers):
                        continue
                    tags = productions(b, helpers)
                    cands.append((-sum(max(0, 4 - count.get(t, 0)) for t in tags), len(cands), b))
                for _score, _k, b in sorted(cands):
                    if _varies(compile_predicate(defs, b), samples, action):
                        body = b
                        break
            assert body is not None, "no varying predicate for " + name
            for t in productions(body, helpers):
                count[t] = count.get(t, 0) + 1
            preds.append((name, body))
        programs.append(Program(helpers, preds, action))
    return tuple(programs)


def program(kind, p):
    return pool(kind)[p]


def module_text(prog, minimal):
    from tests import action_cases as AC
    from tests import predicate_cases as PC
    if prog.action:
        return AC.module_with(prog.definitions(minimal))
    return PC.module_with(prog.definitions(minimal))


# ---- the cases: states, pairs, the evaluator's verdicts (cached; shared by the host and device tests)
N_STATES = 200


@functools.lru_cache(maxsize=None)
def states(name):
    """200 states of a model of invariant_cases: the first 100 of each family."""
    from tests import invariant_cases as IC
    st = IC.states(name)
    h = N_STATES // 2
    return st[:h] + st[IC.N_PER_FAMILY:IC.N_PER_FAMILY + h]


@functools.lru_cache(maxsize=None)
def pairs(name, K):
    """action_cases.pairs(name, K), then a stuttering pair (s, s) per source."""
    from tests import action_cases as AC
    ps = AC.pairs(name, K)
    src = []
    for s, _t in ps:
        if not src or src[-1] != s:
            src.append(s)
    return ps + tuple((s, s) for s in src)


@functools.lru_cache(maxsize=None)
def inv_verdicts(p, name):
    from tests import invariant_cases as IC
    return tuple(program("inv", p).verdicts(IC.CASES[name][0].n_servers, states(name)))


@functools.lru_cache(maxsize=None)
def act_verdicts(p, name, K):
    from tests import invariant_cases as IC
    return tuple(program("act", p).verdicts(IC.CASES[name][0].n_servers, pairs(name, K)))


def write_program(dirpath, prog, model, minimal, names=None):
    """The program's module and a cfg that names its predicates; -> (cfg path, tla path)."""
    from tests import action_cases as AC
    from tests import predicate_cases as PC
    names = prog.names if names is None else names
    if prog.action:
        return AC.write_model(dirpath, names, n_servers=model.n_servers, n_values=model.n_values,
                              module=module_text(prog, minimal))
    return PC.write_model(dirpath, names, n_servers=model.n_servers, n_values=model.n_values,
                          module=module_text(prog, minimal))


# ---- the reachable graph of a small model: which pool predicates the BFS passes can be tested with --
@functools.lru_cache(maxsize=None)
def reachable_levels():
    """graph_cases.TINY2 by the oracle: per level (Init = level 1) its states, each with its
    transitions (s, t) to successors inside the CONSTRAINT (stuttering ones included)."""
    from tests import graph_cases as G
    p = G.TINY2
    model = R.Model(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"], max_log=p["max_log_len"],
                    max_msgs=p["max_msgs"], max_dup=p["max_dup"])
    assert (p["max_term"], p["max_log_len"], p["max_msgs"], p["max_dup"]) == tuple(
        CONSTS[k] for k in ("MaxTerm", "MaxLogLen", "MaxMsgs", "MaxDup"))
    s0 = R.init_state(model)
    seen, frontier, levels = {s0}, [s0], []
    while frontier:
        steps, nxt = [], []
        for s in frontier:
            for _f, _p, t in R.successors(model, s):
                if R.in_constraint(model, t):
                    steps.append((s, t))
                    if t not in seen:
                        seen.add(t)
                        nxt.append(t)
        levels.append((tuple(frontier), tuple(steps)))
        frontier = nxt
    return model, tuple(levels)


@functools.lru_cache(maxsize=None)
def first_failing(kind, p, q):
    """The oracle's BFS with pool predicate q of program p: (depth, verdicts) of the first level with a
    state (depth = the level), or a transition out of it (depth = the level + 1), that does not get
    HOLDS -- verdicts: the set of the verdicts that are not HOLDS there; (None, ()) if there is none;
    ("order", ()) if a case on the way depends on the bag's order (such a predicate is not chosen)."""
    model, levels = reachable_levels()
    prog = program(kind, p)
    fn = prog.compiled()[q]
    for lv, (sts, steps) in enumerate(levels, 1):
        evs = [evaluate(fn, model.n_servers, s, t) for s, t in steps] if prog.action else \
            [evaluate(fn, model.n_servers, s) for s in sts]
        if any(ev.order_dependent for ev in evs):
            return "order", ()
        bad = frozenset(ev.verdict for ev in evs if ev.verdict != HOLDS)
        if bad:
            return lv + (1 if prog.action else 0), bad
    return None, ()


@functools.lru_cache(maxsize=None)
def bfs_cases(kind, want=4):
    """Up to `want` pool predicates for the BFS passes, from the evaluator over the oracle's graph
    alone: ((program, predicate, depth, verdicts, holders), ...) -- the first level without HOLDS is
    3 or later, `holders` are the predicates of the same program that hold on every reachable state
    (or transition), at least one; the first case ends in an error on every failing state of its level.
    The programs are scanned in order until there is an error case and `want` cases in all."""
    err, other = [], []
    for p in range(N_ACT_PROGRAMS if kind == "act" else N_INV_PROGRAMS):
        n = len(program(kind, p).preds)
        ff = [first_failing(kind, p, q) for q in range(n)]
        holders = tuple(q for q in range(n) if ff[q][0] is None)
        if not holders:
            continue
        for q in range(n):
            d, vs = ff[q]
            if isinstance(d, int) and d >= 3:
                (err if vs == {ERROR} else other).append((p, q, d, vs, holders))
        if err and len(err) + len(other) >= want:
            break
    return tuple(err[:1] + (other + err[1:])[:want - 1])
