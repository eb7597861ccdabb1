"""Inputs of the action property tests (test_actions.py on the GPU, test_actions_native.py on
the host): the properties [][A]_vars as TLA+ text, each A with a Python twin over pairs of
oracle.raft_spec states, the model files that carry them, and the pairs (s, t) they are
evaluated on.  A twin returns A's verdict on (s, t): 0 it holds, 1 it is violated, 2
evaluating it is an error; `expected` applies the stutter rule of [A]_vars (violated on t = s
is holds).  Everything expected here comes from oracle/raft_spec.py; nothing is read from the
engine.  Test infrastructure only."""
import functools
import os

from oracle import raft_spec as R
from tests import invariant_cases as IC
from tests import predicate_cases as PC

HOLDS, VIOLATED, ERROR = 0, 1, 2

DEFINITIONS = r"""
NoLeader == \A i \in Server : state[i] /= Leader
Granted(i) == votesGranted[i]
LogSize(i) == Len(log[i]) + commitIndex[i]

ATermsMonotonic == \A i \in Server : currentTerm'[i] >= currentTerm[i]
TermsMonotonic == [][ATermsMonotonic]_vars

ACommitMonotonic == \A i \in Server : commitIndex'[i] >= commitIndex[i]
CommitMonotonic == [][ACommitMonotonic]_vars

LeaderAppendOnly == [][
    \A i \in Server :
        (state[i] = Leader /\ state'[i] = Leader /\ currentTerm'[i] = currentTerm[i])
        => /\ Len(log'[i]) >= Len(log[i])
           /\ \A n \in DOMAIN log[i] : /\ log'[i][n].term = log[i][n].term
                                       /\ log'[i][n].value = log[i][n].value
    ]_vars

VoteOncePerTerm == [][
    \A i \in Server :
        (currentTerm'[i] = currentTerm[i] /\ votedFor[i] /= Nil) => votedFor'[i] = votedFor[i]
    ]_vars

MsgsGrowByOne == [][Cardinality(DOMAIN messages') <= Cardinality(DOMAIN messages) + 1]_vars

NewMsgTerms == [][\A m \in DOMAIN messages' : m.mterm <= currentTerm'[m.msource] /\ messages'[m] >= 1]_vars

NoLeaderKept == [][NoLeader => NoLeader']_vars

PrimedForms == [][
    \A i \in Server : /\ currentTerm'[i] = currentTerm[i] => Granted(i) \subseteq Granted(i)'
                      /\ (Len(log[i]) + commitIndex[i])' = LogSize(i)'
                      /\ matchIndex'[i][i] + 1 <= nextIndex'[i][i] + LastTerm(log'[i]) + 4
    ]_vars

UnguardedNext == [][\A i \in Server : log'[i][1].term >= 0]_vars

AlwaysFalse == [][FALSE]_vars

NamesR1 == [][state'[r1] /= Leader \/ state[r1] = Leader]_vars

CandStays == [][\A i \in Server : state[i] = Candidate => state'[i] /= Follower]_vars
"""

MODULE = PC.module_with(DEFINITIONS).replace("PredCases", "ActCases")


def _terms(model, s, t):
    return all(t.currentTerm[i] >= s.currentTerm[i] for i in model.servers)


def _commit(model, s, t):
    return all(t.commitIndex[i] >= s.commitIndex[i] for i in model.servers)


def _leader_append(model, s, t):
    for i in model.servers:
        if s.state[i] == R.LEADER and t.state[i] == R.LEADER and t.currentTerm[i] == s.currentTerm[i]:
            if len(t.log[i]) < len(s.log[i]) or tuple(t.log[i][:len(s.log[i])]) != tuple(s.log[i]):
                return False
    return True


def _vote_once(model, s, t):
    return all(not (t.currentTerm[i] == s.currentTerm[i] and s.votedFor[i] != R.NIL) or t.votedFor[i] == s.votedFor[i]
               for i in model.servers)


def _grow(model, s, t):
    return len(t.messages) <= len(s.messages) + 1


def _new_msg_terms(model, s, t):
    return all(R.rget(m, "mterm") <= t.currentTerm[R.rget(m, "msource")] and c >= 1 for m, c in t.messages)


def _no_leader(s):
    return all(r != R.LEADER for r in s.state)


def _no_leader_kept(model, s, t):
    return not _no_leader(s) or _no_leader(t)


def _primed_forms(model, s, t):
    for i in model.servers:
        if t.currentTerm[i] == s.currentTerm[i] and not s.votesGranted[i] <= t.votesGranted[i]:
            return False
        if not t.matchIndex[i][i] + 1 <= t.nextIndex[i][i] + R.last_term(t.log[i]) + 4:
            return False
    return True


def _cand_stays(model, s, t):
    return all(not (s.state[i] == R.CANDIDATE and t.state[i] == R.FOLLOWER) for i in model.servers)


def _bool(f):
    return lambda model, s, t: HOLDS if f(model, s, t) else VIOLATED


# name -> twin(model, s, t) -> A's verdict
TWINS = {
    "TermsMonotonic": _bool(_terms),
    "CommitMonotonic": _bool(_commit),
    "LeaderAppendOnly": _bool(_leader_append),
    "VoteOncePerTerm": _bool(_vote_once),
    "MsgsGrowByOne": _bool(_grow),
    "NewMsgTerms": _bool(_new_msg_terms),
    "NoLeaderKept": _bool(_no_leader_kept),
    "PrimedForms": _bool(_primed_forms),
    # log'[i][1] of an empty successor log is outside its domain; a term is never negative
    "UnguardedNext": lambda model, s, t: ERROR if any(len(lg) == 0 for lg in t.log) else HOLDS,
    "AlwaysFalse": lambda model, s, t: VIOLATED,
    "NamesR1": _bool(lambda model, s, t: t.state[0] != R.LEADER or s.state[0] == R.LEADER),
    "CandStays": _bool(_cand_stays),
}
# The verdicts each twin can produce on transitions of raft.tla's Next.  The first five hold on
# every step of Next (they are theorems of raft.tla's actions); AlwaysFalse is constant.
ALWAYS_HOLD = ("TermsMonotonic", "LeaderAppendOnly", "VoteOncePerTerm", "MsgsGrowByOne")
CONSTANT_FALSE = ("AlwaysFalse",)
CAN_PRODUCE = {"CommitMonotonic": {HOLDS, VIOLATED}, "NewMsgTerms": {HOLDS, VIOLATED},
               "NoLeaderKept": {HOLDS, VIOLATED}, "PrimedForms": {HOLDS, VIOLATED},
               "UnguardedNext": {HOLDS, ERROR}, "NamesR1": {HOLDS, VIOLATED}, "CandStays": {HOLDS, VIOLATED}}
# at most RMC_MAX_ACTION_PROPS = 4 per program: three groups cover the twelve
GROUPS = {"a": ("TermsMonotonic", "CommitMonotonic", "LeaderAppendOnly", "VoteOncePerTerm"),
          "b": ("MsgsGrowByOne", "NewMsgTerms", "NoLeaderKept", "PrimedForms"),
          "c": ("UnguardedNext", "AlwaysFalse", "NamesR1", "CandStays")}


def expected(name, model, s, t):
    """[A]_vars on (s, t): A's verdict, "violated" on a stuttering step being "holds"."""
    v = TWINS[name](model, s, t)
    return HOLDS if v == VIOLATED and s == t else v


def write_model(dirpath, properties, n_servers=3, n_values=2, max_term=2, max_log=1, max_msgs=2, max_dup=1,
                symmetry=False, module=MODULE, name="ActCases", invariants=(), extra=""):
    """Writes <dirpath>/<name>.tla and .cfg; returns (cfg path, tla path)."""
    tla, cfg = os.path.join(str(dirpath), name + ".tla"), os.path.join(str(dirpath), name + ".cfg")
    with open(tla, "w") as f:
        f.write(module)
    with open(cfg, "w") as f:
        f.write(PC.cfg_text(n_servers, n_values, max_term, max_log, max_msgs, max_dup, invariants, symmetry,
                            extra="".join("PROPERTY %s\n" % p for p in properties) + extra))
    return cfg, tla


def module_with(definitions):
    """MODULE with more definitions before its end (the refusal tests)."""
    end = MODULE.rindex("ServerSymmetry ==")
    return MODULE[:end] + definitions + "\n\n" + MODULE[end:]


# (model of invariant_cases, bag slots K of the ctx): test_predicates.SHAPES, every packed shape
SHAPES = [("fuzz2", 4), ("fuzz2", 8), ("fuzz0", 4), ("fuzz1", 8), ("edge0", 8), ("fuzz3", 4), ("edge3", 8),
          ("fuzz4", 4), ("fuzz4", 8), ("edge1", 8)]
N_SOURCES = 40


@functools.lru_cache(maxsize=None)
def pairs(name, K):
    """Every transition (s, t) of Next out of the first N_SOURCES states of the case with at most K
    messages, whose successor satisfies the CONSTRAINT and has at most K messages."""
    m, _ = IC.CASES[name]
    src = [s for s in IC.states(name) if len(s.messages) <= K][:N_SOURCES]
    return tuple((s, t) for s in src for _f, _p, t in R.successors(m, s)
                 if R.in_constraint(m, t) and len(t.messages) <= K)


@functools.lru_cache(maxsize=None)
def verdicts(name, K, group):
    m, _ = IC.CASES[name]
    return tuple(tuple(expected(p, m, s, t) for p in GROUPS[group]) for s, t in pairs(name, K))


def _check_pairs():
    seen = {p: set() for p in TWINS}
    for name, K in SHAPES:
        m, _ = IC.CASES[name]
        ps = pairs(name, K)
        assert len(ps) >= 250, (name, K, len(ps))
        assert sum(1 for s, t in ps if s == t) >= 20, (name, K)
        for p in TWINS:
            seen[p] |= {TWINS[p](m, s, t) for s, t in ps}
    for p in ALWAYS_HOLD:
        assert seen[p] == {HOLDS}, (p, seen[p])
    for p, can in CAN_PRODUCE.items():
        assert seen[p] == can, (p, seen[p])
    assert set(ALWAYS_HOLD) | set(CONSTANT_FALSE) | set(CAN_PRODUCE) == set(TWINS)


_check_pairs()


def oracle_violation(model, name, symmetry=False, max_levels=None):
    """The oracle's BFS, level by level: the least level (Init = 1) with a state s that has a
    transition to an in-CONSTRAINT t on which [A]_vars of `name` does not hold, as (level + 1);
    None if the search ends (or passes max_levels) without one."""
    key = (lambda t: R.canonical(model, t)) if symmetry else (lambda t: t)
    s0 = R.init_state(model)
    seen, frontier, depth = {key(s0)}, [s0], 1
    while frontier:
        nxt, bad = [], False
        for s in frontier:
            for _f, _p, t in R.successors(model, s):
                if R.in_constraint(model, t):
                    bad = bad or expected(name, model, s, t) != HOLDS
                    k = key(t)
                    if k not in seen:
                        seen.add(k)
                        nxt.append(t)
        if bad:
            return depth + 1
        if max_levels is not None and depth >= max_levels:
            return None
        frontier = nxt
        depth += 1
    return None
