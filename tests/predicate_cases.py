"""Inputs of the model-defined invariant tests (test_predicates.py on the GPU,
test_predicates_native.py on the host): the predicates as TLA+ text, each with a
Python twin over oracle.raft_spec states, and the model files that carry them.
A twin returns the interpreter's verdict: 0 the predicate holds, 1 it is violated,
2 evaluating it is an error (a read outside a domain, as in TLC).  Everything
expected here comes from oracle/raft_spec.py; nothing is read from the engine.
Test infrastructure only."""
import functools
import os

from oracle import raft_spec as R

HOLDS, VIOLATED, ERROR = 0, 1, 2

# The module: raft.tla's variables, the bounds of specs/MCraftBounded.tla, then the
# predicates.  The first three are the texts of OneLeaderPerTerm, LeaderVotesQuorum and
# CandidateTermNotInLog of specs/MCraftBounded.tla under new names.
MODULE = r"""---------------------------- MODULE PredCases ----------------------------
EXTENDS raft, FiniteSets, TLC

CONSTANTS r1, r2, r3, r4, r5, v1, v2
CONSTANTS MaxTerm, MaxLogLen, MaxMsgs, MaxDup

Servers2 == {r1, r2}
Servers3 == {r1, r2, r3}
Servers4 == {r1, r2, r3, r4}
Servers5 == {r1, r2, r3, r4, r5}
Values1 == {v1}
Values2 == {v1, v2}

StateConstraint ==
    /\ \A i \in Server : currentTerm[i] <= MaxTerm /\ Len(log[i]) <= MaxLogLen
    /\ Cardinality(DOMAIN messages) <= MaxMsgs
    /\ \A m \in DOMAIN messages : messages[m] <= MaxDup

UserOneLeader ==
    \A i, j \in Server :
        (state[i] = Leader /\ state[j] = Leader /\ currentTerm[i] = currentTerm[j]) => i = j

UserLeaderVotes ==
    \A i \in Server : state[i] = Leader =>
        {j \in Server : \/ currentTerm[j] > currentTerm[i]
                        \/ currentTerm[j] = currentTerm[i] /\ votedFor[j] = i} \in Quorum

UserCandTerm ==
    \A i \in Server :
        (/\ state[i] = Candidate
         /\ {j \in Server : currentTerm[j] = currentTerm[i] /\ votedFor[j] \in {i, Nil}} \in Quorum)
        => \A j \in Server : \A n \in DOMAIN log[j] : log[j][n].term /= currentTerm[i]

UserMsgTerms ==
    \A m \in DOMAIN messages : m.mterm <= currentTerm[m.msource] /\ messages[m] >= 1

UserQuorumCommit ==
    \A Q \in Quorum : \E j \in Q : commitIndex[j] <= Len(log[j])

UserNoLeader ==
    \A i \in Server : state[i] /= Leader

Behind(i, j) == matchIndex[i][j] + 1 <= nextIndex[i][j]
Granted(i) == votesGranted[i]

UserMixed ==
    \A i \in Server :
        IF state[i] = Leader
        THEN \A j \in Server : Behind(i, j)
        ELSE /\ Granted(i) \subseteq votesResponded[i]
             /\ Cardinality(Granted(i)) + 1 <= Cardinality(Server) + 1

UserGuardedLog ==
    \A i \in Server : \A n \in DOMAIN log[i] : log[i][n].term <= currentTerm[i]

UserUnguardedLog ==
    \A i \in Server : log[i][1].term >= 0

UserWrongField ==
    \A m \in DOMAIN messages : m.mvoteGranted => TRUE

UserEntryMatch ==
    \A i, j \in Server :
        \A n \in (1..Len(log[i])) \cap (1..Len(log[j])) :
            log[i][n].term = log[j][n].term => log[i][n].value = log[j][n].value

UserOps ==
    \A i \in Server :
        /\ (votedFor[i] \notin ((Server \ {i}) \cup {Nil})) <=> (votedFor[i] = i)
        /\ \E j \in Server : \/ LastTerm(log[j]) - currentTerm[i] <= 0
                             \/ commitIndex[j] \in 1..2
        /\ \/ (votesGranted[i] \cap votesResponded[i]) # {}
           \/ state[i] # Leader
           \/ i \in votesGranted[i]

UserNamesServer ==
    state[r1] /= Leader \/ votedFor[r1] = Nil

ServerSymmetry == Permutations(Server)
=============================================================================
"""


def _msgs(s):
    return [m for m, _c in s.messages]


def _user_msg_terms(model, s):
    return all(R.rget(m, "mterm") <= s.currentTerm[R.rget(m, "msource")] and c >= 1 for m, c in s.messages)


def _quorums(model):
    S = model.n_servers
    return [[j for j in range(S) if mask >> j & 1] for mask in range(1 << S) if 2 * bin(mask).count("1") > S]


def _user_quorum_commit(model, s):
    return all(any(s.commitIndex[j] <= len(s.log[j]) for j in q) for q in _quorums(model))


def _user_no_leader(model, s):
    return all(r != R.LEADER for r in s.state)


def _user_mixed(model, s):
    S = model.n_servers
    for i in range(S):
        if s.state[i] == R.LEADER:
            if not all(s.matchIndex[i][j] + 1 <= s.nextIndex[i][j] for j in range(S)):
                return False
        elif not (s.votesGranted[i] <= s.votesResponded[i] and len(s.votesGranted[i]) + 1 <= S + 1):
            return False
    return True


def _user_guarded_log(model, s):
    return all(R.rget(e, "term") <= s.currentTerm[i] for i in range(model.n_servers) for e in s.log[i])


def _user_entry_match(model, s):
    S = model.n_servers
    return all(R.rget(a, "term") != R.rget(b, "term") or R.rget(a, "value") == R.rget(b, "value")
               for i in range(S) for j in range(S) for a, b in zip(s.log[i], s.log[j]))


def _user_ops(model, s):
    S = model.n_servers
    for i in range(S):
        others_or_nil = (set(range(S)) - {i}) | {R.NIL}
        if (s.votedFor[i] not in others_or_nil) != (s.votedFor[i] == i):
            return False
        if not any(R.last_term(s.log[j]) - s.currentTerm[i] <= 0 or s.commitIndex[j] in (1, 2) for j in range(S)):
            return False
        if not (s.votesGranted[i] & s.votesResponded[i] or s.state[i] != R.LEADER or i in s.votesGranted[i]):
            return False
    return True


def _bool(f):
    return lambda model, s: HOLDS if f(model, s) else VIOLATED


# name -> twin(model, state) -> verdict
TWINS = {
    "UserOneLeader": _bool(R.INVARIANTS["OneLeaderPerTerm"]),
    "UserLeaderVotes": _bool(R.INVARIANTS["LeaderVotesQuorum"]),
    "UserCandTerm": _bool(R.INVARIANTS["CandidateTermNotInLog"]),
    "UserMsgTerms": _bool(_user_msg_terms),
    "UserQuorumCommit": _bool(_user_quorum_commit),
    "UserNoLeader": _bool(_user_no_leader),
    "UserMixed": _bool(_user_mixed),
    "UserGuardedLog": _bool(_user_guarded_log),
    "UserEntryMatch": _bool(_user_entry_match),
    "UserOps": _bool(_user_ops),
    # log[i][1] of an empty log is outside its domain; an entry's term is never negative
    "UserUnguardedLog": lambda model, s: ERROR if any(len(lg) == 0 for lg in s.log) else HOLDS,
    # m.mvoteGranted of a message that is no RequestVoteResponse: no such field
    "UserWrongField": lambda model, s: ERROR if any(R.rget(m, "mtype") != R.RVP for m in _msgs(s)) else HOLDS,
}
# the restated built-ins and the bit of the compiled-in check they must equal
RESTATED = {"UserOneLeader": 2, "UserLeaderVotes": 16, "UserCandTerm": 32}
# at most RMC_MAX_PREDICATES = 8 per program: two groups cover the twelve
GROUPS = {"a": ("UserOneLeader", "UserLeaderVotes", "UserCandTerm", "UserMsgTerms", "UserQuorumCommit",
                "UserNoLeader"),
          "b": ("UserMixed", "UserGuardedLog", "UserUnguardedLog", "UserWrongField", "UserEntryMatch", "UserOps")}


def cfg_text(n_servers, n_values, max_term, max_log, max_msgs, max_dup, invariants, symmetry=False, extra=""):
    mv = "\n".join("    %s = %s" % (x, x) for x in (
        "r1", "r2", "r3", "r4", "r5", "v1", "v2", "Follower", "Candidate", "Leader", "Nil", "RequestVoteRequest",
        "RequestVoteResponse", "AppendEntriesRequest", "AppendEntriesResponse"))
    return ("CONSTANTS\n%s\n    Server <- Servers%d\n    Value <- Values%d\n    MaxTerm = %d\n    MaxLogLen = %d\n"
            "    MaxMsgs = %d\n    MaxDup = %d\nSPECIFICATION Spec\nCONSTRAINT StateConstraint\n%s%s%s"
            % (mv, n_servers, n_values, max_term, max_log, max_msgs, max_dup,
               "SYMMETRY ServerSymmetry\n" if symmetry else "",
               "".join("INVARIANT %s\n" % i for i in invariants), extra))


def write_model(dirpath, invariants, n_servers=3, n_values=2, max_term=2, max_log=1, max_msgs=2, max_dup=1,
                symmetry=False, module=MODULE, name="PredCases"):
    """Writes <dirpath>/<name>.tla and .cfg; returns (cfg path, tla path)."""
    tla, cfg = os.path.join(str(dirpath), name + ".tla"), os.path.join(str(dirpath), name + ".cfg")
    with open(tla, "w") as f:
        f.write(module)
    with open(cfg, "w") as f:
        f.write(cfg_text(n_servers, n_values, max_term, max_log, max_msgs, max_dup, invariants, symmetry))
    return cfg, tla


def module_with(definitions, name="PredCases"):
    """MODULE with more definitions before its end (the refusal tests)."""
    end = MODULE.rindex("ServerSymmetry ==")
    return MODULE[:end] + definitions + "\n\n" + MODULE[end:]


@functools.lru_cache(maxsize=None)
def verdicts(case, group):
    """Per state of invariant_cases.states(case): the twins' verdicts of the group, in order."""
    from tests import invariant_cases as IC
    m, _ = IC.CASES[case]
    return tuple(tuple(TWINS[p](m, s) for p in GROUPS[group]) for s in IC.states(case))


def oracle_violation_depth(model, twin, symmetry=False, max_levels=None):
    """The first level of the oracle's BFS with a state the twin does not report HOLDS
    on; None if the search ends (or reaches max_levels) without one."""
    key = (lambda t: R.canonical(model, t)) if symmetry else (lambda t: t)
    s0 = R.init_state(model)
    seen, frontier, depth = {key(s0)}, [s0], 1
    while frontier:
        if any(twin(model, s) != HOLDS for s in frontier):
            return depth
        if max_levels is not None and depth >= max_levels:
            return None
        nxt = []
        for s in frontier:
            for _f, _p, t in R.successors(model, s):
                if R.in_constraint(model, t):
                    k = key(t)
                    if k not in seen:
                        seen.add(k)
                        nxt.append(t)
        frontier = nxt
        depth += 1
    return None
