"""Inputs of the model-defined constraint tests (test_constraints.py on the GPU,
test_constraints_front.py and test_constraints_native.py on the host): residual
CONSTRAINT conjuncts as TLA+ text, each with a Python twin over oracle.raft_spec
states, the model files that carry them, and the oracle of a constrained search.

The oracle is a level loop over oracle.raft_spec.successors and in_constraint
with the twin conjoined, by the rules of oracle.raft_spec.bfs: a successor the
constraint fails counts in `generated` and nowhere else, a level whose states
are all filtered adds nothing to the depth, an initial state that fails gives
distinct 0, generated 1, depth 0.  It also counts, per level, the successors the
residual alone removed, so that a test can assert that it removed any.
Everything expected here comes from oracle/raft_spec.py; nothing is read from
the engine.  Test infrastructure only."""
import functools
import os
from dataclasses import dataclass, field

from oracle import raft_spec as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class EvalError(Exception):
    """A twin's read outside a domain (TLC: an evaluation error)."""


# ---- the residuals: TLA+ text and twin(model, state) -> bool (or EvalError) ----------
def _no_leader(model, s):
    return all(r != R.LEADER for r in s.state)


def _one_candidate(model, s):
    return sum(1 for r in s.state if r == R.CANDIDATE) <= 1


def _no_commit_no_leader(model, s):
    return all(c == 0 for c in s.commitIndex) and _no_leader(model, s)


def _term_implies_few_msgs(model, s):
    return not any(t == model.max_term for t in s.currentTerm) or len(s.messages) <= 1


def _no_ae_request(model, s):
    return all(R.rget(m, "mtype") != R.AEQ for m, _c in s.messages)


def _one_leader_at_most(model, s):
    return sum(1 for r in s.state if r == R.LEADER) <= 1


def _leader_first_entry(model, s):
    # \A i : state[i] = Leader => log[i][1].term >= 1, left to right: a leader with an empty
    # log is a read outside DOMAIN log[i] (in a reachable state an entry's term is at least 1)
    for i in range(model.n_servers):
        if s.state[i] == R.LEADER:
            if len(s.log[i]) == 0:
                raise EvalError("log[%d][1]" % i)
            if R.rget(s.log[i][0], "term") < 1:
                return False
    return True


def _never(model, s):
    return False


def _always(model, s):
    return True


def _short_terms(model, s):
    # currentTerm[i] < MaxTerm for all i: no state of the level that first reaches MaxTerm stays
    return all(t < model.max_term for t in s.currentTerm)


# name -> (the conjunct's TLA+ text, twin)
RESIDUALS = {
    "NoLeader": (r"\A i \in Server : state[i] /= Leader", _no_leader),
    "OneCandidate": (r"Cardinality({i \in Server : state[i] = Candidate}) <= 1", _one_candidate),
    "NoCommitNoLeader": (r"\A i \in Server : commitIndex[i] = 0 /\ state[i] /= Leader", _no_commit_no_leader),
    "TermImpliesFewMsgs": (r"(\E i \in Server : currentTerm[i] = MaxTerm) => Cardinality(DOMAIN messages) <= 1",
                           _term_implies_few_msgs),
    "NoAERequest": (r"\A m \in DOMAIN messages : m.mtype /= AppendEntriesRequest", _no_ae_request),
    "TwoCandidates": (r"Cardinality({i \in Server : state[i] = Candidate}) <= 2",
                      lambda model, s: sum(1 for r in s.state if r == R.CANDIDATE) <= 2),
    "OneLeaderAtMost": (r"Cardinality({i \in Server : state[i] = Leader}) <= 1", _one_leader_at_most),
    "LeaderFirstEntry": (r"\A i \in Server : state[i] = Leader => log[i][1].term >= 1", _leader_first_entry),
    "Never": (r"\E i \in Server : currentTerm[i] < 0", _never),
    "Always": ("TRUE", _always),
    "ShortTerms": (r"~(\E i \in Server : currentTerm[i] >= MaxTerm)", _short_terms),
    "NamesServer": (r"state[r1] /= Leader", lambda model, s: s.state[0] != R.LEADER),
}

# The model's own predicate of the invariant tests: the text of OneLeaderPerTerm under another name.
USER_ONE_LEADER = r"""UserOneLeader ==
    \A i, j \in Server :
        (state[i] = Leader /\ state[j] = Leader /\ currentTerm[i] = currentTerm[j]) => i = j
"""


def with_definitions(text, definitions):
    """A module's text with more definitions before its closing ==== line."""
    end = text.rindex("\n====") + 1
    return text[:end] + definitions + "\n" + text[end:]


def module_text(name="ConsCases"):
    """specs/MCraftBounded.tla under the module name `name`, with one definition per residual:
    Cons<R> conjoins it to the bounds in one CONSTRAINT, Only<R> is the residual alone (a second
    CONSTRAINT name)."""
    text = open(os.path.join(ROOT, "specs", "MCraftBounded.tla")).read()
    text = text.replace("MODULE MCraftBounded", "MODULE " + name, 1)
    defs = [USER_ONE_LEADER]
    for rname, (tla, _twin) in RESIDUALS.items():
        defs.append("Only%s ==\n    %s\n" % (rname, tla))
        defs.append("Cons%s ==\n    /\\ StateConstraint\n    /\\ %s\n" % (rname, tla))
    return with_definitions(text, "\n".join(defs))


def cfg_text(n_servers, n_values, max_term, max_log, max_msgs, max_dup, constraints, invariants=(), symmetry=False,
             bug=False):
    mv = "\n".join("    %s = %s" % (x, x) for x in (
        "r1", "r2", "r3", "r4", "r5", "v1", "v2", "Follower", "Candidate", "Leader", "Nil", "RequestVoteRequest",
        "RequestVoteResponse", "AppendEntriesRequest", "AppendEntriesResponse"))
    return ("CONSTANTS\n%s\n    Server <- Servers%d\n    Value <- Values%d\n    MaxTerm = %d\n    MaxLogLen = %d\n"
            "    MaxMsgs = %d\n    MaxDup = %d\n%sSPECIFICATION Spec\n%s%s%s"
            % (mv, n_servers, n_values, max_term, max_log, max_msgs, max_dup,
               "    BecomeLeader <- BugBecomeLeader\n" if bug else "",
               "".join("CONSTRAINT %s\n" % c for c in constraints),
               "SYMMETRY ServerSymmetry\n" if symmetry else "",
               "".join("INVARIANT %s\n" % i for i in invariants)))


def write_model(dirpath, model, constraints, invariants=(), symmetry=False, name="ConsCases"):
    """Writes <dirpath>/<name>.tla and .cfg for the oracle Model `model`; returns (cfg path, tla path)."""
    tla, cfg = os.path.join(str(dirpath), name + ".tla"), os.path.join(str(dirpath), name + ".cfg")
    with open(tla, "w") as f:
        f.write(module_text(name))
    with open(cfg, "w") as f:
        f.write(cfg_text(model.n_servers, model.n_values, model.max_term, model.max_log, model.max_msgs,
                         model.max_dup, constraints, invariants, symmetry, model.bug_quorum))
    return cfg, tla


# ---- the models ------------------------------------------------------------------------
TINY2 = R.Model(n_servers=2, n_values=1, max_term=2, max_log=1, max_msgs=2, max_dup=1)   # specs/MCraftTiny2.cfg
SMALL3 = R.Model(n_servers=3, n_values=2, max_term=2, max_log=1, max_msgs=2, max_dup=1)  # predicate_cases' bounds


@dataclass
class ConsResult:
    generated: int = 0
    distinct: int = 0
    depth: int = 0
    left_on_queue: int = 0
    level_new: list = field(default_factory=list)
    level_generated: list = field(default_factory=list)   # [d]: generated expanding level d (index 0: the seed)
    level_removed: list = field(default_factory=list)     # [d]: successors the residual alone removed there
    levels: list = field(default_factory=list)            # the kept states of each level
    violated: str | None = None
    violation_depth: int | None = None
    error_depth: int | None = None                        # the level of the first state the residual raises on


def bfs(model, residual, invariants=(), max_levels=None, symmetry=False):
    """oracle.raft_spec.bfs with `residual` conjoined to in_constraint.  A state the residual
    raises EvalError on is kept; the search stops at the end of its level (error_depth).  An
    invariant violation ends the search at the end of its level too (the engine finishes the
    level; only violated / violation_depth are compared then)."""
    key = (lambda t: R.canonical(model, t)) if symmetry else (lambda t: t)
    out = ConsResult()
    erred = []

    def keep(t):
        try:
            return residual(model, t)
        except EvalError:
            erred.append(t)
            return True

    def end_level(states, depth):
        for name in invariants:
            if out.violated is None and any(not R.INVARIANTS[name](model, s) for s in states):
                out.violated, out.violation_depth = name, depth
        if erred and out.error_depth is None:
            out.error_depth = depth
        return out.violated is not None or out.error_depth is not None

    s0 = R.init_state(model)
    seen, frontier, removed = {}, [], 0
    if R.in_constraint(model, s0):
        if keep(s0):
            seen[key(s0)] = None
            frontier.append(s0)
        else:
            removed = 1
    out.generated = 1
    out.level_new, out.level_generated, out.level_removed = [len(frontier)], [1], [removed]
    out.levels = [list(frontier)]
    out.depth = 1 if frontier else 0
    stop = end_level(frontier, 1)
    while frontier and not stop and (max_levels is None or out.depth < max_levels):
        nxt, gen, removed = [], 0, 0
        for s in frontier:
            for _f, _p, t in R.successors(model, s):
                gen += 1
                if not R.in_constraint(model, t):
                    continue
                k = key(t)
                if k in seen:
                    continue
                if not keep(t):
                    removed += 1
                    seen[k] = False  # (its fingerprint stays in the set: later copies are duplicates)
                    continue
                seen[k] = None
                nxt.append(t)
        out.generated += gen
        out.level_generated.append(gen)
        out.level_removed.append(removed)
        if nxt:
            out.level_new.append(len(nxt))
            out.levels.append(nxt)
            out.depth += 1
            stop = end_level(nxt, out.depth)
        frontier = nxt
    out.distinct = sum(1 for v in seen.values() if v is None)
    out.left_on_queue = len(frontier) if not stop else 0
    return out


@functools.lru_cache(maxsize=None)
def oracle(model, residual_name, invariants=(), max_levels=None, symmetry=False):
    return bfs(model, RESIDUALS[residual_name][1], invariants, max_levels, symmetry)
