--------------------------- MODULE MCraftPredicates ---------------------------
\* Invariants of the model's own (DESIGN.md "Model-defined invariants"): state
\* predicates that are none of the ten the engine compiles in.  rmc-tlc compiles
\* each to the bytecode of its predicate interpreter and checks it on every state
\* the search stores.  The bounds are those of ../MCraftBounded.tla; the module
\* stands in a directory of its own because a cfg next to the other models is
\* read without the front-end's predicate option too.
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

\* One of the ten compiled-in invariants (the text of ../MCraftBounded.tla): it
\* keeps its fused check, beside the predicates below.
OneLeaderPerTerm ==
    \A i, j \in Server :
        (state[i] = Leader /\ state[j] = Leader /\ currentTerm[i] = currentTerm[j]) => i = j

\* A message never carries a term its sender has not reached, and every message
\* in the bag is there at least once.
MsgTermsBounded ==
    \A m \in DOMAIN messages : m.mterm <= currentTerm[m.msource] /\ messages[m] >= 1

\* Every quorum has a member whose commit index lies within its log.
QuorumHasCommitted ==
    \A Q \in Quorum : \E j \in Q : commitIndex[j] <= Len(log[j])

\* No log holds an entry of a term its server has not reached.
NoFutureEntry(i) == \A n \in DOMAIN log[i] : log[i][n].term <= currentTerm[i]
LogTermsBounded == \A i \in Server : NoFutureEntry(i)

\* Not an invariant: a leader can be elected.  Its counterexample is a shortest
\* election (TLC reports the same depth).
NoLeaderElected ==
    \A i \in Server : state[i] /= Leader
=============================================================================
