---------------------------- MODULE MCraftActions ----------------------------
\* Action properties (DESIGN.md "Action properties"): PROPERTY P with
\* P == [][A]_vars, a safety property of every transition.  rmc-tlc compiles each A
\* to the bytecode of its predicate interpreter, with primes, and checks it on every
\* transition the search generates inside the CONSTRAINT.  The bounds are those of
\* ../MCraftTiny2.cfg; the module stands in a directory of its own because a cfg next
\* to the other models is read without the front-end's action option too.
EXTENDS raft, FiniteSets, TLC

CONSTANTS r1, r2, r3, r4, r5, v1, v2
CONSTANTS MaxTerm, MaxLogLen, MaxMsgs, MaxDup

Servers2 == {r1, r2}
Servers3 == {r1, r2, r3}
Values1 == {v1}
Values2 == {v1, v2}

StateConstraint ==
    /\ \A i \in Server : currentTerm[i] <= MaxTerm /\ Len(log[i]) <= MaxLogLen
    /\ Cardinality(DOMAIN messages) <= MaxMsgs
    /\ \A m \in DOMAIN messages : messages[m] <= MaxDup

\* Terms never go back.
TermsMonotonic == [][\A i \in Server : currentTerm'[i] >= currentTerm[i]]_vars

\* A server that stays leader of its term only appends to its log.
LeaderAppendOnly == [][
    \A i \in Server :
        (state[i] = Leader /\ state'[i] = Leader /\ currentTerm'[i] = currentTerm[i])
        => /\ Len(log'[i]) >= Len(log[i])
           /\ \A n \in DOMAIN log[i] : /\ log'[i][n].term = log[i][n].term
                                       /\ log'[i][n].value = log[i][n].value
    ]_vars

\* A server votes once per term.
VoteOncePerTerm == [][
    \A i \in Server :
        (currentTerm'[i] = currentTerm[i] /\ votedFor[i] /= Nil) => votedFor'[i] = votedFor[i]
    ]_vars

\* commitIndex never decreases.  raft.tla's Restart (raft.tla:136-143) resets it to 0,
\* so this one is violated: the checker shows the behaviour that ends in that Restart.
CommitMonotonic == [][\A i \in Server : commitIndex'[i] >= commitIndex[i]]_vars
=============================================================================
