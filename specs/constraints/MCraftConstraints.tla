--------------------------- MODULE MCraftConstraints ---------------------------
\* A state constraint of the model's own (DESIGN.md "Model-defined constraints"):
\* conjuncts of a CONSTRAINT that are none of the four bounds the engine implements
\* inside its expansion kernel.  rmc-tlc compiles each such *residual* to the bytecode
\* of its predicate interpreter and filters the states every launch stores: a state
\* that fails one is counted as generated and dropped, as TLC drops it.  The bounds
\* are those of ../MCraftTiny2.cfg; the module stands in a directory of its own
\* because a cfg next to the other models is read without the front-end's
\* constraint option too.
EXTENDS raft, FiniteSets, TLC

CONSTANTS r1, r2, r3, r4, r5, v1, v2
CONSTANTS MaxTerm, MaxLogLen, MaxMsgs, MaxDup

Servers2 == {r1, r2}
Servers3 == {r1, r2, r3}
Servers4 == {r1, r2, r3, r4}
Servers5 == {r1, r2, r3, r4, r5}
Values1 == {v1}
Values2 == {v1, v2}

\* The four bounds, and a scenario cut: never two candidates at once.
StateConstraint ==
    /\ \A i \in Server : currentTerm[i] <= MaxTerm /\ Len(log[i]) <= MaxLogLen
    /\ Cardinality(DOMAIN messages) <= MaxMsgs
    /\ \A m \in DOMAIN messages : messages[m] <= MaxDup
    /\ Cardinality({i \in Server : state[i] = Candidate}) <= 1

\* A second CONSTRAINT of the cfg: once a server has reached the last term, at most
\* one message is in flight.
Scenario ==
    (\E i \in Server : currentTerm[i] = MaxTerm) => Cardinality(DOMAIN messages) <= 1

\* An invariant of the model's own, checked on the states the constraint keeps.
MsgTermsBounded ==
    \A m \in DOMAIN messages : m.mterm <= currentTerm[m.msource] /\ messages[m] >= 1
=============================================================================
