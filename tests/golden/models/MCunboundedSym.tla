---- MODULE MCunboundedSym ----
\* Fixture: MCunbounded (a Toolbox-style model module with NO state constraint,
\* the shape of the reference's MCraft.cfg as shipped) with the one addition a
\* user makes first to reach deeper: a symmetry set over the servers.
\* Its state space is infinite; it runs only under a depth bound (-depth N),
\* on the wide layout, with one state kept per orbit of Permutations(Server).
EXTENDS raft, TLC

CONSTANTS
s1, s2, s3
----

CONSTANTS
w1, w2
----

const_300 ==
{w1, w2}
----

const_400 ==
{s1, s2, s3}
----

symm_500 ==
Permutations(const_400)
----
====
