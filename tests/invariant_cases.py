"""Inputs of the per-state invariant tests (test_invariants.py on the GPU,
test_invariants_native.py on the host): the models, their seeded states and the
oracle's verdicts.  Test infrastructure only."""
import functools
import random

from oracle import raft_spec as R
from tests.convert import near_invariant_state, random_state, random_state_edge
from tests.test_gpu import FUZZ, FUZZ_EDGE

BITS = sorted(R.INV_BITS)          # 1, 2, .. 512 in first-violated order
ALL = sum(BITS)
N_PER_FAMILY = 600


def _model(p):  # BecomeLeader's guard does not enter a predicate
    return R.Model(**{k: v for k, v in p.items() if k != "bug_quorum"})


# every packed model of the successor fuzz tests: S = 2..5, K = 4 and 8, |Value| 1 and 2
PACKED = [("fuzz%d" % k, _model(p), random_state) for k, p in enumerate(FUZZ)] + \
         [("edge%d" % k, _model(p), random_state_edge) for k, p in enumerate(FUZZ_EDGE)]
# beyond the packed capacity (the wide layout only)
WIDE = [("wide_s3", R.Model(n_servers=3, n_values=2, max_term=255, max_log=8, max_msgs=20, max_dup=255), random_state),
        ("wide_s5", R.Model(n_servers=5, n_values=2, max_term=255, max_log=32, max_msgs=64, max_dup=255), random_state)]
CASES = {name: (m, gen) for name, m, gen in PACKED + WIDE}


def kcap(model):  # bag slots of the packed shape (rmc_api.cpp kcap_for)
    return 4 if model.max_msgs <= 4 else 8


@functools.lru_cache(maxsize=None)
def states(name):
    """The two families of a model, N_PER_FAMILY states each, from fixed seeds:
    the uniform generator of the successor fuzz tests and near_invariant_state."""
    m, gen = CASES[name]
    k = sorted(CASES).index(name)
    r1, r2 = random.Random(7000 + k), random.Random(8000 + k)
    return tuple([gen(m, r1) for _ in range(N_PER_FAMILY)] + [near_invariant_state(m, r2) for _ in range(N_PER_FAMILY)])


def oracle_bits(model, s):
    """The RMC_INV_* bits of the invariants s violates (oracle/raft_spec.py)."""
    return sum(b for b in BITS if not R.INVARIANTS[R.INV_BITS[b]](model, s))


@functools.lru_cache(maxsize=None)
def verdicts(name):
    m, _ = CASES[name]
    return tuple(oracle_bits(m, s) for s in states(name))


# (model, invariant) pairs where one verdict is impossible, with the reason; TypeOK
# is never violated by these generators (the encoders would refuse most type errors;
# the representable ones have tests of their own)
ONE_SIDED = {
    # every quorum of two servers is both of them, so it contains server i itself, whose
    # log has Committed(i) as a prefix
    ("fuzz2", "QuorumLogInv"): "S = 2",
    ("edge2", "QuorumLogInv"): "S = 2",
    # logs of at most one entry over one value: equal terms at index 1 are equal entries
    ("fuzz2", "LogMatching"): "|Value| = 1, MaxLogLen = 1",
}


# TypeOK: the type errors a view can carry are entry values outside Value at |Value| = 1
# (the encoders refuse the others, test_codec_native).  One model per packed S and one
# beyond the packed capacity.
TYPEOK = {"typeok_s%d" % s: R.Model(n_servers=s, n_values=1, max_term=3, max_log=3, max_msgs=4, max_dup=2)
          for s in (2, 3, 4, 5)}
TYPEOK["typeok_wide"] = R.Model(n_servers=3, n_values=1, max_term=255, max_log=8, max_msgs=20, max_dup=255)
TYPEOK_PLACES = ("server log", "mentries", "mlog")


@functools.lru_cache(maxsize=None)
def typeok_states(name):
    """[(place, state with an entry of value 1 there, the same state with value 0)]:
    five base states, each with the entry in a server's log, in an
    AppendEntriesRequest's mentries and in a RequestVoteResponse's mlog (at a
    random index of a log of random length up to MaxLogLen)."""
    m = TYPEOK[name]
    rng = random.Random(9000 + m.n_servers + m.max_log)
    out = []
    for _ in range(5):
        base = near_invariant_state(m, rng)._replace(messages=frozenset())
        n = rng.randint(1, m.max_log)
        x = rng.randrange(n)
        t = base.currentTerm[0]
        i, j = rng.randrange(m.n_servers), rng.randrange(m.n_servers)
        cnt = rng.randint(1, m.max_dup)

        def put(v):
            lg = tuple(R.entry(t, v if k == x else 0) for k in range(n))
            aeq = R.rec(mtype=R.AEQ, mterm=t, mprevLogIndex=0, mprevLogTerm=0, mentries=(R.entry(t, v),),
                        mcommitIndex=0, msource=i, mdest=j)
            rvp = R.rec(mtype=R.RVP, mterm=t, mvoteGranted=True, mlog=lg, msource=i, mdest=j)
            return (base._replace(log=R.tset(base.log, i, lg)),
                    base._replace(messages=frozenset({(aeq, 1)})),
                    base._replace(messages=frozenset({(rvp, cnt)})))
        for place, bad, good in zip(TYPEOK_PLACES, put(1), put(0)):
            assert not R.type_ok(m, bad) and R.type_ok(m, good)
            out.append((place, bad, good))
    return tuple(out)


def mixed_verdict_counts(name):
    """{invariant: (holds, violated)} over the model's states, from the oracle alone."""
    v = verdicts(name)
    return {R.INV_BITS[b]: (sum(1 for x in v if not x & b), sum(1 for x in v if x & b)) for b in BITS if b != 1}


def check_mixed_verdicts(name):
    """The inputs are not vacuous: every named invariant holds on at least 10 of the
    model's states and is violated on at least 10, but for the pairs of ONE_SIDED."""
    for inv, (holds, violated) in mixed_verdict_counts(name).items():
        if (name, inv) in ONE_SIDED:
            assert violated == 0, (name, inv)
            continue
        assert holds >= 10 and violated >= 10, (name, inv, holds, violated)
    assert not any(v & 1 for v in verdicts(name))  # TypeOK has cases of its own (TYPEOK)
