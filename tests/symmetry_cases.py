"""Inputs of the per-state SYMMETRY tests (test_symmetry.py on the GPU,
test_symmetry_native.py on the host): the models, their seeded states (uniform and
tie-heavy), permuted copies and twins, and the oracle's orbits.  Everything here
comes from oracle/raft_spec.py; nothing is read from the engine.  Test
infrastructure only."""
import functools
import itertools
import random
from collections import defaultdict

from oracle import raft_spec as R
from tests.convert import random_state, random_state_edge

# every symmetric shape the library instantiates (S = 2..5, bags of 4 and of 8 slots; S = 2
# with the 8-slot bag has no model of its own: its permutations are those of sym_s2k4)
CASES = {
    "sym_s2k4": R.Model(n_servers=2, n_values=1, max_term=2, max_log=1, max_msgs=2, max_dup=1),
    "sym_s3k4": R.Model(n_servers=3, n_values=2, max_term=3, max_log=2, max_msgs=4, max_dup=2),
    "sym_s3k8": R.Model(n_servers=3, n_values=2, max_term=14, max_log=3, max_msgs=8, max_dup=3),
    "sym_s4k4": R.Model(n_servers=4, n_values=2, max_term=3, max_log=2, max_msgs=4, max_dup=2),
    "sym_s4k8": R.Model(n_servers=4, n_values=1, max_term=13, max_log=3, max_msgs=8, max_dup=3),
    "sym_s5k4": R.Model(n_servers=5, n_values=2, max_term=3, max_log=1, max_msgs=3, max_dup=1),
    "sym_s5k8": R.Model(n_servers=5, n_values=2, max_term=14, max_log=3, max_msgs=8, max_dup=3),
}
# base states per S (half uniform, half tied_state) and drawn permutations per base state
# (None: all S! - 1 of them; the identity's copy is the base state itself)
N_BASE = {2: 150, 3: 150, 4: 120, 5: 44}
N_SIGMA = {2: None, 3: None, 4: 6, 5: 6}
# the partitions tied_state draws from (sizes of the classes of servers built alike), and
# how often it adds messages
SHAPES = {2: [(2,), (2,), (2,), (1, 1)],
          3: [(3,), (3,), (2, 1), (2, 1), (2, 1), (2, 1)],
          4: [(2, 2), (2, 2), (2, 2), (3, 1), (3, 1), (3, 1), (4,), (2, 1, 1)],
          5: [(3, 2)] * 10 + [(2, 2, 1), (4, 1)]}
P_MESSAGES = {2: 0.4, 3: 0.25, 4: 0.25, 5: 0.25}


def kcap(model):  # bag slots of the packed shape (rmc_api.cpp kcap_for)
    return 4 if model.max_msgs <= 4 else 8


def _body(model, rng, t):
    """The fields of a message of type t other than its servers."""
    V, T, L = model.n_values, model.max_term, model.max_log
    ent = lambda: R.entry(rng.randint(0, T), rng.randrange(V))
    c = dict(mtype=t, mterm=rng.randint(0, T))
    if t == R.RVQ:
        c.update(mlastLogTerm=rng.randint(0, T), mlastLogIndex=rng.randint(0, L))
    elif t == R.RVP:
        c.update(mvoteGranted=rng.random() < 0.5, mlog=tuple(ent() for _ in range(rng.randint(0, L))))
    elif t == R.AEQ:
        c.update(mprevLogIndex=rng.randint(-1, L), mprevLogTerm=rng.randint(0, T),
                 mentries=tuple(ent() for _ in range(rng.randint(0, 1))), mcommitIndex=rng.randint(0, L))
    else:
        c.update(msuccess=rng.random() < 0.5, mmatchIndex=rng.randint(0, L))
    return c


def tied_state(model, rng):
    """(state, class of every server): servers of one class share every field a
    permutation leaves alone (term, role, commitIndex, log, votedFor as Nil / self /
    another, the sizes of the vote sets and whether they hold the server itself, its
    own (nextIndex, matchIndex) and the multiset of its peers' pairs, the messages it
    sends and receives up to their counterpart) and draw for themselves which peers
    those are: who they voted for, who sits in the vote sets, which peer has which
    pair, who the messages' counterparts are.  So servers tie without a permutation
    that swaps them fixing the state."""
    S, V, T, L = model.n_servers, model.n_values, model.max_term, model.max_log
    shape = rng.choice(SHAPES[S])
    order = list(range(S))
    rng.shuffle(order)
    cls = [0] * S
    members = []
    for c, n in enumerate(shape):
        members.append(sorted(order[:n]))
        for i in order[:n]:
            cls[i] = c
        order = order[n:]
    # messages in a minority of the states: a message ties its sender's class and, landing on
    # one member of another class and not on the next, unties that one
    n_tmpl = rng.choice([1, 1, 2, 3]) if rng.random() < P_MESSAGES[S] else 0
    kinds = []
    for c in range(len(shape)):
        kinds.append(dict(
            term=rng.choice([rng.randint(0, T), T]), role=rng.choice([R.FOLLOWER, R.CANDIDATE, R.LEADER]),
            ci=rng.randint(0, L), log=tuple(R.entry(rng.randint(0, T), rng.randrange(V)) for _ in range(rng.randint(0, L))),
            vf=rng.choice(["nil", "self", "other"]), self_vr=rng.random() < 0.5, self_vg=rng.random() < 0.5,
            peers_vr=rng.randint(0, S - 1), peers_vg=rng.randint(0, S - 1),
            own=(rng.randint(1, L + 1), rng.randint(0, L)),
            pairs=[(rng.randint(1, L + 1), rng.randint(0, L)) for _ in range(S - 1)]))
    if n_tmpl == 0 and all(k["peers_vr"] == 0 and k["peers_vg"] == 0 for k in kinds):
        kinds[0]["peers_vr"] = 1  # something a twin can move
    ct, st, vf, lg, ci, vr, vg, ni, mi = [], [], [], [], [], [], [], [], []
    for i in range(S):
        k = kinds[cls[i]]
        peers = [j for j in range(S) if j != i]
        ct.append(k["term"])
        st.append(k["role"])
        lg.append(k["log"])
        ci.append(k["ci"])
        vf.append(R.NIL if k["vf"] == "nil" else i if k["vf"] == "self" else rng.choice(peers))
        vr.append(frozenset(rng.sample(peers, k["peers_vr"]) + ([i] if k["self_vr"] else [])))
        vg.append(frozenset(rng.sample(peers, k["peers_vg"]) + ([i] if k["self_vg"] else [])))
        pairs = list(k["pairs"])
        rng.shuffle(pairs)
        row = dict(zip(peers, pairs))
        row[i] = k["own"]
        ni.append(tuple(row[j][0] for j in range(S)))
        mi.append(tuple(row[j][1] for j in range(S)))
    msgs = {}
    for _ in range(n_tmpl):
        c = rng.randrange(len(shape))
        if len(msgs) + len(members[c]) > model.max_msgs:
            break
        body = _body(model, rng, rng.choice([R.RVQ, R.RVP, R.AEQ, R.AEP]))
        count, sends = rng.randint(1, model.max_dup), rng.random() < 0.5
        for i in members[c]:
            peers = [j for j in range(S) if j != i]
            rng.shuffle(peers)
            for j in peers:  # the first counterpart that gives a message not yet in the bag
                m = R.rec(msource=i if sends else j, mdest=j if sends else i, **body)
                if m not in msgs:
                    msgs[m] = count
                    break
    s = R.State(messages=frozenset(msgs.items()), currentTerm=tuple(ct), state=tuple(st), votedFor=tuple(vf),
                log=tuple(lg), commitIndex=tuple(ci), votesResponded=tuple(vr), votesGranted=tuple(vg),
                nextIndex=tuple(ni), matchIndex=tuple(mi))
    assert R.in_constraint(model, s)
    return s, tuple(cls)


def twin_of(model, s, cls, rng):
    """s with one peer in one vote set, or one end of one message, moved to a server
    of another class (where the state offers no such move: to any other server, and
    at last the peer in a vote set to the set's own server); None if it offers no
    move at all."""
    S = model.n_servers
    bag = dict(s.messages)
    for other_class in (True, False):
        moves = []
        for field in ("votesResponded", "votesGranted"):
            for i in range(S):
                have = getattr(s, field)[i]
                for p in sorted(have - {i}):
                    for q in range(S):
                        if q != i and q not in have and (cls[q] != cls[p] or not other_class):
                            moves.append((field, i, p, q))
        for m in sorted(bag, key=repr):
            for end in ("msource", "mdest"):
                old = R.rget(m, end)
                for q in range(S):
                    if q != old and (cls[q] != cls[old] or not other_class):
                        d = dict(m)
                        d[end] = q
                        if R.rec(**d) not in bag:
                            moves.append((m, end, q))
        if moves:
            break
    if not moves:  # (S = 2: a server has one peer) the peer in a vote set gives way to the server itself
        moves = [(field, i, p, i) for field in ("votesResponded", "votesGranted") for i in range(S)
                 for p in sorted(getattr(s, field)[i] - {i}) if i not in getattr(s, field)[i]]
    if not moves:
        return None
    mv = rng.choice(moves)
    if len(mv) == 4:
        field, i, p, q = mv
        have = getattr(s, field)
        return s._replace(**{field: R.tset(have, i, (have[i] - {p}) | {q})})
    m, end, q = mv
    d = dict(m)
    d[end] = q
    cnt = bag.pop(m)
    bag[R.rec(**d)] = cnt
    return s._replace(messages=frozenset(bag.items()))


# ---- the oracle's side ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def orbit_key(model, t):
    return R.canonical(model, t)


def inverse(p):
    inv = [0] * len(p)
    for a, b in enumerate(p):
        inv[b] = a
    return tuple(inv)


def summary(model, s, i):
    """What a permutation cannot change of server i."""
    mask = lambda m: tuple((k, v) for k, v in m if k not in ("msource", "mdest"))
    sent = sorted(repr((mask(m), c)) for m, c in s.messages if R.rget(m, "msource") == i)
    recv = sorted(repr((mask(m), c)) for m, c in s.messages if R.rget(m, "mdest") == i)
    v = s.votedFor[i]
    return (s.currentTerm[i], s.state[i], s.commitIndex[i], s.log[i], "nil" if v == R.NIL else "self" if v == i else "other",
            len(s.votesResponded[i]), len(s.votesGranted[i]), i in s.votesResponded[i], i in s.votesGranted[i],
            (s.nextIndex[i][i], s.matchIndex[i][i]),
            tuple(sorted((s.nextIndex[i][j], s.matchIndex[i][j]) for j in range(model.n_servers) if j != i)),
            tuple(sent), tuple(recv))


def ties(model, s):
    """The classes of two or more servers with equal summaries (lists of servers)."""
    groups = defaultdict(list)
    for i in range(model.n_servers):
        groups[summary(model, s, i)].append(i)
    return sorted((g for g in groups.values() if len(g) >= 2), key=lambda g: (-len(g), g))


def automorphisms(model, s):
    return sum(1 for p in itertools.permutations(range(model.n_servers)) if R.permute_state(model, s, p) == s)


# ---- the inputs ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _drawn(name):
    m = CASES[name]
    k = sorted(CASES).index(name)
    r1, r2, r3 = random.Random(11000 + k), random.Random(12000 + k), random.Random(13000 + k)
    n = N_BASE[m.n_servers]
    uniform = [(random_state if t % 2 == 0 else random_state_edge)(m, r1) for t in range(n // 2)]
    tied = [tied_state(m, r2) for _ in range(n - n // 2)]
    twins = [twin_of(m, s, cls, r3) for s, cls in tied]
    return tuple(uniform), tuple(tied), tuple(twins)


def bases(name):
    """The base states: the uniform half, then the tied_state half."""
    uniform, tied, _ = _drawn(name)
    return uniform + tuple(s for s, _c in tied)


def tied_bases(name):
    """Indices into bases() of the tied_state half."""
    uniform, tied, _ = _drawn(name)
    return range(len(uniform), len(uniform) + len(tied))


@functools.lru_cache(maxsize=None)
def sigmas(name):
    """Per base state the permutations of its copies (old id -> new id), the identity
    left out: all of them at S <= 3; at S = 4 and 5 six drawn ones, among them a
    transposition (inside a tie class where the state has one) and a 3-cycle."""
    m = CASES[name]
    S = m.n_servers
    every = [p for p in itertools.permutations(range(S)) if p != tuple(range(S))]
    if N_SIGMA[S] is None:
        return tuple(tuple(every) for _ in bases(name))
    rng = random.Random(14000 + sorted(CASES).index(name))
    out = []
    for s in bases(name):
        t = ties(m, s)
        a, b = rng.sample(t[0], 2) if t else rng.sample(range(S), 2)
        swap = list(range(S))
        swap[a], swap[b] = b, a
        x, y, z = rng.sample(range(S), 3)
        cyc = list(range(S))
        cyc[x], cyc[y], cyc[z] = y, z, x
        ps = [tuple(swap), tuple(cyc)]
        while len(ps) < N_SIGMA[S]:
            p = rng.choice(every)
            if p not in ps:
                ps.append(p)
        out.append(tuple(ps))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def copies(name):
    """[(index of the base state, sigma, sigma(base state))]"""
    m = CASES[name]
    return tuple((b, p, R.permute_state(m, s, p)) for b, s in enumerate(bases(name)) for p in sigmas(name)[b])


@functools.lru_cache(maxsize=None)
def twins(name):
    """([(index of the base state, twin)] for the twins in another orbit than their
    original, the number of twins dropped: in the original's orbit, or never built)."""
    m = CASES[name]
    _, _, drawn = _drawn(name)
    keep, dropped = [], 0
    for b, tw in zip(tied_bases(name), drawn):
        if tw is not None and orbit_key(m, tw) != orbit_key(m, bases(name)[b]):
            keep.append((b, tw))
        else:
            dropped += 1
    return tuple(keep), dropped


@functools.lru_cache(maxsize=None)
def states_and_orbits(name):
    """Base states, copies and surviving twins in that order, and per state the number
    of its orbit (equal numbers: one orbit)."""
    m = CASES[name]
    base = bases(name)
    states = list(base) + [t for _b, _p, t in copies(name)] + [t for _b, t in twins(name)[0]]
    ids = {}
    orbit = [ids.setdefault(orbit_key(m, s), len(ids)) for s in base]
    orbit += [orbit[b] for b, _p, _t in copies(name)]  # a copy's orbit is its original's, by definition
    orbit += [ids.setdefault(orbit_key(m, t), len(ids)) for _b, t in twins(name)[0]]
    return tuple(states), tuple(orbit)


def expand_inputs(name):
    """The states the successor tests expand: the base states and their copies."""
    return bases(name) + tuple(t for _b, _p, t in copies(name))


@functools.lru_cache(maxsize=None)
def successor_orbits(name):
    """{in-CONSTRAINT successor of a state of expand_inputs: its orbit key}.  The
    successors of a copy sigma(s) are taken back through sigma's inverse, where they
    must be the successors of s (Next is symmetric), whose keys are cached."""
    m = CASES[name]
    base = bases(name)
    out = {}
    base_succ = []
    for s in base:
        ts = {t for _f, _p, t in R.successors(m, s) if R.in_constraint(m, t)}
        base_succ.append(ts)
        for t in ts:
            out[t] = orbit_key(m, t)
    for b, p, c in copies(name):
        inv = inverse(p)
        back = set()
        for _f, _p, u in R.successors(m, c):
            if R.in_constraint(m, u):
                t = R.permute_state(m, u, inv)
                back.add(t)
                out[u] = orbit_key(m, t)
        assert back == base_succ[b], (name, b, p)  # sigma(successors(s)) = successors(sigma(s))
    return out


@functools.lru_cache(maxsize=None)
def vacuity_figures(name):
    m = CASES[name]
    S = m.n_servers
    base = bases(name)
    t = [ties(m, s) for s in base]
    members = defaultdict(set)
    for u, k in successor_orbits(name).items():
        members[k].add(u)
    kept, dropped = twins(name)
    return dict(base=len(base), tied=sum(1 for x in t if x),
                tied_rigid=sum(1 for s, x in zip(base, t) if x and automorphisms(m, s) == 1),
                class3=sum(1 for x in t if x and len(x[0]) >= 3), two_classes=sum(1 for x in t if len(x) >= 2),
                twins_kept=len(kept), twins_dropped=dropped,
                successors=len(successor_orbits(name)), orbits_with_2=sum(1 for v in members.values() if len(v) >= 2))


def check_not_vacuous(name):
    """Conditions on the inputs, from the oracle alone: enough ties, enough ties
    without a non-trivial automorphism, tie classes of three and two classes at once
    (S >= 4), twins that left their orbit, and orbits with several successors in them."""
    S = CASES[name].n_servers
    f = vacuity_figures(name)
    assert f["base"] >= {2: 150, 3: 150, 4: 60, 5: 20}[S], f
    assert 3 * f["tied"] >= f["base"], f
    if S >= 3:
        assert 4 * f["tied_rigid"] >= f["base"], f
    if S >= 4:
        assert f["class3"] >= 10 and f["two_classes"] >= 10, f
    assert f["twins_kept"] + f["twins_dropped"] == len(tied_bases(name)), f
    assert f["twins_kept"] >= f["twins_dropped"], f
    assert f["orbits_with_2"] >= 50, f
    return f
