"""Inputs of the per-state SYMMETRY tests of the wide layout (test_wide_symmetry.py on
the GPU, test_wide_symmetry_native.py on the host), beyond those of
tests/symmetry_cases.py: per S states past the packed capacity from random walks of the
unconstrained spec (as tests/test_wide.py draws them), tie-heavy states and their
one-field twins built with symmetry_cases' helpers on bounds only the wide record holds,
permuted copies of all of them, and the oracle's orbits.  Everything here comes from
oracle/raft_spec.py; nothing is read from the engine.  Test infrastructure only."""
import functools
import itertools
import random
from collections import defaultdict

from oracle import raft_spec as R
from tests import symmetry_cases as SC

# the walks' model (nothing bounded) and the tie-heavy states' bounds per case
WALK = {"wide_s3": R.Model(), "wide_s5": R.Model(n_servers=5)}
TIED = {"wide_s3": R.Model(n_servers=3, n_values=2, max_term=40, max_log=6, max_msgs=12, max_dup=5),
        "wide_s5": R.Model(n_servers=5, n_values=2, max_term=40, max_log=6, max_msgs=12, max_dup=5)}
CASES = sorted(WALK)
# (walks, steps at most, seed): wide_s3 is tests/test_wide.py's draw
WALKS = {"wide_s3": (300, 60, 7), "wide_s5": (120, 60, 8)}
N_TIED = {"wide_s3": 120, "wide_s5": 40}
# the bounds of the ctx the GPU tests run these on (every state below fits them)
CTX_BOUNDS = dict(max_term=255, max_log_len=8, max_msgs=16, max_dup=255)


def walk_states(model, n, depth, seed):
    """Random walks from Init of the unconstrained spec (tests/test_wide.py _walk_states)."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = R.init_state(model)
        for _ in range(rng.randint(1, depth)):
            s = rng.choice(R.successors(model, s))[2]
        out.append(s)
    return out


def fits_wide(s):
    return (all(t <= 250 for t in s.currentTerm) and all(len(lg) <= 7 for lg in s.log) and len(s.messages) <= 15
            and all(c <= 250 for _, c in s.messages))


def beyond_packed(s):
    return (max(s.currentTerm) > 15 or max(len(x) for x in s.log) > 3 or len(s.messages) > 8
            or any(c > 3 for _, c in s.messages))


def model_of(name):
    """The model the orbits are taken in: only n_servers matters to permutations."""
    return WALK[name]


@functools.lru_cache(maxsize=None)
def _drawn(name):
    k = CASES.index(name)
    n, depth, seed = WALKS[name]
    walked = tuple(dict.fromkeys(s for s in walk_states(WALK[name], n, depth, seed) if fits_wide(s)))
    r2, r3 = random.Random(21000 + k), random.Random(22000 + k)
    tied = tuple(SC.tied_state(TIED[name], r2) for _ in range(N_TIED[name]))
    twins = tuple(SC.twin_of(TIED[name], s, cls, r3) for s, cls in tied)
    return walked, tied, twins


def bases(name):
    """The base states: the walks' states, then the tie-heavy ones."""
    walked, tied, _ = _drawn(name)
    return walked + tuple(s for s, _c in tied)


def tied_bases(name):
    walked, tied, _ = _drawn(name)
    return range(len(walked), len(walked) + len(tied))


@functools.lru_cache(maxsize=None)
def sigmas(name):
    """Per base state the permutations of its copies (old id -> new id), the identity
    left out: all of them at S = 3; at S = 5 six drawn ones, among them a
    transposition (inside a tie class where the state has one) and a 3-cycle."""
    m = model_of(name)
    S = m.n_servers
    every = [p for p in itertools.permutations(range(S)) if p != tuple(range(S))]
    if S <= 3:
        return tuple(tuple(every) for _ in bases(name))
    rng = random.Random(24000 + CASES.index(name))
    out = []
    for s in bases(name):
        t = SC.ties(m, s)
        a, b = rng.sample(t[0], 2) if t else rng.sample(range(S), 2)
        swap = list(range(S))
        swap[a], swap[b] = b, a
        x, y, z = rng.sample(range(S), 3)
        cyc = list(range(S))
        cyc[x], cyc[y], cyc[z] = y, z, x
        ps = [tuple(swap), tuple(cyc)]
        while len(ps) < 6:
            p = rng.choice(every)
            if p not in ps:
                ps.append(p)
        out.append(tuple(ps))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def copies(name):
    """[(index of the base state, sigma, sigma(base state))]"""
    m = model_of(name)
    return tuple((b, p, R.permute_state(m, s, p)) for b, s in enumerate(bases(name)) for p in sigmas(name)[b])


@functools.lru_cache(maxsize=None)
def twins(name):
    """([(index of the base state, twin)] for the twins in another orbit than their
    original, the number of twins dropped)."""
    m = model_of(name)
    _, _, drawn = _drawn(name)
    keep, dropped = [], 0
    for b, tw in zip(tied_bases(name), drawn):
        if tw is not None and SC.orbit_key(m, tw) != SC.orbit_key(m, bases(name)[b]):
            keep.append((b, tw))
        else:
            dropped += 1
    return tuple(keep), dropped


@functools.lru_cache(maxsize=None)
def states_and_orbits(name):
    """Base states, copies and surviving twins in that order, and per state the number
    of its orbit (equal numbers: one orbit)."""
    m = model_of(name)
    base = bases(name)
    states = list(base) + [t for _b, _p, t in copies(name)] + [t for _b, t in twins(name)[0]]
    ids = {}
    orbit = [ids.setdefault(SC.orbit_key(m, s), len(ids)) for s in base]
    orbit += [orbit[b] for b, _p, _t in copies(name)]  # a copy's orbit is its original's, by definition
    orbit += [ids.setdefault(SC.orbit_key(m, t), len(ids)) for _b, t in twins(name)[0]]
    return tuple(states), tuple(orbit)


# base states the successor tests expand, with their copies: (walked past the packed
# capacity, tie-heavy) — the oracle canonicalises every successor, 120 permutations at S = 5
N_EXPAND = {"wide_s3": (40, 40), "wide_s5": (6, 6)}


@functools.lru_cache(maxsize=None)
def expand_bases(name):
    """Indices into bases() of the states the successor tests expand."""
    walked, _tied, _ = _drawn(name)
    nw, nt = N_EXPAND[name]
    return tuple([b for b, s in enumerate(walked) if beyond_packed(s)][:nw]) + tuple(tied_bases(name)[:nt])


@functools.lru_cache(maxsize=None)
def expand_inputs(name):
    """[(index of the base state, sigma or None, state)]: the expanded base states and their copies."""
    base, chosen = bases(name), set(expand_bases(name))
    return tuple((b, None, base[b]) for b in expand_bases(name)) + tuple(c for c in copies(name) if c[0] in chosen)


@functools.lru_cache(maxsize=None)
def successor_orbits(name):
    """{successor of a state of expand_inputs: its orbit key} (SC.successor_orbits' way:
    the successors of a copy sigma(s) are taken back through sigma's inverse, where they
    must be the successors of s, whose keys are cached)."""
    m = model_of(name)
    out, base_succ = {}, {}
    for b, p, s in expand_inputs(name):
        if p is None:
            base_succ[b] = {t for _f, _p, t in R.successors(m, s)}
            for t in base_succ[b]:
                out[t] = SC.orbit_key(m, t)
            continue
        inv, back = SC.inverse(p), set()
        for _f, _p, u in R.successors(m, s):
            t = R.permute_state(m, u, inv)
            back.add(t)
            out[u] = SC.orbit_key(m, t)
        assert back == base_succ[b], (name, b, p)  # sigma(successors(s)) = successors(sigma(s))
    return out


def members_per_orbit(states, orbits):
    members = defaultdict(set)
    for s, o in zip(states, orbits):
        members[o].add(s)
    return members


@functools.lru_cache(maxsize=None)
def vacuity_figures(name):
    m = model_of(name)
    base = bases(name)
    states, orbits = states_and_orbits(name)
    t = [SC.ties(m, s) for s in base]
    kept, dropped = twins(name)
    return dict(base=len(base), beyond_packed=sum(1 for s in base if beyond_packed(s)), tied=sum(1 for x in t if x),
                tied_rigid=sum(1 for s, x in zip(base, t) if x and SC.automorphisms(m, s) == 1),
                twins_kept=len(kept), twins_dropped=dropped,
                orbits_with_2=sum(1 for v in members_per_orbit(states, orbits).values() if len(v) >= 2))


def check_not_vacuous(name):
    """Conditions on the inputs, from the oracle alone: states past the packed capacity,
    orbits with several distinct members, tied servers that no automorphism swaps, and
    twins that left their orbit."""
    f = vacuity_figures(name)
    assert f["beyond_packed"] > 30, f
    assert f["orbits_with_2"] >= 50, f
    assert f["tied_rigid"] >= 10, f
    assert f["twins_kept"] >= f["twins_dropped"] and f["twins_kept"] >= 10, f
    return f


def check_packed_case_not_vacuous(name):
    """A case of tests/symmetry_cases.py: SC.check_not_vacuous (at least 50 orbits with
    two or more distinct members among the successors the tests key, ties, twins), and
    on the states themselves such orbits for half of the base states at least (S = 5 draws
    44 of them) and tied servers that no automorphism swaps."""
    m = SC.CASES[name]
    SC.check_not_vacuous(name)
    states, orbits = SC.states_and_orbits(name)
    several = sum(1 for v in members_per_orbit(states, orbits).values() if len(v) >= 2)
    assert several >= min(50, len(SC.bases(name)) // 2), name
    if m.n_servers >= 3:  # (two servers that tie are swapped by an automorphism: SC.check_not_vacuous)
        assert any(SC.ties(m, s) and SC.automorphisms(m, s) == 1 for s in SC.bases(name)), name
