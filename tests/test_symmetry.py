"""The device SYMMETRY canonical keys and orbit comparison against the oracle,
state by state: canon_delta through rmc_expand (k_list<S, K, true>), canon_state
and same_orbit / same_state through rmc_state_keys, on every symmetric shape
(S = 2..5, bags of 4 and of 8 slots, logs of up to 3 entries, terms to 14, counts
to 3).

The symmetric goldens show whole searches with logs of one entry and three
messages.  Here the keys of single states are compared with oracle.raft_spec's
orbits (tests/symmetry_cases.py): uniform states, tie-heavy states whose tied
servers no automorphism swaps, all (S <= 3) or six drawn (S >= 4) permuted copies
of each, and twins that differ from a tied state in one peer of one vote set or one
end of one message.  Same orbit, same key (else the orbit count inflates); another
orbit, another key (else states are lost).  tests/test_symmetry_native.py runs the
same comparison on the host compilation of the same functions."""
import ctypes as C
import functools
import random

import pytest

import rmc
from oracle import raft_spec as R
from tests import symmetry_cases as SC
from tests.convert import from_view, random_state, random_state_edge, to_view
from tests.test_gpu import FUZZ, FUZZ_EDGE, compare_expand

pytestmark = pytest.mark.gpu


def checker(m, symmetry=True):
    return rmc.Checker(rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, max_term=m.max_term,
                                       max_log_len=m.max_log, max_msgs=m.max_msgs, max_dup=m.max_dup,
                                       symmetry=symmetry, state_capacity=1 << 12))


def assert_partition(keys, orbits, what):
    """keys[t] == keys[u] exactly when orbits[t] == orbits[u], over all pairs."""
    key_of, orbit_of = {}, {}
    for t, (k, o) in enumerate(zip(keys, orbits)):
        a = key_of.setdefault(o, (k, t))
        assert a[0] == k, "%s: %d and %d are one orbit with keys %#x and %#x (an orbit split)\n%r\n%r" % (
            (what[0], a[1], t, a[0], k) + (what[1][a[1]], what[1][t]))
        b = orbit_of.setdefault(k, (o, t))
        assert b[0] == o, "%s: %d and %d of two orbits share the key %#x (orbits merged)\n%r\n%r" % (
            (what[0], b[1], t, k) + (what[1][b[1]], what[1][t]))


@functools.lru_cache(maxsize=None)
def view_array(name):
    m = SC.CASES[name]
    views = [to_view(m, s) for s in SC.states_and_orbits(name)[0]]
    return (rmc.StateView * len(views))(*views)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_successor_keys_partition_successors_into_orbits(name):
    """rmc_expand under SYMMETRY on the base states and their copies: the per-lane
    successor sets equal the oracle's (compare_expand), and over all in-CONSTRAINT
    successors of the case two have one fingerprint (canon_delta) exactly when the
    oracle puts them in one orbit.  At least 50 orbits hold two or more distinct
    successors (check_not_vacuous)."""
    SC.check_not_vacuous(name)
    m = SC.CASES[name]
    fps, _out = compare_expand(m, list(SC.expand_inputs(name)), symmetry=True)
    want = SC.successor_orbits(name)
    assert set(fps) == set(want)
    succ = sorted(fps, key=repr)
    assert_partition([fps[t] for t in succ], [want[t] for t in succ], (name, succ))


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_state_keys_equal_successor_keys(name):
    """canon_state against canon_delta on the device: rmc_state_keys of every
    in-CONSTRAINT successor view that rmc_expand returns is that record's
    fingerprint."""
    m = SC.CASES[name]
    with checker(m) as ck:
        out = [sv for sv in ck.expand([to_view(m, s) for s in SC.expand_inputs(name)]) if sv.in_constraint]
        assert len(out) >= len(SC.successor_orbits(name))
        keys = ck.state_keys([sv.state for sv in out])
    for sv, k in zip(out, keys):
        assert k == sv.fingerprint, (name, sv.parent, sv.instance, from_view(sv.state))


@pytest.mark.parametrize("params,gen,seed", [(FUZZ[1], random_state, 3001), (FUZZ_EDGE[1], random_state_edge, 3002)])
def test_state_keys_equal_successor_keys_without_symmetry(params, gen, seed):
    """The same without SYMMETRY: state_fp against delta_fp, on 200 states of the
    successor fuzz models (S = 3 with 7 messages, S = 5 at the capacity's edges)."""
    m = R.Model(**params)
    rng = random.Random(seed)
    states = [gen(m, rng) for _ in range(200)]
    with checker(m, symmetry=False) as ck:
        out = [sv for sv in ck.expand([to_view(m, s) for s in states]) if sv.in_constraint]
        assert len(out) >= 200
        keys = ck.state_keys([sv.state for sv in out])
    for sv, k in zip(out, keys):
        assert k == sv.fingerprint, (sv.parent, sv.instance, from_view(sv.state))


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_state_keys_are_orbit_invariants(name):
    """rmc_state_keys (canon_state) on the base states, their copies and the twins
    that left their orbit: one key exactly where the oracle has one orbit; in
    particular every surviving twin's key differs from its original's."""
    SC.check_not_vacuous(name)
    m = SC.CASES[name]
    states, orbits = SC.states_and_orbits(name)
    with checker(m) as ck:
        keys = ck.state_keys(view_array(name))
    assert_partition(keys, orbits, (name, states))
    kept, _dropped = SC.twins(name)
    first_twin = len(states) - len(kept)
    for x, (b, tw) in enumerate(kept):
        assert states[first_twin + x] == tw
        assert keys[first_twin + x] != keys[b], (name, b, states[b], tw)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_same_orbit_equals_the_oracle(name):
    """Verification's comparison through rmc_state_keys' ref: every copy is its
    original's orbit, no surviving twin is, 200 drawn pairs of states are one orbit
    exactly when the oracle says so; and on a ctx without SYMMETRY (same_state) a
    state equals itself, and a copy its original exactly when they are one state."""
    m = SC.CASES[name]
    states, orbits = SC.states_and_orbits(name)
    n_base, n_copies = len(SC.bases(name)), len(SC.copies(name))
    kept, _dropped = SC.twins(name)
    arr = view_array(name)
    ref = list(range(n_base)) + [b for b, _p, _t in SC.copies(name)] + [b for b, _tw in kept]
    with checker(m) as ck:
        _keys, same = ck.state_keys(arr, ref)
        assert same[:n_base] == [1] * n_base
        for x, (b, p, t) in enumerate(SC.copies(name)):
            assert same[n_base + x] == 1, (name, b, p, states[b], t)
        for x, (b, tw) in enumerate(kept):
            assert same[n_base + n_copies + x] == 0, (name, b, states[b], tw)
        # drawn pairs: half of them inside one orbit's images, half anywhere
        rng = random.Random(15000 + sorted(SC.CASES).index(name))
        pairs = []
        for _ in range(100):
            b, p, _t = SC.copies(name)[rng.randrange(n_copies)]
            others = [n_base + x for x, (b2, _p2, _t2) in enumerate(SC.copies(name)) if b2 == b]
            pairs.append((rng.choice(others), rng.choice(others + [b])))
        pairs += [(rng.randrange(len(states)), rng.randrange(len(states))) for _ in range(100)]
        ref2 = list(range(len(states)))
        for i, j in pairs:
            ref2[i] = j  # (a later pair with the same i replaces an earlier one)
        _keys, same2 = ck.state_keys(arr, ref2)
        want = [int(orbits[i] == orbits[ref2[i]]) for i in range(len(states))]
        assert sum(want) > n_base and sum(want) < len(states)
        for i in range(len(states)):
            assert same2[i] == want[i], (name, i, ref2[i], states[i], states[ref2[i]])
    with checker(m, symmetry=False) as ck:
        _keys, same = ck.state_keys(arr, ref)
        assert same[:n_base] == [1] * n_base
        moved = 0
        for x, (b, p, t) in enumerate(SC.copies(name)):
            assert same[n_base + x] == int(t == states[b]), (name, b, p, states[b], t)
            moved += t != states[b]
        assert moved >= n_copies // 2
        assert same[n_base + n_copies:] == [0] * len(kept)


def test_state_keys_refuses_bad_arguments(monkeypatch):
    """RMC_E_INVAL with the reason for a wide ctx, a NULL array with n > 0, a ref
    entry not below n and a view the encoder refuses; n = 0 is accepted (nothing to
    launch)."""
    m = SC.CASES["sym_s3k4"]
    ok = to_view(m, R.init_state(m))
    for symmetry in (True, False):
        with checker(m, symmetry) as ck:
            assert ck.state_keys([]) == []
            assert ck.state_keys([], []) == ([], [])
            assert ck.lib.rmc_state_keys(ck.ctx, None, 0, None, None, None) == 0
            keys, same = ck.state_keys([ok, ok], [1, 0])
            assert keys[0] == keys[1] and same == [1, 1]
            arr = (rmc.StateView * 1)(ok)
            out = (C.c_uint64 * 1)()
            ref = (C.c_uint32 * 1)(0)
            same = (C.c_uint8 * 1)()
            assert ck.lib.rmc_state_keys(ck.ctx, None, 1, out, None, None) == -22
            assert b"NULL" in ck.lib.rmc_last_error(ck.ctx)
            assert ck.lib.rmc_state_keys(ck.ctx, arr, 1, None, None, None) == -22
            assert ck.lib.rmc_state_keys(ck.ctx, arr, 1, out, ref, None) == -22
            assert b"NULL" in ck.lib.rmc_last_error(ck.ctx)
            assert ck.lib.rmc_state_keys(ck.ctx, arr, 1, out, ref, same) == 0
            with pytest.raises(rmc.RmcError) as e:
                ck.state_keys([ok, ok], [0, 2])
            assert e.value.code == -22 and "ref[1]" in str(e.value)
            bad = to_view(m, R.init_state(m))
            bad.currentTerm[1] = 256
            with pytest.raises(rmc.RmcError) as e:
                ck.state_keys([ok, bad])
            assert e.value.code == -22 and "state 1: currentTerm" in str(e.value)
            other = to_view(R.Model(n_servers=2), R.init_state(R.Model(n_servers=2)))
            with pytest.raises(rmc.RmcError) as e:
                ck.state_keys([other])
            assert e.value.code == -22 and "n_servers" in str(e.value)
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    with checker(m, symmetry=False) as ck:
        with pytest.raises(rmc.RmcError) as e:
            ck.state_keys([ok])
        assert e.value.code == -22 and "packed layout" in str(e.value)
        assert ck.lib.rmc_state_keys(ck.ctx, None, 0, None, None, None) == -22
