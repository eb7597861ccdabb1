"""The wide layout's device SYMMETRY keys and orbit comparison against the oracle,
state by state, through the C ABI on a wide ctx: wcanon and wsame_orbit / wsame through
rmc_state_keys (k_wkeys; a wide ctx under SYMMETRY), the successor's canonical key through
rmc_expand (k_wlist).

Inputs: (a) every case of tests/symmetry_cases.py on a wide ctx of its own bounds
(RMC_FORCE_WIDE=1); (b) tests/wide_symmetry_cases.py on real wide bounds — states past
the packed capacity from random walks, tie-heavy states and their twins, S = 3 and 5.
Same orbit, same key; another orbit, another key.  tests/test_wide_symmetry_native.py
runs the same comparison on the host compilation of the same functions."""
import functools
import random

import pytest

import rmc
from oracle import raft_spec as R
from tests import symmetry_cases as SC
from tests import wide_symmetry_cases as WC
from tests.convert import from_view, to_view
from tests.test_gpu import compare_expand
from tests.test_symmetry import assert_partition

pytestmark = pytest.mark.gpu

ALL = sorted(SC.CASES) + WC.CASES


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)


def model_of(name):
    return SC.CASES[name] if name in SC.CASES else WC.model_of(name)


def expand_model(name):
    """The model compare_expand filters by: the case's own (a); the ctx's bounds (b), which
    no successor of the case's states exceeds."""
    if name in SC.CASES:
        return SC.CASES[name]
    m, b = WC.model_of(name), WC.CTX_BOUNDS
    return R.Model(n_servers=m.n_servers, n_values=m.n_values, max_term=b["max_term"], max_log=b["max_log_len"],
                   max_msgs=b["max_msgs"], max_dup=b["max_dup"])


def checker(name, symmetry=True):
    """A wide ctx: of the case's own bounds (a), of real wide bounds (b)."""
    m = model_of(name)
    b = (dict(max_term=m.max_term, max_log_len=m.max_log, max_msgs=m.max_msgs, max_dup=m.max_dup)
         if name in SC.CASES else WC.CTX_BOUNDS)
    # (b): under a depth bound, as the wide layout runs SYMMETRY on bounds past the packed capacity
    cfg = rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, symmetry=symmetry, state_capacity=1 << 12,
                          max_depth=0 if name in SC.CASES else 1, **b)
    assert rmc.native().rmc_state_bytes(cfg) in (336, 904, 5080)  # a wide record
    return rmc.Checker(cfg)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(states, orbit numbers, index of every state's original, surviving twins, base states)"""
    mod = SC if name in SC.CASES else WC
    states, orbits = mod.states_and_orbits(name)
    kept, _dropped = mod.twins(name)
    n_base = len(mod.bases(name))
    ref = list(range(n_base)) + [b for b, _p, _t in mod.copies(name)] + [b for b, _tw in kept]
    return states, orbits, ref, kept, n_base


@functools.lru_cache(maxsize=None)
def view_array(name):
    m = model_of(name)
    views = [to_view(m, s) for s in inputs(name)[0]]
    return (rmc.StateView * len(views))(*views)


def expanded(name):
    """(states to expand, {successor: orbit key})"""
    if name in SC.CASES:
        return list(SC.expand_inputs(name)), SC.successor_orbits(name)
    return [s for _b, _p, s in WC.expand_inputs(name)], WC.successor_orbits(name)


def not_vacuous(name):
    if name in SC.CASES:
        WC.check_packed_case_not_vacuous(name)
    else:
        WC.check_not_vacuous(name)


@pytest.mark.parametrize("name", ALL)
def test_state_keys_are_orbit_invariants(name):
    """rmc_state_keys (wcanon) on the base states, their copies and the twins that left
    their orbit: one key exactly where the oracle has one orbit; in particular every
    surviving twin's key differs from its original's."""
    not_vacuous(name)
    states, orbits, _ref, kept, _n_base = inputs(name)
    with checker(name) as ck:
        keys = ck.state_keys(view_array(name))
    assert_partition(keys, orbits, (name, states))
    first_twin = len(states) - len(kept)
    for x, (b, tw) in enumerate(kept):
        assert states[first_twin + x] == tw
        assert keys[first_twin + x] != keys[b], (name, b, states[b], tw)


@pytest.mark.parametrize("name", ALL)
def test_same_orbit_equals_the_oracle(name):
    """Verification's comparison through rmc_state_keys' ref (wsame_orbit): every copy
    is its original's orbit, no surviving twin is, 200 drawn pairs of states are one
    orbit exactly when the oracle says so."""
    states, orbits, ref, kept, n_base = inputs(name)
    n = len(states)
    n_twins = len(kept)
    arr = view_array(name)
    with checker(name) as ck:
        _keys, same = ck.state_keys(arr, ref)
        assert same[:n - n_twins] == [1] * (n - n_twins)
        assert same[n - n_twins:] == [0] * n_twins
        rng = random.Random(25000 + ALL.index(name))
        ref2 = list(range(n))
        for _ in range(100):  # inside one orbit's images
            i = rng.randrange(n_base, n - n_twins)
            ref2[i] = rng.choice([j for j in range(n - n_twins) if ref[j] == ref[i]])
        for _ in range(100):  # anywhere
            ref2[rng.randrange(n)] = rng.randrange(n)
        _keys, same2 = ck.state_keys(arr, ref2)
        want = [int(orbits[i] == orbits[ref2[i]]) for i in range(n)]
        assert sum(want) < n
        assert same2 == want, [(i, ref2[i]) for i in range(n) if same2[i] != want[i]][:5]


@pytest.mark.parametrize("name", ALL)
def test_successor_keys_partition_successors_into_orbits(name):
    """rmc_expand under SYMMETRY on a wide ctx: the per-lane successor multisets equal
    the oracle's (compare_expand), the fingerprint of every returned successor is
    rmc_state_keys of its view, and over all successors of the case two have one
    fingerprint exactly when the oracle puts them in one orbit."""
    m = expand_model(name)
    states, want = expanded(name)
    with checker(name) as ck:
        fps, out = compare_expand(m, states, symmetry=True, ck=ck)
        out = [sv for sv in out if sv.in_constraint]
        keys = ck.state_keys([sv.state for sv in out])
    assert set(fps) == set(want)
    succ = sorted(fps, key=repr)
    assert_partition([fps[t] for t in succ], [want[t] for t in succ], (name, succ))
    assert len(out) >= len(want)
    for sv, k in zip(out, keys):
        assert k == sv.fingerprint, (name, sv.parent, sv.instance, from_view(sv.state))
    several = {}
    for t in succ:
        several.setdefault(want[t], set()).add(t)
    assert sum(1 for v in several.values() if len(v) >= 2) >= 50


def test_state_keys_on_a_wide_ctx_checks_its_arguments():
    """A wide ctx under SYMMETRY is accepted; a NULL array with n > 0, a ref entry not
    below n and a view the encoder refuses are RMC_E_INVAL with the reason; n = 0
    launches nothing.  A wide ctx without SYMMETRY stays refused (tests/test_symmetry.py)."""
    m = SC.CASES["sym_s3k4"]
    ok = to_view(m, R.init_state(m))
    with checker("sym_s3k4", symmetry=False) as ck:
        with pytest.raises(rmc.RmcError) as e:
            ck.state_keys([ok])
        assert e.value.code == -22 and "RMC_FLAG_SYMMETRY" in str(e.value)
    for symmetry in (True,):
        with checker("sym_s3k4", symmetry) as ck:
            assert ck.state_keys([]) == []
            assert ck.lib.rmc_state_keys(ck.ctx, None, 0, None, None, None) == 0
            keys, same = ck.state_keys([ok, ok], [1, 0])
            assert keys[0] == keys[1] and same == [1, 1]
            assert ck.lib.rmc_state_keys(ck.ctx, None, 1, None, None, None) == -22
            with pytest.raises(rmc.RmcError) as e:
                ck.state_keys([ok, ok], [0, 2])
            assert e.value.code == -22 and "ref[1]" in str(e.value)
            other = to_view(R.Model(n_servers=2), R.init_state(R.Model(n_servers=2)))
            with pytest.raises(rmc.RmcError) as e:
                ck.state_keys([other])
            assert e.value.code == -22 and "state 0" in str(e.value)
