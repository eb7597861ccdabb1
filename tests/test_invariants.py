"""The device invariant predicates against the oracle, state by state
(rmc_check_states): the packed check_invariants<S, K> of every shape, and on the
wide layout both wcheck_invariants (one thread per state, the BFS's check) and
w_check_invariants_wave (one wave per state, the wave simulator's).

The BFS goldens only show the predicates where they hold, and one bug model per
invariant shows one violating state each.  Here every predicate is compared with
oracle.raft_spec.INVARIANTS on the same states (tests/invariant_cases.py: per
model 600 uniform states and 600 of near_invariant_state, so that both verdicts
of every invariant occur), alone and in first-violated order, on all S = 2..5,
both bag sizes, |Value| 1 and 2, and past the packed capacity (logs of 8 and 32
entries, terms to 255, 20 and 64 messages).  tests/test_invariants_native.py runs
the same comparison on the host compilation of the same predicates."""
import ctypes as C
import functools
import json
import os

import pytest

import rmc
from oracle import raft_spec as R
from tests import invariant_cases as IC
from tests.convert import from_view, to_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_levels.json")))
# the layout and, on the wide one, the check (RMC_WSIM: 0 the thread's, 1 the wave's)
LAYOUTS = {"packed": (False, None), "wide_thread": (True, "0"), "wide_wave": (True, "1")}


def checker(model, layout, monkeypatch, invariants=IC.ALL):
    wide, wsim = LAYOUTS[layout]
    monkeypatch.setenv("RMC_FORCE_WIDE", "1" if wide else "0")
    if wsim is not None:
        monkeypatch.setenv("RMC_WSIM", wsim)
    cfg = rmc.make_config(n_servers=model.n_servers, n_values=model.n_values, max_term=model.max_term,
                          max_log_len=model.max_log, max_msgs=model.max_msgs, max_dup=model.max_dup,
                          invariants=invariants, max_depth=1, state_capacity=1 << 12)
    ck = rmc.Checker(cfg)
    assert (rmc.native().rmc_state_bytes(C.byref(cfg)) >= 336) == wide  # the layout asked for
    return ck


@functools.lru_cache(maxsize=None)
def view_array(name):
    m, _ = IC.CASES[name]
    views = [to_view(m, s) for s in IC.states(name)]
    return (rmc.StateView * len(views))(*views)


def layouts_of(name):
    return ("wide_thread", "wide_wave") if name.startswith("wide") or name == "typeok_wide" else tuple(LAYOUTS)


@pytest.mark.parametrize("name,layout", [(n, lay) for n in sorted(IC.CASES) for lay in layouts_of(n)])
def test_device_predicates_equal_the_oracle_state_by_state(name, layout, monkeypatch):
    """On the model's 1,200 states: with each single RMC_INV_* bit as the mask,
    violated[t] is that bit exactly where the oracle's predicate is false, else 0;
    with all ten bits it is the lowest bit the oracle finds violated (the
    first-violated order of rmc_result.violated_inv, on every state).  The inputs
    show both verdicts of every invariant at least 10 times (ONE_SIDED lists the
    pairs where one is impossible)."""
    IC.check_mixed_verdicts(name)
    m, _ = IC.CASES[name]
    states, want = IC.states(name), IC.verdicts(name)
    arr = view_array(name)
    with checker(m, layout, monkeypatch) as ck:
        for b in IC.BITS:
            got = ck.check_states(arr, b)
            for t, (g, w) in enumerate(zip(got, want)):
                assert g == (w & b), "%s alone on state %d: device %d, oracle %s\n%r" % (
                    R.INV_BITS[b], t, g, "violated" if w & b else "holds", states[t])
        got = ck.check_states(arr, IC.ALL)
        for t, (g, w) in enumerate(zip(got, want)):
            assert g == (w & -w), "first violated of state %d: device %d, oracle %d\n%r" % (t, g, w & -w, states[t])
        assert ck.check_states(arr, 0) == got  # mask 0: the ctx's own, here all ten


@pytest.mark.parametrize("name,layout", [(n, lay) for n in sorted(IC.TYPEOK) for lay in layouts_of(n)])
def test_typeok_sees_entry_values_outside_value(name, layout, monkeypatch):
    """|Value| = 1: an entry of value 1 in a server's log, in an
    AppendEntriesRequest's mentries or in a RequestVoteResponse's mlog (the type
    errors a view can carry) is reported as TypeOK, alone and with all ten
    invariants named; the same state with the value 0 is not."""
    m = IC.TYPEOK[name]
    cases = IC.typeok_states(name)
    assert {p for p, _b, _g in cases} == set(IC.TYPEOK_PLACES)
    with checker(m, layout, monkeypatch) as ck:
        bad = [to_view(m, b) for _p, b, _g in cases]
        good = [to_view(m, g) for _p, _b, g in cases]
        for mask in (rmc.INV_TYPEOK, IC.ALL):
            for (place, b, _g), v in zip(cases, ck.check_states(bad, mask)):
                assert v == rmc.INV_TYPEOK, (place, mask, v, b)
        for (place, _b, g), v in zip(cases, ck.check_states(good, rmc.INV_TYPEOK)):
            assert v == 0, (place, v, g)
        want = [IC.oracle_bits(m, g) for _p, _b, g in cases]
        assert ck.check_states(good, IC.ALL) == [w & -w for w in want]


@pytest.mark.parametrize("name", ["bug_leader_votes", "bug_quorum_log", "bug_leader_complete"])
def test_check_states_agrees_with_the_search_on_its_counterexample(name, monkeypatch):
    """The hook and the BFS agree: on the counterexample of a bug model,
    rmc_check_states reports the violated invariant on the last state and nothing
    on every earlier one, on the packed layout and with both wide checks."""
    g = GOLDEN[name]
    p = g["params"]
    monkeypatch.setenv("RMC_FORCE_WIDE", "0")
    cfg = rmc.make_config(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"],
                          max_log_len=p["max_log_len"], max_msgs=p["max_msgs"], max_dup=p["max_dup"],
                          bug_quorum=bool(p["bug_quorum"]), invariants=p["invariants"],
                          state_capacity=int(g["distinct"] * 1.25) + (1 << 16))
    with rmc.Checker(cfg) as ck:
        res = ck.run()
        assert res.violated_inv == g["violated_inv"] and res.violation_depth == g["violation_depth"]
        views = [v for _f, _i, v in ck.trace()]
        want = [0] * (len(views) - 1) + [g["violated_inv"]]
        assert ck.check_states(views) == want  # mask 0: the invariant the search checked
    model = R.Model(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"], max_log=p["max_log_len"],
                    max_msgs=p["max_msgs"], max_dup=p["max_dup"])
    assert [IC.oracle_bits(model, from_view(v)) & g["violated_inv"] for v in views] == want
    for layout in ("wide_thread", "wide_wave"):
        with checker(model, layout, monkeypatch, invariants=p["invariants"]) as ck:
            assert ck.check_states(views) == want
            assert ck.check_states(views, g["violated_inv"]) == want


def test_check_states_refuses_bad_arguments(monkeypatch):
    """RMC_E_INVAL with the reason for a mask bit above RMC_INV_LEADER_COMPLETE, a
    NULL array with n > 0 and a view the layout's encoder refuses; n = 0 is
    accepted (nothing to launch)."""
    m = IC.CASES["fuzz0"][0]
    ok = to_view(m, R.init_state(m))
    for layout in ("packed", "wide_wave"):
        with checker(m, layout, monkeypatch) as ck:
            assert ck.check_states([]) == []
            assert ck.lib.rmc_check_states(ck.ctx, None, 0, 0, None) == 0
            assert ck.check_states([ok]) == [0]
            with pytest.raises(rmc.RmcError) as e:
                ck.check_states([ok], 1 << 10)
            assert e.value.code == -22 and "invariant bit" in str(e.value)
            out = (C.c_int32 * 1)()
            assert ck.lib.rmc_check_states(ck.ctx, None, 1, 0, out) == -22
            assert b"NULL" in ck.lib.rmc_last_error(ck.ctx)
            arr = (rmc.StateView * 1)(ok)
            assert ck.lib.rmc_check_states(ck.ctx, arr, 1, 0, None) == -22
            bad = to_view(m, R.init_state(m))
            bad.currentTerm[1] = 256  # beyond both layouts
            with pytest.raises(rmc.RmcError) as e:
                ck.check_states([ok, bad])
            assert e.value.code == -22 and "state 1: currentTerm" in str(e.value)
            other = to_view(R.Model(n_servers=2), R.init_state(R.Model(n_servers=2)))
            with pytest.raises(rmc.RmcError) as e:
                ck.check_states([other])
            assert e.value.code == -22 and "n_servers" in str(e.value)
