"""Action properties on the GPU (rmc.h "action properties"): PROPERTY [][A]_vars of the model,
compiled by the front-end to two-state bytecode and evaluated by the device interpreter (k_act
over the parents of every expansion launch, k_act_eval on caller pairs).  The properties, their
Python twins, the model files and the pairs are tests/action_cases.py.  Everything expected
comes from oracle/raft_spec.py."""
import ctypes as C
import functools
import os
import subprocess

import pytest

import rmc
from oracle import raft_spec as R
from tests import action_cases as AC
from tests import graph_cases as G
from tests import invariant_cases as IC
from tests.convert import from_view, to_view
from tests.test_actions_native import build_act_check, host_verdicts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
SPECS = os.path.join(ROOT, "specs")


@pytest.fixture(scope="module")
def act_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("act_check_gpu") / "act_check"
    build_act_check(exe)
    return str(exe)


def load(tmp_path, names, **kw):
    """(Config, Actions) of ActCases with the PROPERTY names `names`."""
    cfg_path, tla = AC.write_model(tmp_path, names, **kw)
    cfg, _notes, _preds, acts = rmc.load_model(cfg_path, tla, builtin_raft=True, actions=True)
    assert acts.names == list(names)
    return cfg, acts


def bounds(params):
    return dict(n_servers=params["n_servers"], n_values=params["n_values"], max_term=params["max_term"],
                max_log=params["max_log_len"], max_msgs=params["max_msgs"], max_dup=params["max_dup"])


def model_of(params):
    return R.Model(**bounds(params))


@pytest.mark.parametrize("group", sorted(AC.GROUPS))
@pytest.mark.parametrize("name,K", AC.SHAPES, ids=["%s-K%d" % s for s in AC.SHAPES])
def test_eval_actions_equals_twins_and_host_vm_on_packed_shapes(name, K, group, act_check, tmp_path):
    m, _ = IC.CASES[name]
    names = AC.GROUPS[group]
    _cfg, acts = load(tmp_path, names, n_servers=m.n_servers, n_values=m.n_values)
    cfg = rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, max_term=m.max_term, max_log_len=m.max_log,
                          max_msgs=5 if K == 8 else 4, max_dup=m.max_dup, state_capacity=1 << 12)
    pairs = [(to_view(m, s), to_view(m, t)) for s, t in AC.pairs(name, K)]
    with rmc.Checker(cfg) as ck:
        assert ck.lib.rmc_state_bytes(C.byref(cfg)) == (2 * m.n_servers + K) * 4
        ck.set_actions(acts)
        got = ck.eval_actions(pairs)
        assert got == list(AC.verdicts(name, K, group))
        assert got == host_verdicts(act_check, tmp_path, name, K, group)
        assert ck.eval_actions([]) == []


# ---- the BFS pass ---------------------------------------------------------------------------
HOLDING = ("TermsMonotonic", "LeaderAppendOnly", "VoteOncePerTerm", "MsgsGrowByOne")
VARIANTS = {"resident": {}, "symmetry": dict(symmetry=True), "spill": dict(spill=True, device_window=4096),
            "verify": dict(verify_states=True), "coverage": dict(coverage=True)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_properties_that_hold_change_no_count(variant, tmp_path):
    kw = VARIANTS[variant]
    _cfg, acts = load(tmp_path, HOLDING, symmetry=kw.get("symmetry", False), **bounds(G.TINY2))
    out = []
    for with_acts in (False, True):
        with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2, **kw)) as ck:
            if with_acts:
                ck.set_actions(acts)
            res = ck.run()
            out.append((res.distinct, res.generated, res.depth, res.violated_inv, res.left_on_queue))
            if with_acts:
                with pytest.raises(rmc.RmcError) as e:
                    ck.action_violation()
                assert e.value.code == -71
    assert out[0] == out[1] and out[0][3] == 0
    if variant != "symmetry":
        assert out[0][0] == G.CASES["tiny2"].distinct == 12975
    ref = oracle_bfs(variant == "symmetry")
    assert out[1][:3] == (ref.distinct, ref.generated, ref.depth)


@functools.lru_cache(maxsize=None)
def oracle_bfs(symmetry):
    return R.bfs(model_of(G.TINY2), invariants=(), symmetry=symmetry)


@functools.lru_cache(maxsize=None)
def oracle_depth(name, symmetry=False):
    return AC.oracle_violation(model_of(G.TINY2), name, symmetry=symmetry)


def check_action_trace(model, trace, name, depth):
    """The trace is a behaviour of the spec from Init, of `depth` states; its last step alone does
    not satisfy [A]_vars of `name`."""
    assert len(trace) == depth
    states = [from_view(v) for _f, _i, v in trace]
    assert states[0] == R.init_state(model) and trace[0][0] == -1
    for a, b, (fam, _inst, _v) in zip(states, states[1:], trace[1:]):
        assert (rmc.FAMILIES[fam], b) in {(f, t) for f, _p, t in R.successors(model, a)}
        assert R.in_constraint(model, b)
    assert AC.expected(name, model, states[-2], states[-1]) != AC.HOLDS
    assert all(AC.expected(name, model, a, b) == AC.HOLDS for a, b in zip(states[:-2], states[1:-1]))


@pytest.mark.parametrize("variant", ["resident", "spill", "verify"])
@pytest.mark.parametrize("name", ["CandStays", "CommitMonotonic"])
def test_violated_property_is_reported_with_its_transition(name, variant, tmp_path):
    model = model_of(G.TINY2)
    names = ("TermsMonotonic", name)  # the first holds everywhere: property 1 is the violated one
    _cfg, acts = load(tmp_path, names, **bounds(G.TINY2))
    want = oracle_depth(name)
    assert want is not None and want >= 3
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2, **VARIANTS[variant])) as ck:
        ck.set_actions(acts)
        res = ck.run()
        assert res.violated_inv == rmc.ACT_USER0 << 1 and acts.name_of(res.violated_inv) == name
        assert res.violation_depth == want and not res.deadlock
        assert not ck.predicate_error()
        trace = ck.trace()
        check_action_trace(model, trace, name, want)
        hit = ck.action_violation()
        assert hit["property"] == 1 and hit["name"] == name and not hit["is_error"]
        assert (hit["family"], hit["instance"]) == (trace[-1][0], trace[-1][1])
        starts = ck.levels() if variant == "resident" else None
        if starts:  # the source is a state of level violation_depth - 1
            assert starts[want - 2] <= hit["src_index"] < starts[want - 1]
            src = ck.read_states(hit["src_index"], 1)
            assert from_view(src[0]) == from_view(trace[-2][2])
        ck.set_actions(None)
        assert ck.lib.rmc_eval_actions(ck.ctx, None, None, 0, None) == -71


def test_violated_property_under_symmetry(tmp_path):
    """Stored representatives to raw successors: the trace's steps are steps of Next up to a
    permutation of Server, and its last step violates the property."""
    model = model_of(G.TINY2)
    _cfg, acts = load(tmp_path, ("CommitMonotonic",), symmetry=True, **bounds(G.TINY2))
    want = oracle_depth("CommitMonotonic", True)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, symmetry=True, **G.TINY2)) as ck:
        ck.set_actions(acts)
        res = ck.run()
        assert res.violated_inv == rmc.ACT_USER0 and res.violation_depth == want
        trace = ck.trace()
        assert len(trace) == want
        a, b = from_view(trace[-2][2]), from_view(trace[-1][2])
        assert (rmc.FAMILIES[trace[-1][0]], b) in {(f, t) for f, _p, t in R.successors(model, a)}
        assert AC.expected("CommitMonotonic", model, a, b) == AC.VIOLATED


def test_evaluation_error_is_reported_as_an_error(tmp_path):
    _cfg, acts = load(tmp_path, ("TermsMonotonic", "UnguardedNext"), **bounds(G.TINY2))
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2)) as ck:
        ck.set_actions(acts)
        res = ck.run()
        # every successor of Init has an empty log: the first transition of the search
        assert res.violated_inv == rmc.ACT_USER0 << 1 and res.violation_depth == 2
        hit = ck.action_violation()
        assert hit["is_error"] and hit["src_index"] == 0 and hit["instance"] == 0 and hit["property"] == 1
        trace = ck.trace()
        assert len(trace) == 2 and from_view(trace[0][2]) == R.init_state(model_of(G.TINY2))


def test_invariant_violated_in_the_same_level_wins(tmp_path):
    """NoLeaderKept is violated by the transition into the first state with a leader, which
    violates the model-defined invariant UserNoLeader: found in the same level, the invariant
    is reported exactly as without properties."""
    cfg_path, tla = AC.write_model(tmp_path, ("NoLeaderKept",), invariants=("UserNoLeader",), **bounds(G.TINY2))
    _cfg, _notes, preds, acts = rmc.load_model(cfg_path, tla, builtin_raft=True, predicates=True, actions=True)
    assert preds.names == ["UserNoLeader"] and acts.names == ["NoLeaderKept"]
    out = {}
    for which in ("invariant", "both", "property"):
        with rmc.Checker(rmc.make_config(state_capacity=1 << 16, invariants=0, **G.TINY2)) as ck:
            if which != "property":
                ck.set_predicates(preds)
            if which != "invariant":
                ck.set_actions(acts)
            res = ck.run()
            out[which] = (res.violated_inv, res.violation_depth, res.distinct, res.generated,
                          [from_view(v) for _f, _i, v in ck.trace()])
    assert out["both"] == out["invariant"] and out["both"][0] == rmc.INV_USER0
    assert out["property"][0] == rmc.ACT_USER0 and out["property"][1] == out["invariant"][1]
    assert out["property"][1] == oracle_depth("NoLeaderKept")


_KEEP = []


def transport():
    def alltoallv(_u, send, send_bytes, recv, _recv_bytes):
        C.memmove(recv, send, send_bytes[0])
        return 0

    def allgather(_u, send, nbytes, recv):
        C.memmove(recv, send, nbytes)
        return 0
    tr = rmc.Transport(None, rmc.ALLTOALLV_FN(alltoallv), rmc.ALLGATHER_FN(allgather))
    _KEEP.append(tr)
    return tr


def test_refusals(tmp_path, monkeypatch):
    b = bounds(G.TINY2)
    _cfg, acts = load(tmp_path, ("TermsMonotonic",), **b)
    _cfg, named = load(tmp_path, ("NamesR1",), **b)
    _cfg, three = load(tmp_path, ("TermsMonotonic",), **dict(b, n_servers=3))
    resid = "Resid == \\A i \\in Server : state[i] /= Leader"
    cfg_path, tla = AC.write_model(tmp_path, (), module=AC.module_with(resid), extra="CONSTRAINT Resid\n", **b)
    cons = rmc.load_model(cfg_path, tla, builtin_raft=True, constraints=True)[3]
    assert len(cons) == 1
    cfg_path, tla = AC.write_model(tmp_path, (), invariants=("UserNoLeader",), **b)
    preds = rmc.load_model(cfg_path, tla, builtin_raft=True, predicates=True)[2]

    def refused(call, code, *needles):
        with pytest.raises(rmc.RmcError) as e:
            call()
        assert e.value.code == code and all(n in str(e.value) for n in needles), str(e.value)

    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, continue_=True, **G.TINY2)) as ck:
        refused(lambda: ck.set_actions(acts), -22, "RMC_FLAG_CONTINUE")
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, symmetry=True, **G.TINY2)) as ck:
        refused(lambda: ck.set_actions(named), -22, "server model value", "SYMMETRY")
        ck.set_actions(acts)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2)) as ck:
        refused(lambda: ck.set_predicates(acts), -22, "not a program of rmc_predicates_from_files")
        refused(lambda: ck.set_actions(preds), -22, "not a program of rmc_actions_from_files")
        ck.set_actions(named)  # without SYMMETRY the one that names a server is accepted
        refused(lambda: ck.set_actions(three), -22, "3 servers", "the ctx has 2")
        refused(lambda: ck.set_constraints(cons), -22, "action properties are set")
        for call, code in ((lambda: ck.simulate(behaviours=8, depth=4, smoke_k=0), -71),
                           (lambda: ck.checkpoint(str(tmp_path / "ck")), -71),
                           (lambda: ck.recover(str(tmp_path / "ck")), -71),
                           (lambda: ck.shard(0, 1, transport=transport(), keys_per_dest=1 << 12,
                                             sent_cache_slots=1 << 12), -22)):
            refused(call, code, "action properties")
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2)) as ck:
        ck.set_constraints(cons)
        refused(lambda: ck.set_actions(acts), -22, "model-defined constraints are set")
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2)) as ck:
        ck.shard(0, 1, transport=transport(), keys_per_dest=1 << 12, sent_cache_slots=1 << 12)
        refused(lambda: ck.set_actions(acts), -22, "sharded")
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    with rmc.Checker(rmc.make_config(state_capacity=1 << 12, max_depth=6, **G.TINY2)) as ck:
        refused(lambda: ck.set_actions(acts), -22, "wide layout")


# ---- rmc-tlc ----------------------------------------------------------------------------------
def test_cli_reports_the_violated_property_and_its_final_action(tmp_path):
    tla = os.path.join(SPECS, "actions", "MCraftActions.tla")
    text = open(os.path.join(SPECS, "actions", "MCraftActions.cfg")).read()
    assert "\\* PROPERTY CommitMonotonic" in text
    cfg = tmp_path / "MCraftActions.cfg"
    cfg.write_text(text.replace("\\* PROPERTY CommitMonotonic", "PROPERTY CommitMonotonic"))
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536", "-config", str(cfg), tla], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 12, r.stdout + r.stderr
    out = r.stdout
    assert "Compiled action properties: TermsMonotonic, LeaderAppendOnly, VoteOncePerTerm, CommitMonotonic" in out
    assert "PROPERTY CommitMonotonic: action property [][A]_vars" in out
    assert "Error: Action property CommitMonotonic is violated." in out
    assert "Error: The behavior up to this point is:" in out
    want = oracle_depth("CommitMonotonic")
    headers = [ln for ln in out.splitlines() if ln.startswith("State ")]
    assert len(headers) == want and headers[0] == "State 1: <Initial predicate>"
    assert headers[-1].startswith("State %d: <Restart line " % want) and headers[-1].endswith("of module raft>")


def test_cli_holding_properties_and_refusals(tmp_path):
    tla = os.path.join(SPECS, "actions", "MCraftActions.tla")
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536", tla], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Compiled action properties: TermsMonotonic, LeaderAppendOnly, VoteOncePerTerm" in r.stdout
    assert "Model checking completed. No error has been found." in r.stdout
    assert "12975 distinct states found" in r.stdout
    for flag in (["-continue"], ["-gpus", "2"], ["-simulate"], ["-checkpoint", "x.ck"], ["-recover", "x.ck"]):
        r = subprocess.run([CLI, "-builtin-raft"] + flag + [tla], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "PROPERTY TermsMonotonic is an action property" in r.stdout, r.stdout
        assert flag[0] in r.stdout


def test_cli_prints_an_evaluation_error_of_its_own(tmp_path):
    cfg_path, tla = AC.write_model(tmp_path, ("UnguardedNext",), **bounds(G.TINY2))
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536", "-config", cfg_path, tla], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Error: Evaluating action property UnguardedNext failed" in r.stdout
    assert "is violated" not in r.stdout
