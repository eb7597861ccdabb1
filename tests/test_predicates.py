"""Model-defined invariants on the GPU (rmc.h "model-defined invariants"): predicates of
the model's own, compiled by the front-end to bytecode and evaluated by the device
interpreter (k_pred / k_wpred after every expansion launch, k_pred_eval / k_wpred_eval on
caller states).  The predicates, their Python twins and the model files are
tests/predicate_cases.py; the states are those of the invariant tests
(tests/invariant_cases.py).  Everything expected comes from oracle/raft_spec.py."""
import ctypes as C
import os
import subprocess

import pytest

import rmc
from oracle import raft_spec as R
from tests import graph_cases as G
from tests import invariant_cases as IC
from tests import predicate_cases as PC
from tests.convert import from_view, to_view
from tests.test_predicates_native import build_pred_check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
SPECS = os.path.join(ROOT, "specs")

# (model of invariant_cases, bag slots K of the ctx): every packed shape, S = 2..5 x K = 4, 8.
# A ctx of K = 8 takes the states of a model with fewer messages as they are; the S = 5
# models have up to 6 or 8 messages, so the K = 4 ctx gets their states of at most 4.
SHAPES = [("fuzz2", 4), ("fuzz2", 8), ("fuzz0", 4), ("fuzz1", 8), ("edge0", 8), ("fuzz3", 4), ("edge3", 8),
          ("fuzz4", 4), ("fuzz4", 8), ("edge1", 8)]


def test_shapes_cover_every_packed_shape():
    assert {(IC.CASES[n][0].n_servers, k) for n, k in SHAPES} == {(s, k) for s in (2, 3, 4, 5) for k in (4, 8)}


@pytest.fixture(scope="module")
def pred_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pred_check_gpu") / "pred_check"
    build_pred_check(exe)
    return str(exe)


def load(tmp_path, names, model=None, **kw):
    """(Config, Predicates) of PredCases with the INVARIANTs `names`."""
    if model is not None:
        kw.update(n_servers=model.n_servers, n_values=model.n_values)
    cfg_path, tla = PC.write_model(tmp_path, names, **kw)
    cfg, _notes, preds = rmc.load_model(cfg_path, tla, builtin_raft=True, predicates=True)
    assert preds.names == list(names) and cfg.invariants == 0
    return cfg, preds


def host_vm(pred_check, tmp_path, names, model, states, K):
    """The host interpreter's verdicts (tests/native/pred_check.cpp) on the same states."""
    cfg_path, tla = PC.write_model(tmp_path, names, n_servers=model.n_servers, n_values=model.n_values)
    views, out = tmp_path / "views.bin", tmp_path / "host.bin"
    with open(views, "wb") as f:
        for s in states:
            f.write(bytes(to_view(model, s)))
    r = subprocess.run([pred_check, cfg_path, tla, str(views), str(model.n_servers), str(K), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    raw = out.read_bytes()
    return [tuple(raw[t * len(names):(t + 1) * len(names)]) for t in range(len(states))]


@pytest.mark.parametrize("group", sorted(PC.GROUPS))
@pytest.mark.parametrize("name,K", SHAPES, ids=["%s-K%d" % s for s in SHAPES])
def test_eval_predicates_equals_twins_and_host_vm_on_packed_shapes(name, K, group, pred_check, tmp_path):
    m, _ = IC.CASES[name]
    names = PC.GROUPS[group]
    keep = [t for t, s in enumerate(IC.states(name)) if len(s.messages) <= K]
    assert len(keep) >= 100
    states = [IC.states(name)[t] for t in keep]
    want = [PC.verdicts(name, group)[t] for t in keep]
    _cfg, preds = load(tmp_path, names, model=m)
    cfg = rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, max_term=m.max_term, max_log_len=m.max_log,
                          max_msgs=5 if K == 8 else 4, max_dup=m.max_dup, state_capacity=1 << 12)
    views = (rmc.StateView * len(states))(*[to_view(m, s) for s in states])
    with rmc.Checker(cfg) as ck:
        assert ck.lib.rmc_state_bytes(C.byref(cfg)) == (2 * m.n_servers + K) * 4
        ck.set_predicates(preds)
        got = ck.eval_predicates(views)
        assert got == want
        assert got == host_vm(pred_check, tmp_path, names, m, states, K)
        for p, pname in enumerate(names):  # the restated built-ins: the compiled-in check of that bit
            if pname in PC.RESTATED:
                builtin = ck.check_states(views, PC.RESTATED[pname])
                assert [1 if b else 0 for b in builtin] == [row[p] for row in got], pname
        assert ck.eval_predicates([]) == []


RECORDS = {0: (32, 64), 1: (16, 16), 2: (4, 12)}  # RMC_WIDE_COMPACT: (log entries, messages) of the record


def fits(s, record):
    L, K = RECORDS[record]
    return (len(s.messages) <= K and all(len(lg) <= L for lg in s.log) and
            all(len(R.rget(m, "mlog")) <= L for m, _c in s.messages if R.rget(m, "mtype") == R.RVP))


@pytest.mark.parametrize("group", sorted(PC.GROUPS))
@pytest.mark.parametrize("record", [0, 1, 2])
@pytest.mark.parametrize("name", ["wide_s3", "wide_s5"])
def test_eval_predicates_on_the_three_wide_records(name, record, group, pred_check, tmp_path, monkeypatch):
    monkeypatch.setenv("RMC_WIDE_COMPACT", str(record))
    m, _ = IC.CASES[name]
    names = PC.GROUPS[group]
    keep = [t for t, s in enumerate(IC.states(name)) if fits(s, record)]
    assert len(keep) >= 10, (name, record, len(keep))
    states = [IC.states(name)[t] for t in keep]
    want = [PC.verdicts(name, group)[t] for t in keep]
    _cfg, preds = load(tmp_path, names, model=m)
    cfg = rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, max_term=m.max_term, max_log_len=m.max_log,
                          max_msgs=m.max_msgs, max_dup=m.max_dup, state_capacity=1 << 10)
    views = (rmc.StateView * len(states))(*[to_view(m, s) for s in states])
    with rmc.Checker(cfg) as ck:
        assert ck.lib.rmc_state_bytes(C.byref(cfg)) == {0: 5080, 1: 904, 2: 336}[record]
        ck.set_predicates(preds)
        got = ck.eval_predicates(views)
        assert got == want
        assert got == host_vm(pred_check, tmp_path, names, m, states, 0)
        for p, pname in enumerate(names):
            if pname in PC.RESTATED:
                builtin = ck.check_states(views, PC.RESTATED[pname])
                assert [1 if b else 0 for b in builtin] == [row[p] for row in got], pname
        if record:  # a state beyond the ctx's record is refused by name
            big = next(s for s in IC.states(name) if not fits(s, record))
            with pytest.raises(rmc.RmcError, match="state 0: beyond the ctx's store record"):
                ck.eval_predicates([to_view(m, big)])


# ---- the BFS pass ---------------------------------------------------------------------------
def model_of(params):
    return R.Model(n_servers=params["n_servers"], n_values=params["n_values"], max_term=params["max_term"],
                   max_log=params["max_log_len"], max_msgs=params["max_msgs"], max_dup=params["max_dup"])


def check_user_trace(model, trace, twin, depth):
    """The trace is a behaviour of the spec from Init, of `depth` states, whose last state
    alone does not satisfy the twin."""
    assert len(trace) == depth
    states = [from_view(v) for _f, _i, v in trace]
    assert states[0] == R.init_state(model) and trace[0][0] == -1
    for a, b, (fam, _inst, _v) in zip(states, states[1:], trace[1:]):
        assert (rmc.FAMILIES[fam], b) in {(f, t) for f, _p, t in R.successors(model, a)}
        assert R.in_constraint(model, b)
    assert twin(model, states[-1]) != PC.HOLDS
    assert all(twin(model, s) == PC.HOLDS for s in states[:-1])


REACHABLE = {
    "tiny2": dict(params=G.TINY2),
    "small": dict(params=G.SMALL),
    "sym9": dict(params=G.SYM9, symmetry=True),
    "tiny2-spill": dict(params=G.TINY2, spill=True, device_window=4096),
    "tiny2-wide": dict(params=G.TINY2, wide=True),
}


@pytest.mark.parametrize("case", sorted(REACHABLE))
def test_reachable_predicate_is_reported_like_a_builtin(case, tmp_path, monkeypatch):
    spec = dict(REACHABLE[case])
    params, wide = spec.pop("params"), spec.pop("wide", False)
    if wide:
        monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    model = model_of(params)
    names = ("UserMsgTerms", "UserNoLeader")  # the first holds everywhere: predicate 1 is the violated one
    cfg, preds = load(tmp_path, names, n_servers=params["n_servers"], n_values=params["n_values"],
                      max_term=params["max_term"], max_log=params["max_log_len"], max_msgs=params["max_msgs"],
                      max_dup=params["max_dup"], symmetry=spec.get("symmetry", False))
    want_depth = PC.oracle_violation_depth(model, PC.TWINS["UserNoLeader"], symmetry=spec.get("symmetry", False))
    assert want_depth is not None and want_depth > 3
    run_cfg = rmc.make_config(state_capacity=1 << 16, invariants=0, **params, **spec)
    assert run_cfg.flags & ~rmc.FLAG_SPILL == cfg.flags  # the front-end's model is the one run
    with rmc.Checker(run_cfg) as ck:
        ck.set_predicates(preds)
        res = ck.run()
        assert res.violated_inv == rmc.INV_USER0 << 1 and ck.predicate_name(res.violated_inv) == "UserNoLeader"
        assert not ck.predicate_error() and not res.deadlock
        assert res.violation_depth == want_depth and res.depth == want_depth
        check_user_trace(model, ck.trace(), PC.TWINS["UserNoLeader"], want_depth)
        # removed again: the same ctx searches on to the fixpoint or, here, a depth bound
        ck.set_predicates(None)
        assert ck.lib.rmc_eval_predicates(ck.ctx, None, 0, None) == -71


@pytest.mark.parametrize("variant", ["plain", "spill", "verify", "coverage", "wide"])
def test_predicates_that_hold_change_no_count(variant, tmp_path, monkeypatch):
    if variant == "wide":
        monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    kw = {"spill": dict(spill=True, device_window=4096), "verify": dict(verify_states=True),
          "coverage": dict(coverage=True)}.get(variant, {})
    names = ("UserOneLeader", "UserLeaderVotes", "UserCandTerm", "UserMsgTerms", "UserQuorumCommit", "UserGuardedLog")
    _cfg, preds = load(tmp_path, names, n_servers=2, n_values=1)
    out = []
    for with_preds in (False, True):
        with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2, **kw)) as ck:
            if with_preds:
                ck.set_predicates(preds)
            res = ck.run()
            out.append((res.distinct, res.generated, res.depth, res.violated_inv, res.left_on_queue))
    assert out[0] == out[1] and out[0][0] == G.CASES["tiny2"].distinct == 12975 and out[0][3] == 0


def test_init_evaluation_error_is_reported_at_depth_1(tmp_path):
    _cfg, preds = load(tmp_path, ("UserGuardedLog", "UserUnguardedLog"), n_servers=2, n_values=1)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2)) as ck:
        ck.set_predicates(preds)
        res = ck.run()
        assert res.violated_inv == rmc.INV_USER0 << 1 and res.violation_depth == 1 and res.depth == 1
        assert ck.predicate_error()
        trace = ck.trace()
        assert len(trace) == 1 and from_view(trace[0][2]) == R.init_state(model_of(G.TINY2))


FEW_LEADERS = "UserFewLeaders ==\n    Cardinality({i \\in Server : state[i] = Leader}) <= 1"


@pytest.mark.parametrize("user", ["UserOneLeader", "UserFewLeaders"])
def test_builtin_and_user_violation_follow_the_least_index_rule(user, tmp_path):
    """The weakened quorum guard elects two leaders in one term.  With the restated
    OneLeaderPerTerm as the user predicate the same states violate both, so at the least
    index the built-in wins.  With UserFewLeaders more states violate the user predicate:
    whichever kind holds the least index of the level is the one reported."""
    p = G.SMALL
    cfg_path, tla = PC.write_model(tmp_path, [user], module=PC.module_with(FEW_LEADERS), n_servers=3, n_values=2,
                                   max_term=p["max_term"], max_log=p["max_log_len"], max_msgs=p["max_msgs"],
                                   max_dup=p["max_dup"])
    preds = rmc.Predicates(cfg_path, tla, builtin_raft=True)
    cfg = rmc.make_config(bug_quorum=True, invariants=rmc.INV_TYPEOK | rmc.INV_ONE_LEADER, state_capacity=1 << 18, **p)
    with rmc.Checker(cfg) as ck:
        ck.set_predicates(preds)
        res = ck.run()
        assert res.violated_inv in (rmc.INV_ONE_LEADER, rmc.INV_USER0)
        starts = ck.levels()
        lo, hi = starts[res.violation_depth - 1], starts[res.violation_depth]
        assert hi == res.distinct  # the level was finished, and is the last
        st = ck.read_states(lo, hi - lo)
        builtin = [t for t, b in enumerate(ck.check_states(st, rmc.INV_ONE_LEADER)) if b]
        users = [t for t, row in enumerate(ck.eval_predicates(st)) if row[0]]
        before = ck.read_states(0, lo)
        assert not any(ck.check_states(before, rmc.INV_ONE_LEADER)) and not any(r[0] for r in ck.eval_predicates(before))
        least_b, least_u = min(builtin, default=None), min(users, default=None)
        if user == "UserOneLeader":
            assert builtin == users and builtin
        want = rmc.INV_USER0 if least_b is None or (least_u is not None and least_u < least_b) else rmc.INV_ONE_LEADER
        assert res.violated_inv == want
        last = from_view(ck.trace()[-1][2])
        assert last == from_view(st[least_u if want == rmc.INV_USER0 else least_b])


def test_refusals(tmp_path, monkeypatch):
    _cfg, preds = load(tmp_path, ("UserNoLeader",), n_servers=2, n_values=1)
    _cfg, named = load(tmp_path, ("UserNamesServer",), n_servers=2, n_values=1)
    _cfg, three = load(tmp_path, ("UserNoLeader",), n_servers=3)

    def refused(ck, p, code, *needles):
        with pytest.raises(rmc.RmcError) as e:
            ck.set_predicates(p)
        assert e.value.code == code and all(n in str(e.value) for n in needles), str(e.value)

    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, continue_=True, **G.TINY2)) as ck:
        refused(ck, preds, -22, "RMC_FLAG_CONTINUE")
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, symmetry=True, **G.TINY2)) as ck:
        refused(ck, named, -22, "server model value", "SYMMETRY")
        ck.set_predicates(preds)  # a predicate that names none is accepted under SYMMETRY
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2)) as ck:
        ck.set_predicates(named)  # and without SYMMETRY the one that does
        refused(ck, three, -22, "3 servers", "the ctx has 2")
        # with predicates set: no simulation, checkpoint, recovery or sharding
        for call, code in ((lambda: ck.simulate(behaviours=8, depth=4, smoke_k=0), -71),
                           (lambda: ck.checkpoint(str(tmp_path / "ck")), -71),
                           (lambda: ck.recover(str(tmp_path / "ck")), -71),
                           (lambda: ck.shard(0, 1, transport=transport(), keys_per_dest=1 << 12,
                                             sent_cache_slots=1 << 12), -22)):
            with pytest.raises(rmc.RmcError) as e:
                call()
            assert e.value.code == code and "model-defined invariants" in str(e.value), str(e.value)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2)) as ck:
        ck.shard(0, 1, transport=transport(), keys_per_dest=1 << 12, sent_cache_slots=1 << 12)
        refused(ck, preds, -22, "sharded")
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    with rmc.Checker(rmc.make_config(state_capacity=1 << 12, spill=True, device_window=1 << 12, max_depth=6,
                                     **G.TINY2)) as ck:
        refused(ck, preds, -22, "wide layout", "RMC_FLAG_SPILL")


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


def test_front_end_option(tmp_path):
    """Without RMC_FRONT_PREDICATES the refusal of today stands; with it the INVARIANT is
    accepted and left out of the mask; the ten known names keep their bits."""
    cfg_path, tla = PC.write_model(tmp_path, ("TypeOK", "UserNoLeader"))
    with pytest.raises(rmc.RmcError, match="INVARIANT UserNoLeader is not compiled into the engine"):
        rmc.model_from_files(cfg_path, tla, builtin_raft=True)
    cfg, _sc, _notes = rmc.model_from_files(cfg_path, tla, builtin_raft=True, predicates=True)
    assert cfg.invariants == rmc.INV_TYPEOK
    assert rmc.Predicates(cfg_path, tla, builtin_raft=True).names == ["UserNoLeader"]


# ---- rmc-tlc ----------------------------------------------------------------------------------
def test_cli_reports_the_predicate_like_tlc(monkeypatch):
    from tests import tla_transcript
    tla = os.path.join(SPECS, "predicates", "MCraftPredicates.tla")
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536", tla], capture_output=True, text=True, timeout=120)
    assert r.returncode == 12, r.stdout + r.stderr
    out = r.stdout
    assert "Compiled model-defined invariants: MsgTermsBounded, QuorumHasCommitted, LogTermsBounded, NoLeaderElected" in out
    assert "Error: Invariant NoLeaderElected is violated." in out
    assert "Error: The behavior up to this point is:" in out
    model = model_of(G.SMALL)
    monkeypatch.setitem(R.INVARIANTS, "NoLeaderElected", lambda m, s: PC.TWINS["UserNoLeader"](m, s) == PC.HOLDS)
    inv, n = tla_transcript.validate(out, model)
    assert inv == "NoLeaderElected"
    assert n == PC.oracle_violation_depth(model, PC.TWINS["UserNoLeader"])
    # the searches that do not run the predicate pass refuse the model by the predicate's name
    for flag in (["-continue"], ["-gpus", "2"], ["-simulate"], ["-checkpoint", "x.ck"], ["-recover", "x.ck"]):
        r = subprocess.run([CLI, "-builtin-raft"] + flag + [tla], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "INVARIANT MsgTermsBounded is defined by the model" in r.stdout, r.stdout
        assert flag[0] in r.stdout


def test_cli_prints_an_evaluation_error_of_its_own(tmp_path):
    cfg_path, tla = PC.write_model(tmp_path, ("UserUnguardedLog",), n_servers=2, n_values=1)
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536", "-config", cfg_path, tla], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Error: Evaluating invariant UserUnguardedLog failed" in r.stdout
    assert "is violated" not in r.stdout
