"""Model-defined constraints on the GPU (rmc.h "model-defined constraints"): residual
CONSTRAINT conjuncts, compiled by the front-end, filter the states every expansion launch
stores.  Every expected number comes from tests/constraint_cases.py, a level loop over
oracle/raft_spec.py with the residual's Python twin conjoined to in_constraint."""
import collections
import json
import os
import re
import subprocess
import sys

import pytest

import rmc
from oracle import raft_spec as R
from tests import constraint_cases as CC
from tests.convert import from_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = os.path.join(ROOT, "specs")
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
BUG2 = R.Model(n_servers=2, n_values=1, max_term=2, max_log=1, max_msgs=2, max_dup=1, bug_quorum=True)


def load(tmp_path, model, constraints, invariants=(), symmetry=False, capacity=1 << 18):
    cfg_path, tla = CC.write_model(tmp_path, model, constraints, invariants, symmetry)
    cfg, _notes, preds, cons = rmc.load_model(cfg_path, tla, builtin_raft=True, predicates=True, constraints=True)
    cfg.state_capacity = capacity
    assert bool(cfg.flags & rmc.FLAG_SYMMETRY) == symmetry and bool(cfg.flags & rmc.FLAG_BUG_QUORUM) == model.bug_quorum
    return cfg, preds, cons


def check_counts(o, res, rows, starts):
    """rows: Checker.levels after run(), (level, cumulative generated, distinct, new, seconds);
    starts: rmc_get_levels."""
    print("levels", [b - a for a, b in zip(starts, starts[1:])], "rows", [r[1:4] for r in rows])
    assert [b - a for a, b in zip(starts, starts[1:])] == o.level_new
    assert [r[3] for r in rows if r[3]] == o.level_new[1:]
    for k, r in enumerate(rows):
        assert r[1] == sum(o.level_generated[:k + 2]), (k, r)
    assert len(rows) == len(o.level_generated) - 1
    assert (res.distinct, res.generated, res.depth, res.left_on_queue) == \
        (o.distinct, o.generated, o.depth, o.left_on_queue)


def not_vacuous(o):
    """The residual alone removed successors in at least two levels, and states remain."""
    assert sum(1 for x in o.level_removed if x > 0) >= 2 and o.distinct > 1, o.level_removed


def run(cfg, cons, preds=None, max_depth=0):
    cfg.max_depth = max_depth
    with rmc.Checker(cfg) as ck:
        ck.set_constraints(cons)
        if preds is not None and len(preds):
            ck.set_predicates(preds)
        res = ck.run()
        rows = list(ck.levels)
        return res, rows, ck.levels(), ck.constraint_error()


# (model, the cfg's CONSTRAINTs, the residual, depth bound): the five residuals on specs/MCraftTiny2's
# bounds, and at S = 3 on tests/predicate_cases.py's bounds under a depth bound
COUNTS = {
    "no-leader": (CC.TINY2, ["ConsNoLeader"], "NoLeader", 0),
    "one-candidate": (CC.TINY2, ["ConsOneCandidate"], "OneCandidate", 0),
    "no-commit-no-leader": (CC.TINY2, ["ConsNoCommitNoLeader"], "NoCommitNoLeader", 0),
    "term-implies-few-msgs": (CC.TINY2, ["ConsTermImpliesFewMsgs"], "TermImpliesFewMsgs", 0),
    "second-constraint-name": (CC.TINY2, ["StateConstraint", "OnlyNoAERequest"], "NoAERequest", 0),
    "s3-one-candidate": (CC.SMALL3, ["ConsOneCandidate"], "OneCandidate", 8),
    "s3-term-implies-few-msgs": (CC.SMALL3, ["StateConstraint", "OnlyTermImpliesFewMsgs"], "TermImpliesFewMsgs", 8),
}


@pytest.mark.parametrize("case", sorted(COUNTS))
def test_counts_equal_the_oracle_level_by_level(case, tmp_path):
    model, constraints, residual, bound = COUNTS[case]
    o = CC.oracle(model, residual, max_levels=bound or None)
    not_vacuous(o)
    cfg, _preds, cons = load(tmp_path, model, constraints)
    res, rows, starts, err = run(cfg, cons, max_depth=bound)
    check_counts(o, res, rows, starts)
    assert res.violated_inv == 0 and not res.deadlock and err == 0


def test_true_as_residual_changes_no_count(tmp_path):
    cfg, _preds, cons = load(tmp_path, CC.TINY2, ["ConsAlways"])
    assert len(cons) == 1
    res, rows, starts, _err = run(cfg, cons)
    o = CC.oracle(CC.TINY2, "Always")
    check_counts(o, res, rows, starts)
    with rmc.Checker(cfg) as ck:  # and without constraints
        plain = ck.run()
    assert (plain.distinct, plain.generated, plain.depth) == (res.distinct, res.generated, res.depth) == (12975, 130639, 31)


def test_initial_state_that_fails_is_generated_and_dropped(tmp_path):
    cfg, _preds, cons = load(tmp_path, CC.TINY2, ["StateConstraint", "OnlyNever"])
    res, rows, starts, err = run(cfg, cons)
    assert (res.distinct, res.generated, res.depth, res.left_on_queue) == (0, 1, 0, 0)
    assert rows == [] and starts == [0, 0] and err == 0 and res.violated_inv == 0
    check_counts(CC.oracle(CC.TINY2, "Never"), res, rows, starts)


def test_a_level_removed_whole_adds_nothing_to_the_depth(tmp_path):
    """Every state of level 2 has a server in MaxTerm (the two Timeouts): with ShortTerms the
    search expands level 1, stores nothing, and ends at depth 1, one less than without."""
    o = CC.oracle(CC.TINY2, "ShortTerms")
    assert o.depth == 1 and o.level_removed == [0, 2] and o.level_generated == [1, 4]
    cfg, _preds, cons = load(tmp_path, CC.TINY2, ["ConsShortTerms"])
    res, rows, starts, _err = run(cfg, cons, max_depth=2)
    check_counts(o, res, rows, starts)
    with rmc.Checker(cfg) as ck:
        assert ck.run().depth == 2


def test_symmetry(tmp_path):
    o = CC.oracle(CC.SMALL3, "OneCandidate", max_levels=8, symmetry=True)
    not_vacuous(o)
    cfg, _preds, cons = load(tmp_path, CC.SMALL3, ["ConsOneCandidate"], symmetry=True)
    res, rows, starts, _err = run(cfg, cons, max_depth=8)
    check_counts(o, res, rows, starts)


def test_stored_states_are_the_oracles_and_satisfy_the_residual(tmp_path):
    model, residual = CC.TINY2, "TermImpliesFewMsgs"
    o = CC.oracle(model, residual)
    not_vacuous(o)
    twin = CC.RESIDUALS[residual][1]
    cfg, _preds, cons = load(tmp_path, model, ["ConsTermImpliesFewMsgs"])
    with rmc.Checker(cfg) as ck:
        ck.set_constraints(cons)
        res = ck.run()
        starts = ck.levels()
        assert len(starts) == o.depth + 1 and starts[-1] == res.distinct == o.distinct
        for lv, (a, b) in enumerate(zip(starts, starts[1:])):
            got = [from_view(v) for v in ck.read_states(a, b - a)]
            assert all(twin(model, s) and R.in_constraint(model, s) for s in got), lv
            assert collections.Counter(got) == collections.Counter(o.levels[lv]), lv
        # the graph calls that probe the set are refused: it holds keys without a stored state
        for call in (lambda: ck.graph_edges(0, 1), lambda: ck.find_states(ck.read_states(0, 1))):
            with pytest.raises(rmc.RmcError) as e:
                call()
            assert e.value.code == -71 and "model-defined constraints" in str(e.value)
        # ... of this run's set, whether or not the constraints are still set
        ck.set_constraints(None)
        with pytest.raises(rmc.RmcError, match="the run had model-defined constraints set"):
            ck.graph_edges(0, 1)
        assert len(ck.read_states(0, 1)) == 1


CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], 'raft.tla_amd'))
sys.path.insert(0, sys.argv[1])
import rmc
cfg, _notes, _preds, cons = rmc.load_model(sys.argv[2], sys.argv[3], builtin_raft=True, predicates=True, constraints=True)
cfg.state_capacity = 1 << 22
with rmc.Checker(cfg) as ck:
    ck.set_constraints(cons)
    res = ck.run()
    rows, starts = [list(r[:4]) for r in ck.levels], ck.levels()
    # the largest level, state by state: the sorted raw records and how many of them are distinct
    lv = max(range(len(starts) - 1), key=lambda k: starts[k + 1] - starts[k])
    recs = sorted(bytes(v) for v in ck.read_states(starts[lv], starts[lv + 1] - starts[lv]))
    print(json.dumps({'rows': rows, 'starts': starts, 'launches': res.expand_launches,
                      'totals': [res.distinct, res.generated, res.depth, res.left_on_queue, res.violated_inv],
                      'largest': [lv, len(recs), len(set(recs)), hashlib.sha256(b''.join(recs)).hexdigest()]}))
"""


def test_compaction_at_launch_boundaries_inside_a_level(tmp_path):
    """RMC_LAUNCH_LOG2=16 (read once per process: a fresh child) cuts every level above 65,536
    states into equal launches, each followed by its own filter and compaction.  A Python oracle
    of this model is out of reach, so the test pins what can go wrong only here: cutting a level
    into launches changes no level's count (the reference is the search with one launch a level,
    whose rules the other tests compare with the oracle); states are removed and moved by
    passes inside cut levels (the pass's statistic, and more passes than levels); and the
    largest level, read back state by state, holds the same states in both runs, each once."""
    from tests.test_gpu import GOLDEN
    # the bounds of golden "small" (2,466,993 states without the residual, levels of up to 147,462):
    # the residual removes the states in which all three servers are candidates
    g = GOLDEN["small"]
    model = R.Model(n_servers=3, n_values=2, max_term=2, max_log=1, max_msgs=1, max_dup=1)
    assert (g["params"]["max_msgs"], g["params"]["n_servers"], g["distinct"]) == (1, 3, 2466993)
    cfg_path, tla = CC.write_model(tmp_path, model, ["ConsTwoCandidates"])
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    out, stats = {}, {}
    for log2 in ("16", ""):
        env = dict(os.environ, RMC_CONS_STATS="1")
        env.pop("RMC_LAUNCH_LOG2", None)
        if log2:
            env["RMC_LAUNCH_LOG2"] = log2
        r = subprocess.run([sys.executable, str(script), ROOT, cfg_path, tla], capture_output=True, text=True,
                           timeout=240, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        out[log2] = json.loads(r.stdout.strip().splitlines()[-1])
        m = re.findall(r"constraint pass: (\d+) passes, (\d+) states removed, (\d+) states moved", r.stderr)
        stats[log2] = tuple(int(x) for x in m[-1])
    cut, whole = out["16"], out[""]
    expanded = len(whole["rows"])
    print("launches", cut["launches"], "against", whole["launches"], "levels", expanded, "largest", whole["largest"][:3],
          "passes, removed, moved: cut", stats["16"], "whole", stats[""])
    assert whole["launches"] == expanded and cut["launches"] > expanded + 4
    # a pass after the seed and after every launch that added states: more of them in the cut run;
    # both runs remove the same states, and move some
    assert stats[""][0] <= expanded + 1 and stats[""][0] < stats["16"][0] <= cut["launches"] + 1
    assert stats["16"][1] == stats[""][1] > 0 and stats["16"][2] > 0 and stats[""][2] > 0
    assert cut["rows"] == whole["rows"] and cut["starts"] == whole["starts"] and cut["totals"] == whole["totals"]
    assert whole["totals"][4] == 0 and whole["totals"][3] == 0 and whole["totals"][0] < g["distinct"]
    # the largest level was cut into launches (its parents are more than 65,536) and holds the same
    # states, each once, however many launches filtered and compacted it
    lv, n, distinct, _digest = whole["largest"]
    assert cut["largest"] == whole["largest"] and n == distinct > 1 << 16
    assert whole["rows"][lv - 2][3] > 1 << 16          # rows[k]: the expansion of level k + 1 into level k + 2


# ---- invariants ----------------------------------------------------------------------------
def check_trace(model, twin, trace, depth):
    """A behaviour of the spec from Init of `depth` states, every one kept by the constraint."""
    assert len(trace) == depth
    states = [from_view(v) for _f, _i, v in trace]
    assert states[0] == R.init_state(model) and trace[0][0] == -1
    for a, b, (fam, _inst, _v) in zip(states, states[1:], trace[1:]):
        assert (rmc.FAMILIES[fam], b) in {(f, t) for f, _p, t in R.successors(model, a)}
    assert all(R.in_constraint(model, s) for s in states)
    return states


@pytest.mark.parametrize("invariant", ["OneLeaderPerTerm", "UserOneLeader"])
def test_no_removed_state_is_reported_by_an_invariant(invariant, tmp_path):
    """The weakened quorum guard elects two leaders in one term at depth 11.  The residual
    removes every state with two leaders before any invariant sees it — the built-in check
    (run over the kept states) and the same text as the model's own predicate alike."""
    assert CC.oracle(BUG2, "Always", invariants=("OneLeaderPerTerm",)).violation_depth == 11
    o = CC.oracle(BUG2, "OneLeaderAtMost", invariants=("OneLeaderPerTerm",))
    not_vacuous(o)
    assert o.violated is None
    cfg, preds, cons = load(tmp_path, BUG2, ["ConsOneLeaderAtMost"], invariants=[invariant])
    assert (cfg.invariants, len(preds)) == ((rmc.INV_ONE_LEADER, 0) if invariant == "OneLeaderPerTerm" else (0, 1))
    res, rows, starts, _err = run(cfg, cons, preds)
    assert res.violated_inv == 0
    check_counts(o, res, rows, starts)


@pytest.mark.parametrize("invariant", ["OneLeaderPerTerm", "UserOneLeader"])
def test_a_kept_violating_state_is_reported_at_the_oracles_depth(invariant, tmp_path):
    residual = "NoAERequest"
    twin = CC.RESIDUALS[residual][1]
    o = CC.oracle(BUG2, residual, invariants=("OneLeaderPerTerm",))
    assert o.violated == "OneLeaderPerTerm" and sum(1 for x in o.level_removed if x > 0) >= 2
    cfg, preds, cons = load(tmp_path, BUG2, ["StateConstraint", "OnlyNoAERequest"], invariants=[invariant])
    cfg.max_depth = 0
    with rmc.Checker(cfg) as ck:
        ck.set_constraints(cons)
        if len(preds):
            ck.set_predicates(preds)
        res = ck.run()
        assert res.violated_inv == (rmc.INV_ONE_LEADER if invariant == "OneLeaderPerTerm" else rmc.INV_USER0)
        assert res.violation_depth == res.depth == o.violation_depth and ck.constraint_error() == 0
        # the levels up to the violation are the oracle's (it stops inside the level; the engine ends it)
        starts = ck.levels()
        assert [b - a for a, b in zip(starts, starts[1:])] == o.level_new
        states = check_trace(BUG2, twin, ck.trace(), o.violation_depth)
        assert all(twin(BUG2, s) for s in states)
        assert not R.INVARIANTS["OneLeaderPerTerm"](BUG2, states[-1])
        assert all(R.INVARIANTS["OneLeaderPerTerm"](BUG2, s) for s in states[:-1])


def test_evaluation_error_in_a_residual(tmp_path):
    """log[i][1] of a leader with an empty log: the first leader, at the oracle's level."""
    residual = "LeaderFirstEntry"
    twin = CC.RESIDUALS[residual][1]
    o = CC.oracle(CC.TINY2, residual)
    assert o.error_depth == 10
    cfg, _preds, cons = load(tmp_path, CC.TINY2, ["ConsLeaderFirstEntry"])
    with rmc.Checker(cfg) as ck:
        ck.set_constraints(cons)
        res = ck.run()
        assert ck.constraint_error() == 1 and res.violated_inv == 0 and not res.deadlock
        assert res.depth == o.error_depth == res.violation_depth
        starts = ck.levels()
        assert [b - a for a, b in zip(starts, starts[1:])] == o.level_new  # the state is kept, the level finished
        states = check_trace(CC.TINY2, twin, ck.trace(), o.error_depth)
        for s in states[:-1]:
            assert twin(CC.TINY2, s)
        with pytest.raises(CC.EvalError):
            twin(CC.TINY2, states[-1])
        # a second run on the same ctx without the constraint: no error is left over
        ck.set_constraints(None)
        assert ck.run().distinct == 12975 and ck.constraint_error() == 0


# ---- refusals ------------------------------------------------------------------------------
def test_refusals(tmp_path, monkeypatch):
    from tests.test_predicates import transport
    tiny = dict(n_servers=2, n_values=1, max_term=2, max_log_len=1, max_msgs=2, max_dup=1)
    _c, _p, cons = load(tmp_path, CC.TINY2, ["ConsNoLeader"])
    _c, _p, named = load(tmp_path, CC.TINY2, ["StateConstraint", "OnlyNamesServer"])
    _c, _p, three = load(tmp_path, CC.SMALL3, ["ConsNoLeader"])

    def refused(ck, p, *needles):
        with pytest.raises(rmc.RmcError) as e:
            ck.set_constraints(p)
        assert e.value.code == -22 and str(e.value).count("rmc_set_constraints") == 1, str(e.value)
        assert all(n in str(e.value) for n in needles), str(e.value)

    for kw, needles in ((dict(verify_states=True), ("RMC_FLAG_VERIFY_STATES", "never gets an owner")),
                        (dict(continue_=True), ("RMC_FLAG_CONTINUE",)),
                        (dict(coverage=True), ("RMC_FLAG_COVERAGE",)),
                        (dict(spill=True, device_window=4096), ("RMC_FLAG_SPILL", "resident"))):
        with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **tiny, **kw)) as ck:
            refused(ck, cons, *needles)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, symmetry=True, **tiny)) as ck:
        refused(ck, named, "server model value", "SYMMETRY")
        ck.set_constraints(cons)  # a residual that names none is accepted under SYMMETRY
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **tiny)) as ck:
        ck.set_constraints(named)  # and without SYMMETRY the one that does
        refused(ck, three, "3 servers", "the ctx has 2")
        # with constraints set: no simulation, checkpoint, recovery or sharding
        for call, code in ((lambda: ck.simulate(behaviours=8, depth=4, smoke_k=0), -71),
                           (lambda: ck.checkpoint(str(tmp_path / "ck")), -71),
                           (lambda: ck.recover(str(tmp_path / "ck")), -71),
                           (lambda: ck.shard(0, 1, transport=transport(), keys_per_dest=1 << 12,
                                             sent_cache_slots=1 << 12), -22)):
            with pytest.raises(rmc.RmcError) as e:
                call()
            assert e.value.code == code and "model-defined constraints" in str(e.value), str(e.value)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, max_depth=5, **tiny)) as ck:
        ck.run()
        ck.checkpoint(str(tmp_path / "plain.ck"))
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **tiny)) as ck:
        ck.recover(str(tmp_path / "plain.ck"))  # the recovered set lacks the keys a constraint would have removed
        with pytest.raises(rmc.RmcError, match="rmc_set_constraints: rmc_recover loaded a checkpoint") as e:
            ck.set_constraints(cons)
        assert e.value.code == -71
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **tiny)) as ck:
        ck.shard(0, 1, transport=transport(), keys_per_dest=1 << 12, sent_cache_slots=1 << 12)
        refused(ck, cons, "sharded")
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    with rmc.Checker(rmc.make_config(state_capacity=1 << 12, max_depth=6, **tiny)) as ck:
        refused(ck, cons, "wide layout")


# ---- rmc-tlc -------------------------------------------------------------------------------
def test_cli_transcript():
    """specs/constraints/MCraftConstraints against tests/golden/cli_MCraftConstraints.txt; its
    counts are the oracle's."""
    both = lambda m, s: CC.RESIDUALS["OneCandidate"][1](m, s) and CC.RESIDUALS["TermImpliesFewMsgs"][1](m, s)
    o = CC.bfs(CC.TINY2, both)
    assert sum(1 for x in o.level_removed if x > 0) >= 2
    tla = os.path.join(SPECS, "constraints", "MCraftConstraints.tla")
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536", tla], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    volatile = ("Finished in", "Progress(", "  calculated (optimistic)", "rmc-tlc: ")
    got = [ln for ln in r.stdout.splitlines() if not ln.startswith(volatile)]
    want = open(os.path.join(ROOT, "tests", "golden", "cli_MCraftConstraints.txt")).read().splitlines()
    assert got == want
    assert "%d states generated, %d distinct states found, 0 states left on queue." % (o.generated, o.distinct) in got
    assert "The depth of the complete state graph search is %d." % o.depth in got
    assert "Compiled 2 residual constraint conjuncts of: StateConstraint, Scenario" in got
    progress = [ln for ln in r.stdout.splitlines() if ln.startswith("Progress(")]
    assert [int(ln.split()[-5]) for ln in progress if int(ln.split()[-5])] == o.level_new[1:]
    # the searches that do not run the constraint pass refuse the model by the constraint's name
    for flag in (["-verify"], ["-continue"], ["-coverage"], ["-dump", str("x.dump")], ["-gpus", "2"], ["-simulate"],
                 ["-checkpoint", "x.ck"], ["-recover", "x.ck"]):
        r = subprocess.run([CLI, "-builtin-raft"] + flag + [tla], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "CONSTRAINT StateConstraint has a conjunct that is no bound" in r.stdout, r.stdout
        assert "not with " + flag[0] in r.stdout


def test_cli_prints_an_evaluation_error_of_its_own(tmp_path):
    cfg_path, tla = CC.write_model(tmp_path, CC.TINY2, ["ConsLeaderFirstEntry"])
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536", "-config", cfg_path, tla], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 12, r.stdout + r.stderr
    assert "Error: Evaluating constraint ConsLeaderFirstEntry failed." in r.stdout
    assert "Error: The behavior up to this point is:" in r.stdout and "State 10:" in r.stdout
