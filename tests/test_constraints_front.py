"""Model-defined constraints in the front-end (no GPU): under RMC_FRONT_CONSTRAINTS the
CONSTRAINT conjuncts that are none of the four bounds become residuals, in order, under
the name of the cfg's CONSTRAINT they came from; without the option every refusal of
tests/test_front.py stays.  The six bodies that test refuses are accepted or classified
here; the residuals compile with the limits and the refusals of the predicate language."""
import os
import shutil

import pytest

import rmc
from tests import constraint_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = os.path.join(ROOT, "specs")

# the bodies tests/test_front.py test_constraint_forms_outside_the_bounds_are_refused pins, with
# what each is refused for without the option, and the residuals it gives with it
BODIES = [
    ("~(\\A i \\in Server : currentTerm[i] <= MaxTerm)", "not a state bound",
     ["~ ( \\A i \\in Server : currentTerm [ i ] <= MaxTerm )"]),
    ("\\/ \\A i \\in Server : currentTerm[i] <= MaxTerm\n    \\/ Cardinality(DOMAIN messages) <= MaxMsgs",
     "not a state bound", None),
    ("(\\A i \\in Server : Len(log[i]) <= MaxLogLen) => Cardinality(DOMAIN messages) <= MaxMsgs",
     "not a state bound", None),
    ("\\A i \\in Server : currentTerm[i] <= MaxTerm /\\ state[i] /= Leader", "state",
     ["\\A i \\in Server : state [ i ] /= Leader"]),
    ("\\A i \\in Server : currentTerm[i] >= 1", "currentTerm", ["\\A i \\in Server : currentTerm [ i ] >= 1"]),
    ("TRUE", "TRUE", ["TRUE"]),
]


def model_dir(tmp_path, body, old_too):
    """specs/ with StateConstraint's body replaced as tests/test_front.py does (the shipped
    bounds stay behind as OldConstraint); old_too: the cfg names OldConstraint as well."""
    for f in os.listdir(SPECS):
        if f.endswith((".tla", ".cfg")):
            shutil.copy(os.path.join(SPECS, f), tmp_path / f)
    p = tmp_path / "MCraftBounded.tla"
    p.write_text(p.read_text().replace("StateConstraint ==\n", f"StateConstraint ==\n    {body}\nOldConstraint ==\n"))
    if old_too:
        c = tmp_path / "MCraftBench.cfg"
        c.write_text(c.read_text().replace("CONSTRAINT StateConstraint", "CONSTRAINT StateConstraint OldConstraint"))
    return tmp_path / "MCraftBench.cfg"


def residual_notes(notes):
    return [ln for ln in notes.splitlines() if ": residual " in ln]


@pytest.mark.parametrize("body,refused_for,residuals", BODIES, ids=[b[1] + str(k) for k, b in enumerate(BODIES)])
def test_the_pinned_refusals_with_and_without_the_option(tmp_path, body, refused_for, residuals):
    cfg = model_dir(tmp_path, body, old_too=True)
    with pytest.raises(rmc.RmcError, match=refused_for):  # without the option: refused as before
        rmc.model_from_files(str(cfg), builtin_raft=True)
    if residuals is None:
        # the disjunction and the implication hold the model's only bounds: as residuals they bound
        # nothing, and the model stays infinite
        alone = model_dir(tmp_path, body, old_too=False)
        with pytest.raises(rmc.RmcError, match="infinite"):
            rmc.model_from_files(str(alone), builtin_raft=True, constraints=True)
        return
    c, _sc, notes = rmc.model_from_files(str(cfg), builtin_raft=True, constraints=True)
    assert (c.n_servers, c.max_term, c.max_log_len, c.max_msgs, c.max_dup) == (3, 2, 1, 3, 1)
    got = residual_notes(notes)
    assert len(got) == len(residuals)
    for k, (ln, text) in enumerate(zip(got, residuals)):
        assert ln.startswith("CONSTRAINT StateConstraint: residual %d `%s`" % (k, text)), ln
    cons = rmc.Constraints(str(cfg), builtin_raft=True)
    assert cons.names == ["StateConstraint"] * len(residuals)


def test_a_bound_and_a_residual_in_one_quantifier(tmp_path):
    """`\\A i : currentTerm[i] <= MaxTerm /\\ state[i] /= Leader` alone: the term bound is taken
    (the other three are missing, so the model is infinite), the rest is a residual."""
    cfg = model_dir(tmp_path, BODIES[3][0], old_too=False)
    with pytest.raises(rmc.RmcError, match="infinite"):
        rmc.model_from_files(str(cfg), builtin_raft=True, constraints=True)
    c, _sc, notes = rmc.model_from_files(str(cfg), builtin_raft=True, constraints=True, depth_bounded=True)
    assert c.max_term == 2 and not c.flags & rmc.FLAG_UNBOUNDED_TERM and c.flags & rmc.FLAG_UNBOUNDED_LOG
    assert len(residual_notes(notes)) == 1


def test_residuals_keep_cfg_order_and_names(tmp_path):
    cfg, tla = CC.write_model(tmp_path, CC.TINY2, ["ConsNoCommitNoLeader", "OnlyOneCandidate", "OnlyAlways"])
    c, notes, preds, cons = rmc.load_model(cfg, tla, builtin_raft=True, constraints=True)
    assert preds is None and (c.n_servers, c.max_term, c.max_log_len, c.max_msgs, c.max_dup) == (2, 2, 1, 2, 1)
    # the quantified conjunction splits like the bounds' own quantifier does
    assert cons.names == ["ConsNoCommitNoLeader", "ConsNoCommitNoLeader", "OnlyOneCandidate", "OnlyAlways"]
    assert len(cons) == 4 and len(residual_notes(notes)) == 4
    # a model without residuals: count 0, and the old return shape without the argument
    cfg2 = os.path.join(SPECS, "MCraftTiny2.cfg")
    out = rmc.load_model(cfg2, builtin_raft=True)
    assert len(out) == 3 and out[2] is None
    assert len(rmc.load_model(cfg2, builtin_raft=True, constraints=True)[3]) == 0
    assert len(rmc.model_from_files(cfg2, builtin_raft=True)) == 3


def test_shipped_example(tmp_path):
    d = os.path.join(SPECS, "constraints")
    c, notes, preds, cons = rmc.load_model(os.path.join(d, "MCraftConstraints.cfg"), builtin_raft=True,
                                           predicates=True, constraints=True)
    assert cons.names == ["StateConstraint", "Scenario"] and preds is not None and preds.names == ["MsgTermsBounded"]
    with pytest.raises(rmc.RmcError, match="StateConstraint: conjunct .*Candidate"):
        rmc.model_from_files(os.path.join(d, "MCraftConstraints.cfg"), builtin_raft=True, predicates=True)


REFUSALS = [
    ("\\A i \\in Server : SubSeq(log[i], 1, 1) = SubSeq(log[i], 1, 1)", "SubSeq"),
    ("\\A i, j \\in Server : log[i] = log[j]", "sequence"),
    ("Cardinality(Server)", "not Boolean"),
    ("\\A i \\in Server : currentTerm[i] <= NoSuchName", "unknown identifier NoSuchName"),
]


@pytest.mark.parametrize("body,needle", REFUSALS, ids=[n for _b, n in REFUSALS])
def test_a_residual_outside_the_language_is_refused_by_name(tmp_path, body, needle):
    cfg, tla = CC.write_model(tmp_path, CC.TINY2, ["StateConstraint", "Bad"])
    text = open(tla).read()
    with open(tla, "w") as f:
        f.write(CC.with_definitions(text, "Bad ==\n    " + body))
    rmc.model_from_files(cfg, tla, builtin_raft=True, constraints=True)  # recorded, not compiled
    with pytest.raises(rmc.RmcError, match="CONSTRAINT Bad: conjunct ") as e:
        rmc.Constraints(cfg, tla, builtin_raft=True)
    assert needle in str(e.value)
    assert needle == "not Boolean" or (" line " in str(e.value) and " col " in str(e.value))


def test_more_than_eight_residuals_are_refused_with_the_count(tmp_path):
    cfg, tla = CC.write_model(tmp_path, CC.TINY2, ["StateConstraint", "Many"])
    text = open(tla).read()
    many = "Many ==\n" + "".join("    /\\ \\E i \\in Server : currentTerm[i] >= %d\n" % k for k in range(9))
    with open(tla, "w") as f:
        f.write(CC.with_definitions(text, many))
    with pytest.raises(rmc.RmcError, match="9 residual constraint conjuncts exceed RMC_MAX_PREDICATES = 8"):
        rmc.Constraints(cfg, tla, builtin_raft=True)


def test_abi_lists_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "rmc.h")).read()
    assert "#define RMC_ABI_VERSION 16" in text and "#define RMC_FRONT_CONSTRAINTS (1u << 4)" in text
    assert rmc.FRONT_CONSTRAINTS == 16
    for name in ("rmc_constraints_from_files", "rmc_set_constraints", "rmc_constraint_error"):
        assert name in rmc.EXPORTS and hasattr(rmc.native(), name)
