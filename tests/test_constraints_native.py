"""Model-defined constraints on the host (no GPU): tests/native/cons_check.cpp, the
front-end (rmc_front.cpp) and rmc_codec.cpp compiled with plain g++ and no ROCm include
path.  `plan`: the index arithmetic of the in-place compaction (rmc_cons_plan.h, what the
kernels of rmc_dev_cons.h run) over every keep pattern and size.  `verdicts`: the residual
conjuncts of tests/constraint_cases.py compiled to bytecode and evaluated by the
interpreter of rmc_pred.h through ViewAcc on the fixture states of
tests/invariant_cases.py: the verdicts equal the Python twins'."""
import ctypes as C
import os
import subprocess

import pytest

import rmc
from tests import constraint_cases as CC
from tests import invariant_cases as IC
from tests.convert import to_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")
HOLDS, FALSE, ERROR = 0, 1, 2
# seven residual conjuncts (NoCommitNoLeader's quantified conjunction is two): within RMC_MAX_PREDICATES
NAMES = ("NoLeader", "OneCandidate", "NoCommitNoLeader", "TermImpliesFewMsgs", "NoAERequest", "LeaderFirstEntry")
MODELS = ("fuzz0", "fuzz1", "edge1")


@pytest.fixture(scope="module")
def cons_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cons_check") / "cons_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "cons_check.cpp"),
                    os.path.join(CSRC, "rmc_front.cpp"), os.path.join(CSRC, "rmc_codec.cpp"), "-o", str(exe)],
                   check=True)
    return str(exe)


def test_compaction_arithmetic(cons_check):
    r = subprocess.run([cons_check, "plan"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # 8 sizes x (6 fixed patterns + 12 random ones)
    assert r.stdout.strip() == "ok 144"


def twin_verdict(model, name, s):
    try:
        return HOLDS if CC.RESIDUALS[name][1](model, s) else FALSE
    except CC.EvalError:
        return ERROR


@pytest.mark.parametrize("name", MODELS)
def test_host_verdicts_equal_the_twins(name, cons_check, tmp_path):
    m, _gen = IC.CASES[name]
    states = IC.states(name)
    views = tmp_path / "views.bin"
    with open(views, "wb") as f:
        for s in states:
            f.write(bytes(to_view(m, s)))
    assert os.path.getsize(views) == len(states) * C.sizeof(rmc.StateView)
    cfg, tla = CC.write_model(tmp_path, m, ["StateConstraint"] + ["Only" + n for n in NAMES])
    out = tmp_path / "verdicts.bin"
    r = subprocess.run([cons_check, "verdicts", cfg, tla, str(views), str(m.n_servers), str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    owners = [ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith("residual ")]
    assert owners == ["OnlyNoLeader", "OnlyOneCandidate", "OnlyNoCommitNoLeader", "OnlyNoCommitNoLeader",
                      "OnlyTermImpliesFewMsgs", "OnlyNoAERequest", "OnlyLeaderFirstEntry"]
    got = out.read_bytes()
    assert len(got) == len(states) * len(owners)
    seen = {n: set() for n in NAMES}
    for t, s in enumerate(states):
        row = got[t * len(owners):(t + 1) * len(owners)]
        for n in NAMES:
            # a CONSTRAINT's verdict: its conjuncts in order, the first that does not hold decides
            mine = [v for v, o in zip(row, owners) if o == "Only" + n]
            verdict = next((v for v in mine if v), HOLDS)
            assert verdict == twin_verdict(m, n, s), (name, t, n)
            seen[n].add(verdict)
    for n in NAMES:  # not vacuous, from the twins alone
        assert seen[n] >= ({HOLDS, ERROR} if n == "LeaderFirstEntry" else {HOLDS, FALSE}), (n, seen[n])


def test_a_refused_residual_is_named(cons_check, tmp_path):
    cfg, tla = CC.write_model(tmp_path, CC.TINY2, ["StateConstraint", "Bad"])
    text = open(tla).read()
    with open(tla, "w") as f:
        f.write(CC.with_definitions(text, "Bad ==\n    \\A i \\in Server : SubSeq(log[i], 1, 1) = SubSeq(log[i], 1, 1)"))
    r = subprocess.run([cons_check, "verdicts", cfg, tla, "-", "2", "-"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and r.stdout.startswith("refused: CONSTRAINT Bad: conjunct "), r.stdout
    assert "SubSeq at line " in r.stdout


def test_server_model_value_is_recorded(cons_check, tmp_path):
    """(rmc_set_constraints refuses such a program under SYMMETRY: test_constraints.py)"""
    for name, flag in (("OnlyNamesServer", 1), ("OnlyNoLeader", 0)):
        cfg, tla = CC.write_model(tmp_path, CC.TINY2, ["StateConstraint", name])
        r = subprocess.run([cons_check, "verdicts", cfg, tla, "-", "2", "-"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "residual 0 " + name in r.stdout, r.stdout
        assert "names a server: %d" % flag in r.stdout, r.stdout
