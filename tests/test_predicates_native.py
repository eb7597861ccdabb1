"""Model-defined invariants on the host (no GPU): tests/native/pred_check.cpp, the
front-end (rmc_front.cpp) and rmc_codec.cpp compiled with plain g++ and no ROCm include
path.  The predicates of tests/predicate_cases.py are compiled to bytecode and the
interpreter of rmc_pred.h evaluates them on the 1,200 states per model of
tests/invariant_cases.py through every state accessor (the view, the packed words, the
three wide records): the accessors agree (the program compares) and the verdicts equal
the Python twins'.  Then the refusals: every construct outside the language is named,
and the size limits hold."""
import ctypes as C
import os
import subprocess

import pytest

import rmc
from tests import invariant_cases as IC
from tests import predicate_cases as PC
from tests.convert import to_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")


def build_pred_check(exe, extra=()):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", *extra, "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "pred_check.cpp"),
                    os.path.join(CSRC, "rmc_front.cpp"), os.path.join(CSRC, "rmc_codec.cpp"), "-o", str(exe)],
                   check=True)


@pytest.fixture(scope="module")
def pred_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pred_check") / "pred_check"
    build_pred_check(exe)
    return str(exe)


@pytest.fixture(scope="module")
def view_files(tmp_path_factory):
    """One file of raw rmc_state_view records per model, shared by both groups."""
    d = tmp_path_factory.mktemp("pred_views")
    out = {}
    for name in sorted(IC.CASES):
        m, _ = IC.CASES[name]
        path = d / (name + ".bin")
        with open(path, "wb") as f:
            for s in IC.states(name):
                f.write(bytes(to_view(m, s)))
        assert os.path.getsize(path) == len(IC.states(name)) * C.sizeof(rmc.StateView)
        out[name] = str(path)
    return out


def run(exe, cfg, tla, views="-", S=3, K=4, out="-"):
    return subprocess.run([exe, cfg, tla, views, str(S), str(K), out], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("group", sorted(PC.GROUPS))
@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_host_vm_equals_the_twins_state_by_state(name, group, pred_check, view_files, tmp_path):
    m, _ = IC.CASES[name]
    packable = not name.startswith("wide")
    cfg, tla = PC.write_model(tmp_path, PC.GROUPS[group], n_servers=m.n_servers, n_values=m.n_values)
    out = tmp_path / "verdicts.bin"
    r = run(pred_check, cfg, tla, view_files[name], m.n_servers, IC.kcap(m) if packable else 0, str(out))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert [ln.split()[2] for ln in lines if ln.startswith("predicate ")] == list(PC.GROUPS[group])
    shapes = {ln.rsplit(" ", 1)[0]: int(ln.rsplit(" ", 1)[1]) for ln in lines if ln.startswith("shape ")}
    n = len(IC.states(name))
    assert shapes["shape view"] == n and shapes["shape wide full"] == n
    if packable:
        assert shapes["shape packed S=%d K=%d" % (m.n_servers, IC.kcap(m))] == n
    if name != "wide_s5":
        assert shapes["shape wide compact"] >= IC.N_PER_FAMILY // 2
    assert shapes["shape wide depth-sized"] > 0 or name.startswith("wide")
    got = out.read_bytes()
    np_ = len(PC.GROUPS[group])
    assert len(got) == n * np_
    want = PC.verdicts(name, group)
    for t in range(n):
        assert tuple(got[t * np_:(t + 1) * np_]) == want[t], (name, t, PC.GROUPS[group])


@pytest.mark.parametrize("group", sorted(PC.GROUPS))
def test_twins_show_every_verdict_they_can(group):
    """The inputs are not vacuous (from the twins alone): over the packed S = 3 models
    every Boolean predicate holds on at least 10 states and is violated on at least 10,
    and the two error predicates show both an error and a clean evaluation."""
    seen = {p: set() for p in PC.GROUPS[group]}
    count = {p: [0, 0, 0] for p in PC.GROUPS[group]}
    for name in sorted(IC.CASES):
        for row in PC.verdicts(name, group):
            for p, v in zip(PC.GROUPS[group], row):
                seen[p].add(v)
                count[p][v] += 1
    for p in PC.GROUPS[group]:
        if p in ("UserUnguardedLog", "UserWrongField"):
            assert seen[p] == {PC.HOLDS, PC.ERROR}, (p, count[p])
        else:
            assert seen[p] == {PC.HOLDS, PC.VIOLATED} and min(count[p][:2]) >= 10, (p, count[p])


def refusal(exe, tmp_path, body, invariant="Bad", **kw):
    cfg, tla = PC.write_model(tmp_path, [invariant], module=PC.module_with(body), **kw)
    r = run(exe, cfg, tla)
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout.startswith("refused: INVARIANT " + invariant), r.stdout
    return r.stdout


REFUSALS = [
    ("Bad == \\A i \\in Server : SubSeq(log[i], 1, 1) = SubSeq(log[i], 1, 1)", "SubSeq"),
    ("Bad == \\A i, j \\in Server : log[i] = log[j]", "sequence"),
    ("Bad == \\A i, j \\in Server : \\A n \\in DOMAIN log[i] : log[i][n] = log[j][n]", "record"),
    ("Bad == \\A m \\in DOMAIN messages : m.mentries = m.mentries", "m.mentries"),
    ("Bad == \\A m \\in DOMAIN messages : m.mlog = m.mlog", "m.mlog"),
    ("Bad == \\A m, k \\in DOMAIN messages : m = k", "record equality"),
    ("Bad == LET x == 1 IN x = 1", "LET"),
    ("Bad == (CHOOSE i \\in Server : TRUE) \\in Server", "CHOOSE"),
    ("Bad == currentTerm' = currentTerm", "primed"),
    ("Bad == [currentTerm EXCEPT ![r1] = 1] = currentTerm", "EXCEPT"),
    ("Bad == [i \\in Server |-> 1] = currentTerm", "function or record constructor"),
    ("Bad == \"a\" = \"a\"", "string"),
    ("Bad == \\A i \\in Server : \\A n \\in DOMAIN log[i] : log[i][n].value = v1", "Value-typed"),
    ("Bad == \\A i \\in Server : currentTerm[i] <= NoSuchName", "unknown identifier NoSuchName"),
    ("Bad == Cardinality(Server)", "not Boolean"),
    ("Loop(i) == Loop(i)\nBad == \\A i \\in Server : Loop(i)", "recursive definition Loop"),
    ("Bad == <<1, 2>> = <<1, 2>>", "tuple"),
    ("Bad == \\A i \\in Server : currentTerm[i] < Leader", "integer"),
]


@pytest.mark.parametrize("body,needle", REFUSALS, ids=[n for _b, n in REFUSALS])
def test_every_refusal_names_its_construct(body, needle, pred_check, tmp_path):
    out = refusal(pred_check, tmp_path, body)
    assert needle in out, out
    assert " line " in out and " col " in out or needle == "not Boolean", out


def test_refusal_gives_the_line_and_column_of_the_construct(pred_check, tmp_path):
    body = "Bad ==\n    /\\ TRUE\n    /\\ \\A i \\in Server : SubSeq(log[i], 1, 1) = SubSeq(log[i], 1, 1)"
    out = refusal(pred_check, tmp_path, body)
    module = PC.module_with(body).split("\n")
    line = next(k for k, ln in enumerate(module) if "SubSeq" in ln) + 1
    col = module[line - 1].index("SubSeq") + 1
    assert "SubSeq at line %d, col %d" % (line, col) in out, out


def test_size_limits(pred_check, tmp_path):
    # more than RMC_MAX_PREDICATES = 8 predicates
    body = "\n".join("P%d == \\A i \\in Server : currentTerm[i] >= %d" % (k, k) for k in range(9))
    cfg, tla = PC.write_model(tmp_path, ["P%d" % k for k in range(9)], module=PC.module_with(body))
    r = run(pred_check, cfg, tla)
    assert r.returncode == 3 and "9 model-defined invariants exceed RMC_MAX_PREDICATES = 8" in r.stdout, r.stdout
    # exactly 8 are accepted
    cfg, tla = PC.write_model(tmp_path, ["P%d" % k for k in range(8)], module=PC.module_with(body))
    assert run(pred_check, cfg, tla).returncode == 0
    # more than 8 bound names in scope
    names = ["a%d" % k for k in range(9)]
    out = refusal(pred_check, tmp_path, "Bad == \\A %s \\in Server : %s = %s" % (", ".join(names), names[0], names[8]))
    assert "9 bound names in scope exceed 8" in out, out
    # evaluation stack deeper than 16: a right-nested sum of 17 operands
    out = refusal(pred_check, tmp_path, "Bad == 0 <= " + " + (".join(["1"] * 18) + ")" * 17)
    assert "evaluation stack depth" in out and "exceeds 16" in out, out
    # more than 1024 code words in all
    conj = " /\\ ".join("currentTerm[i] + %d >= %d" % (k, k) for k in range(200))
    out = refusal(pred_check, tmp_path, "Bad == \\A i \\in Server : " + conj)
    assert "code words in all exceed 1024" in out, out


def test_known_invariants_keep_their_digest_rule(pred_check, tmp_path):
    """A definition under one of the ten compiled-in names that is not the compiled-in
    text is refused as before, predicates or not."""
    body = "OneLeaderPerTerm == \\A i \\in Server : state[i] /= Leader"
    cfg, tla = PC.write_model(tmp_path, ["OneLeaderPerTerm"], module=PC.module_with(body))
    r = run(pred_check, cfg, tla)
    assert r.returncode == 3 and "is not the one compiled into the engine" in r.stdout, r.stdout


def test_server_model_value_is_recorded(pred_check, tmp_path):
    cfg, tla = PC.write_model(tmp_path, ["UserNamesServer"])
    r = run(pred_check, cfg, tla)
    assert r.returncode == 0 and "names a server: 1" in r.stdout, r.stdout
    cfg, tla = PC.write_model(tmp_path, ["UserNoLeader"])
    r = run(pred_check, cfg, tla)
    assert r.returncode == 0 and "names a server: 0" in r.stdout, r.stdout
