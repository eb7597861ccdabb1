"""Generated predicates against the host VM (no GPU).  tests/predicate_gen.py generates
well-typed expressions of the predicate language, prints each twice (fully parenthesised;
minimal parentheses with bulleted junction lists) and evaluates it with an evaluator of its
own; the stand-alone programs tests/native/pred_check.cpp, act_check.cpp and cons_check.cpp
compile both texts with the front-end and run the interpreter of rmc_pred.h through every
state accessor.  The verdicts must be equal: integers, no tolerance."""
import os
import subprocess

import pytest

from oracle import raft_spec as R
from tests import action_cases as AC
from tests import invariant_cases as IC
from tests import predicate_cases as PC
from tests import predicate_gen as PG
from tests.convert import to_view
from tests.test_actions_native import SANITIZE, build_act_check, write_pairs
from tests.test_predicates_native import build_pred_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")
MODELS = sorted(IC.CASES)
INV = range(PG.N_INV_PROGRAMS)
ACT = range(PG.N_ACT_PROGRAMS)


@pytest.fixture(scope="module")
def pred_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pg_pred_check") / "pred_check"
    build_pred_check(exe)
    return str(exe)


@pytest.fixture(scope="module")
def act_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pg_act_check") / "act_check"
    build_act_check(exe)
    return str(exe)


@pytest.fixture(scope="module")
def view_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("pg_views")
    out = {}
    for name in MODELS:
        m, _ = IC.CASES[name]
        out[name] = str(d / (name + ".bin"))
        with open(out[name], "wb") as f:
            for s in PG.states(name):
                f.write(bytes(to_view(m, s)))
    return out


def run_pred_check(exe, tmp_path, prog, name, views, minimal, n_states=PG.N_STATES):
    """The host VM's verdict rows of a program on a model's states (every accessor agreeing)."""
    m, _ = IC.CASES[name]
    cfg, tla = PG.write_program(tmp_path, prog, m, minimal)
    out = tmp_path / "verdicts.bin"
    K = IC.kcap(m) if not name.startswith("wide") else 0
    r = subprocess.run([exe, cfg, tla, views, str(m.n_servers), str(K), str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (prog.names, minimal, r.stdout[-3000:] + r.stderr[-3000:], open(tla).read()[-6000:])
    lines = r.stdout.splitlines()
    assert [ln.split()[2] for ln in lines if ln.startswith("predicate ")] == list(prog.names)
    assert "shape view %d" % n_states in lines and "shape wide full %d" % n_states in lines
    if K:
        assert "shape packed S=%d K=%d %d" % (m.n_servers, K, n_states) in lines
    raw = out.read_bytes()
    n = len(prog.names)
    assert len(raw) == n * n_states
    return [tuple(raw[t * n:(t + 1) * n]) for t in range(n_states)]


def compare(got, want, what):
    """Verdict rows against the evaluator's, but for the cases that depend on the bag's order."""
    for t, (row, evs) in enumerate(zip(got, want)):
        for p, (v, ev) in enumerate(zip(row, evs)):
            assert ev.order_dependent or v == ev.verdict, (what, "case", t, "predicate", p, "engine", v, "evaluator",
                                                           ev.verdict)


@pytest.mark.parametrize("name", MODELS)
def test_host_vm_equals_the_evaluator_on_every_invariant_program(name, pred_check, view_files, tmp_path):
    for p in INV:
        prog = PG.program("inv", p)
        full = run_pred_check(pred_check, tmp_path, prog, name, view_files[name], False)
        mini = run_pred_check(pred_check, tmp_path, prog, name, view_files[name], True)
        assert full == mini, (name, p)  # two printings of one AST: equal verdicts, order-dependent cases included
        compare(full, PG.inv_verdicts(p, name), (name, p, prog.definitions(True)))


# ---- actions -------------------------------------------------------------------------------------
def run_act_check(exe, tmp_path, prog, name, K, minimal):
    m, _ = IC.CASES[name]
    cfg, tla = PG.write_program(tmp_path, prog, m, minimal)
    pairs, out = tmp_path / "pairs.bin", tmp_path / "verdicts.bin"
    if not pairs.exists():
        write_pairs(pairs, m, PG.pairs(name, K))
    r = subprocess.run([exe, cfg, tla, str(pairs), str(m.n_servers), str(K), str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (prog.names, minimal, r.stdout[-3000:] + r.stderr[-3000:], open(tla).read()[-6000:])
    lines = r.stdout.splitlines()
    assert [ln.split()[2] for ln in lines if ln.startswith("property ")] == list(prog.names)
    n, np_ = len(PG.pairs(name, K)), len(prog.names)
    assert lines[-1] == "ok %d" % (2 * np_ * n)  # the views, then the packed words with the strided successor column
    raw = out.read_bytes()
    assert len(raw) == np_ * n
    return [tuple(raw[t * np_:(t + 1) * np_]) for t in range(n)]


@pytest.mark.parametrize("name,K", AC.SHAPES, ids=["%s-K%d" % s for s in AC.SHAPES])
def test_host_vm_equals_the_evaluator_on_every_action_program(name, K, act_check, tmp_path):
    assert sum(1 for s, t in PG.pairs(name, K) if s == t) >= AC.N_SOURCES
    for p in ACT:
        prog = PG.program("act", p)
        full = run_act_check(act_check, tmp_path, prog, name, K, False)
        mini = run_act_check(act_check, tmp_path, prog, name, K, True)
        assert full == mini, (name, K, p)
        compare(full, PG.act_verdicts(p, name, K), (name, K, p, prog.definitions(True)))


# ---- residual conjuncts of a CONSTRAINT ----------------------------------------------------------
def unsplit(body):
    """The front-end takes a conjunction apart, also under one `\\A i \\in Server :`, and reads
    Cardinality(DOMAIN messages) <= N as a bound: such conjuncts would not stay one residual."""
    def conj(n):
        return n[0] == "bin" and n[1] == "/\\"
    if conj(body) or body[0] in ("card", "cardmsgs") or (body[0] == "bin" and body[2][0] in ("card", "cardmsgs")):
        return False
    if body[0] == "q" and body[1] == "\\A" and len(body[2]) == 1 and len(body[2][0][0]) == 1:
        return not conj(body[3])
    return True


def residual_programs():
    """(program, indices of its conjuncts) until 32 pool invariants are conjuncts."""
    out, n = [], 0
    for p in INV:
        prog = PG.program("inv", p)
        idx = [q for q, (_nm, b) in enumerate(prog.preds) if unsplit(b)][:32 - n]
        if idx:
            out.append((p, tuple(idx)))
            n += len(idx)
        if n == 32:
            break
    assert n == 32
    return out


@pytest.fixture(scope="module")
def cons_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pg_cons_check") / "cons_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "cons_check.cpp"),
                    os.path.join(CSRC, "rmc_front.cpp"), os.path.join(CSRC, "rmc_codec.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def constraint_module(prog, idx):
    """The program's module with the chosen predicates as further items of StateConstraint's list."""
    text = PG.module_text(prog, True)
    last = "    /\\ \\A m \\in DOMAIN messages : messages[m] <= MaxDup\n"
    assert text.count(last) == 1
    items = "".join("    /\\ " + "\n".join(PG.text_min(prog.preds[q][1], 7)) + "\n" for q in idx)
    return text.replace(last, last + items)


@pytest.mark.parametrize("name", ["fuzz0", "edge1"])
def test_pool_invariants_as_residual_conjuncts(name, cons_check, view_files, tmp_path):
    m, _ = IC.CASES[name]
    for p, idx in residual_programs():
        prog = PG.program("inv", p)
        cfg, tla = PC.write_model(tmp_path, (), n_servers=m.n_servers, n_values=m.n_values,
                                  module=constraint_module(prog, idx))
        out = tmp_path / "residuals.bin"
        r = subprocess.run([cons_check, "verdicts", cfg, tla, view_files[name], str(m.n_servers), str(out)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (p, idx, r.stdout[-3000:] + r.stderr[-3000:], open(tla).read()[-6000:])
        assert sum(1 for ln in r.stdout.splitlines() if ln.startswith("residual ")) == len(idx), r.stdout
        raw = out.read_bytes()
        assert len(raw) == len(idx) * PG.N_STATES
        got = [tuple(raw[t * len(idx):(t + 1) * len(idx)]) for t in range(PG.N_STATES)]
        compare(got, [tuple(row[q] for q in idx) for row in PG.inv_verdicts(p, name)], (name, p, idx))


# ---- the sanitizers --------------------------------------------------------------------------------
def test_pool_under_the_sanitizers(view_files, tmp_path):
    """Each stand-alone program built with -fsanitize=address,undefined and run directly over the pool."""
    pred_san, act_san = str(tmp_path / "pred_check_san"), str(tmp_path / "act_check_san")
    build_pred_check(pred_san, SANITIZE)
    build_act_check(act_san, SANITIZE)
    for p in INV:
        prog = PG.program("inv", p)
        compare(run_pred_check(pred_san, tmp_path, prog, "edge1", view_files["edge1"], True),
                PG.inv_verdicts(p, "edge1"), ("edge1", p))
    for p in ACT:
        prog = PG.program("act", p)
        compare(run_act_check(act_san, tmp_path, prog, "edge1", 8, True), PG.act_verdicts(p, "edge1", 8), ("edge1", p))


# ---- non-vacuity, from the evaluator alone -----------------------------------------------------------
def all_cases():
    """(kind, program, model key, [per case: tuple of Evaluated])."""
    for p in INV:
        for name in MODELS:
            yield "inv", p, name, PG.inv_verdicts(p, name)
    for p in ACT:
        for name, K in AC.SHAPES:
            yield "act", p, (name, K), PG.act_verdicts(p, name, K)


def test_every_production_occurs_in_at_least_four_pool_predicates():
    count = {t: 0 for t in PG.PRODUCTIONS + PG.ACTION_PRODUCTIONS}
    for kind, n in (("inv", PG.N_INV_PROGRAMS), ("act", PG.N_ACT_PROGRAMS)):
        for p in range(n):
            prog = PG.program(kind, p)
            for q in range(len(prog.preds)):
                for t in prog.productions(q):
                    count[t] += 1
    assert sum(len(PG.program("inv", p).preds) for p in INV) == 128
    assert sum(len(PG.program("act", p).preds) for p in ACT) == 64
    few = {t: c for t, c in count.items() if c < 4}
    assert not few, few


def test_the_cases_are_not_vacuous():
    seen, sources, masked = {}, {"log": 0, "nil": 0, "field": 0}, {t: 0 for t in ("/\\", "\\/", "=>", "IF", "\\A", "\\E")}
    nil_iter = nil_card = 0
    quorum_at = set()
    od = {}
    for kind, p, key, rows in all_cases():
        S = IC.CASES[key if kind == "inv" else key[0]][0].n_servers
        tot = od.setdefault((kind, key), [0, 0])
        for row in rows:
            for q, ev in enumerate(row):
                seen.setdefault((kind, p, q), set()).add(ev.verdict)
                tot[0] += 1
                if ev.order_dependent:
                    tot[1] += 1
                    continue
                if ev.verdict == PG.ERROR:
                    sources[ev.error_source] += 1
                for t in ev.masked:
                    masked[t] += 1
                nil_iter += ev.nil_iter
                nil_card += ev.nil_card
                if ev.quorum_iter:
                    quorum_at.add(S)
    for (kind, p, q), vs in seen.items():
        prog = PG.program(kind, p)
        if PG.reads_state(prog.preds[q][1], prog.helpers):
            assert len(vs) >= 2, (prog.preds[q][0], vs)
    assert min(sources.values()) >= 10, sources
    assert min(masked.values()) >= 10, masked
    assert nil_iter >= 10 and nil_card >= 10, (nil_iter, nil_card)
    assert quorum_at == {2, 3, 4, 5}
    # the bag's order decides at most 3 % of a model's cases (they are left out of the comparison)
    for key, (n, dep) in od.items():
        assert dep * 100 <= 3 * n, (key, n, dep)


# ---- the evaluator and printer (b) by hand: answers independent of the engine -----------------------
def hand_state():
    """S = 3: r1 a leader of term 2 with log <<(1, v1), (2, v2)>>, r2 a follower of term 3 with an empty
    log that voted for nobody, r3 a candidate of term 3 with log <<(1, v1)>> that voted for itself."""
    s = R.init_state(R.Model(n_servers=3))
    rvq = R.rec(mtype=R.RVQ, mterm=3, mlastLogTerm=1, mlastLogIndex=1, msource=2, mdest=0)
    return s._replace(currentTerm=(2, 3, 3), state=(R.LEADER, R.FOLLOWER, R.CANDIDATE), votedFor=(0, R.NIL, 2),
                      log=((R.entry(1, 0), R.entry(2, 1)), (), (R.entry(1, 0),)), commitIndex=(1, 0, 0),
                      votesGranted=(frozenset({0, 1}), frozenset(), frozenset({2})), messages=frozenset({(rvq, 2)}))


def _v(x):
    return ("var", x)


def _n(x):
    return ("num", x)


def _q(q, name, dom, body):
    return ("q", q, (((name,), dom),), body)


SERVER = ("d_set", ("server_set",))
R1, R2, R3 = ("srv", 0), ("srv", 1), ("srv", 2)
ERR = ("bin", "=", ("logterm", ("log", R2, False), _n(1)), _n(0))   # log[r2][1] of an empty log
T, F = ("true",), ("false",)
TERM1 = lambda i, v: ("bin", "=", ("logterm", ("log", _v(i), False), _n(1)), _n(v))   # log[i][1].term = v
HAND_DEFS = {
    "Other": (("x",), _q("\\E", "i", SERVER, ("bin", "/=", _v("i"), _v("x")))),
    "Less": (("x", "y"), ("bin", "<", ("sv", "currentTerm", _v("x"), False), ("sv", "currentTerm", _v("y"), False))),
    "Last": (("l",), ("lastterm", _v("l"))),
    "Via": (("x",), ("call", "Last", (("log", _v("x"), False),))),
}
NILSET = ("setlit", (R1, ("nil",)))
HAND = [  # (predicate, verdict on hand_state())
    (("bin", "=", ("bin", "-", ("bin", "-", _n(1), _n(2)), _n(3)), _n(-4)), 0),        # 1 - 2 - 3 = -4
    (("bin", "=", ("bin", "-", _n(1), ("bin", "-", _n(2), _n(3))), _n(2)), 0),         # 1 - (2 - 3) = 2
    (_q("\\A", "i", SERVER, ("call", "Other", (_v("i"),))), 0),                        # the caller's i, not Other's
    (("call", "Less", (R2, R1)), 1), (("call", "Less", (R1, R2)), 0),                  # 3 < 2, 2 < 3
    (_q("\\A", "n", ("d_range", _n(2), _n(1)), F), 0), (_q("\\E", "n", ("d_range", _n(2), _n(1)), T), 1),
    (_q("\\E", "n", ("d_cap", _n(1), _n(2), _n(3), _n(4)), T), 1),                     # an empty meet
    (("bin", "=", ("card", ("setcomp", "i", NILSET, T)), _n(2)), 0),                   # Nil iterated and counted
    (("in", "\\in", ("nil",), ("d_set", NILSET)), 0),
    (("in", "\\in", NILSET, ("d_quorum",)), 1), (("in", "\\in", ("setlit", (R1, R2)), ("d_quorum",)), 0),
    (("bin", "=", ("bin", "\\", NILSET, ("setlit", (("nil",),))), ("setlit", (R1,))), 0),
    (("bin", "\\/", T, ERR), 0), (("bin", "\\/", F, ERR), 2),                           # an error after a deciding disjunct
    (("q", "\\A", ((("i",), SERVER), (("n",), ("d_log", ("log", _v("i"), False)))),
      ("bin", "<=", ("logterm", ("log", _v("i"), False), _v("n")), ("sv", "currentTerm", _v("i"), False))), 0),
    (("if", ("bin", "=", ("sv", "state", R1, False), ("role", "Leader")),
      ("bin", "/\\", ("bin", "/\\", T, ("bin", "\\/", ("bin", "\\/", F, ("bin", "/\\", ("bin", "/\\", T, T),
                                                                              ("bin", "=", _n(1), _n(1)))), F)), T), F), 0),
    (_q("\\E", "i", ("d_set", NILSET), ("bin", "=", ("sv", "currentTerm", _v("i"), False), _n(2))), 0),   # r1 first
    (_q("\\A", "i", ("d_set", NILSET), ("bin", "=", ("sv", "currentTerm", _v("i"), False), _n(2))), 2),   # then Nil
    (_q("\\A", "i", ("d_set", ("setlit", (("nil",), R2))), ("bin", "=", ("sv", "currentTerm", _v("i"), False), _n(2))), 1),
    (_q("\\A", "m", ("d_msgs", False), ("mf", _v("m"), "mvoteGranted")), 2),           # a field of another type
    (("bin", "=", ("sv", "currentTerm", ("sv", "votedFor", R2, False), False), _n(0)), 2),   # indexed by Nil
    (("not", ("bin", "=", _n(1), _n(2))), 0), (("bin", "=", ("bin", "-", _n(2), _n(-1)), _n(3)), 0),
    (_q("\\A", "i", ("d_quorum",), _q("\\E", "j", ("d_set", _v("i")), ("bin", "/=", ("sv", "state", _v("j"), False),
                                                                        ("role", "Follower")))), 0),
    (("bin", "=", ("call", "Via", (R1,)), _n(2)), 0),                                  # a log through two definitions
    # one masked and one unmasked error per short-circuiting construct
    (("bin", "/\\", F, ERR), 1), (("bin", "/\\", T, ERR), 2), (("bin", "=>", F, ERR), 0), (("bin", "=>", T, ERR), 2),
    (("if", T, T, ERR), 0), (("if", F, T, ERR), 2),
    (_q("\\A", "i", SERVER, TERM1("i", 5)), 1), (_q("\\A", "i", SERVER, TERM1("i", 1)), 2),
    (_q("\\E", "i", SERVER, TERM1("i", 1)), 0), (_q("\\E", "i", SERVER, TERM1("i", 5)), 2),
]
MASKED = {"/\\": ("bin", "/\\", F, ERR), "\\/": ("bin", "\\/", T, ERR), "=>": ("bin", "=>", F, ERR), "IF": ("if", T, T, ERR),
          "\\A": _q("\\A", "i", SERVER, TERM1("i", 5)), "\\E": _q("\\E", "i", SERVER, TERM1("i", 1))}


def test_evaluator_by_hand():
    s = hand_state()
    evs = [PG.evaluate(PG.compile_predicate(HAND_DEFS, b), 3, s) for b, _w in HAND]
    assert [ev.verdict for ev in evs] == [w for _b, w in HAND]
    at = {b: k for k, (b, _w) in enumerate(HAND)}
    for tag, b in MASKED.items():   # the part left out would have been an error, and the evaluator says so
        assert evs[at[b]].masked == {tag} and HAND[at[b]][1] != PG.ERROR, (tag, evs[at[b]].masked)
    assert all(not ev.masked for ev in evs if ev.verdict == PG.ERROR)
    sources = {ev.error_source for ev in evs}
    assert sources == {None, "field", "nil", "log"}
    assert evs[at[("bin", "\\/", F, ERR)]].error_source == "log"


def test_stutter_rule_by_hand():
    s = hand_state()
    t = s._replace(commitIndex=(2, 0, 0))
    grows = _q("\\A", "i", SERVER, ("bin", ">", ("sv", "commitIndex", _v("i"), True), ("sv", "commitIndex", _v("i"), False)))
    f, g, e = (PG.compile_predicate({}, b) for b in (F, grows, ERR))
    assert PG.evaluate(f, 3, s, t).verdict == PG.VIOLATED and PG.evaluate(f, 3, s, s).verdict == PG.HOLDS
    assert PG.evaluate(g, 3, s, t).verdict == PG.VIOLATED and PG.evaluate(g, 3, s, s).verdict == PG.HOLDS
    assert PG.evaluate(e, 3, s, s).verdict == PG.ERROR   # an error stays an error
    primed = ("prime", ("bin", "=", ("sv", "commitIndex", R1, False), _n(2)))   # (commitIndex[r1] = 2)'
    assert PG.evaluate(PG.compile_predicate({}, primed), 3, s, t).verdict == PG.HOLDS


def test_the_engine_agrees_on_the_hand_made_predicates(pred_check, tmp_path):
    """The same predicates through both printers, the front-end and the host VM, on the same state."""
    m = R.Model(n_servers=3, n_values=2)
    helpers = {nm: (ps, None, None, b) for nm, (ps, b) in HAND_DEFS.items()}
    with open(tmp_path / "views.bin", "wb") as f:
        f.write(bytes(to_view(m, hand_state())))
    for lo in range(0, len(HAND), 8):
        chunk = HAND[lo:lo + 8]
        prog = PG.Program(helpers, [("Hand%d" % (lo + k), b) for k, (b, _w) in enumerate(chunk)], False)
        for minimal in (False, True):
            cfg, tla = PG.write_program(tmp_path, prog, m, minimal)
            out = tmp_path / "hand.bin"
            r = subprocess.run([pred_check, cfg, tla, str(tmp_path / "views.bin"), "3", "4", str(out)],
                               capture_output=True, text=True, timeout=60)
            assert r.returncode == 0, r.stdout + open(tla).read()[-3000:]
            assert list(out.read_bytes()) == [w for _b, w in chunk], (lo, minimal)


A, B_, C_, D = (("bin", "=", ("sv", "commitIndex", _v("i"), False), _n(k)) for k in range(4))
PRINTED = [  # (AST, printer (b)'s text from column 4)
    (("bin", "=>", ("bin", "<=>", A, B_), C_), "commitIndex[i] = 0 <=> commitIndex[i] = 1 => commitIndex[i] = 2"),
    (("bin", "<=>", A, ("bin", "=>", B_, C_)), "commitIndex[i] = 0 <=> (commitIndex[i] = 1 => commitIndex[i] = 2)"),
    (("bin", "/\\", ("bin", "\\/", A, B_), C_), "(commitIndex[i] = 0 \\/ commitIndex[i] = 1) /\\ commitIndex[i] = 2"),
    (("not", ("bin", "=", _n(1), _n(2))), "~1 = 2"),
    (("bin", "=", ("not", T), F), "(~TRUE) = FALSE"),
    (("bin", "-", ("bin", "-", _n(1), _n(2)), _n(3)), "1 - 2 - 3"),
    (("bin", "-", _n(1), ("bin", "-", _n(2), _n(3))), "1 - (2 - 3)"),
    (("bin", "-", ("bin", "+", _n(1), _n(2)), _n(-3)), "(1 + 2) - -3"),
    (("bin", "+", _n(1), ("bin", "-", _n(2), _n(3))), "1 + 2 - 3"),
    (("bin", "\\cup", ("bin", "\\cap", NILSET, ("server_set",)), NILSET), "({r1, Nil} \\cap Server) \\cup {r1, Nil}"),
    (("bin", "/\\", _q("\\A", "i", SERVER, A), T), "(\\A i \\in Server : commitIndex[i] = 0) /\\ TRUE"),
    (("bin", "/\\", T, _q("\\A", "i", SERVER, A)), "TRUE /\\ \\A i \\in Server : commitIndex[i] = 0"),
    (("bin", "+", ("if", T, _n(1), _n(2)), _n(3)), "(IF TRUE THEN 1 ELSE 2) + 3"),
    # a chain of two or more junctions is a bulleted list; a nested list is indented deeper
    (("bin", "/\\", ("bin", "/\\", A, ("bin", "\\/", ("bin", "\\/", B_, C_), D)), T),
     "/\\ commitIndex[i] = 0\n    /\\ \\/ commitIndex[i] = 1\n       \\/ commitIndex[i] = 2\n"
     "       \\/ commitIndex[i] = 3\n    /\\ TRUE"),
    # a list item ended by a token left of the bullets' column: no parentheses round the list
    (("bin", "=>", ("bin", "/\\", ("bin", "/\\", A, B_), C_), D),
     "   /\\ commitIndex[i] = 0\n       /\\ commitIndex[i] = 1\n       /\\ commitIndex[i] = 2\n    => commitIndex[i] = 3"),
    (("if", A, ("bin", "\\/", ("bin", "\\/", B_, C_), D), F),
     "IF commitIndex[i] = 0\n    THEN \\/ commitIndex[i] = 1\n         \\/ commitIndex[i] = 2\n"
     "         \\/ commitIndex[i] = 3\n    ELSE FALSE"),
]


def test_printer_b_by_hand():
    for ast, text in PRINTED:
        assert "\n".join(PG.text_min(ast, 4)) == text, ast


def test_order_dependence_is_flagged_by_hand():
    """Two messages, one on which the body is an error and one that decides: either verdict is
    possible, so the evaluator flags the case; where every element errs, or none decides, it does not."""
    s = hand_state()
    rvp = R.rec(mtype=R.RVP, mterm=3, mvoteGranted=True, mlog=(), msource=1, mdest=2)
    two = s._replace(messages=frozenset(s.messages | {(rvp, 1)}))
    granted = _q("\\E", "m", ("d_msgs", False), ("mf", _v("m"), "mvoteGranted"))   # TRUE on one, no field on the other
    none = _q("\\A", "m", ("d_msgs", False), ("mf", _v("m"), "mvoteGranted"))      # TRUE decides no \A
    ev = PG.evaluate(PG.compile_predicate({}, granted), 3, two)
    assert ev.order_dependent
    ev = PG.evaluate(PG.compile_predicate({}, none), 3, two)
    assert not ev.order_dependent and ev.verdict == PG.ERROR and ev.error_source == "field"
    ev = PG.evaluate(PG.compile_predicate({}, granted), 3, s)
    assert not ev.order_dependent and ev.verdict == PG.ERROR


def test_the_limit_predicates_sit_exactly_at_the_limits(pred_check, tmp_path):
    """deep_sum(15) and deep_scope(8) are in the pool and compile; one more of either is refused with
    the count: stack depth 17, 9 bound names."""
    m = R.Model(n_servers=3, n_values=2)
    assert PG.program("inv", 0).preds[0][1] == PG.deep_sum(15) and PG.program("inv", 0).preds[1][1] == PG.deep_scope(8)
    for body, needle in ((PG.deep_sum(16), "evaluation stack depth 17 exceeds 16"),
                         (PG.deep_scope(9), "9 bound names in scope exceed 8")):
        for minimal in (False, True):
            cfg, tla = PG.write_program(tmp_path, PG.Program({}, [("Over", body)], False), m, minimal)
            r = subprocess.run([pred_check, cfg, tla, "-", "3", "4", "-"], capture_output=True, text=True, timeout=60)
            assert r.returncode == 3 and needle in r.stdout, r.stdout
    for body in (PG.deep_sum(15), PG.deep_scope(8)):
        cfg, tla = PG.write_program(tmp_path, PG.Program({}, [("AtLimit", body)], False), m, True)
        r = subprocess.run([pred_check, cfg, tla, "-", "3", "4", "-"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout


SHIFTED = """Shifted ==
    \\A i \\in Server :  /\\ currentTerm[i] < 0
                      /\\ TRUE \\/ currentTerm[i] >= 0"""


def test_a_bullet_left_of_its_list_is_an_infix_operator(pred_check, tmp_path):
    """The second /\\ stands one column left of the first, so it is no item of that list: the list
    ends there and the text reads (currentTerm[i] < 0 /\\ TRUE) \\/ currentTerm[i] >= 0, which
    holds.  As an item of the list it would read currentTerm[i] < 0 /\\ (TRUE \\/ ...): violated."""
    m = R.Model(n_servers=3, n_values=2)
    cfg, tla = PC.write_model(tmp_path, ("Shifted",), module=PC.module_with(SHIFTED))
    with open(tmp_path / "views.bin", "wb") as f:
        f.write(bytes(to_view(m, hand_state())))
    out = tmp_path / "shifted.bin"
    r = subprocess.run([pred_check, cfg, tla, str(tmp_path / "views.bin"), "3", "4", str(out)], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert list(out.read_bytes()) == [PG.HOLDS]


def test_stuttering_pairs_meet_violated_bodies():
    """Without the stutter rule these cases would read violated: every shape has some."""
    for name, K in AC.SHAPES:
        n = sum(1 for p in ACT for row, (s, t) in zip(PG.act_verdicts(p, name, K), PG.pairs(name, K)) if s == t
                for ev in row if ev.raw == PG.VIOLATED and ev.verdict == PG.HOLDS)
        assert n >= 10, (name, K, n)


def test_the_pool_has_cases_for_the_bfs_passes():
    """From the evaluator over the oracle's graph of graph_cases.TINY2 alone: at least two invariants
    and two action properties whose first level without HOLDS is 3 or later, one of each ending in an
    error, each beside a predicate of its program that holds everywhere.  For one action case an
    engine that read the current state in place of the successor would report another depth."""
    model, levels = PG.reachable_levels()
    assert sum(len(sts) for sts, _steps in levels) == 12975
    for kind in ("inv", "act"):
        cases = PG.bfs_cases(kind)
        assert len(cases) >= 2 and cases[0][3] == {PG.ERROR}, (kind, cases)
        assert all(c[2] >= 3 and c[4] for c in cases)
    shifted = []
    for p, q, depth, _v, _h in PG.bfs_cases("act"):
        fn = PG.program("act", p).compiled()[q]
        other = None
        for lv, (_sts, steps) in enumerate(levels, 1):
            if any(r == PG.ERROR or (r == PG.VIOLATED and s != t)
                   for s, t in steps for r in [PG.evaluate(fn, model.n_servers, s, s).raw]):
                other = lv + 1
                break
        shifted.append(other != depth)
    assert any(shifted)
