"""Action properties on the host (no GPU): tests/native/act_check.cpp, the front-end
(rmc_front.cpp) and rmc_codec.cpp compiled with plain g++ and no ROCm include path.  The
properties of tests/action_cases.py are compiled to bytecode and the two-state interpreter of
rmc_pred.h evaluates them on the pairs of tests/action_cases.py through the view accessors and
through the device pass's accessors (the packed words in place, the successor as a strided
column): the two agree (the program compares) and the verdicts equal the Python twins' with the
stutter rule applied.  Then the refusals: every construct outside the language is named with
its line and column, the limits hold, and without RMC_FRONT_ACTIONS nothing changes."""
import os
import subprocess

import pytest

import rmc
from tests import action_cases as AC
from tests import invariant_cases as IC
from tests.convert import to_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def build_act_check(exe, flags=("-O2",)):
    subprocess.run(["g++", *flags, "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "act_check.cpp"),
                    os.path.join(CSRC, "rmc_front.cpp"), os.path.join(CSRC, "rmc_codec.cpp"), "-o", str(exe)],
                   check=True)


@pytest.fixture(scope="module")
def act_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("act_check") / "act_check"
    build_act_check(exe)
    return str(exe)


@pytest.fixture(scope="module")
def act_check_san(tmp_path_factory):
    exe = tmp_path_factory.mktemp("act_check_san") / "act_check_san"
    build_act_check(exe, SANITIZE)
    return str(exe)


def write_pairs(path, model, pairs):
    with open(path, "wb") as f:
        for s, t in pairs:
            f.write(bytes(to_view(model, s)))
            f.write(bytes(to_view(model, t)))


def run(exe, cfg, tla, pairs="-", S=3, K=4, out="-", options=None):
    cmd = [exe, cfg, tla, str(pairs), str(S), str(K), str(out)] + ([str(options)] if options is not None else [])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def host_verdicts(exe, tmp_path, name, K, group):
    m, _ = IC.CASES[name]
    cfg, tla = AC.write_model(tmp_path, AC.GROUPS[group], n_servers=m.n_servers, n_values=m.n_values)
    pairs, out = tmp_path / "pairs.bin", tmp_path / "verdicts.bin"
    write_pairs(pairs, m, AC.pairs(name, K))
    r = run(exe, cfg, tla, pairs, m.n_servers, K, out)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert [ln.split()[2] for ln in lines if ln.startswith("property ")] == list(AC.GROUPS[group])
    for p in AC.GROUPS[group]:  # the note line of rmc_model_from_files names each
        assert "PROPERTY %s: action property" % p in r.stdout
    np_ = len(AC.GROUPS[group])
    assert lines[-1] == "ok %d" % (2 * np_ * len(AC.pairs(name, K)))
    raw = out.read_bytes()
    assert len(raw) == np_ * len(AC.pairs(name, K))
    return [tuple(raw[t * np_:(t + 1) * np_]) for t in range(len(AC.pairs(name, K)))]


@pytest.mark.parametrize("group", sorted(AC.GROUPS))
@pytest.mark.parametrize("name,K", AC.SHAPES, ids=["%s-K%d" % s for s in AC.SHAPES])
def test_host_vm_equals_the_twins_pair_by_pair(name, K, group, act_check, tmp_path):
    got = host_verdicts(act_check, tmp_path, name, K, group)
    want = AC.verdicts(name, K, group)
    for t, row in enumerate(got):
        assert row == want[t], (name, K, t, AC.GROUPS[group])


@pytest.mark.parametrize("group", sorted(AC.GROUPS))
@pytest.mark.parametrize("name,K", [("fuzz2", 4), ("edge1", 8)])
def test_host_vm_under_the_sanitizers(name, K, group, act_check_san, tmp_path):
    """The stand-alone program built with -fsanitize=address,undefined, run directly."""
    assert list(AC.verdicts(name, K, group)) == host_verdicts(act_check_san, tmp_path, name, K, group)


def test_stutter_rule_is_what_makes_the_constant_false_body_hold():
    p = AC.GROUPS["c"].index("AlwaysFalse")
    for name, K in AC.SHAPES:
        for (s, t), row in zip(AC.pairs(name, K), AC.verdicts(name, K, "c")):
            assert row[p] == (AC.HOLDS if s == t else AC.VIOLATED)


def test_front_option_value_and_exports():
    assert rmc.FRONT_ACTIONS == 32 and rmc.ACT_USER0 == 1 << 24 and rmc.MAX_ACTION_PROPS == 4
    text = open(os.path.join(ROOT, "include", "rmc.h")).read()
    assert "#define RMC_FRONT_ACTIONS (1u << 5)" in text and "#define RMC_ACT_USER0 (1u << 24)" in text
    assert "#define RMC_MAX_ACTION_PROPS 4" in text and "#define RMC_ABI_VERSION 16" in text
    new = ("rmc_actions_from_files", "rmc_set_actions", "rmc_eval_actions", "rmc_action_violation")
    assert all(n in rmc.EXPORTS for n in new)
    lib = os.path.join(ROOT, "raft.tla_amd", "lib", "librmc.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for n in new:
        assert " T %s\n" % n in syms, n


def refusal(exe, tmp_path, body, prop="Bad", **kw):
    cfg, tla = AC.write_model(tmp_path, [prop] if isinstance(prop, str) else prop, module=AC.module_with(body), **kw)
    r = run(exe, cfg, tla)
    assert r.returncode == 3, r.stdout + r.stderr
    assert r.stdout.startswith("refused: "), r.stdout
    return r.stdout


def where(body, needle, nth=0):
    """" at line L, col C" of the nth occurrence of needle in the module with `body`."""
    lines = AC.module_with(body).split("\n")
    hits = [(k + 1, c + 1) for k, ln in enumerate(lines) for c in range(len(ln)) if ln.startswith(needle, c)]
    hits = [h for h in hits if lines[h[0] - 1] in body.split("\n")]
    return " at line %d, col %d" % hits[nth]


# (definitions, message fragment, the token the line:column points at, which occurrence)
REFUSALS = [
    ("Bad == [][\\A i \\in Server : currentTerm'[i] >= currentTerm[i]]_<<currentTerm, state>>",
     "the subscript <<currentTerm,state>>", "_<<", 0),
    ("Bad == [][\\A i \\in Server : currentTerm'[i] >= currentTerm[i]]_currentTerm",
     "the subscript currentTerm", "_currentTerm", 0),
    ("Bad == <>(\\A i \\in Server : state[i] = Leader)", "<> (eventually)", "<>", 0),
    ("Bad == [][TRUE]_vars /\\ WF_vars(Next)", "WF_ (weak fairness)", "WF_vars", 0),
    ("Bad == (\\A i \\in Server : state[i] = Leader) ~> (\\A i \\in Server : state[i] = Follower)",
     "~> (leads to)", "~>", 0),
    ("Bad == []NoLeader", "[] applied to a state predicate", "[]", 0),
    ("Bad == [][UNCHANGED currentTerm]_vars", "UNCHANGED", "UNCHANGED", 0),
    ("Bad == [][ENABLED Next]_vars", "ENABLED", "ENABLED", 0),
    ("Bad == [][currentTerm' = [currentTerm EXCEPT ![r1] = 1]]_vars", "EXCEPT", "EXCEPT", 0),
    ("Bad == [][\\A i \\in Server : (currentTerm'[i] + 1)' >= 0]_vars",
     "a prime inside an already primed expression", "'[i]", 0),
    ("Bad == [][(NoLeader')']_vars", "a prime inside an already primed expression", "')'", 0),
    ("Bad == [][\\A m \\in DOMAIN messages : messages'[m] >= 1]_vars",
     "a message bound in DOMAIN messages as an index of messages'", "[m]", 0),
    ("Bad == [][\\A m \\in DOMAIN messages' : messages[m] >= 1]_vars",
     "a message bound in DOMAIN messages' as an index of messages", "[m]", 0),
    ("Bad == [][log' = log]_vars", "the variable log as a whole (function, sequence or record equality", "log'", 0),
    ("Bad == [][\\A i \\in Server : log'[i] = log[i]]_vars", "the sequence log[i] as a value", "[i]", 0),
]


@pytest.mark.parametrize("body,needle,token,nth", REFUSALS, ids=[r[1][:40] for r in REFUSALS])
def test_every_refusal_names_its_construct_with_line_and_column(body, needle, token, nth, act_check, tmp_path):
    out = refusal(act_check, tmp_path, body)
    assert out.startswith("refused: PROPERTY Bad"), out
    assert needle in out, out
    assert where(body, token, nth) in out, (out, where(body, token, nth))


def test_liveness_refusals_say_liveness(act_check, tmp_path):
    for body in [r[0] for r in REFUSALS[2:6]]:
        assert "liveness" in refusal(act_check, tmp_path, body)


def test_five_properties_are_refused_with_the_count(act_check, tmp_path):
    body = "\n".join("Q%d == [][\\A i \\in Server : currentTerm'[i] + %d >= currentTerm[i]]_vars" % (k, k)
                     for k in range(5))
    out = refusal(act_check, tmp_path, body, prop=["Q%d" % k for k in range(5)])
    assert "5 action properties exceed RMC_MAX_ACTION_PROPS = 4" in out, out
    cfg, tla = AC.write_model(tmp_path, ["Q%d" % k for k in range(4)], module=AC.module_with(body))
    assert run(act_check, cfg, tla).returncode == 0


def test_shared_limits_hold_for_properties(act_check, tmp_path):
    out = refusal(act_check, tmp_path, "Bad == [][0 <= " + " + (".join(["1"] * 18) + ")" * 17 + "]_vars")
    assert "evaluation stack depth" in out and "exceeds 16" in out, out
    names = ["a%d" % k for k in range(9)]
    out = refusal(act_check, tmp_path, "Bad == [][\\A %s \\in Server : %s = %s]_vars" % (", ".join(names), names[0], names[8]))
    assert "9 bound names in scope exceed 8" in out, out
    conj = " /\\ ".join("currentTerm'[i] + %d >= %d" % (k, k) for k in range(200))
    out = refusal(act_check, tmp_path, "Bad == [][\\A i \\in Server : " + conj + "]_vars")
    assert "code words in all exceed 1024" in out, out


def test_prime_in_an_invariant_stays_refused(tmp_path):
    """INVARIANT and CONSTRAINT bodies keep today's refusal of a prime, ACTIONS or not."""
    body = "BadInv == \\A i \\in Server : currentTerm'[i] >= currentTerm[i]"
    cfg, tla = AC.write_model(tmp_path, ["TermsMonotonic"], module=AC.module_with(body), invariants=["BadInv"])
    with pytest.raises(rmc.RmcError, match=r"INVARIANT BadInv: in BadInv: a primed variable \(a state predicate reads one state\) at "
                                           r"line \d+, col \d+"):
        rmc.Predicates(cfg, tla, builtin_raft=True, options=rmc.FRONT_ACTIONS)


def test_without_the_option_the_old_refusal_is_unchanged(act_check, tmp_path):
    cfg, tla = AC.write_model(tmp_path, ["TermsMonotonic", "CommitMonotonic"])
    r = run(act_check, cfg, tla, options=rmc.FRONT_BUILTIN_RAFT)
    assert r.returncode == 3 and r.stdout == "refused: PROPERTY TermsMonotonic (liveness) is out of scope\n", r.stdout
    with pytest.raises(rmc.RmcError, match=r"^.*PROPERTY TermsMonotonic \(liveness\) is out of scope$"):
        rmc.load_model(cfg, tla, builtin_raft=True, predicates=True, constraints=True)
    out = rmc.load_model(cfg, tla, builtin_raft=True, actions=True)
    assert out[-1].names == ["TermsMonotonic", "CommitMonotonic"]
    assert out[-1].name_of(rmc.ACT_USER0 << 1) == "CommitMonotonic"


def test_programs_without_primes_encode_as_before_and_primed_reads_are_flagged(act_check, tmp_path):
    cfg, tla = AC.write_model(tmp_path, ["AlwaysFalse"])
    r = run(act_check, cfg, tla)
    assert r.returncode == 0 and " 0 primed reads" in r.stdout, r.stdout
    cfg, tla = AC.write_model(tmp_path, ["TermsMonotonic"])
    r = run(act_check, cfg, tla)
    assert r.returncode == 0 and " 1 primed reads" in r.stdout, r.stdout


def test_server_model_value_is_recorded(act_check, tmp_path):
    cfg, tla = AC.write_model(tmp_path, ["NamesR1"])
    assert "names a server: 1" in run(act_check, cfg, tla).stdout
    cfg, tla = AC.write_model(tmp_path, ["TermsMonotonic"])
    assert "names a server: 0" in run(act_check, cfg, tla).stdout


def test_shipped_example_model_compiles(act_check):
    cfg = os.path.join(ROOT, "specs", "actions", "MCraftActions.cfg")
    tla = os.path.join(ROOT, "specs", "actions", "MCraftActions.tla")
    r = run(act_check, cfg, tla)
    assert r.returncode == 0, r.stdout
    assert [ln.split()[2] for ln in r.stdout.splitlines() if ln.startswith("property ")] == \
        ["TermsMonotonic", "LeaderAppendOnly", "VoteOncePerTerm"]
