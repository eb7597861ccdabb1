"""Continue past violations (RMC_FLAG_CONTINUE, TLC -continue): the search does
not stop at a violated invariant, stores and expands the violating states, and
counts them per invariant (rmc_get_violations, rmc_trace_violation, rmc-tlc
-continue).

The expected values come from a continue-mode BFS over the Python restatement
of the spec (tests/continue_cases.py), stored by tests/golden/make_continue_golden.py
in tests/golden/continue_cases.json; the smallest case is recomputed live.  The
cases have first != each (a state that violates two invariants counts once in
`first`, under its lowest bit, and in both rows of `each`), a seed level and a
last level that is never expanded."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import rmc
from tests import continue_cases, convert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "continue_cases.json")))
LEVELS = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_levels.json")))
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
SPECS = os.path.join(ROOT, "specs")
PACKED = ["bug_small_d12", "bug_small_sym_d12", "bug_s2_msgs2_full", "bug_msgs5_d9", "bug_s5_d8", "small_d15",
          "tiny2_full"]
ROW1, ROW3 = "bug_small_d12", "bug_s2_msgs2_full"


def config(case, flag=True, **kw):
    p = dict(GOLDEN[case]["params"])
    kw.setdefault("state_capacity", 1 << 17)
    kw.setdefault("invariants", p.pop("invariants"))
    p.pop("invariants", None)
    return rmc.make_config(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"],
                           max_log_len=p["max_log_len"], max_msgs=p["max_msgs"], max_dup=p["max_dup"],
                           bug_quorum=bool(p["bug_quorum"]), symmetry=bool(p["symmetry"]), max_depth=p["max_depth"],
                           continue_=flag, **kw)


def model(case):
    p = GOLDEN[case]["params"]
    return continue_cases.model_of(tuple(p[k] for k in ("n_servers", "n_values", "max_term", "max_log_len", "max_msgs",
                                                        "max_dup")), p["bug_quorum"])


def tallies(v):
    return dict(states=v.states, first=list(v.first), each=list(v.each), inv_depth=list(v.depth))


def run(cfg):
    """(Result, per-level new_states, rmc_violations as a dict or None)."""
    with rmc.Checker(cfg) as ck:
        res = ck.run()
        news = [lv[3] for lv in ck.levels if lv[3]]
        return res, news, tallies(ck.violations()) if cfg.flags & rmc.FLAG_CONTINUE else None


def check_against_oracle(case, res, news, viol):
    g = GOLDEN[case]
    print(case, "violations", viol, "oracle", {k: g[k] for k in ("states", "first", "each", "inv_depth")})
    print(case, "result", res.distinct, res.generated, res.depth, res.left_on_queue, "oracle", g["distinct"],
          g["generated"], g["depth"], g["left_on_queue"])
    assert viol == {k: g[k] for k in ("states", "first", "each", "inv_depth")}
    assert sum(viol["first"]) == viol["states"]
    assert (res.distinct, res.generated, res.depth, res.left_on_queue) == (g["distinct"], g["generated"], g["depth"],
                                                                          g["left_on_queue"])
    assert news == g["level_new"][1:]


# ---- CPU ------------------------------------------------------------------------------------
def test_golden_cases_are_the_generators_and_the_smallest_is_recomputed():
    assert list(GOLDEN) == list(continue_cases.CASES)
    for name, (bounds, bug, sym, depth, mask) in continue_cases.CASES.items():
        p = GOLDEN[name]["params"]
        assert (p["n_servers"], p["n_values"], p["max_term"], p["max_log_len"], p["max_msgs"], p["max_dup"]) == bounds
        assert (p["bug_quorum"], p["symmetry"], p["max_depth"], p["invariants"]) == (bug, sym, depth, mask)
        g = GOLDEN[name]
        assert sum(g["first"]) == g["states"] and all(e >= f for e, f in zip(g["each"], g["first"]))
        assert sum(g["level_new"]) == g["distinct"] and len(g["level_new"]) == g["depth"]
    assert continue_cases.run_case(continue_cases.SMALLEST) == GOLDEN[continue_cases.SMALLEST]
    # the notions differ where a state violates two invariants
    assert any(GOLDEN[n]["first"] != GOLDEN[n]["each"] for n in PACKED)
    # the same state spaces as the stopping oracle's goldens of the same bounds
    assert (GOLDEN["tiny2_full"]["distinct"], GOLDEN["tiny2_full"]["generated"]) == (
        LEVELS["tiny2"]["distinct"], LEVELS["tiny2"]["generated"])
    assert GOLDEN["small_d15"]["level_new"] == LEVELS["small"]["level_new"][:15]
    c = GOLDEN["cli_messages_small"]
    assert (c["distinct"], c["generated"], c["depth"]) == (LEVELS["small"]["distinct"], LEVELS["small"]["generated"],
                                                            LEVELS["small"]["depth"])


def test_flag_bits_and_create_refusals(capfd):
    """Bit 11 is RMC_FLAG_CONTINUE: a valid config, so rmc_create goes on to look for
    a device (0 with one, RMC_E_NOGPU without); bit 10 (not assigned: tests/test_coverage.py
    pins it as unknown) and bit 12 are unknown, with or without the flag; the wide
    layout refuses the flag with RMC_FLAG_SPILL, and says why."""
    lib = rmc.native()
    ctx = C.c_void_p()
    assert rmc.FLAG_CONTINUE == 1 << 11
    ok = config("tiny2_full")
    assert ok.flags & rmc.FLAG_CONTINUE
    rc = lib.rmc_create(C.byref(ok), C.byref(ctx))
    assert rc in (0, -19)
    if rc == 0:
        lib.rmc_destroy(ctx)
    for bit in (10, 12):
        for flag in (True, False):
            bad = config("tiny2_full", flag=flag)
            bad.flags |= 1 << bit
            assert lib.rmc_create(C.byref(bad), C.byref(ctx)) == -22
    capfd.readouterr()
    wide = config("tiny2_full", spill=True)
    wide.max_log_len = 4  # beyond the packed capacity
    assert lib.rmc_create(C.byref(wide), C.byref(ctx)) == -22
    err = capfd.readouterr().err
    assert "RMC_FLAG_CONTINUE" in err and "RMC_FLAG_SPILL" in err


def test_cli_refuses_what_coverage_refuses():
    model_args = [os.path.join(SPECS, "MCraftTiny2.tla")]
    for refused in (["-gpus", "2"], ["-checkpoint", "x"], ["-recover", "x"], ["-simulate"]):
        r = subprocess.run([CLI, "-builtin-raft", "-continue"] + refused + model_args, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and "-continue counts whole single-GPU searches" in r.stderr
    assert "-continue" in subprocess.run([CLI], capture_output=True, text=True).stderr


# ---- GPU ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", PACKED)
def test_packed_counts_match_the_oracle(case):
    res, news, viol = run(config(case))
    check_against_oracle(case, res, news, viol)
    # the search itself is that of the model with no violated invariant in its mask
    plain, plain_news, _ = run(config(case, flag=False, invariants=rmc.INV_TYPEOK))
    assert plain.violated_inv == 0
    assert (res.distinct, res.generated, res.depth, res.left_on_queue, news) == (
        plain.distinct, plain.generated, plain.depth, plain.left_on_queue, plain_news)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [ROW1, ROW3])
def test_wide_counts_match_the_oracle(case, monkeypatch):
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    res, news, viol = run(config(case))
    check_against_oracle(case, res, news, viol)
    plain, plain_news, _ = run(config(case, flag=False, invariants=rmc.INV_TYPEOK))
    assert (res.distinct, res.generated, res.depth, res.left_on_queue, news) == (
        plain.distinct, plain.generated, plain.depth, plain.left_on_queue, plain_news)


def spill_config(case, slack=2048, **kw):
    """The sizes of the spill tests of test_gpu.py: a window of the two largest
    adjacent levels + slack states, a set for max(2^20, 1.25 x distinct)."""
    g = GOLDEN[case]
    L = g["level_new"]
    return config(case, state_capacity=max(1 << 20, int(g["distinct"] * 1.25)), spill=True,
                  device_window=max(a + b for a, b in zip(L, L[1:])) + slack, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("links", ["device", "host"])
@pytest.mark.parametrize("case", [ROW1, ROW3])
def test_spill_paths_give_the_same_violations(case, links, monkeypatch):
    """The ring (links in HBM) and the linear window (links on the host).  Row 3's
    ring of 16,384 states wraps three times; a trace from it is replayed."""
    monkeypatch.delenv("RMC_SPILL_HOST_LINKS", raising=False)
    if links == "host":
        monkeypatch.setenv("RMC_SPILL_HOST_LINKS", "1")
    cfg = spill_config(case)
    assert cfg.device_window < GOLDEN[case]["distinct"]
    with rmc.Checker(cfg) as ck:
        res = ck.run()
        news = [lv[3] for lv in ck.levels if lv[3]]
        viol = tallies(ck.violations())
        print(case, links, "spills", res.spills, "spilled", res.spilled)
        assert res.spill_links_on_device == (1 if links == "device" else 0)
        if case == ROW3 or links == "host":
            assert res.spills > 0
        check_against_oracle(case, res, news, viol)
        bit = rmc.INV_LEADER_VOTES  # violated from level 6 on: its least state has left the window
        convert.check_trace(model(case), ck.trace_violation(bit), bit, viol["inv_depth"][4])


@pytest.mark.gpu
def test_verification_and_coverage_give_the_same_violations():
    res, news, viol = run(config(ROW1, verify_states=True))
    assert res.collisions == 0 and res.verified > 0
    check_against_oracle(ROW1, res, news, viol)
    with rmc.Checker(config(ROW1, coverage=True)) as ck:
        res = ck.run()
        news = [lv[3] for lv in ck.levels if lv[3]]
        check_against_oracle(ROW1, res, news, tallies(ck.violations()))
        cov = ck.coverage()
        assert sum(g for g, _ in cov.values()) == res.generated
        assert sum(d for _, d in cov.values()) == res.distinct


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("case", [ROW1, ROW3])
def test_traces_to_every_violated_invariant(case, wide, monkeypatch):
    if wide:
        monkeypatch.setenv("RMC_FORCE_WIDE", "1")
        monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    g = GOLDEN[case]
    m = model(case)
    with rmc.Checker(config(case)) as ck:
        res = ck.run()
        first_run = tallies(ck.violations())
        traced = 0
        for r, bit in enumerate(continue_cases.BITS):
            if not g["each"][r]:
                with pytest.raises(rmc.RmcError, match="no stored state violates") as e:
                    ck.trace_violation(bit)
                assert e.value.code == -71
                continue
            trace = ck.trace_violation(bit)
            print(case, rmc.INV_NAMES[bit], "trace of", len(trace), "states, oracle depth", g["inv_depth"][r])
            # from Init, oracle successors through the named families, the last state the
            # first to fail the predicate, depth[r] states
            convert.check_trace(m, trace, bit, g["inv_depth"][r])
            traced += 1
        assert traced == sum(1 for e in g["each"] if e) >= 3
        # rmc_result and rmc_trace: what the run without the flag reports
        shallowest = min(d for d in g["inv_depth"] if d)
        assert res.violation_depth == shallowest == 6 and res.violated_inv == rmc.INV_LEADER_VOTES
        convert.check_trace(m, ck.trace(), res.violated_inv, res.violation_depth)
        res2 = ck.run()  # tallies from zero
        assert tallies(ck.violations()) == first_run
        assert (res2.distinct, res2.generated, res2.violated_inv, res2.violation_depth) == (
            res.distinct, res.generated, res.violated_inv, res.violation_depth)


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth", [("bug_both", 12), ("messages_small", 15)])
def test_parity_with_the_stopping_run(name, depth):
    """violated_inv / violation_depth of the goldens of the run that stops: the flag
    run searches on (here one level further) and reports the same."""
    g = LEVELS[name]
    assert (g["violated_inv"], g["violation_depth"]) == {"bug_both": (2, 11), "messages_small": (8, 14)}[name]
    p = {k: g["params"][k] for k in ("n_servers", "n_values", "max_term", "max_log_len", "max_msgs", "max_dup")}
    kw = dict(bug_quorum=bool(g["params"]["bug_quorum"]), invariants=g["params"]["invariants"],
              state_capacity=1 << 22, **p)
    with rmc.Checker(rmc.make_config(**kw)) as ck:
        stop = ck.run()
    with rmc.Checker(rmc.make_config(continue_=True, max_depth=depth, **kw)) as ck:
        res = ck.run()
        viol = ck.violations()
        assert len(ck.trace()) == g["violation_depth"]
    assert (stop.violated_inv, stop.violation_depth) == (g["violated_inv"], g["violation_depth"])
    assert (res.violated_inv, res.violation_depth) == (g["violated_inv"], g["violation_depth"])
    assert res.depth == depth > stop.depth and res.distinct > stop.distinct
    r = g["violated_inv"].bit_length() - 1
    assert viol.depth[r] == g["violation_depth"] and viol.each[r] > 0


@pytest.mark.gpu
def test_refusals(tmp_path):
    lib = rmc.native()
    with rmc.Checker(config(ROW1)) as ck:
        v = rmc.Violations()
        assert lib.rmc_get_violations(ck.ctx, C.byref(v)) == -71  # before a run
        assert b"no completed rmc_run_bfs" in lib.rmc_last_error(ck.ctx)
        with pytest.raises(rmc.RmcError, match="no completed rmc_run_bfs") as e:
            ck.trace_violation(rmc.INV_LEADER_VOTES)
        assert e.value.code == -71
        with pytest.raises(rmc.RmcError, match="RMC_FLAG_CONTINUE") as e:
            ck.shard(0, 1, rccl_id=b"\0" * 128)
        assert e.value.code == -22
        ck.run()
        with pytest.raises(rmc.RmcError, match="RMC_FLAG_CONTINUE") as e:
            ck.checkpoint(str(tmp_path / "ck"))
        assert e.value.code == -71
        with pytest.raises(rmc.RmcError, match="RMC_FLAG_CONTINUE") as e:
            ck.recover(str(tmp_path / "ck"))
        assert e.value.code == -71
        for bit in (0, 1 << 10, rmc.INV_LEADER_VOTES | rmc.INV_MESSAGES):  # not one bit of RMC_INV_*
            with pytest.raises(rmc.RmcError, match="one RMC_INV_\\* bit") as e:
                ck.trace_violation(bit)
            assert e.value.code == -22
    with rmc.Checker(config(ROW1, invariants=rmc.INV_TYPEOK | rmc.INV_LEADER_VOTES)) as ck:
        ck.run()
        assert ck.violations().each[4] == GOLDEN[ROW1]["each"][4]
        with pytest.raises(rmc.RmcError, match="one RMC_INV_\\* bit") as e:
            ck.trace_violation(rmc.INV_MESSAGES)  # a bit outside the mask
        assert e.value.code == -22
    with rmc.Checker(config(ROW1, flag=False, invariants=rmc.INV_TYPEOK)) as ck:  # without the flag
        ck.run()
        with pytest.raises(rmc.RmcError, match="without RMC_FLAG_CONTINUE") as e:
            ck.violations()
        assert e.value.code == -71
        with pytest.raises(rmc.RmcError, match="without RMC_FLAG_CONTINUE") as e:
            ck.trace_violation(rmc.INV_TYPEOK)
        assert e.value.code == -71


@pytest.mark.gpu
def test_cli_continue_on_mcraft_messages():
    """rmc-tlc -continue on specs/MCraftMessages.tla (`small` bounds, the full
    2,466,993-state search): the deterministic lines — the violated invariants,
    the length of each trace, our own line of counts, TLC's summary."""
    g = GOLDEN["cli_messages_small"]
    assert g["distinct"] == 2466993 and [r for r, e in enumerate(g["each"]) if e] == [3]
    r = subprocess.run([CLI, "-builtin-raft", "-continue", os.path.join(SPECS, "MCraftMessages.tla")],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-1000:])
    assert r.returncode == 12
    lines = r.stdout.splitlines()
    errors = [k for k, x in enumerate(lines) if x.startswith("Error: Invariant")]
    assert [lines[k] for k in errors] == ["Error: Invariant MessagesInv is violated."]
    assert lines[errors[0] + 1] == "Error: The behavior up to this point is:"
    states = [x for x in lines if re.match(r"State \d+: ", x)]
    assert len(states) == g["inv_depth"][3] == 14 and states[0] == "State 1: <Initial predicate>"
    own = [x for x in lines if x.startswith("Violations (-continue):")]
    assert own == ["Violations (-continue): %d states violate an invariant. MessagesInv: each %d, first %d, depth %d."
                   % (g["states"], g["each"][3], g["first"][3], g["inv_depth"][3])]
    k = lines.index(own[0])
    assert lines[k + 1] == "%d states generated, %d distinct states found, 0 states left on queue." % (
        g["generated"], g["distinct"])
    assert lines[k + 2] == "The depth of the complete state graph search is %d." % g["depth"]
    assert "No error has been found" not in r.stdout
