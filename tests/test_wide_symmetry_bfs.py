"""Whole searches under SYMMETRY Permutations(Server) on the wide layout: one state per
orbit is stored and expanded (the set holds canonical keys, raft_wide.h wcanon), the
records, trace links and lanes are those of the states found.

  * the symmetric goldens of the packed layout, forced wide (RMC_FORCE_WIDE=1), on the
    three records;
  * the reference's own MCraft.cfg layout with SYMMETRY (tests/golden/models/
    MCunboundedSym) under -depth: depths 6, 8, 10 against the C oracle run live, depth
    12 against tests/golden/wide_symmetry_levels.json, resident and through the ring;
  * full-state verification (orbit comparison, wsame_orbit), with full and weakened keys;
  * -coverage and -continue against the packed SYMMETRY run of the same model."""
import json
import os
import subprocess

import pytest

import rmc
from oracle import raft_spec as R
from tests import oracle_c
from tests.convert import check_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_levels.json")))
WIDE_SYM = json.load(open(os.path.join(ROOT, "tests", "golden", "wide_symmetry_levels.json")))["mcraft_shipped_sym_d12"]
MODELS = os.path.join(ROOT, "tests", "golden", "models")
FIXTURE = os.path.join(MODELS, "MCunboundedSym.cfg")
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
RECORDS = {"full": ("0", 5080), "compact": ("1", 904), "depth": ("2", 336)}
UNBOUNDED = rmc.FLAG_UNBOUNDED_TERM | rmc.FLAG_UNBOUNDED_LOG | rmc.FLAG_UNBOUNDED_MSGS | rmc.FLAG_UNBOUNDED_DUP


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    for v in ("RMC_WIDE_COMPACT", "RMC_WIDE_WORK", "RMC_WIDE_VCAP"):
        monkeypatch.delenv(v, raising=False)


def golden_cfg(name, **over):
    g = GOLDEN[name]
    p = g["params"]
    assert p["symmetry"] == 1
    return rmc.make_config(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"],
                           max_log_len=p["max_log_len"], max_msgs=p["max_msgs"], max_dup=p["max_dup"],
                           bug_quorum=bool(p["bug_quorum"]), invariants=p["invariants"], max_depth=p["max_depth"],
                           symmetry=True, state_capacity=max(1 << 20, int(g["distinct"] * 1.25)), **over)


def model_of(p):
    return R.Model(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"], max_log=p["max_log_len"],
                   max_msgs=p["max_msgs"], max_dup=p["max_dup"], bug_quorum=bool(p["bug_quorum"]))


def run_levels(cfg, fp_bits=None):
    with rmc.Checker(cfg) as ck:
        if fp_bits is not None:
            ck.set_fp_bits(fp_bits)
        r = ck.run()
        levels = [1] + [lv[3] for lv in ck.levels if lv[3]]
    return r, levels


def check_golden(g, r, levels):
    assert levels == g["level_new"]
    assert (r.distinct, r.generated, r.depth, r.left_on_queue) == (g["distinct"], g["generated"], g["depth"],
                                                                  g["left_on_queue"])


def fixture_cfg(depth):
    c, _, _ = rmc.model_from_files(FIXTURE, builtin_raft=True, depth_bounded=True)
    c.max_depth = depth
    c.state_capacity = int(sum(WIDE_SYM["level_new"][:depth]) * 1.1) + 4096
    return c


# ---- the front-end (no GPU) -------------------------------------------------------------
def test_fixture_sets_symmetry_and_the_unbounded_bits():
    c, _, _ = rmc.model_from_files(FIXTURE, builtin_raft=True, depth_bounded=True)
    assert c.flags & rmc.FLAG_SYMMETRY
    assert c.flags & UNBOUNDED == UNBOUNDED
    assert (c.n_servers, c.n_values, c.invariants) == (3, 2, rmc.INV_TYPEOK)
    plain, _, _ = rmc.model_from_files(os.path.join(MODELS, "MCunbounded.cfg"), builtin_raft=True, depth_bounded=True)
    assert c.flags == plain.flags | rmc.FLAG_SYMMETRY
    assert (c.max_term, c.max_log_len, c.max_msgs, c.max_dup) == (plain.max_term, plain.max_log_len, plain.max_msgs,
                                                                 plain.max_dup)


def test_golden_is_the_generators():
    """tests/golden/wide_symmetry_levels.json against the figures its generator printed
    (tests/golden/make_wide_symmetry_golden.py), and its depth-10 prefix against the C
    oracle run here."""
    g = WIDE_SYM
    assert g["level_new"] == [1, 1, 5, 20, 89, 386, 1730, 7738, 34929, 157632, 711555, 3207663]
    assert (g["distinct"], g["generated"], g["depth"], g["left_on_queue"]) == (4121749, 19045064, 12, 3207663)
    assert sum(g["level_new"]) == g["distinct"] and sum(g["level_generated"]) == g["generated"]
    assert (sum(g["level_new"][:8]), sum(g["level_generated"][:8])) == (9970, 34940)
    ref, levels, gen = oracle_c.bfs(3, 2, -1, 8, 12, -1, sym=1, max_levels=10, wide=True)
    assert levels == g["level_new"][:10] and gen[:10] == g["level_generated"][:10]


# ---- 3. the symmetric goldens, forced wide ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small_sym", "bounded_sym_prefix16", "s4_sym_prefix16", "s5_sym_prefix16",
                                  "sym_msgs5_dup2_prefix11", "s4_sym_msgs5_prefix10", "s5_sym_log2_dup2_prefix10"])
def test_symmetric_goldens_forced_wide(name):
    cfg = golden_cfg(name)
    assert rmc.native().rmc_state_bytes(cfg) == 336
    check_golden(GOLDEN[name], *run_levels(cfg))


@pytest.mark.gpu
@pytest.mark.parametrize("record", ["full", "compact", "depth"])
@pytest.mark.parametrize("name", ["bounded_sym_prefix16", "sym_msgs5_dup2_prefix11"])
def test_symmetric_goldens_on_every_record(name, record, monkeypatch):
    monkeypatch.setenv("RMC_WIDE_COMPACT", RECORDS[record][0])
    cfg = golden_cfg(name)
    assert rmc.native().rmc_state_bytes(cfg) == RECORDS[record][1]
    check_golden(GOLDEN[name], *run_levels(cfg))


@pytest.mark.gpu
def test_symmetric_violation_and_trace_forced_wide():
    """sym_bug_one_leader: the violated invariant, its depth and the counts of the
    golden; the trace is a behaviour of the spec as it is (no permuted state in it)
    from Init to a violating state."""
    g = GOLDEN["sym_bug_one_leader"]
    with rmc.Checker(golden_cfg("sym_bug_one_leader")) as ck:
        r = ck.run()
        trace = ck.trace()
    assert r.violated_inv == g["violated_inv"] and r.violation_depth == g["violation_depth"]
    assert (r.distinct, r.generated) == (g["distinct"], g["generated"])
    check_trace(model_of(g["params"]), trace, r.violated_inv, r.violation_depth)


# ---- 4. the reference layout with SYMMETRY ----------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [6, 8, 10])
def test_reference_layout_with_symmetry_against_the_live_oracle(depth, monkeypatch):
    monkeypatch.delenv("RMC_FORCE_WIDE")
    ref, levels, gen = oracle_c.bfs(3, 2, -1, 8, 12, -1, sym=1, max_levels=depth, wide=True)
    r, got = run_levels(fixture_cfg(depth))
    assert got == levels
    assert (r.distinct, r.generated, r.depth, r.left_on_queue) == (ref.distinct, ref.generated, depth, levels[-1])
    if depth == 8:
        assert (r.distinct, r.generated) == (9970, 34940)


@pytest.mark.gpu
def test_reference_layout_with_symmetry_depth_12(monkeypatch):
    """4,121,749 orbits where the search without SYMMETRY stores 24,551,858 states."""
    monkeypatch.delenv("RMC_FORCE_WIDE")
    cfg = fixture_cfg(12)
    assert rmc.native().rmc_state_bytes(cfg) == 336
    check_golden(WIDE_SYM, *run_levels(cfg))
    assert WIDE_SYM["distinct"] * 5 < sum(GOLDEN["mcraft_shipped_d12"]["level_new"])


@pytest.mark.gpu
def test_cli_runs_the_fixture(monkeypatch):
    monkeypatch.delenv("RMC_FORCE_WIDE")
    r = subprocess.run([CLI, "-depth", "8", "-builtin-raft", os.path.join(MODELS, "MCunboundedSym.tla")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", SYMMETRY Permutations(Server)" in r.stdout
    g = WIDE_SYM
    summary = (f"{sum(g['level_generated'][:8])} states generated, {sum(g['level_new'][:8])} distinct states found, "
               f"{g['level_new'][7]} states left on queue.")
    assert summary == "34940 states generated, 9970 distinct states found, 7738 states left on queue."
    assert summary in r.stdout.splitlines()
    assert "The depth of the complete state graph search is 8." in r.stdout


# ---- 5. the ring ------------------------------------------------------------------------
def window_of(levels):
    """tests/test_wide_spill.py's choice: the smallest power of two holding 256 + the two
    largest adjacent levels."""
    need = 256 + max(a + b for a, b in zip(levels, levels[1:]))
    w = 1
    while w < need:
        w <<= 1
    return w


@pytest.mark.gpu
def test_reference_layout_with_symmetry_through_the_ring(monkeypatch):
    """Depth 12 of MCunboundedSym through the ring, 336-B records: the counts of the
    resident run.  The window is 256 + levels 10 and 11 (869,443 records, no power of
    two), below the 3,207,663 orbits of level 12, which is never stored.

    This run cannot wrap three times.  A window holds the frontier left and the level
    being built (rmc_plan.h ring_room), so it exceeds the largest stored level, 711,555
    at level 11, and a depth-bounded run writes no record of its last level: 914,086
    records in all, 1.28 times the largest level (the levels grow 4.5-fold), one pass at
    most at any depth.  spills == 1 is asserted here; the symmetric instantiations on a
    ring that wraps six times are test_symmetric_golden_through_a_wrapping_ring."""
    monkeypatch.delenv("RMC_FORCE_WIDE")
    L = WIDE_SYM["level_new"]
    window = 256 + L[9] + L[10]
    stored = sum(L[:11])
    assert max(L[:11]) < window < L[11] and stored // window == 1
    cfg = fixture_cfg(12)
    cfg.flags |= rmc.FLAG_SPILL
    cfg.device_window = window
    assert rmc.native().rmc_state_bytes(cfg) == 336
    r, levels = run_levels(cfg)
    check_golden(WIDE_SYM, r, levels)
    assert r.spills == 1 and r.spilled == stored - window
    assert r.spill_links_on_device == 1


@pytest.mark.gpu
def test_symmetric_golden_through_a_wrapping_ring():
    """small_sym (49 levels, 411,914 orbits, no depth bound) forced wide in a ring of
    65,536 records: six passes, every count the golden's."""
    g = GOLDEN["small_sym"]
    window = window_of(g["level_new"])
    assert window == 65536
    r, levels = run_levels(golden_cfg("small_sym", spill=True, device_window=window))
    check_golden(g, r, levels)
    assert r.spills >= 3 and r.spills == g["distinct"] // window
    assert r.spilled == g["distinct"] - window


# ---- 6. verification under SYMMETRY -----------------------------------------------------
def check_tallies(r, collisions_expected):
    print(f"distinct {r.distinct} probes {r.probes} verified {r.verified} collisions {r.collisions}")
    # rmc.h: every probe is a new state or a compared hit (Init is seeded, not probed)
    assert r.verified == r.probes - (r.distinct - 1)
    assert r.verified_spilled == 0
    assert (r.collisions > 0) if collisions_expected else (r.collisions == 0)


@pytest.mark.gpu
def test_verification_under_symmetry_full_keys(monkeypatch):
    monkeypatch.delenv("RMC_FORCE_WIDE")
    cfg = fixture_cfg(10)
    cfg.flags |= rmc.FLAG_VERIFY_STATES
    r, levels = run_levels(cfg)
    L = WIDE_SYM["level_new"][:10]
    assert levels == L
    assert (r.distinct, r.generated, r.depth, r.left_on_queue) == (sum(L), sum(WIDE_SYM["level_generated"][:10]), 10, L[-1])
    assert r.verified > 0
    check_tallies(r, False)


@pytest.mark.gpu
def test_verification_under_symmetry_weakened_keys(monkeypatch):
    """14 bits of the key: 202,531 orbits at depth 10 against 16,384 keys, so by
    pigeonhole some successor meets another orbit's key — found by wsame_orbit,
    counted and dropped."""
    monkeypatch.delenv("RMC_FORCE_WIDE")
    orbits = sum(WIDE_SYM["level_new"][:10])
    assert orbits > 8 * 2 ** 14
    cfg = fixture_cfg(10)
    cfg.flags |= rmc.FLAG_VERIFY_STATES
    r, _ = run_levels(cfg, fp_bits=14)
    assert r.distinct <= 2 ** 14 and r.distinct < orbits
    check_tallies(r, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bounded_sym_prefix16", "s4_sym_msgs5_prefix10"])
def test_verification_under_symmetry_forced_wide(name):
    """Packed-size symmetric goldens (S = 3 and 4) on the wide store under verification."""
    r, levels = run_levels(golden_cfg(name, verify_states=True))
    check_golden(GOLDEN[name], r, levels)
    assert r.verified > 0
    check_tallies(r, False)


# ---- 7. coverage and continue -----------------------------------------------------------
@pytest.mark.gpu
def test_coverage_with_symmetry_forced_wide(monkeypatch):
    name = "bounded_sym_prefix16"
    with rmc.Checker(golden_cfg(name, coverage=True)) as ck:
        r = ck.run()
        wide = ck.coverage()
    check_golden(GOLDEN[name], r, GOLDEN[name]["level_new"])
    assert sum(g for g, _d in wide.values()) == r.generated
    assert sum(d for _g, d in wide.values()) == r.distinct
    monkeypatch.delenv("RMC_FORCE_WIDE")
    cfg = golden_cfg(name, coverage=True)
    assert rmc.native().rmc_state_bytes(cfg) < 336  # the packed layout
    with rmc.Checker(cfg) as ck:
        ck.run()
        packed = ck.coverage()
    assert {a: g for a, (g, _d) in wide.items()} == {a: g for a, (g, _d) in packed.items()}


@pytest.mark.gpu
def test_continue_with_symmetry_forced_wide(monkeypatch):
    """sym_bug_one_leader searched past its violation (depth 11) to depth 12 — its whole
    state space is beyond 2^26 orbits — on both layouts."""
    name = "sym_bug_one_leader"
    g = GOLDEN[name]
    bit = g["violated_inv"]
    monkeypatch.setitem(g["params"], "max_depth", g["violation_depth"] + 1)
    with rmc.Checker(golden_cfg(name, continue_=True)) as ck:
        ck.run()
        wide = ck.violations()
        r = bit.bit_length() - 1
        trace = ck.trace_violation(bit)
        assert len(trace) == wide.depth[r] == g["violation_depth"]
        check_trace(model_of(g["params"]), trace, bit, wide.depth[r])
    monkeypatch.delenv("RMC_FORCE_WIDE")
    with rmc.Checker(golden_cfg(name, continue_=True)) as ck:
        ck.run()
        packed = ck.violations()
    assert wide.states == packed.states and wide.states > 0
    assert list(wide.first) == list(packed.first) and list(wide.each) == list(packed.each)
    assert list(wide.depth) == list(packed.depth)
    assert wide.each[r] > 0
