"""Full-state verification on the wide layout (RMC_FLAG_VERIFY_STATES on a
resident wide ctx): every fingerprint hit is compared with the stored state
that owns the set slot — in the expansion kernel when the owner was stored by
an earlier launch, by k_wverify after the launch otherwise — and a successor
that differs from its key's owner is a collision, counted and dropped.

Every probe is then either a new state or a compared hit:
verified == probes - (distinct - 1) (Init is seeded, not probed).  Counts are
the golden ones of the resident wide layout (tests/test_wide.py)."""
import json
import os
import subprocess

import pytest

import rmc
from oracle import raft_spec as R
from tests.convert import check_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_levels.json")))
MODELS = os.path.join(ROOT, "tests", "golden", "models")
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
RECORDS = {"full": ("0", 5080), "compact": ("1", 904), "depth": ("2", 336)}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    monkeypatch.delenv("RMC_WIDE_WORK", raising=False)
    monkeypatch.delenv("RMC_WIDE_VCAP", raising=False)


def verify_cfg(name, verify=True, **over):
    g = GOLDEN[name]
    p = g["params"]
    return rmc.make_config(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"],
                           max_log_len=p["max_log_len"], max_msgs=p["max_msgs"], max_dup=p["max_dup"],
                           bug_quorum=bool(p["bug_quorum"]), invariants=p["invariants"], max_depth=p["max_depth"],
                           state_capacity=max(1 << 20, int(g["distinct"] * 1.25)), verify_states=verify, **over)


def run_levels(cfg, fp_bits=None):
    with rmc.Checker(cfg) as ck:
        if fp_bits is not None:
            ck.set_fp_bits(fp_bits)
        r = ck.run()
        levels = [1] + [lv[3] for lv in ck.levels if lv[3]]
    return r, levels


def check_tallies(r, collisions_expected):
    print(f"distinct {r.distinct} probes {r.probes} verified {r.verified} collisions {r.collisions} "
          f"launches {r.expand_launches}")
    assert r.verified == r.probes - (r.distinct - 1)
    assert r.verified_spilled == 0
    assert (r.collisions > 0) if collisions_expected else (r.collisions == 0)


def check_exact(name, r, levels):
    g = GOLDEN[name]
    assert levels == g["level_new"]
    assert (r.distinct, r.generated, r.depth, r.left_on_queue) == (g["distinct"], g["generated"], g["depth"],
                                                                  g["left_on_queue"])
    check_tallies(r, False)


@pytest.mark.parametrize("record", ["full", "compact", "depth"])
def test_exact_counts_and_no_collision_on_every_record(record, monkeypatch):
    """tiny2 on the 5,080-B, 904-B and 336-B records: the oracle's counts, every
    hit compared, none differing."""
    monkeypatch.setenv("RMC_WIDE_COMPACT", RECORDS[record][0])
    cfg = verify_cfg("tiny2")
    assert rmc.native().rmc_state_bytes(cfg) == RECORDS[record][1]
    check_exact("tiny2", *run_levels(cfg))


@pytest.mark.parametrize("name", ["small", "s4_prefix10", "msgs5_dup2_prefix9"])
def test_exact_counts_and_no_collision(name):
    check_exact(name, *run_levels(verify_cfg(name)))


def test_reference_config_is_certified_to_depth_10(monkeypatch):
    """MCraft.cfg as shipped (no CONSTRAINT) under verification, ten levels on
    the 336-B record: the mcraft_shipped_d12 prefix, 1,191,690 states, no
    collision."""
    monkeypatch.delenv("RMC_FORCE_WIDE")
    g = GOLDEN["mcraft_shipped_d12"]
    c, _, _ = rmc.model_from_files(os.path.join(MODELS, "MCunbounded.cfg"), builtin_raft=True, depth_bounded=True)
    c.max_depth = 10
    c.flags |= rmc.FLAG_VERIFY_STATES
    c.state_capacity = int(1191690 * 1.1) + 4096
    assert rmc.native().rmc_state_bytes(c) == 336
    r, levels = run_levels(c)
    assert levels == g["level_new"][:10]
    assert r.distinct == 1191690 == sum(g["level_new"][:10])
    assert r.generated == sum(g["level_generated"][:10])
    check_tallies(r, False)


@pytest.mark.parametrize("name,bits", [("small", 16), ("small", 20), ("tiny2", 12)])
def test_weakened_fingerprints_report_collisions(name, bits):
    """rmc_set_fp_bits keeps `bits` bits of the key: more states than keys
    (small: 2,466,993 against 2^20; tiny2: 12,975 against 2^12), so by pigeonhole
    some successor meets another state's key — found, counted and dropped."""
    g = GOLDEN[name]
    assert g["distinct"] > 2 ** bits
    r, _ = run_levels(verify_cfg(name), fp_bits=bits)
    assert r.distinct <= 2 ** bits
    assert r.distinct < g["distinct"]
    check_tallies(r, True)


def test_many_launches_per_level(monkeypatch):
    """A deferred-hit buffer of 8,192 records: launches of about a hundred
    states, so most owners are of an earlier launch of the same level (compared
    in the expansion kernel) and the rest of the same launch (k_wverify)."""
    r0, _ = run_levels(verify_cfg("small"))
    monkeypatch.setenv("RMC_WIDE_VCAP", "8192")
    r, levels = run_levels(verify_cfg("small"))
    check_exact("small", r, levels)
    assert r.verified == r0.verified
    assert r.expand_launches > r0.expand_launches


@pytest.mark.parametrize("name", ["bug_one_leader", "messages_small"])
def test_violation_and_trace_under_verification(name):
    g = GOLDEN[name]
    p = g["params"]
    with rmc.Checker(verify_cfg(name)) as ck:
        r = ck.run()
        trace = ck.trace()
    assert r.violated_inv == g["violated_inv"] and r.violation_depth == g["violation_depth"]
    assert (r.distinct, r.generated) == (g["distinct"], g["generated"])
    assert r.collisions == 0
    model = R.Model(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"], max_log=p["max_log_len"],
                    max_msgs=p["max_msgs"], max_dup=p["max_dup"], bug_quorum=bool(p["bug_quorum"]))
    check_trace(model, trace, r.violated_inv, r.violation_depth)


def test_verification_with_spill_is_refused(capfd):
    """The wide ring keeps no record of a spilled owner to compare with:
    RMC_E_INVAL, the message (rmc_create prints it) naming both flags."""
    with pytest.raises(rmc.RmcError) as e:
        rmc.Checker(verify_cfg("tiny2", spill=True))
    assert e.value.code == -22
    err = capfd.readouterr().err
    assert "VERIFY_STATES" in err and "SPILL" in err


def test_set_fp_bits_needs_the_flag():
    with rmc.Checker(verify_cfg("tiny2", verify=False)) as ck:
        with pytest.raises(rmc.RmcError) as e:
            ck.set_fp_bits(16)
    assert e.value.code == -22


def test_cli_verify_on_the_reference_config(monkeypatch):
    """rmc-tlc -verify on a wide model: the summary line of the run without
    -verify (the oracle's depth-8 counts, which tests/test_wide.py holds that
    run to) and the collision line."""
    monkeypatch.delenv("RMC_FORCE_WIDE")
    g = GOLDEN["mcraft_shipped_d12"]
    r = subprocess.run([CLI, "-verify", "-depth", "8", "-builtin-raft", os.path.join(MODELS, "MCunbounded.tla")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    summary = (f"{sum(g['level_generated'][:8])} states generated, {sum(g['level_new'][:8])} distinct states found, "
               f"{g['level_new'][7]} states left on queue.")
    assert summary in r.stdout.splitlines()
    assert "The depth of the complete state graph search is 8." in r.stdout
    assert "Full-state verification: " in r.stdout and ", 0 collisions." in r.stdout
