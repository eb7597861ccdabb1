"""The wide layout's frontier spill (RMC_FLAG_SPILL on a wide ctx): the records
live in a ring window of exactly device_window slots (state i at slot
i % window, trace links of every state in HBM), a depth-bounded run does not
store its last level, the store's record may be narrower than the record the
expansion works on, and a counterexample is replayed on the host from Init.

Parity is against the same golden counts as the resident wide layout
(tests/test_wide.py).  W(name), the window of most tests, is the smallest
power of two holding 256 + the two largest adjacent levels: always enough —
the live set is at most the frontier and the level being built, and one
state yields at most 232 new ones — and small enough that the ring wraps."""
import json
import os

import pytest

import rmc
from oracle import raft_spec as R
from tests.convert import check_trace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_levels.json")))
MCRAFT = os.path.join(ROOT, "tests", "golden", "models", "MCunbounded.cfg")
RECORDS = {"full": ("0", 5080), "compact": ("1", 904), "depth": ("2", 336)}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    monkeypatch.delenv("RMC_WIDE_WORK", raising=False)


def window_of(name):
    L = GOLDEN[name]["level_new"]
    need = 256 + max(a + b for a, b in zip(L, L[1:]))
    w = 1
    while w < need:
        w <<= 1
    return w


def spilled_cfg(name, window, **over):
    g = GOLDEN[name]
    p = dict(g["params"], **over)
    return rmc.make_config(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"],
                           max_log_len=p["max_log_len"], max_msgs=p["max_msgs"], max_dup=p["max_dup"],
                           bug_quorum=bool(p["bug_quorum"]), invariants=p["invariants"], max_depth=p["max_depth"],
                           state_capacity=int(g["distinct"] * 1.25) + (1 << 16), spill=True, device_window=window)


def model_of(p):
    return R.Model(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"], max_log=p["max_log_len"],
                   max_msgs=p["max_msgs"], max_dup=p["max_dup"], bug_quorum=bool(p["bug_quorum"]))


def run_levels(cfg):
    with rmc.Checker(cfg) as ck:
        r = ck.run()
        levels = [1] + [lv[3] for lv in ck.levels if lv[3]]
    return r, levels


def check_parity(name, window):
    g = GOLDEN[name]
    r, levels = run_levels(spilled_cfg(name, window))
    assert levels == g["level_new"]
    assert (r.distinct, r.generated, r.depth, r.left_on_queue) == (g["distinct"], g["generated"], g["depth"],
                                                                  g["left_on_queue"])
    assert r.spills >= 1 and r.spills == g["distinct"] // window
    assert r.spilled == g["distinct"] - window
    assert r.spill_links_on_device == 1


def test_window_sizes_are_the_ones_the_ring_wraps_at():
    assert [window_of(n) for n in ("tiny2", "s3_v1_msgs1", "small", "votes_granted_small", "messages_small",
                                   "bug_votes_granted")] == [4096, 262144, 524288, 262144, 32768, 262144]


@pytest.mark.parametrize("record", ["full", "compact", "depth"])
def test_ring_parity_tiny2_on_every_record(record, monkeypatch):
    """3.2 passes of a 4,096-record ring, on each of the three records."""
    monkeypatch.setenv("RMC_WIDE_COMPACT", RECORDS[record][0])
    assert rmc.native().rmc_state_bytes(spilled_cfg("tiny2", 4096)) == RECORDS[record][1]
    check_parity("tiny2", window_of("tiny2"))


@pytest.mark.parametrize("name", ["s3_v1_msgs1", "small"])
def test_ring_parity_with_a_wrapping_ring(name):
    """5.9 and 4.7 passes of the ring: every per-level count, distinct,
    generated, depth and the queue equal the oracle's."""
    check_parity(name, window_of(name))


def test_ring_window_is_not_rounded_to_a_power_of_two():
    """`small` in 300,311 records, an odd number above 256 + its two largest
    adjacent levels (290,055) and far from the 524,288 a power of two would
    take: the same counts, and the spill tallies of exactly that window."""
    L = GOLDEN["small"]["level_new"]
    assert 256 + max(a + b for a, b in zip(L, L[1:])) == 290311 <= 300311
    check_parity("small", 300311)


@pytest.mark.parametrize("name", ["votes_granted_small", "messages_small", "bug_votes_granted"])
def test_ring_trace_is_replayed_from_init(name):
    """A counterexample of a spilled wide run does not read the store: its
    states — votes_granted_small's 336,159 states overwrite Init's slot in a
    262,144-record ring — are re-derived from Init by their lanes."""
    g = GOLDEN[name]
    with rmc.Checker(spilled_cfg(name, window_of(name))) as ck:
        r = ck.run()
        trace = ck.trace()
    assert r.violated_inv == g["violated_inv"] and r.violation_depth == g["violation_depth"]
    assert (r.distinct, r.generated) == (g["distinct"], g["generated"])
    assert r.spilled > 0
    check_trace(model_of(g["params"]), trace, r.violated_inv, r.violation_depth)


def test_violation_in_the_unstored_last_level():
    """messages_small bounded at its violation depth, 14: level 14 is never
    expanded, so no record of it is written — its states are still inserted,
    linked and checked on the expansion's private copy, and the trace ends in
    one of them."""
    g = GOLDEN["messages_small"]
    assert g["violation_depth"] == 14
    with rmc.Checker(spilled_cfg("messages_small", window_of("messages_small"), max_depth=14)) as ck:
        r = ck.run()
        trace = ck.trace()
    assert r.violated_inv == g["violated_inv"] and r.violation_depth == 14
    assert (r.distinct, r.generated) == (g["distinct"], g["generated"])
    assert len(trace) == 14
    check_trace(model_of(g["params"]), trace, r.violated_inv, r.violation_depth)


@pytest.mark.parametrize("depth,window", [(8, 0), (10, 1 << 18)])
def test_store_record_narrower_than_the_work_record(depth, window, monkeypatch):
    """MCraft.cfg as shipped, stored in 336-B records and expanded in 904-B
    ones: the mcraft_shipped_d12 prefix.  At depth 10 the window (2^18) is
    below the 930,857 states of the last level and above levels 8 + 9 (248,571)
    + 256: the run fits only because the last level is not stored."""
    monkeypatch.delenv("RMC_FORCE_WIDE")
    monkeypatch.setenv("RMC_WIDE_COMPACT", "2")
    monkeypatch.setenv("RMC_WIDE_WORK", "1")
    g = GOLDEN["mcraft_shipped_d12"]
    L = g["level_new"]
    assert window == 0 or L[7] + L[8] + 256 < window < L[9]
    c, _, _ = rmc.model_from_files(MCRAFT, builtin_raft=True, depth_bounded=True)
    c.max_depth = depth
    c.state_capacity = int(sum(L[:depth]) * 1.1) + 4096
    c.flags |= rmc.FLAG_SPILL
    c.device_window = window
    assert rmc.native().rmc_state_bytes(c) == 336
    r, levels = run_levels(c)
    assert levels == L[:depth]
    assert r.distinct == sum(L[:depth]) and r.depth == depth
    assert r.left_on_queue == L[depth - 1]
    assert r.generated == sum(g["level_generated"][:depth])
    assert r.spill_links_on_device == 1
    # the records written are every level but the last: 260,833 at depth 10, within the window
    assert sum(L[:depth - 1]) < (window or c.state_capacity) and (r.spilled, r.spills) == (0, 0)


def test_window_too_small_is_a_capacity_error():
    """1,024 records cannot hold `small`'s frontier and the level being built:
    RMC_E_CAPACITY naming the window — no hang, no wrong counts."""
    with rmc.Checker(spilled_cfg("small", 1024)) as ck:
        with pytest.raises(rmc.RmcError, match="cannot hold the frontier and the level being built") as e:
            ck.run()
    assert e.value.code == -28
