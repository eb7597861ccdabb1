"""Action coverage (RMC_FLAG_COVERAGE, TLC -coverage): per-action generated /
distinct counts of the BFS (rmc_get_coverage, rmc-tlc -coverage).

The expected rows come from the Python oracle (oracle/raft_spec.py), computed
here by cover_bfs: a level-synchronous BFS that puts every successor into its
action's row — a Receive successor by the rule of the trace headers, UpdateTerm
when the message's term is newer than its receiver's, else the disjunct of its
mtype.  `generated[a]` must equal the oracle's exactly.  A state reached by
two actions in one level is credited to whichever lane won the set insert, so
`distinct[a]` lies between lo[a], the new states all of whose in-edges from
the previous level are of action a, and hi[a], those with at least one; both
sums equal rmc_result's.  tests/golden/coverage_tiny2.json is a second anchor
for MCraftTiny2 beside the live computation."""
import collections
import ctypes as C
import functools
import json
import os
import re
import subprocess

import pytest

import rmc
from oracle import raft_spec as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_levels.json")))
COVERAGE_TINY2 = json.load(open(os.path.join(ROOT, "tests", "golden", "coverage_tiny2.json")))
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
SPECS = os.path.join(ROOT, "specs")
ROWS = ("Init", "Restart", "Timeout", "RequestVote", "BecomeLeader", "ClientRequest", "AdvanceCommitIndex",
        "AppendEntries", "UpdateTerm", "Receive:RequestVoteRequest", "Receive:RequestVoteResponse",
        "Receive:AppendEntriesRequest", "Receive:AppendEntriesResponse", "DuplicateMessage", "DropMessage")

TINY2 = dict(n_servers=2, n_values=1, max_term=2, max_log_len=1, max_msgs=2, max_dup=1)
SMALL = dict(n_servers=3, n_values=2, max_term=2, max_log_len=1, max_msgs=1, max_dup=1)
SYM9 = dict(n_servers=3, n_values=2, max_term=2, max_log_len=1, max_msgs=2, max_dup=1)


# ---- the oracle's rows ------------------------------------------------------------------
def action_of(s, family, params):
    if family != "Receive":
        return family
    m = params[0]
    if R.rget(m, "mterm") > s.currentTerm[R.rget(m, "mdest")]:
        return "UpdateTerm"
    return "Receive:" + R.rget(m, "mtype")


Cover = collections.namedtuple("Cover", "gen lo hi distinct generated expanded_levels")


@functools.lru_cache(maxsize=None)
def cover_bfs(params, symmetry=False, max_levels=None):
    """params: sorted (name, value) pairs of n_servers .. max_dup (and bug_quorum).
    Levels are expanded while depth < max_levels (rmc_config.max_depth)."""
    p = dict(params)
    model = R.Model(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"], max_log=p["max_log_len"],
                    max_msgs=p["max_msgs"], max_dup=p["max_dup"], bug_quorum=bool(p.get("bug_quorum")))
    key = (lambda t: R.canonical(model, t)) if symmetry else (lambda t: t)
    s0 = R.init_state(model)
    seen = {key(s0)}
    frontier = [s0]
    gen, lo, hi = collections.Counter(Init=1), collections.Counter(Init=1), collections.Counter(Init=1)
    depth, expanded = 1, 0
    while frontier and (max_levels is None or depth < max_levels):
        edges = {}  # key of a new state -> (state, actions of its in-edges from this level)
        for s in frontier:
            for family, prm, t in R.successors(model, s):
                a = action_of(s, family, prm)
                gen[a] += 1
                if not R.in_constraint(model, t):
                    continue
                k = key(t)
                if k in seen:
                    continue
                edges.setdefault(k, (t, set()))[1].add(a)
        expanded += 1
        for t, acts in edges.values():
            for a in acts:
                hi[a] += 1
            if len(acts) == 1:
                lo[next(iter(acts))] += 1
        seen.update(edges)
        frontier = [t for t, _ in edges.values()]
        depth += 1 if frontier else 0
    return Cover(gen, lo, hi, len(seen), sum(gen.values()), expanded)


def oracle(p, symmetry=False, max_levels=None):
    return cover_bfs(tuple(sorted(p.items())), symmetry, max_levels)


def check_rows(cov, res, ref, distinct_bounds=True):
    """cov: Checker.coverage(); res: the run's Result; ref: cover_bfs's rows."""
    assert tuple(cov) == ROWS
    for a in ROWS:
        print(a, "generated", cov[a][0], "oracle", ref.gen[a], "distinct", cov[a][1], "bounds", ref.lo[a], ref.hi[a])
    for a in ROWS:
        assert cov[a][0] == ref.gen[a], a
        if distinct_bounds:
            assert ref.lo[a] <= cov[a][1] <= ref.hi[a], a
    assert sum(g for g, _ in cov.values()) == res.generated == ref.generated
    assert sum(d for _, d in cov.values()) == res.distinct == ref.distinct


def run_cover(cfg):
    with rmc.Checker(cfg) as ck:
        res = ck.run()
        return res, ck.coverage()


def config(p, **kw):
    kw.setdefault("state_capacity", 1 << 16)
    return rmc.make_config(coverage=True, **p, **kw)


# ---- CPU ------------------------------------------------------------------------------------
def test_oracle_rows_of_tiny2_are_the_recorded_ones():
    """The live computation against tests/golden/coverage_tiny2.json and against
    the oracle's totals: every action fires, MaxDup = 1 makes DuplicateMessage vacuous."""
    ref = oracle(TINY2)
    g = GOLDEN["tiny2"]
    assert (ref.distinct, ref.generated) == (g["distinct"], g["generated"]) == (12975, 130639)
    assert {a: ref.gen[a] for a in ROWS} == COVERAGE_TINY2["generated"]
    assert all(ref.gen[a] > 0 for a in ROWS)
    assert (ref.lo["DuplicateMessage"], ref.hi["DuplicateMessage"], ref.gen["DuplicateMessage"]) == (0, 0, 20666)
    assert (ref.gen["BecomeLeader"], ref.gen["UpdateTerm"]) == (276, 28)
    assert (sum(ref.lo.values()), sum(ref.hi.values())) == (COVERAGE_TINY2["sum_lo"], COVERAGE_TINY2["sum_hi"])
    assert sum(ref.lo.values()) <= ref.distinct <= sum(ref.hi.values())


def test_row_names_and_locations():
    lib = rmc.native()
    names = [lib.rmc_coverage_action(k) for k in range(15)]
    assert tuple(n.decode() for n in names) == ROWS == rmc.COVERAGE_ACTIONS
    assert lib.rmc_coverage_action(-1) is None and lib.rmc_coverage_action(15) is None
    for a in ROWS[1:]:
        loc = rmc.action_location(a)
        assert loc[0] <= loc[2] and loc[1] > 0, (a, loc)
    assert rmc.action_location("Init")[0::2] == (125, 129)  # raft.tla:125-129


def test_flag_bits():
    """Bit 9 is RMC_FLAG_COVERAGE: a valid config, so rmc_create goes on to look
    for a device (0 with one, RMC_E_NOGPU without); bit 10 and above are still
    unknown."""
    lib = rmc.native()
    ctx = C.c_void_p()
    assert rmc.FLAG_COVERAGE == 1 << 9
    bad = rmc.make_config(**TINY2)
    bad.flags |= 1 << 10
    assert lib.rmc_create(C.byref(bad), C.byref(ctx)) == -22
    both = rmc.make_config(coverage=True, **TINY2)
    both.flags |= 1 << 10
    assert lib.rmc_create(C.byref(both), C.byref(ctx)) == -22
    ok = config(TINY2)
    assert ok.flags & rmc.FLAG_COVERAGE
    rc = lib.rmc_create(C.byref(ok), C.byref(ctx))
    assert rc in (0, -19)
    if rc == 0:
        lib.rmc_destroy(ctx)


# ---- GPU ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny2", "small_prefix9", "sym_prefix9"])
def test_packed_rows_match_the_oracle(name):
    """Resident packed runs: MCraftTiny2 to fixpoint; the `small` bounds and a
    SYMMETRY model (S = 3, |Value| = 2, MaxMsgs 2) to depth 9."""
    p, sym, depth = {"tiny2": (TINY2, False, 0), "small_prefix9": (SMALL, False, 9), "sym_prefix9": (SYM9, True, 9)}[name]
    ref = oracle(p, sym, depth or None)
    assert ref.distinct == {"tiny2": 12975, "small_prefix9": 2433, "sym_prefix9": 1277}[name]
    res, cov = run_cover(config(p, symmetry=sym, max_depth=depth))
    check_rows(cov, res, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("host_links", [False, True])
def test_packed_spill_rows_match_the_oracle(host_links, monkeypatch):
    """MCraftTiny2 in a window of its two largest adjacent levels + 4,096
    states: the ring (links in HBM) and the linear window (links on the host)."""
    monkeypatch.delenv("RMC_SPILL_HOST_LINKS", raising=False)
    if host_links:
        monkeypatch.setenv("RMC_SPILL_HOST_LINKS", "1")
    L = GOLDEN["tiny2"]["level_new"]
    cfg = config(TINY2, state_capacity=1 << 20, spill=True, device_window=max(a + b for a, b in zip(L, L[1:])) + 4096)
    res, cov = run_cover(cfg)
    assert res.spill_links_on_device == (0 if host_links else 1)
    check_rows(cov, res, oracle(TINY2))


@pytest.mark.gpu
@pytest.mark.parametrize("record", ["0", "1", "2"])
@pytest.mark.parametrize("ring", [False, True])
def test_wide_rows_match_the_oracle(record, ring, monkeypatch):
    """MCraftTiny2 on the wide layout, resident and in a 4,096-record ring (3.2
    passes), on each of the three records."""
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    monkeypatch.setenv("RMC_WIDE_COMPACT", record)
    monkeypatch.delenv("RMC_WIDE_WORK", raising=False)
    cfg = config(TINY2, spill=ring, device_window=4096 if ring else 0)
    assert rmc.native().rmc_state_bytes(cfg) == {"0": 5080, "1": 904, "2": 336}[record]
    res, cov = run_cover(cfg)
    assert (res.spills > 0) == ring
    check_rows(cov, res, oracle(TINY2))


@pytest.mark.gpu
def test_wide_ring_unstored_last_level(monkeypatch):
    """max_depth = 20 in the ring: level 20 is never expanded and gets no record
    (its states have their links), so its distinct rows are read from the links
    and the parents' records alone.  The ring has wrapped by then."""
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    monkeypatch.delenv("RMC_WIDE_WORK", raising=False)
    ref = oracle(TINY2, False, 20)
    res, cov = run_cover(config(TINY2, spill=True, device_window=4096, max_depth=20))
    assert res.depth == 20 and res.left_on_queue > 0 and res.spills >= 1
    check_rows(cov, res, ref)


@pytest.mark.gpu
def test_many_launches_per_level_packed_and_wide(monkeypatch):
    """`small` (2.47 M states) in windows that cut its levels into several
    launches: the per-launch ranges must tile each level.  Both sums hold, and
    the packed and the wide run — two independent lane implementations — give
    the same generated[] row by row."""
    g = GOLDEN["small"]
    L = g["level_new"]
    monkeypatch.delenv("RMC_SPILL_HOST_LINKS", raising=False)
    cap = int(g["distinct"] * 1.25)
    window = max(a + b for a, b in zip(L, L[1:])) + 65536
    res_p, cov_p = run_cover(config(SMALL, state_capacity=cap, spill=True, device_window=window))
    monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    monkeypatch.delenv("RMC_WIDE_WORK", raising=False)
    res_w, cov_w = run_cover(config(SMALL, state_capacity=cap + (1 << 16), spill=True, device_window=1 << 19))
    for res, cov in ((res_p, cov_p), (res_w, cov_w)):
        print("launches", res.expand_launches, "levels", res.depth)
        assert res.expand_launches > res.depth - 1  # more launches than expanded levels
        assert (res.distinct, res.generated) == (g["distinct"], g["generated"])
        assert sum(x for x, _ in cov.values()) == res.generated
        assert sum(d for _, d in cov.values()) == res.distinct
    assert res_w.spills >= 1
    assert [cov_p[a][0] for a in ROWS] == [cov_w[a][0] for a in ROWS]
    assert all(cov_p[a][0] > 0 for a in ROWS)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
def test_rows_under_full_state_verification(wide, monkeypatch):
    """RMC_FLAG_VERIFY_STATES + coverage on MCraftTiny2: the rows of the plain
    run (the oracle's), no collisions."""
    if wide:
        monkeypatch.setenv("RMC_FORCE_WIDE", "1")
        monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    plain, cov_plain = run_cover(config(TINY2))
    res, cov = run_cover(config(TINY2, verify_states=True))
    assert res.collisions == 0 and res.verified > 0
    assert [cov[a][0] for a in ROWS] == [cov_plain[a][0] for a in ROWS]
    check_rows(cov, res, oracle(TINY2))


@pytest.mark.gpu
def test_bug_quorum_counts_in_row_become_leader():
    """RMC_FLAG_BUG_QUORUM weakens BecomeLeader's guard (golden case
    bug_leader_votes: LeaderVotesQuorum is violated at level 6 of 293 states).
    The run stops at the violation, after the level that found it was expanded
    whole, and its rows are the oracle's of the weakened spec to that depth."""
    g = GOLDEN["bug_leader_votes"]
    assert (g["distinct"], g["generated"], g["violation_depth"]) == (293, 1777, 6)
    ref = oracle(dict(SMALL, bug_quorum=1), False, 6)
    res, cov = run_cover(rmc.make_config(coverage=True, bug_quorum=True, invariants=rmc.INV_LEADER_VOTES,
                                         state_capacity=1 << 16, **SMALL))
    assert res.violated_inv == rmc.INV_LEADER_VOTES and res.violation_depth == 6
    check_rows(cov, res, ref)
    assert cov["BecomeLeader"][0] > oracle(SMALL, False, 6).gen["BecomeLeader"]  # the quorum guard fires less often


@pytest.mark.gpu
def test_rerun_resets_and_refusals(tmp_path):
    lib = rmc.native()
    ref = oracle(TINY2)
    with rmc.Checker(config(TINY2)) as ck:
        cv = rmc.Coverage()
        assert lib.rmc_get_coverage(ck.ctx, C.byref(cv)) == -71  # before a run
        res1 = ck.run()
        cov1 = ck.coverage()
        res2 = ck.run()  # the next set epoch, tallies from zero
        cov2 = ck.coverage()
        check_rows(cov1, res1, ref)
        check_rows(cov2, res2, ref)
        with pytest.raises(rmc.RmcError, match="RMC_FLAG_COVERAGE") as e:
            ck.shard(0, 1, rccl_id=b"\0" * 128)
        assert e.value.code == -22
    with rmc.Checker(config(TINY2, max_depth=5)) as ck:
        ck.run()
        with pytest.raises(rmc.RmcError, match="RMC_FLAG_COVERAGE") as e:
            ck.checkpoint(str(tmp_path / "ck"))
        assert e.value.code == -71
        with pytest.raises(rmc.RmcError, match="RMC_FLAG_COVERAGE") as e:
            ck.recover(str(tmp_path / "ck"))
        assert e.value.code == -71
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **TINY2)) as ck:  # without the flag
        ck.run()
        with pytest.raises(rmc.RmcError, match="without RMC_FLAG_COVERAGE") as e:
            ck.coverage()
        assert e.value.code == -71


@pytest.mark.gpu
def test_cli_coverage_block():
    """rmc-tlc -coverage (with TLC's optional interval): 15 lines between the
    markers, `<Action line .. of module raft>: distinct:generated`, before the
    unchanged summary; without the option no block."""
    ref = oracle(TINY2)
    model = ["-capacity", "65536", os.path.join(SPECS, "MCraftTiny2.tla")]  # (a small store: the run starts at once)
    plain = subprocess.run([CLI, "-builtin-raft"] + model, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "coverage" not in plain.stdout and "End of statistics" not in plain.stdout
    for opt in (["-coverage"], ["-coverage", "1"]):
        r = subprocess.run([CLI, "-builtin-raft"] + opt + model, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = r.stdout.splitlines()
        a, b = lines.index("The coverage statistics :"), lines.index("End of statistics.")
        block = lines[a + 1:b]
        assert len(block) == 15
        assert lines[b + 1] == "130639 states generated, 12975 distinct states found, 0 states left on queue."
        assert lines[b + 2] == "The depth of the complete state graph search is 31."
        shown = [x if not x.startswith("Receive:") else "Receive" for x in ROWS]
        total_d = 0
        for row, name, line in zip(ROWS, shown, block):
            m = re.fullmatch(r"<(\w+) line (\d+), col (\d+) to line (\d+), col (\d+) of module raft>: (\d+):(\d+)", line)
            assert m, line
            assert m.group(1) == name
            assert tuple(int(x) for x in m.group(2, 3, 4, 5)) == rmc.action_location(row)
            d, gen = int(m.group(6)), int(m.group(7))
            assert gen == ref.gen[row] and ref.lo[row] <= d <= ref.hi[row], line
            total_d += d
        assert total_d == 12975
        assert block[13].endswith("of module raft>: 0:20666")  # DuplicateMessage: vacuous under MaxDup = 1
        strip = lambda out: [x for x in out.splitlines() if not x.startswith(("Finished in", "Progress("))]
        assert strip(plain.stdout) == [x for x in strip(r.stdout) if x not in lines[a:b + 1]]
    for refused in (["-gpus", "2"], ["-checkpoint", "x"], ["-recover", "x"], ["-simulate"]):
        r = subprocess.run([CLI, "-builtin-raft", "-coverage"] + refused + model, capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 2 and "-coverage counts whole single-GPU searches" in r.stderr
