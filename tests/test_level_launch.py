"""Level-long expansion launches (DESIGN.md "Kernels", round 16): one launch per level up
to 2^28 states, and on the ring window (RMC_FLAG_SPILL with the trace links in HBM) the
device-side admission of rmc_plan.h — a launch the worst-case bound would cut is launched
whole, stops claiming work units before the ring could wrap onto live states, and is
launched again from where it stopped.  Every case is compared level by level (new states,
cumulative generated) and in its totals with tests/golden/oracle_levels.json."""
import json
import os
import subprocess
import sys

import pytest

import rmc
from tests.test_gpu import GOLDEN, ROOT, cfg_from, spill_cfg

pytestmark = pytest.mark.gpu


def expanded_levels(g):
    """Levels the search expands: all of them (the last one yields nothing new), or all
    but the last under a depth bound."""
    return g["depth"] - (1 if g["left_on_queue"] else 0)


def check_counts(g, res, rows):
    """rows: Checker.levels after run(), (level, cumulative generated, distinct, new, seconds)."""
    assert [1] + [r[3] for r in rows if r[3]] == g["level_new"]
    lg = g["level_generated"]  # [Init, by expanding level 1, ...]
    for k, r in enumerate(rows):
        if k + 2 <= len(lg):
            assert r[1] == sum(lg[:k + 2]), (k, r)
    assert (res.distinct, res.generated, res.depth, res.left_on_queue) == \
        (g["distinct"], g["generated"], g["depth"], g["left_on_queue"])
    assert res.violated_inv == 0 and res.deadlock == 0


def run_rows(cfg):
    with rmc.Checker(cfg) as ck:
        res = ck.run()
        return res, list(ck.levels)


@pytest.mark.parametrize("name", ["small", "tiny2_v2"])
def test_a_resident_level_is_one_launch(name):
    g = GOLDEN[name]
    assert max(g["level_new"]) < 1 << 28 and "RMC_LAUNCH_LOG2" not in os.environ
    res, rows = run_rows(cfg_from(g["params"], capacity=max(1 << 22, int(g["distinct"] * 1.25))))
    check_counts(g, res, rows)
    assert res.expand_launches == expanded_levels(g)


def test_spill_with_device_links_on_the_default_grid():
    """tiny2_log3 (14 M states, levels of up to 0.84 M) in a ring of the two largest
    consecutive levels + 4096 states, rounded up to a power of two."""
    g, cfg = spill_cfg("tiny2_log3", 4096)
    assert cfg.device_window < g["distinct"]
    res, rows = run_rows(cfg)
    assert res.spill_links_on_device and res.spills > 0
    check_counts(g, res, rows)


def test_reserve_that_does_not_fit_falls_back_to_the_bound():
    """The window of test_spill_completes_with_the_oracle_counts[small]: on the default grid
    the reserve of a level's launch exceeds the ring, so its launches are sized on the host
    by the worst-case bound as before."""
    g, cfg = spill_cfg("small", 1 << 16)
    res, rows = run_rows(cfg)
    assert res.spill_links_on_device and res.spills > 0
    check_counts(g, res, rows)
    assert res.expand_launches > expanded_levels(g)


# ---- forced admission stops ------------------------------------------------------------------
# RMC_EXPAND_GRID (read once per process: a fresh child) keeps the launch to a few waves, so
# its reserve is small against the levels and a ring below the largest two consecutive
# levels + reserve must stop some launch.  The predicate of each case first fails on a state
# of the search's last level, so a second run with it set ends at that level with
# rmc_trace's target in it: a trace through states the ring has overwritten, whose links
# were written by launches that stopped and were launched again.  UserNotDeepest fails on
# exactly one state up to the value of the one replicated log entry (a Value cannot be
# named in the predicate language; raft.tla treats the values alike), pinned field for
# field (with MaxMsgs = 1 the one message pins the bag): one of the 30 states of level 49
# of s3_v1_msgs1 and two of the 60 of small, as oracle/raft_spec.py's BFS lists them.
# UserFewIdle (four servers timed out and restarted) first fails at level 9 of the S = 5 model by tests/predicate_cases.py oracle_violation_depth on its twin below.
DEEPEST = r"""UserNotDeepest ==
    \/ \E j \in Server : currentTerm[j] /= 2 \/ Len(log[j]) /= 1 \/ Cardinality(votesResponded[j]) /= 3
    \/ \E j \in Server : \E n \in DOMAIN log[j] : log[j][n].term /= 2 \/ log[j][n].value /= log[r1][n].value
    \/ state[r1] /= Leader \/ state[r2] /= Follower \/ state[r3] /= Follower
    \/ votedFor[r1] /= r1 \/ votedFor[r2] /= r1 \/ votedFor[r3] /= r2
    \/ commitIndex[r1] /= 1 \/ commitIndex[r2] /= 0 \/ commitIndex[r3] /= 0
    \/ Cardinality(votesGranted[r1]) /= 2 \/ r3 \in votesGranted[r1]
    \/ Cardinality(votesGranted[r2]) /= 0 \/ Cardinality(votesGranted[r3]) /= 0
    \/ nextIndex[r1][r1] /= 1 \/ nextIndex[r1][r2] /= 2 \/ nextIndex[r1][r3] /= 2
    \/ \E j \in Server : nextIndex[r2][j] /= 1 \/ nextIndex[r3][j] /= 1
    \/ matchIndex[r1][r1] /= 0 \/ matchIndex[r1][r2] /= 1 \/ matchIndex[r1][r3] /= 1
    \/ \E j \in Server : matchIndex[r2][j] /= 0 \/ matchIndex[r3][j] /= 0
    \/ \A m \in DOMAIN messages :
           IF m.mtype = AppendEntriesResponse
           THEN m.msource /= r2 \/ m.mdest /= r1 \/ m.mterm /= 2 \/ m.mmatchIndex /= 1 \/ (m.msuccess => FALSE)
           ELSE TRUE"""
IDLE = r"""UserFewIdle ==
    Cardinality({j \in Server : currentTerm[j] = 2 /\ state[j] = Follower /\ votedFor[j] = Nil}) <= 3"""
FORCED = {  # fixture: (RMC_EXPAND_GRID, device_window, predicate name, its definition)
    "small": (1, 1 << 18, "UserNotDeepest", DEEPEST),
    "s3_v1_msgs1": (2, 1 << 18, "UserNotDeepest", DEEPEST),
    "s5_prefix9": (4, 1 << 19, "UserFewIdle", IDLE),  # S = 5: 92 lanes, the 128-bit lane mask at 5 waves/SIMD
}

CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], 'raft.tla_amd'))
sys.path.insert(0, sys.argv[1])
import rmc
from oracle import raft_spec as R
from tests import predicate_cases as PC
from tests.test_gpu import GOLDEN, spill_cfg
from tests.test_predicates import check_user_trace, model_of
name, window, pred, tmp = sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5]
definition = open(os.path.join(tmp, 'definition.tla')).read()


def twin(model, s):
    S = model.n_servers
    if pred == 'UserFewIdle':
        bad = sum(1 for j in range(S) if s.currentTerm[j] == 2 and s.state[j] == R.FOLLOWER
                  and s.votedFor[j] == R.NIL) > 3
    else:  # the state UserNotDeepest pins, field for field
        bad = (s.currentTerm == (2, 2, 2) and s.state == (R.LEADER, R.FOLLOWER, R.FOLLOWER) and s.votedFor == (0, 0, 1)
               and s.commitIndex == (1, 0, 0) and s.nextIndex == ((1, 2, 2), (1, 1, 1), (1, 1, 1))
               and s.matchIndex == ((0, 1, 1), (0, 0, 0), (0, 0, 0))
               and all(len(lg) == 1 and R.rget(lg[0], 'term') == 2 and lg[0] == s.log[0][0] for lg in s.log)
               and all(v == frozenset({0, 1, 2}) for v in s.votesResponded)
               and s.votesGranted == (frozenset({0, 1}), frozenset(), frozenset())
               and any(R.rget(m, 'mtype') == R.AEP and R.rget(m, 'msource') == 1 and R.rget(m, 'mdest') == 0
                       and R.rget(m, 'mterm') == 2 and R.rget(m, 'mmatchIndex') == 1 and R.rget(m, 'msuccess')
                       for m, _c in s.messages))
    return PC.VIOLATED if bad else PC.HOLDS


g, cfg = spill_cfg(name, 0)
cfg.device_window = window
out = {}
with rmc.Checker(cfg) as ck:
    res = ck.run()
    out['rows'] = [list(r[:4]) for r in ck.levels]
    out['totals'] = [res.distinct, res.generated, res.depth, res.left_on_queue, res.violated_inv, res.deadlock]
    out['launches'], out['spills'], out['dev_links'] = res.expand_launches, res.spills, res.spill_links_on_device
p = g['params']
cfg_path, tla = PC.write_model(tmp, (pred,), n_servers=p['n_servers'], n_values=p['n_values'], max_term=p['max_term'],
                               max_log=p['max_log_len'], max_msgs=p['max_msgs'], max_dup=p['max_dup'],
                               module=PC.module_with(definition))
_c, _notes, preds = rmc.load_model(cfg_path, tla, builtin_raft=True, predicates=True)
g, cfg = spill_cfg(name, 0, invariants=0)
cfg.device_window = window
with rmc.Checker(cfg) as ck:
    ck.set_predicates(preds)
    res = ck.run()
    out['pred'] = [res.violated_inv == rmc.INV_USER0, res.violation_depth, res.depth, ck.predicate_error(),
                   res.expand_launches]
    trace = ck.trace()
    # a behaviour of the spec from Init whose last state alone fails the predicate's twin
    check_user_trace(model_of(p), trace, twin, res.violation_depth)
    out['trace_len'] = len(trace)
print(json.dumps(out))
"""


def new_states_bound(p):
    """rmc_plan.h new_states_bound for the packed shape of the model (4 bag slots up to MaxMsgs = 4)."""
    S, V, K = p["n_servers"], p["n_values"], 4 if p["max_msgs"] <= 4 else 8
    return S * max(2, S + 3, S + V + 1) + 3 * K


def launch_reserve(nf, grid_env, bound):
    """rmc_plan.h admit_reserve of the launch of a whole level of nf states: blocks cut to
    RMC_EXPAND_GRID, windows of up to 16 tiles, units of up to 8, WCAP = 512 list entries."""
    grid = min(-(-nf // 256), grid_env)
    wt = max(1, min(16, -(-nf // (grid * 256))))
    ut = 8
    units = -(-nf // (256 * wt)) * 4 * -(-wt // ut)
    return min(grid * 4, units) * (min(wt, ut) * 64 * bound + 512)


@pytest.mark.parametrize("name", sorted(FORCED))
def test_forced_admission_stops_keep_every_count_and_the_trace(name, tmp_path):
    grid, window, pred, definition = FORCED[name]
    g = GOLDEN[name]
    L, bound, E = g["level_new"], new_states_bound(g["params"]), expanded_levels(g)
    assert 1 <= grid <= 4 and window & (window - 1) == 0
    # the search completes: every level is launched whole — the bound leaves it room, or its
    # reserve fits beside it (admit_stop > count) — so no launch is cut on the host, and a
    # launch count above the levels can only come from admission stops
    for k in range(E):
        assert L[k] * bound + L[k] <= window or L[k] + launch_reserve(L[k], grid, bound) < window, k
    # ... and cannot without a stop: the ring is below the largest two consecutive levels
    # + the reserve of the first one's launch
    assert window < max(L[k] + L[k + 1] + launch_reserve(L[k], grid, bound) for k in range(min(E, len(L) - 1)))
    (tmp_path / "definition.tla").write_text(definition)
    script = tmp_path / "forced.py"
    script.write_text(CHILD)
    env = dict(os.environ, RMC_EXPAND_GRID=str(grid))
    r = subprocess.run([sys.executable, str(script), ROOT, name, str(window), pred, str(tmp_path)],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(name, "launches", out["launches"], "expanded levels", E, "spills", out["spills"], "predicate run", out["pred"])

    class Res:
        distinct, generated, depth, left_on_queue, violated_inv, deadlock = out["totals"]
    # (s5_prefix9's 137,482 states never wrap a ring its reserve fits in: its stops come from
    # the reserve alone; the two S = 3 searches pass out of their window several times)
    assert out["dev_links"] and (out["spills"] > 0) == (window < g["distinct"])
    assert name == "s5_prefix9" or out["spills"] > 0
    check_counts(g, Res, [tuple(r) for r in out["rows"]])
    assert out["launches"] > E
    # the predicate's run: its target is a state of the search's last level, traced back to Init
    is_user0, vdepth, depth, error, launches = out["pred"]
    assert is_user0 and not error and vdepth == depth == g["depth"] == out["trace_len"]
    assert launches > g["depth"] - 1
