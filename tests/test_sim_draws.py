"""The simulators (k_simulate, k_wsimulate_w, k_wsimulate) held to the stated draw
rules: every draw is a function of (seed, behaviour), so tests/sim_rules.py
predicts a run's replays, tallies and violation report exactly, and the device
must give exactly those.  The enabled lanes the prediction stands on come from
rmc_expand (the kernels' own notion of enabled and of within the bounds), one
call per step, and every parent so expanded is also compared with the Python
restatement of Next (oracle/raft_spec.py) as test_gpu.py's compare_expand does;
the first violated invariant comes from the Python invariants.

Seeds and what the predictions held on an MI355X (N = 32 behaviours, depth 10;
steps / truncated / deadlocked / mode-0 steps that filtered a lane / of those, the
steps whose pick differs from mode 1's / behaviours that ran to depth) are listed
in OBSERVED below, next to the seed."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from collections import Counter
from dataclasses import dataclass

import pytest

import rmc
from oracle import raft_spec as R
from tests import sim_rules as SR
from tests.convert import from_view, to_view
from tests.test_sim import smoke_cfg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, DEPTH = 32, 10
ALL_INVARIANTS = 1023


def _fixture_cfg(**kw):
    c, _, _ = rmc.model_from_files(os.path.join(ROOT, "tests", "golden", "models", "SmokeFixture.cfg"),
                                   builtin_raft=True, simulate=True)
    c.state_capacity = 1 << 12
    c.invariants = kw.get("invariants", rmc.INV_TYPEOK)
    return c


def _cfg(S, V, term, log, msgs, dup):
    return lambda **kw: rmc.make_config(n_servers=S, n_values=V, max_term=term, max_log_len=log, max_msgs=msgs,
                                        max_dup=dup, state_capacity=1 << 12, **kw)


@dataclass(frozen=True)
class Spec:
    layout: str
    S: int
    V: int
    bounds: tuple  # max_term, max_log_len, max_msgs, max_dup
    make: object
    tight: bool

    @property
    def modes(self):
        return (0, 1) if self.layout == "packed" else (0, 1, 2)

    @property
    def model(self):
        t, lg, m, d = self.bounds
        return R.Model(n_servers=self.S, n_values=self.V, max_term=t, max_log=lg, max_msgs=m, max_dup=d)


MODELS = {
    "packed-loose": Spec("packed", 3, 2, (14, 3, 8, 3), smoke_cfg, False),
    "packed-tight": Spec("packed", 3, 1, (2, 1, 3, 1), _cfg(3, 1, 2, 1, 3, 1), True),
    "wide-loose": Spec("wide", 3, 2, (255, 32, 64, 255), _fixture_cfg, False),
    "wide-tight": Spec("wide", 3, 1, (2, 4, 3, 1), _cfg(3, 1, 2, 4, 3, 1), True),  # Len(log) <= 4: the wide layout
    "wide-s2": Spec("wide", 2, 1, (3, 4, 4, 2), _cfg(2, 1, 3, 4, 4, 2), True),     # the smallest lane table, |Value| = 1
}
# SmokeInit's states all hold a log of 3 entries, beyond packed-tight's MaxLogLen 1.  From a
# parent outside the CONSTRAINT the packed layout's bound check (delta_fp: the fields a lane
# changes, which is the whole CONSTRAINT for a parent within it) and the oracle's whole-state
# CONSTRAINT differ, so the lane lists could not be held to the oracle: that model starts
# from Init only.
CASES = [(name, init, mode) for name, sp in MODELS.items() for init in ("smoke", "init") for mode in sp.modes
         if (name, init) != ("packed-tight", "smoke")]
# The seed of every case: the first of 1, 2, .. whose predictions meet vacuous() in every
# mode of every model and in the wrapped-grid tests (found on an MI355X: the lane lists
# come from rmc_expand).  Seed 1 met them all.
SEED = 1
# (steps, truncated, deadlocked, mode-0 steps that filtered a lane, of those the steps whose
# pick is not mode 1's, behaviours that ran to depth) of every prediction, as observed then;
# the wrapped grids' 64 behaviours at depth 8: packed-tight from Init in mode 1 (306, 40, 0,
# 0, 0, 24), wide-tight from SmokeInit in mode 2 (189, 59, 0, 0, 0, 5)
OBSERVED = {
    ("packed-loose", "smoke", 0): (288, 0, 0, 132, 81, 32),
    ("packed-loose", "smoke", 1): (265, 7, 0, 0, 0, 25),
    ("packed-loose", "init", 0): (288, 0, 0, 3, 1, 32),
    ("packed-loose", "init", 1): (287, 1, 0, 0, 0, 31),
    ("packed-tight", "init", 0): (288, 0, 0, 230, 158, 32),
    ("packed-tight", "init", 1): (170, 27, 0, 0, 0, 5),
    ("wide-loose", "smoke", 0): (288, 0, 0, 0, 0, 32),
    ("wide-loose", "smoke", 1): (288, 0, 0, 0, 0, 32),
    ("wide-loose", "smoke", 2): (288, 0, 0, 0, 0, 32),
    ("wide-loose", "init", 0): (288, 0, 0, 0, 0, 32),
    ("wide-loose", "init", 1): (288, 0, 0, 0, 0, 32),
    ("wide-loose", "init", 2): (288, 0, 0, 0, 0, 32),
    ("wide-tight", "smoke", 0): (288, 0, 0, 90, 90, 32),
    ("wide-tight", "smoke", 1): (66, 31, 0, 0, 0, 1),
    ("wide-tight", "smoke", 2): (72, 31, 0, 0, 0, 1),
    ("wide-tight", "init", 0): (288, 0, 0, 52, 52, 32),
    ("wide-tight", "init", 1): (172, 27, 0, 0, 0, 5),
    ("wide-tight", "init", 2): (166, 27, 0, 0, 0, 5),
    ("wide-s2", "smoke", 0): (288, 0, 0, 20, 20, 32),
    ("wide-s2", "smoke", 1): (231, 15, 0, 0, 0, 17),
    ("wide-s2", "smoke", 2): (240, 15, 0, 0, 0, 17),
    ("wide-s2", "init", 0): (288, 0, 0, 18, 18, 32),
    ("wide-s2", "init", 1): (256, 12, 0, 0, 0, 20),
    ("wide-s2", "init", 2): (265, 6, 0, 0, 0, 26),
}


def first_violated(model, mask):
    def check(s):
        for r in range(10):
            if mask >> r & 1 and not R.INVARIANTS[R.INV_BITS[1 << r]](model, s):
                return r
        return None
    return check


class Lanes:
    """expand(states) for SR.predict from rmc_expand: per state its enabled lanes as
    (lane, within the bounds, successor), each parent checked against the oracle."""
    CAP = 2048  # rmc_succ_view records per call (about 46 MB)
    _buf = None

    def __init__(self, ck, model):
        self.ck, self.model, self.cache, self.calls = ck, model, {}, 0

    def __call__(self, states):
        need = [s for s in states if s not in self.cache]
        if need:
            self._expand(need)
        return [self.cache[s] for s in states]

    def _expand(self, states):
        if Lanes._buf is None:
            Lanes._buf = (rmc.SuccView * Lanes.CAP)()
        views = (rmc.StateView * len(states))(*[to_view(self.model, s) for s in states])
        n = C.c_size_t()
        self.ck._check(self.ck.lib.rmc_expand(self.ck.ctx, views, len(states), Lanes._buf, Lanes.CAP, C.byref(n)))
        self.calls += 1
        if n.value > Lanes.CAP:  # more successors than the buffer holds: in two halves
            assert len(states) > 1
            self._expand(states[:len(states) // 2])
            self._expand(states[len(states) // 2:])
            return
        per = [[] for _ in states]
        gen = [Counter() for _ in states]
        inm = [Counter() for _ in states]
        for q in range(n.value):
            sv = Lanes._buf[q]
            fam = rmc.FAMILIES[sv.family]
            gen[sv.parent][fam] += 1
            t = from_view(sv.state) if sv.in_constraint else None
            if t is not None:
                inm[sv.parent][(fam, t)] += 1
            per[sv.parent].append((sv.instance, bool(sv.in_constraint), t))
        for k, s in enumerate(states):
            ora_gen, ora_in = Counter(), Counter()
            for f, _p, t in R.successors(self.model, s):
                ora_gen[f] += 1
                if R.in_constraint(self.model, t):
                    ora_in[(f, t)] += 1
            assert gen[k] == ora_gen, s
            assert inm[k] == ora_in, s
            assert [l for l, _i, _t in per[k]] == sorted({l for l, _i, _t in per[k]}), s  # lane order, each once
            self.cache[s] = per[k]


class Bench:
    """One open Checker, lane cache and set of predictions per model."""

    def __init__(self):
        self.open, self.preds, self.inits = {}, {}, {}

    def ck(self, name, invariants=rmc.INV_TYPEOK):
        key = (name, invariants)
        if key not in self.open:
            sp = MODELS[name]
            ck = rmc.Checker(sp.make(invariants=invariants))
            assert bool(rmc.native().rmc_state_bytes(ck.cfg) > 100) == (sp.layout == "wide")
            self.open[key] = (ck, Lanes(ck, sp.model))
        return self.open[key]

    def initial(self, name, init, seed):
        key = (name, init, seed)
        if key not in self.inits:
            sp = MODELS[name]
            if init == "smoke":
                cfg = self.ck(name)[0].cfg
                self.inits[key] = [from_view(v) for v in rmc.smoke_init(cfg, 2, 2, seed)]
            else:
                self.inits[key] = [R.init_state(sp.model)]
        return self.inits[key]

    def predict(self, name, init, mode, seed, behaviours=range(N), depth=DEPTH, invariants=rmc.INV_TYPEOK):
        key = (name, init, mode, seed, behaviours, depth, invariants)
        if key not in self.preds:
            sp = MODELS[name]
            _ck, lanes = self.ck(name, invariants)
            self.preds[key] = SR.predict(sp.layout, mode, self.initial(name, init, seed), behaviours, depth, seed,
                                         lanes, first_violated(sp.model, invariants), S=sp.S, V=sp.V)
        return self.preds[key]

    def close(self):
        for ck, _l in self.open.values():
            ck.close()


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


def vacuous(name, init, mode, pred):
    """What keeps a prediction from exercising the rule it is used to check."""
    sp = MODELS[name]
    ends = Counter(w.end for w in pred.walks.values())
    why = []
    if pred.steps == 0 or len({tuple(w.states) for w in pred.walks.values()}) < 2:
        why.append("no two different walks")
    if ends["depth"] < 1:
        why.append("no behaviour runs to depth")
    if sp.tight and mode in (1, 2) and pred.truncated < 1:
        why.append("no truncated behaviour")
    if sp.tight and mode == 0 and pred.diverted_steps < 1:
        why.append("mode 0 never picks differently from mode 1")
    return why


def observed(pred):
    return (pred.steps, pred.truncated, pred.deadlocked, pred.filtered_steps, pred.diverted_steps,
            sum(w.end == "depth" for w in pred.walks.values()))


def smoke_k(init):
    return 2 if init == "smoke" else 0


def some_behaviours(pred):
    """A handful: the first three, the last, and the first of every other ending."""
    bs = sorted(pred.walks)
    pick = bs[:3] + bs[-1:]
    for end in ("truncated", "deadlocked"):
        pick += [b for b in bs if pred.walks[b].end == end][:1]
    return list(dict.fromkeys(pick))


@pytest.mark.parametrize("name,init,mode", CASES, ids=lambda x: str(x))
def test_replays_equal_the_prediction(bench, name, init, mode):
    """sim_replay(b) returns exactly the predicted states, and as many."""
    seed = SEED
    pred = bench.predict(name, init, mode, seed)
    assert not vacuous(name, init, mode, pred), observed(pred)
    ck, _ = bench.ck(name)
    for b in some_behaviours(pred):
        got = [from_view(v) for v in ck.sim_replay(b, behaviours=N, depth=DEPTH, smoke_k=smoke_k(init), seed=seed,
                                                   mode=mode)]
        want = pred.walks[b].states
        assert len(got) == len(want), (b, pred.walks[b].end, pred.walks[b].picks)
        assert got == want, (b, pred.walks[b].picks)


@pytest.mark.parametrize("name,init,mode", CASES, ids=lambda x: str(x))
def test_tallies_equal_the_prediction(bench, name, init, mode):
    """simulate(behaviours=N) returns exactly the predicted steps, truncated,
    deadlocked and init_states; the prediction is not vacuous and holds
    what OBSERVED recorded when the seed was chosen."""
    seed = SEED
    pred = bench.predict(name, init, mode, seed)
    assert not vacuous(name, init, mode, pred), observed(pred)
    assert observed(pred) == OBSERVED[(name, init, mode)]
    ck, _ = bench.ck(name)
    r = ck.simulate(behaviours=N, depth=DEPTH, smoke_k=smoke_k(init), seed=seed, mode=mode)
    assert (r.steps, r.truncated, r.deadlocked) == pred.tallies
    assert r.init_states == len(bench.initial(name, init, seed)) == (512 if init == "smoke" else 1)
    assert r.behaviours == N and r.violated_inv == 0 and pred.violation is None


@pytest.mark.parametrize("name,mode", [("packed-loose", 1), ("wide-loose", 0), ("wide-tight", 2)])
def test_the_seed_matters(bench, name, mode):
    """Another seed gives other predicted walks (other SmokeInit states too: the seed
    draws them), and the device follows each seed's."""
    seeds = (SEED, 1000003)
    preds = [bench.predict(name, "smoke", mode, s, behaviours=range(8)) for s in seeds]
    for b in range(8):
        assert preds[0].walks[b].states != preds[1].walks[b].states
    ck, _ = bench.ck(name)
    for seed, pred in zip(seeds, preds):
        r = ck.simulate(behaviours=8, depth=DEPTH, smoke_k=2, seed=seed, mode=mode)
        assert (r.steps, r.truncated, r.deadlocked) == pred.tallies
        for b in (0, 5):
            got = [from_view(v) for v in ck.sim_replay(b, behaviours=8, depth=DEPTH, smoke_k=2, seed=seed, mode=mode)]
            assert got == pred.walks[b].states


@pytest.mark.parametrize("name", ["packed-loose", "wide-loose"])
def test_violation_report_is_the_least_depth_invariant_behaviour(bench, name):
    """All ten invariants on SmokeInit's states, seed 8 (chosen on the CPU from
    rmc_smoke_init, the Python invariants and the restated init index): all 32
    behaviours start in a violating state, 17 of them violating MessagesInv first
    (bit 3) and 15 LogMatching (bit 2); behaviour 0 is the least violating
    behaviour and violates MessagesInv, behaviour 2 is the least that violates
    LogMatching.  The report must be (LogMatching, depth 1, behaviour 2): the
    invariant's index beats the behaviour's."""
    seed = 8
    pred = bench.predict(name, "smoke", 1, seed, depth=6, invariants=ALL_INVARIANTS)
    check = first_violated(MODELS[name].model, ALL_INVARIANTS)
    violating = [(check(w.states[0]), b) for b, w in pred.walks.items() if check(w.states[0]) is not None]
    assert len(violating) >= 2 and len({v for v, _b in violating}) >= 2
    assert min(violating)[1] != min(b for _v, b in violating)
    assert pred.violation == (1, 2, 2)
    ck, _ = bench.ck(name, ALL_INVARIANTS)
    r = ck.simulate(behaviours=N, depth=6, smoke_k=2, seed=seed, mode=1)
    assert (r.violation_depth, r.violated_inv, r.violation_behaviour) == (1, 1 << 2, 2)
    assert (r.steps, r.truncated, r.deadlocked) == pred.tallies
    got = ck.sim_replay(r.violation_behaviour, behaviours=N, depth=6, smoke_k=2, seed=seed, mode=1)
    assert len(got) == r.violation_depth
    assert [from_view(v) for v in got] == pred.walks[2].states


@pytest.mark.parametrize("name,init,mode,n1", [("packed-tight", "init", 1, 1 << 20), ("wide-tight", "smoke", 2, 32768)])
def test_wrapped_grids_walk_the_behaviours_past_the_launch(bench, name, init, mode, n1):
    """k_simulate launches at most 2^20 threads and k_wsimulate_w at most 32,768
    waves; behaviours past that are a thread's or a wave's second one.  Behaviour
    b's walk does not depend on the number of behaviours, so the tallies of
    N1 + 64 behaviours minus those of N1 are exactly the predicted tallies of
    behaviours N1 .. N1 + 63, and the replay of N1 + 5 is its prediction."""
    seed, depth = SEED, 8
    pred = bench.predict(name, init, mode, seed, behaviours=range(n1, n1 + 64), depth=depth)
    assert pred.steps > 0 and pred.truncated > 0 and any(w.end == "depth" for w in pred.walks.values())
    ck, _ = bench.ck(name)
    lo = ck.simulate(behaviours=n1, depth=depth, smoke_k=smoke_k(init), seed=seed, mode=mode)
    hi = ck.simulate(behaviours=n1 + 64, depth=depth, smoke_k=smoke_k(init), seed=seed, mode=mode)
    assert lo.violated_inv == 0 and hi.violated_inv == 0
    assert (hi.steps - lo.steps, hi.truncated - lo.truncated, hi.deadlocked - lo.deadlocked) == pred.tallies
    got = [from_view(v) for v in ck.sim_replay(n1 + 5, behaviours=n1 + 64, depth=depth, smoke_k=smoke_k(init), seed=seed,
                                               mode=mode)]
    assert got == pred.walks[n1 + 5].states


_THREAD_KERNEL_PROBE = r"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], "raft.tla_amd"))
sys.path.insert(0, sys.argv[1])
import rmc
from tests import sim_rules as SR
from tests.convert import from_view
n, depth, seed, b = (int(x) for x in sys.argv[2:6])
cfg = rmc.make_config(n_servers=3, n_values=1, max_term=2, max_log_len=4, max_msgs=3, max_dup=1, state_capacity=1 << 12)
out = {}
with rmc.Checker(cfg) as ck:
    for mode in (0, 1, 2):
        r = ck.simulate(behaviours=n, depth=depth, smoke_k=2, seed=seed, mode=mode)
        views = ck.sim_replay(b, behaviours=n, depth=depth, smoke_k=2, seed=seed, mode=mode)
        h = hashlib.sha256(repr(SR.plain([from_view(v) for v in views])).encode()).hexdigest()
        out[mode] = [r.steps, r.truncated, r.deadlocked, len(views), h]
print(json.dumps(out))
"""


def test_thread_kernel_follows_the_prediction(bench):
    """k_wsimulate (RMC_WSIM=0, read once per process: a fresh child) on the wide
    tight model in the three modes: the tallies and one replayed behaviour equal
    the prediction, as the wave kernel's do in the tests above."""
    seed, b = SEED, 1
    env = dict(os.environ, RMC_WSIM="0")
    p = subprocess.run([sys.executable, "-c", _THREAD_KERNEL_PROBE, ROOT, str(N), str(DEPTH), str(seed), str(b)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in (0, 1, 2):
        pred = bench.predict("wide-tight", "smoke", mode, seed)
        states = pred.walks[b].states
        want = [*pred.tallies, len(states), hashlib.sha256(repr(SR.plain(states)).encode()).hexdigest()]
        assert got[str(mode)] == want, mode
