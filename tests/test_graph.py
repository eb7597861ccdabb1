"""The state graph export on the GPU (rmc_get_levels, rmc_read_states, rmc_find_states,
rmc_graph_edges; rmc-tlc -dump) against the Python oracle (oracle/raft_spec.py through
tests/graph_cases.py): the levels, the stored states and their keys, the lookup, and
every edge of every expanded source, on the smallest shapes where each path can go wrong
(graph_cases.CASES).  One finished search per case is shared by the tests of the case."""
import collections
import ctypes as C
import os
import subprocess

import pytest

import rmc
from oracle import raft_spec as R
from tests import graph_cases as G
from tests.convert import from_view, to_view

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
SPECS = os.path.join(ROOT, "specs")
NAMES = list(G.CASES)
READ = 512  # views per read (a StateView is about 20 KB)


def config(name, **kw):
    c = G.CASES[name]
    kw.setdefault("state_capacity", 1 << 16)
    return rmc.make_config(symmetry=c.symmetry, max_depth=c.max_depth, **c.params, **kw)


class Finished:
    """A finished search and its graph as the calls return it."""

    def __init__(self, name, ck, res):
        self.name, self.ck, self.res = name, ck, res
        self.cb_levels = list(ck.levels)  # run()'s progress rows
        self.starts = ck.levels()
        self.states, self.keys = [], []
        for a in range(0, res.distinct, READ):
            st, ks = ck.read_states(a, min(READ, res.distinct - a), keys=True)
            self.states += [from_view(v) for v in st]
            self.keys += ks
        self.edges = [(e.src, e.dst, e.family, e.instance) for e in ck.graph_edges(0, res.distinct)]
        self.expanded = res.distinct - res.left_on_queue


def finish(name, ck):
    res = ck.run()
    return Finished(name, ck, res)


_OPEN = {}


def finished(name):
    if name not in _OPEN:
        _OPEN[name] = finish(name, rmc.Checker(config(name)))
    return _OPEN[name]


@pytest.fixture(scope="module", autouse=True)
def _close_ctxs():
    yield
    for f in _OPEN.values():
        f.ck.close()
    _OPEN.clear()


def check_edges(f):
    """Every expanded source's edges are the oracle's in-CONSTRAINT successors of the state
    stored there (as a multiset of (family, node of the destination)); no other source has
    any; the order is (src, instance)."""
    name = f.name
    by_src = collections.defaultdict(collections.Counter)
    for src, dst, fam, inst in f.edges:
        assert dst < f.res.distinct, (src, dst, fam, inst)
        assert 0 <= fam < 10 and inst >= 0
        by_src[src][(rmc.FAMILIES[fam], G.key_of(name, f.states[dst]))] += 1
    assert [(e[0], e[3]) for e in f.edges] == sorted((e[0], e[3]) for e in f.edges)
    assert len({(e[0], e[3]) for e in f.edges}) == len(f.edges)  # one edge per (source, lane)
    assert all(src < f.expanded for src in by_src)
    for src in range(f.expanded):
        assert by_src[src] == G.out_edges(name, f.states[src]), (src, f.states[src])
    assert any(e[0] == e[1] for e in f.edges), "no stuttering edge in the graph: the case shows nothing about them"
    if f.res.left_on_queue:
        assert f.expanded == f.starts[-2]  # the unexpanded sources are the last level


@pytest.mark.parametrize("name", NAMES)
def test_levels(name):
    f = finished(name)
    lv, expanded_levels = G.levels(name)
    want = [0]
    for level in lv:
        want.append(want[-1] + len(level))
    print(name, "starts", f.starts, "oracle", want)
    assert f.starts == want and f.starts[-1] == f.res.distinct == len(f.states)
    if G.CASES[name].distinct is not None:
        assert f.res.distinct == G.CASES[name].distinct
    assert len(f.starts) == f.res.depth + 1
    # the progress callback: one row per expanded level, cumulative distinct after it
    assert len(f.cb_levels) == expanded_levels
    assert [f.starts[1]] + [row[2] for row in f.cb_levels if row[3]] == f.starts[1:]


@pytest.mark.parametrize("name", NAMES)
def test_states_are_the_oracles(name):
    f = finished(name)
    lv, _ = G.levels(name)
    for d, level in enumerate(lv):
        got = [G.key_of(name, s) for s in f.states[f.starts[d]:f.starts[d + 1]]]
        assert len(got) == len(set(got)) == len(level)  # one stored member per node
        assert set(got) == level, d + 1


@pytest.mark.parametrize("name", NAMES)
def test_keys_are_rmc_state_keys(name):
    f = finished(name)
    assert len(set(f.keys)) == f.res.distinct
    for a in range(0, f.res.distinct, READ):
        st = f.ck.read_states(a, min(READ, f.res.distinct - a))
        assert f.ck.state_keys(st) == f.keys[a:a + len(st)]


@pytest.mark.parametrize("name", NAMES)
def test_lookup(name):
    f = finished(name)
    model = G.model_of(name)
    for a in range(0, f.res.distinct, READ):
        st = f.ck.read_states(a, min(READ, f.res.distinct - a))
        assert f.ck.find_states(st) == list(range(a, a + len(st)))
    if G.CASES[name].symmetry:  # any member of an orbit finds the stored representative
        S = model.n_servers
        for a in range(0, f.res.distinct, READ):
            part = f.states[a:a + READ]
            perms = [tuple((i + 1 + (a + t) % (S - 1)) % S for i in range(S)) for t in range(len(part))]  # rotations
            copies = [R.permute_state(model, s, p) for s, p in zip(part, perms)]
            assert any(c != s for c, s in zip(copies, part))
            assert f.ck.find_states([to_view(model, c) for c in copies]) == list(range(a, a + len(part)))
    out = G.beyond(name)
    assert f.ck.find_states([to_view(model, s) for s in out]) == [rmc.NO_STATE] * len(out)


@pytest.mark.parametrize("name", NAMES)
def test_edges_are_the_oracles(name):
    check_edges(finished(name))


@pytest.mark.parametrize("name", NAMES)
def test_edge_counts_equal_rmc_expand(name):
    """Device against device: per expanded source as many edges as rmc_expand lists
    in-CONSTRAINT successors of the state stored there."""
    f = finished(name)
    p = G.CASES[name].params
    S, K = p["n_servers"], 4 if p["max_msgs"] <= 4 else 8
    lanes = 4 * S + 2 * S * S + 2 * S + 3 * K
    chunk = max(1, 4096 // lanes)
    out = (rmc.SuccView * (chunk * lanes))()
    n = C.c_size_t()
    want = collections.Counter(e[0] for e in f.edges)
    got = collections.Counter()
    for a in range(0, f.expanded, chunk):
        st = f.ck.read_states(a, min(chunk, f.expanded - a))
        f.ck._check(f.ck.lib.rmc_expand(f.ck.ctx, st, len(st), out, len(out), C.byref(n)))
        assert n.value <= len(out)
        for q in range(n.value):
            if out[q].in_constraint:
                got[a + out[q].parent] += 1
    assert got == want


@pytest.mark.parametrize("name", NAMES)
def test_chunking_and_cap(name, monkeypatch):
    f = finished(name)
    D = f.res.distinct
    as_list = lambda es: [(e.src, e.dst, e.family, e.instance) for e in es]
    cuts = sorted({0, 1, 7, D // 3 + 1, f.expanded - 1, f.expanded, D})
    parts = []
    for a, b in zip(cuts, cuts[1:]):
        parts += as_list(f.ck.graph_edges(a, b))
    assert parts == f.edges
    assert as_list(f.ck.graph_edges(5, 5)) == []
    few, n_out = f.ck.graph_edges(0, D, cap=5)
    assert n_out == len(f.edges) and as_list(few) == f.edges[:5]
    none, n_out = f.ck.graph_edges(0, D, cap=0)
    assert n_out == len(f.edges) and len(none) == 0
    # the internal chunks (2^18 and 2^16 states by default): an odd size below the model's
    monkeypatch.setenv("RMC_GRAPH_CHUNK", "333")
    assert as_list(f.ck.graph_edges(0, D)) == f.edges
    few, n_out = f.ck.graph_edges(0, D, cap=400)
    assert n_out == len(f.edges) and as_list(few) == f.edges[:400]
    st, ks = f.ck.read_states(0, min(D, 1000), keys=True)
    assert ks == f.keys[:len(st)] and [from_view(v) for v in st] == f.states[:len(st)]
    assert f.ck.find_states(st) == list(range(len(st)))


def test_verification_ctx():
    """A RMC_FLAG_VERIFY_STATES ctx: the index is the one verification published during
    the run (an untagged set)."""
    with rmc.Checker(config("tiny2", verify_states=True)) as ck:
        f = finish("tiny2", ck)
        assert f.res.collisions == 0 and f.res.distinct == 12975
        check_edges(f)
        # the same keys (no salt, no epoch in a key); the order inside a level is the run's own
        assert sorted(f.keys) == sorted(finished("tiny2").keys)


def test_second_run_on_a_ctx():
    """The next set epoch (the first run's entries stay in the set as another epoch's),
    another fingerprint salt, and the index rebuilt: a graph call between the runs
    builds the first run's."""
    first = finished("tiny2")
    with rmc.Checker(config("tiny2")) as ck:
        ck.run()
        assert len(ck.graph_edges(0, 100)) == sum(1 for e in first.edges if e[0] < 100)
        ck.set_seed(12345)
        f = finish("tiny2", ck)
        check_edges(f)
        assert set(f.keys).isdisjoint(first.keys)  # another member of the hash family
        assert f.ck.find_states(f.ck.read_states(0, 200)) == list(range(200))


def refused(code, *words):
    class Ctx:
        def __enter__(self):
            self.info = pytest.raises(rmc.RmcError)
            self.exc = self.info.__enter__()
            return self

        def __exit__(self, *a):
            r = self.info.__exit__(*a)
            assert self.exc.value.code == code, str(self.exc.value)
            for w in words:
                assert w in str(self.exc.value), str(self.exc.value)
            return r
    return Ctx()


def test_refusals_of_arguments():
    f = finished("small9")
    ck, D = f.ck, f.res.distinct
    with refused(-22, "beyond the", str(D)):
        ck.read_states(D, 1)
    with refused(-22, "beyond the"):
        ck.read_states(0, D + 1)
    with refused(-22, "beyond the"):
        ck.graph_edges(0, D + 1)
    with refused(-22, "beyond the"):
        ck.graph_edges(5, 4)
    n = C.c_size_t()
    idx = (C.c_uint64 * 1)()
    st = ck.read_states(0, 1)
    assert ck.lib.rmc_read_states(ck.ctx, 0, 1, None, None) == -22 and b"NULL" in ck.lib.rmc_last_error(ck.ctx)
    assert ck.lib.rmc_find_states(ck.ctx, None, 1, idx) == -22 and b"NULL" in ck.lib.rmc_last_error(ck.ctx)
    assert ck.lib.rmc_find_states(ck.ctx, st, 1, None) == -22
    assert ck.lib.rmc_graph_edges(ck.ctx, 0, 1, None, 4, C.byref(n)) == -22 and b"NULL" in ck.lib.rmc_last_error(ck.ctx)
    assert ck.lib.rmc_graph_edges(ck.ctx, 0, 1, None, 0, None) == -22
    assert ck.lib.rmc_get_levels(ck.ctx, None, 3, C.byref(n)) == -22
    bad = ck.read_states(0, 2)
    bad[1].currentTerm[0] = 99  # no packed word holds it
    with refused(-22, "state 1"):
        ck.find_states(bad)
    assert ck.find_states(ck.read_states(0, 0)) == [] and len(ck.read_states(D, 0)) == 0


def test_refusals_of_ctx_states(tmp_path):
    calls = [lambda ck: ck.levels(), lambda ck: ck.read_states(0, 1), lambda ck: ck.find_states([rmc.StateView()]),
             lambda ck: ck.graph_edges(0, 1)]
    # before a completed run
    with rmc.Checker(config("tiny2")) as ck:
        for call in calls:
            with refused(-71, "no completed rmc_run_bfs"):
                call(ck)
    # a ctx created with RMC_FLAG_SPILL
    with rmc.Checker(config("tiny2", spill=True, device_window=4096)) as ck:
        ck.run()
        for call in calls:
            with refused(-71, "RMC_FLAG_SPILL", "resident"):
                call(ck)
    # after rmc_recover and before the next run; then the continued search's graph
    with rmc.Checker(rmc.make_config(max_depth=8, state_capacity=1 << 16, **G.TINY2)) as ck:
        ck.run()
        assert len(ck.graph_edges(0, 10)) > 0
        ck.checkpoint(str(tmp_path / "ck"))
        ck.recover(str(tmp_path / "ck"))
        for call in calls:
            with refused(-71, "rmc_recover"):
                call(ck)
    # a wide ctx: the levels only
    wide = rmc.make_config(n_servers=2, n_values=1, max_term=20, max_log_len=1, max_msgs=2, max_dup=1, max_depth=4,
                           state_capacity=1 << 12)
    with rmc.Checker(wide) as ck:
        res = ck.run()
        starts = ck.levels()
        assert starts[0] == 0 and starts[-1] == res.distinct and len(starts) == res.depth + 1
        for call in calls[1:]:
            with refused(-71, "wide layout"):
                call(ck)
    # a run that stopped at a violation: no edges (the other three still work); with
    # RMC_FLAG_CONTINUE the same search has them
    bug = dict(G.SMALL)
    stop = rmc.make_config(bug_quorum=True, invariants=rmc.INV_TYPEOK | rmc.INV_ONE_LEADER, state_capacity=1 << 18, **bug)
    with rmc.Checker(stop) as ck:
        res = ck.run()
        assert res.violated_inv and res.distinct > 300
        with refused(-71, "violation", "RMC_FLAG_CONTINUE"):
            ck.graph_edges(0, 1)
        st = ck.read_states(res.distinct - 300, 300)
        assert ck.find_states(st) == list(range(res.distinct - 300, res.distinct)) and ck.levels()[-1] == res.distinct
    with rmc.Checker(rmc.make_config(bug_quorum=True, invariants=rmc.INV_TYPEOK | rmc.INV_ONE_LEADER, continue_=True,
                                     max_depth=res.violation_depth, state_capacity=1 << 18, **bug)) as ck:
        res = ck.run()
        assert res.violated_inv and len(ck.graph_edges(0, res.distinct)) > res.distinct
    # a sharded ctx (a world of one over a host transport that copies)
    def alltoallv(_u, send, send_bytes, recv, _recv_bytes):
        C.memmove(recv, send, send_bytes[0])
        return 0

    def allgather(_u, send, nbytes, recv):
        C.memmove(recv, send, nbytes)
        return 0
    tr = rmc.Transport(None, rmc.ALLTOALLV_FN(alltoallv), rmc.ALLGATHER_FN(allgather))
    with rmc.Checker(config("tiny2")) as ck:
        ck.shard(0, 1, transport=tr, keys_per_dest=1 << 12, sent_cache_slots=1 << 12)
        for call in calls:
            with refused(-71, "sharded"):
                call(ck)


# ---- rmc-tlc -dump ----------------------------------------------------------------------
def cli(*args):
    r = subprocess.run([CLI, "-builtin-raft", "-capacity", "65536"] + list(args), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_cli_dump_dot_is_the_oracles_graph(tmp_path):
    """-dump dot,actionlabels of MCraftTiny2 -depth 6: the node ids are the keys, nodes and
    edges are the oracle's graph, one rank line per level; a second run writes the same bytes."""
    a, b = tmp_path / "a.dot", tmp_path / "b.dot"
    out = cli("-dump", "dot,actionlabels", str(a), "-depth", "6", os.path.join(SPECS, "MCraftTiny2.tla"))
    assert "State graph written to" in out
    cli("-dump", "dot,actionlabels", str(b), "-depth", "6", os.path.join(SPECS, "MCraftTiny2.tla"))
    text = a.read_text()
    assert text == b.read_text()
    d = G.read_dot(text)
    # the same search through the library: states, keys, edges
    with rmc.Checker(rmc.make_config(max_depth=6, state_capacity=1 << 16, **G.TINY2)) as ck:
        f = finish("tiny2", ck)
    lv_sizes = [b - a for a, b in zip(f.starts, f.starts[1:])]
    assert lv_sizes == [1, 2, 7, 16, 35, 72]  # the oracle's first six levels (graph_cases.levels("tiny2"))
    assert [len(level) for level in G.levels("tiny2")[0][:6]] == lv_sizes
    ids = [G.signed(k) for k in f.keys]
    assert sorted(d.nodes) == sorted(ids) and d.initial == {ids[0]}
    assert [sorted(r) for r in d.ranks] == [sorted(ids[a:b]) for a, b in zip(f.starts, f.starts[1:])]
    assert all(r == sorted(r) for r in d.ranks)
    # every node's label is its state's text: the oracle's state read back from the label's fields
    state_of = dict(zip(ids, f.states))
    for i, s in state_of.items():
        assert d.nodes[i].count("\\n") == 9 and d.nodes[i].startswith("/\\\\ messages = ")
        terms = "(" + " @@ ".join(f"r{k + 1} :> {t}" for k, t in enumerate(s.currentTerm)) + ")"
        assert f"/\\\\ currentTerm = {terms}\\n" in d.nodes[i]
    # the edges: the oracle's successors of every expanded state, by family
    got = collections.defaultdict(collections.Counter)
    for x, y, fam in d.edges:
        got[x][(fam, state_of[y])] += 1
    assert d.edges == sorted(d.edges, key=lambda e: (e[0], e[1], rmc.FAMILIES.index(e[2])))
    for i, s in state_of.items():
        expanded = f.keys.index(i % (1 << 64)) < f.expanded
        assert got[i] == (G.out_edges("tiny2", s) if expanded else collections.Counter()), s
    assert len(d.edges) == len(f.edges)


def test_cli_dump_symmetry_and_plain(tmp_path):
    """Under SYMMETRY two runs write the same file up to the labels (which member of an
    orbit is stored may differ); -dump FILE has one block per distinct state."""
    a, b = tmp_path / "a.dot", tmp_path / "b.dot"
    for p in (a, b):
        out = cli("-dump", "dot,actionlabels", str(p), "-depth", "7", os.path.join(SPECS, "MCraftBenchSym.tla"))
        assert "SYMMETRY Permutations(Server)" in out
    assert G.strip_labels(a.read_text()) != a.read_text()
    assert G.strip_labels(a.read_text()) == G.strip_labels(b.read_text())
    d = G.read_dot(a.read_text())
    assert len(d.ranks) == 7 and sum(len(r) for r in d.ranks) == len(d.nodes) and len(d.edges) > len(d.nodes)
    plain = tmp_path / "states.dump"
    out = cli("-dump", str(plain), os.path.join(SPECS, "MCraftTiny2.tla"))
    assert "12975 distinct states found" in out and "States written to" in out
    blocks = plain.read_text().split("\n\n")
    assert blocks[-1] == "" and len(blocks) - 1 == 12975
    assert all(b.startswith(f"State {k + 1}:\n/\\ messages = ") and b.count("\n") == 10 for k, b in enumerate(blocks[:-1]))
    assert len(set(b.split("\n", 1)[1] for b in blocks[:-1])) == 12975
