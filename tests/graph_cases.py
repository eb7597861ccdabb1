"""Inputs and expected values of the state graph tests (test_graph.py): the models, the
oracle's levels and out-edges, states the oracle did not reach, and a reader of the dot
files rmc-tlc -dump writes.  Everything expected here comes from oracle/raft_spec.py
(successors, in_constraint, canonical); nothing is read from the engine.  Test
infrastructure only."""
import collections
import functools
import itertools
import re

from oracle import raft_spec as R

TINY2 = dict(n_servers=2, n_values=1, max_term=2, max_log_len=1, max_msgs=2, max_dup=1)
SMALL = dict(n_servers=3, n_values=2, max_term=2, max_log_len=1, max_msgs=1, max_dup=1)
SYM9 = dict(n_servers=3, n_values=2, max_term=2, max_log_len=1, max_msgs=2, max_dup=1)
K8 = dict(n_servers=3, n_values=2, max_term=2, max_log_len=1, max_msgs=5, max_dup=1)
S5 = dict(n_servers=5, n_values=1, max_term=2, max_log_len=1, max_msgs=2, max_dup=1)
S5K8 = dict(n_servers=5, n_values=1, max_term=2, max_log_len=1, max_msgs=5, max_dup=1)

Case = collections.namedtuple("Case", "params symmetry max_depth distinct")
# the smallest shapes where each path can go wrong: a fixpoint (no unexpanded level, stutters, 31
# levels), depth-bounded prefixes (an unexpanded last level), SYMMETRY (canonical keys, ties), a
# bag of 8 slots, 5 servers (more than 64 lanes), and the largest shape under SYMMETRY
CASES = {
    "tiny2": Case(TINY2, False, 0, 12975),
    "small9": Case(SMALL, False, 9, 2433),
    "sym9": Case(SYM9, True, 9, 1277),
    "k8": Case(K8, False, 7, None),
    "s5": Case(S5, False, 6, 5657),
    "s5k8sym": Case(S5K8, True, 5, 55),
}


def model_of(name):
    p = CASES[name].params
    return R.Model(n_servers=p["n_servers"], n_values=p["n_values"], max_term=p["max_term"], max_log=p["max_log_len"],
                   max_msgs=p["max_msgs"], max_dup=p["max_dup"])


@functools.lru_cache(maxsize=None)
def _canonical(model, s):
    return R.canonical(model, s)


def key_of(name, s):
    """The oracle's name of the node state s belongs to: s itself, under SYMMETRY the
    representative of its orbit."""
    return _canonical(model_of(name), s) if CASES[name].symmetry else s


@functools.lru_cache(maxsize=None)
def out_edges(name, s):
    """Counter of (family, key of the successor) over the in-CONSTRAINT successors of s:
    the edges an expanded source must have (stutters included, one per enabled lane)."""
    m = model_of(name)
    return collections.Counter((f, key_of(name, t)) for f, _p, t in R.successors(m, s) if R.in_constraint(m, t))


@functools.lru_cache(maxsize=None)
def levels(name):
    """The oracle's levels as frozensets of keys: level d is expanded while d < max_depth
    (rmc_config.max_depth; 0: to fixpoint).  Returns (levels, expanded levels)."""
    c = CASES[name]
    m = model_of(name)
    s0 = R.init_state(m)
    seen = {key_of(name, s0)}
    frontier, out, depth, expanded = [s0], [frozenset(seen)], 1, 0
    while frontier and (c.max_depth == 0 or depth < c.max_depth):
        new = {}
        for s in frontier:
            for f, _p, t in R.successors(m, s):
                if R.in_constraint(m, t):
                    k = key_of(name, t)
                    if k not in seen:
                        new.setdefault(k, t)
        expanded += 1
        seen.update(new)
        frontier = list(new.values())
        if frontier:
            out.append(frozenset(new))
            depth += 1
    return tuple(out), expanded


def all_keys(name):
    return frozenset().union(*levels(name)[0])


def beyond(name, limit=200):
    """States the oracle did not reach: in-CONSTRAINT successors of the last level that
    are in no level (one level past a depth bound), then stored states with a mutated
    field (a term, a vote, a commit index) whose key is in no level either."""
    m = model_of(name)
    lv, _ = levels(name)
    seen = all_keys(name)
    out = []
    if CASES[name].max_depth:
        for k in sorted(lv[-1], key=repr):
            for _f, _p, t in R.successors(m, k):
                if R.in_constraint(m, t) and key_of(name, t) not in seen:
                    out.append(t)
            if len(out) >= limit:
                break
    S = m.n_servers
    for k in itertools.islice(sorted(lv[len(lv) // 2], key=repr), limit):
        for i in range(S):
            for t in (k._replace(currentTerm=R.tset(k.currentTerm, i, (k.currentTerm[i] + 1) % (m.max_term + 1))),
                      k._replace(votedFor=R.tset(k.votedFor, i, (i + 1) % S)),
                      k._replace(commitIndex=R.tset(k.commitIndex, i, m.max_log - k.commitIndex[i]))):
                if t != k and R.in_constraint(m, t) and key_of(name, t) not in seen:
                    out.append(t)
    assert len(out) >= 20, (name, len(out))
    return out[:limit]


# ---- a reader of rmc-tlc -dump dot files -------------------------------------------------
NODE_RE = re.compile(r'^(-?\d+) \[label="(.*)"(,style = filled\]|\];)$')
EDGE_RE = re.compile(r'^(-?\d+) -> (-?\d+)(?: \[label="([A-Za-z]+)"\])?;$')
RANK_RE = re.compile(r'^\{rank = same; ((?:-?\d+;)+)\}$')
Dot = collections.namedtuple("Dot", "nodes initial edges ranks")


def read_dot(text):
    """nodes: {id: label}; initial: ids drawn filled; edges: [(a, b, label or None)] in
    file order; ranks: [[id]] per rank line."""
    lines = text.split("\n")
    assert lines[:4] == ["strict digraph DiskGraph {", "nodesep=0.35;", "subgraph cluster_graph {", 'color="white";']
    assert lines[-3:] == ["}", "}", ""]
    nodes, initial, edges, ranks = {}, set(), [], []
    for ln in lines[4:-3]:
        if (g := NODE_RE.match(ln)):
            assert int(g[1]) not in nodes, ln
            nodes[int(g[1])] = g[2]
            if g[3].startswith(","):
                initial.add(int(g[1]))
        elif (g := EDGE_RE.match(ln)):
            edges.append((int(g[1]), int(g[2]), g[3]))
        elif (g := RANK_RE.match(ln)):
            ranks.append([int(x) for x in g[1].split(";") if x])
        else:
            raise AssertionError("unrecognised line: " + ln[:200])
    return Dot(nodes, initial, edges, ranks)


def strip_labels(text):
    """A dot file without its state and action labels (under SYMMETRY which member of an
    orbit is stored, and so printed, may differ between runs; the ids do not)."""
    return re.sub(r'label="[^"]*(?:\\.[^"]*)*"', 'label=""', text)


def signed(key):
    return key - (1 << 64) if key >> 63 else key
