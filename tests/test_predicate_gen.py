"""Generated predicates on the GPU: the pool of tests/predicate_gen.py through
rmc_eval_predicates (k_pred_eval on the eight packed shapes, k_wpred_eval on the three wide
records) and rmc_eval_actions (k_act_eval).  The device's verdicts equal the evaluator's of
predicate_gen.py and the host VM's (tests/native/pred_check.cpp, act_check.cpp) byte for
byte: integers, no tolerance."""
import ctypes as C

import pytest

import rmc
from tests import action_cases as AC
from tests import graph_cases as G
from tests import invariant_cases as IC
from tests import predicate_gen as PG
from tests.convert import to_view
from tests.test_actions_native import build_act_check
from tests.test_predicate_gen_native import compare, run_act_check, run_pred_check
from tests.test_predicates import SHAPES, fits
from tests.test_predicates_native import build_pred_check

pytestmark = pytest.mark.gpu

INV = range(PG.N_INV_PROGRAMS)
ACT = range(PG.N_ACT_PROGRAMS)


@pytest.fixture(scope="module")
def pred_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pg_pred_check_gpu") / "pred_check"
    build_pred_check(exe)
    return str(exe)


@pytest.fixture(scope="module")
def act_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pg_act_check_gpu") / "act_check"
    build_act_check(exe)
    return str(exe)


@pytest.fixture(scope="module")
def host_rows(pred_check, tmp_path_factory):
    """The host VM's verdict rows of invariant program p on the 200 states of a model (cached)."""
    cache = {}
    d = tmp_path_factory.mktemp("pg_host_rows")

    def rows(p, name):
        if (p, name) not in cache:
            m, _ = IC.CASES[name]
            views = d / (name + ".bin")
            if not views.exists():
                with open(views, "wb") as f:
                    for s in PG.states(name):
                        f.write(bytes(to_view(m, s)))
            cache[p, name] = run_pred_check(pred_check, d, PG.program("inv", p), name, str(views), True)
        return cache[p, name]
    return rows


def load_predicates(tmp_path, prog, model, minimal=True, **kw):
    cfg_path, tla = PG.write_program(tmp_path, prog, model, minimal)
    out = rmc.load_model(cfg_path, tla, builtin_raft=True, predicates=not prog.action, actions=prog.action, **kw)
    handle = out[-1] if prog.action else out[2]
    assert handle.names == list(prog.names)
    return handle


def packed_config(m, K):
    return rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, max_term=m.max_term, max_log_len=m.max_log,
                           max_msgs=5 if K == 8 else 4, max_dup=m.max_dup, state_capacity=1 << 12)


@pytest.mark.parametrize("name,K", SHAPES, ids=["%s-K%d" % s for s in SHAPES])
def test_eval_predicates_on_every_packed_shape(name, K, host_rows, tmp_path):
    m, _ = IC.CASES[name]
    keep = [t for t, s in enumerate(PG.states(name)) if len(s.messages) <= K]
    assert len(keep) >= 50
    views = (rmc.StateView * len(keep))(*[to_view(m, PG.states(name)[t]) for t in keep])
    cfg = packed_config(m, K)
    with rmc.Checker(cfg) as ck:
        assert ck.lib.rmc_state_bytes(C.byref(cfg)) == (2 * m.n_servers + K) * 4
        for p in INV:
            ck.set_predicates(load_predicates(tmp_path, PG.program("inv", p), m))
            got = ck.eval_predicates(views)
            assert got == [host_rows(p, name)[t] for t in keep], (name, K, p)
            compare(got, [PG.inv_verdicts(p, name)[t] for t in keep], (name, K, p))


@pytest.mark.parametrize("record", [0, 1, 2])
@pytest.mark.parametrize("name", ["wide_s3", "wide_s5"])
def test_eval_predicates_on_the_three_wide_records(name, record, pred_check, tmp_path, monkeypatch):
    """The first 200 states of the model that fit the record (of all 1,200: few fit the smallest)."""
    monkeypatch.setenv("RMC_WIDE_COMPACT", str(record))
    m, _ = IC.CASES[name]
    states = [s for s in IC.states(name) if fits(s, record)][:PG.N_STATES]
    assert len(states) >= 10, (name, record, len(states))
    views = (rmc.StateView * len(states))(*[to_view(m, s) for s in states])
    with open(tmp_path / "views.bin", "wb") as f:
        f.write(bytes(views))
    cfg = rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, max_term=m.max_term, max_log_len=m.max_log,
                          max_msgs=m.max_msgs, max_dup=m.max_dup, state_capacity=1 << 10)
    with rmc.Checker(cfg) as ck:
        assert ck.lib.rmc_state_bytes(C.byref(cfg)) == {0: 5080, 1: 904, 2: 336}[record]
        for p in INV:
            prog = PG.program("inv", p)
            ck.set_predicates(load_predicates(tmp_path, prog, m))
            got = ck.eval_predicates(views)
            host = run_pred_check(pred_check, tmp_path, prog, name, str(tmp_path / "views.bin"), True, len(states))
            assert got == host, (name, record, p)
            compare(got, prog.verdicts(m.n_servers, states), (name, record, p))


@pytest.mark.parametrize("name,K", AC.SHAPES, ids=["%s-K%d" % s for s in AC.SHAPES])
def test_eval_actions_on_every_packed_shape(name, K, act_check, tmp_path):
    m, _ = IC.CASES[name]
    pairs = [(to_view(m, s), to_view(m, t)) for s, t in PG.pairs(name, K)]
    with rmc.Checker(packed_config(m, K)) as ck:
        for p in ACT:
            prog = PG.program("act", p)
            ck.set_actions(load_predicates(tmp_path, prog, m))
            got = ck.eval_actions(pairs)
            assert got == run_act_check(act_check, tmp_path, prog, name, K, True), (name, K, p)
            compare(got, PG.act_verdicts(p, name, K), (name, K, p))


EDGES = (1, 255, 256, 257, 513)  # threads past n, a second and a third block's own LDS copy, columns 0 and 255


@pytest.mark.parametrize("layout", ["packed", "wide"])
def test_block_edges_give_the_rows_of_the_plain_run(layout, tmp_path, monkeypatch):
    name, K = ("fuzz0", 4) if layout == "packed" else ("wide_s3", 0)
    m, _ = IC.CASES[name]
    if layout == "wide":
        monkeypatch.setenv("RMC_WIDE_COMPACT", "1")
        base = [s for s in PG.states(name) if fits(s, 1)]
        cfg = rmc.make_config(n_servers=m.n_servers, n_values=m.n_values, max_term=m.max_term, max_log_len=m.max_log,
                              max_msgs=m.max_msgs, max_dup=m.max_dup, state_capacity=1 << 10)
    else:
        base = [s for s in PG.states(name) if len(s.messages) <= K]
        cfg = packed_config(m, K)
    assert len(base) >= 20
    base_views = [to_view(m, s) for s in base]
    with rmc.Checker(cfg) as ck:
        for p in (0, 5, 11):
            ck.set_predicates(load_predicates(tmp_path, PG.program("inv", p), m))
            plain = ck.eval_predicates(base_views)
            assert len({row for row in plain}) >= 2  # rows differ, so a row at the wrong place shows
            for n in EDGES:
                views = (rmc.StateView * n)(*[base_views[t % len(base)] for t in range(n)])
                assert ck.eval_predicates(views) == [plain[t % len(base)] for t in range(n)], (layout, p, n)


def test_symmetry_refuses_a_generated_predicate_that_names_a_server(tmp_path):
    m = IC.CASES["fuzz2"][0]
    assert m.n_servers == G.TINY2["n_servers"] == 2
    named = free = None
    for p in INV:
        prog = PG.program("inv", p)
        flags = [PG.names_server(b, prog.helpers) for _nm, b in prog.preds]
        if named is None and any(flags):
            named = (prog, prog.names[flags.index(True)])
        if free is None and not all(flags):
            free = (prog, prog.names[flags.index(False)])
    assert named and free

    def handle(prog, pname):
        cfg_path, tla = PG.write_program(tmp_path, prog, m, True, names=(pname,))
        return rmc.Predicates(cfg_path, tla, builtin_raft=True)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, symmetry=True, **G.TINY2)) as ck:
        with pytest.raises(rmc.RmcError) as e:
            ck.set_predicates(handle(*named))
        assert e.value.code == -22 and "server model value" in str(e.value) and "SYMMETRY" in str(e.value)
        ck.set_predicates(handle(*free))


# ---- the BFS passes: k_pred / k_wpred through first_failing and wslot, k_act's strided successor column
from oracle import raft_spec as R  # noqa: E402
from tests.convert import from_view  # noqa: E402
from tests.test_predicates import check_user_trace  # noqa: E402

BFS_VARIANTS = {"resident": {}, "spill": dict(spill=True, device_window=4096)}


def bfs_program(kind, case):
    """The case's predicate after the predicates of its program that hold everywhere."""
    p, q, depth, verdicts, holders = case
    prog = PG.program(kind, p)
    names = tuple(prog.names[h] for h in holders[:3]) + (prog.names[q],)
    return prog, names, prog.compiled()[q]


@pytest.mark.parametrize("variant", ["resident", "spill", "wide"])
@pytest.mark.parametrize("k", range(4))
def test_bfs_reports_a_generated_invariant(k, variant, tmp_path, monkeypatch):
    cases = PG.bfs_cases("inv")
    assert len(cases) == 4
    if variant == "wide":
        monkeypatch.setenv("RMC_FORCE_WIDE", "1")
    model, _levels = PG.reachable_levels()
    prog, names, fn = bfs_program("inv", cases[k])
    depth, verdicts = cases[k][2], cases[k][3]
    cfg_path, tla = PG.write_program(tmp_path, prog, model, True, names=names)
    preds = rmc.load_model(cfg_path, tla, builtin_raft=True, predicates=True)[2]
    assert preds.names == list(names)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, invariants=0, **G.TINY2,
                                     **BFS_VARIANTS.get(variant, {}))) as ck:
        ck.set_predicates(preds)
        res = ck.run()
        assert res.violated_inv == rmc.INV_USER0 << (len(names) - 1) and not res.deadlock
        assert res.violation_depth == depth and res.depth == depth
        trace = ck.trace()
        last = PG.evaluate(fn, model.n_servers, from_view(trace[-1][2])).verdict
        assert last in verdicts and ck.predicate_error() == (last == PG.ERROR)
        check_user_trace(model, trace, lambda m, s: PG.evaluate(fn, m.n_servers, s).verdict, depth)


@pytest.mark.parametrize("variant", ["resident", "spill"])
@pytest.mark.parametrize("k", range(4))
def test_bfs_reports_a_generated_action_property(k, variant, tmp_path):
    cases = PG.bfs_cases("act")
    assert len(cases) == 4
    model, _levels = PG.reachable_levels()
    prog, names, fn = bfs_program("act", cases[k])
    depth, verdicts = cases[k][2], cases[k][3]
    cfg_path, tla = PG.write_program(tmp_path, prog, model, True, names=names)
    acts = rmc.load_model(cfg_path, tla, builtin_raft=True, actions=True)[-1]
    assert acts.names == list(names)
    with rmc.Checker(rmc.make_config(state_capacity=1 << 16, **G.TINY2, **BFS_VARIANTS[variant])) as ck:
        ck.set_actions(acts)
        res = ck.run()
        assert res.violated_inv == rmc.ACT_USER0 << (len(names) - 1) and res.violation_depth == depth
        trace = ck.trace()
        assert len(trace) == depth
        states = [from_view(v) for _f, _i, v in trace]
        assert states[0] == R.init_state(model)
        for a, b, (fam, _inst, _v) in zip(states, states[1:], trace[1:]):
            assert (rmc.FAMILIES[fam], b) in {(f, t) for f, _p, t in R.successors(model, a)}
        steps = [PG.evaluate(fn, model.n_servers, a, b).verdict for a, b in zip(states, states[1:])]
        assert steps[-1] in verdicts and all(v == PG.HOLDS for v in steps[:-1])
        hit = ck.action_violation()
        assert hit["property"] == len(names) - 1 and hit["is_error"] == (steps[-1] == PG.ERROR)
        assert (hit["family"], hit["instance"]) == (trace[-1][0], trace[-1][1])


def test_symmetry_counts_are_those_of_the_run_without_predicates(tmp_path):
    """Predicates that name no server model value and hold on every reachable state, under SYMMETRY."""
    model, _levels = PG.reachable_levels()
    chosen = None
    for p, _q, _d, _v, holders in PG.bfs_cases("inv"):
        prog = PG.program("inv", p)
        free = tuple(prog.names[h] for h in holders if not PG.names_server(prog.preds[h][1], prog.helpers))
        if free:
            chosen = (prog, free)
            break
    assert chosen, "no program with a predicate that holds everywhere and names no server"
    cfg_path, tla = PG.write_program(tmp_path, chosen[0], model, True, names=chosen[1])
    preds = rmc.Predicates(cfg_path, tla, builtin_raft=True)
    out = []
    for with_preds in (False, True):
        with rmc.Checker(rmc.make_config(state_capacity=1 << 16, symmetry=True, **G.TINY2)) as ck:
            if with_preds:
                ck.set_predicates(preds)
            res = ck.run()
            out.append((res.distinct, res.generated, res.depth, res.violated_inv, res.left_on_queue))
    ref = R.bfs(model, invariants=(), symmetry=True)
    assert out[0] == out[1] and out[0][3] == 0 and out[0][:3] == (ref.distinct, ref.generated, ref.depth)
