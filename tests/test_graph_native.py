"""The host-only parts of the state graph export (no GPU): rmc-tlc -dump's writers
(raft.tla_amd/csrc/rmc_dump.cpp, compiled for the host with g++ into
tests/native/dump_check.cpp) on a hand-made five-node graph, against the text written
out here; the CLI's refusals by name, which come before any device is opened; and the
NULL-argument refusals of the four C entry points."""
import ctypes as C
import os
import subprocess

import pytest

import rmc
from tests import graph_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")
CLI = os.path.join(ROOT, "raft.tla_amd", "bin", "rmc-tlc")
TINY2_TLA = os.path.join(ROOT, "specs", "MCraftTiny2.tla")

HEAD = 'strict digraph DiskGraph {\nnodesep=0.35;\nsubgraph cluster_graph {\ncolor="white";\n'
NODES = ('42 [label="/\\\\ x = 0\\n/\\\\ y = \\"a\\"",style = filled]\n'
         '-1 [label="/\\\\ x = 2"];\n'
         '7 [label="/\\\\ x = 1"];\n'
         '-9223372036854775808 [label="/\\\\ x = 3"];\n'
         '5 [label="/\\\\ x = 4"];\n')
# (source id, destination id, family, instance) order; ids compare as signed numbers
EDGES = [("-1", "-1", "Receive"), ("-1", "5", "DropMessage"),
         ("7", "-9223372036854775808", "Timeout"), ("7", "-9223372036854775808", "RequestVote"),
         ("7", "-9223372036854775808", "RequestVote"),
         ("42", "-1", "Restart"), ("42", "7", "Timeout"), ("42", "42", "DuplicateMessage")]
RANKS = "{rank = same; 42;}\n{rank = same; -1;7;}\n{rank = same; -9223372036854775808;5;}\n"
TAIL = "}\n}\n"


def build(exe, flags):
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "dump_check.cpp"),
                                                             os.path.join(CSRC, "rmc_dump.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def dump_check(tmp_path_factory):
    return build(tmp_path_factory.mktemp("dump_check") / "dump_check", ["-O2"])


def run(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_dot_writer_with_action_labels(dump_check):
    want = HEAD + NODES + "".join(f'{a} -> {b} [label="{f}"];\n' for a, b, f in EDGES) + RANKS + TAIL
    got = run(dump_check, "dotlabels")
    assert got == want
    d = G.read_dot(got)  # and the tests' own reader reads it back
    assert d.initial == {42} and sorted(d.nodes) == [-(1 << 63), -1, 5, 7, 42]
    assert d.edges == [(int(a), int(b), f) for a, b, f in EDGES]
    assert d.ranks == [[42], [-1, 7], [-(1 << 63), 5]]
    assert d.nodes[42] == '/\\\\ x = 0\\n/\\\\ y = \\"a\\"'


def test_dot_writer_without_labels(dump_check):
    assert run(dump_check, "dot") == HEAD + NODES + "".join(f"{a} -> {b};\n" for a, b, _f in EDGES) + RANKS + TAIL


def test_plain_writer(dump_check):
    assert run(dump_check, "states") == ('State 1:\n/\\ x = 0\n/\\ y = "a"\n\nState 2:\n/\\ x = 1\n\nState 3:\n/\\ x = 2\n\n'
                                         "State 4:\n/\\ x = 3\n\nState 5:\n/\\ x = 4\n\n")


def test_dot_writer_refuses_an_edge_to_no_node(dump_check):
    assert run(dump_check, "badedge") == ""


def test_writers_under_sanitizers(tmp_path):
    """The stand-alone program under ASan + UBSan (host code only, the runtimes linked
    into the program): the sorts and the label escaping on every mode."""
    exe = build(tmp_path / "dump_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                              "-static-libasan", "-static-libubsan"])
    for mode in ("dot", "dotlabels", "states", "badedge"):
        run(exe, mode)


@pytest.mark.parametrize("args, named", [
    (["-dump", "dot,colorize", "FILE"], "colorize"),
    (["-dump", "dot,actionlabels,snapshot", "FILE"], "snapshot"),
    (["-gpus", "2", "-dump", "FILE"], "-gpus N > 1"),
    (["-dump", "dot", "FILE", "-simulate"], "-simulate"),
    (["-recover", "ckpt", "-dump", "dot,actionlabels", "FILE"], "-recover"),
])
def test_cli_refuses_by_name_before_any_device(args, named, tmp_path):
    out = tmp_path / "graph.out"
    r = subprocess.run([CLI] + [str(out) if a == "FILE" else a for a in args] + [TINY2_TLA], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    assert "-dump" in r.stderr and named in r.stderr.split("usage:")[0], r.stderr
    assert "Computing initial states" not in r.stdout and not out.exists()


def test_null_arguments_are_invalid():
    lib = rmc.native()
    n = C.c_size_t(7)
    assert lib.rmc_get_levels(None, None, 0, C.byref(n)) == -22
    assert lib.rmc_read_states(None, 0, 0, None, None) == -22
    assert lib.rmc_find_states(None, None, 0, None) == -22
    assert lib.rmc_graph_edges(None, 0, 0, None, 0, C.byref(n)) == -22
    assert C.sizeof(rmc.Edge) == 24 and rmc.NO_STATE == 2 ** 64 - 1
    assert b"null context" in lib.rmc_last_error(None)
