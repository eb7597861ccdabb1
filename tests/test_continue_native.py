"""Host-side check of the violation classifiers (raft.tla_amd/csrc/rmc_viol.h, compiled
for the host with g++; no GPU): tests/native/viol_check.cpp searches past violations
with the packed lane code and again with the wide lane code, classifies every stored
state through the functions the kernels k_violations / k_wviolations call, and must
find the two layouts and the oracle's recorded tallies
(tests/golden/continue_cases.json) equal."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "continue_cases.json")))
KEYS = ("n_servers", "n_values", "max_term", "max_log_len", "max_msgs", "max_dup", "bug_quorum", "max_depth",
        "invariants")


def build(exe, flags):
    subprocess.run(["g++", "-std=c++17", "-fno-strict-aliasing", "-Wno-unknown-pragmas"] + flags +
                   ["-I", os.path.join(ROOT, "raft.tla_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "viol_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def viol_check(tmp_path_factory):
    return build(tmp_path_factory.mktemp("viol_check") / "viol_check", ["-O2"])


def test_classifiers_under_sanitizers(tmp_path):
    """The stand-alone program itself under ASan + UBSan (host code only, the runtimes
    linked into the program) on row 1: a read past a bag slot or a record, or a
    shift out of range in either classifier, would stop it."""
    exe = build(tmp_path / "viol_check_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"])
    g = GOLDEN["bug_small_d12"]
    r = subprocess.run([exe] + [str(g["params"][k]) for k in KEYS], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(r.stdout)
    assert rec["same"] and rec["packed"]["each"] == rec["wide"]["each"] == g["each"]


@pytest.mark.parametrize("case", ["bug_small_d12", "bug_s2_msgs2_full", "small_d15", "tiny2_full"])
def test_classifiers_agree_across_layouts_and_with_the_oracle(case, viol_check):
    """The K = 4 cases without SYMMETRY: rows 1 and 3 (first != each), the unmodified
    spec's MessagesInv violations at depth 14, and a model that violates nothing."""
    g = GOLDEN[case]
    assert not g["params"]["symmetry"]
    r = subprocess.run([viol_check] + [str(g["params"][k]) for k in KEYS], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rec = json.loads(r.stdout)
    assert rec["same"]
    for layout in ("packed", "wide"):
        got = rec[layout]
        assert got["misclassified"] == 0
        assert {k: got[k] for k in ("distinct", "generated", "depth", "states", "first", "each", "inv_depth")} == {
            k: g[k] for k in ("distinct", "generated", "depth", "states", "first", "each", "inv_depth")}, layout
