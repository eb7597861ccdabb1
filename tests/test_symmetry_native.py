"""The SYMMETRY canonical keys against the oracle's orbits, state by state, on the
host (no GPU): tests/native/canon_check.cpp and rmc_codec.cpp compiled with plain
g++ and no ROCm include path.  The states are those of the GPU test
(tests/test_symmetry.py): per model uniform and tie-heavy base states, their
permuted copies and their twins (tests/symmetry_cases.py).  A wrong canon_state or
canon_delta fails here; one right here and wrong on the device is a code generation
problem."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import pytest

import rmc
from tests import symmetry_cases as SC
from tests.convert import to_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")


def build_canon_check(exe, extra=(), csrc=CSRC):
    # as librmc's rmc_codec.o is built (raft_wide.h compares records as 64-bit words): -fno-strict-aliasing
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", *extra, "-I", csrc,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "canon_check.cpp"),
                    os.path.join(CSRC, "rmc_codec.cpp"), "-o", str(exe)], check=True)


@pytest.fixture(scope="module")
def canon_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("canon_check") / "canon_check"
    build_canon_check(exe)
    return str(exe)


def write_case(tmp_path, model, states, orbits):
    views, ids = tmp_path / "views.bin", tmp_path / "orbits.bin"
    with open(views, "wb") as f:
        for s in states:
            f.write(bytes(to_view(model, s)))
    ids.write_bytes(struct.pack("<%dI" % len(orbits), *orbits))
    assert os.path.getsize(views) == len(states) * C.sizeof(rmc.StateView)
    return str(views), str(ids)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_host_keys_partition_the_states_into_the_oracles_orbits(name, canon_check, tmp_path):
    """canon_state<S, K> of the model's shape on its base states, copies and twins:
    two states have one key (k and s) exactly when the oracle puts them in one
    orbit; and on every in-model successor of every one of them canon_delta equals
    canon_state of the materialised successor, with and without NOTIE (the program
    compares; its exit code is the verdict)."""
    SC.check_not_vacuous(name)
    m = SC.CASES[name]
    states, orbits = SC.states_and_orbits(name)
    views, ids = write_case(tmp_path, m, states, orbits)
    r = subprocess.run([canon_check, views, ids, str(m.n_servers), str(m.n_values), str(SC.kcap(m)), str(m.max_term),
                        str(m.max_log), str(m.max_msgs), str(m.max_dup)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok "), r.stdout
    got = re.fullmatch(r"shape packed S=(\d+) K=(\d+) (\d+) tied (\d+) successors (\d+) tied (\d+) orbits (\d+)", lines[0])
    assert got, r.stdout
    S, K, n, tied, succ, succ_tied, n_orbits = map(int, got.groups())
    assert (S, K, n) == (m.n_servers, SC.kcap(m), len(states)), r.stdout
    assert n_orbits == len(set(orbits))
    # the engine's signature ties wherever the oracle's summaries do (it may tie more often)
    assert tied >= sum(1 for s in states if SC.ties(m, s))
    # both branches of canon_sorted on the incremental path, the deferred one (NOTIE) included
    assert succ_tied >= 50 and succ - succ_tied >= 50, r.stdout
    assert int(lines[-1].split()[1]) >= 3 * succ + n * n


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_states_tie_without_being_symmetric(name):
    """The inputs are not vacuous (tests/symmetry_cases.py check_not_vacuous, from
    the oracle alone)."""
    SC.check_not_vacuous(name)


def test_generated_states_keep_their_key_under_every_permutation(canon_check):
    """No oracle: per shape (S = 2..5, bags of 4 and of 8 slots) 20,000 packed
    states (2,000 at S = 5), every second one tie-heavy, each permuted by all S!
    server permutations written on the decoded fields; every image has the state's
    key.  At least a quarter of each shape's tie-heavy states tie.  On a quarter
    of the states every single bit of a field that is no server id is flipped in
    turn, which takes the state out of its orbit: the key must change (a key that
    ignores a field merges orbits without ever splitting one)."""
    r = subprocess.run([canon_check, "gen", "20000", "2000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok "), r.stdout
    seen = {}
    for ln in lines[:-1]:
        got = re.fullmatch(r"shape packed S=(\d) K=(\d) (\d+) tied (\d+) of (\d+) tie-heavy, (\d+) of (\d+) uniform", ln)
        assert got, ln
        S, K, n, tied, heavy, _tu, _u = map(int, got.groups())
        assert n >= (2000 if S == 5 else 20000) and 2 * heavy == n, ln
        assert 4 * tied >= heavy, ln
        seen[(S, K)] = n
    assert set(seen) == {(S, K) for S in (2, 3, 4, 5) for K in (4, 8)}, r.stdout
    images = sum(n * math.factorial(S) for (S, _K), n in seen.items())
    # and per checked state (a quarter of them) at least the eight term, role and commitIndex bits of every server
    assert int(lines[-1].split()[1]) >= images + sum(n // 4 * 8 * S for (S, _K), n in seen.items())
