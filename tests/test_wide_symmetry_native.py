"""The wide layout's SYMMETRY keys and orbit comparison against the oracle's orbits,
state by state, on the host (no GPU): tests/native/wide_canon_check.cpp and
rmc_codec.cpp compiled with plain g++ and no ROCm include path.  The states are those
of the GPU test (tests/test_wide_symmetry.py): (a) every case of
tests/symmetry_cases.py encoded as wide records, (b) per S states past the packed
capacity from random walks, tie-heavy states on wide bounds and their twins
(tests/wide_symmetry_cases.py), all with permuted copies.  A wrong wcanon, wcanon_succ
or wsame_orbit fails here; one right here and wrong on the device is a code generation
problem."""
import os
import re
import subprocess

import pytest

from tests import symmetry_cases as SC
from tests import wide_symmetry_cases as WC
from tests.test_symmetry_native import write_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")


def build_wide_canon_check(exe, extra=()):
    # as librmc's rmc_codec.o is built (raft_wide.h compares records as 64-bit words): -fno-strict-aliasing
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", *extra, "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "wide_canon_check.cpp"),
                    os.path.join(CSRC, "rmc_codec.cpp"), "-o", str(exe)], check=True)


@pytest.fixture(scope="module")
def wide_canon_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wide_canon_check") / "wide_canon_check"
    build_wide_canon_check(exe)
    return str(exe)


def inputs_of(name):
    """(model, states, orbit numbers) of a case of either module."""
    if name in SC.CASES:
        return (SC.CASES[name],) + SC.states_and_orbits(name)
    return (WC.model_of(name),) + WC.states_and_orbits(name)


def run_case(exe, tmp_path, name):
    m, states, orbits = inputs_of(name)
    views, ids = write_case(tmp_path, m, states, orbits)
    r = subprocess.run([exe, views, ids, str(m.n_servers), str(m.n_values)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok "), r.stdout
    got = re.fullmatch(r"shape wide S=(\d+) (\d+) tied (\d+) successors (\d+) tied (\d+) orbits (\d+) narrow (\d+) (\d+)", lines[0])
    assert got, r.stdout
    S, n, tied, succ, succ_tied, n_orbits, narrow_c, narrow_d = map(int, got.groups())
    assert (S, n) == (m.n_servers, len(states)), r.stdout
    assert n_orbits == len(set(orbits))
    # the engine's signature ties wherever the oracle's summaries do (it may tie more often)
    assert tied >= sum(1 for s in states if SC.ties(m, s))
    # both branches of wcanon_based on the expansion's path
    assert succ_tied >= 50 and succ - succ_tied >= 50, r.stdout
    assert int(lines[-1].split()[1]) >= 3 * succ + 2 * n * n
    return narrow_c, narrow_d


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_host_wide_keys_partition_the_packed_size_cases_into_the_oracles_orbits(name, wide_canon_check, tmp_path):
    """(a) wcanon on the base states, copies and twins of every case of
    tests/symmetry_cases.py as wide records: one key (k and s) exactly when the oracle
    puts two states in one orbit, surviving twins included; wsame_orbit is the oracle's
    orbit equality over all pairs; wcanon_succ on every successor is wcanon of it (the
    program compares; its exit code is the verdict)."""
    SC.check_not_vacuous(name)
    WC.check_packed_case_not_vacuous(name)
    narrow_c, narrow_d = run_case(wide_canon_check, tmp_path, name)
    assert narrow_c > 0 and narrow_d > 0  # the compact and depth-sized records are compared too


@pytest.mark.parametrize("name", WC.CASES)
def test_host_wide_keys_partition_states_beyond_the_packed_capacity(name, wide_canon_check, tmp_path):
    """(b) the same on states past the packed capacity (random walks of the
    unconstrained spec), tie-heavy states on wide bounds, their copies and twins."""
    WC.check_not_vacuous(name)
    run_case(wide_canon_check, tmp_path, name)


@pytest.mark.parametrize("name", WC.CASES)
def test_wide_inputs_are_not_vacuous(name):
    """More than 30 states past the packed capacity, at least 50 orbits with two or more
    distinct members, tied servers that no automorphism swaps, twins that left their
    orbit (tests/wide_symmetry_cases.py check_not_vacuous, from the oracle alone)."""
    f = WC.check_not_vacuous(name)
    kept, _ = WC.twins(name)
    m = WC.model_of(name)
    for b, tw in kept:  # a surviving twin is in another orbit than its original
        assert SC.orbit_key(m, tw) != SC.orbit_key(m, WC.bases(name)[b])
    assert f["base"] >= 100
