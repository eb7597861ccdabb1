"""The invariant predicates of both layouts against the oracle, state by state,
on the host (no GPU): tests/native/inv_check.cpp and rmc_codec.cpp compiled with
plain g++ and no ROCm include path.  The states are those of the GPU test
(tests/test_invariants.py): per model the uniform family and near_invariant_state,
plus the TypeOK cases.  A wrong predicate fails here; a predicate right here and
wrong on the device is a code generation problem."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import rmc
from tests import invariant_cases as IC
from tests.convert import to_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")


def build_inv_check(exe, extra=()):
    # as librmc's rmc_codec.o is built (raft_wide.h compares records as 64-bit words): -fno-strict-aliasing
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", *extra, "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "inv_check.cpp"),
                    os.path.join(CSRC, "rmc_codec.cpp"), "-o", str(exe)], check=True)


@pytest.fixture(scope="module")
def inv_check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("inv_check") / "inv_check"
    build_inv_check(exe)
    return str(exe)


def write_case(tmp_path, model, states, bits):
    views, verdicts = tmp_path / "views.bin", tmp_path / "verdicts.bin"
    with open(views, "wb") as f:
        for s in states:
            f.write(bytes(to_view(model, s)))
    verdicts.write_bytes(struct.pack("<%dI" % len(bits), *bits))
    assert os.path.getsize(views) == len(states) * C.sizeof(rmc.StateView)
    return str(views), str(verdicts)


def run_case(exe, tmp_path, model, states, bits, packable):
    views, verdicts = write_case(tmp_path, model, states, bits)
    k = IC.kcap(model) if packable else 0
    r = subprocess.run([exe, views, verdicts, str(model.n_servers), str(model.n_values), str(k)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok ") and int(lines[-1].split()[1]) >= 11 * len(states), r.stdout
    shapes = {ln.rsplit(" ", 1)[0]: int(ln.rsplit(" ", 1)[1]) for ln in lines if ln.startswith("shape ")}
    sv = "S=%d V=%d" % (model.n_servers, model.n_values)
    want = {"shape wide full " + sv, "shape wide compact " + sv}
    if packable:
        want.add("shape packed S=%d K=%d V=%d" % (model.n_servers, k, model.n_values))
    assert set(shapes) == want, r.stdout
    assert all(n > 0 for n in shapes.values()), r.stdout
    assert all(n == len(states) for name, n in shapes.items() if "compact" not in name), r.stdout
    return shapes


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_host_predicates_equal_the_oracle_state_by_state(name, inv_check, tmp_path):
    """check_invariants<S, K> of the model's packed shape and wcheck_invariants on
    the full and the compact wide record, on the model's 1,200 states: each
    invariant alone is violated exactly where the oracle says, all ten together
    name the oracle's lowest violated one, and the single-bit results agree with
    the full-mask result (the program compares; its exit code is the verdict)."""
    m, _ = IC.CASES[name]
    shapes = run_case(inv_check, tmp_path, m, IC.states(name), IC.verdicts(name), packable=not name.startswith("wide"))
    if name != "wide_s5":  # (its bags of up to 64 messages and logs of up to 32 leave few states to the compact record)
        assert shapes["shape wide compact S=%d V=%d" % (m.n_servers, m.n_values)] >= IC.N_PER_FAMILY // 2


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_states_show_both_verdicts_of_every_invariant(name):
    """The inputs are not vacuous (computed from the oracle alone): for every named
    invariant at least 10 of the model's states satisfy it and at least 10 violate
    it, except the pairs of ONE_SIDED, where one verdict is impossible."""
    IC.check_mixed_verdicts(name)


@pytest.mark.parametrize("name", sorted(IC.TYPEOK))
def test_host_typeok_sees_entry_values_outside_value(name, inv_check, tmp_path):
    """|Value| = 1 and an entry of value 1 in a server's log, in an
    AppendEntriesRequest's mentries, in a RequestVoteResponse's mlog: TypeOK is
    violated (and reported first) on every layout, and holds once the value is 0."""
    m = IC.TYPEOK[name]
    states, bits = [], []
    for _place, bad, good in IC.typeok_states(name):
        for s in (bad, good):
            states.append(s)
            bits.append(IC.oracle_bits(m, s))
        assert bits[-2] & 1 and not bits[-1] & 1
    run_case(inv_check, tmp_path, m, states, bits, packable=name != "typeok_wide")
