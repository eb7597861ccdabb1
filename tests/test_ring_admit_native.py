"""Host model of the ring window's device-side admission (rmc_plan.h admit_*: what
rmc_run_bfs sizes DevBufs.lim and DevBufs.admit_reserve by; rmc_units.h kStopBit: what
flush_new raises and expand_body's claim obeys), compiled for the host with g++ (no GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ring_admit_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_admission_keeps_the_ring_and_claims_every_unit_once(tmp_path, flags):
    """W in {1, 4, 64} waves, units of 64 and 512 states, bounds 30 and 52, per-state
    yields all 0 / all `bound` / uniform / sparse (the bound once in `bound` states),
    windows from "the reserve does not fit" to "never stops", three random
    interleavings each in which other waves claim between a flush that takes the count
    past the stop and its raise of the stop bit, and lists of up to WCAP entries are
    carried into a unit: the count never passes
    live_lo + window, every unit is claimed exactly once over the re-launches, the
    live_lo taken from wnext passes no unfinished state, a re-launch progresses or
    ends in the too-small verdict.  The same program also runs built with the
    address and undefined-behaviour sanitizers."""
    exe = tmp_path / "ring_admit_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "raft.tla_amd", "csrc"), SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.splitlines()[-1]
    assert last.startswith("ok 1152 cases, "), r.stdout
    assert " 288 reserve does not fit" in last, r.stdout
