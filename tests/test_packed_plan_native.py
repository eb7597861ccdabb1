"""Host-side check of the packed layout's HBM division (rmc_plan.h packed_plan,
what rmc_create allocates by) and of the ring window's launch bound, compiled
for the host with g++ (no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "golden", "packed_plan_cases.txt")


def test_packed_plan_matches_the_recorded_sizing_and_keeps_its_invariants(tmp_path):
    """tests/golden/packed_plan_cases.txt holds what rmc_create's inline sizing
    gave, before it became packed_plan, over 648 cases: 10 and 18 state words x
    verification x {resident, spill, spill with host links} x budgets of 2 GB
    and 230.4 GB x given and derived state_capacity, set and device_window.
    packed_plan must give the same capacity, slots, window, link capacity,
    device-links decision and "capacity exceeds the set" outcome for every one.
    Every plan has a power-of-two set of at least two slots per state, a window
    of at most the capacity, a power-of-two ring and links for every state with
    device links (links for the window without), and stays within its budget
    unless a given value or a 1024 floor binds.  MCraftBenchXL's shape on a
    288-GB device gets device links and a power-of-two ring; new_states_bound
    is 30 for S = 3, V = 2, K = 4 and 64 for S = 5, V = 1, K = 8, and the packed
    bound never exceeds the lane count."""
    exe = tmp_path / "packed_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "raft.tla_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "packed_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), CASES], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].startswith("XL: ") and " dev_links 1 " in lines[0], r.stdout
    assert lines[-1].startswith("ok 648 cases "), r.stdout
