"""Host-side check of the sharded BFS's round arithmetic (rmc_dist_plan.h: the
count row, the byte blocks of the three all-to-alls, the round sizing) and of
the set-epoch decision (rmc_plan.h next_set_epoch), compiled for the host with
g++ (no HIP, no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_rank_plans_the_same_exchange_and_rounds_size_as_before(tmp_path):
    """tests/native/dist_plan_check.cpp plays worlds of 1, 2, 3, 8 and 64 ranks
    on the host, 12 rounds each, with key counts from a fixed seed (zeros, full
    outboxes, a rank that sends nothing, a round in which nobody sends).  Every
    rank decodes its own count row, and: the bytes a plans to send b are the
    bytes b plans to receive from a, for keys, replies (the reverse) and states;
    receive offsets are the prefix sums in rank order; every block ends inside
    its buffer of W * kcap records; tot_in and tot_st are the sums; no rank
    sends itself states; a verifying rank receives a state per key; a full
    parking buffer on one rank is seen by all; novf is clamped to the buffer
    and newly_parked never goes below zero.  Round sizing over frontier x rho x
    fill x split x kcap: the rounds sum to the frontier, none exceeds its cap,
    a level of 2^21 states or more takes at least `split` rounds, rounds differ
    by at most one state, and each equals the level loop's expression from
    before the split into functions.  next_set_epoch equals the `if` it
    replaced over epoch 0..255 x ep_max {0, 1, 2, 255} x tagged, never exceeds
    ep_max, and clears whenever it returns 0 or 1."""
    exe = tmp_path / "dist_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "raft.tla_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "dist_plan_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith("ok 60 exchange rounds over 5 worlds, 288 levels "), r.stdout
