"""Host-side checks of the wide layout's full-state verification (no GPU): the
state equality the kernels compare with (raft_wide.h wsame), the HBM division
of a verifying ctx (rmc_wide_plan.h), both compiled for the host with g++, and
what rmc_create accepts and refuses before it looks for a device."""
import ctypes as C
import os
import subprocess

import rmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I",
                    os.path.join(ROOT, "raft.tla_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", name + ".cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_wsame_equals_across_records_and_sees_every_field(tmp_path):
    """Random walks from Init (S = 3, |Value| = 2, nothing bounded, 300 walks of
    up to 14 states): a state narrowed into the 904-B or 336-B record equals
    its 5,080-B original, and a change of any one semantic field — server
    scalars, log entries and lengths, vote sets, nextIndex / matchIndex, message
    fields, counts, a message removed or added — makes them differ."""
    r = subprocess.run([build(tmp_path, "wide_same_check"), "300", "14", "7"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 100000


def test_verifying_ctx_plan_keeps_depth_14_resident(tmp_path):
    """With state_capacity = 0 on a 288-GB device, 16 B per set slot and the
    deferred-hit buffer leave room for the 499.4 M 336-B records of MCraft.cfg
    as shipped at depth 14, at two set slots per state or more; the plan
    without the flag is unchanged and every plan stays within its budget."""
    r = subprocess.run([build(tmp_path, "wide_plan_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout


def test_create_accepts_verification_on_the_wide_layout_and_refuses_it_with_spill():
    """max_log_len = 4 is beyond the packed capacity: a wide ctx.  With
    RMC_FLAG_VERIFY_STATES the config is valid (rmc_create goes on to look for a
    device: 0 with one, RMC_E_NOGPU without); with RMC_FLAG_SPILL too it is
    RMC_E_INVAL."""
    lib = rmc.native()
    ctx = C.c_void_p()
    ok = rmc.make_config(max_log_len=4, verify_states=True, state_capacity=1 << 16)
    rc = lib.rmc_create(C.byref(ok), C.byref(ctx))
    assert rc in (0, -19)
    if rc == 0:
        lib.rmc_destroy(ctx)
    bad = rmc.make_config(max_log_len=4, verify_states=True, spill=True)
    assert lib.rmc_create(C.byref(bad), C.byref(ctx)) == -22
