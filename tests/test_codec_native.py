"""Host-side check of the codecs between rmc_state_view and the two state
layouts (rmc_codec.h), no GPU: tests/native/codec_check.cpp and rmc_codec.cpp
compiled together with plain g++ and no ROCm include path — the codec unit is
host arithmetic only — and run against the kernels' own lane code."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raft.tla_amd", "csrc")


def test_codecs_round_trip_the_kernels_states(tmp_path):
    """Random walks from Init with the kernels' lane code (1,500 walks of 60
    steps for each packed shape S = 2..5, K in {4, 8}, |Value| in {1, 2}; 300
    walks of 14 steps on the wide record for S in {2, 3, 5}, nothing bounded):
    every visited state decodes to a view that encodes back to the same 2S + K
    words (the same wide record under wsame), n_msgs is the number of bag slots
    in use, the encoded bag is sorted descending, a state the compact records
    hold decodes from them to the same view, and a view with any one bounded
    field a step past its packed range, or a message twice, is refused with a
    reason."""
    exe = tmp_path / "codec_check"
    # as librmc's rmc_codec.o is built (raft_wide.h compares records as 64-bit words): -fno-strict-aliasing
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fno-strict-aliasing", "-I", CSRC,
                    "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "codec_check.cpp"), os.path.join(CSRC, "rmc_codec.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "1500", "60", "300", "14", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok ") and int(lines[-1].split()[1]) > 0, r.stdout
    shapes = {ln.rsplit(" ", 1)[0]: int(ln.rsplit(" ", 1)[1]) for ln in lines if ln.startswith("shape ")}
    want = {f"shape packed S={s} K={k} V={v}" for s in (2, 3, 4, 5) for k in (4, 8) for v in (1, 2)}
    want |= {f"shape wide S={s}" for s in (2, 3, 5)}
    assert set(shapes) == want, r.stdout
    assert all(n > 0 for n in shapes.values()), r.stdout


def test_codec_unit_includes_no_hip():
    """rmc_codec.h / .cpp include only rmc.h, the two layout headers and the
    standard library."""
    for name in ("rmc_codec.h", "rmc_codec.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            incs = re.findall(r'#include\s+[<"]([^>"]+)[>"]', f.read())
        local = [i for i in incs if "/" in i or i.endswith(".h")]
        assert set(local) <= {"../../include/rmc.h", "raft_packed.h", "raft_wide.h", "rmc_codec.h"}, (name, local)
