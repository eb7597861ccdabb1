"""A/B bench of alternative librmc.so builds on one GPU box (measurement tool,
not shipped).  Copy the builds to abtest/librmc_<name>.so (git-ignored .so),
then `bash tools/ab_bench.sh` under gpurun runs bench.py against each in turn.

    python tools/ab_bench.py librmc_old.so [bench.py arguments]
    RMC_LIB=librmc_old.so python tools/ab_bench.py - [bench.py arguments]

"-" keeps the library the binding chose (RMC_LIB: a build under
raft.tla_amd/lib/); arguments after the library replace the default ones.
"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "raft.tla_amd"))
import rmc  # noqa: E402

if sys.argv[1] != "-":
    rmc.LIB_PATH = os.path.join(ROOT, "abtest", sys.argv[1])
sys.argv = ["bench.py"] + (sys.argv[2:] or ["--full", "--no-cpu", "--no-probe-ceiling", "--steps", "5", "--warmup", "1"])
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
