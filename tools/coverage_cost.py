"""What action coverage (RMC_FLAG_COVERAGE) costs on a bench model (measurement
tool): python tools/coverage_cost.py specs/X.cfg on|off [runs]
One ctx sized like bench.py's (MCraftBench.cfg resident, MCraftBenchXL.cfg in
its ring window), one warm-up run, then `runs` timed ones; prints one JSON
line: wall time and expand_kernel_seconds per run (with the flag the level's
event bracket holds the coverage passes and their count read-backs too), the
launches, and with the flag the rows.  Run it alternately with `off` and `on`
in one session to compare."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raft.tla_amd"))
import rmc  # noqa: E402

cfg_path, on = sys.argv[1], sys.argv[2] == "on"
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
cfg = rmc.config_from_files(cfg_path, builtin_raft=True)
xl = os.path.basename(cfg_path) == "MCraftBenchXL.cfg"
cfg.state_capacity = int(4.14e9) if xl else int(1.5e9)
if xl:
    cfg.flags |= rmc.FLAG_SPILL
if on:
    cfg.flags |= rmc.FLAG_COVERAGE
wall, kern = [], []
with rmc.Checker(cfg) as ck:
    ck.run(record_levels=False)  # the ctx's first run clears the set
    for _ in range(runs):
        r = ck.run(record_levels=False)
        wall.append(r.seconds)
        kern.append(r.expand_kernel_seconds)
    rows = ck.coverage() if on else None
out = {"cfg": os.path.basename(cfg_path), "coverage": on, "runs": runs, "seconds_median": statistics.median(wall),
       "kernel_seconds_median": statistics.median(kern), "seconds": wall, "kernel_seconds": kern,
       "distinct": r.distinct, "generated": r.generated, "depth": r.depth, "launches": r.expand_launches}
if rows:
    out["rows"] = {a: {"generated": g, "distinct": d} for a, (g, d) in rows.items()}
    out["sums_ok"] = (sum(g for g, _ in rows.values()) == r.generated and
                      sum(d for _, d in rows.values()) == r.distinct)
print(json.dumps(out))
