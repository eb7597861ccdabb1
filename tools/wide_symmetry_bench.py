#!/usr/bin/env python3
"""One depth-bounded run of the reference's MCraft.cfg layout on the wide layout, with or
without SYMMETRY Permutations(Server) (tests/golden/models/MCunboundedSym.cfg /
MCunbounded.cfg), configured as rmc-tlc configures it (RMC_FLAG_SPILL unless --nospill),
and one JSON line with the counts, the wall time, the expansion kernels' device time and
the store's record.  One run per process: start it once per configuration.

    python tools/wide_symmetry_bench.py --depth 14 --symmetry --capacity 120000000
    python tools/wide_symmetry_bench.py --depth 14 --capacity 520000000
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "raft.tla_amd")]

import rmc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, required=True)
    ap.add_argument("--symmetry", action="store_true")
    ap.add_argument("--capacity", type=int, required=True, help="states the set and the links are sized for")
    ap.add_argument("--nospill", action="store_true", help="every record resident (rmc-tlc -nospill)")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0, help="fingerprint salt (rmc-tlc -fpseed)")
    a = ap.parse_args()
    name = "MCunboundedSym.cfg" if a.symmetry else "MCunbounded.cfg"
    c, _, _ = rmc.model_from_files(os.path.join(ROOT, "tests", "golden", "models", name), builtin_raft=True,
                                   depth_bounded=True)
    c.max_depth = a.depth
    c.state_capacity = a.capacity
    c.seed = a.seed
    if not a.nospill:
        c.flags |= rmc.FLAG_SPILL
        c.device_window = a.window
    out = dict(model=name, depth=a.depth, symmetry=bool(c.flags & rmc.FLAG_SYMMETRY), spill=not a.nospill,
               capacity=a.capacity, seed=a.seed, record_bytes=rmc.native().rmc_state_bytes(c))
    try:
        with rmc.Checker(c) as ck:
            r = ck.run(record_levels=True)
            levels = [1] + [lv[3] for lv in ck.levels if lv[3]]
        out.update(distinct=r.distinct, generated=r.generated, left_on_queue=r.left_on_queue, reached=r.depth,
                   seconds=round(r.seconds, 4), expand_kernel_seconds=round(r.expand_kernel_seconds, 4),
                   launches=r.expand_launches, spills=r.spills, spilled=r.spilled, set_slots=r.set_slots, levels=levels)
    except rmc.RmcError as e:
        out.update(error=str(e), code=e.code)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
