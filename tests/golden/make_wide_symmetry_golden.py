"""Writes tests/golden/wide_symmetry_levels.json: the reference's own MCraft.cfg layout
(no CONSTRAINT) with SYMMETRY Permutations(Server) — tests/golden/models/MCunboundedSym.cfg
— under a depth bound of 12, from the C oracle's wide build (liboracle_wide.so: logs of 8
entries and 12 messages, which never bind within 11 steps; terms and counts unbounded).
One state per orbit is stored and expanded, so level_new counts orbits.

    python tests/golden/make_wide_symmetry_golden.py     (about 10 s on 16 threads)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import oracle_c  # noqa: E402

# S, V, MaxTerm, MaxLogLen, MaxMsgs, MaxDup (-1: unbounded), bug, invariants, sym, levels
CONFIGS = {
    "mcraft_shipped_sym_d12": (3, 2, -1, 8, 12, -1, 0, 1, 1, 12),
}


def main():
    out = {}
    for name, (S, V, mt, ml, mm, md, bug, inv, sym, lv) in CONFIGS.items():
        r, level_new, level_gen = oracle_c.bfs(S, V, mt, ml, mm, md, bug=bug, inv=inv, sym=sym,
                                               threads=min(16, os.cpu_count() or 1), max_levels=lv,
                                               capacity=1 << 24, wide=True)
        out[name] = dict(
            params=dict(n_servers=S, n_values=V, max_term=mt, max_log_len=ml, max_msgs=mm, max_dup=md,
                        bug_quorum=bug, invariants=inv, symmetry=sym, max_depth=lv),
            level_new=level_new, level_generated=level_gen, distinct=r.distinct, generated=r.generated,
            depth=r.depth, left_on_queue=level_new[-1])
        print(name, r.distinct, r.generated, r.depth)
    with open(os.path.join(ROOT, "tests", "golden", "wide_symmetry_levels.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
