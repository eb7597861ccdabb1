"""What the constraint pass costs (measurement tool; DESIGN.md "Model-defined constraints",
"Measured"): specs/MCraftBench.cfg on this build without constraints, with the residual
TRUE (the filter pass alone: nothing is removed, nothing moves) and with
`\\A i \\in Server : state[i] /= Leader` (real removal) — and, given another checkout of
this project with its library built (e.g. the parent commit's, under abtest/), the model
on that build and its binding too.

    python tools/constraints_cost.py [--parent abtest/parent] [--rounds 3] [--runs 5] [--out FILE.json]

The variants alternate: every round starts one fresh process and ctx per variant, which
runs one warm-up search and `runs` timed ones (rmc_result.seconds: the wall time of
rmc_run_bfs).  Median and min-max per variant; a child's stderr carries the pass's
statistic line (RMC_CONS_STATS: passes, states removed, states moved)."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDUALS = {"true": "TRUE", "noleader": "\\A i \\in Server : state[i] /= Leader"}


def child(variant, cfg_path, runs):
    sys.path.insert(0, os.path.join(os.environ.get("RMC_COST_ROOT", ROOT), "raft.tla_amd"))
    import rmc
    cons = None
    if variant in RESIDUALS:
        cfg, _notes, _preds, cons = rmc.load_model(cfg_path, builtin_raft=True, constraints=True)
    else:
        cfg = rmc.config_from_files(cfg_path, builtin_raft=True)
    cfg.state_capacity = 1_500_000_000
    out = []
    with rmc.Checker(cfg) as ck:
        if cons is not None:
            ck.set_constraints(cons)
        for k in range(runs + 1):
            r = ck.run(record_levels=False)
            if k:
                out.append({"seconds": r.seconds, "expand_kernel_seconds": r.expand_kernel_seconds,
                            "launches": r.expand_launches, "distinct": r.distinct, "generated": r.generated,
                            "depth": r.depth, "violated": r.violated_inv})
    print(json.dumps(out))


def model_with(tmp, residual):
    """specs/MCraftBench with `residual` as one more conjunct of StateConstraint."""
    d = os.path.join(tmp, residual)
    os.makedirs(d)
    for f in ("MCraftBench.cfg", "MCraftBench.tla", "MCraftBounded.tla"):
        shutil.copy(os.path.join(ROOT, "specs", f), d)
    p = os.path.join(d, "MCraftBounded.tla")
    text = open(p).read()
    bullet = "    /\\ \\A m \\in DOMAIN messages : messages[m] <= MaxDup\n"
    assert text.count(bullet) == 1
    with open(p, "w") as f:
        f.write(text.replace(bullet, bullet + "    /\\ " + RESIDUALS[residual] + "\n"))
    return os.path.join(d, "MCraftBench.cfg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs)
    variants = (["parent"] if a.parent else []) + ["new", "true", "noleader"]
    raw, stats = {v: [] for v in variants}, {}
    with tempfile.TemporaryDirectory() as tmp:
        cfgs = {v: model_with(tmp, v) if v in RESIDUALS else os.path.join(ROOT, "specs", "MCraftBench.cfg")
                for v in variants}
        for _ in range(a.rounds):
            for v in variants:
                env = dict(os.environ, RMC_CONS_STATS="1")
                if v == "parent":
                    env["RMC_COST_ROOT"] = os.path.abspath(a.parent)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", v, cfgs[v]],
                                   capture_output=True, text=True, env=env, timeout=600)
                if r.returncode:  # nothing more is started after a failing child
                    sys.exit("variant %s failed:\n%s%s" % (v, r.stdout[-2000:], r.stderr[-3000:]))
                raw[v] += json.loads(r.stdout.strip().splitlines()[-1])
                m = re.findall(r"constraint pass: (\d+) passes, (\d+) states removed, (\d+) states moved", r.stderr)
                if m:
                    stats[v] = dict(zip(("passes", "removed", "moved"), map(int, m[-1])))
    summary = {}
    for v in variants:
        ms = [x["seconds"] * 1e3 for x in raw[v]]
        counts = {(x["distinct"], x["generated"], x["depth"], x["violated"]) for x in raw[v]}
        assert len(counts) == 1, (v, counts)
        summary[v] = {"n": len(ms), "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                      "median_expand_kernel_ms": statistics.median(x["expand_kernel_seconds"] * 1e3 for x in raw[v]),
                      "launches": raw[v][0]["launches"], "counts": list(counts.pop()), "pass": stats.get(v)}
    doc = {"model": "specs/MCraftBench.cfg", "residuals": RESIDUALS, "runs_per_child": a.runs, "rounds": a.rounds,
           "summary": summary, "raw": raw}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
