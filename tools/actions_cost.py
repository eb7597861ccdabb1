"""What the action property pass costs (measurement tool; DESIGN.md "Action properties",
"Measured"): specs/MCraftBench.cfg on this build without properties and with
`TermsMonotonic == [][\\A i \\in Server : currentTerm'[i] >= currentTerm[i]]_vars` set — and,
given another checkout of this project with its library built (e.g. the parent commit's, under
abtest/), the model on that build and its binding too.

    python tools/actions_cost.py [--parent abtest/parent] [--rounds 1] [--runs 5] [--out FILE.json]

The variants alternate: every round starts one fresh process and ctx per variant, which runs
one warm-up search and `runs` timed ones (rmc_result.seconds: the wall time of rmc_run_bfs).
Median and min-max per variant.  A last process counts the transitions the pass checks: the
edges of the state graph (rmc_graph_edges' count over every stored state)."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPERTY = "TermsMonotonic == [][\\A i \\in Server : currentTerm'[i] >= currentTerm[i]]_vars\n"


def child(variant, cfg_path, runs):
    sys.path.insert(0, os.path.join(os.environ.get("RMC_COST_ROOT", ROOT), "raft.tla_amd"))
    import rmc
    acts = None
    if variant == "actions":
        cfg, _notes, _preds, acts = rmc.load_model(cfg_path, builtin_raft=True, actions=True)
    else:
        cfg = rmc.config_from_files(cfg_path, builtin_raft=True)
    cfg.state_capacity = 1_500_000_000
    out = []
    with rmc.Checker(cfg) as ck:
        if acts is not None:
            ck.set_actions(acts)
        if variant == "edges":  # the transitions the pass checks: one search, then the graph's count
            r = ck.run(record_levels=False)
            _none, n = ck.graph_edges(0, r.distinct, cap=0)
            print(json.dumps({"edges": n, "distinct": r.distinct, "generated": r.generated}))
            return
        for k in range(runs + 1):
            r = ck.run(record_levels=False)
            if k:
                out.append({"seconds": r.seconds, "expand_kernel_seconds": r.expand_kernel_seconds,
                            "launches": r.expand_launches, "distinct": r.distinct, "generated": r.generated,
                            "depth": r.depth, "violated": r.violated_inv})
    print(json.dumps(out))


def model_with_property(tmp):
    """specs/MCraftBench with TermsMonotonic defined and named as a PROPERTY."""
    d = os.path.join(tmp, "actions")
    os.makedirs(d)
    for f in ("MCraftBench.cfg", "MCraftBench.tla", "MCraftBounded.tla"):
        shutil.copy(os.path.join(ROOT, "specs", f), d)
    p = os.path.join(d, "MCraftBounded.tla")
    lines = open(p).read().rstrip("\n").split("\n")
    assert lines[-1].startswith("====")
    with open(p, "w") as f:
        f.write("\n".join(lines[:-1]) + "\n\n" + PROPERTY + lines[-1] + "\n")
    with open(os.path.join(d, "MCraftBench.cfg"), "a") as f:
        f.write("PROPERTY TermsMonotonic\n")
    return os.path.join(d, "MCraftBench.cfg")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-edges", action="store_true")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs)
    variants = (["parent"] if a.parent else []) + ["new", "actions"]
    raw = {v: [] for v in variants}
    edges = None

    def start(v, cfg):
        env = dict(os.environ)
        if v == "parent":
            env["RMC_COST_ROOT"] = os.path.abspath(a.parent)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--runs", str(a.runs), "--child", v, cfg],
                           capture_output=True, text=True, env=env, timeout=900)
        if r.returncode:  # nothing more is started after a failing child
            sys.exit("variant %s failed:\n%s%s" % (v, r.stdout[-2000:], r.stderr[-3000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    with tempfile.TemporaryDirectory() as tmp:
        plain = os.path.join(ROOT, "specs", "MCraftBench.cfg")
        cfgs = {v: model_with_property(tmp) if v == "actions" else plain for v in variants}
        for _ in range(a.rounds):
            for v in variants:
                raw[v] += start(v, cfgs[v])
                print("%s: %s ms" % (v, ["%.1f" % (x["seconds"] * 1e3) for x in raw[v][-a.runs:]]), flush=True)
        if not a.no_edges:
            edges = start("edges", plain)
    summary = {}
    for v in variants:
        ms = [x["seconds"] * 1e3 for x in raw[v]]
        counts = {(x["distinct"], x["generated"], x["depth"], x["violated"]) for x in raw[v]}
        assert len(counts) == 1, (v, counts)
        summary[v] = {"n": len(ms), "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
                      "median_expand_kernel_ms": statistics.median(x["expand_kernel_seconds"] * 1e3 for x in raw[v]),
                      "launches": raw[v][0]["launches"], "counts": list(counts.pop())}
    assert summary["new"]["counts"] == summary["actions"]["counts"]
    added = summary["actions"]["median_ms"] - summary["new"]["median_ms"]
    summary["pass"] = {"added_ms": added, "ratio": summary["actions"]["median_ms"] / summary["new"]["median_ms"],
                       "checked_transitions": edges["edges"] if edges else None,
                       "ns_per_checked_transition": added * 1e6 / edges["edges"] if edges else None,
                       "ns_per_generated_transition": added * 1e6 / summary["new"]["counts"][1]}
    doc = {"model": "specs/MCraftBench.cfg", "property": PROPERTY.strip(), "runs_per_child": a.runs, "rounds": a.rounds,
           "summary": summary, "raw": raw}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))


if __name__ == "__main__":
    main()
