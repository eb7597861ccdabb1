"""Generates tests/golden/continue_cases.json: what a search that continues past
violations (RMC_FLAG_CONTINUE, TLC -continue) must report, computed by the Python
restatement of the spec (tests/continue_cases.py over oracle/raft_spec.py).  One
process per case; the `cli_messages_small` case is the full 2.47 M-state search
of specs/MCraftMessages.cfg and takes some minutes and a few GB, the others
seconds.  Run from the repo root:
    python tests/golden/make_continue_golden.py [case ...]
"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import continue_cases  # noqa: E402


def main(only=None):
    """`only`: names to (re)generate, merged into the existing file."""
    path = os.path.join(ROOT, "tests", "golden", "continue_cases.json")
    out = json.load(open(path)) if only and os.path.exists(path) else {}
    names = [n for n in continue_cases.CASES if not only or n in only]
    with multiprocessing.Pool(min(len(names), os.cpu_count() or 1)) as pool:
        for name, rec in zip(names, pool.imap(continue_cases.run_case, names)):
            out[name] = rec
            print(name, rec["distinct"], rec["generated"], rec["depth"], rec["states"], rec["first"], rec["each"],
                  rec["inv_depth"], flush=True)
    with open(path, "w") as f:
        json.dump({n: out[n] for n in continue_cases.CASES if n in out}, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1:] or None)
