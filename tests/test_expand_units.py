"""The expansion kernel's tile-group work units (rmc_units.h; expand_body, DYN)
at window sizes and launch cuts the default grid never gives the small golden
models: every per-level count must stay the oracle's.

librmc reads RMC_EXPAND_GRID and RMC_LAUNCH_LOG2 once per process, so each
setting runs the three models in a process of its own."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "oracle_levels.json")))
MODELS = ("small", "tiny2_v2", "bounded_prefix14")

SCRIPT = r"""
import json, os, sys
sys.path.insert(0, os.path.join(sys.argv[1], 'raft.tla_amd'))
sys.path.insert(0, sys.argv[1])
import rmc
from tests.test_gpu import cfg_from, GOLDEN, run
out = {}
for name in sys.argv[2:]:
    g = GOLDEN[name]
    res, levels, _ = run(cfg_from(g["params"], capacity=max(1 << 22, int(g["distinct"] * 1.25))))
    out[name] = {"levels": levels, "distinct": res.distinct, "generated": res.generated, "depth": res.depth,
                 "launches": int(res.expand_launches)}
print(json.dumps(out))
"""


def run_models(tmp_path, **env):
    script = tmp_path / "expand_units.py"
    script.write_text(SCRIPT)
    e = {k: v for k, v in os.environ.items() if k not in ("RMC_EXPAND_GRID", "RMC_LAUNCH_LOG2")}
    e.update(env)
    r = subprocess.run([sys.executable, str(script), ROOT, *MODELS], capture_output=True, text=True, timeout=240,
                       env=e, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_counts(out):
    for name in MODELS:
        g, o = GOLDEN[name], out[name]
        assert o["levels"] == g["level_new"], name
        assert (o["distinct"], o["generated"], o["depth"]) == (g["distinct"], g["generated"], g["depth"]), name


def test_units_of_windows_of_up_to_15_tiles(tmp_path):
    """RMC_EXPAND_GRID=64: 256 waves, so levels of up to 0.24 M states are cut
    into windows of up to 15 tiles (ceil(states / 16384)): whole and partial
    last tile groups, partial last windows, and many units per wave."""
    assert max(max(GOLDEN[m]["level_new"][:-1]) for m in MODELS) > 8 * 64 * 256  # some window of more than 8 tiles
    check_counts(run_models(tmp_path, RMC_EXPAND_GRID="64"))


def test_units_of_windows_of_4_tiles_over_many_launches(tmp_path):
    """RMC_EXPAND_GRID=64 with RMC_LAUNCH_LOG2=16: launches of at most 65,536
    states, i.e. windows of 4 tiles (and fewer in a level's last launch),
    partial windows and many launches per level."""
    out = run_models(tmp_path, RMC_EXPAND_GRID="64", RMC_LAUNCH_LOG2="16")
    check_counts(out)
    for name in MODELS:
        assert out[name]["launches"] >= sum(-(-x // 65536) for x in GOLDEN[name]["level_new"][:-1]), name


def test_units_of_one_tile_windows_on_the_default_grid(tmp_path):
    """The default grid (one round of resident blocks) gives these models one
    block per 256 states: windows of one tile, one tile group per quarter."""
    check_counts(run_models(tmp_path))
