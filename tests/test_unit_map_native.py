"""Host-side check of the expansion launch's work-unit map (rmc_units.h: the
arithmetic expand_body decodes its work counter with), compiled for the host
with g++ (no GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unit_map_covers_every_window_tile_and_quarter_exactly_once(tmp_path):
    """For every window size wt in 1..16 tiles, every unit size of the ladder
    (16, 8, 4, 2 tiles) and launches of nf in {1, 63, 64, 65, 255, 256, 257,
    256 wt - 1, 256 wt, 256 wt + 1, 3 * 256 wt + 77} states: the units with a
    counter value below units_total cover every (window, tile, quarter) whose
    first position lies inside its window exactly once and none twice, no unit
    reaches a tile >= wt, every counter value from units_total on (the next
    65,536 and the largest of 32 bits) decodes to a window past the launch, and
    a unit of 16 tiles is the wave's quarter of a whole window
    (id >> 2, id & 3, 0, wt)."""
    exe = tmp_path / "unit_map_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "raft.tla_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "unit_map_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith("ok 704 cases, "), r.stdout
