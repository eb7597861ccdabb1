"""The simulators' draw rules (tests/sim_rules.py, the Python restatement the GPU
tests in test_sim_draws.py predict with) against the real host code of
raft_wide.h (tests/native/sim_draw_check.cpp, also built with the address and
undefined-behaviour sanitizers), and the uniformity the rules claim.  No GPU."""
import os
import random
import subprocess
from fractions import Fraction

import pytest

from tests import sim_rules as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sim_draw_check.cpp")
NC = 5  # mask words of the wide lane table (WLMASK)


def _lanes(words):
    return [64 * c + k for c, w in enumerate(words) for k in range(64) if w >> k & 1]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_restated_draws_equal_the_native_draws(tmp_path, flags):
    """w_rand, uniform_draw and tlc_draw of raft_wide.h, compiled for the host, on
    random enabled / excluded masks at (S, V) = (2,1), (3,1), (3,2), (5,2): the
    restatement picks the same lane and leaves the stream at the same position
    (so it consumed the same number of draws), 300 masks per shape and draw."""
    exe = tmp_path / "sim_draw_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-I",
                    os.path.join(ROOT, "raft.tla_amd", "csrc"), SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "300", "9"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = {"stream": 0, "uni": 0, "tlc": 0}
    shapes, none_enabled, all_excluded = set(), 0, 0
    for line in r.stdout.splitlines():
        f = line.split()
        seen[f[0]] += 1
        if f[0] == "stream":
            st = SR.Stream(int(f[1], 16), int(f[2], 16))
            assert [st.draw() for _ in range(4)] == [int(x, 16) for x in f[3:7]], line
            continue
        S, V, rs = int(f[1]), int(f[2]), int(f[3], 16)
        en = _lanes([int(x, 16) for x in f[4:4 + NC]])
        st = SR.Stream.at(rs)
        shapes.add((S, V))
        if f[0] == "uni":
            excl = set(_lanes([int(x, 16) for x in f[4 + NC:4 + 2 * NC]]))
            pick = SR.uniform_draw(st, en, excl)
            none_enabled += not en
            all_excluded += bool(en) and set(en) <= excl
        else:
            pick = SR.tlc_draw(st, en, S, V)
        assert (pick, st.rs) == (int(f[-2]), int(f[-1], 16)), line
    assert seen == {"stream": 16, "uni": 1200, "tlc": 1200}
    assert shapes == {(2, 1), (3, 1), (3, 2), (5, 2)}
    assert none_enabled > 0 and all_excluded > 100  # the -1 returns are among the cases


def test_the_action_list_is_the_models():
    """S, S, S^2, S, S*|Value|, S, S^2 server actions and three message actions; with
    |Value| = 2 an action's index is its lane, with |Value| = 1 the ClientRequest
    lanes of value 1 are no action."""
    for S in (2, 3, 4, 5):
        off = SR.wide_offsets(S)
        for V in (1, 2):
            acts = SR.tlc_actions(S, V)
            assert len(acts) == 3 * S + 2 * S * S + S * V + S + 3
            assert acts[-3:] == [("family", off[7], off[8]), ("family", off[8], off[9]), ("family", off[9], off[10])]
            lanes = [a[1] for a in acts[:-3]]
            assert lanes == sorted(lanes)
            missing = set(range(off[7])) - set(lanes)
            assert missing == ({off[4] + 2 * i + 1 for i in range(S)} if V == 1 else set())


def _tlc_exact(en, S, V):
    """The stated rule's exact probability of every lane: all start x stride pairs."""
    acts = SR.tlc_actions(S, V)
    n = len(acts)
    p = {}
    for start in range(n):
        for stride in SR.PRIMES:
            for i in range(n):
                a = acts[(start + i * stride) % n]
                fam = [a[1]] if a[0] == "lane" else list(range(a[1], a[2]))
                on = [l for l in fam if l in en]
                if on:
                    for l in on:
                        p[l] = p.get(l, 0) + Fraction(1, n * 8 * len(on))
                    break
    return p


def test_tlc_rule_at_one_value_weighs_the_models_actions():
    """S = 3, |Value| = 1, server 0 leader, two followers, two messages in the bag:
    the stated rule draws AdvanceCommitIndex(0) with probability 0.066; over the
    lane table's 39 slots (three ClientRequest lanes that no model action owns)
    it would be 0.038.  The restated draw follows the exact probabilities."""
    S, V = 3, 1
    off = SR.wide_offsets(S)
    en = set(range(off[0], off[1]))                       # Restart: every server
    en |= {off[1] + 1, off[1] + 2}                        # Timeout: the followers
    en |= {off[4]}                                        # ClientRequest(0, v0)
    en |= {off[5]}                                        # AdvanceCommitIndex(0)
    en |= {off[6] + 1, off[6] + 2}                        # AppendEntries(0, 1), (0, 2)
    en |= {off[7], off[7] + 1, off[8], off[8] + 1, off[9], off[9] + 1}
    p = _tlc_exact(en, S, V)
    assert sum(p.values()) == 1
    assert round(float(p[off[5]]), 3) == 0.066
    st = SR.Stream(3, 0)
    n = 40000
    hist = {}
    for _ in range(n):
        l = SR.tlc_draw(st, en, S, V)
        hist[l] = hist.get(l, 0) + 1
    assert set(hist) == set(p)
    for l, pl in p.items():
        e = float(pl) * n
        assert abs(hist[l] - e) <= 6 * (e * (1 - float(pl))) ** 0.5, (l, hist[l], e)


def _random_lanes(rng, n_lanes=40):
    """(lane, in_bounds) of a random set of enabled lanes, some beyond the bounds."""
    dens, out_dens = rng.choice([0.15, 0.4, 0.8]), rng.choice([0.0, 0.3, 0.7])
    lanes = [(l, rng.random() >= out_dens) for l in range(n_lanes) if rng.random() < dens]
    return lanes or [(rng.randrange(n_lanes), True)]


def _assert_uniform(hist, eligible, n, what):
    assert set(hist) <= set(eligible), what
    p = 1.0 / len(eligible)
    e, sd = p * n, (n * p * (1 - p)) ** 0.5
    for l in eligible:
        assert abs(hist.get(l, 0) - e) <= 6 * sd, (what, l, hist.get(l, 0), e)


@pytest.mark.parametrize("mode", [SR.WITHIN_CAPACITY, SR.TRUNCATE])
def test_packed_reservoir_is_uniform_over_the_eligible_lanes(mode):
    """One reservoir pass over random lane sets with a random subset beyond the
    bounds: mode 0 takes every lane within the bounds, mode 1 every enabled lane
    (truncated when beyond), with probability 1 / eligible each, within 6 standard
    deviations over 6,000 steps per set; no eligible lane means deadlocked."""
    rng = random.Random(17 + mode)
    for t in range(10):
        lanes = _random_lanes(rng)
        eligible = [l for l, inb in lanes if inb or mode == SR.TRUNCATE]
        st = SR.Stream(5, t)
        hist, n = {}, 6000
        for _ in range(n):
            pick, end = SR.packed_step(st, lanes, mode)
            if not eligible:
                assert (pick, end) == (-1, "deadlocked")
                continue
            assert end == (None if dict(lanes)[pick] else "truncated")
            hist[pick] = hist.get(pick, 0) + 1
        if eligible:
            _assert_uniform(hist, eligible, n, (mode, t))


@pytest.mark.parametrize("mode", [SR.WITHIN_CAPACITY, SR.TRUNCATE])
def test_wide_uniform_step_is_uniform_over_the_eligible_lanes(mode):
    """The wide step over the same kind of sets: mode 0's exclude-and-redraw ends on
    every lane within the bounds with probability 1 / (lanes within the bounds) and
    reports the behaviour truncated when every enabled lane is beyond them; mode 1
    takes every enabled lane with probability 1 / enabled."""
    rng = random.Random(29 + mode)
    for t in range(10):
        lanes = _random_lanes(rng)
        inb = dict(lanes)
        eligible = [l for l, i in lanes if i or mode == SR.TRUNCATE]
        st = SR.Stream(6, t)
        hist, n = {}, 6000
        for _ in range(n):
            pick, end, excl = SR.wide_uniform_step(st, lanes, mode)
            if not eligible:
                assert (pick, end) == (-1, "truncated") and excl == set(inb)
                continue
            assert end == (None if inb[pick] else "truncated")
            assert all(not inb[l] for l in excl) and (mode == SR.WITHIN_CAPACITY or not excl)
            hist[pick] = hist.get(pick, 0) + 1
        if eligible:
            _assert_uniform(hist, eligible, n, (mode, t))
