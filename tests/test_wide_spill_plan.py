"""The wide layout's record choice under RMC_FLAG_SPILL (no device needed).

A depth-bounded spilled run never stores its last level, so the store's
record is sized from max_depth - 2 steps instead of max_depth - 1
(rmc_wide.cpp wide_compact): MCraft.cfg as shipped keeps the 336-B record one
level deeper, to depth 15.  Without the flag nothing changes."""
import os

import pytest

import rmc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "tests", "golden", "models", "MCunbounded.cfg")


@pytest.fixture(autouse=True)
def _no_record_override(monkeypatch):
    monkeypatch.delenv("RMC_WIDE_COMPACT", raising=False)
    monkeypatch.delenv("RMC_WIDE_WORK", raising=False)
    monkeypatch.delenv("RMC_FORCE_WIDE", raising=False)


def _state_bytes(depth, spill):
    c, _, _ = rmc.model_from_files(CFG, builtin_raft=True, depth_bounded=True)
    c.max_depth = depth
    if spill:
        c.flags |= rmc.FLAG_SPILL
    return rmc.native().rmc_state_bytes(c)


@pytest.mark.parametrize("depth,want", [(14, 336), (15, 336), (16, 904)])
def test_spilled_store_record_is_sized_from_the_last_stored_level(depth, want):
    assert _state_bytes(depth, spill=True) == want


def test_resident_store_record_is_unchanged():
    assert _state_bytes(14, spill=False) == 336
    assert _state_bytes(15, spill=False) == 904
