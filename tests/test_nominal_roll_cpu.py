"""csrc/solve_order.h nominal_roll and splits_next, printed by tests/cpp/nominal_roll_dump.cpp (host-only C++17, no HIP), against the rule
restated here.  No GPU.

nominal_roll is THE rule for the nominal rollout of an iteration -- not at all, in front of the region, beside it -- for every launch order:
every combination of reuse_rollout, overlap_rollout, first_aside, LaunchPlan::reroll_aside, LaunchPlan::cold_start_aside over the
iterations 0, 1, 2.  splits_next is the early-continuation split's condition with the re-rollout taken out of it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc")
NONE, BEFORE, ASIDE = 0, 1, 2                                            # NominalRoll
MAX_ITER = 3                                                             # the solve the dump asks splits_next about


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nominal_roll") / "nominal_roll_dump")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "nominal_roll_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    cols = lines[0].split()
    return [dict(zip(cols, map(int, line.split()))) for line in lines[1:]]


def expected_roll(r):
    # the trajectory the buffers hold is what the rollout would write: iterations >= 1 where the line search and the rollout run the same step
    # implementation, iteration 0 behind a cold start by the rollout kernel
    same = r["reroll_aside"] if r["iter"] > 0 else (r["first_aside"] and r["cold_start_aside"])
    if r["reuse"]:
        return NONE if same else BEFORE                                 # (ILQR_OVERLAP_ROLLOUT has nothing to move)
    return ASIDE if same and r["overlap"] else BEFORE                   # the re-roll of every iteration: rolls_aside


def test_every_combination_once(rows):
    keys = {tuple(r[k] for k in ("reuse", "overlap", "first_aside", "can_split", "reroll_aside", "cold_start_aside", "iter")) for r in rows}
    assert len(rows) == len(keys) == 64 * 3
    assert {r["iter"] for r in rows} == {0, 1, 2}


def test_nominal_roll_equals_the_rule(rows):
    for r in rows:
        assert r["nominal_roll"] == expected_roll(r), r


def test_without_reuse_the_rule_is_rolls_aside(rows):
    for r in rows:
        if not r["reuse"]:
            assert r["nominal_roll"] == (ASIDE if r["rolls_aside"] else BEFORE), r
        # rolls_aside keeps its meaning: never with reuse
        assert r["rolls_aside"] == int(bool((r["reroll_aside"] if r["iter"] > 0 else (r["first_aside"] and r["cold_start_aside"])) and not r["reuse"] and r["overlap"])), r


def test_default_rolls_nothing_where_the_buffers_hold_the_result(rows):
    """the benchmark's headline: reuse, cold start, the shipped kernel family -- no rollout in any iteration; a warm start: iteration 0 alone"""
    for r in rows:
        if r["reuse"] and r["reroll_aside"] and r["cold_start_aside"]:
            assert r["nominal_roll"] == (NONE if r["iter"] > 0 or r["first_aside"] else BEFORE), r
        if r["reuse"] and not r["reroll_aside"]:                         # mixed cross-check families: every iteration >= 1 rolls out first, as before
            assert r["iter"] == 0 or r["nominal_roll"] == BEFORE, r
        if r["reuse"]:
            assert r["nominal_roll"] != ASIDE, r


def test_split_rests_on_the_equality_not_on_the_re_rollout(rows):
    for r in rows:
        nxt = dict(r, iter=r["iter"] + 1)
        want = bool(r["can_split"] and r["iter"] + 1 < MAX_ITER and r["reroll_aside"] and expected_roll(nxt) != BEFORE)
        assert r["splits_next"] == int(want), r
        if r["reuse"]:                                                   # the default keeps the split wherever the parent's re-roll aside had it
            assert r["splits_next"] == int(bool(r["can_split"] and r["iter"] + 1 < MAX_ITER and r["reroll_aside"])), r
