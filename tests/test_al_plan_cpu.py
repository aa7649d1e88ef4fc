"""csrc/al_plan.h: resolve_al_plan over the augmented Lagrangian on / off and, per family, {nothing, table of 1, table of B, window of 1,
window of B} -- 50 combinations, printed by tests/cpp/al_plan_dump.cpp (host-only C++17, no HIP) -- against the rules restated here from
the header's own text and the texts of the bounds setters in include/ilqr_hip.h.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc")
AL_OFF, AL_MODEL, AL_TABLE, AL_TABLE_STATE, AL_KNOT_TABLE, AL_KNOT_TABLE_STATE = range(6)      # the cost kernels' template axis
NONE, MODEL_RANGES, MODEL_RECORD, TABLE, WINDOW, TABLE_EXPANDED, MODEL_EXPANDED = range(7)      # AlSource
NOTHING, TABLE_1, TABLE_B, WINDOW_1, WINDOW_B = range(5)                                         # what a family has installed (the dump's jc= / st=)
KEYS = ("on", "jc", "st")


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("al_plan") / "al_plan_dump")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "al_plan_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [{k: int(v) for k, v in (tok.split("=") for tok in line.split())} for line in r.stdout.splitlines()]
    assert len(out) == 50
    assert len({tuple(d[k] for k in KEYS) for d in out}) == 50        # every combination once
    return out


def expected(d):
    """the plan of one combination, rule by rule"""
    e = {}
    fam = ("jc", "st")
    if not d["on"]:
        # "Augmented Lagrangian off: the plain penalties, no bounds" -- whatever the families' records say
        for f in fam:
            e.update({"p.%s.source" % f: NONE, "p.%s.shared" % f: 1, "p.%s.per_knot" % f: 0})
        e.update({"p.variant": AL_OFF, "p.upload_model": 0, "p.expand_jc": 0, "p.expand_st": 0, "p.module": 0})
        return e
    installed = {f: d[f] != NOTHING for f in fam}
    window = {f: d[f] in (WINDOW_1, WINDOW_B) for f in fam}
    one = {f: d[f] in (TABLE_1, WINDOW_1) for f in fam}
    # "A window of either family installed: both families read windows"
    knot = window["jc"] or window["st"]
    # the joint / torque family: its window; its table -- "repeated over the knots" while the other family has a window; without either "the
    # model's ranges at the installed margin, formed in the kernels", "while a state family is installed ONE record of those same doubles",
    # which is what gets repeated under a state window
    if window["jc"]:
        jc = WINDOW
    elif installed["jc"]:
        jc = TABLE_EXPANDED if knot else TABLE
    elif knot:
        jc = MODEL_EXPANDED
    else:
        jc = MODEL_RECORD if installed["st"] else MODEL_RANGES
    # the state family: nothing, its window, or its table (repeated under a joint / torque window)
    st = NONE if not installed["st"] else WINDOW if window["st"] else TABLE_EXPANDED if knot else TABLE
    e["p.jc.source"], e["p.st.source"] = jc, st
    # "One set serves every rollout through a set stride of 0"; the model's record is one record, a family without a pointer has no stride
    e["p.jc.shared"] = int(one["jc"] or not installed["jc"])
    e["p.st.shared"] = int(one["st"] or not installed["st"])
    e["p.jc.per_knot"] = int(knot)
    e["p.st.per_knot"] = int(knot and installed["st"])
    # the work: the model record exists on the device only where something reads it; an expansion per family whose record is repeated; the
    # per-knot instantiations "live in the per-knot module"
    e["p.upload_model"] = int(jc in (MODEL_RECORD, MODEL_EXPANDED))
    e["p.expand_jc"] = int(jc in (TABLE_EXPANDED, MODEL_EXPANDED))
    e["p.expand_st"] = int(st == TABLE_EXPANDED)
    e["p.module"] = int(knot)
    # the variant: per knot or not, with the state family or not; without either the table's instantiation or the model's
    if knot:
        e["p.variant"] = AL_KNOT_TABLE_STATE if installed["st"] else AL_KNOT_TABLE
    elif installed["st"]:
        e["p.variant"] = AL_TABLE_STATE
    else:
        e["p.variant"] = AL_TABLE if installed["jc"] else AL_MODEL
    return e


def test_plan_equals_the_rules_in_all_50_combinations(rows):
    fields = set(expected(rows[0]))
    assert fields == {k for k in rows[0] if k.startswith("p.")}      # every field of the dump is compared
    bad = [(k, d[k], e[k], d) for d in rows for e in [expected(d)] for k in fields if d[k] != e[k]]
    assert not bad, (len(bad), bad[:3])


def test_the_launchers_find_the_plans_variant_in_the_pointers(rows):
    """al_variant, fed the nullness of ProblemDev::al / alb / alsb / alb_knot that the plan's sources imply, returns the plan's variant: the
    launchers and the handle cannot disagree in any installable state"""
    for d in rows:
        assert d["launcher"] == d["p.variant"], d


def test_module_safety(rows):
    for d in rows:
        if not d["p.module"]:
            assert d["p.variant"] not in (AL_KNOT_TABLE, AL_KNOT_TABLE_STATE), d      # never a call through a module nobody loaded
            assert not d["p.expand_jc"] and not d["p.expand_st"], d                   # (the expansion kernel lives there too)
        if not d["on"]:
            assert d["p.variant"] == AL_OFF and d["p.jc.source"] == NONE and d["p.st.source"] == NONE, d
        if d["p.st.source"] != NONE:
            assert d["p.jc.source"] not in (NONE, MODEL_RANGES), d      # the state instantiations take every bound from a record


def test_windows_bring_both_knot_strides_and_one_set_has_set_stride_zero(rows):
    for d in rows:
        if not d["on"]:
            continue
        if d["jc"] in (WINDOW_1, WINDOW_B) or d["st"] in (WINDOW_1, WINDOW_B):
            assert d["p.jc.per_knot"] and (d["p.st.per_knot"] or d["p.st.source"] == NONE), d
        for f in ("jc", "st"):
            if d[f] in (TABLE_1, WINDOW_1):
                assert d["p.%s.shared" % f], d
            if d[f] in (TABLE_B, WINDOW_B):
                assert not d["p.%s.shared" % f], d
