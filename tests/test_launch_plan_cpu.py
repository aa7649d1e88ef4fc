"""csrc/launch_plan.h: resolve_plan over every combination of the kernel-family switches (ILQR_DYN, ILQR_ROLLOUT, ILQR_LS, ILQR_BACKWARD,
ILQR_LINT), contact mode, joint-limit option and Jacobian mode -- 2880 combinations, printed by tests/cpp/launch_plan_dump.cpp (host-only
C++17, no HIP) -- against the rules restated here from the description of the switches above read_variants (ilqr_kernels.hip) and from
the refusal messages of the C ABI.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc")
ONE_LANE, TWO_LANE, SCALAR = 0, 1, 2                                    # DynFamily
LIN_TWO_KNOT, LIN_ONE_KNOT, LIN_FD_TWO_LANE, LIN_FD_SCALAR = 0, 1, 2, 3  # LinKernel
PACK, WAVE_GENERIC, WAVE_FOLDED, FOUR_WAVE, VALU = 0, 1, 2, 3, 4        # BackwardKernel


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_dump")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "launch_plan_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [{k: int(v) for k, v in (tok.split("=") for tok in line.split())} for line in r.stdout.splitlines()]
    assert len(out) == 2880
    keys = ("scalar_dyn", "rollout_split", "ls_split", "backward", "fold", "lin_one_knot", "contact", "limits", "jac_mode")
    assert len({tuple(d[k] for k in keys) for d in out}) == 2880        # every combination once
    return out


def expected(d):
    """the plan of one combination, rule by rule"""
    scalar, contact, limits = bool(d["scalar_dyn"]), d["contact"], bool(d["limits"])
    rows_on = contact != 0 or limits                                    # stance rows and / or joint-limit rows: the constrained step
    e = {}

    def family(split):
        # ILQR_DYN=s: the scalar kernels for every dynamics stage; else two lanes where the switch says so and wherever the step is
        # constrained (the one-lane register kernels are constraint-free only)
        return SCALAR if scalar else TWO_LANE if (split or rows_on) else ONE_LANE
    e["p.rollout"] = family(d["rollout_split"])
    e["p.line_search"] = family(d["ls_split"])
    e["p.step"] = family(False)                                         # the single step has no switch: two lanes only when constrained
    # 0 free; 1 stance rows, 2 with kinetic friction (contact mode 4); 3 / 4 the same with joint-limit rows; 5 limits only
    e["p.step_kind"] = {(False, False): 0, (True, False): 2 if contact == 4 else 1, (True, True): 4 if contact == 4 else 3, (False, True): 5}[(contact != 0, limits)]
    # analytic Jacobians: everywhere but under ILQR_DYN=s in contact ("the analytic kernels are constraint-free only" there)
    analytic = d["jac_mode"] == 0 and not (scalar and contact != 0)
    if analytic:
        e["p.lin"] = LIN_ONE_KNOT if d["lin_one_knot"] else LIN_TWO_KNOT
    else:
        e["p.lin"] = LIN_FD_SCALAR if scalar else LIN_FD_TWO_LANE
    e["p.primal_dump"] = ONE_LANE if scalar else e["p.rollout"]         # beside the rollout kernels; ILQR_DYN=s: the one-lane dump
    e["p.lin_contact_tangent"] = int(analytic and contact != 0)
    e["p.lin_friction"] = {3: 1, 4: 2}.get(contact, 0)
    e["p.limits"] = int(limits)
    e["p.lin_stance_prepass"] = int(d["jac_mode"] == 0 and not scalar and contact != 0)
    # ILQR_BACKWARD: valu -> 1, wave* -> 2 (fold: wave-generic 0, wave-fold 1, wave 2), wg -> 0
    plain = {0: FOUR_WAVE, 1: VALU, 2: WAVE_GENERIC}[d["backward"]]
    foldable = {0: WAVE_GENERIC, 1: WAVE_FOLDED, 2: PACK}[d["fold"]] if d["backward"] == 2 else plain
    folds = analytic and d["backward"] == 2 and d["fold"] != 0
    e["p.backward_plain"], e["p.backward_foldable"], e["p.folds_h"] = plain, foldable, int(folds)
    e["p.backward"] = foldable if folds else plain
    e["p.pack"] = int(e["p.backward"] == PACK)
    e["p.lxx_layout"] = {PACK: 2, WAVE_GENERIC: 1, WAVE_FOLDED: 1, FOUR_WAVE: 0, VALU: 0}[e["p.backward"]]
    e["p.ls_costs_per_knot"] = int(e["p.line_search"] == TWO_LANE)
    e["p.spec_dual"] = int(e["p.line_search"] == TWO_LANE and d["backward"] == 2)
    e["p.lin_lists"] = int(analytic)
    # the re-rollout reproduces the accepted candidate when both stages run the same step: constrained (both on two lanes) or equal switches
    e["p.reroll_aside"] = int(rows_on or d["ls_split"] == d["rollout_split"])
    e["p.cold_start_aside"] = int(e["p.reroll_aside"] and not scalar)
    # "weight sets exist in the default family's cost kernels only; unset ILQR_DYN=s / ILQR_ROLLOUT=r / ILQR_LS=r"
    e["p.weight_sets"] = int(not scalar and d["rollout_split"] and d["ls_split"])
    # "... exist(s) on the two-lane kernels only; unset ILQR_DYN=s"
    e["p.stance_geometry"] = e["p.cone_and_limits"] = int(not scalar)
    # "analytic Jacobians are not available in this kernel family (ILQR_LIN / ILQR_DYN)"
    e["p.analytic_full"] = int(not scalar and not d["lin_one_knot"])
    # the product library holds the default family alone: two-lane rollout and line search, the one-wave Riccati kernels but the folded
    # one on the standard layout, the two-knot tangent kernels
    e["supported"] = int(not scalar and d["rollout_split"] and d["ls_split"] and d["backward"] == 2 and d["fold"] != 1 and not d["lin_one_knot"])
    e["supported_legacy"] = 1
    return e


def test_plan_equals_the_rules_of_the_switches_in_all_2880_combinations(rows):
    fields = set(expected(rows[0]))
    assert fields == {k for k in rows[0] if k.startswith("p.") or k.startswith("supported")}      # every field of the dump is compared
    bad = [(k, d[k], e[k], d) for d in rows for e in [expected(d)] for k in fields if d[k] != e[k]]
    assert not bad, (len(bad), bad[:3])


def test_product_build_accepts_exactly_the_default_family(rows):
    ok = {tuple(d[k] for k in ("scalar_dyn", "rollout_split", "ls_split", "backward", "fold", "lin_one_knot")) for d in rows if d["supported"]}
    assert ok == {(0, 1, 1, 2, 0, 0), (0, 1, 1, 2, 2, 0)}
    assert all(d["supported_legacy"] for d in rows)


def test_default_family_plan(rows):
    """the headline: two lanes everywhere they exist, two-knot analytic kernels into the operand layout, the pack kernel behind them"""
    for d in rows:
        if (d["scalar_dyn"], d["rollout_split"], d["ls_split"], d["backward"], d["fold"], d["lin_one_knot"], d["jac_mode"]) != (0, 1, 1, 2, 2, 0, 0):
            continue
        assert d["p.rollout"] == d["p.line_search"] == TWO_LANE and d["p.lin"] == LIN_TWO_KNOT and d["p.backward"] == PACK and d["p.pack"] and d["p.lxx_layout"] == 2
        assert d["p.step"] == (TWO_LANE if d["contact"] or d["limits"] else ONE_LANE)
        assert all(d[k] for k in ("p.ls_costs_per_knot", "p.spec_dual", "p.lin_lists", "p.reroll_aside", "p.cold_start_aside", "p.weight_sets", "p.stance_geometry", "p.cone_and_limits", "p.analytic_full"))
