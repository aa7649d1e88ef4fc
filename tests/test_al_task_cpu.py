"""CPU checks of the restatement of the task family of the augmented-Lagrangian limits (tests/al_task_ref.py) the GPU tests compare
against, and of the inputs they use (tests/al_task_cases.py): the composed Jacobians and second-order sums against their own redundancy
(two weights) and the term against central differences of itself, known answers (a switched-off side, a stance knot, knot 0), proof that
the stage inputs discriminate, the reference driver on the end-to-end inputs, the plan's function with the third family, the entry points'
checks that need no handle, the scenario helper and the declarations (a handle needs a GPU: test_gpu_al_task.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import al_bounds_ref as br
import al_state_ref as sr
import al_task_cases as tc
import al_task_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the quadratics carry the reference's slot convention: the derivative with respect to the quaternion's (x, y, z, w)
# sits in the slots 3..6, whose state entries are (w, x, y, z).  PERM[slot] = the state entry the slot's derivative is taken along.
PERM = np.arange(51); PERM[3:7] = [4, 5, 6, 3]
GPU_TOL = 1e-10


def _active(t, g):
    return g < 2 and not (t == 0 and g > 0)


def test_composed_reference_against_its_own_redundancy():
    """The Jacobian rows and the second-order sums composed from the oracle's tracking terms under two weights w = 1 and w = 8: printed, and
    bounded at 1e-12 relative to the largest entry -- a hundredth of the GPU tolerance of 1e-10."""
    X, _, _, _, _, mu_t, rho, win, stance, _, _, cases, _ = tc.regimes()
    P = tr.points(X)
    worst = dict(J=0.0, C=0.0)
    for i, (k, side, t, g) in enumerate(cases):
        m, _ = tr.m_and_scale(P[i, t], win[i, t], stance[i, t], mu_t[i, t], rho[i, 3])
        J1, J8 = tr.kin(1.0).jacobian(X[i, t], P[i, t]), tr.kin(8.0).jacobian(X[i, t], P[i, t])
        worst["J"] = max(worst["J"], np.abs(J1 - J8).max() / np.abs(J1).max())
        if m.any():
            C1, C8 = tr.kin(1.0).curvature(X[i, t], m, P[i, t]), tr.kin(8.0).curvature(X[i, t], m, P[i, t])
            worst["C"] = max(worst["C"], np.abs(C1 - C8).max() / np.abs(C1).max())
    print("two weights, relative to the largest entry: Jacobian %.2e, second-order sum %.2e" % (worst["J"], worst["C"]))
    assert worst["J"] <= 1e-12 and worst["C"] <= 1e-12


def test_term_against_central_differences_of_itself():
    """Gradient and Hessian of the restated term at the excited knot of every regime case against central differences of its own phi / of its
    own gradient.  Step h = 1e-6 in every state entry (metres, radians, quaternion units).  The term is (rho / 2) c^2 + ... with rho ~ 5e4
    .. 1e5, |J| <= ~2 and second derivatives of the points of O(1): the gradient is ~4e2, the Hessian ~4e5 (printed below); a central
    difference then carries a rounding error ~ eps |f| / h ~ 1e-16 x 1e1 / 1e-6 = 1e-9 on the gradient (1e-16 x 4e2 / 1e-6 = 4e-8 on the
    Hessian) and a truncation error ~ h^2 f''' / 6 ~ 1e-12 x 1e6 = 1e-6: bound 1e-6 relative to the largest entry, and every regime keeps
    |mu + rho c| >= 100 off the kink while a step moves it by rho |J| h ~ 0.2."""
    X, _, _, _, _, mu_t, rho, win, stance, _, _, cases, _ = tc.regimes()
    h = 1e-6
    worst = dict(g=0.0, H=0.0, gmax=0.0, Hmax=0.0)
    seen = set()
    for i, (k, side, t, g) in enumerate(cases):
        x, w, st, mu, r = X[i, t], win[i, t], stance[i, t], mu_t[i, t], rho[i, 3]

        def f(v):
            return float(tr.phi(tr.points(v), w, st, mu, r).sum())

        def grad(v):
            _, gx, _ = tr.traj_terms(v[None], mu[None], r, w[None], st[None])
            return gx[0]

        _, gx, hxx = tr.traj_terms(x[None], mu[None], r, w[None], st[None])
        gx, hxx = gx[0], hxx[0]
        if g == 3 or not _active(t, g):
            assert not gx.any() and not hxx.any(), (i, cases[i])      # the constant only (a stance knot; an inactive regime; knot 0 inside)
            continue
        seen.add((side, g))
        s = (mu + r * tr.constraints(tr.points(x), w, st))[k, side]
        assert s > 100.0, (i, s)
        g_fd, H_fd = np.zeros(51), np.zeros((51, 51))
        for a in range(51):
            e = np.zeros(51); e[PERM[a]] = h
            g_fd[a] = (f(x + e) - f(x - e)) / (2 * h)
            H_fd[a] = (grad(x + e) - grad(x - e)) / (2 * h)
        worst["gmax"], worst["Hmax"] = max(worst["gmax"], np.abs(gx).max()), max(worst["Hmax"], np.abs(hxx).max())
        worst["g"] = max(worst["g"], np.abs(g_fd - gx).max() / np.abs(gx).max())
        worst["H"] = max(worst["H"], np.abs(H_fd - hxx).max() / np.abs(hxx).max())
        assert np.abs(hxx - hxx.T).max() <= 1e-12 * np.abs(hxx).max()
    print("central differences, h = %.0e: gradient %.2e of %.1e, Hessian %.2e of %.1e" % (h, worst["g"], worst["gmax"], worst["H"], worst["Hmax"]))
    assert len(seen) == 4
    assert worst["g"] <= 1e-6 and worst["H"] <= 1e-6


def test_known_answers_switched_off_side_stance_knot_and_knot_0():
    X, _, _, _, _, _, _, _, _, _, _, _, _ = tc.regimes()
    N = tc.N_STAGE
    Xb = np.array(X[0]); P = tr.points(Xb)
    stance = np.zeros((N + 1, 2), dtype=np.int32); stance[2, 1] = 1
    win = np.tile(tr.NO_BOUNDS, (N + 1, 1))
    win[:, 9 + 2] = P[:, 2] + 1.0                          # CoM z <= 1 above it: inactive, lower side off with a multiplier
    win[:, 8] = P[:, 8] + 0.01                             # the right ankle 1 cm below its floor at every knot
    mu = np.zeros((N + 1, 9, 2)); mu[1:, 2, 0] = 3.0
    rho = 50.0
    ck, gx, hxx = tr.traj_terms(Xb, mu, rho, win, stance)
    want = 0.5 * rho * 1e-4
    # the switched-off side: -mu^2 / (2 rho) per knot; the stance knot 2: no floor term, no gradient, no curvature
    assert abs(ck[0] - want) < 1e-12 and abs(ck[1] - (want - 9.0 / 100.0)) < 1e-12 and ck[2] == -9.0 / 100.0
    assert gx[1].any() and hxx[1].any() and not gx[2].any() and not hxx[2].any()
    nt, viol = tr.update_task(Xb, mu, rho, win, stance)
    assert not nt[:, 2].any() and not nt[0].any() and not nt[2].any() and abs(viol - 0.01) < 1e-12
    assert abs(nt[1, 8, 0] - rho * 0.01) < 1e-9 and abs(tr.violation(Xb, win, stance) - 0.01) < 1e-12
    # violated at knot 0 only, or at a stance knot only: no violation, nothing to update
    only0 = np.tile(tr.NO_BOUNDS, (N + 1, 1)); only0[0, 9 + 0] = P[0, 0] - 0.05
    only_st = np.tile(tr.NO_BOUNDS, (N + 1, 1)); only_st[2, 6] = P[2, 6] + 0.05
    for w in (only0, only_st):
        nt, viol = tr.update_task(Xb, np.zeros_like(mu), rho, w, stance)
        assert viol == 0.0 and not nt.any()
    assert tr.traj_terms(Xb, np.zeros_like(mu), rho, only0, stance)[0][0] > 0.0      # knot 0 carries the cost term
    assert tr.update_task(Xb, np.zeros_like(mu), rho, only_st, np.zeros_like(stance))[1] > 0.0
    assert np.array_equal(tr.shift(np.arange(90.0).reshape(5, 9, 2), 1)[1:4], np.arange(90.0).reshape(5, 9, 2)[2:5])


def test_stage_inputs_discriminate():
    """Reading row t +- 1 of the window, the other foot's rows, the other side's multiplier or a neighbouring axis' bounds moves the gradient
    or the cost of every stage case in which the excited side is active (g = 0; g = 1 off knot 0: an inactive constraint leaves its
    constant, whatever its bound) by more than 1e6 x the GPU tolerance: 1e-4 max(1, |want|) on lx, want the full expected gradient, or 1e-5
    relative on the cost.  Ignoring the stance rule moves the stance cases by as much.  Every other constraint is inactive."""
    X, U, mu_j, mu_c, mu_s, mu_t, rho, win, stance, srec, rec, cases, inf = tc.regimes()
    B = X.shape[0]
    assert B == 60 and len(set(cases)) == 60 and sum(1 for c in cases if c[3] == 3) == tc.STANCE_CASES
    assert sorted({c[2] for c in cases}) == list(range(tc.N_STAGE + 1))
    base, orc = tc.task_terms(), tc.oracle_stage()
    wrong = {"row t+1": tc.task_terms(shift_row=1), "row t-1": tc.task_terms(shift_row=-1), "other foot": tc.task_terms(swap_feet=True),
             "other side": tc.task_terms(swap_sides=True), "next axis": tc.task_terms(roll_axis=1), "no stance rule": tc.task_terms(use_stance=False)}
    least = {}
    for i, (k, side, t, g) in enumerate(cases):
        want_lx, want_c = tc.stage_expected(orc[i][0], orc[i][1], i, False, False)
        scale_g, scale_c = max(1.0, np.abs(want_lx["lx"]).max()), max(1.0, abs(want_c))
        ck, gx, hxx = base[i]
        assert np.count_nonzero(np.abs(gx).max(axis=1)) == (1 if (g < 3 and _active(t, g)) else 0), (i, cases[i])
        for what, terms in wrong.items():
            ck2, gx2, _ = terms[i]
            moved = max(np.abs(gx2 - gx).max() / scale_g / 1e-4, abs(ck2.sum() - ck.sum()) / scale_c / 1e-5)
            if what == "no stance rule":
                if g == 3:
                    least[what] = min(least.get(what, np.inf), moved); assert moved > 1.0, (i, what, moved)
            elif what == "other foot" and k < 3:
                continue                                   # (the CoM's rows are not a foot's)
            elif what == "other side":
                if g == 1 and t > 0:
                    least[what] = min(least.get(what, np.inf), moved); assert moved > 1.0, (i, what, moved)
            elif g < 3 and _active(t, g):
                least[what] = min(least.get(what, np.inf), moved); assert moved > 1.0, (i, what, moved)
    print("least movement in units of 1e6 x the GPU tolerance: " + ", ".join("%s %.1f" % kv for kv in least.items()))
    assert len(least) == 6
    # the other families ride along inactive under each of their bound sources; the infinite sides carry multipliers and stay finite
    for i in (0, 31, 59):
        for jrec in (rec[i], br.default_record(tc.STAGE_MARGIN)):
            ck, gx, hx, gu, hu = br.traj_terms(X[i], U[i], mu_j[i], mu_c[i], rho[i, :2], jrec)
            assert not gx.any() and not hx.any() and not gu.any() and not hu.any() and ck.sum() < 0.0
        sk, sg, sh = sr.traj_terms(X[i], mu_s[i], rho[i, 2], srec[i])
        assert not sg.any() and not sh.any() and sk.sum() < 0.0
    for i, (other, s_) in inf.items():
        assert np.isinf(win[i, :, 9 * s_ + other]).all() and mu_t[i, 1:, other, s_].all()
        assert all(np.isfinite(a).all() for a in base[i])


def test_reference_driver_meets_the_end_to_end_conditions():
    """The conditions test_gpu_al_task.py's end-to-end case relies on, on the restatement alone."""
    al = tc.AL_E2E
    prob, x0, ui, win, info = tc.end_to_end()
    assert al["rounds"] <= 8 and info["left_below"] > 10 * al["tol_task"], info
    assert info["viol0"][0] >= 9 * al["tol_task"] and info["viol0"][1] >= 9 * al["tol_task"] and info["viol0"][2] == 0.0, info      # (far more than tol_task)
    assert abs(info["viol0"][0] - tc.FOOT_LIFT[0]) < 1e-12 and abs(info["viol0"][1] - tc.FOOT_LIFT[1]) < 1e-12
    assert np.isinf(win[2]).all() and np.count_nonzero(np.isfinite(win[0, 0])) == 1 and np.count_nonzero(np.isfinite(win[1, 0])) == 2
    assert (prob["stance"][:, :, 0] == 1).all() and (prob["stance"][:, :, 1] == 0).all()
    for early_exit in (True, False):
        sol, free = tc.reference_solves(early_exit), tc.free_solves(early_exit)
        for b in range(3):
            s = sol[b]
            assert s["done"], (early_exit, b, s["viol"])
            assert s["viol"][0] <= al["tol_joint"] and s["viol"][1] <= al["tol_ctrl"] and s["viol"][3] <= al["tol_task"], (b, s["viol"])
            assert tr.violation(s["X"], win[b], prob["stance"][b]) == s["viol"][3]
            v = s["task_trace"][:, 0]; v = v[~np.isnan(v)]
            assert (np.diff(v) <= 0.0).all(), (b, v)      # viol_task falls round over round
        assert sol[0]["mu_t"][:, 8, 0].max() > 0.0 and sol[1]["mu_t"][:, 8, 0].max() > 0.0 and not sol[1]["mu_t"][:, 3:6].any() and not sol[2]["mu_t"].any()
        # the bounded foot ends within tol_task of its floor where the free solve leaves it below
        for b in range(2):
            assert tr.points(sol[b]["X"])[1:, 8].min() >= info["z_min"][b] + tc.FOOT_LIFT[b] - al["tol_task"]
            assert tr.points(free[b]["X"])[1:, 8].min() < info["z_min"][b] + tc.FOOT_LIFT[b] - 9 * al["tol_task"]
        # rollout 2, all bounds infinite: the solve without a window, to the bit
        for k in ("X", "U", "mu_j", "mu_c"):
            assert np.array_equal(sol[2][k], free[2][k]), k
        assert np.array_equal(sol[2]["al_trace"], free[2]["al_trace"], equal_nan=True)
    counts = [int((~np.isnan(s["al_trace"][:, 0])).sum()) for s in tc.reference_solves(True)]
    print("rounds run per rollout under the convergence exit:", counts)


def test_plan_with_the_task_family(tmp_path):
    """resolve_al_plan(on, jc, st, tk) over every combination: without a task window its base is resolve_al_plan(on, jc, st) field for field;
    with one, the base is that of the same installation with a window somewhere -- per-knot variant, module, the other families expanded."""
    src = tmp_path / "plan.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "al_plan.h"
using namespace ilqr;
static void dump(const AlPlan& p) {
  std::printf("%d %d%d%d %d%d%d %d%d%d%d", p.variant, (int)p.jc.source, p.jc.shared, p.jc.per_knot, (int)p.st.source, p.st.shared, p.st.per_knot, p.upload_model, p.expand_jc, p.expand_st, p.module);
}
int main() {
  const AlInstalled opts[5] = {{0, false}, {1, false}, {3, false}, {1, true}, {3, true}};
  int bad = 0;
  for (int on = 0; on < 2; ++on) for (const auto& jc : opts) for (const auto& st : opts) for (int tk = 0; tk < 3; ++tk) {
    const AlInstalled t{tk == 0 ? 0 : tk == 1 ? 1 : 3, true};
    const AlTaskPlan p = resolve_al_plan(on, jc, st, t);
    const AlPlan b = resolve_al_plan(on, jc, st);
    const bool task = on && tk > 0;
    if (p.task != task) ++bad;
    if (!task) { if (std::memcmp(&p.base, &b, sizeof b) || p.tk.source != AL_SRC_NONE) ++bad; continue; }
    if (p.tk.source != AL_SRC_WINDOW || p.tk.shared != (tk == 1) || !p.tk.per_knot) ++bad;
    if (!p.base.module || !p.base.jc.per_knot || (st.sets > 0 && !p.base.st.per_knot)) ++bad;
    if (p.base.variant != (st.sets > 0 ? h1::AL_KNOT_TABLE_STATE : h1::AL_KNOT_TABLE)) ++bad;
    const AlSource wj = (jc.sets > 0 && jc.window) ? AL_SRC_WINDOW : jc.sets > 0 ? AL_SRC_TABLE_EXPANDED : AL_SRC_MODEL_EXPANDED;
    const AlSource ws = st.sets == 0 ? AL_SRC_NONE : st.window ? AL_SRC_WINDOW : AL_SRC_TABLE_EXPANDED;
    if (p.base.jc.source != wj || p.base.st.source != ws) ++bad;
    if (p.base.expand_jc != (wj != AL_SRC_WINDOW) || p.base.expand_st != (ws == AL_SRC_TABLE_EXPANDED) || p.base.upload_model != (wj == AL_SRC_MODEL_EXPANDED)) ++bad;
    // a window of another family installed already: the task family changes nothing in the base
    if ((jc.sets > 0 && jc.window) || (st.sets > 0 && st.window)) { if (std::memcmp(&p.base, &b, sizeof b)) ++bad; }
  }
  std::printf("%d\n", bad);
  return bad != 0;
}
''')
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout


def test_entry_points_without_a_handle():
    import ctypes as C
    import test_capi_cpu as tcc
    sv, L = tcc._lib()
    d = C.c_double
    ok = (C.c_double * 18)(*tr.NO_BOUNDS)
    assert L.ilqr_hip_set_al_task_bounds(None, ok, 1, d(1.0), d(1e-3)) == 1      # ILQR_ERR_ARG
    assert L.ilqr_hip_set_al_task_bounds(None, None, 1, d(1.0), d(1e-3)) == 1
    assert L.ilqr_hip_clear_al_task_bounds(None) == 1
    assert L.ilqr_hip_num_al_task_bound_sets(None) == -1
    for name in ("ilqr_hip_get_al_task_bounds", "ilqr_hip_get_al_task_multipliers", "ilqr_hip_get_al_task_penalties", "ilqr_hip_get_al_task_violation",
                 "ilqr_hip_get_al_task_trace", "ilqr_hip_get_al_task_points"):
        assert getattr(L, name)(None, None) == 1, name
    assert L.ilqr_hip_set_al_task_multipliers(None, None, None) == 1
    assert sv.AL_TASK_BOUNDS == 18 and sv.AL_TASK_COORDS == 9


def test_scenario_helper_shapes_and_refusals():
    st = tc.sc.stack_al_task_bounds
    N = 4
    t = st(dict(), 5, N)
    assert t.shape == (1, N + 1, 18) and np.array_equal(t[0], np.tile(tr.NO_BOUNDS, (N + 1, 1)))
    rows = np.arange(15.0).reshape(N + 1, 3)
    t = st([dict(com=(-1.0, [1.0, 2.0, 3.0]), com_xy=((-0.1, -0.2), (0.3, 0.4))), dict(left_foot=(rows, rows + 1.0), swing_clearance=0.03),
            dict(right_foot=((-np.inf, -np.inf, 0.05), np.inf))], 3, N)
    assert t.shape == (3, N + 1, 18)
    assert list(t[0, 2, :3]) == [-0.1, -0.2, -1.0] and list(t[0, 2, 9:12]) == [0.3, 0.4, 3.0] and np.isinf(t[0, :, 3:9]).all() and np.isinf(t[0, :, 12:]).all()
    assert np.array_equal(t[1, :, 3:5], rows[:, :2]) and (t[1, :, 5] == 0.03).all() and (t[1, :, 8] == 0.03).all() and np.array_equal(t[1, :, 12:15], rows + 1.0)
    assert np.isinf(t[1, :, 6:8]).all() and np.isinf(t[1, :, :3]).all()
    assert (t[2, :, 8] == 0.05).all() and np.isinf(np.delete(t[2], 8, axis=1)).all()
    for bad in (dict(pelvis=(0, 1)), dict(com=(0.0,)), dict(com=([0, 0], 1.0)), dict(left_foot=(np.zeros((N, 3)), 1.0)), dict(com=(1.0, 0.5)),
                dict(com=(np.inf, np.inf)), dict(right_foot=(-np.inf, -np.inf)), dict(com=(np.nan, 1.0)), dict(swing_clearance=[0.1, 0.2]),
                dict(com_xy=(0.0, 1.0)), dict(com_xy=((1.0, 0.0), (0.0, 1.0))), dict(com=3.0)):
        with pytest.raises(ValueError):
            st(bad, 1, N)
    with pytest.raises(ValueError):
        st([dict(), dict()], 3, N)
    with pytest.raises(ValueError):
        st(["com"], 1, N)
    with pytest.raises(ValueError):
        st(dict(), 0, N)


def test_declarations():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    names = ("ilqr_hip_set_al_task_bounds", "ilqr_hip_clear_al_task_bounds", "ilqr_hip_num_al_task_bound_sets", "ilqr_hip_get_al_task_bounds",
             "ilqr_hip_get_al_task_multipliers", "ilqr_hip_set_al_task_multipliers", "ilqr_hip_get_al_task_penalties", "ilqr_hip_get_al_task_violation",
             "ilqr_hip_get_al_task_trace", "ilqr_hip_get_al_task_points")
    for n in names:
        assert re.search(r"^int " + n + r"\(", hdr, re.M), n
        assert n in sv.EXPORTS, n
    assert re.search(r"^#define ILQR_AL_TASK_COORDS 9$", hdr, re.M) and re.search(r"^#define ILQR_AL_TASK_BOUNDS 18$", hdr, re.M)
    assert "int ilqr_hip_set_al_task_bounds(ilqr_hip_ctx* ctx, const double* bounds /*[n_sets][N+1][18]*/, int n_sets, double rho_task0, double tol_task);" in hdr
    for n in ("set_al_task_bounds", "clear_al_task_bounds", "al_task_bounds", "al_task_multipliers", "set_al_task_multipliers", "al_task_penalties",
              "al_task_violation", "al_task_trace", "al_task_points"):
        assert callable(getattr(sv.BatchedILQR, n)), n
