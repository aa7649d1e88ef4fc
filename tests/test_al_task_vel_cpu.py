"""CPU checks of the restatement of the task-velocity family of the augmented-Lagrangian limits (tests/al_task_vel_ref.py) the GPU tests
compare against, and of the inputs they use (tests/al_task_vel_cases.py): the dump program anchored to the oracle, the composed Jacobians
and second-order sums against their own redundancy (two weights) and the term against central differences of itself, known answers (a
switched-off side, a swing knot, knot 0, the terminal knot), proof that the stage inputs discriminate, the reference driver on the
end-to-end inputs, the window builder, and -- the part the library has so far -- the velocity getter's check that needs no handle and its
declarations (a handle needs a GPU: test_gpu_al_task_vel.py).  The family itself is not in the library yet; these tests keep its
reference and its inputs sound for the change that adds it."""
import os
import re

import numpy as np
import pytest

import al_bounds_ref as br
import al_state_ref as sr
import al_task_ref as tr
import al_task_vel_cases as vc
import al_task_vel_ref as vr
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the quadratics carry the reference's slot convention: the derivative with respect to the quaternion's (x, y, z, w) sits in the slots 3..6,
# whose state entries are (w, x, y, z).  PERM[slot] = the state entry the slot's derivative is taken along.
PERM = np.arange(51); PERM[3:7] = [4, 5, 6, 3]


def _active(t, g):
    return g < 2 and not (t == 0 and g > 0)


def test_dump_program_is_anchored_to_the_oracle():
    """tests/cpp/al_task_vel_dump.cpp against Oracle.knot_quadratics: with target 0 and weight w on a stance foot its (lx, lxx) are the
    one-knot oracle's with only w_ee_vel = w on (the other foot swinging); on the CoM set with a reference its (lx, lxx) are the oracle's
    with only w_com_vel = w on.  Same arithmetic (the oracle's own functions, no contraction on either side): bounded at 1e-14 relative to
    the largest entry, the figure is printed."""
    R = vc.regimes()
    X, V = R["X"], R["V"]
    worst = 0.0
    for w in (1.0, 8.0):
        for foot in (0, 1):
            stance = np.zeros((2, 2), dtype=np.int32); stance[:, foot] = 1
            p = dict(vc.sc.make_problem(ol.reference_kinematics, N=1, stance=stance))
            p["Q"] = np.zeros(51); p["Qf"] = np.zeros(51); p["R"] = np.zeros(19)
            p["task_weights"] = (0.0, 0.0, 0.0, w, 0.0, 0.0); p["w_joint"] = 0.0; p["w_ctrl"] = 0.0
            o = ol.Oracle(1, p["dt"]); o.set_problem(p)
            for i in (0, 17, 41):
                x = X[i, 2]
                lx, _, lxx, _ = o.knot_quadratics(0, x, None, 0)
                v, g, H = vr.vel_terms([1 + foot], w, x[None], np.zeros((1, 3)))
                assert np.abs(lx).max() > 0.0 and np.abs(lxx).max() > 0.0
                worst = max(worst, np.abs(g[0] - lx).max() / np.abs(lx).max(), np.abs(H[0] - lxx).max() / np.abs(lxx).max())
                assert np.abs(v[0] - V[i, 2, 3 + 3 * foot:6 + 3 * foot]).max() == 0.0
        k = vr.Kin(w)
        for i in (5, 33):
            x, ref = X[i, 1], V[i, 1, :3] - np.array([0.3, -0.2, 0.1])
            lx, lxx = k._com(x, ref)
            v, g, H = vr.vel_terms([0], w, x[None], ref[None])
            worst = max(worst, np.abs(g[0] - lx).max() / np.abs(lx).max(), np.abs(H[0] - lxx).max() / np.abs(lxx).max())
    print("dump program against the oracle, relative to the largest entry: %.2e" % worst)
    assert worst <= 1e-14


def test_composed_reference_against_its_own_redundancy():
    """The Jacobian rows and the second-order sums composed from the oracle's velocity terms under two weights w = 1 and w = 8: printed, and
    bounded at 1e-12 relative to the largest entry -- a hundredth of the task family's GPU tolerance of 1e-10, which a GPU test of this family
    would take over."""
    R = vc.regimes()
    X, V, mu_v, rho, win, stance, cases = R["X"], R["V"], R["mu_v"], R["rho"], R["win"], R["stance"], R["cases"]
    worst = dict(J=0.0, C=0.0)
    for i, (k, side, t, g) in enumerate(cases):
        m, _ = vr.m_and_scale(V[i, t], win[i, t], stance[i, t], mu_v[i, t], rho[i, 4])
        J1, J8 = vr.kin(1.0).jacobian(X[i, t], V[i, t]), vr.kin(8.0).jacobian(X[i, t], V[i, t])
        worst["J"] = max(worst["J"], np.abs(J1 - J8).max() / np.abs(J1).max())
        if m.any():
            C1, C8 = vr.kin(1.0).curvature(X[i, t], m, V[i, t]), vr.kin(8.0).curvature(X[i, t], m, V[i, t])
            worst["C"] = max(worst["C"], np.abs(C1 - C8).max() / np.abs(C1).max())
    print("two weights, relative to the largest entry: Jacobian %.2e, second-order sum %.2e" % (worst["J"], worst["C"]))
    assert worst["J"] <= 1e-12 and worst["C"] <= 1e-12


def test_term_against_central_differences_of_itself():
    """Gradient and Hessian of the restated term at the excited knot of every regime case against central differences of its own phi / of
    its own gradient, step h = 1e-6 in every state entry.  The term is (rho / 2) c^2 + ... with rho ~ 6e4 .. 1.4e5, |J| <= ~1 and second
    derivatives of the velocities of O(1): the same error budget as al_task_ref's test (rounding ~1e-9 / 4e-8, truncation ~1e-6 relative):
    bound 1e-6 relative to the largest entry, and every regime keeps |mu + rho c| >= 100 off the kink while a step moves it by
    rho |J| h ~ 0.1."""
    R = vc.regimes()
    X, mu_v, rho, win, stance, cases = R["X"], R["mu_v"], R["rho"], R["win"], R["stance"], R["cases"]
    h = 1e-6
    worst = dict(g=0.0, H=0.0, gmax=0.0, Hmax=0.0)
    seen = set()
    for i, (k, side, t, g) in enumerate(cases):
        x, w, st, mu, r = X[i, t], win[i, t], stance[i, t], mu_v[i, t], rho[i, 4]

        def f(v):
            return float(vr.phi(vr.velocities(v), w, st, mu, r).sum())

        def grad(v):
            return vr.traj_terms(v[None], mu[None], r, w[None], st[None])[1][0]

        _, gx, hxx = vr.traj_terms(x[None], mu[None], r, w[None], st[None])
        gx, hxx = gx[0], hxx[0]
        if g == 3 or not _active(t, g):
            assert not gx.any() and not hxx.any(), (i, cases[i])      # the constant only (a swing knot; an inactive regime; knot 0 inside)
            continue
        seen.add((side, g))
        s = (mu + r * vr.constraints(vr.velocities(x), w, st))[k, side]
        assert s > 100.0, (i, s)
        if i % 2:                                            # (every other active case: the differences cost 200 evaluations each)
            continue
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


def test_known_answers_switched_off_side_swing_knot_knot_0_and_terminal_knot():
    R = vc.regimes()
    N = vc.N_STAGE
    Xb = np.array(R["X"][0]); V = vr.velocities(Xb)
    stance = np.ones((N + 1, 2), dtype=np.int32); stance[2, 1] = 0
    win = np.tile(vr.NO_BOUNDS, (N + 1, 1))
    win[:, 9 + 2] = V[:, 2] + 1.0                          # CoM v_z <= 1 above it: inactive, lower side off with a multiplier
    win[:, 9 + 8] = V[:, 8] - 0.01                         # the right ankle 1 cm/s faster upwards than allowed at every knot
    mu = np.zeros((N + 1, 9, 2)); mu[1:, 2, 0] = 3.0
    rho = 50.0
    ck, gx, hxx = vr.traj_terms(Xb, mu, rho, win, stance)
    want = 0.5 * rho * 1e-4
    # the switched-off side: -mu^2 / (2 rho) per knot; the swing knot 2: no term of the foot, no gradient, no curvature; the terminal knot counts
    assert abs(ck[0] - want) < 1e-12 and abs(ck[1] - (want - 9.0 / 100.0)) < 1e-12 and ck[2] == -9.0 / 100.0 and abs(ck[N] - (want - 9.0 / 100.0)) < 1e-12
    assert gx[1].any() and hxx[1].any() and not gx[2].any() and not hxx[2].any() and gx[N].any() and hxx[N].any()
    nv, viol = vr.update_taskvel(Xb, mu, rho, win, stance)
    assert not nv[:, 2].any() and not nv[0].any() and not nv[2].any() and abs(viol - 0.01) < 1e-12
    assert abs(nv[1, 8, 1] - rho * 0.01) < 1e-9 and abs(nv[N, 8, 1] - rho * 0.01) < 1e-9 and abs(vr.violation(Xb, win, stance) - 0.01) < 1e-12
    # violated at knot 0 only, or at a swing knot only: no violation, nothing to update; at knot N only (a CoM row): a violation
    only0 = np.tile(vr.NO_BOUNDS, (N + 1, 1)); only0[0, 9 + 0] = V[0, 0] - 0.05
    only_sw = np.tile(vr.NO_BOUNDS, (N + 1, 1)); only_sw[2, 6] = V[2, 6] + 0.05
    onlyN = np.tile(vr.NO_BOUNDS, (N + 1, 1)); onlyN[N, 1] = V[N, 1] + 0.05
    for w in (only0, only_sw):
        nv, viol = vr.update_taskvel(Xb, np.zeros_like(mu), rho, w, stance)
        assert viol == 0.0 and not nv.any()
    nv, viol = vr.update_taskvel(Xb, np.zeros_like(mu), rho, onlyN, stance)
    assert abs(viol - 0.05) < 1e-12 and abs(nv[N, 1, 0] - rho * 0.05) < 1e-9 and np.count_nonzero(nv) == 1
    assert vr.traj_terms(Xb, np.zeros_like(mu), rho, only0, stance)[0][0] > 0.0      # knot 0 carries the cost term
    assert vr.update_taskvel(Xb, np.zeros_like(mu), rho, only_sw, np.ones_like(stance))[1] > 0.0      # (the same row with the foot standing)
    assert np.array_equal(vr.shift(np.arange(90.0).reshape(5, 9, 2), 1)[1:4], np.arange(90.0).reshape(5, 9, 2)[2:5])
    # the swing rule is the complement of the task family's stance rule
    st = np.array([[1, 0], [0, 1], [2, 1]])
    assert np.array_equal(vr.rows_off(st)[:, 3:], ~tr.rows_off(st)[:, 3:]) and not vr.rows_off(st)[:, :3].any()


def test_stage_inputs_discriminate():
    """Each regime changes the quantity it is meant to change, and reading row t +- 1 of the window, the other foot's rows, the other
    side's multiplier or a neighbouring axis' bounds moves the gradient or the cost of every stage case in which the excited side is
    active by more than 1e6 x the GPU tolerance: 1e-4 max(1, |want|) on lx, want the full expected gradient, or 1e-5 relative on the
    cost.  Ignoring the swing rule (a stance / swing flip of the excited foot) moves the swing cases by as much."""
    R = vc.regimes()
    cases, inf, win, mu_v, stance = R["cases"], R["inf"], R["win"], R["mu_v"], R["stance"]
    B = R["X"].shape[0]
    assert B == 60 and len(set(cases)) == 60 and sum(1 for c in cases if c[3] == 3) == vc.SWING_CASES
    assert sorted({c[2] for c in cases}) == list(range(vc.N_STAGE + 1))
    assert any(c[2] == vc.N_STAGE and c[0] < 3 and c[3] < 3 for c in cases) and any(c[2] == vc.N_STAGE and c[0] >= 3 and c[3] < 3 for c in cases)
    assert len(set(R["rho"][:, 4])) == B
    base = vc.taskvel_terms()
    wrong = {"row t+1": vc.taskvel_terms(shift_row=1), "row t-1": vc.taskvel_terms(shift_row=-1), "other foot": vc.taskvel_terms(swap_feet=True),
             "other side": vc.taskvel_terms(swap_sides=True), "next axis": vc.taskvel_terms(roll_axis=1), "no swing rule": vc.taskvel_terms(use_swing=False)}
    least = {}
    for i, (k, side, t, g) in enumerate(cases):
        want, want_c = vc.stage_expected(i)
        scale_g, scale_c = max(1.0, np.abs(want["lx"]).max()), max(1.0, abs(want_c))
        ck, gx, hxx = base[i]
        # what each regime is meant to change: g = 0 and g = 1 (off knot 0) a gradient and a curvature at the excited knot alone; g = 2 and
        # the swing cases the constant only
        assert np.count_nonzero(np.abs(gx).max(axis=1)) == (1 if (g < 3 and _active(t, g)) else 0), (i, cases[i])
        assert np.count_nonzero(np.abs(hxx).max(axis=(1, 2))) == (1 if (g < 3 and _active(t, g)) else 0), (i, cases[i])
        if g < 3 and _active(t, g):
            assert gx[t].any() and hxx[t].any()
            assert np.abs(gx[t]).max() > 1e-4 * scale_g
        if g in (1, 2, 3) and t > 0:
            assert mu_v[i, t, k, side] > 0.0
        for what, terms in wrong.items():
            ck2, gx2, _ = terms[i]
            moved = max(np.abs(gx2 - gx).max() / scale_g / 1e-4, abs(ck2.sum() - ck.sum()) / scale_c / 1e-5)
            if what == "no swing rule":
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
    # the position window that rides along: active where the docstring of regimes() says, and only there
    pos = vc.position_terms()
    for i, (k, side, t, g) in enumerate(cases):
        ck, gx, hxx = pos[i]
        if g == 3:
            assert not gx.any()
            continue
        tp = t if k < 3 else (t + 2) % (vc.N_STAGE + 1)
        assert np.count_nonzero(np.abs(gx).max(axis=1)) == 1 and gx[tp].any() and hxx[tp].any(), (i, cases[i])
        if k >= 3:
            f = vr.FOOT_OF[k]
            assert stance[i, t, f] == 1 and stance[i, tp, f] == 0
    # the other families ride along inactive under each of their bound sources; the infinite sides carry multipliers and stay finite
    for i in (0, 31, 59):
        for jrec in (R["rec"][i], br.default_record(vc.STAGE_MARGIN)):
            ck, gx, hx, gu, hu = br.traj_terms(R["X"][i], R["U"][i], R["mu_j"][i], R["mu_c"][i], R["rho"][i, :2], jrec)
            assert not gx.any() and not hx.any() and not gu.any() and not hu.any() and ck.sum() < 0.0
        sk, sg, sh = sr.traj_terms(R["X"][i], R["mu_s"][i], R["rho"][i, 2], R["srec"][i])
        assert not sg.any() and not sh.any() and sk.sum() < 0.0
    assert len(inf) == 4
    for i, (other, s_) in inf.items():
        assert np.isinf(win[i, :, 9 * s_ + other]).all() and mu_v[i, 1:, other, s_].all()
        assert all(np.isfinite(a).all() for a in base[i])


def test_reference_driver_meets_the_end_to_end_conditions():
    """The conditions a GPU end-to-end case of this family would rely on, on the restatement alone: the reference driver drives rollouts 0
    and 1 to done within the installed rounds, and the bound is active in the result (a multiplier > 0)."""
    al = vc.AL_E2E
    prob, x0, ui, win, info = vc.end_to_end()
    print("end to end: axis %s, cap %s m/s (fractions %s), right foot over the cap by %.3e m/s, violation of the free solves %s"
          % (info["axis"], info["cap"], vc.CAP_FRACTION, info["right_over"], info["viol0"]))
    assert al["rounds"] <= 8
    assert info["right_over"] > 10 * al["tol_taskvel"], info
    assert info["viol0"][0] >= 9 * al["tol_taskvel"] and info["viol0"][1] >= 9 * al["tol_taskvel"] and info["viol0"][2] == 0.0, info
    for b in range(2):      # (the free solve is over the cap by (1 - fraction) / fraction of it)
        assert abs(info["viol0"][b] - info["cap"][b] * (1.0 - vc.CAP_FRACTION[b]) / vc.CAP_FRACTION[b]) < 1e-12
    assert np.isinf(win[2]).all() and np.count_nonzero(np.isfinite(win[0, 0])) == 2 and np.count_nonzero(np.isfinite(win[1, 0])) == 12
    assert (prob["stance"][:, :, 0] == 1).all() and (prob["stance"][:, :, 1] == 0).all()
    for early_exit in (True, False):
        sol, free = vc.reference_solves(early_exit), vc.free_solves(early_exit)
        for b in range(3):
            s = sol[b]
            assert s["done"], (early_exit, b, s["viol"], s["taskvel_trace"])
            assert s["viol"][0] <= al["tol_joint"] and s["viol"][1] <= al["tol_ctrl"] and s["viol"][4] <= al["tol_taskvel"], (b, s["viol"])
            assert vr.violation(s["X"], win[b], prob["stance"][b]) == s["viol"][4]
        assert sol[0]["mu_v"][:, 3:6].max() > 0.0 and sol[1]["mu_v"][:, 3:6].max() > 0.0 and not sol[1]["mu_v"][:, 6:9].any() and not sol[2]["mu_v"].any()
        # the capped foot ends within tol_taskvel of its cap where the free solve leaves it faster
        for b in range(2):
            rows = slice(3, 6) if b else slice(3 + info["axis"][0], 4 + info["axis"][0])
            assert np.abs(vr.velocities(sol[b]["X"])[1:, rows]).max() <= info["cap"][b] + al["tol_taskvel"]
            assert np.abs(vr.velocities(free[b]["X"])[1:, rows]).max() > info["cap"][b] + 9 * al["tol_taskvel"]
        # rollout 2, all bounds infinite: the solve without a window, to the bit
        for k in ("X", "U", "mu_j", "mu_c"):
            assert np.array_equal(sol[2][k], free[2][k]), k
        assert np.array_equal(sol[2]["al_trace"], free[2]["al_trace"], equal_nan=True)
    counts = [int((~np.isnan(s["al_trace"][:, 0])).sum()) for s in vc.reference_solves(True)]
    print("rounds run per rollout under the convergence exit:", counts)


def test_entry_point_without_a_handle():
    import ctypes as C
    import test_capi_cpu as tcc
    sv, L = tcc._lib()
    assert L.ilqr_hip_get_al_task_velocities(None, None) == 1      # ILQR_ERR_ARG
    assert sv.AL_TASK_VEL_COORDS == 9
    # the kernel lives in the per-knot module, whose table the library resolves through one symbol
    M = C.CDLL(os.path.join(os.path.dirname(sv.LIB_PATH), "libilqr_hip_alknot.so"))
    for name in ("ilqr_alknot_module", "ilqr_alknot_module_task_velocities"):
        assert hasattr(M, name), name


def test_window_builder_shapes_shorthands_and_refusals():
    st = vr.stack_al_task_vel_bounds
    N = 4
    t = st(dict(), 5, N)
    assert t.shape == (1, N + 1, 18) and np.array_equal(t[0], np.tile(vr.NO_BOUNDS, (N + 1, 1)))      # everything left out is infinite
    rows = np.arange(15.0).reshape(N + 1, 3)
    t = st([dict(com_vel=(-1.0, [1.0, 2.0, 3.0]), com_speed_xy=(0.3, 0.4)), dict(left_foot_vel=(rows, rows + 1.0)), dict(stance_slip=0.01),
            dict(right_foot_vel=((-np.inf, -np.inf, -0.3), np.inf), stance_slip=0.0)], 4, N)
    assert t.shape == (4, N + 1, 18)
    assert list(t[0, 2, :3]) == [-0.3, -0.4, -1.0] and list(t[0, 2, 9:12]) == [0.3, 0.4, 3.0] and np.isinf(t[0, :, 3:9]).all() and np.isinf(t[0, :, 12:]).all()
    assert np.array_equal(t[1, :, 3:6], rows) and np.array_equal(t[1, :, 12:15], rows + 1.0) and np.isinf(t[1, :, :3]).all() and np.isinf(t[1, :, 6:9]).all()
    assert (t[2, :, 3:9] == -0.01).all() and (t[2, :, 12:18] == 0.01).all() and np.isinf(t[2, :, :3]).all() and np.isinf(t[2, :, 9:12]).all()
    assert (t[3, :, 3:9] == 0.0).all() and (t[3, :, 12:18] == 0.0).all()                     # the shorthand is applied after the key it refines
    for bad in (dict(pelvis_vel=(0, 1)), dict(com=(0, 1)), dict(com_vel=(0.0,)), dict(com_vel=([0, 0], 1.0)), dict(left_foot_vel=(np.zeros((N, 3)), 1.0)),
                dict(com_vel=(1.0, 0.5)), dict(com_vel=(np.inf, np.inf)), dict(right_foot_vel=(-np.inf, -np.inf)), dict(com_vel=(np.nan, 1.0)),
                dict(stance_slip=[0.1, 0.2]), dict(stance_slip=-0.1), dict(com_speed_xy=1.0), dict(com_speed_xy=(1.0, -1.0)), dict(com_vel=3.0)):
        with pytest.raises(ValueError):
            st(bad, 1, N)
    with pytest.raises(ValueError):
        st([dict(), dict()], 3, N)
    with pytest.raises(ValueError):
        st(["com_vel"], 1, N)
    with pytest.raises(ValueError):
        st(dict(), 0, N)


def test_declarations():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    assert re.search(r"^int ilqr_hip_get_al_task_velocities\(", hdr, re.M) and "ilqr_hip_get_al_task_velocities" in sv.EXPORTS
    assert re.search(r"^#define ILQR_AL_TASK_VEL_COORDS 9$", hdr, re.M)
    assert "int ilqr_hip_get_al_task_velocities(ilqr_hip_ctx* ctx, double* out /*[B][N+1][9]*/);" in hdr
    assert callable(sv.BatchedILQR.al_task_velocities)
