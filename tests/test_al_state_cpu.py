"""CPU checks of the restatement of the state family of the augmented-Lagrangian limits (tests/al_state_ref.py) the GPU tests compare
against, and of the inputs they use (tests/al_state_cases.py): the NumPy term against central differences of itself in its three regimes,
known answers (a switched-off side, knot 0, a rollout done on joints but not on the state family), proof that the stage inputs
discriminate, the reference driver on the end-to-end inputs, the entry points' checks that need no handle, the scenario helper and the
declarations (a handle needs a GPU: the range checks of the setter are in test_gpu_al_state.py)."""
import os
import re

import numpy as np
import pytest

import al_bounds_ref as br
import al_cases as ac
import al_state_cases as sc_
import al_state_ref as sr
import cost_envelope_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slots_and_term_against_central_differences_of_itself():
    """gradient and curvature of the NumPy term in the three regimes, every coordinate and side: O(eps^2) central differences of phi / of
    grad with eps = 1e-6 of the box width (phi is piecewise quadratic and every regime keeps |mu + rho c| >= 0.5 rho 0.02 width off the kink)"""
    assert list(sr.SLOTS) == [0, 1, 2] + list(range(26, 51))
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, inf = sc_.regimes()
    assert X.shape == (168, 5, 51) and len(cases) == 168 and len(set(cases)) == 168
    seen = set()
    for i, (k, side, t, g) in enumerate(cases):
        lo, hi = sr.split(srec[i]); w = hi[k] - lo[k]
        assert np.isfinite(w)
        eps = 1e-6 * w
        x = X[i, t].copy(); e = np.zeros(51); e[sr.SLOTS[k]] = eps
        r, mu = rho[i, 2], mu_s[i, t]
        f = lambda v: sr.phi(v, srec[i], mu, r).sum()
        g_fd = (f(x + e) - f(x - e)) / (2 * eps)
        h_fd = (sr.grad(x + e, srec[i], mu, r)[k] - sr.grad(x - e, srec[i], mu, r)[k]) / (2 * eps)
        g_, h_ = sr.grad(x, srec[i], mu, r)[k], sr.hess(x, srec[i], mu, r)[k]
        s = (mu + r * sr.constraints(x, srec[i]))[k, side]
        if t == 0 and g > 0:
            assert g_ == 0.0 and h_ == 0.0               # knot 0 keeps a zero multiplier: inside the bound nothing is active
        else:
            assert (s > 0) == (g < 2), (i, s)
            seen.add((side, g))
            assert (g_ != 0.0) == (g < 2) and (h_ == r) == (g < 2) and (g < 2 or h_ == 0.0), (i, g_, h_)
            if g < 2:
                assert (g_ > 0) == bool(side)            # the sign of its side
            if g == 2:
                assert sr.phi(x, srec[i], mu, r)[k, side] == -mu[k, side] ** 2 / (2 * r)
        assert abs(g_fd - g_) <= 1e-6 * max(1.0, abs(g_)), (i, g_fd, g_)
        assert abs(h_fd - h_) <= 1e-6 * max(1.0, abs(h_)), (i, h_fd, h_)
        # every other constraint of the rollout is inactive: the gradient and the curvature have this one entry at most
        G, H = sr.grad(X[i], srec[i], mu_s[i], r), sr.hess(X[i], srec[i], mu_s[i], r)
        assert np.count_nonzero(G) == np.count_nonzero(H) == (1 if (g < 2 and not (t == 0 and g > 0)) else 0), (i, np.count_nonzero(G))
    assert len(seen) == 6
    # the joint / torque family rides along inactive under both of its bound sources
    for i in (0, 83, 167):
        for jrec in (rec[i], br.default_record(sc_.STAGE_MARGIN)):
            ck, gx, hx, gu, hu = br.traj_terms(X[i], U[i], mu_j[i], mu_c[i], rho[i, :2], jrec)
            assert not gx.any() and not hx.any() and not gu.any() and not hu.any() and ck.sum() < 0.0


def test_known_answers_switched_off_side_knot_0_and_the_done_rule():
    N = 4
    X = np.tile(cc.sweep_base_state(), (N + 1, 1)); U = np.zeros((N, 19))
    X[:, 32:51] = 0.0
    jrec = br.default_record(0.0)
    srec = sr.NO_BOUNDS.copy()
    srec[9 + 4] = -1.0; srec[28 + 9 + 4] = 1.0           # joint 4: |qdot| <= 1
    srec[28 + 2] = 2.0                                   # pelvis z <= 2, its lower side off
    mu = np.zeros((N + 1, 28, 2)); mu[1:, 2, 0] = 3.0    # a multiplier on the switched-off side
    rho3, rmax, tol = (10.0, 20.0, 50.0), (1e3, 1e3, 200.0), (1e-3, 1e-2, 1e-3)
    # the switched-off side: the constant -mu^2 / (2 rho) per knot, no gradient, no curvature, no violation, multiplier driven to zero
    ck, g, h = sr.traj_terms(X, mu, 50.0, srec)
    assert np.array_equal(ck, np.array([0.0] + [-9.0 / 100.0] * N)) and not g.any() and not h.any()
    nj, nc, ns, r2, done, viol = sr.update(X, U, np.zeros((N + 1, 19, 2)), np.zeros((N, 19, 2)), mu, rho3, False, jrec, srec, 10.0, rmax, tol)
    assert done and viol == (0.0, 0.0, 0.0) and not ns.any() and r2 == rho3
    # knot 0 alone violates: it carries the cost term, keeps a zero multiplier and is left out of the violation
    X[0, 32 + 4] = 1.5
    ck, g, h = sr.traj_terms(X, np.zeros_like(mu), 50.0, srec)
    assert ck[0] == 0.5 * 50.0 * 0.25 and g[0, 9 + 4] == 25.0 and h[0, 9 + 4] == 50.0 and not ck[1:].any()
    nj, nc, ns, r2, done, viol = sr.update(X, U, np.zeros((N + 1, 19, 2)), np.zeros((N, 19, 2)), np.zeros_like(mu), rho3, False, jrec, srec, 10.0, rmax, tol)
    assert done and viol == (0.0, 0.0, 0.0) and not ns.any()
    # done on joints and torques, not on the state family: not done, ALL three penalties grow (the state one up to its cap)
    X[3, 32 + 4] = -1.25
    nj, nc, ns, r2, done, viol = sr.update(X, U, np.zeros((N + 1, 19, 2)), np.zeros((N, 19, 2)), np.zeros_like(mu), rho3, False, jrec, srec, 10.0, rmax, tol)
    assert not done and viol == (0.0, 0.0, 0.25) and r2 == (100.0, 200.0, 200.0)
    assert np.count_nonzero(ns) == 1 and ns[3, 9 + 4, 0] == 12.5 and not nj.any() and not nc.any()
    # a rollout that was done keeps everything; the shift moves knot 3 to knot 2 / 1 and drops what would land on knot 0
    same = sr.update(X, U, nj, nc, ns, r2, True, jrec, srec, 10.0, rmax, tol)
    assert same[2] is ns and same[3] == r2 and same[4] is True and same[5] == viol
    assert sr.shift(ns, 1)[2, 13, 0] == 12.5 and np.count_nonzero(sr.shift(ns, 1)) == 1 and sr.shift(ns, 2)[1, 13, 0] == 12.5
    assert not sr.shift(ns, 3).any() and not sr.shift(ns, N + 1).any()
    full = np.arange(1.0, 1.0 + (N + 1) * 56).reshape(N + 1, 28, 2); full[0] = 0.0
    s1 = sr.shift(full, 1)
    assert np.array_equal(s1[1:N], full[2:]) and not s1[0].any() and not s1[N].any()


def test_stage_inputs_discriminate():
    """On the restatement alone: with a neighbour's state record, the other side's multiplier or the neighbouring slot, the added gradient,
    curvature or cost of the stage case change by far more than the GPU test's tolerance (1e-10 max(1, |want|); 1e-11 relative on a cost
    of ~1e3)."""
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, inf = sc_.regimes()
    B = X.shape[0]
    wrong_slots = np.roll(sr.SLOTS, 1)
    for i, (k, side, t, g) in enumerate(cases):
        ck, gx, hx = sr.traj_terms(X[i], mu_s[i], rho[i, 2], srec[i])
        for what, (ck2, gx2, hx2) in (("neighbour's record", sr.traj_terms(X[i], mu_s[i], rho[i, 2], srec[(i + 1) % B])),
                                      ("neighbour's multipliers", sr.traj_terms(X[i], mu_s[(i + 1) % B], rho[i, 2], srec[i])),
                                      ("wrong side", sr.traj_terms(X[i], mu_s[i][:, :, ::-1], rho[i, 2], srec[i])),
                                      ("wrong slot", sr.traj_terms(X[i], mu_s[i], rho[i, 2], srec[i], wrong_slots)),
                                      ("neighbour's penalty", sr.traj_terms(X[i], mu_s[i], rho[(i + 1) % B, 2], srec[i]))):
            # A record or a slot shows where a bound is active (g = 0; g = 1 off knot 0) -- an inactive constraint leaves its constant,
            # whatever its bound.  The sides swapped: the sum of mu^2 stays, so the cost moves only where the excited side's own multiplier
            # holds the bound active (g = 1 off knot 0), the gradient wherever a multiplier lands on an active side (off knot 0, which holds none).
            active = g < 2 and not (t == 0 and g > 0)
            dc, dg = abs(ck2.sum() - ck.sum()), np.abs(gx2 - gx).max()
            if what.startswith("neighbour's m") or what.startswith("neighbour's p"):
                assert dc > 1e-6 * max(1.0, abs(ck.sum())), (i, what, dc)
            elif what == "wrong side":
                assert not (t > 0 and g == 1) or dc > 1e-6 * max(1.0, abs(ck.sum())), (i, what, dc)
                assert not (active and t > 0) or dg > 1e-3, (i, what, dg)
            elif active:
                assert dc > 1e-6 * max(1.0, abs(ck.sum())) and dg > 1e-3, (i, what, dc, dg)
    # the wrong slot moves the active entry of lx itself
    i = 3 * (2 * 5 + 1)
    k, side, t, g = cases[i]
    _, gx, _ = sr.traj_terms(X[i], mu_s[i], rho[i, 2], srec[i])
    lx = np.zeros((5, 51)); lx[:, sr.SLOTS] += gx
    assert np.flatnonzero(lx[t]).tolist() == [23 + k] and abs(lx[t, 23 + k]) > 1.0
    # the infinite sides: finite results, and the switched-off side really carries a multiplier
    for i, (other, s_) in inf.items():
        assert np.isinf(srec[i, 28 * s_ + other]) and mu_s[i, 1:, other, s_].all()
        ck, gx, hx = sr.traj_terms(X[i], mu_s[i], rho[i, 2], srec[i])
        assert np.isfinite(ck).all() and np.isfinite(gx).all() and np.isfinite(hx).all()


def test_reference_driver_meets_the_end_to_end_conditions():
    """The conditions test_gpu_al_state.py's end-to-end case relies on, on the restatement alone."""
    al = sc_.AL_E2E
    prob, x0, ui, srec, info = sc_.end_to_end()
    assert al["rounds"] <= 8
    assert info["viol0"][0] >= 10 * al["tol_state"] and info["viol0"][1] >= 10 * al["tol_state"] and info["viol0"][2] == 0.0, info
    assert abs(info["viol0"][0] - 0.5 * info["peak"]) < 1e-15 and abs(info["viol0"][1] - sc_.PELVIS_LIFT) < 1e-12
    assert np.isinf(srec[2]).all() and np.count_nonzero(np.isfinite(srec[0])) == 2 and np.count_nonzero(np.isfinite(srec[1])) == 1
    assert np.isfinite(srec[1, 2]) and np.isfinite(srec[0, [9 + info["joint"], 28 + 9 + info["joint"]]]).all()
    free, _ = ac.reference_solves(True)
    for early_exit in (True, False):
        sol = sc_.reference_solves(early_exit)
        for b in range(3):
            s = sol[b]
            assert s["done"], (early_exit, b, s["viol"])
            assert s["viol"][0] <= al["tol_joint"] and s["viol"][1] <= al["tol_ctrl"] and s["viol"][2] <= al["tol_state"], (b, s["viol"])
            assert sr.violation(s["X"], srec[b]) == s["viol"][2]
        assert sol[0]["mu_s"].max() > 0.0 and sol[1]["mu_s"][:, 2, 0].max() > 0.0 and not sol[2]["mu_s"].any()
        if early_exit:
            counts = [int((~np.isnan(s["al_trace"][:, 0])).sum()) for s in sol]
            assert len(set(counts)) >= 2, counts
            # rollout 2, all bounds infinite: the solve without a table, to the bit
            for k in ("X", "U", "mu_j", "mu_c"):
                assert np.array_equal(sol[2][k], free[2][k]), k
            n = free[2]["al_trace"].shape[0]
            assert np.array_equal(sol[2]["al_trace"][:n], free[2]["al_trace"], equal_nan=True) and np.isnan(sol[2]["al_trace"][n:]).all()
            assert sol[2]["rho"] == free[2]["rho"]


def test_entry_points_without_a_handle():
    import ctypes as C
    import test_capi_cpu as tc
    sv, L = tc._lib()
    d = C.c_double
    ok = (C.c_double * 56)(*sr.NO_BOUNDS)
    assert L.ilqr_hip_set_al_state_bounds(None, ok, 1, d(1.0), d(1e-3)) == 1      # ILQR_ERR_ARG
    assert L.ilqr_hip_set_al_state_bounds(None, None, 1, d(1.0), d(1e-3)) == 1
    assert L.ilqr_hip_clear_al_state_bounds(None) == 1
    assert L.ilqr_hip_num_al_state_bound_sets(None) == -1
    for name in ("ilqr_hip_get_al_state_bounds", "ilqr_hip_get_al_state_multipliers", "ilqr_hip_get_al_state_penalties", "ilqr_hip_get_al_state_violation",
                 "ilqr_hip_get_al_state_trace"):
        assert getattr(L, name)(None, None) == 1, name
    assert L.ilqr_hip_set_al_state_multipliers(None, None, None) == 1
    assert [L.ilqr_hip_al_state_slot(k) for k in range(28)] == list(sr.SLOTS)
    assert [sv.al_state_slot(k) for k in (-1, 28, 1000)] == [-1, -1, -1] and sv.al_state_slot(27) == 50
    assert sv.AL_STATE_BOUNDS == 56 and sv.AL_STATE_COORDS == 28


def test_scenario_helper_shapes_and_refusals():
    st = sc_.sc.stack_al_state_bounds
    t = st(dict(), 5)
    assert t.shape == (1, 56) and np.array_equal(t[0], sr.NO_BOUNDS)
    t = st([dict(pelvis_pos=(-1.0, [1.0, 2.0, 3.0]), pelvis_z=(0.7, np.inf)), dict(pelvis_lin_vel=(-0.5, 0.5), pelvis_ang_vel=([-1, -2, -3], 4.0)),
            dict(joint_vel=(-np.arange(1.0, 20.0), 7.0), joint_speed=np.arange(2.0, 21.0))], 3)
    assert t.shape == (3, 56)
    assert list(t[0, :3]) == [-1.0, -1.0, 0.7] and list(t[0, 28:31]) == [1.0, 2.0, np.inf] and np.isinf(t[0, 3:28]).all()
    assert list(t[1, 3:9]) == [-0.5, -0.5, -0.5, -1.0, -2.0, -3.0] and list(t[1, 31:37]) == [0.5, 0.5, 0.5, 4.0, 4.0, 4.0]
    assert np.array_equal(t[2, 9:28], -np.arange(2.0, 21.0)) and np.array_equal(t[2, 37:56], np.arange(2.0, 21.0))
    assert st(dict(joint_speed=3.0), 2)[0, 9] == -3.0 and st(dict(joint_speed=3.0), 2)[0, 55] == 3.0
    for bad in (dict(pelvis=(0, 1)), dict(pelvis_pos=(0.0,)), dict(pelvis_pos=([0, 0], 1.0)), dict(joint_vel=(np.zeros(18), 1.0)), dict(pelvis_z=(1.0, 0.5)),
                dict(pelvis_z=(np.inf, np.inf)), dict(pelvis_z=(-np.inf, -np.inf)), dict(pelvis_lin_vel=(np.nan, 1.0)), dict(joint_speed=-1.0),
                dict(joint_speed=np.ones(3)), dict(pelvis_pos=3.0)):
        with pytest.raises(ValueError):
            st(bad, 1)
    with pytest.raises(ValueError):
        st([dict(), dict()], 3)
    with pytest.raises(ValueError):
        st(["pelvis_z"], 1)
    with pytest.raises(ValueError):
        st(dict(), 0)


def test_declarations():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    names = ("ilqr_hip_set_al_state_bounds", "ilqr_hip_clear_al_state_bounds", "ilqr_hip_num_al_state_bound_sets", "ilqr_hip_get_al_state_bounds",
             "ilqr_hip_get_al_state_multipliers", "ilqr_hip_set_al_state_multipliers", "ilqr_hip_get_al_state_penalties", "ilqr_hip_get_al_state_violation",
             "ilqr_hip_get_al_state_trace", "ilqr_hip_al_state_slot")
    for n in names:
        assert re.search(r"^int " + n + r"\(", hdr, re.M), n
        assert n in sv.EXPORTS, n
    assert re.search(r"^#define ILQR_AL_STATE_COORDS 28$", hdr, re.M) and re.search(r"^#define ILQR_AL_STATE_BOUNDS 56$", hdr, re.M)
    assert "int ilqr_hip_set_al_state_bounds(ilqr_hip_ctx* ctx, const double* bounds /*[n_sets][56]*/, int n_sets, double rho_state0, double tol_state);" in hdr
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    for n in ("setAlStateBounds", "clearAlStateBounds", "numAlStateBoundSets", "getAlStateBounds", "getAlStateMultipliers", "getAlStateViolation"):
        assert re.search(r"\b" + n + r"\(", hpp), n
    for n in ("set_al_state_bounds", "clear_al_state_bounds", "al_state_bounds", "al_state_multipliers", "set_al_state_multipliers", "al_state_penalties",
              "al_state_violation", "al_state_trace"):
        assert callable(getattr(sv.BatchedILQR, n)), n
