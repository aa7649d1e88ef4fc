"""CPU checks of the augmented-Lagrangian restatement (tests/al_ref.py) the GPU tests compare against, and of the inputs they use
(tests/al_cases.py): the NumPy term against central differences of itself in its three regimes, against the plain penalty at zero
multipliers, the reference driver on the end-to-end inputs, and the entry points' null-handle checks (a handle needs a GPU: the range
checks of the setter are in test_gpu_augmented_lagrangian.py)."""
import numpy as np

import al_cases as ac
import al_ref as ar
import cost_envelope_cases as cc


def test_term_against_central_differences_of_itself():
    """gradient and diagonal Hessian of the NumPy term in the three regimes, both margins, both families: O(eps^2) central differences of
    phi / of grad with eps = 1e-6 relative to the range (phi is piecewise quadratic: the differences are exact up to rounding away
    from the kink, and every regime keeps |mu + rho c| >= 0.5 rho 0.02 range from it)."""
    jr, cr = ar.ranges()
    seen = set()
    for m in (0.0, 0.1):
        X, U, mu_j, mu_c, rho, cases = ac.regimes(m)
        for i, (kind, j, side, t, g) in enumerate(cases):
            table, val, mu, r = (jr, X[i, t, 7:26], mu_j[i, t], rho[i, 0]) if kind == "joint" else (cr, U[i, t], mu_c[i, t], rho[i, 1])
            eps = 1e-6 * (table[j, 1] - table[j, 0])
            e = np.zeros(19); e[j] = eps
            f = lambda v: ar.phi(v, table, mu, r, m).sum()
            g_fd = (f(val + e) - f(val - e)) / (2 * eps)
            h_fd = (ar.grad(val + e, table, mu, r, m)[j] - ar.grad(val - e, table, mu, r, m)[j]) / (2 * eps)
            g_, h_ = ar.grad(val, table, mu, r, m)[j], ar.hess(val, table, mu, r, m)[j]
            s = (mu + r * ar.constraints(val, table, m))[j, side]
            if kind == "joint" and t == 0 and g > 0:
                assert g_ == 0.0 and h_ == 0.0           # knot 0 keeps a zero multiplier: inside the bound nothing is active
            else:
                assert (s > 0) == (g < 2), (i, s)
                seen.add((kind, side, g))
                assert (g_ != 0.0) == (g < 2) and (h_ == r) == (g < 2) and (g < 2 or h_ == 0.0), (i, g_, h_)
                if g == 2:
                    assert ar.phi(val, table, mu, r, m)[j, side] == -mu[j, side] ** 2 / (2 * r)
            assert abs(g_fd - g_) <= 1e-6 * max(1.0, abs(g_)), (i, g_fd, g_)
            assert abs(h_fd - h_) <= 1e-6 * max(1.0, abs(h_)), (i, h_fd, h_)
    assert len(seen) == 12


def test_zero_multipliers_are_the_plain_penalty():
    """mu = 0, rho = 2 w, m = 0.1: phi, its gradient and its Hessian are pen / pen_grad / pen_hess (a handful of roundings apart)"""
    jr, cr = ar.ranges()
    X, U, _, _, _, _ = ac.regimes(0.1)
    z = np.zeros((19, 2))
    for table, vals, w in ((jr, X[:, :, 7:26].reshape(-1, 19), 1300.0), (cr, U.reshape(-1, 19), 1700.0)):
        hit = 0
        for v in vals:
            want = cc.pen(v, table, w)
            got = ar.phi(v, table, z, 2 * w, 0.1).sum()
            assert abs(got - want) <= 1e-13 * max(1.0, abs(want))
            assert np.abs(ar.grad(v, table, z, 2 * w, 0.1) - cc.pen_grad(v, table, w)).max() <= 1e-13 * max(1.0, np.abs(cc.pen_grad(v, table, w)).max())
            assert np.array_equal(ar.hess(v, table, z, 2 * w, 0.1), cc.pen_hess(v, table, w))
            hit += want > 0
        assert hit >= 38        # every rollout in regime 0 of this family


def test_update_and_shift_rules():
    jr, cr = ar.ranges()
    N = 4
    X = np.tile(cc.sweep_base_state(), (N + 1, 1)); U = np.zeros((N, 19))
    X[0, 7] = jr[0, 1] + 0.2                      # knot 0 alone violates: done, multipliers stay zero
    mj, mc = np.zeros((N + 1, 19, 2)), np.zeros((N, 19, 2))
    nj, nc, rho, done, viol = ar.update(X, U, mj, mc, (10.0, 20.0), False, 0.0, 10.0, (1e3, 1e3), (1e-3, 1e-2))
    assert done and viol == (0.0, 0.0) and not nj.any() and not nc.any() and rho == (10.0, 20.0)
    X[2, 7 + 3] = jr[3, 0] - 0.1; U[1, 5] = cr[5, 1] + 2.0
    nj, nc, rho, done, viol = ar.update(X, U, mj, mc, (500.0, 20.0), False, 0.0, 10.0, (1e3, 1e3), (1e-3, 1e-2))
    assert not done and abs(viol[0] - 0.1) < 1e-15 and viol[1] == 2.0 and rho == (1e3, 200.0)
    assert np.count_nonzero(nj) == 1 and abs(nj[2, 3, 0] - 50.0) < 1e-12 and np.count_nonzero(nc) == 1 and nc[1, 5, 1] == 40.0
    sj, scc = ar.shift(nj, nc, 1)
    assert np.count_nonzero(sj) == 1 and sj[1, 3, 0] == nj[2, 3, 0] and np.count_nonzero(scc) == 1 and scc[0, 5, 1] == 40.0
    sj, scc = ar.shift(nj, nc, 2)
    assert not sj.any() and not scc.any()          # hinge knot 2 would land on knot 0, actuator knot 1 before it


def test_reference_driver_meets_the_end_to_end_conditions():
    """Under the plain penalties at the shipped weights the reference's solve leaves rollouts 1 and 2 violating the hard range by more than
    10 tol; under AL their violation after the last round is <= tol, and rollout 0 has every multiplier zero."""
    al = ac.AL_E2E
    for early_exit in (True, False):
        sol, plain = ac.reference_solves(early_exit)
        pj = [ar.hard_violation(p["X"], p["U"]) for p in plain]
        assert pj[0] == (0.0, 0.0)
        assert pj[1][1] > 10 * al["tol_ctrl"] and pj[2][0] > 10 * al["tol_joint"], pj
        for b in range(3):
            assert sol[b]["viol"][0] <= al["tol_joint"] and sol[b]["viol"][1] <= al["tol_ctrl"], (b, sol[b]["viol"])
            assert sol[b]["done"]
            assert ar.hard_violation(sol[b]["X"], sol[b]["U"]) == sol[b]["viol"]
        assert not sol[0]["mu_j"].any() and not sol[0]["mu_c"].any()
        assert sol[1]["al_trace"][0, 1] > 10 * al["tol_ctrl"] and sol[2]["al_trace"][0, 0] > 10 * al["tol_joint"]      # the first round alone does not do it
        assert sol[2]["mu_j"].max() > 0.0


def test_entry_points_check_a_null_handle():
    import test_capi_cpu as tc
    sv, L = tc._lib()
    import ctypes as C
    d = C.c_double
    assert L.ilqr_hip_set_augmented_lagrangian(None, 3, d(1.0), d(1.0), d(10.0), d(100.0), d(0.0), d(1e-3), d(1e-2)) == 1      # ILQR_ERR_ARG
    assert L.ilqr_hip_clear_augmented_lagrangian(None) == 1
    assert L.ilqr_hip_augmented_lagrangian_rounds(None) == -1
    for name in ("ilqr_hip_get_al_multipliers", "ilqr_hip_get_al_violation"):
        assert getattr(L, name)(None, None, None) == 1
    assert L.ilqr_hip_set_al_multipliers(None, None, None, None) == 1
    assert L.ilqr_hip_get_al_trace(None, None) == 1 and L.ilqr_hip_get_al_penalties(None, None) == 1 and L.ilqr_hip_al_update(None, 0) == 1
