"""CPU checks of the per-rollout bounds table of the augmented-Lagrangian limits (ilqr_hip_set_al_bounds): the host entry point
ilqr_hip_al_default_bounds against al_ref.bounds, the null-handle checks of the new entry points (a handle needs a GPU: the range checks
of the setter are in test_gpu_al_bounds.py), the restatement tests/al_bounds_ref.py against al_ref.py under the default bounds, the
helpers of scenario.py, and the reference driver on the end-to-end inputs of tests/al_bounds_cases.py."""
import ctypes as C

import numpy as np
import pytest

import al_bounds_cases as bc
import al_bounds_ref as br
import al_cases as ac
import al_ref as ar


def _lib():
    import test_capi_cpu as tc
    return tc._lib()


def test_default_bounds_are_al_ref_bounds_bit_for_bit():
    sv, L = _lib()
    jr, cr = ar.ranges()
    for m in (0.0, 0.1, 0.25):
        got = sv.al_default_bounds(m)
        want = np.concatenate(ar.bounds(jr, m) + ar.bounds(cr, m))
        assert got.shape == (76,) and np.array_equal(got, want), (m, np.abs(got - want).max())
        assert np.array_equal(br.default_record(m), want)
    assert np.array_equal(sv.al_default_bounds()[:19], jr[:, 0]) and np.array_equal(sv.al_default_bounds()[57:], cr[:, 1])      # margin 0: the model's ranges
    out = np.zeros(76)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    for bad in (0.5, -0.1, float("nan")):
        assert L.ilqr_hip_al_default_bounds(C.c_double(bad), p) == 1      # ILQR_ERR_ARG
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            sv.al_default_bounds(bad)
    assert L.ilqr_hip_al_default_bounds(C.c_double(0.1), None) == 1
    assert not out.any()


def test_new_entry_points_check_a_null_handle():
    sv, L = _lib()
    rec = np.zeros(76)
    p = rec.ctypes.data_as(C.POINTER(C.c_double))
    assert L.ilqr_hip_set_al_bounds(None, p, 1) == 1      # ILQR_ERR_ARG
    assert L.ilqr_hip_clear_al_bounds(None) == 1
    assert L.ilqr_hip_num_al_bound_sets(None) == -1
    assert L.ilqr_hip_get_al_bounds(None, p) == 1


@pytest.mark.parametrize("m", [0.0, 0.1])
def test_new_reference_reproduces_the_old_under_the_default_bounds(m):
    X, U, mu_j, mu_c, rho, cases = ac.regimes(m)
    rec = br.default_record(m)
    for b in range(X.shape[0]):
        old, new = ar.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b], m), br.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b], rec)
        for a, c in zip(old, new):
            assert np.array_equal(a, c), (b, cases[b])
        for done in (False, True):
            args = (X[b], U[b], mu_j[b], mu_c[b], tuple(rho[b]), done)
            rest = (7.0, (5000.0, 100.0), (1e-3, 1e-2))
            o, n = ar.update(*args, m, *rest), br.update(*args, rec, *rest)
            assert np.array_equal(o[0], n[0]) and np.array_equal(o[1], n[1]) and o[2:] == n[2:], (b, done)
        assert br.violation(X[b], U[b], rec) == o[4]
    # an infinite side: constant term, no gradient, no curvature, no violation, multiplier driven to zero -- and no NaN anywhere
    rec2 = rec.copy(); rec2[19 + 4] = np.inf; rec2[38 + 6] = -np.inf
    b = 17
    with np.errstate(invalid="raise"):
        ck, gx, hx, gu, hu = br.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b], rec2)
        nj, nc, _, _, viol = br.update(X[b], U[b], mu_j[b], mu_c[b], tuple(rho[b]), False, rec2, 7.0, (5000.0, 100.0), (1e-3, 1e-2))
    (jl, jh), (cl, ch) = br.split(rec2)
    t = br.phi(X[b][:, 7:26], jl, jh, mu_j[b], rho[b, 0])
    assert np.array_equal(t[:, 4, 1], -mu_j[b][:, 4, 1] ** 2 / (2 * rho[b, 0])) and mu_j[b][1:, 4, 1].all()
    assert np.all(np.isfinite(ck)) and np.all(np.isfinite(gx)) and np.all(np.isfinite(gu)) and np.isfinite(viol).all()
    assert not nj[:, 4, 1].any() and not nc[:, 6, 0].any() and mu_c[b][:, 6, 0].all()


def test_scenario_helpers():
    sv, _ = _lib()
    import mpc_ilqr_mujoco_amd as pkg
    sc = pkg.scenario
    d0, d1 = sv.al_default_bounds(0.0), sv.al_default_bounds(0.1)
    one = sc.stack_al_bounds({}, 4, margin=0.1)
    assert one.shape == (1, 76) and np.array_equal(one[0], d1)
    t = sc.stack_al_bounds(dict(torque_scale=0.5), 3)
    assert t.shape == (1, 76) and np.array_equal(t[0, :38], d0[:38]) and np.array_equal(t[0, 38:], 0.5 * d0[38:])
    assert t[0, 38 + 13] == -9.0 and t[0, 57 + 13] == 9.0
    recs = [dict(), dict(joint_hi={14: 2.58}, ctrl_lo={13: -16.2}, ctrl_hi={13: 16.2}), dict(torque_scale=np.r_[np.ones(18), 0.0], joint_lo=np.full(19, -np.inf))]
    t = sc.stack_al_bounds(recs, 3)
    assert t.shape == (3, 76) and np.array_equal(t[0], d0)
    want = d0.copy(); want[19 + 14] = 2.58; want[38 + 13] = -16.2; want[57 + 13] = 16.2
    assert np.array_equal(t[1], want)
    assert t[2, 38 + 18] == 0.0 and t[2, 57 + 18] == 0.0 and np.array_equal(t[2, 38:56], d0[38:56]) and np.all(t[2, :19] == -np.inf)      # a dead motor: lo = hi = 0
    for bad in (dict(joint_lo={14: 3.0}), dict(ctrl_lo={0: 1.0}, ctrl_hi={0: -1.0}), dict(joint_hi={3: float("nan")}), dict(ctrl_lo={2: np.inf}), dict(ctrl_hi={2: -np.inf}),
                dict(knee=1.0), dict(joint_lo=np.zeros(18)), dict(joint_lo={19: 0.0}), dict(torque_scale=-1.0)):
        with pytest.raises(ValueError):
            sc.stack_al_bounds(bad, 2)
    with pytest.raises(ValueError):
        sc.stack_al_bounds([{}, {}], 3)
    # the table in which the solver knows each rollout's range_scale
    joints = sc.stack_plant_joints([dict(), dict(range_scale=0.5, gain=0.7), dict(range_scale=np.r_[0.0, np.ones(18)])], 3)
    t = sc.al_bounds_from_plant_joints(joints, margin=0.1)
    assert t.shape == (3, 76) and np.array_equal(t[0], d1) and np.array_equal(t[:, :38], np.tile(d1[:38], (3, 1)))
    assert np.array_equal(t[1, 38:], 0.5 * d1[38:])      # (the gain is not folded in)
    assert t[2, 38] == 0.0 and t[2, 57] == 0.0 and np.array_equal(t[2, 39:57], d1[39:57])
    assert "gain" in sc.al_bounds_from_plant_joints.__doc__ and "NOT folded" in sc.al_bounds_from_plant_joints.__doc__


def test_reference_driver_meets_the_end_to_end_conditions():
    """Rollout 0 touches no limit; rollout 1 (default bounds) is done with a wrist torque well past 16.2 N m; rollout 2, the same problem
    bounded at +-16.2, gets within 0.1 N m of it but is not done after three rounds; rollout 3, the elbow bounded at 2.58 rad, is done
    within tol_joint of it while its twin under the default bounds peaks more than 10 tol_joint past it."""
    for early_exit in (True, False):
        sol = bc.reference_solves(early_exit)
        twin = ac.reference_solves(early_exit)[0][2]
        figures = bc.effect_assertions(sol, twin["X"])
        print("reference driver, %s: %s" % ("convergence exit" if early_exit else "fixed", ", ".join("%s %.6g" % kv for kv in figures.items())))
        assert sol[0]["done"] and not sol[0]["mu_j"].any() and not sol[0]["mu_c"].any()
        assert sol[1]["done"] and np.isnan(sol[1]["al_trace"][2]).all() == early_exit      # done after two rounds
        assert not np.isnan(sol[2]["al_trace"]).any()
        assert sol[2]["viol"][1] > bc.TOL_CTRL
        # rollouts 0 and 1 are al_ref's own solves of the same sets
        old = ac.reference_solves(early_exit)[0]
        for b, s in ((0, 0), (1, 1)):
            assert np.array_equal(sol[b]["X"], old[s]["X"]) and np.array_equal(sol[b]["U"], old[s]["U"]) and np.array_equal(sol[b]["al_trace"], old[s]["al_trace"], equal_nan=True)
