"""The velocities of the task coordinates on the GPU (ilqr_hip_get_al_task_velocities: k_al_task_velocities on al_task_dev.h's
al_task_velocities) against the CPU reference tests/al_task_vel_ref.py -- the oracle's own velocity functionals R0 gamma_s through
tests/cpp/al_task_vel_dump.cpp, which test_al_task_vel_cpu.py anchors to the oracle -- on the states of tests/al_task_vel_cases.py.

Tolerance: 1e-12 m/s, the task family's own for its coordinates (test_gpu_al_task.py: 1e-12 m on points of |p| ~ 1 m; here |v| < 1 m/s):
a velocity is a sum of ~60 products of O(1) factors, each rounded once on either side, so the two differ by a few 1e-16."""
import numpy as np
import pytest

import al_cases as ac
import al_task_vel_cases as vc
import al_task_vel_ref as vr
from test_gpu_configs import _solver

pytestmark = pytest.mark.gpu


def test_getter_against_the_reference():
    """al_task_velocities() on the 60 x 5 states of regimes() (off the standing pose, turned pelvis, random velocities up to 0.3), 1e-12; it
    needs an installed augmented Lagrangian and a trajectory, no window, and leaves the points' getter as it was."""
    R = vc.regimes()
    X, U = R["X"], R["U"]
    B, N = X.shape[0], vc.N_STAGE
    s = _solver(B, N=N); s.set_problem(vc.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=vc.STAGE_MARGIN)
    pts = s.al_task_points()
    got = s.al_task_velocities()
    assert np.array_equal(s.al_task_points(), pts) and np.array_equal(s.al_task_velocities(), got)      # (the two getters share a buffer)
    s.close()
    e, ep = np.abs(got - R["V"]).max(), np.abs(pts - R["P"]).max()
    print("velocities against the reference: %.2e m/s (largest |v| %.3f); points %.2e m" % (e, np.abs(R["V"]).max(), ep))
    assert got.shape == (60, 5, 9) and 0.3 < np.abs(R["V"]).max() < 1.0 and e <= 1e-12 and ep <= 1e-12
    # every coordinate is exercised: none of the nine is small everywhere
    assert (np.abs(R["V"]).reshape(-1, 9).max(axis=0) > 0.05).all()


def test_getter_follows_a_solve_and_its_refusals():
    """After a solve the getter returns the velocities of the new nominal trajectory (B = 3, N = 6); ILQR_ERR_STATE without an augmented
    Lagrangian and without a trajectory, ILQR_ERR_ARG for a null pointer."""
    from mpc_ilqr_mujoco_amd import solver as sv
    prob, x0, ui = vc.e2e_problem()
    N = prob["N"]
    s = _solver(3, N=N); s.set_problem(prob); s.set_max_iterations(vc.MAX_ITER)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.al_task_velocities()
    s.set_augmented_lagrangian(**vc.al_args())
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):      # an installed augmented Lagrangian, no trajectory yet
        s.al_task_velocities()
    assert s.L.ilqr_hip_get_al_task_velocities(s.h, None) == 1
    s.initialize(x0, ui)
    v0 = s.al_task_velocities()
    s.solve(x0)
    v1, X = s.al_task_velocities(), s.xbar()
    s.clear_augmented_lagrangian()
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.al_task_velocities()
    s.close()
    e = np.abs(v1 - vr.velocities(X)).max()
    print("velocities of the solved trajectories against the reference: %.2e m/s" % e)
    assert e <= 1e-12 and not np.array_equal(v0, v1) and not v1[:, 0, 3:].any() and np.abs(v1[1]).max() > 0.1
