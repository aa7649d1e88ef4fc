"""Inputs and helpers of the tests of the rigid payload on the pelvis (include/ilqr_hip.h ilqr_hip_plant_set_payload; test_payload_cpu.py,
test_gpu_payload.py).  Test infrastructure only; NumPy and the CPU oracle, no GPU.

Two yardsticks that share no code with the kernels and none with each other:
  * the golden (tests/golden/payload_golden.npz, written by tests/golden/gen_payload_golden.py): single steps in all six step kinds from the
    NumPy Kane / KKT restatement, the payload merged into the pelvis body by the parallel-axis theorem -- a composite rigid body;
  * the closed form on the CPU oracle's inverse dynamics.  The oracle has no payload; with qacc = (v+ - v) / h of a step of the LOADED
    robot, its inverse dynamics of the unloaded one misses exactly what the payload's own Newton-Euler equations ask of the pelvis.  With
    w, dw the pelvis' angular velocity and acceleration (body frame), R0 its rotation, g gravity:
        a_c = qacc[0:3] + R0 (dw x c + w x (w x c))        acceleration of the payload's centre of mass, world frame
        Fw  = m (a_c - g)                                   force on the payload, world frame
        tb  = c x R0^T Fw + Ic dw + w x Ic w                its moment about the pelvis origin, body frame
    and on a constraint-free step (wrench_cases.inverse_dynamics_residual conventions) res[0:6] = Wg - [Fw ; tb], res[6:] = 0 on every
    hinge that is not stopped, Wg the generalized force of a wrench beside it (zero without one)."""
import os

import numpy as np

import wrench_cases as wc

NX, NU, NQ = 51, 19, 26
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ID_TOL = 1e-6      # N, N m: a step error of 1e-11 divided by h = 0.02 and multiplied by the loaded robot's 70 kg is 4e-8, with margin


def golden():
    return np.load(os.path.join(G, "payload_golden.npz"))


def inertia_matrix(i6):
    xx, yy, zz, xy, xz, yz = i6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def payload_base_force(x, xn, h, gravity, pl):
    """[Fw ; tb] [6] of the payload pl [10] over the step x -> xn: what it asks of the pelvis, conjugate to qvel[0:6]"""
    m, c, Ic = pl[0], pl[1:4], inertia_matrix(pl[4:10])
    R0 = wc.rotation(x[3:7])
    qacc = (xn[NQ:] - x[NQ:]) / h
    w, dw = x[NQ + 3:NQ + 6], qacc[3:6]
    a_c = qacc[0:3] + R0 @ (np.cross(dw, c) + np.cross(w, np.cross(w, c)))
    Fw = m * (a_c - np.asarray(gravity))
    tb = np.cross(c, R0.T @ Fw) + Ic @ dw + np.cross(w, Ic @ w)
    return np.concatenate([Fw, tb])


def expected_base_rows(x, xn, h, gravity, pl, w9=None):
    """the base rows of wc.inverse_dynamics_residual of a constraint-free step of the loaded robot"""
    Wg = np.zeros(6) if w9 is None else wc.generalized_force(x, w9)
    return Wg - payload_base_force(x, xn, h, gravity, pl)


def random_payloads(n, seed):
    """[n, 10]: 2-20 kg, centre of mass within 0.3 m of the pelvis origin, a random positive-definite Ic of up to about 1 kg m^2"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 10))
    out[:, 0] = rng.uniform(2.0, 20.0, n)
    d = rng.normal(size=(n, 3))
    out[:, 1:4] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.05, 0.3, (n, 1))
    for i in range(n):
        A = rng.normal(size=(3, 3))
        I = rng.uniform(0.05, 0.4) * (A @ A.T / 3.0 + 0.05 * np.eye(3))
        out[i, 4:10] = [I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
    return np.ascontiguousarray(out)
