"""Inputs and helpers of the tests of the external wrench on the pelvis (include/ilqr_hip.h ilqr_hip_plant_set_wrench; test_wrench_cpu.py,
test_gpu_wrench.py).  Test infrastructure only; NumPy and the CPU oracle, no GPU.

The golden (tests/golden/wrench_golden.npz, written by tests/golden/gen_wrench_golden.py) holds single steps under a wrench in all six step
kinds from the NumPy Kane / KKT restatement.  The oracle has no wrench; what it can say about a step under one is its inverse dynamics:
with qacc = (v+ - v) / h of the step,
    inverse_dynamics(x, qacc, armature + h damping) = clamp(u) - damping v + Wg (base rows) + J^T lambda + E^T nu
so on the constraint-free plant (with or without joint-limit rows, which act on hinge rows only) the base rows ARE the generalized force
of the wrench, Wg = [F ; R0^T T + r x (R0^T F)], and under stance rows the torso and arm hinge rows, which no foot reaches, still close on
clamp(u) - damping v wherever the hinge is not stopped."""
import os

import numpy as np

import oracle_lib as ol
from conftest import load_package

pkg = load_package()
sc = pkg.scenario
NX, NU, NQ = 51, 19, 26
ARMATURE, DAMPING = 0.1, 1.0                  # h1.xml joint defaults (tests/golden/gen_golden.py kane_step_c)
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
UPPER = np.arange(10, 19)                     # torso and arm hinges: no stance row reaches them


def golden():
    return np.load(os.path.join(G, "wrench_golden.npz"))


def rotation(quat):
    w, x, y, z = np.asarray(quat, dtype=np.float64) / np.linalg.norm(quat)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def generalized_force(x, w):
    """Wg [6] of wrench w = (F, T, r) at state x: conjugate to qvel[0:6] (world linear, body angular)"""
    R0 = rotation(x[3:7])
    Fb = R0.T @ w[0:3]
    return np.concatenate([w[0:3], R0.T @ w[3:6] + np.cross(w[6:9], Fb)])


def world_torque_of_offset(x, w):
    """the world torque that moving the force of w from r to the origin of the pelvis frame leaves behind: R0 (r x R0^T F)"""
    R0 = rotation(x[3:7])
    return R0 @ np.cross(w[6:9], R0.T @ w[0:3])


def inverse_dynamics_residual(x, xn, u, h, gravity):
    """[25]: inverse dynamics of the step x -> xn less the hinge torques clamp(u) - damping v; what is left is whatever else acted"""
    xu = x.copy(); xu[3:7] /= np.linalg.norm(xu[3:7])
    qacc = (xn[NQ:] - x[NQ:]) / h
    tau = ol.inverse_dynamics(xu, qacc, ARMATURE + h * DAMPING, gravity)
    uc = np.clip(u, -sc.CTRLRANGE, sc.CTRLRANGE)
    tau[6:] -= uc - DAMPING * x[NQ + 6:]
    return tau


def golden_oracle(g, i):
    """the oracle configured as case i of the golden: one knot under the case's stance pattern"""
    mode = int(g["contact"][i])
    prob = sc.make_problem(ol.reference_kinematics, N=1, gravity=tuple(g["gravity"]), stance=np.tile(g["stance"][i], (2, 1)).astype(np.int32))
    o = ol.Oracle(1, float(g["h"])); o.set_problem(prob); o.set_contact_mode(mode, float(g["soft"]) if mode else 0.0)
    o.set_friction(float(g["mu"][i])); o.set_joint_limits(bool(g["limits"][i])); o.set_joint_limit_stiffness(0.0)
    return o


def random_wrenches(n, seed, point=True):
    """[n, 9]: forces of 50-150 N and torques of 10-40 N m in random directions, points of application within 0.15 m of the pelvis origin"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)); F = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(50.0, 150.0, (n, 1))
    d = rng.normal(size=(n, 3)); T = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(10.0, 40.0, (n, 1))
    r = rng.uniform(-0.15, 0.15, (n, 3)) if point else np.zeros((n, 3))
    return np.ascontiguousarray(np.hstack([F, T, r]))
