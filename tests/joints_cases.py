"""Inputs and helpers of the tests of the per-rollout joint records (include/ilqr_hip.h ilqr_hip_plant_set_joints; test_joints_cpu.py,
test_gpu_joints.py).  Test infrastructure only; NumPy and the CPU oracle, no GPU.

Two yardsticks that share no code with the kernels and none with each other:
  * the golden (tests/golden/joints_golden.npz, written by tests/golden/gen_joints_golden.py): single steps in all six step kinds from the
    NumPy Kane / KKT restatement called with ctrlrange * s, g * u, damping = d, armature = a; beside each x_next the nominal twin and the
    steps of five wrong readings of the record (MUTANTS);
  * the closed form on the CPU oracle's inverse dynamics.  The oracle knows one armature for every hinge; with qacc = (v+ - v) / h of a step
    under the record (g, s, d, a), its inverse dynamics under the effective armature of the MODEL, ARM0 = 0.1 + h * 1 = 0.12 at h = 0.02,
    misses on hinge i exactly the inertia the record adds:
        inverse_dynamics(x, qacc, ARM0, gravity)[6 + i] = clamp(g_i u_i, -s_i R_i, s_i R_i) - d_i v_i - (a_i + h d_i - ARM0) qacc_i
    on every hinge that is not stopped and that no stance row reaches; the base rows are those of wrench_cases / payload_cases (zero on the
    free plant without either)."""
import os

import numpy as np

import payload_cases as plc
import wrench_cases as wc

NX, NU, NQ = 51, 19, 26
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ID_TOL = plc.ID_TOL
FREE_TOL = 1e-10                     # the GPU step in mode 0 without rows, absolute (tests/test_gpu_payload.py)
NOMINAL = np.concatenate([np.ones(3 * NU), 0.1 * np.ones(NU)])
NOMINAL.setflags(write=False)
KNEE = 3                             # left knee, in the order of u
MUTANTS = ("gain_behind_clamp", "scale_ignored", "damping_not_in_armature", "mean_armature", "legs_swapped")


def golden():
    return np.load(os.path.join(G, "joints_golden.npz"))


def fields(rec):
    rec = np.asarray(rec)
    return rec[..., 0:19], rec[..., 19:38], rec[..., 38:57], rec[..., 57:76]


def applied_torque(u, rec):
    """clamp(g u, -s R, s R) [.., 19]"""
    g, s, _, _ = fields(rec)
    return np.clip(g * u, -s * wc.sc.CTRLRANGE, s * wc.sc.CTRLRANGE)


def hinge_residual(x, xn, u, h, gravity, rec):
    """[25]: the oracle's inverse dynamics of the step x -> xn under the model's effective armature, less the record's closed form on the hinge
    rows; what is left is whatever else acted (stance rows, stops, and on the base rows a wrench and a payload)"""
    import oracle_lib as ol
    _, _, d, a = fields(rec)
    arm0 = wc.ARMATURE + h * wc.DAMPING
    xu = x.copy(); xu[3:7] /= np.linalg.norm(xu[3:7])
    qacc = (xn[NQ:] - x[NQ:]) / h
    tau = ol.inverse_dynamics(xu, qacc, arm0, gravity)
    tau[6:] -= applied_torque(u, rec) - d * x[NQ + 6:] - (a + h * d - arm0) * qacc[6:]
    return tau


def expected_base_rows(x, xn, h, gravity, w9, pl):
    """the base rows of hinge_residual on a step without stance rows: the wrench's generalized force less what the payload asks of the pelvis"""
    return plc.expected_base_rows(x, xn, h, gravity, pl, w9)


def checked_hinges(act, lock):
    """the hinges the closed form holds on: not stopped, and -- with a foot held -- out of the reach of its rows (torso and arms)"""
    free = np.asarray(lock) == 0
    if np.any(act):
        up = np.zeros(NU, dtype=bool); up[wc.UPPER] = True
        free &= up
    return free


def bound_units(got, want, free):
    """the error in units of the bound the GPU step is held to: FREE_TOL absolute in mode 0 without rows, 1e-9 relative otherwise"""
    if free:
        return float(np.abs(got - want).max()) / FREE_TOL
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) / 1e-9


def random_records(n, seed, dead=()):
    """[n, 76]: gains 0.6-1.2, range scales 0.05-1, dampings 0.3-3, armatures 0.03-0.3 per joint; the rows `dead` have a dead left knee"""
    rng = np.random.default_rng(seed)
    out = np.hstack([rng.uniform(0.6, 1.2, (n, NU)), rng.uniform(0.05, 1.0, (n, NU)), rng.uniform(0.3, 3.0, (n, NU)), rng.uniform(0.03, 0.3, (n, NU))])
    for b in dead:
        out[b, NU + KNEE] = 0.0
    return np.ascontiguousarray(out)
