"""The yardstick of the closed-loop score (include/ilqr_hip.h ilqr_hip_plant_set_score): one term of one interval from the CPU oracle.
Test infrastructure only, shared by tests/test_plant_score_cpu.py and tests/test_gpu_plant_score.py.

The oracle exposes the whole of computeTotalCost (oracle/h1_costs.hpp total_cost), not its terms.  A term of interval k is isolated with a
horizon-1 oracle, Oracle(1, dt):
  * its row 0 holds row k of the window (x_ref, u_ref, com_ref, ee_ref, com_vel_ref, stance) of the rollout's reference set,
  * its terminal knot costs nothing: Qf = 0, stance row 1 = (0, 0) (no support point: no balance term), terminal state with the identity
    quaternion (upright term exactly 0) and every hinge at mid-range (no joint penalty); the terminal control penalty is evaluated at u = 0,
  * every weight is zero except the one of the term under test.
total_cost() is then that term of that interval.  tests/test_plant_score_cpu.py checks the construction against a horizon-N total_cost()."""
import numpy as np

import oracle_lib as ol

NX, NU, NQ = 51, 19, 26
TERMS = ("state", "control", "upright", "balance", "joint_limits", "control_limits")      # slots 0-5 of the record
REF_KEYS = ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref")


def free_terminal_state():
    jr = ol.joint_ranges()
    x = np.zeros(NX)
    x[3] = 1.0
    x[7:NQ] = 0.5 * (jr[:, 0] + jr[:, 1])
    return x


def pick(a, b):
    """rollout b's set of a reference array whose leading axis is 1 (shared) or B"""
    a = np.asarray(a)
    return a[b] if a.shape[0] > 1 else a[0]


def weights_of_term(score, i):
    """oracle weights under which total_cost() is term i alone; score: the arguments of plant_set_score"""
    w = dict(Q=np.zeros(NX), R=np.zeros(NU), Qf=np.zeros(NX), task_weights=[0.0] * 6, w_joint=0.0, w_ctrl=0.0)
    if i == 0:
        w["Q"] = np.asarray(score["Q"], dtype=np.float64)
    elif i == 1:
        w["R"] = np.asarray(score["R"], dtype=np.float64)
    elif i == 2:
        w["task_weights"][4] = float(score.get("upright", 0.0))
    elif i == 3:
        w["task_weights"][5] = float(score.get("balance", 0.0))
    elif i == 4:
        w["w_joint"] = float(score.get("joint_limits", 0.0))
    else:
        w["w_ctrl"] = float(score.get("control_limits", 0.0))
    return w


class IntervalOracle:
    def __init__(self, dt):
        self.o = ol.Oracle(1, dt)
        self.xT = free_terminal_state()

    def window_row(self, prob, b, k):
        """the horizon-1 reference data: row k of rollout b's sets, then the free terminal row"""
        two = lambda key: np.stack([pick(prob[key], b)[k], pick(prob[key], b)[k]])[None]
        sub = dict(gravity=prob["gravity"], x_ref=np.stack([pick(prob["x_ref"], b)[k], self.xT])[None], u_ref=pick(prob["u_ref"], b)[k][None, None],
                   com_ref=two("com_ref"), ee_ref=two("ee_ref"), com_vel_ref=two("com_vel_ref"))
        sub["stance"] = np.array([[pick(prob["stance"], b)[k], (0, 0)]], dtype=np.int32)
        return sub

    def terms(self, prob, b, k, x, u, score):
        """[6]: the terms of interval k of rollout b at the state x and control u, under the scoring weights"""
        sub = self.window_row(prob, b, k)
        out = np.zeros(len(TERMS))
        for i in range(len(TERMS)):
            sub.update(weights_of_term(score, i))
            self.o.set_problem(sub)
            self.o.set_trajectory(np.stack([x, self.xT]), np.asarray(u)[None])
            out[i] = self.o.total_cost()
        return out


def expected_record(orc, rows, hx, hu, score):
    """[B, 8]: the record of the ring rows hx [r,B,51] / hu [r,B,19]; rows[r] = (problem dict, knot) the interval was scored against.
    Sums run in interval order, as the device adds them."""
    r, B = hx.shape[0], hx.shape[1]
    rec = np.zeros((B, 8))
    rec[:, 6] = np.inf
    for j, (prob, k) in enumerate(rows):
        for b in range(B):
            rec[b, :6] += orc.terms(prob, b, k, hx[j, b], hu[j, b], score)
            v = hx[j, b, 2]
            rec[b, 6] = v if v < rec[b, 6] else rec[b, 6]
        rec[:, 7] += 1.0
    assert r == len(rows)
    return rec


def close_enough(got, want):
    """|got - want| <= 1e-11 |want| + 1e-11 (that rollout's total over slots 0-5): the 1e-11 tests/test_gpu_parity.py grants the same cost
    function against the same oracle; the second term keeps a term that is tiny beside the total from being held to its own last bits.
    Returns (ok [B,6], worst ratio of error to bound)."""
    err = np.abs(got[:, :6] - want[:, :6])
    bound = 1e-11 * np.abs(want[:, :6]) + 1e-11 * np.abs(want[:, :6]).sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return err <= bound, float(ratio.max())
