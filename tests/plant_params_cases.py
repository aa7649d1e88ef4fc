"""Inputs and the yardstick of the tests of the plant's own model and its parameter sets (include/ilqr_hip.h ilqr_hip_plant_set_model /
ilqr_hip_plant_set_params; test_plant_params_cpu.py, test_gpu_plant_params.py).  Test infrastructure only.

Shape: B = 37 rollouts, N = 6, DT = 0.02, SUBSTEPS = 2 -- at feedback mode 0 two workgroups of the plant kernels (32 rollouts each, the second
with five), at feedback mode 1 ten (four each, the last with one).  Rollout b steps with parameter set b % 3 (SETS), so the two rollouts of
neighbouring lane pairs never share a set, under the stance pattern STANCE_ROWS[(b // 3) % 4] at every knot (a per-rollout schedule), from
envelope state (b + STATE_OFFSET) % 16 of tests/contact_envelope_cases.py / tests/dynamics_envelope_cases.py with that state's own control.

STATE_OFFSET = 2 was chosen on the CPU oracle, before any kernel ran: of the sixteen offsets it is the first at which the first plant step
(h = DT / SUBSTEPS) of every case moves by more than 1e-6 in at least four rollouts, one of them among b = 32..36, when any one acting
column of the table is set back to the value of set 0 (test_plant_params_cpu.py test_the_batch_exercises_every_column_in_both_workgroups).
Of b = 32..36 only b = 32 (set 2, right foot) has a stance foot and a set other than 0: friction and softness have that one rollout to show
themselves in.  The model-mismatch case (plant mode 3 WITH joint-limit rows on the limit states) meets the same conditions at no offset
that serves the others, and takes STATE_OFFSET_MODE3_LIMITS = 3, chosen the same way.

The yardstick (Yardstick) is never a plant kernel: it is the teacher-forced composition A.compute_control -> gain * u -> P_s.step /
step_stance / step_geometry on one handle P_s per distinct parameter set, created at DT / SUBSTEPS with that set's gravity, friction,
softness and stiffness and the PLANT's contact mode and joint-limit option."""
import numpy as np

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import oracle_lib as ol

NX, NU, NQ = 51, 19, 26
B, N, DT, SUBSTEPS = 37, 6, 0.02, 2
STATE_OFFSET = 2
STATE_OFFSET_MODE3_LIMITS = 3
COLUMNS = dict(gravity=(0, 1, 2), friction=(3,), softness=(4,), limit_stiffness=(5,), torque_gain=(6,))
#                 gx    gy     gz     mu    soft   k       gain
SETS = np.array([[0.0, 0.0, -9.81, 0.3, 1e-5, 0.0, 1.0],           # the handle's defaults with mu 0.3
                 [0.6, -0.4, -9.5, 1e3, 1e-5, 625.0, 1.0],          # a floor that is not level, feet that never slide, MuJoCo's default stop
                 [0.0, 0.0, -9.81, 0.7, 1e-4, 156.25, 0.8]])        # softer ground, a softer stop, weaker motors
SETS.setflags(write=False)


def set_of(b):
    return np.asarray(b) % 3


def pattern_of(b):
    return (np.asarray(b) // 3) % 4


def state_of(b, offset=STATE_OFFSET):
    return (np.asarray(b) + offset) % dc.NS


def params(sets=SETS):
    """[B, 7]: the table of the batch"""
    return np.ascontiguousarray(np.asarray(sets)[set_of(np.arange(B))])


def schedule():
    """[B, N + 1, 2]: rollout b under its pattern at every knot"""
    return np.ascontiguousarray(np.repeat(dc.STANCE_ROWS[pattern_of(np.arange(B))][:, None, :], N + 1, axis=1))


def batch(x16, u16, offset=STATE_OFFSET):
    """(x0 [B,51], u_init [B,N,19]) from the sixteen states of an envelope group and their controls"""
    idx = state_of(np.arange(B), offset)
    return np.ascontiguousarray(x16[idx]), np.ascontiguousarray(np.repeat(u16[idx][:, None, :], N, axis=1))


def acting_columns(mode, limits):
    """the columns of a set that reach the step in a plant of this contact mode / joint-limit option (include/ilqr_hip.h)"""
    cols = ["gravity", "torque_gain"]
    if mode >= 3:
        cols.append("friction")
    if mode >= 1:
        cols.append("softness")
    if limits:
        cols.append("limit_stiffness")
    return cols


def with_column_shared(p, name):
    """the table with column `name` set back to the value of set 0 in every row"""
    q = np.array(p, dtype=np.float64)
    q[:, list(COLUMNS[name])] = SETS[0, list(COLUMNS[name])]
    return q


def check_column_conditions(moved, fb, tag):
    """moved {column: [B] bool}: at least four rollouts, and at feedback mode 0 at least one in each workgroup of 32"""
    for name, mv in moved.items():
        n = (int(mv[:32].sum()), int(mv[32:].sum()))
        print("%s: column %-15s moves %2d + %d rollouts" % (tag, name, n[0], n[1]))
        assert n[0] + n[1] >= 4, (tag, name, n)
        if fb == 0:
            assert n[0] >= 1 and n[1] >= 1, (tag, name, n)


# ---- the CPU oracle's step under a parameter set (what the table is meant to do, on code that shares nothing with the kernels)
def oracle_of(p, mode, limits, h):
    prob = dc.problem(4 if mode else 1, dc.SCHEDULE if mode else None, tuple(p[:3]))
    o = ol.Oracle(prob["N"], h); o.set_problem(prob); o.set_contact_mode(mode, p[4] if mode else 0.0)
    return cc.configure(o, p[3] if mode >= 3 else None, limits, p[5])


def oracle_steps(p, mode, limits, x, u, h):
    """[n, P, 51]: the oracle's step of every (state, stance pattern) under the set p, the control scaled by the set's gain"""
    return cc.steps(oracle_of(p, mode, limits, h), x, p[6] * u, mode)


def oracle_first_step(table, mode, limits, x16, u16, offset=STATE_OFFSET):
    """[B, 51]: the first plant step of the batch on the CPU oracle"""
    out = np.zeros((B, NX))
    for s in np.unique(table, axis=0):
        st = oracle_steps(s, mode, limits, x16, u16, DT / SUBSTEPS)
        for b in np.flatnonzero((table == s).all(axis=1)):
            out[b] = st[state_of(b, offset), pattern_of(b) if mode else 0]
    return out


# ---- the yardstick on the GPU: entry points that existed before the table
class Yardstick:
    """One handle per distinct (gravity, friction, softness, stiffness) at h = DT / SUBSTEPS, in the plant's mode and limits; created on
    demand and kept until close()."""

    def __init__(self, sv, sc, mode, limits, source="schedule"):
        self.sv, self.sc, self.mode, self.limits, self.source = sv, sc, int(mode), bool(limits), source
        self.handles = {}

    def handle(self, p):
        key = tuple(float(v) for v in p[:6])
        P = self.handles.get(key)
        if P is None:
            P = self.sv.BatchedILQR(B, N=N, dt=DT / SUBSTEPS)
            P.set_problem(self.sc.make_problem(self.sv.reference_kinematics, N=N, gravity=key[:3]))
            P.set_contact_mode(self.mode, key[4])
            P.set_friction(key[3])
            P.set_joint_limits(self.limits)
            P.set_joint_limit_stiffness(key[5])
            self.handles[key] = P
        return P

    def step(self, table, x, u, flags):
        """one plant step of every rollout under its row of `table`: (x_next [B,51], stance [B,2])"""
        xn, st = np.empty_like(x), np.array(flags, dtype=np.int32)
        ua = table[:, 6:7] * u                                              # the torque gain, on the host
        for s in np.unique(table[:, :6], axis=0):
            rows = np.flatnonzero((table[:, :6] == s).all(axis=1))
            P = self.handle(s)
            if self.mode and self.source == "geometry":
                xn[rows], st[rows] = P.step_geometry(x[rows], ua[rows])
            elif self.mode:
                for l, r in {(int(a), int(c)) for a, c in flags[rows]}:     # step_stance takes one flag pair per call
                    idx = rows[(flags[rows, 0] == l) & (flags[rows, 1] == r)]
                    xn[idx] = P.step_stance(x[idx], ua[idx], l, r)
            else:
                xn[rows] = P.step(x[rows], ua[rows])
        return xn, st

    def advance(self, A, table, x, flags, fb, knot=0):
        """what one MPC interval has to produce from the state x it starts from: (x_next, reported u, stance)"""
        xc, u, st = x.copy(), None, np.array(flags, dtype=np.int32)
        for k in range(SUBSTEPS):
            if k == 0 or fb:
                u = A.compute_control(xc, knot=knot)
                u[~np.isfinite(u).all(axis=1)] = 0.0                        # main/humanoid_mpc.cpp:162-165, in front of the gain
            xc, st = self.step(table, xc, u, flags)
        return xc, u, st

    def close(self):
        for P in self.handles.values():
            P.close()
        self.handles = {}
