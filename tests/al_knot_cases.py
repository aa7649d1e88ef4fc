"""Inputs of the tests of the per-knot bounds of the augmented-Lagrangian limits (test_al_knot_cpu.py, test_gpu_al_knot.py).  NumPy and the
oracle's host helpers only; no GPU.

  * joint_windows(): al_bounds_cases.regimes_table() (228 rollouts, N = 4) with rollout b's record as row t of its window, t the case's own
    knot, and every other row moved so that reading it at knot t puts the case into another regime.
  * state_windows(): the same for al_state_cases.regimes() (168 rollouts), with a joint / torque window that differs from row to row.
  * end_to_end(): B = 4, N = 6 on the references of al_cases.end_to_end(), with the windows of the issue's four rollouts.
"""
import functools

import numpy as np

import al_bounds_cases as bc
import al_bounds_ref as br
import al_cases as ac
import al_knot_ref as kr
import al_state_cases as stc
import al_state_ref as sr

sc = ac.sc
N_STAGE = ac.N_STAGE
MOVE = 0.06      # of the coordinate's own width: the excited value sits 0.02 of it from its bound


def _moved(value_active, lo_hi_side, width):
    """the excited bound of a row other than the case's own: 6 % of the width further OUT where the case is active under its own bound
    (value 2 % outside, or 2 % inside with mu + rho c > 0: it becomes inactive, mu + rho c < 0), 6 % further IN where it is inactive (the
    value ends 4 % outside: active); side 0 = lower bound, 1 = upper"""
    bound, side = lo_hi_side
    out = 1.0 if side else -1.0
    return bound + (out if value_active else -out) * MOVE * width


@functools.lru_cache(maxsize=None)
def joint_windows():
    """win [228, 5, 76]; read-only.  Row t of rollout b (t = the knot of cases[b]) is regimes_table()'s record rec[b]; in every other row
    the excited coordinate's excited bound is moved by _moved.  The other knots' own values of that coordinate stay where regimes_table put
    them (at least 1 % inside rec[b]): under a row moved inward some of them become active, which the restatement carries."""
    X, U, mu_j, mu_c, rho, rec, cases, inf = bc.regimes_table()
    B, N = X.shape[0], N_STAGE
    win = np.repeat(rec[:, None, :], N + 1, axis=1).copy()
    for b, (kind, j, side, t, g) in enumerate(cases):
        f = 0 if kind == "joint" else 38
        lo, hi = rec[b, f + j], rec[b, f + 19 + j]
        val = X[b, t, 7 + j] if kind == "joint" else U[b, t, j]
        mu = (mu_j[b, t, j, side] if kind == "joint" else mu_c[b, t, j, side])
        c = val - hi if side else lo - val
        active = mu + rho[b, 0 if kind == "joint" else 1] * c > 0.0
        new = _moved(active, (hi if side else lo, side), hi - lo)
        for s in range(N + 1):
            if s != t:
                win[b, s, f + 19 * side + j] = new
    sc._check_al_bounds(win.reshape(-1, 76))
    win.setflags(write=False)
    return win


@functools.lru_cache(maxsize=None)
def state_windows():
    """(swin [168, 5, 56], jwin [168, 5, 76]); read-only.  swin: al_state_cases.regimes()'s srec[b] in the row of the case's own knot, the
    excited bound moved by _moved in every other row.  jwin: row t of rollout b is the model's record at the margin of rollout
    (b + 7 t) % 168 of regimes() -- every row another record, every hinge and actuator inactive under each of them."""
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, inf = stc.regimes()
    B, N = X.shape[0], N_STAGE
    swin = np.repeat(srec[:, None, :], N + 1, axis=1).copy()
    for b, (k, side, t, g) in enumerate(cases):
        lo, hi = srec[b, k], srec[b, 28 + k]
        val = X[b, t, sr.SLOTS[k]]
        c = val - hi if side else lo - val
        active = mu_s[b, t, k, side] + rho[b, 2] * c > 0.0
        new = _moved(active, (hi if side else lo, side), hi - lo)
        for s in range(N + 1):
            if s != t:
                swin[b, s, 28 * side + k] = new
    jwin = np.stack([[rec[(b + 7 * t) % B] for t in range(N + 1)] for b in range(B)])
    for a in (swin, jwin):
        a.setflags(write=False)
    return swin, jwin


def misread_rows(t, N, last):
    """the rows a kernel that mis-addresses knot t's bounds would read: t - 1, t + 1, 0 and N (`last` = the last row that exists for the
    family: N; the actuators of knot t < N may mis-read row N as well), without t itself"""
    return sorted({s for s in (t - 1, t + 1, 0, last) if 0 <= s <= last and s != t})


# ---------------------------------------------------------------------------------------------------------------------------------------
# The end-to-end case.  al_bounds_cases.end_to_end() puts reference set 0 behind rollout 0; its wrist torque is identically zero, so no bound
# on it can be exceeded at any knot.  The four rollouts here take the sets (1, 1, 1, 2) of al_cases.end_to_end() instead -- rollout 0 is then
# the problem whose wrist torque passes 0.9 x its range at knot 0 -- with N, weights, x0 and u_init as they are there.
E2E_SETS = (1, 1, 1, 2)
WRIST, WRIST_BOUND = bc.WRIST, bc.WRIST_BOUND
T_S = 1                        # rollout 0: the tight wrist bound holds from this knot on
Z_LIFT = 2e-4                  # m: the pelvis-height bound of rollout 2 ends this far above the unconstrained height at knot N
Z_FLOOR = 1.03                 # m: and starts here at knot 0, below every height of the horizon
AL_E2E = stc.AL_E2E            # (al_cases.AL_E2E with one more round, rho_state0 and tol_state: the pelvis moves 5e-6 m per N m and step)
MAX_ITER = ac.MAX_ITER
TOL_CTRL = ac.AL_E2E["tol_ctrl"]


class StateDriver(sr.Driver):
    """al_state_ref.Driver (one rollout) under the windows win [N+1,76] and swin [N+1,56]: the parents' inner solve with the three
    families' terms, violation and update taken from al_knot_ref"""

    def __init__(self, prob, b, al, win, swin, **kw):
        super().__init__(prob, b, al, np.asarray(win)[0], np.asarray(swin)[0], **kw)
        self.win, self.swin = np.array(win, dtype=np.float64), np.array(swin, dtype=np.float64)

    def _al(self, X, U):
        return kr.traj_terms(X, U, self.mu_j, self.mu_c, self.rho, self.win)

    def cost(self, X, U):
        return br.Driver.cost(self, X, U) + float(kr.state_traj_terms(X, self.mu_s, self.rho_s, self.swin)[0].sum())

    def inner(self, x0, X, U):
        real = sr.traj_terms
        sr.traj_terms = lambda X_, mu, rho, srec: kr.state_traj_terms(X_, mu, rho, self.swin)      # (the parent's loop, the window's terms)
        try:
            return super().inner(x0, X, U)
        finally:
            sr.traj_terms = real

    def solve(self, x0, u_init):
        real = sr.update
        sr.update = lambda X, U, mj, mc, ms, rho, done, rec, srec, *rest: kr.state_update(X, U, mj, mc, ms, rho, done, self.win, self.swin, *rest)
        try:
            return super().solve(x0, u_init)
        finally:
            sr.update = real


@functools.lru_cache(maxsize=None)
def end_to_end():
    """(prob, x0 [4,51], u_init [4,6,19], win [4,7,76], swin [4,7,56], info); read-only.
      rollout 0  the wrist actuator bounded at +-16.2 N m (0.9 x its range) on the knots >= T_S only;
      rollout 1  the same bound on every knot;
      rollout 2  pelvis_z bounded below by a line that rises from Z_FLOOR at knot 0 to Z_LIFT above the unconstrained height at knot N;
      rollout 3  the default rows: no bound of its own.
    The unconstrained solution is al_cases.reference_solves(True) of the rollout's set."""
    prob3, x03, ui3 = ac.end_to_end()
    idx = np.array(E2E_SETS)
    prob = dict(prob3)
    for k in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        prob[k] = np.ascontiguousarray(prob3[k][idx])
    x0, ui = np.ascontiguousarray(x03[idx]), np.ascontiguousarray(ui3[idx])
    N = prob["N"]
    free, _ = ac.reference_solves(True)
    z_end = float(free[E2E_SETS[2]]["X"][N, 2])
    tight = dict(ctrl_lo={WRIST: -WRIST_BOUND}, ctrl_hi={WRIST: WRIST_BOUND})
    win = sc.stack_al_knot_bounds([{k: (T_S, N + 1, v) for k, v in tight.items()}, tight, {}, {}], 4, N, margin=AL_E2E["margin"])
    z_lo = np.linspace(Z_FLOOR, z_end + Z_LIFT, N + 1)
    swin = sc.stack_al_state_knot_bounds([{}, {}, dict(pelvis_z=[(t, t + 1, (z_lo[t], np.inf)) for t in range(N + 1)]), {}], 4, N)
    for a in (x0, ui, win, swin, prob["x_ref"]):
        a.setflags(write=False)
    return prob, x0, ui, win, swin, dict(z_lo=z_lo, z_free=free[E2E_SETS[2]]["X"][:, 2].copy())


def al_args(al=AL_E2E):
    return stc.al_args(al)


def problem_of(prob, b):
    return ac.problem_of(prob, b)


@functools.lru_cache(maxsize=None)
def reference_solves(early_exit):
    """the reference driver (StateDriver) on end_to_end(): [solve of rollout b under its two windows]; computed once, read-only"""
    prob, x0, ui, win, swin, _ = end_to_end()
    return [StateDriver(prob, b, AL_E2E, win[b], swin[b], max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(4)]


def effect_assertions(sols):
    """The conditions of the end-to-end case on results sols[b] = dict(U [N,19], X [N+1,51]) of the four rollouts: rollout 0 exceeds the
    tight wrist bound by more than tol_ctrl at some knot < T_S and respects it within tol_ctrl at every knot >= T_S; rollout 1, bounded on
    every knot, exceeds it nowhere by what rollout 0 exceeds it at knot 0."""
    u0, u1 = (np.abs(np.asarray(sols[b]["U"])[:, WRIST]) for b in (0, 1))
    assert u0[:T_S].max() > WRIST_BOUND + TOL_CTRL, u0
    assert u0[T_S:].max() <= WRIST_BOUND + TOL_CTRL, u0
    assert u1.max() < u0[:T_S].max() - 1.0, (u0, u1)
    return dict(peak_u13_before=float(u0[:T_S].max()), peak_u13_from_ts=float(u0[T_S:].max()), peak_u13_all_knots=float(u1.max()))
