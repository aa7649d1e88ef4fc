"""CPU restatement of a task-velocity family of the augmented-Lagrangian limits -- not built in the library yet, which so
far returns the coordinates alone (include/ilqr_hip.h ilqr_hip_get_al_task_velocities; velocities() below is that getter's reference):
bounds on nine velocities in the world frame -- task-velocity coordinate k = 0..2 the velocity of the whole-body CoM, 3..5 of the left ankle
origin, 6..8 of the right ankle origin -- with the term, its gradient and its exact Hessian, the update over five families, the violation,
the done rule, the growth of the penalties and the warm-start shift in NumPy, on top of al_task_ref.py / al_state_ref.py, and an AL solve
driver with the fifth family.

The velocities are the quantities R(quat) gamma_s(theta, v) the cost's velocity terms (w_com_vel, w_ee_vel) penalise -- Pinocchio's velocity
convention (base linear velocity in the body frame), the rotation polynomial on the raw quaternion, for the CoM the URDF link masses --
because the family's gradient and Hessian are those quantities'.  They, their Jacobian rows J_k and the second-order sum  sum_k m_k d2 v_k
come from the oracle's own velocity terms, never from the code under test.  A velocity term  w |v - ref|^2  has the gradient
2 w J^T (v - ref) and the Hessian 2 w J^T J + sum_k 2 w (v - ref)_k d2 v_k: with ref = v - e_k / (2 w) the gradient is J_k, and the Hessian at
ref = v - m / (2 w) minus the Hessian at ref = v is  sum_k m_k d2 v_k.
  * CoM: a one-knot oracle whose only weight is w_com_vel = w, whose reference com_vel_ref is free (Oracle.knot_quadratics).
  * feet: the oracle's foot-velocity term has a fixed zero target, so tests/cpp/al_task_vel_dump.cpp (built here with g++) runs the oracle's
    own prepare_terms and add_vel_term on a point set with a target of the caller's choice and returns what they add to a zero lx, lxx, in
    the slot convention of Oracle.knot_quadratics.  test_al_task_vel_cpu.py anchors it: with target 0 on a stance foot its (lx, lxx) are
    knot_quadratics' with only w_ee_vel on; on the CoM set its rows are the one-knot oracle's.
The velocities themselves are the program's R0 gamma_s (the oracle's prepare_terms).

A window is [N+1, 18], row t = lo[9], hi[9] in m/s; multipliers are arrays [..., 9, 2] = (lower, upper).  An infinite side gives c = -inf,
max(0, mu + rho c) = 0 and the constant term -mu^2 / (2 rho).  THE SWING RULE, the complement of the task family's stance rule: a foot's
three rows count only at knots where the schedule has that foot in stance (flag 1); at every other knot they are rows with both sides
switched off.  The terminal knot is included for all nine rows.  No GPU."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import al_bounds_ref as br
import al_ref as ar
import al_state_ref as sr
import al_task_ref as tr
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NU, NQ = ar.NX, ar.NU, ar.NQ
COORDS, AL_TASK_VEL_BOUNDS = 9, 18
NO_BOUNDS = np.concatenate([np.full(COORDS, -np.inf), np.full(COORDS, np.inf)])
FOOT_OF = tr.FOOT_OF      # the foot a coordinate belongs to (-1: the CoM)


# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dump_exe():
    d = tempfile.mkdtemp(prefix="al_task_vel_dump_")
    atexit.register(shutil.rmtree, d, True)
    exe = os.path.join(d, "al_task_vel_dump")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-variable", "-Wno-missing-braces", "-I", os.path.join(ROOT, "oracle"),
                        os.path.join(ROOT, "tests", "cpp", "al_task_vel_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def vel_terms(sets, w, X, targets):
    """tests/cpp/al_task_vel_dump.cpp on n queries: point set sets[i], weight w, state X[i] [51], target targets[i] [3].  Returns
    (v [n,3] the set's velocity, lx [n,51], lxx [n,51,51] of the oracle's add_vel_term on zeros)."""
    sets, X, targets = np.atleast_1d(sets), np.asarray(X, dtype=np.float64).reshape(-1, NX), np.asarray(targets, dtype=np.float64).reshape(-1, 3)
    n = X.shape[0]
    q = np.zeros((n, 56))
    q[:, 0], q[:, 1], q[:, 2:53], q[:, 53:] = sets, float(w), X, targets
    r = subprocess.run([_dump_exe()], input=q.tobytes(), capture_output=True)
    assert r.returncode == 0, r.stderr
    out = np.frombuffer(r.stdout, dtype=np.float64).reshape(n, 3 + NX + NX * NX)
    return out[:, :3].copy(), out[:, 3:3 + NX].copy(), out[:, 3 + NX:].reshape(n, NX, NX).copy()


def velocities(X):
    """task-velocity coordinates [..., 9] of states X [..., 51]"""
    X = np.asarray(X, dtype=np.float64)
    flat = X.reshape(-1, NX)
    n = flat.shape[0]
    v, _, _ = vel_terms(np.repeat(np.arange(3), n), 0.0, np.tile(flat, (3, 1)), np.zeros((3 * n, 3)))
    return np.concatenate([v[:n], v[n:2 * n], v[2 * n:]], axis=1).reshape(X.shape[:-1] + (COORDS,))


def rows_off(stance):
    """[..., 9] bool: the rows the swing rule switches off, from stance flags [..., 2]: a foot's rows wherever its flag is not 1"""
    stance = np.asarray(stance)
    off = np.zeros(stance.shape[:-1] + (COORDS,), dtype=bool)
    off[..., 3:6] = (stance[..., 0] != 1)[..., None]
    off[..., 6:9] = (stance[..., 1] != 1)[..., None]
    return off


def effective_window(win, stance, use_swing=True):
    """the window with the rows of swinging feet made infinite: what the solver acts on"""
    win = np.array(win, dtype=np.float64)
    assert win.shape[-1] == AL_TASK_VEL_BOUNDS
    if use_swing:
        off = rows_off(stance)
        win[..., :COORDS] = np.where(off, -np.inf, win[..., :COORDS])
        win[..., COORDS:] = np.where(off, np.inf, win[..., COORDS:])
    return win


def constraints(V, win, stance, use_swing=True):
    """c [..., 9, 2] = (lo - v, v - hi) of velocities V [..., 9] against rows win [..., 18] under stance flags [..., 2]"""
    w = effective_window(win, stance, use_swing)
    return np.stack([w[..., :COORDS] - V, V - w[..., COORDS:]], axis=-1)


def phi(V, win, stance, mu, rho, use_swing=True):
    """the term (max(0, mu + rho c)^2 - mu^2) / (2 rho) per constraint [..., 9, 2]"""
    return (np.maximum(mu + rho * constraints(V, win, stance, use_swing), 0.0) ** 2 - mu ** 2) / (2.0 * rho)


def m_and_scale(V, win, stance, mu, rho, use_swing=True):
    """(m [..., 9] = s_hi - s_lo, the gradient with respect to the velocity; n [..., 9] = rho per active side, its curvature along J_k)"""
    s = mu + rho * constraints(V, win, stance, use_swing)
    sp = np.maximum(s, 0.0)
    return sp[..., 1] - sp[..., 0], (rho * (s > 0.0)).sum(axis=-1)


# keys of a task-velocity-bounds record: name -> first coordinate (three each), in the order of the coordinates
_AL_TASK_VEL_FIELDS = {"com_vel": 0, "left_foot_vel": 3, "right_foot_vel": 6}


def stack_al_task_vel_bounds(records, B, N):
    """Task-velocity windows [n, N+1, 18] of the restated family (the solver has no setter for them yet): row t holds knot t's lo[9], hi[9] in m/s over the
    velocities of the CoM x, y, z, of the left ankle origin x, y, z and of the right ankle origin x, y, z (world frame).  records is one
    dict (n = 1: every rollout reads the window) or a sequence of B dicts (n = B).  Every key is optional: "com_vel", "left_foot_vel",
    "right_foot_vel" take a pair (lo, hi), each a scalar, [3] (the whole horizon) or [N+1, 3] (one row per knot); the shorthands
    "stance_slip": s sets |v| <= s on the three axes of both feet (a foot's rows count at its stance knots only, so this bounds
    the slip of the stance phases) and "com_speed_xy": (vx, vy) the symmetric caps |v_x| <= vx, |v_y| <= vy on the CoM.  A shorthand is
    applied after the key it refines.  A key left out gives -inf / +inf: no bound.  Raises ValueError for another key, a wrong shape, a
    negative cap, a sequence that is not B long, or a window with a NaN, lo > hi, lo = +inf or hi = -inf."""
    B, N = int(B), int(N)
    if B < 1 or N < 1:
        raise ValueError("B and N must be positive")
    if isinstance(records, dict):
        records = [records]
    else:
        records = list(records)
        if len(records) != B:
            raise ValueError("records must be one dict or B of them")
    out = np.empty((len(records), N + 1, 18))
    out[:, :, :9] = -np.inf; out[:, :, 9:] = np.inf

    def rows(name, v):
        v = np.asarray(v, dtype=np.float64)
        if v.shape not in ((), (3,), (N + 1, 3)):
            raise ValueError("%s: lo and hi are scalars, [3] or [N+1, 3]" % name)
        return np.broadcast_to(v, (N + 1, 3))

    for b, rec in enumerate(records):
        if not isinstance(rec, dict):
            raise ValueError("a task-velocity-bounds record is a dict")
        extra = set(rec) - set(_AL_TASK_VEL_FIELDS) - {"stance_slip", "com_speed_xy"}
        if extra:
            raise ValueError("unknown task-velocity-bounds field(s) %s: a record has %s, stance_slip and com_speed_xy" % (sorted(extra), list(_AL_TASK_VEL_FIELDS)))
        for name, k0 in _AL_TASK_VEL_FIELDS.items():
            if rec.get(name) is not None:
                try:
                    lo, hi = rec[name]
                except (TypeError, ValueError):
                    raise ValueError("%s takes a pair (lo, hi)" % name)
                out[b, :, k0:k0 + 3], out[b, :, 9 + k0:9 + k0 + 3] = rows(name, lo), rows(name, hi)
        if rec.get("stance_slip") is not None:
            s_ = np.asarray(rec["stance_slip"], dtype=np.float64)
            if s_.shape != () or not s_ >= 0.0:
                raise ValueError("stance_slip is one speed >= 0")
            out[b, :, 3:9], out[b, :, 12:18] = -float(s_), float(s_)
        if rec.get("com_speed_xy") is not None:
            c = np.asarray(rec["com_speed_xy"], dtype=np.float64)
            if c.shape != (2,) or not (c >= 0.0).all():
                raise ValueError("com_speed_xy is (vx, vy), both >= 0")
            out[b, :, 0:2], out[b, :, 9:11] = -c, c
    lo, hi = out[..., :9], out[..., 9:]
    if np.isnan(out).any() or (lo > hi).any() or (lo == np.inf).any() or (hi == -np.inf).any():
        raise ValueError("task-velocity bounds: no NaN, lo <= hi, lo < +inf, hi > -inf")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
class Kin:
    """Jacobian rows and second-order sums of the nine velocities from the oracle's velocity terms (module docstring)."""

    def __init__(self, w=1.0):
        import al_cases as ac
        self.w = float(w)
        p = dict(ac.sc.make_problem(ol.reference_kinematics, N=1, stance=np.zeros((2, 2), dtype=np.int32)))
        p["Q"] = np.zeros(NX); p["Qf"] = np.zeros(NX); p["R"] = np.zeros(NU)
        p["task_weights"] = (0.0, self.w, 0.0, 0.0, 0.0, 0.0); p["w_joint"] = 0.0; p["w_ctrl"] = 0.0
        self.p = p
        self.o = ol.Oracle(1, p["dt"])

    def _com(self, x, ref):
        """(lx, lxx) of the one-knot oracle whose only term is w |v_com - ref|^2"""
        p = self.p
        p["com_vel_ref"] = np.tile(np.asarray(ref, dtype=np.float64), (1, 2, 1))
        self.o.set_problem(p)
        lx, _, lxx, _ = self.o.knot_quadratics(0, x, None, 0)
        return lx, lxx

    def jacobian(self, x, vel=None):
        """J [9, 51]: row k = d v_k / d x (slot convention of the quadratics)"""
        vel = velocities(x) if vel is None else vel
        J = np.zeros((COORDS, NX))
        E = np.eye(3) / (2.0 * self.w)
        for k in range(3):
            J[k] = self._com(x, vel[:3] - E[k])[0]
        sets = np.repeat([1, 2], 3)
        tg = np.concatenate([vel[3:6] - E, vel[6:9] - E])
        J[3:] = vel_terms(sets, self.w, np.tile(x, (6, 1)), tg)[1]
        return J

    def curvature(self, x, m, vel=None):
        """sum_k m_k d2 v_k / dx2 [51, 51]"""
        vel = velocities(x) if vel is None else vel
        m = np.asarray(m, dtype=np.float64)
        H = np.zeros((NX, NX))
        if m[:3].any():
            H += self._com(x, vel[:3] - m[:3] / (2.0 * self.w))[1] - self._com(x, vel[:3])[1]
        for s_ in (1, 2):
            ms = m[3 * s_:3 * s_ + 3]
            if ms.any():
                vs = vel[3 * s_:3 * s_ + 3]
                _, _, h = vel_terms([s_, s_], self.w, np.tile(x, (2, 1)), np.stack([vs - ms / (2.0 * self.w), vs]))
                H += h[0] - h[1]
        return H


@functools.lru_cache(maxsize=None)
def kin(w=1.0):
    return Kin(w)


def traj_terms(X, mu_v, rho_v, win, stance, use_swing=True, k=None):
    """One rollout: X [N+1,51], mu_v [N+1,9,2], win [N+1,18], stance [N+1,2].  Returns (cost added per knot [N+1], gx [N+1,51] to add to lx,
    hxx [N+1,51,51] to add to lxx); every knot, the terminal one included.  Exact Hessian: sum_k n_k J_k^T J_k + sum_k m_k d2 v_k."""
    k = k or kin()
    V = velocities(X)
    ck = phi(V, win, stance, mu_v, rho_v, use_swing).sum(axis=(1, 2))
    m, n = m_and_scale(V, win, stance, mu_v, rho_v, use_swing)
    gx, hxx = np.zeros((X.shape[0], NX)), np.zeros((X.shape[0], NX, NX))
    for t in range(X.shape[0]):
        if not (m[t].any() or n[t].any()):
            continue
        J = k.jacobian(X[t], V[t])
        gx[t] = J.T @ m[t]
        hxx[t] = (J.T * n[t]) @ J + k.curvature(X[t], m[t], V[t])
    return ck, gx, hxx


add_to_quadratics = tr.add_to_quadratics


def violation(X, win, stance):
    """the largest max(0, c) over the knots 1..N (x_0 is given), rows of swinging feet left out; m/s"""
    return max(0.0, float(constraints(velocities(X[1:]), win[1:], stance[1:]).max()))


def update_taskvel(X, mu_v, rho_v, win, stance):
    """(mu_v+ [N+1,9,2], viol_taskvel): mu <- max(0, mu + rho c) at the knots 1..N, knot 0 kept"""
    c = constraints(velocities(X), win, stance)
    nv = np.maximum(0.0, mu_v + rho_v * c); nv[0] = mu_v[0]
    return nv, max(0.0, float(c[1:].max()))


def update(X, U, mu_j, mu_c, mu_s, mu_t, mu_v, rho, done, rec, srec, twin, vwin, stance, growth, rho_max, tol):
    """The update after an inner solve over the five families, one rollout.  rho, rho_max, tol: 5-tuples (joint, ctrl, state, task, taskvel);
    srec / twin / vwin None: that family is not installed (its entries of rho / tol are carried along unread).  Returns (mu_j+, mu_c+, mu_s+,
    mu_t+, mu_v+, rho+, done+, viol [5]).  Done needs every family within tolerance; otherwise all penalties grow.  A rollout that was done
    keeps everything."""
    N1 = X.shape[0]
    tw = np.tile(tr.NO_BOUNDS, (N1, 1)) if twin is None else twin
    vw = np.tile(NO_BOUNDS, (N1, 1)) if vwin is None else vwin
    nj, nc, ns, nt, _, _, v4 = tr.update(X, U, mu_j, mu_c, mu_s, mu_t, rho[:4], False, rec, srec, tw, stance, growth, rho_max[:4], tol[:4])
    nv, vv = update_taskvel(X, mu_v, rho[4], vw, stance)
    viol = tuple(v4) + (vv,)
    if done:
        return mu_j, mu_c, mu_s, mu_t, mu_v, tuple(rho), True, viol
    ok = all(v <= t for v, t in zip(viol, tol))
    rho2 = tuple(rho) if ok else tuple(min(r * growth, m) for r, m in zip(rho, rho_max))
    return nj, nc, ns, nt, nv, rho2, ok, viol


def shift(mu_v, s):
    """Warm start shifted by s knots: new[t] = old[t + s] for 1 <= t <= N - s, zero elsewhere (knot 0 and the tail)."""
    return sr.shift(mu_v, s)


class Driver(tr.Driver):
    """al_task_ref.Driver with the task-velocity family on top: AL solve of ONE rollout under its joint / torque record rec [76], its state
    record srec [56] (None: every side off), its task window win [N+1, 18] (None: no task family) and its task-velocity window vwin
    [N+1, 18] (None: no task-velocity family).  al: the dict of al_task_cases.AL_E2E plus rho_taskvel0 and tol_taskvel."""

    def __init__(self, prob, b, al, rec, srec, win, vwin, **kw):
        super().__init__(prob, b, al, rec, srec, win, **kw)
        self.vwin = None if vwin is None else np.array(vwin, dtype=np.float64)
        self.mu_v = np.zeros((self.N + 1, COORDS, 2))
        self.rho_v = al.get("rho_taskvel0", 1.0)

    def cost(self, X, U):
        c = super().cost(X, U)
        if self.vwin is not None:
            c += float(phi(velocities(X), self.vwin, self.stance, self.mu_v, self.rho_v).sum())
        return c

    def _task(self, X):
        """the task family's terms with this family's added (al_task_ref.Driver.inner adds what this returns to lx and lxx)"""
        N1 = X.shape[0]
        ck, gx, hx = (np.zeros(N1), np.zeros((N1, NX)), np.zeros((N1, NX, NX))) if self.win is None else super()._task(X)
        if self.vwin is not None:
            c2, g2, h2 = traj_terms(X, self.mu_v, self.rho_v, self.vwin, self.stance)
            ck, gx, hx = ck + c2, gx + g2, hx + h2
        return ck, gx, hx

    def inner(self, x0, X, U):
        # al_task_ref.Driver.inner adds _task() where its window is set: lend it an all-infinite one (every term of it is an exact zero) while
        # only this family is installed
        lend = self.win is None and self.vwin is not None
        if lend:
            self.win = np.tile(tr.NO_BOUNDS, (self.N + 1, 1))
        try:
            return super().inner(x0, X, U)
        finally:
            if lend:
                self.win = None

    def solve(self, x0, u_init):
        """Cold start and up to `rounds` rounds.  The dict of al_task_ref.Driver.solve plus mu_v, rho_v, viol (five values) and taskvel_trace
        [rounds, 2] = (viol_taskvel, rho_taskvel the round ran with)."""
        al = self.al
        rounds = al["rounds"]
        U = np.array(u_init, dtype=np.float64); X = self.roll(x0, U)
        out = dict(rounds=[], al_trace=np.full((rounds, 5), np.nan), state_trace=np.full((rounds, 2), np.nan), task_trace=np.full((rounds, 2), np.nan),
                   taskvel_trace=np.full((rounds, 2), np.nan))
        done, viol = False, (0.0,) * 5
        rho0 = (al["rho_joint0"], al["rho_ctrl0"], al.get("rho_state0", 1.0), al.get("rho_task0", 1.0), al.get("rho_taskvel0", 1.0))
        rho_max = tuple(r * al["rho_max_factor"] for r in rho0)
        tol = (al["tol_joint"], al["tol_ctrl"], al.get("tol_state", 0.0), al.get("tol_task", 0.0), al.get("tol_taskvel", 0.0))
        for r in range(rounds):
            if done and self.early_exit:
                break
            X, U, J, tc, ta, tl, it = self.inner(x0, X, U)
            out["rounds"].append(dict(trace_cost=tc, trace_alpha=ta, trace_lambda=tl, iterations=it, cost=J))
            used = tuple(self.rho) + (self.rho_s, self.rho_t, self.rho_v)
            self.mu_j, self.mu_c, self.mu_s, self.mu_t, self.mu_v, rho5, done, viol = update(
                X, U, self.mu_j, self.mu_c, self.mu_s, self.mu_t, self.mu_v, used, done, self.rec, self.srec, self.win, self.vwin, self.stance,
                al["growth"], rho_max, tol)
            self.rho, self.rho_s, self.rho_t, self.rho_v = rho5[:2], rho5[2], rho5[3], rho5[4]
            out["al_trace"][r] = (viol[0], viol[1], used[0], used[1], it)
            out["state_trace"][r] = (viol[2], used[2])
            out["task_trace"][r] = (viol[3], used[3])
            out["taskvel_trace"][r] = (viol[4], used[4])
        out.update(X=X, U=U, cost=J, mu_j=self.mu_j, mu_c=self.mu_c, mu_s=self.mu_s, mu_t=self.mu_t, mu_v=self.mu_v, rho=self.rho, rho_s=self.rho_s,
                   rho_t=self.rho_t, rho_v=self.rho_v, viol=viol, done=done, lam=self.lam)
        return out
