"""CPU restatement of the task family of the augmented-Lagrangian limits (include/ilqr_hip.h ilqr_hip_set_al_task_bounds): bounds on nine
points of the robot in the world frame -- task coordinate k = 0..2 the whole-body CoM, 3..5 the left ankle origin, 6..8 the right ankle
origin -- with the term, its gradient and its exact Hessian, the update over four families, the violation, the done rule, the growth of
the penalties and the warm-start shift in NumPy, on top of al_state_ref.py, and an AL solve driver with the fourth family.

The points are the ones the cost's tracking terms (w_com, w_ee_pos) track -- Pinocchio conventions, the rotation polynomial on the raw
quaternion, for the CoM the URDF link masses -- because the family's gradient and Hessian are those points'.  For a unit quaternion the
ankle origins are oracle_lib.reference_kinematics' to 1e-16; its CoM is that of the MuJoCo model (other ankle and hand masses), ~3 mm
away.  Each point is read off the oracle's tracking term: with only that point's weight w on and reference r (reference_kinematics'
value), lx[0:3] = 2 w (p - r).  Their Jacobian rows J_k and the second-order sum  sum_k m_k d2 p_k  come from the
oracle's own tracking terms, never from the code under test: on a one-knot oracle whose only weights are w_com = w_ee_pos = w and whose
feet are in swing, the tracking cost  w |p - ref|^2  has the gradient 2 w J^T (p - ref) and the Hessian 2 w J^T J + sum_k 2 w (p - ref)_k
d2 p_k.  So with ref = p - e_k / (2 w) the gradient is J_k, and the Hessian at ref = p - m / (2 w) minus the Hessian at ref = p is
sum_k m_k d2 p_k.  Two weights w give the same numbers to ~1e-13 (test_al_task_cpu.py prints the figure).

A window is [N+1, 18], row t = lo[9], hi[9]; task multipliers are arrays [..., 9, 2] = (lower, upper), as the interface has them.  An
infinite side gives c = -inf, max(0, mu + rho c) = 0 and the constant term -mu^2 / (2 rho).  A foot's three rows at a knot where the
schedule has it in stance (flag 1) are rows with both sides switched off.  No GPU."""
import functools

import numpy as np

import al_bounds_ref as br
import al_ref as ar
import al_state_ref as sr
import oracle_lib as ol

NX, NU, NQ = ar.NX, ar.NU, ar.NQ
COORDS, AL_TASK_BOUNDS = 9, 18
NO_BOUNDS = np.concatenate([np.full(COORDS, -np.inf), np.full(COORDS, np.inf)])
FOOT_OF = np.array([-1, -1, -1, 0, 0, 0, 1, 1, 1])      # the foot a task coordinate belongs to (-1: the CoM)


def points(X):
    """task coordinates [..., 9] of states X [..., 51]"""
    X = np.asarray(X, dtype=np.float64)
    flat = X.reshape(-1, NX)
    out = np.zeros((flat.shape[0], COORDS))
    for i, x in enumerate(flat):
        com, ee = ol.reference_kinematics(x)
        r = np.concatenate([com, ee[0], ee[1]])
        for s_ in range(3):
            out[i, 3 * s_:3 * s_ + 3] = r[3 * s_:3 * s_ + 3] + kin_set(s_)._quad(x, r)[0][:3] / 2.0
    return out.reshape(X.shape[:-1] + (COORDS,))


def rows_off(stance):
    """[..., 9] bool: the rows the stance rule switches off, from stance flags [..., 2]"""
    stance = np.asarray(stance)
    off = np.zeros(stance.shape[:-1] + (COORDS,), dtype=bool)
    off[..., 3:6] = (stance[..., 0] == 1)[..., None]
    off[..., 6:9] = (stance[..., 1] == 1)[..., None]
    return off


def effective_window(win, stance, use_stance=True):
    """the window with the rows of stance feet made infinite: what the solver acts on"""
    win = np.array(win, dtype=np.float64)
    assert win.shape[-1] == AL_TASK_BOUNDS
    if use_stance:
        off = rows_off(stance)
        win[..., :COORDS] = np.where(off, -np.inf, win[..., :COORDS])
        win[..., COORDS:] = np.where(off, np.inf, win[..., COORDS:])
    return win


def constraints(P, win, stance, use_stance=True):
    """c [..., 9, 2] = (lo - p, p - hi) of points P [..., 9] against rows win [..., 18] under stance flags [..., 2]"""
    w = effective_window(win, stance, use_stance)
    return np.stack([w[..., :COORDS] - P, P - w[..., COORDS:]], axis=-1)


def phi(P, win, stance, mu, rho, use_stance=True):
    """the term (max(0, mu + rho c)^2 - mu^2) / (2 rho) per constraint [..., 9, 2]"""
    return (np.maximum(mu + rho * constraints(P, win, stance, use_stance), 0.0) ** 2 - mu ** 2) / (2.0 * rho)


def m_and_scale(P, win, stance, mu, rho, use_stance=True):
    """(m [..., 9] = s_hi - s_lo, the gradient with respect to the point; n [..., 9] = rho per active side, its curvature along J_k)"""
    s = mu + rho * constraints(P, win, stance, use_stance)
    sp = np.maximum(s, 0.0)
    return sp[..., 1] - sp[..., 0], (rho * (s > 0.0)).sum(axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
class Kin:
    """Jacobian rows and second-order sums of the nine task coordinates from the oracle's tracking terms (module docstring)."""

    def __init__(self, w=1.0, only=None):
        """only: None every point; else the one point set 0 (CoM), 1 (left ankle), 2 (right ankle) -- the other foot in stance, whose position
        term is then off"""
        import al_cases as ac
        self.w = float(w)
        w_com = self.w if only in (None, 0) else 0.0
        w_ee = self.w if only in (None, 1, 2) else 0.0
        stance = np.zeros((2, 2), dtype=np.int32)
        if only in (1, 2):
            stance[:, 2 - only] = 1
        p = dict(ac.sc.make_problem(ol.reference_kinematics, N=1, stance=stance))
        p["Q"] = np.zeros(NX); p["Qf"] = np.zeros(NX); p["R"] = np.zeros(NU)
        p["task_weights"] = (w_com, 0.0, w_ee, 0.0, 0.0, 0.0); p["w_joint"] = 0.0; p["w_ctrl"] = 0.0
        self.p = p
        self.o = ol.Oracle(1, p["dt"])

    def _quad(self, x, ref):
        p = self.p
        p["com_ref"] = np.tile(ref[:3], (1, 2, 1)); p["ee_ref"] = np.tile(ref[3:].reshape(2, 3), (1, 2, 1, 1))
        self.o.set_problem(p)
        lx, _, lxx, _ = self.o.knot_quadratics(0, x, None, 0)
        return lx, lxx

    def jacobian(self, x, pts=None):
        """J [9, 51]: row k = d p_k / d x"""
        pts = points(x) if pts is None else pts
        J = np.zeros((COORDS, NX))
        for k in range(COORDS):
            e = np.zeros(COORDS); e[k] = 1.0
            J[k] = self._quad(x, pts - e / (2.0 * self.w))[0]
        return J

    def curvature(self, x, m, pts=None):
        """sum_k m_k d2 p_k / dx2 [51, 51]"""
        pts = points(x) if pts is None else pts
        if not np.any(m):
            return np.zeros((NX, NX))
        return self._quad(x, pts - np.asarray(m) / (2.0 * self.w))[1] - self._quad(x, pts)[1]


@functools.lru_cache(maxsize=None)
def kin(w=1.0):
    return Kin(w)


@functools.lru_cache(maxsize=None)
def kin_set(s_):
    """the oracle with the tracking term of point set s_ alone, weight 1 (points())"""
    return Kin(1.0, s_)


def traj_terms(X, mu_t, rho_t, win, stance, use_stance=True, k=None):
    """One rollout: X [N+1,51], mu_t [N+1,9,2], win [N+1,18], stance [N+1,2].  Returns (cost added per knot [N+1], gx [N+1,51] to add to lx,
    hxx [N+1,51,51] to add to lxx); every knot, the terminal one included.  Exact Hessian: sum_k n_k J_k^T J_k + sum_k m_k d2 p_k."""
    k = k or kin()
    P = points(X)
    ck = phi(P, win, stance, mu_t, rho_t, use_stance).sum(axis=(1, 2))
    m, n = m_and_scale(P, win, stance, mu_t, rho_t, use_stance)
    gx, hxx = np.zeros((X.shape[0], NX)), np.zeros((X.shape[0], NX, NX))
    for t in range(X.shape[0]):
        if not (m[t].any() or n[t].any()):
            continue
        J = k.jacobian(X[t], P[t])
        gx[t] = J.T @ m[t]
        hxx[t] = (J.T * n[t]) @ J + k.curvature(X[t], m[t], P[t])
    return ck, gx, hxx


def add_to_quadratics(q, gx, hxx):
    q["lx"] += gx; q["lxx"] += hxx
    return q


def violation(X, win, stance):
    """the largest max(0, c) over the knots 1..N (x_0 is given), rows of stance feet left out"""
    return max(0.0, float(constraints(points(X[1:]), win[1:], stance[1:]).max()))


def update_task(X, mu_t, rho_t, win, stance):
    """(mu_t+ [N+1,9,2], viol_task): mu <- max(0, mu + rho c) at the knots 1..N, knot 0 kept"""
    c = constraints(points(X), win, stance)
    nt = np.maximum(0.0, mu_t + rho_t * c); nt[0] = mu_t[0]
    return nt, max(0.0, float(c[1:].max()))


def update(X, U, mu_j, mu_c, mu_s, mu_t, rho, done, rec, srec, win, stance, growth, rho_max, tol):
    """The update after an inner solve over the four families, one rollout.  rho, rho_max, tol: 4-tuples (joint, ctrl, state, task); srec None:
    no state family (its entries of rho / tol are carried along unread).  Returns (mu_j+, mu_c+, mu_s+, mu_t+, rho+, done+, viol [4]).  Done
    needs every family within tolerance; otherwise all penalties grow.  A rollout that was done keeps everything."""
    s_rec = sr.NO_BOUNDS if srec is None else srec
    nj, nc, ns, _, _, v3 = sr.update(X, U, mu_j, mu_c, mu_s, rho[:3], False, rec, s_rec, growth, rho_max[:3], tol[:3])
    nt, vt = update_task(X, mu_t, rho[3], win, stance)
    viol = tuple(v3) + (vt,)
    if done:
        return mu_j, mu_c, mu_s, mu_t, tuple(rho), True, viol
    ok = all(v <= t for v, t in zip(viol, tol))
    rho2 = tuple(rho) if ok else tuple(min(r * growth, m) for r, m in zip(rho, rho_max))
    return nj, nc, ns, nt, rho2, ok, viol


def shift(mu_t, s):
    """Warm start shifted by s knots: new[t] = old[t + s] for 1 <= t <= N - s, zero elsewhere (knot 0 and the tail)."""
    return sr.shift(mu_t, s)


class Driver(sr.Driver):
    """al_state_ref.Driver with the task family on top: AL solve of ONE rollout under its joint / torque record rec [76], its state record
    srec [56] (None: every side off) and its task window win [N+1, 18] (None: no task family).  al: the dict of al_state_cases.AL_E2E plus
    rho_task0 and tol_task.  The contact schedule is reference set b's of prob."""

    def __init__(self, prob, b, al, rec, srec, win, **kw):
        super().__init__(prob, b, al, rec, sr.NO_BOUNDS if srec is None else srec, **kw)
        st = np.asarray(prob["stance"])
        self.stance = np.array(st[b] if st.shape[0] > 1 else st[0])
        self.win = None if win is None else np.array(win, dtype=np.float64)
        self.mu_t = np.zeros((self.N + 1, COORDS, 2))
        self.rho_t = al.get("rho_task0", 1.0)

    def _task(self, X):
        return traj_terms(X, self.mu_t, self.rho_t, self.win, self.stance)

    def cost(self, X, U):
        c = super().cost(X, U)
        if self.win is not None:
            c += float(phi(points(X), self.win, self.stance, self.mu_t, self.rho_t).sum())
        return c

    def inner(self, x0, X, U):
        """al_state_ref.Driver.inner with the task terms added to lx and lxx"""
        o, n = self.o, self.max_iter
        tc, ta, tl = np.full(n + 1, np.nan), np.full(n, np.nan), np.full(n, np.nan)
        J = self.cost(X, U); tc[0] = J
        it = 0
        for i in range(n):
            it = i + 1
            Jprev = J
            X = self.roll(x0, U)
            o.set_trajectory(X, U); o.linearize(); o.cost_quadratics()
            q = {k: o.get(k) for k in ("lx", "lu", "lxx", "luu")}
            _, gx, hx, gu, hu = self._al(X, U)
            idx = np.arange(7, NQ)
            q["lx"][:, 7:NQ] += gx; q["lu"] += gu; q["luu"] += hu; q["lxx"][:, idx, idx] += hx
            _, sg, sh = sr.traj_terms(X, self.mu_s, self.rho_s, self.srec)
            sr.add_to_quadratics(q, sg, sh)
            if self.win is not None:
                _, tg, th = self._task(X)
                add_to_quadratics(q, tg, th)
            quad = (q["lx"], q["lu"], q["lxx"], q["luu"])
            J0 = self.cost(X, U)
            used = self.lam
            ok, Xn, Un, Jn, a = self._pass(x0, X, U, quad, self.lam, J0)
            if not ok:
                self.lam = min(self.lam * 10.0, 1e-3); used = self.lam
                ok, Xn, Un, Jn, a = self._pass(x0, X, U, quad, self.lam, J0)
                if not ok:
                    tc[i + 1], ta[i], tl[i] = J, 0.0, used
                    if self.early_exit and i > 1:
                        break
                    continue
            X, U, J = Xn, Un, Jn
            tc[i + 1], ta[i], tl[i] = J, a, used
            self.lam = max(self.lam / 2.0, 1e-6)
            if self.early_exit and (abs(J - Jprev) < self.tol or J > 1e6):
                break
        return X, U, J, tc, ta, tl, it

    def solve(self, x0, u_init):
        """Cold start and up to `rounds` rounds.  The dict of al_state_ref.Driver.solve plus mu_t, rho_t, viol (four values) and task_trace
        [rounds, 2] = (viol_task, rho_task the round ran with)."""
        al = self.al
        rounds = al["rounds"]
        U = np.array(u_init, dtype=np.float64); X = self.roll(x0, U)
        out = dict(rounds=[], al_trace=np.full((rounds, 5), np.nan), state_trace=np.full((rounds, 2), np.nan), task_trace=np.full((rounds, 2), np.nan))
        done, viol = False, (0.0, 0.0, 0.0, 0.0)
        rho0 = (al["rho_joint0"], al["rho_ctrl0"], al.get("rho_state0", 1.0), al.get("rho_task0", 1.0))
        rho_max = tuple(r * al["rho_max_factor"] for r in rho0)
        win = np.tile(NO_BOUNDS, (self.N + 1, 1)) if self.win is None else self.win
        for r in range(rounds):
            if done and self.early_exit:
                break
            X, U, J, tc, ta, tl, it = self.inner(x0, X, U)
            out["rounds"].append(dict(trace_cost=tc, trace_alpha=ta, trace_lambda=tl, iterations=it, cost=J))
            used = tuple(self.rho) + (self.rho_s, self.rho_t)
            self.mu_j, self.mu_c, self.mu_s, self.mu_t, rho4, done, viol = update(
                X, U, self.mu_j, self.mu_c, self.mu_s, self.mu_t, used, done, self.rec, self.srec, win, self.stance, al["growth"], rho_max,
                (al["tol_joint"], al["tol_ctrl"], al.get("tol_state", 0.0), al.get("tol_task", 0.0)))
            self.rho, self.rho_s, self.rho_t = rho4[:2], rho4[2], rho4[3]
            out["al_trace"][r] = (viol[0], viol[1], used[0], used[1], it)
            out["state_trace"][r] = (viol[2], used[2])
            out["task_trace"][r] = (viol[3], used[3])
        out.update(X=X, U=U, cost=J, mu_j=self.mu_j, mu_c=self.mu_c, mu_s=self.mu_s, mu_t=self.mu_t, rho=self.rho, rho_s=self.rho_s, rho_t=self.rho_t,
                   viol=viol, done=done, lam=self.lam)
        return out
