"""CPU restatement of the state family of the augmented-Lagrangian limits (include/ilqr_hip.h ilqr_hip_set_al_state_bounds): bounds on the
28 box coordinates -- pelvis position (state slots 0..2), pelvis linear and angular velocity (26..31), joint velocities (32..50) -- with
the term, its gradient and curvature, the update over three families, the violation, the done rule, the growth of the penalties and the
warm-start shift in NumPy, next to al_bounds_ref.py (whose joint / torque family it reuses under an explicit record: the model's bounds
are al_bounds_ref.default_record(margin)), and an AL solve driver on the oracle's stage calls extended by the state terms.

A state record is [56] = lo[28], hi[28]; state multipliers are arrays [..., 28, 2] = (lower, upper), as the interface has them.  An
infinite side gives c = -inf, max(0, mu + rho c) = 0 and the constant term -mu^2 / (2 rho).  No GPU."""
import numpy as np

import al_bounds_ref as br
import al_ref as ar

NX, NU, NQ = ar.NX, ar.NU, ar.NQ
COORDS, AL_STATE_BOUNDS = 28, 56
SLOTS = np.array([k if k < 3 else 23 + k for k in range(COORDS)])
NO_BOUNDS = np.concatenate([np.full(COORDS, -np.inf), np.full(COORDS, np.inf)])


def split(srec):
    srec = np.asarray(srec, dtype=np.float64)
    assert srec.shape == (AL_STATE_BOUNDS,)
    return srec[:COORDS], srec[COORDS:]


def constraints(X, srec, slots=SLOTS):
    """c [..., 28, 2] = (lo - x_slot, x_slot - hi) of states X [..., 51]"""
    lo, hi = split(srec)
    v = X[..., slots]
    return np.stack([lo - v, v - hi], axis=-1)


def _s(X, srec, mu, rho, slots):
    return mu + rho * constraints(X, srec, slots)


def phi(X, srec, mu, rho, slots=SLOTS):
    """the term (max(0, mu + rho c)^2 - mu^2) / (2 rho) per constraint [..., 28, 2]"""
    return (np.maximum(_s(X, srec, mu, rho, slots), 0.0) ** 2 - mu ** 2) / (2.0 * rho)


def grad(X, srec, mu, rho, slots=SLOTS):
    """d / d x_slot of the two terms of each coordinate [..., 28]"""
    sp = np.maximum(_s(X, srec, mu, rho, slots), 0.0)
    return sp[..., 1] - sp[..., 0]


def hess(X, srec, mu, rho, slots=SLOTS):
    """its second derivative [..., 28]: rho per constraint with mu + rho c > 0"""
    return (rho * (_s(X, srec, mu, rho, slots) > 0.0)).sum(axis=-1)


def traj_terms(X, mu_s, rho_s, srec, slots=SLOTS):
    """One rollout: X [N+1,51], mu_s [N+1,28,2].  Returns (cost added per knot [N+1], gx [N+1,28] to add to lx[:, slots], hx [N+1,28] to the
    diagonal of lxx at the slots); every knot, the terminal one included."""
    return phi(X, srec, mu_s, rho_s, slots).sum(axis=(1, 2)), grad(X, srec, mu_s, rho_s, slots), hess(X, srec, mu_s, rho_s, slots)


def add_to_quadratics(q, gx, hx, slots=SLOTS):
    """lx, lxx of one rollout (dict, modified in place) with the state family's gradient and curvature"""
    q["lx"][:, slots] += gx
    q["lxx"][:, slots, slots] += hx
    return q


def violation(X, srec):
    """the largest max(0, c) over the knots 1..N (x_0 is given)"""
    return max(0.0, float(constraints(X[1:], srec).max()))


def update(X, U, mu_j, mu_c, mu_s, rho, done, rec, srec, growth, rho_max, tol):
    """The update after an inner solve over the three families, one rollout.  rho, rho_max, tol: triples (joint, ctrl, state); rec [76] the
    joint / torque record, srec [56] the state record.  Returns (mu_j+, mu_c+, mu_s+, rho+, done+, (viol_joint, viol_ctrl, viol_state)).  Done
    needs all three within tolerance; otherwise all three penalties grow.  A rollout that was done keeps everything."""
    (jl, jh), (cl, ch) = br.split(rec)
    cj, cc, cs = br.constraints(X[:, 7:NQ], jl, jh), br.constraints(U, cl, ch), constraints(X, srec)
    viol = (max(0.0, float(cj[1:].max())), max(0.0, float(cc.max())), max(0.0, float(cs[1:].max())))
    if done:
        return mu_j, mu_c, mu_s, tuple(rho), True, viol
    nj = np.maximum(0.0, mu_j + rho[0] * cj); nj[0] = mu_j[0]
    nc = np.maximum(0.0, mu_c + rho[1] * cc)
    ns = np.maximum(0.0, mu_s + rho[2] * cs); ns[0] = mu_s[0]
    ok = all(v <= t for v, t in zip(viol, tol))
    rho2 = tuple(rho) if ok else tuple(min(r * growth, m) for r, m in zip(rho, rho_max))
    return nj, nc, ns, rho2, ok, viol


def shift(mu_s, s):
    """Warm start shifted by s knots: new[t] = old[t + s] for 1 <= t <= N - s, zero elsewhere (knot 0 and the tail)."""
    ns = np.zeros_like(mu_s)
    N = mu_s.shape[-3] - 1
    if s <= N - 1:
        ns[..., 1:N - s + 1, :, :] = mu_s[..., 1 + s:N + 1, :, :]
    return ns


class Driver(br.Driver):
    """al_bounds_ref.Driver with the state family on top: AL solve of ONE rollout under its joint / torque record rec [76] and its state
    record srec [56].  al: the dict of al_cases.AL_E2E plus rho_state0 and tol_state.  The line search, the lambda schedule, the retry and
    the exits are al_ref.Driver's; the cost, the quadratics and the update carry the third family."""

    def __init__(self, prob, b, al, rec, srec, **kw):
        super().__init__(prob, b, al, rec, **kw)
        self.srec = np.array(srec, dtype=np.float64)
        self.mu_s = np.zeros((self.N + 1, COORDS, 2))
        self.rho_s = al["rho_state0"]

    def cost(self, X, U):
        return super().cost(X, U) + float(traj_terms(X, self.mu_s, self.rho_s, self.srec)[0].sum())

    def inner(self, x0, X, U):
        """al_ref.Driver.inner with the state terms added to lx and the diagonal of lxx"""
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
            _, sg, sh = traj_terms(X, self.mu_s, self.rho_s, self.srec)
            add_to_quadratics(q, sg, sh)
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
        """Cold start and up to `rounds` rounds.  The dict of al_ref.Driver.solve plus mu_s, rho_s, viol (three values) and state_trace
        [rounds, 2] = (viol_state, rho_state the round ran with); al_trace stays [rounds, 5]."""
        al = self.al
        rounds = al["rounds"]
        U = np.array(u_init, dtype=np.float64); X = self.roll(x0, U)
        out = dict(rounds=[], al_trace=np.full((rounds, 5), np.nan), state_trace=np.full((rounds, 2), np.nan))
        done, viol = False, (0.0, 0.0, 0.0)
        rho0 = (al["rho_joint0"], al["rho_ctrl0"], al["rho_state0"])
        rho_max = tuple(r * al["rho_max_factor"] for r in rho0)
        for r in range(rounds):
            if done and self.early_exit:
                break
            X, U, J, tc, ta, tl, it = self.inner(x0, X, U)
            out["rounds"].append(dict(trace_cost=tc, trace_alpha=ta, trace_lambda=tl, iterations=it, cost=J))
            used = tuple(self.rho) + (self.rho_s,)
            self.mu_j, self.mu_c, self.mu_s, rho3, done, viol = update(X, U, self.mu_j, self.mu_c, self.mu_s, used, done, self.rec, self.srec, al["growth"], rho_max,
                                                                       (al["tol_joint"], al["tol_ctrl"], al["tol_state"]))
            self.rho, self.rho_s = rho3[:2], rho3[2]
            out["al_trace"][r] = (viol[0], viol[1], used[0], used[1], it)
            out["state_trace"][r] = (viol[2], used[2])
        out.update(X=X, U=U, cost=J, mu_j=self.mu_j, mu_c=self.mu_c, mu_s=self.mu_s, rho=self.rho, rho_s=self.rho_s, viol=viol, done=done, lam=self.lam)
        return out
