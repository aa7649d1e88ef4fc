"""CPU restatement of the augmented-Lagrangian joint and torque limits (include/ilqr_hip.h ilqr_hip_set_augmented_lagrangian): the term,
its gradient and diagonal Hessian, the multiplier update, the violations and the warm-start shift in NumPy, next to pen / pen_grad /
pen_hess of cost_envelope_cases.py; and an AL solve driver built from the oracle's stage calls with both constraint weights at zero --
linearize and cost_quadratics give the quadratics, the NumPy terms are added to lx, lu and the diagonals, set_quadratics and
backward_pass follow, the eight-alpha line search is restated here with `step` for the rollouts and total_cost + the NumPy term for the
candidates, lambda schedule, retry and exits as SURVEY Appendix A (ilqr.cpp:619-655; control flow of tests/golden/gen_golden.py gen_solve).

Multipliers are arrays [..., 19, 2] = (lower, upper) per coordinate, as the interface has them.  No GPU."""
import numpy as np

import oracle_lib as ol
from cost_envelope_cases import cost_golden

NX, NU, NQ = 51, 19, 26
ALPHAS = (1.0, 0.8, 0.6, 0.4, 0.2, 0.1, 0.05, 0.01)


def ranges():
    c = cost_golden()
    return np.array(c["jrange"], dtype=np.float64), np.array(c["ctrlrange"], dtype=np.float64)


def bounds(rng_, m):
    """lo = r0 + m (r1 - r0), hi = r1 - m (r1 - r0), each operation rounded once"""
    d = rng_[:, 1] - rng_[:, 0]
    mg = m * d
    return rng_[:, 0] + mg, rng_[:, 1] - mg


def constraints(val, rng_, m):
    """c [..., 19, 2] = (lo - val, val - hi): every constraint reads c <= 0"""
    lo, hi = bounds(rng_, m)
    return np.stack([lo - val, val - hi], axis=-1)


def _s(val, rng_, mu, rho, m):
    rho = np.asarray(rho, dtype=np.float64)[..., None, None] if np.ndim(rho) else rho
    return mu + rho * constraints(val, rng_, m), rho


def phi(val, rng_, mu, rho, m):
    """the term (max(0, mu + rho c)^2 - mu^2) / (2 rho), per constraint [..., 19, 2]"""
    s, rho = _s(val, rng_, mu, rho, m)
    return (np.maximum(s, 0.0) ** 2 - mu ** 2) / (2.0 * rho)


def grad(val, rng_, mu, rho, m):
    """d/d val of the sum of the two terms of each coordinate [..., 19]"""
    s, _ = _s(val, rng_, mu, rho, m)
    sp = np.maximum(s, 0.0)
    return sp[..., 1] - sp[..., 0]


def hess(val, rng_, mu, rho, m):
    """its second derivative [..., 19]: rho per constraint with mu + rho c > 0"""
    s, rho = _s(val, rng_, mu, rho, m)
    return (rho * (s > 0.0)).sum(axis=-1)


def traj_terms(X, U, mu_j, mu_c, rho, m):
    """One rollout: X [N+1,51], U [N,19], mu_j [N+1,19,2], mu_c [N,19,2], rho = (rho_joint, rho_ctrl).  Returns (cost added per knot
    [N+1], gx [N+1,19] to add to lx[:, 7:26], hx [N+1,19] to its diagonal, gu [N,19], hu [N,19])."""
    jr, cr = ranges()
    q = X[:, 7:NQ]
    ck = phi(q, jr, mu_j, rho[0], m).sum(axis=(1, 2))
    ck[:-1] += phi(U, cr, mu_c, rho[1], m).sum(axis=(1, 2))
    return ck, grad(q, jr, mu_j, rho[0], m), hess(q, jr, mu_j, rho[0], m), grad(U, cr, mu_c, rho[1], m), hess(U, cr, mu_c, rho[1], m)


def update(X, U, mu_j, mu_c, rho, done, m, growth, rho_max, tol):
    """The update after an inner solve, one rollout.  rho, rho_max, tol: pairs (joint, ctrl).  Returns (mu_j+, mu_c+, rho+, done+,
    (viol_joint, viol_ctrl)); a rollout that was done keeps its multipliers and penalties.  Knot 0 of the hinges is left out."""
    jr, cr = ranges()
    cj, cc = constraints(X[:, 7:NQ], jr, m), constraints(U, cr, m)
    vj = max(0.0, float(cj[1:].max())); vc = max(0.0, float(cc.max()))
    if done:
        return mu_j, mu_c, tuple(rho), True, (vj, vc)
    nj = np.maximum(0.0, mu_j + rho[0] * cj); nj[0] = mu_j[0]
    nc = np.maximum(0.0, mu_c + rho[1] * cc)
    ok = vj <= tol[0] and vc <= tol[1]
    rho2 = tuple(rho) if ok else (min(rho[0] * growth, rho_max[0]), min(rho[1] * growth, rho_max[1]))
    return nj, nc, rho2, ok, (vj, vc)


def shift(mu_j, mu_c, s):
    """Warm start shifted by s knots: hinges new[t] = old[t + s] for 1 <= t <= N - s, actuators for 0 <= t <= N - 1 - s, zero elsewhere."""
    nj, nc = np.zeros_like(mu_j), np.zeros_like(mu_c)
    N = mu_c.shape[-3]
    if s <= N - 1:
        nj[..., 1:N - s + 1, :, :] = mu_j[..., 1 + s:N + 1, :, :]
        nc[..., 0:N - s, :, :] = mu_c[..., s:N, :, :]
    return nj, nc


# ---------------------------------------------------------------------------------------------------------------------------------------
class Driver:
    """AL solve of ONE rollout (reference set b of prob) on the oracle's stages.  plain=True: the plain penalties at prob's weights, one
    round, no AL term (the reference's own solve loop restated the same way: the comparison case of the end-to-end test)."""

    def __init__(self, prob, b, al=None, max_iter=3, tol=1e-4, lam=1e-6, early_exit=True):
        self.N, self.m = prob["N"], (al or {}).get("margin", 0.0)
        self.al, self.max_iter, self.tol, self.lam, self.early_exit = al, max_iter, tol, lam, early_exit
        p = dict(prob)
        if al is not None:
            p["w_joint"] = 0.0; p["w_ctrl"] = 0.0
        self.o = ol.Oracle(self.N, prob["dt"]); self.o.set_problem(p, b)
        N = self.N
        self.mu_j, self.mu_c = np.zeros((N + 1, NU, 2)), np.zeros((N, NU, 2))
        self.rho = (al["rho_joint0"], al["rho_ctrl0"]) if al else (1.0, 1.0)

    def _al(self, X, U):
        if self.al is None:
            return np.zeros(self.N + 1), 0, 0, 0, 0
        return traj_terms(X, U, self.mu_j, self.mu_c, self.rho, self.m)

    def cost(self, X, U):
        self.o.set_trajectory(X, U)
        return self.o.total_cost() + float(self._al(X, U)[0].sum())

    def roll(self, x0, U):
        X = np.zeros((self.N + 1, NX)); X[0] = x0
        for t in range(self.N):
            X[t + 1] = self.o.step(X[t], U[t])
        return X

    def _pass(self, x0, X, U, quad, lam, J0):
        o = self.o
        o.set_trajectory(X, U); o.set_quadratics(*quad); o.set_options(lam=lam, max_iter=self.max_iter, tol=self.tol)
        o.backward_pass()
        K, k = o.get("K"), o.get("kff")
        for a in ALPHAS:
            Xn, Un = np.zeros_like(X), np.zeros_like(U); Xn[0] = x0
            for t in range(self.N):
                Un[t] = U[t] + a * k[t] + K[t] @ (Xn[t] - X[t]); Xn[t + 1] = o.step(Xn[t], Un[t])
            Jn = self.cost(Xn, Un)
            if Jn < J0 - 1e-6:
                return True, Xn, Un, Jn, a
        return False, X, U, J0, 0.0

    def inner(self, x0, X, U):
        """iLQR::solve (ilqr.cpp:521-660) on the augmented cost.  Returns (X, U, J, trace_cost, trace_alpha, trace_lambda, iterations)."""
        o, n = self.o, self.max_iter
        tc, ta, tl = np.full(n + 1, np.nan), np.full(n, np.nan), np.full(n, np.nan)
        J = self.cost(X, U); tc[0] = J
        it = 0
        for i in range(n):
            it = i + 1
            Jprev = J
            X = self.roll(x0, U)
            o.set_trajectory(X, U); o.linearize(); o.cost_quadratics()
            lx, lu, lxx, luu = (o.get(k) for k in ("lx", "lu", "lxx", "luu"))
            if self.al is not None:
                _, gx, hx, gu, hu = self._al(X, U)
                lx[:, 7:NQ] += gx; lu += gu; luu += hu
                idx = np.arange(7, NQ)
                lxx[:, idx, idx] += hx
            quad = (lx, lu, lxx, luu)
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
        """Cold start and up to `rounds` rounds.  Returns a dict: X, U, cost, the per-round inner traces, mu_j, mu_c, rho, viol, done and
        al_trace [rounds, 5] (NaN rows: rounds that did not run)."""
        al = self.al
        rounds = al["rounds"] if al else 1
        U = np.array(u_init, dtype=np.float64); X = self.roll(x0, U)
        out = dict(rounds=[], al_trace=np.full((rounds, 5), np.nan))
        done, viol = False, (0.0, 0.0)
        for r in range(rounds):
            if done and self.early_exit:
                break
            X, U, J, tc, ta, tl, it = self.inner(x0, X, U)
            out["rounds"].append(dict(trace_cost=tc, trace_alpha=ta, trace_lambda=tl, iterations=it, cost=J))
            if al:
                used = self.rho
                rho_max = (al["rho_joint0"] * al["rho_max_factor"], al["rho_ctrl0"] * al["rho_max_factor"])
                self.mu_j, self.mu_c, self.rho, done, viol = update(X, U, self.mu_j, self.mu_c, self.rho, done, self.m, al["growth"], rho_max, (al["tol_joint"], al["tol_ctrl"]))
                out["al_trace"][r] = (viol[0], viol[1], used[0], used[1], it)
        out.update(X=X, U=U, cost=J, mu_j=self.mu_j, mu_c=self.mu_c, rho=self.rho, viol=viol, done=done, lam=self.lam)
        return out


def hard_violation(X, U):
    """(joint, ctrl) violation of the hard ranges (margin 0), the hinges from knot 1 on"""
    jr, cr = ranges()
    return max(0.0, float(constraints(X[1:, 7:NQ], jr, 0.0).max())), max(0.0, float(constraints(U, cr, 0.0).max()))
