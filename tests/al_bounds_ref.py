"""CPU restatement of the augmented-Lagrangian limits under a table of bounds per rollout (include/ilqr_hip.h ilqr_hip_set_al_bounds):
al_ref.py's constraints, term, gradient, curvature, traj_terms and update restated from an explicit (lo, hi) per coordinate, and its
reference driver taking the rollout's record.  The constraints are formed directly as c = (lo - val, val - hi): an infinite side gives
c = -inf, max(0, mu + rho c) = 0, the constant term -mu^2 / (2 rho), no gradient, no curvature, no violation and a multiplier the update
drives to zero.  (al_ref.bounds is not used for a table: its m * (hi - lo) is NaN for an infinite side.)

A record is [76] = joint_lo[19], joint_hi[19], ctrl_lo[19], ctrl_hi[19], as the interface has it.  No GPU."""
import numpy as np

import al_ref as ar
from al_ref import ALPHAS, shift  # noqa: F401  (need no ranges)

NX, NU, NQ = ar.NX, ar.NU, ar.NQ
AL_BOUNDS = 76


def default_record(m):
    """the record of the model's bounds at margin m: al_ref.bounds of the two range tables"""
    jr, cr = ar.ranges()
    return np.concatenate(ar.bounds(jr, m) + ar.bounds(cr, m))


def split(rec):
    """((joint_lo, joint_hi), (ctrl_lo, ctrl_hi)) of one record"""
    rec = np.asarray(rec, dtype=np.float64)
    assert rec.shape == (AL_BOUNDS,)
    return (rec[0:19], rec[19:38]), (rec[38:57], rec[57:76])


def constraints(val, lo, hi):
    """c [..., 19, 2] = (lo - val, val - hi): every constraint reads c <= 0"""
    return np.stack([lo - val, val - hi], axis=-1)


def _s(val, lo, hi, mu, rho):
    rho = np.asarray(rho, dtype=np.float64)[..., None, None] if np.ndim(rho) else rho
    return mu + rho * constraints(val, lo, hi), rho


def phi(val, lo, hi, mu, rho):
    """the term (max(0, mu + rho c)^2 - mu^2) / (2 rho), per constraint [..., 19, 2]"""
    s, rho = _s(val, lo, hi, mu, rho)
    return (np.maximum(s, 0.0) ** 2 - mu ** 2) / (2.0 * rho)


def grad(val, lo, hi, mu, rho):
    """d/d val of the sum of the two terms of each coordinate [..., 19]"""
    s, _ = _s(val, lo, hi, mu, rho)
    sp = np.maximum(s, 0.0)
    return sp[..., 1] - sp[..., 0]


def hess(val, lo, hi, mu, rho):
    """its second derivative [..., 19]: rho per constraint with mu + rho c > 0"""
    s, rho = _s(val, lo, hi, mu, rho)
    return (rho * (s > 0.0)).sum(axis=-1)


def traj_terms(X, U, mu_j, mu_c, rho, rec):
    """al_ref.traj_terms under the record rec [76]"""
    (jl, jh), (cl, ch) = split(rec)
    q = X[:, 7:NQ]
    ck = phi(q, jl, jh, mu_j, rho[0]).sum(axis=(1, 2))
    ck[:-1] += phi(U, cl, ch, mu_c, rho[1]).sum(axis=(1, 2))
    return ck, grad(q, jl, jh, mu_j, rho[0]), hess(q, jl, jh, mu_j, rho[0]), grad(U, cl, ch, mu_c, rho[1]), hess(U, cl, ch, mu_c, rho[1])


def violation(X, U, rec):
    """(joint, ctrl) violation of the record, the hinges from knot 1 on"""
    (jl, jh), (cl, ch) = split(rec)
    return max(0.0, float(constraints(X[1:, 7:NQ], jl, jh).max())), max(0.0, float(constraints(U, cl, ch).max()))


def update(X, U, mu_j, mu_c, rho, done, rec, growth, rho_max, tol):
    """al_ref.update under the record rec [76]"""
    (jl, jh), (cl, ch) = split(rec)
    cj, cc = constraints(X[:, 7:NQ], jl, jh), constraints(U, cl, ch)
    vj = max(0.0, float(cj[1:].max())); vc = max(0.0, float(cc.max()))
    if done:
        return mu_j, mu_c, tuple(rho), True, (vj, vc)
    nj = np.maximum(0.0, mu_j + rho[0] * cj); nj[0] = mu_j[0]
    nc = np.maximum(0.0, mu_c + rho[1] * cc)
    ok = vj <= tol[0] and vc <= tol[1]
    rho2 = tuple(rho) if ok else (min(rho[0] * growth, rho_max[0]), min(rho[1] * growth, rho_max[1]))
    return nj, nc, rho2, ok, (vj, vc)


class Driver(ar.Driver):
    """al_ref.Driver (AL solve of ONE rollout, reference set b of prob) under the rollout's record rec [76]: the inner solve, the line
    search, the lambda schedule and the rounds are the parent's; the term and the update take their bounds from the record."""

    def __init__(self, prob, b, al, rec, **kw):
        assert al is not None
        super().__init__(prob, b, al, **kw)
        self.rec = np.array(rec, dtype=np.float64)

    def _al(self, X, U):
        return traj_terms(X, U, self.mu_j, self.mu_c, self.rho, self.rec)

    def solve(self, x0, u_init):
        al = self.al
        rounds = al["rounds"]
        U = np.array(u_init, dtype=np.float64); X = self.roll(x0, U)
        out = dict(rounds=[], al_trace=np.full((rounds, 5), np.nan))
        done, viol = False, (0.0, 0.0)
        rho_max = (al["rho_joint0"] * al["rho_max_factor"], al["rho_ctrl0"] * al["rho_max_factor"])
        for r in range(rounds):
            if done and self.early_exit:
                break
            X, U, J, tc, ta, tl, it = self.inner(x0, X, U)
            out["rounds"].append(dict(trace_cost=tc, trace_alpha=ta, trace_lambda=tl, iterations=it, cost=J))
            used = self.rho
            self.mu_j, self.mu_c, self.rho, done, viol = update(X, U, self.mu_j, self.mu_c, self.rho, done, self.rec, al["growth"], rho_max, (al["tol_joint"], al["tol_ctrl"]))
            out["al_trace"][r] = (viol[0], viol[1], used[0], used[1], it)
        out.update(X=X, U=U, cost=J, mu_j=self.mu_j, mu_c=self.mu_c, rho=self.rho, viol=viol, done=done, lam=self.lam)
        return out
