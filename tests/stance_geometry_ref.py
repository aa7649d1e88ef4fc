"""CPU reference of the stance source GEOMETRY (include/ilqr_hip.h ilqr_hip_set_stance_source), built only from existing pieces:
the host contact rule `solver.foot_clearance` (get_contacts.py:96-147) and the oracle's constrained step / linearisation / cost /
backward pass (oracle/ilqr_oracle.cpp).

  * step(): the plant step -- flags = foot_clearance(qpos) < 0, then Oracle.step_stance with the oracle's contact mode.
  * solve(): the loop of ilqr_oracle.cpp:199-240 (rollout, linearisation, cost quadratics, backward pass, line search over the eight
    alphas, the lambda retry) with every step deciding its own stance.  Two oracle handles: the dynamics handle gets its contact schedule
    set to the nominal trajectory's decisions, so that orc_linearize differentiates the step with those decisions held fixed (analytic
    Jacobians); forward differences are taken here, each perturbed step deciding again.  The cost handle keeps the true schedule for the
    cost quadratics, the backward pass (after orc_set_linearization) and the total cost: the cost reads the schedule (ilqr.cpp:403-404).
"""
import ctypes as C

import numpy as np

import oracle_lib as ol

NX, NU, NQ = 51, 19, 26
ALPHAS = (1.0, 0.8, 0.6, 0.4, 0.2, 0.1, 0.05, 0.01)


def decide(sv, x):
    """(left, right) stance flags of the host rule at state x: foot f touches iff its clearance is negative."""
    return (sv.foot_clearance(np.asarray(x)[:NQ]) < 0).astype(np.int32)


class GeometryReference:
    def __init__(self, sv, prob, b=0, mode=2, limits=False, mu=None, jac_mode=0, fd_eps=1e-5):
        self.sv, self.N, self.mode, self.jac_mode, self.fd_eps = sv, prob["N"], mode, jac_mode, fd_eps
        self.dyn = ol.Oracle(prob["N"], prob["dt"])
        self.cost = ol.Oracle(prob["N"], prob["dt"])
        for o in (self.dyn, self.cost):
            o.set_problem(prob, b)
            o.set_contact_mode(mode)
            if limits:
                o.set_joint_limits(True)
            if mu is not None:
                o.set_friction(mu)
        self.lam = 1e-6

    def step(self, x, u):
        """(x_next, flags): the plant step with contacts from geometry."""
        st = decide(self.sv, x)
        return self.dyn.step_stance(np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), st), st

    def rollout(self, x0, ubar):
        xs = np.zeros((self.N + 1, NX)); xs[0] = x0
        for t in range(self.N):
            xs[t + 1] = self.step(xs[t], ubar[t])[0]
        return xs

    def total_cost(self, xs, us):
        self.cost.set_trajectory(xs, us)
        return self.cost.total_cost()

    def decisions(self, xbar):
        return np.array([decide(self.sv, xbar[t]) for t in range(self.N)])

    def linearize(self, xbar, ubar):
        if self.jac_mode == 0:
            sched = np.zeros((self.N + 1, 2), dtype=np.int32)
            sched[: self.N] = self.decisions(xbar)
            sched[self.N] = sched[self.N - 1]
            self._sched = np.ascontiguousarray(sched)
            self.dyn.L.orc_set_contact_schedule(self.dyn.h, self._sched.ctypes.data_as(C.POINTER(C.c_int)))
            self.dyn.set_options(jac_mode=0)
            self.dyn.set_trajectory(xbar, ubar)
            self.dyn.linearize()
            return self.dyn.get("A"), self.dyn.get("B")
        A, B = np.zeros((self.N, NX, NX)), np.zeros((self.N, NX, NU))
        eps = self.fd_eps
        for t in range(self.N):
            base = self.step(xbar[t], ubar[t])[0]
            for c in range(NX + NU):
                x, u = xbar[t].copy(), ubar[t].copy()
                if c < NX:
                    x[c] += eps
                else:
                    u[c - NX] += eps
                d = (self.step(x, u)[0] - base) / eps
                if c < NX:
                    A[t][:, c] = d
                else:
                    B[t][:, c - NX] = d
        return A, B

    def backward(self):
        self.cost.set_options(lam=self.lam, max_iter=1, early_exit=0)
        self.cost.backward_pass()
        return self.cost.get("K"), self.cost.get("kff")

    def line_search(self, x0, xbar, ubar, K, kff):
        baseline = self.total_cost(xbar, ubar)
        for a in ALPHAS:
            xs = np.zeros((self.N + 1, NX)); us = np.zeros((self.N, NU)); xs[0] = x0
            for t in range(self.N):
                us[t] = ubar[t] + a * kff[t] + K[t] @ (xs[t] - xbar[t])
                xs[t + 1] = self.step(xs[t], us[t])[0]
            c = self.total_cost(xs, us)
            if c < baseline - 1e-6:
                return True, xs, us, c, a
        return False, xbar, ubar, baseline, 0.0

    def solve(self, x0, u_init, iters):
        """Fixed iteration count (no convergence exit).  Returns dict(cost_trace, alpha, lam, xbar, ubar, K, decisions)."""
        ubar = np.array(u_init, dtype=np.float64)
        xbar = self.rollout(x0, ubar)
        J = self.total_cost(xbar, ubar)
        tc, ta, tl = [J], [], []
        K = None
        for _ in range(iters):
            xbar = self.rollout(x0, ubar)
            A, B = self.linearize(xbar, ubar)
            self.cost.set_trajectory(xbar, ubar)
            self.cost.set_linearization(A, B)
            self.cost.cost_quadratics()
            K, kff = self.backward()
            ok, xs, us, Jn, a = self.line_search(x0, xbar, ubar, K, kff)
            lam_used = self.lam
            if not ok:
                self.lam = min(self.lam * 10.0, 1e-3)
                lam_used = self.lam
                self.cost.set_trajectory(xbar, ubar)
                K, kff = self.backward()
                ok, xs, us, Jn, a = self.line_search(x0, xbar, ubar, K, kff)
                if not ok:
                    tc.append(J); ta.append(0.0); tl.append(lam_used)
                    continue
            xbar, ubar, J = xs, us, Jn
            self.lam = max(self.lam / 2.0, 1e-6)
            tc.append(J); ta.append(a); tl.append(lam_used)
        return dict(cost_trace=np.array(tc), alpha=np.array(ta), lam=np.array(tl), xbar=xbar, ubar=ubar, K=K, decisions=self.decisions(xbar))
