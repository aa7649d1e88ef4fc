"""CPU restatement of the augmented-Lagrangian limits under WINDOWS of bounds (include/ilqr_hip.h ilqr_hip_set_al_knot_bounds,
ilqr_hip_set_al_state_knot_bounds): traj_terms, violation and update of al_bounds_ref.py / al_state_ref.py with knot t's bounds taken from
row t of a window, win [N+1, 76] for the joint / torque family and swin [N+1, 56] for the state family; the actuators of knot t < N read
row t, the torque fields of row N are never read.  With constant rows every function returns exactly what its whole-horizon counterpart
returns (test_al_knot_cpu.py).  The track cut (ilqr_hip_al_bounds_window_from_track) is restated as NumPy indexing, and the reference
drivers take windows.  No GPU."""
import numpy as np

import al_bounds_ref as br
import al_ref as ar
import al_state_ref as sr

NX, NU, NQ = ar.NX, ar.NU, ar.NQ
COORDS = sr.COORDS
SLOTS = sr.SLOTS


def as_window(rec, N):
    """a whole-horizon record [W] repeated over the knots: [N+1, W]"""
    return np.tile(np.asarray(rec, dtype=np.float64), (N + 1, 1))


def split(win):
    """((joint_lo, joint_hi) [N+1,19], (ctrl_lo, ctrl_hi) [N,19]) of one window [N+1,76]"""
    win = np.asarray(win, dtype=np.float64)
    assert win.ndim == 2 and win.shape[1] == br.AL_BOUNDS
    return (win[:, 0:19], win[:, 19:38]), (win[:-1, 38:57], win[:-1, 57:76])


def state_split(swin):
    swin = np.asarray(swin, dtype=np.float64)
    assert swin.ndim == 2 and swin.shape[1] == sr.AL_STATE_BOUNDS
    return swin[:, :COORDS], swin[:, COORDS:]


# ---- joint / torque family: al_bounds_ref's elementwise formulas broadcast over [N+1,19] bounds as they do over [19]
def traj_terms(X, U, mu_j, mu_c, rho, win):
    """al_bounds_ref.traj_terms under the window win [N+1,76]"""
    (jl, jh), (cl, ch) = split(win)
    q = X[:, 7:NQ]
    ck = br.phi(q, jl, jh, mu_j, rho[0]).sum(axis=(1, 2))
    ck[:-1] += br.phi(U, cl, ch, mu_c, rho[1]).sum(axis=(1, 2))
    return ck, br.grad(q, jl, jh, mu_j, rho[0]), br.hess(q, jl, jh, mu_j, rho[0]), br.grad(U, cl, ch, mu_c, rho[1]), br.hess(U, cl, ch, mu_c, rho[1])


def violation(X, U, win):
    (jl, jh), (cl, ch) = split(win)
    return max(0.0, float(br.constraints(X[1:, 7:NQ], jl[1:], jh[1:]).max())), max(0.0, float(br.constraints(U, cl, ch).max()))


def update(X, U, mu_j, mu_c, rho, done, win, growth, rho_max, tol):
    """al_bounds_ref.update under the window win [N+1,76]"""
    (jl, jh), (cl, ch) = split(win)
    cj, cc = br.constraints(X[:, 7:NQ], jl, jh), br.constraints(U, cl, ch)
    vj = max(0.0, float(cj[1:].max())); vc = max(0.0, float(cc.max()))
    if done:
        return mu_j, mu_c, tuple(rho), True, (vj, vc)
    nj = np.maximum(0.0, mu_j + rho[0] * cj); nj[0] = mu_j[0]
    nc = np.maximum(0.0, mu_c + rho[1] * cc)
    ok = vj <= tol[0] and vc <= tol[1]
    rho2 = tuple(rho) if ok else (min(rho[0] * growth, rho_max[0]), min(rho[1] * growth, rho_max[1]))
    return nj, nc, rho2, ok, (vj, vc)


# ---- state family
def state_constraints(X, swin):
    """c [N+1, 28, 2] = (lo_t - x_slot, x_slot - hi_t) of the states X [N+1, 51]"""
    lo, hi = state_split(swin)
    v = X[..., SLOTS]
    return np.stack([lo - v, v - hi], axis=-1)


def state_traj_terms(X, mu_s, rho_s, swin):
    """al_state_ref.traj_terms under the window swin [N+1,56]"""
    s = mu_s + rho_s * state_constraints(X, swin)
    sp = np.maximum(s, 0.0)
    return ((sp ** 2 - mu_s ** 2) / (2.0 * rho_s)).sum(axis=(1, 2)), sp[..., 1] - sp[..., 0], (rho_s * (s > 0.0)).sum(axis=-1)


def state_violation(X, swin):
    return max(0.0, float(state_constraints(X, swin)[1:].max()))


def state_update(X, U, mu_j, mu_c, mu_s, rho, done, win, swin, growth, rho_max, tol):
    """al_state_ref.update under the windows win [N+1,76] and swin [N+1,56]"""
    (jl, jh), (cl, ch) = split(win)
    cj, cc, cs = br.constraints(X[:, 7:NQ], jl, jh), br.constraints(U, cl, ch), state_constraints(X, swin)
    viol = (max(0.0, float(cj[1:].max())), max(0.0, float(cc.max())), max(0.0, float(cs[1:].max())))
    if done:
        return mu_j, mu_c, mu_s, tuple(rho), True, viol
    nj = np.maximum(0.0, mu_j + rho[0] * cj); nj[0] = mu_j[0]
    nc = np.maximum(0.0, mu_c + rho[1] * cc)
    ns = np.maximum(0.0, mu_s + rho[2] * cs); ns[0] = mu_s[0]
    ok = all(v <= t for v, t in zip(viol, tol))
    rho2 = tuple(rho) if ok else tuple(min(r * growth, m) for r, m in zip(rho, rho_max))
    return nj, nc, ns, rho2, ok, viol


# ---- the track cut
def cut(track, starts, step, N, B):
    """Windows [B, N+1, W] cut from track [rows, W]: rollout b, knot t reads row min(start[b] + step + t, rows - 1); starts one entry
    (shared) or B of them"""
    track = np.asarray(track)
    starts = np.atleast_1d(np.asarray(starts, dtype=np.int64))
    starts = np.broadcast_to(starts, (B,)) if starts.shape[0] == 1 else starts
    assert starts.shape == (B,) and (starts >= 0).all() and step >= 0
    rows = np.minimum(starts[:, None] + step + np.arange(N + 1)[None, :], track.shape[0] - 1)
    return track[rows]


# ---- reference drivers under windows: the record-reading hooks of the parents replaced
class Driver(br.Driver):
    """al_bounds_ref.Driver (one rollout) under the window win [N+1,76]"""

    def __init__(self, prob, b, al, win, **kw):
        super().__init__(prob, b, al, np.asarray(win)[0], **kw)
        self.win = np.array(win, dtype=np.float64)

    def _al(self, X, U):
        return traj_terms(X, U, self.mu_j, self.mu_c, self.rho, self.win)

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
            self.mu_j, self.mu_c, self.rho, done, viol = update(X, U, self.mu_j, self.mu_c, self.rho, done, self.win, al["growth"], rho_max, (al["tol_joint"], al["tol_ctrl"]))
            out["al_trace"][r] = (viol[0], viol[1], used[0], used[1], it)
        out.update(X=X, U=U, cost=J, mu_j=self.mu_j, mu_c=self.mu_c, rho=self.rho, viol=viol, done=done, lam=self.lam)
        return out
