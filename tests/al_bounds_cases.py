"""Inputs of the tests of the per-rollout bounds table of the augmented-Lagrangian limits (test_al_bounds_cpu.py, test_gpu_al_bounds.py).
NumPy and the oracle's host helpers only; no GPU.

  * regimes_table(): the construction of al_cases.regimes (76 cases x 3 regimes = 228 rollouts, N = 4) under a [228][76] table whose
    bounds differ for every rollout and every coordinate; a dozen rollouts carry an infinite side besides.
  * end_to_end(): al_cases.end_to_end() rebuilt as B = 4 by repeating its reference set 1, with one record per rollout.
"""
import functools

import numpy as np

import al_bounds_ref as br
import al_cases as ac
import al_ref as ar
import cost_envelope_cases as cc

NX, NU, NQ = 51, 19, 26
N_STAGE = ac.N_STAGE
INF_ROLLOUTS = tuple(range(5, 228, 19))      # 12 rollouts, every regime among them (5 + 19 k mod 3 takes 0, 1, 2)
TOL_JOINT, TOL_CTRL = ac.AL_E2E["tol_joint"], ac.AL_E2E["tol_ctrl"]


@functools.lru_cache(maxsize=None)
def regimes_table():
    """(X [228,5,51], U [228,4,19], mu_j [228,5,19,2], mu_c [228,4,19,2], rho [228,2], rec [228,76], cases, inf); read-only.
    rec[i]: the model's ranges moved inward by a seeded 0 .. 20 % of the range on each side, drawn per rollout and coordinate.  Rollout
    3 r + g is case r of limit_sweep in regime g of al_cases.regimes, placed relative to ITS OWN bound: the value 2 % of its own width
    outside the bound with multiplier 0 (g = 0), 2 % inside with multiplier 1.5 rho |c| (g = 1) or 0.5 rho |c| (g = 2).  Every other
    coordinate is clipped at least 1 % of its own width inside its own bounds and carries a multiplier < rho times that distance: its only
    trace is its constant in the cost.  inf[i] = (kind, j, side) for the rollouts INF_ROLLOUTS: that side of a coordinate other than the
    excited one is switched off (-inf / +inf) and carries a multiplier of the size of the others at every knot."""
    N = N_STAGE
    X0, U0, sweep = cc.limit_sweep(N)
    jr, cr = ar.ranges()
    rng = np.random.default_rng(43)
    B = 3 * len(sweep)
    assert B == 228
    inward = rng.uniform(0.0, 0.2, (B, 2, 19, 2))                        # [rollout][family][coordinate][side]
    rec = np.zeros((B, 76))
    for f, table in enumerate((jr, cr)):
        w = table[:, 1] - table[:, 0]
        rec[:, 38 * f:38 * f + 19] = table[:, 0] + inward[:, f, :, 0] * w
        rec[:, 38 * f + 19:38 * f + 38] = table[:, 1] - inward[:, f, :, 1] * w
    fin = rec.copy()                                                     # (the finite table: widths and clipping)
    inf = {}
    for n, i in enumerate(INF_ROLLOUTS):
        kind, j, side, _ = sweep[i // 3]
        other = (j + 1 + n) % 19
        fam = n % 2                                                      # the switched-off side alternates between the families ...
        if (fam == 0) == (kind == "joint") and other == j:
            other = (other + 1) % 19
        s_ = (n // 2) % 2                                                # ... and between the sides
        rec[i, 38 * fam + 19 * s_ + other] = np.inf if s_ else -np.inf
        inf[i] = ("joint" if fam == 0 else "ctrl", other, s_)
    jl, jh, cl, ch = fin[:, 0:19], fin[:, 19:38], fin[:, 38:57], fin[:, 57:76]
    wj, wc_ = jh - jl, ch - cl                                           # own widths [B,19]
    X = np.tile(X0[0, 0], (B, N + 1, 1)); U = np.tile(U0[0, 0], (B, N, 1))
    X[:, :, 7:NQ] = np.clip(X[:, :, 7:NQ], (jl + 0.01 * wj)[:, None], (jh - 0.01 * wj)[:, None])
    U[:] = np.clip(U, (cl + 0.01 * wc_)[:, None], (ch - 0.01 * wc_)[:, None])
    rho = np.stack([300.0 * (1.0 + 0.011 * np.arange(B)), 40.0 * (1.0 + 0.013 * np.arange(B))], axis=1)
    mu_j = rng.uniform(0.1, 0.9, (B, N + 1, NU, 2)) * rho[:, 0, None, None, None] * 0.01 * wj[:, None, :, None]
    mu_c = rng.uniform(0.1, 0.9, (B, N, NU, 2)) * rho[:, 1, None, None, None] * 0.01 * wc_[:, None, :, None]
    mu_j[:, 0] = 0.0                                                     # (x_0 is given: the store keeps these zero)
    cases = []
    for r, (kind, j, side, _) in enumerate(sweep):
        t = r % (N + 1) if kind == "joint" else r % N
        for g in range(3):
            i = 3 * r + g
            lo, hi, width = (jl[i], jh[i], wj[i]) if kind == "joint" else (cl[i], ch[i], wc_[i])
            d = 0.02 * width[j] * (1.0 if g == 0 else -1.0)              # signed distance past the rollout's own bound
            v = hi[j] + d if side else lo[j] - d
            mu = 0.0 if g == 0 else (1.5 if g == 1 else 0.5) * rho[i, 0 if kind == "joint" else 1] * 0.02 * width[j]
            if kind == "joint":
                X[i, t, 7 + j] = v
                if t > 0:
                    mu_j[i, t, j, side] = mu
            else:
                U[i, t, j] = v; mu_c[i, t, j, side] = mu
            cases.append((kind, j, side, t, g))
    for a in (X, U, mu_j, mu_c, rho, rec):
        a.setflags(write=False)
    return X, U, mu_j, mu_c, rho, rec, cases, inf


# ---------------------------------------------------------------------------------------------------------------------------------------
E2E_SETS = (0, 1, 1, 2)      # reference set of al_cases.end_to_end() behind each of the four rollouts
WRIST, ELBOW = 13, 14
WRIST_BOUND = 16.2           # 0.9 x the wrist actuator's range of 18 N m
ELBOW_DROP = 0.03            # rad


@functools.lru_cache(maxsize=None)
def end_to_end():
    """(prob, x0 [4,51], u_init [4,6,19], rec [4,76]); read-only.  Rollout 0 = set 0 and rollout 1 = set 1 of al_cases.end_to_end() under
    the default bounds (margin 0); rollout 2 = set 1 with the wrist actuator 13 bounded at +-16.2 N m (0.9 x its range); rollout 3 = set 2
    with the upper bound of elbow hinge 14 lowered by 0.03 rad."""
    prob3, x03, ui3 = ac.end_to_end()
    idx = np.array(E2E_SETS)
    prob = dict(prob3)
    for k in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        prob[k] = np.ascontiguousarray(prob3[k][idx])
    x0, ui = np.ascontiguousarray(x03[idx]), np.ascontiguousarray(ui3[idx])
    rec = np.tile(br.default_record(0.0), (4, 1))
    rec[2, 38 + WRIST] = -WRIST_BOUND; rec[2, 57 + WRIST] = WRIST_BOUND
    rec[3, 19 + ELBOW] -= ELBOW_DROP
    for a in (x0, ui, rec, prob["x_ref"]):
        a.setflags(write=False)
    return prob, x0, ui, rec


def problem_of(prob, b):
    return ac.problem_of(prob, b)


@functools.lru_cache(maxsize=None)
def reference_solves(early_exit):
    """the reference driver (al_bounds_ref.Driver) on end_to_end(): [solve of rollout b under its record]; computed once, read-only"""
    prob, x0, ui, rec = end_to_end()
    return [br.Driver(prob, b, ac.AL_E2E, rec[b], max_iter=ac.MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(4)]


def effect_assertions(sols, twin):
    """The four conditions of the end-to-end case on results sols[b] = dict(U [N,19], X [N+1,51], viol (joint, ctrl), done) of the four
    rollouts and twin = the X of rollout 3's problem solved under the default bounds."""
    peak_u = lambda s: float(np.abs(np.asarray(s["U"])[:, WRIST]).max())
    peak_q = lambda X: float(np.asarray(X)[1:, 7 + ELBOW].max())
    bound = ar.ranges()[0][ELBOW, 1] - ELBOW_DROP
    assert abs(bound - 2.58) < 1e-12
    assert sols[2]["viol"][1] < 0.1 and not sols[2]["done"], (sols[2]["viol"], sols[2]["done"])
    assert peak_u(sols[1]) > WRIST_BOUND + 1.0, peak_u(sols[1])
    assert sols[3]["done"] and peak_q(sols[3]["X"]) <= bound + TOL_JOINT, (sols[3]["done"], peak_q(sols[3]["X"]))
    assert peak_q(twin) > bound + 10 * TOL_JOINT, peak_q(twin)
    return dict(peak_u13_default=peak_u(sols[1]), peak_u13_bounded=peak_u(sols[2]), viol_ctrl_bounded=float(sols[2]["viol"][1]),
                peak_q14_bounded=peak_q(sols[3]["X"]), viol_joint_bounded=float(sols[3]["viol"][0]), peak_q14_default=peak_q(twin))
