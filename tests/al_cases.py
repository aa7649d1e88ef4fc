"""Inputs of the augmented-Lagrangian tests (test_augmented_lagrangian_cpu.py, test_gpu_augmented_lagrangian.py).  NumPy and the
oracle's host helpers only; no GPU.

  * regimes(): the 76 rollouts of cost_envelope_cases.limit_sweep x three regimes of the term = 228 rollouts at N = 4, with a multiplier
    on every constraint, distinct penalties per rollout, the excursions spread over every knot (knot 0 and the terminal one included).
  * end_to_end(): B = 3, N = 6 -- rollout 0 touches no limit, rollout 1 is torque-limited (a kicked wrist under a heavy velocity weight,
    R scaled down), rollout 2 joint-limited (an elbow whose reference posture lies past its range).
"""
import functools

import numpy as np

import al_ref as ar
import cost_envelope_cases as cc
import oracle_lib as ol

sc = cc.sc
NX, NU, NQ = 51, 19, 26
N_STAGE = 4
# the outer loop of the end-to-end case; tolerances in rad / N m, margin 0: the hard ranges
AL_E2E = dict(rounds=3, rho_joint0=1e5, rho_ctrl0=1e3, growth=10.0, rho_max_factor=1e4, margin=0.0, tol_joint=1e-3, tol_ctrl=1e-2)
MAX_ITER = 3


@functools.lru_cache(maxsize=None)
def regimes(m):
    """(X [228,5,51], U [228,4,19], mu_j [228,5,19,2], mu_c [228,4,19,2], rho [228,2], cases) for margin fraction m; read-only.
    Rollout 3 r + g is case r of limit_sweep (hinge or actuator j, side) in regime g at knot r % (N + 1) (hinges) / r % N (actuators):
      g = 0  the value 2 % of the range OUTSIDE the bound, multiplier 0;
      g = 1  2 % inside, multiplier 1.5 rho |c|: mu + rho c > 0;
      g = 2  2 % inside, multiplier 0.5 rho |c|: mu + rho c < 0, the term is the constant -mu^2 / (2 rho).
    Every other constraint sits at least 1 % of its range inside its bound (sweep_base_state, gravity-compensation torques) and carries
    a multiplier of its own small enough that mu + rho c < 0: its only trace is its constant in the cost.  cases[i] = (kind, j, side, knot, g)."""
    N = N_STAGE
    X0, U0, sweep = cc.limit_sweep(N)
    jr, cr = ar.ranges()
    rng = np.random.default_rng(41)
    B = 3 * len(sweep)
    X = np.tile(X0[0, 0], (B, N + 1, 1)); U = np.tile(U0[0, 0], (B, N, 1))
    rho = np.stack([300.0 * (1.0 + 0.011 * np.arange(B)), 40.0 * (1.0 + 0.013 * np.arange(B))], axis=1)
    wj, wc_ = jr[:, 1] - jr[:, 0], cr[:, 1] - cr[:, 0]
    mu_j = rng.uniform(0.1, 0.9, (B, N + 1, NU, 2)) * rho[:, 0, None, None, None] * 0.01 * wj[None, None, :, None]
    mu_c = rng.uniform(0.1, 0.9, (B, N, NU, 2)) * rho[:, 1, None, None, None] * 0.01 * wc_[None, None, :, None]
    mu_j[:, 0] = 0.0                                                   # (x_0 is given: the store keeps these zero)
    cases = []
    for r, (kind, j, side, _) in enumerate(sweep):
        table, width = (jr, wj) if kind == "joint" else (cr, wc_)
        lo, hi = ar.bounds(table, m)
        t = r % (N + 1) if kind == "joint" else r % N
        for g in range(3):
            i = 3 * r + g
            d = 0.02 * width[j] * (1.0 if g == 0 else -1.0)            # signed distance past the bound
            v = hi[j] + d if side else lo[j] - d
            mu = 0.0 if g == 0 else (1.5 if g == 1 else 0.5) * rho[i, 0 if kind == "joint" else 1] * 0.02 * width[j]
            if kind == "joint":
                X[i, t, 7 + j] = v
                if t > 0:
                    mu_j[i, t, j, side] = mu
            else:
                U[i, t, j] = v; mu_c[i, t, j, side] = mu
            cases.append((kind, j, side, t, g))
    for a in (X, U, mu_j, mu_c, rho):
        a.setflags(write=False)
    return X, U, mu_j, mu_c, rho, cases


def stage_problem():
    """the shipped problem at N = 4 with BOTH plain penalties on: while AL is installed they must not be read"""
    return sc.make_problem(ol.reference_kinematics, N=N_STAGE)


@functools.lru_cache(maxsize=None)
def end_to_end():
    """(prob, x0 [3,51], u_init [3,6,19]); read-only.  Shipped weights except R / 100 and two heavy tracking weights that pull rollouts 1
    and 2 past a range: the velocity of wrist hinge 13 (range +-18 N m; rollout 1 starts with 5 rad/s on it) and the position of elbow
    hinge 14 (rollout 2 starts 0.05 rad inside its upper end, its reference posture lies 1 rad past it)."""
    N, B, jt, jj = 6, 3, 13, 14
    prob = sc.make_problem(ol.reference_kinematics, N=N)
    prob["R"] = prob["R"] * 0.01
    for k in ("Q", "Qf"):
        prob[k] = prob[k].copy(); prob[k][7 + jj] = 2000.0; prob[k][NQ + 6 + jt] = 20000.0
    jr, _ = ar.ranges()
    xs = sc.standing_state()
    x_ref = np.tile(xs, (B, N + 1, 1)); x_ref[2, :, 7 + jj] = jr[jj, 1] + 1.0
    prob["x_ref"] = x_ref
    for k in ("u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        prob[k] = np.repeat(prob[k], B, axis=0)
    x0 = np.tile(xs, (B, 1))
    x0[1, NQ + 6 + jt] = 5.0
    x0[2, 7 + jj] = jr[jj, 1] - 0.05
    o = ol.Oracle(N, prob["dt"]); o.set_problem(prob)
    ui = np.tile(o.grav_comp(xs), (B, N, 1))
    for a in (x0, ui, prob["x_ref"], prob["Q"], prob["Qf"], prob["R"]):
        a.setflags(write=False)
    return prob, x0, ui


def problem_of(prob, b):
    """rollout b's problem of end_to_end(), for a B = 1 handle"""
    p = dict(prob)
    for k in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        p[k] = np.ascontiguousarray(prob[k][b:b + 1])
    return p


@functools.lru_cache(maxsize=None)
def reference_solves(early_exit):
    """the reference driver on end_to_end(): ([AL solve of rollout b], [plain-penalty solve of rollout b]); computed once, read-only"""
    prob, x0, ui = end_to_end()
    al = [ar.Driver(prob, b, AL_E2E, max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(3)]
    plain = [ar.Driver(prob, b, None, max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(3)]
    return al, plain
