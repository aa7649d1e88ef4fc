"""Inputs of the tests of the state family of the augmented-Lagrangian limits (test_al_state_cpu.py, test_gpu_al_state.py).  NumPy and
the oracle's host helpers only; no GPU.

  * regimes(): 28 box coordinates x 2 sides x 3 regimes = 168 rollouts at N = al_cases.N_STAGE, one state record per rollout whose
    bounds differ for every rollout and every coordinate, a multiplier on every constraint, distinct penalties per rollout, the excursions
    spread over every knot (knot 0 and the terminal one included); the joint / torque family rides along inactive with multipliers of its own.
  * end_to_end(): al_cases.end_to_end() (B = 3, N = 6) with a joint-speed bound on rollout 0, a pelvis-height bound on rollout 1 and no
    state bound on rollout 2, placed relative to the solution WITHOUT a state table (al_cases.reference_solves).
"""
import functools

import numpy as np

import al_bounds_ref as br
import al_cases as ac
import al_ref as ar
import al_state_ref as sr
import cost_envelope_cases as cc

sc = ac.sc
NX, NU, NQ = 51, 19, 26
N_STAGE = ac.N_STAGE
COORDS = sr.COORDS
# widths of the drawn boxes per coordinate: pelvis position [m], linear velocity [m/s], angular velocity [rad/s], joint velocities [rad/s]
WIDTH = np.concatenate([np.full(3, 0.4), np.full(3, 1.0), np.full(3, 2.0), np.full(19, 4.0)])
STAGE_MARGIN = 0.05            # margin of the run without a joint / torque table
INF_ROLLOUTS = tuple(range(4, 168, 17))      # 10 rollouts, every regime among them


@functools.lru_cache(maxsize=None)
def regimes():
    """(X [168,5,51], U [168,4,19], mu_j, mu_c, mu_s [168,5,28,2], rho [168,3] = (joint, ctrl, state), srec [168,56], rec [168,76],
    cases, inf); read-only.  Rollout 3 (2 k + side) + g is box coordinate k, side (0 lower, 1 upper), regime g of al_cases.regimes at knot
    (2 k + side) % (N + 1):
      g = 0  the value 2 % of the rollout's own box width OUTSIDE its bound, multiplier 0;
      g = 1  2 % inside, multiplier 1.5 rho |c|: mu + rho c > 0;
      g = 2  2 % inside, multiplier 0.5 rho |c|: mu + rho c < 0, the term is the constant -mu^2 / (2 rho).
    srec[i]: around a seeded centre per coordinate a box lo = centre - a w, hi = centre + b w with a, b in 0.3 .. 0.5 drawn per rollout and
    coordinate (w = WIDTH); every other value is drawn per knot at least 10 % of its own box width inside both bounds and carries a
    multiplier < rho times 1 % of that width: its only trace is its constant in the cost.  The quaternion and the hinges stay those of
    sweep_base_state under gravity-compensation torques; rec[i] is the model's joint / torque record at margin 0.09 i / 167 (every row its own),
    under which -- and under STAGE_MARGIN -- every hinge and actuator stays inactive with the multipliers mu_j, mu_c of al_cases.regimes' size.
    inf[i] = (k, side) for the rollouts INF_ROLLOUTS: that side of a coordinate other than the excited one is switched off and carries a
    multiplier of the others' size at every knot >= 1.  cases[i] = (k, side, knot, g)."""
    N = N_STAGE
    X0, U0, _ = cc.limit_sweep(N)
    jr, cr = ar.ranges()
    rng = np.random.default_rng(47)
    B = 6 * COORDS
    X = np.tile(X0[0, 0], (B, N + 1, 1)); U = np.tile(U0[0, 0], (B, N, 1))
    centre = np.concatenate([X0[0, 0, :3], rng.uniform(-0.2, 0.2, COORDS - 3)])
    ab = rng.uniform(0.3, 0.5, (B, COORDS, 2))
    srec = np.concatenate([centre - ab[:, :, 0] * WIDTH, centre + ab[:, :, 1] * WIDTH], axis=1)
    lo, hi = srec[:, :COORDS], srec[:, COORDS:]
    w = hi - lo                                                          # own widths [B,28]
    X[:, :, sr.SLOTS] = lo[:, None] + w[:, None] * rng.uniform(0.1, 0.9, (B, N + 1, COORDS))
    rho = np.stack([300.0 * (1.0 + 0.011 * np.arange(B)), 40.0 * (1.0 + 0.013 * np.arange(B)), 70.0 * (1.0 + 0.017 * np.arange(B))], axis=1)
    wj, wc_ = jr[:, 1] - jr[:, 0], cr[:, 1] - cr[:, 0]
    mu_j = rng.uniform(0.1, 0.9, (B, N + 1, NU, 2)) * rho[:, 0, None, None, None] * 0.01 * wj[None, None, :, None]
    mu_c = rng.uniform(0.1, 0.9, (B, N, NU, 2)) * rho[:, 1, None, None, None] * 0.01 * wc_[None, None, :, None]
    mu_s = rng.uniform(0.1, 0.9, (B, N + 1, COORDS, 2)) * rho[:, 2, None, None, None] * 0.01 * w[:, None, :, None]
    mu_j[:, 0] = 0.0; mu_s[:, 0] = 0.0                                   # (x_0 is given: the stores keep these zero)
    cases = []
    for k in range(COORDS):
        for side in range(2):
            r = 2 * k + side
            t = r % (N + 1)
            for g in range(3):
                i = 3 * r + g
                d = 0.02 * w[i, k] * (1.0 if g == 0 else -1.0)           # signed distance past the rollout's own bound
                X[i, t, sr.SLOTS[k]] = hi[i, k] + d if side else lo[i, k] - d
                mu_s[i, t, k, :] = 0.0 if t == 0 else mu_s[i, t, k, :]
                if t > 0:
                    mu_s[i, t, k, side] = 0.0 if g == 0 else (1.5 if g == 1 else 0.5) * rho[i, 2] * 0.02 * w[i, k]
                cases.append((k, side, t, g))
    inf = {}
    for n, i in enumerate(INF_ROLLOUTS):
        k = cases[i][0]
        other, s_ = (k + 1 + n) % COORDS, n % 2
        srec[i, COORDS * s_ + other] = np.inf if s_ else -np.inf
        inf[i] = (other, s_)
    rec = np.stack([br.default_record(0.09 * i / (B - 1)) for i in range(B)])
    for a in (X, U, mu_j, mu_c, mu_s, rho, srec, rec):
        a.setflags(write=False)
    return X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, inf


def stage_problem():
    return ac.stage_problem()


def stage_expected(want, cost0, b, table):
    """Oracle quadratics `want` (dict of one rollout, zero constraint weights) and cost `cost0` of rollout b of regimes() -> the same with the
    three families' terms added: the joint / torque family under rec[b] (table) or the model's bounds at STAGE_MARGIN."""
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, _, _ = regimes()
    jrec = rec[b] if table else br.default_record(STAGE_MARGIN)
    ck, gx, hx, gu, hu = br.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b, :2], jrec)
    sk, sg, sh = sr.traj_terms(X[b], mu_s[b], rho[b, 2], srec[b])
    w = {n: want[n].copy() for n in want}
    idx = np.arange(7, NQ)
    w["lx"][:, 7:NQ] += gx; w["lu"] += gu; w["luu"] += hu; w["lxx"][:, idx, idx] += hx
    sr.add_to_quadratics(w, sg, sh)
    return w, cost0 + ck.sum() + sk.sum()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The outer loop of the end-to-end case: al_cases.AL_E2E with one more round and the state family's penalty and tolerance (rad/s and m).  The
# horizon is 0.12 s of a robot without ground contact: joint torques move the pelvis against the rest of the body only, 5e-6 m per N m and
# step, and rollout 1 carries a cost of 1e5..1e6 whose line searches stall after the second round -- so the height bound is 0.2 mm and the
# penalty starts large enough for the first round to act on it (test_al_state_cpu.py shows the conditions the GPU test relies on).
AL_E2E = dict(ac.AL_E2E, rounds=4, rho_state0=1e9, tol_state=1.5e-5)
MAX_ITER = ac.MAX_ITER
PELVIS_LIFT = 2e-4             # m above the unconstrained minimum


def al_args(al=AL_E2E):
    """the arguments of set_augmented_lagrangian among `al`"""
    return {k: v for k, v in al.items() if k not in ("rho_state0", "tol_state")}


@functools.lru_cache(maxsize=None)
def end_to_end():
    """(prob, x0 [3,51], u_init [3,6,19], srec [3,56], info); read-only.  prob, x0, u_init: al_cases.end_to_end().  From the solution
    WITHOUT a state table (al_cases.reference_solves, convergence exit):
      rollout 0  joint_vel of the joint whose peak |qdot| over the knots 1..N is largest, bounded at +- half that peak;
      rollout 1  pelvis_z bounded below PELVIS_LIFT above its minimum over the knots 1..N;
      rollout 2  every bound infinite.
    info = dict(joint, peak, z_min, viol0 = the violation of these bounds by that solution per rollout)."""
    prob, x0, ui = ac.end_to_end()
    free, _ = ac.reference_solves(True)
    qd = np.abs(free[0]["X"][1:, 32:51])
    j = int(qd.max(axis=0).argmax()); peak = float(qd[:, j].max())
    v = np.full(19, np.inf); v[j] = 0.5 * peak
    z_min = float(free[1]["X"][1:, 2].min())
    srec = sc.stack_al_state_bounds([dict(joint_speed=v), dict(pelvis_z=(z_min + PELVIS_LIFT, np.inf)), dict()], 3)
    viol0 = tuple(sr.violation(free[b]["X"], srec[b]) for b in range(3))
    srec.setflags(write=False)
    return prob, x0, ui, srec, dict(joint=j, peak=peak, z_min=z_min, viol0=viol0)


@functools.lru_cache(maxsize=None)
def reference_solves(early_exit):
    """the reference driver (al_state_ref.Driver) on end_to_end(): [solve of rollout b under its state record and the model's joint / torque
    bounds at margin 0]; computed once, read-only"""
    prob, x0, ui, srec, _ = end_to_end()
    rec = br.default_record(AL_E2E["margin"])
    return [sr.Driver(prob, b, AL_E2E, rec, srec[b], max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(3)]
