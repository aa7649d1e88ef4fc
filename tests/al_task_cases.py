"""Inputs of the tests of the task family of the augmented-Lagrangian limits (test_al_task_cpu.py, test_gpu_al_task.py).  NumPy and the
oracle's host helpers only; no GPU.

  * regimes(): 9 task coordinates x 2 sides x 3 regimes = 54 rollouts at N = al_cases.N_STAGE, then STANCE_CASES more with the excited foot
    in stance at the excited knot; one window per rollout whose bounds are placed relative to that rollout's own points, a multiplier on
    every constraint, distinct penalties per rollout, the excited knot walking over 0..N; the joint / torque family and (in one of the runs)
    a state window ride along inactive with multipliers of their own.
  * end_to_end(): al_cases.end_to_end() (B = 3, N = 6) under a contact schedule with the right foot in swing, with a floor under the right
    foot of rollout 0, a swing clearance on BOTH feet of rollout 1 (the left one stands: its rows must be ignored) and no bound on rollout
    2, placed relative to the solution WITHOUT a task window.  No CoM bound here: the horizon is 0.12 s of a robot without ground contact,
    whose CoM is ballistic -- no torque moves it, no bound inside its excursion can be reached (the CoM rows are covered by regimes() and by
    the update test).
"""
import functools

import numpy as np

import al_bounds_ref as br
import al_cases as ac
import al_ref as ar
import al_state_cases as asc
import al_state_ref as sr
import al_task_ref as tr
import cost_envelope_cases as cc

sc = ac.sc
NX, NU, NQ = 51, 19, 26
N_STAGE = ac.N_STAGE
COORDS = tr.COORDS
WIDTH = 0.2                    # m: width scale of the drawn boxes
STAGE_MARGIN = asc.STAGE_MARGIN
STANCE_CASES = 6               # rollouts 54..59: foot coordinate 3 + n, side n % 2, regime 0 with a multiplier, the foot in stance there
INF_ROLLOUTS = (4, 21, 38, 47)      # a switched-off side that carries a multiplier, every regime among them


@functools.lru_cache(maxsize=None)
def regimes():
    """(X [60,5,51], U [60,4,19], mu_j, mu_c, mu_s [60,5,28,2], mu_t [60,5,9,2], rho [60,4] = (joint, ctrl, state, task), win [60,5,18],
    stance [60,5,2], srec [60,56], rec [60,76], cases, inf); read-only.  Rollout 3 (2 k + side) + g, g < 3, is task coordinate k, side
    (0 lower, 1 upper), regime g of al_cases.regimes at knot (2 k + side) % (N + 1):
      g = 0  the point 2 % of WIDTH OUTSIDE its bound, multiplier 0;
      g = 1  2 % inside, multiplier 1.5 rho |c|: mu + rho c > 0;
      g = 2  2 % inside, multiplier 0.5 rho |c|: mu + rho c < 0, the term is the constant -mu^2 / (2 rho).
    The states are sweep_base_state (off the standing pose) with the pelvis moved and turned per rollout and knot and the leg hinges moved by up
    to 0.03 rad, so that no two knots share their points.  win[i, t]: around rollout i's own points at knot t a box lo = p - a w, hi = p + b w
    with a, b in 0.1 .. 0.5 drawn per rollout, knot and coordinate (w = WIDTH): every point lies at least 10 % of WIDTH inside both bounds and
    carries a multiplier < rho times 1 % of WIDTH -- its only trace is its constant in the cost -- except the excited one, whose bound is moved
    to the stated distance from the point.  stance: drawn per rollout, knot and foot; the excited foot swings at the excited knot.
    Rollouts 54 + n: foot coordinate 3 + n, side n % 2 at knot 1 + n % N, the point 2 % OUTSIDE with a multiplier, and that foot in STANCE
    at that knot: the constant only.  inf[i] = (k, side) for the rollouts INF_ROLLOUTS: that side of a coordinate other than the excited one
    is switched off at every knot and carries a multiplier at every knot >= 1.  cases[i] = (k, side, knot, g); g = 3 marks the stance cases.
    The other families: rec[i] the model's joint / torque record at margin 0.09 i / 59, srec[i] a box of +-50 around zero (pelvis height
    included), mu_j, mu_c, mu_s of al_cases.regimes' size: inactive under rec, under STAGE_MARGIN and under srec."""
    N = N_STAGE
    X0, U0, _ = cc.limit_sweep(N)
    jr, cr = ar.ranges()
    rng = np.random.default_rng(53)
    B = 6 * COORDS + STANCE_CASES
    X = np.tile(X0[0, 0], (B, N + 1, 1)); U = np.tile(U0[0, 0], (B, N, 1))
    X[:, :, :3] += rng.uniform(-0.1, 0.1, (B, N + 1, 3))
    q = np.array([1.0, 0.0, 0.0, 0.0]) + rng.uniform(-0.15, 0.15, (B, N + 1, 4))
    X[:, :, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    X[:, :, 7:17] += rng.uniform(-0.03, 0.03, (B, N + 1, 10))            # (the legs' hinges; 0.03 rad is inside every margin used here)
    X[:, :, NQ:] = rng.uniform(-0.3, 0.3, (B, N + 1, NX - NQ))
    P = tr.points(X)
    ab = rng.uniform(0.1, 0.5, (B, N + 1, COORDS, 2))
    win = np.concatenate([P - ab[..., 0] * WIDTH, P + ab[..., 1] * WIDTH], axis=-1)
    stance = rng.integers(0, 2, (B, N + 1, 2)).astype(np.int32)
    rho = np.stack([300.0 * (1.0 + 0.011 * np.arange(B)), 40.0 * (1.0 + 0.013 * np.arange(B)), 70.0 * (1.0 + 0.017 * np.arange(B)),
                    5e4 * (1.0 + 0.019 * np.arange(B))], axis=1)
    wj, wc_ = jr[:, 1] - jr[:, 0], cr[:, 1] - cr[:, 0]
    mu_j = rng.uniform(0.1, 0.9, (B, N + 1, NU, 2)) * rho[:, 0, None, None, None] * 0.01 * wj[None, None, :, None]
    mu_c = rng.uniform(0.1, 0.9, (B, N, NU, 2)) * rho[:, 1, None, None, None] * 0.01 * wc_[None, None, :, None]
    mu_s = rng.uniform(0.1, 0.9, (B, N + 1, sr.COORDS, 2)) * rho[:, 2, None, None, None]
    mu_t = rng.uniform(0.1, 0.9, (B, N + 1, COORDS, 2)) * rho[:, 3, None, None, None] * 0.01 * WIDTH
    mu_j[:, 0] = 0.0; mu_s[:, 0] = 0.0; mu_t[:, 0] = 0.0                 # (x_0 is given: the stores keep these zero)

    def excite(i, k, side, t, d, mu):
        """the bound of side `side` of coordinate k at knot t a signed distance d inside the point (d > 0: the point is outside)"""
        w = win[i, t, COORDS + k] - win[i, t, k]
        if side:
            win[i, t, COORDS + k] = P[i, t, k] - d; win[i, t, k] = win[i, t, COORDS + k] - w
        else:
            win[i, t, k] = P[i, t, k] + d; win[i, t, COORDS + k] = win[i, t, k] + w
        mu_t[i, t, k, :] = 0.0 if t == 0 else mu_t[i, t, k, :]
        if t > 0:
            mu_t[i, t, k, side] = mu

    cases = []
    for k in range(COORDS):
        for side in range(2):
            r = 2 * k + side
            t = r % (N + 1)
            for g in range(3):
                i = 3 * r + g
                d = 0.02 * WIDTH * (1.0 if g == 0 else -1.0)
                excite(i, k, side, t, d, 0.0 if g == 0 else (1.5 if g == 1 else 0.5) * rho[i, 3] * 0.02 * WIDTH)
                if k >= 3:
                    stance[i, t, tr.FOOT_OF[k]] = 0
                cases.append((k, side, t, g))
    for n in range(STANCE_CASES):
        i, k, side, t = 6 * COORDS + n, 3 + n, n % 2, 1 + n % N
        excite(i, k, side, t, 0.02 * WIDTH, 0.7 * rho[i, 3] * 0.02 * WIDTH)
        stance[i, t, tr.FOOT_OF[k]] = 1
        cases.append((k, side, t, 3))
    inf = {}
    for n, i in enumerate(INF_ROLLOUTS):
        k = cases[i][0]
        other, s_ = (k + 1 + n) % COORDS, n % 2
        win[i, :, COORDS * s_ + other] = np.inf if s_ else -np.inf
        inf[i] = (other, s_)
    rec = np.stack([br.default_record(0.09 * i / (B - 1)) for i in range(B)])
    srec = np.tile(np.concatenate([np.full(sr.COORDS, -50.0), np.full(sr.COORDS, 50.0)]), (B, 1)) * (1.0 + 0.01 * np.arange(B))[:, None]
    for a in (X, U, mu_j, mu_c, mu_s, mu_t, rho, win, stance, srec, rec):
        a.setflags(write=False)
    return X, U, mu_j, mu_c, mu_s, mu_t, rho, win, stance, srec, rec, cases, inf


@functools.lru_cache(maxsize=None)
def stage_problem():
    """al_cases.stage_problem() with regimes()' contact schedule, one per rollout (every other reference set stays shared)"""
    prob = dict(ac.stage_problem())
    prob["stance"] = regimes()[8]
    return prob


@functools.lru_cache(maxsize=None)
def task_terms(use_stance=True, shift_row=0, swap_feet=False, swap_sides=False, roll_axis=0):
    """[(cost per knot, gx, hxx) per rollout] of regimes() under the restatement; the keyword arguments misread the inputs on purpose
    (test_al_task_cpu.py's discrimination): row t + shift_row of the window, the other foot's rows, the two sides' multipliers exchanged,
    the neighbouring axis' bounds, the stance rule ignored."""
    X, _, _, _, _, mu_t, rho, win, stance, _, _, _, _ = regimes()
    out = []
    for b in range(X.shape[0]):
        w, mu = np.array(win[b]), mu_t[b]
        if shift_row:
            w = np.roll(w, -shift_row, axis=0)
        if swap_feet:
            w = w[:, [0, 1, 2, 6, 7, 8, 3, 4, 5, 9, 10, 11, 15, 16, 17, 12, 13, 14]]
        if swap_sides:
            mu = mu[:, :, ::-1]
        if roll_axis:
            idx = np.concatenate([3 * s_ + (np.arange(3) + roll_axis) % 3 for s_ in range(3)])
            w = np.concatenate([w[:, idx], w[:, COORDS + idx]], axis=1)
        out.append(tr.traj_terms(X[b], mu, rho[b, 3], w, stance[b], use_stance))
    return out


@functools.lru_cache(maxsize=None)
def oracle_stage():
    """the oracle at ZERO constraint weights on regimes(): [(quadratics, cost) per rollout]; computed once"""
    import oracle_lib as ol
    prob = dict(stage_problem()); prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    o = ol.Oracle(prob["N"], prob["dt"])
    X, U = regimes()[:2]
    rows = []
    for b in range(X.shape[0]):
        o.set_problem(prob, b); o.set_trajectory(X[b], U[b]); o.cost_quadratics()
        rows.append(({n: o.get(n) for n in ("lx", "lu", "lxx", "luu")}, o.total_cost()))
    return rows


def stage_expected(want, cost0, b, table, state):
    """Oracle quadratics `want` (dict of one rollout, zero constraint weights) and cost `cost0` of rollout b of regimes() -> the same with the
    families' terms added: the joint / torque family under rec[b] (table) or the model's bounds at STAGE_MARGIN, the state family under
    srec[b] (state), the task family under win[b]."""
    X, U, mu_j, mu_c, mu_s, mu_t, rho, win, stance, srec, rec, _, _ = regimes()
    jrec = rec[b] if table else br.default_record(STAGE_MARGIN)
    ck, gx, hx, gu, hu = br.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b, :2], jrec)
    w = {n: want[n].copy() for n in want}
    idx = np.arange(7, NQ)
    w["lx"][:, 7:NQ] += gx; w["lu"] += gu; w["luu"] += hu; w["lxx"][:, idx, idx] += hx
    c = cost0 + ck.sum()
    if state:
        sk, sg, sh = sr.traj_terms(X[b], mu_s[b], rho[b, 2], srec[b])
        sr.add_to_quadratics(w, sg, sh); c += sk.sum()
    tk, tg, th = task_terms()[b]
    tr.add_to_quadratics(w, tg, th)
    return w, c + tk.sum()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The outer loop of the end-to-end case: al_state_cases.AL_E2E (whose note on the horizon holds here: 0.12 s of a robot without ground
# contact) with the task family's penalty and tolerance in metres.  The right foot swings over the whole horizon, so that its rows count.
AL_E2E = dict(asc.AL_E2E, rounds=4, rho_task0=1e7, tol_task=2e-5)
MAX_ITER = ac.MAX_ITER
FOOT_LIFT = (2e-4, 5e-4)       # m above the unconstrained minimum of the right ankle's height, rollouts 0 and 1


def al_args(al=AL_E2E):
    """the arguments of set_augmented_lagrangian among `al`"""
    return {k: v for k, v in al.items() if k not in ("rho_state0", "tol_state", "rho_task0", "tol_task")}


@functools.lru_cache(maxsize=None)
def e2e_problem():
    """al_cases.end_to_end() with the right foot in swing at every knot (left foot in stance)"""
    prob, x0, ui = ac.end_to_end()
    prob = dict(prob)
    st = np.array(prob["stance"]); st[:, :, 1] = 0
    st.setflags(write=False)
    prob["stance"] = st
    return prob, x0, ui


@functools.lru_cache(maxsize=None)
def free_solves(early_exit):
    """the reference driver on e2e_problem() WITHOUT a task window"""
    prob, x0, ui = e2e_problem()
    rec = br.default_record(AL_E2E["margin"])
    return [tr.Driver(prob, b, AL_E2E, rec, None, None, max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(3)]


@functools.lru_cache(maxsize=None)
def end_to_end():
    """(prob, x0 [3,51], u_init [3,6,19], win [3,7,18], info); read-only.  From the solution WITHOUT a task window (free_solves, convergence exit):
      rollout 0  the right ankle's height bounded below FOOT_LIFT[0] above its minimum over the knots 1..N (the key right_foot);
      rollout 1  both ankles' heights bounded below FOOT_LIFT[1] above the right ankle's minimum (the shorthand swing_clearance): the left
                 foot stands, its ankle is BELOW that floor at some knot (info["left_below"] > 0), and its rows must not count;
      rollout 2  every bound infinite.
    info = dict(z_min [2], left_below, viol0 = the violation of these bounds by that solution per rollout)."""
    prob, x0, ui = e2e_problem()
    free = free_solves(True)
    N = prob["N"]
    P = [tr.points(free[b]["X"]) for b in range(2)]
    z_min = [float(P[b][1:, 8].min()) for b in range(2)]
    win = sc.stack_al_task_bounds([dict(right_foot=((-np.inf, -np.inf, z_min[0] + FOOT_LIFT[0]), np.inf)), dict(swing_clearance=z_min[1] + FOOT_LIFT[1]), dict()], 3, N)
    viol0 = tuple(tr.violation(free[b]["X"], win[b], prob["stance"][b]) for b in range(3))
    win.setflags(write=False)
    return prob, x0, ui, win, dict(z_min=z_min, left_below=float(z_min[1] + FOOT_LIFT[1] - P[1][1:, 5].min()), viol0=viol0)


@functools.lru_cache(maxsize=None)
def reference_solves(early_exit):
    """the reference driver (al_task_ref.Driver) on end_to_end(): [solve of rollout b under its task window and the model's joint / torque
    bounds at margin 0]; computed once, read-only"""
    prob, x0, ui, win, _ = end_to_end()
    rec = br.default_record(AL_E2E["margin"])
    return [tr.Driver(prob, b, AL_E2E, rec, None, win[b], max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(3)]
