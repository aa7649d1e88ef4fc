"""Inputs of the tests of the task-velocity family of the augmented-Lagrangian limits (test_al_task_vel_cpu.py, test_gpu_al_task_vel.py).
NumPy and the oracle's host helpers only; no GPU.

  * regimes(): 9 velocity coordinates x 2 sides x 3 regimes = 54 rollouts at N = al_cases.N_STAGE, then SWING_CASES more whose excited foot
    SWINGS at the excited knot (only the constant remains); the states of al_task_cases.regimes(); one window per rollout whose bounds are
    placed relative to that rollout's own velocities, a multiplier on every constraint, distinct penalties per rollout, the excited knot
    walking over 0..N (knot N for the CoM's z row and for two foot rows); the joint / torque family, a state window and a POSITION task
    window ride along -- the position window active on the CoM's position at the knot where this family excites the CoM's velocity, and on
    the excited foot's position at a knot where that foot swings.
  * end_to_end(): al_cases.end_to_end() (B = 3, N = 6) under a schedule with the left foot in stance and the right one in swing, with a cap
    on the stance foot's speed on rollout 0, the same cap on BOTH feet on rollout 1 (the right one swings: its rows must be ignored) and no
    bound on rollout 2, placed relative to the solution WITHOUT a window.  No CoM bound here: the horizon is 0.12 s of a robot without ground
    contact, whose CoM is ballistic (al_task_cases says so for positions; regimes() and the update test cover the CoM rows).
"""
import functools

import numpy as np

import al_bounds_ref as br
import al_cases as ac
import al_ref as ar
import al_state_cases as asc
import al_state_ref as sr
import al_task_cases as tc
import al_task_ref as tr
import al_task_vel_ref as vr

sc = ac.sc
NX, NU, NQ = 51, 19, 26
N_STAGE = ac.N_STAGE
COORDS = vr.COORDS
WIDTH = 0.2                    # m/s: width scale of the drawn boxes
STAGE_MARGIN = asc.STAGE_MARGIN
SWING_CASES = 6                # rollouts 54..59: foot coordinate 3 + n, side n % 2, 2 % outside with a multiplier, the foot in SWING there
INF_ROLLOUTS = (4, 21, 38, 47)      # a switched-off side that carries a multiplier, every regime among them


@functools.lru_cache(maxsize=None)
def regimes():
    """dict, read-only arrays: X [60,5,51], U [60,4,19], mu_j, mu_c, mu_s, mu_p [60,5,9,2] (the position task family's), mu_v [60,5,9,2],
    rho [60,5] = (joint, ctrl, state, task, taskvel), pwin [60,5,18] (the position window), win [60,5,18], stance [60,5,2], srec [60,56],
    rec [60,76], cases, inf.  Rollout 3 (2 k + side) + g, g < 3, is velocity coordinate k, side (0 lower, 1 upper), regime g of
    al_cases.regimes at knot (2 k + side) % (N + 1):
      g = 0  the velocity 2 % of WIDTH OUTSIDE its bound, multiplier 0;
      g = 1  2 % inside, multiplier 1.5 rho |c|: mu + rho c > 0;
      g = 2  2 % inside, multiplier 0.5 rho |c|: mu + rho c < 0, the term is the constant -mu^2 / (2 rho).
    X, U, mu_j, mu_c, mu_s, srec, rec and the first four penalties are al_task_cases.regimes()': states off the standing pose, random
    velocities up to 0.3.  win[i, t]: around rollout i's own velocities at knot t a box lo = v - a w, hi = v + b w with a, b in 0.1 .. 0.5
    drawn per rollout, knot and coordinate (w = WIDTH): every velocity lies at least 10 % of WIDTH inside both bounds and carries a
    multiplier < rho times 1 % of WIDTH -- its only trace is its constant in the cost -- except the excited one, whose bound is moved to
    the stated distance.  stance: drawn per rollout, knot and foot; the excited foot STANDS at the excited knot.
    Rollouts 54 + n: foot coordinate 3 + n, side n % 2 at knot 1 + n % N, 2 % OUTSIDE with a multiplier, and that foot in SWING at that
    knot: the constant only.  inf[i] = (k, side) for the rollouts INF_ROLLOUTS: that side of a coordinate other than the excited one is
    switched off at every knot and carries a multiplier at every knot >= 1.  cases[i] = (k, side, knot, g); g = 3 marks the swing cases.
    The position window pwin / mu_p: boxes around the same states' points drawn as al_task_cases.regimes() draws its own (every point
    well inside, a small multiplier on every constraint), then excited by hand: on rollouts of a CoM row (k < 3, g < 3) the CoM's position coordinate k at the
    SAME knot, 2 % of tc.WIDTH outside with multiplier 0 -- slot 0 and slot 1 of that knot's record both carry a family's term; on rollouts
    of a foot row the same foot's position coordinate at knot (t + 2) % (N + 1), where the schedule here makes that foot swing -- position
    rows active at a swing knot, velocity rows at a stance knot of one foot."""
    N = N_STAGE
    X, U, mu_j, mu_c, mu_s, _, rho4, _, _, srec, rec, _, _ = tc.regimes()
    rng = np.random.default_rng(97)
    B = 6 * COORDS + SWING_CASES
    assert X.shape[0] == B
    V = vr.velocities(X)
    P = tr.points(X)
    ab = rng.uniform(0.1, 0.5, (B, N + 1, COORDS, 2))
    win = np.concatenate([V - ab[..., 0] * WIDTH, V + ab[..., 1] * WIDTH], axis=-1)
    stance = rng.integers(0, 2, (B, N + 1, 2)).astype(np.int32)
    rho = np.concatenate([rho4, (6e4 * (1.0 + 0.023 * np.arange(B)))[:, None]], axis=1)
    mu_v = rng.uniform(0.1, 0.9, (B, N + 1, COORDS, 2)) * rho[:, 4, None, None, None] * 0.01 * WIDTH
    mu_v[:, 0] = 0.0                                                     # (x_0 is given: the store keeps these zero)
    # the position window: boxes drawn as al_task_cases.regimes() draws its own, every point at least 10 % of tc.WIDTH inside
    abp = rng.uniform(0.1, 0.5, (B, N + 1, COORDS, 2))
    pwin = np.concatenate([P - abp[..., 0] * tc.WIDTH, P + abp[..., 1] * tc.WIDTH], axis=-1)
    mu_p = rng.uniform(0.1, 0.9, (B, N + 1, COORDS, 2)) * rho[:, 3, None, None, None] * 0.01 * tc.WIDTH
    mu_p[:, 0] = 0.0

    def excite(w_, val, mu_, i, k, side, t, d, mu, width):
        """the bound of side `side` of coordinate k at knot t a signed distance d inside the value (d > 0: the value is outside)"""
        w = w_[i, t, COORDS + k] - w_[i, t, k]
        if side:
            w_[i, t, COORDS + k] = val[i, t, k] - d; w_[i, t, k] = w_[i, t, COORDS + k] - w
        else:
            w_[i, t, k] = val[i, t, k] + d; w_[i, t, COORDS + k] = w_[i, t, k] + w
        mu_[i, t, k, :] = 0.0 if t == 0 else mu_[i, t, k, :]
        if t > 0:
            mu_[i, t, k, side] = mu

    cases = []
    for k in range(COORDS):
        for side in range(2):
            r = 2 * k + side
            t = r % (N + 1)
            for g in range(3):
                i = 3 * r + g
                d = 0.02 * WIDTH * (1.0 if g == 0 else -1.0)
                excite(win, V, mu_v, i, k, side, t, d, 0.0 if g == 0 else (1.5 if g == 1 else 0.5) * rho[i, 4] * 0.02 * WIDTH, WIDTH)
                if k >= 3:
                    f, t2 = vr.FOOT_OF[k], (t + 2) % (N + 1)
                    stance[i, t, f] = 1; stance[i, t2, f] = 0
                    excite(pwin, P, mu_p, i, k, side, t2, 0.02 * tc.WIDTH, 0.0, tc.WIDTH)
                else:
                    excite(pwin, P, mu_p, i, k, side, t, 0.02 * tc.WIDTH, 0.0, tc.WIDTH)
                cases.append((k, side, t, g))
    for n in range(SWING_CASES):
        i, k, side, t = 6 * COORDS + n, 3 + n, n % 2, 1 + n % N
        excite(win, V, mu_v, i, k, side, t, 0.02 * WIDTH, 0.7 * rho[i, 4] * 0.02 * WIDTH, WIDTH)
        stance[i, t, vr.FOOT_OF[k]] = 0
        cases.append((k, side, t, 3))
    inf = {}
    for n, i in enumerate(INF_ROLLOUTS):
        k = cases[i][0]
        other, s_ = (k + 1 + n) % COORDS, n % 2
        win[i, :, COORDS * s_ + other] = np.inf if s_ else -np.inf
        inf[i] = (other, s_)
    out = dict(X=X, U=U, mu_j=mu_j, mu_c=mu_c, mu_s=mu_s, mu_p=mu_p, mu_v=mu_v, rho=rho, pwin=pwin, win=win, stance=stance, srec=srec, rec=rec, V=V, P=P)
    for a in out.values():
        a.setflags(write=False)
    out.update(cases=cases, inf=inf)
    return out


@functools.lru_cache(maxsize=None)
def stage_problem():
    """al_cases.stage_problem() with regimes()' contact schedule, one per rollout (every other reference set stays shared)"""
    prob = dict(ac.stage_problem())
    prob["stance"] = regimes()["stance"]
    return prob


@functools.lru_cache(maxsize=None)
def taskvel_terms(use_swing=True, shift_row=0, swap_feet=False, swap_sides=False, roll_axis=0):
    """[(cost per knot, gx, hxx) per rollout] of regimes() under the restatement; the keyword arguments misread the inputs on purpose
    (test_al_task_vel_cpu.py's discrimination): row t + shift_row of the window, the other foot's rows, the two sides' multipliers
    exchanged, the neighbouring axis' bounds, the swing rule ignored."""
    R = regimes()
    X, mu_v, rho, win, stance = R["X"], R["mu_v"], R["rho"], R["win"], R["stance"]
    out = []
    for b in range(X.shape[0]):
        w, mu = np.array(win[b]), mu_v[b]
        if shift_row:
            w = np.roll(w, -shift_row, axis=0)
        if swap_feet:
            w = w[:, [0, 1, 2, 6, 7, 8, 3, 4, 5, 9, 10, 11, 15, 16, 17, 12, 13, 14]]
        if swap_sides:
            mu = mu[:, :, ::-1]
        if roll_axis:
            idx = np.concatenate([3 * s_ + (np.arange(3) + roll_axis) % 3 for s_ in range(3)])
            w = np.concatenate([w[:, idx], w[:, COORDS + idx]], axis=1)
        out.append(vr.traj_terms(X[b], mu, rho[b, 4], w, stance[b], use_swing))
    return out


@functools.lru_cache(maxsize=None)
def position_terms():
    """[(cost per knot, gx, hxx) per rollout] of the position task family under regimes()' pwin, mu_p and schedule (al_task_ref)"""
    R = regimes()
    return [tr.traj_terms(R["X"][b], R["mu_p"][b], R["rho"][b, 3], R["pwin"][b], R["stance"][b]) for b in range(R["X"].shape[0])]


@functools.lru_cache(maxsize=None)
def oracle_stage():
    """the oracle at ZERO constraint weights on regimes(): [(quadratics, cost) per rollout]; computed once"""
    import oracle_lib as ol
    prob = dict(stage_problem()); prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    o = ol.Oracle(prob["N"], prob["dt"])
    R = regimes()
    rows = []
    for b in range(R["X"].shape[0]):
        o.set_problem(prob, b); o.set_trajectory(R["X"][b], R["U"][b]); o.cost_quadratics()
        rows.append(({n: o.get(n) for n in ("lx", "lu", "lxx", "luu")}, o.total_cost()))
    return rows


def stage_expected(b, table=False, state=False, position=False):
    """The oracle's quadratics and cost of rollout b of regimes() (zero constraint weights) with the families' terms added: the joint /
    torque family under rec[b] (table) or the model's bounds at STAGE_MARGIN, the state family under srec[b] (state), the position task
    family under pwin[b] (position), this family under win[b].  Returns (dict of lx, lu, lxx, luu; cost)."""
    R = regimes()
    want, cost0 = oracle_stage()[b]
    jrec = R["rec"][b] if table else br.default_record(STAGE_MARGIN)
    ck, gx, hx, gu, hu = br.traj_terms(R["X"][b], R["U"][b], R["mu_j"][b], R["mu_c"][b], R["rho"][b, :2], jrec)
    w = {n: want[n].copy() for n in want}
    idx = np.arange(7, NQ)
    w["lx"][:, 7:NQ] += gx; w["lu"] += gu; w["luu"] += hu; w["lxx"][:, idx, idx] += hx
    c = cost0 + ck.sum()
    if state:
        sk, sg, sh = sr.traj_terms(R["X"][b], R["mu_s"][b], R["rho"][b, 2], R["srec"][b])
        sr.add_to_quadratics(w, sg, sh); c += sk.sum()
    if position:
        pk, pg, ph = position_terms()[b]
        tr.add_to_quadratics(w, pg, ph); c += pk.sum()
    vk, vg, vh = taskvel_terms()[b]
    vr.add_to_quadratics(w, vg, vh)
    return w, c + vk.sum()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The outer loop of the end-to-end case: al_task_cases.AL_E2E's joint / torque part with this family's penalty and tolerance in m/s.  The
# left foot stands over the whole horizon, so that its rows count; the right one swings.
AL_E2E = dict(asc.AL_E2E, rounds=4, rho_taskvel0=1e5, tol_taskvel=1e-4)
MAX_ITER = ac.MAX_ITER
# The cap on the stance foot's speed as a fraction of the largest speed that foot reaches over the knots 1..N in the solution without a
# window, per rollout (0, 1).  Adjusted on the CPU until the reference driver alone meets the end-to-end conditions
# (test_al_task_vel_cpu.py: done within the installed rounds in both exit modes, a multiplier > 0 in the result).  Rollout 1 meets them at a
# half.  Rollout 0 does not: its stance foot moves most along z, where the contact-free horizon lets it fall with the robot; at a half the
# driver is done with the foot strictly inside the cap and every multiplier back at zero, at 0.7 the cap is active in the result (at
# rho_taskvel0 = 1e5; at 1e3 neither is done in four rounds).
CAP_FRACTION = (0.7, 0.5)


def al_args(al=AL_E2E):
    """the arguments of set_augmented_lagrangian among `al`"""
    return {k: v for k, v in al.items() if k not in ("rho_state0", "tol_state", "rho_task0", "tol_task", "rho_taskvel0", "tol_taskvel")}


def e2e_problem():
    """al_cases.end_to_end() with the left foot in stance and the right foot in swing at every knot (al_task_cases.e2e_problem)"""
    return tc.e2e_problem()


@functools.lru_cache(maxsize=None)
def free_solves(early_exit):
    """the reference driver on e2e_problem() WITHOUT a window"""
    prob, x0, ui = e2e_problem()
    rec = br.default_record(AL_E2E["margin"])
    return [vr.Driver(prob, b, AL_E2E, rec, None, None, None, max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(3)]


@functools.lru_cache(maxsize=None)
def end_to_end():
    """(prob, x0 [3,51], u_init [3,6,19], win [3,7,18], info); read-only.  From the solution WITHOUT a window (free_solves, convergence exit):
      rollout 0  |v| <= cap on the axis of the LEFT (stance) ankle's velocity on which it moves most, cap = CAP_FRACTION[0] x the largest
                 speed it reaches there over the knots 1..N (the key left_foot_vel);
      rollout 1  the same construction from its own solution, as |v| <= cap on all three axes of BOTH feet (the shorthand stance_slip): the
                 right foot swings and is faster than the cap at some knot (info["right_over"] > 0), and its rows must not count;
      rollout 2  every bound infinite.
    info = dict(axis [2], cap [2], right_over, viol0 = the violation of these bounds by that solution per rollout)."""
    prob, x0, ui = e2e_problem()
    free = free_solves(True)
    N = prob["N"]
    V = [vr.velocities(free[b]["X"]) for b in range(2)]
    axis = [int(np.abs(V[b][1:, 3:6]).max(axis=0).argmax()) for b in range(2)]
    cap = [CAP_FRACTION[b] * float(np.abs(V[b][1:, 3 + axis[b]]).max()) for b in range(2)]
    lo, hi = np.full(3, -np.inf), np.full(3, np.inf)
    lo[axis[0]], hi[axis[0]] = -cap[0], cap[0]
    cap1 = CAP_FRACTION[1] * float(np.abs(V[1][1:, 3:6]).max())
    cap[1] = cap1
    win = vr.stack_al_task_vel_bounds([dict(left_foot_vel=(lo, hi)), dict(stance_slip=cap1), dict()], 3, N)
    viol0 = tuple(vr.violation(free[b]["X"], win[b], prob["stance"][b]) for b in range(3))
    win.setflags(write=False)
    return prob, x0, ui, win, dict(axis=axis, cap=cap, right_over=float(np.abs(V[1][1:, 6:9]).max() - cap1), viol0=viol0)


@functools.lru_cache(maxsize=None)
def reference_solves(early_exit):
    """the reference driver (al_task_vel_ref.Driver) on end_to_end(): [solve of rollout b under its window and the model's joint / torque
    bounds at margin 0]; computed once, read-only"""
    prob, x0, ui, win, _ = end_to_end()
    rec = br.default_record(AL_E2E["margin"])
    return [vr.Driver(prob, b, AL_E2E, rec, None, None, win[b], max_iter=MAX_ITER, early_exit=early_exit).solve(x0[b], ui[b]) for b in range(3)]
