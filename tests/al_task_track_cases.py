"""Inputs of the tests of the task family's bounds track and of the task score of the resident plant (test_al_task_track_cpu.py,
test_gpu_al_task_track.py, test_gpu_plant_task_score.py).  NumPy and the oracle's host helpers only; no GPU.

  * N = al_cases.N_STAGE = 4, the smallest horizon tests/test_gpu_al_knot.py uses; tracks of ROWS = N + 4 rows, so that the end clamp is hit
    from step 3 on; B = 3 and B = 70 (a wave plus six lanes).
  * SCHEDULE / FOOTSTEPS: a hand-written 12-row contact schedule and its footstep plan for scenario.al_task_track_from_footsteps.
  * task_track(): a task track whose every row and coordinate is a different pair of finite numbers (a cut that reads another row, or
    another column, gives other bits) but for a few infinite sides.
  * score_case(): B = 70 plant states, a window and a schedule per rollout and a tolerance for the task score.  The windows are placed
    relative to the points of the plant's initial state, which is ring row 0 of the scored run bit for bit (a kick changes velocities
    only); see the function.
"""
import functools

import numpy as np

import al_cases as ac
import al_task_ref as tr

sc = ac.sc
NX, NU, NQ, NV = 51, 19, 26, 25
N = ac.N_STAGE
ROWS = N + 4
B_SMALL, B_WAVE = 3, 70
COORDS = tr.COORDS
DT = 0.02

# ---- the footstep helper: 12 rows, (left, right), 1 = stance.  Left swings in rows 2..5; right in rows 0..1 and 8..11 (reaching the last row)
SCHEDULE = np.array([(1, 0), (1, 0), (0, 1), (0, 1), (0, 1), (0, 1), (1, 1), (1, 1), (1, 0), (1, 0), (1, 0), (1, 0)], dtype=np.int32)
PHASES = {"left": [(2, 6)], "right": [(0, 2), (8, 12)]}
FOOTSTEPS = {"left": [(0.30, 0.20)], "right": [(0.10, -0.20), (0.50, -0.21)]}
HALF = (0.05, 0.03)
CLEARANCE = 0.10


@functools.lru_cache(maxsize=None)
def task_track(rows=ROWS):
    """[rows, 18]: lo = -(1 + r / 8 + k / 128), hi = 2 + r / 16 + k / 256: every finite entry distinct; the lower bound of coordinate 4 is
    -inf in rows 2 and 5, the upper bound of coordinate 7 +inf in row 3"""
    r, k = np.arange(rows)[:, None], np.arange(COORDS)[None, :]
    lo = -(1.0 + r / 8.0 + k / 128.0)
    hi = 2.0 + r / 16.0 + k / 256.0
    t = np.concatenate([lo, hi], axis=1)
    t[[2, 5], 4] = -np.inf
    t[3, COORDS + 7] = np.inf
    assert len(np.unique(t[np.isfinite(t)])) == np.isfinite(t).sum()
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def active_track(rows=ROWS):
    """[rows, 18] around the standing pose, for solves that feel the bounds: a floor under both ankles that rises by half a millimetre per
    row from 2 mm above the standing ankle height (felt by a foot in swing), and a CoM box in y, 4 mm wide, that drifts by a millimetre per
    row.  Every row differs from every other, so a solve under a window cut from other rows is another solve."""
    p = tr.points(sc.standing_state())
    r = np.arange(rows)
    lo, hi = np.full((rows, 3), -np.inf), np.full((rows, 3), np.inf)
    zl, zr = lo.copy(), lo.copy()
    zl[:, 2] = p[5] + 2e-3 + 5e-4 * r; zr[:, 2] = p[8] + 2e-3 + 5e-4 * r
    clo, chi = lo.copy(), hi.copy()
    clo[:, 1] = p[1] - 2e-3 + 1e-3 * r; chi[:, 1] = p[1] + 2e-3 + 1e-3 * r
    t = sc.stack_al_task_bounds(dict(com=(clo, chi), left_foot=(zl, hi), right_foot=(zr, hi)), 1, rows - 1)[0]
    t.setflags(write=False)
    return t


def install_window():
    """the window a handle installs the task family with before a track is cut: [1, N+1, 18] with no bound (the installation supplies
    rho_task0 and tol_task; the track the bounds)"""
    return np.tile(tr.NO_BOUNDS, (1, N + 1, 1))


# ---- the score
TOL = 0.02                    # m: the threshold of the counts
SMALL, LARGE = 0.01, 0.04     # m: designed violations below and above TOL
KICK = 0.05                   # m/s on the pelvis' y velocity: the points move ~1 mm per interval
STANCE_PATTERN = np.array([(1, 1), (1, 0), (0, 1), (0, 0), (0, 1), (1, 0), (1, 1)], dtype=np.int32)
INF_ROLLOUTS = (5, 40, 66)    # rollouts whose excited side is switched off: the same point, no violation


@functools.lru_cache(maxsize=None)
def score_problem(B=B_WAVE, seed=41):
    """(prob, x0, ui): the standing problem at N with a contact schedule per rollout whose rows differ from knot to knot and from rollout to
    rollout; ui: scenario.synthetic_batch's noise around ZERO torque (u_init(ug) adds a gravity compensation, which the GPU tests take
    from the library); read-only"""
    import oracle_lib as ol
    prob = sc.make_problem(ol.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    x0, ui = sc.synthetic_batch(B, N, seed, np.zeros(NU))
    st = np.ascontiguousarray(STANCE_PATTERN[(np.arange(B)[:, None] + 2 * np.arange(N + 1)[None, :]) % len(STANCE_PATTERN)])
    for b in range(B):      # the foot whose side score_case excites (coordinate b % 9): in swing at the knots 0 and 2, in stance at knot 1
        if b % COORDS >= 3:
            st[b, [0, 2], tr.FOOT_OF[b % COORDS]] = 0; st[b, 1, tr.FOOT_OF[b % COORDS]] = 1
    assert all((st[:, t] != st[:, t + 1]).any() for t in range(N)) and (st[1:] != st[:-1]).any()
    st.setflags(write=False)
    prob["stance"] = st
    for a in (x0, ui):
        a.setflags(write=False)
    return prob, x0, ui


@functools.lru_cache(maxsize=None)
def score_case(B=B_WAVE):
    """(prob, x0, ui, win [B, N+1, 18], P0 [B, 9], excited [B] = (k, side, size)); read-only.
    Around rollout b's own points P0[b] = points(x0[b]) every knot t gets a box lo = P0 - a, hi = P0 + c with a, c in 0.1 .. 0.3 m drawn per
    rollout, knot and coordinate: far inside.  Then ONE side per rollout is excited at every knot: coordinate k = b % 9, side (b // 9) % 2
    (0 the lower bound), the bound moved so that the point lies SMALL ((b // 18) % 2 == 0) or LARGE outside it, plus 1 mm per knot (rows
    differ: scoring against another knot's row changes the record by 1e-3).  Over B = 70 rollouts every one of the 18 sides is excited
    with both sizes.  The rollouts INF_ROLLOUTS have their excited side switched off instead.  Whether a foot's violation counts is the
    schedule's business: score_problem's schedule has the excited foot in swing at the knots 0 and 2 and in stance at knot 1, where its
    violation must not count; the other foot follows the pattern."""
    prob, x0, ui = score_problem(B)
    rng = np.random.default_rng(43)
    P0 = tr.points(x0)
    a = rng.uniform(0.1, 0.3, (B, N + 1, COORDS, 2))
    win = np.concatenate([P0[:, None] - a[..., 0], P0[:, None] + a[..., 1]], axis=-1)
    excited = []
    for b in range(B):
        k, side, size = b % COORDS, (b // COORDS) % 2, (SMALL if (b // (2 * COORDS)) % 2 == 0 else LARGE)
        for t in range(N + 1):
            d = size + 1e-3 * t
            if side:
                win[b, t, COORDS + k] = P0[b, k] - d
                win[b, t, k] = min(win[b, t, k], win[b, t, COORDS + k] - 0.1)
            else:
                win[b, t, k] = P0[b, k] + d
                win[b, t, COORDS + k] = max(win[b, t, COORDS + k], win[b, t, k] + 0.1)
        if b in INF_ROLLOUTS:
            win[b, :, COORDS * side + k] = np.inf if side else -np.inf
        excited.append((k, side, size))
    win.setflags(write=False); P0.setflags(write=False)
    return prob, x0, ui, win, P0, tuple(excited)


def u_init(ui, ug):
    """synthetic_batch's initial controls around the gravity compensation ug [19]"""
    return np.clip(ui + np.asarray(ug)[None, None, :], -0.8 * sc.CTRLRANGE, 0.8 * sc.CTRLRANGE)


def kick(B=B_WAVE):
    dv = np.zeros((B, NV)); dv[:, 1] = KICK
    return dv
