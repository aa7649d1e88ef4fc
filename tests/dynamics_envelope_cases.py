"""Input builders for the dynamics tests away from the standing pose (test_dynamics_envelope_cpu.py, test_gpu_dynamics_envelope.py):
seeded STATES and CONTROLS at which every branch and factor of the analytic linearisation (h1_linearize_dev.h lin_prologue /
lin_column, h1_linearize_contact_dev.h) and of the step carries weight.  NumPy and the CPU oracle only; no GPU.

Sixteen states per group, physical gravity, h = 0.02 unless `h` is given (TIMESTEPS: the other steps the kernels are held to the oracle
at; the builders set prob["dt"] = h, and a handle must be constructed with dt = prob["dt"]); hinges strictly inside their ranges (the joint-limit rows have goldens of their own, and
contact_envelope_cases.py takes them and contact modes 3 / 4 off the standing pose).

  * wide():     hinges at 2 % .. 98 % of their ranges, base rotation vectors in +-3 rad (state 0: an angle of pi - 1e-3), all 25
                velocities in +-5, controls in +-0.9 ctrlrange.
  * nonunit():  wide() with the quaternion of state i scaled by a factor in [0.5, 1.6]  (2 / |q| in Hq, the normalised qh).
  * negq():     wide() with the quaternion negated  (w < 0).
  * clamped():  wide() with actuator j of state i at +1.3 ctrlrange where (i + j) % 4 == 0 and at -1.2 ctrlrange where (i + j) % 4 == 2
                -- every actuator beyond each end in four states -- and one further actuator per state exactly ON a limit.
  * spin():     wide() with the base angular velocity solved for a prescribed POST-step angular velocity w' (the oracle's step), so that
                s = |h w'|^2 -- the argument of the small-spin Taylor branch, threshold 1e-6 -- takes the values of SPIN_S.
  * rest():     four wide() poses at rest without torque, for ZERO gravity: s == 0.0 exactly.
  * mid():      hinges +-0.4 about standing, rotation +-0.5 rad, velocities +-3: the states of the contact modes.
  * contact_kept(): which (state, stance pattern) pairs of a set the contact-mode step is continuous at (no active-set decision on a tie).
"""
import functools

import numpy as np

import oracle_lib as ol
from conftest import load_package

sc = load_package().scenario
NX, NU, NQ, NV = 51, 19, 26, 25
NS = 16                                     # states per group
H = 0.02
TIMESTEPS = (0.005, 0.01, 0.04)               # the other time steps of test_timestep_cpu.py / test_gpu_timestep.py
GRAVITY = (0.0, 0.0, -9.81)
SEED = 20
STANCE_ROWS = np.array([[1, 1], [1, 0], [0, 1], [0, 0]], dtype=np.int32)
SCHEDULE = np.vstack([STANCE_ROWS, STANCE_ROWS[:1]])       # N = 4: knot p steps under STANCE_ROWS[p] (the terminal row steps nothing)
SPIN_THRESHOLD = 1e-6
# s = |h w'|^2 of spin() state i: eight below the threshold (one within a factor 2), eight above (one within a factor 2, two above 1e-2)
SPIN_S = np.array([1e-14, 1e-11, 1e-9, 3e-8, 1e-7, 3e-7, 6e-7, 9.5e-7, 1.05e-6, 1.6e-6, 4e-6, 3e-5, 1e-3, 6e-3, 2e-2, 6e-2])
POS = np.r_[0:3, 7:26]; VEL = np.r_[26:29, 32:51]          # position rows of A and the velocity rows they are e_p + h x of
E_POS = np.zeros((22, NX)); E_POS[np.arange(22), POS] = 1.0
QUAT_SCALE = np.array([0.5, 1.6, 0.7, 1.3, 0.9, 1.1, 0.6, 1.45, 0.8, 1.2, 0.55, 1.55, 0.95, 1.05, 0.65, 1.35])


def problem(N=2, stance=None, gravity=GRAVITY, h=H):
    """shipped problem under physical gravity with prob["dt"] = h; `stance` [N+1,2] (default: both feet at every knot)"""
    prob = sc.make_problem(ol.reference_kinematics, N=N, gravity=gravity, stance=stance)
    assert prob["dt"] == H
    prob["dt"] = float(h)
    return prob


def oracle(N=2, mode=0, stance=None, gravity=GRAVITY, h=H, **opts):
    prob = problem(N, stance, gravity, h)
    o = ol.Oracle(N, prob["dt"]); o.set_problem(prob); o.set_contact_mode(mode)
    if opts:
        o.set_options(**opts)
    return o


def _inside(frac):
    jr = ol.joint_ranges()
    return jr[:, 0] + frac * (jr[:, 1] - jr[:, 0])


def wide():
    """(x [16,51], u [16,19])"""
    rng = np.random.default_rng(SEED)
    x = np.tile(sc.standing_state(), (NS, 1))
    x[:, 0:3] += rng.uniform(-0.3, 0.3, (NS, 3))
    rv = rng.uniform(-3.0, 3.0, (NS, 3))
    rv[0] *= (np.pi - 1e-3) / np.linalg.norm(rv[0])                    # a rotation next to pi: w = cos(angle / 2) = 5e-4
    x[:, 3:7] = sc._axis_angle_quat(rv)
    x[:, 7:NQ] = _inside(rng.uniform(0.02, 0.98, (NS, NQ - 7)))
    x[:, NQ:] = rng.uniform(-5.0, 5.0, (NS, NV))
    u = rng.uniform(-0.9, 0.9, (NS, NU)) * sc.CTRLRANGE
    return x, u


def normalised(x):
    y = x.copy()
    y[:, 3:7] /= np.linalg.norm(y[:, 3:7], axis=1, keepdims=True)
    return y


def nonunit(xu=None):
    x, u = wide() if xu is None else xu
    x = x.copy(); x[:, 3:7] *= QUAT_SCALE[:, None]
    return x, u


def negq():
    x, u = wide()
    x = x.copy(); x[:, 3:7] *= -1.0
    return x, u


def clamp_pattern():
    """(above [16,19], below [16,19], on_limit [16,19]) boolean masks of clamped(); on_limit: +limit in even states, -limit in odd ones"""
    i, j = np.arange(NS)[:, None], np.arange(NU)[None, :]
    above, below = (i + j) % 4 == 0, (i + j) % 4 == 2
    on = (j == (5 * i + 1) % NU) | (j == (5 * i + 2) % NU)
    on &= ~(above | below)
    return above, below, on


def clamped(xu=None):
    """(x, u, beyond [16,19]): beyond = the controls outside ctrlrange (their columns of B are zero); the ones ON a limit are inside"""
    x, u = wide() if xu is None else xu
    above, below, on = clamp_pattern()
    sign = np.where(np.arange(NS)[:, None] % 2 == 0, 1.0, -1.0)
    cr = np.broadcast_to(sc.CTRLRANGE, (NS, NU))
    u = np.where(above, 1.3 * cr, np.where(below, -1.2 * cr, np.where(on, sign * cr, u)))
    return x, u, above | below


def pulled_inside(u):
    """clamped controls with everything beyond a limit pulled back to 0.9 of it"""
    return np.clip(u, -0.9 * sc.CTRLRANGE, 0.9 * sc.CTRLRANGE)


def spin_s(x, u, o=None, h=H):
    """s = |h w'|^2 of every state: w' the post-step base angular velocity of the oracle's constraint-free step (`o`: an oracle AT `h`)"""
    o = o or oracle(h=h)
    return np.array([(h * h) * (o.step(xi, ui)[NQ + 3:NQ + 6] ** 2).sum() for xi, ui in zip(x, u)])


def spin(h=H):
    """(x, u): wide() with w chosen so that w' = sqrt(SPIN_S[i]) / h along a seeded direction (fixed point of w <- w - (w'(w) - target):
    d w' / d w = I + O(h): it contracts by 0.03 per pass at h = 0.02 and by 0.74 at h = 0.04, hence the cap of 600 passes)"""
    x, u = wide()
    x = x.copy()
    o = oracle(h=h)
    rng = np.random.default_rng(SEED + 1)
    d = rng.standard_normal((NS, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    for i in range(NS):
        target = d[i] * np.sqrt(SPIN_S[i]) / h
        for _ in range(600):
            r = o.step(x[i], u[i])[NQ + 3:NQ + 6] - target
            if np.abs(r).max() < 1e-13 * max(1.0, np.abs(target).max()):
                break
            x[i, NQ + 3:NQ + 6] -= r
    return x, u


def rest():
    """(x [4,51], u [4,19]): the first four wide() poses at rest, no torque -- under ZERO gravity (pass gravity=(0, 0, 0)) every
    acceleration is an exact zero, so s = |h w'|^2 == 0.0: the point the Taylor branch exists for (sin(a / 2) / a at a = 0)"""
    x = wide()[0][:4].copy()
    x[:, NQ:] = 0.0
    return x, np.zeros((4, NU))


def mid():
    rng = np.random.default_rng(SEED + 2)
    x = np.tile(sc.standing_state(), (NS, 1))
    x[:, 0:3] += rng.uniform(-0.05, 0.05, (NS, 3))
    x[:, 3:7] = sc._axis_angle_quat(rng.uniform(-0.5, 0.5, (NS, 3)))
    x[:, 7:NQ] = np.clip(x[:, 7:NQ] + rng.uniform(-0.4, 0.4, (NS, NQ - 7)), _inside(0.02), _inside(0.98))
    x[:, NQ:] = rng.uniform(-3.0, 3.0, (NS, NV))
    u = rng.uniform(-0.9, 0.9, (NS, NU)) * sc.CTRLRANGE
    return x, u


def contact_kept(mode, x, u, o=None, rows=STANCE_ROWS, h=H):
    """kept [16,4] (bool; column p = STANCE_ROWS[p]): the oracle's contact-mode step is continuous at the state -- its result at the
    state and at the state with its velocities scaled by (1 +- 1e-7) differ by less than 1e-4 -- so no active-set decision of the
    unilateral rule sits on a rounding tie that the device may settle the other way.  `o`: an oracle with further settings (friction,
    joint-limit rows) in place of the plain one of `mode`; `rows`: the stance patterns, one column of `kept` each."""
    o = o or oracle(mode=mode, h=h)
    kept = np.zeros((len(x), len(rows)), dtype=bool)
    for i, (xi, ui) in enumerate(zip(x, u)):
        for p, st in enumerate(rows):
            f0 = o.step_stance(xi, ui, st)
            ok = True
            for sgn in (1.0, -1.0):
                xs = xi.copy(); xs[NQ:] *= 1.0 + sgn * 1e-7
                ok &= np.abs(o.step_stance(xs, ui, st) - f0).max() < 1e-4
            kept[i, p] = ok
    return kept


def stage_trajectory(x, u, N=2):
    """(X [B,N+1,51], U [B,N,19]): every knot of rollout i carries state x[i] and control u[i]"""
    return np.repeat(x[:, None, :], N + 1, axis=1), np.repeat(u[:, None, :], N, axis=1)


FREE_GROUPS = ("wide", "nonunit", "negq", "clamped", "spin")


def group(name, h=H):
    """(x, u) of a free-flight group (only spin depends on the time step)"""
    return dict(wide=wide, nonunit=nonunit, negq=negq, clamped=lambda: clamped()[:2], spin=lambda: spin(h))[name]()


def oracle_jacobians(x, u, mode=0, jac_mode=0, fd_eps=1e-5, gravity=GRAVITY, h=H):
    """AD (jac_mode 0) or forward-difference Jacobians of the oracle's step at every state: (A [n,51,51], B [n,51,19]); in a contact mode
    (A [n,4,51,51], B [n,4,51,19]), knot p under STANCE_ROWS[p]"""
    if mode == 0:
        o = oracle(N=1, gravity=gravity, h=h, jac_mode=jac_mode, fd_eps=fd_eps)
    else:
        o = oracle(N=4, mode=mode, stance=SCHEDULE, gravity=gravity, h=h, jac_mode=jac_mode, fd_eps=fd_eps)
    As, Bs = [], []
    for xi, ui in zip(x, u):
        X, U = stage_trajectory(xi[None], ui[None], o.N)
        o.set_trajectory(X[0], U[0]); o.linearize()
        A, B = o.get("A"), o.get("B")
        As.append(A[0] if mode == 0 else A); Bs.append(B[0] if mode == 0 else B)
    return np.array(As), np.array(Bs)


@functools.lru_cache(maxsize=None)
def group_ad(name, h=H):
    """the oracle's AD Jacobians of a free-flight group, computed once per time step and shared: treat as read-only"""
    A, B = oracle_jacobians(*group(name, h), h=h)
    A.setflags(write=False); B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def mid_cases(mode, variant="mid", h=H):
    """(x, u, kept [16,4], A [16,4,51,51], B [16,4,51,19], beyond [16,19]) of the contact modes: variant "mid", or its "nonunit" /
    "clamped" transformation; computed once per time step and shared: treat as read-only"""
    x, u = mid()
    beyond = np.zeros((NS, NU), dtype=bool)
    if variant == "nonunit":
        x, u = nonunit((x, u))
    elif variant == "clamped":
        x, u, beyond = clamped((x, u))
    kept = contact_kept(mode, x, u, h=h)
    A, B = oracle_jacobians(x, u, mode=mode, h=h)
    for a in (x, u, kept, A, B, beyond):
        a.setflags(write=False)
    return x, u, kept, A, B, beyond
