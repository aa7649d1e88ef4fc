"""Input builders for the tests of sliding contact (contact modes 3 / 4) and of the joint-limit rows away from the standing pose
(test_contact_envelope_cpu.py, test_gpu_contact_envelope.py), beside dynamics_envelope_cases.py, whose states, schedule and step-continuity
rule they reuse.  NumPy and the CPU oracle only; no GPU.

Sixteen states per group, physical gravity, h = 0.02 unless `h` is given, N = 4 under SCHEDULE: knot p steps under STANCE_ROWS[p] (both feet, left only, right
only, none) and every knot of rollout i carries state i.  Contact mode 0 has no stance rows: one case per state there, not four.

  * sliding group:  mid() (rotation +-0.5 rad, hinges +-0.4 about standing, velocities +-3) at the friction coefficients MUS, and for
                    MUS[0] its nonunit / clamped transformations.  MU_STICK is a coefficient at which no foot of mid() leaves the cone.
  * limits group:   mid() with hinge j of state i, c = (i + j) % 8:
                      c = 0   0.03 past the upper limit, velocity +1.5   (moving out: stopped)
                      c = 4   0.03 past the lower limit, velocity -1.5   (moving out: stopped)
                      c = 2   0.03 past the upper limit, velocity -0.2   (moving in slowly: the restoring term h k r = 0.375 decides)
                      c = 6   exactly ON a limit (upper in even states, lower in odd ones), velocity 1.5 outward: the comparison is
                              strict, so never a stop
                    restoring stiffness K_STIFF (0 and 625 = 1 / (2 h)^2, the value of the committed stiffness golden); MU_LIMITS in modes
                    3 / 4.
  * kept cases:     the step-continuity rule of contact_kept AND the oracle's AD Jacobian A at the state and at the state with its
                    velocities scaled by (1 +- 1e-7) agree to 1e-4 max(1, |A|max): a branch flip moves A by more than 1e-3.
"""
import functools

import numpy as np

import dynamics_envelope_cases as dc
import oracle_lib as ol

NS, NX, NU, NQ, NJ, H = dc.NS, dc.NX, dc.NU, dc.NQ, 19, dc.H
MUS = (0.3, 0.7)
MU_LIMITS = 0.3
MU_STICK = 1e3                 # (test_contact_envelope_cpu.py: the oracle's mode-3 / mode-4 step IS its mode-2 step at this coefficient, in all 64 cases)
K_STIFF = (0.0, 625.0)
PAST = 0.03
STEP_TOL, JAC_TOL = 1e-9, 1e-8  # the bounds of the existing tests of the stance-constrained step and of the contact Jacobians, relative to max(1, max |want|)
SLIDING_VARIANTS = (("mid", 0.3), ("mid", 0.7), ("nonunit", 0.3), ("clamped", 0.3))
# step_kind (dyn_step_shared.h) -> (contact mode, joint-limit rows): the instantiations of the rollout / line-search kernels
STEP_KINDS = {1: (2, False), 2: (4, False), 3: (2, True), 4: (4, True), 5: (0, True)}
# (kind, h) of test_gpu_timestep.py: sliding in modes 3 / 4 (mid, mu 0.3) and the joint-limit rows (mode 2, k 625) at the steps of
# dc.TIMESTEPS at which the reference keeps at least the share of cases it keeps at 0.02 (test_timestep_cpu.py measures it)
TIMESTEP_CASES = tuple((kind, h) for kind in ("sliding3", "sliding4", "limits2") for h in dc.TIMESTEPS)      # all of them: 64 of 64 pairs kept


def rows(mode):
    """the stance patterns of a contact mode: STANCE_ROWS, or one (ignored) pattern in mode 0"""
    return dc.STANCE_ROWS if mode else dc.STANCE_ROWS[:1]


def configure(o, mu=None, limits=False, k=0.0):
    """friction and joint-limit rows on an oracle or on a solver handle (the same setter names)"""
    if mu is not None:
        o.set_friction(mu)
    o.set_joint_limits(bool(limits))
    o.set_joint_limit_stiffness(k if limits else 0.0)
    return o


def oracle(mode, mu=None, limits=False, k=0.0, h=H, **opts):
    """the oracle of a mode: N = 4 under SCHEDULE, or (mode 0) N = 1"""
    o = dc.oracle(N=4, mode=mode, stance=dc.SCHEDULE, h=h, **opts) if mode else dc.oracle(N=1, h=h, **opts)
    return configure(o, mu, limits, k)


def steps(o, x, u, mode):
    """the oracle's step of every (state, stance pattern): [n,P,51]"""
    return np.array([[o.step_stance(xi, ui, st) for st in rows(mode)] for xi, ui in zip(x, u)])


def jacobians(o, x, u):
    """the oracle's Jacobians (AD, or what its options select) at every state, knot p under pattern p: (A [n,P,51,51], B [n,P,51,19])"""
    As, Bs = [], []
    for xi, ui in zip(x, u):
        X, U = dc.stage_trajectory(xi[None], ui[None], o.N)
        o.set_trajectory(X[0], U[0]); o.linearize()
        As.append(o.get("A")); Bs.append(o.get("B"))
    return np.array(As), np.array(Bs)


def scaled(x, sgn):
    xs = x.copy(); xs[..., NQ:] *= 1.0 + sgn * 1e-7
    return xs


def kept_cases(o, x, u, mode, A=None):
    """(kept [n,P], drift): step continuity (contact_kept) and Jacobian continuity under the (1 +- 1e-7) velocity scaling; drift = the
    largest relative change of A among the kept cases"""
    if A is None:
        A = jacobians(o, x, u)[0]
    kept = dc.contact_kept(mode, x, u, o=o, rows=rows(mode))
    d = np.zeros(kept.shape)
    for sgn in (1.0, -1.0):
        As = jacobians(o, scaled(x, sgn), u)[0]
        d = np.maximum(d, np.abs(As - A).max(axis=(2, 3)) / np.maximum(1.0, np.abs(A).max(axis=(2, 3))))
    kept &= d <= 1e-4
    return kept, float(d[kept].max()) if kept.any() else 0.0


FD_LADDER = (4e-4, 1.6e-3, 1e-4, 2.5e-5)
FD_CONVERGED = 1e-11


def central_differences(o, x, u, st):
    """(J [51,70] = [A B], gap [70]) of the oracle's step under the stance pattern `st` by sixth-order central differences of step_stance,
    a derivation that shares nothing with its forward-mode AD but the step itself (truncation eps^6 f^(7) / 140, rounding about 1e-15 / eps).
    gap: per column, how far the fourth-order quotient of the same samples is from the sixth-order one, relative to max(1, |J|max) -- the
    quotient's own measure of its convergence, no AD involved.  A column whose gap exceeds FD_CONVERGED at the first step of FD_LADDER (a
    branch of the step within three steps of the state, or a stiff stance solve) takes the step of the ladder with the smallest gap."""
    z = np.concatenate([x, u])

    def column(c, eps):
        f = []
        for a in (1, 2, 3):
            zp, zm = z.copy(), z.copy()
            zp[c] += a * eps; zm[c] -= a * eps
            f.append(o.step_stance(zp[:NX], zp[NX:], st) - o.step_stance(zm[:NX], zm[NX:], st))
        return (45.0 * f[0] - 9.0 * f[1] + f[2]) / (60.0 * eps), (8.0 * f[0] - f[1]) / (12.0 * eps)

    first = [column(c, FD_LADDER[0]) for c in range(NX + NU)]
    J = np.array([d6 for d6, _ in first]).T
    scale = max(1.0, np.abs(J).max())
    gap = np.array([np.abs(d6 - d4).max() for d6, d4 in first]) / scale
    for c in np.flatnonzero(gap > FD_CONVERGED):
        for eps in FD_LADDER[1:]:
            d6, d4 = column(c, eps)
            g = np.abs(d6 - d4).max() / scale
            if g < gap[c]:
                gap[c], J[:, c] = g, d6
    return J, gap


def sliding_states(variant="mid"):
    """(x, u, beyond [16,19])"""
    x, u = dc.mid()
    beyond = np.zeros((NS, NU), dtype=bool)
    if variant == "nonunit":
        x, u = dc.nonunit((x, u))
    elif variant == "clamped":
        x, u, beyond = dc.clamped((x, u))
    return x, u, beyond


def limit_pattern():
    """(cls [16,19] = (i + j) % 8, end [16,19]: +1 a hinge set at / past its upper limit, -1 its lower one, 0 untouched)"""
    i, j = np.arange(NS)[:, None], np.arange(NJ)[None, :]
    cls = (i + j) % 8
    end = np.where((cls == 0) | (cls == 2), 1, np.where(cls == 4, -1, 0))
    end = np.where(cls == 6, np.where(i % 2 == 0, 1, -1), end)
    return cls, end


def limit_states():
    """(x, u): mid() with the pattern of the module docstring"""
    x, u = dc.mid()
    x = x.copy()
    jr = ol.joint_ranges()
    cls, end = limit_pattern()
    lim = np.where(end > 0, jr[:, 1], jr[:, 0])
    th, v = x[:, 7:NQ], x[:, NQ + 6:]
    past = (cls == 0) | (cls == 2) | (cls == 4)
    th[past] = (lim + PAST * end)[past]
    th[cls == 6] = lim[cls == 6]                                       # exactly the table's value
    v[(cls == 0) | (cls == 4) | (cls == 6)] = (1.5 * end)[(cls == 0) | (cls == 4) | (cls == 6)]
    v[cls == 2] = -0.2
    return x, u


def violation(x):
    """r [.., 19]: how far every hinge is past its range (signed; 0 inside and ON a limit)"""
    jr = ol.joint_ranges()
    th = x[..., 7:NQ]
    return np.where(th > jr[:, 1], th - jr[:, 1], np.where(th < jr[:, 0], th - jr[:, 0], 0.0))


def stopped_hinges(x, xn, k, h=H):
    """[n,P,19] bool: hinge j of state i is stopped in the step x[i] -> xn[i,p] when its new velocity is the row's, v+ = -h k r, to 1e-10"""
    r = violation(x)[:, None, :]
    return np.abs(xn[..., NQ + 6:] + h * k * r) < 1e-10


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def mode2_steps(variant="mid", h=H):
    """the oracle's mode-2 step of the sliding states, [16,4,51]: what a step without the cone is; computed once per time step, read-only"""
    x, u, _ = sliding_states(variant)
    return _freeze(steps(oracle(2, h=h), x, u, 2))[0]


@functools.lru_cache(maxsize=None)
def sliding_cases(mode, mu, variant="mid", h=H):
    """dict of a sliding parametrisation: x, u, beyond, kept [16,4], A, B (AD), step [16,4,51], slides [16,4] (the oracle's mode-3 step
    differs from its mode-2 step by more than 1e-6), drift.  Computed once per time step and shared: read-only"""
    x, u, beyond = sliding_states(variant)
    o = oracle(mode, mu, h=h)
    A, B = jacobians(o, x, u)
    kept, drift = kept_cases(o, x, u, mode, A)
    xn = steps(o, x, u, mode)
    x3 = xn if mode == 3 else steps(oracle(3, mu, h=h), x, u, 3)
    slides = np.abs(x3 - mode2_steps(variant, h)).max(axis=2) > 1e-6
    _freeze(x, u, beyond, kept, A, B, xn, slides)
    return dict(x=x, u=u, beyond=beyond, kept=kept, A=A, B=B, step=xn, slides=slides, drift=drift)


@functools.lru_cache(maxsize=None)
def limit_cases(mode, k, h=H):
    """dict of a joint-limit parametrisation: x, u, kept [16,P], A, B (AD), step [16,P,51], stopped [16,P,19], drift, cls, end; P = 4, or 1
    in mode 0.  Computed once per time step and shared: read-only"""
    x, u = limit_states()
    cls, end = limit_pattern()
    o = oracle(mode, MU_LIMITS if mode >= 3 else None, True, k, h=h)
    A, B = jacobians(o, x, u)
    kept, drift = kept_cases(o, x, u, mode, A)
    xn = steps(o, x, u, mode)
    stopped = stopped_hinges(x, xn, k, h)
    _freeze(x, u, kept, A, B, xn, stopped, cls, end)
    return dict(x=x, u=u, kept=kept, A=A, B=B, step=xn, stopped=stopped, drift=drift, cls=cls, end=end)


def check_sliding_caps(kept, slides, tag):
    """the caps of a sliding parametrisation (`slides` of the mid states at its mu): (dropped, sliding stance cases)"""
    assert (~kept).sum() * 8 <= kept.size, (tag, "dropped", int((~kept).sum()))
    n = (slides & kept)[:, :3].sum(axis=0)
    assert n.sum() >= 24 and n[1] >= 4 and n[2] >= 4, (tag, "sliding cases per pattern", n.tolist())
    assert not slides[:, 3].any(), tag                                 # (no foot in stance: nothing to slide)
    return int((~kept).sum()), int(n.sum())


def check_limit_caps(kept, stopped, tag):
    """the caps of a joint-limit parametrisation: (dropped, stopped hinge-cases, hinges stopped at the upper end, at the lower end)"""
    cls, end = limit_pattern()
    assert (~kept).sum() * 8 <= kept.size, (tag, "dropped", int((~kept).sum()))
    st = stopped & kept[:, :, None]
    assert st.any(axis=(0, 1)).all(), (tag, "hinges never stopped", np.flatnonzero(~st.any(axis=(0, 1))).tolist())
    up = (st & (end > 0)[:, None, :]).any(axis=(0, 1)).sum(); lo = (st & (end < 0)[:, None, :]).any(axis=(0, 1)).sum()
    assert up >= 12 and lo >= 12, (tag, "hinges stopped at the upper / lower end", int(up), int(lo))
    assert not (stopped & (cls == 6)[:, None, :]).any(), (tag, "a hinge ON its limit was stopped")
    assert not (stopped & (end == 0)[:, None, :]).any(), (tag, "a hinge inside its range was stopped")
    return int((~kept).sum()), int(st.sum()), int(up), int(lo)
