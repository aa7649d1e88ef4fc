"""Sliding contact (contact modes 3 / 4: stance_correct<KIN>, lin_slide_tangent<KIN>, lin_contact_multipliers, the up-axis recursion of
h1_linearize_contact_dev.h) and the joint-limit rows (limit_lock_mask, apply_lock_mask, step_lim<KIN>, the CONTACT == 5 path with
lim_second_pass_lds, lin2_tangent_legs_c<.., LIM> with lockc2) away from the standing pose: the states of tests/contact_envelope_cases.py
-- rotations of +-0.5 rad, velocities of +-3, both feet, either foot alone and no foot in stance, friction coefficients 0.3 and 0.7,
non-unit quaternions, controls beyond and on ctrlrange; every hinge past its upper and its lower limit moving out, moving back in slowly,
and exactly ON a limit, with and without the restoring stiffness -- against the oracle's step and forward-mode AD.  Small shapes (16
rollouts, N = 2 or 4: every knot of rollout i carries state i); test_contact_envelope_cpu.py shows that these inputs discriminate, that they
stay inside the caps asserted again here on what the device computes, and how far the oracle's two derivations agree on them.

Tolerances are those of the existing tests of the same quantities, relative to max(1, max |want|): 1e-9 the stance-constrained step, 1e-8
the contact Jacobians; the rows of a stopped hinge 1e-10 (1e-12 with the pure stop and on B), as the golden tests hold them.  Every test
prints the worst error it saw and the counts seen on the device."""
import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
from test_gpu_configs import _solver, env, rel  # noqa: F401  (env, rel: the helpers of the sibling GPU tests)
from test_gpu_dynamics_envelope import _check, _report, _stage_jacobians

pytestmark = pytest.mark.gpu
NS, NX, NU, NQ, H = cc.NS, cc.NX, cc.NU, cc.NQ, cc.H
STEP_TOL, JAC_TOL = cc.STEP_TOL, cc.JAC_TOL


def _handle(mode, mu=None, limits=False, k=0.0, N=2, schedule=False):
    s = _solver(NS, N=N); s.set_problem(dc.problem(N, dc.SCHEDULE if schedule else None)); s.set_contact_mode(mode)
    s.set_options(jacobian_mode=0)
    return cc.configure(s, mu, limits, k)


def _device_steps(s, x, u, mode):
    """[16,P,51]: the device's step of every (state, stance pattern)"""
    return np.stack([s.step_stance(x, u, int(sl), int(sr)) for sl, sr in cc.rows(mode)], axis=1)


@pytest.mark.parametrize("mu", cc.MUS)
@pytest.mark.parametrize("mode", [3, 4])
def test_sliding_step_matches_oracle_on_the_kept_cases(mode, mu):
    c = cc.sliding_cases(mode, mu)
    x, u, kept = c["x"], c["u"], c["kept"]
    s = _handle(mode, mu)
    got = _device_steps(s, x, u, mode)
    s.set_contact_mode(3); got3 = got if mode == 3 else _device_steps(s, x, u, 3)
    s.set_contact_mode(2); got2 = _device_steps(s, x, u, 2)
    s.set_contact_mode(mode); s.set_friction(cc.MU_STICK); stick = _device_steps(s, x, u, mode)
    s.close()
    worst = {}
    for i, p in np.argwhere(kept):
        _check(got[i, p], c["step"][i, p], STEP_TOL, worst, "stance %d%d" % tuple(dc.STANCE_ROWS[p]), (mode, mu, i))
    slides = np.abs(got3 - got2).max(axis=2) > 1e-6                   # the cone decision, as the device took it
    dropped, sliding = cc.check_sliding_caps(kept, slides, (mode, mu, "device"))
    assert np.array_equal(slides[kept], c["slides"][kept])
    assert np.array_equal(stick, got2)                                  # cone inactive: modes 3 / 4 ARE mode 2, bit for bit, in all 64 cases
    n = (slides & kept).sum(axis=0)
    _report("sliding step, mode %d, mu %.1f (%d of %d cases kept; on the device %d of 48 stance cases slide: both feet %d, left only %d, right only %d)"
            % (mode, mu, kept.sum(), kept.size, sliding, n[0], n[1], n[2]), worst)


@pytest.mark.parametrize("variant,mu", cc.SLIDING_VARIANTS)
@pytest.mark.parametrize("mode", [3, 4])
def test_sliding_analytic_jacobians_match_oracle_ad(mode, variant, mu):
    """N = 4, one stance pattern per knot (dynamics_envelope_cases.SCHEDULE).  The oracle's AD agrees with central differences of its own
    step to 6e-11 max(1, |want|) on these inputs, 1.6e-10 in mode 4 at mu 0.7, where the quotient's rounding is the limit
    (test_contact_envelope_cpu.py QUOTIENT_LIMITED): the bound stays the project's 1e-8."""
    c = cc.sliding_cases(mode, mu, variant)
    x, u, kept, beyond = c["x"], c["u"], c["kept"], c["beyond"]
    s = _handle(mode, mu, N=4, schedule=True)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    worst = {}
    cc.check_sliding_caps(kept, c["slides"], (mode, variant, mu))
    for i, p in np.argwhere(kept):
        key = "sliding" if c["slides"][i, p] else "sticking or free"
        _check(A[i, p], c["A"][i, p], JAC_TOL, worst, "A, " + key, (mode, variant, mu, i, p))
        _check(Bm[i, p], c["B"][i, p], JAC_TOL, worst, "B, " + key, (mode, variant, mu, i, p))
        assert np.all(Bm[i, p][:, beyond[i]] == 0.0), (i, p)
        if beyond[i].any():
            assert np.abs(Bm[i, p][:, ~beyond[i]]).max(axis=0).min() > 1e-3
    _report("sliding Jacobians, mode %d, %s, mu %.1f (%d of %d cases kept, %d of them slide)"
            % (mode, variant, mu, kept.sum(), kept.size, (c["slides"] & kept).sum()), worst)


@pytest.mark.parametrize("k", cc.K_STIFF)
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_joint_limit_step_and_jacobians_match_oracle_hinge_by_hinge(mode, k):
    """Step (step_kind 3 / 4, and 5 in mode 0) and Jacobians with the rows; for every hinge the oracle stops, the rows the golden tests pin:
    v+ = -h k r, velocity row of A = -h k e_theta, row of B = 0, position row (1 - h^2 k) e_theta.  A hinge exactly ON a limit is free.
    The oracle's AD agrees with central differences of its own step to 3e-11 max(1, |want|) on these inputs; in mode 1 to 1.4e-9, where
    the rounding noise of the rigid double-support solve limits the quotient (test_contact_envelope_cpu.py QUOTIENT_LIMITED): the bound
    stays the project's 1e-8 there too."""
    c = cc.limit_cases(mode, k)
    x, u, kept = c["x"], c["u"], c["kept"]
    mu = cc.MU_LIMITS if mode >= 3 else None
    s = _handle(mode, mu, True, k)
    got = _device_steps(s, x, u, mode)
    s.close()
    worst = {}
    for i, p in np.argwhere(kept):
        _check(got[i, p], c["step"][i, p], STEP_TOL, worst, "step", (mode, k, i, p))
    stopped = cc.stopped_hinges(x, got, k)                              # as the device decided
    dropped, n_stopped, up, lo = cc.check_limit_caps(kept, stopped, (mode, k, "device"))
    assert np.array_equal(stopped[kept], c["stopped"][kept])
    s = _handle(mode, mu, True, k, N=4, schedule=True) if mode else _handle(0, None, True, k, N=2)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    row_tol = 1e-10 if k else 1e-12
    for i, p in np.argwhere(kept):
        _check(A[i, p], c["A"][i, p], JAC_TOL, worst, "A", (mode, k, i, p))
        _check(Bm[i, p], c["B"][i, p], JAC_TOL, worst, "B", (mode, k, i, p))
        if mode == 0:
            assert np.array_equal(A[i, 1], A[i, 0]) and np.array_equal(Bm[i, 1], Bm[i, 0])
        for j in np.flatnonzero(c["stopped"][i, p]):
            e = np.zeros(NX); e[7 + j] = -H * k
            e2 = np.zeros(NX); e2[7 + j] = 1.0 - H * H * k
            for key, err, tol in (("stopped hinge, velocity row of A (absolute)", np.abs(A[i, p][NQ + 6 + j] - e).max(), row_tol),
                                  ("stopped hinge, row of B (absolute)", np.abs(Bm[i, p][NQ + 6 + j]).max(), 1e-12),
                                  ("stopped hinge, position row of A (absolute)", np.abs(A[i, p][7 + j] - e2).max(), row_tol)):
                worst[key] = max(worst.get(key, 0.0), err)
                assert err <= tol, (mode, k, i, p, j, key, err)
        for j in np.flatnonzero(c["cls"][i] == 6):                      # ON the limit: the free hinge's velocity row, not the stop's
            e = np.zeros(NX); e[7 + j] = -H * k
            assert np.abs(A[i, p][NQ + 6 + j] - e).max() > 1e-3, (mode, k, i, p, j)
    _report("joint-limit rows, mode %d, k %g (%d of %d cases kept; on the device %d hinge-cases stopped, %d distinct hinges at the upper end, %d at the lower)"
            % (mode, k, kept.sum(), kept.size, n_stopped, up, lo), worst)


@pytest.mark.parametrize("kind", sorted(cc.STEP_KINDS))
def test_rollout_instantiations_follow_the_oracle_knot_by_knot(kind):
    """step_kind 1 .. 5 of the rollout kernel (dyn_step_shared.h step_any<CONTACT>): a cold start rolls the group's controls, held over the
    horizon, out from the group's states under SCHEDULE; every knot of xbar is the oracle's step of the device's own previous knot.  The
    continuity filter is recomputed at those knots."""
    mode, limits = cc.STEP_KINDS[kind]
    k = cc.K_STIFF[1] if limits else 0.0
    mu = cc.MU_LIMITS if mode >= 3 else None
    x0, u = cc.limit_states() if limits else cc.sliding_states()[:2]
    N = 4
    ui = np.repeat(u[:, None, :], N, axis=1)
    s = _handle(mode, mu, limits, k, N=N, schedule=True)
    s.initialize(x0, ui)
    X, U = s.xbar(), s.ubar()
    s.close()
    assert np.array_equal(X[:, 0], x0) and np.array_equal(U, ui) and np.all(np.isfinite(X))
    o = cc.configure(dc.oracle(N=N, mode=mode, stance=dc.SCHEDULE), mu, limits, k)
    kept = np.zeros((NS, N), dtype=bool)
    drift = np.zeros((NS, N))
    for b in range(NS):
        As = []
        for sgn in (0.0, 1.0, -1.0):
            o.set_trajectory(cc.scaled(X[b], sgn), U[b]); o.linearize()
            As.append(o.get("A"))
        drift[b] = [max(np.abs(As[q][t] - As[0][t]).max() for q in (1, 2)) / max(1.0, np.abs(As[0][t]).max()) for t in range(N)]
        for t in range(N):
            kept[b, t] = dc.contact_kept(mode, X[b, t][None], u[b][None], o=o, rows=dc.SCHEDULE[t][None])[0, 0] and drift[b, t] <= 1e-4
    assert (~kept).sum() * 8 <= kept.size, (kind, int((~kept).sum()))
    worst = {}
    moved = 0
    for b, t in np.argwhere(kept):
        want = o.step_stance(X[b, t], u[b], dc.SCHEDULE[t])
        _check(X[b, t + 1], want, STEP_TOL, worst, "knot %d (stance %d%d)" % (t + 1, *dc.SCHEDULE[t]), (kind, b, t))
        if limits:
            moved += int(cc.stopped_hinges(X[b, t][None], X[b, t + 1][None, None], k).sum())
    if limits:
        assert moved >= 64                                             # (the states stop 73 hinges or more at the first knot alone)
    _report("rollout, step_kind %d (mode %d%s; %d of %d knots kept%s)"
            % (kind, mode, ", joint-limit rows, k %g" % k if limits else "", kept.sum(), kept.size, "; %d hinge-knots stopped" % moved if limits else ""), worst)
