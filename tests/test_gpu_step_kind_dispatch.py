"""Every launcher of the two-lane family reaches the step kind it is asked for (dyn_step_shared.h with_step_kind): for each of the six
kinds -- 0, and 1 .. 5 of contact_envelope_cases.STEP_KINDS -- the step of (x, u) under both feet is taken through every kernel that is
instantiated per kind and compared with ref = step_stance(x, u, 1, 1) of the same handle:

  rollout      knot 1 of a cold start                                                     k_rollout_s<K>
  last step    last knot after initialize_warm_resident on a trajectory of (x, u)         k_last_step_s<K>
  warm tail    the re-rolled knot of ilqr_hip_initialize_warm_resident_shifted(.., 1)     k_warm_tail_s<K>
  advance      plant_advance: one substep, feedback mode 0, schedule source               k_plant_advance<K, 0>
  follow       first interval of plant_follow(0, 2) (row 1 of the history ring)           k_plant_follow<K, 0>
  fd           three columns of the forward-difference Jacobians of the stage API         k_fd_steps_s<K>
               (a hinge angle, a hinge rate, a control) against the quotient of step_stance itself

16 states, N = 4, both feet in stance over the horizon: the limit states for the kinds with joint-limit rows, the sliding states for the
others, friction and stiffness as test_gpu_contact_envelope.py chooses them.

Kinds 1 .. 5: every comparison of a step is BITWISE -- one non-inlined constrained step per translation unit, the same machine code behind
every kernel.  Kind 0, the inlined constraint-free step: an unconstrained handle takes ref, the last step and the warm tail on the one-lane
kernels (k_step_r, k_last_step_r, k_warm_tail_r) -- BITWISE --, the rollout and the plant on the two-lane ones: NOT bitwise (3.6e-16 of
max(1, |ref|) on these states), bound contact_envelope_cases.STEP_TOL.  fd: 2e-5 absolute, the bound of
test_forward_difference_jacobians_two_lane_vs_scalar_kernels (measured: exact for kinds 1 .. 5, 1.1e-9 for kind 0).  Which comparisons are
bitwise was measured on the commit before the dispatch helpers, with this file unchanged.

That the kinds can be told apart at all: at state DISCRIMINATING of the limit states the oracle's six steps differ pairwise by 9.3 or more
(smallest gap over the fifteen pairs; computed with dynamics_envelope_cases.oracle / contact_envelope_cases.configure); the device's six
steps of that state are asserted to differ pairwise by more than 1e-6, so a launcher that landed on another instantiation cannot pass."""
import ctypes
import itertools

import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
from test_gpu_contact_envelope import _handle

pytestmark = pytest.mark.gpu
NS, NX, NU, NQ = cc.NS, cc.NX, cc.NU, cc.NQ
N = 4
KINDS = {0: (0, False), **cc.STEP_KINDS}
DISCRIMINATING = 6
FD_EPS, FD_TOL = 1e-5, 2e-5
FD_COLUMNS = (7 + 3, NQ + 6 + 12, NX + 5)       # left knee angle, a left-arm hinge rate, a right-leg control
STEPS = ("rollout", "last step", "warm tail", "advance", "follow")
BITWISE = {kind: STEPS if kind else ("last step", "warm tail") for kind in KINDS}


def _run(kind):
    mode, limits = KINDS[kind]
    k = cc.K_STIFF[1] if limits else 0.0
    mu = cc.MU_LIMITS if mode >= 3 else None
    x, u = (np.ascontiguousarray(a, dtype=np.float64) for a in (cc.limit_states() if limits else cc.sliding_states()[:2]))
    X, U = dc.stage_trajectory(x, u, N)
    s = _handle(mode, mu, limits, k, N=N)
    s.set_max_iterations(1)
    r = dict(x=x, u=u, ref=s.step_stance(x, u, 1, 1))
    xl, ul = cc.limit_states()
    r["disc"] = s.step_stance(xl[DISCRIMINATING:DISCRIMINATING + 1], ul[DISCRIMINATING:DISCRIMINATING + 1], 1, 1)[0]
    s.initialize(x, U)
    r["rollout"] = s.xbar()[:, 1]
    s.solve(x)                                                        # (the plant follows the policy of a solve: its gains multiply x - xbar_0 = 0 below)
    assert np.all(np.isfinite(s.gains_K()))
    s.set_trajectory(X, U); s.initialize_warm_resident(x)
    r["last step"] = s.xbar()[:, N]
    assert np.array_equal(s.xbar()[:, N - 1], x) and np.array_equal(s.ubar()[:, N - 1], u)
    s.set_trajectory(X, U)
    s._chk(s.L.ilqr_hip_initialize_warm_resident_shifted(s.h, x.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1))
    r["warm tail"] = s.xbar()[:, N]
    s.set_trajectory(X, U)
    s.plant_configure(substeps=1, feedback_mode=0, contact_source="schedule")
    s.plant_reset(x); s.plant_advance(); s.synchronize()
    r["advance"] = s.plant_state()
    assert np.array_equal(s.plant_control(), u) and s.plant_alive().all()
    s.plant_set_history(2); s.plant_reset(x); s.plant_follow(0, 2); s.synchronize()
    hx, hu = s.plant_history()
    assert np.array_equal(hx[0], x) and np.array_equal(hu[0], u)
    r["follow"] = hx[1]
    s.set_options(jacobian_mode=1, fd_eps=FD_EPS)
    s.set_trajectory(X, U); s.stage_linearize()
    A, Bm = s.linearization()
    J = np.concatenate([A[:, 0], Bm[:, 0]], axis=2)                   # [16,51,70]
    r["fd"] = np.stack([J[:, :, c] for c in FD_COLUMNS], axis=1)
    want = []
    for c in FD_COLUMNS:
        z = np.concatenate([x, u], axis=1); z[:, c] += FD_EPS
        want.append((s.step_stance(z[:, :NX], z[:, NX:], 1, 1) - r["ref"]) / FD_EPS)
    r["fd want"] = np.stack(want, axis=1)
    s.close()
    return r


@pytest.fixture(scope="module")
def runs():
    return {kind: _run(kind) for kind in sorted(KINDS)}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_every_launcher_takes_the_step_of_its_kind(runs, kind):
    r = runs[kind]
    ref = r["ref"]
    assert np.all(np.isfinite(ref)) and np.abs(ref - r["x"]).max() > 1e-3
    scale = np.maximum(1.0, np.abs(ref).max(axis=1, keepdims=True))
    errs = {key: (np.abs(r[key] - ref) / scale).max() for key in STEPS}
    fd_err = np.abs(r["fd"] - r["fd want"]).max()
    for key in STEPS:                                                  # (every figure first, then the assertions)
        print("step kind %d, %-9s: %s, worst error relative to max(1, |ref|) %.2e" % (kind, key, "bitwise" if np.array_equal(r[key], ref) else "not bitwise", errs[key]))
    print("step kind %d, fd       : worst absolute error of three columns %.2e (largest entry %.2e)" % (kind, fd_err, np.abs(r["fd want"]).max()))
    for key in STEPS:
        if key in BITWISE[kind]:
            assert np.array_equal(r[key], ref), (kind, key, errs[key])
        else:
            assert errs[key] <= cc.STEP_TOL, (kind, key, errs[key])
    assert fd_err < FD_TOL, (kind, fd_err)
    assert np.abs(r["fd want"]).max(axis=(0, 2)).min() > 1e-3         # (every chosen column moves the step)


def test_the_six_kinds_differ_pairwise_at_the_discriminating_state(runs):
    gaps = {(a, b): np.abs(runs[a]["disc"] - runs[b]["disc"]).max() for a, b in itertools.combinations(sorted(KINDS), 2)}
    print("smallest pairwise gap of the six kinds at limit state %d: %.3g" % (DISCRIMINATING, min(gaps.values())))
    assert len(gaps) == 15 and min(gaps.values()) > 1e-6, gaps
