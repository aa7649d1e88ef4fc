"""The step and linearisation kernels (k_lin_tangent2 / k_lin_tangent2c, h1_linearize_dev.h, h1_linearize_contact_dev.h, the two-lane step
and stance-constrained step) away from the standing pose: the states of tests/dynamics_envelope_cases.py -- hinges across their ranges,
rotations up to pi, velocities of +-5, non-unit and negated quaternions, controls beyond and on ctrlrange, post-step spins on both sides
of the small-spin Taylor branch and exactly zero, contact modes 1 / 2 under every stance pattern -- against the oracle's forward-mode AD
and step.  Small shapes (16 rollouts, N = 2 or 4: every knot of rollout i carries state i); test_dynamics_envelope_cpu.py shows that these
inputs discriminate and that the oracle is well conditioned on them (two derivations agree to 2.3e-15 max(1, |want|)).

Tolerances are those of the existing tests of the same quantities, scaled by max(1, max |want|) as the contact tests already do: 1e-9
analytic Jacobians, 2e-5 forward differences (eps 1e-5), 1e-8 contact Jacobians, 1e-11 step, 1e-9 stance-constrained step, 1e-12 between
the layouts of one kernel, 2.3e-16 on the position-row structure.  Every test prints the worst error it saw."""
import numpy as np
import pytest

import dynamics_envelope_cases as dc
from test_gpu_configs import _solver, env, rel  # noqa: F401  (env, rel: the helpers of the sibling GPU tests)

pytestmark = pytest.mark.gpu
NS, NX, NU, NQ, H = dc.NS, dc.NX, dc.NU, dc.NQ, dc.H
POS = np.r_[0:3, 7:26]; VEL = np.r_[26:29, 32:51]
E_POS = np.zeros((22, NX)); E_POS[np.arange(22), POS] = 1.0
C_LIN = np.zeros((NX, 3)); C_LIN[0:3] = H * np.eye(3); C_LIN[26:29] = np.eye(3)       # d f / d v_lin = [h I; 0; I; 0]


def _report(title, worst):
    print("%s: worst error relative to max(1, |want|): %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _check(got, want, tol, worst, key, tag):
    scale = max(1.0, np.abs(want).max())
    err = np.abs(got - want).max()
    worst[key] = max(worst.get(key, 0.0), err / scale)
    assert err <= tol * scale, (tag, key, err, scale)           # (a NaN fails this comparison)


def _stage_jacobians(s, x, u):
    """every knot of rollout i carries (x[i], u[i]): (A [B,N,51,51], B [B,N,51,19]) of the stage API (standard layout)"""
    X, U = dc.stage_trajectory(x, u, s.N)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.stage_linearize()
    return s.linearization()


def _check_structure(A, Bm, worst, tag, h=H):
    """what the folded Riccati kernels rely on, exactly: base-linear-velocity columns [h I; 0; I; 0]; position rows e_p + h x velocity row"""
    c_lin = C_LIN.copy(); c_lin[0:3] = h * np.eye(3)
    assert np.array_equal(A[..., 26:29], np.broadcast_to(c_lin, A[..., 26:29].shape)), tag
    e = np.abs(A[..., POS, :] - (E_POS + h * A[..., VEL, :])).max()
    worst["position rows (absolute)"] = max(worst.get("position rows (absolute)", 0.0), e)
    assert e <= 2.3e-16, (tag, e)
    assert np.array_equal(Bm[..., POS, :], h * Bm[..., VEL, :]), tag


@pytest.mark.parametrize("name", dc.FREE_GROUPS)
def test_free_flight_analytic_jacobians_match_oracle_ad(name):
    """spin: besides the matrix bound, the quaternion rows in the hinge and velocity columns are held to 1e-12 max(1, max |want|), the
    bound the layouts of one kernel are held to.  Below the branch threshold the dso term of dE (lin_prologue) moves those entries by at
    most 2 h s / 48 = 8e-10: the matrix bound (2e-8 at |A|max = 17) cannot see whether that term is right.  The rows are
    d q' = qhat (x) (dE d w'): seven multiply-adds with factors below 1 on the three angular rows of d v', and the oracle's two derivations
    agree on them to 1e-14 max(1, max |want|) (test_dynamics_envelope_cpu.py), so 1e-12 leaves two orders over the reference's own spread
    while a wrong sign of the first Taylor coefficient at s = 9.5e-7 exceeds it more than tenfold (shown there as well)."""
    x, u = dc.group(name)
    want_A, want_B = dc.group_ad(name)
    s = _solver(NS, N=2); s.set_problem(dc.problem(2)); s.set_options(jacobian_mode=0)
    A, Bm = _stage_jacobians(s, x, u)
    worst = {}
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(Bm))
    for i in range(NS):
        for t in range(2):
            _check(A[i, t], want_A[i], 1e-9, worst, "A", (name, i, t))
            _check(Bm[i, t], want_B[i], 1e-9, worst, "B", (name, i, t))
            if name == "spin":
                _check(A[i, t][3:7, 7:], want_A[i][3:7, 7:], 1e-12 * max(1.0, np.abs(want_A[i]).max()), worst, "quaternion rows", (i, t))
    _check_structure(A, Bm, worst, name)
    if name == "clamped":
        beyond = dc.clamped()[2]
        for i in range(NS):
            assert np.all(Bm[i][:, :, beyond[i]] == 0.0), i
            assert np.abs(Bm[i][:, :, ~beyond[i]]).max(axis=1).min() > 1e-3, i        # the others, a control ON its limit among them, are live
    if name == "spin":
        xr, ur = dc.rest()                                            # s == 0.0: at rest without torque, zero and physical gravity
        for g in ((0.0, 0.0, 0.0), dc.GRAVITY):
            s.set_problem(dc.problem(2, gravity=g))
            Ar, Br = _stage_jacobians(s, np.tile(xr, (4, 1)), np.tile(ur, (4, 1)))
            wr = dc.oracle_jacobians(xr, ur, gravity=g)
            for i in range(NS):
                for t in range(2):
                    _check(Ar[i, t], wr[0][i % 4], 1e-9, worst, "A at rest", (g, i, t))
                    _check(Br[i, t], wr[1][i % 4], 1e-9, worst, "B at rest", (g, i, t))
    s.close()
    _report("analytic Jacobians, %s" % name, worst)


@pytest.mark.parametrize("name", ["wide", "nonunit"])
def test_free_flight_forward_difference_jacobians_match_oracle(name):
    x, u = dc.group(name)
    want_A, want_B = dc.oracle_jacobians(x, u, jac_mode=1, fd_eps=1e-5)
    s = _solver(NS, N=2); s.set_problem(dc.problem(2)); s.set_options(jacobian_mode=1, fd_eps=1e-5)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    worst = {}
    for i in range(NS):
        for t in range(2):
            _check(A[i, t], want_A[i], 2e-5, worst, "A", (name, i, t))
            _check(Bm[i, t], want_B[i], 2e-5, worst, "B", (name, i, t))
    _report("forward-difference Jacobians, %s" % name, worst)


@pytest.mark.parametrize("mode,variant", [(1, "mid"), (2, "mid"), (1, "nonunit"), (1, "clamped")])
def test_contact_analytic_jacobians_match_oracle_ad(mode, variant):
    """N = 4, one stance pattern per knot: both feet, left only, right only, none (dynamics_envelope_cases.SCHEDULE)"""
    x, u, kept, want_A, want_B, beyond = dc.mid_cases(mode, variant)
    s = _solver(NS, N=4); s.set_problem(dc.problem(4, dc.SCHEDULE)); s.set_contact_mode(mode); s.set_options(jacobian_mode=0)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    worst = {}
    assert kept[:, :3].sum() >= 40
    for i, p in np.argwhere(kept):
        _check(A[i, p], want_A[i, p], 1e-8, worst, "A", (mode, variant, i, p))
        _check(Bm[i, p], want_B[i, p], 1e-8, worst, "B", (mode, variant, i, p))
        assert np.all(Bm[i, p][:, beyond[i]] == 0.0), (i, p)
        if beyond[i].any():
            assert np.abs(Bm[i, p][:, ~beyond[i]]).max(axis=0).min() > 1e-3
    _report("contact Jacobians, mode %d, %s (%d of %d cases kept)" % (mode, variant, kept.sum(), kept.size), worst)


def test_free_flight_step_matches_oracle_on_every_group():
    s = _solver(NS, N=2); s.set_problem(dc.problem(2))
    o = dc.oracle()
    worst = {}
    got = {}
    for name in dc.FREE_GROUPS:
        x, u = dc.group(name)
        got[name] = s.step(x, u)
        for i in range(NS):
            _check(got[name][i], o.step(x[i], u[i]), 1e-11, worst, name, i)
    # A scaled quaternion is the same state.  The step divides by |q| first, so c q and q / |q| round alike in most states but not in all:
    # the oracle itself steps 13 of these 16 to the same bits and 3 to a last-bit neighbour.  Bit-for-bit invariance is therefore no
    # property of the operation; it is demanded of the device only if the oracle has it in every state, else both hold the step tolerance.
    xn, un = dc.group("nonunit")
    gpu_unit = s.step(dc.normalised(xn), un)
    s.close()
    same = same_gpu = 0
    for i in range(NS):
        w_scaled, w_unit = o.step(xn[i], un[i]), o.step(dc.normalised(xn)[i], un[i])
        _check(gpu_unit[i], w_unit, 1e-11, worst, "nonunit, normalised first", i)
        _check(got["nonunit"][i], gpu_unit[i], 1e-11, worst, "nonunit, scaled against normalised on the device", i)
        same += int(np.array_equal(w_scaled, w_unit)); same_gpu += int(np.array_equal(got["nonunit"][i], gpu_unit[i]))
    print("scaled and normalised quaternion step to the same bits in %d of %d states on the oracle, %d on the device" % (same, NS, same_gpu))
    if same == NS:
        assert same_gpu == NS
    _report("step", worst)


@pytest.mark.parametrize("mode", [1, 2])
def test_stance_constrained_step_matches_oracle_on_the_kept_cases(mode):
    x, u, kept = dc.mid_cases(mode)[:3]
    s = _solver(NS, N=2); s.set_problem(dc.problem(2)); s.set_contact_mode(mode)
    o = dc.oracle(mode=mode)
    worst = {}
    for p, (sl, sr) in enumerate(dc.STANCE_ROWS):
        got = s.step_stance(x, u, int(sl), int(sr))
        for i in np.flatnonzero(kept[:, p]):
            _check(got[i], o.step_stance(x[i], u[i], dc.STANCE_ROWS[p]), 1e-9, worst, "stance %d%d" % (sl, sr), i)
    s.close()
    _report("stance-constrained step, mode %d (%d of %d cases kept)" % (mode, kept.sum(), kept.size), worst)


def test_operand_layout_jacobians_inside_a_solve_match_the_stage_api_and_oracle_ad():
    """B = 5, N = 5: 25 knots, so the two-knot kernel has an odd item count and a pair that crosses from one rollout into the next.
    One iteration, no convergence exit: ilqr_capi.hip enqueue_solve linearises once, in iteration 0 (enqueue_region), the nominal trajectory
    -- the cold start's rollout of u_init from x0, which the solve re-rolls to the same bits (solve_order.h rolls_aside) -- and starts no later
    iteration's linearisation (enqueue_sequential_iteration: split_next needs iter + 1 < max_iter); the line search then replaces xbar / ubar by the accepted candidate.  So the Jacobians a
    solve leaves behind (operand layout, converted back by the getter) belong to the trajectory read BEFORE the solve."""
    B = N = 5
    rng = np.random.default_rng(dc.SEED + 3)
    x0 = dc.group("wide")[0][:B].copy()
    x0[:, NQ:] *= 2.0 / 5.0                                          # velocities scaled to +-2
    ui = rng.uniform(-0.9, 0.9, (B, N, NU)) * dc.sc.CTRLRANGE
    prob = dc.problem(N)
    s = _solver(B, N=N); s.set_problem(prob); s.set_max_iterations(1); s.set_options(jacobian_mode=0, early_exit=False)
    s.initialize(x0, ui)
    X0, U0 = s.xbar(), s.ubar()
    assert np.array_equal(X0[:, 0], x0) and np.array_equal(U0, ui) and np.all(np.isfinite(X0))
    s.solve(x0)
    A2, B2 = s.linearization()
    X1, U1 = s.xbar(), s.ubar()
    s.close()
    s = _solver(B, N=N); s.set_problem(prob); s.set_options(jacobian_mode=0)
    s.initialize(x0, ui); s.set_trajectory(X0, U0); s.stage_linearize()
    A1, B1 = s.linearization()
    s.close()
    worst = {"layouts, A (absolute)": np.abs(A2 - A1).max(), "layouts, B (absolute)": np.abs(B2 - B1).max()}
    assert np.abs(A2 - A1).max() <= 1e-12 and np.abs(B2 - B1).max() <= 1e-12, worst
    o = dc.oracle(N=N, jac_mode=0)
    moved = 0
    for b in range(B):
        o.set_trajectory(X0[b], U0[b]); o.linearize()
        wA, wB = o.get("A"), o.get("B")
        for t in range(N):
            _check(A2[b, t], wA[t], 1e-9, worst, "A", (b, t))
            _check(B2[b, t], wB[t], 1e-9, worst, "B", (b, t))
        if not np.array_equal(U1[b], U0[b]):                          # an accepted step: the Jacobians are NOT those of the trajectory left behind
            moved += 1
            o.set_trajectory(X1[b], U1[b]); o.linearize()
            assert np.abs(A2[b] - o.get("A")).max() > 1e-6
    print("line search accepted a step in %d of %d rollouts" % (moved, B))
    _report("operand-layout Jacobians inside a solve", worst)
