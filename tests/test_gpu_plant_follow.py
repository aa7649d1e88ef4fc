"""Following the policy over several knots between solves, on the GPU (include/ilqr_hip.h ilqr_hip_plant_follow, ilqr_hip_initialize_warm_*_shifted,
ilqr_hip_compute_control_at; csrc/plant_kernels.hip k_plant_follow, the k_warm_shift_m / k_warm_tail_* kernels).

The yardstick is never the new kernels: it is the entry points that existed before them, TEACHER-FORCED as in tests/test_gpu_plant.py, with the
tolerances that file takes from the parent commit:
  u       np.allclose(rtol=1e-12, atol=1e-12)
  x_next  1e-11 absolute per plant step, times the substeps
  stance flags and alive: equal for every rollout and every interval.
Where two compositions of the SAME kernels are compared (one interval against the advance, a fused group against its single intervals, a
shift of one against the one-knot warm start) the comparison is bit for bit.

N = 6 and two iterations keep every test at seconds; B = 33 (feedback mode 0: 32 rollouts per wave) and B = 5 (feedback mode 1: 4 per wave)
leave the last workgroup partial."""
import numpy as np
import pytest

from conftest import load_package
from test_gpu_plant import DT, NQ, NU, NV, NX, U_TOL, X_TOL_PER_STEP, _geometry_states, _pair, _sv

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
N, ITERS, M = 6, 2, 3
BATCH = {0: 33, 1: 5}      # by feedback mode


def _problem(B, seed, per_rollout_schedule=False):
    """standing problem; per_rollout_schedule: a stance set per rollout whose rows differ from knot to knot and from rollout to rollout"""
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
    x0, ui = sc.synthetic_batch(B, N, seed, ug)
    if per_rollout_schedule:
        pattern = np.array([(1, 1), (1, 0), (0, 1), (1, 1), (0, 1), (1, 0), (1, 1)], dtype=np.int32)
        prob["stance"] = np.ascontiguousarray(pattern[(np.arange(B)[:, None] + np.arange(N + 1)[None, :]) % len(pattern)])
        assert all((prob["stance"][:, t] != prob["stance"][:, t + 1]).any() for t in range(N))
    return prob, x0, ui


def _solved(B, prob, x0, ui, substeps=1, fb=0, mode=0, source="schedule", limits=False, mu=None, ring=M, xp=None):
    """a handle that has solved `prob` from x0 and carries the plant at xp (default x0); two calls give twins"""
    sv = _sv()
    A = sv.BatchedILQR(B, N=N, dt=DT)
    A.set_contact_mode(mode)
    if mu is not None:
        A.set_friction(mu)
    if limits:
        A.set_joint_limits(True)
    A.set_max_iterations(ITERS)
    A.plant_configure(substeps, fb, source)
    A.plant_set_history(ring)
    A.set_problem(prob); A.initialize(x0, ui); A.solve(x0)
    A.plant_reset(x0 if xp is None else xp)
    return A


def _plant(A):
    return A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("fb", [0, 1])
def test_one_interval_is_the_advance(mode, fb):
    B = BATCH[fb]
    prob, x0, ui = _problem(B, 11, per_rollout_schedule=bool(mode))
    A, T = (_solved(B, prob, x0, ui, substeps=2, fb=fb, mode=mode) for _ in range(2))
    dv = np.zeros((B, NV)); dv[:, 1] = 0.3
    A.plant_kick(dv); T.plant_kick(dv)
    A.plant_follow(0, 1); T.plant_advance()
    assert _same(_plant(A), _plant(T)) and _same(A.plant_history(), T.plant_history())
    assert not np.array_equal(A.plant_state(), x0) and A.plant_history()[0].shape == (1, B, NX)
    A.plant_follow(0, 1); T.plant_advance()      # the kick is gone, the ring has a second row
    assert _same(_plant(A), _plant(T)) and _same(A.plant_history(), T.plant_history())
    A.close(); T.close()


@pytest.mark.parametrize("substeps,fb,ring", [(1, 0, M), (4, 0, 2), (1, 1, 2), (4, 1, M)])
def test_fusing_changes_nothing(substeps, fb, ring):
    """plant_follow(0, m) against plant_follow(j, 1), j = 0..m-1; with a ring of two rows it wraps inside the launch"""
    B = BATCH[fb]
    prob, x0, ui = _problem(B, 12, per_rollout_schedule=True)
    A, T = (_solved(B, prob, x0, ui, substeps=substeps, fb=fb, mode=2, ring=ring) for _ in range(2))
    A.plant_follow(0, M)
    singles = []
    for j in range(M):
        T.plant_follow(j, 1)
        singles.append(T.plant_state())
    assert _same(_plant(A), _plant(T))
    (ax, au), (tx, tu) = A.plant_history(), T.plant_history()
    assert ax.shape == (min(ring, M), B, NX) and np.array_equal(ax, tx) and np.array_equal(au, tu)
    assert np.array_equal(ax[-1], singles[-2])      # the newest row is the state the last interval started from
    assert not np.array_equal(singles[0], singles[1]) and np.all(A.plant_alive() == 1)
    A.close(); T.close()


def _control_law(A, x, knot):
    """u = ubar_k + K_k (x - xbar_k) in NumPy from the getters; a non-finite u becomes zero"""
    u = A.ubar()[:, knot] + np.einsum("bij,bj->bi", A.gains_K()[:, knot], x - A.xbar()[:, knot])
    u[~np.isfinite(u).all(axis=1)] = 0.0
    return u


def _host_interval(A, P, x, knot, substeps, fb, source, mode, flags):
    """what interval `knot` has to produce from the state x: (x_next, u reported, stance)"""
    xc, u, st = x.copy(), None, np.asarray(flags, dtype=np.int32).copy()
    for k in range(substeps):
        if k == 0 or fb:
            u = _control_law(A, xc, knot)
        if mode and source == "geometry":
            xc, st = P.step_geometry(xc, u)
        elif mode:
            xn = np.empty_like(xc)
            for l, r in {(int(a), int(b)) for a, b in flags}:
                idx = np.where((flags[:, 0] == l) & (flags[:, 1] == r))[0]
                xn[idx] = P.step_stance(xc[idx], u[idx], l, r)
            xc = xn
        else:
            xc = P.step(xc, u)
    return xc, u, st


def _check_against_host(B, prob, x0, ui, substeps, fb, mode=0, source="schedule", limits=False, mu=None):
    A, T = (_solved(B, prob, x0, ui, substeps=substeps, fb=fb, mode=mode, source=source, limits=limits, mu=mu) for _ in range(2))
    _, P = _pair(B, N, substeps, mode=mode, limits=limits, mu=mu)
    P.set_problem(prob)
    A.plant_follow(0, M)
    hx, hu = A.plant_history()
    states = list(hx) + [A.plant_state()]
    assert hx.shape == (M, B, NX) and np.array_equal(hx[0], x0)
    sched = prob["stance"] if prob["stance"].shape[0] > 1 else np.repeat(prob["stance"], B, axis=0)
    seen = []
    for j in range(M):
        want_x, want_u, want_st = _host_interval(A, P, states[j], j, substeps, fb, source, mode, sched[:, j])
        T.plant_follow(j, 1)      # the stance flags of interval j (the fused launch reports the last interval's; fusing changes nothing, above)
        err = np.abs(states[j + 1] - want_x).max()
        print("interval %d: |dx| %.3e  |du| %.3e" % (j, err, np.abs(hu[j] - want_u).max()))
        assert np.allclose(hu[j], want_u, **U_TOL), (j, np.abs(hu[j] - want_u).max())
        assert err < X_TOL_PER_STEP * substeps, (j, err)
        if mode:
            assert np.array_equal(T.plant_stance(), want_st), j
        seen.append(want_st)
    assert np.array_equal(A.plant_stance(), T.plant_stance()) and np.all(A.plant_alive() == 1) and np.array_equal(A.plant_control(), hu[-1])
    A.close(); T.close(); P.close()
    return np.array(seen)


@pytest.mark.parametrize("substeps,fb", [(1, 0), (4, 0), (1, 1), (4, 1)])
def test_each_interval_is_the_host_composition_free_plant(substeps, fb):
    B = BATCH[fb]
    _check_against_host(B, *_problem(B, 13), substeps, fb)


@pytest.mark.parametrize("substeps,fb", [(2, 0), (2, 1)])
def test_each_interval_is_the_host_composition_contact_mode_2(substeps, fb):
    """the schedule rows differ over the first m knots and between rollouts: a wrong row index or set stride fails"""
    B = BATCH[fb]
    flags = _check_against_host(B, *_problem(B, 14, per_rollout_schedule=True), substeps, fb, mode=2)
    assert (flags[0] != flags[1]).any() and (flags[1] != flags[2]).any()


@pytest.mark.parametrize("substeps,fb", [(2, 0), (2, 1)])
def test_each_interval_is_the_host_composition_mode_3_on_geometry_with_joint_limit_rows(substeps, fb):
    sv = _sv()
    B = BATCH[fb]
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    _, P = _pair(B, N, substeps, mode=3, limits=True, mu=0.3)
    xs = _geometry_states(P, 33, np.random.default_rng(14))
    order = np.argsort(P.step_geometry(xs, np.zeros((len(xs), NU)))[1].sum(axis=1), kind="stable")      # feet in the air first
    x0 = xs[np.concatenate([order[:B // 2], order[::-1][:B - B // 2]])]                                  # ... and both kinds in a small batch
    P.close()
    ui = np.tile(sv.gravity_compensation(sc.standing_state(), prob["gravity"]), (B, N, 1))
    flags = _check_against_host(B, prob, x0, ui, substeps, fb, mode=3, source="geometry", limits=True, mu=0.3)
    assert 0 < flags.sum() < flags.size      # feet on the floor and feet in the air both occur


def test_compute_control_at_a_knot():
    B = 5
    prob, x0, ui = _problem(B, 15)
    A = _solved(B, prob, x0, ui)
    x = x0 + np.random.default_rng(1).uniform(-1e-2, 1e-2, size=x0.shape)
    for knot in (0, 1, N - 1):
        got, want = A.compute_control(x, knot=knot), _control_law(A, x, knot)
        assert np.allclose(got, want, **U_TOL), (knot, np.abs(got - want).max())
    assert not np.allclose(A.compute_control(x, knot=1), A.compute_control(x, knot=0), **U_TOL)      # the knots differ
    import ctypes as C
    u_at = np.zeros((B, NU))      # the new entry point itself at knot 0 (the wrapper calls the one-knot symbol there)
    A._chk(A.L.ilqr_hip_compute_control_at(A.h, 0, x.ctypes.data_as(C.POINTER(C.c_double)), u_at.ctypes.data_as(C.POINTER(C.c_double))))
    assert np.array_equal(u_at, A.compute_control(x))
    A.close()


@pytest.mark.parametrize("mode", [0, 2])
def test_warm_start_by_m(mode):
    """mode 0: the unconstrained family of the tail kernel; mode 2: the two-lane family, on a schedule whose last three rows differ"""
    B, sh = 5, 3
    prob, x0, ui = _problem(B, 16, per_rollout_schedule=bool(mode))
    A, T = (_solved(B, prob, x0, ui, mode=mode) for _ in range(2))
    _, P = _pair(B, N, 1, mode=mode)
    P.set_problem(prob)
    for s in (A, T):
        s.plant_follow(0, sh)
    xp, pxb, pub = A.plant_state(), A.xbar(), A.ubar()
    # a shift of one: the new entry point against the one-knot warm start
    A._chk(A.L.ilqr_hip_initialize_warm_from_plant_shifted(A.h, 1)); T.initialize_warm_from_plant()
    assert np.array_equal(A.xbar(), T.xbar()) and np.array_equal(A.ubar(), T.ubar())
    A.initialize_warm_from_plant(shift=1)      # (the wrapper's default path, on the already shifted solution)
    T.initialize_warm_from_plant()
    assert np.array_equal(A.xbar(), T.xbar()) and np.array_equal(A.ubar(), T.ubar())
    # a shift of three
    for s in (A, T):
        s.set_trajectory(pxb, pub)
    A.initialize_warm_from_plant(shift=sh)
    xb, ub = A.xbar(), A.ubar()
    assert np.array_equal(xb[:, 0], xp) and np.array_equal(xb[:, 1:N - sh + 1], pxb[:, 1 + sh:N + 1])
    assert np.array_equal(ub, pub[:, np.minimum(np.arange(N) + sh, N - 1)])
    sched = prob["stance"] if prob["stance"].shape[0] > 1 else np.repeat(prob["stance"], B, axis=0)
    for t in range(N - sh, N):
        if mode:
            want = np.empty((B, NX))
            for l, r in {(int(a), int(b)) for a, b in sched[:, t]}:
                idx = np.where((sched[:, t, 0] == l) & (sched[:, t, 1] == r))[0]
                want[idx] = P.step_stance(xb[idx, t], ub[idx, t], l, r)
        else:
            want = P.step(xb[:, t], ub[:, t])
        err = np.abs(xb[:, t + 1] - want).max()
        print("re-rolled knot %d: |dx| %.3e" % (t + 1, err))
        assert err < X_TOL_PER_STEP, (t, err)
    assert not np.array_equal(xb[:, N - sh + 1:], pxb[:, N - sh + 1:])
    if mode:
        assert all((sched[:, t] != sched[:, t + 1]).any() for t in range(N - sh, N - 1))
    # x0 from the host: the same kernels
    T.initialize_warm_resident(xp, shift=sh)
    assert np.array_equal(T.xbar(), xb) and np.array_equal(T.ubar(), ub)
    A.close(); T.close(); P.close()


def _rate_that_fails_in_the_second_interval(prob, x0, ui, col, fb, substeps):
    """A hinge rate whose velocity products stay finite in the first interval and overflow in the second: arithmetic only, nothing that
    faults the device.  The velocity terms of the dynamics square the rate per step, so between "finite for good" and "non-finite at once"
    lies a band of rates that fail in the second interval; where it lies depends on the step's arithmetic, so it is looked up here with
    single intervals, one candidate per rollout of a scout handle that solves what the tested rollout solves (rollouts are independent)."""
    rates = 10.0 ** np.arange(2.0, 30.5, 0.5)
    xs, us = np.tile(x0, (len(rates), 1)), np.tile(ui, (len(rates), 1, 1))
    xp = xs.copy(); xp[:, col] = rates
    A = _solved(len(rates), prob, xs, us, substeps=substeps, fb=fb, xp=xp)
    alive = []
    for j in range(M):
        A.plant_follow(j, 1)
        alive.append(A.plant_alive())
    A.close()
    alive = np.array(alive).T
    hit = np.where((alive == [1, 0, 0]).all(axis=1))[0]
    print("alive after each interval, by rate:", {"%.1e" % r: a.tolist() for r, a in zip(rates, alive)})
    assert len(hit) > 0, "no candidate rate fails in the second interval"
    return rates[hit[len(hit) // 2]]


def test_non_finite_state_in_the_middle_of_a_group():
    B, bad, fb, substeps = 5, 2, 1, 1
    prob, x0, ui = _problem(B, 17)
    col = NQ + 6 + 3
    xp = x0.copy(); xp[bad, col] = _rate_that_fails_in_the_second_interval(prob, x0[bad], ui[bad], col, fb, substeps)
    F = _solved(B, prob, x0, ui, substeps=substeps, fb=fb, xp=xp)      # fused
    S = _solved(B, prob, x0, ui, substeps=substeps, fb=fb, xp=xp)      # the same three intervals, one launch each
    C = _solved(B, prob, x0, ui, substeps=substeps, fb=fb)             # unpoisoned, fused
    F.plant_follow(0, M); C.plant_follow(0, M)
    alive, xs = [], []
    for j in range(M):
        S.plant_follow(j, 1)
        alive.append(S.plant_alive()); xs.append(S.plant_state())
    print("alive of the poisoned rollout after each interval:", [int(a[bad]) for a in alive])
    assert [int(a[bad]) for a in alive] == [1, 0, 0]      # it fails in the second interval of three
    assert _same(_plant(F), _plant(S)) and _same(F.plant_history(), S.plant_history())
    fx, fu, _, fa = _plant(F)
    hx, hu = F.plant_history()
    assert fa[bad] == 0 and np.all(fu[bad] == 0.0) and np.array_equal(fx[bad], xs[0][bad]) and np.all(np.isfinite(fx[bad]))      # frozen where interval 1 left it
    assert np.array_equal(hx[1, bad], fx[bad]) and np.array_equal(hx[2, bad], fx[bad]) and np.array_equal(hx[0, bad], xp[bad])
    assert np.all(hu[1:, bad] == 0.0) and np.any(hu[0, bad] != 0.0)
    keep = np.arange(B) != bad
    cx, cu, cs, ca = _plant(C)
    chx, chu = C.plant_history()
    assert np.all(fa[keep] == 1) and np.all(ca == 1)
    assert np.array_equal(fx[keep], cx[keep]) and np.array_equal(fu[keep], cu[keep]) and np.array_equal(hx[:, keep], chx[:, keep]) and np.array_equal(hu[:, keep], chu[:, keep])
    F.close(); S.close(); C.close()


def test_runner_solves_every_third_interval_on_both_paths():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    B, steps = 4, 6
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (40, 1))); rd.contact = np.ones((40, 2), dtype=np.int32)
    ug = sv.gravity_compensation(sc.standing_state(), base["gravity"])
    x0, ui = sc.synthetic_batch(B, N, 0, ug)
    res, solves = {}, {}
    for resident in (False, True):
        s = sv.BatchedILQR(B, N=N, dt=DT); s.set_max_iterations(ITERS); s.set_contact_mode(2)
        run = ml.MPCRunner(s, rd, base, resident=resident, solve_every=M)
        res[resident] = run.run(x0, steps, u_init=ui)
        solves[resident] = len(run.prof["MPC_iLQR_solve"])
        assert run.t_idx == steps
        run.close(); s.close()
    assert solves == {False: 2, True: 2}
    assert res[True][0].shape == res[False][0].shape == (steps + 1, B, NX) and np.all(np.isfinite(res[True][0]))
    assert np.array_equal(res[True][0][0], res[False][0][0])
    # the two paths see the same policy until the second solve, whose x0 already differs by the plant steps' rounding: per-step tolerance,
    # accumulated over the intervals taken so far as in test_runner_resident_and_host_visit_the_same_first_state (its one step: 1e-11)
    for k in range(1, steps + 1):
        err = np.abs(res[True][0][k] - res[False][0][k]).max()
        print("state %d, resident vs host: %.3e" % (k, err))
        assert err < X_TOL_PER_STEP * k, (k, err)
    assert np.allclose(res[True][1][0], res[False][1][0], **U_TOL)
