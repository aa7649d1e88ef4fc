"""Noisy and biased state observation per rollout on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_observation; csrc/plant_kernels.hip
k_observation_draw, k_observe_apply, k_plant_follow_o of the module libilqr_hip_observe.so).

Ground truth in two layers, neither of them the new kernels:
  * the draws against the golden of the NumPy restatement (tests/observation_cases.py, tests/golden/gen_observation_golden.py), which is
    held to the published Philox4x32-10 vectors on the CPU;
  * the plant kernels against the TEACHER-FORCED composition of entry points that existed before: the host forms x [+] delta from the
    downloaded error rows, calls compute_control at the interval's knot and steps with step / step_stance (tests/plant_params_cases.py
    Yardstick; with every table installed step_payload, tests/test_gpu_payload.py PayloadYardstick) in the plant's mode.
B = 37 (two workgroups at feedback mode 0, ten at mode 1, the last one not full), N = 6, SUBSTEPS = 2, as tests/test_gpu_plant_params.py.

Bounds.  Draws: 1e-13 absolute for |bias|, sigma <= 1 -- the integer part is exact, the arguments of log and cos / sin are bit-identical on
both sides, a few ulp of libm difference at r <= 8.7 stay below 1e-14, a factor ten of margin.  x [+] delta against the host: 1e-15
relative to max(1, |want|) (four products of magnitude <= 1, fused on the device).  Plant: reported u U_TOL (1e-12), state cc.STEP_TOL x
SUBSTEPS relative, as tests/test_gpu_plant_params.py."""
import numpy as np
import pytest

import dynamics_envelope_cases as dc
import observation_cases as oc
import plant_params_cases as pc
import plant_score_ref as ps
from conftest import load_package
from test_gpu_payload import NO_PAYLOAD, NO_WRENCH, PayloadYardstick, _payload_table
from test_gpu_plant import U_TOL
from test_gpu_plant_params import CASES, _problem, _solver, _state_error, _states
from test_gpu_wrench import OWN, _same, _snapshot, _wrench_table

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU = 51, 19
B, N, DT, SUBSTEPS = pc.B, pc.N, pc.DT, pc.SUBSTEPS
DRAW_TOL = 1e-13
SEED = 0xC0FFEE12345


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


IDENTITY = oc.error_rows(np.zeros((B, 50)))


# ---- 1: the draws
def test_draws_match_the_golden_and_do_not_depend_on_split_grouping_or_call():
    sv = _sv()
    g = oc.golden()
    rec, seed, count = g["records"], int(g["seed"]), int(g["count"])
    assert rec.shape[0] == B and count == N and np.abs(rec).max() <= 1.0
    A = _solver(0, False)
    assert A.plant_num_observation_sets() == 0
    none, s0, s1 = A.plant_get_observation()
    assert np.array_equal(none, np.zeros((B, 100))) and (s0, s1) == (0, 0)
    A.plant_set_observation(rec, seed=seed, stream0=0)
    back, s0, s1 = A.plant_get_observation()
    assert A.plant_num_observation_sets() == B and np.array_equal(back, rec) and (s0, s1) == (seed, 0)
    got = A.plant_observation_errors(0, count)
    err = float(np.abs(got - g["delta"]).max())
    print("draws against the golden: worst |error| %.3e (bound %.0e), largest |delta| %.2f" % (err, DRAW_TOL, np.abs(got).max()))
    assert got.shape == (count, B, NX) and err < DRAW_TOL
    zero = np.arange(B) % 4 == 3
    assert np.array_equal(got[:, zero], np.broadcast_to(IDENTITY[0], got[:, zero].shape))                  # a zero record: exactly the identity, whatever was drawn
    assert np.array_equal(A.plant_observation_errors(0, count), got)                                       # a second call: the same bits
    assert np.array_equal(A.plant_observation_errors(2, 3), got[2:5]) and np.array_equal(A.plant_observation_errors(5, 1), got[5:])      # call grouping
    # a batch of 37 with stream0 = 0 is handles of 20 and 17 with stream0 = 0 and 20
    for lo, hi in ((0, 20), (20, B)):
        P = sv.BatchedILQR(hi - lo, N=N, dt=DT)
        P.plant_set_observation(rec[lo:hi], seed=seed, stream0=lo)
        assert np.array_equal(P.plant_observation_errors(0, count), got[:, lo:hi]), (lo, hi)
        P.close()
    # B identical records are one record; the streams still differ per rollout
    A.plant_set_observation(np.repeat(rec[:1], B, axis=0), seed=seed)
    many = A.plant_observation_errors(0, count)
    A.plant_set_observation(rec[:1], seed=seed)
    assert A.plant_num_observation_sets() == 1 and np.array_equal(A.plant_get_observation()[0], np.repeat(rec[:1], B, axis=0))
    one = A.plant_observation_errors(0, count)
    assert np.array_equal(one, many) and np.array_equal(one[:, 0], got[:, 0]) and not np.array_equal(one[:, 1], one[:, 0])
    # another seed, another stream0: other draws; a 64-bit seed and stream reach the generator whole
    A.plant_set_observation(rec[:1], seed=seed ^ (1 << 40))
    assert not np.array_equal(A.plant_observation_errors(0, 1), one[:1])
    A.plant_set_observation(rec[:1], seed=seed, stream0=1 << 33)
    hi = A.plant_observation_errors(0, 1)
    assert not np.array_equal(hi, one[:1]) and np.abs(hi - oc.errors(rec[:1], seed, 1 << 33, 0, 1, B=B)).max() < DRAW_TOL
    A.close()


# ---- 2: one measurement for the solver and the law
def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


@pytest.mark.parametrize("shift", [1, 2])
def test_warm_start_and_control_law_read_the_same_measurement(shift):
    A = _solver(0, False, fb=0, ring=4)
    x0, ui = _states("mid")
    A.initialize(x0, ui); A.solve(x0)
    A.plant_reset(x0)
    assert np.array_equal(A.plant_get_observed(), x0)                                                      # without a table: the plant's state
    A.plant_set_observation(oc.plant_records(B), seed=SEED)
    A.plant_follow(0, shift)
    i = A.plant_intervals()
    assert i == shift
    x_true = A.plant_state()
    x_obs = A.plant_get_observed()
    want = oc.boxplus(x_true, A.plant_observation_errors(i, 1)[0])
    err = _rel(x_obs, want)
    print("shift %d: x [+] delta against the host %.3e (bound 1e-15); moved %d rollouts" % (shift, err, (np.abs(x_obs - x_true).max(axis=1) > 1e-6).sum()))
    assert err <= 1e-15 and (np.abs(x_obs - x_true).max(axis=1) > 1e-6).sum() >= B // 2
    assert np.array_equal(x_obs[np.arange(B) % 3 == 2], x_true[np.arange(B) % 3 == 2])                     # zero records see the truth
    A.initialize_warm_from_plant(shift=shift)
    assert np.array_equal(A.xbar()[:, 0], x_obs)                                                           # the solve starts from the measurement, bit for bit
    assert np.array_equal(A.plant_state(), x_true)                                                         # ... and the plant keeps the truth
    A.solve(None)
    assert np.array_equal(A.xbar()[:, 0], x_obs)
    ub0 = A.ubar()[:, 0]
    assert np.all(np.isfinite(ub0)) and np.all(np.isfinite(A.gains_K()))
    A.plant_advance()                                                                                      # feedback mode 0, no kick: x_obs - xbar_0 is exactly zero
    assert np.array_equal(A.plant_control(), ub0) and np.all(A.plant_alive() == 1)
    A.close()


# ---- 3: the plant against the teacher-forced composition
def _advance_o(A, step, delta, x, fb, knot=0):
    """one MPC interval whose control law reads x [+] delta: (x_next, reported u, stance); step(x, u) -> (x_next, stance) is the plant's step"""
    xc, u, st = x.copy(), None, None
    for k in range(SUBSTEPS):
        if k == 0 or fb:
            u = A.compute_control(oc.boxplus(xc, delta), knot=knot)
            u[~np.isfinite(u).all(axis=1)] = 0.0
        xc, st = step(xc, u)
    return xc, u, st


def _every_workgroup(moved, fb, tag):
    rpw = 4 if fb else 32
    per = [int(moved[k:k + rpw].sum()) for k in range(0, B, rpw)]
    print("%s: the table moves the control of %d rollouts, per workgroup %s" % (tag, int(moved.sum()), per))
    assert moved.sum() >= 4 and min(per) >= 1, (tag, per)


def _check_interval(tag, Y, group, got_x, got_u, got_st, want):
    want_x, want_u, want_st = want
    err, bound = _state_error(got_x, want_x, group)
    du = float(np.abs(got_u - want_u).max())
    print("%s: state error %.3e (bound %.1e)  |du| %.3e" % (tag, err, bound, du))
    assert np.all(np.isfinite(want_x)), tag
    assert np.allclose(got_u, want_u, **U_TOL), (tag, du)
    assert err < bound, (tag, err)
    if Y.mode and got_st is not None:
        assert np.array_equal(got_st, want_st), tag
    return err


def _teacher_forced_o(A, Y, step, x0, fb, group, tag):
    """one advance, then -- from the reset -- a follow(0, 3), each interval held to the yardstick from the state it started from"""
    A.plant_reset(x0)
    delta = A.plant_observation_errors(0, 3)
    # on the yardstick alone: the table moves the control
    u_obs, u_true = (_advance_o(A, step, d, x0, fb)[1] for d in (delta[0], IDENTITY))
    _every_workgroup(np.abs(u_obs - u_true).max(axis=1) > 1e-6, fb, tag)
    A.plant_advance()
    worst = _check_interval(tag + " advance", Y, group, A.plant_state(), A.plant_control(), A.plant_stance(), _advance_o(A, step, delta[0], x0, fb))
    assert np.all(A.plant_alive() == 1) and A.plant_intervals() == 1
    A.plant_reset(x0)
    A.plant_follow(0, 3)
    hx, hu = A.plant_history()
    assert hx.shape == (3, B, NX) and np.array_equal(hx[0], x0) and np.all(A.plant_alive() == 1) and A.plant_intervals() == 3
    ends = [hx[1], hx[2], A.plant_state()]
    for j in range(3):
        st = A.plant_stance() if j == 2 else None
        worst = max(worst, _check_interval("%s follow interval %d" % (tag, j), Y, group, ends[j], hu[j], st, _advance_o(A, step, delta[j], hx[j], fb, knot=j)))
    assert np.array_equal(A.plant_control(), hu[2])
    return worst


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", ["free", "mode3_sliding", "mode4_limits"])
def test_plant_under_an_observation_table_matches_the_host_composition(case, fb):
    mode, limits, source, group = CASES[case]
    sv = _sv()
    A = _solver(mode, limits, source=source, fb=fb, ring=3)
    Y = pc.Yardstick(sv, sc, mode, limits, source)
    x0, ui = _states(group, Y.handle(pc.SETS[0]))
    flags = pc.schedule()[:, 0]
    A.initialize(x0, ui); A.solve(x0)
    assert np.all(np.isfinite(A.ubar())) and np.all(np.isfinite(A.gains_K()))
    A.plant_set_observation(oc.plant_records(B), seed=SEED)
    worst = _teacher_forced_o(A, Y, lambda x, u: Y.step(OWN, x, u, flags), x0, fb, group, "%s fb%d" % (case, fb))
    print("%s fb%d: worst state error under the observation table %.3e" % (case, fb, worst))
    A.close(); Y.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_parameter_wrench_payload_and_observation_tables_together(fb):
    mode, limits, source, group = CASES["mode4_limits"]
    sv = _sv()
    A = _solver(mode, limits, fb=fb, ring=3)
    Y = PayloadYardstick(sv, sc, mode, limits, source)
    x0, ui = _states(group)
    flags = pc.schedule()[:, 0]
    A.initialize(x0, ui); A.solve(x0)
    table, payload = pc.params(), _payload_table()
    wrench = _wrench_table(); wrench[:, 9] = 1.0; wrench[:, 10] = np.inf                                   # every window opens at interval 1
    A.plant_set_params(table); A.plant_set_wrench(wrench); A.plant_set_payload(payload)
    A.plant_set_observation(oc.plant_records(B), seed=SEED)
    A.plant_reset(x0)
    delta = A.plant_observation_errors(0, 3)

    def want(j, x, knot):
        w9 = np.where(((wrench[:, 9] <= j) & (j < wrench[:, 10]))[:, None], wrench[:, :9], 0.0)
        return _advance_o(A, lambda xc, u: Y.step_m(table, xc, u, flags, w9, payload), delta[j], x, fb, knot=knot)      # (the gain on the host, inside step_m)

    tag = "all tables fb%d" % fb
    A.plant_advance()
    _check_interval(tag + " advance", Y, group, A.plant_state(), A.plant_control(), A.plant_stance(), want(0, x0, 0))
    A.plant_reset(x0); A.plant_follow(0, 3)
    hx, hu = A.plant_history()
    ends = [hx[1], hx[2], A.plant_state()]
    for j in range(3):
        _check_interval("%s follow interval %d" % (tag, j), Y, group, ends[j], hu[j], A.plant_stance() if j == 2 else None, want(j, hx[j], j))
    assert np.all(A.plant_alive() == 1)
    # the wrench and the payload act beside the observation: each alone moves the plant
    pushed = want(1, hx[1], 1)[0]
    w_off = _advance_o(A, lambda xc, u: Y.step_m(table, xc, u, flags, NO_WRENCH[:, :9], payload), delta[1], hx[1], fb, knot=1)[0]
    m_off = _advance_o(A, lambda xc, u: Y.step_m(table, xc, u, flags, np.where((wrench[:, 9] <= 1)[:, None], wrench[:, :9], 0.0), NO_PAYLOAD), delta[1], hx[1], fb, knot=1)[0]
    assert (np.abs(pushed - w_off).max(axis=1) > 1e-6).sum() >= 4 and (np.abs(pushed - m_off).max(axis=1) > 1e-6).sum() >= 4
    A.close(); Y.close()


# ---- 4: bit for bit
SCORE = dict(R=0.05 + 0.01 * np.arange(NU), upright=7.0, balance=11.0, joint_limits=900.0, control_limits=1300.0)


def _run(A, x0, calls="advance_follow"):
    A.plant_reset(x0)
    if calls == "advance_follow":
        A.plant_advance(); A.plant_follow(1, 2)
    elif calls == "fused":
        A.plant_follow(0, 3)
    else:
        for j in range(3):
            A.plant_follow(j, 1)
    return _snapshot(A)


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("mode,group", [(0, "mid"), (2, "sliding")])
def test_a_table_of_zeros_is_no_table(mode, group, fb):
    Q, _, _ = sc.build_cost_matrices()
    x0, ui = _states(group)
    A = _solver(mode, False, fb=fb, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_set_score(Q=0.37 * Q + 1.0, **SCORE)
    none = _run(A, x0); none_score = A.plant_score()
    A.plant_set_observation(np.zeros((1, 100)), seed=SEED)
    assert np.array_equal(A.plant_get_observed(), A.plant_state())
    zero = _run(A, x0); zero_score = A.plant_score()
    assert np.all(none[3] == 1) and none[4].shape == (3, B, NX)
    for name, p, q in zip(("state", "control", "stance", "alive", "ring x", "ring u"), none, zero):
        assert np.array_equal(p, q), (name, float(np.abs(np.asarray(p, dtype=np.float64) - q).max()))
    assert np.array_equal(none_score, zero_score)
    # ... per rollout as well, and the warm start hands the solve the plant's state
    A.plant_set_observation(np.zeros((B, 100)), seed=SEED + 1)
    assert _same(none, _run(A, x0)) and np.array_equal(A.plant_score(), none_score)
    A.initialize_warm_from_plant()
    assert np.array_equal(A.xbar()[:, 0], A.plant_state())
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_equivalences_of_the_observation_table(fb):
    mode, limits, source, group = CASES["mode4_limits"]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    none = _run(A, x0, "fused")
    rec = oc.plant_records(B)
    A.plant_set_observation(rec, seed=SEED)
    fused = _run(A, x0, "fused")
    split = _run(A, x0, "split")
    assert A.plant_intervals() == 3 and _same(fused, split) and np.all(fused[3] == 1)                      # follow(0, 3) is three follow(j, 1)
    assert _same(fused, _run(A, x0, "fused"))                                                              # plant_reset and the same calls: the same run
    assert (np.abs(fused[0] - none[0]).max(axis=1) > 1e-6).sum() >= 4                                       # ... and not the run without a table
    # the table survives plant_reset and plant_configure
    A.plant_configure(SUBSTEPS, fb, "schedule")
    assert A.plant_num_observation_sets() == B and _same(fused, _run(A, x0, "fused"))
    # another seed: another run (the rollouts that see the truth excepted)
    A.plant_set_observation(rec, seed=SEED + 1)
    other = _run(A, x0, "fused")
    noisy = np.arange(B) % 3 != 2
    assert (np.abs(other[0] - fused[0]).max(axis=1)[noisy] > 0).sum() >= 4 and np.array_equal(other[0][~noisy], none[0][~noisy])
    # clear: the results without a table, bit for bit
    A.plant_clear_observation()
    assert A.plant_num_observation_sets() == 0 and _same(none, _run(A, x0, "fused"))
    A.plant_clear_observation()                                                                            # (clearing nothing is fine)
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_a_non_finite_rollout_freezes_alone_under_the_observation_table(fb):
    bad = 33                                                                                               # in the second workgroup at feedback mode 0
    x0, ui = _states("mid")
    out = {}
    for poisoned in (False, True):
        A = _solver(0, False, fb=fb, ring=2)
        A.initialize(x0, ui); A.solve(x0)
        A.plant_set_observation(oc.plant_records(B), seed=SEED)
        xp = x0.copy()
        if poisoned:
            xp[bad, 9] = np.nan
        A.plant_reset(xp); A.plant_follow(0, 2)
        out[poisoned] = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        A.close()
    x, u, st, alive = out[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(u[bad] == 0.0) and np.array_equal(x[bad], np.where(np.arange(NX) == 9, np.nan, x0[bad]), equal_nan=True)
    assert np.all(alive[keep] == 1) and np.all(out[False][3] == 1)
    assert np.array_equal(x[keep], out[False][0][keep]) and np.array_equal(u[keep], out[False][1][keep])      # bit for bit


# ---- 5: the ruler stays on the truth
def test_score_under_an_observation_table_is_the_score_of_the_true_states():
    Q, _, _ = sc.build_cost_matrices()
    score = dict(Q=0.37 * Q + 1.0, **SCORE)
    x0, ui = _states("limits")
    A = _solver(4, True, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_set_observation(oc.plant_records(B), seed=SEED)
    A.plant_set_score(**score)
    A.plant_reset(x0)
    A.plant_advance(); A.plant_follow(1, 2)
    got = A.plant_score()
    hx, hu = A.plant_history()
    assert np.array_equal(hx[0], x0)                                                                       # the ring holds the true state, not the measurement
    prob = _problem()
    want = ps.expected_record(ps.IntervalOracle(DT), [(prob, k) for k in range(3)], hx, hu, score)
    ok, worst = ps.close_enough(got, want)
    print("score under an observation table: worst |got - want| / bound = %.3f" % worst)
    assert ok.all() and np.array_equal(got[:, 6:], want[:, 6:])
    A.close()


# ---- 6: the runner
def test_runner_biased_pelvis_position_moves_the_closed_loop():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, Nn, steps = 4, 25, 6
    base = sc.make_problem(sv.reference_kinematics, N=Nn, gravity=dc.GRAVITY)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(Bn, Nn, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    biased = np.array([False, False, True, True])
    table = sc.stack_plant_observation(Bn, position_bias=np.outer(biased, (0.01, 0.0, 0.0)))
    res = {}
    for tab in (False, True):
        # (contact mode 2, as the runner test of tests/test_gpu_plant.py: a standing robot needs its feet -- the constraint-free solve of this
        # scenario returns a non-finite cost and keeps its initial guess, with or without a table, so nothing the solve is told could show)
        s = sv.BatchedILQR(Bn, N=Nn, dt=DT); s.set_max_iterations(2); s.set_contact_mode(2)
        run = ml.MPCRunner(s, rd, base, resident=True, plant_observation=table if tab else None, observation_seed=SEED)
        res[tab] = run.run(x0, steps, u_init=ui)[0][-1]
        assert np.all(s.plant_alive() == 1) and np.all(np.isfinite(run.last_cost))
        if tab:
            assert s.plant_num_observation_sets() == Bn and np.array_equal(s.plant_get_observation()[0], table) and s.plant_intervals() == steps
        s.close()
    d = res[True] - res[False]
    dist = np.abs(d).max(axis=1)
    print("after %d intervals: |x - x(no table)| per rollout %s; pelvis x of the biased rollouts moved by %s (bias +0.01 on the measured x)" % (steps, dist, d[biased, 0]))
    assert np.all(dist[biased] > 1e-6)
    assert np.all(np.abs(res[True][biased] - res[True][~biased]).max(axis=1) > 1e-6)                       # ... and from the unbiased pair of the same run


# ---- 7: refusals on a live handle
def test_refusals_on_a_live_handle():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    sv = _sv()
    A = _solver(0, False)
    rec = oc.plant_records(B)
    for bad in (np.ones((2, 100)), np.ones((B, 99))):
        with pytest.raises(ValueError):
            A.plant_set_observation(bad)
    two = np.ascontiguousarray(rec[:2])
    import ctypes as C
    assert A.L.ilqr_hip_plant_set_observation(A.h, two.ctypes.data_as(sv._dp), 2, C.c_ulonglong(1), C.c_ulonglong(0)) == 1      # n neither 1 nor B, past the wrapper
    assert A.L.ilqr_hip_plant_set_observation(A.h, None, 1, C.c_ulonglong(1), C.c_ulonglong(0)) == 1
    for col, v in ((0, np.nan), (49, np.inf), (50, np.nan), (99, -np.inf), (50, -1e-12), (99, -1.0)):      # non-finite, a negative sigma
        q = rec.copy(); q[B - 1, col] = v
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_observation(q)
    assert A.plant_num_observation_sets() == 0
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        A.plant_observation_errors(0, 1)                                                                   # no table: nothing to draw from
    A.plant_set_observation(rec[:1], seed=5)
    assert A.plant_num_observation_sets() == 1
    assert A.plant_observation_errors(0, N).shape == (N, B, NX)
    with pytest.raises(ValueError):
        A.plant_observation_errors(0, N + 1)                                                               # count beyond N: the wrapper ...
    buf = np.zeros((N + 1, B, NX))
    assert A.L.ilqr_hip_plant_observation_errors(A.h, C.c_long(0), N + 1, buf.ctypes.data_as(sv._dp)) == 1      # ... and the entry point
    assert A.L.ilqr_hip_plant_observation_errors(A.h, C.c_long(-1), 1, buf.ctypes.data_as(sv._dp)) == 1
    assert np.all(buf == 0.0)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(A, None, None, plant_observation=rec)
    A.close()
