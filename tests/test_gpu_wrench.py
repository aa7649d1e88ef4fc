"""The sustained external wrench on the pelvis on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_wrench, ilqr_hip_step_wrench;
csrc/plant_kernels.hip k_plant_follow_w, k_step_w).

No entry point that existed before the feature carries a wrench, so the ground truth is in two layers:
  * ilqr_hip_step_wrench against the golden of the NumPy Kane / KKT restatement (tests/golden/gen_wrench_golden.py) in all six step kinds,
    and against the CPU oracle's inverse dynamics on the envelope states (tests/wrench_cases.py: the base rows of the inverse dynamics of
    a constraint-free step ARE the generalized force of the wrench);
  * the plant kernels against the TEACHER-FORCED composition compute_control -> step_wrench per substep on handles at DT / SUBSTEPS
    (tests/plant_params_cases.py Yardstick with step_wrench in the place of step / step_stance), on the cases and state groups of
    tests/test_gpu_plant_params.py: B = 37 (two workgroups at feedback mode 0, ten at mode 1), N = 6, SUBSTEPS = 2.

Bounds: 1e-10 absolute for a step of contact mode 0 without rows (dynamics_golden's), cc.STEP_TOL = 1e-9 relative to max(1, max |want|)
otherwise; plant: U_TOL, X_TOL_PER_STEP x SUBSTEPS, cc.STEP_TOL x SUBSTEPS as tests/test_gpu_plant_params.py.  Inverse dynamics: 1e-6 N --
a step error of 1e-11 divided by h = 0.02 and multiplied by the robot's 50 kg is 3e-8, with margin."""
import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import plant_params_cases as pc
import wrench_cases as wc
from conftest import load_package
from test_gpu_plant import U_TOL
from test_gpu_plant_params import CASES, _solver, _state_error, _states

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU, NQ = 51, 19, 26
B, N, DT, SUBSTEPS = pc.B, pc.N, pc.DT, pc.SUBSTEPS
ID_TOL = 1e-6
KINDS = {0: (0, 0), 1: (1, 0), 2: (4, 0), 3: (1, 1), 4: (4, 1), 5: (0, 1)}      # step kind -> (a contact mode of the kind, joint-limit rows); kinds 1 / 3 serve modes 1-3


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _kind_of(mode, limits):
    return 5 if (mode == 0 and limits) else 0 if mode == 0 else (2 if mode == 4 else 1) + (2 if limits else 0)


def _step_handle(count, h, gravity, mode, limits, mu=1.0, soft=1e-5, k=0.0):
    sv = _sv()
    P = sv.BatchedILQR(count, N=1, dt=h)
    P.set_problem(sc.make_problem(sv.reference_kinematics, N=1, gravity=tuple(gravity)))
    P.set_contact_mode(mode, soft); P.set_friction(mu); P.set_joint_limits(bool(limits)); P.set_joint_limit_stiffness(k)
    return P


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want).max(axis=-1, keepdims=True))).max())


# ---- 1, 3a: the step kernel against the golden, every kind; a zero wrench against step_stance
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_step_wrench_matches_the_golden(kind):
    g = wc.golden()
    cases = [i for i in range(len(g["x"])) if _kind_of(int(g["contact"][i]), int(g["limits"][i])) == kind]
    assert cases, kind
    for i in cases:
        mode, limits = int(g["contact"][i]), int(g["limits"][i])
        P = _step_handle(1, float(g["h"]), g["gravity"], mode, limits, float(g["mu"][i]), float(g["soft"]))
        sl, sr = (int(v) for v in g["stance"][i])
        x, u, w, want = g["x"][i][None], g["u"][i][None], g["wrench"][i][None], g["x_next"][i][None]
        got = P.step_wrench(x, u, sl, sr, w)
        free = mode == 0 and not limits
        err, bound = (float(np.abs(got - want).max()), 1e-10) if free else (_rel(got, want), cc.STEP_TOL)
        zero = P.step_wrench(x, u, sl, sr, np.zeros((1, 9)))
        plain = P.step_stance(x, u, sl, sr)
        errz = float(np.abs(zero - plain).max()) if free else _rel(zero, plain)
        print("kind %d case %2d (mode %d, limits %d, stance %d%d, changed %d): error %.3e (bound %.0e); zero wrench against step_stance %.3e"
              % (kind, i, mode, limits, sl, sr, int(g["changed"][i]), err, bound, errz))
        assert np.all(np.isfinite(got)) and err < bound, (i, err)
        assert errz < bound, (i, errz)                                                       # (not bit for bit: another instantiation)
        if np.abs(w).max() > 0:
            assert np.abs(got - plain).max() > 1e-6, i                                          # the wrench acts
        P.close()


# ---- 2: the oracle's inverse dynamics of the GPU step on the envelope states
@pytest.mark.parametrize("group,limits", [("mid", False), ("limits", True)])
def test_base_rows_of_the_inverse_dynamics_are_the_wrench(group, limits):
    x, u = dc.mid() if group == "mid" else cc.limit_states()
    w = wc.random_wrenches(dc.NS, 5 + int(limits))
    P = _step_handle(dc.NS, dc.H, dc.GRAVITY, 0, limits)
    xn = P.step_wrench(x, u, 1, 1, w)
    plain = P.step(x, u)
    P.close()
    assert np.all(np.isfinite(xn))
    stopped = cc.stopped_hinges(x, xn[:, None, :], 0.0)[:, 0, :] & (cc.violation(x) != 0.0) if limits else np.zeros((dc.NS, NU), dtype=bool)
    worst_b = worst_h = 0.0
    for i in range(dc.NS):
        res = wc.inverse_dynamics_residual(x[i], xn[i], u[i], dc.H, np.array(dc.GRAVITY))
        worst_b = max(worst_b, float(np.abs(res[:6] - wc.generalized_force(x[i], w[i])).max()))
        worst_h = max(worst_h, float(np.abs(res[6:][~stopped[i]]).max()))
        assert np.abs(xn[i] - plain[i]).max() > 1e-6, i
    print("%s: base rows against Wg %.3e, free hinge rows %.3e (bound %.0e); %d hinges stopped" % (group, worst_b, worst_h, ID_TOL, int(stopped.sum())))
    assert worst_b < ID_TOL and worst_h < ID_TOL
    if limits:
        assert stopped.sum() >= 16                                                              # the second pass ran, under the wrench


# ---- 4: a force at r is the force at the origin plus the torque of its lever arm
@pytest.mark.parametrize("mode,limits", [(0, False), (3, False), (4, True), (0, True)])
def test_point_of_application_is_a_lever_arm(mode, limits):
    x, u = cc.limit_states() if limits else dc.mid()
    w = wc.random_wrenches(dc.NS, 9)
    moved = w.copy()
    moved[:, 6:9] = 0.0
    for i in range(dc.NS):
        moved[i, 3:6] += wc.world_torque_of_offset(x[i], w[i])
    P = _step_handle(dc.NS, dc.H, dc.GRAVITY, mode, limits, mu=0.3)
    a, b_ = P.step_wrench(x, u, 1, 1, w), P.step_wrench(x, u, 1, 1, moved)
    nolever = P.step_wrench(x, u, 1, 1, np.hstack([w[:, :6], np.zeros((dc.NS, 3))]))
    P.close()
    err = _rel(a, b_)
    print("mode %d limits %d: F at r against F at 0 + R0 (r x R0^T F): %.3e" % (mode, limits, err))
    assert np.all(np.isfinite(a)) and err < 1e-12
    assert (np.abs(a - nolever).max(axis=1) > 1e-6).all()                                        # the lever arm acts


# ---- the yardstick of the plant: compute_control, then step_wrench per substep
class WrenchYardstick(pc.Yardstick):
    def step_w(self, table, x, u, flags, w9):
        xn, st = np.empty_like(x), np.array(flags, dtype=np.int32)
        ua = table[:, 6:7] * u
        for s in np.unique(table[:, :6], axis=0):
            rows = np.flatnonzero((table[:, :6] == s).all(axis=1))
            P = self.handle(s)
            fl = np.array(flags[rows], dtype=np.int32)
            if self.mode and self.source == "geometry":
                _, fl = P.step_geometry(x[rows], ua[rows])                                   # the flags each rollout's own feet decide (mode 2: then the scheduled step)
                st[rows] = fl
            for l, r in {(int(a), int(c)) for a, c in fl}:
                idx = rows[(fl[:, 0] == l) & (fl[:, 1] == r)]
                xn[idx] = P.step_wrench(x[idx], ua[idx], l, r, w9[idx])
        return xn, st

    def advance_w(self, A, table, wrench, interval, x, flags, fb, knot=0):
        """one MPC interval under the records of `wrench` [B, 11] whose window holds `interval`: (x_next, reported u, stance)"""
        on = (wrench[:, 9] <= interval) & (interval < wrench[:, 10])
        w9 = np.where(on[:, None], wrench[:, :9], 0.0)
        xc, u, st = x.copy(), None, np.array(flags, dtype=np.int32)
        for k in range(SUBSTEPS):
            if k == 0 or fb:
                u = A.compute_control(xc, knot=knot)
                u[~np.isfinite(u).all(axis=1)] = 0.0
            xc, st = self.step_w(table, xc, u, flags, w9)
        return xc, u, st


def _wrench_table(seed=3):
    """set b % 3: always on / opens at interval 1 / never (an empty window)"""
    w9 = wc.random_wrenches(B, seed)
    b = np.arange(B)
    first = np.where(b % 3 == 1, 1.0, 0.0)
    end = np.where(b % 3 == 2, 0.0, np.inf)
    return np.ascontiguousarray(np.hstack([w9, first[:, None], end[:, None]]))


OWN = pc.params(pc.SETS[[0, 0, 0]])      # the handle's own values for every rollout: the parameter record of a plant without a parameter table


def _teacher_forced_w(A, Y, table, wrench, x0, flags, fb, advances, group, tag):
    A.plant_reset(x0)
    assert A.plant_intervals() == 0
    x, worst, moved = x0.copy(), 0.0, np.zeros(B, dtype=bool)
    none = np.zeros((B, 11))
    for k in range(advances):
        want_x, want_u, want_st = Y.advance_w(A, table, wrench, k, x, flags, fb)
        moved |= np.abs(want_x - Y.advance_w(A, table, none, k, x, flags, fb)[0]).max(axis=1) > 1e-6
        A.plant_advance()
        got_x, got_u, got_st, alive = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        err, bound = _state_error(got_x, want_x, group)
        print("%s advance %d: state error %.3e (bound %.1e)  |du| %.3e  alive %d/%d" % (tag, k, err, bound, np.abs(got_u - want_u).max(), alive.sum(), B))
        assert np.all(alive == 1) and np.all(np.isfinite(want_x)), (tag, k)
        assert np.allclose(got_u, want_u, **U_TOL), (tag, k, np.abs(got_u - want_u).max())
        assert err < bound, (tag, k, err)
        if Y.mode:
            assert np.array_equal(got_st, want_st), (tag, k)
        worst = max(worst, err)
        x = got_x
    assert A.plant_intervals() == advances
    return worst, moved


# ---- 5: teacher-forced plant, both feedback modes, the cases of the parameter-table tests
@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plant_under_a_wrench_table_matches_the_host_composition(case, fb):
    mode, limits, source, group = CASES[case]
    sv = _sv()
    A = _solver(mode, limits, source=source, fb=fb)
    Y = WrenchYardstick(sv, sc, mode, limits, source)
    x0, ui = _states(group, Y.handle(pc.SETS[0]))
    flags = pc.schedule()[:, 0]
    A.initialize(x0, ui); A.solve(x0)
    assert np.all(np.isfinite(A.ubar())) and np.all(np.isfinite(A.gains_K()))
    wrench = _wrench_table()
    tag = "%s fb%d" % (case, fb)
    assert A.plant_num_wrench_sets() == 0 and np.array_equal(A.plant_wrench(), np.zeros((B, 11)))
    control, _ = _teacher_forced_w(A, Y, OWN, np.zeros((B, 11)), x0, flags, fb, 2, group, tag + " control (no table)")
    A.plant_set_wrench(wrench)
    assert A.plant_num_wrench_sets() == B and np.array_equal(A.plant_wrench(), wrench)
    worst, moved = _teacher_forced_w(A, Y, OWN, wrench, x0, flags, fb, 2, group, tag + " wrench")
    print("%s: worst state error under the wrenches %.3e, without a table (control) %.3e" % (tag, worst, control))
    pc.check_column_conditions({"wrench": moved}, fb, tag)                                    # on the yardstick alone: the wrench matters in every workgroup
    assert not moved[np.arange(B) % 3 == 2].any()                                             # a window that never opens moves nothing
    A.close(); Y.close()


# ---- 3b: a table whose windows never open is the plant without a table
@pytest.mark.parametrize("case,fb", [("free", 0), ("mode4_limits", 1)])
def test_a_table_whose_windows_never_open_is_no_table(case, fb):
    mode, limits, source, group = CASES[case]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_reset(x0); A.plant_advance()
    none = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
    shut = _wrench_table(); shut[:, 9] = 5.0; shut[:, 10] = 9.0
    A.plant_set_wrench(shut)
    A.plant_reset(x0); A.plant_advance()
    got = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
    err, bound = _state_error(got[0], none[0], group)
    print("%s fb%d: shut windows against no table: state error %.3e (bound %.1e)" % (case, fb, err, bound))
    assert err < bound and np.allclose(got[1], none[1], **U_TOL) and np.array_equal(got[2], none[2]) and np.array_equal(got[3], none[3])
    # the table survives plant_reset and plant_configure; clearing it gives today's results bit for bit
    A.plant_configure(SUBSTEPS, fb, "schedule")
    assert A.plant_num_wrench_sets() == B
    A.plant_clear_wrench()
    assert A.plant_num_wrench_sets() == 0
    A.plant_reset(x0); A.plant_advance()
    assert np.array_equal(A.plant_state(), none[0]) and np.array_equal(A.plant_control(), none[1])
    A.plant_clear_wrench()                                                                    # (clearing nothing is fine)
    A.close()


# ---- 6: a window that opens and closes inside a group
def _snapshot(A):
    hx, hu = A.plant_history()
    return A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive(), hx, hu


def _same(a, b_):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b_))


@pytest.mark.parametrize("fb", [0, 1])
def test_window_inside_a_group_is_the_same_in_one_launch_and_in_three(fb):
    """first = 1, end = 2, m = 3.  plant_follow(0, m) against m calls (j, 1): bit for bit in state, control, stance, alive and ring rows.  An
    advance applies knot 0 of the policy, so m advances are held to m calls (0, 1): the interval counter, not the knot, opens the window."""
    m = 3
    mode, limits, source, group = CASES["mode4_limits"]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb, ring=m)
    A.initialize(x0, ui); A.solve(x0)
    wrench = _wrench_table(); wrench[:, 9] = 1.0; wrench[:, 10] = 2.0
    A.plant_set_wrench(wrench)
    A.plant_reset(x0); assert A.plant_intervals() == 0
    A.plant_follow(0, m); fused = _snapshot(A)
    assert A.plant_intervals() == m
    A.plant_reset(x0); assert A.plant_intervals() == 0
    for j in range(m):
        A.plant_follow(j, 1)
    split = _snapshot(A)
    assert A.plant_intervals() == m and _same(fused, split) and np.all(fused[3] == 1)
    A.plant_reset(x0)
    for j in range(m):
        A.plant_advance()
    adv = _snapshot(A)
    assert A.plant_intervals() == m
    A.plant_reset(x0)
    for j in range(m):
        A.plant_follow(0, 1)
    assert _same(adv, _snapshot(A))
    # the window really opened in interval 1 and only there: against no table, ring row 1 (the state interval 1 starts from) is the same, row 2 is not
    A.plant_clear_wrench()
    A.plant_reset(x0); A.plant_follow(0, m); none = _snapshot(A)
    d1 = np.abs(none[4][1] - fused[4][1]).max(); d2 = np.abs(none[4][2] - fused[4][2]).max(axis=1)
    print("fb%d: ring row 1 differs from the run without a table by %.3e (other instantiation), row 2 by more than 1e-6 in %d rollouts" % (fb, d1, int((d2 > 1e-6).sum())))
    assert d1 < cc.STEP_TOL * SUBSTEPS * max(1.0, np.abs(none[4][1]).max()) and (d2 > 1e-6).sum() >= B // 2
    A.plant_set_history(0)
    assert A.plant_intervals() == m                                                           # set_history does not touch the counter
    A.close()


# ---- 7: parameter table and wrench table together
@pytest.mark.parametrize("fb", [0, 1])
def test_parameter_table_and_wrench_table_together(fb):
    mode, limits, source, group = CASES["mode4_limits"]
    sv = _sv()
    A = _solver(mode, limits, fb=fb)
    Y = WrenchYardstick(sv, sc, mode, limits, source)
    x0, ui = _states(group)
    flags, table, wrench = pc.schedule()[:, 0], pc.params(), _wrench_table(7)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_set_params(table); A.plant_set_wrench(wrench)
    worst, moved = _teacher_forced_w(A, Y, table, wrench, x0, flags, fb, 2, group, "both tables fb%d" % fb)
    pc.check_column_conditions({"wrench": moved}, fb, "both tables fb%d" % fb)
    # ... and the parameter table acts under the wrenches: the yardstick with the handle's own values goes elsewhere
    other = Y.advance_w(A, OWN, wrench, 0, x0, flags, fb)[0]
    assert (np.abs(other - Y.advance_w(A, table, wrench, 0, x0, flags, fb)[0]).max(axis=1) > 1e-6).sum() >= 4
    A.close(); Y.close()


# ---- 8: a wrench that makes one rollout non-finite freezes that rollout alone
@pytest.mark.parametrize("fb", [0, 1])
def test_an_overflowing_wrench_freezes_its_rollout_alone(fb):
    bad = 33                                                                                   # in the second workgroup at feedback mode 0
    x0, ui = _states("mid")
    out = {}
    for poisoned in (False, True):
        A = _solver(0, False, fb=fb, ring=2)
        A.initialize(x0, ui); A.solve(x0)
        wrench = _wrench_table()
        wrench[bad] = 0.0
        if poisoned:
            wrench[bad, 0] = 1e308; wrench[bad, 10] = np.inf
        A.plant_set_wrench(wrench)
        A.plant_reset(x0)
        A.plant_advance()
        out[poisoned] = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        A.close()
    x, u, st, alive = out[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(u[bad] == 0.0) and np.array_equal(x[bad], x0[bad])         # frozen in the state before the advance
    assert np.all(alive[keep] == 1) and np.all(out[False][3] == 1)
    assert np.array_equal(x[keep], out[False][0][keep]) and np.array_equal(u[keep], out[False][1][keep])      # bit for bit


# ---- 9: the runner pushes the plant
def test_runner_pushes_the_pelvis_in_the_direction_of_the_force():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, Nn, steps = 4, 25, 6
    base = sc.make_problem(sv.reference_kinematics, N=Nn, gravity=dc.GRAVITY)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(Bn, Nn, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    push = sc.stack_plant_wrench(Bn, force=(0.0, 40.0, 0.0), point=sv.pelvis_inertial_offset(), first=1, end=4)
    res = {}
    for pushed in (False, True):
        s = sv.BatchedILQR(Bn, N=Nn, dt=DT); s.set_contact_mode(2); s.set_max_iterations(2)
        run = ml.MPCRunner(s, rd, base, resident=True, substeps=2, plant_wrench=push if pushed else None)
        res[pushed] = run.run(x0, steps, u_init=ui)[0]
        assert np.all(s.plant_alive() == 1)
        if pushed:
            assert s.plant_num_wrench_sets() == Bn and np.array_equal(s.plant_wrench(), push) and s.plant_intervals() == steps
        s.close()
    dy = res[True][-1][:, 1] - res[False][-1][:, 1]
    print("pelvis y, pushed less unpushed, after %d intervals: %s" % (steps, dy))
    assert np.all(dy > 0.0)


def test_refusals_on_a_live_handle():
    sv = _sv()
    A = _solver(0, False)
    for bad in (np.ones((2, 11)), np.ones((B, 10))):
        with pytest.raises(ValueError):
            A.plant_set_wrench(bad)
    w = _wrench_table()
    for col, v in ((0, np.nan), (4, np.inf), (9, -1.0), (9, 0.5), (10, 2.5), (10, -np.inf)):
        q = w.copy(); q[B - 1, col] = v
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_wrench(q)
    q = w.copy(); q[:, 9] = 3.0; q[:, 10] = 2.0
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        A.plant_set_wrench(q)
    assert A.plant_num_wrench_sets() == 0
    A.plant_set_wrench(w[:1])                                                                  # one record for all rollouts
    assert A.plant_num_wrench_sets() == 1 and np.array_equal(A.plant_wrench(), np.repeat(w[:1], B, axis=0))
    A.close()
