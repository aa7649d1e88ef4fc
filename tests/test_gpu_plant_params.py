"""The plant's own model and one parameter set per rollout on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_model /
ilqr_hip_plant_set_params; csrc/plant_kernels.hip k_plant_follow_p).

Method of tests/test_gpu_plant.py: the yardstick is never the new kernel but the TEACHER-FORCED composition of entry points that existed
before it -- A.compute_control, the torque gain applied to u on the host, then step / step_stance / step_geometry on one handle per distinct
parameter set, created at DT / SUBSTEPS with that set's gravity, friction, softness and stiffness and the PLANT's contact mode and
joint-limit option (tests/plant_params_cases.py, where the batch is described: B = 37, N = 6, set b % 3, stance pattern (b // 3) % 4).

Every table case first asserts, on the yardstick alone, that each column acting in the case matters: the yardstick with that column set back
to set 0's value differs from the true one by more than 1e-6 in at least four rollouts, at feedback mode 0 one of them in each workgroup.

Bounds: reported u -- U_TOL of tests/test_gpu_plant.py; state on the walking rows of the GEOMETRY case -- X_TOL_PER_STEP x SUBSTEPS; state on
the envelope states -- cc.STEP_TOL x SUBSTEPS relative to max(1, max |want|) of the rollout.  Each case runs the same comparison with NO
table installed first, as a control (the kernel without a table on the same inputs, against the handle's own values), and prints both worst
errors."""
import os

import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import oracle_lib as ol
import plant_params_cases as pc
import plant_score_ref as ps
from conftest import load_package
from test_gpu_plant import U_TOL, X_TOL_PER_STEP, _geometry_states

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU, NQ = 51, 19, 26
B, N, DT, SUBSTEPS = pc.B, pc.N, pc.DT, pc.SUBSTEPS
HANDLE_MU = 0.3      # the solving handle's friction coefficient: set 0 is then "the handle's values"


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _problem():
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=dc.GRAVITY)
    prob["stance"] = pc.schedule()
    return prob


def _solver(mode=0, limits=False, plant_model=None, source="schedule", fb=0, ring=0):
    """the solving handle: one iteration per solve, friction HANDLE_MU, stiffness 0, softness 1e-5 -- the values of set 0"""
    sv = _sv()
    A = sv.BatchedILQR(B, N=N, dt=DT)
    A.set_contact_mode(mode); A.set_friction(HANDLE_MU); A.set_joint_limits(limits); A.set_max_iterations(1)
    if plant_model is not None:
        A.plant_set_model(*plant_model)
    A.plant_configure(SUBSTEPS, fb, source)
    A.plant_set_history(ring)
    A.set_problem(_problem())
    return A


def _states(group, P=None, offset=pc.STATE_OFFSET):
    if group == "geometry":
        x0 = _geometry_states(P, B, np.random.default_rng(14))
        ug = _sv().gravity_compensation(sc.standing_state(), dc.GRAVITY)
        return x0, np.tile(ug, (B, N, 1))
    x16, u16 = dc.mid() if group == "mid" else cc.sliding_states("mid")[:2] if group == "sliding" else cc.limit_states()
    return pc.batch(x16, u16, offset)


def _state_error(got, want, group):
    """(worst error in units of the bound's scale, bound): absolute on the walking rows, relative to max(1, max |want|) per rollout on the envelope"""
    if group == "geometry":
        return float(np.abs(got - want).max()), X_TOL_PER_STEP * SUBSTEPS
    scale = np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))
    return float((np.abs(got - want) / scale).max()), cc.STEP_TOL * SUBSTEPS


def _teacher_forced(A, Y, table, x0, flags, fb, advances, group, tag):
    """`advances` plant_advance calls from ONE solve, each held to the yardstick from the state it started from; returns (worst state error,
    the states the advances started from)"""
    A.plant_reset(x0)
    x, worst, starts = x0.copy(), 0.0, []
    for k in range(advances):
        want_x, want_u, want_st = Y.advance(A, table, x, flags, fb)
        A.plant_advance()
        got_x, got_u, got_st, alive = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        err, bound = _state_error(got_x, want_x, group)
        print("%s advance %d: state error %.3e (bound %.1e)  |du| %.3e  alive %d/%d" % (tag, k, err, bound, np.abs(got_u - want_u).max(), alive.sum(), B))
        assert np.all(alive == 1) and np.all(np.isfinite(want_x)), (tag, k)                  # no rollout is left out
        assert np.allclose(got_u, want_u, **U_TOL), (tag, k, np.abs(got_u - want_u).max())   # the REPORTED control: the law's output, unscaled
        assert err < bound, (tag, k, err)
        if Y.mode:
            assert np.array_equal(got_st, want_st), (tag, k)
        worst = max(worst, err); starts.append(x)
        x = got_x
    return worst, starts


def _assert_columns_matter(A, Y, table, starts, flags, fb, mode, limits, tag):
    """on the yardstick alone: every acting column moves at least four rollouts, at feedback mode 0 one in each workgroup"""
    true = [Y.advance(A, table, x, flags, fb)[0] for x in starts]
    moved = {}
    for name in pc.acting_columns(mode, limits):
        alt = pc.with_column_shared(table, name)
        moved[name] = np.any([np.abs(Y.advance(A, alt, x, flags, fb)[0] - t).max(axis=1) > 1e-6 for x, t in zip(starts, true)], axis=0)
    pc.check_column_conditions(moved, fb, tag)


#            plant mode, limits, stance source, states
CASES = {
    "free": (0, False, "schedule", "mid"),
    "mode3_sliding": (3, False, "schedule", "sliding"),
    "mode4_limits": (4, True, "schedule", "limits"),
    "mode0_limits_kind5": (0, True, "schedule", "limits"),
    "mode2_geometry": (2, False, "geometry", "geometry"),
}


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plant_with_a_table_matches_the_host_composition(case, fb):
    mode, limits, source, group = CASES[case]
    sv = _sv()
    A = _solver(mode, limits, source=source, fb=fb)
    Y = pc.Yardstick(sv, sc, mode, limits, source)
    x0, ui = _states(group, Y.handle(pc.SETS[0]))
    flags = pc.schedule()[:, 0]
    A.initialize(x0, ui); A.solve(x0)
    assert np.all(np.isfinite(A.ubar())) and np.all(np.isfinite(A.gains_K()))
    table = pc.params()
    tag = "%s fb%d" % (case, fb)
    # control: no table, the handle's own values (set 0 for every rollout) -- the kernel without a table on the same inputs
    assert A.plant_num_param_sets() == 0
    control, _ = _teacher_forced(A, Y, pc.params(pc.SETS[[0, 0, 0]]), x0, flags, fb, 2, group, tag + " control (no table)")
    A.plant_set_params(table)
    assert A.plant_num_param_sets() == B and np.array_equal(A.plant_params(), table)
    worst, starts = _teacher_forced(A, Y, table, x0, flags, fb, 2, group, tag + " table")
    print("%s: worst state error with the table %.3e, without (control) %.3e" % (tag, worst, control))
    assert np.abs(starts[1] - starts[0]).max() > 1e-3                                        # the second advance has x != xbar_0: the gains act
    _assert_columns_matter(A, Y, table, starts, flags, fb, mode, limits, tag)
    A.close(); Y.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_followed_intervals_with_a_table_match_the_host_composition(fb):
    """one plant_follow(0, 3) in plant mode 4 with joint-limit rows: interval j under knot j of the policy and row j of the schedule, held to
    the yardstick from the ring row it started from"""
    mode, limits, group = 4, True, "limits"
    sv = _sv()
    A = _solver(mode, limits, fb=fb, ring=3)
    Y = pc.Yardstick(sv, sc, mode, limits)
    x0, ui = _states(group)
    flags, table = pc.schedule()[:, 0], pc.params()
    A.initialize(x0, ui); A.solve(x0)
    A.plant_set_params(table)
    A.plant_reset(x0)
    A.plant_follow(0, 3)
    hx, hu = A.plant_history()
    assert hx.shape == (3, B, NX) and np.array_equal(hx[0], x0) and np.all(A.plant_alive() == 1)
    ends = [hx[1], hx[2], A.plant_state()]
    for j in range(3):
        want_x, want_u, want_st = Y.advance(A, table, hx[j], flags, fb, knot=j)
        err, bound = _state_error(ends[j], want_x, group)
        print("follow fb%d interval %d: state error %.3e (bound %.1e)  |du| %.3e" % (fb, j, err, bound, np.abs(hu[j] - want_u).max()))
        assert np.allclose(hu[j], want_u, **U_TOL) and err < bound, (j, err)
    assert np.array_equal(A.plant_stance(), want_st) and np.array_equal(A.plant_control(), hu[2])
    # ... and the same three intervals as three advances-by-follow, bit for bit
    A.plant_reset(x0)
    for j in range(3):
        A.plant_follow(j, 1)
    hx1, hu1 = A.plant_history()
    assert np.array_equal(hx1, hx) and np.array_equal(hu1, hu) and np.array_equal(A.plant_state(), ends[2])
    A.close(); Y.close()


def test_model_mismatch_plant_in_mode_3_with_limits_under_a_free_solver():
    """the solver plans constraint-free without joint-limit rows; the plant steps in contact mode 3 with them.  Yardstick: handles in mode 3
    with the rows.  The solver's own step and solve do not change by a bit."""
    sv = _sv()
    x0, ui = _states("limits", offset=pc.STATE_OFFSET_MODE3_LIMITS)
    flags, table = pc.schedule()[:, 0], pc.params()
    ref = _solver(0, False)
    ref.initialize(x0, ui); cost_ref = ref.solve(x0)
    xb_ref, ub_ref, K_ref, step_ref = ref.xbar(), ref.ubar(), ref.gains_K(), ref.step(x0, ui[:, 0])
    A = _solver(0, False, plant_model=(3, True))
    A.initialize(x0, ui); cost = A.solve(x0)
    assert np.array_equal(cost, cost_ref) and np.array_equal(A.xbar(), xb_ref) and np.array_equal(A.ubar(), ub_ref) and np.array_equal(A.gains_K(), K_ref)
    assert np.array_equal(A.step(x0, ui[:, 0]), step_ref)                                    # (the constraint-free step of the SOLVER's model)
    Y = pc.Yardstick(sv, sc, 3, True)
    for fb in (0, 1):
        A.plant_configure(SUBSTEPS, fb, "schedule")
        A.plant_clear_params()
        control, _ = _teacher_forced(A, Y, pc.params(pc.SETS[[0, 0, 0]]), x0, flags, fb, 2, "limits", "mismatch fb%d control (no table)" % fb)
        A.plant_set_params(table)
        worst, starts = _teacher_forced(A, Y, table, x0, flags, fb, 2, "limits", "mismatch fb%d table" % fb)
        print("mismatch fb%d: worst state error with the table %.3e, without (control) %.3e" % (fb, worst, control))
        _assert_columns_matter(A, Y, table, starts, flags, fb, 3, True, "mismatch fb%d" % fb)
    # the plant really is another model: the solver's own model, stepped from the same state under the same control, goes elsewhere
    free = pc.Yardstick(sv, sc, 0, False)
    other = free.advance(A, table, x0, flags, 0)[0]
    assert (np.abs(other - Y.advance(A, table, x0, flags, 0)[0]).max(axis=1) > 1e-6).sum() >= B // 2
    # ... and the solve after the plant ran is still the solver's: the second solve of a handle (it inherits the first one's regularisation)
    # against the second solve of the handle that never had a plant model or a table
    A.initialize(x0, ui); ref.initialize(x0, ui)
    assert np.array_equal(A.solve(x0), ref.solve(x0)) and np.array_equal(A.gains_K(), ref.gains_K()) and np.array_equal(A.xbar(), ref.xbar())
    # back to following the solver: the plant is the free plant again, bit for bit the handle that never had a model of its own
    A.plant_set_model(None, None); A.plant_clear_params(); A.plant_configure(SUBSTEPS, 0, "schedule")
    ref.plant_reset(x0); ref.plant_advance(); A.plant_reset(x0); A.plant_advance()
    assert np.array_equal(A.plant_state(), ref.plant_state())
    A.close(); ref.close(); Y.close(); free.close()


def _one_advance(A, x0):
    A.plant_reset(x0)
    A.plant_advance()
    return A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()


def _two_advances(A, x0, follow=False):
    A.plant_reset(x0)
    if follow:
        A.plant_follow(0, 2)
    else:
        A.plant_follow(0, 1); A.plant_follow(1, 1)
    return A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


@pytest.mark.parametrize("case,fb", [("free", 0), ("free", 1), ("mode4_limits", 0), ("mode4_limits", 1)])
def test_equivalences_of_the_table(case, fb):
    mode, limits, source, group = CASES[case]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb, ring=2)
    A.initialize(x0, ui); A.solve(x0)
    # plant_params() without a table: the handle's values and gain 1
    own = A.plant_params()
    assert np.array_equal(own, np.tile([0.0, 0.0, -9.81, HANDLE_MU, 1e-5, 0.0, 1.0], (B, 1)))
    none1, none = _one_advance(A, x0), _two_advances(A, x0)
    # a uniform table of the handle's own values and gain 1 is the plant without a table, within the bound of the teacher-forced tests
    # (one interval from the same state: a second one would start from two different states)
    A.plant_set_params(own[:1])
    assert A.plant_num_param_sets() == 1 and np.array_equal(A.plant_params(), own)
    uni = _one_advance(A, x0)
    err, bound = _state_error(uni[0], none1[0], group)
    print("%s fb%d: uniform table of the handle's values against no table: state error %.3e, bit-identical: %s" % (case, fb, err, _same(uni, none1)))
    assert err < bound and np.allclose(uni[1], none1[1], **U_TOL) and np.array_equal(uni[2], none1[2]) and np.array_equal(uni[3], none1[3])
    # one record for all rollouts against B identical records: bit for bit
    one = pc.SETS[2:3]
    A.plant_set_params(one); r1 = _two_advances(A, x0)
    A.plant_set_params(np.repeat(one, B, axis=0)); rB = _two_advances(A, x0)
    assert _same(r1, rB) and not np.array_equal(r1[0], none[0])
    # follow(0, 2) against two calls, under the per-rollout table: bit for bit
    A.plant_set_params(pc.params())
    assert np.array_equal(A.plant_params(), pc.params())                                      # round trip
    split = _two_advances(A, x0)
    h_split = A.plant_history()
    fused = _two_advances(A, x0, follow=True)
    assert _same(split, fused) and _same(h_split, A.plant_history()) and not np.array_equal(split[0], none[0])
    # the table survives plant_reset and plant_configure
    A.plant_configure(SUBSTEPS, fb, "schedule")
    assert A.plant_num_param_sets() == B and _same(_two_advances(A, x0), split)
    # clear_params: today's results, bit for bit
    A.plant_clear_params()
    assert A.plant_num_param_sets() == 0 and _same(_two_advances(A, x0), none)
    A.plant_clear_params()                                                                    # (clearing nothing is fine)
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_a_non_finite_rollout_freezes_alone_under_a_table(fb):
    bad = 33                                                                                   # in the second workgroup at feedback mode 0
    x0, ui = _states("mid")
    out = {}
    for poisoned in (False, True):
        A = _solver(0, False, fb=fb, ring=2)
        A.initialize(x0, ui); A.solve(x0)
        A.plant_set_params(pc.params())
        xp = x0.copy()
        if poisoned:
            xp[bad, 9] = np.nan
        out[poisoned] = _two_advances(A, xp, follow=True)
        A.close()
    x, u, st, alive = out[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(u[bad] == 0.0) and np.array_equal(x[bad], np.where(np.arange(NX) == 9, np.nan, x0[bad]), equal_nan=True)
    assert np.all(alive[keep] == 1) and np.all(out[False][3] == 1)
    assert np.array_equal(x[keep], out[False][0][keep]) and np.array_equal(u[keep], out[False][1][keep])      # bit for bit


def test_score_under_a_table_is_the_score_of_the_ring():
    """the record is a function of ring rows, reference rows and scoring weights: with a table (and a torque gain) it scores the REPORTED,
    unscaled control of the ring"""
    Q, R, _ = sc.build_cost_matrices()
    score = dict(Q=0.37 * Q + 1.0, R=0.05 + 0.01 * np.arange(NU), upright=7.0, balance=11.0, joint_limits=900.0, control_limits=1300.0)
    x0, ui = _states("limits")
    A = _solver(4, True, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_set_params(pc.params())
    A.plant_set_score(**score)
    A.plant_reset(x0)
    A.plant_advance(); A.plant_follow(1, 2)
    got = A.plant_score()
    hx, hu = A.plant_history()
    prob = _problem()
    want = ps.expected_record(ps.IntervalOracle(DT), [(prob, k) for k in range(3)], hx, hu, score)
    ok, worst = ps.close_enough(got, want)
    print("score under a table: worst |got - want| / bound = %.3f" % worst)
    assert ok.all() and np.array_equal(got[:, 6:], want[:, 6:])
    assert np.any(want[:, 5] != 0.0)                                                           # (the control-limit term is alive: it sees the unscaled u)
    A.close()


def test_refusals_on_a_live_handle():
    sv = _sv()
    A = _solver(0, False)
    for bad in (np.ones((2, 7)), np.ones((B, 6))):
        with pytest.raises(ValueError):
            A.plant_set_params(bad)
    p = pc.params()
    for col, v in ((3, -1.0), (4, 0.0), (5, -1.0), (6, -0.1), (0, np.nan)):
        q = p.copy(); q[B - 1, col] = v
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_params(q)
    assert A.plant_num_param_sets() == 0
    # the geometry refusal follows the PLANT's mode: a welded plant foot never leaves the floor, whatever the solver plans with
    A.set_contact_mode(2)
    A.plant_configure(SUBSTEPS, 0, "geometry")
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        A.plant_set_model(1, None)
    A.plant_configure(SUBSTEPS, 0, "schedule")
    A.plant_set_model(1, None)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        A.plant_configure(SUBSTEPS, 0, "geometry")
    A.set_contact_mode(1)                                                                      # the solver welded, the plant unilateral: allowed
    A.plant_set_model(2, None)
    A.plant_configure(SUBSTEPS, 0, "geometry")
    A.close()


def test_runner_installs_model_and_table():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, Nn, steps = 4, 25, 3
    base = sc.make_problem(sv.reference_kinematics, N=Nn, gravity=dc.GRAVITY)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(Bn, Nn, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    table = sc.stack_plant_params(Bn, friction=[0.3, 0.5, 0.7, 1.0], torque_gain=[1.0, 0.9, 0.8, 1.0])
    res = {}
    for with_table in (False, True):
        s = sv.BatchedILQR(Bn, N=Nn, dt=DT); s.set_max_iterations(2)
        run = ml.MPCRunner(s, rd, base, resident=True, substeps=2, plant_model=(3, True) if with_table else None, plant_params=table if with_table else None)
        res[with_table] = run.run(x0, steps, u_init=ui)
        if with_table:
            assert np.array_equal(s.plant_params(), table) and s.plant_num_param_sets() == Bn
        s.close()
    assert np.all(np.isfinite(res[True][0])) and res[True][0].shape == (steps + 1, Bn, NX)
    assert np.abs(res[True][0][-1] - res[False][0][-1]).max() > 1e-6                           # another plant: another closed loop
