"""The task family's part of the bounds track on the GPU (include/ilqr_hip.h ilqr_hip_set_al_task_bounds_track,
ilqr_hip_al_bounds_window_from_track; csrc/al_bounds_track_kernels.hip).

The cut is a pure copy, so everything here is bit for bit: the window read back through al_task_bounds() against NumPy indexing
(al_knot_ref.cut), and the stages and whole solves of a handle after a cut against a FRESH handle that was given the host-cut window through
set_al_task_bounds.  N = 4 (the smallest horizon of tests/test_gpu_al_knot.py), tracks of N + 4 rows (the end clamp is hit from step 3
on), B = 3 and B = 70 (tests/al_task_track_cases.py)."""
import numpy as np
import pytest

import al_knot_ref as kr
import al_state_ref as sr
import al_task_cases as atc
import al_task_ref as tr
import al_task_track_cases as tc
import test_gpu_linearization_cache as lc
from test_gpu_configs import _solver

pytestmark = pytest.mark.gpu

sc = tc.sc
N, ROWS = tc.N, tc.ROWS
AL = atc.AL_E2E
NAMES = ("lx", "lu", "lxx", "luu")
ERR_ARG, ERR_STATE = 1, 4


def _ug():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv.gravity_compensation(sc.standing_state(), (0.0, 0.0, -9.81))


def _handle(B, task=True, max_iter=atc.MAX_ITER, early_exit=True):
    """a handle on score_problem(B) with AL and (task) the task family installed on a window without bounds"""
    prob, x0, ui = tc.score_problem(B)
    s = _solver(B, N=N); s.set_problem(prob); s.set_max_iterations(max_iter)
    s.set_options(jacobian_mode=0, fd_eps=1e-5, early_exit=early_exit)
    s.set_augmented_lagrangian(**atc.al_args())
    if task:
        s.set_al_task_bounds(tc.install_window(), AL["rho_task0"], AL["tol_task"])
    return s, prob, np.array(x0), tc.u_init(ui, _ug())


def _starts(B):
    """one start per rollout: 0, 1, 2, ... with the last two beyond the last row"""
    st = np.arange(B) % (ROWS - 1)
    st[-1] = ROWS + 5; st[-2] = ROWS
    return st


@pytest.mark.parametrize("B", [tc.B_SMALL, tc.B_WAVE])
def test_cut_equals_numpy_indexing_bit_for_bit(B):
    track = tc.task_track()
    s, prob, x0, ui = _handle(B)
    assert s.al_task_bounds_track_rows() == 0 and s.al_bounds_track_rows() == 0
    s.set_al_task_bounds_track(track)
    assert s.al_task_bounds_track_rows() == ROWS and s.al_bounds_track_rows() == 0
    assert np.array_equal(s.al_task_bounds(), np.tile(tr.NO_BOUNDS, (B, N + 1, 1)))      # installing a track cuts nothing
    for starts in ([0], _starts(B)):
        if len(starts) > 1:
            s.set_al_bounds_track_starts(starts)
        for step in (0, 3):
            s.al_bounds_window_from_track(step)
            got = s.al_task_bounds()
            assert np.array_equal(got, kr.cut(track, starts, step, N, B)), (len(starts), step)
            assert s.num_al_task_bound_sets() == len(starts)
    assert np.array_equal(got[-1], np.tile(track[-1], (N + 1, 1))) and np.array_equal(got[0, -1], track[-1])      # the clamp, at step 3
    assert s.al_bounds_per_knot() == 0      # (the other families have no window of their own: the library repeats their records)
    # installing a track of either kind resets the starts to one shared 0
    s.set_al_task_bounds_track(track[::-1].copy())
    s.al_bounds_window_from_track(1)
    assert np.array_equal(s.al_task_bounds(), kr.cut(track[::-1], [0], 1, N, B)) and s.num_al_task_bound_sets() == 1
    s.set_al_bounds_track_starts(_starts(B))
    s.set_al_bounds_track(np.tile(sv_default_bounds(), (3, 1)))
    s.al_bounds_window_from_track(1)
    assert np.array_equal(s.al_task_bounds(), kr.cut(track[::-1], [0], 1, N, B)) and s.num_al_task_bound_sets() == 1
    # clearing the task track leaves the window last written, and the other track in place
    s.clear_al_task_bounds_track()
    assert s.al_task_bounds_track_rows() == 0 and s.al_bounds_track_rows() == 3
    assert np.array_equal(s.al_task_bounds(), kr.cut(track[::-1], [0], 1, N, B))
    s.close()


def sv_default_bounds():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv.al_default_bounds(0.0)


def _other_tracks(rows):
    """a joint / torque and a state track of `rows` rows whose rows differ"""
    jc = np.stack([sv_default_bounds() * (1.0 - 0.01 * r) for r in range(rows)])
    st = sc.stack_al_state_knot_bounds(dict(pelvis_z=[(r, r + 1, (0.5 + 1e-3 * r, np.inf)) for r in range(rows)]), 1, rows - 1)[0]
    return jc, st


def test_cut_beside_a_joint_and_a_state_track_with_another_row_count():
    B, rows2 = tc.B_WAVE, ROWS + 3
    track = tc.task_track()
    jc, st = _other_tracks(rows2)
    s, prob, x0, ui = _handle(B)
    s.set_al_state_bounds(sr.NO_BOUNDS, 1.0, 1e-3)
    s.set_al_bounds_track(jc, st)
    s.set_al_task_bounds_track(track)
    assert (s.al_bounds_track_rows(), s.al_task_bounds_track_rows()) == (rows2, ROWS)
    starts = _starts(B)
    s.set_al_bounds_track_starts(starts)
    for step in (0, 3, 6):                                        # 6: the task track is clamped where the other is not yet
        s.al_bounds_window_from_track(step)
        gj, gs = s.al_knot_bounds()
        assert np.array_equal(s.al_task_bounds(), kr.cut(track, starts, step, N, B)), step
        assert np.array_equal(gj, kr.cut(jc, starts, step, N, B)) and np.array_equal(gs, kr.cut(st, starts, step, N, B)), step
        assert s.al_bounds_per_knot() == 3 and s.num_al_task_bound_sets() == B
    # a joint / torque track alone leaves a hand-set task window untouched
    s.clear_al_task_bounds_track()
    hand = np.array(tc.score_case(B)[3])
    s.set_al_task_bounds(hand, AL["rho_task0"], AL["tol_task"])
    s.al_bounds_window_from_track(2)
    assert np.array_equal(s.al_task_bounds(), hand) and np.array_equal(s.al_knot_bounds()[0], kr.cut(jc, starts, 2, N, B))
    s.close()


def _stage(s):
    s.stage_cost_quadratics()
    return dict(zip(NAMES, s.quadratics())), s.stage_total_cost()


def _al_observables(s, cost):
    obs, counters = lc.observables(s, cost)
    assert counters["adopt"] == 0
    mj, mc = s.al_multipliers(); viol, done = s.al_violation()
    extra = dict(mu_j=mj, mu_c=mc, rho=s.al_penalties(), viol=viol, done=done, al_trace=s.al_trace(), mu_t=s.al_task_multipliers(), rho_t=s.al_task_penalties(),
                 viol_t=s.al_task_violation(), task_trace=s.al_task_trace(), win=s.al_task_bounds(), points=s.al_task_points())
    return obs, extra


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_stages_and_a_whole_solve_after_a_cut_equal_a_fresh_handle_bit_for_bit(early_exit):
    B, step = tc.B_SMALL, 3
    track = tc.active_track()
    starts = [0, 2, ROWS]
    want_win = kr.cut(track, starts, step, N, B)
    out = []
    for how in ("track", "setter"):
        s, prob, x0, ui = _handle(B, task=how == "track", early_exit=early_exit)
        if how == "track":
            s.set_al_task_bounds_track(track); s.set_al_bounds_track_starts(starts)
            s.al_bounds_window_from_track(0)                      # (an earlier cut must leave no trace)
            s.al_bounds_window_from_track(step)
        else:
            s.set_al_task_bounds(want_win, AL["rho_task0"], AL["tol_task"])
        s.initialize(x0, ui)
        if how == "track":                                         # the track survives the initialisers and set_al_multipliers
            s.set_al_multipliers(None, None, np.tile([AL["rho_joint0"], AL["rho_ctrl0"]], (B, 1)))
            assert s.al_task_bounds_track_rows() == ROWS and np.array_equal(s.al_task_bounds(), want_win)
        quad, total = _stage(s)
        s.initialize(x0, ui)
        cost = s.solve(x0)
        out.append((quad, total, _al_observables(s, cost)))
        s.close()
    (qa, ta, (oa, ea)), (qb, tb, (ob, eb)) = out
    for n in NAMES:
        assert np.array_equal(qa[n], qb[n]), n
    assert np.array_equal(ta, tb)
    lc.assert_same(oa, ob)
    for k in ea:
        assert np.array_equal(ea[k], eb[k], equal_nan=True), k
    # the bounds are felt: the schedule has feet in swing under a floor above the standing ankle height
    print("task violation at the end %s, largest task multiplier %.3g" % (ea["viol_t"], ea["mu_t"].max()))
    assert ea["mu_t"].max() > 0.0 or ea["task_trace"][0, :, 0].max() > 0.0


def test_refusals_leave_the_handle_usable():
    from mpc_ilqr_mujoco_amd import solver as sv
    B = tc.B_SMALL
    track = tc.task_track()
    s, prob, x0, ui = _handle(B, task=False)
    # without a task family: ILQR_ERR_STATE, from the setter and (a track left over from an earlier installation) from the cut
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.set_al_task_bounds_track(track)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.al_bounds_window_from_track(0)                          # no track of either kind
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.set_al_bounds_track_starts([0])
    s.set_al_task_bounds(tc.install_window(), AL["rho_task0"], AL["tol_task"])
    s.set_al_task_bounds_track(track)
    s.set_al_bounds_track_starts([1])                             # accepted with the task track alone
    nan, up, dn, cross = (np.array(track) for _ in range(4))
    nan[2, 5] = np.nan; up[0, 3] = np.inf; dn[ROWS - 1, 9 + 7] = -np.inf; cross[1, 2] = 3.0; cross[1, 11] = 2.5
    for bad in (nan, up, dn, cross):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_al_task_bounds_track(bad)
    assert s.L.ilqr_hip_set_al_task_bounds_track(s.h, 0, track.ctypes.data_as(sv.C.POINTER(sv.C.c_double))) == ERR_ARG
    assert s.L.ilqr_hip_set_al_task_bounds_track(s.h, ROWS, None) == ERR_ARG
    with pytest.raises(ValueError):
        s.set_al_task_bounds_track(track[:, :17])
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        s.al_bounds_window_from_track(-1)
    # every refusal left the installed track and its starts as they were
    assert s.al_task_bounds_track_rows() == ROWS
    s.al_bounds_window_from_track(2)
    assert np.array_equal(s.al_task_bounds(), kr.cut(track, [1], 2, N, B))
    # the task family goes, the track stays: the cut refuses; the family comes back: it cuts again
    s.clear_al_task_bounds()
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.al_bounds_window_from_track(0)
    assert s.al_task_bounds_track_rows() == ROWS
    s.set_al_task_bounds(tc.install_window(), AL["rho_task0"], AL["tol_task"])
    s.al_bounds_window_from_track(0)
    assert np.array_equal(s.al_task_bounds(), kr.cut(track, [1], 0, N, B))
    # without an augmented Lagrangian
    s.clear_augmented_lagrangian()
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.set_al_task_bounds_track(track)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.al_bounds_window_from_track(0)
    s.clear_al_task_bounds_track()
    assert s.al_task_bounds_track_rows() == 0
    # ... and the handle still solves
    s.initialize(x0, ui)
    assert np.all(np.isfinite(s.solve(x0)))
    s.close()


def test_resident_runner_cuts_the_task_track_like_the_loop_driven_by_hand():
    """MPCRunner(resident=True, device_refs=True, track_starts=...) under a task track, two steps, against the same runner whose solver's cut
    is replaced by set_al_task_bounds of the NumPy cut: states and controls bit for bit; the runner cuts once per solve with the step index
    of its reference windows and feeds track_starts to the shared start rows"""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    from mpc_ilqr_mujoco_amd import solver as sv
    B, steps = 2, 2
    base = sc.make_problem(sv.reference_kinematics, N=N)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (40, 1))); rd.contact = np.ones((40, 2), dtype=np.int32); rd.contact[:, 1] = 0
    x0, ui = sc.synthetic_batch(B, N, 44, _ug())
    track = tc.active_track()
    starts = [0, 2]
    runs, calls = {}, []
    for how in ("track", "setter", "none"):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(atc.MAX_ITER); s.set_contact_mode(2); s.set_augmented_lagrangian(**atc.al_args())
        if how != "none":
            s.set_al_task_bounds(tc.install_window(), AL["rho_task0"], AL["tol_task"])
        if how == "track":
            s.set_al_task_bounds_track(track)
        elif how == "setter":
            s.al_task_bounds_track_rows = lambda: ROWS
            s.set_al_bounds_track_starts = lambda st: calls.append(("starts", list(st)))
            s.al_bounds_window_from_track = lambda step, s=s: (calls.append(step), s.set_al_task_bounds(kr.cut(track, starts, step, N, B), AL["rho_task0"], AL["tol_task"]))
        r = ml.MPCRunner(s, rd, base, resident=True, device_refs=True, track_starts=starts)
        xs, us = r.run(x0, steps, u_init=ui)
        if how != "none":
            assert np.array_equal(s.al_task_bounds(), kr.cut(track, starts, steps - 1, N, B)) and s.num_al_task_bound_sets() == B, how
        s.close()
        runs[how] = (np.asarray(xs), np.asarray(us))
    assert calls == [("starts", starts)] + list(range(steps)), calls
    for a_, b_ in zip(runs["track"], runs["setter"]):
        assert np.array_equal(a_, b_)
    felt = not np.array_equal(runs["track"][1], runs["none"][1])
    print("resident loop under a task track: plan differs from the loop without one: %s" % felt)
    assert felt and np.all(np.isfinite(runs["track"][0]))
