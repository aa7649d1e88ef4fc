"""The task score of the resident plant on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_task_score, csrc/plant_task_score_kernels.hip).

Yardstick of the values: tests/plant_task_score_ref.py (NumPy on al_task_ref.points, checked on the CPU by tests/test_al_task_track_cpu.py)
applied to the rows of the downloaded history ring.  Slots 0..2 to 1e-12 m -- what tests/test_gpu_al_task.py holds the points to --, slot 6
to 1e-12 scaled by its own magnitude, the counts exact.  The counts compare V_g with tol and a side with its bound; the case set keeps
every such decision at least 1e-6 away from equality (asserted on the CPU for the plant's initial state, and again here, on the
reference's side, for the rows the plant produced), so 1e-12 on a point cannot flip one.  Where two compositions of the same kernels are
compared the comparison is bit for bit.

N = 4, two iterations; B = 70: two 64-lane chunks per interval, the second with 6 rollouts.  The handle SOLVES under a task window without
bounds and is given the scored window afterwards: the score reads the window the handle holds when the plant is called."""
import ctypes as C

import numpy as np
import pytest

import al_task_cases as atc
import al_task_ref as tr
import al_task_track_cases as tc
import plant_task_score_ref as pts
from test_gpu_plant import _sv
from test_gpu_plant_score import SCORE

pytestmark = pytest.mark.gpu

sc = tc.sc
N, B, DT = tc.N, tc.B_WAVE, tc.DT
NX, NQ = tc.NX, tc.NQ
AL = atc.AL_E2E
ITERS = 2
ERR_STATE = 4


def _ug():
    return _sv().gravity_compensation(sc.standing_state(), (0.0, 0.0, -9.81))


def _solved(ring=3, xp=None, task=True, tol=tc.TOL, score_window=True):
    """a handle that has solved score_problem() under AL (and a task window without bounds) and carries the plant at xp (default x0), with
    the scored window of score_case() installed afterwards; two calls give twins"""
    sv = _sv()
    prob, x0, ui, win, P0, _ = tc.score_case()
    A = sv.BatchedILQR(B, N=N, dt=DT)
    A.set_contact_mode(2); A.set_max_iterations(ITERS)
    A.plant_configure(1, 0, "schedule"); A.plant_set_history(ring)
    A.set_problem(prob)
    A.set_augmented_lagrangian(**atc.al_args())
    if task:
        A.set_al_task_bounds(tc.install_window(), AL["rho_task0"], AL["tol_task"])
    x0 = np.array(x0)
    A.initialize(x0, tc.u_init(ui, _ug())); A.solve(x0)
    if task and score_window:
        A.set_al_task_bounds(win, AL["rho_task0"], AL["tol_task"])
    if tol is not None:
        A.plant_set_task_score(tol)
    A.plant_reset(x0 if xp is None else xp)
    return A


def _plant(A):
    return A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()


def _same(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def _rows(first, count):
    """(window rows, schedule rows) [count, B, .] of the knots first .. first + count - 1 of score_case()"""
    prob, _, _, win, _, _ = tc.score_case()
    k = slice(first, first + count)
    return np.moveaxis(win[:, k], 1, 0), np.moveaxis(prob["stance"][:, k], 1, 0)


def _check(got, hx, w, st, what, tol=tc.TOL):
    P = tr.points(hx)
    side, decision = pts.margins(P, w, st, tol)
    want = pts.fold(np.zeros((hx.shape[1], 8)), pts.interval_terms(P, w, st, tol))
    d = np.abs(got - want)
    print("%s: worst error slots 0..2 %.2e m, slot 6 %.2e; smallest |p - bound| %.2e m, smallest |V_g - tol| %.2e m" % (what, np.nanmax(d[:, :3]), np.nanmax(d[:, 6]), side, decision))
    assert side >= 1e-6 and decision >= 1e-6, (what, side, decision)          # (a condition on the inputs, stated on the reference's side)
    ok = pts.close_enough(got, want)
    assert ok.all(), (what, np.argwhere(~ok)[:8].tolist(), got[~ok][:4], want[~ok][:4])
    return want


def test_record_matches_the_reference_over_a_three_interval_follow():
    prob, x0, ui, win, P0, excited = tc.score_case()
    A = _solved()
    assert np.array_equal(A.plant_task_score(), np.zeros((B, 8)))
    A.plant_kick(tc.kick())
    A.plant_follow(0, 3)
    got = A.plant_task_score()
    hx, hu = A.plant_history()
    assert hx.shape == (3, B, NX) and np.all(A.plant_alive() == 1) and np.all(np.isfinite(hx))
    assert np.array_equal(hx[0][:, :NQ], x0[:, :NQ])                         # row 0: the initial configuration, whose points place the windows
    moved = np.abs(tr.points(hx[2]) - tr.points(hx[0])).max(axis=1)
    print("largest displacement of a point over the call, per rollout: %.2e .. %.2e m" % (moved.min(), moved.max()))
    assert np.all(moved > 1e-9), moved.min()                                 # the points move: rows 1 and 2 are not row 0 again
    w, st = _rows(0, 3)
    want = _check(got, hx, w, st, "follow(0, 3)")
    assert np.all(got[:, 7] == 3.0)
    # non-vacuity on the reference's side: every group violated and counted somewhere, in both chunks; violations below the tolerance too
    assert np.all((want[:, :3] > 0).sum(axis=0) > 0) and np.all(want[:, 3:6].sum(axis=0) > 0) and want[64:, :3].max() > 0
    assert ((want[:, :3].max(axis=1) > 0) & (want[:, 3:6].sum(axis=1) == 0)).any()
    # the record is that of ITS rows: other knots' window rows, another rollout's window, the stance rule dropped -- each is another record
    for other_w, other_st in ((np.roll(w, 1, axis=0), st), (np.roll(w, 1, axis=1), st), (w, np.zeros_like(st))):
        other = pts.fold(np.zeros((B, 8)), pts.interval_terms(tr.points(hx), other_w, other_st, tc.TOL))
        assert not pts.close_enough(got, other).all()
    p = C.c_void_p()
    assert A.L.ilqr_hip_plant_task_score_device(A.h, C.byref(p)) == 0 and p.value
    A.close()


def test_fusing_changes_nothing_and_advance_scores_row_0():
    """one advance, then follow(0, 3) on a ring of three rows (the call wraps inside the ring) against follow(j, 1)"""
    A, T = (_solved(ring=3) for _ in range(2))
    for s in (A, T):
        s.plant_kick(tc.kick())
        s.plant_advance()
    one = A.plant_task_score()
    hx0 = A.plant_history()[0]
    w0, st0 = _rows(0, 1)
    _check(one, hx0, w0, st0, "advance")                                     # row 0 of window and schedule
    assert np.all(one[:, 7] == 1.0)
    A.plant_follow(0, 3)
    for j in range(3):
        T.plant_follow(j, 1)
    a, t = A.plant_task_score(), T.plant_task_score()
    assert np.array_equal(a, t) and np.all(a[:, 7] == 4.0) and np.all(np.isfinite(a))
    assert _same(_plant(A), _plant(T)) and _same(A.plant_history(), T.plant_history())
    # ... and the four intervals are the reference's: the ring holds the last three, folded onto the advance's record
    hx = A.plant_history()[0]
    w, st = _rows(0, 3)
    want = pts.fold(one, pts.interval_terms(tr.points(hx), w, st, tc.TOL))
    assert pts.close_enough(a, want).all()
    A.close(); T.close()


def test_lifecycle_clear_and_both_scores():
    sv = _sv()
    prob, x0, ui, win, P0, _ = tc.score_case()
    x0 = np.array(x0)
    out = np.zeros((B, 8)); dp = out.ctypes.data_as(C.POINTER(C.c_double)); p = C.c_void_p()
    A, T = _solved(ring=3), _solved(ring=3, tol=None)                       # T never has the task score
    assert T.L.ilqr_hip_plant_get_task_score(T.h, dp) == ERR_STATE and T.L.ilqr_hip_plant_task_score_device(T.h, C.byref(p)) == ERR_STATE
    for bad in (-1e-9, np.inf, np.nan):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_task_score(bad)
    # both scores installed: the cost score's record is bitwise what it is alone
    A.plant_set_score(**SCORE); T.plant_set_score(**SCORE)
    for s in (A, T):
        s.plant_kick(tc.kick()); s.plant_advance(); s.plant_follow(1, 2)
    assert np.array_equal(A.plant_score(), T.plant_score()) and np.all(A.plant_score()[:, 7] == 3.0)
    rec = A.plant_task_score()
    assert np.all(rec[:, 7] == 3.0) and rec[:, :3].max() > 0
    assert _same(_plant(A), _plant(T)) and _same(A.plant_history(), T.plant_history())
    # set_task_score and plant_reset empty the record; the same intervals from the same state give the same record
    A.plant_set_task_score(tc.TOL)
    assert np.array_equal(A.plant_task_score(), np.zeros((B, 8)))
    A.plant_advance()
    assert np.all(A.plant_task_score()[:, 7] == 1.0)
    A.plant_reset(x0); T.plant_reset(x0)
    assert np.array_equal(A.plant_task_score(), np.zeros((B, 8)))
    for s in (A, T):
        s.plant_kick(tc.kick()); s.plant_advance(); s.plant_follow(1, 2)
    assert np.array_equal(A.plant_task_score(), rec)
    # another tolerance: the same maxima and sum, other counts
    A.plant_set_task_score(0.5 * tc.SMALL); A.plant_reset(x0); T.plant_reset(x0)
    for s in (A, T):
        s.plant_kick(tc.kick()); s.plant_advance(); s.plant_follow(1, 2)
    low = A.plant_task_score()
    assert np.array_equal(low[:, [0, 1, 2, 6, 7]], rec[:, [0, 1, 2, 6, 7]]) and low[:, 3:6].sum() > rec[:, 3:6].sum()
    # after clear: states and controls bitwise those of the handle that never had it, and the getters refuse
    A.plant_clear_task_score()
    assert A.L.ilqr_hip_plant_get_task_score(A.h, dp) == ERR_STATE and A.L.ilqr_hip_plant_task_score_device(A.h, C.byref(p)) == ERR_STATE
    A.plant_clear_task_score()                                               # (again: nothing to do)
    for s in (A, T):
        s.initialize_warm_from_plant(shift=3); s.solve(None); s.plant_advance(); s.plant_follow(1, 2)
    assert _same(_plant(A), _plant(T)) and _same(A.plant_history(), T.plant_history()) and np.array_equal(A.plant_score(), T.plant_score())
    A.close(); T.close()


def test_refusals_happen_before_any_launch():
    A = _solved(ring=2)
    A.plant_advance()
    def state():
        return _plant(A), A.plant_history(), A.plant_task_score(), A.plant_intervals()
    def same(a, b):
        return _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    before = state()
    assert before[3] == 1
    # three intervals do not fit a ring of two rows
    assert A.L.ilqr_hip_plant_follow(A.h, 0, 3) == ERR_STATE and "ring" in A.L.ilqr_hip_last_error(A.h).decode()
    assert same(before, state())
    # no task family: the plant calls refuse, the ring and the interval counter stay
    A.clear_al_task_bounds()
    assert A.L.ilqr_hip_plant_advance(A.h) == ERR_STATE and "task" in A.L.ilqr_hip_last_error(A.h).decode()
    assert A.L.ilqr_hip_plant_follow(A.h, 0, 2) == ERR_STATE
    assert same(before, state())
    # the family back: two intervals fit
    A.set_al_task_bounds(np.array(tc.score_case()[3]), AL["rho_task0"], AL["tol_task"])
    A.plant_follow(0, 2)
    assert np.all(A.plant_task_score()[:, 7] == 3.0) and A.plant_intervals() == 3
    # no ring at all
    A.plant_set_history(0)
    assert A.L.ilqr_hip_plant_advance(A.h) == ERR_STATE and "ring" in A.L.ilqr_hip_last_error(A.h).decode()
    assert np.all(A.plant_task_score()[:, 7] == 3.0) and A.plant_intervals() == 3
    # without the score the same calls are the parent's
    A.plant_clear_task_score()
    A.plant_advance(); A.synchronize()
    assert A.plant_intervals() == 4
    A.close()


def test_a_rollout_reset_to_a_nan_state_touches_no_other():
    """the pattern of tests/test_gpu_plant_score.py: arithmetic on a NaN, nothing that faults the device"""
    bad = 65      # in the partial chunk
    x0 = np.array(tc.score_case()[1])
    recs = {}
    for poisoned in (False, True):
        xp = x0.copy()
        if poisoned:
            xp[bad, 9] = np.nan                                              # a joint angle: every point of the rollout goes with it
        A = _solved(ring=3, xp=xp)
        A.plant_advance()
        A.plant_follow(1, 2)
        recs[poisoned] = (A.plant_task_score(), A.plant_alive(), A.plant_history()[0])
        A.close()
    rec, alive, hx = recs[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(alive[keep] == 1) and np.all(recs[False][1] == 1)
    assert np.array_equal(rec[keep], recs[False][0][keep]) and np.all(np.isfinite(rec[keep]))      # bit for bit
    assert np.all(np.isnan(hx[:, bad, 9]))
    assert np.isnan(rec[bad, 6]) and rec[bad, 7] == 3.0 and np.all(rec[bad, :6] == 0.0)
    assert np.isfinite(recs[False][0][bad]).all() and recs[False][0][bad, 7] == 3.0


def test_runner_scores_a_floor_raised_under_the_swing_foot():
    """MPCRunner(plant_contacts="geometry", plant_terrain=..., task_score=0.0): rollout 1's floor is raised by 5 cm under the right foot,
    which the schedule has in swing; each rollout's window holds the clearance floor of ITS terrain (2 cm below where the ankle would rest
    on it).  The true foot of rollout 1 is below that floor, the flat-floor rollout's foot is not; both against the reference applied to
    the downloaded ring."""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, steps, raised = 2, 3, 0.05
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (40, 1))); rd.contact = np.ones((40, 2), dtype=np.int32); rd.contact[:, 1] = 0
    x0 = np.tile(sc.standing_state(), (Bn, 1))
    ui = np.tile(sv.gravity_compensation(sc.standing_state(), base["gravity"]), (Bn, N, 1))
    z_rest = float(tr.points(x0[0])[8])
    win = sc.stack_al_task_bounds([dict(right_foot=((-np.inf, -np.inf, z_rest + h - 0.02), np.inf)) for h in (0.0, raised)], Bn, N)
    T = sc.stack_plant_terrain([dict(), dict(z_right=raised)], Bn)
    s = sv.BatchedILQR(Bn, N=N, dt=DT); s.set_contact_mode(2); s.set_max_iterations(ITERS)
    s.set_augmented_lagrangian(**atc.al_args())
    s.set_al_task_bounds(win, AL["rho_task0"], AL["tol_task"])
    run = ml.MPCRunner(s, rd, base, resident=True, plant_contacts="geometry", plant_terrain=T, task_score=0.0)
    xs, hu = run.run(x0, steps, u_init=ui)
    rec = run.task_score()
    assert np.array_equal(s.al_task_bounds(), win)
    run.close(); s.close()
    xs = np.asarray(xs)
    assert xs.shape == (steps + 1, Bn, NX) and np.all(np.isfinite(xs))
    hx = xs[:steps]
    # every solve's window is `win` and every interval is an advance: row 0 of window and schedule (left foot in stance, right in swing)
    w = np.tile(win[None, :, 0], (steps, 1, 1)); st = np.tile(np.array([1, 0], dtype=np.int32), (steps, Bn, 1))
    P = tr.points(hx)
    side, decision = pts.margins(P, w, st, 0.0)
    want = pts.fold(np.zeros((Bn, 8)), pts.interval_terms(P, w, st, 0.0))
    print("flat floor %s\nraised floor %s\nright ankle heights %s, floors %s; margins %.2e %.2e" % (rec[0], rec[1], P[:, :, 8].T.tolist(), win[:, 0, 8].tolist(), side, decision))
    assert side >= 1e-6 and decision >= 1e-6
    assert pts.close_enough(rec, want).all()
    assert np.all(rec[0, :7] == 0.0) and rec[0, 7] == steps                  # the flat-floor rollout scores nothing
    assert rec[1, 2] > 1e-3 and rec[1, 5] >= 1.0 and rec[1, 6] > 0.0 and np.all(rec[1, [0, 1, 3, 4]] == 0.0) and rec[1, 7] == steps
    with pytest.raises(ValueError):
        ml.MPCRunner(None, rd, base, task_score=0.0)                         # needs the resident plant
