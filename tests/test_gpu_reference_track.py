"""Reference windows cut from a track on the device (include/ilqr_hip.h ilqr_hip_set_reference_track / ilqr_hip_window_from_track;
csrc/reference_track_kernels.hip k_window_from_track).

Yardstick: references.ReferenceData.problem_at_starts, the host statement of the rule (checked against problem_at rollout by rollout in
tests/test_reference_track_cpu.py), uploaded through the three reference setters that existed before.  The feature moves bytes: EVERY
comparison is bit for bit, and no tolerance is involved.

T = 200 walking rows, N = 6, two iterations, B = 70 (two 64-lane chunks, the second with 6 rollouts) as tests/test_gpu_plant_score.py;
the inputs and the CPU-side proof that they reach the clamp and the end of the contact table are tests/reference_track_cases.py."""
import ctypes as C

import numpy as np
import pytest

import reference_track_cases as rc
from conftest import load_package
from test_gpu_plant import DT, NU, NX, _sv

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
T, N, B, KEYS = rc.T, rc.N, rc.B, rc.KEYS
ITERS = 2
OK, ERR_ARG, ERR_STATE = 0, 1, 4
_Q, _R, _ = sc.build_cost_matrices()
SCORE = dict(Q=0.37 * _Q + 1.0, R=0.05 + 0.01 * np.arange(NU), upright=7.0, balance=11.0, joint_limits=900.0, control_limits=1300.0)


def _handle(mode=0):
    s = _sv().BatchedILQR(B, N=N, dt=DT)
    s.set_max_iterations(ITERS)
    s.set_contact_mode(mode)
    return s


def _tracked(rd, starts, mode=0):
    s = _handle(mode)
    s.set_problem_constants(rc.base_problem())
    s.set_reference_track(rd)
    s.set_track_starts(starts)
    return s


def _same_windows(win, prob):
    """the getter's B windows against a problem's sets (one, or one per rollout)"""
    return all(win[k].dtype == prob[k].dtype and np.array_equal(win[k], np.broadcast_to(prob[k], win[k].shape)) for k in KEYS)


def _initial(rd, starts, seed):
    """scenario.walking_batch's initial states and controls on the rows `starts`"""
    rng = np.random.default_rng(seed)
    x0 = rd.x_ref[starts].copy()
    x0[:, 7:26] += rng.uniform(-0.02, 0.02, (B, 19)); x0[:, 0:3] += rng.uniform(-0.01, 0.01, (B, 3)); x0[:, 26:] *= 0.5
    ug = _sv().gravity_compensation(sc.standing_state(), rc.GRAVITY)
    return x0, np.tile(ug, (B, N, 1)) + rng.uniform(-0.5, 0.5, (B, N, 19))


def _solution(s):
    return s.trace() + (s.xbar(), s.ubar(), s.gains_K(), s.gains_kff())


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("follow", [False, True])
@pytest.mark.parametrize("shared", [False, True])
def test_windows_are_the_host_rule_bit_for_bit(shared, follow):
    rd, base = rc.track(rc.CONTACT_ROWS), rc.base_problem()
    per = rc.starts_for(follow)
    rc.check_starts_reach_the_edges(rd, per, follow)      # on the CPU, before the GPU is touched
    starts = np.array([141 if follow else 195]) if shared else per      # shared: crosses the table's end / clamps from t = 5 on
    want = {step: rd.problem_at_starts(starts, step, N, base, follow_schedule=follow) for step in rc.STEPS}
    if shared:
        w = want[rc.STEPS[-1]]
        assert (not follow and np.array_equal(w["x_ref"][0, -1], w["x_ref"][0, -2])) or (follow and (w["stance"] == 0).any() and np.all(w["stance"][0, -1] == 1))
    s = _tracked(rd, starts)
    assert s.reference_track_rows() == T
    for step in rc.STEPS + (0,):      # (and back: nothing of step 3 is left behind)
        s.window_from_track(step, follow)
        win = s.reference_windows()
        assert all(win[k].shape[0] == B for k in KEYS)
        assert _same_windows(win, want[step]), (step, [k for k in KEYS if not np.array_equal(win[k], np.broadcast_to(want[step][k], win[k].shape))])
    assert not _same_windows(win, want[3])
    # a second track replaces the first and returns to one shared start of 0; the windows stay where they are until the next call
    rd2 = rc.track()
    s.set_reference_track(rd2)
    assert _same_windows(s.reference_windows(), want[0])
    s.window_from_track(2, follow)
    assert _same_windows(s.reference_windows(), rd2.problem_at_starts([0], 2, N, base, follow_schedule=follow))
    s.clear_reference_track()
    assert s.reference_track_rows() == 0
    assert _same_windows(s.reference_windows(), rd2.problem_at_starts([0], 2, N, base, follow_schedule=follow))      # what was written stays
    s.close()


def test_the_getter_reads_what_a_host_setter_wrote():
    rd, base = rc.track(rc.CONTACT_ROWS), rc.base_problem()
    s = _handle()
    shared = rd.problem_at(40, N, base, follow_schedule=True)
    s.set_problem(shared)
    assert _same_windows(s.reference_windows(), shared)
    stacked = rd.problem_at_starts(rc.starts_for(True), 3, N, base, follow_schedule=True)
    s.set_problem(stacked)
    assert _same_windows(s.reference_windows(), stacked)
    # mixed strides: a shared schedule under per-rollout state references
    mixed = dict(stacked); mixed.update({k: shared[k] for k in ("stance", "ee_ref", "com_vel_ref")})
    s.set_problem(mixed)
    assert _same_windows(s.reference_windows(), mixed)
    s.close()


def test_refusals_come_before_anything_is_launched():
    rd, base = rc.track(rc.CONTACT_ROWS), rc.base_problem()
    s = _handle()
    L, h = s.L, s.h
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    zero = np.zeros(B, dtype=np.int32)
    s.set_problem(rd.problem_at(10, N, base))
    before = s.reference_windows()
    assert L.ilqr_hip_reference_track_rows(h) == 0
    assert L.ilqr_hip_window_from_track(h, 0, 0) == ERR_STATE and "track" in L.ilqr_hip_last_error(h).decode()
    assert L.ilqr_hip_set_track_starts(h, ip(zero), B) == ERR_STATE
    x = np.zeros((1, NX))
    assert L.ilqr_hip_set_reference_track(h, 0, x.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, None, 0) == ERR_ARG      # rows < 1
    s.set_reference_track(rd)
    neg = zero.copy(); neg[B - 1] = -1
    assert L.ilqr_hip_set_track_starts(h, ip(neg), B) == ERR_ARG                                      # a negative start
    for n in (0, 2, B - 1, B + 1):
        assert L.ilqr_hip_set_track_starts(h, ip(zero), n) == ERR_ARG                                # n_sets not in {1, B}
    assert L.ilqr_hip_window_from_track(h, -1, 0) == ERR_ARG                                         # a negative step
    st = zero.copy(); st[B - 1] = T - N - 3
    assert L.ilqr_hip_set_track_starts(h, ip(st), B) == OK
    assert L.ilqr_hip_window_from_track(h, 3, 1) == ERR_ARG and "beyond" in L.ilqr_hip_last_error(h).decode()      # row T of the foot references
    with pytest.raises(IndexError):
        rd.problem_at_starts(st, 3, N, base, follow_schedule=True)                                   # ... where the host rule raises
    assert _same_windows(s.reference_windows(), before)                                              # none of them wrote anything
    assert L.ilqr_hip_window_from_track(h, 2, 1) == OK                                               # the last row allowed
    assert _same_windows(s.reference_windows(), rd.problem_at_starts(st, 2, N, base, follow_schedule=True))
    assert L.ilqr_hip_window_from_track(h, 3, 0) == OK                                               # horizon-local rows: the same step is fine
    assert _same_windows(s.reference_windows(), rd.problem_at_starts(st, 3, N, base))
    s.close()


@pytest.mark.parametrize("follow", [False, True])
def test_the_solve_on_track_windows_is_the_solve_on_uploaded_windows(follow):
    rd, base = rc.track(rc.CONTACT_ROWS), rc.base_problem()
    starts = rc.starts_for(follow)
    x0, ui = _initial(rd, np.minimum(starts, T - 1), 43)
    H = _handle(mode=2)
    H.set_problem(rd.problem_at_starts(starts, 3, N, base, follow_schedule=follow))
    D = _tracked(rd, starts, mode=2)
    D.window_from_track(3, follow)
    for s in (H, D):
        s.initialize(x0, ui)
        s.solve(x0)
    h, d = _solution(H), _solution(D)
    assert _same(h, d)
    assert np.all(np.isfinite(H.cost())) and np.all(np.isfinite(h[3])) and (h[1] > 0.0).any()      # the solves did something: steps were accepted
    assert not np.array_equal(h[3][63], h[3][64])
    H.close(); D.close()


def _explicit_loop(rd, base, starts, x0, ui, steps, m):
    """the resident loop with host-stacked windows per solve (the pattern of test_contact_mode_2_on_the_advancing_schedule)"""
    E = _handle(mode=2)
    E.plant_configure(2, 0, "schedule")
    E.plant_set_history(steps)
    E.plant_set_score(**SCORE)
    E.plant_reset(x0)
    stood = []
    for k in range(0, steps, m):
        E.set_problem(rd.problem_at_starts(starts, k, N, base, follow_schedule=True))
        if k == 0:
            E.initialize(x0, ui); E.solve(x0)
        else:
            E.initialize_warm_from_plant(shift=m); E.solve(None)
        if m == 1:
            E.plant_advance()
        else:
            E.plant_follow(0, m)
        stood.append(E.plant_stance())
    hx, hu = E.plant_history()
    out = (hx, hu, E.plant_state(), E.plant_stance(), E.plant_alive(), E.plant_score())
    E.close()
    return out, stood


@pytest.mark.parametrize("solve_every", [1, 2])
def test_runner_with_device_references_is_the_loop_with_uploaded_windows(solve_every):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    rd, base = rc.track(rc.CONTACT_ROWS), rc.base_problem()
    steps = 4
    starts = rc.starts_for(True)      # start + 3 + N <= T - 1: four steps of the advancing schedule fit
    rows = np.array([[rd.is_stance(e, int(s) + k) for e in range(2)] for k in range(steps) for s in starts]).reshape(steps, B, 2)
    assert (rows != rows[0]).any() and 0 < rows.sum() < rows.size      # the schedule row under the plant advances, both kinds of flag occur
    x0, ui = _initial(rd, starts, 44)
    (hx, hu, xf, stf, alive, rec), stood = _explicit_loop(rd, base, starts, x0, ui, steps, solve_every)
    s = _handle(mode=2)
    run = ml.MPCRunner(s, rd, base, follow_schedule=True, resident=True, substeps=2, solve_every=solve_every, score=SCORE, device_refs=True, track_starts=starts)
    xs, us = run.run(x0, steps, u_init=ui)
    assert np.array_equal(xs[:steps], hx) and np.array_equal(us, hu) and np.array_equal(xs[steps], xf)
    assert np.array_equal(s.plant_stance(), stf) and np.array_equal(s.plant_alive(), alive) and np.array_equal(run.score(), rec)
    assert np.array_equal(run.last_stance0, rows[steps - solve_every, 0].astype(np.int32))
    # the run is a run: every rollout alive and finite, the plant moved, the flags it stood on changed, the score counted every interval
    assert np.all(alive == 1) and np.all(np.isfinite(xs)) and np.abs(xs[steps] - x0).max() > 1e-3
    assert any((st != stood[0]).any() for st in stood[1:]) and np.all(rec[:, 7] == steps) and np.all(rec[:, 0] > 0.0)
    # the windows the last solve read are those of its step, cut on the device
    assert _same_windows(s.reference_windows(), rd.problem_at_starts(starts, steps - solve_every, N, base, follow_schedule=True))
    run.close(); s.close()


def test_a_host_setter_overwrites_what_the_track_wrote():
    rd, base = rc.track(rc.CONTACT_ROWS), rc.base_problem()
    starts = rc.starts_for(True)
    shared = rd.problem_at(25, N, base, follow_schedule=True)
    x0, ui = _initial(rd, np.full(B, 25), 45)
    D = _tracked(rd, starts, mode=2)
    D.window_from_track(3, True)
    D.set_problem(shared)
    H = _handle(mode=2)
    H.set_problem(shared)
    assert _same_windows(D.reference_windows(), shared)
    for s in (H, D):
        s.initialize(x0, ui)
        s.solve(x0)
    assert _same(_solution(H), _solution(D)) and np.all(np.isfinite(H.cost()))
    H.close(); D.close()


def test_logged_reference_rows_are_each_logged_rollouts_own(tmp_path):
    """with logs on, the reference columns of mpc_log.csv come from the host's copy of the rule, for the logged rollouts only"""
    import os
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    rd, base = rc.track(rc.CONTACT_ROWS), rc.base_problem()
    steps, logged = 3, (0, 65)
    starts = rc.starts_for(True)
    assert starts[logged[0]] != starts[logged[1]]
    x0, ui = _initial(rd, starts, 46)
    s = _handle(mode=2)
    run = ml.MPCRunner(s, rd, base, log_dir=str(tmp_path), log_rollouts=logged, follow_schedule=True, resident=True, device_refs=True, track_starts=starts)
    xs, us = run.run(x0, steps, u_init=ui)
    run.close(); s.close()
    six = lambda a: np.array([float("%.6g" % v) for v in a])
    for b in logged:
        rows = np.genfromtxt(os.path.join(str(tmp_path), "rollout_%d" % b, "mpc_log.csv"), delimiter=",", skip_header=1)
        assert rows.shape == (steps, 4 + 2 * (NX + NU))
        for k in range(steps):
            assert np.array_equal(rows[k, 4:4 + NX], six(xs[k, b])) and np.array_equal(rows[k, 4 + NX:4 + NX + NU], six(us[k, b]))
            assert np.array_equal(rows[k, 4 + NX + NU:4 + 2 * NX + NU], six(rd.x_ref[starts[b] + k]))
            assert np.array_equal(rows[k, 4 + 2 * NX + NU:], six(rd.u_ref[starts[b] + k]))
