"""The closed-loop score of the resident plant on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_score, csrc/plant_score_kernels.hip).

Yardstick of the values: the CPU oracle's computeTotalCost, one term of one interval at a time through the horizon-1 construction of
tests/plant_score_ref.py (checked on the CPU by tests/test_plant_score_cpu.py), evaluated at the rows of the history ring:
    |got - want| <= 1e-11 |want| + 1e-11 (that rollout's total over slots 0-5)
-- the 1e-11 tests/test_gpu_parity.py grants the same cost function against the same oracle.  Slots 6 and 7 are exact.  Where two
compositions of the same kernels are compared (fused against single intervals, a small ring against a large one, a twin without the score)
the comparison is bit for bit.

N = 6 and two iterations as tests/test_gpu_plant_follow.py; B = 70: two 64-lane chunks per interval, the second with 6 rollouts."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import plant_score_ref as ps
from conftest import load_package
from test_gpu_plant import DT, NQ, NU, NV, NX, _sv
from test_gpu_plant_follow import ITERS, N, _plant, _problem, _same, _solved

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
B = 70
ERR_STATE = 4
_Q, _R, _ = sc.build_cost_matrices()
# scoring weights: none equals the solver's (shipped Q, R = 0.001, upright 20, balance 30, joint / control limits 1500)
SCORE = dict(Q=0.37 * _Q + 1.0 + 0.1 * np.arange(NX), R=0.05 + 0.01 * np.arange(NU), upright=7.0, balance=11.0, joint_limits=900.0, control_limits=1300.0)
PUSHED = ((0, 1, 2, 63), (64, 65, B - 1))      # candidates for a plant that starts away from xbar_0, by 64-lane chunk (63 / 64: the boundary)


def _distinct_refs(prob, sets, seed):
    """reference rows that differ from knot to knot and, with sets = B, from rollout to rollout (the schedule stays the problem's)"""
    rng = np.random.default_rng(seed)
    p = dict(prob)
    shp = lambda k: (sets,) + prob[k].shape[1:]
    p["x_ref"] = prob["x_ref"][:1] + rng.uniform(-0.01, 0.01, shp("x_ref"))
    p["u_ref"] = rng.uniform(-1.0, 1.0, shp("u_ref"))
    p["com_ref"] = prob["com_ref"][:1] + rng.uniform(-0.01, 0.01, shp("com_ref"))
    p["ee_ref"] = prob["ee_ref"][:1] + rng.uniform(-0.02, 0.02, shp("ee_ref"))
    p["com_vel_ref"] = rng.uniform(-0.01, 0.01, shp("com_vel_ref"))
    return p


def _shared_weights(prob, b):
    """rollout b's weights of a problem that may carry per-rollout weight sets, as a shared-weight problem for the oracle"""
    p = dict(prob)
    for k, nd in (("Q", 1), ("R", 1), ("Qf", 1), ("task_weights", 1), ("w_joint", 0), ("w_ctrl", 0)):
        a = np.asarray(prob[k], dtype=np.float64)
        p[k] = a[b] if a.ndim > nd else prob[k]
    p["w_joint"], p["w_ctrl"] = float(p["w_joint"]), float(p["w_ctrl"])
    return p


def _pushed_plant(prob, x0, ui, mode):
    """Plant states for plant_reset: some rollouts start with hinge offsets large enough that the reported u = ubar_0 + K_0 (x - xbar_0)
    leaves the control range's 10 % margin (|u_i| > 0.8 of the range; the batch's own controls are clipped to exactly 0.8).  Chosen on the
    CPU with the oracle's solve of the same rollout: the offset runs along the signs of the row of K_0 with the largest hinge gain per
    range, grown until Oracle.compute_control reports |u_i| > 0.9 of the range (room for the two solves' difference).  A candidate whose
    gains are too small for an offset of 1.6 rad stays where it is; each 64-lane chunk must keep at least one.  (The free plant of contact
    mode 0 falls: its six-knot policy holds about one control range per radian, so its offsets are of that size; with stance rows 0.05-0.4.)"""
    xp = x0.copy()
    for chunk in PUSHED:
        done = 0
        for b in chunk:
            o = ol.Oracle(N, DT); o.set_problem(_shared_weights(prob, b), b); o.set_options(max_iter=ITERS); o.set_contact_mode(mode)
            o.initialize(x0[b], ui[b]); o.solve(x0[b])
            K0 = o.get("K")[0][:, 7:NQ]
            row = int(np.argmax(np.abs(K0).sum(axis=1) / sc.CTRLRANGE))
            for scale in (0.05, 0.1, 0.2, 0.4, 0.8, 1.2, 1.6):
                x = x0[b].copy(); x[7:NQ] += scale * np.sign(K0[row])
                if np.any(np.abs(o.compute_control(x)) > 0.9 * sc.CTRLRANGE):
                    xp[b] = x; done += 1
                    break
        assert done > 0, "no hinge offset up to 1.6 rad drives a control of rollouts %s past the margin" % (chunk,)
    return xp


def _check_record(got, want, what):
    ok, worst = ps.close_enough(got, want)
    print("%s: worst |got - want| / bound = %.3f; totals %.6e .. %.6e" % (what, worst, want[:, :6].sum(axis=1).min(), want[:, :6].sum(axis=1).max()))
    assert ok.all(), (what, worst, np.argwhere(~ok)[:8].tolist())
    assert np.array_equal(got[:, 6:], want[:, 6:]), what


CASES = {
    "mode0_shared_set": dict(mode=0, sets=1, wsets=False),
    "mode2_per_rollout_sets": dict(mode=2, sets=B, wsets=False),
    "mode0_weight_sets": dict(mode=0, sets=1, wsets=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_terms_match_the_oracle_term_by_term(case):
    cfg = CASES[case]
    sv = _sv()
    prob, x0, ui = _problem(B, 21, per_rollout_schedule=cfg["mode"] != 0)
    prob = _distinct_refs(prob, cfg["sets"], 22)
    if cfg["wsets"]:
        prob = sc.stack_weight_sets(prob, [dict(Q=prob["Q"] * (1.0 + 0.01 * b), w_joint=prob["w_joint"] + b) for b in range(B)])
    xp = _pushed_plant(prob, x0, ui, cfg["mode"])
    A = _solved(B, prob, x0, ui, mode=cfg["mode"], ring=4, xp=xp)
    assert A.num_weight_sets() == (B if cfg["wsets"] else 0)
    A.plant_set_score(**SCORE)
    A.plant_advance()
    A.plant_follow(1, 3)
    got = A.plant_score()
    hx, hu = A.plant_history()
    assert hx.shape == (4, B, NX) and np.all(A.plant_alive() == 1) and np.all(np.isfinite(hx)) and np.all(np.isfinite(hu))
    assert np.array_equal(hx[0], xp)
    orc = ps.IntervalOracle(DT)
    rows = [(prob, k) for k in range(4)]
    want = ps.expected_record(orc, rows, hx, hu, SCORE)
    # non-vacuity, on the oracle's side: every term is alive somewhere, the balance term in both chunks
    alive = (want[:, :6] != 0.0).sum(axis=0)
    print("rollouts with a non-zero term, by slot:", alive.tolist())
    assert np.all(alive > 0) and np.all(alive[:4] == B) and np.any(want[64:, 5] != 0.0) and np.any(want[:64, 5] != 0.0)
    _check_record(got, want, case)
    assert np.all(got[:, 7] == 4.0) and np.array_equal(got[:, 6], hx[:, :, 2].min(axis=0))
    # the record is not the solver's cost: the same rows under the solver's own weights
    base = _shared_weights(prob, 0)
    own = dict(Q=base["Q"], R=base["R"], upright=base["task_weights"][4], balance=base["task_weights"][5], joint_limits=base["w_joint"], control_limits=base["w_ctrl"])
    other = ps.expected_record(orc, rows, hx, hu, own)
    rel = np.abs(other[:, :6].sum(axis=1) - got[:, :6].sum(axis=1)) / np.abs(got[:, :6].sum(axis=1))
    assert np.all(rel > 1e-6), rel.min()
    if cfg["sets"] == B:      # ... nor that of another rollout's reference set
        assert not ps.close_enough(got, np.roll(want, 1, axis=0))[0].all()
    # the device pointer is the record
    p = C.c_void_p()
    assert A.L.ilqr_hip_plant_score_device(A.h, C.byref(p)) == 0 and p.value
    A.close()


def test_fusing_changes_nothing():
    """one advance, then follow(0, 3) on a ring of three rows -- the call's rows are 1, 2, 0: it wraps inside the call -- against follow(j, 1)"""
    prob, x0, ui = _problem(B, 23, per_rollout_schedule=True)
    prob = _distinct_refs(prob, B, 24)
    A, T = (_solved(B, prob, x0, ui, mode=2, ring=3) for _ in range(2))
    for s in (A, T):
        s.plant_set_score(**SCORE)
        s.plant_advance()
    A.plant_follow(0, 3)
    for j in range(3):
        T.plant_follow(j, 1)
    a, t = A.plant_score(), T.plant_score()
    assert np.array_equal(a, t) and np.all(a[:, 7] == 4.0) and np.all(np.isfinite(a)) and np.all(a[:, :2] > 0.0)
    assert _same(_plant(A), _plant(T)) and _same(A.plant_history(), T.plant_history())
    A.close(); T.close()


def test_ring_size_is_invisible():
    prob, x0, ui = _problem(B, 25)
    prob = _distinct_refs(prob, 1, 26)
    recs = []
    for ring in (2, 8):
        A = _solved(B, prob, x0, ui, ring=ring)
        A.plant_set_score(**SCORE)
        for k in range(5):
            if k:
                A.initialize_warm_from_plant(); A.solve(None)
            A.plant_advance()
        recs.append(A.plant_score())
        assert A.plant_history()[0].shape[0] == min(ring, 5)
        A.close()
    assert np.array_equal(recs[0], recs[1]) and np.all(recs[0][:, 7] == 5.0) and np.all(np.isfinite(recs[0]))


def test_scoring_changes_nothing_else():
    prob, x0, ui = _problem(B, 27, per_rollout_schedule=True)
    A, T = (_solved(B, prob, x0, ui, mode=2, substeps=2, ring=4) for _ in range(2))
    A.plant_set_score(**SCORE)
    dv = np.zeros((B, NV)); dv[:, 1] = 0.3
    for s in (A, T):
        s.plant_kick(dv)
        s.plant_advance()
        s.plant_follow(1, 2)
        s.initialize_warm_from_plant(shift=3); s.solve(None)
        s.plant_advance()
    assert np.all(A.plant_score()[:, 7] == 4.0)
    assert _same(_plant(A), _plant(T)) and _same(A.plant_history(), T.plant_history())
    assert np.array_equal(A.xbar(), T.xbar()) and np.array_equal(A.ubar(), T.ubar()) and np.array_equal(A.cost(), T.cost())
    assert _same(A.trace(), T.trace()) and np.array_equal(A.gains_K(), T.gains_K())
    A.close(); T.close()


def test_lifecycle_and_refusals():
    prob, x0, ui = _problem(B, 28)
    A = _solved(B, prob, x0, ui, ring=2)
    out = np.zeros((B, 8)); p = C.c_void_p()
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert A.L.ilqr_hip_plant_get_score(A.h, dp) == ERR_STATE and A.L.ilqr_hip_plant_score_device(A.h, C.byref(p)) == ERR_STATE
    empty = np.zeros((B, 8)); empty[:, 6] = np.inf
    A.plant_set_score(**SCORE)
    assert np.array_equal(A.plant_score(), empty)
    A.plant_advance()
    one = A.plant_score()
    assert np.all(one[:, 7] == 1.0) and np.array_equal(one[:, 6], x0[:, 2]) and np.all(one[:, 0] > 0.0)
    A.plant_set_score(**SCORE)      # again: the record is empty again
    assert np.array_equal(A.plant_score(), empty)
    A.plant_advance()
    A.plant_reset(x0)               # ... and so does a reset of the plant
    assert np.array_equal(A.plant_score(), empty)
    A.plant_advance()
    assert np.array_equal(A.plant_score(), one)      # the same interval from the same state
    # three intervals do not fit a ring of two rows: refused before anything moves
    before = (_plant(A), A.plant_history(), A.plant_score())
    assert A.L.ilqr_hip_plant_follow(A.h, 0, 3) == ERR_STATE
    assert "ring" in A.L.ilqr_hip_last_error(A.h).decode()
    after = (_plant(A), A.plant_history(), A.plant_score())
    assert _same(before[0], after[0]) and _same(before[1], after[1]) and np.array_equal(before[2], after[2])
    A.plant_follow(0, 2)            # two do
    assert np.all(A.plant_score()[:, 7] == 3.0)
    # no ring at all
    A.plant_set_history(0)
    assert A.L.ilqr_hip_plant_advance(A.h) == ERR_STATE and "ring" in A.L.ilqr_hip_last_error(A.h).decode()
    assert np.all(A.plant_score()[:, 7] == 3.0)
    # without the score the same calls are today's
    A.plant_set_history(2)
    A.plant_clear_score()
    assert A.L.ilqr_hip_plant_get_score(A.h, dp) == ERR_STATE
    A.plant_follow(0, 3)
    assert A.plant_history()[0].shape[0] == 2 and np.all(A.plant_alive() == 1)
    A.plant_set_history(0)
    A.plant_advance()
    A.synchronize()
    A.close()


def test_a_rollout_reset_to_a_nan_state_touches_no_other():
    """the pattern of tests/test_gpu_plant.py: arithmetic on a NaN, nothing that faults the device"""
    bad = 65      # in the partial chunk
    prob, x0, ui = _problem(B, 29)
    recs = {}
    for poisoned in (False, True):
        xp = x0.copy()
        if poisoned:
            xp[bad, 9] = np.nan
        A = _solved(B, prob, x0, ui, ring=3, xp=xp)
        A.plant_set_score(**SCORE)
        A.plant_advance()
        A.plant_follow(1, 2)
        recs[poisoned] = (A.plant_score(), A.plant_alive(), A.plant_history())
        A.close()
    rec, alive, (hx, hu) = recs[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(alive[keep] == 1) and np.all(recs[False][1] == 1)
    assert np.array_equal(rec[keep], recs[False][0][keep]) and np.all(np.isfinite(rec[keep]))      # bit for bit
    # its own record is what the ring dictates: every row logs the NaN state and zero control
    assert np.all(np.isnan(hx[:, bad, 9])) and np.all(hu[:, bad] == 0.0)
    assert np.isnan(rec[bad, 0]) and rec[bad, 7] == 3.0 and rec[bad, 6] == xp[bad, 2]
    assert np.isfinite(rec[bad, 1]) and rec[bad, 5] == 0.0      # (u = 0 against u_ref; no control penalty)


def _runner_refs(rows):
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    xs = np.tile(sc.standing_state(), (rows, 1))
    xs[:, 7:NQ] += np.random.default_rng(30).uniform(-0.02, 0.02, (rows, NQ - 7))      # the rows of the reference differ
    rd.set_states(xs); rd.contact = np.ones((rows, 2), dtype=np.int32)
    return rd


@pytest.mark.parametrize("solve_every", [1, 2])
def test_runner_returns_the_score_of_its_run(solve_every):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    sv = _sv()
    Br, steps = 70, 4
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = _runner_refs(40)
    x0, ui = sc.synthetic_batch(Br, N, 31, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    out = {}
    for rows in (None, solve_every):
        s = sv.BatchedILQR(Br, N=N, dt=DT); s.set_max_iterations(ITERS); s.set_contact_mode(2)
        run = ml.MPCRunner(s, rd, base, resident=True, solve_every=solve_every, score=SCORE, history_rows=rows)
        xs, hu = run.run(x0, steps, u_init=ui)
        out[rows] = (xs, hu, run.score())
        run.close(); s.close()
    xs, hu, rec = out[None]
    assert xs.shape == (steps + 1, Br, NX) and hu.shape == (steps, Br, NU) and np.all(np.isfinite(xs))
    windows = [rd.problem_at(t0, N, base) for t0 in range(0, steps, solve_every)]      # the windows problem_at gave the runner
    rows = [(windows[k // solve_every], k % solve_every) for k in range(steps)]
    assert not np.array_equal(windows[0]["x_ref"][0, 0], windows[0]["x_ref"][0, 1])
    want = ps.expected_record(ps.IntervalOracle(DT), rows, xs[:steps], hu, SCORE)
    _check_record(rec, want, "runner, solve_every %d" % solve_every)
    # a ring of one group: the same record bit for bit, and the rows the ring still holds
    xs2, hu2, rec2 = out[solve_every]
    assert np.array_equal(rec2, rec)
    assert xs2.shape == (solve_every + 1, Br, NX) and np.array_equal(xs2, xs[steps - solve_every:]) and np.array_equal(hu2, hu[steps - solve_every:])
