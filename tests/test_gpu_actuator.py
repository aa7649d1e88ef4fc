"""Actuator delay, lag and torque noise per rollout on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_actuator; csrc/plant_kernels.hip
k_actuator_draw, k_plant_follow_a of the module libilqr_hip_actuator.so).

Ground truth in two layers, neither of them the new kernels:
  * the draws against the golden of the NumPy restatement (tests/actuator_cases.py, tests/golden/gen_actuator_golden.py), which is held to
    the published Philox4x32-10 vectors on the CPU;
  * the plant kernels against the TEACHER-FORCED composition of entry points that existed before: per substep the host forms the command
    with compute_control at the interval's knot, runs the NumPy chain (delay line, lag, noise) with the handle's own beta rows and draws,
    and steps with step / step_stance (tests/plant_params_cases.py Yardstick; with every table installed step_payload) in the plant's mode.
B = 37 (two workgroups at feedback mode 0, ten at mode 1, the last one of a single rollout), N = 6, SUBSTEPS = 3: delays of 0..8 substeps lie
below, at and above an interval, and follow(0, 3) runs nine substeps, once round the nine slots of the delay line.

Bounds.  Draws: 1e-13 absolute, the bound of tests/test_gpu_observation.py for the same arithmetic.  Plant, from that file as well: state
2e-9 relative to max(1, max |want|) of the rollout, reported control U_TOL (1e-12), applied torque 1e-12 x max(1, |t|).
tests/test_actuator_cpu.py shows on the restatement that every wrong chain misses the torque bound by eleven orders of magnitude.

Measured on an MI355X, worst over the cases: draws 4.4e-16; plant state 4.9e-16, reported control 1.2e-13 relative, applied torque 5.4e-14;
with all five tables 4.3e-13, 1.0e-13 and 9.3e-15 (DESIGN 4.1 "An actuator")."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import actuator_cases as ac
import dynamics_envelope_cases as dc
import observation_cases as oc
import plant_params_cases as pc
import plant_score_ref as ps
from conftest import load_package
from test_gpu_payload import PayloadYardstick, _payload_table
from test_gpu_plant import U_TOL
from test_gpu_plant_params import CASES, HANDLE_MU, _problem, _states
from test_gpu_wrench import OWN, _same, _wrench_table

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU = 51, 19
B, N, DT, SUBSTEPS = pc.B, pc.N, pc.DT, 3
DRAW_TOL, X_TOL, T_TOL = 1e-13, 2e-9, 1e-12
SEED = 0xAC7_0A70_5EED
ZERO = np.zeros((1, 39))


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _solver(mode=0, limits=False, source="schedule", fb=0, ring=0, substeps=SUBSTEPS, rows=None):
    """the solving handle of tests/test_gpu_plant_params.py with three substeps; rows: a slice of the batch (a shard)"""
    sv = _sv()
    prob = _problem()
    if rows is not None:
        prob["stance"] = np.ascontiguousarray(prob["stance"][rows])
    A = sv.BatchedILQR(B if rows is None else len(prob["stance"]), N=N, dt=DT)
    A.set_contact_mode(mode); A.set_friction(HANDLE_MU); A.set_joint_limits(limits); A.set_max_iterations(1)
    A.plant_configure(substeps, fb, source)
    A.plant_set_history(ring)
    A.set_problem(prob)
    return A


class _ThreeSubsteps:
    """the yardstick's handles at h = DT / 3"""

    def handle(self, p):
        key = tuple(float(v) for v in p[:6])
        P = self.handles.get(key)
        if P is None:
            P = self.sv.BatchedILQR(B, N=N, dt=DT / SUBSTEPS)
            P.set_problem(self.sc.make_problem(self.sv.reference_kinematics, N=N, gravity=key[:3]))
            P.set_contact_mode(self.mode, key[4])
            P.set_friction(key[3])
            P.set_joint_limits(self.limits)
            P.set_joint_limit_stiffness(key[5])
            self.handles[key] = P
        return P


class Yardstick3(_ThreeSubsteps, pc.Yardstick):
    pass


class PayloadYardstick3(_ThreeSubsteps, PayloadYardstick):
    pass


def _rel(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def _state_err(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))).max())


# ---- 1: the draws
def test_draws_match_the_golden_and_do_not_depend_on_split_grouping_or_call():
    sv = _sv()
    g = ac.golden()
    rec, seed, count = g["records"], int(g["seed"]), int(g["count"])
    assert rec.shape[0] == B and count == N
    A = _solver()
    assert A.plant_num_actuator_sets() == 0
    none, s0, s1 = A.plant_get_actuator()
    assert np.array_equal(none, np.zeros((B, 39))) and (s0, s1) == (0, 0)
    A.plant_set_actuator(rec, seed=seed, stream0=0)
    back, s0, s1 = A.plant_get_actuator()
    assert A.plant_num_actuator_sets() == B and np.array_equal(back, rec) and (s0, s1) == (seed, 0)
    got = A.plant_actuator_draws(0, count)
    err = float(np.abs(got - g["z"]).max())
    print("draws against the golden: worst |error| %.3e (bound %.0e), largest |z| %.2f" % (err, DRAW_TOL, np.abs(got).max()))
    assert got.shape == (count, B, NU) and err < DRAW_TOL
    # beta as the host derived it: the restatement's expm1 to an ulp (libm), 1 where tau == 0
    beta = A.plant_actuator_blend()
    print("beta against the restatement: %.3e" % np.abs(beta - g["beta"]).max())
    assert np.abs(beta - g["beta"]).max() < 1e-15 and np.all(beta[rec[:, 1:20] == 0.0] == 1.0)
    assert np.array_equal(A.plant_actuator_draws(0, count), got)                                           # a second call: the same bits
    assert np.array_equal(A.plant_actuator_draws(2, 3), got[2:5]) and np.array_equal(A.plant_actuator_draws(5, 1), got[5:])      # call grouping
    # a batch of 37 with stream0 = 0 is handles of 20 and 17 with stream0 = 0 and 20
    for lo, hi in ((0, 20), (20, B)):
        P = sv.BatchedILQR(hi - lo, N=N, dt=DT)
        P.plant_set_actuator(rec[lo:hi], seed=seed, stream0=lo)
        assert np.array_equal(P.plant_actuator_draws(0, count), got[:, lo:hi]), (lo, hi)
        P.close()
    # the draws do not depend on the records; one record for all keeps one stream per rollout
    A.plant_set_actuator(rec[:1], seed=seed)
    assert A.plant_num_actuator_sets() == 1 and np.array_equal(A.plant_get_actuator()[0], np.repeat(rec[:1], B, axis=0))
    assert np.array_equal(A.plant_actuator_draws(0, count), got) and np.array_equal(A.plant_actuator_blend(), np.repeat(beta[:1], B, axis=0))
    # another seed, another stream0: other draws; a 64-bit seed and stream reach the generator whole
    A.plant_set_actuator(rec[:1], seed=seed ^ (1 << 40))
    assert not np.array_equal(A.plant_actuator_draws(0, 1), got[:1])
    A.plant_set_actuator(rec[:1], seed=seed, stream0=1 << 33)
    hi = A.plant_actuator_draws(0, 1)
    assert not np.array_equal(hi, got[:1]) and np.abs(hi - ac.draws(seed, 1 << 33, 0, 1, B)).max() < DRAW_TOL
    # beta follows the substeps of plant_configure
    A.plant_set_actuator(rec, seed=seed)
    A.plant_configure(2, 0, "schedule")
    assert np.abs(A.plant_actuator_blend() - ac.blend(rec, DT / 2)).max() < 1e-15 and A.plant_num_actuator_sets() == B
    A.close()


# ---- 2: the plant against the teacher-forced composition
def _interval(A, chain, step, z, x, fb, knot, delta=None):
    """one MPC interval from the state x: (x_next, reported command, stance, applied torque of the last substep).  The chain moves on."""
    xc, u, st, t = x.copy(), None, None, None
    for k in range(SUBSTEPS):
        if k == 0 or fb:
            u = A.compute_control(xc if delta is None else oc.boxplus(xc, delta), knot=knot)
        t = chain.substep(u, z)
        xc, st = step(xc, t)
    return xc, ac.guard(u), st, t


def _check(tag, mode, got, want, worst):
    (gx, gu, gst, gt), (wx, wu, wst, wt) = got, want
    ex, eu = _state_err(gx, wx), float(np.abs(gu - wu).max())
    et = None if gt is None else _rel(gt, wt)
    print("%s: state %.3e (bound %.0e)  |du| %.3e  applied %s (bound %.0e)" % (tag, ex, X_TOL, eu, "-" if et is None else "%.3e" % et, T_TOL))
    assert np.all(np.isfinite(wx)), tag
    assert np.allclose(gu, wu, **U_TOL), (tag, eu)
    assert ex < X_TOL, (tag, ex)
    if et is not None:
        assert et <= T_TOL, (tag, et)
    if mode and gst is not None:
        assert np.array_equal(gst, wst), tag
    worst["state"], worst["control"] = max(worst["state"], ex), max(worst["control"], _rel(gu, wu))
    if et is not None:
        worst["applied"] = max(worst["applied"], et)


def _teacher_forced(A, rec, step, x0, fb, mode, tag, delta_of=lambda j: None):
    """one advance, then -- from the reset -- a follow(0, 3), each interval held to the host composition from the state it started from"""
    worst = dict(state=0.0, control=0.0, applied=0.0)
    beta, z = A.plant_actuator_blend(), A.plant_actuator_draws(0, 3)
    A.plant_reset(x0)
    A.plant_advance()
    chain = ac.Chain(rec, beta)
    want = _interval(A, chain, step, z[0], x0, fb, 0, delta_of(0))
    # on the yardstick alone: the table moves what the joints get
    moved = np.abs(want[3] - want[1]).max(axis=1) > 1e-6
    per = [int(moved[k:k + (4 if fb else 32)].sum()) for k in range(0, B, 4 if fb else 32)]
    print("%s: the table moves the torque of %d rollouts, per workgroup %s" % (tag, int(moved.sum()), per))
    assert moved.sum() >= 25 and min(per) >= 1
    _check(tag + " advance", mode, (A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_get_applied()), want, worst)
    assert np.all(A.plant_alive() == 1) and A.plant_intervals() == 1
    A.plant_reset(x0)
    A.plant_follow(0, 3)
    hx, hu = A.plant_history()
    assert hx.shape == (3, B, NX) and np.array_equal(hx[0], x0) and np.all(A.plant_alive() == 1) and A.plant_intervals() == 3
    ends = [hx[1], hx[2], A.plant_state()]
    chain = ac.Chain(rec, beta)
    for j in range(3):
        last = j == 2
        got = (ends[j], hu[j], A.plant_stance() if last else None, A.plant_get_applied() if last else None)
        _check("%s follow interval %d" % (tag, j), mode, got, _interval(A, chain, step, z[j], hx[j], fb, j, delta_of(j)), worst)
    assert np.array_equal(A.plant_control(), hu[2]) and chain.n == 9
    return worst


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", ["free", "mode3_sliding", "mode4_limits"])
def test_plant_under_an_actuator_table_matches_the_host_composition(case, fb):
    mode, limits, source, group = CASES[case]
    sv = _sv()
    A = _solver(mode, limits, source=source, fb=fb, ring=3)
    Y = Yardstick3(sv, sc, mode, limits, source)
    x0, ui = _states(group)
    flags = pc.schedule()[:, 0]
    A.initialize(x0, ui); A.solve(x0)
    assert np.all(np.isfinite(A.ubar())) and np.all(np.isfinite(A.gains_K()))
    rec = ac.golden_records()
    A.plant_set_actuator(rec, seed=SEED)
    worst = _teacher_forced(A, rec, lambda x, u: Y.step(OWN, x, u, flags), x0, fb, mode, "%s fb%d" % (case, fb))
    print("%s fb%d: worst under the actuator table: state %.3e, reported control %.3e, applied torque %.3e" % (case, fb, worst["state"], worst["control"], worst["applied"]))
    A.close(); Y.close()


# ---- 3: all five tables
@pytest.mark.parametrize("fb", [0, 1])
def test_parameter_wrench_payload_observation_and_actuator_tables_together(fb):
    mode, limits, source, group = CASES["mode4_limits"]
    sv = _sv()
    A = _solver(mode, limits, fb=fb, ring=3)
    Y = PayloadYardstick3(sv, sc, mode, limits, source)
    x0, ui = _states(group)
    flags = pc.schedule()[:, 0]
    A.initialize(x0, ui); A.solve(x0)
    table, payload = pc.params(), _payload_table()
    wrench = _wrench_table(); wrench[:, 9] = 1.0; wrench[:, 10] = np.inf                                   # every window opens at interval 1
    rec = ac.golden_records()
    A.plant_set_params(table); A.plant_set_wrench(wrench); A.plant_set_payload(payload)
    A.plant_set_observation(oc.plant_records(B), seed=SEED + 1)
    A.plant_set_actuator(rec, seed=SEED)
    A.plant_reset(x0)
    delta = A.plant_observation_errors(0, 3)
    interval = [0]

    def step(xc, t):                                                                                       # (the gain on the host, inside step_m)
        j = interval[0]
        w9 = np.where(((wrench[:, 9] <= j) & (j < wrench[:, 10]))[:, None], wrench[:, :9], 0.0)
        return Y.step_m(table, xc, t, flags, w9, payload)

    worst = dict(state=0.0, control=0.0, applied=0.0)
    beta, z = A.plant_actuator_blend(), A.plant_actuator_draws(0, 3)
    tag = "all tables fb%d" % fb
    A.plant_advance()
    _check(tag + " advance", mode, (A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_get_applied()),
           _interval(A, ac.Chain(rec, beta), step, z[0], x0, fb, 0, delta[0]), worst)
    A.plant_reset(x0); A.plant_follow(0, 3)
    hx, hu = A.plant_history()
    ends = [hx[1], hx[2], A.plant_state()]
    chain = ac.Chain(rec, beta)
    for j in range(3):
        interval[0] = j
        got = (ends[j], hu[j], A.plant_stance() if j == 2 else None, A.plant_get_applied() if j == 2 else None)
        _check("%s follow interval %d" % (tag, j), mode, got, _interval(A, chain, step, z[j], hx[j], fb, j, delta[j]), worst)
    assert np.all(A.plant_alive() == 1)
    print("%s: worst state %.3e, reported control %.3e, applied torque %.3e" % (tag, worst["state"], worst["control"], worst["applied"]))
    A.close(); Y.close()


# ---- 4, 5: bit for bit
SCORE = dict(R=0.05 + 0.01 * np.arange(NU), upright=7.0, balance=11.0, joint_limits=900.0, control_limits=1300.0)


def _snapshot(A):
    hx, hu = A.plant_history()
    return A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive(), hx, hu, A.plant_get_applied()


def _run(A, x0, calls="advance_follow"):
    A.plant_reset(x0)
    if calls == "advance_follow":
        A.plant_advance(); A.plant_follow(1, 2)
    elif calls == "fused":
        A.plant_follow(0, 3)
    elif calls == "advance":
        A.plant_advance()
    elif calls == "follow1":
        A.plant_follow(0, 1)
    else:
        for j in range(3):
            A.plant_follow(j, 1)
    return _snapshot(A)


@pytest.mark.parametrize("observed", [False, True])
@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("mode,group", [(0, "mid"), (2, "sliding")])
def test_a_zero_record_is_no_table(mode, group, fb, observed):
    Q, _, _ = sc.build_cost_matrices()
    x0, ui = _states(group)
    A = _solver(mode, False, fb=fb, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    if observed:
        A.plant_set_observation(oc.plant_records(B), seed=SEED + 1)
    A.plant_set_score(Q=0.37 * Q + 1.0, **SCORE)
    none = _run(A, x0); none_score = A.plant_score()
    assert np.array_equal(none[6], none[1])                                                                # without a table: the reported control
    A.plant_set_actuator(ZERO, seed=SEED)
    zero = _run(A, x0); zero_score = A.plant_score()
    assert np.all(none[3] == 1) and none[4].shape == (3, B, NX)
    for name, p, q in zip(("state", "control", "stance", "alive", "ring x", "ring u", "applied"), none, zero):
        assert np.array_equal(p, q), (name, float(np.abs(np.asarray(p, dtype=np.float64) - q).max()))
    assert np.array_equal(none_score, zero_score) and np.array_equal(zero[6], zero[1])                     # the applied torque is the reported one
    # ... per rollout as well
    A.plant_set_actuator(np.zeros((B, 39)), seed=SEED + 2)
    assert _same(none, _run(A, x0)) and np.array_equal(A.plant_score(), none_score)
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_equivalences_of_the_actuator_table(fb):
    mode, limits, source, group = CASES["mode4_limits"]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    none = _run(A, x0, "fused")
    rec = ac.golden_records()
    A.plant_set_actuator(rec, seed=SEED)
    fused = _run(A, x0, "fused")
    split = _run(A, x0, "split")
    assert A.plant_intervals() == 3 and _same(fused, split) and np.all(fused[3] == 1)                      # follow(0, 3) is three follow(j, 1): delay line, y and n persist
    assert _same(_run(A, x0, "advance"), _run(A, x0, "follow1"))                                           # an advance is follow(0, 1)
    assert _same(fused, _run(A, x0, "fused"))                                                              # plant_reset and the same calls: the same run
    assert (np.abs(fused[0] - none[0]).max(axis=1) > 1e-6).sum() >= 25                                      # ... and not the run without a table
    assert np.array_equal(fused[1], A.plant_history()[1][2]) and not np.array_equal(fused[6], fused[1])    # reported: the command; applied: not
    # the table survives plant_reset and plant_configure (which primes the state again, as the reset does)
    A.plant_configure(SUBSTEPS, fb, "schedule")
    assert A.plant_num_actuator_sets() == B and _same(fused, _run(A, x0, "fused"))
    # B identical records are one shared record
    A.plant_set_actuator(np.repeat(rec[5:6], B, axis=0), seed=SEED)
    many = _run(A, x0, "fused")
    A.plant_set_actuator(rec[5:6], seed=SEED)
    assert _same(many, _run(A, x0, "fused")) and not _same(many, fused)
    # another seed: another run (the rollouts without noise excepted)
    A.plant_set_actuator(rec, seed=SEED + 1)
    other = _run(A, x0, "fused")
    noisy = np.arange(B) % 4 != 2
    assert (np.abs(other[0] - fused[0]).max(axis=1)[noisy] > 0).sum() >= 25 and np.array_equal(other[0][~noisy], fused[0][~noisy])
    # clear: the results without a table, bit for bit
    A.plant_clear_actuator()
    assert A.plant_num_actuator_sets() == 0 and _same(none, _run(A, x0, "fused"))
    A.plant_clear_actuator()                                                                               # (clearing nothing is fine)
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_a_batch_of_37_is_shards_of_20_and_17(fb):
    x0, ui = _states("mid")
    rec = ac.golden_records()
    A = _solver(0, False, fb=fb, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_set_actuator(rec, seed=SEED)
    whole = _run(A, x0, "fused")
    A.close()
    for lo, hi in ((0, 20), (20, B)):
        P = _solver(0, False, fb=fb, ring=3, rows=slice(lo, hi))
        P.initialize(x0[lo:hi], ui[lo:hi]); P.solve(x0[lo:hi])
        P.plant_set_actuator(rec[lo:hi], seed=SEED, stream0=lo)
        part = _run(P, x0[lo:hi], "fused")
        for name, w, p in zip(("state", "control", "stance", "alive", "ring x", "ring u", "applied"), whole, part):
            assert np.array_equal(w[lo:hi] if w.ndim < 3 else w[:, lo:hi], p), (lo, hi, name)
        P.close()


# ---- 6: the reported control stays the command
def test_reported_control_is_the_command_and_the_joints_get_it_late():
    x0, ui = _states("mid")
    A = _solver(0, False, fb=0, ring=1)
    A.initialize(x0, ui); A.solve(x0)
    ub0 = A.ubar()[:, 0]
    A.plant_set_actuator(sc.stack_plant_actuator(B, delay=3), seed=SEED)
    A.plant_reset(x0); A.plant_advance()                                                                   # feedback mode 0, right after the solve: x - xbar_0 is exactly zero
    assert np.array_equal(A.plant_control(), ub0) and np.array_equal(A.plant_history()[1][0], ub0) and np.all(A.plant_alive() == 1)
    assert np.array_equal(A.plant_get_applied(), ub0)                                                      # primed with c_0: the joints were holding it
    # one substep per interval: the applied torque per substep.  Knot j commands c_j; with a delay of 3 the joints get c_0 four times, then c_1, c_2
    A.plant_configure(1, 0, "schedule")
    A.plant_reset(x0)
    c, t = [], []
    for j in range(6):
        A.plant_follow(j, 1)
        c.append(A.plant_control()); t.append(A.plant_get_applied())
    assert all(not np.array_equal(c[j], c[j + 1]) for j in range(5))                                       # the knots differ
    for j, src in enumerate((0, 0, 0, 0, 1, 2)):
        assert np.array_equal(t[j], c[src]), (j, src)
    assert np.all(A.plant_alive() == 1)
    A.close()


# ---- 7: a non-finite rollout
@pytest.mark.parametrize("fb", [0, 1])
def test_a_non_finite_rollout_freezes_alone_under_the_actuator_table(fb):
    bad = 33                                                                                               # in the second workgroup at feedback mode 0
    x0, ui = _states("mid")
    rec = ac.golden_records()
    rec[bad, 0] = 0.0; rec[bad, 1:20] = 0.0                                                                # no delay, no lag: what the joints of the frozen rollout get is zeros and noise
    out = {}
    for poisoned in (False, True):
        A = _solver(0, False, fb=fb, ring=2)
        A.initialize(x0, ui); A.solve(x0)
        A.plant_set_actuator(rec, seed=SEED)
        xp = x0.copy()
        if poisoned:
            xp[bad, 9] = np.nan
        A.plant_reset(xp); A.plant_follow(0, 2)
        out[poisoned] = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive(), A.plant_get_applied(), A.plant_actuator_draws(1, 1)[0]
        A.close()
    x, u, st, alive, applied, z = out[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(u[bad] == 0.0) and np.array_equal(x[bad], np.where(np.arange(NX) == 9, np.nan, x0[bad]), equal_nan=True)
    assert np.all(alive[keep] == 1) and np.all(out[False][3] == 1)
    assert np.array_equal(x[keep], out[False][0][keep]) and np.array_equal(u[keep], out[False][1][keep]) and np.array_equal(applied[keep], out[False][4][keep])      # bit for bit
    # the non-finite command entered the delay line as zeros: zeros plus the interval's noise come out
    assert np.array_equal(applied[bad], np.where(rec[bad, 20:] == 0.0, 0.0, rec[bad, 20:] * z[bad]))


# ---- 8: the score
def test_score_under_an_actuator_table_is_the_score_of_the_ring():
    Q, _, _ = sc.build_cost_matrices()
    score = dict(Q=0.37 * Q + 1.0, **SCORE)
    x0, ui = _states("limits")
    A = _solver(4, True, ring=3)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_set_actuator(ac.golden_records(), seed=SEED)
    A.plant_set_score(**score)
    A.plant_reset(x0)
    A.plant_advance(); A.plant_follow(1, 2)
    got = A.plant_score()
    hx, hu = A.plant_history()
    assert np.array_equal(hx[0], x0) and not np.array_equal(hu[2], A.plant_get_applied())                  # the ring holds the commands
    prob = _problem()
    want = ps.expected_record(ps.IntervalOracle(DT), [(prob, k) for k in range(3)], hx, hu, score)
    ok, worst = ps.close_enough(got, want)
    print("score under an actuator table: worst |got - want| / bound = %.3f" % worst)
    assert ok.all() and np.array_equal(got[:, 6:], want[:, 6:])
    A.close()


# ---- 9: refusals on a live handle
def test_refusals_on_a_live_handle(tmp_path):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    sv = _sv()
    A = _solver()
    rec = ac.golden_records()
    for bad in (np.ones((2, 39)), np.ones((B, 38))):
        with pytest.raises(ValueError):
            A.plant_set_actuator(bad)
    two = np.ascontiguousarray(rec[:2])
    assert A.L.ilqr_hip_plant_set_actuator(A.h, two.ctypes.data_as(sv._dp), 2, C.c_ulonglong(1), C.c_ulonglong(0)) == 1      # n neither 1 nor B, past the wrapper
    assert A.L.ilqr_hip_plant_set_actuator(A.h, None, 1, C.c_ulonglong(1), C.c_ulonglong(0)) == 1
    for col, v in ((0, 9.0), (0, 1.5), (0, -1.0), (0, np.nan), (1, -1e-12), (19, np.inf), (20, -1e-12), (38, -1.0), (38, np.nan)):
        q = rec.copy(); q[B - 1, col] = v
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_actuator(q)
    assert A.plant_num_actuator_sets() == 0
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        A.plant_actuator_draws(0, 1)                                                                       # no table: nothing to draw for
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        A.plant_actuator_blend()
    A.plant_set_actuator(rec[:1], seed=5)
    assert A.plant_num_actuator_sets() == 1 and A.plant_actuator_draws(0, N).shape == (N, B, NU)
    with pytest.raises(ValueError):
        A.plant_actuator_draws(0, N + 1)                                                                   # count beyond N: the wrapper ...
    buf = np.zeros((N + 1, B, NU))
    assert A.L.ilqr_hip_plant_actuator_draws(A.h, C.c_long(0), N + 1, buf.ctypes.data_as(sv._dp)) == 1     # ... and the entry point
    assert A.L.ilqr_hip_plant_actuator_draws(A.h, C.c_long(-1), 1, buf.ctypes.data_as(sv._dp)) == 1
    assert np.all(buf == 0.0)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(A, None, None, plant_actuator=rec)
    A.close()
    # a library whose directory holds no actuator module: an error that names the path it looked for, never a fall-back
    lonely = tmp_path / "libilqr_hip.so"
    shutil.copyfile(sv.LIB_PATH, lonely)
    P = sv.BatchedILQR(B, N=N, dt=DT, lib_path=str(lonely))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED") as e:
        P.plant_set_actuator(rec, seed=5)
    assert os.path.join(str(tmp_path), "libilqr_hip_actuator.so") in str(e.value)
    assert P.plant_num_actuator_sets() == 0
    P.close()


# ---- 10: the runner
def test_runner_delayed_and_lagged_actuators_move_the_closed_loop():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, Nn, steps = 4, 25, 6
    base = sc.make_problem(sv.reference_kinematics, N=Nn, gravity=dc.GRAVITY)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(Bn, Nn, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    slow = np.array([False, False, True, True])
    table = sc.stack_plant_actuator(Bn, delay=np.where(slow, 2, 0), tau=np.where(slow, 0.02, 0.0))
    res = {}
    for tab in (False, True):
        # (contact mode 2, as the runner test of tests/test_gpu_observation.py and for its reason: the constraint-free standing solve returns a
        # non-finite cost and keeps its initial guess either way)
        s = sv.BatchedILQR(Bn, N=Nn, dt=DT); s.set_max_iterations(2); s.set_contact_mode(2)
        run = ml.MPCRunner(s, rd, base, resident=True, plant_actuator=table if tab else None, actuator_seed=SEED)
        res[tab] = run.run(x0, steps, u_init=ui)[0][-1]
        assert np.all(s.plant_alive() == 1) and np.all(np.isfinite(run.last_cost))
        if tab:
            assert s.plant_num_actuator_sets() == Bn and np.array_equal(s.plant_get_actuator()[0], table) and s.plant_intervals() == steps
        s.close()
    dist = np.abs(res[True] - res[False]).max(axis=1)
    print("after %d intervals: |x - x(no table)| per rollout %s" % (steps, dist))
    assert np.all(np.isfinite(dist)) and np.all(dist[slow] > 0.0)
    assert np.array_equal(res[True][~slow], res[False][~slow])                                             # the untouched pair ends exactly where it was
