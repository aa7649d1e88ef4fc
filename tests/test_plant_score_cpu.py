"""CPU checks of the closed-loop score of the resident plant (include/ilqr_hip.h ilqr_hip_plant_set_score ...): the entry points validate
their arguments without a device, the header declares them, MPCRunner issues the documented call sequence against a recording stand-in
for the solver, and the horizon-1 oracle construction that the GPU tests use as their yardstick (tests/plant_score_ref.py) reproduces a
horizon-N total_cost()."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import plant_score_ref as ps
from conftest import load_package
from test_plant_cpu import NU, NV, NX, _base, _Recorder, _Refs

pkg = load_package()
sc = pkg.scenario
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = 1, 4


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    L = sv.load_library()
    L.ilqr_hip_plant_set_score.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.c_double]
    return sv, L


def test_score_entry_points_refuse_a_null_handle():
    sv, L = _lib()
    q, r, out = (C.c_double * NX)(), (C.c_double * NU)(), (C.c_double * 64)()
    p = C.c_void_p()
    assert L.ilqr_hip_plant_set_score(None, q, r, 0.0, 0.0, 0.0, 0.0) == ERR_ARG
    assert L.ilqr_hip_plant_clear_score(None) == ERR_ARG
    assert L.ilqr_hip_plant_get_score(None, out) == ERR_ARG
    assert L.ilqr_hip_plant_score_device(None, C.byref(p)) == ERR_ARG


def test_score_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    """as tests/test_plant_cpu.py: the handle is a block of zeroed memory that a call which got past its checks would have to read"""
    sv, L = _lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    q, r = (C.c_double * NX)(*([1.0] * NX)), (C.c_double * NU)(*([1.0] * NU))
    assert L.ilqr_hip_plant_set_score(h, None, r, 0.0, 0.0, 0.0, 0.0) == ERR_ARG
    assert L.ilqr_hip_plant_set_score(h, q, None, 0.0, 0.0, 0.0, 0.0) == ERR_ARG
    for slot in range(4):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            w = [1.0, 2.0, 3.0, 4.0]
            w[slot] = bad
            assert L.ilqr_hip_plant_set_score(h, q, r, *w) == ERR_ARG, (slot, bad)
    for bad in (-1.0, float("nan"), float("inf")):      # ... and an entry of the two diagonals
        qb = (C.c_double * NX)(*([1.0] * NX)); qb[NX - 1] = bad
        rb = (C.c_double * NU)(*([1.0] * NU)); rb[0] = bad
        assert L.ilqr_hip_plant_set_score(h, qb, r, 0.0, 0.0, 0.0, 0.0) == ERR_ARG
        assert L.ilqr_hip_plant_set_score(h, q, rb, 0.0, 0.0, 0.0, 0.0) == ERR_ARG
    assert L.ilqr_hip_plant_get_score(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_score_device(h, None) == ERR_ARG
    # no score installed on the zeroed handle: the getters say so without a device
    out, p = (C.c_double * 64)(), C.c_void_p()
    assert L.ilqr_hip_plant_get_score(h, out) == ERR_STATE
    assert L.ilqr_hip_plant_score_device(h, C.byref(p)) == ERR_STATE


def test_header_and_wrappers_declare_the_score():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    names = ("ilqr_hip_plant_set_score", "ilqr_hip_plant_clear_score", "ilqr_hip_plant_get_score", "ilqr_hip_plant_score_device")
    for name in names:
        assert re.search(r"^int " + name + r"\s*\(", hdr, re.M), name
        assert name in sv.EXPORTS
    assert re.search(r"^#define\s+ILQR_PLANT_SCORE_TERMS\s+8\s*$", hdr, re.M)
    assert sv.PLANT_SCORE_TERMS == ("state", "control", "upright", "balance", "joint_limits", "control_limits", "min_pelvis_height", "intervals")
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    assert all(m in hpp for m in ("plantSetScore", "plantClearScore", "plantScore"))
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the shape check fails before the library is reached
    s.B, s.N, s.h = 3, 25, None
    with pytest.raises(ValueError):
        s.plant_set_score(np.ones(NX - 1), np.ones(NU))
    with pytest.raises(ValueError):
        s.plant_set_score(np.ones(NX), np.ones((2, NU)))


class _ScoreRecorder(_Recorder):
    def plant_set_score(self, Q, R, upright=0.0, balance=0.0, joint_limits=0.0, control_limits=0.0):
        self._rec("plant_set_score(%g,%g,%g,%g)" % (upright, balance, joint_limits, control_limits))

    def plant_follow(self, first_knot, count):
        self._rec("plant_follow(%d,%d)" % (first_knot, count)); self.advances += count

    def plant_history(self):
        self._rec("plant_history")
        rows = min(self.advances, self.hist_rows)
        return np.zeros((rows, self.B, NX)), np.zeros((rows, self.B, NU))

    def initialize_warm_from_plant(self, shift=1): self._rec("initialize_warm_from_plant")

    def plant_score(self):
        self._rec("plant_score"); return np.zeros((self.B, 8))


def _todays_sequence(steps, ring):
    want = ["plant_configure(1,0,schedule)", "plant_set_history(%d)" % ring, "plant_reset", "set_problem", "initialize", "solve(x)", "plant_advance"]
    for _ in range(1, steps):
        want += ["set_problem", "initialize_warm_from_plant", "solve(None)", "plant_advance"]
    return want + ["plant_history", "plant_state"]


def test_runner_sequence_is_todays_with_the_defaults():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, N, steps = 3, 25, 4
    s = _ScoreRecorder(B, N)
    run = ml.MPCRunner(s, _Refs(N), _base(N), resident=True)
    xs, us = run.run(np.zeros((B, NX)), steps)
    assert s.calls == _todays_sequence(steps, steps), s.calls
    assert xs.shape == (steps + 1, B, NX) and us.shape == (steps, B, NU)
    with pytest.raises(ValueError):
        run.score()      # none was asked for


def test_runner_installs_the_score_before_the_reset_and_sizes_the_ring():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, N, steps = 3, 25, 4
    s = _ScoreRecorder(B, N)
    score = dict(Q=np.ones(NX), R=np.ones(NU), upright=1.0, balance=2.0, joint_limits=3.0, control_limits=4.0)
    run = ml.MPCRunner(s, _Refs(N), _base(N), resident=True, score=score, history_rows=2)
    xs, us = run.run(np.zeros((B, NX)), steps)
    want = _todays_sequence(steps, 2)
    want.insert(2, "plant_set_score(1,2,3,4)")
    assert s.calls == want, s.calls
    assert s.calls.index("plant_set_score(1,2,3,4)") == s.calls.index("plant_reset") - 1 == s.calls.index("plant_set_history(2)") + 1
    assert xs.shape == (2 + 1, B, NX) and us.shape == (2, B, NU)      # the rows the ring still holds, and the final state
    assert run.score().shape == (B, 8) and s.calls[-1] == "plant_score"
    # groups of two intervals: a ring of exactly one group
    s = _ScoreRecorder(B, N)
    run = ml.MPCRunner(s, _Refs(N), _base(N), resident=True, solve_every=2, history_rows=2, score=score)
    run.run(np.zeros((B, NX)), steps)
    assert s.calls[:4] == ["plant_configure(1,0,schedule)", "plant_set_history(2)", "plant_set_score(1,2,3,4)", "plant_reset"]
    assert s.calls.count("plant_follow(0,2)") == 2 and s.calls.count("plant_set_score(1,2,3,4)") == 1


def test_runner_refuses_a_ring_below_one_group_and_a_score_on_the_host_path():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    N = 25
    s = _ScoreRecorder(3, N)
    score = dict(Q=np.ones(NX), R=np.ones(NU))
    with pytest.raises(ValueError):
        ml.MPCRunner(s, _Refs(N), _base(N), resident=True, solve_every=3, history_rows=2)
    with pytest.raises(ValueError):
        ml.MPCRunner(s, _Refs(N), _base(N), resident=False, score=score)
    ml.MPCRunner(s, _Refs(N), _base(N), resident=True, solve_every=3, history_rows=3, score=score)
    assert s.calls == []      # (the constructor calls nothing)


def _trajectory(N, seed):
    """a trajectory off the standing pose with every term alive: hinges past the 10 % margins, controls past theirs, a tilted pelvis"""
    rng = np.random.default_rng(seed)
    jr = ol.joint_ranges()
    xs = np.tile(sc.standing_state(), (N + 1, 1))
    xs[:, 0:3] += rng.uniform(-0.05, 0.05, (N + 1, 3))
    xs[:, 3:7] = sc._axis_angle_quat(rng.uniform(-0.3, 0.3, (N + 1, 3)))
    xs[:, 7:26] += rng.uniform(-0.3, 0.3, (N + 1, 19))
    xs[:, 26:] = rng.uniform(-0.5, 0.5, (N + 1, 25))
    xs[1, 7 + 3] = jr[3, 1] - 0.02 * (jr[3, 1] - jr[3, 0])       # inside the upper margin
    xs[2, 7 + 12] = jr[12, 0] + 0.05 * (jr[12, 1] - jr[12, 0])   # inside the lower margin
    us = rng.uniform(-20.0, 20.0, (N, NU))
    us[0, 4] = 0.95 * sc.CTRLRANGE[4]; us[3, 13] = -1.2 * sc.CTRLRANGE[13]      # past the margin, and past the range itself
    return xs, us


def test_horizon_1_terms_add_up_to_the_horizon_N_cost():
    N, dt = 6, 0.02
    prob = sc.make_problem(ol.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rng = np.random.default_rng(5)
    prob["x_ref"] = prob["x_ref"] + rng.uniform(-0.02, 0.02, prob["x_ref"].shape)
    prob["u_ref"] = rng.uniform(-2.0, 2.0, prob["u_ref"].shape)
    prob["ee_ref"] = prob["ee_ref"] + rng.uniform(-0.05, 0.05, prob["ee_ref"].shape)
    pattern = np.array([(1, 1), (1, 0), (0, 1), (0, 0), (1, 1), (0, 1), (0, 0)], dtype=np.int32)      # every kind of row; the terminal one without a foot
    prob["stance"] = pattern[None, :N + 1].copy()
    score = dict(Q=rng.uniform(1.0, 100.0, NX), R=rng.uniform(0.01, 1.0, NU), upright=7.0, balance=11.0, joint_limits=900.0, control_limits=1300.0)
    orc = ps.IntervalOracle(dt)
    xs, us = _trajectory(N, 6)
    xs[N] = orc.xT
    # the free terminal knot is free: exactly zero under every weight
    sub = orc.window_row(prob, 0, 2)
    sub.update(Q=score["Q"], R=score["R"], Qf=np.zeros(NX), task_weights=[0, 0, 0, 0, score["upright"], score["balance"]], w_joint=score["joint_limits"], w_ctrl=score["control_limits"])
    sub["x_ref"] = np.stack([orc.xT, orc.xT])[None]; sub["u_ref"] = np.zeros((1, 1, NU)); sub["stance"] = np.zeros((1, 2, 2), dtype=np.int32)      # (both knots the terminal one)
    orc.o.set_problem(sub); orc.o.set_trajectory(np.stack([orc.xT, orc.xT]), np.zeros((1, NU)))
    assert orc.o.total_cost() == 0.0
    # the horizon-N cost under all six weights at once, with the same free terminal knot
    full = dict(prob)
    full.update(Q=score["Q"], R=score["R"], Qf=np.zeros(NX), task_weights=[0, 0, 0, 0, score["upright"], score["balance"]], w_joint=score["joint_limits"], w_ctrl=score["control_limits"])
    o = ol.Oracle(N, dt); o.set_problem(full); o.set_trajectory(xs, us)
    want = o.total_cost()
    terms = np.array([orc.terms(prob, 0, k, xs[k], us[k], score) for k in range(N)])
    print("terms by knot:\n", terms, "\nsum %.17g  horizon-N %.17g" % (terms.sum(), want))
    assert np.all((terms != 0.0).any(axis=0)), "a term is dead on this trajectory"
    assert np.all(terms[3, 3] == 0.0) and np.all(terms[[0, 1, 2, 4, 5], 3] > 0.0)      # the balance term follows the schedule row
    assert abs(terms.sum() - want) <= 1e-13 * abs(want)      # (the two sums differ in the order of ~50 additions only)
    # a term alone is what the oracle gives under that weight alone over the whole horizon
    for i in range(6):
        one = dict(full); one.update(ps.weights_of_term(score, i))
        o.set_problem(one); o.set_trajectory(xs, us)
        assert abs(terms[:, i].sum() - o.total_cost()) <= 1e-13 * abs(o.total_cost()), i
    # ... and the record of those rows as the device accumulates it
    rec = ps.expected_record(orc, [(prob, k) for k in range(N)], xs[:N, None], us[:, None], score)
    assert rec.shape == (1, 8) and rec[0, 7] == N and rec[0, 6] == xs[:N, 2].min() and np.allclose(rec[0, :6], terms.sum(axis=0), rtol=1e-14, atol=0)
