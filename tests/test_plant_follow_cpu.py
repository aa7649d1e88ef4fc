"""CPU checks of following the policy between solves (include/ilqr_hip.h ilqr_hip_plant_follow, ilqr_hip_initialize_warm_*_shifted,
ilqr_hip_compute_control_at; mpc_loop.MPCRunner(solve_every=m)): the new entry points validate their arguments without a device, the
Python wrappers check ranges and shapes, and MPCRunner issues exactly the documented call sequences against the recording stand-in of
tests/test_plant_cpu.py -- whose methods have today's signatures, so solve_every=1 cannot pass a new argument unnoticed."""
import ctypes as C

import numpy as np
import pytest

from test_plant_cpu import ERR_ARG, NU, NV, NX, _base, _lib, _Recorder, _Refs

ERR_STATE = 4
N = 6


def test_the_new_entry_points_refuse_a_null_handle():
    sv, L = _lib()
    buf = (C.c_double * (NX * 4))()
    assert L.ilqr_hip_plant_follow(None, 0, 1) == ERR_ARG
    assert L.ilqr_hip_initialize_warm_from_plant_shifted(None, 1) == ERR_ARG
    assert L.ilqr_hip_initialize_warm_resident_shifted(None, buf, 1) == ERR_ARG
    assert L.ilqr_hip_compute_control_at(None, 0, buf, buf) == ERR_ARG


def test_the_new_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    """as test_plant_cpu: the handle is a block of zeroed memory, here with the batch and the horizon (the second and third int of the
    handle) filled in, which ilqr_hip_horizon confirms.  A shift in range gets as far as the state check -- nothing initialised:
    ILQR_ERR_STATE -- so ILQR_ERR_ARG is the range check and not the empty handle.  (plant_follow writes its error text before it returns
    ILQR_ERR_STATE, which this block of memory cannot take: its in-range arguments are exercised on the GPU.)"""
    sv, L = _lib()
    fake = C.create_string_buffer(1 << 16)
    C.cast(fake, C.POINTER(C.c_int))[1] = 2
    C.cast(fake, C.POINTER(C.c_int))[2] = N
    h = C.cast(fake, C.c_void_p)
    assert L.ilqr_hip_horizon(h) == N and L.ilqr_hip_batch(h) == 2
    buf = (C.c_double * (NX * 4))()
    for first, count in ((0, 0), (0, -1), (-1, 1), (0, N + 1), (1, N), (N, 1), (N - 1, 2), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert L.ilqr_hip_plant_follow(h, first, count) == ERR_ARG, (first, count)
    for shift in (0, -1, N, N + 3):
        assert L.ilqr_hip_initialize_warm_from_plant_shifted(h, shift) == ERR_ARG, shift
        assert L.ilqr_hip_initialize_warm_resident_shifted(h, buf, shift) == ERR_ARG, shift
    for shift in (1, 3, N - 1):
        assert L.ilqr_hip_initialize_warm_from_plant_shifted(h, shift) == ERR_STATE, shift
        assert L.ilqr_hip_initialize_warm_resident_shifted(h, buf, shift) == ERR_STATE, shift
    assert L.ilqr_hip_initialize_warm_resident_shifted(h, None, 1) == ERR_ARG
    for knot in (N, -1, N + 7):
        assert L.ilqr_hip_compute_control_at(h, knot, buf, buf) == ERR_ARG, knot
    assert L.ilqr_hip_compute_control_at(h, 0, None, buf) == ERR_ARG and L.ilqr_hip_compute_control_at(h, 0, buf, None) == ERR_ARG


def test_python_wrappers_check_ranges_and_shapes():
    from mpc_ilqr_mujoco_amd import solver as sv
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the checks below fail before the library is reached
    s.B, s.N, s.h = 3, N, None
    for first, count in ((0, 0), (-1, 1), (0, N + 1), (N - 1, 2)):
        with pytest.raises(ValueError):
            s.plant_follow(first, count)
    for shift in (0, N, -2):
        with pytest.raises(ValueError):
            s.initialize_warm_from_plant(shift=shift)
        with pytest.raises(ValueError):
            s.initialize_warm_resident(np.zeros((3, NX)), shift=shift)
    with pytest.raises(ValueError):
        s.initialize_warm_resident(np.zeros((2, NX)), shift=2)
    for knot in (N, -1):
        with pytest.raises(ValueError):
            s.compute_control(np.zeros((3, NX)), knot=knot)
    with pytest.raises(ValueError):
        s.compute_control(np.zeros((3, NU)), knot=1)


class _Recorder3(_Recorder):
    """the stand-in with the new keywords"""

    def initialize_warm_resident(self, x0, shift=None):
        self._rec("initialize_warm_resident" if shift is None else "initialize_warm_resident(shift=%d)" % shift)

    def initialize_warm_from_plant(self, shift=None):
        self._rec("initialize_warm_from_plant" if shift is None else "initialize_warm_from_plant(shift=%d)" % shift)

    def compute_control(self, x, knot=None):
        self._rec("compute_control" if knot is None else "compute_control(knot=%d)" % knot); return np.zeros((self.B, NU))

    def plant_follow(self, first_knot, count):
        self._rec("plant_follow(%d,%d)" % (first_knot, count)); self.advances += count


def test_solve_every_1_issues_todays_sequences_unchanged():
    """against the stand-in with TODAY's signatures: a shift or knot argument would be a TypeError"""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, NN, steps = 3, 25, 4
    s = _Recorder(B, NN)
    run = ml.MPCRunner(s, _Refs(NN), _base(NN), resident=True, substeps=4, feedback_mode=1, solve_every=1)
    run.run(np.zeros((B, NX)), steps, kicks={2: np.zeros((B, NV))})
    want = ["plant_configure(4,1,schedule)", "plant_set_history(4)", "plant_reset", "set_problem", "initialize", "solve(x)", "plant_advance"]
    for k in range(1, steps):
        want += ["set_problem", "initialize_warm_from_plant", "solve(None)"] + (["plant_kick"] if k == 2 else []) + ["plant_advance"]
    want += ["plant_history", "plant_state"]
    assert s.calls == want and run.t_idx == steps and run.refs.calls == list(range(steps))
    s = _Recorder(B, NN, 2)
    run = ml.MPCRunner(s, _Refs(NN), _base(NN), solve_every=1)
    run.run(np.zeros((B, NX)), steps)
    want = ["set_problem", "initialize", "solve(x)", "compute_control", "step_stance"]
    for _ in range(1, steps):
        want += ["set_problem", "initialize_warm_resident", "solve(x)", "compute_control", "step_stance"]
    assert s.calls == want and run.refs.calls == list(range(steps))


def test_resident_runner_solves_every_third_interval():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, NN, steps = 3, 25, 8      # two whole groups and one of two intervals
    s = _Recorder3(B, NN)
    run = ml.MPCRunner(s, _Refs(NN), _base(NN), resident=True, substeps=2, solve_every=3)
    xs, us = run.run(np.zeros((B, NX)), steps, kicks={3: np.zeros((B, NV))})
    want = ["plant_configure(2,0,schedule)", "plant_set_history(8)", "plant_reset",
            "set_problem", "initialize", "solve(x)", "plant_follow(0,3)",
            "set_problem", "initialize_warm_from_plant(shift=3)", "solve(None)", "plant_kick", "plant_follow(0,3)",
            "set_problem", "initialize_warm_from_plant(shift=3)", "solve(None)", "plant_follow(0,2)",
            "plant_history", "plant_state"]
    assert s.calls == want, s.calls
    assert run.t_idx == steps and run.refs.calls == [0, 3, 6]      # the window advances by the group
    assert xs.shape == (steps + 1, B, NX) and us.shape == (steps, B, NU)
    # the next run starts a group of its own; its warm start shifts by the two intervals the last group applied
    s.calls.clear()
    run.run(np.zeros((B, NX)), 3)
    assert s.calls[3:7] == ["set_problem", "initialize_warm_from_plant(shift=2)", "solve(None)", "plant_follow(0,3)"], s.calls
    assert run.refs.calls[-1] == 8 and run.t_idx == 11


@pytest.mark.parametrize("contact_mode,plant_contacts,step_call", [(0, "schedule", "step"), (2, "schedule", "step_stance"), (2, "geometry", "step_geometry")])
def test_host_runner_solves_every_third_interval(contact_mode, plant_contacts, step_call):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, NN, steps = 3, 25, 7

    class Refs(_Refs):
        def problem_at(self, t0, N, base, follow_schedule=False):      # row j of the window is recognisable: (j % 2, 1)
            prob = super().problem_at(t0, N, base, follow_schedule)
            prob["stance"][0, :, 0] = np.arange(N + 1) % 2
            return prob

    class Rec(_Recorder3):
        def step_stance(self, x, u, l, r):
            self._rec("step_stance(%d,%d)" % (l, r)); return np.array(x)

    s = Rec(B, NN, contact_mode)
    run = ml.MPCRunner(s, Refs(NN), _base(NN), plant_contacts=plant_contacts, solve_every=3)
    xs, us = run.run(np.zeros((B, NX)), steps)
    step = lambda j: "step_stance(%d,1)" % (j % 2) if step_call == "step_stance" else step_call
    group = lambda warm: ["set_problem", warm, "solve(x)", "compute_control", step(0), "compute_control(knot=1)", step(1), "compute_control(knot=2)", step(2)]
    want = group("initialize") + group("initialize_warm_resident(shift=3)") + ["set_problem", "initialize_warm_resident(shift=3)", "solve(x)", "compute_control", step(0)]
    assert s.calls == want, s.calls
    assert run.t_idx == steps and run.refs.calls == [0, 3, 6]
    assert xs.shape == (steps + 1, B, NX) and us.shape == (steps, B, NU)


def test_logs_keep_one_main_row_per_plant_interval(tmp_path):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, NN, steps = 2, 25, 6
    heads = {}
    for resident in (False, True):
        d = tmp_path / ("resident" if resident else "host")
        run = ml.MPCRunner(_Recorder3(B, NN), _Refs(NN), _base(NN), log_dir=str(d), log_rollouts=(0, 1), resident=resident, solve_every=3)
        run.run(np.zeros((B, NX)), steps)
        run.close()
        for b in (0, 1):
            for name in ("mpc_log.csv", "q_optimal.csv", "u_optimal.csv"):
                lines = (d / ("rollout_%d" % b) / name).read_text().splitlines()
                assert len(lines) == steps + 1, (resident, b, name)
                heads.setdefault((b, name), []).append((lines[0], [ln.split(",")[0] for ln in lines[1:]]))
            main = [ln.split(",") for ln in (d / ("rollout_%d" % b) / "mpc_log.csv").read_text().splitlines()[1:]]
            assert [r[0] for r in main] == [str(k + 1) for k in range(steps)]
            assert main[0][2:4] == main[1][2:4] == main[2][2:4] and main[3][2:4] == main[4][2:4] == main[5][2:4]      # solve cost and time repeat over the group
    for key, (host, res) in heads.items():
        assert host == res, key


def test_a_resident_kick_off_the_first_interval_of_a_group_raises():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, NN = 2, 25
    s = _Recorder3(B, NN)
    run = ml.MPCRunner(s, _Refs(NN), _base(NN), resident=True, solve_every=3)
    with pytest.raises(ValueError, match="first interval of a group"):
        run.run(np.zeros((B, NX)), 6, kicks={4: np.zeros((B, NV))})
    assert s.calls == []      # refused before anything was issued
    run.run(np.zeros((B, NX)), 6, kicks={3: np.zeros((B, NV))})
    assert s.calls.count("plant_kick") == 1
    # the host path takes a kick in any interval
    h = _Recorder3(B, NN)
    ml.MPCRunner(h, _Refs(NN), _base(NN), solve_every=3).run(np.zeros((B, NX)), 6, kicks={4: np.zeros((B, NV))})
    assert h.calls.count("compute_control(knot=1)") == 2
    for bad in (0, NN, -1):
        with pytest.raises(ValueError):
            ml.MPCRunner(s, _Refs(NN), _base(NN), solve_every=bad)
