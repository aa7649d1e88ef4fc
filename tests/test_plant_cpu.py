"""CPU checks of the device-resident plant (include/ilqr_hip.h ilqr_hip_plant_*): the new entry points validate their arguments
without a device, and MPCRunner issues exactly the documented call sequence -- the resident one with resident=True, the host one
otherwise -- against a recording stand-in for the solver."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_package

pkg = load_package()
sc = pkg.scenario
NX, NU, NV = 51, 19, 25
ERR_ARG = 1


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv, sv.load_library()


def test_every_plant_entry_point_refuses_a_null_handle():
    sv, L = _lib()
    buf = (C.c_double * (NX * 4))()
    ibuf = (C.c_int * 8)()
    n = C.c_int(0)
    p = C.c_void_p()
    assert L.ilqr_hip_plant_reset(None, buf) == ERR_ARG
    assert L.ilqr_hip_plant_configure(None, 1, 0, 0) == ERR_ARG
    assert L.ilqr_hip_plant_kick(None, buf) == ERR_ARG
    assert L.ilqr_hip_plant_advance(None) == ERR_ARG
    assert L.ilqr_hip_initialize_warm_from_plant(None) == ERR_ARG
    assert L.ilqr_hip_plant_set_history(None, 4) == ERR_ARG
    assert L.ilqr_hip_plant_get_history(None, buf, buf, C.byref(n)) == ERR_ARG
    assert L.ilqr_hip_plant_get_state(None, buf) == ERR_ARG
    assert L.ilqr_hip_plant_get_control(None, buf) == ERR_ARG
    assert L.ilqr_hip_plant_get_stance(None, ibuf) == ERR_ARG
    assert L.ilqr_hip_plant_get_alive(None, ibuf) == ERR_ARG
    assert L.ilqr_hip_plant_state_device(None, C.byref(p)) == ERR_ARG


def test_plant_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    """Argument checks come first in every entry point, so they can be exercised without a device: the handle here is a block of zeroed
    memory that a call which got past its checks would have to read."""
    sv, L = _lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    for substeps, mode, source in ((0, 0, 0), (-3, 0, 0), (1, 2, 0), (1, -1, 0), (1, 0, 2), (1, 0, -1), (4, 1, 7)):
        assert L.ilqr_hip_plant_configure(h, substeps, mode, source) == ERR_ARG, (substeps, mode, source)
    n = C.c_int(0)
    assert L.ilqr_hip_plant_reset(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_kick(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_set_history(h, -1) == ERR_ARG
    assert L.ilqr_hip_plant_get_history(h, None, None, None) == ERR_ARG
    assert L.ilqr_hip_plant_get_state(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_get_control(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_get_stance(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_get_alive(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_state_device(h, None) == ERR_ARG


def test_python_wrappers_check_shapes_and_names():
    from mpc_ilqr_mujoco_amd import solver as sv
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the checks below fail before the library is reached
    s.B, s.N, s.h = 3, 25, None
    with pytest.raises(ValueError):
        s.plant_reset(np.zeros((2, NX)))
    with pytest.raises(ValueError):
        s.plant_kick(np.zeros((3, NX)))
    with pytest.raises(ValueError):
        s.plant_configure(1, 0, "mujoco")


class _Refs:
    """stand-in for references.ReferenceData: one fixed window"""

    def __init__(self, N):
        self.N = N
        self.calls = []

    def problem_at(self, t0, N, base, follow_schedule=False):
        self.calls.append(t0)
        prob = dict(base)
        prob.update(N=N, x_ref=np.zeros((1, N + 1, NX)), u_ref=np.zeros((1, N, NU)), stance=np.ones((1, N + 1, 2), dtype=np.int32))
        return prob


class _Recorder:
    """stand-in for solver.BatchedILQR: records every call, answers with arrays of the right shape"""

    def __init__(self, B, N, contact_mode=0):
        self.B, self.N = B, N
        self.contact_mode = contact_mode
        self.calls = []
        self.hist_rows = 0
        self.advances = 0

    def _rec(self, name):
        self.calls.append(name)

    def set_problem(self, prob): self._rec("set_problem")
    def initialize(self, x0, u_init=None): self._rec("initialize")
    def initialize_warm_resident(self, x0): self._rec("initialize_warm_resident")
    def initialize_warm_from_plant(self): self._rec("initialize_warm_from_plant")

    def solve(self, x0=None):
        self._rec("solve(None)" if x0 is None else "solve(x)")
        return np.zeros(self.B)

    def compute_control(self, x):
        self._rec("compute_control"); return np.zeros((self.B, NU))

    def step(self, x, u):
        self._rec("step"); return np.array(x)

    def step_stance(self, x, u, l, r):
        self._rec("step_stance"); return np.array(x)

    def step_geometry(self, x, u):
        self._rec("step_geometry"); return np.array(x), np.ones((self.B, 2), dtype=np.int32)

    def plant_configure(self, substeps, feedback_mode, source):
        self._rec("plant_configure(%d,%d,%s)" % (substeps, feedback_mode, source))

    def plant_set_history(self, steps):
        self._rec("plant_set_history(%d)" % steps); self.hist_rows = steps

    def plant_reset(self, x): self._rec("plant_reset")
    def plant_kick(self, dv): self._rec("plant_kick")

    def plant_advance(self):
        self._rec("plant_advance"); self.advances += 1

    def plant_history(self):
        self._rec("plant_history")
        return np.zeros((self.advances, self.B, NX)), np.zeros((self.advances, self.B, NU))

    def plant_state(self):
        self._rec("plant_state"); return np.zeros((self.B, NX))

    def xbar(self):
        self._rec("xbar"); return np.zeros((self.B, self.N + 1, NX))

    def ubar(self):
        self._rec("ubar"); return np.zeros((self.B, self.N, NU))


def _base(N):
    return dict(N=N, dt=0.02)


def test_resident_runner_issues_the_resident_call_sequence():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, N, steps = 3, 25, 4
    s = _Recorder(B, N)
    run = ml.MPCRunner(s, _Refs(N), _base(N), resident=True, substeps=4, feedback_mode=1)
    xs, us = run.run(np.zeros((B, NX)), steps, kicks={2: np.zeros((B, NV))})
    want = ["plant_configure(4,1,schedule)", "plant_set_history(4)", "plant_reset",
            "set_problem", "initialize", "solve(x)", "plant_advance"]                               # cold start through the host path
    for k in range(1, steps):
        want += ["set_problem", "initialize_warm_from_plant", "solve(None)"] + (["plant_kick"] if k == 2 else []) + ["plant_advance"]
    want += ["plant_history", "plant_state"]                                                       # one download at the end
    assert s.calls == want, s.calls
    assert s.calls.count("plant_reset") == 1
    assert not any(c in ("compute_control", "step", "step_stance", "step_geometry", "initialize_warm_resident") for c in s.calls)
    assert xs.shape == (steps + 1, B, NX) and us.shape == (steps, B, NU)
    assert run.t_idx == steps and run.refs.calls == list(range(steps))


def test_resident_runner_writes_the_same_log_files(tmp_path):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, N, steps = 2, 25, 3
    heads = {}
    for resident in (False, True):
        d = tmp_path / ("resident" if resident else "host")
        run = ml.MPCRunner(_Recorder(B, N), _Refs(N), _base(N), log_dir=str(d), log_rollouts=(0, 1), resident=resident)
        run.run(np.zeros((B, NX)), steps)
        run.close()
        for b in (0, 1):
            for name in ("mpc_log.csv", "q_optimal.csv", "u_optimal.csv"):
                lines = (d / ("rollout_%d" % b) / name).read_text().splitlines()
                assert len(lines) == steps + 1, (resident, b, name)
                heads.setdefault((b, name), []).append((lines[0], [ln.split(",")[0] for ln in lines[1:]]))
    for key, (host, res) in heads.items():
        assert host == res, key      # same header, same step indices


@pytest.mark.parametrize("contact_mode,plant_contacts,step_call", [(0, "schedule", "step"), (2, "schedule", "step_stance"), (2, "geometry", "step_geometry")])
def test_host_runner_issues_todays_call_sequence(contact_mode, plant_contacts, step_call):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, N, steps = 3, 25, 3
    s = _Recorder(B, N, contact_mode)
    run = ml.MPCRunner(s, _Refs(N), _base(N), plant_contacts=plant_contacts)
    run.run(np.zeros((B, NX)), steps)
    want = ["set_problem", "initialize", "solve(x)", "compute_control", step_call]
    for _ in range(1, steps):
        want += ["set_problem", "initialize_warm_resident", "solve(x)", "compute_control", step_call]
    assert s.calls == want, s.calls
    assert not any(c.startswith("plant_") or c == "initialize_warm_from_plant" for c in s.calls)
    # finer plant steps and the feedback mode exist on the resident path only
    with pytest.raises(ValueError):
        ml.MPCRunner(s, _Refs(N), _base(N), substeps=4)
    with pytest.raises(ValueError):
        ml.MPCRunner(s, _Refs(N), _base(N), feedback_mode=1)


def test_host_runner_applies_a_kick_between_the_solve_and_the_control_law():
    """the host path's branch of run(..., kicks=...): the solve sees the measured state, the control law and the plant step the kicked one,
    and the recorded state of that step is the kicked one -- the ordering of the resident path"""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    B, N, steps = 2, 25, 3

    class Rec(_Recorder):
        def __init__(self, *a):
            super().__init__(*a); self.solved_with, self.controlled_with, self.stepped_with = [], [], []

        def solve(self, x0=None):
            self.solved_with.append(np.array(x0)); return super().solve(x0)

        def compute_control(self, x):
            self.controlled_with.append(np.array(x)); return super().compute_control(x)

        def step(self, x, u):
            self.stepped_with.append(np.array(x)); return super().step(x, u)      # the stand-in plant holds its state

    s = Rec(B, N)
    dv = np.zeros((B, NV)); dv[:, 1] = 0.6
    x0 = np.zeros((B, NX)); x0[:, 2] = 1.0
    xs, us = ml.MPCRunner(s, _Refs(N), _base(N)).run(x0, steps, kicks={1: dv})
    kicked = x0.copy(); kicked[:, 27] = 0.6
    assert np.array_equal(s.solved_with[1], x0)                                   # the solver meets the push one step later
    assert np.array_equal(s.controlled_with[1], kicked) and np.array_equal(s.stepped_with[1], kicked)
    assert np.array_equal(s.controlled_with[0], x0) and np.array_equal(s.solved_with[2], kicked)
    assert np.array_equal(xs[0], x0) and np.array_equal(xs[1], kicked) and np.array_equal(xs[2], kicked) and xs.shape == (steps + 1, B, NX)
    assert s.calls.count("compute_control") == steps and s.calls.count("step") == steps
