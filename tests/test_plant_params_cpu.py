"""CPU checks of the plant's own model and its parameter sets (include/ilqr_hip.h ilqr_hip_plant_set_model, ilqr_hip_plant_set_params ...):
the entry points validate their arguments without a device, header and wrappers declare them, scenario.stack_plant_params broadcasts and
validates, MPCRunner refuses and sequences, and the inputs of the GPU tests (tests/plant_params_cases.py) exercise every column of a set --
checked on the CPU oracle, which shares no code with the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import plant_params_cases as pc
from conftest import load_package
from test_plant_cpu import NU, NX, _base, _Recorder, _Refs

pkg = load_package()
sc = pkg.scenario
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NAMES = ("ilqr_hip_plant_set_model", "ilqr_hip_plant_set_params", "ilqr_hip_plant_clear_params", "ilqr_hip_plant_num_param_sets", "ilqr_hip_plant_get_params")


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv, sv.load_library()


def test_entry_points_are_exported_and_refuse_a_null_handle():
    sv, L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
    buf = (C.c_double * 7)(0.0, 0.0, -9.81, 1.0, 1e-5, 0.0, 1.0)
    assert L.ilqr_hip_plant_set_model(None, -1, -1) == ERR_ARG
    assert L.ilqr_hip_plant_set_params(None, buf, 1) == ERR_ARG
    assert L.ilqr_hip_plant_clear_params(None) == ERR_ARG
    assert L.ilqr_hip_plant_num_param_sets(None) == -1
    assert L.ilqr_hip_plant_get_params(None, buf) == ERR_ARG


def test_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    """as tests/test_plant_cpu.py: the handle is a block of zeroed memory (batch 0) that a call which got past its checks would have to use"""
    sv, L = _lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    for mode, lim in ((-2, -1), (5, -1), (0, -2), (0, 2), (7, 7)):
        assert L.ilqr_hip_plant_set_model(h, mode, lim) == ERR_ARG, (mode, lim)
    good = [0.0, 0.0, -9.81, 1.0, 1e-5, 0.0, 1.0]
    assert L.ilqr_hip_plant_set_params(h, None, 1) == ERR_ARG
    for n_sets in (0, -1, 2, 37):                                          # neither 1 nor the batch (0 on this handle, and 0 sets is no table)
        assert L.ilqr_hip_plant_set_params(h, (C.c_double * (7 * 37))(*(good * 37)), n_sets) == ERR_ARG, n_sets
    bad_values = [(c, v) for c in range(7) for v in (float("nan"), float("inf"), -float("inf"))]
    bad_values += [(3, -1e-3), (4, 0.0), (4, -1e-5), (5, -1.0), (6, -0.5)]      # mu < 0, softness <= 0, stiffness < 0, gain < 0
    for col, v in bad_values:
        p = list(good); p[col] = v
        assert L.ilqr_hip_plant_set_params(h, (C.c_double * 7)(*p), 1) == ERR_ARG, (col, v)
    assert L.ilqr_hip_plant_get_params(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_num_param_sets(h) == 0                              # no table on the zeroed handle


def test_header_and_wrappers_declare_the_feature():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", hdr, re.M), name
        assert name in sv.EXPORTS
    assert re.search(r"^#define\s+ILQR_PLANT_PARAMS\s+7\b", hdr, re.M)
    assert len(sv.PLANT_PARAMS) == 7
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    assert all(m in hpp for m in ("plantSetModel", "plantSetParams", "plantClearParams", "plantParams"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in NAMES)
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the shape checks fail before the library is reached
    s.B, s.N, s.h = 3, 25, None
    for bad in (np.ones(6), np.ones((2, 7)), np.ones((3, 8)), np.ones((1, 3, 7))):
        with pytest.raises(ValueError):
            s.plant_set_params(bad)
    for bad in (5, -1):
        with pytest.raises(ValueError):
            s.plant_set_model(bad, None)


def test_stack_plant_params_broadcasts_and_validates():
    d = sc.PLANT_PARAM_DEFAULTS
    p = sc.stack_plant_params(4)
    assert p.shape == (4, 7) and p.dtype == np.float64
    assert np.array_equal(p, np.tile([0.0, 0.0, -9.81, 1.0, 1e-5, 0.0, 1.0], (4, 1)))      # what ilqr_hip_create leaves in a handle
    assert d["gravity"] == (0.0, 0.0, -9.81) and d["friction"] == 1.0 and d["softness"] == 1e-5 and d["limit_stiffness"] == 0.0 and d["torque_gain"] == 1.0
    g = np.arange(12.0).reshape(4, 3) - 20.0
    p = sc.stack_plant_params(4, gravity=g, friction=[0.1, 0.2, 0.3, 0.4], softness=2e-5, limit_stiffness=np.array([0.0, 1.0, 2.0, 3.0]), torque_gain=0.5)
    assert np.array_equal(p[:, :3], g) and np.array_equal(p[:, 3], [0.1, 0.2, 0.3, 0.4]) and np.all(p[:, 4] == 2e-5)
    assert np.array_equal(p[:, 5], [0.0, 1.0, 2.0, 3.0]) and np.all(p[:, 6] == 0.5)
    p = sc.stack_plant_params(3, gravity=(0.6, -0.4, -9.5))
    assert np.array_equal(p[:, :3], np.tile([0.6, -0.4, -9.5], (3, 1)))
    assert np.array_equal(sc.stack_plant_params(pc.B, gravity=pc.params()[:, :3], friction=pc.params()[:, 3], softness=pc.params()[:, 4],
                                                limit_stiffness=pc.params()[:, 5], torque_gain=pc.params()[:, 6]), pc.params())
    for kw in (dict(gravity=(0.0, -9.81)), dict(gravity=np.zeros((3, 3))), dict(friction=[1.0, 2.0]), dict(softness=np.ones((4, 1))), dict(torque_gain=np.ones(5)),
               dict(friction=-0.1), dict(softness=0.0), dict(softness=[1e-5, 1e-5, -1e-5, 1e-5]), dict(limit_stiffness=-1.0), dict(torque_gain=-1.0),
               dict(friction=float("nan")), dict(gravity=(0.0, 0.0, float("inf")))):
        with pytest.raises(ValueError):
            sc.stack_plant_params(4, **kw)
    with pytest.raises(ValueError):
        sc.stack_plant_params(0)


class _ParamsRecorder(_Recorder):
    def plant_set_model(self, contact_mode=None, joint_limits=None):
        self._rec("plant_set_model(%s,%s)" % (contact_mode, joint_limits))

    def plant_set_params(self, params):
        self._rec("plant_set_params(%d)" % len(params))


def test_runner_refuses_without_the_resident_plant_and_installs_in_order():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    Bn, Nn = 3, 25
    p = sc.stack_plant_params(Bn, friction=[0.3, 0.5, 0.7])
    for kw in (dict(plant_params=p), dict(plant_model=(3, True)), dict(plant_params=p, plant_model=(None, None))):
        with pytest.raises(ValueError, match="resident"):
            ml.MPCRunner(_ParamsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), **kw)
    for bad in (np.ones((2, 7)), np.ones((Bn, 6)), np.ones((1, Bn, 7))):
        with pytest.raises(ValueError):
            ml.MPCRunner(_ParamsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_params=bad)
    with pytest.raises(ValueError):
        ml.MPCRunner(_ParamsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_model=(3,))
    s = _ParamsRecorder(Bn, Nn)
    run = ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True, plant_params=p, plant_model=(3, True))
    run.run(np.zeros((Bn, NX)), 2)
    assert s.calls[:5] == ["plant_set_model(3,True)", "plant_configure(1,0,schedule)", "plant_set_params(3)", "plant_set_history(2)", "plant_reset"], s.calls
    assert s.calls.count("plant_set_params(3)") == 1 and s.calls.count("plant_advance") == 2
    # without either argument the runner issues exactly the calls it issued before
    s = _ParamsRecorder(Bn, Nn)
    ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True).run(np.zeros((Bn, NX)), 2)
    assert not any(c.startswith(("plant_set_model", "plant_set_params")) for c in s.calls)
    one = ml.MPCRunner(_ParamsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_params=p[0])      # one set, given as a vector
    assert one.plant_params.shape == (1, 7)


# ---- the inputs exercise every column (CPU oracle)
def _moved(a, b):
    return np.abs(a - b).max(axis=-1) > 1e-6


def test_every_column_moves_the_oracles_step_on_the_envelope_states():
    """h = 0.02, the envelope's own step: contact mode 3 on the sliding states, modes 0 and 4 with joint-limit rows on the limit states"""
    x, u, _ = cc.sliding_states("mid")
    base_p = pc.SETS[0]
    base = pc.oracle_steps(base_p, 3, False, x, u, dc.H)
    counts = {}
    for name, col, val in (("mu 1e3", 3, 1e3), ("mu 0.7", 3, 0.7), ("softness 1e-4", 4, 1e-4), ("gain 0.8", 6, 0.8)):
        p = base_p.copy(); p[col] = val
        counts[name] = int(_moved(pc.oracle_steps(p, 3, False, x, u, dc.H), base).sum())
    print(counts)
    assert counts == {"mu 1e3": 38, "mu 0.7": 10, "softness 1e-4": 39, "gain 0.8": 64}
    g = base_p.copy(); g[:3] = pc.SETS[1, :3]
    xl, ul = cc.limit_states()
    for mode, limits, xs, us in ((0, False, *dc.mid()), (2, False, x, u), (3, False, x, u), (4, True, xl, ul), (0, True, xl, ul)):
        b0 = pc.oracle_steps(base_p, mode, limits, xs, us, dc.H)
        assert _moved(pc.oracle_steps(g, mode, limits, xs, us, dc.H), b0).all(), ("gravity", mode, limits)
        h8 = base_p.copy(); h8[6] = 0.8
        assert _moved(pc.oracle_steps(h8, mode, limits, xs, us, dc.H), b0).all(), ("gain", mode, limits)
        if limits:
            for k in (625.0, 156.25):
                pk = base_p.copy(); pk[5] = k
                assert _moved(pc.oracle_steps(pk, mode, limits, xs, us, dc.H), b0).all(), ("stiffness", mode, k)


CASES = {"free": (0, False, "mid", pc.STATE_OFFSET), "mode3_sliding": (3, False, "sliding", pc.STATE_OFFSET), "mode4_limits": (4, True, "limits", pc.STATE_OFFSET),
         "mode0_limits": (0, True, "limits", pc.STATE_OFFSET), "mismatch_mode3_limits": (3, True, "limits", pc.STATE_OFFSET_MODE3_LIMITS)}


def envelope_states(group):
    return dc.mid() if group == "mid" else cc.sliding_states("mid")[:2] if group == "sliding" else cc.limit_states()


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_batch_exercises_every_column_in_both_workgroups(case):
    """the first plant step (h = DT / SUBSTEPS) of the batch of the GPU tests: setting any acting column back to set 0's value moves at least
    four rollouts by more than 1e-6, one of them among b = 32..36"""
    mode, limits, group, off = CASES[case]
    x16, u16 = envelope_states(group)
    table = pc.params()
    true = pc.oracle_first_step(table, mode, limits, x16, u16, off)
    assert np.all(np.isfinite(true))
    moved = {name: _moved(pc.oracle_first_step(pc.with_column_shared(table, name), mode, limits, x16, u16, off), true) for name in pc.acting_columns(mode, limits)}
    pc.check_column_conditions(moved, 0, case)
    # ... and a column that does not act in this plant moves nothing at all
    for name in set(pc.COLUMNS) - set(pc.acting_columns(mode, limits)):
        assert np.array_equal(pc.oracle_first_step(pc.with_column_shared(table, name), mode, limits, x16, u16, off), true), (case, name)


def test_batch_layout():
    b = np.arange(pc.B)
    assert pc.B == 37 and pc.N == 6 and pc.SUBSTEPS == 2
    assert np.all(pc.set_of(b[::2]) != pc.set_of(b[::2] + 1)[: len(b[::2])])      # the two rollouts of neighbouring lane pairs never share a set
    assert {(int(s), int(p)) for s, p in zip(pc.set_of(b), pc.pattern_of(b))} == {(s, p) for s in range(3) for p in range(4)}
    assert pc.schedule().shape == (pc.B, pc.N + 1, 2) and np.array_equal(pc.schedule()[5, 3], dc.STANCE_ROWS[1])
    assert np.array_equal(pc.params()[4], pc.SETS[1]) and pc.params().shape == (pc.B, 7)
