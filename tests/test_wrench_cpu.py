"""The external wrench on the pelvis without a GPU (include/ilqr_hip.h ilqr_hip_plant_set_wrench and companions): the golden against the CPU
oracle -- which has no wrench, so on what the oracle can say about a step under one, tests/wrench_cases.py --, the entry points' argument
checks, the Python mirrors and the runner's call order."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wrench_cases as wc
from conftest import load_package
from test_plant_cpu import NX, _base, _Recorder, _Refs

pkg = load_package()
sc = pkg.scenario
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
INT_NAMES = ("ilqr_hip_plant_set_wrench", "ilqr_hip_plant_clear_wrench", "ilqr_hip_plant_num_wrench_sets", "ilqr_hip_plant_get_wrench", "ilqr_hip_step_wrench")
NAMES = INT_NAMES + ("ilqr_hip_plant_intervals", "ilqr_hip_pelvis_inertial_offset")


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv, sv.load_library()


# ---- the golden, on the golden alone
def test_golden_covers_the_cases():
    g = wc.golden()
    n = len(g["x"])
    assert n <= 40
    W, contact, limits = g["wrench"], g["contact"], g["limits"]
    zero = np.abs(W).max(axis=1) == 0
    kinds = {(int(c), int(l)) for c, l in zip(contact, limits)}
    assert {(0, 0), (0, 1), (4, 0), (4, 1)} <= kinds and any(c in (1, 2, 3) and l == 0 for c, l in kinds) and any(c in (1, 2, 3) and l == 1 for c, l in kinds)      # six step kinds
    assert {tuple(s) for s in g["stance"]} >= {(1, 1), (1, 0), (0, 1)}
    nz = ~zero
    assert (np.abs(W[nz, 6:9]).max(axis=1) == 0).any() and (np.abs(W[nz, 6:9]).max(axis=1) > 0).any()              # r = 0 and r != 0
    f, t = np.abs(W[:, 0:3]).max(axis=1) > 0, np.abs(W[:, 3:6]).max(axis=1) > 0
    assert (f & ~t).any() and (~f & t).any() and (f & t).any()                                                     # force only, torque only, both
    assert np.linalg.norm(W[:, 0:3], axis=1).max() <= 150.0 + 1e-9 and np.linalg.norm(W[:, 3:6], axis=1).max() <= 40.0 + 1e-9
    tilt = 2.0 * np.arccos(np.clip(np.abs(g["x"][:, 3]), 0.0, 1.0))
    assert (tilt[nz] > 0.15).any()                                                                                 # a tilted pelvis
    for mode in range(5):
        assert (zero & (contact == mode)).any(), mode
    for mode in (2, 3, 4):                                                                                         # (mode 1 is bilateral: no active set)
        assert (g["changed"][contact == mode] == 1).any(), mode
    assert (g["lock"].sum(axis=1)[limits == 1] > 0).any()


def test_zero_wrench_cases_are_the_oracles_step():
    g = wc.golden()
    zero = np.flatnonzero(np.abs(g["wrench"]).max(axis=1) == 0)
    assert len(zero) >= 5
    for i in zero:
        got = wc.golden_oracle(g, i).step_stance(g["x"][i], g["u"][i], g["stance"][i])
        want = g["x_next"][i]
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        assert err < 1e-9, (i, err)


def test_base_rows_of_the_inverse_dynamics_are_the_wrench():
    """contact mode 0, without and with joint-limit rows (step kinds 0 and 5)"""
    g = wc.golden()
    h, grav = float(g["h"]), g["gravity"]
    cases = np.flatnonzero(g["contact"] == 0)
    assert len(cases) >= 8
    worst = 0.0
    for i in cases:
        res = wc.inverse_dynamics_residual(g["x"][i], g["x_next"][i], g["u"][i], h, grav)
        err = np.abs(res[:6] - wc.generalized_force(g["x"][i], g["wrench"][i])).max()
        worst = max(worst, err)
        assert err < 1e-9, (i, err)
        free = g["lock"][i] == 0
        assert np.abs(res[6:][free]).max() < 1e-9, (i, np.abs(res[6:][free]).max())
    print("mode 0: base rows of the inverse dynamics against Wg, worst %.3e" % worst)


def test_upper_body_hinge_rows_close_under_stance_rows():
    g = wc.golden()
    h, grav = float(g["h"]), g["gravity"]
    cases = np.flatnonzero(g["contact"] > 0)
    assert len(cases) >= 15
    worst = 0.0
    for i in cases:
        res = wc.inverse_dynamics_residual(g["x"][i], g["x_next"][i], g["u"][i], h, grav)
        rows = [j for j in wc.UPPER if g["lock"][i][j] == 0]
        err = np.abs(res[6:][rows]).max()
        worst = max(worst, err)
        assert err < 1e-11, (i, err)
    print("contact modes: torso and arm hinge rows, worst %.3e" % worst)


def test_every_wrench_moves_the_step():
    g = wc.golden()
    for i in np.flatnonzero(np.abs(g["wrench"]).max(axis=1) > 0):
        twin = wc.golden_oracle(g, i).step_stance(g["x"][i], g["u"][i], g["stance"][i])
        assert np.abs(g["x_next"][i] - twin).max() > 1e-6, i


# ---- entry points
def test_entry_points_are_exported_and_refuse_a_null_handle():
    sv, L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
    rec = (C.c_double * 11)(*([0.0] * 10 + [1.0]))
    x, u = (C.c_double * 51)(), (C.c_double * 19)()
    assert L.ilqr_hip_plant_set_wrench(None, rec, 1) == ERR_ARG
    assert L.ilqr_hip_plant_clear_wrench(None) == ERR_ARG
    assert L.ilqr_hip_plant_num_wrench_sets(None) == -1
    assert L.ilqr_hip_plant_get_wrench(None, rec) == ERR_ARG
    L.ilqr_hip_plant_intervals.restype = C.c_long
    assert L.ilqr_hip_plant_intervals(None) == -1
    assert L.ilqr_hip_step_wrench(None, 1, x, u, 1, 1, rec, x) == ERR_ARG


def test_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    """as tests/test_plant_cpu.py: the handle is a block of zeroed memory (batch 0) that a call which got past its checks would have to use"""
    sv, L = _lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    good = [10.0, 0.0, -5.0, 1.0, 2.0, 3.0, 0.01, 0.0, -0.04, 2.0, 5.0]
    assert L.ilqr_hip_plant_set_wrench(h, None, 1) == ERR_ARG
    for n_sets in (0, -1, 2, 37):                                          # neither 1 nor the batch (0 on this handle, and 0 sets is no table)
        assert L.ilqr_hip_plant_set_wrench(h, (C.c_double * (11 * 37))(*(good * 37)), n_sets) == ERR_ARG, n_sets
    inf, nan = float("inf"), float("nan")
    bad = [(c, v) for c in range(10) for v in (nan, inf, -inf)] + [(10, nan), (10, -inf)]
    bad += [(9, -1.0), (10, -1.0), (9, 2.5), (10, 5.5), (9, 6.0)]              # negative, non-integral, end < first
    for col, v in bad:
        p = list(good); p[col] = v
        assert L.ilqr_hip_plant_set_wrench(h, (C.c_double * 11)(*p), 1) == ERR_ARG, (col, v)
    p = list(good); p[9] = inf; p[10] = inf                                     # (first must be finite even under an infinite end)
    assert L.ilqr_hip_plant_set_wrench(h, (C.c_double * 11)(*p), 1) == ERR_ARG
    assert L.ilqr_hip_plant_get_wrench(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_num_wrench_sets(h) == 0 and L.ilqr_hip_plant_intervals(h) == 0      # no table, no interval on the zeroed handle
    x, u, w = (C.c_double * 51)(), (C.c_double * 19)(), (C.c_double * 9)(*good[:9])
    for args in ((0, x, u, 1, 1, w, x), (-3, x, u, 1, 1, w, x), (1, None, u, 1, 1, w, x), (1, x, None, 1, 1, w, x), (1, x, u, 1, 1, None, x), (1, x, u, 1, 1, w, None)):
        assert L.ilqr_hip_step_wrench(h, *args) == ERR_ARG, args
    for col in range(9):
        for v in (nan, inf):
            p = list(good[:9]); p[col] = v
            assert L.ilqr_hip_step_wrench(h, 1, x, u, 1, 1, (C.c_double * 9)(*p), x) == ERR_ARG, (col, v)


def test_header_and_wrappers_declare_the_feature():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for name in INT_NAMES:
        assert re.search(r"^int " + name + r"\s*\(", hdr, re.M), name
    assert re.search(r"^long ilqr_hip_plant_intervals\s*\(", hdr, re.M) and re.search(r"^void ilqr_hip_pelvis_inertial_offset\s*\(", hdr, re.M)
    assert all(name in sv.EXPORTS for name in NAMES)
    assert re.search(r"^#define\s+ILQR_PLANT_WRENCH\s+11\b", hdr, re.M)
    assert len(sv.PLANT_WRENCH) == 11
    assert "Not provided: external wrenches" not in hdr
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    assert all(m in hpp for m in ("plantSetWrench", "plantClearWrench", "plantNumWrenchSets", "plantWrench", "plantIntervals", "stepWrench", "pelvisInertialOffset"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ilqr_hip_plant_set_wrench" in design and "k_plant_follow_w" in design
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the shape checks fail before the library is reached
    s.B, s.N, s.h = 3, 25, None
    for bad in (np.ones(10), np.ones((2, 11)), np.ones((3, 12)), np.ones((1, 3, 11))):
        with pytest.raises(ValueError):
            s.plant_set_wrench(bad)
    with pytest.raises(ValueError):
        s.step_wrench(np.zeros((2, 51)), np.zeros((2, 19)), 1, 1, np.zeros((2, 11)))


def test_pelvis_inertial_offset_is_the_model_constant():
    sv, L = _lib()
    r = sv.pelvis_inertial_offset()
    assert r.shape == (3,) and np.array_equal(r, wc.golden()["pelvis_com"])      # h1.xml: <inertial pos> of the pelvis, as the generator parsed it
    assert np.array_equal(r, [-0.0002, 4e-05, -0.04522])


def test_stack_plant_wrench_broadcasts_and_validates():
    w = sc.stack_plant_wrench(4)
    assert w.shape == (4, 11) and w.dtype == np.float64
    assert np.array_equal(w[:, :10], np.zeros((4, 10))) and np.all(np.isposinf(w[:, 10]))
    F = np.arange(12.0).reshape(4, 3)
    w = sc.stack_plant_wrench(4, force=F, torque=(1.0, 2.0, 3.0), point=[0.1, 0.0, -0.2], first=[0, 1, 2, 3], end=7)
    assert np.array_equal(w[:, 0:3], F) and np.array_equal(w[:, 3:6], np.tile([1.0, 2.0, 3.0], (4, 1))) and np.array_equal(w[:, 6:9], np.tile([0.1, 0.0, -0.2], (4, 1)))
    assert np.array_equal(w[:, 9], [0, 1, 2, 3]) and np.all(w[:, 10] == 7)
    w = sc.stack_plant_wrench(2, force=(0.0, 50.0, 0.0), first=3, end=[3, np.inf])                               # an empty window is allowed
    assert np.array_equal(w[:, 9], [3, 3]) and w[0, 10] == 3 and np.isposinf(w[1, 10])
    for kw in (dict(force=(1.0, 2.0)), dict(force=np.zeros((3, 3))), dict(torque=np.zeros((4, 1))), dict(point=np.zeros(4)), dict(first=[0, 1]), dict(end=np.ones((4, 1))),
               dict(force=(0.0, np.nan, 0.0)), dict(torque=(np.inf, 0.0, 0.0)), dict(point=(0.0, 0.0, -np.inf)), dict(first=np.inf), dict(first=np.nan), dict(end=np.nan), dict(end=-np.inf),
               dict(first=-1), dict(end=-2), dict(first=0.5), dict(end=2.5), dict(first=3, end=2)):
        with pytest.raises(ValueError):
            sc.stack_plant_wrench(4, **kw)
    with pytest.raises(ValueError):
        sc.stack_plant_wrench(0)


class _WrenchRecorder(_Recorder):
    def plant_set_model(self, contact_mode=None, joint_limits=None):
        self._rec("plant_set_model(%s,%s)" % (contact_mode, joint_limits))

    def plant_set_params(self, params):
        self._rec("plant_set_params(%d)" % len(params))

    def plant_set_wrench(self, wrench):
        self._rec("plant_set_wrench(%d)" % len(wrench))


def test_runner_refuses_without_the_resident_plant_and_installs_in_order():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    Bn, Nn = 3, 25
    w = sc.stack_plant_wrench(Bn, force=(0.0, 40.0, 0.0), first=1, end=3)
    p = sc.stack_plant_params(Bn, friction=[0.3, 0.5, 0.7])
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_WrenchRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_wrench=w)
    for bad in (np.ones((2, 11)), np.ones((Bn, 10)), np.ones((1, Bn, 11))):
        with pytest.raises(ValueError):
            ml.MPCRunner(_WrenchRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_wrench=bad)
    s = _WrenchRecorder(Bn, Nn)
    run = ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True, plant_params=p, plant_model=(3, True), plant_wrench=w)
    run.run(np.zeros((Bn, NX)), 2)
    assert s.calls[:6] == ["plant_set_model(3,True)", "plant_configure(1,0,schedule)", "plant_set_params(3)", "plant_set_wrench(3)", "plant_set_history(2)", "plant_reset"], s.calls
    assert s.calls.count("plant_set_wrench(3)") == 1 and s.calls.count("plant_advance") == 2
    s = _WrenchRecorder(Bn, Nn)
    ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True).run(np.zeros((Bn, NX)), 2)
    assert not any(c.startswith("plant_set_wrench") for c in s.calls)
    one = ml.MPCRunner(_WrenchRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_wrench=w[0])      # one record, given as a vector
    assert one.plant_wrench.shape == (1, 11)
