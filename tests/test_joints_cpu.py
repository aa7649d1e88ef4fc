"""The per-rollout joint records without a GPU (include/ilqr_hip.h ilqr_hip_plant_set_joints and companions): the golden against the CPU
oracle -- which knows one armature for every hinge, so on the closed form of tests/joints_cases.py --, the nominal record, five wrong
readings of the record, the entry points' argument checks, the Python mirrors and the runner.

Bounds: the closed form at jc.ID_TOL = 1e-6 N / N m (payload_cases.ID_TOL); nominal cases against the oracle's own step 1e-9 relative as
tests/test_payload_cpu.py; every mutant misses the golden by at least 1000 times the bound of the GPU step (1e-10 absolute in mode 0 without
rows, 1e-9 relative otherwise)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import joints_cases as jc
import wrench_cases as wc
from conftest import load_package
from test_plant_cpu import NX, _base, _Recorder, _Refs

pkg = load_package()
sc = pkg.scenario
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NAMES = ("ilqr_hip_plant_set_joints", "ilqr_hip_plant_get_joints", "ilqr_hip_step_joints")


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv, sv.load_library()


# ---- the golden, on the golden alone
def test_golden_covers_the_cases():
    g = jc.golden()
    n = len(g["x"])
    assert 28 <= n <= 40
    J, W, PL, contact, limits, kind = g["joints"], g["wrench"], g["payload"], g["contact"], g["limits"], g["kind"]
    kinds = {(int(c), int(l)) for c, l in zip(contact, limits)}
    assert {(0, 0), (0, 1), (4, 0), (4, 1)} <= kinds and any(c in (1, 2, 3) and l == 0 for c, l in kinds) and any(c in (1, 2, 3) and l == 1 for c, l in kinds)      # six step kinds
    assert {tuple(s) for s in g["stance"]} >= {(1, 1), (1, 0), (0, 1)}
    nominal = (J == jc.NOMINAL).all(axis=1)
    for mode in range(5):
        assert (nominal & (contact == mode)).any(), mode
    gn, sn, dn, an = ((f != 1.0).any(axis=1) if k < 3 else (f != 0.1).any(axis=1) for k, f in enumerate(jc.fields(J)))
    for only, rest in ((gn, sn | dn | an), (sn, gn | dn | an), (dn, gn | sn | an), (an, gn | sn | dn)):
        assert (only & ~rest).any()                                                                                # each field alone
    assert (gn & sn & dn & an).any()                                                                               # all four at once
    assert (J[:, 19 + jc.KNEE] == 0.0).any()                                                                       # a dead knee
    R = g["ctrlrange"]
    gs, ss, _, _ = jc.fields(J)
    u = g["u"]
    assert ((kind == "gain_clamped") & ((np.abs(u) < R) & (np.abs(gs * u) > ss * R)).any(axis=1)).any()            # g u clamped, u not
    assert ((kind == "scale_clamped") & (gs == 1.0).all(axis=1) & ((np.abs(u) < R) & (np.abs(u) > ss * R)).any(axis=1)).any()      # clamped by the scaled range only
    assert (~nominal & (np.abs(W).max(axis=1) > 0)).any() and (~nominal & (PL[:, 0] > 0)).any() and (~nominal & (np.abs(W).max(axis=1) > 0) & (PL[:, 0] > 0)).any()
    tilt = 2.0 * np.arccos(np.clip(np.abs(g["x"][:, 3]), 0.0, 1.0))
    assert (tilt[~nominal] > 0.15).any()                                                                           # a tilted pelvis
    for mode in (2, 3, 4):
        assert (g["changed"][contact == mode] == 1).any(), mode                                                    # another active set than nominal
    assert (g["changed"][limits == 1] == 1).any()
    assert (g["lock"].sum(axis=1)[limits == 1] > 0).any()
    for i in range(n):                                                                                             # what ilqr_hip_plant_set_joints accepts
        gi, si, di, ai = jc.fields(J[i])
        assert np.array_equal(sc.stack_plant_joints(dict(gain=gi, range_scale=si, damping=di, armature=ai), 1)[0], J[i])
        if not nominal[i]:
            assert np.abs(g["x_next"][i] - g["x_next_nominal"][i]).max() > 1e-6, i                                 # the record acts


def test_nominal_record_as_vectors_is_the_scalar_step_to_zero():
    g = jc.golden()
    assert np.array_equal(g["x_next_nominal_vectors"], g["x_next_nominal"])
    nominal = np.flatnonzero((g["joints"] == jc.NOMINAL).all(axis=1))
    assert np.array_equal(g["x_next"][nominal], g["x_next_nominal"][nominal])
    plain = [i for i in nominal if np.abs(g["wrench"][i]).max() == 0 and g["payload"][i, 0] == 0]
    assert len(plain) >= 5
    for i in plain:                                                                                                # ... and the oracle's own step
        got = wc.golden_oracle(g, i).step_stance(g["x"][i], g["u"][i], g["stance"][i])
        want = g["x_next"][i]
        assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) < 1e-9, i


def test_closed_form_on_the_oracles_inverse_dynamics_holds_on_the_golden():
    """the two yardsticks against each other, every case: hinge rows that are not stopped and that no stance row reaches; the base rows on the
    cases without stance rows"""
    g = jc.golden()
    h, grav = float(g["h"]), g["gravity"]
    worst_h = worst_b = 0.0
    rows = bases = 0
    for i in range(len(g["x"])):
        res = jc.hinge_residual(g["x"][i], g["x_next"][i], g["u"][i], h, grav, g["joints"][i])
        free = jc.checked_hinges(g["act"][i], g["lock"][i])
        eh = float(np.abs(res[6:][free]).max())
        worst_h, rows = max(worst_h, eh), rows + int(free.sum())
        eb = -1.0
        if int(g["contact"][i]) == 0:
            eb = float(np.abs(res[:6] - jc.expected_base_rows(g["x"][i], g["x_next"][i], h, grav, g["wrench"][i], g["payload"][i])).max())
            worst_b, bases = max(worst_b, eb), bases + 1
        print("case %2d (%s, mode %d, limits %d): hinge rows %.3e on %2d hinges, base rows %.3e" % (i, g["kind"][i], g["contact"][i], g["limits"][i], eh, free.sum(), eb))
    print("closed form: hinge rows %.3e over %d rows, base rows %.3e over %d cases (bound %.0e)" % (worst_h, rows, worst_b, bases, jc.ID_TOL))
    assert rows >= 300 and bases >= 12
    assert worst_h < jc.ID_TOL and worst_b < jc.ID_TOL


def test_closed_form_tells_the_record_from_the_model():
    """the same residual under the NOMINAL record does not close on the cases whose record is not nominal: the check is not vacuous (without
    stance rows, where every hinge that is not stopped is checked)"""
    g = jc.golden()
    h, grav = float(g["h"]), g["gravity"]
    cases = np.flatnonzero(~(g["joints"] == jc.NOMINAL).all(axis=1) & (g["contact"] == 0))
    assert len(cases) >= 12
    for i in cases:
        res = jc.hinge_residual(g["x"][i], g["x_next"][i], g["u"][i], h, grav, jc.NOMINAL)
        free = jc.checked_hinges(g["act"][i], g["lock"][i])
        assert np.abs(res[6:][free]).max() > 1e3 * jc.ID_TOL, i


@pytest.mark.parametrize("k", range(len(jc.MUTANTS)))
def test_every_wrong_reading_of_the_record_misses_the_golden(k):
    g = jc.golden()
    assert tuple(g["mutants"]) == jc.MUTANTS
    units = [jc.bound_units(g["x_next_mutant"][i, k], g["x_next"][i], int(g["contact"][i]) == 0 and not int(g["limits"][i])) for i in range(len(g["x"]))]
    print("%s: misses the golden by %.2e bounds of the GPU step at most, in %d cases by more than 1000" % (jc.MUTANTS[k], max(units), sum(v >= 1000.0 for v in units)))
    assert max(units) >= 1000.0
    nominal = (g["joints"] == jc.NOMINAL).all(axis=1)
    # no reading is wrong about the model's joints (the mean of nineteen 0.1 is 0.1 to rounding only)
    assert np.abs(g["x_next_mutant"][nominal, k] - g["x_next"][nominal]).max() < 1e-12


# ---- entry points
def test_entry_points_are_exported_and_refuse_a_null_handle():
    sv, L = _lib()
    legacy = C.CDLL(sv.LEGACY_LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name) and hasattr(legacy, name), name
    rec = (C.c_double * 76)(*jc.NOMINAL)
    x, u = (C.c_double * 51)(), (C.c_double * 19)()
    assert L.ilqr_hip_plant_set_joints(None, rec, 1) == ERR_ARG
    assert L.ilqr_hip_plant_get_joints(None, rec) == ERR_ARG
    assert L.ilqr_hip_step_joints(None, 1, x, u, 1, 1, None, None, rec, x) == ERR_ARG


def test_the_built_module_exports_its_entry_points():
    sv, L = _lib()
    path = os.path.join(os.path.dirname(sv.LIB_PATH), "libilqr_hip_joints.so")
    assert os.path.exists(path), path
    M = C.CDLL(path)
    for name in ("ilqr_joints_module_set_attr", "ilqr_joints_module_follow", "ilqr_joints_module_step"):
        assert hasattr(M, name), name


def test_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    """as tests/test_plant_cpu.py: the handle is a block of zeroed memory (batch 0) that a call which got past its checks would have to use"""
    sv, L = _lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    good = list(jc.NOMINAL)
    assert L.ilqr_hip_plant_set_joints(h, None, 1) == ERR_ARG                 # (NULL clears only with n_sets 0)
    assert L.ilqr_hip_plant_set_joints(h, (C.c_double * 76)(*good), 0) == ERR_ARG
    for n_sets in (-1, 2, 37):                                                # neither 1 nor the batch (0 on this handle)
        assert L.ilqr_hip_plant_set_joints(h, (C.c_double * (76 * 37))(*(good * 37)), n_sets) == ERR_ARG, n_sets
    x, u = (C.c_double * 51)(), (C.c_double * 19)()
    for col in (0, 18, 19, 37, 38, 56, 57, 75):
        for v in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-300):
            p = list(good); p[col] = v
            assert L.ilqr_hip_plant_set_joints(h, (C.c_double * 76)(*p), 1) == ERR_ARG, (col, v)
            assert L.ilqr_hip_step_joints(h, 1, x, u, 1, 1, None, None, (C.c_double * 76)(*p), x) == ERR_ARG, (col, v)
    assert L.ilqr_hip_plant_get_joints(h, None) == ERR_ARG
    j, w, m = (C.c_double * 76)(*good), (C.c_double * 9)(), (C.c_double * 10)()
    for args in ((0, x, u, 1, 1, w, m, j, x), (-3, x, u, 1, 1, w, m, j, x), (1, None, u, 1, 1, w, m, j, x), (1, x, None, 1, 1, w, m, j, x), (1, x, u, 1, 1, w, m, None, x),
                 (1, x, u, 1, 1, w, m, j, None)):
        assert L.ilqr_hip_step_joints(h, *args) == ERR_ARG, args
    wb = [0.0] * 9; wb[4] = float("nan")
    assert L.ilqr_hip_step_joints(h, 1, x, u, 1, 1, (C.c_double * 9)(*wb), m, j, x) == ERR_ARG
    mb = [0.0] * 10; mb[0] = -1.0
    assert L.ilqr_hip_step_joints(h, 1, x, u, 1, 1, w, (C.c_double * 10)(*mb), j, x) == ERR_ARG


def test_header_and_wrappers_declare_the_feature():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", hdr, re.M), name
    assert all(name in sv.EXPORTS for name in NAMES)
    assert re.search(r"^#define\s+ILQR_PLANT_JOINTS\s+76\b", hdr, re.M)
    assert sv.PLANT_JOINTS == 76 and [f for f, _ in sv.PLANT_JOINT_FIELDS] == ["gain", "range_scale", "damping", "armature"]
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    assert all(m in hpp for m in ("plantSetJoints", "plantClearJoints", "plantJoints", "stepJoints"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ilqr_hip_plant_set_joints" in design and "k_plant_follow_j" in design and "A joint that is not the model's" in design
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the shape checks fail before the library is reached
    s.B, s.N, s.h = 3, 25, None
    for bad in (np.ones(75), np.ones((2, 76)), np.ones((3, 77)), np.ones((1, 3, 76))):
        with pytest.raises(ValueError):
            s.plant_set_joints(bad)
    with pytest.raises(ValueError):
        s.step_joints(np.zeros((2, 51)), np.zeros((2, 19)), 1, 1, np.zeros((2, 75)))
    with pytest.raises(ValueError):
        s.step_joints(np.zeros((2, 51)), np.zeros((2, 19)), 1, 1, np.ones((2, 76)), wrench=np.zeros((2, 11)))
    with pytest.raises(ValueError):
        s.step_joints(np.zeros((2, 51)), np.zeros((2, 19)), 1, 1, np.ones((2, 76)), payload=np.zeros((2, 9)))


def test_stack_plant_joints_defaults_broadcasts_and_validates():
    B = 4
    assert np.array_equal(sc.stack_plant_joints({}, B), np.tile(jc.NOMINAL, (B, 1)))                   # defaults: the model's joints
    t = sc.stack_plant_joints(dict(gain=0.8, armature=np.linspace(0.05, 0.2, 19)), B)
    assert t.shape == (B, 76) and (t[:, 0:19] == 0.8).all() and (t[:, 19:57] == 1.0).all() and np.array_equal(t[2, 57:76], np.linspace(0.05, 0.2, 19))
    recs = [dict(), dict(range_scale=np.r_[np.ones(3), 0.0, np.ones(15)]), dict(damping=2.0), dict(gain=np.arange(19.0), range_scale=0.5, damping=0.0, armature=0.0)]
    t = sc.stack_plant_joints(recs, B)
    assert np.array_equal(t[0], jc.NOMINAL) and t[1, 19 + jc.KNEE] == 0.0 and (t[1, 0:19] == 1.0).all() and (t[2, 38:57] == 2.0).all() and (t[2, 57:76] == 0.1).all()
    assert np.array_equal(t[3], np.r_[np.arange(19.0), 0.5 * np.ones(19), np.zeros(38)])
    assert sc.stack_plant_joints([dict(gain=2.0)], 1).shape == (1, 76)
    for bad, Bn in ((dict(gain=-0.1), B), (dict(damping=float("nan")), B), (dict(armature=float("inf")), B), (dict(range_scale=np.ones(18)), B), (dict(gain=np.ones((B, 19))), B),
                    (dict(stiffness=1.0), B), ([dict()] * 3, B), ([dict(), 1.0, dict(), dict()], B), (dict(), 0)):
        with pytest.raises(ValueError):
            sc.stack_plant_joints(bad, Bn)


class _JointsRecorder(_Recorder):
    def plant_set_actuator(self, actuator, seed=0, stream0=0):
        self._rec("plant_set_actuator(%d,%d,%d)" % (len(actuator), seed, stream0))

    def plant_set_joints(self, joints):
        self._rec("plant_set_joints(%d)" % len(joints))


def test_runner_refuses_without_the_resident_plant_and_installs_in_order():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    Bn, Nn = 3, 25
    j = sc.stack_plant_joints([dict(gain=0.9), dict(damping=2.0), dict(range_scale=0.5)], Bn)
    a = sc.stack_plant_actuator(Bn, delay=[0, 2, 4], tau=0.02)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_JointsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_joints=j)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_JointsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_joints=j, resident=False)
    for bad in (np.ones((2, 76)), np.ones((Bn, 75)), np.ones((1, Bn, 76))):
        with pytest.raises(ValueError):
            ml.MPCRunner(_JointsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_joints=bad)
    s = _JointsRecorder(Bn, Nn)
    run = ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True, substeps=3, plant_actuator=a, actuator_seed=77, actuator_stream0=5, plant_joints=j)
    run.run(np.zeros((Bn, NX)), 2)
    head = ["plant_configure(3,0,schedule)", "plant_set_actuator(3,77,5)", "plant_set_joints(3)", "plant_set_history(2)", "plant_reset"]
    assert s.calls[:5] == head, s.calls
    assert s.calls.count("plant_advance") == 2
    s = _JointsRecorder(Bn, Nn)
    ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True).run(np.zeros((Bn, NX)), 2)
    assert not any(c.startswith("plant_set_joints") for c in s.calls)
    one = ml.MPCRunner(_JointsRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_joints=j[1])      # one record, given as a vector
    assert one.plant_joints.shape == (1, 76)
