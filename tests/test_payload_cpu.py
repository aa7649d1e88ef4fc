"""The rigid payload on the pelvis without a GPU (include/ilqr_hip.h ilqr_hip_plant_set_payload and companions): the golden against the CPU
oracle -- which has no payload, so on what the oracle can say about a step under one, tests/payload_cases.py --, the entry points' argument
checks, the Python mirrors and the runner's call order.

Bounds: zero-payload cases and the hinge rows as tests/test_wrench_cpu.py (1e-9 relative, 1e-11 N m); the closed form of the payload on
the kind-0 golden cases at pc.ID_TOL = 1e-6 N."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import payload_cases as pc
import wrench_cases as wc
from conftest import load_package
from test_plant_cpu import NX, _base, _Recorder, _Refs

pkg = load_package()
sc = pkg.scenario
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NAMES = ("ilqr_hip_plant_set_payload", "ilqr_hip_plant_clear_payload", "ilqr_hip_plant_num_payload_sets", "ilqr_hip_plant_get_payload", "ilqr_hip_step_payload")


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv, sv.load_library()


# ---- the golden, on the golden alone
def test_golden_covers_the_cases():
    g = pc.golden()
    n = len(g["x"])
    assert 28 <= n <= 40
    PL, W, contact, limits = g["payload"], g["wrench"], g["contact"], g["limits"]
    zero = np.abs(PL).max(axis=1) == 0
    kinds = {(int(c), int(l)) for c, l in zip(contact, limits)}
    assert {(0, 0), (0, 1), (4, 0), (4, 1)} <= kinds and any(c in (1, 2, 3) and l == 0 for c, l in kinds) and any(c in (1, 2, 3) and l == 1 for c, l in kinds)      # six step kinds
    assert {tuple(s) for s in g["stance"]} >= {(1, 1), (1, 0), (0, 1)}
    for mode in range(5):
        assert (zero & (contact == mode)).any(), mode                                                              # a zero payload per contact mode
    nz = ~zero
    at_origin, with_ic = np.abs(PL[:, 1:4]).max(axis=1) == 0, np.abs(PL[:, 4:10]).max(axis=1) > 0
    assert (nz & at_origin & ~with_ic).any() and (nz & ~at_origin & ~with_ic).any() and (nz & with_ic).any()        # point mass at the origin / at an offset / with Ic
    assert (PL[:, 0] == 20.0).any() and PL[:, 0].max() <= 20.0 and abs(float(g["pelvis_mass"]) - 5.39) < 1e-9       # the heavy one against the pelvis
    tilt = 2.0 * np.arccos(np.clip(np.abs(g["x"][:, 3]), 0.0, 1.0))
    assert (tilt[nz] > 0.15).any()                                                                                 # a tilted pelvis
    assert (nz & (np.abs(W).max(axis=1) > 0)).any()                                                                # a payload and a wrench together
    for mode in (2, 3, 4):
        assert (g["changed"][contact == mode] == 1).any(), mode                                                    # another active set than unloaded
    assert (g["lock"].sum(axis=1)[limits == 1] > 0).any()
    for i in range(n):                                                                                             # what ilqr_hip_plant_set_payload accepts
        assert np.array_equal(sc.stack_plant_payload(1, PL[i, 0], PL[i, 1:4], PL[i, 4:10])[0], PL[i])


def test_zero_payload_cases_are_the_oracles_step():
    g = pc.golden()
    zero = np.flatnonzero((np.abs(g["payload"]).max(axis=1) == 0) & (np.abs(g["wrench"]).max(axis=1) == 0))
    assert len(zero) >= 5
    for i in zero:
        got = wc.golden_oracle(g, i).step_stance(g["x"][i], g["u"][i], g["stance"][i])
        want = g["x_next"][i]
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        assert err < 1e-9, (i, err)


def test_closed_form_of_the_payload_holds_on_the_kind0_golden_cases():
    """the two yardsticks against each other: the oracle's inverse dynamics of the golden's own x_next, contact mode 0 without limit rows"""
    g = pc.golden()
    h, grav = float(g["h"]), g["gravity"]
    cases = np.flatnonzero((g["contact"] == 0) & (g["limits"] == 0))
    assert len(cases) >= 5 and (g["payload"][cases, 0] > 0).sum() >= 4
    worst_b = worst_h = 0.0
    for i in cases:
        res = wc.inverse_dynamics_residual(g["x"][i], g["x_next"][i], g["u"][i], h, grav)
        want = pc.expected_base_rows(g["x"][i], g["x_next"][i], h, grav, g["payload"][i], g["wrench"][i])
        eb, eh = float(np.abs(res[:6] - want).max()), float(np.abs(res[6:]).max())
        print("case %2d: payload %.1f kg, |Fw ; tb| %.1f: base rows against the closed form %.3e, hinge rows %.3e" % (i, g["payload"][i, 0], np.abs(want).max(), eb, eh))
        worst_b, worst_h = max(worst_b, eb), max(worst_h, eh)
    assert worst_b < pc.ID_TOL and worst_h < pc.ID_TOL, (worst_b, worst_h)


def test_closed_form_holds_with_limit_rows_on_the_hinges_that_are_free():
    """contact mode 0 with joint-limit rows (step kind 5): limit rows act on hinge rows only"""
    g = pc.golden()
    h, grav = float(g["h"]), g["gravity"]
    cases = np.flatnonzero((g["contact"] == 0) & (g["limits"] == 1))
    assert len(cases) >= 3
    for i in cases:
        res = wc.inverse_dynamics_residual(g["x"][i], g["x_next"][i], g["u"][i], h, grav)
        want = pc.expected_base_rows(g["x"][i], g["x_next"][i], h, grav, g["payload"][i], g["wrench"][i])
        free = g["lock"][i] == 0
        assert np.abs(res[:6] - want).max() < pc.ID_TOL and np.abs(res[6:][free]).max() < pc.ID_TOL, i


def test_upper_body_hinge_rows_close_under_stance_rows():
    g = pc.golden()
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


def test_every_payload_moves_the_step():
    g = pc.golden()
    nz = np.flatnonzero(np.abs(g["payload"]).max(axis=1) > 0)
    assert len(nz) >= 20
    for i in nz:
        assert np.abs(g["x_next"][i] - g["x_next_nopayload"][i]).max() > 1e-6, i


# ---- entry points
GOOD = [8.0, -0.12, 0.03, 0.25, 0.2, 0.3, 0.25, 0.02, -0.01, 0.03]


def test_entry_points_are_exported_and_refuse_a_null_handle():
    sv, L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
    rec = (C.c_double * 10)(*GOOD)
    x, u = (C.c_double * 51)(), (C.c_double * 19)()
    assert L.ilqr_hip_plant_set_payload(None, rec, 1) == ERR_ARG
    assert L.ilqr_hip_plant_clear_payload(None) == ERR_ARG
    assert L.ilqr_hip_plant_num_payload_sets(None) == -1
    assert L.ilqr_hip_plant_get_payload(None, rec) == ERR_ARG
    assert L.ilqr_hip_step_payload(None, 1, x, u, 1, 1, None, rec, x) == ERR_ARG


BAD_RECORDS = [(c, v) for c in range(10) for v in (float("nan"), float("inf"), -float("inf"))] + [
    (0, -1.0), (0, -1e-300),                        # m < 0
    (4, -0.1), (5, -0.1), (6, -1e-9),               # a negative principal moment
    (7, 0.3), (8, -0.3), (9, 0.3),                  # a 2 x 2 minor below zero: Ixy^2 > Ixx Iyy, ...
]
# all 2 x 2 minors positive, the determinant negative
INDEFINITE = [1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.9, 0.9, -0.9]


def test_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    """as tests/test_plant_cpu.py: the handle is a block of zeroed memory (batch 0) that a call which got past its checks would have to use"""
    sv, L = _lib()
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert L.ilqr_hip_plant_set_payload(h, None, 1) == ERR_ARG
    for n_sets in (0, -1, 2, 37):                                          # neither 1 nor the batch (0 on this handle, and 0 sets is no table)
        assert L.ilqr_hip_plant_set_payload(h, (C.c_double * (10 * 37))(*(GOOD * 37)), n_sets) == ERR_ARG, n_sets
    x, u = (C.c_double * 51)(), (C.c_double * 19)()
    for col, v in BAD_RECORDS:
        p = list(GOOD); p[col] = v
        assert L.ilqr_hip_plant_set_payload(h, (C.c_double * 10)(*p), 1) == ERR_ARG, (col, v)
        assert L.ilqr_hip_step_payload(h, 1, x, u, 1, 1, None, (C.c_double * 10)(*p), x) == ERR_ARG, (col, v)
    assert L.ilqr_hip_plant_set_payload(h, (C.c_double * 10)(*INDEFINITE), 1) == ERR_ARG
    assert L.ilqr_hip_plant_get_payload(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_num_payload_sets(h) == 0                        # no table on the zeroed handle
    m, w = (C.c_double * 10)(*GOOD), (C.c_double * 9)()
    for args in ((0, x, u, 1, 1, w, m, x), (-3, x, u, 1, 1, w, m, x), (1, None, u, 1, 1, w, m, x), (1, x, None, 1, 1, w, m, x), (1, x, u, 1, 1, w, None, x), (1, x, u, 1, 1, w, m, None)):
        assert L.ilqr_hip_step_payload(h, *args) == ERR_ARG, args
    for col in range(9):
        wb = [0.0] * 9; wb[col] = float("nan")
        assert L.ilqr_hip_step_payload(h, 1, x, u, 1, 1, (C.c_double * 9)(*wb), m, x) == ERR_ARG, col


def test_header_and_wrappers_declare_the_feature():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", hdr, re.M), name
    assert all(name in sv.EXPORTS for name in NAMES)
    assert re.search(r"^#define\s+ILQR_PLANT_PAYLOAD\s+10\b", hdr, re.M)
    assert len(sv.PLANT_PAYLOAD) == 10
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    assert all(m in hpp for m in ("plantSetPayload", "plantClearPayload", "plantNumPayloadSets", "plantPayload", "stepPayload"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ilqr_hip_plant_set_payload" in design and "k_plant_follow_m" in design
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the shape checks fail before the library is reached
    s.B, s.N, s.h = 3, 25, None
    for bad in (np.ones(9), np.ones((2, 10)), np.ones((3, 11)), np.ones((1, 3, 10))):
        with pytest.raises(ValueError):
            s.plant_set_payload(bad)
    with pytest.raises(ValueError):
        s.step_payload(np.zeros((2, 51)), np.zeros((2, 19)), 1, 1, np.zeros((2, 9)))
    with pytest.raises(ValueError):
        s.step_payload(np.zeros((2, 51)), np.zeros((2, 19)), 1, 1, np.zeros((2, 10)), wrench=np.zeros((2, 11)))


def test_stack_plant_payload_broadcasts_and_validates():
    p = sc.stack_plant_payload(4, 0.0)
    assert p.shape == (4, 10) and p.dtype == np.float64 and np.array_equal(p, np.zeros((4, 10)))
    m = np.array([0.0, 5.0, 10.0, 20.0])
    p = sc.stack_plant_payload(4, m, com=(-0.1, 0.0, 0.3), inertia=[0.2, 0.3, 0.25, 0.02, -0.01, 0.03])
    assert np.array_equal(p[:, 0], m) and np.array_equal(p[:, 1:4], np.tile([-0.1, 0.0, 0.3], (4, 1))) and np.array_equal(p[:, 4:10], np.tile([0.2, 0.3, 0.25, 0.02, -0.01, 0.03], (4, 1)))
    c = np.arange(12.0).reshape(4, 3) / 40.0
    p = sc.stack_plant_payload(4, 3.0, com=c)
    assert np.array_equal(p[:, 0], np.full(4, 3.0)) and np.array_equal(p[:, 1:4], c) and np.array_equal(p[:, 4:], np.zeros((4, 6)))
    p = sc.stack_plant_payload(2, 1.0, inertia=[1.0, 1.0, 0.0, 1.0, 0.0, 0.0])                                        # semidefinite (rank one) is allowed
    assert p.shape == (2, 10)
    for kw in (dict(mass=[1.0, 2.0]), dict(mass=np.ones((4, 1))), dict(mass=1.0, com=(0.1, 0.2)), dict(mass=1.0, com=np.zeros((3, 3))), dict(mass=1.0, inertia=np.zeros(3)),
               dict(mass=1.0, inertia=np.zeros((4, 3))), dict(mass=np.nan), dict(mass=np.inf), dict(mass=-1.0), dict(mass=[1.0, 1.0, 1.0, -0.5]), dict(mass=1.0, com=(0.0, np.nan, 0.0)),
               dict(mass=1.0, com=(np.inf, 0.0, 0.0)), dict(mass=1.0, inertia=[0.1, 0.1, np.nan, 0, 0, 0]), dict(mass=1.0, inertia=[-0.1, 0.1, 0.1, 0, 0, 0]),
               dict(mass=1.0, inertia=[0.1, 0.1, 0.1, 0.2, 0, 0]), dict(mass=1.0, inertia=INDEFINITE[4:])):
        with pytest.raises(ValueError):
            sc.stack_plant_payload(4, **kw)
    with pytest.raises(ValueError):
        sc.stack_plant_payload(0, 1.0)


class _PayloadRecorder(_Recorder):
    def plant_set_model(self, contact_mode=None, joint_limits=None):
        self._rec("plant_set_model(%s,%s)" % (contact_mode, joint_limits))

    def plant_set_params(self, params):
        self._rec("plant_set_params(%d)" % len(params))

    def plant_set_wrench(self, wrench):
        self._rec("plant_set_wrench(%d)" % len(wrench))

    def plant_set_payload(self, payload):
        self._rec("plant_set_payload(%d)" % len(payload))


def test_runner_refuses_without_the_resident_plant_and_installs_in_order():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    Bn, Nn = 3, 25
    w = sc.stack_plant_wrench(Bn, force=(0.0, 40.0, 0.0), first=1, end=3)
    p = sc.stack_plant_params(Bn, friction=[0.3, 0.5, 0.7])
    m = sc.stack_plant_payload(Bn, [0.0, 5.0, 15.0], com=(-0.1, 0.0, 0.3))
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_PayloadRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_payload=m)
    for bad in (np.ones((2, 10)), np.ones((Bn, 11)), np.ones((1, Bn, 10))):
        with pytest.raises(ValueError):
            ml.MPCRunner(_PayloadRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_payload=bad)
    s = _PayloadRecorder(Bn, Nn)
    run = ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True, plant_params=p, plant_model=(3, True), plant_wrench=w, plant_payload=m)
    run.run(np.zeros((Bn, NX)), 2)
    assert s.calls[:7] == ["plant_set_model(3,True)", "plant_configure(1,0,schedule)", "plant_set_params(3)", "plant_set_wrench(3)", "plant_set_payload(3)", "plant_set_history(2)", "plant_reset"], s.calls
    assert s.calls.count("plant_set_payload(3)") == 1 and s.calls.count("plant_advance") == 2
    s = _PayloadRecorder(Bn, Nn)
    ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True).run(np.zeros((Bn, NX)), 2)
    assert not any(c.startswith("plant_set_payload") for c in s.calls)
    one = ml.MPCRunner(_PayloadRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_payload=m[1])      # one record, given as a vector
    assert one.plant_payload.shape == (1, 10)
