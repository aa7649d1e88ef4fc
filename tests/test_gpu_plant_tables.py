"""The host plumbing the six plant tables share (csrc/ilqr_capi.hip table_install / table_clear / table_read, grow_step_scratch,
step_in_module; csrc/plant_plan.h), on the GPU.

What the tables DO is the business of the suites of each table.  Here the yardstick is a handle that never exercised the path:
  * lifecycle: every table installed with one record, with B records and with one again, read back each time, cleared twice -- after which the
    handle's plant calls equal, bit for bit, those of a handle that never had a table;
  * scratch growth: the single-step calls with counts 1, 5, 2, each finding scratch another call sized, against the same call on a fresh
    handle, bit for bit.

Shape: B = 3 rollouts under the stance patterns both / left / right, N = 4, one iteration per solve, two substeps, contact mode 2."""
import numpy as np
import pytest

import actuator_cases as ac
import dynamics_envelope_cases as dc
import joints_cases as jc
import observation_cases as oc
import payload_cases as plc
import plant_params_cases as pc
import wrench_cases as wc
from conftest import load_package

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
B, N, DT, SUBSTEPS, RING = 3, 4, 0.02, 2, 3
MODE, MU, SOFT = 2, 0.3, 1e-5
PATTERNS = dc.STANCE_ROWS[[0, 1, 2]]


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _handle(count, n, dt):
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=n, gravity=dc.GRAVITY)
    A = sv.BatchedILQR(count, N=n, dt=dt)
    A.set_contact_mode(MODE, SOFT); A.set_friction(MU); A.set_joint_limits(False); A.set_joint_limit_stiffness(0.0)
    return A, prob


def _ready(fb):
    """a handle behind one solve and a plant_reset: the same on every call"""
    A, prob = _handle(B, N, DT)
    prob["stance"] = np.ascontiguousarray(np.repeat(PATTERNS[:, None, :], N + 1, axis=1))
    A.set_max_iterations(1)
    A.plant_configure(SUBSTEPS, fb, "schedule")
    A.plant_set_history(RING)
    A.set_problem(prob)
    x16, u16 = dc.mid()
    x0, ui = np.ascontiguousarray(x16[2:2 + B]), np.ascontiguousarray(np.repeat(u16[2:2 + B][:, None, :], N, axis=1))
    A.initialize(x0, ui); A.solve(x0)
    A.plant_reset(x0)
    return A


def _snapshot(A):
    hx, hu = A.plant_history()
    return A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive(), hx, hu


def _wrench_table(n, seed):
    w = np.zeros((n, 11))
    w[:, :9] = wc.random_wrenches(n, seed)
    w[:, 9], w[:, 10] = 0.0, np.inf
    return w


def _tables(A):
    """name -> (set, clear, num or None, get, records(n, seed), the documented read-back without a table)"""
    own = np.tile(np.array([dc.GRAVITY[0], dc.GRAVITY[1], dc.GRAVITY[2], MU, SOFT, 0.0, 1.0]), (B, 1))      # the handle's own values with gain 1
    seeds = {}      # what the last install of a seeded table passed: the read-back returns it

    def seeded(setter, name):
        def install(rec):
            seeds[name] = (len(rec) + 7, 1000 + len(rec))
            setter(rec, *seeds[name])
        return install

    def seeded_get(getter, name):
        def get():
            rec, seed, stream0 = getter()
            assert (seed, stream0) == seeds.get(name, (0, 0)), name
            return rec
        return get

    def clear_seeded(clear, name):
        def run():
            clear()
            seeds.pop(name, None)
        return run

    return {
        "params": (A.plant_set_params, A.plant_clear_params, A.plant_num_param_sets, A.plant_params, lambda n, s: np.ascontiguousarray(pc.SETS[(np.arange(n) + s) % 3]), own),
        "wrench": (A.plant_set_wrench, A.plant_clear_wrench, A.plant_num_wrench_sets, A.plant_wrench, _wrench_table, np.zeros((B, 11))),
        "payload": (A.plant_set_payload, A.plant_clear_payload, A.plant_num_payload_sets, A.plant_get_payload, plc.random_payloads, np.zeros((B, 10))),
        "observation": (seeded(A.plant_set_observation, "o"), clear_seeded(A.plant_clear_observation, "o"), A.plant_num_observation_sets, seeded_get(A.plant_get_observation, "o"),
                        oc.plant_records, np.zeros((B, 100))),
        "actuator": (seeded(A.plant_set_actuator, "a"), clear_seeded(A.plant_clear_actuator, "a"), A.plant_num_actuator_sets, seeded_get(A.plant_get_actuator, "a"),
                     ac.golden_records, np.zeros((B, 39))),
        "joints": (A.plant_set_joints, A.plant_clear_joints, None, A.plant_get_joints, jc.random_records, np.tile(jc.NOMINAL, (B, 1))),
    }


@pytest.mark.parametrize("fb", [0, 1])
def test_tables_installed_resized_and_cleared_leave_a_handle_that_never_had_one(fb):
    A, ref = _ready(fb), _ready(fb)
    for name, (install, clear, num, get, records, none) in _tables(A).items():
        for k, n in enumerate((1, B, 1)):
            rec = records(n, 40 + k)
            assert rec.shape[0] == n and np.any(rec != 0.0), name
            install(rec)
            assert num is None or num() == n, name
            assert np.array_equal(get(), np.broadcast_to(rec, (B, rec.shape[1])) if n == 1 else rec), (name, n)
        for _ in range(2):
            clear()
            assert num is None or num() == 0, name
            assert np.array_equal(get(), none), name
    for H in (A, ref):
        H.plant_advance()
        H.plant_follow(0, 2)
        assert H.plant_intervals() == 3
    a, r = _snapshot(A), _snapshot(ref)
    assert all(np.all(np.isfinite(v)) for v in r[:2]) and np.any(r[0] != 0.0)
    for got, want, what in zip(a, r, ("state", "control", "stance", "alive", "ring x", "ring u")):
        assert np.array_equal(got, want), what
    A.close(); ref.close()


def test_single_steps_on_scratch_another_call_sized_equal_a_fresh_handle():
    x16, u16 = dc.mid()
    H, prob = _handle(1, 1, DT)
    H.set_problem(prob)
    calls = {
        "wrench": lambda P, x, u, w, m, j: P.step_wrench(x, u, 1, 1, w),
        "payload": lambda P, x, u, w, m, j: P.step_payload(x, u, 1, 1, m, w),
        "joints": lambda P, x, u, w, m, j: P.step_joints(x, u, 1, 1, j, w, m),
        "stance": lambda P, x, u, w, m, j: P.step_stance(x, u, 1, 1),
    }
    names = list(calls)
    for k, count in enumerate((1, 5, 2)):
        x, u = np.ascontiguousarray(x16[k:k + count]), np.ascontiguousarray(u16[k:k + count])
        w, m, j = wc.random_wrenches(count, 50 + k), plc.random_payloads(count, 60 + k), jc.random_records(count, 70 + k)
        for name in names[k:] + names[:k]:      # each count is first met by another call: it finds scratch the call before it sized
            got = calls[name](H, x, u, w, m, j)
            F, fprob = _handle(1, 1, DT)
            F.set_problem(fprob)
            want = calls[name](F, x, u, w, m, j)
            F.close()
            assert got.shape == (count, 51) and np.all(np.isfinite(want)) and np.any(want != x), (name, count)
            assert np.array_equal(got, want), (name, count)
    H.close()
