"""The per-rollout joint records on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_joints, ilqr_hip_step_joints; csrc/plant_kernels.hip
k_plant_follow_j, k_step_j).

No entry point that existed before the feature reads a joint record, so the ground truth is in two layers:
  * ilqr_hip_step_joints against the golden of the NumPy Kane / KKT restatement (tests/golden/gen_joints_golden.py) in all six step kinds,
    and against the closed form on the CPU oracle's inverse dynamics (tests/joints_cases.py) on those outputs;
  * the plant kernel against the TEACHER-FORCED composition compute_control -> step_joints per substep on a handle at DT / SUBSTEPS, every
    interval of a follow(0, 4) held to the composition from the ring row it started from.

Shape: B = 5 rollouts (one partial workgroup at feedback mode 0, one full and one partial at mode 1), N = 6, SUBSTEPS = 3, four intervals.
Rollout b starts from envelope state (b + 2) % 16 under the stance pattern PATTERNS[b] at every knot; rollout DEAD has a dead left knee.

Bounds: 1e-10 absolute for a step of contact mode 0 without rows, cc.STEP_TOL = 1e-9 relative to max(1, max |want|) otherwise (tests/
test_gpu_payload.py); inverse dynamics jc.ID_TOL = 1e-6 N; plant: U_TOL on the reported control and cc.STEP_TOL x SUBSTEPS relative on the
state per interval (tests/test_gpu_plant_params.py)."""
import os
import shutil

import numpy as np
import pytest

import actuator_cases as ac
import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import joints_cases as jc
import observation_cases as oc
import payload_cases as plc
import wrench_cases as wc
from conftest import load_package
from test_gpu_plant import U_TOL
from test_gpu_wrench import KINDS, _kind_of, _rel, _same, _snapshot, _step_handle

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU, NQ = 51, 19, 26
B, N, DT, SUBSTEPS, INTERVALS = 5, 6, 0.02, 3, 4
HANDLE_MU = 0.3
PATTERNS = dc.STANCE_ROWS[[0, 1, 2, 0, 0]]
DEAD = 1
SEED = 0x101_75
#            plant mode, limits, states
CASES = {"free": (0, False, "mid"), "mode2": (2, False, "mid"), "mode4_limits": (4, True, "limits")}


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _schedule():
    return np.ascontiguousarray(np.repeat(PATTERNS[:, None, :], N + 1, axis=1))


def _solver(mode=0, limits=False, fb=0, ring=0):
    """the solving handle: one iteration per solve, friction HANDLE_MU, stiffness 0, softness 1e-5"""
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=dc.GRAVITY)
    prob["stance"] = _schedule()
    A = sv.BatchedILQR(B, N=N, dt=DT)
    A.set_contact_mode(mode); A.set_friction(HANDLE_MU); A.set_joint_limits(limits); A.set_max_iterations(1)
    A.plant_configure(SUBSTEPS, fb, "schedule")
    A.plant_set_history(ring)
    A.set_problem(prob)
    return A


def _plant_step_handle(mode, limits):
    """the yardstick's handle: the plant's step size and the solving handle's parameters"""
    return _step_handle(B, DT / SUBSTEPS, dc.GRAVITY, mode, limits, HANDLE_MU, 1e-5, 0.0)


def _states(group):
    x16, u16 = dc.mid() if group == "mid" else cc.limit_states()
    idx = (np.arange(B) + 2) % dc.NS
    return np.ascontiguousarray(x16[idx]), np.ascontiguousarray(np.repeat(u16[idx][:, None, :], N, axis=1))


def _records(seed=3):
    return jc.random_records(B, seed, dead=(DEAD,))


def _ready(mode, limits, group, fb, ring=0):
    A = _solver(mode, limits, fb=fb, ring=ring)
    x0, ui = _states(group)
    A.initialize(x0, ui); A.solve(x0)
    assert np.all(np.isfinite(A.ubar())) and np.all(np.isfinite(A.gains_K()))
    return A, x0


def _step(P, x, u, joints, w9=None, m10=None):
    """step_joints of the batch, each rollout under its stance pattern"""
    xn = np.empty_like(x)
    for l, r in {(int(a), int(c)) for a, c in PATTERNS}:
        idx = np.flatnonzero((PATTERNS[:, 0] == l) & (PATTERNS[:, 1] == r))
        xn[idx] = P.step_joints(x[idx], u[idx], l, r, joints[idx], None if w9 is None else w9[idx], None if m10 is None else m10[idx])
    return xn


def _state_err(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))).max())


# ---- 1: the step kernel against the golden and against the closed form, every kind
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_step_joints_matches_the_golden_and_the_closed_form(kind):
    g = jc.golden()
    h, grav = float(g["h"]), g["gravity"]
    cases = [i for i in range(len(g["x"])) if _kind_of(int(g["contact"][i]), int(g["limits"][i])) == kind]
    assert cases, kind
    groups = {}
    for i in cases:
        groups.setdefault((int(g["contact"][i]), int(g["limits"][i]), float(g["mu"][i]), tuple(int(v) for v in g["stance"][i])), []).append(i)
    for (mode, limits, mu, (sl, sr)), idx in sorted(groups.items()):
        pad = idx + idx[:1]                                                                   # the kind's cases and one padding item: a partial workgroup
        P = _step_handle(len(pad), h, grav, mode, limits, mu, float(g["soft"]))
        J = g["joints"][pad].copy(); J[-1] = jc.NOMINAL
        W, M = g["wrench"][pad].copy(), g["payload"][pad].copy(); W[-1] = 0.0; M[-1] = 0.0
        got = P.step_joints(g["x"][pad], g["u"][pad], sl, sr, J, W, M)
        plain = P.step_stance(g["x"][pad[-1:]], g["u"][pad[-1:]], sl, sr)
        free = mode == 0 and not limits
        for k, i in enumerate(idx):
            want = g["x_next"][i]
            err, bound = (float(np.abs(got[k] - want).max()), 1e-10) if free else (_rel(got[k], want), cc.STEP_TOL)
            res = jc.hinge_residual(g["x"][i], got[k], g["u"][i], h, grav, g["joints"][i])
            hinges = jc.checked_hinges(g["act"][i], g["lock"][i])
            eh = float(np.abs(res[6:][hinges]).max())
            eb = float(np.abs(res[:6] - jc.expected_base_rows(g["x"][i], got[k], h, grav, g["wrench"][i], g["payload"][i])).max()) if mode == 0 else 0.0
            print("kind %d case %2d (%s, mode %d, limits %d, stance %d%d, changed %d): error %.3e (bound %.0e); closed form hinge rows %.3e base rows %.3e (bound %.0e)"
                  % (kind, i, g["kind"][i], mode, limits, sl, sr, int(g["changed"][i]), err, bound, eh, eb, jc.ID_TOL))
            assert np.all(np.isfinite(got[k])) and err < bound, (i, err)
            assert eh < jc.ID_TOL and eb < jc.ID_TOL, (i, eh, eb)
        # the padding item: the nominal record without wrench and payload is the handle's own step
        errp = float(np.abs(got[-1] - plain[0]).max()) if free else _rel(got[-1], plain[0])
        print("kind %d: nominal record against step_stance %.3e" % (kind, errp))
        assert errp < (1e-10 if free else cc.STEP_TOL)
        # wrench / payload NULL are a wrench / payload of zero
        none = P.step_joints(g["x"][pad[-1:]], g["u"][pad[-1:]], sl, sr, J[-1:])
        assert np.array_equal(none[0], got[-1])
        P.close()


# ---- 2: the plant against the teacher-forced composition
def _interval(A, step, x, fb, knot, chain=None, z=None, delta=None):
    """one MPC interval from the state x: (x_next, reported command)"""
    xc, u = x.copy(), None
    for k in range(SUBSTEPS):
        if k == 0 or fb:
            u = A.compute_control(xc if delta is None else oc.boxplus(xc, delta), knot=knot)
        t = ac.guard(u) if chain is None else chain.substep(u, z)
        xc = step(xc, t)
    return xc, ac.guard(u)


def _held_to_the_composition(A, x0, fb, mode, tag, step, chain_of=lambda: None, z=None, delta=None):
    """follow(0, INTERVALS) in one launch; every interval against the host composition from the ring row it started from"""
    A.plant_reset(x0)
    A.plant_follow(0, INTERVALS)
    hx, hu = A.plant_history()
    assert hx.shape == (INTERVALS, B, NX) and np.array_equal(hx[0], x0) and np.all(A.plant_alive() == 1) and A.plant_intervals() == INTERVALS
    ends = [hx[j + 1] for j in range(INTERVALS - 1)] + [A.plant_state()]
    chain, worst = chain_of(), 0.0
    for j in range(INTERVALS):
        want_x, want_u = _interval(A, lambda xc, t: step(j, xc, t), hx[j], fb, j, chain, None if z is None else z[j], None if delta is None else delta[j])
        ex, eu = _state_err(ends[j], want_x), float(np.abs(hu[j] - want_u).max())
        print("%s interval %d: state error %.3e (bound %.1e)  |du| %.3e" % (tag, j, ex, cc.STEP_TOL * SUBSTEPS, eu))
        assert np.all(np.isfinite(want_x)), (tag, j)
        assert np.allclose(hu[j], want_u, **U_TOL), (tag, j, eu)                              # the REPORTED control: the command
        assert ex < cc.STEP_TOL * SUBSTEPS, (tag, j, ex)
        worst = max(worst, ex)
    assert np.array_equal(A.plant_control(), hu[-1])
    if mode:
        assert np.array_equal(A.plant_stance(), PATTERNS)
    return worst


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plant_under_a_joint_table_matches_the_host_composition(case, fb):
    mode, limits, group = CASES[case]
    A, x0 = _ready(mode, limits, group, fb, ring=INTERVALS)
    P = _plant_step_handle(mode, limits)
    J = _records()
    nominal = np.tile(jc.NOMINAL, (B, 1))
    assert np.array_equal(A.plant_get_joints(), nominal)
    # on the yardstick alone: the records matter in every rollout
    loaded, bare = (_interval(A, lambda xc, t: _step(P, xc, t, jj), x0, fb, 0)[0] for jj in (J, nominal))
    assert np.all(np.abs(loaded - bare).max(axis=1) > 1e-6)
    A.plant_set_joints(J)
    assert np.array_equal(A.plant_get_joints(), J)
    tag = "%s fb%d" % (case, fb)
    worst = _held_to_the_composition(A, x0, fb, mode, tag, lambda j, xc, t: _step(P, xc, t, J))
    print("%s: worst state error under the joint table %.3e" % (tag, worst))
    A.close(); P.close()


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plant_under_all_six_tables_matches_the_host_composition(case, fb):
    """parameter (the handle's values and a torque gain per rollout), wrench (window from interval 1), payload, observation, actuator, joints"""
    mode, limits, group = CASES[case]
    A, x0 = _ready(mode, limits, group, fb, ring=INTERVALS)
    P = _plant_step_handle(mode, limits)
    J = _records(4)
    gain = np.linspace(0.8, 1.0, B)
    params = np.tile([dc.GRAVITY[0], dc.GRAVITY[1], dc.GRAVITY[2], HANDLE_MU, 1e-5, 0.0, 1.0], (B, 1)); params[:, 6] = gain
    wrench = np.hstack([wc.random_wrenches(B, 3), np.ones((B, 1)), np.full((B, 1), np.inf)])
    payload = plc.random_payloads(B, 5)
    rec = ac.golden_records(B)
    A.plant_set_params(params); A.plant_set_wrench(wrench); A.plant_set_payload(payload)
    A.plant_set_observation(oc.plant_records(B), seed=SEED + 1)
    A.plant_set_actuator(rec, seed=SEED)
    A.plant_set_joints(J)
    A.plant_reset(x0)
    delta, z, beta = A.plant_observation_errors(0, INTERVALS), A.plant_actuator_draws(0, INTERVALS), A.plant_actuator_blend()

    def step(j, xc, t):
        w9 = wrench[:, :9] if j >= 1 else np.zeros((B, 9))
        return _step(P, xc, gain[:, None] * t, J, w9, payload)

    tag = "%s fb%d all six tables" % (case, fb)
    worst = _held_to_the_composition(A, x0, fb, mode, tag, step, lambda: ac.Chain(rec, beta), z, delta)
    # the joint table acts beside the others: the composition under the nominal record goes elsewhere
    other = _interval(A, lambda xc, t: _step(P, xc, gain[:, None] * t, np.tile(jc.NOMINAL, (B, 1)), np.zeros((B, 9)), payload), x0, fb, 0, ac.Chain(rec, beta), z[0], delta[0])[0]
    A.plant_reset(x0); A.plant_advance()
    assert np.all(np.abs(other - A.plant_state()).max(axis=1) > 1e-6)
    print("%s: worst state error %.3e" % (tag, worst))
    A.close(); P.close()


# ---- 3: bit for bit
def _run(A, x0, calls):
    A.plant_reset(x0)
    for c in calls:
        A.plant_advance() if c is None else A.plant_follow(*c)
    return _snapshot(A)


@pytest.mark.parametrize("fb", [0, 1])
def test_one_record_for_all_is_b_identical_records(fb):
    A, x0 = _ready(4, True, "limits", fb, ring=3)
    rec = _records()[2:3]
    A.plant_set_joints(rec)
    assert np.array_equal(A.plant_get_joints(), np.repeat(rec, B, axis=0))
    one = _run(A, x0, [(0, 3)])
    A.plant_set_joints(np.repeat(rec, B, axis=0))
    assert _same(one, _run(A, x0, [(0, 3)])) and np.all(one[3] == 1)
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_a_group_of_three_is_the_same_in_one_launch_and_in_three(fb):
    A, x0 = _ready(4, True, "limits", fb, ring=3)
    A.plant_set_joints(_records())
    fused = _run(A, x0, [(0, 3)])
    assert _same(fused, _run(A, x0, [(0, 1), (1, 1), (2, 1)])) and np.all(fused[3] == 1) and A.plant_intervals() == 3
    assert _same(_run(A, x0, [None, None, None]), _run(A, x0, [(0, 1), (0, 1), (0, 1)]))      # an advance is the kernel over one interval
    A.close()


@pytest.mark.parametrize("mode,limits,group", [(0, False, "mid"), (4, True, "limits")])
@pytest.mark.parametrize("fb", [0, 1])
def test_clearing_and_an_all_nominal_table_launch_what_no_table_launches(fb, mode, limits, group):
    A, x0 = _ready(mode, limits, group, fb, ring=3)
    calls = [None, (1, 2)]
    none = _run(A, x0, calls)
    A.plant_set_joints(_records())
    table = _run(A, x0, calls)
    assert not _same(none, table) and np.all(np.abs(table[0] - none[0]).max(axis=1) > 1e-6)
    A.plant_clear_joints()
    assert _same(none, _run(A, x0, calls)) and np.array_equal(A.plant_get_joints(), np.tile(jc.NOMINAL, (B, 1)))
    A.plant_set_joints(np.tile(jc.NOMINAL, (B, 1)))                                           # every record nominal: no table, bit for bit
    assert _same(none, _run(A, x0, calls))
    A.plant_set_joints(jc.NOMINAL)                                                            # ... one nominal record for all as well
    assert _same(none, _run(A, x0, calls))
    A.plant_set_joints(None)                                                                  # (None clears)
    assert _same(none, _run(A, x0, calls))
    # under another family: the payload family before, the payload family after
    A.plant_set_payload(plc.random_payloads(B, 5))
    loaded = _run(A, x0, calls)
    A.plant_set_joints(_records()); assert not _same(loaded, _run(A, x0, calls))
    A.plant_clear_joints(); assert _same(loaded, _run(A, x0, calls))
    A.close()


@pytest.mark.parametrize("mode,limits,group", [(0, False, "mid"), (2, False, "mid"), (4, True, "limits")])
@pytest.mark.parametrize("fb", [0, 1])
def test_a_nominal_record_inside_a_mixed_table_is_its_rollouts_run_without_a_table(fb, mode, limits, group):
    """the joints family runs the per-hinge recursion with adds of 0.0 and a disturbance row of zeros, and 1 * x, x + 0.0 and x - 1 * v round
    as x, x and x - v: bit for bit (DESIGN 4.1 "A joint that is not the model's")"""
    A, x0 = _ready(mode, limits, group, fb, ring=1)
    nom = [0, 3]
    J = _records(); J[nom] = jc.NOMINAL
    A.plant_reset(x0); A.plant_advance(); none = _snapshot(A)
    A.plant_set_joints(J)
    A.plant_reset(x0); A.plant_advance(); mixed = _snapshot(A)
    err = _state_err(mixed[0][nom], none[0][nom])
    du = float(np.abs(mixed[1][nom] - none[1][nom]).max())
    rest = [b for b in range(B) if b not in nom]
    print("mode %d limits %d fb%d: nominal records in a mixed table against no table: state %.3e, control %.3e" % (mode, limits, fb, err, du))
    assert all(np.array_equal(m[nom], n[nom]) for m, n in zip(mixed[:4], none[:4]))
    assert np.all(np.abs(mixed[0][rest] - none[0][rest]).max(axis=1) > 1e-6)
    A.close()


# ---- 4: a dead knee
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_dead_knee_gets_no_torque(kind):
    """s = 0 on the knee: the step is the step with u_knee = 0 under s = 1, bit for bit"""
    mode, limits = KINDS[kind]
    x16, u16 = cc.limit_states() if limits else dc.mid()
    x, u = np.ascontiguousarray(x16[:3]), np.ascontiguousarray(u16[:3]).copy()
    u[:, jc.KNEE] = [35.0, -60.0, 400.0]                                                      # inside the range twice, beyond it once
    J = jc.random_records(3, 9)
    J[:, NU + jc.KNEE] = 0.0
    J1, u0 = J.copy(), u.copy()
    J1[:, NU + jc.KNEE] = 1.0; u0[:, jc.KNEE] = 0.0
    P = _step_handle(3, DT, dc.GRAVITY, mode, limits, HANDLE_MU)
    dead, zero, live = P.step_joints(x, u, 1, 0, J), P.step_joints(x, u0, 1, 0, J1), P.step_joints(x, u, 1, 0, J1)
    P.close()
    assert np.all(np.isfinite(dead)) and np.array_equal(dead, zero)
    moved = np.abs(dead - live).max(axis=1) > 1e-6                                            # (a knee that the limit rows stop has its torque prescribed)
    assert moved.any() if limits else moved.all()


# ---- 5: a record that makes one rollout non-finite freezes that rollout alone
@pytest.mark.parametrize("fb", [0, 1])
def test_an_overflowing_record_freezes_its_rollout_alone(fb):
    bad = 4                                                                                    # in the second workgroup at feedback mode 1
    out = {}
    for poisoned in (False, True):
        A, x0 = _ready(0, False, "mid", fb, ring=2)
        J = _records()
        if poisoned:
            J[bad, 0:2 * NU] = 1e308                                                           # gain and range scale: the clamp lets an infinite torque through
        A.plant_set_joints(J)
        A.plant_reset(x0)
        A.plant_advance()
        out[poisoned] = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        A.close()
    x, u, st, alive = out[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(u[bad] == 0.0) and np.array_equal(x[bad], x0[bad])         # frozen in the state before the advance
    assert np.all(alive[keep] == 1) and np.all(out[False][3] == 1)
    assert np.array_equal(x[keep], out[False][0][keep]) and np.array_equal(u[keep], out[False][1][keep])      # bit for bit


# ---- 6: the runner
def test_runner_with_plant_joints_is_the_call_sequence_made_by_hand():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, Nn, steps = 4, 25, 3
    base = sc.make_problem(sv.reference_kinematics, N=Nn, gravity=dc.GRAVITY)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(Bn, Nn, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    J = sc.stack_plant_joints([dict(), dict(gain=0.7), dict(range_scale=np.r_[np.ones(3), 0.0, np.ones(15)], damping=2.0), dict(armature=0.25, damping=0.5)], Bn)
    s = sv.BatchedILQR(Bn, N=Nn, dt=DT); s.set_contact_mode(2); s.set_max_iterations(2)
    xs, us = ml.MPCRunner(s, rd, base, resident=True, substeps=2, plant_joints=J).run(x0, steps, u_init=ui)
    assert np.all(s.plant_alive() == 1) and np.array_equal(s.plant_get_joints(), J) and s.plant_intervals() == steps
    s.close()
    h = sv.BatchedILQR(Bn, N=Nn, dt=DT); h.set_contact_mode(2); h.set_max_iterations(2)
    run = ml.MPCRunner(h, rd, base, resident=True, substeps=2)
    h.plant_set_joints(J)                                                                      # (survives the runner's configure and reset)
    xh, uh = run.run(x0, steps, u_init=ui)
    assert np.array_equal(h.plant_get_joints(), J)
    h.close()
    assert np.array_equal(xs, xh) and np.array_equal(us, uh)
    p = sv.BatchedILQR(Bn, N=Nn, dt=DT); p.set_contact_mode(2); p.set_max_iterations(2)
    xp, _ = ml.MPCRunner(p, rd, base, resident=True, substeps=2).run(x0, steps, u_init=ui)
    p.close()
    d = np.abs(np.asarray(xs)[-1] - np.asarray(xp)[-1]).max(axis=1)
    print("last state against the run without a table, per rollout: %s" % d)
    assert d[0] == 0.0 and np.all(d[1:] > 1e-6)                                               # rollout 0 has the model's joints: bit for bit


# ---- 7: refusals
def test_refusals_on_a_live_handle(tmp_path):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    sv = _sv()
    A = _solver(0, False)
    for bad in (np.ones((2, 76)), np.ones((B, 75))):
        with pytest.raises(ValueError):
            A.plant_set_joints(bad)
    J = _records()
    for col, v in ((0, np.nan), (20, np.inf), (40, -np.inf), (5, -1.0), (19 + jc.KNEE, -1e-300), (50, -0.5), (75, -0.1)):
        q = J.copy(); q[B - 1, col] = v
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_joints(q)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.step_joints(np.zeros((B, NX)), np.zeros((B, NU)), 1, 1, q)
    assert np.array_equal(A.plant_get_joints(), np.tile(jc.NOMINAL, (B, 1)))
    A.plant_set_joints(J[:1])                                                                  # one record for all rollouts
    assert np.array_equal(A.plant_get_joints(), np.repeat(J[:1], B, axis=0))
    A.plant_set_joints(J); A.plant_configure(2, 1, "schedule")
    assert np.array_equal(A.plant_get_joints(), J)                                             # survives configure
    A.plant_clear_joints(); A.plant_clear_joints()                                             # clearing twice is fine
    two = np.ascontiguousarray(J[:2])
    assert A.L.ilqr_hip_plant_set_joints(A.h, two.ctypes.data_as(sv._dp), 2) == 1              # n neither 1 nor B, past the wrapper
    assert A.L.ilqr_hip_plant_set_joints(A.h, None, 1) == 1 and A.L.ilqr_hip_plant_set_joints(A.h, two.ctypes.data_as(sv._dp), 0) == 1
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(A, None, None, plant_joints=J)
    A.close()
    # a library whose directory holds no joints module: an error that names the path it looked for, never a fall-back
    lonely = tmp_path / "libilqr_hip.so"
    shutil.copyfile(sv.LIB_PATH, lonely)
    P = sv.BatchedILQR(B, N=N, dt=DT, lib_path=str(lonely))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED") as e:
        P.plant_set_joints(J)
    assert os.path.join(str(tmp_path), "libilqr_hip_joints.so") in str(e.value)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        P.step_joints(np.zeros((1, NX)), np.zeros((1, NU)), 1, 1, J[:1])
    assert np.array_equal(P.plant_get_joints(), np.tile(jc.NOMINAL, (B, 1)))
    P.close()
