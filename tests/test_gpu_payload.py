"""The rigid payload on the pelvis on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_payload, ilqr_hip_step_payload;
csrc/plant_kernels.hip k_plant_follow_m, k_step_m).

No entry point that existed before the feature carries a payload, so the ground truth is in two layers:
  * ilqr_hip_step_payload against the golden of the NumPy Kane / KKT restatement with the payload merged into the pelvis body
    (tests/golden/gen_payload_golden.py) in all six step kinds, and against the closed form of the payload's own Newton-Euler equations on
    the CPU oracle's inverse dynamics on the envelope states (tests/payload_cases.py);
  * the plant kernels against the TEACHER-FORCED composition compute_control -> step_payload per substep on handles at DT / SUBSTEPS
    (WrenchYardstick of tests/test_gpu_wrench.py with the payload added), on the cases and state groups of tests/test_gpu_plant_params.py:
    B = 37 (two workgroups at feedback mode 0, ten at mode 1, the last one not full), N = 6, SUBSTEPS = 2.

Bounds: 1e-10 absolute for a step of contact mode 0 without rows, cc.STEP_TOL = 1e-9 relative to max(1, max |want|) otherwise; plant:
U_TOL, X_TOL_PER_STEP x SUBSTEPS, cc.STEP_TOL x SUBSTEPS as tests/test_gpu_plant_params.py; inverse dynamics: pc.ID_TOL = 1e-6 N."""
import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import payload_cases as plc
import plant_params_cases as pc
import wrench_cases as wc
from conftest import load_package
from test_gpu_plant import U_TOL
from test_gpu_plant_params import CASES, _solver, _state_error, _states
from test_gpu_wrench import KINDS, OWN, WrenchYardstick, _kind_of, _rel, _same, _snapshot, _step_handle, _wrench_table

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU, NQ = 51, 19, 26
B, N, DT, SUBSTEPS = pc.B, pc.N, pc.DT, pc.SUBSTEPS
ID_TOL = plc.ID_TOL


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


# ---- 1: the step kernel against the golden, every kind; a zero payload against step_wrench
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_step_payload_matches_the_golden(kind):
    g = plc.golden()
    cases = [i for i in range(len(g["x"])) if _kind_of(int(g["contact"][i]), int(g["limits"][i])) == kind]
    assert cases, kind
    for i in cases:
        mode, limits = int(g["contact"][i]), int(g["limits"][i])
        P = _step_handle(1, float(g["h"]), g["gravity"], mode, limits, float(g["mu"][i]), float(g["soft"]))
        sl, sr = (int(v) for v in g["stance"][i])
        x, u, w, m, want = g["x"][i][None], g["u"][i][None], g["wrench"][i][None], g["payload"][i][None], g["x_next"][i][None]
        got = P.step_payload(x, u, sl, sr, m, w)
        free = mode == 0 and not limits
        err, bound = (float(np.abs(got - want).max()), 1e-10) if free else (_rel(got, want), cc.STEP_TOL)
        zero = P.step_payload(x, u, sl, sr, np.zeros((1, 10)), w)
        plain = P.step_wrench(x, u, sl, sr, w)
        errz = float(np.abs(zero - plain).max()) if free else _rel(zero, plain)
        nowrench = P.step_payload(x, u, sl, sr, m)                                              # wrench NULL is a wrench of zero
        errn = float(np.abs(nowrench - P.step_payload(x, u, sl, sr, m, np.zeros((1, 9)))).max())
        print("kind %d case %2d (mode %d, limits %d, stance %d%d, %.1f kg, changed %d): error %.3e (bound %.0e); zero payload against step_wrench %.3e; moved by %.3e"
              % (kind, i, mode, limits, sl, sr, m[0, 0], int(g["changed"][i]), err, bound, errz, np.abs(got - plain).max()))
        assert np.all(np.isfinite(got)) and err < bound, (i, err)
        assert errz < bound, (i, errz)                                                       # (not bit for bit: another instantiation)
        if np.abs(m).max() > 0:
            assert np.abs(got - plain).max() > 1e-6, i                                          # the payload acts
        if np.abs(w).max() == 0:
            assert errn == 0.0, (i, errn)
        P.close()


# ---- 2: the oracle's inverse dynamics of the GPU step on the envelope states: the payload's closed form
@pytest.mark.parametrize("group,limits", [("mid", False), ("limits", True)])
def test_inverse_dynamics_of_the_step_is_the_payloads_closed_form(group, limits):
    x, u = dc.mid() if group == "mid" else cc.limit_states()
    m = plc.random_payloads(dc.NS, 11 + int(limits))
    P = _step_handle(dc.NS, dc.H, dc.GRAVITY, 0, limits)
    xn = P.step_payload(x, u, 1, 1, m)
    plain = P.step(x, u)
    P.close()
    assert np.all(np.isfinite(xn))
    stopped = cc.stopped_hinges(x, xn[:, None, :], 0.0)[:, 0, :] & (cc.violation(x) != 0.0) if limits else np.zeros((dc.NS, NU), dtype=bool)
    worst_b = worst_h = 0.0
    for i in range(dc.NS):
        res = wc.inverse_dynamics_residual(x[i], xn[i], u[i], dc.H, np.array(dc.GRAVITY))
        worst_b = max(worst_b, float(np.abs(res[:6] - plc.expected_base_rows(x[i], xn[i], dc.H, np.array(dc.GRAVITY), m[i])).max()))
        worst_h = max(worst_h, float(np.abs(res[6:][~stopped[i]]).max()))
        assert np.abs(xn[i] - plain[i]).max() > 1e-6, i
    print("%s: base rows against the closed form %.3e, free hinge rows %.3e (bound %.0e); %d hinges stopped" % (group, worst_b, worst_h, ID_TOL, int(stopped.sum())))
    assert worst_b < ID_TOL and worst_h < ID_TOL
    if limits:
        assert stopped.sum() >= 16                                                              # the second pass ran, under the payload


# ---- the yardstick of the plant: compute_control, then step_payload per substep
class PayloadYardstick(WrenchYardstick):
    def step_m(self, table, x, u, flags, w9, m10):
        xn, st = np.empty_like(x), np.array(flags, dtype=np.int32)
        ua = table[:, 6:7] * u
        for s in np.unique(table[:, :6], axis=0):
            rows = np.flatnonzero((table[:, :6] == s).all(axis=1))
            P = self.handle(s)
            fl = np.array(flags[rows], dtype=np.int32)
            if self.mode and self.source == "geometry":
                _, fl = P.step_geometry(x[rows], ua[rows])                                   # the flags each rollout's own feet decide
                st[rows] = fl
            for l, r in {(int(a), int(c)) for a, c in fl}:
                idx = rows[(fl[:, 0] == l) & (fl[:, 1] == r)]
                xn[idx] = P.step_payload(x[idx], ua[idx], l, r, m10[idx], w9[idx])
        return xn, st

    def advance_m(self, A, table, wrench, payload, interval, x, flags, fb, knot=0):
        """one MPC interval under the payloads [B, 10] and the records of `wrench` [B, 11] whose window holds `interval`"""
        on = (wrench[:, 9] <= interval) & (interval < wrench[:, 10])
        w9 = np.where(on[:, None], wrench[:, :9], 0.0)
        xc, u, st = x.copy(), None, np.array(flags, dtype=np.int32)
        for k in range(SUBSTEPS):
            if k == 0 or fb:
                u = A.compute_control(xc, knot=knot)
                u[~np.isfinite(u).all(axis=1)] = 0.0
            xc, st = self.step_m(table, xc, u, flags, w9, payload)
        return xc, u, st


NO_WRENCH, NO_PAYLOAD = np.zeros((B, 11)), np.zeros((B, 10))


def _payload_table(seed=5):
    return plc.random_payloads(B, seed)


def _every_workgroup(moved, fb, tag):
    """at least four rollouts, and one in each workgroup of the plant kernel (32 rollouts at feedback mode 0, 4 at mode 1)"""
    rpw = 4 if fb else 32
    per = [int(moved[k:k + rpw].sum()) for k in range(0, B, rpw)]
    print("%s: the payload moves %d rollouts, per workgroup %s" % (tag, int(moved.sum()), per))
    assert moved.sum() >= 4 and min(per) >= 1, (tag, per)


def _teacher_forced_m(A, Y, table, wrench, payload, x0, flags, fb, advances, group, tag):
    A.plant_reset(x0)
    x, worst = x0.copy(), 0.0
    for k in range(advances):
        want_x, want_u, want_st = Y.advance_m(A, table, wrench, payload, k, x, flags, fb)
        A.plant_advance()
        got_x, got_u, got_st, alive = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        err, bound = _state_error(got_x, want_x, group)
        print("%s advance %d: state error %.3e (bound %.1e)  |du| %.3e  alive %d/%d" % (tag, k, err, bound, np.abs(got_u - want_u).max(), alive.sum(), B))
        assert np.all(alive == 1) and np.all(np.isfinite(want_x)), (tag, k)
        assert np.allclose(got_u, want_u, **U_TOL), (tag, k, np.abs(got_u - want_u).max())
        assert err < bound, (tag, k, err)
        if Y.mode:
            assert np.array_equal(got_st, want_st), (tag, k)
        worst = max(worst, err)
        x = got_x
    assert A.plant_intervals() == advances
    return worst


# ---- 3: teacher-forced plant, both feedback modes, the cases of the parameter-table tests, the payload alone / with either other table
@pytest.mark.parametrize("config", ["payload", "payload_params", "payload_wrench"])
@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plant_under_a_payload_table_matches_the_host_composition(case, fb, config):
    mode, limits, source, group = CASES[case]
    sv = _sv()
    A = _solver(mode, limits, source=source, fb=fb)
    Y = PayloadYardstick(sv, sc, mode, limits, source)
    x0, ui = _states(group, Y.handle(pc.SETS[0]))
    flags = pc.schedule()[:, 0]
    A.initialize(x0, ui); A.solve(x0)
    assert np.all(np.isfinite(A.ubar())) and np.all(np.isfinite(A.gains_K()))
    payload, table, wrench = _payload_table(), OWN, NO_WRENCH
    tag = "%s fb%d %s" % (case, fb, config)
    assert A.plant_num_payload_sets() == 0 and np.array_equal(A.plant_get_payload(), NO_PAYLOAD)
    if config == "payload_params":
        table = pc.params()
        A.plant_set_params(table)
    if config == "payload_wrench":
        wrench = _wrench_table(); wrench[:, 9] = 1.0; wrench[:, 10] = np.inf                  # every window opens at interval 1
        A.plant_set_wrench(wrench)
    # first, on the yardstick alone: the payload matters in every workgroup
    loaded, bare = (Y.advance_m(A, table, wrench, m, 0, x0, flags, fb)[0] for m in (payload, NO_PAYLOAD))
    _every_workgroup(np.abs(loaded - bare).max(axis=1) > 1e-6, fb, tag)
    A.plant_set_payload(payload)
    assert A.plant_num_payload_sets() == B and np.array_equal(A.plant_get_payload(), payload)
    worst = _teacher_forced_m(A, Y, table, wrench, payload, x0, flags, fb, 2, group, tag)
    print("%s: worst state error under the payloads %.3e" % (tag, worst))
    A.close(); Y.close()


# ---- 4: bit for bit
@pytest.mark.parametrize("fb", [0, 1])
def test_one_record_for_all_is_b_identical_records(fb):
    mode, limits, source, group = CASES["mode4_limits"]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb, ring=2)
    A.initialize(x0, ui); A.solve(x0)
    rec = _payload_table()[3:4]
    A.plant_set_payload(rec)
    assert A.plant_num_payload_sets() == 1 and np.array_equal(A.plant_get_payload(), np.repeat(rec, B, axis=0))
    A.plant_reset(x0); A.plant_follow(0, 2); one = _snapshot(A)
    A.plant_set_payload(np.repeat(rec, B, axis=0))
    assert A.plant_num_payload_sets() == B
    A.plant_reset(x0); A.plant_follow(0, 2); many = _snapshot(A)
    assert _same(one, many) and np.all(one[3] == 1)
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_a_followed_group_is_the_same_in_one_launch_and_in_three(fb):
    m = 3
    mode, limits, source, group = CASES["mode4_limits"]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb, ring=m)
    A.initialize(x0, ui); A.solve(x0)
    wrench = _wrench_table(); wrench[:, 9] = 1.0; wrench[:, 10] = 2.0                         # a window inside the group, beside the payload
    A.plant_set_wrench(wrench); A.plant_set_payload(_payload_table())
    A.plant_reset(x0); A.plant_follow(0, m); fused = _snapshot(A)
    A.plant_reset(x0)
    for j in range(m):
        A.plant_follow(j, 1)
    split = _snapshot(A)
    assert A.plant_intervals() == m and _same(fused, split) and np.all(fused[3] == 1)
    # the payload survives plant_reset and plant_configure
    A.plant_configure(SUBSTEPS, fb, "schedule")
    assert A.plant_num_payload_sets() == B
    A.close()


@pytest.mark.parametrize("case,fb", [("free", 0), ("mode4_limits", 1)])
def test_clearing_the_payload_restores_what_was_launched_before(case, fb):
    mode, limits, source, group = CASES[case]
    x0, ui = _states(group)
    A = _solver(mode, limits, fb=fb, ring=2)
    A.initialize(x0, ui); A.solve(x0)
    A.plant_reset(x0); A.plant_follow(0, 2); none = _snapshot(A)
    wrench = _wrench_table(7)
    A.plant_set_wrench(wrench)
    A.plant_reset(x0); A.plant_follow(0, 2); pushed = _snapshot(A)
    A.plant_set_payload(_payload_table())
    A.plant_reset(x0); A.plant_follow(0, 2); loaded = _snapshot(A)
    assert (np.abs(loaded[0] - pushed[0]).max(axis=1) > 1e-6).all()                            # the payload acts beside the wrench
    A.plant_clear_payload()
    assert A.plant_num_payload_sets() == 0 and np.array_equal(A.plant_get_payload(), NO_PAYLOAD) and A.plant_num_wrench_sets() == B
    A.plant_reset(x0); A.plant_follow(0, 2)
    assert _same(pushed, _snapshot(A))                                                         # the wrench table alone
    A.plant_set_payload(_payload_table())
    A.plant_clear_wrench(); A.plant_clear_payload()
    A.plant_reset(x0); A.plant_follow(0, 2)
    assert _same(none, _snapshot(A))                                                           # the handle without a table
    A.plant_clear_payload()                                                                    # (clearing nothing is fine)
    A.close()


def test_a_handle_with_a_payload_solves_and_steps_as_one_without():
    mode, limits, source, group = CASES["mode4_limits"]
    x0, ui = _states(group)
    out = {}
    for loaded in (False, True):
        A = _solver(mode, limits)
        if loaded:
            A.plant_set_payload(_payload_table())
        A.initialize(x0, ui)
        cost = A.solve(x0)
        out[loaded] = cost, A.xbar(), A.ubar(), A.gains_K(), A.step(x0, ui[:, 0]), A.step_stance(x0, ui[:, 0], 1, 0), A.compute_control(x0)
        A.close()
    assert _same(out[False], out[True])


@pytest.mark.parametrize("table", [False, True])
def test_a_first_knot_gather_and_the_payload_table_do_not_meet(table):
    """ilqr_hip_gather_first_knot stages its rows in a buffer of its own: the gather leaves table, count and plant results as they were, with
    and without a table, and installing / clearing a table between two gathers leaves the gathered rows as they were -- all bit for bit"""
    import torch
    from mpc_ilqr_mujoco_amd import sharding as sh
    mode, limits, source, group = CASES["mode4_limits"]
    x0, ui = _states(group)
    A = _solver(mode, limits, ring=2)
    A.initialize(x0, ui); A.solve(x0)
    payload = _payload_table()

    def gather():
        rows = torch.zeros(B, sh.payload_width(True), dtype=torch.float64, device="cuda:0")
        A.comm_init(1, 0)
        A.gather_first_knot(rows.data_ptr(), root=0, with_gains=True); A.synchronize()
        A.comm_destroy()
        return rows.cpu().numpy()

    if table:
        A.plant_set_payload(payload)
    A.plant_reset(x0); A.plant_follow(0, 2); before = _snapshot(A)
    rows = gather()
    assert np.all(np.isfinite(rows)) and np.abs(rows).max() > 0
    assert A.plant_num_payload_sets() == (B if table else 0) and np.array_equal(A.plant_get_payload(), payload if table else NO_PAYLOAD)
    A.plant_reset(x0); A.plant_follow(0, 2)
    assert _same(before, _snapshot(A))
    A.plant_set_payload(payload[:1]); A.plant_clear_payload()
    assert np.array_equal(gather(), rows) and A.plant_num_payload_sets() == 0
    A.close()


# ---- 5: a rollout that overflows freezes alone, the payload table beside the wrench that overflows it
@pytest.mark.parametrize("fb", [0, 1])
def test_an_overflowing_rollout_freezes_alone_under_the_payload_table(fb):
    bad = 33                                                                                   # in the second workgroup at feedback mode 0
    x0, ui = _states("mid")
    out = {}
    for poisoned in (False, True):
        A = _solver(0, False, fb=fb, ring=2)
        A.initialize(x0, ui); A.solve(x0)
        wrench = _wrench_table()
        wrench[bad] = 0.0
        if poisoned:
            wrench[bad, 0] = 1e308; wrench[bad, 10] = np.inf
        A.plant_set_wrench(wrench); A.plant_set_payload(_payload_table())
        A.plant_reset(x0)
        A.plant_advance()
        out[poisoned] = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        A.close()
    x, u, st, alive = out[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(u[bad] == 0.0) and np.array_equal(x[bad], x0[bad])         # frozen in the state before the advance
    assert np.all(alive[keep] == 1) and np.all(out[False][3] == 1)
    assert np.array_equal(x[keep], out[False][0][keep]) and np.array_equal(u[keep], out[False][1][keep])      # bit for bit


# ---- 6: the runner loads the plant
def test_runner_loaded_pelvises_end_lower():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, Nn, steps, sub = 4, 25, 5, 2
    base = sc.make_problem(sv.reference_kinematics, N=Nn, gravity=dc.GRAVITY)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(Bn, Nn, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    heavy = np.array([False, False, True, True])
    load = sc.stack_plant_payload(Bn, np.where(heavy, 15.0, 0.0), com=(-0.1, 0.0, 0.3), inertia=np.outer(heavy, (0.3, 0.3, 0.2, 0.0, 0.0, 0.0)))      # 0 kg: no inertia either
    res = {}
    for loaded in (False, True):
        s = sv.BatchedILQR(Bn, N=Nn, dt=DT); s.set_max_iterations(2)
        run = ml.MPCRunner(s, rd, base, resident=True, substeps=sub, plant_model=(2, None), plant_payload=load if loaded else None)      # the plant in contact mode 2
        res[loaded] = run.run(x0, steps, u_init=ui)[0]
        assert np.all(s.plant_alive() == 1)
        if loaded:
            assert s.plant_num_payload_sets() == Bn and np.array_equal(s.plant_get_payload(), load)
        s.close()
    dz = res[True][-1][:, 2] - res[False][-1][:, 2]
    # the same sign on the yardstick: the open-loop steps of step_payload from the same states under the same first control
    P = _step_handle(Bn, DT / sub, dc.GRAVITY, 2, False)
    ya, yb = x0.copy(), x0.copy()
    for _ in range(steps * sub):
        ya, yb = P.step_payload(ya, ui[:, 0], 1, 1, load), P.step_payload(yb, ui[:, 0], 1, 1, np.zeros((Bn, 10)))
    P.close()
    dzy = ya[:, 2] - yb[:, 2]
    print("pelvis z, loaded run less unloaded run, after %d intervals: %s; yardstick (open loop): %s" % (steps, dz, dzy))
    assert np.all(dz[heavy] < -1e-6) and np.all(dzy[heavy] < -1e-6)
    assert np.all(np.abs(dzy[~heavy]) == 0.0)


# ---- 7: refusals on a live handle
def test_refusals_on_a_live_handle():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    sv = _sv()
    A = _solver(0, False)
    for bad in (np.ones((2, 10)), np.ones((B, 11))):
        with pytest.raises(ValueError):
            A.plant_set_payload(bad)
    m = _payload_table()
    two = np.ascontiguousarray(m[:2])
    assert A.L.ilqr_hip_plant_set_payload(A.h, two.ctypes.data_as(sv._dp), 2) == 1              # n_sets neither 1 nor B, past the wrapper
    assert A.L.ilqr_hip_plant_set_payload(A.h, None, 1) == 1
    assert A.L.ilqr_hip_plant_get_payload(A.h, None) == 1
    for col, v in ((0, np.nan), (2, np.inf), (5, -np.inf), (0, -1.0), (4, -0.5), (7, 5.0), (9, -5.0)):      # non-finite, m < 0, Ic not positive semidefinite
        q = m.copy(); q[B - 1, col] = v
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_payload(q)
    q = m.copy(); q[0, 4:10] = [1.0, 1.0, 1.0, 0.9, 0.9, -0.9]                                  # every 2 x 2 minor positive, the determinant negative
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        A.plant_set_payload(q)
    x, u = dc.mid()
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        A.step_payload(x[:1], u[:1], 1, 1, q[:1])
    assert A.plant_num_payload_sets() == 0
    A.plant_set_payload(m[:1])                                                                 # one record for all rollouts
    assert A.plant_num_payload_sets() == 1 and np.array_equal(A.plant_get_payload(), np.repeat(m[:1], B, axis=0))
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(A, None, None, plant_payload=m)
    A.close()
