"""CPU checks of the per-knot bounds of the augmented-Lagrangian limits (ilqr_hip_set_al_knot_bounds, ilqr_hip_set_al_state_knot_bounds,
ilqr_hip_al_bounds_window_from_track): the restatement tests/al_knot_ref.py against al_bounds_ref.py / al_state_ref.py under constant rows,
the discrimination of the stage inputs of tests/al_knot_cases.py (a kernel that reads another row than knot t's changes gradient or cost by
more than the GPU tolerance in every case), the helpers of scenario.py, the track cut as NumPy indexing, the null-handle checks of the new
entry points, and the conditions of the end-to-end case on the reference driver alone."""
import ctypes as C

import numpy as np
import pytest

import al_bounds_cases as bc
import al_bounds_ref as br
import al_cases as ac
import al_knot_cases as kc
import al_knot_ref as kr
import al_state_cases as stc
import al_state_ref as sr
import oracle_lib as ol

sc = ac.sc
N = ac.N_STAGE
# the GPU tolerances of test_gpu_al_bounds._check_stage: 1e-10 max(1, |want|) on a quadratic, 1e-11 max(1, |cost|) on the cost; a mis-read
# has to move one of them by MARGIN times that
QUAD_TOL, COST_TOL, MARGIN = 1e-10, 1e-11, 100.0


def _lib():
    import test_capi_cpu as tc
    return tc._lib()


def test_new_entry_points_check_a_null_handle():
    sv, L = _lib()
    buf = np.zeros(76 * 5)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    ip = np.zeros(1, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert L.ilqr_hip_set_al_knot_bounds(None, p, 1) == 1      # ILQR_ERR_ARG
    assert L.ilqr_hip_set_al_state_knot_bounds(None, p, 1, C.c_double(1.0), C.c_double(1e-3)) == 1
    assert L.ilqr_hip_get_al_knot_bounds(None, p, p) == 1
    assert L.ilqr_hip_al_bounds_per_knot(None) == -1
    assert L.ilqr_hip_set_al_bounds_track(None, 1, p, None) == 1
    assert L.ilqr_hip_clear_al_bounds_track(None) == 1
    assert L.ilqr_hip_al_bounds_track_rows(None) == -1
    assert L.ilqr_hip_set_al_bounds_track_starts(None, ip, 1) == 1
    assert L.ilqr_hip_al_bounds_window_from_track(None, 0) == 1


def test_constant_rows_reproduce_the_whole_horizon_restatement_exactly():
    X, U, mu_j, mu_c, rho, rec, cases, _ = bc.regimes_table()
    rest = (7.0, (5000.0, 100.0), (1e-3, 1e-2))
    for b in range(0, X.shape[0], 5):
        win = kr.as_window(rec[b], N)
        for a, c in zip(br.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b], rec[b]), kr.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b], win)):
            assert np.array_equal(a, c), (b, cases[b])
        assert br.violation(X[b], U[b], rec[b]) == kr.violation(X[b], U[b], win)
        for done in (False, True):
            old = br.update(X[b], U[b], mu_j[b], mu_c[b], tuple(rho[b]), done, rec[b], *rest)
            new = kr.update(X[b], U[b], mu_j[b], mu_c[b], tuple(rho[b]), done, win, *rest)
            assert all(np.array_equal(a, c) for a, c in zip(old[:2], new[:2])) and old[2:] == new[2:], (b, done)
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, _ = stc.regimes()
    rest = (7.0, (5000.0, 100.0, 900.0), (1e-3, 1e-2, 1e-3))
    for b in range(0, X.shape[0], 5):
        win, swin = kr.as_window(rec[b], N), kr.as_window(srec[b], N)
        for a, c in zip(sr.traj_terms(X[b], mu_s[b], rho[b, 2], srec[b]), kr.state_traj_terms(X[b], mu_s[b], rho[b, 2], swin)):
            assert np.array_equal(a, c), (b, cases[b])
        assert sr.violation(X[b], srec[b]) == kr.state_violation(X[b], swin)
        for done in (False, True):
            old = sr.update(X[b], U[b], mu_j[b], mu_c[b], mu_s[b], tuple(rho[b]), done, rec[b], srec[b], *rest)
            new = kr.state_update(X[b], U[b], mu_j[b], mu_c[b], mu_s[b], tuple(rho[b]), done, win, swin, *rest)
            assert all(np.array_equal(a, c) for a, c in zip(old[:3], new[:3])) and old[3:] == new[3:], (b, done)


def _oracle_scales(X, U):
    """per rollout (max |lx|, max |lu|, |cost|) of the oracle at zero constraint weights: what the GPU tolerances are relative to"""
    prob = dict(ac.stage_problem()); prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob)
    out = []
    for b in range(X.shape[0]):
        o.set_trajectory(X[b], U[b]); o.cost_quadratics()
        out.append((np.abs(o.get("lx")).max(), np.abs(o.get("lu")).max(), abs(o.total_cost())))
    return out


def test_the_joint_and_torque_windows_discriminate_every_case():
    """228 cases: under the window the case is in its designed regime (the terms of knot t are those of regimes_table's record); with row t
    replaced by row t - 1, t + 1, 0 or N the gradient entry of the case, or where the case has none (knot 0 of a hinge carries no
    multiplier but its cost term) the cost, moves by more than MARGIN x the GPU tolerance"""
    X, U, mu_j, mu_c, rho, rec, cases, _ = bc.regimes_table()
    win = kc.joint_windows()
    assert win.shape == (228, N + 1, 76) and len(cases) == 228
    scales = _oracle_scales(X, U)
    least = np.inf
    for b, (kind, j, side, t, g) in enumerate(cases):
        assert np.array_equal(win[b, t], rec[b])
        args = (X[b], U[b], mu_j[b], mu_c[b], rho[b])
        ck, gx, hx, gu, hu = kr.traj_terms(*args, win[b])
        ck0, gx0, hx0, gu0, hu0 = br.traj_terms(*args, rec[b])
        assert ck[t] == ck0[t] and (np.array_equal(gx[t], gx0[t]) if kind == "joint" else np.array_equal(gu[t], gu0[t]))
        lxs, lus, cs = scales[b]
        for s in kc.misread_rows(t, N, N):
            bad = win[b].copy(); bad[t] = win[b, s]
            if kind == "ctrl":
                bad[t, :38] = win[b, t, :38]       # (the mis-read of the torque fields alone)
            ck2, gx2, _, gu2, _ = kr.traj_terms(*args, bad)
            dg = abs(gx2[t, j] - gx[t, j]) / (QUAD_TOL * max(1.0, lxs)) if kind == "joint" else abs(gu2[t, j] - gu[t, j]) / (QUAD_TOL * max(1.0, lus))
            dc = abs(ck2.sum() - ck.sum()) / (COST_TOL * max(1.0, cs + abs(ck.sum())))
            least = min(least, max(dg, dc))
            assert max(dg, dc) > MARGIN, (b, cases[b], s, dg, dc)
    print("joint / torque windows: the weakest mis-read moves gradient or cost by %.3g x the GPU tolerance" % least)


def test_the_state_windows_discriminate_every_case():
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, _ = stc.regimes()
    swin, jwin = kc.state_windows()
    assert swin.shape == (168, N + 1, 56) and jwin.shape == (168, N + 1, 76) and len(cases) == 168
    assert len({jwin[0, t].tobytes() for t in range(N + 1)}) == N + 1      # every row of the joint / torque window another record
    scales = _oracle_scales(X, U)
    least = np.inf
    for b, (k, side, t, g) in enumerate(cases):
        assert np.array_equal(swin[b, t], srec[b])
        sk, sg, sh = kr.state_traj_terms(X[b], mu_s[b], rho[b, 2], swin[b])
        sk0, sg0, _ = sr.traj_terms(X[b], mu_s[b], rho[b, 2], srec[b])
        assert sk[t] == sk0[t] and np.array_equal(sg[t], sg0[t])
        lxs, _, cs = scales[b]
        for s in kc.misread_rows(t, N, N):
            bad = swin[b].copy(); bad[t] = swin[b, s]
            sk2, sg2, _ = kr.state_traj_terms(X[b], mu_s[b], rho[b, 2], bad)
            dg = abs(sg2[t, k] - sg[t, k]) / (QUAD_TOL * max(1.0, lxs))
            dc = abs(sk2.sum() - sk.sum()) / (COST_TOL * max(1.0, cs + abs(sk.sum())))
            least = min(least, max(dg, dc))
            assert max(dg, dc) > MARGIN, (b, cases[b], s, dg, dc)
        # the joint / torque family under jwin: inactive in every row, as under the whole-horizon record
        _, gx, hx, gu, hu = kr.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b, :2], jwin[b])
        assert not gx.any() and not gu.any() and not hx.any() and not hu.any(), b
    print("state windows: the weakest mis-read moves gradient or cost by %.3g x the GPU tolerance" % least)


def test_stack_al_knot_bounds_triples_defaults_and_refusals():
    sv, _ = _lib()
    B, Nn = 3, 6
    d0, d1 = sv.al_default_bounds(0.0), sv.al_default_bounds(0.1)
    w = sc.stack_al_knot_bounds({}, B, Nn)
    assert w.shape == (1, Nn + 1, 76) and np.array_equal(w[0], np.tile(d0, (Nn + 1, 1)))
    w = sc.stack_al_knot_bounds([dict(ctrl_hi=(2, 5, {13: 16.2})), dict(torque_scale=[(0, 2, 0.5), (4, 7, 0.0)], joint_lo={3: -0.1}), {}], B, Nn, margin=0.1)
    assert w.shape == (B, Nn + 1, 76)
    want = np.tile(d1, (Nn + 1, 1)); want[2:5, 57 + 13] = 16.2
    assert np.array_equal(w[0], want)
    want = np.tile(d1, (Nn + 1, 1)); want[:, 3] = -0.1; want[0:2, 38:] *= 0.5; want[4:7, 38:] = 0.0
    assert np.array_equal(w[1], want) and np.array_equal(w[2], np.tile(d1, (Nn + 1, 1)))
    assert np.array_equal(sc.stack_al_knot_bounds(dict(ctrl_hi=np.full(19, 5.0)), B, Nn)[0, :, 57:], np.full((Nn + 1, 19), 5.0))      # a plain value: every knot
    s = sc.stack_al_state_knot_bounds([dict(pelvis_z=(3, 7, (0.9, np.inf))), dict(joint_speed=[(0, 1, 2.0), (1, 7, 3.0)]), {}], B, Nn)
    assert s.shape == (B, Nn + 1, 56)
    assert np.all(s[0, :3, 2] == -np.inf) and np.all(s[0, 3:, 2] == 0.9) and np.all(s[0, :, 30] == np.inf)
    assert np.all(s[1, 0, 9:28] == -2.0) and np.all(s[1, 1:, 28 + 9:] == 3.0)
    assert np.all(s[2, :, :28] == -np.inf) and np.all(s[2, :, 28:] == np.inf)
    for bad in (dict(ctrl_hi=(2, 9, {13: 1.0})), dict(ctrl_hi=(-1, 2, {13: 1.0})), dict(ctrl_hi=(3, 2, {13: 1.0})), dict(nonsense=(0, 1, 2.0)),
                dict(ctrl_lo=(0, 2, {13: 50.0})), dict(joint_lo=(1, 2, {0: float("nan")}))):
        with pytest.raises(ValueError):
            sc.stack_al_knot_bounds(bad, B, Nn)
    with pytest.raises(ValueError):
        sc.stack_al_knot_bounds([{}, {}], B, Nn)
    with pytest.raises(ValueError):
        sc.stack_al_state_knot_bounds(dict(pelvis_z=(0, 3, (1.0, 0.5))), B, Nn)
    with pytest.raises(ValueError):
        sc.stack_al_state_knot_bounds(dict(pelvis_z=(0, 8, (0.5, 1.0))), B, Nn)


def test_the_track_cut_is_numpy_indexing():
    rows, Nn, B = 11, 4, 3
    track = np.arange(rows * 76, dtype=np.float64).reshape(rows, 76)
    w = kr.cut(track, [0], 0, Nn, B)
    assert w.shape == (B, Nn + 1, 76) and all(np.array_equal(w[b], track[:Nn + 1]) for b in range(B))
    w = kr.cut(track, [0, 3, 9], 1, Nn, B)
    assert np.array_equal(w[0], track[1:6]) and np.array_equal(w[1], track[4:9])
    assert np.array_equal(w[2], track[[10, 10, 10, 10, 10]])               # the end clamp: rows past the track repeat its last row
    w = kr.cut(track, [5], 4, Nn, B)
    assert np.array_equal(w[1], track[[9, 10, 10, 10, 10]])
    assert np.array_equal(kr.cut(track, [2], 100, Nn, B)[0], np.tile(track[-1], (Nn + 1, 1)))


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_the_reference_driver_meets_the_conditions_of_the_end_to_end_case(early_exit):
    prob, x0, ui, win, swin, info = kc.end_to_end()
    Nn = prob["N"]
    assert x0.shape[0] == 4 and win.shape == (4, Nn + 1, 76) and swin.shape == (4, Nn + 1, 56)
    d = br.default_record(kc.AL_E2E["margin"])
    assert np.array_equal(win[0, :kc.T_S], np.tile(d, (kc.T_S, 1))) and np.all(win[0, kc.T_S:, 57 + kc.WRIST] == kc.WRIST_BOUND)
    assert np.all(win[1, :, 57 + kc.WRIST] == kc.WRIST_BOUND) and np.all(win[1, :, 38 + kc.WRIST] == -kc.WRIST_BOUND)
    assert np.array_equal(win[3], np.tile(d, (Nn + 1, 1))) and np.all(np.isinf(swin[[0, 1, 3]]))
    assert np.all(np.diff(swin[2, :, 2]) > 0) and np.all(np.isinf(np.delete(swin[2], 2, axis=1)))      # the height bound rises over the window
    sols = kc.reference_solves(early_exit)
    figures = kc.effect_assertions(sols)
    # rollout 2: the unconstrained solution violates the rising bound at the end of the horizon alone; the solve under it ends closer
    v_free = kr.state_violation(np.column_stack([np.zeros((Nn + 1, 2)), info["z_free"], np.zeros((Nn + 1, 48))]), swin[2])
    assert abs(v_free - kc.Z_LIFT) < 1e-12 and np.all(info["z_free"][:-1] > info["z_lo"][:-1] + 1e-3)
    assert sols[2]["viol"][2] < 0.5 * v_free and sols[2]["mu_s"][Nn, 2, 0] > 0.0 and not sols[2]["mu_s"][:Nn].any(), sols[2]["viol"]
    # rollout 3: the solve without any table (al_state_ref.Driver under the model's record and no state bounds)
    plain = sr.Driver(prob, 3, kc.AL_E2E, d, sr.NO_BOUNDS, max_iter=kc.MAX_ITER, early_exit=early_exit).solve(x0[3], ui[3])
    for k in ("X", "U", "mu_j", "mu_c", "mu_s", "al_trace"):
        assert np.array_equal(sols[3][k], plain[k], equal_nan=True), k
    assert sols[3]["cost"] == plain["cost"] and sols[3]["done"] == plain["done"]
    print("end-to-end conditions on the reference driver: %s, viol_state of rollout 2 %.3g (unconstrained %.3g)" % (figures, sols[2]["viol"][2], v_free))
