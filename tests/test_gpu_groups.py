"""Solve groups on the GPU (include/ilqr_hip.h ilqr_hip_set_groups ...; csrc/group_kernels.hip k_group_perturb, k_group_select, k_group_adopt of
the module libilqr_hip_groups.so), on the product library.

Ground truth, none of it the new kernels: the NumPy restatement of the selection rule and of the perturbation (tests/group_ref.py, held to the
published Philox vectors on the CPU); for the adoption a second handle R whose every member is GIVEN the start of the winner, solved by the
kernels that existed before -- after the adoption the grouped handle must equal it bit for bit, and go on equal through a warm start and another
solve; the CPU oracle fixes the winners of those cases with a margin of 1e-3 (tests/test_groups_cpu.py).  The designed starts go in through
set_trajectory as (the oracle's rollout of the controls, the controls): a solve reports the cost of the trajectory it is given for a rollout
that accepts no step, so the trajectory has to be the one the oracle's keys were computed from.

Shapes (tests/group_cases.py): (B, G) = (40, 8), (40, 5), (128, 64), (39, 3); N = 6 and N = 5 -- odd and even doubles per rollout in xbar, ubar and
the gains, the 8-byte-off and the 16-byte-aligned path of k_group_adopt.

Bound of the perturbation: PERTURB_TOL = 1e-13 max(1, sigma) absolute on ubar.  The draws: the bound tests/test_gpu_observation.py derives --
the integer part of the generator is exact, the arguments of log and cos / sin are bit-identical on both sides, a few ulp of libm difference at
r <= 8.7 stay below 1e-14 -- times sigma for the product; the sum then rounds to half an ulp of a control below 256 Nm, 1.4e-14, and a product
that differs by that much can move the rounded sum by one more ulp, 2.8e-14: 1e-14 sigma + 4.2e-14 < 1e-13 max(1, sigma)."""
import os
import shutil

import numpy as np
import pytest

import group_cases as gc
import group_ref as gr
import handle_walk_cases as hw
from conftest import load_package

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU = 51, 19
DRAW_TOL = 1e-13                    # tests/test_gpu_observation.py
STEP_ABS = 1e-10                    # a step of contact mode 0 without rows against ilqr_hip_step (tests/test_gpu_payload.py, dynamics golden)


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _solver(B, N, iters):
    s = _sv().BatchedILQR(B, N=N, dt=gc.DT)
    s.set_problem(gc.problem(N))
    s.set_options(early_exit=False)
    s.set_max_iterations(iters)
    return s


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _solution(s):
    """what the getters report of a solved handle"""
    return dict(xbar=s.xbar(), ubar=s.ubar(), K=s.gains_K(), kff=s.gains_kff(), cost=s.cost(), lam=s.lambdas(), iters=s.iterations())


def _assert_equal(got, want, tag, rows=None):
    for k in want:
        g, w = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        assert _same(g, w), (tag, k, int(np.sum(g != w)))


# ---- 1: select on caller keys
@pytest.mark.parametrize("B,G", gc.SHAPES)
def test_select_on_caller_keys_is_the_numpy_rule(B, G):
    import torch
    s = _sv().BatchedILQR(B, N=5, dt=gc.DT)
    try:
        s.set_groups(G)
        assert s.num_groups() == B // G
        for i, keys in enumerate(gc.select_batches(B, G)):
            want_w, want_r = gr.select(keys, G)
            t = torch.tensor(keys, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            s.group_select(t if i % 2 == 0 else t.data_ptr())                                  # a tensor or a device pointer
            w, r = s.group_winners()
            assert np.array_equal(w, want_w) and _same(r, want_r), (B, G, i)
        wp, rp = s.group_winners_device()
        assert wp and rp
    finally:
        s.close()


# ---- 2: perturb
@pytest.mark.parametrize("B,G,N,hold,rows", [(40, 8, 6, 1, "G"), (39, 3, 5, 2, "1"), (128, 64, 6, 4, "G"), (40, 5, 5, 7, "1")])
def test_perturb_matches_the_restatement_and_the_solve_rolls_from_it(B, G, N, hold, rows):
    sv = _sv()
    seed, stream0 = 0xFEED_0000_0000_0001 + B, (1 << 34) + G
    x0, ui = gc.group_inputs(B // G, G, N)
    sigma = sc.stack_group_sigma(G, np.linspace(0.05, 2.0, NU), ladder=np.linspace(1.0, 0.25, G - 1)) if rows == "G" else np.linspace(2.0, 0.0, NU)[None]
    tol = DRAW_TOL * np.maximum(1.0, np.atleast_2d(sigma).max())
    s = _solver(B, N, 1)
    p = _solver(B, N, 1)
    try:
        s.set_groups(G)
        s.group_set_perturbation(sigma, hold=hold, seed=seed, stream0=stream0)
        assert s.group_draws() == 0
        s.initialize(x0, ui)
        u0 = s.ubar()
        assert np.array_equal(u0, ui)
        s.group_perturb()
        u1 = s.ubar()
        assert s.group_draws() == 1
        member = np.arange(B) % G
        assert np.array_equal(u1[member == 0], ui[member == 0])                                 # the incumbents: bit-identical
        want1 = gr.perturbed(ui, G, sigma, hold, seed, stream0, 0)
        err1 = float(np.abs(u1 - want1).max())
        moved = np.abs(u1 - ui).max(axis=(1, 2)) > 1e-3
        assert err1 < tol and np.array_equal(moved, member != 0), (err1, tol)
        if rows == "1":                                                                          # the last actuator's sigma is zero: its controls keep their bits
            assert np.array_equal(u1[:, :, NU - 1], ui[:, :, NU - 1])
        if hold > 1:                                                                             # one draw per `hold` knots
            d = u1 - ui
            assert np.abs(d[:, 1] - d[:, 0]).max() < 1e-12 and (hold >= N or np.abs(d[:, hold] - d[:, 0]).max() > 1e-3)
        # the solve that follows rolls the trajectory out from the perturbed controls: one iteration equals, bit for bit, the iteration of a plain
        # handle that is given the downloaded controls and rolls them out in front of its iteration 0 as well (solve(x0): a new x0) -- a grouped
        # handle that kept the trajectory of the unperturbed controls would differ in every member g >= 1 ...
        s.solve(None)
        p.initialize(x0, u1); p.solve(x0)
        got, want = _solution(s), _solution(p)
        _assert_equal(got, want, "one iteration behind the perturbation")
        # ... and what it leaves is a rollout of the controls it leaves, knot by knot against ilqr_hip_step
        worst = 0.0
        for t in range(N):
            nxt = s.step(got["xbar"][:, t], got["ubar"][:, t])
            worst = max(worst, float((np.abs(nxt - got["xbar"][:, t + 1]) / np.maximum(1.0, np.abs(nxt))).max()))
        assert worst < STEP_ABS, worst
        # a second call: draw 1, on top of what the solve left
        ub = got["ubar"]
        s.group_perturb()
        u2 = s.ubar()
        err2 = float(np.abs(u2 - gr.perturbed(ub, G, sigma, hold, seed, stream0, 1)).max())
        assert s.group_draws() == 2 and err2 < tol and np.array_equal(u2[member == 0], ub[member == 0])
        assert not np.array_equal(u2 - ub, u1 - ui)
        # installing again returns the counter to 0; clearing removes the perturbation
        s.group_set_perturbation(sigma, hold=hold, seed=seed, stream0=stream0)
        assert s.group_draws() == 0
        s.group_clear_perturbation()
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            s.group_perturb()
        print("(%d, %d) N = %d hold %d: draw 0 %.2e, draw 1 %.2e (bound %.1e); rollout against step %.2e (bound %.0e)" % (B, G, N, hold, err1, err2, tol, worst, STEP_ABS))
    finally:
        s.close(); p.close()


# ---- 3: the incumbent
def test_member_0_is_the_plain_solve_and_the_group_never_does_worse():
    B, G, N = gc.INC_B, gc.INC_G, gc.INC_N
    x0, ui = gc.incumbent_starts()
    s, p = _solver(B, N, gc.INC_ITERS), _solver(B, N, gc.INC_ITERS)
    try:
        s.set_groups(G)
        s.group_set_perturbation(gc.incumbent_sigma(), hold=gc.INC_HOLD, seed=gc.INC_SEED, stream0=gc.INC_STREAM0)
        s.initialize(x0, ui); s.group_perturb(); s.solve(None)
        p.initialize(x0, ui); p.solve(x0)                                                        # (a new x0: the plain handle rolls out in front of iteration 0 too)
        got, want = _solution(s), _solution(p)
        _assert_equal(got, want, "member 0 against the plain handle", rows=np.arange(0, B, G))
        s.group_select()
        w, rec = s.group_winners()
        assert np.all(rec[:, 0] <= rec[:, 1]) and np.array_equal(rec[:, 1], want["cost"][::G]) and np.array_equal(rec[:, 0], got["cost"][w])
        assert np.array_equal(rec[:, 2], np.full(B // G, float(G))) and np.array_equal(rec[:, 3], got["cost"].reshape(-1, G).max(axis=1))
        ow, _ = gr.select(gc.incumbent_oracle_keys(), G)
        rel = float((np.abs(got["cost"] - gc.incumbent_oracle_keys()) / gc.incumbent_oracle_keys()).max())
        print("incumbent: winners %s (oracle %s), cost against the oracle %.2e relative" % (w - np.arange(B // G) * G, ow - np.arange(B // G) * G, rel))
        assert np.array_equal(w, ow) and (w % G != 0).any() and (w % G == 0).any()
    finally:
        s.close(); p.close()


# ---- 4: adopt copies everything that matters
def _al_table(M, G):
    """one table of joint / torque bounds per group, repeated over its members"""
    return sc.repeat_for_groups(hw.al_jc_table(M), G)


def _install_al(s, M, G):
    s.set_augmented_lagrangian(**hw.al_install_args(hw.START, s.B))
    s.set_al_bounds(_al_table(M, G))


def _al_state(s):
    joint, ctrl = s.al_multipliers()
    viol, done = s.al_violation()
    return dict(mu_joint=joint, mu_ctrl=ctrl, rho=s.al_penalties(), viol=viol, done=done)


@pytest.mark.parametrize("N", gc.HORIZONS)
@pytest.mark.parametrize("al", [False, True])
def test_adopt_leaves_the_handle_that_was_given_the_winners_start(N, al):
    B, G = gc.ADOPT_B, gc.ADOPT_G
    M = B // G
    x0, ui = gc.adopt_starts(N)
    xg = gc.adopt_trajectory(N)
    A, R = _solver(B, N, gc.ADOPT_ITERS), _solver(B, N, gc.ADOPT_ITERS)
    try:
        if al:
            _install_al(A, M, G); _install_al(R, M, G)
        A.set_groups(G)
        A.set_trajectory(xg, ui); A.solve(None)
        before = _solution(A)
        A.group_select()
        w, rec = A.group_winners()
        member = w - np.arange(M) * G
        if not al:                                                                               # the winners the oracle fixed (tests/test_groups_cpu.py)
            assert np.array_equal(member, [gc.good_member(m) for m in range(M)]), member
            assert gc.margins(before["cost"], G).min() > gc.MARGIN
        print("N = %d, augmented Lagrangian %s: winners' members %s" % (N, al, member))
        assert (member != 0).any()
        A.group_adopt()
        src = np.repeat(w, G)                                                                    # every member <- its group's winner
        after = _solution(A)
        _assert_equal(after, {k: v[src] for k, v in before.items()}, "adopt is a copy of the winner")
        # handle R: every member of group m is given the start of A's winner of group m
        R.set_trajectory(xg[src], ui[src]); R.solve(None)
        _assert_equal(after, _solution(R), "after the adoption")
        if al:
            al_before = _al_state(R)
            _assert_equal(_al_state(A), al_before, "multipliers, penalties, violation after the adoption")
            assert np.abs(al_before["mu_ctrl"]).max() > 0.0 or np.abs(al_before["mu_joint"]).max() > 0.0      # (the update has written multipliers)
        # both go on: warm start from the same state, solve, control law at knots 0 and 3
        xw = sc.repeat_for_groups(hw.inputs(gc.POOL)["x_warm"][np.array(gc.POOL_ROWS)[np.arange(M) % len(gc.POOL_ROWS)]], G)
        for h in (A, R):
            h.initialize_warm_resident(xw); h.solve(None)
        _assert_equal(_solution(A), _solution(R), "the solve after the adoption")
        xm = xw + 0.01
        for knot in (0, 3):
            assert np.array_equal(A.compute_control(xm, knot=knot), R.compute_control(xm, knot=knot)), knot
        if al:
            _assert_equal(_al_state(A), _al_state(R), "multipliers, penalties, violation after the second solve")
        # within a group every member is now one rollout
        sol = _solution(A)
        assert all(np.array_equal(sol[k].reshape((M, G) + sol[k].shape[1:])[:, g], sol[k].reshape((M, G) + sol[k].shape[1:])[:, 0]) for k in sol for g in range(G))
    finally:
        A.close(); R.close()


@pytest.mark.parametrize("B,G,N", [(40, 5, 6), (128, 64, 5), (39, 3, 6), (39, 3, 5)])
def test_adopt_on_the_other_shapes_copies_the_winner_chosen_by_a_key(B, G, N):
    """the groups that do not fill or divide a wave, winners spread over the members by a caller's key: every slab of every member equals the
    winner's afterwards and nothing outside the solution state moves (the traces stay the member's own)"""
    import torch
    M = B // G
    x0, ui = gc.group_inputs(M, G, N)
    rng = np.random.default_rng(B + G + N)
    ui = np.clip(ui + rng.uniform(-3.0, 3.0, ui.shape), -0.8 * sc.CTRLRANGE, 0.8 * sc.CTRLRANGE)      # every member its own start
    keys = rng.uniform(1.0, 2.0, B)
    keys[np.arange(M) * G + (np.arange(M) * 2 + 1) % G] = 0.5                                     # the winner of group m: member (2 m + 1) mod G
    s = _solver(B, N, 2)
    try:
        s.set_groups(G)
        s.initialize(x0, ui); s.solve(None)
        before, trace = _solution(s), s.trace()
        t = torch.tensor(keys, dtype=torch.float64, device="cuda:0"); torch.cuda.synchronize()
        s.group_select(t); s.group_adopt()
        w, rec = s.group_winners()
        assert np.array_equal(w, gr.select(keys, G)[0]) and np.array_equal(rec[:, 0], np.full(M, 0.5))
        src = np.repeat(w, G)
        assert not np.array_equal(before["ubar"], before["ubar"][src])
        _assert_equal(_solution(s), {k: v[src] for k, v in before.items()}, (B, G, N))
        assert all(_same(a, b) for a, b in zip(s.trace(), trace))
    finally:
        s.close()


# ---- 5: a winner that is already member 0, and G = 1 after G = 8
def test_a_winning_incumbent_keeps_every_bit_and_groups_off_leave_a_fresh_handle():
    import torch
    B, G, N = 40, 8, 6
    x0, ui = gc.adopt_starts(N)
    s, f = _solver(B, N, 2), _solver(B, N, 2)
    try:
        s.set_groups(G)
        s.initialize(x0, ui); s.solve(None)
        before = _solution(s)
        keys = np.tile(np.arange(G, dtype=np.float64), B // G)                                   # member 0 wins every group
        keys[G:2 * G] = np.nan                                                                   # ... group 1 by default: no finite key
        t = torch.tensor(keys, dtype=torch.float64, device="cuda:0"); torch.cuda.synchronize()
        s.group_select(t); s.group_adopt()
        w, _ = s.group_winners()
        assert np.array_equal(w, np.arange(0, B, G))
        after = _solution(s)
        src = np.repeat(w, G)
        _assert_equal(after, {k: v[src] for k, v in before.items()}, "adopt from member 0")
        _assert_equal(after, before, "the incumbents keep every bit", rows=w)
        s.set_groups(1)
        assert s.num_groups() == 0
        with pytest.raises(_sv().ILQRError, match="ILQR_ERR_STATE"):
            s.group_adopt()
        # (lambda survives a solve by design, tests/test_gpu_handle_walk.py: both handles start the comparison from the initial value)
        s.set_regularization(hw.LAMBDA0); s.initialize(x0, ui); s.solve(None)
        f.set_regularization(hw.LAMBDA0); f.initialize(x0, ui); f.solve(None)
        _assert_equal(_solution(s), _solution(f), "groups off: the next solve is a fresh handle's")
        _assert_equal(_solution(s), before, "... which is the solve in front of the adoption")
    finally:
        s.close(); f.close()


# ---- 6: closed loop
def _runner_inputs(M, G, N):
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    base = sc.make_problem(sv.reference_kinematics, N=N)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (40, 1))); rd.contact = np.ones((40, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(M, N, 31, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    return base, rd, sc.repeat_for_groups(x0, G), sc.repeat_for_groups(ui, G)


def test_closed_loop_with_starts_keeps_the_plants_of_a_group_identical():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    sv = _sv()
    B, G, N, steps = 8, 4, 6, 4
    base, rd, x0, ui = _runner_inputs(B // G, G, N)

    def run(**kw):
        # (contact mode 2, as the runner tests of the plant tables: the constraint-free standing solve returns a non-finite cost)
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(3); s.set_contact_mode(2)
        r = ml.MPCRunner(s, rd, base, resident=True, **kw)
        xs, us = r.run(x0, steps, u_init=ui)
        groups = s.num_groups()
        s.close()
        return xs, us, r.winners, groups

    xp, up, wp, gp = run()
    assert wp is None and gp == 0
    # sigma = 0: every member solves the plain problem; states and controls of every member are the plain runner's, bit for bit
    xz, uz, wz, gz = run(starts=G, start_sigma=0.0)
    assert gz == B // G and np.array_equal(xz, xp) and np.array_equal(uz, up)
    assert wz.shape == (steps, B // G) and np.all(wz // G == np.arange(B // G)[None, :])
    # a non-zero sigma: the plants of a group stay bit-identical to each other, one row of winners per solve, every winner inside its group
    xs, us, w, _ = run(starts=G, start_sigma=sc.stack_group_sigma(G, 1.5), start_hold=2, start_seed=5)
    assert np.all(np.isfinite(xs)) and w.shape == (steps, B // G)
    assert np.all(w // G == np.arange(B // G)[None, :])
    for g in range(1, G):
        assert np.array_equal(xs[:, g::G], xs[:, 0::G]) and np.array_equal(us[:, g::G], us[:, 0::G]), g
    xs2, us2, w2, _ = run(starts=G, start_sigma=sc.stack_group_sigma(G, 1.5), start_hold=2, start_seed=5, solve_every=2)
    assert w2.shape == (steps // 2, B // G) and np.all(w2 // G == np.arange(B // G)[None, :]) and np.array_equal(xs2[:, 1::G], xs2[:, 0::G])
    print("closed loop: winners' members per solve %s; sigma moved the controls by %.2e" % ((w % G).tolist(), float(np.abs(us - up).max())))


# ---- 7: refusals
REF_B, REF_G, REF_N = 8, 4, 5


def _ref_inputs():
    return gc.group_inputs(REF_B // REF_G, REF_G, REF_N)


_fresh_solution = {}


def _fresh():
    """a fresh handle's cold solve of the refusal batch, computed once and left unchanged"""
    if not _fresh_solution:
        x0, ui = _ref_inputs()
        f = _solver(REF_B, REF_N, 2)
        try:
            f.set_regularization(hw.LAMBDA0); f.initialize(x0, ui); f.solve(None)
            _fresh_solution.update(_solution(f))
        finally:
            f.close()
    return _fresh_solution


def _c(s, name, *args):
    """the C entry point itself (the Python methods check some arguments before the library sees them)"""
    s._chk(getattr(s.L, name)(s.h, *args))


def _sigma_call(n_sets, values, hold=1):
    import ctypes as C
    v = np.ascontiguousarray(values, dtype=np.float64)
    return lambda s: _c(s, "ilqr_hip_group_set_perturbation", n_sets, v.ctypes.data_as(C.POINTER(C.c_double)), hold, C.c_ulonglong(1), C.c_ulonglong(0))


def _refusals():
    import ctypes as C
    ok = sc.stack_group_sigma(REF_G, 1.0)
    row0 = ok.copy(); row0[0, 3] = 1e-3
    neg = ok.copy(); neg[2, 5] = -1e-9
    nan = ok.copy(); nan[1, 0] = np.nan
    inf = ok.copy(); inf[3, 18] = np.inf
    on = lambda s: s.set_groups(REF_G)
    on_sigma = lambda s: (s.set_groups(REF_G), s.group_set_perturbation(ok))
    nothing = lambda s: None
    return [
        # (name, state: cold | solved | fresh, before, the refused call, code)
        ("set_groups_0", "solved", nothing, lambda s: _c(s, "ilqr_hip_set_groups", 0), "ILQR_ERR_ARG"),
        ("set_groups_does_not_divide", "solved", on, lambda s: _c(s, "ilqr_hip_set_groups", 3), "ILQR_ERR_ARG"),
        ("sigma_sets_neither_1_nor_G", "solved", on, _sigma_call(2, ok[:2]), "ILQR_ERR_ARG"),
        ("sigma_row_0_not_zero", "solved", on, _sigma_call(REF_G, row0), "ILQR_ERR_ARG"),
        ("sigma_negative", "solved", on, _sigma_call(REF_G, neg), "ILQR_ERR_ARG"),
        ("sigma_nan", "solved", on, _sigma_call(REF_G, nan), "ILQR_ERR_ARG"),
        ("sigma_inf", "solved", on, _sigma_call(REF_G, inf), "ILQR_ERR_ARG"),
        ("sigma_null", "solved", on, lambda s: _c(s, "ilqr_hip_group_set_perturbation", 1, None, 1, C.c_ulonglong(1), C.c_ulonglong(0)), "ILQR_ERR_ARG"),
        ("hold_0", "solved", on, _sigma_call(1, ok[1:2], hold=0), "ILQR_ERR_ARG"),
        ("sigma_while_groups_are_off", "solved", nothing, _sigma_call(1, ok[1:2]), "ILQR_ERR_STATE"),
        ("perturb_before_initialize", "fresh", on_sigma, lambda s: s.group_perturb(), "ILQR_ERR_STATE"),
        ("perturb_while_groups_are_off", "solved", nothing, lambda s: s.group_perturb(), "ILQR_ERR_STATE"),
        ("perturb_without_a_perturbation", "solved", on, lambda s: s.group_perturb(), "ILQR_ERR_STATE"),
        ("select_while_groups_are_off", "solved", nothing, lambda s: s.group_select(), "ILQR_ERR_STATE"),
        ("select_on_the_cost_before_a_solve", "cold", on, lambda s: s.group_select(), "ILQR_ERR_STATE"),
        ("winners_before_a_select", "solved", on, lambda s: s.group_winners(), "ILQR_ERR_STATE"),
        ("adopt_before_a_select", "solved", on, lambda s: s.group_adopt(), "ILQR_ERR_STATE"),
        ("adopt_while_groups_are_off", "solved", nothing, lambda s: s.group_adopt(), "ILQR_ERR_STATE"),
    ]


REFUSALS = ("set_groups_0", "set_groups_does_not_divide", "sigma_sets_neither_1_nor_G", "sigma_row_0_not_zero", "sigma_negative", "sigma_nan", "sigma_inf",
            "sigma_null", "hold_0", "sigma_while_groups_are_off", "perturb_before_initialize", "perturb_while_groups_are_off", "perturb_without_a_perturbation",
            "select_while_groups_are_off", "select_on_the_cost_before_a_solve", "winners_before_a_select", "adopt_before_a_select", "adopt_while_groups_are_off")


@pytest.mark.parametrize("case", REFUSALS)
def test_refused_group_call_leaves_the_next_solve_unchanged(case):
    sv = _sv()
    assert [r[0] for r in _refusals()] == list(REFUSALS)
    name, state, before, call, code = next(r for r in _refusals() if r[0] == case)
    x0, ui = _ref_inputs()
    want = _fresh()
    s = _solver(REF_B, REF_N, 2)
    try:
        if state != "fresh":
            s.initialize(x0, ui)
        if state == "solved":
            s.solve(None)
        before(s)
        with pytest.raises(sv.ILQRError, match=code):
            call(s)
        s.set_regularization(hw.LAMBDA0); s.initialize(x0, ui); s.solve(None)      # (lambda survives a solve by design: back to the initial value, as the fresh handle's)
        _assert_equal(_solution(s), want, name)
    finally:
        s.close()


def test_a_missing_module_is_an_error_not_a_fall_back(tmp_path):
    """a copy of the product library in a directory without libilqr_hip_groups.so: set_groups says which file is missing"""
    sv = _sv()
    lib = str(tmp_path / "libilqr_hip.so")
    shutil.copy(sv.LIB_PATH, lib)
    s = sv.BatchedILQR(REF_B, N=REF_N, dt=gc.DT, lib_path=lib)
    try:
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED.*libilqr_hip_groups.so"):
            s.set_groups(REF_G)
        assert s.num_groups() == 0
        s.set_groups(1)                                                                          # switching off needs no module
    finally:
        s.close()
    assert os.path.exists(os.path.join(os.path.dirname(sv.LIB_PATH), "libilqr_hip_groups.so"))
