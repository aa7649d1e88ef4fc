"""The task family of the augmented-Lagrangian limits on the GPU (ilqr_hip_set_al_task_bounds: the task instantiations of k_quad_kin,
k_cost_quadratics and k_al_update, k_al_task_knot_cost, k_al_task_shift, k_al_task_points) against the CPU restatement
tests/al_task_ref.py on the inputs of tests/al_task_cases.py, which test_al_task_cpu.py shows to discriminate.

Tolerances are those of test_gpu_augmented_lagrangian.py for the same quantities: 1e-10 max(1, |want|) on the quadratics and 1e-11
relative on the total cost against oracle + restatement, 1e-5 on the cost trace, exact step sizes, 1e-12 on lambda, 1e-5 relative on
multipliers and violations.  The composed reference meets its own redundancy (two weights) to 1e-15 relative on the CPU
(test_al_task_cpu.py), so no margin is taken.  Every test prints the worst error it saw."""
import numpy as np
import pytest

import al_bounds_ref as br
import al_cases as ac
import al_state_ref as sr
import al_task_cases as tc
import al_task_ref as tr
import test_gpu_linearization_cache as lc
from test_gpu_configs import _solver, env

pytestmark = pytest.mark.gpu
NAMES = ("lx", "lu", "lxx", "luu")
SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")
AL = tc.AL_E2E
REF_KEYS = ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref")


def _report(title, worst):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _stage(s):
    s.stage_cost_quadratics()
    return dict(zip(NAMES, s.quadratics())), s.stage_total_cost()


def _install_task(s, win, al=AL):
    s.set_al_task_bounds(win, al["rho_task0"], al["tol_task"])


def _stage_handle(with_task=True):
    X, U, mu_j, mu_c, mu_s, mu_t, rho, win, stance, srec, rec, cases, inf = tc.regimes()
    B, N = X.shape[0], tc.N_STAGE
    s = _solver(B, N=N); s.set_problem(tc.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=tc.STAGE_MARGIN)
    if with_task:
        s.set_al_task_bounds(win, 1.0, 1e-3)
        s.set_al_task_multipliers(mu_t, rho[:, 3])
    s.set_al_multipliers(mu_j, mu_c, rho[:, :2])
    return s


@pytest.mark.parametrize("beside", ["alone", "state_window", "bounds_table"])
def test_stage_parity_every_coordinate_and_side_in_three_regimes_and_stance(beside):
    """Quadratics and total cost of the 54 regime rollouts and the stance rollouts: the task window alone (the model's joint / torque bounds
    repeated over the knots by the library), beside a state window, and beside a whole-horizon joint / torque table (the expanded case)."""
    X, U, mu_j, mu_c, mu_s, mu_t, rho, win, stance, srec, rec, cases, inf = tc.regimes()
    B, N = X.shape[0], tc.N_STAGE
    assert B == 60
    orc = tc.oracle_stage()
    s = _stage_handle()
    if beside == "state_window":
        s.set_al_state_knot_bounds(np.tile(srec[:, None], (1, N + 1, 1)), 1.0, 1e-3); s.set_al_state_multipliers(mu_s, rho[:, 2])
    elif beside == "bounds_table":
        s.set_al_bounds(rec)
    assert s.num_al_task_bound_sets() == B and np.array_equal(s.al_task_bounds(), win)
    assert np.array_equal(s.al_task_multipliers(), mu_t) and np.array_equal(s.al_task_penalties(), rho[:, 3])
    gj, gc = s.al_multipliers()
    assert np.array_equal(gj, mu_j) and np.array_equal(gc, mu_c) and np.array_equal(s.al_penalties(), rho[:, :2])
    got, cost = _stage(s)
    pts = s.al_task_points()
    s.close()
    worst = {}
    want_pts = tr.points(X)
    worst["points"] = np.abs(pts - want_pts).max()
    assert worst["points"] <= 1e-12, worst                                  # (metres; the ankle origins are reference_kinematics' own)
    for b in range(B):
        want, c0 = orc[b]
        w, c = tc.stage_expected(want, c0, b, beside == "bounds_table", beside == "state_window")
        for n in NAMES:
            err = np.abs(got[n][b] - w[n]).max() / max(1.0, np.abs(w[n]).max())
            worst[n] = max(worst.get(n, 0.0), err)
            assert err <= 1e-10, (n, b, cases[b], err)
        worst["cost"] = max(worst.get("cost", 0.0), abs(cost[b] - c) / max(1.0, abs(c)))
        assert abs(cost[b] - c) <= 1e-11 * max(1.0, abs(c)), (b, cases[b], cost[b], c)
        k, side, t, g = cases[b]
        moved = np.abs(got["lx"][b] - (w["lx"] - tc.task_terms()[b][1])).max()      # what the task family adds to lx
        if g < 3 and g < 2 and not (t == 0 and g > 0):
            assert moved > 1.0, (b, cases[b], moved)
        else:
            assert moved <= 1e-10 * max(1.0, np.abs(w["lx"]).max()), (b, cases[b], moved)      # the constant only (inactive; stance)
    _report("stage parity, %s, relative to max(1, |want|)" % beside, worst)


def test_a_window_of_infinite_bounds_is_no_window_and_clear_is_a_fresh_handle():
    """Quadratics and costs under a window of infinite bounds against the same handle's per-knot path without it (a joint / torque window),
    to 1e-13 relative; a three-iteration solve takes the same step sizes and iteration counts, costs to 1e-9.  clear_al_task_bounds against
    a handle that never had a window: bit for bit."""
    X, U, mu_j, mu_c, mu_s, mu_t, rho, win, stance, srec, rec, cases, inf = tc.regimes()
    B, N = X.shape[0], tc.N_STAGE
    s = _stage_handle(with_task=False)
    assert np.isinf(s.al_task_bounds()).all() and s.num_al_task_bound_sets() == 0 and not s.al_task_multipliers().any()
    fresh, cost_f = _stage(s)
    s.set_al_task_bounds(np.tile(tr.NO_BOUNDS, (N + 1, 1)), 5.0, 1e-3)
    assert s.num_al_task_bound_sets() == 1
    inf1, cost1 = _stage(s)
    s.set_al_task_bounds(win, 5.0, 1e-3); s.set_al_task_multipliers(mu_t, rho[:, 3])
    bound, _ = _stage(s)
    assert np.abs(bound["lx"] - fresh["lx"]).max() > 1.0
    s.clear_al_task_bounds()
    assert s.num_al_task_bound_sets() == 0 and not s.al_task_multipliers().any() and not s.al_task_violation().any()
    cleared, cost_c = _stage(s)
    s.close()
    worst = {}
    for n in NAMES:
        assert np.array_equal(cleared[n], fresh[n]), n
        scale = np.maximum(1.0, np.abs(fresh[n]).reshape(B, -1).max(axis=1)).reshape((B,) + (1,) * (fresh[n].ndim - 1))
        e = (np.abs(inf1[n] - fresh[n]) / scale).max(); worst[n] = e
        assert e <= 1e-13, (n, e)
    assert np.array_equal(cost_c, cost_f)
    e = (np.abs(cost1 - cost_f) / np.maximum(1.0, np.abs(cost_f))).max(); worst["cost"] = e
    assert e <= 1e-13, e
    prob, x0, ui = tc.e2e_problem()
    out = []
    for use in (False, True):
        s = _solver(3, N=prob["N"]); s.set_problem(prob); s.set_max_iterations(3)
        s.set_augmented_lagrangian(**dict(tc.al_args(), rounds=1))
        if use:
            s.set_al_task_bounds(np.tile(tr.NO_BOUNDS, (prob["N"] + 1, 1)), 1e3, 1e-3)
        s.initialize(x0, ui); cost = s.solve(x0)
        out.append((cost, s.trace(), s.iterations(), s.al_task_violation(), s.al_task_multipliers()))
        s.close()
    (c0, (tc0, ta0, tl0), it0, _, _), (c1, (tc1, ta1, tl1), it1, v1, m1) = out
    assert np.array_equal(ta0, ta1, equal_nan=True) and np.array_equal(it0, it1) and np.array_equal(tl0, tl1, equal_nan=True)
    assert not v1.any() and not m1.any()
    worst["solve cost"] = (np.abs(c1 - c0) / np.abs(c0)).max()
    assert worst["solve cost"] <= 1e-9
    _report("infinite task window against no window (relative)", worst)


def test_update_kernel_against_numpy():
    N, B = 4, 8
    X = np.array(tc.regimes()[0][:B]); U = np.array(tc.regimes()[1][:B])
    P = tr.points(X)
    stance = np.zeros((B, N + 1, 2), dtype=np.int32); stance[1, 2, 0] = 1
    prob = dict(ac.stage_problem()); prob["stance"] = stance
    win = np.concatenate([P - 0.05, P + 0.06], axis=-1)                     # every point inside its box
    win[0, 2, 9 + 1] = P[0, 2, 1] - 0.03                                    # the task family alone violates (CoM y): not done, every penalty grows
    win[1, 2, 3 + 2] = P[1, 2, 5] + 0.04                                    # violated at a knot where that foot stands only: done
    win[2, 0, 6] = P[2, 0, 6] + 0.055                                      # violated at knot 0 only: done, zero multipliers there
    win[3, N, 9 + 8] = P[3, N, 8] - 0.0005                                  # the terminal knot, within tol_task: done
    win[4, :, 7] = -np.inf; win[4, 3, 9 + 7] = P[4, 3, 7] - 0.01            # a switched-off side beside a violated one
    win[6, 1, 2] = P[6, 1, 2] + 0.02                                        # at the cap of rho_task already
    win[7, 4, 9 + 4] = P[7, 4, 4] - 0.01                                    # growth would pass the cap
    rng = np.random.default_rng(8)
    mu_j = np.zeros((B, N + 1, 19, 2)); mu_c = np.zeros((B, N, 19, 2)); mu_t = np.zeros((B, N + 1, 9, 2))
    mu_t[:, 1:] = rng.uniform(0.0, 30.0, (B, N, 9, 2)); mu_t[2] = 0.0
    al = dict(rounds=2, rho_joint0=100.0, rho_ctrl0=2.0, growth=7.0, rho_max_factor=50.0, margin=0.0, tol_joint=10.0, tol_ctrl=1e6)
    rho = np.tile([100.0, 2.0, 1.0, 400.0], (B, 1)) * (1.0 + 0.1 * np.arange(B))[:, None]
    rho[6] = (5000.0, 100.0, 1.0, 20000.0); rho[7] = (1000.0, 20.0, 1.0, 4000.0)
    rho_max, tol = (5000.0, 100.0, 1e9, 20000.0), (10.0, 1e6, 1.0, 1e-3)
    s = _solver(B, N=N); s.set_problem(prob)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(**al)
    s.set_al_task_bounds(win, 400.0, 1e-3)
    s.set_al_multipliers(mu_j, mu_c, rho[:, :2]); s.set_al_task_multipliers(mu_t, rho[:, 3])
    s.al_update(1)
    gt = s.al_task_multipliers(); grho = np.concatenate([s.al_penalties(), s.al_task_penalties()[:, None]], axis=1)
    viol, done = s.al_violation(); vt = s.al_task_violation(); tr_, tt = s.al_trace(), s.al_task_trace()
    assert np.isnan(s.al_state_trace()).all() and not s.al_state_violation().any()
    s.close()
    assert np.isnan(tr_[0]).all() and np.isnan(tt[0]).all() and tt.shape == (2, B, 2) and vt.shape == (B,)
    jrec = br.default_record(0.0)
    worst = {}
    for b in range(B):
        _, _, _, nt, r2, d2, v2 = tr.update(X[b], U[b], mu_j[b], mu_c[b], np.zeros((N + 1, 28, 2)), mu_t[b], tuple(rho[b]), False, jrec, None, win[b], stance[b],
                                            al["growth"], rho_max, tol)
        assert bool(done[b]) == d2, (b, done[b], d2, vt[b], v2)
        e = abs(vt[b] - v2[3]) / max(1e-3, abs(v2[3])); worst["violation"] = max(worst.get("violation", 0.0), e)
        assert e <= 1e-5 and (vt[b] > 0) == (v2[3] > 0), (b, vt[b], v2)
        assert np.array_equal(gt[b] > 0, nt > 0), b
        err = (np.abs(gt[b] - nt) / np.maximum(1e-300, np.abs(nt)))[nt > 0].max() if nt.any() else np.abs(gt[b]).max()
        worst["mu_task"] = max(worst.get("mu_task", 0.0), err)
        assert err <= 1e-5, (b, err)
        assert tuple(grho[b]) == (r2[0], r2[1], r2[3]), (b, grho[b], r2)
        assert tt[1, b, 0] == vt[b] and tt[1, b, 1] == rho[b, 3] and tuple(tr_[1, b, 2:4]) == tuple(rho[b, :2]), (b, tt[1, b])
        assert not gt[b, 0].any()
    assert list(done) == [0, 1, 1, 1, 0, 1, 0, 0]
    assert vt[1] == 0.0 and vt[2] == 0.0 and not gt[1, 2, 3:6].any() and not gt[4, :, 7, 0].any() and abs(vt[0] - 0.03) < 1e-9
    assert grho[6, 2] == 20000.0 and grho[7, 2] == 20000.0 and abs(grho[0, 2] - 2800.0) < 1e-9 and abs(grho[0, 0] - 700.0) < 1e-9 and grho[3, 2] == rho[3, 3]
    _report("update kernel against NumPy (relative)", worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
def _al_solve(B, prob, x0, ui, win, early_exit, gate=True, setup=None):
    """(observables, AL observables) of one AL solve with the task window on a fresh handle; win None: no window"""
    s = _solver(B, N=prob["N"])
    s.set_problem(prob)
    s.set_options(jacobian_mode=0, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(tc.MAX_ITER)
    s.set_early_exit_gate(gate)
    s.set_augmented_lagrangian(**tc.al_args())
    if setup:
        setup(s)
    if win is not None:
        _install_task(s, win)
    s.initialize(x0, ui); cost = s.solve(x0)
    obs, counters = lc.observables(s, cost)
    mj, mc = s.al_multipliers(); viol, done = s.al_violation()
    extra = dict(mu_j=mj, mu_c=mc, rho=s.al_penalties(), viol=viol, done=done, al_trace=s.al_trace(), mu_t=s.al_task_multipliers(), rho_t=s.al_task_penalties(),
                 viol_t=s.al_task_violation(), task_trace=s.al_task_trace(), win=s.al_task_bounds(), points=s.al_task_points())
    s.close()
    assert counters["adopt"] == 0
    return obs, extra


def _same(a, b):
    lc.assert_same(a[0], b[0])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k


@pytest.fixture(scope="module")
def e2e_runs():
    """the end-to-end case in both exit modes and both launch orders, solved once each: {(early_exit, order): (observables, AL observables)}"""
    prob, x0, ui, win, _ = tc.end_to_end()
    runs = {}
    for early_exit in (False, True):
        runs[early_exit, "default"] = _al_solve(3, prob, x0, ui, win, early_exit)
        with env(**SEQ):
            runs[early_exit, "seq"] = _al_solve(3, prob, x0, ui, win, early_exit)
    return runs


@pytest.mark.parametrize("order", ["default", "seq"])
@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_end_to_end_against_the_reference_driver(early_exit, order, e2e_runs):
    obs, ex = e2e_runs[early_exit, order]
    sol = tc.reference_solves(early_exit)
    prob, x0, ui, win, info = tc.end_to_end()
    tols = (AL["tol_joint"], AL["tol_ctrl"], AL["tol_task"])
    worst = {}
    for b in range(3):
        ref = sol[b]
        want_tr = np.concatenate([ref["al_trace"][:, :2], ref["task_trace"][:, :1]], axis=1)
        got_tr = np.concatenate([ex["al_trace"][:, b, :2], ex["task_trace"][:, b, :1]], axis=1)
        ran = ~np.isnan(want_tr[:, 0])
        assert np.array_equal(~np.isnan(ex["al_trace"][:, b, 0]), ran) and np.array_equal(~np.isnan(ex["task_trace"][:, b, 0]), ran), (b, ex["al_trace"][:, b], want_tr)
        assert np.array_equal(ex["al_trace"][ran, b, 2:], ref["al_trace"][ran, 2:]) and np.array_equal(ex["task_trace"][ran, b, 1], ref["task_trace"][ran, 1]), (b, ex["task_trace"][:, b])
        for r in np.flatnonzero(ran):
            for k in range(3):
                e = abs(got_tr[r, k] - want_tr[r, k]) / max(tols[k], abs(want_tr[r, k]))
                worst["violation"] = max(worst.get("violation", 0.0), e)
                assert e <= 1e-5, (b, r, k, got_tr[r], want_tr[r])
        last = ref["rounds"][-1]                                                 # the existing getters: the last round that ran for the rollout
        n = last["iterations"]
        assert obs["iterations"][b] == n
        assert np.array_equal(obs["trace_alpha"][b, :n], last["trace_alpha"][:n]), (b, obs["trace_alpha"][b], last["trace_alpha"])
        e = np.abs(obs["trace_cost"][b, :n + 1] / last["trace_cost"][:n + 1] - 1).max(); worst["cost trace"] = max(worst.get("cost trace", 0.0), e)
        assert e <= 1e-5, (b, obs["trace_cost"][b], last["trace_cost"])
        e = np.abs(obs["trace_lambda"][b, :n] / last["trace_lambda"][:n] - 1).max(); worst["lambda"] = max(worst.get("lambda", 0.0), e)
        assert e <= 1e-12
        assert bool(ex["done"][b]) == ref["done"] and tuple(ex["rho"][b]) == tuple(ref["rho"]) and ex["rho_t"][b] == ref["rho_t"]
        for name, g_, w_ in (("mu_joint", ex["mu_j"][b], ref["mu_j"]), ("mu_ctrl", ex["mu_c"][b], ref["mu_c"]), ("mu_task", ex["mu_t"][b], ref["mu_t"])):
            e = np.abs(g_ - w_).max() / max(1.0, np.abs(w_).max()); worst[name] = max(worst.get(name, 0.0), e)
            assert e <= 1e-5, (b, name, e)
        assert ex["viol"][b, 0] <= AL["tol_joint"] and ex["viol"][b, 1] <= AL["tol_ctrl"] and ex["viol_t"][b] <= AL["tol_task"] and ex["done"][b]
        e = np.abs(ex["points"][b] - tr.points(obs["xbar"][b])).max(); worst["points"] = max(worst.get("points", 0.0), e)
        assert e <= 1e-12
    assert ex["mu_t"][0, :, 8, 0].max() > 0.0 and ex["mu_t"][1, :, 8, 0].max() > 0.0 and not ex["mu_t"][1, :, 3:6].any() and not ex["mu_t"][2].any()
    # the bounds bind: the right ankle ends within tol_task of its floor where the solve without a window leaves it below
    free = tc.free_solves(early_exit)
    for b in range(2):
        floor = info["z_min"][b] + tc.FOOT_LIFT[b]
        assert ex["points"][b, 1:, 8].min() >= floor - AL["tol_task"] and tr.points(free[b]["X"])[1:, 8].min() < floor - 9 * AL["tol_task"]
    assert np.array_equal(ex["win"], win)
    _report("end to end, %s, %s order (relative)" % ("convergence exit" if early_exit else "fixed", order), worst)


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_rollout_without_bounds_matches_the_solve_without_a_window(early_exit, e2e_runs):
    prob, x0, ui, win, _ = tc.end_to_end()
    obs, ex = e2e_runs[early_exit, "default"]
    o0, e0 = _al_solve(3, prob, x0, ui, None, early_exit)
    # (decisions exactly; values to 1e-9 relative: with a task window the batch runs the per-knot instantiations and takes the model's joint /
    # torque bounds from a window, the same doubles through other machine code)
    for k in ("trace_alpha", "trace_lambda", "iterations"):
        assert np.array_equal(obs[k][2], o0[k][2], equal_nan=True), k
    assert np.array_equal(ex["done"][2], e0["done"][2]) and np.array_equal(ex["rho"][2], e0["rho"][2]) and np.array_equal(ex["al_trace"][:, 2, 2:], e0["al_trace"][:, 2, 2:], equal_nan=True)
    worst = 0.0
    for got, want in [(obs[k][2], o0[k][2]) for k in ("cost", "trace_cost", "xbar", "ubar", "K")] + [(ex[k][2], e0[k][2]) for k in ("mu_j", "mu_c", "viol")] + [(ex["al_trace"][:, 2], e0["al_trace"][:, 2])]:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        worst = max(worst, np.nanmax(np.abs(got - want), initial=0.0) / max(1.0, np.nanmax(np.abs(want), initial=0.0)))
    print("rollout without bounds against the solve without a window (relative to max(1, |want|)): %.2e" % worst)
    assert worst <= 1e-9
    assert np.isnan(e0["task_trace"]).all() and not e0["mu_t"].any() and np.isinf(e0["win"]).all()
    assert not np.array_equal(obs["xbar"][0], o0["xbar"][0]) and not np.array_equal(obs["xbar"][1], o0["xbar"][1])


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_orders_caches_and_listed_spec_match_the_default_bit_for_bit(early_exit, e2e_runs):
    prob, x0, ui, win, _ = tc.end_to_end()
    base = e2e_runs[early_exit, "default"]
    _same(base, e2e_runs[early_exit, "seq"])
    # the three caches switched off -- every rollout linearised, the full first pass, every nominal rollout run -- and the listed order
    for var in (dict(ILQR_RELIN="1"), dict(ILQR_REPASS="1"), dict(ILQR_DEDUP_RETRY="0")):
        with env(**var):
            _same(base, _al_solve(3, prob, x0, ui, win, early_exit))
    _same(base, _al_solve(3, prob, x0, ui, win, early_exit, setup=lambda s: s.set_reroll_nominal(True)))
    _same(base, _al_solve(3, prob, x0, ui, win, early_exit, setup=lambda s: s.set_listed_spec(True)))
    if early_exit:      # the host stops enqueuing rounds once every rollout is done: with the gate off all rounds are enqueued, same results
        _same(base, _al_solve(3, prob, x0, ui, win, True, gate=False))


def _tiled(B, sel=None):
    prob3, x03, ui3, win3, _ = tc.end_to_end()
    idx = np.arange(B) % 3 if sel is None else sel
    pb = dict(prob3)
    for k in REF_KEYS:
        pb[k] = np.ascontiguousarray(prob3[k][idx])
    win = win3[idx].copy()
    for b in range(B):                                                  # every window its own: the floors lifted per rollout
        win[b, :, 8] += np.where(np.isfinite(win[b, :, 8]), 1e-6 * (b // 3), 0.0)
    return pb, np.ascontiguousarray(x03[idx]), np.ascontiguousarray(ui3[idx]), win, idx


def test_windows_permute_and_broadcast_bit_for_bit_at_b_70():
    """B = 70, wider than one control group and one wave of the knot-cost kernels, 70 windows of their own: permuting the windows with the
    rollouts permutes the results (the windows are indexed by the rollout, never by a list position); one window equals B copies of it."""
    B = 70
    pb, x0, ui, win, idx = _tiled(B)
    perm = np.random.default_rng(3).permutation(B)
    a = _al_solve(B, pb, x0, ui, win, True)
    pb2 = dict(pb)
    for k in REF_KEYS:
        pb2[k] = np.ascontiguousarray(pb[k][perm])
    b = _al_solve(B, pb2, np.ascontiguousarray(x0[perm]), np.ascontiguousarray(ui[perm]), win[perm], True)
    for k in lc.NAMES:
        assert np.array_equal(a[0][k][perm], b[0][k], equal_nan=True), k
    for k in a[1]:
        ak = a[1][k][:, perm] if k in ("al_trace", "task_trace") else a[1][k][perm]
        assert np.array_equal(ak, b[1][k], equal_nan=True), k
    assert len({tuple(r) for r in a[0]["xbar"][0::3, -1]}) > 1                # the lifted floors are felt
    one = _al_solve(B, pb, x0, ui, win[1], True)
    many = _al_solve(B, pb, x0, ui, np.tile(win[1], (B, 1, 1)), True)
    _same(one, many)


def test_two_batch_slices_carry_their_own_windows():
    """ILQR_SLICES=2 at B = 128 (a slice holds at least 64 rollouts): the second slice moved on by one, so that rollout 64 + i carries another
    window than rollout i -- a slice that forgot the offset b0 * stride of the window or of the store would solve it under rollout i's.
    Every rollout repeats the unsliced run of its own inputs to 1e-9, decisions exactly."""
    B = 128
    sel = (np.arange(B) + (np.arange(B) >= 64)) % 3
    pb, x0, ui, win, idx = _tiled(B, sel)
    assert idx[64] != idx[0]
    whole = _al_solve(B, pb, x0, ui, win, True)
    with env(ILQR_SLICES="2"):
        s = _solver(B, N=pb["N"]); assert s.L.ilqr_hip_num_slices(s.h) == 2; s.close()
        obs, ex = _al_solve(B, pb, x0, ui, win, True)
    worst = 0.0
    for k in ("trace_alpha", "trace_lambda", "iterations"):
        assert np.array_equal(obs[k], whole[0][k], equal_nan=True), k
    assert np.array_equal(ex["done"], whole[1]["done"])
    assert np.array_equal(ex["win"], whole[1]["win"])
    for got, want in [(obs[k], whole[0][k]) for k in ("trace_cost", "xbar", "ubar", "K")] + [(ex[k], whole[1][k]) for k in ex if k != "win"]:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        worst = max(worst, np.nanmax(np.abs(got - want), initial=0.0) / max(1.0, np.nanmax(np.abs(want), initial=0.0)))
    print("ILQR_SLICES=2, B = 128 against the unsliced run (relative to max(1, |want|)): %.2e" % worst)
    assert worst <= 1e-9, worst


def test_warm_start_shifts_the_task_multipliers_and_keeps_the_window():
    prob, x0, ui, win, _ = tc.end_to_end()
    N = prob["N"]
    rng = np.random.default_rng(10)
    for path, shift in (("resident", 1), ("resident", 3), ("host", 1)):
        s = _solver(3, N=N); s.set_problem(prob); s.set_max_iterations(tc.MAX_ITER); s.set_augmented_lagrangian(**tc.al_args())
        _install_task(s, win)
        s.initialize(x0, ui); s.solve(x0)
        assert s.al_task_multipliers().max() > 0.0 and not np.array_equal(s.al_task_penalties(), np.full(3, AL["rho_task0"]))
        mt = rng.uniform(1.0, 2.0, (3, N + 1, 9, 2)); mt[:, 0] = 0.0      # (fill the store so that every slot of the shift is checked)
        mj, mc = s.al_multipliers()
        s.set_al_task_multipliers(mt, None)
        assert np.array_equal(s.al_task_multipliers(), mt)
        if path == "resident":
            s.initialize_warm_resident(x0, shift=shift)
        else:
            s.initialize(x0, None, s.xbar(), s.ubar())
        want = tr.shift(mt, shift)
        got = s.al_task_multipliers()
        assert np.array_equal(got, want) and want[:, 1:N - shift + 1].all() and not got[:, N - shift + 1:].any() and not got[:, 0].any(), (path, shift)
        assert np.array_equal(s.al_task_penalties(), np.full(3, AL["rho_task0"])) and not s.al_task_violation().any()
        wj, wc_ = ac.ar.shift(mj, mc, shift)
        gj, gc = s.al_multipliers()
        assert np.array_equal(gj, wj) and np.array_equal(gc, wc_)
        assert s.num_al_task_bound_sets() == 3 and np.array_equal(s.al_task_bounds(), win)      # horizon-local: the window stays
        s.initialize(x0, ui)                                                # a cold start zeros them
        assert not s.al_task_multipliers().any() and s.num_al_task_bound_sets() == 3
        s.close()


def test_closed_loop_runner_under_a_window_equals_the_loop_driven_by_hand():
    """A two-step MPCRunner loop (no argument of its own: the window lives on the solver handle) against the same two steps driven by hand,
    bit for bit; the window stays, the second solve starts from shifted multipliers, and the floor is felt."""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    from mpc_ilqr_mujoco_amd import solver as sv
    sc = tc.sc
    prob3, x03, ui3 = ac.end_to_end()
    B, steps, N = 2, 2, prob3["N"]
    base = sc.make_problem(sv.reference_kinematics, N=N)
    for k in ("Q", "R", "Qf"):
        base[k] = np.array(prob3[k])
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (40, 1))); rd.contact = np.ones((40, 2), dtype=np.int32); rd.contact[:, 1] = 0
    x0 = np.array(x03[[0, 0]]); ui = np.array(ui3[[0, 0]])
    z0 = float(tr.points(x0[0])[8])
    win = sc.stack_al_task_bounds([dict(swing_clearance=z0 - 2e-4), dict()], B, N)
    runs = {}
    for how in ("runner", "hand", "none"):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(tc.MAX_ITER); s.set_augmented_lagrangian(**tc.al_args())
        if how != "none":
            _install_task(s, win)
        if how != "hand":
            xs, us = ml.MPCRunner(s, rd, base).run(x0, steps, u_init=ui)
        else:
            x = x0.copy(); xs, us = [x.copy()], []
            for k in range(steps):
                s.set_problem(rd.problem_at(k, N, base, follow_schedule=False))
                if k == 0:
                    s.initialize(x, ui)
                else:
                    s.initialize_warm_resident(x)
                    assert not s.al_task_multipliers()[:, [0, N]].any() and np.array_equal(s.al_task_penalties(), np.full(B, AL["rho_task0"]))
                s.solve(x)
                u = s.compute_control(x); x = s.step(x, u)
                xs.append(x.copy()); us.append(u.copy())
        mt = s.al_task_multipliers()
        if how != "none":
            assert np.array_equal(s.al_task_bounds(), win) and s.num_al_task_bound_sets() == B
        s.close()
        runs[how] = (np.asarray(xs), np.asarray(us), mt)
    for a_, b_ in zip(runs["runner"], runs["hand"]):
        assert np.array_equal(a_, b_)
    # (the multipliers themselves may end at zero: a round that lifts the foot past its floor clears them)
    assert not runs["runner"][2][1].any() and not runs["runner"][2][0, :, 3:6].any()
    felt = not np.array_equal(runs["runner"][1][:, 0], runs["none"][1][:, 0])
    print("closed loop under a task window: largest task multiplier at the end %.3g, plan differs from the loop without a window: %s" % (runs["runner"][2].max(), felt))
    # (the unbounded rollout beside it: the same plan through the per-knot instantiations, to 1e-9)
    assert felt and np.abs(runs["runner"][1][:, 1] - runs["none"][1][:, 1]).max() <= 1e-9 * max(1.0, np.abs(runs["none"][1][:, 1]).max())


def test_lifecycle_and_refusals():
    from mpc_ilqr_mujoco_amd import solver as sv
    import weight_set_cases as wc
    prob, x0, ui, win, _ = tc.end_to_end()
    N = prob["N"]
    s = _solver(3, N=N); s.set_problem(prob); s.set_max_iterations(tc.MAX_ITER)
    for call in (lambda: _install_task(s, win), s.clear_al_task_bounds, s.al_task_bounds, s.al_task_multipliers, s.al_task_penalties, s.al_task_violation, s.al_task_points,
                 lambda: s.set_al_task_multipliers(np.zeros((3, N + 1, 9, 2)))):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            call()
    assert s.num_al_task_bound_sets() == 0
    s.set_augmented_lagrangian(**tc.al_args())
    assert np.array_equal(s.al_task_bounds(), np.tile(tr.NO_BOUNDS, (3, N + 1, 1))) and not s.al_task_multipliers().any() and not s.al_task_violation().any()
    assert np.isnan(s.al_task_trace()).all()
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.set_al_task_multipliers(np.zeros((3, N + 1, 9, 2)))
    _install_task(s, win)
    nan, up, dn, cross = (win.copy() for _ in range(4))
    nan[1, 2, 5] = np.nan; up[0, 3, 3] = np.inf; dn[2, N, 9 + 7] = -np.inf; cross[1, 1, 2] = 2.0; cross[1, 1, 11] = 1.0
    for bad, rho0, tol in ((nan, 1.0, 1e-3), (up, 1.0, 1e-3), (dn, 1.0, 1e-3), (cross, 1.0, 1e-3), (win[:2], 1.0, 1e-3), (win, 0.0, 1e-3), (win, -1.0, 1e-3),
                           (win, np.inf, 1e-3), (win, np.nan, 1e-3), (win, 1.0, -1e-9), (win, 1.0, np.nan)):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_al_task_bounds(bad, rho0, tol)
        assert s.num_al_task_bound_sets() == 3 and np.array_equal(s.al_task_bounds(), win) and np.array_equal(s.al_task_penalties(), np.full(3, AL["rho_task0"]))
    with pytest.raises(ValueError):
        s.set_al_task_bounds(win[:, :N], 1.0)
    assert s.L.ilqr_hip_set_al_task_bounds(s.h, None, 3, sv.C.c_double(1.0), sv.C.c_double(1e-3)) == 1
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        s.set_al_task_multipliers(-np.ones((3, N + 1, 9, 2)))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        s.set_al_task_multipliers(None, np.zeros(3))
    # survives the initialisers, set_al_multipliers, the other families coming and going and a repeated install; weight sets stay refused
    s.initialize(x0, ui); s.solve(x0)
    first = s.al_task_multipliers()
    assert first.max() > 0.0
    s.set_al_multipliers(None, None, np.tile([1e5, 1e3], (3, 1)))
    s.set_al_bounds(sv.al_default_bounds(0.0)); s.clear_al_bounds()
    s.set_al_state_bounds(sr.NO_BOUNDS, 1.0); s.clear_al_state_bounds()
    s.set_al_knot_bounds(np.tile(sv.al_default_bounds(0.0), (N + 1, 1))); s.clear_al_bounds()
    assert s.al_bounds_per_knot() == 0
    s.initialize_warm_resident(x0, shift=1)
    s.set_augmented_lagrangian(**tc.al_args())
    assert s.num_al_task_bound_sets() == 3 and np.array_equal(s.al_task_bounds(), win) and not s.al_task_multipliers().any()
    sets = wc.one_set_arrays(wc.problem_of_set(wc.weight_set_problem(3, N, 3), 0))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        s.set_weight_sets(*sets)
    s.set_regularization(1e-6)                                                # (lambda outlives a solve)
    s.initialize(x0, ui); s.solve(x0)
    assert np.array_equal(s.al_task_multipliers(), first)                     # and the solve is the first one again
    # a one-set window, then cleared with AL: a fresh installation has none
    s.set_al_task_bounds(win[1], 1.0); assert s.num_al_task_bound_sets() == 1 and np.array_equal(s.al_task_bounds(), np.tile(win[1], (3, 1, 1)))
    s.clear_augmented_lagrangian()
    assert s.num_al_task_bound_sets() == 0
    s.set_augmented_lagrangian(**tc.al_args())
    assert s.num_al_task_bound_sets() == 0 and np.isinf(s.al_task_bounds()).all()
    s.close()
    # a family of the test library that evaluates the cost inside its own rollout / line-search kernels
    t = _solver(3, N=N, legacy=True); t.set_problem(prob); t.set_max_iterations(tc.MAX_ITER)
    t.set_augmented_lagrangian(**tc.al_args()); _install_task(t, win)
    t.initialize(x0, ui)
    with env(ILQR_DYN="s"):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            t.solve(x0)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            t.set_augmented_lagrangian(**tc.al_args())
    t.solve(x0)
    assert t.num_al_task_bound_sets() == 3
    t.close()
