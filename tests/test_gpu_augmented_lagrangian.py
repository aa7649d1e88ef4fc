"""Augmented-Lagrangian joint and torque limits on the GPU (ilqr_hip_set_augmented_lagrangian: the AL instantiations of k_cost_quadratics and
k_traj_knot_cost, k_al_update, k_al_shift, k_solve_begin_al and the round loop of the solve) against the CPU restatement tests/al_ref.py on
the inputs of tests/al_cases.py, which test_augmented_lagrangian_cpu.py shows to discriminate.

Tolerances are those of the existing tests of the same quantities: 1e-10 max(1, |want|) on the quadratics and 1e-11 relative on the total
cost against the oracle (test_limit_sweep_every_row_and_side_of_both_tables, test_scrambled_problem_stage_by_stage), 1e-5 on the cost
trace, exact step sizes and 1e-12 on lambda against the reference driver (test_full_solve_parity_trace_and_gains), 1e-5 relative on
multipliers and violations.  Every test prints the worst error it saw."""
import numpy as np
import pytest

import al_cases as ac
import al_ref as ar
import oracle_lib as ol
import test_gpu_linearization_cache as lc
from test_gpu_configs import _solver, env

pytestmark = pytest.mark.gpu
sc = ac.sc
NAMES = ("lx", "lu", "lxx", "luu")
SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")      # the sequential order of the headline batch (test_gpu_first_pass_skip.py)
DIAG = np.arange(7, 26)


def _report(title, worst):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _stage(s, X, U):
    s.stage_cost_quadratics()
    return dict(zip(NAMES, s.quadratics())), s.stage_total_cost()


@pytest.fixture(scope="module")
def oracle_stage():
    """the oracle at ZERO constraint weights on the two regime sets: {m: [(quadratics, cost) per rollout]}; computed once"""
    prob = dict(ac.stage_problem()); prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob)
    out = {}
    for m in (0.0, 0.1):
        X, U = ac.regimes(m)[:2]
        rows = []
        for b in range(X.shape[0]):
            o.set_trajectory(X[b], U[b]); o.cost_quadratics()
            rows.append(({n: o.get(n) for n in NAMES}, o.total_cost()))
        out[m] = rows
    return out


@pytest.mark.parametrize("m", [0.0, 0.1])
def test_stage_parity_every_row_and_side_in_three_regimes(m, oracle_stage):
    X, U, mu_j, mu_c, rho, cases = ac.regimes(m)
    B, N = X.shape[0], ac.N_STAGE
    assert B == 228
    s = _solver(B, N=N); s.set_problem(ac.stage_problem())             # (both plain penalties on: AL must replace them)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=m)
    s.set_al_multipliers(mu_j, mu_c, rho)
    gj, gc = s.al_multipliers()
    assert np.array_equal(gj, mu_j) and np.array_equal(gc, mu_c) and np.array_equal(s.al_penalties(), rho)
    got, cost = _stage(s, X, U)
    s.close()
    worst = {}
    for b in range(B):
        want, c0 = oracle_stage[m][b]
        ck, gx, hx, gu, hu = ar.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b], m)
        w = {n: want[n].copy() for n in NAMES}
        w["lx"][:, 7:26] += gx; w["lu"] += gu; w["luu"] += hu; w["lxx"][:, DIAG, DIAG] += hx
        for n in NAMES:
            err = np.abs(got[n][b] - w[n]).max() / max(1.0, np.abs(w[n]).max())
            worst[n] = max(worst.get(n, 0.0), err)
            assert err <= 1e-10, (n, b, cases[b], err)
        c = c0 + ck.sum()
        worst["cost"] = max(worst.get("cost", 0.0), abs(cost[b] - c) / max(1.0, abs(c)))
        assert abs(cost[b] - c) <= 1e-11 * max(1.0, abs(c)), (b, cases[b], cost[b], c)
        kind, j, side, t, g = cases[b]
        if g == 0:                                                     # the active entry is there, with the sign of its side
            v = got["lx"][b, t, 7 + j] - want["lx"][t, 7 + j] if kind == "joint" else got["lu"][b, t, j] - want["lu"][t, j]
            assert (v > 0) == bool(side) and abs(v) > 1.0, (b, cases[b], v)
    _report("stage parity, margin %g, relative to max(1, |want|)" % m, worst)


def test_zero_multiplier_identity_against_the_plain_penalty():
    """mu = 0, rho = 2 w, m = 0.1 against the same handle with AL cleared and the plain weights w: costs and every entry of the quadratics to
    1e-13 relative (the total cost, a sum of five knot costs, stands for the per-knot costs, which no getter exposes); a three-iteration
    solve at rounds = 1 takes the same step sizes and iteration counts."""
    X, U = ac.regimes(0.1)[:2]
    B = X.shape[0]
    prob = ac.stage_problem()
    w = prob["w_joint"]
    assert prob["w_ctrl"] == w
    s = _solver(B, N=ac.N_STAGE); s.set_problem(prob)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    plain, cost0 = _stage(s, X, U)
    s.set_augmented_lagrangian(1, 2 * w, 2 * w, margin=0.1)
    assert s.augmented_lagrangian_rounds() == 1
    al, cost1 = _stage(s, X, U)
    s.clear_augmented_lagrangian()
    assert s.augmented_lagrangian_rounds() == 0
    again, cost2 = _stage(s, X, U)
    s.close()
    worst = {}
    for n in NAMES:
        assert np.array_equal(plain[n], again[n]), n
        scale = np.maximum(1.0, np.abs(plain[n]).reshape(B, -1).max(axis=1)).reshape((B,) + (1,) * (plain[n].ndim - 1))
        worst[n] = (np.abs(al[n] - plain[n]) / scale).max()
        assert worst[n] <= 1e-13, (n, worst[n])
    assert np.array_equal(cost0, cost2)
    worst["cost"] = (np.abs(cost1 - cost0) / np.maximum(1.0, np.abs(cost0))).max()
    assert worst["cost"] <= 1e-13 and np.count_nonzero(cost0 > 1.0) >= 76
    # the solve
    prob, x0, ui = ac.end_to_end()
    prob = dict(prob); w = prob["w_joint"]
    out = []
    for use_al in (False, True):
        s = _solver(3, N=prob["N"]); s.set_problem(prob); s.set_max_iterations(3)
        if use_al:
            s.set_augmented_lagrangian(1, 2 * w, 2 * prob["w_ctrl"], margin=0.1)
        s.initialize(x0, ui); cost = s.solve(x0)
        out.append((cost, s.trace(), s.iterations()))
        s.close()
    (c0, (tc0, ta0, tl0), it0), (c1, (tc1, ta1, tl1), it1) = out
    assert np.array_equal(ta0, ta1, equal_nan=True) and np.array_equal(it0, it1) and np.array_equal(tl0, tl1, equal_nan=True)
    worst["solve cost"] = (np.abs(c1 - c0) / np.abs(c0)).max()
    assert worst["solve cost"] <= 1e-9
    _report("zero multipliers against the plain penalty (relative)", worst)


def test_update_kernel_against_numpy():
    N, B = 4, 6
    jr, cr = ar.ranges()
    rng = np.random.default_rng(5)
    prob = ac.stage_problem()
    X = np.tile(sc.standing_state(), (B, N + 1, 1)); X[..., 7:26] += rng.uniform(-0.2, 0.2, (B, N + 1, 19))      # (inside every range)
    U = rng.uniform(-0.7, 0.7, (B, N, 19)) * sc.CTRLRANGE
    X[0, 2, 7 + 3] = jr[3, 1] + 0.07; U[0, 1, 4] = cr[4, 0] - 3.0            # both families violate
    X[1, 0, 7 + 0] = jr[0, 1] + 0.2                                         # knot 0 alone: done, zero multipliers
    X[2, N, 7 + 9] = jr[9, 0] - 0.01                                        # the terminal knot; at the rho cap
    U[3, N - 1, 18] = cr[18, 1] + 0.004                                     # within tol_ctrl: done
    X[4, 1, 7 + 14] = jr[14, 1] + 0.0005                                    # within tol_joint: done
    X[5, 3, 7 + 2] = jr[2, 1] + 0.3                                         # not done: its penalties grow, up to the cap
    mu_j = np.zeros((B, N + 1, 19, 2)); mu_c = np.zeros((B, N, 19, 2))
    mu_j[:, 1:] = rng.uniform(0.0, 30.0, (B, N, 19, 2)); mu_c[:] = rng.uniform(0.0, 30.0, (B, N, 19, 2))
    mu_j[1] = 0.0; mu_c[1] = 0.0
    al = dict(rounds=2, rho_joint0=100.0, rho_ctrl0=2.0, growth=7.0, rho_max_factor=50.0, margin=0.0, tol_joint=1e-3, tol_ctrl=1e-2)
    rho = np.tile([100.0, 2.0], (B, 1)) * (1.0 + 0.1 * np.arange(B))[:, None]
    rho[2] = (5000.0, 100.0)                                                # at the cap already
    rho[5] = (1000.0, 20.0)                                                 # growth would pass the cap
    s = _solver(B, N=N); s.set_problem(prob)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(**al)
    s.set_al_multipliers(mu_j, mu_c, rho)
    s.al_update(1)
    gj, gc = s.al_multipliers(); grho = s.al_penalties(); viol, done = s.al_violation(); tr = s.al_trace()
    s.close()
    assert np.isnan(tr[0]).all()
    worst = {}
    for b in range(B):
        nj, nc, r2, d2, v2 = ar.update(X[b], U[b], mu_j[b], mu_c[b], tuple(rho[b]), False, 0.0, al["growth"], (5000.0, 100.0), (1e-3, 1e-2))
        assert bool(done[b]) == d2 and tuple(viol[b]) == v2, (b, done[b], d2, viol[b], v2)
        assert np.array_equal(gj[b] > 0, nj > 0) and np.array_equal(gc[b] > 0, nc > 0), b
        for name, g_, w_ in (("mu_joint", gj[b], nj), ("mu_ctrl", gc[b], nc), ("rho", grho[b], np.array(r2))):
            err = (np.abs(g_ - w_) / np.maximum(1e-300, np.abs(w_))).max() if w_.any() else np.abs(g_).max()
            worst[name] = max(worst.get(name, 0.0), err)
            assert err <= 1e-14, (b, name, err)
        assert tuple(tr[1, b, :2]) == v2 and tuple(tr[1, b, 2:4]) == tuple(rho[b]) and tr[1, b, 4] == 0.0
    assert list(done) == [0, 1, 0, 1, 1, 0]
    assert not gj[1].any() and not gc[1].any()
    assert tuple(grho[2]) == (5000.0, 100.0) and tuple(grho[5]) == (5000.0, 100.0) and abs(grho[0, 0] - 700.0) < 1e-9
    _report("update kernel against NumPy (relative)", worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
def _al_solve(B, prob, x0, ui, early_exit, setup=None, gate=True):
    """(observables, AL observables) of one AL solve on a fresh handle"""
    s = _solver(B, N=prob["N"])
    s.set_problem(prob)
    s.set_options(jacobian_mode=0, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(ac.MAX_ITER)
    s.set_early_exit_gate(gate)
    if setup:
        setup(s)
    s.set_augmented_lagrangian(**ac.AL_E2E)
    s.initialize(x0, ui); cost = s.solve(x0)
    obs, counters = lc.observables(s, cost)
    mj, mc = s.al_multipliers(); viol, done = s.al_violation()
    extra = dict(mu_j=mj, mu_c=mc, rho=s.al_penalties(), viol=viol, done=done, al_trace=s.al_trace())
    s.close()
    assert counters["adopt"] == 0
    return obs, extra


def _same(a, b):
    lc.assert_same(a[0], b[0])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k


@pytest.fixture(scope="module")
def e2e_runs():
    """the end-to-end case in both modes and both launch orders, solved once: {(early_exit, order): (observables, AL observables)}"""
    prob, x0, ui = ac.end_to_end()
    out = {}
    for early_exit in (False, True):
        out[early_exit, "default"] = _al_solve(3, prob, x0, ui, early_exit)
        with env(**SEQ):
            out[early_exit, "seq"] = _al_solve(3, prob, x0, ui, early_exit)
    return out


@pytest.mark.parametrize("order", ["default", "seq"])
@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_end_to_end_against_the_reference_driver(early_exit, order, e2e_runs):
    obs, ex = e2e_runs[early_exit, order]
    sol, _ = ac.reference_solves(early_exit)
    al = ac.AL_E2E
    worst = {}
    for b in range(3):
        ref = sol[b]
        want_tr = ref["al_trace"]
        ran = ~np.isnan(want_tr[:, 0])
        assert np.array_equal(~np.isnan(ex["al_trace"][:, b, 0]), ran), (b, ex["al_trace"][:, b], want_tr)
        assert np.array_equal(ex["al_trace"][ran, b, 2:], want_tr[ran, 2:]), (b, ex["al_trace"][:, b], want_tr)      # penalties and iteration counts
        for r in np.flatnonzero(ran):
            for k in range(2):
                e = abs(ex["al_trace"][r, b, k] - want_tr[r, k]) / max(al["tol_joint"] if k == 0 else al["tol_ctrl"], abs(want_tr[r, k]))
                worst["violation"] = max(worst.get("violation", 0.0), e)
                assert e <= 1e-5, (b, r, k, ex["al_trace"][r, b], want_tr[r])
        last = ref["rounds"][-1]                                                 # the existing getters: the last round that ran for the rollout
        n = last["iterations"]
        assert obs["iterations"][b] == n
        assert np.array_equal(obs["trace_alpha"][b, :n], last["trace_alpha"][:n]), (b, obs["trace_alpha"][b], last["trace_alpha"])
        e = np.abs(obs["trace_cost"][b, :n + 1] / last["trace_cost"][:n + 1] - 1).max(); worst["cost trace"] = max(worst.get("cost trace", 0.0), e)
        assert e <= 1e-5, (b, obs["trace_cost"][b], last["trace_cost"])
        e = np.abs(obs["trace_lambda"][b, :n] / last["trace_lambda"][:n] - 1).max(); worst["lambda"] = max(worst.get("lambda", 0.0), e)
        assert e <= 1e-12
        assert bool(ex["done"][b]) == ref["done"] and tuple(ex["rho"][b]) == tuple(ref["rho"])
        for name, g_, w_ in (("mu_joint", ex["mu_j"][b], ref["mu_j"]), ("mu_ctrl", ex["mu_c"][b], ref["mu_c"])):
            e = np.abs(g_ - w_).max() / max(1.0, np.abs(w_).max()); worst[name] = max(worst.get(name, 0.0), e)
            assert e <= 1e-5, (b, name, e)
        assert ex["viol"][b, 0] <= al["tol_joint"] and ex["viol"][b, 1] <= al["tol_ctrl"]
    assert not ex["mu_j"][0].any() and not ex["mu_c"][0].any() and ex["mu_j"][2].max() > 0.0
    _report("end to end, %s, %s order (relative)" % ("convergence exit" if early_exit else "fixed", order), worst)


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_caches_do_not_see_through_a_round_boundary(early_exit, e2e_runs):
    """sequential order: the linearisation cache, the first-pass skip and the saturated-retry skip against the full passes, bit for bit"""
    prob, x0, ui = ac.end_to_end()

    def full(s):
        s.set_relinearize_unchanged(True); s.set_repeat_first_pass(True); s.set_dedup_saturated_retry(False)

    with env(**SEQ):
        other = _al_solve(3, prob, x0, ui, early_exit, setup=full)
    _same(e2e_runs[early_exit, "seq"], other)
    _same(e2e_runs[early_exit, "seq"], e2e_runs[early_exit, "default"])      # and the launch order changes nothing


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_batch_invariance_against_three_single_rollout_handles(early_exit, e2e_runs):
    prob, x0, ui = ac.end_to_end()
    obs, ex = e2e_runs[early_exit, "default"]
    for b in range(3):
        o1, e1 = _al_solve(1, ac.problem_of(prob, b), x0[b:b + 1], ui[b:b + 1], early_exit)
        for k in lc.NAMES:
            assert np.array_equal(obs[k][b], o1[k][0], equal_nan=True), (b, k)
        for k in ex:
            a = ex[k][:, b] if k == "al_trace" else ex[k][b]
            c = e1[k][:, 0] if k == "al_trace" else e1[k][0]
            assert np.array_equal(a, c, equal_nan=True), (b, k, a, c)
    if early_exit:      # the host stops enqueuing rounds once every rollout is done: with the gate off all rounds are enqueued, same results
        _same(e2e_runs[True, "default"], _al_solve(3, prob, x0, ui, True, gate=False))
        assert np.isnan(ex["al_trace"][2]).all()


def test_batch_slices_and_forward_difference_jacobians(e2e_runs):
    """Both only change the dynamics side.  ILQR_SLICES=2 on B = 128 (two slices of 64: no compacted lists, the store offset per slice), the
    three rollouts tiled: every rollout repeats the B = 3 run of its own inputs.  Forward differences: the solve runs and enforces the limits."""
    prob, x0, ui = ac.end_to_end()
    B = 128
    idx = np.arange(B) % 3
    worst = {}
    pb = dict(prob)
    for k in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        pb[k] = np.ascontiguousarray(prob[k][idx])
    for early_exit in (False, True):
        with env(ILQR_SLICES="2"):
            s = _solver(B, N=prob["N"])
            assert s.L.ilqr_hip_num_slices(s.h) == 2
            s.close()
            obs, ex = _al_solve(B, pb, np.ascontiguousarray(x0[idx]), np.ascontiguousarray(ui[idx]), early_exit)
        o3, e3 = e2e_runs[early_exit, "default"]
        for b in (0, 1, 2, 62, 63, 64, 65, 66, 127):
            # (decisions exactly; values to 1e-9 relative: a slice runs without compacted lists, on other launch shapes)
            for k in ("trace_alpha", "trace_lambda", "iterations"):
                assert np.array_equal(obs[k][b], o3[k][b % 3], equal_nan=True), (early_exit, b, k)
            pairs = [(obs[k][b], o3[k][b % 3]) for k in ("trace_cost", "xbar", "ubar", "K")]
            pairs += [(ex[k][:, b] if k == "al_trace" else ex[k][b], e3[k][:, b % 3] if k == "al_trace" else e3[k][b % 3]) for k in e3]
            for got, want in pairs:
                got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (early_exit, b)
                err = np.nanmax(np.abs(got - want), initial=0.0) / max(1.0, np.nanmax(np.abs(want), initial=0.0))
                worst["slices"] = max(worst.get("slices", 0.0), err)
                assert err <= 1e-9, (early_exit, b, err)
    al = ac.AL_E2E
    s = _solver(3, N=prob["N"]); s.set_problem(prob); s.set_max_iterations(ac.MAX_ITER)
    s.set_options(jacobian_mode=1, fd_eps=1e-5, early_exit=True)
    s.set_augmented_lagrangian(**al)
    s.initialize(x0, ui); cost = s.solve(x0)
    viol, done = s.al_violation(); mj, _ = s.al_multipliers()
    s.close()
    assert np.all(np.isfinite(cost)) and done.all() and np.all(viol[:, 0] <= al["tol_joint"]) and np.all(viol[:, 1] <= al["tol_ctrl"]), (viol, done)
    assert not mj[0].any() and mj[2].max() > 0.0
    _report("ILQR_SLICES=2, B = 128 against the B = 3 run (relative to max(1, |want|))", worst)


def test_warm_start_shifts_the_multipliers():
    prob, x0, ui = ac.end_to_end()
    N = prob["N"]
    rng = np.random.default_rng(9)
    for shift in (1, 3):
        s = _solver(3, N=N); s.set_problem(prob); s.set_max_iterations(ac.MAX_ITER); s.set_augmented_lagrangian(**ac.AL_E2E)
        s.initialize(x0, ui); s.solve(x0)
        mj, mc = s.al_multipliers()
        assert mj.max() > 0.0 and not np.array_equal(s.al_penalties(), np.tile([1e5, 1e3], (3, 1)))
        # (the solve leaves few multipliers: fill the store so that every slot of the shift is checked)
        mj = mj + rng.uniform(1.0, 2.0, mj.shape); mc = mc + rng.uniform(1.0, 2.0, mc.shape); mj[:, 0] = 0.0
        s.set_al_multipliers(mj, mc, None)
        s.initialize_warm_resident(x0, shift=shift)
        gj, gc = s.al_multipliers()
        wj, wc_ = ar.shift(mj, mc, shift)
        assert np.array_equal(gj, wj) and np.array_equal(gc, wc_) and wj[:, 1:N - shift + 1].all() and not wj[:, N - shift + 1:].any()
        assert np.array_equal(s.al_penalties(), np.tile([1e5, 1e3], (3, 1)))
        s.initialize(x0, ui)                                                  # a cold start zeros them
        gj, gc = s.al_multipliers()
        assert not gj.any() and not gc.any()
        s.close()


def test_closed_loop_runner_carries_the_multipliers():
    """MPCRunner on a solver with AL set: the resident plant and the host path end up in the warm initialisers that shift the multipliers;
    both paths agree as in test_closed_loop_runner_carries_the_sets, and the limited rollout still holds multipliers after step 2."""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    from mpc_ilqr_mujoco_amd import solver as sv
    prob3, x03, ui3 = ac.end_to_end()
    B, steps, N = 2, 3, prob3["N"]
    base = sc.make_problem(sv.reference_kinematics, N=N)
    for k in ("Q", "R", "Qf"):
        base[k] = np.array(prob3[k])
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    xr = np.tile(sc.standing_state(), (40, 1)); xr[:, 7 + 14] = ar.ranges()[0][14, 1] + 1.0      # the elbow's posture past its range, for both rollouts
    rd.set_states(xr); rd.contact = np.ones((40, 2), dtype=np.int32)
    x0 = np.array(x03[[0, 2]]); ui = np.array(ui3[[0, 2]])
    x0[0, 7 + 14] = 0.5                                                       # rollout 0 starts far from the limit
    runs = {}
    for resident in (True, False):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(ac.MAX_ITER); s.set_augmented_lagrangian(**ac.AL_E2E)
        r = ml.MPCRunner(s, rd, base, resident=resident)
        xs, us = r.run(x0, steps, u_init=ui)
        mj, mc = s.al_multipliers()
        assert s.augmented_lagrangian_rounds() == 3
        s.close()
        assert np.all(np.isfinite(xs)) and mj[1].max() > 0.0, (resident, mj[1].max())
        runs[resident] = (xs, us, mj, mc)
    ex, eu = np.abs(runs[True][0] - runs[False][0]).max(), np.abs(runs[True][1] - runs[False][1]).max()
    _report("closed loop, resident against host path (absolute)", {"x": ex, "u": eu})
    assert ex <= 1e-9 and eu <= 1e-8, (ex, eu)


def test_refusals_and_clear():
    from mpc_ilqr_mujoco_amd import solver as sv
    import weight_set_cases as wc
    prob, x0, ui = ac.end_to_end()
    N = prob["N"]
    s = _solver(3, N=N); s.set_problem(prob); s.set_max_iterations(ac.MAX_ITER)
    ok = dict(ac.AL_E2E)
    for bad in (dict(rounds=0), dict(rho_joint0=0.0), dict(rho_ctrl0=-1.0), dict(growth=0.5), dict(rho_max_factor=0.9), dict(margin=0.5), dict(margin=-0.1),
                dict(tol_joint=-1e-3), dict(tol_ctrl=float("nan"))):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_augmented_lagrangian(**dict(ok, **bad))
        assert s.augmented_lagrangian_rounds() == 0
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.al_multipliers()
    # AL <-> weight sets, whichever comes second
    sets = wc.one_set_arrays(wc.problem_of_set(wc.weight_set_problem(3, N, 3), 0))
    s.set_augmented_lagrangian(**ok)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        s.set_weight_sets(*sets)
    assert s.num_weight_sets() == 0
    s.clear_augmented_lagrangian()
    s.set_weight_sets(*sets)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        s.set_augmented_lagrangian(**ok)
    assert s.augmented_lagrangian_rounds() == 0
    s.clear_weight_sets()
    # after a solve under AL and clear: bit-identical to a fresh handle
    s.set_problem(prob)
    s.set_augmented_lagrangian(**ok); s.initialize(x0, ui); s.solve(x0)
    s.clear_augmented_lagrangian()
    s.set_regularization(1e-6)                                                # (lambda outlives a solve)
    s.initialize(x0, ui); a = lc.observables(s, s.solve(x0))[0]
    s.close()
    f = _solver(3, N=N); f.set_problem(prob); f.set_max_iterations(ac.MAX_ITER)
    f.initialize(x0, ui); b = lc.observables(f, f.solve(x0))[0]
    f.close()
    lc.assert_same(a, b)
    # a family of the test library that evaluates the cost inside its own rollout / line-search kernels
    with env(ILQR_DYN="s"):
        t = _solver(3, N=N, legacy=True); t.set_problem(prob)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            t.set_augmented_lagrangian(**ok)
    t.set_augmented_lagrangian(**ok)                                          # (ILQR_ENV_PER_CALL: the default family again)
    t.initialize(x0, ui)
    with env(ILQR_DYN="s"):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            t.solve(x0)
    t.solve(x0)
    t.close()
