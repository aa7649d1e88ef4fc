"""The state family of the augmented-Lagrangian limits on the GPU (ilqr_hip_set_al_state_bounds: the state instantiation of
k_cost_quadratics, k_al_state_knot_cost, the state instantiation of k_al_update, k_al_state_shift) against the CPU restatement
tests/al_state_ref.py on the inputs of tests/al_state_cases.py, which test_al_state_cpu.py shows to discriminate.

Tolerances are those of test_gpu_augmented_lagrangian.py for the same quantities: 1e-10 max(1, |want|) on the quadratics and 1e-11
relative on the total cost against oracle + restatement, 1e-5 on the cost trace, exact step sizes, 1e-12 on lambda, 1e-5 relative on
multipliers and violations.  Every test prints the worst error it saw."""
import numpy as np
import pytest

import al_bounds_ref as br
import al_cases as ac
import al_state_cases as sc_
import al_state_ref as sr
import oracle_lib as ol
import test_gpu_linearization_cache as lc
from test_gpu_configs import _solver, env

pytestmark = pytest.mark.gpu
NAMES = ("lx", "lu", "lxx", "luu")
SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")
AL = sc_.AL_E2E
STATE_KEYS = ("mu_s", "rho_s", "viol_s", "state_trace", "srec")


def _report(title, worst):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _stage(s):
    s.stage_cost_quadratics()
    return dict(zip(NAMES, s.quadratics())), s.stage_total_cost()


def _install_state(s, srec, al=AL):
    s.set_al_state_bounds(srec, al["rho_state0"], al["tol_state"])


@pytest.fixture(scope="module")
def oracle_stage():
    """the oracle at ZERO constraint weights on regimes(): [(quadratics, cost) per rollout]; computed once"""
    prob = dict(sc_.stage_problem()); prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob)
    X, U = sc_.regimes()[:2]
    rows = []
    for b in range(X.shape[0]):
        o.set_trajectory(X[b], U[b]); o.cost_quadratics()
        rows.append(({n: o.get(n) for n in NAMES}, o.total_cost()))
    return rows


@pytest.mark.parametrize("table", [False, True], ids=["model_bounds", "bounds_table"])
def test_stage_parity_every_coordinate_and_side_in_three_regimes(table, oracle_stage):
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, inf = sc_.regimes()
    B, N = X.shape[0], sc_.N_STAGE
    assert B == 168
    s = _solver(B, N=N); s.set_problem(sc_.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=sc_.STAGE_MARGIN)
    if table:
        s.set_al_bounds(rec)
    s.set_al_state_bounds(srec, 1.0, 1e-3)
    assert s.num_al_state_bound_sets() == B and s.num_al_bound_sets() == (B if table else 0)
    s.set_al_multipliers(mu_j, mu_c, rho[:, :2]); s.set_al_state_multipliers(mu_s, rho[:, 2])
    assert np.array_equal(s.al_state_multipliers(), mu_s) and np.array_equal(s.al_state_penalties(), rho[:, 2]) and np.array_equal(s.al_state_bounds(), srec)
    gj, gc = s.al_multipliers()
    assert np.array_equal(gj, mu_j) and np.array_equal(gc, mu_c) and np.array_equal(s.al_penalties(), rho[:, :2])
    got, cost = _stage(s)
    s.close()
    worst = {}
    for b in range(B):
        want, c0 = oracle_stage[b]
        w, c = sc_.stage_expected(want, c0, b, table)
        for n in NAMES:
            err = np.abs(got[n][b] - w[n]).max() / max(1.0, np.abs(w[n]).max())
            worst[n] = max(worst.get(n, 0.0), err)
            assert err <= 1e-10, (n, b, cases[b], err)
        worst["cost"] = max(worst.get("cost", 0.0), abs(cost[b] - c) / max(1.0, abs(c)))
        assert abs(cost[b] - c) <= 1e-11 * max(1.0, abs(c)), (b, cases[b], cost[b], c)
        k, side, t, g = cases[b]
        if g == 0 or (g == 1 and t > 0):                               # the active entry sits at its slot, with the sign of its side
            slot = int(sr.SLOTS[k])
            v = got["lx"][b, t, slot] - want["lx"][t, slot]
            assert (v > 0) == bool(side) and abs(v) > 0.1, (b, cases[b], v)
    _report("stage parity, %s, relative to max(1, |want|)" % ("bounds table" if table else "model bounds"), worst)


def test_a_table_of_infinite_bounds_is_no_table():
    """Quadratics and costs with every state bound infinite against the same handle without the table, to 1e-13 relative; a three-iteration
    solve takes the same step sizes and iteration counts."""
    X, U, mu_j, mu_c, _, rho, _, rec, _, _ = sc_.regimes()
    B = X.shape[0]
    s = _solver(B, N=sc_.N_STAGE); s.set_problem(sc_.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=sc_.STAGE_MARGIN)
    s.set_al_multipliers(mu_j, mu_c, rho[:, :2])
    assert np.isinf(s.al_state_bounds()).all() and s.num_al_state_bound_sets() == 0
    plain, cost0 = _stage(s)
    s.set_al_state_bounds(sr.NO_BOUNDS, 5.0, 1e-3)
    assert s.num_al_state_bound_sets() == 1
    inf1, cost1 = _stage(s)
    s.set_al_bounds(rec[:1])
    s.clear_al_state_bounds()
    tab, cost2 = _stage(s)
    s.set_al_state_bounds(np.tile(sr.NO_BOUNDS, (B, 1)), 5.0, 1e-3)
    inf2, cost3 = _stage(s)
    s.close()
    worst = {}
    for name, (a, ca), (b_, cb) in (("model bounds", (plain, cost0), (inf1, cost1)), ("bounds table", (tab, cost2), (inf2, cost3))):
        for n in NAMES:
            scale = np.maximum(1.0, np.abs(a[n]).reshape(B, -1).max(axis=1)).reshape((B,) + (1,) * (a[n].ndim - 1))
            e = (np.abs(b_[n] - a[n]) / scale).max(); worst[name + " " + n] = e
            assert e <= 1e-13, (name, n, e)
        e = (np.abs(cb - ca) / np.maximum(1.0, np.abs(ca))).max(); worst[name + " cost"] = e
        assert e <= 1e-13, (name, e)
    prob, x0, ui = ac.end_to_end()
    out = []
    for use in (False, True):
        s = _solver(3, N=prob["N"]); s.set_problem(prob); s.set_max_iterations(3)
        s.set_augmented_lagrangian(**dict(ac.AL_E2E, rounds=1))
        if use:
            s.set_al_state_bounds(sr.NO_BOUNDS, 1e3, 1e-3)
        s.initialize(x0, ui); cost = s.solve(x0)
        out.append((cost, s.trace(), s.iterations(), s.al_state_violation(), s.al_state_multipliers()))
        s.close()
    (c0, (tc0, ta0, tl0), it0, _, _), (c1, (tc1, ta1, tl1), it1, v1, m1) = out
    assert np.array_equal(ta0, ta1, equal_nan=True) and np.array_equal(it0, it1) and np.array_equal(tl0, tl1, equal_nan=True)
    assert not v1.any() and not m1.any()
    worst["solve cost"] = (np.abs(c1 - c0) / np.abs(c0)).max()
    assert worst["solve cost"] <= 1e-9
    _report("infinite state bounds against no table (relative)", worst)


def test_update_kernel_against_numpy():
    N, B = 4, 8
    jr, cr = ar_ranges()
    rng = np.random.default_rng(6)
    X = np.tile(sc_.sc.standing_state(), (B, N + 1, 1)); X[..., 7:26] += rng.uniform(-0.2, 0.2, (B, N + 1, 19))      # (inside every range)
    X[..., sr.SLOTS] = rng.uniform(-0.5, 0.5, (B, N + 1, 28)) + np.where(sr.SLOTS == 2, 1.0, 0.0)
    U = rng.uniform(-0.7, 0.7, (B, N, 19)) * sc_.sc.CTRLRANGE
    srec = np.tile(np.concatenate([np.full(28, -0.6), np.full(28, 0.7)]), (B, 1)); srec[:, 2] += 1.0; srec[:, 30] += 1.0
    X[0, 2, 32 + 5] = 0.7 + 0.3                                            # the state family alone violates: not done, all three grow
    X[1, 3, 7 + 3] = jr[3, 1] + 0.07                                       # the hinges alone
    U[2, 1, 4] = cr[4, 0] - 3.0                                            # the actuators alone
    X[3, N, 26] = -0.6 - 0.0005                                            # the terminal knot, within tol_state: done
    X[4, 0, 0] = 0.7 + 0.2                                                 # knot 0 alone: done, zero multipliers
    srec[5, 28 + 9] = np.inf; X[5, 2, 32] = 5.0                            # a switched-off side far past where its bound was: done
    X[6, 1, 2] = 1.0 - 0.6 - 0.05                                          # at the cap of rho_state already
    X[7, 4, 50] = -0.6 - 0.01                                              # growth would pass the cap
    mu_j = np.zeros((B, N + 1, 19, 2)); mu_c = np.zeros((B, N, 19, 2)); mu_s = np.zeros((B, N + 1, 28, 2))
    mu_j[:, 1:] = rng.uniform(0.0, 30.0, (B, N, 19, 2)); mu_c[:] = rng.uniform(0.0, 30.0, (B, N, 19, 2)); mu_s[:, 1:] = rng.uniform(0.0, 30.0, (B, N, 28, 2))
    mu_j[4] = 0.0; mu_c[4] = 0.0; mu_s[4] = 0.0
    al = dict(rounds=2, rho_joint0=100.0, rho_ctrl0=2.0, growth=7.0, rho_max_factor=50.0, margin=0.0, tol_joint=1e-3, tol_ctrl=1e-2)
    rho = np.tile([100.0, 2.0, 40.0], (B, 1)) * (1.0 + 0.1 * np.arange(B))[:, None]
    rho[6] = (5000.0, 100.0, 2000.0); rho[7] = (1000.0, 20.0, 400.0)
    rho_max, tol = (5000.0, 100.0, 2000.0), (1e-3, 1e-2, 1e-3)
    s = _solver(B, N=N); s.set_problem(sc_.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(**al)
    s.set_al_state_bounds(srec, 40.0, 1e-3)
    s.set_al_multipliers(mu_j, mu_c, rho[:, :2]); s.set_al_state_multipliers(mu_s, rho[:, 2])
    s.al_update(1)
    gj, gc = s.al_multipliers(); gs = s.al_state_multipliers(); grho = np.concatenate([s.al_penalties(), s.al_state_penalties()[:, None]], axis=1)
    viol, done = s.al_violation(); vs = s.al_state_violation(); tr, st = s.al_trace(), s.al_state_trace()
    s.close()
    assert np.isnan(tr[0]).all() and np.isnan(st[0]).all() and tr.shape == (2, B, 5) and viol.shape == (B, 2) and st.shape == (2, B, 2)
    jrec = br.default_record(0.0)
    worst = {}
    for b in range(B):
        nj, nc, ns, r2, d2, v2 = sr.update(X[b], U[b], mu_j[b], mu_c[b], mu_s[b], tuple(rho[b]), False, jrec, srec[b], al["growth"], rho_max, tol)
        assert bool(done[b]) == d2 and (viol[b, 0], viol[b, 1], vs[b]) == v2, (b, done[b], d2, viol[b], vs[b], v2)
        assert np.array_equal(gs[b] > 0, ns > 0) and np.array_equal(gj[b] > 0, nj > 0) and np.array_equal(gc[b] > 0, nc > 0), b
        for name, g_, w_ in (("mu_joint", gj[b], nj), ("mu_ctrl", gc[b], nc), ("mu_state", gs[b], ns), ("rho", grho[b], np.array(r2))):
            err = (np.abs(g_ - w_) / np.maximum(1e-300, np.abs(w_))).max() if w_.any() else np.abs(g_).max()
            worst[name] = max(worst.get(name, 0.0), err)
            assert err <= 1e-5, (b, name, err)
        assert tuple(st[1, b]) == (v2[2], rho[b, 2]) and tuple(tr[1, b, :2]) == v2[:2] and tuple(tr[1, b, 2:4]) == tuple(rho[b, :2]), (b, st[1, b], tr[1, b])
        assert not gs[b, 0].any()
    assert list(done) == [0, 0, 0, 1, 1, 1, 0, 0]
    assert not gs[4].any() and not gs[5, :, 9, 1].any() and vs[5] == 0.0 and vs[4] == 0.0 and abs(vs[0] - 0.3) < 1e-12
    assert tuple(grho[6]) == rho_max and tuple(grho[7]) == rho_max and abs(grho[0, 2] - 280.0) < 1e-9 and abs(grho[1, 2] - 44.0 * 7) < 1e-9
    assert tuple(grho[3]) == tuple(rho[3])
    _report("update kernel against NumPy (relative)", worst)


def ar_ranges():
    import al_ref as ar
    return ar.ranges()


def test_warm_start_shifts_the_state_multipliers():
    prob, x0, ui, srec, _ = sc_.end_to_end()
    N = prob["N"]
    rng = np.random.default_rng(10)
    for path, shift in (("resident", 1), ("resident", 3), ("host", 1)):
        s = _solver(3, N=N); s.set_problem(prob); s.set_max_iterations(sc_.MAX_ITER); s.set_augmented_lagrangian(**sc_.al_args())
        _install_state(s, srec)
        s.initialize(x0, ui); s.solve(x0)
        assert s.al_state_multipliers().max() > 0.0 and not np.array_equal(s.al_state_penalties(), np.full(3, AL["rho_state0"]))
        ms = rng.uniform(1.0, 2.0, (3, N + 1, 28, 2)); ms[:, 0] = 0.0      # (fill the store so that every slot of the shift is checked)
        mj, mc = s.al_multipliers()
        s.set_al_state_multipliers(ms, None)
        assert np.array_equal(s.al_state_multipliers(), ms)
        if path == "resident":
            s.initialize_warm_resident(x0, shift=shift)
        else:
            s.initialize(x0, None, s.xbar(), s.ubar())
        want = sr.shift(ms, shift)
        got = s.al_state_multipliers()
        assert np.array_equal(got, want) and want[:, 1:N - shift + 1].all() and not got[:, N - shift + 1:].any() and not got[:, 0].any(), (path, shift)
        assert np.array_equal(s.al_state_penalties(), np.full(3, AL["rho_state0"])) and not s.al_state_violation().any()
        wj, wc_ = ac.ar.shift(mj, mc, shift)
        gj, gc = s.al_multipliers()
        assert np.array_equal(gj, wj) and np.array_equal(gc, wc_)
        assert s.num_al_state_bound_sets() == 3 and np.array_equal(s.al_state_bounds(), srec)
        s.initialize(x0, ui)                                                # a cold start zeros them
        assert not s.al_state_multipliers().any() and s.num_al_state_bound_sets() == 3
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
def _al_solve(B, prob, x0, ui, srec, early_exit, setup=None, gate=True, rec=None):
    """(observables, AL observables) of one AL solve with the state table on a fresh handle; srec None: no state table"""
    s = _solver(B, N=prob["N"])
    s.set_problem(prob)
    s.set_options(jacobian_mode=0, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(sc_.MAX_ITER)
    s.set_early_exit_gate(gate)
    if setup:
        setup(s)
    s.set_augmented_lagrangian(**sc_.al_args())
    if rec is not None:
        s.set_al_bounds(rec)
    if srec is not None:
        _install_state(s, srec)
    s.initialize(x0, ui); cost = s.solve(x0)
    obs, counters = lc.observables(s, cost)
    mj, mc = s.al_multipliers(); viol, done = s.al_violation()
    extra = dict(mu_j=mj, mu_c=mc, rho=s.al_penalties(), viol=viol, done=done, al_trace=s.al_trace(), mu_s=s.al_state_multipliers(), rho_s=s.al_state_penalties(),
                 viol_s=s.al_state_violation(), state_trace=s.al_state_trace(), srec=s.al_state_bounds())
    s.close()
    assert counters["adopt"] == 0
    return obs, extra


def _same(a, b):
    lc.assert_same(a[0], b[0])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k


@pytest.fixture(scope="module")
def e2e_runs():
    """the end-to-end case in both modes, solved once in the default order: {early_exit: (observables, AL observables)}"""
    prob, x0, ui, srec, _ = sc_.end_to_end()
    return {early_exit: _al_solve(3, prob, x0, ui, srec, early_exit) for early_exit in (False, True)}


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_end_to_end_against_the_reference_driver(early_exit, e2e_runs):
    obs, ex = e2e_runs[early_exit]
    sol = sc_.reference_solves(early_exit)
    prob, x0, ui, srec, info = sc_.end_to_end()
    tols = (AL["tol_joint"], AL["tol_ctrl"], AL["tol_state"])
    worst = {}
    for b in range(3):
        ref = sol[b]
        want_tr = np.concatenate([ref["al_trace"][:, :2], ref["state_trace"][:, :1]], axis=1)
        got_tr = np.concatenate([ex["al_trace"][:, b, :2], ex["state_trace"][:, b, :1]], axis=1)
        ran = ~np.isnan(want_tr[:, 0])
        assert np.array_equal(~np.isnan(ex["al_trace"][:, b, 0]), ran) and np.array_equal(~np.isnan(ex["state_trace"][:, b, 0]), ran), (b, ex["al_trace"][:, b], want_tr)
        assert np.array_equal(ex["al_trace"][ran, b, 2:], ref["al_trace"][ran, 2:]) and np.array_equal(ex["state_trace"][ran, b, 1], ref["state_trace"][ran, 1]), (b, ex["al_trace"][:, b])
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
        assert bool(ex["done"][b]) == ref["done"] and tuple(ex["rho"][b]) == tuple(ref["rho"]) and ex["rho_s"][b] == ref["rho_s"]
        for name, g_, w_ in (("mu_joint", ex["mu_j"][b], ref["mu_j"]), ("mu_ctrl", ex["mu_c"][b], ref["mu_c"]), ("mu_state", ex["mu_s"][b], ref["mu_s"])):
            e = np.abs(g_ - w_).max() / max(1.0, np.abs(w_).max()); worst[name] = max(worst.get(name, 0.0), e)
            assert e <= 1e-5, (b, name, e)
        assert ex["viol"][b, 0] <= AL["tol_joint"] and ex["viol"][b, 1] <= AL["tol_ctrl"] and ex["viol_s"][b] <= AL["tol_state"] and ex["done"][b]
    assert ex["mu_s"][0].max() > 0.0 and ex["mu_s"][1, :, 2, 0].max() > 0.0 and not ex["mu_s"][2].any()
    # the bounds bind: the joint speed and the pelvis height of the solution against the unconstrained ones
    j = info["joint"]
    assert np.abs(obs["xbar"][0, 1:, 32 + j]).max() <= 0.5 * info["peak"] + AL["tol_state"] and obs["xbar"][1, 1:, 2].min() >= info["z_min"] + sc_.PELVIS_LIFT - AL["tol_state"]
    if early_exit:
        assert len({int((~np.isnan(ex["al_trace"][:, b, 0])).sum()) for b in range(3)}) >= 2
    _report("end to end, %s (relative)" % ("convergence exit" if early_exit else "fixed"), worst)


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_rollout_without_bounds_matches_the_solve_without_a_table(early_exit, e2e_runs):
    prob, x0, ui, srec, _ = sc_.end_to_end()
    obs, ex = e2e_runs[early_exit]
    o0, e0 = _al_solve(3, prob, x0, ui, None, early_exit)
    # (decisions exactly; values to 1e-9 relative: with a state table the batch runs the state instantiation of k_cost_quadratics and takes
    # the model's joint / torque bounds from a record, the same doubles through other machine code)
    for k in ("trace_alpha", "trace_lambda", "iterations"):
        assert np.array_equal(obs[k][2], o0[k][2], equal_nan=True), k
    assert np.array_equal(ex["done"][2], e0["done"][2]) and np.array_equal(ex["rho"][2], e0["rho"][2]) and np.array_equal(ex["al_trace"][:, 2, 2:], e0["al_trace"][:, 2, 2:], equal_nan=True)
    worst = 0.0
    for got, want in [(obs[k][2], o0[k][2]) for k in ("cost", "trace_cost", "xbar", "ubar", "K")] + [(ex[k][2], e0[k][2]) for k in ("mu_j", "mu_c", "viol")] + [(ex["al_trace"][:, 2], e0["al_trace"][:, 2])]:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        worst = max(worst, np.nanmax(np.abs(got - want), initial=0.0) / max(1.0, np.nanmax(np.abs(want), initial=0.0)))
    print("rollout without bounds against the solve without a table (relative to max(1, |want|)): %.2e" % worst)
    assert worst <= 1e-9
    assert np.isnan(e0["state_trace"]).all() and not e0["mu_s"].any() and np.isinf(e0["srec"]).all()
    assert not np.array_equal(obs["xbar"][0], o0["xbar"][0]) and not np.array_equal(obs["xbar"][1], o0["xbar"][1])


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_orders_and_caches_match_the_default_bit_for_bit(early_exit, e2e_runs):
    prob, x0, ui, srec, _ = sc_.end_to_end()
    base = e2e_runs[early_exit]
    for var in (dict(ILQR_RELIN="1"), dict(ILQR_REPASS="1"), dict(ILQR_DEDUP_RETRY="0"), SEQ):
        with env(**var):
            _same(base, _al_solve(3, prob, x0, ui, srec, early_exit))
    if early_exit:      # the host stops enqueuing rounds once every rollout is done: with the gate off all rounds are enqueued, same results
        _same(base, _al_solve(3, prob, x0, ui, srec, True, gate=False))


def test_per_rollout_records_permute_and_broadcast_bit_for_bit():
    """B = 70, wider than one wave of k_solve_begin_al and of the knot-cost kernels: the three rollouts tiled, 70 records; permuting the
    records with the rollouts permutes the results; a one-record table equals B copies."""
    prob3, x03, ui3, srec3, _ = sc_.end_to_end()
    B = 70
    idx = np.arange(B) % 3
    perm = np.random.default_rng(3).permutation(B)

    def batch(sel):
        pb = dict(prob3)
        for k in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
            pb[k] = np.ascontiguousarray(prob3[k][sel])
        return pb, np.ascontiguousarray(x03[sel]), np.ascontiguousarray(ui3[sel])

    # every record its own: the joint-speed bounds scaled and the height bound lifted per rollout
    srec = srec3[idx].copy()
    for b in range(B):
        if idx[b] == 0:
            srec[b] = np.where(np.isfinite(srec[b]), srec[b] * (1.0 + 0.01 * (b // 3)), srec[b])
        elif idx[b] == 1:
            srec[b, 2] += 0.02 * sc_.PELVIS_LIFT * (b // 3)
    pb, x0, ui = batch(idx)
    a = _al_solve(B, pb, x0, ui, srec, True)
    pb2, x02, ui2 = batch(idx[perm])
    b = _al_solve(B, pb2, x02, ui2, srec[perm], True)
    for k in lc.NAMES:
        assert np.array_equal(a[0][k][perm], b[0][k], equal_nan=True), k
    for k in a[1]:
        ak = a[1][k][:, perm] if k in ("al_trace", "state_trace") else a[1][k][perm]
        assert np.array_equal(ak, b[1][k], equal_nan=True), k
    assert len({tuple(r) for r in a[0]["xbar"][0::3, -1]}) > 1                # the scaled bounds are felt
    one = _al_solve(B, pb, x0, ui, srec3[1:2], True)
    many = _al_solve(B, pb, x0, ui, np.tile(srec3[1], (B, 1)), True)
    _same(one, many)


def test_lifecycle_and_refusals():
    from mpc_ilqr_mujoco_amd import solver as sv
    import weight_set_cases as wc
    prob, x0, ui, srec, _ = sc_.end_to_end()
    N = prob["N"]
    s = _solver(3, N=N); s.set_problem(prob); s.set_max_iterations(sc_.MAX_ITER)
    for call in (lambda: _install_state(s, srec), s.clear_al_state_bounds, s.al_state_bounds, s.al_state_multipliers, s.al_state_penalties, s.al_state_violation,
                 lambda: s.set_al_state_multipliers(np.zeros((3, N + 1, 28, 2)))):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            call()
    assert s.num_al_state_bound_sets() == 0
    s.set_augmented_lagrangian(**sc_.al_args())
    assert np.array_equal(s.al_state_bounds(), np.tile(sr.NO_BOUNDS, (3, 1))) and not s.al_state_multipliers().any() and not s.al_state_violation().any()
    assert np.isnan(s.al_state_trace()).all()
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.set_al_state_multipliers(np.zeros((3, N + 1, 28, 2)))
    _install_state(s, srec)
    nan, up, dn, cross = (srec.copy() for _ in range(4))
    nan[1, 5] = np.nan; up[0, 3] = np.inf; dn[2, 28 + 7] = -np.inf; cross[1, 2] = 2.0; cross[1, 30] = 1.0
    for bad, rho0, tol in ((nan, 1.0, 1e-3), (up, 1.0, 1e-3), (dn, 1.0, 1e-3), (cross, 1.0, 1e-3), (srec[:2], 1.0, 1e-3), (srec, 0.0, 1e-3), (srec, -1.0, 1e-3),
                           (srec, np.inf, 1e-3), (srec, np.nan, 1e-3), (srec, 1.0, -1e-9), (srec, 1.0, np.nan)):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_al_state_bounds(bad, rho0, tol)
        assert s.num_al_state_bound_sets() == 3 and np.array_equal(s.al_state_bounds(), srec) and np.array_equal(s.al_state_penalties(), np.full(3, AL["rho_state0"]))
    assert s.L.ilqr_hip_set_al_state_bounds(s.h, None, 3, sv.C.c_double(1.0), sv.C.c_double(1e-3)) == 1
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        s.set_al_state_multipliers(-np.ones((3, N + 1, 28, 2)))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        s.set_al_state_multipliers(None, np.zeros(3))
    # survives the initialisers, set_al_multipliers, the bounds table coming and going and a repeated install; weight sets stay refused
    s.initialize(x0, ui); s.solve(x0)
    first = s.al_state_multipliers()
    assert first.max() > 0.0
    s.set_al_multipliers(None, None, np.tile([1e5, 1e3], (3, 1)))
    s.set_al_bounds(sv.al_default_bounds(0.0)); s.clear_al_bounds()
    s.initialize_warm_resident(x0, shift=1)
    s.set_augmented_lagrangian(**sc_.al_args())
    assert s.num_al_state_bound_sets() == 3 and np.array_equal(s.al_state_bounds(), srec) and not s.al_state_multipliers().any()
    sets = wc.one_set_arrays(wc.problem_of_set(wc.weight_set_problem(3, N, 3), 0))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        s.set_weight_sets(*sets)
    s.set_regularization(1e-6)                                                # (lambda outlives a solve)
    s.initialize(x0, ui); s.solve(x0)
    assert np.array_equal(s.al_state_multipliers(), first)                    # and the solve is the first one again
    # a one-record table, then cleared with AL: a fresh installation has none
    s.set_al_state_bounds(srec[1], 1.0); assert s.num_al_state_bound_sets() == 1 and np.array_equal(s.al_state_bounds(), np.tile(srec[1], (3, 1)))
    s.clear_augmented_lagrangian()
    assert s.num_al_state_bound_sets() == 0
    s.set_augmented_lagrangian(**sc_.al_args())
    assert s.num_al_state_bound_sets() == 0 and np.isinf(s.al_state_bounds()).all()
    s.close()
    # a family of the test library that evaluates the cost inside its own rollout / line-search kernels
    t = _solver(3, N=N, legacy=True); t.set_problem(prob); t.set_max_iterations(sc_.MAX_ITER)
    t.set_augmented_lagrangian(**sc_.al_args()); _install_state(t, srec)
    t.initialize(x0, ui)
    with env(ILQR_DYN="s"):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            t.solve(x0)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            t.set_augmented_lagrangian(**sc_.al_args())
    t.solve(x0)
    assert t.num_al_state_bound_sets() == 3
    t.close()
