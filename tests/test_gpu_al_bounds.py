"""One table of bounds per rollout for the augmented-Lagrangian limits on the GPU (ilqr_hip_set_al_bounds: the AL_TABLE instantiations of
k_cost_quadratics and k_traj_knot_cost, k_al_update<true>, the table's offset per batch slice) against the CPU restatement
tests/al_bounds_ref.py on the inputs of tests/al_bounds_cases.py, which test_al_bounds_cpu.py shows to discriminate.

Tolerances are those test_gpu_augmented_lagrangian.py takes for the same quantities: 1e-10 max(1, |want|) on the quadratics and 1e-11
relative on the total cost against the oracle, 1e-13 relative for an identity between two of the library's own paths, 1e-14 relative on
the updated multipliers, 1e-5 on the AL and cost traces, exact step sizes and 1e-12 on lambda against the reference driver, 1e-9 relative
between a sliced and an unsliced run, 1e-9 / 1e-8 between the resident and the host path of the runner.  Every test prints the worst
error it saw."""
import numpy as np
import pytest

import al_bounds_cases as bc
import al_bounds_ref as br
import al_cases as ac
import al_ref as ar
import oracle_lib as ol
import test_gpu_linearization_cache as lc
from test_gpu_configs import _solver, env

pytestmark = pytest.mark.gpu
sc = ac.sc
NAMES = ("lx", "lu", "lxx", "luu")
SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")
DIAG = np.arange(7, 26)
REF_KEYS = ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref")


def _report(title, worst):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _stage(s):
    s.stage_cost_quadratics()
    return dict(zip(NAMES, s.quadratics())), s.stage_total_cost()


@pytest.fixture(scope="module")
def oracle_stage():
    """the oracle at ZERO constraint weights on regimes_table(): [(quadratics, cost) per rollout]; computed once"""
    prob = dict(ac.stage_problem()); prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob)
    X, U = bc.regimes_table()[:2]
    rows = []
    for b in range(X.shape[0]):
        o.set_trajectory(X[b], U[b]); o.cost_quadratics()
        rows.append(({n: o.get(n) for n in NAMES}, o.total_cost()))
    return rows


def _check_stage(got, cost, records, oracle_stage, title, regimes_hold):
    X, U, mu_j, mu_c, rho, _, cases, inf = bc.regimes_table()
    worst = {}
    for b in range(X.shape[0]):
        want, c0 = oracle_stage[b]
        ck, gx, hx, gu, hu = br.traj_terms(X[b], U[b], mu_j[b], mu_c[b], rho[b], records[b])
        w = {n: want[n].copy() for n in NAMES}
        w["lx"][:, 7:26] += gx; w["lu"] += gu; w["luu"] += hu; w["lxx"][:, DIAG, DIAG] += hx
        for n in NAMES:
            assert np.all(np.isfinite(got[n][b])), (n, b)
            err = np.abs(got[n][b] - w[n]).max() / max(1.0, np.abs(w[n]).max())
            worst[n] = max(worst.get(n, 0.0), err)
            assert err <= 1e-10, (n, b, cases[b], err)
        c = c0 + ck.sum()
        worst["cost"] = max(worst.get("cost", 0.0), abs(cost[b] - c) / max(1.0, abs(c)))
        assert abs(cost[b] - c) <= 1e-11 * max(1.0, abs(c)), (b, cases[b], cost[b], c)
        if regimes_hold:
            kind, j, side, t, g = cases[b]
            if g == 0:                                                  # the active entry is there, with the sign of its side
                v = got["lx"][b, t, 7 + j] - want["lx"][t, 7 + j] if kind == "joint" else got["lu"][b, t, j] - want["lu"][t, j]
                assert (v > 0) == bool(side) and abs(v) > 1.0, (b, cases[b], v)
    _report(title, worst)


def test_stage_parity_every_row_and_side_in_three_regimes_under_a_table(oracle_stage):
    X, U, mu_j, mu_c, rho, rec, cases, inf = bc.regimes_table()
    B, N = X.shape[0], ac.N_STAGE
    assert B == 228 and len(inf) == 12 and np.isinf(rec).sum() == 12
    s = _solver(B, N=N); s.set_problem(ac.stage_problem())             # (both plain penalties on: AL must replace them)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    runs = {}
    for m in (0.0, 0.1):                                               # the table overrides the margin of the installation
        s.set_augmented_lagrangian(1, 1.0, 1.0, margin=m)
        if m == 0.0:
            s.set_al_bounds(rec)
        assert s.num_al_bound_sets() == B and np.array_equal(s.al_bounds(), rec)      # (it survives the repeated installation)
        s.set_al_multipliers(mu_j, mu_c, rho)
        runs[m] = _stage(s)
    for n in NAMES:
        assert np.array_equal(runs[0.0][0][n], runs[0.1][0][n]), n
    assert np.array_equal(runs[0.0][1], runs[0.1][1])
    for i, (kind, j, side) in inf.items():                              # the switched-off sides carry multipliers
        mu = mu_j[i, 1:, j, side] if kind == "joint" else mu_c[i, :, j, side]
        assert mu.all()
    _check_stage(*runs[0.0], rec, oracle_stage, "stage parity under a [228][76] table, relative to max(1, |want|)", True)
    # n_sets = 1: every rollout under record 0
    s.set_al_bounds(rec[0])
    assert s.num_al_bound_sets() == 1 and np.array_equal(s.al_bounds(), np.tile(rec[0], (B, 1)))
    got, cost = _stage(s)
    s.close()
    _check_stage(got, cost, np.tile(rec[0], (B, 1)), oracle_stage, "stage parity, every rollout under record 0", False)


def _al_solve(B, prob, x0, ui, early_exit, bounds=None, setup=None, jacobian_mode=0, al=None):
    """(observables, AL observables) of one AL solve on a fresh handle; bounds: the table installed behind the AL installation"""
    s = _solver(B, N=prob["N"])
    s.set_problem(prob)
    s.set_options(jacobian_mode=jacobian_mode, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(ac.MAX_ITER)
    s.set_augmented_lagrangian(**(al or ac.AL_E2E))
    if bounds is not None:
        s.set_al_bounds(bounds)
    if setup:
        setup(s)
    s.initialize(x0, ui); cost = s.solve(x0)
    obs, counters = lc.observables(s, cost)
    mj, mc = s.al_multipliers(); viol, done = s.al_violation()
    extra = dict(mu_j=mj, mu_c=mc, rho=s.al_penalties(), viol=viol, done=done, al_trace=s.al_trace())
    assert s.num_al_bound_sets() == (0 if bounds is None else np.atleast_2d(bounds).shape[0])
    s.close()
    assert counters["adopt"] == 0
    return obs, extra


def _same(a, b):
    lc.assert_same(a[0], b[0])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k


@pytest.mark.parametrize("m", [0.0, 0.1])
def test_a_table_of_the_default_bounds_is_no_table(m):
    X, U, mu_j, mu_c, rho, _ = ac.regimes(m)
    B = X.shape[0]
    s = _solver(B, N=ac.N_STAGE); s.set_problem(ac.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=m)
    s.set_al_multipliers(mu_j, mu_c, rho)
    table = s.al_bounds()
    assert np.array_equal(table, np.tile(br.default_record(m), (B, 1)))
    none, cost0 = _stage(s)
    s.set_al_bounds(table)
    tab, cost1 = _stage(s)
    s.close()
    worst, bitwise = {}, True
    for n in NAMES:
        scale = np.maximum(1.0, np.abs(none[n]).reshape(B, -1).max(axis=1)).reshape((B,) + (1,) * (none[n].ndim - 1))
        worst[n] = (np.abs(tab[n] - none[n]) / scale).max()
        bitwise = bitwise and np.array_equal(tab[n], none[n])
        assert worst[n] <= 1e-13, (n, worst[n])
    worst["cost"] = (np.abs(cost1 - cost0) / np.maximum(1.0, np.abs(cost0))).max()
    bitwise = bitwise and np.array_equal(cost0, cost1)
    assert worst["cost"] <= 1e-13
    # the solve
    prob, x0, ui = ac.end_to_end()
    al = dict(ac.AL_E2E, margin=m)
    (o0, e0), (o1, e1) = (_al_solve(3, prob, x0, ui, False, bounds=b_, al=al) for b_ in (None, np.tile(br.default_record(m), (3, 1))))
    assert np.array_equal(o0["trace_alpha"], o1["trace_alpha"], equal_nan=True) and np.array_equal(o0["iterations"], o1["iterations"])
    assert np.array_equal(o0["trace_lambda"], o1["trace_lambda"], equal_nan=True) and np.array_equal(e0["done"], e1["done"])
    worst["solve cost"] = (np.abs(o1["cost"] - o0["cost"]) / np.abs(o0["cost"])).max()
    assert worst["solve cost"] <= 1e-9
    bit_solve = all(np.array_equal(o0[k], o1[k], equal_nan=True) for k in lc.NAMES) and all(np.array_equal(e0[k], e1[k], equal_nan=True) for k in e0)
    _report("default-bounds table against no table, margin %g (relative; stages bitwise equal: %s, solve bitwise equal: %s)" % (m, bitwise, bit_solve), worst)


def test_update_kernel_against_numpy_under_a_table():
    N, B = 4, 9
    jr, cr = ar.ranges()
    rng = np.random.default_rng(5)
    prob = ac.stage_problem()
    X = np.tile(sc.standing_state(), (B, N + 1, 1)); X[..., 7:26] += rng.uniform(-0.2, 0.2, (B, N + 1, 19))      # (inside every range)
    U = rng.uniform(-0.7, 0.7, (B, N, 19)) * sc.CTRLRANGE
    dflt = br.default_record(0.0)
    rec = np.tile(dflt, (B, 1))
    rec[:, 0:19] -= rng.uniform(0.0, 0.05, (B, 19)); rec[:, 19:38] += rng.uniform(0.0, 0.05, (B, 19))      # every record its own: a little wider hinges ...
    rec[:, 38:57] *= rng.uniform(0.8, 1.0, (B, 19)); rec[:, 57:76] *= rng.uniform(0.8, 1.0, (B, 19))          # ... and narrower torques (|U| <= 0.7 range stays inside)
    X[0, 2, 7 + 3] = rec[0, 19 + 3] + 0.07; U[0, 1, 4] = rec[0, 38 + 4] - 3.0   # both families violate
    X[1, 0, 7 + 0] = rec[1, 19 + 0] + 0.2                                       # knot 0 alone: done, zero multipliers
    X[2, N, 7 + 9] = rec[2, 0 + 9] - 0.01                                       # the terminal knot; at the rho cap
    U[3, N - 1, 18] = rec[3, 57 + 18] + 0.004                                   # within tol_ctrl: done
    X[4, 1, 7 + 14] = rec[4, 19 + 14] + 0.0005                                  # within tol_joint: done
    X[5, 3, 7 + 2] = rec[5, 19 + 2] + 0.3                                       # not done: its penalties grow, up to the cap
    rec[6, 19 + 5] = jr[5, 1] + 0.1; X[6, 2, 7 + 5] = jr[5, 1] + 0.05           # past the model's range, inside its own wider record: done only because of it
    rec[7, 57 + 7] = cr[7, 1] * 0.5; U[7, 2, 7] = cr[7, 1] * 0.6                # inside the model's range, past its own narrower record: not done only because of it
    rec[8, 19 + 11] = np.inf; rec[8, 38 + 2] = -np.inf                          # two sides switched off: whatever the value, no violation, multipliers to zero
    X[8, 1:, 7 + 11] = jr[11, 1] + 1.0; U[8, :, 2] = cr[2, 0] * 3.0
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
    s.set_al_bounds(rec)
    s.set_al_multipliers(mu_j, mu_c, rho)
    s.al_update(1)
    gj, gc = s.al_multipliers(); grho = s.al_penalties(); viol, done = s.al_violation(); tr = s.al_trace()
    s.close()
    assert np.isnan(tr[0]).all() and np.all(np.isfinite(gj)) and np.all(np.isfinite(gc)) and np.all(np.isfinite(viol))
    worst = {}
    rest = (al["growth"], (5000.0, 100.0), (1e-3, 1e-2))
    for b in range(B):
        nj, nc, r2, d2, v2 = br.update(X[b], U[b], mu_j[b], mu_c[b], tuple(rho[b]), False, rec[b], *rest)
        assert bool(done[b]) == d2 and tuple(viol[b]) == v2, (b, done[b], d2, viol[b], v2)
        assert np.array_equal(gj[b] > 0, nj > 0) and np.array_equal(gc[b] > 0, nc > 0), b
        for name, g_, w_ in (("mu_joint", gj[b], nj), ("mu_ctrl", gc[b], nc), ("rho", grho[b], np.array(r2))):
            err = (np.abs(g_ - w_) / np.maximum(1e-300, np.abs(w_))).max() if w_.any() else np.abs(g_).max()
            worst[name] = max(worst.get(name, 0.0), err)
            assert err <= 1e-14, (b, name, err)
        assert tuple(tr[1, b, :2]) == v2 and tuple(tr[1, b, 2:4]) == tuple(rho[b]) and tr[1, b, 4] == 0.0
    assert list(done) == [0, 1, 0, 1, 1, 0, 1, 0, 1]
    # rollouts 6 and 7 under the default record: the other way round
    assert not br.update(X[6], U[6], mu_j[6], mu_c[6], tuple(rho[6]), False, dflt, *rest)[3]
    assert br.update(X[7], U[7], mu_j[7], mu_c[7], tuple(rho[7]), False, np.r_[rec[7, :38], dflt[38:]], *rest)[3]
    assert not gj[1].any() and not gc[1].any()
    assert not gj[8, :, 11, 1].any() and not gc[8, :, 2, 0].any() and mu_j[8, 1:, 11, 1].all() and mu_c[8, :, 2, 0].all()
    assert tuple(grho[2]) == (5000.0, 100.0) and tuple(grho[5]) == (5000.0, 100.0) and abs(grho[0, 0] - 700.0) < 1e-9
    _report("update kernel under a table against NumPy (relative)", worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e_runs():
    """the B = 4 case in both modes and both launch orders, solved once: {(early_exit, order): (observables, AL observables)}; and
    {(early_exit, "twin")}: al_cases.end_to_end() under the default bounds, whose rollout 2 is rollout 3's problem without its record"""
    prob, x0, ui, rec = bc.end_to_end()
    out = {}
    for early_exit in (False, True):
        out[early_exit, "default"] = _al_solve(4, prob, x0, ui, early_exit, bounds=rec)
        with env(**SEQ):
            out[early_exit, "seq"] = _al_solve(4, prob, x0, ui, early_exit, bounds=rec)
        out[early_exit, "twin"] = _al_solve(3, *ac.end_to_end(), early_exit)
    return out


@pytest.mark.parametrize("order", ["default", "seq"])
@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_end_to_end_against_the_reference_driver(early_exit, order, e2e_runs):
    obs, ex = e2e_runs[early_exit, order]
    sol = bc.reference_solves(early_exit)
    al = ac.AL_E2E
    worst = {}
    for b in range(4):
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
        for name, g_, w_ in (("x", obs["xbar"][b], ref["X"]), ("u", obs["ubar"][b], ref["U"])):
            e = np.abs(g_ - w_).max() / max(1.0, np.abs(w_).max()); worst[name] = max(worst.get(name, 0.0), e)
            assert e <= 1e-5, (b, name, e)
    assert list(ex["done"]) == [1, 1, 0, 1]
    assert not ex["mu_j"][0].any() and not ex["mu_c"][0].any() and ex["mu_j"][3].max() > 0.0 and ex["mu_c"][2].max() > 0.0
    # the effects, on the GPU's results
    twin = e2e_runs[early_exit, "twin"][0]["xbar"][2]
    got = [dict(X=obs["xbar"][b], U=obs["ubar"][b], viol=tuple(ex["viol"][b]), done=bool(ex["done"][b])) for b in range(4)]
    figures = bc.effect_assertions(got, twin)
    _report("end to end under a table, %s, %s order (relative)" % ("convergence exit" if early_exit else "fixed", order), worst)
    print("  " + ", ".join("%s %.6g" % kv for kv in figures.items()))


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_batch_invariance(early_exit, e2e_runs):
    """the B = 4 handle against four B = 1 handles, each with n_sets = 1 and its own record; a [4][76] table of four equal rows against the
    n_sets = 1 table of that row: bit for bit"""
    prob, x0, ui, rec = bc.end_to_end()
    obs, ex = e2e_runs[early_exit, "default"]
    for b in range(4):
        o1, e1 = _al_solve(1, bc.problem_of(prob, b), x0[b:b + 1], ui[b:b + 1], early_exit, bounds=rec[b])
        for k in lc.NAMES:
            assert np.array_equal(obs[k][b], o1[k][0], equal_nan=True), (b, k)
        for k in ex:
            a = ex[k][:, b] if k == "al_trace" else ex[k][b]
            c = e1[k][:, 0] if k == "al_trace" else e1[k][0]
            assert np.array_equal(a, c, equal_nan=True), (b, k, a, c)
    if early_exit:
        _same(_al_solve(4, prob, x0, ui, True, bounds=np.tile(rec[3], (4, 1))), _al_solve(4, prob, x0, ui, True, bounds=rec[3]))


def test_batch_slices_and_forward_difference_jacobians(e2e_runs):
    """ILQR_SLICES=2: a slice holds at least 64 rollouts, so the B = 4 batch is tiled to B = 128 (two slices of 64) -- in the second slice
    moved on by one, so that rollout 64 + i carries another record than rollout i: a slice that forgot the table's offset b0 * stride
    would solve rollouts 64.. under the records 0...  Every rollout repeats the B = 4 run of its own inputs.  Forward differences: the
    same comparison on the B = 4 batch against the reference driver's effects."""
    prob, x0, ui, rec = bc.end_to_end()
    B = 128
    idx = (np.arange(B) + (np.arange(B) >= 64)) % 4
    assert idx[64] != idx[0] and idx[65] != idx[1]
    worst = {}
    pb = dict(prob)
    for k in REF_KEYS:
        pb[k] = np.ascontiguousarray(prob[k][idx])
    for early_exit in (False, True):
        with env(ILQR_SLICES="2"):
            s = _solver(B, N=prob["N"])
            assert s.L.ilqr_hip_num_slices(s.h) == 2
            s.close()
            obs, ex = _al_solve(B, pb, np.ascontiguousarray(x0[idx]), np.ascontiguousarray(ui[idx]), early_exit, bounds=np.ascontiguousarray(rec[idx]))
        o4, e4 = e2e_runs[early_exit, "default"]
        for b in (0, 1, 2, 3, 62, 63, 64, 65, 66, 67, 127):
            w = idx[b]
            for k in ("trace_alpha", "trace_lambda", "iterations"):      # decisions exactly
                assert np.array_equal(obs[k][b], o4[k][w], equal_nan=True), (early_exit, b, k)
            assert ex["done"][b] == e4["done"][w]
            pairs = [(obs[k][b], o4[k][w]) for k in ("trace_cost", "xbar", "ubar", "K")]
            pairs += [(ex[k][:, b] if k == "al_trace" else ex[k][b], e4[k][:, w] if k == "al_trace" else e4[k][w]) for k in e4]
            for got, want in pairs:
                got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (early_exit, b)
                err = np.nanmax(np.abs(got - want), initial=0.0) / max(1.0, np.nanmax(np.abs(want), initial=0.0))
                worst["slices"] = max(worst.get("slices", 0.0), err)
                assert err <= 1e-9, (early_exit, b, err)
    # forward-difference Jacobians change the dynamics side only: the table's effects are there
    obs, ex = _al_solve(4, prob, x0, ui, True, bounds=rec, jacobian_mode=1)
    twin = _al_solve(3, *ac.end_to_end(), True, jacobian_mode=1)[0]["xbar"][2]
    assert np.all(np.isfinite(obs["cost"]))
    bc.effect_assertions([dict(X=obs["xbar"][b], U=obs["ubar"][b], viol=tuple(ex["viol"][b]), done=bool(ex["done"][b])) for b in range(4)], twin)
    assert not ex["mu_j"][0].any() and ex["mu_j"][3].max() > 0.0
    _report("ILQR_SLICES=2, B = 128 against the B = 4 run (relative to max(1, |want|))", worst)


def test_warm_start_keeps_the_table_and_shifts_the_multipliers():
    prob, x0, ui, rec = bc.end_to_end()
    N = prob["N"]
    rng = np.random.default_rng(9)
    s = _solver(4, N=N); s.set_problem(prob); s.set_max_iterations(ac.MAX_ITER); s.set_augmented_lagrangian(**ac.AL_E2E)
    s.set_al_bounds(rec)
    s.initialize(x0, ui); s.solve(x0)
    mj, mc = s.al_multipliers()
    assert mj[3].max() > 0.0 and mc[2].max() > 0.0
    mj = mj + rng.uniform(1.0, 2.0, mj.shape); mc = mc + rng.uniform(1.0, 2.0, mc.shape); mj[:, 0] = 0.0
    s.set_al_multipliers(mj, mc, None)
    assert np.array_equal(s.al_bounds(), rec)
    s.initialize_warm_resident(x0)
    gj, gc = s.al_multipliers()
    wj, wc_ = ar.shift(mj, mc, 1)
    assert np.array_equal(gj, wj) and np.array_equal(gc, wc_)
    assert s.num_al_bound_sets() == 4 and np.array_equal(s.al_bounds(), rec)
    a = s.solve(x0)                                                       # and the solve behind the warm start still runs under the table
    s.initialize(x0, ui)                                                  # a cold start leaves it too
    assert s.num_al_bound_sets() == 4 and np.array_equal(s.al_bounds(), rec)
    s.close()
    assert np.all(np.isfinite(a))


def test_closed_loop_runner_under_a_two_rollout_table():
    """MPCRunner on a solver with AL and a table set, the setup of test_closed_loop_runner_carries_the_multipliers: resident plant and host
    path agree, the rollout whose elbow bound is lowered by 0.03 rad holds multipliers after step 2, and the table is still there at the end."""
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
    table = sc.stack_al_bounds([dict(), dict(joint_hi={14: ar.ranges()[0][14, 1] - 0.03})], B)
    assert np.array_equal(table[0], br.default_record(0.0)) and table[1, 19 + 14] == ar.ranges()[0][14, 1] - 0.03
    runs = {}
    for resident in (True, False):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(ac.MAX_ITER); s.set_augmented_lagrangian(**ac.AL_E2E)
        s.set_al_bounds(table)
        r = ml.MPCRunner(s, rd, base, resident=resident)
        xs, us = r.run(x0, steps, u_init=ui)
        mj, mc = s.al_multipliers()
        assert s.augmented_lagrangian_rounds() == 3 and s.num_al_bound_sets() == 2 and np.array_equal(s.al_bounds(), table)
        s.close()
        assert np.all(np.isfinite(xs)) and mj[1].max() > 0.0, (resident, mj[1].max())
        runs[resident] = (xs, us, mj, mc)
    ex, eu = np.abs(runs[True][0] - runs[False][0]).max(), np.abs(runs[True][1] - runs[False][1]).max()
    _report("closed loop under a table, resident against host path (absolute)", {"x": ex, "u": eu})
    assert ex <= 1e-9 and eu <= 1e-8, (ex, eu)


def test_life_cycle_and_refusals():
    from mpc_ilqr_mujoco_amd import solver as sv
    import weight_set_cases as wc
    prob, x0, ui, rec = bc.end_to_end()
    N = prob["N"]
    s = _solver(4, N=N); s.set_problem(prob); s.set_max_iterations(ac.MAX_ITER)
    dflt = sv.al_default_bounds(0.0)
    # without AL: ILQR_ERR_STATE from all four handle calls
    for call in (lambda: s.set_al_bounds(rec), s.clear_al_bounds, s.al_bounds):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            call()
    assert s.num_al_bound_sets() == 0
    s.set_augmented_lagrangian(**dict(ac.AL_E2E, margin=0.1))
    assert s.num_al_bound_sets() == 0 and np.array_equal(s.al_bounds(), np.tile(sv.al_default_bounds(0.1), (4, 1)))
    s.set_augmented_lagrangian(**ac.AL_E2E)
    assert np.array_equal(s.al_bounds(), np.tile(dflt, (4, 1)))
    # a set followed by a get round-trips bit for bit; n_sets = 1 is expanded
    odd = rec.copy(); odd[1, 3] = -np.inf; odd[2, 57 + 4] = np.inf; odd[3, 38 + 18] = 0.0; odd[3, 57 + 18] = 0.0; odd[0, 5] = np.nextafter(odd[0, 5], 1.0)
    s.set_al_bounds(odd)
    assert s.num_al_bound_sets() == 4 and np.array_equal(s.al_bounds(), odd)
    s.set_al_bounds(odd[1])
    assert s.num_al_bound_sets() == 1 and np.array_equal(s.al_bounds(), np.tile(odd[1], (4, 1)))
    s.set_al_bounds(odd)
    # every refusal, each leaving the installed table as it was
    def bad(i, v, j=None, w=None):
        b = rec.copy(); b[2, i] = v
        if j is not None:
            b[2, j] = w
        return b
    L = s.L
    for what, arr in (("NaN", bad(7, np.nan)), ("NaN hi", bad(57 + 3, np.nan)), ("lo > hi", bad(4, 1.0, 19 + 4, 0.5)), ("lo > hi ctrl", bad(38 + 2, 5.0, 57 + 2, -5.0)),
                      ("lo = +inf", bad(6, np.inf, 19 + 6, np.inf)), ("hi = -inf", bad(57 + 9, -np.inf, 38 + 9, -np.inf)), ("n_sets 2", rec[:2]), ("n_sets 3", rec[:3])):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_al_bounds(arr)
        assert s.num_al_bound_sets() == 4 and np.array_equal(s.al_bounds(), odd), what
    assert L.ilqr_hip_set_al_bounds(s.h, None, 4) == 1 and L.ilqr_hip_get_al_bounds(s.h, None) == 1 and L.ilqr_hip_set_al_bounds(s.h, sv._p(np.ascontiguousarray(rec)), 0) == 1
    assert np.array_equal(s.al_bounds(), odd)
    with pytest.raises(ValueError):
        s.set_al_bounds(rec[:, :75])
    s.set_al_bounds(bad(38 + 5, 0.0, 57 + 5, 0.0))                            # lo == hi is allowed: a dead motor
    # weight sets are still refused with the table installed
    sets = wc.one_set_arrays(wc.problem_of_set(wc.weight_set_problem(4, N, 4), 0))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        s.set_weight_sets(*sets)
    assert s.num_weight_sets() == 0 and s.num_al_bound_sets() == 4
    # after a solve under the table and clear_al_bounds: bit-identical to a handle that never had a table
    s.set_problem(prob)
    s.set_al_bounds(rec); s.initialize(x0, ui); s.solve(x0)
    s.clear_al_bounds()
    assert s.num_al_bound_sets() == 0 and s.augmented_lagrangian_rounds() == 3 and np.array_equal(s.al_bounds(), np.tile(dflt, (4, 1)))
    s.set_regularization(1e-6)                                                # (lambda outlives a solve)
    s.initialize(x0, ui); a = lc.observables(s, s.solve(x0))[0]
    ea = s.al_multipliers()
    f = _solver(4, N=N); f.set_problem(prob); f.set_max_iterations(ac.MAX_ITER); f.set_augmented_lagrangian(**ac.AL_E2E)
    f.initialize(x0, ui); b = lc.observables(f, f.solve(x0))[0]
    eb = f.al_multipliers()
    f.close()
    lc.assert_same(a, b)
    assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
    # clear_augmented_lagrangian drops the table; a fresh installation starts on the default bounds
    s.set_al_bounds(rec)
    s.clear_augmented_lagrangian()
    assert s.num_al_bound_sets() == 0
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.al_bounds()
    s.set_augmented_lagrangian(**ac.AL_E2E)
    assert s.num_al_bound_sets() == 0 and np.array_equal(s.al_bounds(), np.tile(dflt, (4, 1)))
    s.set_regularization(1e-6)
    s.initialize(x0, ui); c = lc.observables(s, s.solve(x0))[0]
    s.close()
    lc.assert_same(c, b)
