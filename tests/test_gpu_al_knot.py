"""Bounds that change from knot to knot on the GPU (ilqr_hip_set_al_knot_bounds, ilqr_hip_set_al_state_knot_bounds,
ilqr_hip_al_bounds_window_from_track: the per-knot instantiations of k_cost_quadratics, k_traj_knot_cost, k_al_state_knot_cost and k_al_update
in libilqr_hip_alknot.so, the expansion of the other family's record, the track cut) against the CPU restatement tests/al_knot_ref.py on the
inputs of tests/al_knot_cases.py, which test_al_knot_cpu.py shows to discriminate.

Tolerances: those of test_gpu_al_bounds._check_stage on the stages (1e-10 max(1, |want|) on the quadratics, 1e-11 on the cost: the
arithmetic is the table path's), those of test_end_to_end_against_the_reference_driver on the solves, and bit for bit wherever two of the
library's own paths meet the same doubles.  Every test prints the worst error it saw."""
import numpy as np
import pytest

import al_bounds_cases as bc
import al_bounds_ref as br
import al_cases as ac
import al_knot_cases as kc
import al_knot_ref as kr
import al_ref as ar
import al_state_cases as stc
import al_state_ref as sr
import oracle_lib as ol
import test_gpu_linearization_cache as lc
from test_gpu_configs import _solver, env

pytestmark = pytest.mark.gpu
sc = ac.sc
NAMES = ("lx", "lu", "lxx", "luu")
SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")
DIAG = np.arange(7, 26)
REF_KEYS = ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref")
AL = kc.AL_E2E
N4 = ac.N_STAGE


def _report(title, worst):
    print("%s: %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _stage(s):
    s.stage_cost_quadratics()
    return dict(zip(NAMES, s.quadratics())), s.stage_total_cost()


def _oracle_rows(X, U):
    prob = dict(ac.stage_problem()); prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob)
    rows = []
    for b in range(X.shape[0]):
        o.set_trajectory(X[b], U[b]); o.cost_quadratics()
        rows.append(({n: o.get(n) for n in NAMES}, o.total_cost()))
    return rows


@pytest.fixture(scope="module")
def oracle_joint():
    return _oracle_rows(*bc.regimes_table()[:2])


@pytest.fixture(scope="module")
def oracle_state():
    return _oracle_rows(*stc.regimes()[:2])


def _expected(want, c0, X, U, mu_j, mu_c, rho, win, mu_s=None, rho_s=None, swin=None):
    """oracle quadratics and cost of one rollout plus the restatement's terms under its windows"""
    ck, gx, hx, gu, hu = kr.traj_terms(X, U, mu_j, mu_c, rho, win)
    w = {n: want[n].copy() for n in NAMES}
    w["lx"][:, 7:26] += gx; w["lu"] += gu; w["luu"] += hu; w["lxx"][:, DIAG, DIAG] += hx
    c = c0 + ck.sum()
    if swin is not None:
        sk, sg, sh = kr.state_traj_terms(X, mu_s, rho_s, swin)
        sr.add_to_quadratics(w, sg, sh)
        c += sk.sum()
    return w, c


def _compare(got, cost, b, w, c, worst, what):
    for n in NAMES:
        assert np.all(np.isfinite(got[n][b])), (n, b)
        err = np.abs(got[n][b] - w[n]).max() / max(1.0, np.abs(w[n]).max())
        worst[n] = max(worst.get(n, 0.0), err)
        assert err <= 1e-10, (n, b, what, err)
    worst["cost"] = max(worst.get("cost", 0.0), abs(cost[b] - c) / max(1.0, abs(c)))
    assert abs(cost[b] - c) <= 1e-11 * max(1.0, abs(c)), (b, what, cost[b], c)


# ------------------------------------------------------------------------------------------------------------------------ 1. stage parity
def test_stage_parity_of_the_joint_and_torque_family_under_discriminating_windows(oracle_joint):
    X, U, mu_j, mu_c, rho, rec, cases, inf = bc.regimes_table()
    win = kc.joint_windows()
    B = X.shape[0]
    s = _solver(B, N=N4); s.set_problem(ac.stage_problem())             # (both plain penalties on: AL must replace them)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=0.1)                 # (the window overrides the margin)
    s.set_al_knot_bounds(win)
    assert s.al_bounds_per_knot() == 1 and s.num_al_bound_sets() == B and s.num_al_state_bound_sets() == 0
    jc, st = s.al_knot_bounds()
    assert np.array_equal(jc, win) and np.all(np.isinf(st))
    s.set_al_multipliers(mu_j, mu_c, rho)
    got, cost = _stage(s)
    s.close()
    worst = {}
    for b in range(B):
        want, c0 = oracle_joint[b]
        w, c = _expected(want, c0, X[b], U[b], mu_j[b], mu_c[b], rho[b], win[b])
        _compare(got, cost, b, w, c, worst, cases[b])
        kind, j, side, t, g = cases[b]
        if g == 0:                                                      # the active entry is there, with the sign of its side
            v = got["lx"][b, t, 7 + j] - want["lx"][t, 7 + j] if kind == "joint" else got["lu"][b, t, j] - want["lu"][t, j]
            assert (v > 0) == bool(side) and abs(v) > 1.0, (b, cases[b], v)
    _report("stage parity under [228][5][76] windows, relative to max(1, |want|)", worst)


@pytest.mark.parametrize("joint", ["table", "window"])
def test_stage_parity_of_the_state_family_under_discriminating_windows(joint, oracle_state):
    """joint = table: the state window beside a whole-horizon joint / torque table, which the library expands into a window; joint = window:
    both families per knot, every row of the joint / torque window another record"""
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, cases, inf = stc.regimes()
    swin, jwin = kc.state_windows()
    B = X.shape[0]
    if joint == "table":
        jwin = np.repeat(rec[:, None, :], N4 + 1, axis=1)
    s = _solver(B, N=N4); s.set_problem(stc.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=stc.STAGE_MARGIN)
    if joint == "table":
        s.set_al_bounds(rec)
    else:
        s.set_al_knot_bounds(jwin)
    s.set_al_state_knot_bounds(swin, 1.0, 1e-3)
    assert s.al_bounds_per_knot() == (2 if joint == "table" else 3) and s.num_al_state_bound_sets() == B and s.num_al_bound_sets() == B
    gj_, gs_ = s.al_knot_bounds()
    assert np.array_equal(gj_, jwin) and np.array_equal(gs_, swin)
    if joint == "table":
        assert np.array_equal(s.al_bounds(), rec)                       # (the table's own getter still answers)
    s.set_al_multipliers(mu_j, mu_c, rho[:, :2]); s.set_al_state_multipliers(mu_s, rho[:, 2])
    got, cost = _stage(s)
    s.close()
    worst = {}
    for b in range(B):
        want, c0 = oracle_state[b]
        w, c = _expected(want, c0, X[b], U[b], mu_j[b], mu_c[b], rho[b, :2], jwin[b], mu_s[b], rho[b, 2], swin[b])
        _compare(got, cost, b, w, c, worst, cases[b])
        k, side, t, g = cases[b]
        if g == 0 or (g == 1 and t > 0):
            slot = int(sr.SLOTS[k])
            v = got["lx"][b, t, slot] - want["lx"][t, slot]
            assert (v > 0) == bool(side) and abs(v) > 0.1, (b, cases[b], v)
    _report("stage parity of the state family, joint / torque %s, relative to max(1, |want|)" % joint, worst)


# ------------------------------------------------------------------------------------------- 2. constant rows, 3. the torque fields of row N
def _al_solve(B, prob, x0, ui, early_exit, install, jacobian_mode=0):
    """(observables, AL observables) of one AL solve on a fresh handle; install(s): the bounds, behind the AL installation"""
    s = _solver(B, N=prob["N"])
    s.set_problem(prob)
    s.set_options(jacobian_mode=jacobian_mode, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(kc.MAX_ITER)
    s.set_augmented_lagrangian(**kc.al_args())
    install(s)
    s.initialize(x0, ui); cost = s.solve(x0)
    obs, counters = lc.observables(s, cost)
    mj, mc = s.al_multipliers(); viol, done = s.al_violation()
    extra = dict(mu_j=mj, mu_c=mc, rho=s.al_penalties(), viol=viol, done=done, al_trace=s.al_trace(), mu_s=s.al_state_multipliers(), rho_s=s.al_state_penalties(),
                 viol_s=s.al_state_violation(), state_trace=s.al_state_trace())
    s.close()
    assert counters["adopt"] == 0
    return obs, extra


def _same(a, b):
    lc.assert_same(a[0], b[0])
    for k in a[1]:
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True), k


def _windows(win, swin):
    def install(s):
        s.set_al_knot_bounds(win)
        s.set_al_state_knot_bounds(swin, AL["rho_state0"], AL["tol_state"])
    return install


def test_constant_rows_equal_the_whole_horizon_tables_bit_for_bit():
    """the same doubles through the per-knot instantiations: stages and a solve in both exit modes, bitwise"""
    X, U, mu_j, mu_c, mu_s, rho, srec, rec, _, _ = stc.regimes()
    B = X.shape[0]
    s = _solver(B, N=N4); s.set_problem(stc.stage_problem())
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.set_augmented_lagrangian(1, 1.0, 1.0, margin=stc.STAGE_MARGIN)
    s.set_al_bounds(rec); s.set_al_state_bounds(srec, 1.0, 1e-3)
    s.set_al_multipliers(mu_j, mu_c, rho[:, :2]); s.set_al_state_multipliers(mu_s, rho[:, 2])
    tab, cost0 = _stage(s)
    s.set_al_knot_bounds(np.repeat(rec[:, None], N4 + 1, axis=1)); s.set_al_state_knot_bounds(np.repeat(srec[:, None], N4 + 1, axis=1), 1.0, 1e-3)
    assert s.al_bounds_per_knot() == 3 and np.array_equal(s.al_state_multipliers(), mu_s)      # (a window that replaces a table keeps the multipliers)
    s.set_al_state_multipliers(None, rho[:, 2])
    kn, cost1 = _stage(s)
    s.clear_al_state_bounds()                                           # the joint / torque family alone, per knot against its table
    kj, cost2 = _stage(s)
    s.set_al_bounds(rec)
    assert s.al_bounds_per_knot() == 0
    tj, cost3 = _stage(s)
    s.close()
    for n in NAMES:
        assert np.array_equal(tab[n], kn[n]) and np.array_equal(tj[n], kj[n]), n
    assert np.array_equal(cost0, cost1) and np.array_equal(cost2, cost3)
    prob, x0, ui, win, swin, _ = kc.end_to_end()
    rec4, srec4 = win[:, -1], swin[:, -1]                                # (the last rows: the tight wrist bound and the highest floor)
    for early_exit in (False, True):
        def tables(s):
            s.set_al_bounds(rec4); s.set_al_state_bounds(srec4, AL["rho_state0"], AL["tol_state"])
        _same(_al_solve(4, prob, x0, ui, early_exit, tables),
              _al_solve(4, prob, x0, ui, early_exit, _windows(np.repeat(rec4[:, None], prob["N"] + 1, axis=1), np.repeat(srec4[:, None], prob["N"] + 1, axis=1))))


def test_the_torque_fields_of_row_n_are_never_read(e2e_runs):
    prob, x0, ui, win, swin, _ = kc.end_to_end()
    other = win.copy(); other[:, -1, 38:57] = -1.0; other[:, -1, 57:76] = 1.0      # a valid row that would bind every actuator
    _same(e2e_runs[True, "default"], _al_solve(4, prob, x0, ui, True, _windows(other, swin)))
    X, U, mu_j, mu_c, rho, rec, _, _ = bc.regimes_table()
    jw = kc.joint_windows()
    o2 = jw.copy(); o2[:, -1, 38:57] = -1.0; o2[:, -1, 57:76] = 1.0
    s = _solver(X.shape[0], N=N4); s.set_problem(ac.stage_problem())
    s.set_augmented_lagrangian(1, 1.0, 1.0)
    out = []
    for w in (jw, o2):
        s.initialize(X[:, 0], U); s.set_trajectory(X, U)                # (the cold start clears the done flags of the update before)
        s.set_al_multipliers(mu_j, mu_c, rho)
        s.set_al_knot_bounds(w)
        out.append(_stage(s))
        s.al_update(0)
        out[-1] += (s.al_multipliers(), s.al_violation())
    s.close()
    (q0, c0, m0, v0), (q1, c1, m1, v1) = out
    assert all(np.array_equal(q0[n], q1[n]) for n in NAMES) and np.array_equal(c0, c1)
    assert all(np.array_equal(a, b) for a, b in zip(m0 + v0, m1 + v1))


# ------------------------------------------------------------------------------------------------------------------------- 4. the update
def test_update_kernel_against_the_restatement_under_windows():
    N, B = 4, 6
    jr, cr = ar.ranges()
    rng = np.random.default_rng(15)
    X = np.tile(sc.standing_state(), (B, N + 1, 1)); X[..., 7:26] += rng.uniform(-0.2, 0.2, (B, N + 1, 19))
    X[..., sr.SLOTS] = rng.uniform(-0.5, 0.5, (B, N + 1, 28)) + np.where(sr.SLOTS == 2, 1.0, 0.0)
    U = rng.uniform(-0.7, 0.7, (B, N, 19)) * sc.CTRLRANGE
    win = np.tile(br.default_record(0.0), (B, N + 1, 1))
    win[..., 0:19] -= rng.uniform(0.0, 0.05, (B, N + 1, 19)); win[..., 19:38] += rng.uniform(0.0, 0.05, (B, N + 1, 19))      # every row its own
    win[..., 38:57] *= rng.uniform(0.8, 1.0, (B, N + 1, 19)); win[..., 57:76] *= rng.uniform(0.8, 1.0, (B, N + 1, 19))
    swin = np.tile(np.concatenate([np.full(28, -0.6), np.full(28, 0.7)]), (B, N + 1, 1)); swin[..., 2] += 1.0; swin[..., 30] += 1.0
    swin[..., :28] -= rng.uniform(0.0, 0.05, (B, N + 1, 28))
    win[0, 2, 57 + 7] = cr[7, 1] * 0.5; U[0, 2, 7] = cr[7, 1] * 0.6        # one knot's narrower row: not done only because of it
    win[1, 3, 19 + 5] = jr[5, 1] + 0.1; X[1, 3, 7 + 5] = jr[5, 1] + 0.05   # one knot's wider row: done only because of it
    X[2, 0, 7 + 0] = win[2, 0, 19 + 0] + 0.2; X[2, 0, 1] = swin[2, 0, 28 + 1] + 0.3      # violated at knot 0 only: zero violation, zero multipliers
    swin[3, 4, 28 + 9] = 0.1; X[3, 4, 32] = 0.25                           # the state family: the terminal knot's narrower row
    swin[4, 2, 28 + 12] = np.inf; X[4, 2, 35] = 5.0                        # a side switched off at one knot: done
    X[5, 1, 7 + 2] = win[5, 2, 19 + 2] + 0.3; win[5, 1, 19 + 2] = X[5, 1, 7 + 2] + 0.01  # past knot 2's row, inside its own: done
    mu_j = np.zeros((B, N + 1, 19, 2)); mu_c = np.zeros((B, N, 19, 2)); mu_s = np.zeros((B, N + 1, 28, 2))
    mu_j[:, 1:] = rng.uniform(0.0, 30.0, (B, N, 19, 2)); mu_c[:] = rng.uniform(0.0, 30.0, (B, N, 19, 2)); mu_s[:, 1:] = rng.uniform(0.0, 30.0, (B, N, 28, 2))
    mu_j[2] = 0.0; mu_c[2] = 0.0; mu_s[2] = 0.0
    al = dict(rounds=2, rho_joint0=100.0, rho_ctrl0=2.0, growth=7.0, rho_max_factor=50.0, margin=0.0, tol_joint=1e-3, tol_ctrl=1e-2)
    rho = np.tile([100.0, 2.0, 40.0], (B, 1)) * (1.0 + 0.1 * np.arange(B))[:, None]
    rho_max, tol = (5000.0, 100.0, 2000.0), (1e-3, 1e-2, 1e-3)
    worst = {}
    for state in (True, False):
        s = _solver(B, N=N); s.set_problem(ac.stage_problem())
        s.initialize(X[:, 0], U); s.set_trajectory(X, U)
        s.set_augmented_lagrangian(**al)
        s.set_al_knot_bounds(win)
        if state:
            s.set_al_state_knot_bounds(swin, 40.0, 1e-3); s.set_al_state_multipliers(mu_s, rho[:, 2])
        s.set_al_multipliers(mu_j, mu_c, rho[:, :2])
        s.al_update(1)
        gj, gc = s.al_multipliers(); gs = s.al_state_multipliers(); grho = np.concatenate([s.al_penalties(), s.al_state_penalties()[:, None]], axis=1)
        viol, done = s.al_violation(); vs = s.al_state_violation()
        s.close()
        for b in range(B):
            if state:
                nj, nc, ns, r2, d2, v2 = kr.state_update(X[b], U[b], mu_j[b], mu_c[b], mu_s[b], tuple(rho[b]), False, win[b], swin[b], al["growth"], rho_max, tol)
            else:
                nj, nc, r2, d2, v2 = kr.update(X[b], U[b], mu_j[b], mu_c[b], tuple(rho[b, :2]), False, win[b], al["growth"], rho_max[:2], tol[:2])
                ns, r2, v2 = np.zeros_like(mu_s[b]), r2 + (0.0,), v2 + (0.0,)
            assert bool(done[b]) == d2 and (viol[b, 0], viol[b, 1], vs[b]) == v2, (state, b, done[b], d2, viol[b], vs[b], v2)
            for name, g_, w_ in (("mu_joint", gj[b], nj), ("mu_ctrl", gc[b], nc), ("mu_state", gs[b], ns), ("rho", grho[b], np.array(r2))):
                assert np.array_equal(g_ > 0, w_ > 0), (state, b, name)
                err = (np.abs(g_ - w_) / np.maximum(1e-300, np.abs(w_))).max() if w_.any() else np.abs(g_).max()
                worst[name] = max(worst.get(name, 0.0), err)
                assert err <= 1e-14, (state, b, name, err)
        assert list(done) == ([0, 1, 1, 0, 1, 1] if state else [0, 1, 1, 1, 1, 1])
        assert not gj[2].any() and not gc[2].any() and not gs[2].any() and viol[2, 0] == 0.0 and vs[2] == 0.0
    # rollouts 0 and 1 under the default row in place of the one that decides them: the other way round
    w0 = win[0].copy(); w0[2, 57 + 7] = cr[7, 1]
    assert kr.update(X[0], U[0], mu_j[0], mu_c[0], tuple(rho[0, :2]), False, w0, al["growth"], rho_max[:2], tol[:2])[3]
    w1 = win[1].copy(); w1[3, 19 + 5] = jr[5, 1]
    assert not kr.update(X[1], U[1], mu_j[1], mu_c[1], tuple(rho[1, :2]), False, w1, al["growth"], rho_max[:2], tol[:2])[3]
    _report("update kernel under windows against the restatement (relative)", worst)


# ---------------------------------------------------------------------------------------------------------------------- 5. end to end
@pytest.fixture(scope="module")
def e2e_runs():
    """the B = 4 case in both exit modes and both launch orders, solved once: {(early_exit, order): (observables, AL observables)}"""
    prob, x0, ui, win, swin, _ = kc.end_to_end()
    out = {}
    for early_exit in (False, True):
        out[early_exit, "default"] = _al_solve(4, prob, x0, ui, early_exit, _windows(win, swin))
        with env(**SEQ):
            out[early_exit, "seq"] = _al_solve(4, prob, x0, ui, early_exit, _windows(win, swin))
    return out


@pytest.mark.parametrize("order", ["default", "seq"])
@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_end_to_end_against_the_reference_driver(early_exit, order, e2e_runs):
    obs, ex = e2e_runs[early_exit, order]
    sol = kc.reference_solves(early_exit)
    tols = (AL["tol_joint"], AL["tol_ctrl"], AL["tol_state"])
    worst = {}
    for b in range(4):
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
        last = ref["rounds"][-1]
        n = last["iterations"]
        assert obs["iterations"][b] == n
        assert np.array_equal(obs["trace_alpha"][b, :n], last["trace_alpha"][:n]), (b, obs["trace_alpha"][b], last["trace_alpha"])
        e = np.abs(obs["trace_cost"][b, :n + 1] / last["trace_cost"][:n + 1] - 1).max(); worst["cost trace"] = max(worst.get("cost trace", 0.0), e)
        assert e <= 1e-5, (b, obs["trace_cost"][b], last["trace_cost"])
        e = np.abs(obs["trace_lambda"][b, :n] / last["trace_lambda"][:n] - 1).max(); worst["lambda"] = max(worst.get("lambda", 0.0), e)
        assert e <= 1e-12
        assert bool(ex["done"][b]) == ref["done"] and tuple(ex["rho"][b]) == tuple(ref["rho"]) and ex["rho_s"][b] == ref["rho_s"]
        for name, g_, w_ in (("mu_joint", ex["mu_j"][b], ref["mu_j"]), ("mu_ctrl", ex["mu_c"][b], ref["mu_c"]), ("mu_state", ex["mu_s"][b], ref["mu_s"]),
                             ("x", obs["xbar"][b], ref["X"]), ("u", obs["ubar"][b], ref["U"])):
            e = np.abs(g_ - w_).max() / max(1.0, np.abs(w_).max()); worst[name] = max(worst.get(name, 0.0), e)
            assert e <= 1e-5, (b, name, e)
    figures = kc.effect_assertions([dict(X=obs["xbar"][b], U=obs["ubar"][b]) for b in range(4)])
    assert not ex["mu_c"][0, kc.T_S:, kc.WRIST].any() and ex["mu_c"][1, 0, kc.WRIST].max() > 0.0      # the bound of rollout 0 never binds where it holds
    assert ex["mu_s"][2, -1, 2, 0] > 0.0 and not ex["mu_s"][[0, 1, 3]].any()
    _report("end to end under windows, %s, %s order (relative)" % ("convergence exit" if early_exit else "fixed", order), worst)
    print("  " + ", ".join("%s %.6g" % kv for kv in figures.items()))


def test_rollout_without_a_window_of_its_own_repeats_the_solve_without_any_table(e2e_runs):
    """rollout 3 (default rows, infinite state rows) against the same batch without table or window: decisions exactly, values to 1e-9 (the
    same doubles through other machine code, as test_rollout_without_bounds_matches_the_solve_without_a_table has it)"""
    prob, x0, ui, _, _, _ = kc.end_to_end()
    obs, ex = e2e_runs[True, "default"]
    o0, e0 = _al_solve(4, prob, x0, ui, True, lambda s: None)
    for k in ("trace_alpha", "trace_lambda", "iterations"):
        assert np.array_equal(obs[k][3], o0[k][3], equal_nan=True), k
    assert ex["done"][3] == e0["done"][3]
    worst = 0.0
    for got, want in [(obs[k][3], o0[k][3]) for k in ("cost", "trace_cost", "xbar", "ubar", "K")] + [(ex[k][3], e0[k][3]) for k in ("mu_j", "mu_c", "viol")]:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        worst = max(worst, np.nanmax(np.abs(got - want), initial=0.0) / max(1.0, np.nanmax(np.abs(want), initial=0.0)))
    print("rollout 3 against the solve without any table (relative to max(1, |want|)): %.2e" % worst)
    assert worst <= 1e-9
    assert not np.array_equal(obs["ubar"][1], o0["ubar"][1])


# -------------------------------------------------------------------------------------------- 6. permuted, broadcast, sliced, orders, caches
def _tiled(B, sel=None):
    prob4, x04, ui4, win4, swin4, _ = kc.end_to_end()
    idx = np.arange(B) % 4 if sel is None else sel
    pb = dict(prob4)
    for k in REF_KEYS:
        pb[k] = np.ascontiguousarray(prob4[k][idx])
    win, swin = win4[idx].copy(), swin4[idx].copy()
    for b in range(B):                                                  # every window its own
        tighter = 1.0 - 0.002 * (b // 4)
        win[b, :, 38 + kc.WRIST] = np.where(win[b, :, 57 + kc.WRIST] == kc.WRIST_BOUND, -kc.WRIST_BOUND * tighter, win[b, :, 38 + kc.WRIST])
        swin[b, :, 2] += np.where(np.isfinite(swin[b, :, 2]), 1e-6 * (b // 4), 0.0)
    return pb, np.ascontiguousarray(x04[idx]), np.ascontiguousarray(ui4[idx]), win, swin, idx


def test_windows_permute_and_broadcast_bit_for_bit_at_b_70():
    """B = 70, wider than one wave of k_solve_begin_al and of the knot-cost kernels, 70 windows of their own: permuting the windows with the
    rollouts permutes the results (the compacted lists index by the rollout); one window equals B copies of it"""
    B = 70
    pb, x0, ui, win, swin, idx = _tiled(B)
    perm = np.random.default_rng(3).permutation(B)
    a = _al_solve(B, pb, x0, ui, True, _windows(win, swin))
    pb2 = dict(pb)
    for k in REF_KEYS:
        pb2[k] = np.ascontiguousarray(pb[k][perm])
    b = _al_solve(B, pb2, np.ascontiguousarray(x0[perm]), np.ascontiguousarray(ui[perm]), True, _windows(win[perm], swin[perm]))
    for k in lc.NAMES:
        assert np.array_equal(a[0][k][perm], b[0][k], equal_nan=True), k
    for k in a[1]:
        ak = a[1][k][:, perm] if k in ("al_trace", "state_trace") else a[1][k][perm]
        assert np.array_equal(ak, b[1][k], equal_nan=True), k
    assert len({tuple(r) for r in a[0]["ubar"][1::4, 0]}) > 1             # the tightened bounds are felt
    one = _al_solve(B, pb, x0, ui, True, _windows(win[1], swin[2]))
    many = _al_solve(B, pb, x0, ui, True, _windows(np.tile(win[1], (B, 1, 1)), np.tile(swin[2], (B, 1, 1))))
    _same(one, many)


@pytest.mark.parametrize("early_exit", [False, True], ids=["fixed", "convergence_exit"])
def test_orders_and_caches_match_the_default_bit_for_bit(early_exit, e2e_runs):
    prob, x0, ui, win, swin, _ = kc.end_to_end()
    base = e2e_runs[early_exit, "default"]
    _same(base, e2e_runs[early_exit, "seq"])
    for var in (dict(ILQR_RELIN="1"), dict(ILQR_REPASS="1"), dict(ILQR_DEDUP_RETRY="0")):
        with env(**var):
            _same(base, _al_solve(4, prob, x0, ui, early_exit, _windows(win, swin)))


def test_batch_slices_and_forward_difference_jacobians(e2e_runs):
    """ILQR_SLICES=2 at B = 128 (a slice holds at least 64 rollouts): the second slice moved on by one, so that rollout 64 + i carries other
    windows than rollout i -- a slice that forgot the windows' offset b0 * stride would solve it under the windows of rollout i.  Every rollout
    repeats the unsliced run of its own inputs to 1e-9, decisions exactly.  Forward differences: the effects are there."""
    B = 128
    sel = (np.arange(B) + (np.arange(B) >= 64)) % 4
    pb, x0, ui, win, swin, idx = _tiled(B, sel)
    assert idx[64] != idx[0]
    whole = _al_solve(B, pb, x0, ui, True, _windows(win, swin))
    with env(ILQR_SLICES="2"):
        s = _solver(B, N=pb["N"]); assert s.L.ilqr_hip_num_slices(s.h) == 2; s.close()
        obs, ex = _al_solve(B, pb, x0, ui, True, _windows(win, swin))
    worst = 0.0
    for k in ("trace_alpha", "trace_lambda", "iterations"):
        assert np.array_equal(obs[k], whole[0][k], equal_nan=True), k
    assert np.array_equal(ex["done"], whole[1]["done"])
    for got, want in [(obs[k], whole[0][k]) for k in ("trace_cost", "xbar", "ubar", "K")] + [(ex[k], whole[1][k]) for k in ex]:
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        worst = max(worst, np.nanmax(np.abs(got - want), initial=0.0) / max(1.0, np.nanmax(np.abs(want), initial=0.0)))
    assert worst <= 1e-9, worst
    prob, x04, ui4, win4, swin4, _ = kc.end_to_end()
    obs, ex = _al_solve(4, prob, x04, ui4, True, _windows(win4, swin4), jacobian_mode=1)
    assert np.all(np.isfinite(obs["cost"]))
    kc.effect_assertions([dict(X=obs["xbar"][b], U=obs["ubar"][b]) for b in range(4)])
    print("ILQR_SLICES=2, B = 128 against the unsliced run (relative to max(1, |want|)): %.2e" % worst)


# ------------------------------------------------------------------------------------------------------------------------------ 7. the track
def _track(rows, N):
    """a bounds track on the loop's timeline: the wrist bound drops to 0.9 x its range from row 2 + N on (so that it enters the window of
    loop step 2 at its last knot and moves one knot forward per step), the pelvis floor rises row by row"""
    jc = sc.stack_al_knot_bounds(dict(ctrl_lo=(2 + N, rows, {kc.WRIST: -kc.WRIST_BOUND}), ctrl_hi=(2 + N, rows, {kc.WRIST: kc.WRIST_BOUND})), 1, rows - 1)[0]
    st = sc.stack_al_state_knot_bounds(dict(pelvis_z=[(r, r + 1, (0.9 + 1e-3 * r, np.inf)) for r in range(rows)]), 1, rows - 1)[0]
    return jc, st


def test_track_cut_equals_numpy_indexing_bit_for_bit():
    prob, x0, ui, _, _, _ = kc.end_to_end()
    N, B, rows = prob["N"], 4, 12
    jc, st = _track(rows, N)
    s = _solver(B, N=N); s.set_problem(prob); s.set_augmented_lagrangian(**kc.al_args())
    s.set_al_state_bounds(sr.NO_BOUNDS, AL["rho_state0"], AL["tol_state"])
    assert s.al_bounds_track_rows() == 0
    s.set_al_bounds_track(jc, st)
    assert s.al_bounds_track_rows() == rows and s.al_bounds_per_knot() == 0
    for starts in ([0], [0, 3, 5, 9]):
        if len(starts) > 1:
            s.set_al_bounds_track_starts(starts)
        for step in (0, 1, rows - N, rows + 3):                         # the last two: into and past the end clamp
            s.al_bounds_window_from_track(step)
            gj, gs = s.al_knot_bounds()
            assert np.array_equal(gj, kr.cut(jc, starts, step, N, B)) and np.array_equal(gs, kr.cut(st, starts, step, N, B)), (starts, step)
            assert s.al_bounds_per_knot() == 3 and s.num_al_bound_sets() == len(starts) and s.num_al_state_bound_sets() == len(starts)
    assert np.array_equal(gj[3], np.tile(jc[-1], (N + 1, 1)))
    # the joint / torque part alone: the state family keeps its table, expanded by the library
    s.set_al_state_bounds(st[5], AL["rho_state0"], AL["tol_state"])
    s.set_al_bounds_track(jc, None)
    s.al_bounds_window_from_track(2)
    gj, gs = s.al_knot_bounds()
    assert np.array_equal(gj, kr.cut(jc, [0], 2, N, B)) and np.array_equal(gs, np.tile(st[5], (B, N + 1, 1))) and s.al_bounds_per_knot() == 1
    assert np.array_equal(s.al_state_bounds(), np.tile(st[5], (B, 1)))
    s.clear_al_bounds_track()
    assert s.al_bounds_track_rows() == 0 and s.al_bounds_per_knot() == 1 and np.array_equal(s.al_knot_bounds()[0], gj)      # the windows last written stay
    s.close()


def test_warm_started_mpc_on_the_track_equals_the_setters_bit_for_bit():
    prob, x0, ui, _, _, _ = kc.end_to_end()
    N, B, rows = prob["N"], 4, 12
    jc, st = _track(rows, N)
    starts = [0, 1, 0, 2]
    runs = []
    for use_track in (True, False):
        s = _solver(B, N=N); s.set_problem(prob); s.set_max_iterations(kc.MAX_ITER); s.set_augmented_lagrangian(**kc.al_args())
        s.set_al_state_bounds(sr.NO_BOUNDS, AL["rho_state0"], AL["tol_state"])
        if use_track:
            s.set_al_bounds_track(jc, st); s.set_al_bounds_track_starts(starts)
        out = []
        for step in range(3):
            if use_track:
                s.al_bounds_window_from_track(step)
            else:
                s.set_al_knot_bounds(kr.cut(jc, starts, step, N, B))
                rho_s, mu_s = s.al_state_penalties(), s.al_state_multipliers()
                s.set_al_state_knot_bounds(kr.cut(st, starts, step, N, B), AL["rho_state0"], AL["tol_state"])
                s.set_al_state_multipliers(mu_s, rho_s)                 # (the setter resets rho_state; the cut does not touch the store)
            if step == 0:
                s.initialize(x0, ui)
            else:
                s.initialize_warm_resident(x0)
            cost = s.solve(x0)
            out.append((cost, s.xbar(), s.ubar(), s.al_multipliers(), s.al_state_multipliers(), s.al_trace(), s.al_state_trace()))
        s.close()
        runs.append(out)
    for step in range(3):
        for a, b in zip(runs[0][step], runs[1][step]):
            for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
                assert np.array_equal(x, y, equal_nan=True), step
    assert runs[0][2][3][1][:, -1, kc.WRIST].max() >= 0.0 and np.all(np.isfinite(runs[0][2][0]))


def test_closed_loop_runner_follows_the_bounds_track():
    """MPCRunner, resident with device_refs=True, under a track whose torque bounds drop to 5 % of the range at loop step 2: the applied plan
    against the same loop fed through the knot setter -- the same runner, whose solver's al_bounds_window_from_track is replaced by
    set_al_knot_bounds of the NumPy cut -- bit for bit; the runner asks for the step index of its reference windows, once per solve, and
    feeds track_starts to the bounds track's start rows"""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    from mpc_ilqr_mujoco_amd import solver as sv
    prob3, x03, ui3 = ac.end_to_end()
    B, steps, N = 2, 4, prob3["N"]
    base = sc.make_problem(sv.reference_kinematics, N=N)
    for k in ("Q", "R", "Qf"):
        base[k] = np.array(prob3[k])
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    xr = np.tile(sc.standing_state(), (40, 1)); xr[:, 7 + 14] = ar.ranges()[0][14, 1] + 1.0
    rd.set_states(xr); rd.contact = np.ones((40, 2), dtype=np.int32)
    x0 = np.array(x03[[1, 1]]); ui = np.array(ui3[[1, 1]])
    rows = 20
    jc = sc.stack_al_knot_bounds(dict(torque_scale=(2, rows, 0.05)), 1, rows - 1)[0]
    assert np.array_equal(jc[1], br.default_record(0.0)) and np.array_equal(jc[2, 57:], 0.05 * br.default_record(0.0)[57:])
    starts = [0, 1]
    runs, calls = {}, []
    for how in ("track", "setters", "none"):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(ac.MAX_ITER); s.set_augmented_lagrangian(**ac.AL_E2E)
        if how == "track":
            s.set_al_bounds_track(jc)
        elif how == "setters":
            s.al_bounds_track_rows = lambda: rows
            s.set_al_bounds_track_starts = lambda st: calls.append(("starts", list(st)))
            s.al_bounds_window_from_track = lambda step, s=s: (calls.append(step), s.set_al_knot_bounds(kr.cut(jc, starts, step, N, B)))
        r = ml.MPCRunner(s, rd, base, resident=True, device_refs=True, track_starts=starts)
        xs, us = r.run(x0, steps, u_init=ui)
        if how != "none":
            assert s.al_bounds_per_knot() == 1 and np.array_equal(s.al_knot_bounds()[0], kr.cut(jc, starts, steps - 1, N, B)), how
        else:
            assert s.al_bounds_per_knot() == 0                           # no bounds track: no new call
        mc = s.al_multipliers()[1]
        s.close()
        runs[how] = (np.asarray(xs), np.asarray(us), mc)
    assert calls == [("starts", starts)] + list(range(steps)), calls
    for a_, b_ in zip(runs["track"], runs["setters"]):
        assert np.array_equal(a_, b_)
    felt = not np.array_equal(runs["track"][1], runs["none"][1])
    print("closed loop under a bounds track: largest control multiplier at the end %.3g, plan differs from the loop without a track: %s" % (runs["track"][2].max(), felt))
    assert felt


# ------------------------------------------------------------------------------------------------------------ 8. warm start, 9. life cycle
def test_warm_start_shifts_the_multipliers_and_keeps_the_windows():
    prob, x0, ui, win, swin, _ = kc.end_to_end()
    N = prob["N"]
    rng = np.random.default_rng(19)
    s = _solver(4, N=N); s.set_problem(prob); s.set_max_iterations(kc.MAX_ITER); s.set_augmented_lagrangian(**kc.al_args())
    _windows(win, swin)(s)
    s.initialize(x0, ui); s.solve(x0)
    mj, mc = s.al_multipliers(); ms = s.al_state_multipliers()
    mj = mj + rng.uniform(1.0, 2.0, mj.shape); mc = mc + rng.uniform(1.0, 2.0, mc.shape); ms = ms + rng.uniform(1.0, 2.0, ms.shape); mj[:, 0] = 0.0; ms[:, 0] = 0.0
    s.set_al_multipliers(mj, mc, None); s.set_al_state_multipliers(ms, None)
    for shift in (1, 2):
        s.initialize_warm_resident(x0, shift=shift)
        gj, gc = s.al_multipliers()
        wj, wc_ = ar.shift(mj, mc, shift)
        assert np.array_equal(gj, wj) and np.array_equal(gc, wc_) and np.array_equal(s.al_state_multipliers(), sr.shift(ms, shift))
        gw, gs = s.al_knot_bounds()
        assert np.array_equal(gw, win) and np.array_equal(gs, swin) and s.al_bounds_per_knot() == 3      # the window is horizon-local: it stays
        s.set_al_multipliers(mj, mc, None); s.set_al_state_multipliers(ms, None)
    assert np.all(np.isfinite(s.solve(x0)))
    s.initialize(x0, ui)
    assert np.array_equal(s.al_knot_bounds()[0], win) and s.al_bounds_per_knot() == 3
    s.close()


def test_life_cycle_and_refusals():
    from mpc_ilqr_mujoco_amd import solver as sv
    import weight_set_cases as wc
    prob, x0, ui, win, swin, _ = kc.end_to_end()
    N, B = prob["N"], 4
    dflt = sv.al_default_bounds(0.0)
    s = _solver(B, N=N); s.set_problem(prob); s.set_max_iterations(kc.MAX_ITER)
    for call in (lambda: s.set_al_knot_bounds(win), lambda: s.set_al_state_knot_bounds(swin, 1.0), s.al_knot_bounds, lambda: s.set_al_bounds_track(win[0]),
                 lambda: s.al_bounds_window_from_track(0)):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            call()
    assert s.al_bounds_per_knot() == 0
    s.set_augmented_lagrangian(**dict(kc.al_args(), margin=0.1))
    jc, st = s.al_knot_bounds()
    assert np.array_equal(jc, np.tile(sv.al_default_bounds(0.1), (B, N + 1, 1))) and np.all(st[..., :28] == -np.inf) and np.all(st[..., 28:] == np.inf)
    s.set_augmented_lagrangian(**kc.al_args())
    # later call wins, in both directions, per family
    rec = win[:, -1].copy()
    s.set_al_bounds(rec); s.set_al_knot_bounds(win)
    assert s.al_bounds_per_knot() == 1 and s.num_al_bound_sets() == B
    with pytest.raises(sv.ILQRError, match="ilqr_hip_get_al_knot_bounds"):
        s.al_bounds()
    assert np.isinf(s.al_state_bounds()).all()                           # (the other family's getter is untouched)
    s.set_al_bounds(rec[1])
    assert s.al_bounds_per_knot() == 0 and s.num_al_bound_sets() == 1 and np.array_equal(s.al_bounds(), np.tile(rec[1], (B, 1)))
    assert np.array_equal(s.al_knot_bounds()[0], np.tile(rec[1], (B, N + 1, 1)))
    s.set_al_state_bounds(swin[2, -1], 1.0); s.set_al_state_knot_bounds(swin[2], 5.0)
    assert s.al_bounds_per_knot() == 2 and s.num_al_state_bound_sets() == 1 and np.array_equal(s.al_state_penalties(), np.full(B, 5.0))
    with pytest.raises(sv.ILQRError, match="ilqr_hip_get_al_knot_bounds"):
        s.al_state_bounds()
    assert np.array_equal(s.al_bounds(), np.tile(rec[1], (B, 1)))
    jc, st = s.al_knot_bounds()
    assert np.array_equal(jc, np.tile(rec[1], (B, N + 1, 1))) and np.array_equal(st, np.tile(swin[2], (B, 1, 1)))
    s.set_al_state_bounds(swin[:, -1], 1.0)
    assert s.al_bounds_per_knot() == 0 and np.array_equal(s.al_state_bounds(), swin[:, -1])
    s.set_al_knot_bounds(win); s.set_al_state_knot_bounds(swin, AL["rho_state0"], AL["tol_state"])
    # every refusal leaves the handle as it was
    def bad(i, v, j=None, w=None, t=3):
        b_ = win.copy(); b_[2, t, i] = v
        if j is not None:
            b_[2, t, j] = w
        return b_
    sbad = [swin.copy() for _ in range(4)]
    sbad[0][1, 4, 5] = np.nan; sbad[1][0, 0, 3] = np.inf; sbad[2][2, N, 28 + 7] = -np.inf; sbad[3][1, 2, 2] = 2.0; sbad[3][1, 2, 30] = 1.0
    def unchanged():
        jc_, st_ = s.al_knot_bounds()
        return s.al_bounds_per_knot() == 3 and np.array_equal(jc_, win) and np.array_equal(st_, swin) and np.array_equal(s.al_state_penalties(), np.full(B, AL["rho_state0"]))
    for what, arr in (("NaN", bad(7, np.nan)), ("lo > hi", bad(4, 1.0, 19 + 4, 0.5)), ("lo = +inf", bad(6, np.inf, 19 + 6, np.inf)), ("hi = -inf", bad(57 + 9, -np.inf, 38 + 9, -np.inf)),
                      ("torque row N NaN", bad(57 + 3, np.nan, t=N)), ("n_sets 2", win[:2]), ("n_sets 3", win[:3])):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_al_knot_bounds(arr)
        assert unchanged(), what
    for arr, rho0, tol in [(a, 1.0, 1e-3) for a in sbad] + [(swin[:2], 1.0, 1e-3), (swin, 0.0, 1e-3), (swin, np.inf, 1e-3), (swin, 1.0, -1e-9)]:
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_al_state_knot_bounds(arr, rho0, tol)
        assert unchanged()
    assert s.L.ilqr_hip_set_al_knot_bounds(s.h, None, B) == 1 and s.L.ilqr_hip_set_al_knot_bounds(s.h, sv._p(np.ascontiguousarray(win)), 0) == 1
    with pytest.raises(ValueError):
        s.set_al_knot_bounds(win[:, :N])
    for args in ((bad(7, np.nan)[2], None), (None, sbad[0][1]), (None, None)):
        with pytest.raises((sv.ILQRError, ValueError)):
            s.set_al_bounds_track(*args)
    assert s.al_bounds_track_rows() == 0 and unchanged()
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.set_al_bounds_track_starts([0])
    s.set_al_bounds_track(win[1])
    for starts in ([-1], [0, 1], [0, 0, 0, -2]):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_al_bounds_track_starts(starts)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        s.al_bounds_window_from_track(-1)
    assert unchanged()
    # weight sets stay refused; the windows survive the initialisers, set_al_multipliers and a repeated installation
    sets = wc.one_set_arrays(wc.problem_of_set(wc.weight_set_problem(B, N, B), 0))
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        s.set_weight_sets(*sets)
    s.initialize(x0, ui); first = s.solve(x0)
    s.set_al_multipliers(None, None, np.tile([1e5, 1e3], (B, 1)))
    s.initialize_warm_resident(x0)
    s.set_augmented_lagrangian(**kc.al_args())
    assert unchanged()
    s.set_regularization(1e-6)
    s.initialize(x0, ui)
    assert np.array_equal(s.solve(x0), first)
    # clear_* drop whichever is installed; clear_augmented_lagrangian drops the windows; a state part without a state family is refused
    s.clear_al_bounds()
    assert s.al_bounds_per_knot() == 2 and s.num_al_bound_sets() == 0 and np.array_equal(s.al_knot_bounds()[0], np.tile(dflt, (B, N + 1, 1)))
    s.clear_al_state_bounds()
    assert s.al_bounds_per_knot() == 0 and s.num_al_state_bound_sets() == 0
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
        s.set_al_bounds_track(None, swin[2])
    s.set_al_knot_bounds(win)
    s.clear_augmented_lagrangian()
    assert s.al_bounds_per_knot() == 0 and s.num_al_bound_sets() == 0
    s.set_augmented_lagrangian(**kc.al_args())
    assert s.al_bounds_per_knot() == 0 and np.array_equal(s.al_bounds(), np.tile(dflt, (B, 1)))
    s.close()
    # a family of the test library that evaluates the cost inside its own kernels refuses, as for AL today
    t = _solver(B, N=N, legacy=True); t.set_problem(prob); t.set_max_iterations(kc.MAX_ITER)
    t.set_augmented_lagrangian(**kc.al_args()); _windows(win, swin)(t)
    t.initialize(x0, ui)
    with env(ILQR_DYN="s"):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            t.solve(x0)
    assert np.all(np.isfinite(t.solve(x0))) and t.al_bounds_per_knot() == 3
    t.close()


# ------------------------------------------------------------------------------------------------------------- 10. walked installations
def _walk_inputs():
    """B = 3 rollouts: the hinges, controls, joint / torque windows and multipliers of three rollouts of al_bounds_cases.regimes_table(), the box
    coordinates, state windows and state multipliers of three rollouts of al_state_cases.regimes() -- one trajectory that excites both
    families' discriminating windows (al_knot_cases.joint_windows / state_windows).  Tables are row N of the windows."""
    Xj, Uj, mu_j, mu_c, rho, _, jcases, _ = bc.regimes_table()
    Xs, _, _, _, mu_s, rho3, _, _, scases, _ = stc.regimes()
    ji = [next(i for i, c in enumerate(jcases) if c[0] == "joint" and c[4] == 0 and c[3] > 0), next(i for i, c in enumerate(jcases) if c[0] == "ctrl" and c[4] == 1), bc.INF_ROLLOUTS[0]]
    si = [next(i for i, c in enumerate(scases) if c[2] > 0 and c[3] == 0),next(i for i, c in enumerate(scases) if c[0] >= 3 and c[2] > 0 and c[3] == 1), stc.INF_ROLLOUTS[0]]
    assert len(set(ji)) == 3 and len(set(si)) == 3
    X = Xj[ji].copy(); X[:, :, sr.SLOTS] = Xs[si][:, :, sr.SLOTS]
    return dict(X=X, U=Uj[ji].copy(), mu_j=mu_j[ji], mu_c=mu_c[ji], rho=rho[ji], mu_s=mu_s[si], rho_s=rho3[si, 2].copy(),
                jwin=kc.joint_windows()[ji].copy(), swin=kc.state_windows()[0][si].copy())


def test_walked_installation_states_equal_fresh_handles():
    """One long-lived handle walked through every source of bounds the library resolves -- the model's ranges, tables of 1 and B, the model's
    record under a state table, windows, each expansion of the other family's record, a track cut, removal and re-installation -- against a
    fresh handle that installs each state directly: bounds, stage cost, quadratics and the update, bit for bit.  Where a state family is
    installed the stage cost differs from the same state without it (an unread table would pass the comparison)."""
    d = _walk_inputs()
    B, N = 3, N4
    jwin, swin = d["jwin"], d["swin"]
    T, ST = jwin[:, N].copy(), swin[:, N].copy()
    RHO_S, TOL_S, M0, M1 = 1.0, 1e-3, stc.STAGE_MARGIN, 0.1
    jtrack, strack = np.concatenate([jwin[0], jwin[1]]), np.concatenate([swin[0], swin[1]])
    starts, step = [0, 2, 5], 1
    jcut, scut = kr.cut(jtrack, starts, step, N, B), kr.cut(strack, starts, step, N, B)

    def fresh(margin, joint, state):
        s = _solver(B, N=N); s.set_problem(stc.stage_problem())
        s.set_augmented_lagrangian(1, 1.0, 1.0, margin=margin)
        if joint is not None:
            (s.set_al_knot_bounds if joint.ndim == 3 else s.set_al_bounds)(joint)
        if state is not None:
            (s.set_al_state_knot_bounds if state.ndim == 3 else s.set_al_state_bounds)(state, RHO_S, TOL_S)
        return s

    def measure(s, state):
        s.initialize(d["X"][:, 0], d["U"]); s.set_trajectory(d["X"], d["U"])      # (the cold start clears the done flags of the update before)
        s.set_al_multipliers(d["mu_j"], d["mu_c"], d["rho"])
        if state:
            s.set_al_state_multipliers(d["mu_s"], d["rho_s"])
        out = list(s.al_knot_bounds()) + [np.array(s.al_bounds_per_knot()), np.array(s.num_al_bound_sets()), np.array(s.num_al_state_bound_sets())]
        out.append(s.stage_total_cost())
        s.stage_cost_quadratics(); out += list(s.quadratics())
        s.al_update(0)
        out += list(s.al_violation()) + list(s.al_multipliers()) + [s.al_penalties(), s.al_state_multipliers(), s.al_state_penalties(), s.al_state_violation()]
        return out

    w = _solver(B, N=N); w.set_problem(stc.stage_problem())

    def track(s):
        s.set_al_state_bounds(ST, RHO_S, TOL_S)                           # (the track's state part needs an installed state family)
        s.set_al_bounds_track(jtrack, strack); s.set_al_bounds_track_starts(starts); s.al_bounds_window_from_track(step)

    # (name, the step of the walk, what a fresh handle installs: margin, joint / torque bounds, state bounds)
    walk = [
        ("model bounds", lambda: w.set_augmented_lagrangian(1, 1.0, 1.0, margin=M0), (M0, None, None)),
        ("table of 1", lambda: w.set_al_bounds(T[0]), (M0, T[0], None)),
        ("table of B", lambda: w.set_al_bounds(T), (M0, T, None)),
        ("table of B, state table of 1", lambda: w.set_al_state_bounds(ST[0], RHO_S, TOL_S), (M0, T, ST[0])),
        ("state table alone: the model record", lambda: w.clear_al_bounds(), (M0, None, ST[0])),
        ("the model record at the new margin", lambda: w.set_augmented_lagrangian(1, 1.0, 1.0, margin=M1), (M1, None, ST[0])),
        ("joint window alone", lambda: (w.clear_al_state_bounds(), w.set_al_knot_bounds(jwin)), (M1, jwin, None)),
        ("joint window, expanded state table", lambda: w.set_al_state_bounds(ST, RHO_S, TOL_S), (M1, jwin, ST)),
        ("expanded joint table, state window", lambda: (w.set_al_bounds(T), w.set_al_state_knot_bounds(swin, RHO_S, TOL_S)), (M1, T, swin)),
        ("expanded model record, state window", lambda: w.clear_al_bounds(), (M1, None, swin)),
        ("both windows", lambda: w.set_al_knot_bounds(jwin), (M1, jwin, swin)),
        ("joint window after the state family left", lambda: w.clear_al_state_bounds(), (M1, jwin, None)),
        ("both windows cut from a track", lambda: track(w), (M1, jcut, scut)),
        ("removal and re-installation", lambda: (w.clear_augmented_lagrangian(), w.set_augmented_lagrangian(1, 1.0, 1.0, margin=M0)), (M0, None, None)),
    ]
    assert len(walk) == 14
    for name, go, (margin, joint, state) in walk:
        go()
        got = measure(w, state is not None)
        f = fresh(margin, joint, state); want = measure(f, state is not None); f.close()
        assert len(got) == len(want) == 18
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (name, i)
        assert got[2] == (0 if joint is None or joint.ndim < 3 else 1) | (0 if state is None or state.ndim < 3 else 2), name
        if state is not None:
            f = fresh(margin, joint, None); f.initialize(d["X"][:, 0], d["U"]); f.set_trajectory(d["X"], d["U"]); f.set_al_multipliers(d["mu_j"], d["mu_c"], d["rho"])
            without = f.stage_total_cost(); f.close()
            assert np.all(got[5] != without), (name, got[5], without)
    w.close()
