"""The cost kernels (k_quad_kin / k_cost_quadratics, k_traj_knot_cost / k_traj_cost_sum, the candidate costs of the line-search and
rollout kernels, h1_cost_dev.h) over the problem DATA they read: every task term alone against the torch-autograd golden, every
`weight > 0` branch on its off side, per-rollout reference sets in which no two entries are equal (tests/cost_envelope_cases.py:
nonzero u_ref, non-uniform Q / R / Qf, mixed stance rows), every row and side of the two soft-limit tables.  States and shapes are
the small ones the suite already trusts (N = 4); test_cost_envelope_cpu.py shows that these inputs discriminate.

Tolerances are those of the existing tests of the same quantities: 1e-9 max(1, |want|) against the golden (test_oracle_golden.py),
1e-10 max(1, |want|) on the quadratics and 1e-11 relative on the total cost against the oracle (test_gpu_parity.py), 1e-5 / 1e-12 on
the solve (test_full_solve_parity_trace_and_gains).  Every test prints the worst error it saw."""
import numpy as np
import pytest

import cost_envelope_cases as cc
import oracle_lib as ol
from test_gpu_configs import VARIANTS, _solver, env, rel

pytestmark = pytest.mark.gpu
sc = cc.sc
N = 4
NAMES = ("lx", "lu", "lxx", "luu")


def _oracle(prob, b=0, **opts):
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob, b); o.set_options(**opts)
    return o


def _gpu_cost_stage(s, prob, X, U):
    """the stage API on the trajectory (X, U): (dict of lx / lu / lxx / luu, total cost [B])"""
    s.set_problem(prob)
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.stage_cost_quadratics()
    got = dict(zip(NAMES, s.quadratics()))
    return got, s.stage_total_cost()


def _check_against_oracle(prob, X, U, got, cost, worst, tag):
    """rollout b on reference set b: quadratics to 1e-10 max(1, |want|), total cost to 1e-11 relative; returns the oracle's records"""
    wants = []
    for b in range(X.shape[0]):
        o = _oracle(prob, b); o.set_trajectory(X[b], U[b]); o.cost_quadratics()
        want = {n: o.get(n) for n in NAMES}
        for n in NAMES:
            err = np.abs(got[n][b] - want[n]).max()
            worst[n] = max(worst.get(n, 0.0), err / max(1.0, np.abs(want[n]).max()))
            assert err <= 1e-10 * max(1.0, np.abs(want[n]).max()), (tag, n, b, err)
        c = o.total_cost()
        worst["cost"] = max(worst.get("cost", 0.0), abs(cost[b] - c) / abs(c) if c != 0.0 else abs(cost[b]))
        assert abs(cost[b] - c) <= 1e-11 * abs(cost[b]), (tag, b, cost[b], c)
        wants.append((want, c))
    return wants


def _report(title, worst):
    print("%s: worst error relative to max(1, |want|): %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _golden_trajectory(c, rng=None):
    """B = 3: rollout i carries golden state x[i] at every knot; U = 0, or seeded torques inside the soft torque limits"""
    X = np.repeat(c["x"][:, None, :], N + 1, axis=1)
    U = np.zeros((3, N, 19)) if rng is None else rng.uniform(-0.5, 0.5, (3, N, 19)) * sc.CTRLRANGE
    return X, U


SINGLE = cc.single_term_problems(cc.cost_golden(), N=N)


@pytest.mark.parametrize("case", SINGLE, ids=[lab for lab, _, _ in SINGLE])
def test_each_task_term_alone_against_torch_autograd(case):
    label, prob, names = case
    c = cc.cost_golden()
    X, U = _golden_trajectory(c)
    s = _solver(3, N=N)
    got, cost = _gpu_cost_stage(s, prob, X, U)
    s.close()
    worst = {}
    for i in range(3):
        g = sum(c["grad_" + n][i] for n in names)
        H = sum(c["hess_" + n][i] for n in names)
        eg, eH = np.abs(got["lx"][i, 3] - g).max(), np.abs(got["lxx"][i, 3] - H).max()
        worst["golden grad"] = max(worst.get("golden grad", 0.0), eg / max(1.0, np.abs(g).max()))
        worst["golden hess"] = max(worst.get("golden hess", 0.0), eH / max(1.0, np.abs(H).max()))
        assert eg <= 1e-9 * max(1.0, np.abs(g).max()), (label, i, eg)
        assert eH <= 1e-9 * max(1.0, np.abs(H).max()), (label, i, eH)
    assert np.all(got["lu"] == 0.0) and np.all(got["luu"] == 0.0)
    for i in range(3):                                                # the term is live on the device, in every rollout
        if label == "upright" and np.array_equal(X[i, 0, 3:7], [1.0, 0.0, 0.0, 0.0]):
            # golden state 0 is exactly upright: the residual, and with it the gradient, is 0 there; the curvature is not
            assert i == 0 and np.abs(got["lxx"][i, :N]).max() > 1e-3
        else:
            assert np.abs(got["lx"][i, :N]).max(axis=1).min() > 1e-3, (label, i)
    _check_against_oracle(prob, X, U, got, cost, worst, label)
    _report("term %s alone" % label, worst)


def test_everything_off_is_exactly_zero():
    c = cc.cost_golden()
    X, U = _golden_trajectory(c, np.random.default_rng(2))
    prob = cc.golden_problem(c, N=N)
    prob["com_vel_ref"][:] = c["ref_comvel"]; prob["stance"][0, 1::2, 1] = 0; prob["stance"][0, 2, :] = 0
    s = _solver(3, N=N)
    got, cost = _gpu_cost_stage(s, prob, X, U)
    s.close()
    for n in NAMES:
        assert not np.isnan(got[n]).any() and np.all(got[n] == 0.0), n
    assert not np.isnan(cost).any() and np.all(cost == 0.0)


@pytest.mark.parametrize("off", cc.TASK_KEYS)
def test_one_task_weight_off_the_rest_shipped(off):
    """The off side of every `weight > 0.0` branch with the other terms live.  W_com_vel ships as 0, so besides the shipped weights
    the same case runs with W_com_vel = 3 (the value test_gpu_parity.py switches it on with): the CoM-velocity slot is then live
    whenever it is not the term that is off.  Stance rows 11 / 10 / 00 / 01 / 11, so the foot terms and the support point take
    every branch; seeded torques and the golden states keep both soft penalties quiet or active as they fall."""
    c = cc.cost_golden()
    X, U = _golden_trajectory(c, np.random.default_rng(3))
    stance = np.array([[1, 1], [1, 0], [0, 0], [0, 1], [1, 1]], dtype=np.int32)
    worst = {}
    s = _solver(3, N=N)
    for w_com_vel in (sc.SHIPPED_CONFIG["W_com_vel"], 3.0):
        cfg = dict(sc.SHIPPED_CONFIG); cfg["W_com_vel"] = w_com_vel; cfg[off] = 0.0
        prob = sc.make_problem(ol.reference_kinematics, N=N, cfg=cfg, stance=stance)
        prob["com_vel_ref"][:] = c["ref_comvel"]
        assert prob["task_weights"][cc.TASK_KEYS.index(off)] == 0.0
        got, cost = _gpu_cost_stage(s, prob, X, U)
        _check_against_oracle(prob, X, U, got, cost, worst, (off, w_com_vel))
    s.close()
    _report("%s off" % off, worst)


@pytest.mark.parametrize("tracking_only", [False, True], ids=["all_terms", "tracking_only"])
def test_scrambled_problem_stage_by_stage(tracking_only):
    B = 5                                                             # odd: a wave of rollout pairs has a tail
    prob = cc.scrambled_problem(B, N, seed=11)
    if tracking_only:
        prob = cc.tracking_only(prob)
    o = _oracle(prob)
    x0, ui = sc.synthetic_batch(B, N, 11, o.grav_comp(sc.standing_state()))
    s = _solver(B, N=N); s.set_problem(prob)
    s.initialize(x0, ui)                                              # synthetic_batch states rolled out with its controls
    X, U = s.xbar(), s.ubar()
    got, cost = _gpu_cost_stage(s, prob, X, U)
    s.close()
    worst = {}
    _check_against_oracle(prob, X, U, got, cost, worst, "scrambled")
    for b in range(B):
        if tracking_only:
            for n, want in zip(NAMES, cc.tracking_closed_form(prob, b, X[b], U[b])[:4]):
                err = np.abs(got[n][b] - want).max()
                worst["closed form " + n] = max(worst.get("closed form " + n, 0.0), err / max(1.0, np.abs(want).max()))
                assert err <= 1e-10 * max(1.0, np.abs(want).max()), (n, b, err)
            want_cost = cc.tracking_closed_form(prob, b, X[b], U[b])[4]
            assert abs(cost[b] - want_cost) <= 1e-11 * abs(cost[b]), (b, cost[b], want_cost)
        # rollout b did not read set b + 1: the oracle fed that set, on the same trajectory, is far outside the tolerance
        o2 = _oracle(prob, (b + 1) % B); o2.set_trajectory(X[b], U[b]); o2.cost_quadratics()
        for n in ("lx", "lu"):
            other = o2.get(n)
            assert np.abs(got[n][b] - other).max() > 1e-3 * max(1.0, np.abs(other).max()), (n, b)
        assert abs(cost[b] - o2.total_cost()) > 1e-6 * abs(cost[b]), b
    _report("scrambled problem%s" % (" (tracking only)" if tracking_only else ""), worst)


def test_limit_sweep_every_row_and_side_of_both_tables():
    c = cc.cost_golden()
    jr, cr = c["jrange"], c["ctrlrange"]
    X, U, cases = cc.limit_sweep(N)
    B = len(cases)
    assert B == 76
    s = _solver(B, N=N)
    # (i) penalties alone: Q = Qf = R = 0, task weights 0 -- the records ARE the penalty part
    prob = cc.golden_problem(c, N=N)
    prob["w_joint"], prob["w_ctrl"] = 1300.0, 1700.0
    got, cost = _gpu_cost_stage(s, prob, X, U)
    worst = {}
    _check_against_oracle(prob, X, U, got, cost, worst, "penalties alone")
    diag = got["lxx"][:, :, np.arange(51), np.arange(51)]
    worst_pen = 0.0
    for r, (kind, j, side, v) in enumerate(cases):
        gx = np.zeros((N + 1, 51)); hx = np.zeros((N + 1, 51)); gu = np.zeros((N, 19)); hu = np.zeros((N, 19))
        gx[1, 7:26] = cc.pen_grad(X[r, 1, 7:26], jr, prob["w_joint"]); hx[1, 7:26] = cc.pen_hess(X[r, 1, 7:26], jr, prob["w_joint"])
        gu[1] = cc.pen_grad(U[r, 1], cr, prob["w_ctrl"]); hu[1] = cc.pen_hess(U[r, 1], cr, prob["w_ctrl"])
        assert np.count_nonzero(gx) + np.count_nonzero(gu) == 1 and np.count_nonzero(hx) + np.count_nonzero(hu) == 1
        for name, g_, want in (("lx", got["lx"][r], gx), ("lu", got["lu"][r], gu), ("lxx", diag[r], hx), ("luu", got["luu"][r], hu)):
            assert np.array_equal(g_ != 0.0, want != 0.0), (r, kind, j, side, name)      # every other entry exactly zero
            err = np.abs(g_ - want).max()                                                  # (= the error of the one active entry)
            worst_pen = max(worst_pen, err)
            assert err <= 1e-10, (r, kind, j, side, name, err)
        assert np.count_nonzero(got["lxx"][r]) == np.count_nonzero(hx)                     # nothing off the diagonal
        want_cost = cc.pen(X[r, 1, 7:26], jr, prob["w_joint"]) + cc.pen(U[r, 1], cr, prob["w_ctrl"])
        assert want_cost > 0 and abs(cost[r] - want_cost) <= 1e-11 * want_cost, (r, cost[r], want_cost)
    worst["closed form, active entry (absolute)"] = worst_pen
    # (ii) the same trajectories inside the scrambled problem: penalties beside every other term, per-rollout sets, B = 76
    prob = cc.scrambled_problem(B, N, seed=13)
    got, cost = _gpu_cost_stage(s, prob, X, U)
    _check_against_oracle(prob, X, U, got, cost, worst, "scrambled")
    s.close()
    _report("limit sweep", worst)


def _solve_case(contact, var, legacy):
    B = 4
    gravity = (0.0, 0.0, -9.81) if contact else None
    prob = cc.scrambled_problem(B, N, seed=17, gravity=gravity)
    o = _oracle(prob)
    x0, ui = sc.synthetic_batch(B, N, 17, o.grav_comp(sc.standing_state()))
    from mpc_ilqr_mujoco_amd import solver as sv
    with env(**var):
        s = _solver(B, N=N, legacy=legacy); s.set_problem(prob); s.set_contact_mode(contact); s.set_max_iterations(3)
        s.set_options(jacobian_mode=sv.JAC_ANALYTIC, early_exit=False)
        s.initialize(x0, ui)
        cost = s.solve(x0)
        tc, ta, tl = s.trace()
        K, kff, xb, ub, it, lam = s.gains_K(), s.gains_kff(), s.xbar(), s.ubar(), s.iterations(), s.lambdas()
        mism = s.adopt_mismatches()
        s.close()
    assert mism == 0
    worst = {}
    accepted = 0
    for b in range(B):
        ob = _oracle(prob, b, jac_mode=0, early_exit=0, max_iter=3); ob.set_contact_mode(contact)
        ob.initialize(x0[b], ui[b]); ok, c = ob.solve(x0[b])
        n, oc, oa, olam = ob.trace()
        for key, e in (("cost trace", np.abs(tc[b, : n + 1] / oc[: n + 1] - 1).max()), ("K", rel(K[b], ob.get("K"))), ("kff", rel(kff[b], ob.get("kff"))),
                       ("xbar", rel(xb[b], ob.get("xbar"))), ("ubar", rel(ub[b], ob.get("ubar")))):
            worst[key] = max(worst.get(key, 0.0), e)
        assert n == it[b] == 3, (b, n, it[b])
        assert np.allclose(tc[b, : n + 1], oc[: n + 1], rtol=1e-5, atol=0), (b, tc[b, : n + 1], oc[: n + 1])
        assert np.array_equal(ta[b, :n], oa[:n]) and np.allclose(tl[b, :n], olam[:n], rtol=1e-12), (b, ta[b], oa, tl[b], olam)
        assert abs(cost[b] - c) <= 1e-5 * abs(c)
        assert rel(K[b], ob.get("K")) < 1e-5 and rel(kff[b], ob.get("kff")) < 1e-5
        assert rel(xb[b], ob.get("xbar")) < 1e-5 and rel(ub[b], ob.get("ubar")) < 1e-5
        assert abs(lam[b] - ob.get_lambda()) < 1e-18
        accepted += int(np.count_nonzero(oa[:n]))
    assert accepted >= B                                              # the line search accepted steps: the candidate costs decided something
    _report("solve, contact mode %d, %s" % (contact, var or "default family"), worst)


@pytest.mark.parametrize("contact", [0, 2])
def test_scrambled_problem_through_a_solve(contact):
    """Three fixed iterations on the scrambled problem: what reaches the cost code inside the line-search, rollout and re-rollout
    kernels (their candidate costs decide the accepted step sizes the trace is compared on)."""
    _solve_case(contact, {}, legacy=False)


@pytest.mark.parametrize("contact", [0, 2])
def test_scrambled_problem_through_a_solve_on_the_lane_per_trajectory_family(contact):
    """The same under ILQR_BACKWARD=wg, ILQR_LS=r, ILQR_ROLLOUT=r (test library): those families carry their own candidate cost."""
    var = VARIANTS[1]
    assert (var["ILQR_BACKWARD"], var["ILQR_LS"], var["ILQR_ROLLOUT"]) == ("wg", "r", "r")
    _solve_case(contact, var, legacy=True)
