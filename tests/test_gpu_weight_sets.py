"""Per-rollout cost weight sets on the GPU (ilqr_hip_set_weight_sets; the WS instantiations of k_quad_kin, k_cost_quadratics and
k_traj_knot_cost): every rollout against the CPU oracle carrying that rollout's own set.  Inputs: tests/weight_set_cases.py, which
test_weight_sets_cpu.py shows to discriminate a wrong record.  N = 4 throughout.

Tolerances are those the suite already uses for the same quantities: 1e-10 max(1, |want|) on the quadratics and 1e-11 relative on the
total cost (test_gpu_cost_envelope.py / test_gpu_parity.py), 1e-5 on the cost trace, exact step sizes, 1e-12 on lambda and 1e-5 on the
gains and trajectories (test_full_solve_parity_trace_and_gains), 1e-9 on closed-loop states and 1e-8 on controls
(test_gpu_plant.py).  Every test prints the worst error it saw."""
import numpy as np
import pytest

import cost_envelope_cases as cc
import weight_set_cases as wc
from test_gpu_configs import _solver, env, rel

pytestmark = pytest.mark.gpu
sc = wc.sc
N = 4
NAMES = ("lx", "lu", "lxx", "luu")


def _stage(s, X, U):
    s.initialize(X[:, 0], U); s.set_trajectory(X, U)
    s.stage_cost_quadratics()
    return dict(zip(NAMES, s.quadratics())), s.stage_total_cost()


def _report(title, worst):
    print("%s: worst error: %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _check_quadratics(got, cost, want, c, b, worst, tag):
    for n in NAMES:
        err = np.abs(got[n][b] - want[n]).max()
        worst[n] = max(worst.get(n, 0.0), err / max(1.0, np.abs(want[n]).max()))
        assert err <= 1e-10 * max(1.0, np.abs(want[n]).max()), (tag, n, b, err)
    worst["cost"] = max(worst.get("cost", 0.0), abs(cost[b] - c) / abs(c))
    assert abs(cost[b] - c) <= 1e-11 * abs(c), (tag, b, cost[b], c)


@pytest.fixture(scope="module")
def stage_case():
    """B = 5 (odd: a wave of rollout pairs has a tail) on the rolled-out trajectory of synthetic_batch, and the oracle's records of
    every rollout under its own set -- computed once, shared, never modified"""
    B = 5
    prob = wc.weight_set_problem(B, N, 11)
    x0, ui = wc.start(prob, B, 11)
    s = _solver(B, N=N); s.set_problem(prob)
    s.initialize(x0, ui)
    X, U = s.xbar(), s.ubar()
    s.close()
    wants = []
    for b in range(B):
        o = wc.oracle_of_set(prob, b); o.set_trajectory(X[b], U[b]); o.cost_quadratics()
        wants.append(({n: o.get(n) for n in NAMES}, o.total_cost()))
    return prob, X, U, wants


def test_stage_by_stage_under_a_five_set_table(stage_case):
    prob, X, U, wants = stage_case
    B = X.shape[0]
    s = _solver(B, N=N); s.set_problem(prob)
    assert s.num_weight_sets() == B
    got, cost = _stage(s, X, U)
    worst = {}
    for b in range(B):
        _check_quadratics(got, cost, wants[b][0], wants[b][1], b, worst, "five sets")
    # every term off but tracking: the closed form with that set's weights
    trk = cc.tracking_only(prob)
    trk["task_weights"] = np.zeros((B, 6)); trk["w_joint"] = np.zeros(B); trk["w_ctrl"] = np.zeros(B)
    s.set_problem(trk)
    assert s.num_weight_sets() == B
    got, cost = _stage(s, X, U)
    s.close()
    exact = True
    for b in range(B):
        pb = wc.problem_of_set(trk, b)
        want = dict(zip(NAMES, cc.tracking_closed_form(pb, b, X[b], U[b])[:4]))
        c = cc.tracking_closed_form(pb, b, X[b], U[b])[4]
        w2 = {}
        _check_quadratics(got, cost, want, c, b, w2, "tracking only")
        for k, v in w2.items():
            worst["closed form " + k] = max(worst.get("closed form " + k, 0.0), v)
        exact = exact and all(np.array_equal(got[n][b], want[n]) for n in NAMES)
    _report("five-set table, stage by stage", worst)
    print("tracking-only quadratics equal their closed form exactly: %s" % exact)


def test_one_set_table_against_shared_weights(stage_case):
    prob, X, U, wants = stage_case
    B = X.shape[0]
    shared = wc.problem_of_set(prob, 2)
    for key in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        shared[key] = prob[key]
    s = _solver(B, N=N); s.set_problem(shared)
    assert s.num_weight_sets() == 0
    got0, cost0 = _stage(s, X, U)
    s.set_weight_sets(*wc.one_set_arrays(shared))
    assert s.num_weight_sets() == 1
    got1, cost1 = _stage(s, X, U)
    s.close()
    worst = {}
    for b in range(B):
        _check_quadratics(got1, cost1, {n: got0[n][b] for n in NAMES}, cost0[b], b, worst, "one set against shared")
    bitwise = all(np.array_equal(got0[n], got1[n]) for n in NAMES) and np.array_equal(cost0, cost1)
    _report("one-set table against shared weights", worst)
    print("one-set table and shared weights agree bit for bit: %s" % bitwise)
    # and the shared run itself is right (rollout 2 carries its own set there)
    _check_quadratics(got0, cost0, wants[2][0], wants[2][1], 2, {}, "shared")


def _solve_and_compare(B, seed, early_exit, rollouts=None, max_iter=wc.SOLVE_MAX_ITER, slices=None):
    prob = wc.weight_set_problem(B, N, seed)
    x0, ui = wc.start(prob, B, seed)
    from mpc_ilqr_mujoco_amd import solver as sv
    s = _solver(B, N=N); s.set_problem(prob); s.set_max_iterations(max_iter)
    assert s.num_weight_sets() == B
    if slices is not None:
        assert s.L.ilqr_hip_num_slices(s.h) == slices
    s.set_options(jacobian_mode=sv.JAC_ANALYTIC, early_exit=early_exit)
    s.initialize(x0, ui)
    cost = s.solve(x0)
    tc, ta, tl = s.trace()
    K, kff, xb, it, lam = s.gains_K(), s.gains_kff(), s.xbar(), s.iterations(), s.lambdas()
    mism = s.adopt_mismatches()
    s.close()
    assert mism == 0
    worst, its = {}, []
    for b in (range(B) if rollouts is None else rollouts):
        ob, c, n = wc.oracle_solve(prob, b, x0[b], ui[b], early_exit, max_iter)
        _, oc, oa, olam = ob.trace()
        its.append(n)
        for key, e in (("cost trace", np.abs(tc[b, : n + 1] / oc[: n + 1] - 1).max()), ("K", rel(K[b], ob.get("K"))), ("kff", rel(kff[b], ob.get("kff"))), ("xbar", rel(xb[b], ob.get("xbar")))):
            worst[key] = max(worst.get(key, 0.0), e)
        assert n == it[b], (b, n, it[b])
        assert np.allclose(tc[b, : n + 1], oc[: n + 1], rtol=1e-5, atol=0), (b, tc[b, : n + 1], oc[: n + 1])
        assert np.array_equal(ta[b, :n], oa[:n]) and np.allclose(tl[b, :n], olam[:n], rtol=1e-12), (b, ta[b], oa, tl[b], olam)
        assert abs(cost[b] - c) <= 1e-5 * abs(c)
        assert rel(K[b], ob.get("K")) < 1e-5 and rel(kff[b], ob.get("kff")) < 1e-5 and rel(xb[b], ob.get("xbar")) < 1e-5
        assert abs(lam[b] - ob.get_lambda()) < 1e-18
    return worst, its


@pytest.mark.parametrize("early_exit", [True, False], ids=["exit_on", "exit_off"])
def test_solves_under_eight_sets(early_exit):
    """exit_on is the leg that indexes the table through the compacted work lists (rollouts leave after different iteration counts)"""
    worst, its = _solve_and_compare(wc.SOLVE_B, wc.SOLVE_SEED, early_exit)
    if early_exit:
        assert len(set(its)) >= 2, its
    else:
        assert set(its) == {wc.SOLVE_MAX_ITER}, its
    _report("solve under eight sets, convergence exit %s, iterations %s" % ("on" if early_exit else "off", its), worst)


def test_batch_slices_read_their_own_rows():
    with env(ILQR_SLICES="2"):
        worst, its = _solve_and_compare(6, wc.SOLVE_SEED, False, rollouts=(3, 4, 5))
        _report("ILQR_SLICES=2, B = 6, rollouts 3-5", worst)
        # a batch of six is one slice (a slice is at least 64 rollouts): the same leg where the handle does cut the batch in two, with
        # rollouts of the second slice (and the first of each) against their own sets
        worst, its = _solve_and_compare(128, wc.SOLVE_SEED, False, rollouts=(0, 63, 64, 65, 127), max_iter=3, slices=2)
        _report("ILQR_SLICES=2, B = 128 (two slices of 64), rollouts 0, 63, 64, 65, 127", worst)


def test_table_takes_precedence_until_it_is_cleared(stage_case):
    prob, X, U, wants = stage_case
    B = X.shape[0]
    import ctypes as C
    s = _solver(B, N=N); s.set_problem(prob)
    counts = [s.num_weight_sets()]
    other = wc.problem_of_set(wc.weight_set_problem(B, N, 12), 1)
    s._chk(s.L.ilqr_hip_set_cost_weights(s.h, *[np.ascontiguousarray(other[k]).ctypes.data_as(C.POINTER(C.c_double)) for k in ("Q", "R", "Qf")]))
    s._chk(s.L.ilqr_hip_set_task_weights(s.h, *[C.c_double(v) for v in other["task_weights"]]))
    s._chk(s.L.ilqr_hip_set_constraint_weights(s.h, C.c_double(other["w_joint"]), C.c_double(other["w_ctrl"])))
    counts.append(s.num_weight_sets())
    # a count that is neither 1 nor B is refused by the library (the wrapper passes any count on) and leaves the table as it is
    from mpc_ilqr_mujoco_amd import solver as sv
    for n in (2, B + 1):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            s.set_weight_sets(*[np.repeat(a, n, axis=0) for a in wc.one_set_arrays(other)])
        assert s.num_weight_sets() == B
    got, cost = _stage(s, X, U)
    worst = {}
    for b in range(B):
        _check_quadratics(got, cost, wants[b][0], wants[b][1], b, worst, "table installed, shared setters called")
    s.clear_weight_sets()
    counts.append(s.num_weight_sets())
    got, cost = _stage(s, X, U)
    s.close()
    assert counts == [5, 5, 0], counts
    fresh = dict(other)
    for key in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        fresh[key] = prob[key]
    f = _solver(B, N=N); f.set_problem(fresh)
    got_f, cost_f = _stage(f, X, U)
    f.close()
    w2 = {}
    for b in range(B):
        _check_quadratics(got, cost, {n: got_f[n][b] for n in NAMES}, cost_f[b], b, w2, "cleared against a fresh shared handle")
    worst.update({"cleared, " + k: v for k, v in w2.items()})
    # ... and those are the OTHER values: far from set b's
    assert all(abs(cost[b] - wants[b][1]) > 1e-3 * abs(wants[b][1]) for b in range(B))
    _report("precedence", worst)


def test_scalar_family_refuses_weight_sets():
    from mpc_ilqr_mujoco_amd import solver as sv
    prob = wc.weight_set_problem(5, N, 11)
    with env(ILQR_DYN="s"):
        s = _solver(5, N=N, legacy=True)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            s.set_weight_sets(*sv.weight_sets_of(prob, 5))
        assert s.num_weight_sets() == 0
        s.close()


def test_closed_loop_runner_carries_the_sets():
    """MPCRunner hands the base problem's weights through problem_at: B = 3 under three sets against three B = 1 runners that carry
    the same sets as shared weights, on the resident plant (and the host path against the same yardstick)."""
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    from mpc_ilqr_mujoco_amd import solver as sv
    B, steps = 3, 3
    base1 = sc.make_problem(sv.reference_kinematics, N=N)
    wp = wc.weight_set_problem(B, N, 29)
    base = sc.stack_weight_sets(base1, [{k: wp[k][b] for k in wc.WEIGHT_KEYS} for b in range(B)])
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (40, 1))); rd.contact = np.ones((40, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 29, sv.gravity_compensation(sc.standing_state(), base1["gravity"]))

    def run(nb, problem, xs, us, resident):
        s = sv.BatchedILQR(nb, N=N, dt=base1["dt"]); s.set_max_iterations(3)
        r = ml.MPCRunner(s, rd, problem, resident=resident)
        out = r.run(xs, steps, u_init=us)
        n_sets = s.num_weight_sets()
        s.close()
        return out, n_sets

    singles = []
    for b in range(B):
        p1 = dict(base1); p1.update(wc.problem_of_set(base, b))
        (xs, us), n_sets = run(1, {k: p1[k] for k in base1}, x0[b:b + 1], ui[b:b + 1], True)
        assert n_sets == 0
        singles.append((xs[:, 0], us[:, 0]))
    worst = {}
    for resident in (True, False):
        (xs, us), n_sets = run(B, base, x0, ui, resident)
        assert n_sets == B and np.all(np.isfinite(xs))
        ex = max(np.abs(xs[:, b] - singles[b][0]).max() for b in range(B))
        eu = max(np.abs(us[:, b] - singles[b][1]).max() for b in range(B))
        tag = "resident" if resident else "host"
        worst[tag + " x"], worst[tag + " u"] = ex, eu
        assert ex <= 1e-9 and eu <= 1e-8, (tag, ex, eu)
    _report("closed loop, B = 3 under three sets against three B = 1 runners (absolute)", worst)
