"""Per-rollout weight sets without a GPU: the inputs of tests/weight_set_cases.py tell a kernel that reads the right record from one
that reads a neighbour's or an average (on the CPU oracle alone, so that test_gpu_weight_sets.py cannot pass vacuously), the solve of
that file's test 3 ends after different iteration counts in different rollouts (so that the compacted work lists are exercised), and
the host logic: which problem dicts install a table, what stack_weight_sets builds, the three exports and their argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
import weight_set_cases as wc
from conftest import load_package

pkg = load_package()
sc = wc.sc
N = 4


def _evaluate(prob, xs, us, weights_of):
    """(total cost [B], lx [B,N+1,51]) of the oracle: rollout b on reference set b under the weights of set weights_of(b)"""
    B = xs.shape[0]
    cost, lx = np.zeros(B), []
    for b in range(B):
        o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(weights_of(b), b)
        o.set_trajectory(xs[b], us[b]); o.cost_quadratics()
        cost[b] = o.total_cost(); lx.append(o.get("lx"))
    return cost, np.array(lx)


def _rolled_out(prob, B, seed):
    x0, ui = wc.start(prob, B, seed)
    o = wc.oracle_of_set(prob, 0)
    xs = np.zeros((B, prob["N"] + 1, 51))
    for b in range(B):
        o.initialize(x0[b], ui[b]); xs[b] = o.get("xbar")      # (the rollout reads no weight)
    return xs, ui


def test_weight_set_problem_is_what_it_says():
    for B in (3, 5, 6, 8):
        p = wc.weight_set_problem(B, N, 11)
        for key, n in (("Q", 51), ("R", 19), ("Qf", 51)):
            assert p[key].shape == (B, n) and np.all(p[key] > 0) and len(np.unique(p[key])) == B * n
        tw = p["task_weights"]
        assert tw.shape == (B, 6) and np.count_nonzero(tw == 0.0) == 2 and np.all(tw >= 0)
        assert [(b, k) for b, k in zip(*np.nonzero(tw == 0.0))] == sorted(wc.zeroed_task_weights(B))
        assert len(np.unique(tw[tw > 0])) == 6 * B - 2
        shipped = np.array([sc.SHIPPED_CONFIG[k] for k in wc.cc.TASK_KEYS]); shipped[1] = 3.0
        ratio = tw / shipped
        assert np.all((ratio == 0) | ((ratio >= 0.7) & (ratio <= 1.3)))
        for key, ship in (("w_joint", sc.SHIPPED_CONFIG["joint_limit_weight"]), ("w_ctrl", sc.SHIPPED_CONFIG["torque_limit_weight"])):
            assert p[key].shape == (B,) and len(np.unique(p[key])) == B and np.all(p[key] >= 0.7 * ship) and np.all(p[key] <= 1.3 * ship)
        Qs, _, _ = sc.build_cost_matrices(dict(sc.SHIPPED_CONFIG))
        nz = Qs > 0
        assert np.all(p["Q"][:, nz] / Qs[nz] <= 2.5) and np.all(p["Q"][:, nz] / Qs[nz] >= 0.4)
        one = wc.problem_of_set(p, B - 1)
        assert one["Q"].shape == (51,) and np.array_equal(one["Q"], p["Q"][B - 1]) and isinstance(one["w_joint"], float) and len(one["task_weights"]) == 6


@pytest.mark.parametrize("B,seed", [(5, 11), (wc.SOLVE_B, wc.SOLVE_SEED), (6, wc.SOLVE_SEED), (3, 29)])      # the problems of the GPU tests
def test_weight_sets_discriminate(B, seed):
    """Rollout b evaluated with the weights of set (b + 1) % B, or with the mean set, moves every rollout's total cost by more than
    1e-3 relative and every rollout's lx by more than 1e-3 max(1, |lx|) in max-norm."""
    prob = wc.weight_set_problem(B, N, seed)
    xs, us = _rolled_out(prob, B, seed)
    cost, lx = _evaluate(prob, xs, us, lambda b: wc.problem_of_set(prob, b))
    mean = wc.mean_set_problem(prob)
    for label, pick in (("set b + 1", lambda b: wc.problem_of_set(prob, b, weights_of=(b + 1) % B)), ("mean set", lambda b: mean)):
        c2, lx2 = _evaluate(prob, xs, us, pick)
        dc = np.abs(c2 - cost) / np.abs(cost)
        dg = np.array([np.abs(lx2[b] - lx[b]).max() / max(1.0, np.abs(lx[b]).max()) for b in range(B)])
        print("B = %d, %-9s: total cost differs by %.2e .. %.2e relative, lx by %.2e .. %.2e of max(1, |lx|)" % (B, label, dc.min(), dc.max(), dg.min(), dg.max()))
        assert dc.min() > 1e-3 and dg.min() > 1e-3, (label, dc, dg)


def test_solve_inputs_end_after_different_iteration_counts():
    """Test 3 of test_gpu_weight_sets.py with the convergence exit on: at least two distinct executed iteration counts across the
    rollouts, or the compacted work lists would hold every rollout in every pass and index nothing."""
    B = wc.SOLVE_B
    prob = wc.weight_set_problem(B, N, wc.SOLVE_SEED)
    x0, ui = wc.start(prob, B, wc.SOLVE_SEED)
    its = [wc.oracle_solve(prob, b, x0[b], ui[b], early_exit=True)[2] for b in range(B)]
    print("executed iterations per rollout:", its)
    assert len(set(its)) >= 2 and min(its) < wc.SOLVE_MAX_ITER, its


def test_set_problem_picks_the_table_and_broadcasts_what_is_shared():
    from mpc_ilqr_mujoco_amd import solver as sv
    B = 5
    prob = wc.weight_set_problem(B, N, 11)
    assert sv.weight_sets_of(wc.problem_of_set(prob, 2), B) is None                # an ordinary problem dict: shared weights
    base = sc.make_problem(ol.reference_kinematics, N=N)
    assert sv.weight_sets_of(base, B) is None and sv.weight_sets_of(base, 6) is None      # (six task weights are no axis of length B = 6)
    Q, R, Qf, tw, cw = sv.weight_sets_of(prob, B)
    assert np.array_equal(Q, prob["Q"]) and np.array_equal(R, prob["R"]) and np.array_equal(Qf, prob["Qf"]) and np.array_equal(tw, prob["task_weights"])
    assert np.array_equal(cw, np.stack([prob["w_joint"], prob["w_ctrl"]], axis=1))
    for key in wc.WEIGHT_KEYS:                                                      # one item per rollout, the rest shared
        p = wc.problem_of_set(prob, 0); p[key] = prob[key]
        got = dict(zip(("Q", "R", "Qf", "task_weights"), sv.weight_sets_of(p, B)[:4]))
        cwk = sv.weight_sets_of(p, B)[4]
        got["w_joint"], got["w_ctrl"] = cwk[:, 0], cwk[:, 1]
        for k2 in wc.WEIGHT_KEYS:
            want = prob[k2] if k2 == key else np.broadcast_to(np.asarray(wc.problem_of_set(prob, 0)[k2], dtype=np.float64), np.shape(prob[k2]))
            assert got[k2].shape == np.shape(prob[k2]) and np.array_equal(got[k2], want), (key, k2)
            assert all(a.flags["C_CONTIGUOUS"] for a in sv.weight_sets_of(p, B))    # (they go to the library as they are)
    bad = wc.problem_of_set(prob, 0); bad["Q"] = prob["Q"][:3]
    with pytest.raises(ValueError):
        sv.weight_sets_of(bad, B)


def test_stack_weight_sets_shapes():
    base = sc.make_problem(ol.reference_kinematics, N=N)
    sets = [{}, {"Q": 2.0 * base["Q"]}, {"task_weights": (1.0, 2.0, 3.0, 4.0, 5.0, 6.0), "w_ctrl": 7.0}]
    p = sc.stack_weight_sets(base, sets)
    assert p["Q"].shape == (3, 51) and p["R"].shape == (3, 19) and p["Qf"].shape == (3, 51) and p["task_weights"].shape == (3, 6)
    assert p["w_joint"].shape == (3,) and p["w_ctrl"].shape == (3,)
    assert np.array_equal(p["Q"][0], base["Q"]) and np.array_equal(p["Q"][1], 2.0 * base["Q"]) and np.array_equal(p["Q"][2], base["Q"])
    assert np.array_equal(p["task_weights"][0], base["task_weights"]) and np.array_equal(p["task_weights"][2], [1, 2, 3, 4, 5, 6])
    assert list(p["w_ctrl"]) == [base["w_ctrl"], base["w_ctrl"], 7.0] and list(p["w_joint"]) == [base["w_joint"]] * 3
    assert p["x_ref"] is base["x_ref"] and base["Q"].shape == (51,)                # the rest is shared, the base untouched
    with pytest.raises(KeyError):
        sc.stack_weight_sets(base, [{"gravity": (0, 0, -1)}])
    from mpc_ilqr_mujoco_amd import solver as sv
    assert [a.shape for a in sv.weight_sets_of(p, 3)] == [(3, 51), (3, 19), (3, 51), (3, 6), (3, 2)]


def test_library_exports_the_weight_set_entry_points_and_checks_arguments():
    from mpc_ilqr_mujoco_amd import solver as sv
    names = ("ilqr_hip_set_weight_sets", "ilqr_hip_clear_weight_sets", "ilqr_hip_num_weight_sets")
    for path in (sv.LIB_PATH, sv.LEGACY_LIB_PATH):
        L = sv.load_library(path)
        for n in names:
            assert n in sv.EXPORTS and hasattr(L, n), (path, n)
    L = sv.load_library()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ilqr_hip.h")).read()
    for n in names:
        assert n + "(" in hdr
    # without a handle there is no batch for n_sets to equal: ILQR_ERR_ARG whatever the count, and for a missing pointer (a count that
    # is neither 1 nor B on a live handle: test_table_takes_precedence_until_it_is_cleared, which needs a device)
    z = np.zeros(51 * 3)
    p = z.ctypes.data_as(C.POINTER(C.c_double))
    for n_sets in (0, 2, 3, -1, 1):
        assert L.ilqr_hip_set_weight_sets(None, p, p, p, p, p, n_sets) == 1
    assert L.ilqr_hip_set_weight_sets(None, None, p, p, p, p, 1) == 1
    assert L.ilqr_hip_clear_weight_sets(None) == 1 and L.ilqr_hip_num_weight_sets(None) == -1
