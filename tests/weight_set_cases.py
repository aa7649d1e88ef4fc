"""Input builders for the per-rollout weight-set tests (test_weight_sets_cpu.py, test_gpu_weight_sets.py): scrambled_problem
(cost_envelope_cases.py) with a set of Q, R, Qf, task weights and limit weights per rollout, every entry its own draw, so that a
kernel that reads another rollout's record, the shared values or the compacted position of a rollout reads a different number.
NumPy and the oracle's host kinematics only; no GPU."""
import numpy as np

import cost_envelope_cases as cc
import oracle_lib as ol

sc = cc.sc
NX, NU = cc.NX, cc.NU
WEIGHT_KEYS = sc.WEIGHT_KEYS


def zeroed_task_weights(B):
    """[(set, task index)]: the two sets with one task weight exactly 0 -- the CoM-position term (a per-lane branch of k_quad_kin) in
    set 1 and the balance term (k_quad_kin, k_traj_knot_cost and the has_bal flag of the record) in the last set"""
    return [(1 % B, 0), (B - 1, 5)]


def weight_set_problem(B, N, seed):
    """scrambled_problem(B, N, seed) with per-rollout weights: Q [B,51], R [B,19], Qf [B,51] within a factor 2.5 of the shipped value,
    task_weights [B,6] and w_joint [B], w_ctrl [B] at 0.7 .. 1.3 of it, no two entries equal; two sets have one task weight exactly 0."""
    prob = cc.scrambled_problem(B, N, seed)
    rng = np.random.default_rng(seed + 7919)
    cfg = dict(sc.SHIPPED_CONFIG)
    Q, R, Qf = sc.build_cost_matrices(cfg)
    prob["Q"] = Q * np.exp(rng.uniform(-0.9, 0.9, (B, NX)))
    prob["R"] = R * np.exp(rng.uniform(-0.9, 0.9, (B, NU)))
    prob["Qf"] = Qf * np.exp(rng.uniform(-0.9, 0.9, (B, NX)))
    shipped = np.array([cfg[k] for k in cc.TASK_KEYS]); shipped[1] = 3.0      # (W_com_vel ships as 0: the value the parity tests switch it on with)
    tw = shipped * rng.uniform(0.7, 1.3, (B, 6))
    for b, k in zeroed_task_weights(B):
        tw[b, k] = 0.0
    prob["task_weights"] = tw
    prob["w_joint"] = cfg["joint_limit_weight"] * rng.uniform(0.7, 1.3, B)
    prob["w_ctrl"] = cfg["torque_limit_weight"] * rng.uniform(0.7, 1.3, B)
    return prob


def problem_of_set(prob, b, weights_of=None):
    """The 1-D problem of set b, for oracle_lib.Oracle.set_problem(p, b) or a shared-weights handle; weights_of: take the six weight
    items from that set instead (the references stay set b's: Oracle.set_problem picks them by its own argument)"""
    w = b if weights_of is None else weights_of
    p = dict(prob)
    p["Q"], p["R"], p["Qf"] = prob["Q"][w].copy(), prob["R"][w].copy(), prob["Qf"][w].copy()
    p["task_weights"] = tuple(float(v) for v in prob["task_weights"][w])
    p["w_joint"], p["w_ctrl"] = float(prob["w_joint"][w]), float(prob["w_ctrl"][w])
    return p


def mean_set_problem(prob):
    """every rollout under the mean of the B sets"""
    p = dict(prob)
    p["Q"], p["R"], p["Qf"] = prob["Q"].mean(0), prob["R"].mean(0), prob["Qf"].mean(0)
    p["task_weights"] = tuple(float(v) for v in prob["task_weights"].mean(0))
    p["w_joint"], p["w_ctrl"] = float(prob["w_joint"].mean()), float(prob["w_ctrl"].mean())
    return p


def one_set_arrays(p):
    """(Q [1,51], R [1,19], Qf [1,51], task [1,6], constraint [1,2]) of a shared-weights problem: the arguments of set_weight_sets"""
    return (np.asarray(p["Q"], dtype=np.float64)[None], np.asarray(p["R"], dtype=np.float64)[None], np.asarray(p["Qf"], dtype=np.float64)[None],
            np.asarray(p["task_weights"], dtype=np.float64)[None], np.array([[p["w_joint"], p["w_ctrl"]]], dtype=np.float64))


def oracle_of_set(prob, b, **opts):
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(problem_of_set(prob, b), b)
    if opts:
        o.set_options(**opts)
    return o


def start(prob, B, seed):
    """(x0 [B,51], u_init [B,N,19]) of synthetic_batch under the problem's gravity compensation"""
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(problem_of_set(prob, 0), 0)
    return sc.synthetic_batch(B, prob["N"], seed, o.grav_comp(sc.standing_state()))


# the solve of test_gpu_weight_sets.py (test 3): B = 8 sets, six iterations at most
SOLVE_B, SOLVE_SEED, SOLVE_MAX_ITER = 8, 23, 6


def oracle_solve(prob, b, x0, ui, early_exit, max_iter=SOLVE_MAX_ITER):
    """the oracle solving rollout b under its own set: (oracle, cost, executed iterations)"""
    o = oracle_of_set(prob, b, jac_mode=0, early_exit=int(early_exit), max_iter=max_iter)
    o.initialize(x0, ui)
    ok, c = o.solve(x0)
    return o, c, o.trace()[0]
