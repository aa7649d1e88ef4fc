"""The nominal re-rollout is not launched where the buffers already hold its result (solve_order.h nominal_roll; the default).

From iteration 1 on the nominal trajectory is the previous one or an accepted line-search candidate -- a rollout from x0 by the step
implementation the rollout kernel runs -- and S.Jbase its cost, summed in the rollout's order; behind a cold start the same holds for
iteration 0.  ilqr_hip_set_reroll_nominal / ILQR_REUSE_ROLLOUT=0 restores every rollout the reference executes, beside the linearisation
with adoption and mismatch count: the verification mode.  Every test solves on two fresh handles -- default, ILQR_REUSE_ROLLOUT=0 -- and
requires np.array_equal on every observable (lc.NAMES: cost, the three traces, iterations, lambda, gains, value function, trajectory,
Jacobians, quadratics) and on the work counters, adopt_mismatches() == 0 on the verifying handle, and nominal_rollouts() to be what the
rule says: nothing after iteration 0, and nothing in iteration 0 behind a cold start.

B = 40 (three k_control workgroups of 16 / 16 / 8), N = 6, 6 iterations.  A batch of 40 takes the whole-batch side-by-side order by
default; the other orders are reached through the environment as in test_gpu_first_pass_skip.py and test_gpu_listed_spec.py."""
import os

import numpy as np
import pytest

import test_gpu_linearization_cache as lc

pytestmark = pytest.mark.gpu
sc = lc.sc

B, N, ITERS = 40, 6, 6
EARTH = (0.0, 0.0, -9.81)
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TWIN = {}                                                                   # B <= ILQR_SPEC_MAX: both passes side by side in every iteration
SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")                                   # the order of the headline batch
SPLIT = dict(ILQR_SPEC="0")                                                 # with the convergence exit: early continuation in two groups
DUAL = dict(ILQR_SPEC_MAX="16")                                             # with the convergence exit and its gate: 16 < 40 <= 64, both orders enqueued
LISTED = dict(ILQR_SPEC_MAX="0", ILQR_SPLIT="0", ILQR_SPEC_LIST_FROM="1")   # a batch above ILQR_SPEC_MAX: the listed pair from iteration 1 on
VERIFY = dict(ILQR_REUSE_ROLLOUT="0")
COUNTERS = ("linearized", "first_pass", "retry_pass", "split", "spec", "listed", "enqueued", "orders")


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def standing(seed, gravity=None):
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=gravity)
    ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
    x0, ui = sc.synthetic_batch(B, N, seed, ug)
    return prob, x0, ui


def open_handle(prob, early_exit=False, setup=None):
    s = _sv().BatchedILQR(B, N=N, dt=prob["dt"]); s.set_problem(prob)
    if setup:
        setup(s)
    s.set_options(jacobian_mode=0, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(ITERS)
    return s


def read(s, cost):
    """(observables, counters) of the last solve; the counters first (the getters of the Jacobians and quadratics convert layouts in place)"""
    extra = dict(first_pass=s.first_pass_rollouts(), retry_pass=s.retry_pass_rollouts(), listed=s.listed_spec_iterations(), orders=s.iteration_orders(),
                 nominal=s.nominal_rollouts())
    obs, counters = lc.observables(s, cost)
    counters.update(extra)
    return obs, counters


def solve_pair(prob, x0, ui, envs, early_exit=False, setup=None, new_x0=False, verify=None):
    """{verifying: (observables, counters)}: initialize + solve on a fresh handle each.  new_x0: solve(x0) hands the state over again, so
    iteration 0 rolls out first as behind a warm start; else the cold start stands.  verify: how the second handle is told to re-roll."""
    out = {}
    for verifying in (False, True):
        with lc.env(**envs, **(VERIFY if verifying and verify is None else {})):
            s = open_handle(prob, early_exit, setup)
            if verifying and verify is not None:
                verify(s)
            s.initialize(x0, ui)
            cost = s.solve(x0) if new_x0 else s.solve()
            out[verifying] = read(s, cost)
            s.close()
    return out


def assert_pair(on, off, rounds=1, new_x0=False):
    """on: the default handle, off: the verifying one"""
    (obs, c), (ref, cref) = on, off
    lc.assert_same(obs, ref)
    for k in COUNTERS:
        assert c[k] == cref[k], (k, c[k], cref[k])
    assert cref["adopt"] == 0 and c["adopt"] == 0
    ta = ref["trace_alpha"]
    print("nominal rollouts: default %d, verifying %d; iterations enqueued %d; orders %s; split %d; accepted per iteration %s"
          % (c["nominal"], cref["nominal"], cref["enqueued"], cref["orders"], cref["split"], (np.nan_to_num(ta) != 0.0).sum(axis=0).tolist()))
    assert (np.nan_to_num(ta[:, 1:]) != 0.0).any()                          # an iteration >= 1 started from an accepted candidate
    # the default: iteration 0 alone, and only where the trajectory is not a cold start; rounds >= 2 start from the trajectory the round before left
    assert c["nominal"] == (B if new_x0 else 0)
    # the verification mode: every iteration enqueued, in every round (`enqueued` is the last round's: fixed iterations where rounds > 1); an
    # iteration that runs in two groups launches once per group, each launch over the batch with the group's flags -- and with the convergence
    # exit the last iteration may have enqueued a group A for an iteration the host then never enqueued
    launches = (cref["enqueued"] + cref["split"]) * rounds
    assert B * launches <= cref["nominal"] <= B * (launches + (1 if cref["split"] else 0))


@pytest.fixture(scope="module")
def batch():
    return standing(53)


@pytest.mark.parametrize("name, envs, early_exit", [
    ("twin", TWIN, False), ("sequential", SEQ, False), ("listed", LISTED, False),
    ("twin_exit", TWIN, True), ("sequential_exit", SEQ, True), ("split_exit", SPLIT, True), ("dual_exit", DUAL, True)])
def test_every_order_computes_what_the_re_roll_computes(batch, name, envs, early_exit):
    prob, x0, ui = batch
    out = solve_pair(prob, x0, ui, envs, early_exit)
    assert_pair(out[False], out[True])
    c = out[False][1]
    if name == "listed":
        assert c["listed"] > 0 and 4 in c["orders"]                         # ILQR_ORDER_LISTED_SPEC
    if name.startswith("twin"):
        assert c["spec"] == c["enqueued"]
    if name.startswith("sequential"):
        assert c["spec"] == 0 and c["split"] == 0 and c["listed"] == 0
    if name == "split_exit":
        assert c["split"] > 0                                               # the split did not switch itself off with the re-roll
    if name == "dual_exit":
        assert any(o in (2, 3) for o in c["orders"])                        # ILQR_ORDER_DUAL_*


def test_new_state_rolls_out_in_front_of_iteration_0_only(batch):
    """solve(x0): the trajectory is no longer known to be a rollout from x0 -- iteration 0 rolls out first, as the reference does"""
    prob, x0, ui = batch
    for envs in (TWIN, SEQ):
        out = solve_pair(prob, x0, ui, envs, new_x0=True)
        assert_pair(out[False], out[True], new_x0=True)


def test_setter_is_the_environment_switch(batch):
    prob, x0, ui = batch
    out = solve_pair(prob, x0, ui, SEQ, verify=lambda s: s.set_reroll_nominal(True))
    assert_pair(out[False], out[True])
    env = solve_pair(prob, x0, ui, SEQ)
    lc.assert_same(out[True][0], env[True][0])
    assert out[True][1]["nominal"] == env[True][1]["nominal"] == B * ITERS
    # the environment overrides the setter, either way
    with lc.env(ILQR_REUSE_ROLLOUT="1", **SEQ):
        s = open_handle(prob); s.set_reroll_nominal(True); s.initialize(x0, ui); s.solve()
        assert s.nominal_rollouts() == 0
        s.close()


def test_contact_mode_two_under_gravity():
    prob, x0, ui = standing(lc.CONTACT_SEED, gravity=EARTH)
    for envs in (TWIN, SEQ):
        out = solve_pair(prob, x0, ui, envs, setup=lambda s: s.set_contact_mode(2))
        assert_pair(out[False], out[True])


def test_joint_limit_rows(batch):
    """every other rollout starts with the left knee past its upper limit and moving out, every fourth also with the right elbow past its
    lower limit (the case of work_list_cases.py)"""
    prob, x0, ui = batch
    x0 = x0.copy()
    x0[1::2, 7 + 3] = 2.09; x0[1::2, 32 + 3] = 1.5
    x0[3::4, 7 + 18] = -1.29; x0[3::4, 32 + 18] = 0.1
    k = float(np.load(os.path.join(G, "joint_limit_stiffness_golden.npz"))["stiffness"])

    def setup(s):
        s.set_joint_limits(True); s.set_joint_limit_stiffness(k)
    for envs in (TWIN, SEQ):
        out = solve_pair(prob, x0, ui, envs, setup=setup)
        assert_pair(out[False], out[True])


def test_weight_sets(batch):
    prob, x0, ui = batch
    scale = (1.0, 1.5, 0.6)
    prob = sc.stack_weight_sets(prob, [dict(Q=prob["Q"] * scale[b % 3], Qf=prob["Qf"] * scale[b % 3]) for b in range(B)])
    for envs in (TWIN, SEQ):
        out = solve_pair(prob, x0, ui, envs)
        assert_pair(out[False], out[True])


@pytest.mark.parametrize("new_x0", [False, True])
def test_two_augmented_lagrangian_rounds(batch, new_x0):
    """round 2 starts from the trajectory round 1 left, under new multipliers: its baseline comes from the cost-only pass at the top of the round"""
    prob, x0, ui = batch
    w = prob["w_joint"]

    def setup(s):
        s.set_augmented_lagrangian(2, 2 * w, 2 * prob["w_ctrl"], margin=0.1)
    for envs in (TWIN, SEQ):
        pair = {}
        for verifying in (False, True):
            with lc.env(**envs, **(VERIFY if verifying else {})):
                s = open_handle(prob, setup=setup)
                s.initialize(x0, ui)
                cost = s.solve(x0) if new_x0 else s.solve()
                tr, mult = s.al_trace(), s.al_multipliers()
                pair[verifying] = read(s, cost) + (tr, mult)
                s.close()
        on, off = pair[False], pair[True]
        assert np.array_equal(on[2], off[2], equal_nan=True) and all(np.array_equal(a, b) for a, b in zip(on[3], off[3]))
        assert not np.isnan(off[2][1]).any()                                # round 2 ran
        assert off[1]["enqueued"] == ITERS
        assert_pair(on[:2], off[:2], rounds=2, new_x0=new_x0)


def test_warm_started_chain_rolls_out_before_iteration_0(batch):
    """three solves on one handle, the second and third warm-started from the resident solution behind a disturbed state: a shifted
    trajectory is no rollout from the new state, so iteration 0 of those solves rolls out in front of the region -- and nothing after it"""
    prob, x0, ui = batch
    rng = np.random.default_rng(7)
    kicks = [0.1 * rng.uniform(-1.0, 1.0, (B, 51 - 26)) for _ in range(2)]
    for envs in (TWIN, SEQ):
        chain = {}
        for verifying in (False, True):
            with lc.env(**envs, **(VERIFY if verifying else {})):
                s = open_handle(prob)
                s.initialize(x0, ui)
                steps = [read(s, s.solve())]
                for kick in kicks:
                    x = s.xbar()[:, 1].copy(); x[:, 26:] += kick
                    s.initialize_warm_resident(x)
                    steps.append(read(s, s.solve(x)))
                s.close()
            chain[verifying] = steps
        for step, (on, off) in enumerate(zip(chain[False], chain[True])):
            assert_pair(on, off, new_x0=step > 0)
