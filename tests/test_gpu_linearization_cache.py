"""The linearisation cache: an iteration re-linearises only the rollouts whose nominal trajectory the previous iteration changed.

A rollout whose two line searches of an iteration both fail keeps its nominal trajectory bit for bit (k_control copies nothing); its
A_t, B_t, lxx~_t, lx_t, lu_t, luu_t depend on that trajectory and on the problem data only, so the next iteration's primal dump, tangent
sweeps, kinematics record and cost quadratics would rewrite what the buffers hold.  With the cache (default) they run from the compacted
list of the rollouts that accepted a candidate; ilqr_hip_set_relinearize_unchanged / ILQR_RELIN=1 restores the full pass.  Every test
solves twice on fresh handles -- cache on, switch set -- and compares every observable bit for bit; ilqr_hip_get_linearized_rollouts is
compared with the count the comparison run's own trace gives."""
import os

import numpy as np
import pytest

from conftest import load_package

pytestmark = pytest.mark.gpu
pkg = load_package()
sc = pkg.scenario


class env:
    def __init__(self, **kv):
        self.kv = {k: v for k, v in kv.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _needs_legacy():
    e = os.environ
    return (e.get("ILQR_BACKWARD", "wave") not in ("wave", "wave-generic") or e.get("ILQR_LS", "s")[:1] != "s" or e.get("ILQR_ROLLOUT", "s")[:1] != "s"
            or e.get("ILQR_DYN", "")[:1] == "s" or e.get("ILQR_LINT", "0") == "1")


def _solver(B):
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv.BatchedILQR(B, lib_path=sv.LEGACY_LIB_PATH) if _needs_legacy() else sv.BatchedILQR(B)


def standing(B, seed, gravity=None):
    from mpc_ilqr_mujoco_amd import solver as sv
    prob = sc.make_problem(sv.reference_kinematics, N=25, gravity=gravity)
    ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
    x0, ui = sc.synthetic_batch(B, 25, seed, ug)
    return prob, x0, ui


NAMES = ("cost", "trace_cost", "trace_alpha", "trace_lambda", "iterations", "lambdas", "K", "kff", "Vx", "Vxx", "xbar", "ubar", "A", "Bm", "lx", "lu", "lxx", "luu")


def observables(s, cost):
    """Everything a caller can read after a solve (the getters of the Jacobians and quadratics convert layouts in place: last)."""
    tc, ta, tl = s.trace()
    Vx, Vxx = s.value_function()
    out = [cost, tc, ta, tl, s.iterations(), s.lambdas(), s.gains_K(), s.gains_kff(), Vx, Vxx, s.xbar(), s.ubar()]
    counters = dict(linearized=s.linearized_rollouts(), split=s.split_iterations(), spec=s.speculative_iterations(), adopt=s.adopt_mismatches(), enqueued=s.iterations_enqueued())
    out += list(s.linearization()) + list(s.quadratics())
    return dict(zip(NAMES, out)), counters


def solve_pair(B, prob, x0, ui, iters, early_exit=False, setup=None, jacobian_mode=0):
    """{relin: (observables, counters)} of the same solve on two fresh handles: cache on (False), ilqr_hip_set_relinearize_unchanged (True)."""
    out = {}
    for relin in (False, True):
        s = _solver(B); s.set_problem(prob)
        if setup:
            setup(s)
        s.set_options(jacobian_mode=jacobian_mode, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(iters)
        s.set_relinearize_unchanged(relin)
        s.initialize(x0, ui); cost = s.solve(x0)
        out[relin] = observables(s, cost)
        s.close()
    return out


def assert_same(a, b):
    for k in NAMES:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def counts_from_trace(ta):
    """(with the cache, with the switch under the convergence exit, iterations with both skipped and re-linearised rollouts): iteration 0
    takes every rollout; a later iteration the rollouts active in it (they have a trace entry), with the cache those of them whose
    previous iteration accepted a step (trace_alpha != 0)."""
    B, iters = ta.shape
    cached, active, mixed = B, B, []
    for i in range(1, iters):
        act = ~np.isnan(ta[:, i])
        keep, skip = act & (ta[:, i - 1] != 0.0), act & (ta[:, i - 1] == 0.0)
        cached += int(keep.sum()); active += int(act.sum())
        if keep.any() and skip.any():
            mixed.append(i)
    return cached, active, mixed


def check_pair(out, B, iters, early_exit=False, want_mix=True):
    (on, con), (off, coff) = out[False], out[True]
    assert_same(on, off)
    cached, active, mixed = counts_from_trace(off["trace_alpha"])
    print("linearized rollouts: cache %d, switch %d, expected %d / %d, mixed iterations %s" % (con["linearized"], coff["linearized"], cached, active if early_exit else B * iters, mixed))
    if want_mix:
        assert len(mixed) >= 2, mixed
    assert con["linearized"] == cached
    assert coff["linearized"] == (active if early_exit else B * iters)
    assert con["adopt"] == 0 and coff["adopt"] == 0
    return con, coff


@pytest.mark.parametrize("order", ["default", "sequential"])
def test_fixed_iterations_skip_the_unchanged_rollouts_bit_for_bit(order):
    """standing(12, seed=53), 10 fixed iterations (the batch of test_skipping_saturated_lambda_retries_changes_no_observable; the CPU oracle
    gives iterations with both kinds of rollouts for this seed).  `default`: B = 12 <= 512 takes the side-by-side order in every iteration
    (k_control_spec maintains the list too: DESIGN section 4); `sequential`: ILQR_SPEC=0, ILQR_SPLIT=0 (k_control phases 0 / 1, the order
    of the headline batch)."""
    B, iters = 12, 10
    prob, x0, ui = standing(B, 53)
    with env(**(dict(ILQR_SPEC="0", ILQR_SPLIT="0") if order == "sequential" else {})):
        out = solve_pair(B, prob, x0, ui, iters)
    con, coff = check_pair(out, B, iters)
    assert con["spec"] == coff["spec"] == (iters if order == "default" else 0)
    assert con["split"] == 0 and coff["split"] == 0


def test_convergence_exit_with_early_continuation_groups():
    """early_exit=True, ILQR_SPEC=0: the sequential order with the early-continuation groups A / R (on by default in this mode) -- group R's
    region runs over the retry rollouts whose retry accepted --, and the `continue` of iterations 0 / 1 behind a double failure."""
    B, iters = 12, 10
    prob, x0, ui = standing(B, 53)
    with env(ILQR_SPEC="0"):
        out = solve_pair(B, prob, x0, ui, iters, early_exit=True)
    con, coff = check_pair(out, B, iters, early_exit=True, want_mix=False)
    assert con["split"] > 0 and coff["split"] > 0
    assert con["linearized"] < coff["linearized"]      # (a double failure in iteration 0 or 1 does enter the next iteration)


def test_convergence_exit_default_orders():
    """early_exit=True as a caller gets it: B = 12 takes the side-by-side order, the gate stops enqueuing."""
    B, iters = 12, 10
    prob, x0, ui = standing(B, 53)
    out = solve_pair(B, prob, x0, ui, iters, early_exit=True)
    check_pair(out, B, iters, early_exit=True, want_mix=False)


CONTACT_SEED = 0
LIMITS_SEED = 0


def test_contact_mode_two_under_gravity():
    """k_lin_tangent2c: contact mode 2 under gravity -9.81, B = 8, 6 iterations."""
    B, iters = 8, 6
    prob, x0, ui = standing(B, CONTACT_SEED, gravity=(0.0, 0.0, -9.81))
    out = solve_pair(B, prob, x0, ui, iters, setup=lambda s: s.set_contact_mode(2))
    check_pair(out, B, iters)


def test_joint_limit_rows():
    """k_lin_primal_s<true>, k_lin_tangent2<., true>: the default plant with the joint-limit rows, B = 8, 6 iterations."""
    B, iters = 8, 6
    prob, x0, ui = standing(B, LIMITS_SEED)
    out = solve_pair(B, prob, x0, ui, iters, setup=lambda s: s.set_joint_limits(True))
    check_pair(out, B, iters)


def test_forward_differences_and_stage_calls_linearise_everything():
    """The forward-difference kernels select by S.active and use S.A / S.Bm as scratch: they keep the full pass (counter B x iterations in
    both switch states).  The stage API has no list: after a solve that skipped rollouts, stage_linearize / stage_cost_quadratics on
    another trajectory give what a fresh handle gives, for every rollout, and leave the last solve's count alone."""
    B, iters = 12, 10
    prob, x0, ui = standing(B, 53)
    with env(ILQR_SPEC="0", ILQR_SPLIT="0"):
        out = solve_pair(B, prob, x0, ui, iters, jacobian_mode=1)
    (on, con), (off, coff) = out[False], out[True]
    assert_same(on, off)
    assert con["linearized"] == B * iters and coff["linearized"] == B * iters
    _, x0b, uib = standing(B, 54)
    got = {}
    for name in ("solved", "fresh"):
        s = _solver(B); s.set_problem(prob); s.set_options(early_exit=False); s.set_max_iterations(iters)
        if name == "solved":
            s.initialize(x0, ui); s.solve(x0)
            n = s.linearized_rollouts()
            assert n < B * iters
        s.initialize(x0b, uib)
        s.set_trajectory(s.xbar(), s.ubar()); s.stage_linearize(); s.stage_cost_quadratics()
        got[name] = list(s.linearization()) + list(s.quadratics())
        if name == "solved":
            assert s.linearized_rollouts() == n
        s.close()
    for a, b in zip(got["solved"], got["fresh"]):
        assert np.array_equal(a, b, equal_nan=True)


def test_second_solve_on_a_handle_linearises_every_rollout_in_iteration_zero():
    """No list survives a solve: initialize with other inputs, solve -- bit for bit a fresh handle's solve of those inputs."""
    B, iters = 12, 10
    prob, x0, ui = standing(B, 53)
    _, x0b, uib = standing(B, 54)
    got = {}
    for name in ("reused", "fresh"):
        s = _solver(B); s.set_problem(prob); s.set_options(early_exit=False); s.set_max_iterations(iters)
        if name == "reused":
            s.initialize(x0, ui); s.solve(x0)
            assert s.linearized_rollouts() < B * iters
            s.set_regularization(1e-6)      # (lambda is state that survives a solve, as in the reference)
        s.initialize(x0b, uib); cost = s.solve(x0b)
        got[name] = observables(s, cost)
        s.close()
    assert_same(got["reused"][0], got["fresh"][0])
    cached, _, _ = counts_from_trace(got["fresh"][0]["trace_alpha"])
    assert got["reused"][1]["linearized"] == cached and got["fresh"][1]["linearized"] == cached


def test_weight_sets_keep_a_skipped_rollouts_own_quadratics():
    """Two weight sets over B = 8 (even / odd rollouts): a skipped rollout's quadratics stay those of its own set."""
    B, iters = 8, 10
    prob, x0, ui = standing(B, 53)
    prob = dict(prob)
    scale = np.where(np.arange(B) % 2 == 0, 1.0, 1.5)
    prob["Q"] = np.asarray(prob["Q"], dtype=np.float64)[None, :] * scale[:, None]
    prob["Qf"] = np.asarray(prob["Qf"], dtype=np.float64)[None, :] * scale[:, None]
    with env(ILQR_SPEC="0", ILQR_SPLIT="0"):
        out = solve_pair(B, prob, x0, ui, iters)
    con, coff = check_pair(out, B, iters, want_mix=False)
    assert con["linearized"] < B * iters
    on = out[False][0]
    # the terminal knot's lxx carries Qf of the rollout's own set on its diagonal: the two sets differ there
    d = np.einsum("bii->bi", on["lxx"][:, -1])
    assert not np.array_equal(d[0], d[1])
