"""The first-pass skip: from iteration 1 on, the first backward pass, line search and candidate costs of the sequential order run only for
the rollouts that accepted a candidate in the previous iteration.

A rollout whose two line searches of iteration i both fail enters iteration i + 1 with its nominal trajectory, Jacobians, quadratics AND
lambda unchanged (the first pass of i + 1 runs at the lambda of the retry of i): the first pass would rewrite what its last executed pass
left in K, kff, Vx, Vxx, the candidates and their costs, and fail again.  ilqr_hip_set_repeat_first_pass / ILQR_REPASS=1 restores the full
first pass.  Every test solves on fresh handles -- default, switch set -- and compares every observable bit for bit (the pattern of
test_gpu_linearization_cache.py, whose helpers it uses); ilqr_hip_get_first_pass_rollouts is compared with the count the comparison run's
own trace gives, and every test asserts from that trace that the case it is about occurred.

The sequential order is the order of the headline batch (B = 4096 > ILQR_SPEC_MAX); a batch of 12 takes it under ILQR_SPEC=0, and without
the early-continuation groups (they keep the full pass) under ILQR_SPLIT=0."""
import numpy as np
import pytest

import test_gpu_linearization_cache as lc

pytestmark = pytest.mark.gpu

SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")


def solve(B, prob, x0, ui, iters, repass, early_exit=False, setup=None):
    """(observables, counters) of one solve on a fresh handle; repass: ilqr_hip_set_repeat_first_pass."""
    s = lc._solver(B); s.set_problem(prob)
    if setup:
        setup(s)
    s.set_options(jacobian_mode=0, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(iters)
    s.set_repeat_first_pass(repass)
    s.initialize(x0, ui); cost = s.solve(x0)
    first = s.first_pass_rollouts()
    obs, counters = lc.observables(s, cost)
    counters["first_pass"] = first
    s.close()
    return obs, counters


def solve_pair(*a, **kw):
    return {repass: solve(*a, repass=repass, **kw) for repass in (False, True)}


def list_lengths(ta):
    """Per iteration i >= 1 (index i - 1): (rollouts on the first-pass list, rollouts active) from a trace -- a rollout active in i has a trace
    entry there; it is on the list if its iteration i - 1 accepted a step (trace_alpha != 0)."""
    out = []
    for i in range(1, ta.shape[1]):
        act = ~np.isnan(ta[:, i])
        out.append((int((act & (ta[:, i - 1] != 0.0)).sum()), int(act.sum())))
    return out


def check_pair(out, B, iters, early_exit=False, min_mixed=1):
    (on, con), (off, coff) = out[False], out[True]
    lc.assert_same(on, off)
    lens = list_lengths(off["trace_alpha"])
    mixed = [i + 1 for i, (n, a) in enumerate(lens) if 0 < n < a]
    skipped = sum(a - n for n, a in lens)
    expect_on, expect_off = B + sum(n for n, _ in lens), B + sum(a for _, a in lens)
    print("first-pass rollouts: default %d, switch %d, expected %d / %d, list lengths %s, mixed iterations %s"
          % (con["first_pass"], coff["first_pass"], expect_on, expect_off, [n for n, _ in lens], mixed))
    assert len(mixed) >= min_mixed, mixed
    assert skipped > 0
    assert con["first_pass"] == expect_on
    assert coff["first_pass"] == expect_off
    if not early_exit:
        assert expect_off == B * iters
    assert con["adopt"] == 0 and coff["adopt"] == 0
    assert con["spec"] == coff["spec"] == 0 and con["split"] == coff["split"] == 0      # the sequential order, one group
    return on, lens


@pytest.fixture(scope="module")
def standing_fixed():
    """standing(12, seed=53), 10 fixed iterations, sequential order: {repass: (observables, counters)} -- shared, never modified."""
    B, iters = 12, 10
    prob, x0, ui = lc.standing(B, 53)
    with lc.env(**SEQ):
        out = solve_pair(B, prob, x0, ui, iters)
    return prob, x0, ui, out


def test_fixed_iterations_skip_the_repeated_first_pass_bit_for_bit(standing_fixed):
    """The batch of test_skipping_saturated_lambda_retries_changes_no_observable: consecutive double failures, and iterations that hold both
    skipped and executed rollouts."""
    check_pair(standing_fixed[3], 12, 10, min_mixed=2)


def test_convergence_exit_skips_behind_the_continue_of_iterations_0_and_1():
    """early_exit=True: a double failure ends a rollout from iteration 2 on, so only the `continue` of iterations 0 / 1 leaves a rollout that
    enters the next iteration unchanged -- iterations 1 and 2 are the only ones that can hold both kinds.  In this batch (CPU oracle) one
    rollout fails twice in iteration 1 and no rollout in iteration 0: iteration 2 is the one mixed iteration there can be, with a list of
    11 of 12, and that is what is asserted -- two, as in the fixed-iteration run, cannot occur."""
    B, iters = 12, 10
    prob, x0, ui = lc.standing(B, 53)
    with lc.env(**SEQ):
        out = solve_pair(B, prob, x0, ui, iters, early_exit=True)
    _, lens = check_pair(out, B, iters, early_exit=True, min_mixed=1)
    assert out[False][1]["first_pass"] < out[True][1]["first_pass"]
    assert lens[1][0] < lens[1][1]      # iteration 2


def test_list_threshold_sends_lists_to_both_line_search_kernels(standing_fixed):
    """ILQR_LS_LIST_MAX=4: a list of 1..4 rollouts takes the one-rollout-per-wave line search, a longer one the four-per-wave kernel, chosen
    on the device (k_list_gate); the default threshold (1024 >= B) sends every list of this batch to the former."""
    B, iters = 12, 10
    prob, x0, ui, ref = standing_fixed
    with lc.env(ILQR_LS_LIST_MAX="4", **SEQ):
        on, con = solve(B, prob, x0, ui, iters, repass=False)
    off, coff = ref[True]
    lc.assert_same(on, off)
    lens = [n for n, _ in list_lengths(off["trace_alpha"])]
    print("list lengths", lens)
    assert any(n > 4 for n in lens) and any(1 <= n <= 4 for n in lens), lens
    assert con["first_pass"] == B + sum(lens) and con["adopt"] == 0 and con["spec"] == 0
    lc.assert_same(on, ref[False][0])


def test_empty_first_pass_list(standing_fixed):
    """A rollout with two consecutive double failures, alone (B = 1): two iterations in a row have an empty first-pass list -- the launches
    find nothing to do, and the second of them relies on a retry that itself followed a skipped first pass."""
    iters = 10
    prob, x0, ui, ref = standing_fixed
    ta = ref[True][0]["trace_alpha"]
    twice = np.where(((ta[:, :-1] == 0.0) & (ta[:, 1:] == 0.0)).any(axis=1))[0]
    assert twice.size, ta
    b = int(twice[0])
    with lc.env(**SEQ):
        out = solve_pair(1, prob, x0[b:b + 1], ui[b:b + 1], iters)
    on, lens = check_pair(out, 1, iters, min_mixed=0)
    empty = [i + 1 for i, (n, a) in enumerate(lens) if n == 0 and a == 1]
    assert any(i + 1 in empty for i in empty), empty      # two consecutive iterations >= 1 with an empty list
    assert np.array_equal(on["trace_alpha"][0], ta[b], equal_nan=True)      # (batch invariance: the rollout the batch held)


def test_with_saturated_retries_deduplicated_a_stuck_rollout_costs_neither_pass():
    """ilqr_hip_set_dedup_saturated_retry on in both runs: a rollout at the lambda cap that fails takes no retry, and is not on the next
    first-pass list either -- the bookkeeping then reads the costs of the last pass that did run."""
    B, iters = 12, 10
    prob, x0, ui = lc.standing(B, 53)
    with lc.env(**SEQ):
        out = solve_pair(B, prob, x0, ui, iters, setup=lambda s: s.set_dedup_saturated_retry(True))
    on, _ = check_pair(out, B, iters)
    ta, tl = on["trace_alpha"], on["trace_lambda"]
    # failed in i - 1 (skipped in i) and failed in i at the cap (retry deduplicated): neither pass ran for it in iteration i
    stuck = (ta[:, :-1] == 0.0) & (ta[:, 1:] == 0.0) & (tl[:, 1:] == 1e-3) & (tl[:, :-1] == 1e-3)
    assert stuck.any(), (ta, tl)


def test_contact_mode_two_under_gravity():
    """Contact mode 2 under gravity -9.81 (k_line_search_s<1, .>), B = 8, 6 iterations."""
    B, iters = 8, 6
    prob, x0, ui = lc.standing(B, lc.CONTACT_SEED, gravity=(0.0, 0.0, -9.81))
    with lc.env(**SEQ):
        out = solve_pair(B, prob, x0, ui, iters, setup=lambda s: s.set_contact_mode(2))
    check_pair(out, B, iters)


def test_weight_sets_keep_a_skipped_rollouts_own_candidate_costs():
    """Two weight sets over B = 8 (k_traj_knot_cost<true> by flags): a skipped rollout's candidate costs stay those of its own set."""
    B, iters = 8, 10
    prob, x0, ui = lc.standing(B, 53)
    prob = dict(prob)
    scale = np.where(np.arange(B) % 2 == 0, 1.0, 1.5)
    prob["Q"] = np.asarray(prob["Q"], dtype=np.float64)[None, :] * scale[:, None]
    prob["Qf"] = np.asarray(prob["Qf"], dtype=np.float64)[None, :] * scale[:, None]
    with lc.env(**SEQ):
        out = solve_pair(B, prob, x0, ui, iters)
    check_pair(out, B, iters, min_mixed=0)


def test_side_by_side_order_is_left_alone_and_agrees(standing_fixed):
    """ILQR_SPEC=1 (the default of a batch of 12: both passes side by side in every iteration, full first pass) gives what the sequential
    order with the skip gives."""
    B, iters = 12, 10
    prob, x0, ui, ref = standing_fixed
    with lc.env(ILQR_SPEC="1", ILQR_SPLIT="0"):
        on, con = solve(B, prob, x0, ui, iters, repass=False)
    assert con["spec"] == iters and con["first_pass"] == B * iters and con["adopt"] == 0
    seq, cseq = ref[False]
    assert cseq["spec"] == 0 and cseq["first_pass"] < B * iters
    lc.assert_same(on, seq)
