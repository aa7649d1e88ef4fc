"""Saturated lambda retries are skipped by default, and the retry's line search runs from its list through the device-side gate.

lambda is capped: lambda <- min(10 lambda, 1e-3).  A rollout at the cap whose first line search fails would retry at the same lambda, on the
Jacobians, quadratics and nominal trajectory of the pass that has just failed: the retry rewrites K, kff, Vx, Vxx, the candidates and their
costs with what is there and fails again.  k_control phase 0 plays its bookkeeping instead (ilqr_hip_set_dedup_saturated_retry, on by default;
set_dedup_saturated_retry(False) / ILQR_DEDUP_RETRY=0 restore the full retry).  The retries that are left run their line search from the
retry list, one rollout per wave where the list holds at most ILQR_LS_LIST_MAX rollouts (launch_line_search_gated).

Every comparison is bit for bit over lc.NAMES between fresh handles -- the default against the full retry --; what ran is read from
ilqr_hip_get_retry_pass_rollouts and compared with what the trace of the full-retry run predicts (retries_from_trace), and every test asserts
from that trace that its case occurred."""
import numpy as np
import pytest

import test_gpu_linearization_cache as lc
import test_gpu_work_lists as twl
import work_list_cases as wl

pytestmark = pytest.mark.gpu

SEQ = twl.SEQ
FX = twl.FX
LAMBDA_0, LAMBDA_MIN, LAMBDA_CAP = 1e-6, 1e-6, 1e-3      # a fresh handle's lambda (ilqr.cpp:16); the bounds of ilqr.cpp:634,646
DEFAULTS = twl.DEFAULTS


def retries_from_trace(lam0, alpha, lam):
    """(ran, saturated), two bool arrays [B, n], from the trace of a solve with the FULL retry and the lambda the handle held before it.

    lambda entering iteration i is the handle's at i = 0, else trace_lambda[i - 1] after a failure (alpha 0: the raised lambda stays) and
    max(trace_lambda[i - 1] / 2, 1e-6) after an acceptance.  The trace holds the lambda of the last executed pass: a retry ran iff the
    iteration failed or its lambda is not the one it was entered with; it repeated the first pass iff it failed at the cap.  An iteration
    without a trace entry (convergence exit) ran nothing."""
    alpha, lam = np.asarray(alpha, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    B, n = alpha.shape
    lam_in = np.empty((B, n))
    lam_in[:, 0] = lam0
    for i in range(1, n):
        lam_in[:, i] = np.where(alpha[:, i - 1] == 0.0, lam[:, i - 1], np.maximum(lam[:, i - 1] / 2.0, LAMBDA_MIN))
    act = ~np.isnan(alpha)
    ran = act & ((alpha == 0.0) | (lam != lam_in))
    saturated = act & (alpha == 0.0) & (lam_in == LAMBDA_CAP)
    return ran, saturated


def predicted_retries(lam0, obs):
    """(rollout-retries with the full retry, with the saturated ones skipped, saturated repeats per iteration, retry list length per iteration
    with the skip) of a solve, from the observables of its full-retry run"""
    ran, sat = retries_from_trace(lam0, obs["trace_alpha"], obs["trace_lambda"])
    assert not (sat & ~ran).any()
    return int(ran.sum()), int((ran & ~sat).sum()), sat.sum(axis=0).tolist(), (ran & ~sat).sum(axis=0).tolist()


def read(s, cost):
    """(observables, counters) with both pass counters (before the getters that convert layouts)"""
    first, retry = s.first_pass_rollouts(), s.retry_pass_rollouts()
    obs, counters = lc.observables(s, cost)
    counters["first_pass"], counters["retry_pass"] = first, retry
    return obs, counters


def solve(case, dedup, switches=DEFAULTS, **kw):
    """one cold solve on a fresh handle; dedup: None leaves the handle's default, else set_dedup_saturated_retry(dedup)"""
    s = twl.open_handle(case, switches, **kw)
    if dedup is not None:
        s.set_dedup_saturated_retry(dedup)
    s.initialize(case.x0, case.ui); cost = s.solve(case.x0)
    out = read(s, cost)
    s.close()
    return out


def check_default_against_full(on, off, lam0=LAMBDA_0, want_repeats=True):
    """on / off: (observables, counters) of the default and of the full retry.  -> (full, skipped, saturated per iteration, retry lists)"""
    lc.assert_same(on[0], off[0])
    pred = predicted_retries(lam0, off[0])
    full, skipped, sat, lists = pred
    print("retry rollouts: default %d, full %d; predicted %d / %d; saturated repeats %s; retry lists %s" % (on[1]["retry_pass"], off[1]["retry_pass"], skipped, full, sat, lists))
    assert off[1]["retry_pass"] == full and on[1]["retry_pass"] == skipped
    assert (full - skipped == sum(sat)) and ((sum(sat) > 0) if want_repeats else (sum(sat) == 0))
    assert on[1]["first_pass"] == off[1]["first_pass"] and on[1]["linearized"] == off[1]["linearized"]
    assert on[1]["adopt"] == 0 and off[1]["adopt"] == 0
    return pred


# ---- 1. the default ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq12():
    """standing(12, 53), 10 fixed iterations, sequential order: {name: (observables, counters)} of a handle with nothing set, one with
    set_dedup_saturated_retry(False) and one under ILQR_DEDUP_RETRY=0 -- shared, never modified"""
    case = wl.Case("standing12", *lc.standing(12, 53), iters=10, seed=53)
    out = {}
    with lc.env(**SEQ):
        out["default"] = solve(case, None)
        out["off"] = solve(case, False)
        with lc.env(ILQR_DEDUP_RETRY="0"):
            out["env_off"] = solve(case, None)
    return out


def test_saturated_retries_are_skipped_unless_switched_back_on(seq12):
    full, skipped, sat, lists = check_default_against_full(seq12["default"], seq12["off"])
    lc.assert_same(seq12["env_off"][0], seq12["off"][0])
    assert seq12["env_off"][1] == seq12["off"][1]
    for obs, counters in seq12.values():
        twl.assert_sequential(counters)
    assert skipped < full


# ---- 2. three control workgroups ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case40():
    return wl.standing40()


@pytest.fixture(scope="module")
def seq40(case40):
    """standing40, sequential order: {(dedup, (relin, repass)): (observables, counters)} -- shared, never modified"""
    with lc.env(**SEQ):
        return {(dedup, sw): solve(case40, dedup, sw) for dedup in (None, False) for sw in ((False, False), (False, True), (True, False), (True, True))}


FIXED0_REPEATS = [0, 0, 0, 0, 2, 18, 20, 28, 32, 37]      # saturated repeats per iteration of the fixture's standing40 / fixed0 trace


def test_three_workgroups_with_every_switch_combination(seq40):
    r = wl.fixture_run(FX, "standing40")
    assert retries_from_trace(LAMBDA_0, r["alpha"], r["lam"])[1].sum(axis=0).tolist() == FIXED0_REPEATS
    pred = twl.predicted("fixed0")
    ref = seq40[(False, DEFAULTS)][0]
    for sw in ((False, False), (False, True), (True, False), (True, True)):
        on, off = seq40[(None, sw)], seq40[(False, sw)]
        full, skipped, sat, lists = check_default_against_full(on, off)
        assert sat == FIXED0_REPEATS
        for obs, counters in (on, off):
            lc.assert_same(obs, ref)
            twl.check_counters(counters, sw, pred)
            twl.assert_sequential(counters)
    twl.assert_matches_fixture(seq40[(None, DEFAULTS)][0], r)


# ---- 3. later solves on one handle ----------------------------------------------------------------------------------------------------------
def _chain_step(hs, costs, lam0, run, want_repeats_at_0):
    out = {k: read(s, costs[k]) for k, s in hs.items()}
    full, skipped, sat, lists = check_default_against_full(out["default"], out["off"], lam0=lam0)
    assert np.array_equal(out["default"][0]["lambdas"], out["off"][0]["lambdas"])
    if want_repeats_at_0:      # a rollout enters the solve at the cap and fails at once: its skipped retry repeats the first pass of iteration 0
        assert sat[0] > 0, sat
    if run:
        twl.assert_matches_fixture(out["default"][0], wl.fixture_run(FX, "standing40", run))
    return out


@pytest.mark.parametrize("chain", ["warm1", "kick1"])
def test_warm_started_solves_enter_at_the_cap(case40, chain):
    """solve, then twice: the fixture's state one step on, initialize_warm_resident, solve -- what bench.py does.  lambda survives a solve:
    the later solves start with rollouts at the cap, whose iteration 0 fails on the shifted trajectory."""
    shift = wl.CHAINS[chain][0]
    xs = FX["standing40/%s_x" % chain]
    with lc.env(**SEQ):
        hs = {"default": twl.open_handle(case40, DEFAULTS), "off": twl.open_handle(case40, DEFAULTS)}
        hs["off"].set_dedup_saturated_retry(False)
        for step in range(wl.CHAIN_STEPS):
            costs, lam0 = {}, None
            for k, s in hs.items():
                if step == 0:
                    s.initialize(case40.x0, case40.ui)
                else:
                    s.initialize_warm_resident(xs[step], shift=shift)
                lam = s.lambdas()
                assert lam0 is None or np.array_equal(lam, lam0)
                lam0 = lam
                costs[k] = s.solve(xs[step])
            if step > 0:
                print("step %d: rollouts entering at the cap %d of %d" % (step + 1, int((lam0 == LAMBDA_CAP).sum()), case40.B))
                assert (lam0 == LAMBDA_CAP).sum() > 0
            _chain_step(hs, costs, lam0, "fixed0" if step == 0 else "%s_%d" % (chain, step), step > 0)
        for s in hs.values():
            s.close()


def test_a_trajectory_changed_from_outside_never_meets_a_skipped_pass(case40):
    """Three solves with initialize in between: the second and third start from the CONVERGED trajectories of another batch (standing(40, 54),
    solved three times on a handle of its own), with lambda at the cap from the first solve.  Iteration 0 fails for those rollouts, its retry
    is skipped, and the first pass of iteration 1 is skipped behind it: both rest on the first pass of iteration 0, which ran on the new
    trajectory -- bit for bit the handle that retries."""
    other = wl.Case("standing40b", *lc.standing(40, 54), iters=10, seed=54)
    with lc.env(**SEQ):
        s = twl.open_handle(other, DEFAULTS); s.set_dedup_saturated_retry(False)
        ub = other.ui
        for _ in range(3):
            s.initialize(other.x0, ub); s.solve(other.x0)
            ub = s.ubar()
        s.close()
        hs = {"default": twl.open_handle(case40, DEFAULTS), "off": twl.open_handle(case40, DEFAULTS)}
        hs["off"].set_dedup_saturated_retry(False)
        before = None
        for step, (x0, ui) in enumerate(((case40.x0, case40.ui), (other.x0, ub), (case40.x0, case40.ui))):
            costs, lam0 = {}, None
            for k, h in hs.items():
                h.initialize(x0, ui)
                lam0 = h.lambdas()
                if before is not None:
                    assert not np.array_equal(h.xbar(), before)
                costs[k] = h.solve(x0)
            out = _chain_step(hs, costs, lam0, None, step == 1)
            before = out["default"][0]["xbar"]
        for h in hs.values():
            h.close()


# ---- 4. the retry's line search through the gate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("list_max", ["0", "5", "16", None])
def test_retry_line_search_from_its_list_on_either_side_of_the_threshold(case40, seq40, list_max):
    """ILQR_LS_LIST_MAX = 0 (four per wave always), 5 and 16 (retry lists on both sides), default 1024 (one per wave always at B = 40)"""
    ref = seq40[(False, DEFAULTS)]
    lists = predicted_retries(LAMBDA_0, ref[0])[3]
    m = 1024 if list_max is None else int(list_max)
    small, large = [n for n in lists if 0 < n <= m], [n for n in lists if n > m]
    print("retry lists", lists, "one per wave", small, "four per wave", large)
    assert 0 in lists
    assert (large and not small) if m == 0 else (small and not large) if m == 1024 else (small and large)
    with lc.env(ILQR_LS_LIST_MAX=list_max, **SEQ):
        on = solve(case40, None)
    lc.assert_same(on[0], ref[0])
    assert on[1]["retry_pass"] == sum(lists)
    twl.assert_sequential(on[1])


# ---- 5. other plants and orders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["contact2", "weight_sets", "joint_limits"])
def test_modes_on_two_workgroups(name):
    case = wl.mode_case(name, wl.fixture_cases(FX)[name])
    r = wl.fixture_run(FX, name)
    want = retries_from_trace(LAMBDA_0, r["alpha"], r["lam"])[1].sum(axis=0).tolist()
    with lc.env(**SEQ):
        on, off = solve(case, None), solve(case, False)
    full, skipped, sat, lists = check_default_against_full(on, off)
    assert sat == want
    if name == "contact2":
        assert sat == [0, 0, 0, 0, 3, 3]
    twl.assert_matches_fixture(on[0], r, rollouts=(0, wl.GROUP))
    for obs, counters in (on, off):
        twl.assert_sequential(counters)


def test_convergence_exit_meets_no_saturated_retry(case40):
    """early_exit: a rollout leaves after its second double failure at the latest -- before lambda can reach the cap"""
    with lc.env(**SEQ):
        on, off = solve(case40, None, early_exit=True), solve(case40, False, early_exit=True)
    check_default_against_full(on, off, want_repeats=False)
    assert on[1] == off[1]
    twl.assert_matches_fixture(on[0], wl.fixture_run(FX, "standing40", "exit"))


def test_batch_slices_keep_no_lists(case40, seq40):
    """ILQR_SLICES=2 at B = 128 (standing40 tiled): no lists, every retry launch covers its slice -- the counter is batch x iterations, the
    results are those of the B = 40 handle rollout by rollout"""
    B = 128
    tile = np.arange(B) % 40
    with lc.env(ILQR_SLICES="2", **SEQ):
        s = twl.open_handle(case40, DEFAULTS, tile=tile)
        s.initialize(case40.x0[tile], case40.ui[tile]); cost = s.solve(case40.x0[tile])
        assert s.num_slices() == 2
        obs, counters = read(s, cost)
        s.close()
    assert counters["retry_pass"] == B * 10 and counters["first_pass"] == B * 10 and counters["adopt"] == 0
    ref = seq40[(False, DEFAULTS)][0]
    for k in lc.NAMES:
        assert np.array_equal(obs[k], ref[k][tile], equal_nan=True), k


def test_convergence_exit_from_the_sequential_to_the_side_by_side_order(case40):
    """ILQR_SPEC=1 ILQR_SPEC_MAX=6 ILQR_SPLIT=0, early_exit: sequential iterations, then both orders enqueued and the device takes one.  The
    counter adds the retry list where the sequential order ran and the active rollouts where the twin ran: at least the sequential
    order's count, and the same with and without the switch (no rollout reaches the cap)."""
    with lc.env(**SEQ):
        seq = solve(case40, False, early_exit=True)
    with lc.env(ILQR_SPEC="1", ILQR_SPEC_MAX="6", ILQR_SPLIT="0"):
        on, off = solve(case40, None, early_exit=True), solve(case40, False, early_exit=True)
    lc.assert_same(on[0], off[0]); lc.assert_same(on[0], seq[0])
    assert sum(predicted_retries(LAMBDA_0, off[0])[2]) == 0
    print("retry rollouts: dual orders %d, sequential %d; side-by-side iterations %d of %d" % (on[1]["retry_pass"], seq[1]["retry_pass"], on[1]["spec"], on[1]["enqueued"]))
    assert on[1] == off[1] and 0 < on[1]["spec"] < on[1]["enqueued"]
    assert seq[1]["retry_pass"] <= on[1]["retry_pass"] <= seq[1]["retry_pass"] + 6 * on[1]["spec"]      # (at most ILQR_SPEC_MAX go side by side)


def test_side_by_side_order_runs_every_twin_pass(seq12):
    """ILQR_SPEC=1 at B = 12: both passes of every iteration are in flight before either outcome is known -- nothing is skipped, the counter
    is the full count, and the results are those of the sequential order"""
    case = wl.Case("standing12", *lc.standing(12, 53), iters=10, seed=53)
    with lc.env(ILQR_SPEC="1", ILQR_SPLIT="0"):
        on, off = solve(case, None), solve(case, False)
    assert sum(predicted_retries(LAMBDA_0, seq12["off"][0])[2]) > 0
    for obs, counters in (on, off):
        lc.assert_same(obs, seq12["off"][0])
        assert counters["spec"] == 10 and counters["retry_pass"] == 12 * 10 and counters["first_pass"] == 12 * 10 and counters["adopt"] == 0
