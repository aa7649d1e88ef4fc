"""The listed side-by-side order: late iterations of a fixed-iteration solve run their two lambda passes side by side from their lists.

From iteration ILQR_SPEC_LIST_FROM on (1 in these tests), a fixed-iteration solve of a batch above ILQR_SPEC_MAX enqueues two orders per
iteration and the device takes one by 2 chg_n + kr_n <= ILQR_SPEC_LIST_MAX (k_listed_prologue): the sequential order from the lists, or -- side by side -- the first pass of the rollouts
on chg with their retry speculated into the twin, and the known retry of the rollouts on kr on the solve's own buffers (k_control_listed).
Every test compares every observable bit for bit (lc.NAMES) with the sequential order (ILQR_SPEC=0); the batches are small, so
ILQR_SPEC_MAX=0 keeps them out of the whole-batch side-by-side order and ILQR_SPEC_LIST_MAX moves the threshold into their list lengths.

What a rollout does in an iteration is read from the SEQUENTIAL run's traces (classify): chg = accepted in the previous iteration, kr = failed
twice there below the lambda cap, stuck = failed there at the cap.  The decisions of those runs are the CPU oracle's (golden/work_list_traces.npz,
test_gpu_work_lists.py).  Kinds inside side-by-side iterations, over the chain of test_chain_* and the contact batch of
test_contact_batch_*: a changed rollout whose first search accepts / fails and accepts in the twin / fails both, a known retry that accepts /
fails, a stuck rollout.  The seventh kind one could name -- a CHANGED rollout AT THE CAP that fails -- cannot occur: a rollout is on chg because
it accepted a candidate in the previous iteration, and acceptance leaves lambda = max(lambda_used / 2, 1e-6) <= 5e-4 < 1e-3 (ilqr.cpp:646);
k_control_listed still treats it as k_control does (the failing branch from S, the twin not read), and the tests assert it never shows up."""
import numpy as np
import pytest

import test_gpu_linearization_cache as lc
import test_gpu_saturated_retry_default as srd
import test_gpu_work_lists as twl
import work_list_cases as wl

pytestmark = pytest.mark.gpu

FX = twl.FX
DEFAULTS = twl.DEFAULTS
SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")
LST = dict(ILQR_SPEC_MAX="0", ILQR_SPLIT="0", ILQR_SPEC_LIST_FROM="1")      # (the pair of orders from iteration 1 on; default: 3 max_iter / 5)
FULL = dict(ILQR_SPEC_MAX="0", ILQR_SPLIT="0", ILQR_REPASS="1", ILQR_RELIN="1", ILQR_DEDUP_RETRY="0")      # every pass executes
SEQUENTIAL, LISTED = 0, 4      # ILQR_ORDER_SEQUENTIAL, ILQR_ORDER_LISTED_SPEC
LAMBDA_0, CAP = srd.LAMBDA_0, srd.LAMBDA_CAP
KINDS = ("first", "twin", "both", "kr_acc", "kr_fail", "stuck")


def classify(lam0, alpha, lam):
    """bool arrays [B, n] per (rollout, iteration) from the traces of a fixed-iteration solve and the lambda the handle held before it; column 0
    (the full first pass) is False everywhere except in ran / sat.  slots[i] = 2 chg_n + kr_n."""
    alpha, lam = np.asarray(alpha, dtype=np.float64), np.asarray(lam, dtype=np.float64)
    B, n = alpha.shape
    lam_in = np.empty((B, n)); lam_in[:, 0] = lam0
    for i in range(1, n):
        lam_in[:, i] = np.where(alpha[:, i - 1] == 0.0, lam[:, i - 1], np.maximum(lam[:, i - 1] / 2.0, 1e-6))
    later = np.zeros((B, n), dtype=bool); later[:, 1:] = True
    prev_acc = np.zeros((B, n), dtype=bool); prev_acc[:, 1:] = alpha[:, :-1] != 0.0
    capped = np.minimum(lam_in * 10.0, CAP) == lam_in
    acc = alpha != 0.0
    chg, kr, stuck = later & prev_acc, later & ~prev_acc & ~capped, later & ~prev_acc & capped
    ran, sat = srd.retries_from_trace(lam0, alpha, lam)
    k = dict(chg=chg, kr=kr, stuck=stuck, first=chg & acc & (lam == lam_in), twin=chg & acc & (lam != lam_in), both=chg & ~acc & ~capped,
             capfail=chg & ~acc & capped, kr_acc=kr & acc, kr_fail=kr & ~acc, retry_seq=ran & ~sat)
    k["slots"] = (2 * chg.sum(axis=0) + kr.sum(axis=0)).tolist()
    return k


def read(s, cost):
    """(observables, counters) with the order's own counters and the device lists (before the getters that convert layouts)"""
    extra = dict(first_pass=s.first_pass_rollouts(), retry_pass=s.retry_pass_rollouts(), listed=s.listed_spec_iterations(), orders=s.iteration_orders())
    try:
        extra["lists"] = [s.iteration_lists(i) for i in range(len(extra["orders"]))]
    except Exception:      # (no lists: batch slices, forward differences)
        extra["lists"] = None
    obs, counters = lc.observables(s, cost)
    counters.update(extra)
    return obs, counters


def solve(case, envs, tile=None, **kw):
    with lc.env(**envs):
        s = twl.open_handle(case, DEFAULTS, tile=tile, **kw)
        x0, ui = (case.x0, case.ui) if tile is None else (case.x0[tile], case.ui[tile])
        s.initialize(x0, ui); cost = s.solve(x0)
        out = read(s, cost)
        s.close()
    return out


def expected_orders(k, thr, n, start=1):
    return [LISTED if (i >= start and k["slots"][i] <= thr) else SEQUENTIAL for i in range(n)]


def check_against_sequential(on, seq, lam0, thr, kinds_seen=None, start=1):
    """on: the run under test, seq: the ILQR_SPEC=0 run.  Orders, lists and both pass counters of `on` follow from seq's traces."""
    lc.assert_same(on[0], seq[0])
    obs, c = on
    B, n = seq[0]["trace_alpha"].shape
    k = classify(lam0, seq[0]["trace_alpha"], seq[0]["trace_lambda"])
    assert not k["capfail"].any()      # (module docstring: cannot occur)
    want = expected_orders(k, thr, n, start)
    print("slots %s threshold %d orders %s; chg %s kr %s stuck %s" % (k["slots"], thr, c["orders"], k["chg"].sum(axis=0).tolist(), k["kr"].sum(axis=0).tolist(), k["stuck"].sum(axis=0).tolist()))
    assert c["orders"] == want and c["listed"] == want.count(LISTED)
    assert c["spec"] == 0 and c["split"] == 0 and c["adopt"] == 0 and seq[1]["adopt"] == 0 and seq[1]["listed"] == 0
    # the lists the device left: disjoint, and exactly the rollouts whose passes the sequential order runs
    for i in range(1, n):
        for run in (c, seq[1]):
            chg, kr = run["lists"][i]
            assert len(np.intersect1d(chg, kr)) == 0
            assert np.array_equal(chg, np.flatnonzero(k["chg"][:, i])) and np.array_equal(kr, np.flatnonzero(k["kr"][:, i])), (i, chg, kr)
        assert np.array_equal(k["kr"][:, i], k["retry_seq"][:, i] & ~k["chg"][:, i])      # kr = the retries of the sequential order that follow a skipped first pass
    # the counters: rollouts whose pass ran
    assert c["first_pass"] == seq[1]["first_pass"] == B + int(k["chg"][:, 1:].sum())
    retry = sum(int(k["chg"][:, i].sum() + k["kr"][:, i].sum()) if want[i] == LISTED else int(k["retry_seq"][:, i].sum()) for i in range(n))
    assert c["retry_pass"] == retry and seq[1]["retry_pass"] == int(k["retry_seq"].sum())
    if kinds_seen is not None:
        taken = np.array(want) == LISTED
        for name in KINDS:
            kinds_seen[name] = kinds_seen.get(name, 0) + int(k[name][:, taken].sum())
    return k, want


# ---- 1, 2, 8: a warm chain on three workgroups --------------------------------------------------------------------------------------------
CHAIN_THR = 30


def _chain(case40, envs, chain="kick1"):
    """[(observables, counters, lambda before the solve)] of the three solves of the chain on one handle"""
    shift = wl.CHAINS[chain][0]
    xs = FX["standing40/%s_x" % chain]
    out = []
    with lc.env(**envs):
        s = twl.open_handle(case40, DEFAULTS)
        for step in range(wl.CHAIN_STEPS):
            if step == 0:
                s.initialize(case40.x0, case40.ui)
            else:
                s.initialize_warm_resident(xs[step], shift=shift)
            lam0 = s.lambdas()
            cost = s.solve(xs[step])
            out.append(read(s, cost) + (lam0,))
        s.close()
    return out


@pytest.fixture(scope="module")
def case40():
    return wl.standing40()


@pytest.fixture(scope="module")
def chain40(case40):
    """kick1 chain of standing40 (B = 40: control workgroups of 16 / 16 / 8; 10 fixed iterations; solves 2 and 3 enter with rollouts at the cap):
    sequential, every pass executed, and the listed order at CHAIN_THR -- shared, never modified"""
    return dict(seq=_chain(case40, SEQ), full=_chain(case40, FULL), listed=_chain(case40, dict(LST, ILQR_SPEC_LIST_MAX=str(CHAIN_THR))))


def test_chain_of_three_solves_is_bit_identical_and_crosses_the_threshold(chain40):
    seen, listed_total = {}, 0
    for step in range(wl.CHAIN_STEPS):
        on, seq, full = chain40["listed"][step], chain40["seq"][step], chain40["full"][step]
        lam0 = seq[2]
        assert np.array_equal(on[2], lam0) and np.array_equal(full[2], lam0)
        if step > 0:
            assert (lam0 == CAP).sum() > 0      # rollouts enter at the cap
        lc.assert_same(on[0], full[0])
        assert full[1]["listed"] == 0 and full[1]["first_pass"] == 40 * 10
        k, want = check_against_sequential(on[:2], seq[:2], lam0, CHAIN_THR, seen)
        listed_total += on[1]["listed"]
        if step == 0:      # the threshold lies between two list lengths of this solve: sequential from the lists, then side by side
            assert any(want[i] == SEQUENTIAL and want[i + 1] == LISTED for i in range(1, 9)), want
        twl.assert_matches_fixture(on[0], wl.fixture_run(FX, "standing40", "fixed0" if step == 0 else "kick1_%d" % step))
    print("kinds inside side-by-side iterations:", seen)
    assert listed_total >= 3
    for name in ("first", "both", "kr_fail", "stuck"):
        assert seen[name] > 0, (name, seen)


# ---- 2 (the other kinds, and side by side -> sequential): contact mode 4 --------------------------------------------------------------------
@pytest.fixture(scope="module")
def contact4():
    case = wl.mode_case("contact4", wl.fixture_cases(FX)["contact4"])
    return case, solve(case, SEQ)


def test_contact_batch_accepts_in_the_twin_and_in_a_known_retry(contact4):
    """contact mode 4 under gravity, B = 24, every iteration >= 1 side by side (default threshold): lambda retries that ACCEPT -- of a changed rollout
    (the twin's gains, value function and candidate replace the first pass's) and of a known retry"""
    case, seq = contact4
    on = solve(case, LST)
    seen = {}
    k, want = check_against_sequential(on, seq, LAMBDA_0, 1024, seen)
    print("kinds:", seen)
    assert want[1:] == [LISTED] * (case.iters - 1)
    for name in ("first", "twin", "both", "kr_acc", "kr_fail", "stuck"):
        assert seen[name] > 0, (name, seen)
    twl.assert_matches_fixture(on[0], wl.fixture_run(FX, "contact4"), rollouts=(0, wl.GROUP))


def test_side_by_side_then_sequential_when_a_known_retry_accepts(contact4):
    """2 chg_n + kr_n only grows when a known retry accepts (its rollout moves from kr to chg).  The two rollouts of the contact batch that do so,
    alone, with the threshold between their list lengths: sequential from the lists -> side by side -> sequential from the lists."""
    case, seq24 = contact4
    k24 = classify(LAMBDA_0, seq24[0]["trace_alpha"], seq24[0]["trace_lambda"])
    s24 = 2 * k24["chg"].astype(int) + k24["kr"].astype(int)
    tile = np.flatnonzero((np.diff(s24[:, 1:], axis=1) > 0).any(axis=1) & (s24[:, -1] > 0))
    assert len(tile) >= 2, tile
    tile = tile[:2]
    seq = solve(case, SEQ, tile=tile)
    for name in lc.NAMES:      # (batch invariance: the rollouts the batch held)
        assert np.array_equal(seq[0][name], seq24[0][name][tile], equal_nan=True), name
    k = classify(LAMBDA_0, seq[0]["trace_alpha"], seq[0]["trace_lambda"])
    thr = max(k["slots"][1:]) - 1
    on = solve(case, dict(LST, ILQR_SPEC_LIST_MAX=str(thr)), tile=tile)
    _, want = check_against_sequential(on, seq, LAMBDA_0, thr)
    pairs = list(zip(want[1:-1], want[2:]))
    assert (SEQUENTIAL, LISTED) in pairs and (LISTED, SEQUENTIAL) in pairs, want


# ---- 3: threshold edges ---------------------------------------------------------------------------------------------------------------------
def test_threshold_edges(case40, chain40):
    """ILQR_SPEC_LIST_MAX = 2 chg_n + kr_n of an iteration: taken; one less: not taken"""
    seq = chain40["seq"][0]
    k = classify(LAMBDA_0, seq[0]["trace_alpha"], seq[0]["trace_lambda"])
    i = 6
    assert k["slots"][i] < k["slots"][i - 1] and k["slots"][i + 1] < k["slots"][i], k["slots"]
    for thr, taken in ((k["slots"][i], True), (k["slots"][i] - 1, False)):
        on = solve(case40, dict(LST, ILQR_SPEC_LIST_MAX=str(thr)))
        _, want = check_against_sequential(on, seq[:2], LAMBDA_0, thr)
        assert (want[i] == LISTED) == taken and want[i + 1] == LISTED and want[i - 1] == SEQUENTIAL


def test_default_start_iteration(case40, chain40):
    """without ILQR_SPEC_LIST_FROM the pair of orders is enqueued from iteration 3 max_iter / 5 = 6 on: the iterations before it stay sequential
    whatever their lists hold"""
    seq = chain40["seq"][0]
    envs = {k: v for k, v in LST.items() if k != "ILQR_SPEC_LIST_FROM"}
    on = solve(case40, envs)
    _, want = check_against_sequential(on, seq[:2], LAMBDA_0, 1024, start=6)
    assert want == [SEQUENTIAL] * 6 + [LISTED] * 4


# ---- 4: empty lists, one rollout, one workgroup plus one ----------------------------------------------------------------------------------------
def test_single_rollout_with_an_empty_changed_list_then_stuck(case40, chain40):
    seq40 = chain40["seq"][0]
    k40 = classify(LAMBDA_0, seq40[0]["trace_alpha"], seq40[0]["trace_lambda"])
    # a known retry in one iteration and stuck in the next: two consecutive double failures behind it
    cand = np.flatnonzero((k40["kr"][:, 1:-1] & k40["stuck"][:, 2:]).any(axis=1))
    assert cand.size, k40["slots"]
    tile = cand[:1]
    seq = solve(case40, SEQ, tile=tile)
    on = solve(case40, LST, tile=tile)
    k, want = check_against_sequential(on, seq, LAMBDA_0, 1024)
    assert want[1:] == [LISTED] * 9
    chg_n, kr_n = [len(l[0]) for l in on[1]["lists"]], [len(l[1]) for l in on[1]["lists"]]
    print("B = 1: chg", chg_n, "kr", kr_n)
    assert any(chg_n[i] == 0 and kr_n[i] == 1 and chg_n[i + 1] == 0 and kr_n[i + 1] == 0 for i in range(1, 9))
    for name in lc.NAMES:
        assert np.array_equal(on[0][name], seq40[0][name][tile], equal_nan=True), name


def test_one_workgroup_plus_one_rollout(case40, chain40):
    tile = np.arange(17)
    seq = solve(case40, SEQ, tile=tile)
    on = solve(case40, LST, tile=tile)
    _, want = check_against_sequential(on, seq, LAMBDA_0, 1024)
    assert want[1:] == [LISTED] * 9
    for name in lc.NAMES:
        assert np.array_equal(on[0][name], chain40["seq"][0][0][name][tile], equal_nan=True), name


# ---- 5: the lists (also asserted for every run above by check_against_sequential) -------------------------------------------------------------
def test_changed_and_known_retry_lists_are_disjoint_and_cover_the_sequential_passes(case40, chain40):
    seq = chain40["seq"][0]
    on = solve(case40, LST)
    k, want = check_against_sequential(on, seq[:2], LAMBDA_0, 1024)
    assert want[1:] == [LISTED] * 9
    for i in range(1, 10):
        chg, kr = on[1]["lists"][i]
        both = np.concatenate([chg, kr])
        assert len(np.unique(both)) == len(both)
        ran_seq = k["chg"][:, i] | k["retry_seq"][:, i]
        assert np.array_equal(np.sort(both), np.flatnonzero(ran_seq))
    assert sum(len(l[1]) for l in on[1]["lists"]) > 0 and sum(len(l[0]) for l in on[1]["lists"][1:]) > 0


# ---- 6: other modes ---------------------------------------------------------------------------------------------------------------------------
def _pair(case, thr=1024, tile=None, **kw):
    seq = solve(case, SEQ, tile=tile, **kw)
    on = solve(case, dict(LST, ILQR_SPEC_LIST_MAX=str(thr)), tile=tile, **kw)
    lc.assert_same(on[0], seq[0])
    n = seq[0]["trace_alpha"].shape[1]
    print("orders", on[1]["orders"], "listed", on[1]["listed"])
    assert on[1]["listed"] == n - 1 and seq[1]["listed"] == 0 and on[1]["adopt"] == 0 and on[1]["spec"] == 0
    return on, seq


def test_contact_mode_two_under_gravity():
    B = 8
    case = wl.Case("contact2x8", *lc.standing(B, lc.CONTACT_SEED, gravity=(0.0, 0.0, -9.81)), iters=6, plant=dict(contact=2))
    on, seq = _pair(case)
    check_against_sequential(on, seq, LAMBDA_0, 1024)


def test_two_weight_sets_select_candidate_costs_by_flags_on_the_twin():
    B = 8
    prob, x0, ui = lc.standing(B, 53)
    prob = dict(prob)
    scale = np.where(np.arange(B) % 2 == 0, 1.0, 1.5)
    prob["Q"] = np.asarray(prob["Q"], dtype=np.float64)[None, :] * scale[:, None]
    prob["Qf"] = np.asarray(prob["Qf"], dtype=np.float64)[None, :] * scale[:, None]
    on, seq = _pair(wl.Case("weights8", prob, x0, ui, iters=10))
    check_against_sequential(on, seq, LAMBDA_0, 1024)


def test_augmented_lagrangian_two_rounds():
    B = 8
    case = wl.Case("al8", *lc.standing(B, 53), iters=6)
    _pair(case, setup=lambda s: s.set_augmented_lagrangian(2, 1.0, 1.0))      # (counters and orders: of the last round)


def test_joint_limit_rows():
    case = wl.mode_case("joint_limits", wl.fixture_cases(FX)["joint_limits"])
    on, seq = _pair(case, tile=np.arange(8))
    check_against_sequential(on, seq, LAMBDA_0, 1024)


# ---- 7: where the order stays off -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["convergence_exit", "split", "forward_differences", "spec_off", "lists_off", "setter_off"])
def test_order_stays_off(case40, chain40, name):
    envs, kw, ref_kw = dict(LST), {}, None
    if name == "convergence_exit":
        kw = ref_kw = dict(early_exit=True)
    elif name == "split":
        envs["ILQR_SPLIT"] = "1"
    elif name == "forward_differences":
        kw = ref_kw = dict(jacobian_mode=1)
    elif name == "spec_off":
        envs = dict(SEQ)
    elif name == "lists_off":
        envs["ILQR_SPEC_LISTS"] = "0"
    elif name == "setter_off":
        kw = dict(setup=lambda s: s.set_listed_spec(False))
    ref = chain40["seq"][0][:2] if ref_kw is None else solve(case40, SEQ, **ref_kw)
    on = solve(case40, envs, **kw)
    lc.assert_same(on[0], ref[0])
    assert on[1]["listed"] == 0 and LISTED not in on[1]["orders"] and on[1]["adopt"] == 0
    assert on[1]["first_pass"] == ref[1]["first_pass"] or name == "split"      # (the split keeps the full first pass)


def test_batch_slices_keep_the_order_off(case40, chain40):
    B = 128
    tile = np.arange(B) % 40
    with lc.env(ILQR_SLICES="2", **LST):
        s = twl.open_handle(case40, DEFAULTS, tile=tile)
        s.initialize(case40.x0[tile], case40.ui[tile]); cost = s.solve(case40.x0[tile])
        assert s.num_slices() == 2
        obs, c = read(s, cost)
        s.close()
    assert c["listed"] == 0 and LISTED not in c["orders"] and c["adopt"] == 0
    ref = chain40["seq"][0][0]
    for name in lc.NAMES:
        assert np.array_equal(obs[name], ref[name][tile], equal_nan=True), name
