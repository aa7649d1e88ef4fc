"""The linearisation cache and the first-pass skip on batches wider than one k_control workgroup.

k_control / k_control_spec build the lists both shortcuts run from (DevState::chg, chg_f, order): a workgroup handles 16 rollouts and makes
one atomicAdd per list, so positions inside a workgroup follow rollout order and positions across workgroups follow atomic order.  With
B <= 16 (every other test of the two shortcuts) there is one workgroup: no atomic races, every list is sorted, the cross-workgroup offsets
are all zero.  Here B = 40 (16 / 16 / 8), B = 24 (16 / 8), B = 128 and B = 1100, the last one in the configuration bench.py times: ten fixed
iterations, B > 512, no environment override.

Every comparison between device runs is bit for bit over lc.NAMES.  The reference of the decisions is the CPU oracle, through
golden/work_list_traces.npz (work_list_cases.py, test_work_lists_cpu.py): iteration count and alpha trace exact, lambda trace rtol 1e-12, cost
trace rtol 1e-5, final lambda within 1e-18 -- the bounds of test_gpu_parity.py --, and both counters (ilqr_hip_get_first_pass_rollouts,
ilqr_hip_get_linearized_rollouts) equal what work_list_cases.predicted_counts gives for the FIXTURE's traces.  Every test prints the list
lengths of its case and asserts from them that the case occurred."""
import os
import time

import numpy as np
import pytest

import test_gpu_linearization_cache as lc
import work_list_cases as wl

pytestmark = pytest.mark.gpu

SEQ = dict(ILQR_SPEC="0", ILQR_SPLIT="0")
ORDER_VARS = ("ILQR_SPEC", "ILQR_SPEC_MAX", "ILQR_SPLIT", "ILQR_LS_LIST_MAX", "ILQR_SLICES", "ILQR_RELIN", "ILQR_REPASS", "ILQR_EE_GATE")
FX = wl.load_fixture()
MODES = tuple(wl.fixture_cases(FX))
DEFAULTS, SWITCHES = (False, False), (True, True)      # (set_relinearize_unchanged, set_repeat_first_pass)


def _solver(B, N=wl.N):
    if N == wl.N:
        return lc._solver(B)
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv.BatchedILQR(B, N=N, lib_path=sv.LEGACY_LIB_PATH) if lc._needs_legacy() else sv.BatchedILQR(B, N=N)


def open_handle(case, switches, early_exit=False, jacobian_mode=0, setup=None, tile=None):
    """A fresh handle on the case's problem; tile: rollout indices of the case the handle's batch is made of."""
    B = case.B if tile is None else len(tile)
    s = _solver(B, case.prob["N"]); s.set_problem(case.prob)
    case.configure(s)
    if setup:
        setup(s)
    s.set_options(jacobian_mode=jacobian_mode, fd_eps=1e-5, early_exit=early_exit); s.set_max_iterations(case.iters)
    s.set_relinearize_unchanged(switches[0]); s.set_repeat_first_pass(switches[1])
    return s


def read(s, cost):
    first = s.first_pass_rollouts()
    obs, counters = lc.observables(s, cost)
    counters["first_pass"] = first
    return obs, counters


def solve(case, switches, tile=None, **kw):
    """(observables, counters) of one cold solve on a fresh handle"""
    s = open_handle(case, switches, tile=tile, **kw)
    x0, ui = (case.x0, case.ui) if tile is None else (case.x0[tile], case.ui[tile])
    s.initialize(x0, ui); cost = s.solve(x0)
    out = read(s, cost)
    s.close()
    return out


def assert_matches_fixture(obs, want, rollouts=None, tile=None):
    """device traces against the oracle's, with the bounds of test_gpu_parity.py; tile: device rollout j is the fixture's rollout tile[j]"""
    rows = np.arange(len(obs["iterations"])) if rollouts is None else np.asarray(rollouts)
    src = rows if tile is None else np.asarray(tile)[rows]
    it = want["it"][src]
    assert np.array_equal(obs["iterations"][rows], it), (obs["iterations"][rows], it)
    assert np.array_equal(obs["trace_alpha"][rows], want["alpha"][src], equal_nan=True)
    ran = np.arange(want["alpha"].shape[1])[None, :] < it[:, None]
    ran1 = np.arange(want["cost"].shape[1])[None, :] <= it[:, None]
    assert np.allclose(obs["trace_lambda"][rows][ran], want["lam"][src][ran], rtol=1e-12, atol=0)
    assert np.allclose(obs["trace_cost"][rows][ran1], want["cost"][src][ran1], rtol=1e-5, atol=0)
    assert np.isnan(obs["trace_cost"][rows][~ran1]).all()
    assert (np.abs(obs["lambdas"][rows] - want["lam_final"][src]) < 1e-18).all()


def predicted(run, early_exit=False, case="standing40", tile=None):
    r = wl.fixture_run(FX, case, run)
    a, it = (r["alpha"], r["it"]) if tile is None else (r["alpha"][tile], r["it"][tile])
    return wl.predicted_counts(a, it, early_exit)


def check_counters(counters, switches, pred):
    """each counter follows its own switch only, and equals the prediction from the fixture's traces"""
    skip, full, cache, relin = pred[:4]
    assert counters["linearized"] == (relin if switches[0] else cache), (switches, counters, pred)
    assert counters["first_pass"] == (full if switches[1] else skip), (switches, counters, pred)
    assert counters["adopt"] == 0


def assert_sequential(counters):
    assert counters["spec"] == 0 and counters["split"] == 0


# ---- a. three workgroups, sequential order ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case40():
    return wl.standing40()


@pytest.fixture(scope="module")
def seq40(case40):
    """standing40, 10 fixed iterations, sequential order: {(relin, repass): (observables, counters)} -- shared, never modified"""
    with lc.env(**SEQ):
        return {sw: solve(case40, sw) for sw in ((False, False), (False, True), (True, False), (True, True))}


@pytest.fixture(scope="module")
def exit40(case40):
    """the same batch with the convergence exit, sequential order without the split: {switches: (observables, counters)}"""
    with lc.env(**SEQ):
        return {sw: solve(case40, sw, early_exit=True) for sw in (DEFAULTS, SWITCHES)}


def test_three_workgroups_four_switch_combinations(seq40):
    pred = predicted("fixed0")
    r = wl.fixture_run(FX, "standing40")
    print("standing40 lists", pred[4], "iteration 5 per workgroup", wl.per_group(r["alpha"], r["it"], 5))
    mixed, spread = wl.occurrence(r["alpha"], r["it"])
    assert any(i in spread for i in mixed) and pred[0] < pred[1] and 0 in pred[4][1:]
    ref = seq40[DEFAULTS][0]
    for sw, (obs, counters) in seq40.items():
        lc.assert_same(obs, ref)
        check_counters(counters, sw, pred)
        assert_sequential(counters)
    assert pred[1] == 40 * 10
    assert_matches_fixture(ref, r)


def test_two_fresh_handles_with_the_same_settings_agree(case40, seq40):
    """the order of a list across workgroups is the order of their atomics and may differ from run to run: the results may not"""
    with lc.env(**SEQ):
        obs, counters = solve(case40, DEFAULTS)
    lc.assert_same(obs, seq40[DEFAULTS][0])
    assert counters == seq40[DEFAULTS][1]


@pytest.mark.parametrize("variant", ["list_max_0", "list_max_16", "list_max_5", "dedup", "side_by_side"])
def test_on_off_pair_under_other_line_search_thresholds_and_orders(case40, seq40, variant):
    lists = predicted("fixed0")[4][1:]
    kv, setup = dict(SEQ), None
    if variant.startswith("list_max"):
        # k_list_gate: a list of at most ILQR_LS_LIST_MAX rollouts takes the one-rollout-per-wave line search, a longer one four per wave
        m = int(variant.rsplit("_", 1)[1])
        kv["ILQR_LS_LIST_MAX"] = str(m)
        small, large = [n for n in lists if 0 < n <= m], [n for n in lists if n > m]
        print("lists", lists, "one per wave", small, "four per wave", large)
        assert large and (small or m == 0) and 0 in lists
        if m == 5:      # either kernel reads a list with entries of several workgroups (the list of 3: 1 / 2 / 0)
            r = wl.fixture_run(FX, "standing40")
            groups = [wl.per_group(r["alpha"], r["it"], i + 1) for i, n in enumerate(lists)]
            several = lambda g: sum(n > 0 for n in g) >= 2      # noqa: E731
            assert any(0 < sum(g) <= 5 and several(g) for g in groups) and any(sum(g) > 5 and min(g) > 0 for g in groups), groups
    elif variant == "dedup":
        setup = lambda s: s.set_dedup_saturated_retry(True)      # noqa: E731
    else:
        kv["ILQR_SPEC"] = "1"
    with lc.env(**kv):
        out = {sw: solve(case40, sw, setup=setup) for sw in (DEFAULTS, SWITCHES)}
    lc.assert_same(out[DEFAULTS][0], out[SWITCHES][0])
    pred = predicted("fixed0")
    for sw, (obs, counters) in out.items():
        if variant == "side_by_side":      # both passes side by side in every iteration: a full-pass counter, the cache still on
            assert counters["spec"] == 10 and counters["first_pass"] == 40 * 10 and counters["adopt"] == 0
            assert counters["linearized"] == (pred[3] if sw[0] else pred[2])
        else:
            check_counters(counters, sw, pred)
            assert_sequential(counters)
        assert_matches_fixture(obs, wl.fixture_run(FX, "standing40"))
        lc.assert_same(obs, seq40[DEFAULTS][0])


# ---- b. the configuration the benchmark times ------------------------------------------------------------------------------------------
def _groups(s, cost):
    """the observables of lc.NAMES in their order, a few at a time (the getters of the Jacobians and quadratics convert layouts in place: last)"""
    yield ("cost",), lambda: (cost,)
    yield ("trace_cost", "trace_alpha", "trace_lambda"), s.trace
    for name, fn in (("iterations", s.iterations), ("lambdas", s.lambdas), ("K", s.gains_K), ("kff", s.gains_kff)):
        yield (name,), (lambda fn=fn: (fn(),))
    yield ("Vx", "Vxx"), s.value_function
    yield ("xbar",), lambda: (s.xbar(),)
    yield ("ubar",), lambda: (s.ubar(),)
    yield ("A", "Bm"), s.linearization
    yield ("lx", "lu", "lxx", "luu"), s.quadratics


def test_benchmark_configuration_without_overrides(case40, seq40):
    """standing40 tiled to B = 1100 = 27 x 40 + 20 (69 workgroups), 10 fixed iterations, nothing set: the sequential order with the skip and
    the cache, launch_line_search_gated at its own threshold of 1024 with lists on either side of it and two empty ones.  Defaults against
    both switches, every rollout j against rollout j mod 40 of the B = 40 handle of (a), one array at a time."""
    t0 = time.time()
    assert not [v for v in ORDER_VARS if v in os.environ]
    B, iters = 1100, 10
    tile = np.arange(B) % 40
    pred = predicted("fixed0", tile=tile)
    lists = pred[4]
    print("B = 1100 lists", lists)
    # 27 whole copies of standing40's lists and the share of its first 20 rollouts (not exactly half of each list)
    whole, part = predicted("fixed0")[4], predicted("fixed0", tile=np.arange(20))[4]
    assert lists == [27 * w + p for w, p in zip(whole, part)] == [1100, 1100, 1044, 606, 551, 331, 221, 83, 0, 0]
    assert any(n > 1024 for n in lists[1:]) and any(0 < n <= 1024 for n in lists[1:]) and lists[1:].count(0) == 2
    hs = {}
    for sw in (DEFAULTS, SWITCHES):
        s = open_handle(case40, sw, tile=tile)
        s.initialize(case40.x0[tile], case40.ui[tile])
        hs[sw] = (s, s.solve(case40.x0[tile]))
    for sw, (s, _) in hs.items():
        counters = dict(first_pass=s.first_pass_rollouts(), linearized=s.linearized_rollouts(), adopt=s.adopt_mismatches(),
                        spec=s.speculative_iterations(), split=s.split_iterations())
        print(sw, counters)
        assert_sequential(counters)      # sequential order by default at this width ...
        check_counters(counters, sw, pred)
    assert hs[DEFAULTS][0].first_pass_rollouts() < B * iters      # ... and the skip with it
    ref = seq40[DEFAULTS][0]
    small = {}
    for (names, get_a), (_, get_b) in zip(_groups(*hs[DEFAULTS]), _groups(*hs[SWITCHES])):
        got_a, got_b = get_a(), get_b()
        for name, a, b in zip(names, got_a, got_b):
            assert np.array_equal(a, b, equal_nan=True), name
            for k in range(0, B, 40):      # rollout j + 40 k is rollout j, and rollouts 0..39 are the B = 40 handle's
                part = a[k:k + 40]
                assert np.array_equal(part, ref[name][:len(part)], equal_nan=True), (name, k)
            if name in ("trace_cost", "trace_alpha", "trace_lambda", "iterations", "lambdas"):
                small[name] = a
        del got_a, got_b
    assert_matches_fixture(small, wl.fixture_run(FX, "standing40"), tile=tile)
    for s, _ in hs.values():
        s.close()
    print("B = 1100: %.1f s" % (time.time() - t0))


# ---- c. repeated and warm-started solves -----------------------------------------------------------------------------------------------
def _step_checks(hs, costs, run, step):
    pred = predicted(run)
    out = {sw: read(hs[sw], costs[sw]) for sw in hs}
    lc.assert_same(out[DEFAULTS][0], out[SWITCHES][0])
    for sw, (obs, counters) in out.items():
        check_counters(counters, sw, pred)
        assert_sequential(counters)
    assert_matches_fixture(out[DEFAULTS][0], wl.fixture_run(FX, "standing40", run))
    print("step %d (%s): lists %s, first pass %d of %d" % (step + 1, run, pred[4], pred[0], pred[1]))
    if step > 0:
        assert pred[0] < pred[1] and out[DEFAULTS][1]["first_pass"] < out[SWITCHES][1]["first_pass"]      # the later steps skip something


def test_three_solves_on_one_handle_as_the_benchmark_steps(case40):
    """initialize(x0, ui) + solve three times: lambda carries over, no list does"""
    with lc.env(**SEQ):
        hs = {sw: open_handle(case40, sw) for sw in (DEFAULTS, SWITCHES)}
        for step in range(wl.CHAIN_STEPS):
            costs = {}
            for sw, s in hs.items():
                s.initialize(case40.x0, case40.ui); costs[sw] = s.solve(case40.x0)
            _step_checks(hs, costs, "fixed%d" % step, step)
        for s in hs.values():
            s.close()


@pytest.mark.parametrize("chain", list(wl.CHAINS))
def test_warm_started_mpc_steps(case40, chain):
    """solve, then twice: the state `shift` oracle steps along the control law (the fixture's), initialize_warm_resident, solve.  The
    undisturbed chains (warm1, warm2) start their later solves converged: every rollout fails both searches of iteration 0 and nine
    iterations run from empty lists.  kick1 moves the velocities between the solves: its later solves hold lists of every length again."""
    shift = wl.CHAINS[chain][0]
    xs = FX["standing40/%s_x" % chain]
    assert np.array_equal(xs[0], case40.x0)
    later = [predicted("%s_%d" % (chain, k))[4] for k in range(1, wl.CHAIN_STEPS)]
    if chain == "kick1":
        assert all(sum(0 < n < 40 for n in lists[1:]) >= 2 for lists in later), later
    else:
        assert all(set(lists[1:]) == {0} for lists in later), later
    with lc.env(**SEQ):
        hs = {sw: open_handle(case40, sw) for sw in (DEFAULTS, SWITCHES)}
        for step in range(wl.CHAIN_STEPS):
            costs = {}
            for sw, s in hs.items():
                if step == 0:
                    s.initialize(case40.x0, case40.ui)
                else:
                    s.initialize_warm_resident(xs[step], shift=shift)
                costs[sw] = s.solve(xs[step])
            _step_checks(hs, costs, "fixed0" if step == 0 else "%s_%d" % (chain, step), step)
        for s in hs.values():
            s.close()


# ---- d. modes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODES)
def test_modes_on_two_workgroups(name):
    case = wl.mode_case(name, wl.fixture_cases(FX)[name])
    r = wl.fixture_run(FX, name)
    pred = predicted("fixed0", case=name)
    mixed, spread = wl.occurrence(r["alpha"], r["it"])
    print("%s seed %d: lists %s, mixed iterations %s, lists from both workgroups %s" % (name, case.seed, pred[4], mixed, spread))
    assert any(i in spread for i in mixed) and pred[0] < pred[1]
    with lc.env(**SEQ):
        out = {sw: solve(case, sw) for sw in (DEFAULTS, SWITCHES)}
    lc.assert_same(out[DEFAULTS][0], out[SWITCHES][0])
    for sw, (obs, counters) in out.items():
        check_counters(counters, sw, pred)
        assert_sequential(counters)
    assert_matches_fixture(out[DEFAULTS][0], r, rollouts=(0, wl.GROUP))


# ---- e. orders that keep the full pass, and the convergence exit with the skip ---------------------------------------------------------
def test_convergence_exit_sequential_with_the_skip_and_the_host_bound(exit40):
    """ILQR_SPEC=0 ILQR_SPLIT=0, early_exit: the skip is on together with the bound the host hands the line searches (ls_bound)"""
    pred = predicted("exit", early_exit=True)
    r = wl.fixture_run(FX, "standing40", "exit")
    print("convergence exit: lists %s, iterations %s" % (pred[4], np.bincount(r["it"]).tolist()))
    assert pred[0] < pred[1]
    lc.assert_same(exit40[DEFAULTS][0], exit40[SWITCHES][0])
    for sw, (obs, counters) in exit40.items():
        check_counters(counters, sw, pred)
        assert_sequential(counters)
        assert 2 < counters["enqueued"] <= 10
    assert_matches_fixture(exit40[DEFAULTS][0], r)


def test_convergence_exit_with_the_default_split_keeps_the_full_pass(case40, exit40):
    """early_exit=True, ILQR_SPEC=0: the early-continuation groups are on, the skip is not; same results as the sequential order"""
    pred = predicted("exit", early_exit=True)
    with lc.env(ILQR_SPEC="0"):
        obs, counters = solve(case40, DEFAULTS, early_exit=True)
    assert counters["split"] > 0 and counters["spec"] == 0 and counters["adopt"] == 0
    assert counters["first_pass"] == pred[1] and counters["linearized"] == pred[2]
    lc.assert_same(obs, exit40[DEFAULTS][0])


def test_forward_differences_keep_the_full_pass(case40):
    """(the Jacobians differ from the analytic ones: the pair is compared with itself, not with (a))"""
    with lc.env(**SEQ):
        out = {sw: solve(case40, sw, jacobian_mode=1) for sw in (DEFAULTS, SWITCHES)}
    lc.assert_same(out[DEFAULTS][0], out[SWITCHES][0])
    for obs, counters in out.values():
        assert counters["first_pass"] == 40 * 10 and counters["linearized"] == 40 * 10 and counters["adopt"] == 0
        assert_sequential(counters)


def test_batch_slices_keep_the_full_pass(case40, seq40):
    """ILQR_SLICES=2 at B = 128 (standing40 tiled, two slices of 64): no lists, the full pass, the results of (a) rollout by rollout"""
    B = 128
    tile = np.arange(B) % 40
    with lc.env(ILQR_SLICES="2", **SEQ):
        s = open_handle(case40, DEFAULTS, tile=tile)
        s.initialize(case40.x0[tile], case40.ui[tile]); cost = s.solve(case40.x0[tile])
        assert s.num_slices() == 2
        obs, counters = read(s, cost)
        s.close()
    assert counters["first_pass"] == B * 10 and counters["linearized"] == B * 10 and counters["adopt"] == 0
    ref = seq40[DEFAULTS][0]
    for k in lc.NAMES:
        assert np.array_equal(obs[k], ref[k][tile], equal_nan=True), k


def test_convergence_exit_from_the_sequential_to_the_side_by_side_order(case40, exit40):
    """ILQR_SPEC=1 ILQR_SPEC_MAX=6 ILQR_SPLIT=0: 40 rollouts start sequential and listed; once the host's count is at most 4 x 6 both orders
    are enqueued and the device takes one, and at most 6 go side by side"""
    with lc.env(ILQR_SPEC="1", ILQR_SPEC_MAX="6", ILQR_SPLIT="0"):
        out = {sw: solve(case40, sw, early_exit=True) for sw in (DEFAULTS, SWITCHES)}
    lc.assert_same(out[DEFAULTS][0], out[SWITCHES][0])
    pred = predicted("exit", early_exit=True)
    for sw, (obs, counters) in out.items():
        print(sw, counters)
        assert 0 < counters["spec"] < counters["enqueued"] and counters["split"] == 0 and counters["adopt"] == 0
        lc.assert_same(obs, exit40[DEFAULTS][0])
    assert out[SWITCHES][1]["first_pass"] == pred[1]
    assert 40 < out[DEFAULTS][1]["first_pass"] < pred[1]
