"""The fixture of the work-list tests (golden/work_list_traces.npz, golden/gen_work_list_golden.py) against the CPU oracle, and
work_list_cases.predicted_counts on hand-written traces.  test_gpu_work_lists.py compares device runs of batches wider than one k_control
workgroup with that fixture: it is only as good as the fixture is reproducible, decisive (no accept on a tie) and about the cases it claims
(iterations with listed and skipped rollouts, lists assembled from several workgroups)."""
import numpy as np
import pytest

import work_list_cases as wl


@pytest.fixture(scope="module")
def fx():
    return wl.load_fixture()


def _case(fx, name):
    return wl.standing40() if name == "standing40" else wl.mode_case(name, wl.fixture_cases(fx)[name])


def _checked(case):
    """two rollouts per case, one from the first workgroup and one from the last"""
    return (0, case.B - 1) if case.name == "standing40" else (0, wl.GROUP)


@pytest.fixture(scope="module")
def recomputed(fx):
    """{case: {rollout: {run: record}}} of the two checked rollouts of every case in the fixture, solved once on at most 16 threads"""
    jobs = [(name, b) for name in ("standing40",) + tuple(wl.fixture_cases(fx)) for b in _checked(_case(fx, name))]
    cases = {name: _case(fx, name) for name, _ in jobs}
    assert wl.threads() <= 16
    got = wl.pool_map(lambda j: wl.runs_of(cases[j[0]])(cases[j[0]], j[1]), jobs)
    out = {}
    for (name, b), (runs, xs) in zip(jobs, got):
        out.setdefault(name, {})[b] = (runs, xs)
    return cases, out


def test_the_fixture_holds_standing40_and_at_least_four_mode_cases(fx):
    held = wl.fixture_cases(fx)
    print("mode cases and seeds:", held, "left out:", [c for c in wl.MODE_CASES if c not in held])
    assert len(held) >= len(wl.MODE_CASES) - 2
    for run in wl.STANDING_RUNS:
        assert wl.fixture_run(fx, "standing40", run)["alpha"].shape == (40, 10)
    for chain in wl.CHAINS:
        assert fx["standing40/%s_x" % chain].shape == (wl.CHAIN_STEPS, 40, wl.NX)


def test_two_rollouts_of_every_case_recompute_exactly(fx, recomputed):
    cases, out = recomputed
    for name, per in out.items():
        for b, (runs, xs) in per.items():
            for run, rec in runs.items():
                want = wl.fixture_run(fx, name, run)
                for k in wl.TRACE_KEYS:
                    assert np.array_equal(rec[k], want[k][b], equal_nan=True), (name, b, run, k, rec[k], want[k][b])
            for chain, x in xs.items():
                assert np.array_equal(x, fx["%s/%s_x" % (name, chain)][:, b]), (name, b, chain)


def test_every_case_holds_mixed_iterations_and_lists_from_several_workgroups(fx):
    for name in ("standing40",) + tuple(wl.fixture_cases(fx)):
        r = wl.fixture_run(fx, name)
        mixed, spread = wl.occurrence(r["alpha"], r["it"])
        lists = wl.predicted_counts(r["alpha"], r["it"], False)[4]
        print("%-12s lists %s, mixed iterations %s, lists from several workgroups %s" % (name, lists, mixed, spread))
        assert mixed and spread and any(i in spread for i in mixed), (name, mixed, spread)
    r = wl.fixture_run(fx, "standing40")
    a, it = r["alpha"], r["it"]
    assert wl.predicted_counts(a, it, False)[4] == [40, 40, 38, 22, 20, 12, 8, 3, 0, 0]
    assert wl.per_group(a, it, 5) == [6, 4, 2]
    twice = ((a[:, :-1] == 0.0) & (a[:, 1:] == 0.0)).any(axis=1)      # two consecutive double failures: skipped behind a skipped pass
    assert twice.all()
    # every other solve of standing40 skips something too, and the convergence exit leaves rollouts of several lengths
    for run in wl.STANDING_RUNS[1:]:
        r = wl.fixture_run(fx, "standing40", run)
        skip, full = wl.predicted_counts(r["alpha"], r["it"], run == "exit")[:2]
        print("standing40 %-8s first-pass rollouts %d of %d" % (run, skip, full))
        assert skip < full, run
    assert len(set(wl.fixture_run(fx, "standing40", "exit")["it"].tolist())) > 1


def test_no_accept_decision_sits_on_a_tie(fx, recomputed):
    """x0 scaled by (1 +- 1e-9): the same iteration counts and alpha traces in every solve of the case -- two rollouts per case here, all 40
    of standing40 in the generator, which stores the outcome"""
    assert bool(fx["standing40/tie_free"])
    cases, out = recomputed
    jobs = [(name, b) for name, per in out.items() for b in per]
    free = wl.pool_map(lambda j: wl.tie_free(cases[j[0]], j[1], out[j[0]][j[1]][0]), jobs)
    assert all(free), [j for j, ok in zip(jobs, free) if not ok]


# ---- predicted_counts on hand-written traces ---------------------------------------------------------------------------------------------
NAN = float("nan")


def test_predicted_counts_fixed_iterations():
    alpha = np.array([[1.0, 0.0, 0.0, 0.5],      # accepts, fails twice in a row, accepts
                      [0.0, 0.0, 0.0, 0.0],      # never accepts: only iteration 0 takes it
                      [1.0, 1.0, 0.25, 0.0]])
    skip, full, cache, relin, lists = wl.predicted_counts(alpha, np.array([4, 4, 4]), False)
    assert lists == [3, 2, 1, 1]
    assert (skip, full, cache, relin) == (7, 12, 7, 12)
    assert wl.list_members(alpha, np.array([4, 4, 4]), 1).tolist() == [0, 2]
    assert wl.list_members(alpha, np.array([4, 4, 4]), 3).tolist() == [2]


def test_predicted_counts_convergence_exit():
    # rollout 0 converges in iteration 1 (accepted, then inactive: on no list); rollout 1 fails twice in iteration 0, continues, accepts,
    # fails in iteration 2 and ends; rollout 2 runs all four
    alpha = np.array([[1.0, 0.5, NAN, NAN],
                      [0.0, 1.0, 0.0, NAN],
                      [1.0, 0.0, 1.0, 1.0]])
    it = np.array([2, 3, 4])
    skip, full, cache, relin, lists = wl.predicted_counts(alpha, it, True)
    assert lists == [3, 2, 1, 1]      # iteration 1: rollouts 0, 2; iteration 2: rollout 1 (0 has left, 2 failed); iteration 3: rollout 2
    assert (skip, full) == (7, 3 + 3 + 2 + 1) and (cache, relin) == (skip, full)
    assert wl.list_members(alpha, it, 2).tolist() == [1]


def test_predicted_counts_refuses_traces_that_do_not_fit():
    with pytest.raises(AssertionError):
        wl.predicted_counts(np.ones((2, 3)), np.array([3, 2]), False)          # fixed iterations, one rollout short
    with pytest.raises(AssertionError):
        wl.predicted_counts(np.array([[NAN, 1.0]]), np.array([2]), True)       # active in iteration 1 without a trace entry in 0


def test_occurrence_and_per_group():
    alpha = np.zeros((40, 3)); it = np.full(40, 3)
    alpha[:, 0] = 1.0                      # iteration 1: everyone listed -- from three workgroups, but nothing skipped
    alpha[[3, 17, 39], 1] = 0.5            # iteration 2: three listed, one per workgroup
    mixed, spread = wl.occurrence(alpha, it)
    assert mixed == [2] and spread == [1, 2]
    assert wl.per_group(alpha, it, 1) == [16, 16, 8] and wl.per_group(alpha, it, 2) == [1, 1, 1]
    alpha[[17, 39], 1] = 0.0
    assert wl.occurrence(alpha, it) == ([2], [1])
