"""The inputs of tests/solve_envelope_cases.py are fit for holding the Riccati and line-search kernels to the project's tolerances
(test_gpu_solve_envelope.py) -- shown on the CPU oracle and NumPy alone, so that the GPU tests cannot pass vacuously or fail on the
reference's own account:

  * the reference's spread (fp64 against long double, the oracle's backward pass against long double) lies at least a hundred times
    below the tolerance the GPU test applies to the same rollout;
  * natural data reaches every branch of the LLT-failure rule the GPU test is there for, and every branch decision is decisive;
  * a shift of luu at one knot puts three rollouts on the bumped branch, 5e-5 from either edge of its window, at a spread that still
    lies a hundred times below the 1e-6 they are held to;
  * over 16 rollouts x 3 scales every one of the eight alpha slots is the accepted one, one case is rejected, and every accept is decisive;
  * rounding in the gains moves the accepted candidate a hundred times less than the line-search tolerances;
  * at most two of sixteen rollouts are dropped for any of these reasons;
  * every mutant of the references -- the slips a kernel could make -- moves a checked output by a hundred times its tolerance.

Every test prints the figures it measured."""
import numpy as np
import pytest

import solve_envelope_cases as sv

NAMES = ("tame", "contact1", "contact2")
LS_NAMES = ("tame", "contact1")                  # mode 2 decides an active set per candidate: left out of the line search
FACTOR = 100.0
_memo = {}


def _inputs(name, i):
    q = sv.oracle_inputs(name)
    return [q[k][i] for k in ("A", "B", "lx", "lu", "lxx", "luu")]


def _riccati(name):
    """per rollout and scale: (long double, fp64, oracle) results on the oracle's inputs; kept [16]"""
    if ("riccati", name) in _memo:
        return _memo[("riccati", name)]
    prob, mode, X, U = sv.trajectories(name)
    o = sv.oracle_of(prob, mode)
    out, kept = {}, np.ones(sv.NS, dtype=bool)
    for i in range(sv.NS):
        A, B, lx, lu, lxx, luu = _inputs(name, i)
        for s in sv.SCALES:
            slx, slu = sv.scaled(lx, lu, s)
            ld = sv.riccati_ref_cached(A, B, slx, slu, lxx, luu)
            f64 = sv.riccati_ref_cached(A, B, slx, slu, lxx, luu, dtype=np.float64)
            o.set_trajectory(X[i], U[i]); o.set_linearization(A, B); o.set_quadratics(slx, slu, lxx, luu); o.backward_pass()
            orc = dict(K=o.get("K"), k=o.get("kff"), Vx=o.get("Vx"), Vxx=o.get("Vxx"))
            out[i, s] = (ld, f64, orc)
            kept[i] &= sv.branches_decisive(ld, f64)
    _memo[("riccati", name)] = (out, kept)
    return out, kept


def _line_search(name):
    """per rollout and scale: candidates_ref on the oracle's gains; kept [16]: every accept of the rollout is decisive"""
    if ("ls", name) in _memo:
        return _memo[("ls", name)]
    prob, mode, X, U = sv.trajectories(name)
    ric, _ = _riccati(name)
    o = sv.oracle_of(prob, mode)
    out, kept = {}, np.ones(sv.NS, dtype=bool)
    for i in range(sv.NS):
        for s in sv.SCALES:
            orc = ric[i, s][2]
            out[i, s] = sv.candidates_ref(o, X[i], U[i], orc["K"], orc["k"])
            kept[i] &= out[i, s]["decisive"]
    _memo[("ls", name)] = (out, kept)
    return out, kept


def _kept(name):
    kept = _riccati(name)[1].copy()
    if name in LS_NAMES:
        kept &= _line_search(name)[1]
    return kept


@pytest.mark.parametrize("name", NAMES)
def test_the_spread_of_the_reference_is_far_below_the_tolerances(name):
    ric, kept = _riccati(name)
    worst = {}
    for (i, s), (ld, f64, orc) in ric.items():
        if not kept[i]:
            continue
        tol = sv.riccati_tol(ld["branch"])
        for key in sv.RICCATI_KEYS:
            want = ld[key].astype(np.float64)
            for tag, got in (("fp64", f64[key]), ("oracle", orc[key])):
                e = sv.riccati_error(got, want)
                w = worst.setdefault((tag, key, tol), 0.0)
                worst[tag, key, tol] = max(w, e)
                assert FACTOR * e <= tol, (name, i, s, tag, key, e, tol)
    for (tag, key, tol), e in sorted(worst.items()):
        print("%s: %s against long double, %s (rollouts held to %.0e): worst error relative to max(1, |want|) %.2e" % (name, tag, key, tol, e))


def test_natural_data_reaches_every_branch_and_every_decision_is_decisive():
    lxx = sv.oracle_inputs("tame")["lxx"]
    eig = np.array([[np.linalg.eigvalsh(h).min() for h in r] for r in lxx])
    print("tame: smallest eigenvalue of lxx per rollout %.0f .. %.0f" % (eig.min(axis=1).max(), eig.min(axis=1).min()))
    assert (eig.min(axis=1) < -100.0).all()                                   # lxx itself is indefinite on natural data
    for name in NAMES:
        ric, kept = _riccati(name)
        branch = np.array([ric[i, 1][0]["branch"] for i in range(sv.NS)])
        pivot = np.array([ric[i, 1][0]["pivot"] for i in range(sv.NS)])
        ge = np.array([ric[i, 1][0]["ge_pivot"] for i in range(sv.NS)])
        for s in sv.SCALES[1:]:                                               # the scales multiply lx / lu only: the branches stay
            assert all(np.array_equal(ric[i, s][0]["branch"], branch[i]) for i in range(sv.NS))
        n2 = int((branch == 2).any(axis=1).sum())
        print("%s: knots on branch 0 / 1 / 2: %d / %d / %d; rollouts with an indefinite knot: %s; smallest |deciding pivot| / max diag %.2e; "
              "smallest pivot of the elimination %s; dropped as indecisive: %d"
              % (name, (branch == 0).sum(), (branch == 1).sum(), (branch == 2).sum(), np.flatnonzero((branch == 2).any(axis=1)).tolist(),
                 np.abs(pivot).min(), "%.3g" % np.nanmin(ge) if n2 else "-", (~kept).sum()))
        assert (~kept).sum() <= sv.MAX_DROPPED
        if name == "tame":
            assert int(((branch == 2).any(axis=1) & kept).sum()) >= 2
            assert ((branch == 0).all(axis=1) & kept).sum() >= 8              # and the 1e-9 tolerance has rollouts to apply to


def test_a_shifted_luu_diagonal_lands_on_the_bumped_branch_decisively():
    """solve_envelope_cases.bumped_luu(): the rollouts with an indefinite knot, with luu shifted at that one knot, take branch 1 there, in
    long double and fp64 alike, 5e-5 from either edge of the branch's window; the references' spread on them (gains of 1e6: the bumped
    Quu has an eigenvalue of 5e-5) stays a hundred times below the 1e-6 they are held to; and without the bump the gains are others"""
    ric, kept = _riccati("tame")
    n, worst, moved = 0, 0.0, np.inf
    for i in np.flatnonzero(kept):
        A, B, lx, lu, lxx, luu = _inputs("tame", i)
        luu2 = sv.bumped_luu(luu, ric[i, 1][0])
        if luu2 is None:
            continue
        ld = sv.riccati_ref(A, B, lx, lu, lxx, luu2)
        f64 = sv.riccati_ref(A, B, lx, lu, lxx, luu2, dtype=np.float64)
        t = int(np.flatnonzero(ric[i, 1][0]["branch"] == 2).max())
        assert ld["branch"][t] == 1 and np.array_equal(ld["branch"][t + 1:], ric[i, 1][0]["branch"][t + 1:]) and sv.branches_decisive(ld, f64), (i, ld["branch"])
        assert abs(ld["eig"][t] - sv.BUMPED_EIG) < 1e-3 * abs(sv.BUMPED_EIG)
        n += 1
        for key in sv.RICCATI_KEYS:
            worst = max(worst, sv.riccati_error(f64[key].astype(np.float64), ld[key].astype(np.float64)))
        m = sv.riccati_ref(A, B, lx, lu, lxx, luu2, mutant="no_bump")
        moved = min(moved, sv.riccati_error(m["K"].astype(np.float64), ld["K"].astype(np.float64)) / sv.TOL_BUMPED)
        print("rollout %d: knot %d on branch 1 (Quu eigenvalue %.3e, largest diagonal entry %.3g), branches %s, largest gain %.3g"
              % (i, t, ld["eig"][t], ld["diag"][t], ld["branch"], float(np.abs(ld["K"]).max())))
    print("shifted luu: %d rollouts on the bumped branch; fp64 against long double, worst error relative to max(1, |want|) %.2e; "
          "without the bump K moves by at least %.3g times the tolerance" % (n, worst, moved))
    assert n >= 2 and FACTOR * worst <= sv.TOL_BUMPED and moved >= FACTOR


@pytest.mark.parametrize("name", LS_NAMES)
def test_every_alpha_slot_is_accepted_somewhere_and_every_accept_is_decisive(name):
    ls, _ = _line_search(name)
    kept = _kept(name)
    slots = [ls[i, s]["slot"] for i in range(sv.NS) if kept[i] for s in sv.SCALES]
    count = {a: slots.count(k) for k, a in enumerate(sv.ALPHAS)}
    margin = min(c["margin"][: c["slot"] + 1 if c["slot"] >= 0 else 8].min() for (i, s), c in ls.items() if kept[i])
    print("%s: accepted alpha over %d kept cases: %s, none x%d; smallest margin up to the accepted candidate %.2e; dropped rollouts: %d"
          % (name, len(slots), ", ".join("%g x%d" % kv for kv in count.items()), slots.count(-1), margin, (~kept).sum()))
    assert (~kept).sum() <= sv.MAX_DROPPED
    assert all(n >= 1 for n in count.values())
    if name == "tame":
        assert slots.count(-1) >= 1
    assert margin >= sv.MARGIN_DECISIVE
    # the scales shift the slot, not the physics: the candidate of (scale 4, slot of 0.2) is that of (scale 1, slot of 0.8), and so on
    for i in np.flatnonzero(kept)[:4]:
        for (s1, a1), (s2, a2) in (((1, 0.8), (4, 0.2)), ((1, 0.4), (4, 0.1)), ((4, 0.2), (16, 0.05))):
            c1, c2 = ls[i, s1], ls[i, s2]
            k1, k2 = sv.ALPHAS.index(a1), sv.ALPHAS.index(a2)
            assert sv.rel(c2["X"][k2], c1["X"][k1]) < 1e-9 and not np.array_equal(c1["X"][k1], c1["X"][k1 + 1])


@pytest.mark.parametrize("name", LS_NAMES)
def test_rounding_in_the_gains_moves_the_accepted_candidate_far_less_than_the_tolerances(name):
    prob, mode, X, U = sv.trajectories(name)
    ric, _ = _riccati(name)
    ls, _ = _line_search(name)
    kept = _kept(name)
    o = sv.oracle_of(prob, mode)
    worst = dict(x=0.0, u=0.0, cost=0.0)
    for i in np.flatnonzero(kept):
        for s in sv.SCALES:
            ld = ric[i, s][0]
            c1 = ls[i, s]
            c2 = sv.candidates_ref(o, X[i], U[i], ld["K"].astype(np.float64), ld["k"].astype(np.float64))
            assert c2["slot"] == c1["slot"]
            if c1["slot"] < 0:
                continue
            (j1, x1, u1), (j2, x2, u2) = sv.accepted(c1), sv.accepted(c2)
            worst["x"] = max(worst["x"], sv.rel(x1, x2)); worst["u"] = max(worst["u"], sv.rel(u1, u2)); worst["cost"] = max(worst["cost"], abs(j1 - j2) / abs(j2))
    print("%s: the oracle's gains against the long-double ones rounded to fp64 move the accepted candidate by x %.2e, u %.2e, cost %.2e (relative)"
          % (name, worst["x"], worst["u"], worst["cost"]))
    assert FACTOR * worst["x"] <= sv.TOL_X and FACTOR * worst["u"] <= sv.TOL_U and FACTOR * worst["cost"] <= sv.TOL_COST


@pytest.mark.parametrize("mutant", sv.RICCATI_MUTANTS)
def test_every_riccati_mutant_moves_a_checked_output_a_hundredfold_beyond_its_tolerance(mutant):
    best, where = 0.0, None
    for name in NAMES:
        ric, kept = _riccati(name)
        for i in np.flatnonzero(kept):
            ld = ric[i, 1][0]
            if mutant == "no_bump" and np.all(ld["branch"] == 0):
                continue                                                      # (the mutant is the reference there)
            m = sv.riccati_ref(*_inputs(name, i), mutant=mutant)
            tol = sv.riccati_tol(ld["branch"])
            for key in sv.RICCATI_KEYS:
                r = sv.riccati_error(m[key].astype(np.float64), ld[key].astype(np.float64)) / tol
                if r > best:
                    best, where = r, (name, int(i), key, tol)
    print("mutant %s: moves %s of rollout %d (%s) by %.3g times its tolerance %.0e" % ((mutant,) + (where[2], where[1], where[0]) + (best, where[3])))
    assert best >= FACTOR


@pytest.mark.parametrize("mutant", sv.LS_MUTANTS)
def test_every_line_search_mutant_moves_a_checked_output_a_hundredfold_beyond_its_tolerance(mutant):
    best, where, flipped = 0.0, None, 0
    for name in LS_NAMES:
        prob, mode, X, U = sv.trajectories(name)
        ric, _ = _riccati(name)
        ls, _ = _line_search(name)
        kept = _kept(name)
        o = sv.oracle_of(prob, mode)
        for i in np.flatnonzero(kept):
            for s in sv.SCALES:
                c = ls[i, s]
                m = sv.candidates_ref(o, X[i], U[i], ric[i, s][2]["K"], ric[i, s][2]["k"], mutant=mutant)
                if m["slot"] != c["slot"]:
                    flipped += 1                                              # accept flag / alpha are compared exactly
                    continue
                if c["slot"] < 0:
                    continue
                (j1, x1, u1), (j2, x2, u2) = sv.accepted(m), sv.accepted(c)
                for key, r in (("xbar", sv.rel(x1, x2) / sv.TOL_X), ("ubar", sv.rel(u1, u2) / sv.TOL_U), ("cost", abs(j1 - j2) / abs(j2) / sv.TOL_COST)):
                    if r > best:
                        best, where = r, (name, int(i), s, key)
    print("mutant %s: another alpha is accepted in %d cases; where the same one is, the largest move is %s"
          % (mutant, flipped, "%.3g times the tolerance (%s of rollout %d, scale %d, %s)" % (best, where[3], where[1], where[2], where[0]) if where else "-"))
    assert flipped >= 1 or best >= FACTOR
    if mutant != "alpha_shift":
        assert best >= FACTOR                                                  # the feedback mutants are seen in the trajectories themselves
