"""The Riccati pass (riccati_pack.hip k_backward_pack, the shipped operand-layout kernel, and every cross-check family) and the line
search (k_line_search_s, one and four rollouts per wave, and the one-lane family) away from the standing pose: the trajectories of
tests/solve_envelope_cases.py -- sixteen off-pose rollouts whose every knot is another linearisation point, on which lxx is indefinite,
three rollouts reach the `indefinite even after the +1e-4 bump' branch (the Gauss-Jordan fallback, fed by the fold products), and the
three scales of lx / lu let every one of the eight alpha slots be the accepted one; a shift of luu at one knot of those three rollouts
puts the `bumped' branch, which natural data does not reach, on the same Jacobians.  B = 16, N = 5 (N = 4 in the contact modes), and
the same rollouts tiled to B = 1030 for the four-rollouts-per-wave instantiation.

Every stage is judged on the DEVICE's own inputs: A, B, the quadratics, xbar, ubar and (for the line search) the gains are read back
through the getters and handed to the reference, so a difference belongs to the stage under test.  Tolerances are the project's own:
Riccati 1e-9 max(1, max |want|) on a rollout whose knots all factorise (the `spd' golden), 1e-6 with a bumped or indefinite knot (the
`bump' golden, the folded test); line search: accept flag and alpha exact, cost 1e-8, xbar 1e-8, ubar 1e-7 relative (the standing-pose
test).  test_solve_envelope_cpu.py shows that the reference's own spread lies a hundred times below these and that the inputs see every
slip the kernels could make.  Every test prints the worst error it saw."""
import numpy as np
import pytest

import solve_envelope_cases as sv
from test_gpu_configs import _solver, env
from test_gpu_dynamics_envelope import _check_structure

pytestmark = pytest.mark.gpu
NS, NX, H = sv.NS, sv.NX, sv.dc.H
POS = np.r_[0:3, 7:26]; VEL = np.r_[26:29, 32:51]
E_POS = np.zeros((22, NX)); E_POS[np.arange(22), POS] = 1.0
FAMILIES = ("wave", "wave-fold", "wave-generic", "wg", "valu")
WIDE = 1030                                   # above 1024 rollouts: four per wave; 1030 % 4 = 2: the last wave is partly filled
_memo = {}


def _report(title, worst):
    print("%s: worst error: %s" % (title, ", ".join("%s %.2e" % kv for kv in worst.items())))


def _note(worst, key, e):
    worst[key] = max(worst.get(key, 0.0), float(e))


def _tiled(a, B):
    return np.concatenate([a] * ((B + NS - 1) // NS))[:B]


def _run(name, scales=sv.SCALES, families=(None,), line_search=True, B=NS, legacy=False, variant=None, bumped=False, h=H):
    """initialize; set_trajectory; stage_linearize; stage_cost_quadratics; per scale: set_trajectory, set_quadratics, per family
    stage_backward_pass, then stage_line_search (on the last family's gains).  Returns the device's inputs and, per (scale, family), its
    outputs.  B > 16: the sixteen rollouts tiled; the Jacobians are not read back then.  bumped: luu of the rollouts with an indefinite
    knot is replaced by solve_envelope_cases.bumped_luu() of the device's own inputs.  h: the time step of the trajectories, their
    problem and the handle."""
    key = (name, tuple(scales), tuple(families), line_search, B, legacy, tuple(sorted((variant or {}).items())), bumped, h)
    if key in _memo:
        return _memo[key]
    prob, mode, X, U = sv.trajectories(name, h)
    X, U = _tiled(X, B), _tiled(U, B)
    out = dict(prob=prob, mode=mode)
    with env(**(variant or {})):
        s = _solver(B, N=prob["N"], dt=prob["dt"], legacy=legacy)
        assert s.dt == prob["dt"] == h
        s.set_problem(prob); s.set_contact_mode(mode); s.set_options(jacobian_mode=0)
        s.set_regularization(sv.LAMBDA)
        s.initialize(X[:, 0], U); s.set_trajectory(X, U)
        s.stage_linearize(); s.stage_cost_quadratics()
        if B == NS:
            out["A"], out["B"] = s.linearization()
        lx, lu, lxx, luu = s.quadratics()
        if bumped:
            out["shifted"] = []
            for i in range(NS):
                shifted = sv.bumped_luu(luu[i], sv.riccati_ref_cached(out["A"][i], out["B"][i], lx[i], lu[i], lxx[i], luu[i]))
                if shifted is not None:
                    luu[i] = shifted; out["shifted"].append(i)
        if B == NS:
            out.update(lx=lx, lu=lu, lxx=lxx, luu=luu)
        for sc in scales:
            slx, slu = sv.scaled(lx, lu, sc)
            s.set_trajectory(X, U); s.set_quadratics(slx, slu, lxx, luu)
            out["X"], out["U"] = s.xbar(), s.ubar()
            for fam in families:
                with env(ILQR_BACKWARD=fam):
                    s.stage_backward_pass()
                Vx, Vxx = s.value_function()
                out[sc, fam] = dict(K=s.gains_K(), k=s.gains_kff(), Vx=Vx, Vxx=Vxx)
            if line_search:
                imp, cost, alpha = s.stage_line_search()
                out[sc, "ls"] = dict(imp=imp, cost=cost, alpha=alpha, X=s.xbar(), U=s.ubar())
        s.close()
    assert np.array_equal(out["X"], X) and np.array_equal(out["U"], U)
    _memo[key] = out
    return out


def _inputs(dev, i, sc):
    slx, slu = sv.scaled(dev["lx"][i], dev["lu"][i], sc)
    return dev["A"][i], dev["B"][i], slx, slu, dev["lxx"][i], dev["luu"][i]


def _riccati_kept(dev, scales=sv.SCALES):
    """kept [16] on the device's inputs: every branch decision of the long-double reference is decisive and fp64 takes the same branches"""
    kept = np.ones(NS, dtype=bool)
    for i in range(NS):
        for sc in scales:
            a = _inputs(dev, i, sc)
            kept[i] &= sv.branches_decisive(sv.riccati_ref_cached(*a), sv.riccati_ref_cached(*a, dtype=np.float64))
    assert (~kept).sum() <= sv.MAX_DROPPED
    return kept


def _check_riccati(dev, scales, families, kept, worst, tag):
    o = sv.oracle_of(dev["prob"], dev["mode"])
    for i in np.flatnonzero(kept):
        for sc in scales:
            a = _inputs(dev, i, sc)
            ld = sv.riccati_ref_cached(*a)
            tol = sv.riccati_tol(ld["branch"])
            o.set_linearization(a[0], a[1]); o.set_quadratics(*a[2:]); o.backward_pass()
            orc = dict(K=o.get("K"), k=o.get("kff"), Vx=o.get("Vx"), Vxx=o.get("Vxx"))
            for fam in families:
                got = dev[sc, fam]
                for key in sv.RICCATI_KEYS:
                    assert np.all(np.isfinite(got[key][i]))
                    e = sv.riccati_error(got[key][i], ld[key].astype(np.float64))
                    eo = sv.riccati_error(got[key][i], orc[key])
                    _note(worst, "%s (%.0e)" % (key, tol), e); _note(worst, "%s against the oracle (%.0e)" % (key, tol), eo)
                    assert e <= tol and eo <= tol, (tag, fam, i, sc, key, e, eo, tol, ld["branch"])


def _position_rows(A, Bm, worst, tag, h=H):
    """the structure the fold relies on: position rows e_p + h x velocity row (exact off the diagonal, one rounding of 1 + h a on it)"""
    e = np.abs(A[..., POS, :] - (E_POS + h * A[..., VEL, :])).max()
    _note(worst, "position rows (absolute)", e)
    assert e <= 2.3e-16, (tag, e)
    assert np.array_equal(Bm[..., POS, :], h * Bm[..., VEL, :]), tag


def _branches(dev, kept):
    return np.array([sv.riccati_ref_cached(*_inputs(dev, i, 1))["branch"] for i in range(NS)])[kept]


@pytest.mark.parametrize("name", ["tame", "contact1", "contact2"])
def test_riccati_default_family_matches_long_double_and_oracle(name):
    """(a) the shipped kernel with the fold (the product library, no switch set): stage_linearize leaves the analytic Jacobians, so
    stage_backward_pass takes k_backward_pack, as in test_folded_backward_pass_equals_generic_kernel_and_numpy.  Contact modes 1 and 2:
    the Jacobians are the device's, so no active-set tie enters."""
    dev = _run(name, line_search=name != "contact2")
    worst = {}
    if name == "tame":
        _check_structure(dev["A"], dev["B"], worst, name)
    else:
        _position_rows(dev["A"], dev["B"], worst, name)
    kept = _riccati_kept(dev)
    branch = _branches(dev, kept)
    print("%s: kept %d of %d rollouts; knots on branch 0 / 1 / 2: %d / %d / %d" % (name, kept.sum(), NS, (branch == 0).sum(), (branch == 1).sum(), (branch == 2).sum()))
    if name == "tame":
        assert (branch == 2).any(axis=1).sum() >= 2 and (branch == 0).all(axis=1).sum() >= 8
    _check_riccati(dev, sv.SCALES, (None,), kept, worst, name)
    _report("Riccati pass, default family, %s" % name, worst)


def test_riccati_every_family_on_the_same_inputs():
    """(b) the test library: the operand-layout kernel, the folded and the generic one-wave kernels, the four-wave MFMA kernel and the
    VALU kernel on the same Jacobians and quadratics, each against the reference at the tolerances of (a)"""
    dev = _run("tame", families=FAMILIES, line_search=False, legacy=True)
    kept = _riccati_kept(dev)
    for fam in FAMILIES:
        worst = {}
        _check_riccati(dev, sv.SCALES, (fam,), kept, worst, fam)
        _report("Riccati pass, ILQR_BACKWARD=%s" % fam, worst)
    for sc in sv.SCALES:                                       # different kernels did run
        for f, g in (("wave", "wave-generic"), ("wave-fold", "wave-generic"), ("wave", "wave-fold")):
            assert any(not np.array_equal(dev[sc, f][key], dev[sc, g][key]) for key in sv.RICCATI_KEYS), (sc, f, g)
        distinct = len({b"".join(dev[sc, f][key].tobytes() for key in sv.RICCATI_KEYS) for f in FAMILIES})
        print("scale %d: %d distinct outputs among the %d families" % (sc, distinct, len(FAMILIES)))
        assert distinct >= 3


def test_riccati_bumped_branch_on_natural_jacobians_in_every_family():
    """The branch natural data does not reach -- LLT fails, passes after the +1e-4 bump -- on the analytic Jacobians and the indefinite
    lxx of the tame trajectories: solve_envelope_cases.bumped_luu() shifts the diagonal of luu at the one indefinite knot of three
    rollouts so that the smallest eigenvalue of Quu is -5e-5.  The riccati_golden `bump' case reaches this branch through
    set_linearization only, that is on the generic kernel; here the fold products feed it.  Gains of 1e6 (the bumped Quu has an
    eigenvalue of 5e-5), held to the `bump' golden's 1e-6 max(1, max |want|); test_solve_envelope_cpu.py: the reference's spread on
    these is 2e-9."""
    dev = _run("tame", scales=(1,), families=FAMILIES, line_search=False, legacy=True, bumped=True)
    kept = _riccati_kept(dev, (1,))
    on_branch_1 = [i for i in dev["shifted"] if kept[i] and (sv.riccati_ref_cached(*_inputs(dev, i, 1))["branch"] == 1).any()]
    print("shifted luu: rollouts %s take the bumped branch at some knot" % on_branch_1)
    assert len(on_branch_1) >= 2
    for fam in FAMILIES:
        worst = {}
        _check_riccati(dev, (1,), (fam,), kept, worst, "bumped " + fam)
        _report("Riccati pass with a bumped knot, ILQR_BACKWARD=%s" % fam, {k: v for k, v in worst.items() if "1e-06" in k})


def _check_line_search(dev, worst, tag, want_rejection, every_slot=True):
    """accept flag and alpha exactly the reference's on the device's own gains, cost / xbar / ubar at the standing-pose test's tolerances;
    every alpha slot (and a rejection) occurred on the device among the kept cases"""
    o = sv.oracle_of(dev["prob"], dev["mode"])
    kept = _riccati_kept(dev)
    cand = {}
    for i in range(NS):
        for sc in sv.SCALES:
            cand[i, sc] = sv.candidates_ref(o, dev["X"][i], dev["U"][i], dev[sc, None]["K"][i], dev[sc, None]["k"][i])
            kept[i] &= cand[i, sc]["decisive"]
    assert (~kept).sum() <= sv.MAX_DROPPED
    seen = []
    for i in np.flatnonzero(kept):
        for sc in sv.SCALES:
            c, got = cand[i, sc], dev[sc, "ls"]
            assert bool(got["imp"][i]) == (c["slot"] >= 0) and got["alpha"][i] == c["alpha"], (tag, i, sc, got["alpha"][i], c["alpha"])
            cost, xw, uw = sv.accepted(c)
            if c["slot"] < 0:
                xw, uw = dev["X"][i], dev["U"][i]              # a rejection leaves the nominal trajectory
            ec, ex, eu = abs(got["cost"][i] - cost) / abs(cost), sv.rel(got["X"][i], xw), sv.rel(got["U"][i], uw)
            _note(worst, "cost", ec); _note(worst, "xbar", ex); _note(worst, "ubar", eu)
            assert ec < sv.TOL_COST and ex < sv.TOL_X and eu < sv.TOL_U, (tag, i, sc, c["alpha"], ec, ex, eu)
            seen.append(float(got["alpha"][i]))
    count = {a: seen.count(a) for a in sv.ALPHAS + (0.0,)}
    print("%s: accepted alpha on the device over %d kept cases: %s" % (tag, len(seen), ", ".join("%g x%d" % kv for kv in count.items())))
    assert all(count[a] >= 1 for a in sv.ALPHAS) or not every_slot
    assert count[0.0] >= 1 or not want_rejection
    return len(seen)


@pytest.mark.parametrize("ls", ["s", "r"])
def test_line_search_accepts_through_every_alpha_slot(ls):
    """(c) after (a)'s backward pass, for each scale; ILQR_LS=r with ILQR_ROLLOUT=r: the one-lane family of the test library"""
    dev = _run("tame") if ls == "s" else _run("tame", variant=dict(ILQR_LS="r", ILQR_ROLLOUT="r"))
    worst = {}
    _check_line_search(dev, worst, "ILQR_LS=%s" % ls, want_rejection=True)
    _report("line search, ILQR_LS=%s" % ls, worst)


def test_line_search_in_contact_mode_1_accepts_through_every_alpha_slot():
    """(c) rigid stance rows under the schedule both feet / left / right / none.  (Mode 2 decides an active set per candidate and is left
    out; no case of these trajectories is rejected in mode 1 -- test_solve_envelope_cpu.py prints the counts.)"""
    dev = _run("contact1")
    worst = {}
    _check_line_search(dev, worst, "contact mode 1", want_rejection=False)
    _report("line search, contact mode 1", worst)


@pytest.mark.parametrize("name", ["tame", "contact1"])
def test_four_rollouts_per_wave_give_the_bits_of_one_per_wave(name):
    """(d) step kinds 0 (free flight) and 1 (contact mode 1): the sixteen rollouts tiled to B = 1030 take the four-rollouts-per-wave
    line search; the same stage sequence at scale 4 gives, in the first tile, the last complete tile and the partly filled end, the bits
    of the B = 16 run"""
    small = _run(name)
    wide = _run(name, scales=(4,), B=WIDE)
    last = WIDE - WIDE % NS - NS
    for lo, n in ((0, NS), (last, NS), (WIDE - WIDE % NS, WIDE % NS)):
        for key in ("imp", "alpha", "cost", "X", "U"):
            assert np.array_equal(small[4, "ls"][key][:n], wide[4, "ls"][key][lo:lo + n]), (name, lo, key)
        for key in ("K", "k"):
            assert np.array_equal(small[4, None][key][:n], wide[4, None][key][lo:lo + n]), (name, lo, key)
    assert len(set(small[4, "ls"]["alpha"].tolist())) >= 4               # several slots, so several lanes, are the accepted ones
    print("%s: B = %d equals B = %d bit for bit in rollouts 0..15, %d..%d and %d..%d; accepted alpha: %s"
          % (name, WIDE, NS, last, last + NS - 1, WIDE - WIDE % NS, WIDE - 1, sorted(set(small[4, "ls"]["alpha"].tolist()))))


def test_inside_a_solve_the_kernels_read_the_images_the_producers_wrote():
    """(e) one iteration, no convergence exit, cold start from the tame states and controls: the Riccati kernel reads the operand-layout
    Jacobians and the half-stored lxx the tangent and cost kernels wrote, with no conversion in between.  Gains, value function and the
    accepted alpha equal the stage pipeline's on the same trajectory (the device's own rollout of the controls) at the tolerances of (a)
    and (c).  A rollout whose first line search fails is retried inside the solve with lambda = 1e-5 (ilqr.cpp:619-644): its gains are
    those of the retry, and the stage pipeline is run again with that lambda for it."""
    prob, mode, X, U = sv.trajectories("tame")
    s = _solver(NS, N=prob["N"]); s.set_problem(prob); s.set_options(jacobian_mode=0, early_exit=False); s.set_max_iterations(1)
    s.set_regularization(sv.LAMBDA)
    s.initialize(X[:, 0], U)
    X0, U0 = s.xbar(), s.ubar()
    assert np.array_equal(U0, U) and sv.rel(X0, X) < 1e-10
    cost = s.solve(X[:, 0])
    tc, ta, tl = s.trace()
    Vx, Vxx = s.value_function()
    solve = dict(K=s.gains_K(), k=s.gains_kff(), Vx=Vx, Vxx=Vxx, X=s.xbar(), U=s.ubar())
    s.close()
    stage = {}
    s = _solver(NS, N=prob["N"]); s.set_problem(prob); s.set_options(jacobian_mode=0)
    s.initialize(X[:, 0], U); s.set_trajectory(X0, U0)
    s.stage_linearize(); s.stage_cost_quadratics()
    A, Bm = s.linearization(); lx, lu, lxx, luu = s.quadratics()
    for lam in (sv.LAMBDA, 10 * sv.LAMBDA):
        s.set_trajectory(X0, U0); s.set_regularization(lam); s.stage_backward_pass()
        sVx, sVxx = s.value_function()
        st = dict(K=s.gains_K(), k=s.gains_kff(), Vx=sVx, Vxx=sVxx)
        st["imp"], st["cost"], st["alpha"] = s.stage_line_search()
        st["X"], st["U"] = s.xbar(), s.ubar()
        stage[lam] = st
    s.close()
    o = sv.oracle_of(prob, mode)
    worst, retried, compared = {}, 0, 0
    for i in range(NS):
        ld = sv.riccati_ref_cached(A[i], Bm[i], lx[i], lu[i], lxx[i], luu[i])
        c = sv.candidates_ref(o, X0[i], U0[i], stage[sv.LAMBDA]["K"][i], stage[sv.LAMBDA]["k"][i])
        if not (sv.branches_decisive(ld, sv.riccati_ref_cached(A[i], Bm[i], lx[i], lu[i], lxx[i], luu[i], dtype=np.float64)) and c["decisive"]):
            continue
        assert bool(stage[sv.LAMBDA]["imp"][i]) == (c["slot"] >= 0)
        lam = sv.LAMBDA if c["slot"] >= 0 else 10 * sv.LAMBDA
        if c["slot"] < 0:
            ld = sv.riccati_ref(A[i], Bm[i], lx[i], lu[i], lxx[i], luu[i], lam=lam)
            c = sv.candidates_ref(o, X0[i], U0[i], stage[lam]["K"][i], stage[lam]["k"][i])
            if not (sv.branches_decisive(ld) and c["decisive"]):
                continue
            retried += 1
        compared += 1
        assert tl[i, 0] == lam, (i, tl[i, 0], lam)
        st = stage[lam]
        assert ta[i, 0] == st["alpha"][i], (i, ta[i, 0], st["alpha"][i])
        tol = sv.riccati_tol(ld["branch"])
        for key in sv.RICCATI_KEYS:
            e = sv.riccati_error(solve[key][i], st[key][i])
            _note(worst, "%s (%.0e)" % (key, tol), e)
            assert e <= tol, (i, key, e, tol)
            e = sv.riccati_error(solve[key][i], ld[key].astype(np.float64))
            _note(worst, "%s against long double (%.0e)" % (key, tol), e)
            assert e <= tol, (i, key, e, tol)
        ec, ex, eu = abs(cost[i] - st["cost"][i]) / abs(st["cost"][i]), sv.rel(solve["X"][i], st["X"][i]), sv.rel(solve["U"][i], st["U"][i])
        _note(worst, "cost", ec); _note(worst, "xbar", ex); _note(worst, "ubar", eu)
        assert ec < sv.TOL_COST and ex < sv.TOL_X and eu < sv.TOL_U, (i, ec, ex, eu)
    print("inside a solve: %d of %d rollouts compared, %d through the lambda retry; accepted alpha: %s" % (compared, NS, retried, sorted(set(ta[:, 0].tolist()))))
    assert compared >= NS - sv.MAX_DROPPED and len(set(ta[:, 0].tolist())) >= 4
    _report("inside a solve against the stage pipeline", worst)
