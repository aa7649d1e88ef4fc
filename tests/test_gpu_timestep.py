"""Every kernel above the dynamics step at time steps other than the suite's 0.02: h in dynamics_envelope_cases.TIMESTEPS = (0.005, 0.01,
0.04).  The handle takes dt as a free parameter and many kernels use it structurally -- h and h^2 in dE, the position rows
e_p + h (velocity row), the small-spin branch on |h w'|^2, the joint-limit rows, the forward-difference kernels, the operand layout
without the position rows that k_unpack_ab(h) rebuilds, the scalar fold factor of k_backward_pack / k_backward_wave, the rollout, the
line search, the warm-start tail, the plant -- so a baked 0.02, or one factor h too many or too few, shows here and nowhere else.

The inputs are those of dynamics_envelope_cases.py / solve_envelope_cases.py / contact_envelope_cases.py built at h (prob["dt"] = h; every
handle is constructed with dt = prob["dt"], and that is asserted: set_problem ignores prob["dt"]).  References: the CPU oracle at h, the
long-double Riccati restatement, the oracle's candidates.  test_timestep_cpu.py shows that the references' own spread lies two orders
below the bounds, that the caps hold (every contact pair kept, every branch decisive, every line-search case at 0.005 and 0.01 decisive),
and that a baked 0.02 moves the checked outputs by far more than a hundred times the bounds.

Tolerances are the project's own for the same quantities, none widened: analytic Jacobians 1e-9 max(1, |want|), spin quaternion rows 1e-12,
position-row structure 2.3e-16, forward differences 2e-5, contact Jacobians 1e-8, step 1e-11, stance step 1e-9, Riccati 1e-9 / 1e-6 by
branch, line search exact accept and alpha with cost 1e-8, xbar 1e-8, ubar 1e-7, solve traces as test_full_solve_parity_for_every_kernel_variant,
plant as test_gpu_plant.py.  The line search runs at 0.005 and 0.01 only (at 0.04 fifteen of 48 free-flight cases are undecided on the
reference).  Sliding contact (modes 3 / 4, mu 0.3) and the joint-limit rows (mode 2, k = 625) run at every h: the reference keeps 64 of 64
pairs at each, as at 0.02 (contact_envelope_cases.TIMESTEP_CASES).  Every test prints the worst error it saw."""
import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import solve_envelope_cases as sv
from test_gpu_configs import _solver, rel
from test_gpu_dynamics_envelope import _check, _check_structure, _report, _stage_jacobians
from test_gpu_solve_envelope import FAMILIES, WIDE, _branches, _check_line_search, _check_riccati, _position_rows, _riccati_kept, _run
from test_gpu_solve_envelope import _report as _report_solve

pytestmark = pytest.mark.gpu
NS, NX, NU, NQ = dc.NS, dc.NX, dc.NU, dc.NQ
TIMESTEPS = dc.TIMESTEPS


def _handle(h, N=2, mode=0, schedule=False, B=NS):
    """a handle AT h with the problem at h"""
    prob = dc.problem(N, dc.SCHEDULE if schedule else None, h=h)
    s = _solver(B, N=N, dt=prob["dt"])
    assert s.dt == prob["dt"] == h
    s.set_problem(prob); s.set_contact_mode(mode); s.set_options(jacobian_mode=0)
    return s


# ---------------------------------------------------------------------------------------------------------------------------------------
# Jacobians and steps
@pytest.mark.parametrize("name", ["wide", "nonunit", "clamped", "spin"])
@pytest.mark.parametrize("h", TIMESTEPS)
def test_free_flight_analytic_jacobians_match_oracle_ad(h, name):
    """read through linearization(): k_unpack_ab(h) rebuilds the position rows the operand layout does not store.  spin(h): w' solved for
    |h w'|^2 = SPIN_S at this h, eight states on either side of the branch; its quaternion rows beside the quaternion columns to 1e-12"""
    x, u = dc.group(name, h)
    want_A, want_B = dc.group_ad(name, h)
    s = _handle(h)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    worst = {}
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(Bm))
    for i in range(NS):
        for t in range(2):
            _check(A[i, t], want_A[i], 1e-9, worst, "A", (h, name, i, t))
            _check(Bm[i, t], want_B[i], 1e-9, worst, "B", (h, name, i, t))
            if name == "spin":
                _check(A[i, t][3:7, 7:], want_A[i][3:7, 7:], 1e-12 * max(1.0, np.abs(want_A[i]).max()), worst, "quaternion rows", (h, i, t))
    _check_structure(A, Bm, worst, (h, name), h)
    if name == "clamped":
        beyond = dc.clamped()[2]
        for i in range(NS):
            assert np.all(Bm[i][:, :, beyond[i]] == 0.0), i
    _report("analytic Jacobians, h %g, %s" % (h, name), worst)


@pytest.mark.parametrize("h", TIMESTEPS)
def test_free_flight_forward_difference_jacobians_match_oracle(h):
    x, u = dc.group("wide")
    want_A, want_B = dc.oracle_jacobians(x, u, jac_mode=1, fd_eps=1e-5, h=h)
    s = _handle(h); s.set_options(jacobian_mode=1, fd_eps=1e-5)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    worst = {}
    for i in range(NS):
        for t in range(2):
            _check(A[i, t], want_A[i], 2e-5, worst, "A", (h, i, t))
            _check(Bm[i, t], want_B[i], 2e-5, worst, "B", (h, i, t))
    _report("forward-difference Jacobians, h %g" % h, worst)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("h", TIMESTEPS)
def test_contact_analytic_jacobians_match_oracle_ad(h, mode):
    """N = 4, one stance pattern per knot (dynamics_envelope_cases.SCHEDULE); the reference keeps all 64 (state, pattern) pairs at every h"""
    x, u, kept, want_A, want_B, _ = dc.mid_cases(mode, h=h)
    assert kept.all()
    s = _handle(h, N=4, mode=mode, schedule=True)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    worst = {}
    for i, p in np.argwhere(kept):
        _check(A[i, p], want_A[i, p], 1e-8, worst, "A", (h, mode, i, p))
        _check(Bm[i, p], want_B[i, p], 1e-8, worst, "B", (h, mode, i, p))
    # position rows e_p + h x velocity row, as k_unpack_ab(h) rebuilds them: exact but for the one rounding of 1 + h a.  Under the stance
    # rows mid() reaches |A| = 111, so 1 + h a reaches 5 at h = 0.04 and that rounding is an ulp of the ENTRY, not of 1 (the 2.3e-16 absolute
    # of _position_rows presumes |1 + h a| < 2): 2.3e-16 max(1, |entry|), entry by entry
    rows = dc.E_POS + h * A[..., dc.VEL, :]
    worst["position rows (relative to max(1, |entry|))"] = e = (np.abs(A[..., dc.POS, :] - rows) / np.maximum(1.0, np.abs(rows))).max()
    assert e <= 2.3e-16, (h, mode, e)
    assert np.array_equal(Bm[..., dc.POS, :], h * Bm[..., dc.VEL, :]), (h, mode)
    _report("contact Jacobians, h %g, mode %d (%d of %d cases kept)" % (h, mode, kept.sum(), kept.size), worst)


@pytest.mark.parametrize("kind,h", cc.TIMESTEP_CASES)
def test_sliding_and_joint_limit_jacobians_and_steps_match_oracle(kind, h):
    """modes 3 / 4 at mu 0.3 and the joint-limit rows in mode 2 at k = 625: step 1e-9, Jacobians 1e-8; for every hinge the oracle stops,
    the rows with this h: v+ = -h k r, velocity row of A = -h k e_theta, row of B = 0, position row (1 - h^2 k) e_theta (1e-10, B 1e-12)"""
    limits = kind == "limits2"
    mode, mu, k = (2, None, cc.K_STIFF[1]) if limits else (int(kind[-1]), cc.MUS[0], 0.0)
    c = cc.limit_cases(mode, k, h=h) if limits else cc.sliding_cases(mode, mu, h=h)
    x, u, kept = c["x"], c["u"], c["kept"]
    worst = {}
    s = cc.configure(_handle(h, mode=mode), mu, limits, k)
    got = np.stack([s.step_stance(x, u, int(sl), int(sr)) for sl, sr in cc.rows(mode)], axis=1)
    s.close()
    for i, p in np.argwhere(kept):
        _check(got[i, p], c["step"][i, p], cc.STEP_TOL, worst, "step", (kind, h, i, p))
    s = cc.configure(_handle(h, N=4, mode=mode, schedule=True), mu, limits, k)
    A, Bm = _stage_jacobians(s, x, u)
    s.close()
    for i, p in np.argwhere(kept):
        _check(A[i, p], c["A"][i, p], cc.JAC_TOL, worst, "A", (kind, h, i, p))
        _check(Bm[i, p], c["B"][i, p], cc.JAC_TOL, worst, "B", (kind, h, i, p))
    if limits:
        stopped = cc.stopped_hinges(x, got, k, h)
        cc.check_limit_caps(kept, stopped, (kind, h, "device"))
        assert np.array_equal(stopped[kept], c["stopped"][kept])
        for i, p in np.argwhere(kept):
            for j in np.flatnonzero(c["stopped"][i, p]):
                e = np.zeros(NX); e[7 + j] = -h * k
                e2 = np.zeros(NX); e2[7 + j] = 1.0 - h * h * k
                for key, err, tol in (("stopped hinge, velocity row of A (absolute)", np.abs(A[i, p][NQ + 6 + j] - e).max(), 1e-10),
                                      ("stopped hinge, row of B (absolute)", np.abs(Bm[i, p][NQ + 6 + j]).max(), 1e-12),
                                      ("stopped hinge, position row of A (absolute)", np.abs(A[i, p][7 + j] - e2).max(), 1e-10)):
                    worst[key] = max(worst.get(key, 0.0), err)
                    assert err <= tol, (kind, h, i, p, j, key, err)
    else:
        cc.check_sliding_caps(kept, c["slides"], (kind, h))
    _report("%s, h %g (%d of %d cases kept)" % (kind, h, kept.sum(), kept.size), worst)


@pytest.mark.parametrize("h", TIMESTEPS)
def test_step_and_stance_step_match_oracle(h):
    """the anchors of the rollouts below: step on wide() 1e-11, stance-constrained step on mid() in modes 1 / 2 under every pattern 1e-9"""
    worst = {}
    x, u = dc.group("wide")
    s = _handle(h)
    got = s.step(x, u)
    o = dc.oracle(h=h)
    for i in range(NS):
        _check(got[i], o.step(x[i], u[i]), 1e-11, worst, "step", (h, i))
    for mode in (1, 2):
        xm, um, kept = dc.mid_cases(mode, h=h)[:3]
        s.set_contact_mode(mode)
        om = dc.oracle(mode=mode, h=h)
        for p, (sl, sr) in enumerate(dc.STANCE_ROWS):
            gm = s.step_stance(xm, um, int(sl), int(sr))
            for i in np.flatnonzero(kept[:, p]):
                _check(gm[i], om.step_stance(xm[i], um[i], dc.STANCE_ROWS[p]), 1e-9, worst, "mode %d" % mode, (h, i, p))
    s.close()
    _report("step and stance-constrained step, h %g" % h, worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Riccati pass
@pytest.mark.parametrize("name", ["tame", "contact2"])
@pytest.mark.parametrize("h", TIMESTEPS)
def test_riccati_default_family_matches_long_double_and_oracle(h, name):
    """the shipped k_backward_pack with its fold factor at h, on the device's own Jacobians and quadratics; 1e-9 max(1, |want|) on a
    rollout whose knots all factorise, 1e-6 otherwise.  h = 0.04: some rollout takes the indefinite branch, fed by the fold products"""
    dev = _run(name, h=h, line_search=h in sv.LS_TIMESTEPS)
    worst = {}
    if name == "tame":
        _check_structure(dev["A"], dev["B"], worst, (h, name), h)
    else:
        _position_rows(dev["A"], dev["B"], worst, (h, name), h)
    kept = _riccati_kept(dev)
    branch = _branches(dev, kept)
    print("h %g, %s: kept %d of %d rollouts; knots on branch 0 / 1 / 2: %d / %d / %d" % (h, name, kept.sum(), NS, (branch == 0).sum(), (branch == 1).sum(), (branch == 2).sum()))
    if name == "tame" and h == 0.04:
        assert (branch == 2).any(axis=1).sum() >= 1
    _check_riccati(dev, sv.SCALES, (None,), kept, worst, (h, name))
    _report_solve("Riccati pass, default family, h %g, %s" % (h, name), worst)


@pytest.mark.parametrize("name", ["tame", "contact2"])
@pytest.mark.parametrize("h", TIMESTEPS)
def test_riccati_every_family_on_the_same_inputs(h, name):
    """the test library: the folded and the generic one-wave kernels, the four-wave MFMA kernel and the VALU kernel at h"""
    dev = _run(name, families=FAMILIES, line_search=False, legacy=True, h=h)
    kept = _riccati_kept(dev)
    for fam in FAMILIES:
        worst = {}
        _check_riccati(dev, sv.SCALES, (fam,), kept, worst, (h, name, fam))
        _report_solve("Riccati pass, h %g, %s, ILQR_BACKWARD=%s" % (h, name, fam), worst)
    for sc in sv.SCALES:                                       # different kernels did run
        distinct = len({b"".join(dev[sc, f][key].tobytes() for key in sv.RICCATI_KEYS) for f in FAMILIES})
        assert distinct >= 3, (h, name, sc, distinct)


# ---------------------------------------------------------------------------------------------------------------------------------------
# line search
@pytest.mark.parametrize("name", ["tame", "contact2"])
@pytest.mark.parametrize("h", sv.LS_TIMESTEPS)
def test_line_search_matches_the_oracles_candidates(h, name):
    """k_line_search_s, one rollout per wave, after the default family's backward pass, over SCALES: in free flight every alpha slot is the
    accepted one somewhere; mode 2 under the schedule both feet / left / right / none"""
    dev = _run(name, h=h)
    worst = {}
    n = _check_line_search(dev, worst, "h %g, %s" % (h, name), want_rejection=False, every_slot=name == "tame")
    assert n >= len(sv.SCALES) * (NS - sv.MAX_DROPPED)
    _report_solve("line search, h %g, %s" % (h, name), worst)


def test_four_rollouts_per_wave_give_the_bits_of_one_per_wave():
    """the one larger shape: the sixteen free-flight rollouts at h = 0.005 tiled to B = 1030 take the four-rollouts-per-wave line search; at
    scale 1 (five alpha slots are accepted there) the first tile, the last complete tile and the partly filled end give the bits of the
    B = 16 run"""
    h, sc = sv.LS_TIMESTEPS[0], sv.LS_WIDE_SCALE
    small = _run("tame", h=h)
    wide = _run("tame", scales=(sc,), B=WIDE, h=h)
    last = WIDE - WIDE % NS - NS
    for lo, n in ((0, NS), (last, NS), (WIDE - WIDE % NS, WIDE % NS)):
        for key in ("imp", "alpha", "cost", "X", "U"):
            assert np.array_equal(small[sc, "ls"][key][:n], wide[sc, "ls"][key][lo:lo + n]), (lo, key)
        for key in ("K", "k"):
            assert np.array_equal(small[sc, None][key][:n], wide[sc, None][key][lo:lo + n]), (lo, key)
    assert len(set(small[sc, "ls"]["alpha"].tolist())) >= 4
    print("h %g: B = %d equals B = %d bit for bit; accepted alpha: %s" % (h, WIDE, NS, sorted(set(small[sc, "ls"]["alpha"].tolist()))))


# ---------------------------------------------------------------------------------------------------------------------------------------
# one solve per h
@pytest.mark.parametrize("h", TIMESTEPS)
def test_full_solve_and_warm_started_second_solve_match_the_oracle(h):
    """B = 4, N = 8, five iterations at the most, analytic Jacobians, default kernels, from the perturbed standing batch; then the warm
    start (k_warm_shift / tail at h) from the same x0 and a second solve.  Per rollout: iteration count and alpha trace exact, lambda trace
    rtol 1e-12, cost trace rtol 1e-5, K rel < 1e-5 (test_timestep_cpu.py: no decision of these solves sits on a tie)"""
    prob, x0, ui = sv.standing_solve(h)
    B = len(x0)
    s = _solver(B, N=prob["N"], dt=prob["dt"]); assert s.dt == prob["dt"] == h
    s.set_problem(prob); s.set_max_iterations(sv.SOLVE_ITERATIONS); s.set_options(jacobian_mode=0)
    got = []
    for warm in (False, True):
        if warm:
            s.initialize_warm_resident(x0)
        else:
            s.initialize(x0, ui)
        cost = s.solve(x0)
        tc, ta, tl = s.trace()
        got.append(dict(cost=cost, tc=tc, ta=ta, tl=tl, K=s.gains_K(), it=s.iterations()))
        assert s.adopt_mismatches() == 0
    s.close()
    worst = {}
    for b in range(B):
        for tag, g, w in zip(("cold", "warm"), got, sv.standing_solve_ref(prob, x0[b], ui[b])):
            n = w["it"]
            assert n == g["it"][b], (h, b, tag, n, g["it"][b])
            assert np.array_equal(g["ta"][b, :n], w["alpha"][:n]), (h, b, tag, g["ta"][b, :n], w["alpha"][:n])
            assert np.allclose(g["tl"][b, :n], w["lam"][:n], rtol=1e-12, atol=0), (h, b, tag)
            ec = np.abs(g["tc"][b, : n + 1] / w["cost"][: n + 1] - 1.0).max()
            ek = rel(g["K"][b], w["K"])
            worst[tag + " cost trace"] = max(worst.get(tag + " cost trace", 0.0), ec); worst[tag + " K"] = max(worst.get(tag + " K", 0.0), ek)
            assert np.allclose(g["tc"][b, : n + 1], w["cost"][: n + 1], rtol=1e-5, atol=0) and abs(g["cost"][b] - w["final"]) <= 1e-5 * abs(w["final"]), (h, b, tag, ec)
            assert ek < 1e-5, (h, b, tag, ek)
    print("h %g: iterations cold %s, warm %s" % (h, got[0]["it"].tolist(), got[1]["it"].tolist()))
    _report_solve("solve, h %g (relative)" % h, worst)


# ---------------------------------------------------------------------------------------------------------------------------------------
# two handles
def _stages(handles, data):
    """two rounds of stage_linearize / linearization() / stage_cost_quadratics / stage_backward_pass, the calls of the handles alternating;
    per handle, everything it gave"""
    out = [[] for _ in handles]
    for _ in range(2):
        for s, (X, U) in zip(handles, data):
            s.set_trajectory(X, U); s.stage_linearize()
        for s, o in zip(handles, out):
            o.extend(s.linearization())
        for s in handles:
            s.stage_cost_quadratics()
        for s in handles:
            s.stage_backward_pass()
        for s, o in zip(handles, out):
            o.extend([s.gains_K(), s.gains_kff()]); o.extend(s.value_function())
    return out


def test_two_handles_at_two_steps_do_not_share_layout_state():
    """handles at h = 0.005 and h = 0.04 alive together, their calls alternating: every Jacobian (rebuilt by k_unpack_ab with the handle's
    own h), gain and value function equals, bit for bit, that of a handle that ran alone"""
    hs = (TIMESTEPS[0], TIMESTEPS[-1])
    data, probs = [], []
    for h in hs:
        prob, _, X, U = sv.trajectories("tame", h)
        probs.append(prob); data.append((X, U))

    def make(k):
        s = _solver(NS, N=probs[k]["N"], dt=probs[k]["dt"]); assert s.dt == probs[k]["dt"] == hs[k]
        s.set_problem(probs[k]); s.set_options(jacobian_mode=0); s.set_regularization(sv.LAMBDA)
        s.initialize(data[k][0][:, 0], data[k][1])
        return s

    alone = []
    for k in range(2):
        s = make(k)
        alone.append(_stages([s], [data[k]])[0])
        s.close()
    pair = [make(0), make(1)]
    together = _stages(pair, data)
    for s in pair:
        s.close()
    for k in range(2):
        assert len(together[k]) == len(alone[k]) == 12
        for j, (a, b) in enumerate(zip(together[k], alone[k])):
            assert np.all(np.isfinite(a)) and np.array_equal(a, b), (hs[k], j)
    assert not np.array_equal(together[0][0], together[1][0])
    print("handles at h %g and %g: 12 outputs each equal, bit for bit, those of a handle alone" % hs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# plant
@pytest.mark.parametrize("fb", [0, 1])
def test_plant_follows_the_policy_at_another_solver_step(fb):
    """solver at dt = 0.01, two physics substeps of 0.005, contact mode 2 on a per-rollout schedule, B = 5, N = 6, plant_follow(0, 2):
    each interval against the teacher-forced composition control law -> step_stance on a step handle at 0.005; bounds of test_gpu_plant.py"""
    from test_gpu_plant import U_TOL, X_TOL_PER_STEP
    from test_gpu_plant_follow import ITERS, N, _host_interval, _problem
    dt, substeps, B, M = 0.01, 2, 5, 2
    prob, x0, ui = _problem(B, 14, per_rollout_schedule=True)
    prob["dt"] = dt

    def solved():
        A = _solver(B, N=N, dt=prob["dt"]); assert A.dt == prob["dt"] == dt
        A.set_contact_mode(2); A.set_max_iterations(ITERS)
        A.plant_configure(substeps, fb, "schedule"); A.plant_set_history(M)
        A.set_problem(prob); A.initialize(x0, ui); A.solve(x0)
        A.plant_reset(x0)
        return A

    A, T = solved(), solved()
    P = _solver(B, N=N, dt=dt / substeps); assert P.dt == 0.005
    P.set_contact_mode(2); P.set_problem(prob)
    A.plant_follow(0, M)
    hx, hu = A.plant_history()
    states = list(hx) + [A.plant_state()]
    assert hx.shape == (M, B, NX) and np.array_equal(hx[0], x0)
    worst = {}
    for j in range(M):
        want_x, want_u, want_st = _host_interval(A, P, states[j], j, substeps, fb, "schedule", 2, prob["stance"][:, j])
        T.plant_follow(j, 1)
        ex, eu = np.abs(states[j + 1] - want_x).max(), np.abs(hu[j] - want_u).max()
        worst["x (absolute)"] = max(worst.get("x (absolute)", 0.0), ex); worst["u (absolute)"] = max(worst.get("u (absolute)", 0.0), eu)
        assert np.allclose(hu[j], want_u, **U_TOL), (j, eu)
        assert ex < X_TOL_PER_STEP * substeps, (j, ex)
        assert np.array_equal(T.plant_stance(), want_st), j
    assert np.all(A.plant_alive() == 1) and np.abs(A.plant_state() - x0).max() > 1e-4
    A.close(); T.close(); P.close()
    _report_solve("plant at dt 0.01 with two substeps, feedback mode %d" % fb, worst)
