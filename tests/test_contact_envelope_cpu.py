"""The inputs of tests/contact_envelope_cases.py can tell a right sliding-contact / joint-limit kernel from a wrong one, stay inside the caps
the GPU tests (test_gpu_contact_envelope.py) assert again, and the oracle can be trusted on them -- checked on the CPU oracle alone, so
that the GPU tests cannot pass vacuously: enough feet slide in double and in single support, every hinge is stopped somewhere and most at
either end, a hinge ON its limit never is, the branches move the Jacobians by far more than the GPU tolerances, and the oracle's forward-mode
AD agrees with sixth-order central differences of its own step to two orders below those tolerances."""
import numpy as np
import pytest

import contact_envelope_cases as cc
import dynamics_envelope_cases as dc

SLIDING = [(mode, variant, mu) for mode in (3, 4) for variant, mu in cc.SLIDING_VARIANTS]
LIMITS = [(mode, k) for mode in (0, 1, 2, 3, 4) for k in cc.K_STIFF]


@pytest.mark.parametrize("mode,variant,mu", SLIDING)
def test_sliding_cases_stay_inside_the_caps(mode, variant, mu):
    c = cc.sliding_cases(mode, mu, variant)
    assert np.all(np.isfinite(c["A"])) and np.all(np.isfinite(c["B"])) and np.all(np.isfinite(c["step"]))
    dropped, sliding = cc.check_sliding_caps(c["kept"], c["slides"], (mode, variant, mu))
    n = (c["slides"] & c["kept"]).sum(axis=0)
    print("mode %d, %s, mu %.1f: %d of %d cases kept; %d of 48 stance cases slide (both feet %d, left only %d, right only %d); Jacobian drift "
          "under the velocity scaling %.1e; |A|max %.1f" % (mode, variant, mu, c["kept"].sum(), c["kept"].size, sliding, n[0], n[1], n[2], c["drift"], np.abs(c["A"]).max()))
    assert dropped * 8 <= c["kept"].size and c["drift"] <= 1e-4
    if variant == "nonunit":
        assert np.abs(np.linalg.norm(c["x"][:, 3:7], axis=1) - 1.0).min() >= 0.05
    if variant == "clamped":
        assert c["beyond"].sum(axis=0).min() >= 1


@pytest.mark.parametrize("variant,mu", cc.SLIDING_VARIANTS)
def test_sliding_moves_the_jacobians_and_kinetic_friction_moves_them_again(variant, mu):
    """on every kept case that slides: modes 3 and 4 against mode 2, and mode 4 against mode 3, differ by more than 1e-3 in A; on the kept
    cases that do not slide the three modes are one step"""
    c3, c4 = cc.sliding_cases(3, mu, variant), cc.sliding_cases(4, mu, variant)
    A2 = dc.mid_cases(2, variant)[3]
    assert np.array_equal(dc.mid_cases(2, variant)[0], c3["x"]) and np.array_equal(c3["slides"], c4["slides"])
    moved = {"3 vs 2": np.inf, "4 vs 2": np.inf, "4 vs 3": np.inf}
    for i, p in np.argwhere(c3["kept"] & c4["kept"]):
        if c3["slides"][i, p]:
            for key, a, b in (("3 vs 2", c3["A"], A2), ("4 vs 2", c4["A"], A2), ("4 vs 3", c4["A"], c3["A"])):
                d = np.abs(a[i, p] - b[i, p]).max()
                moved[key] = min(moved[key], d)
                assert d > 1e-3, (variant, mu, key, i, p, d)
            assert np.abs(c4["step"][i, p] - c3["step"][i, p]).max() > 1e-6
        else:
            assert np.array_equal(c3["step"][i, p], cc.mode2_steps(variant)[i, p]) and np.array_equal(c4["step"][i, p], c3["step"][i, p])
    print("%s, mu %.1f: the least a sliding case moves A: %s" % (variant, mu, ", ".join("mode %s %.2e" % kv for kv in moved.items())))


def test_no_foot_slides_at_the_large_friction_coefficient():
    """MU_STICK: the cone is inactive in all 64 cases, so modes 3 and 4 ARE mode 2, bit for bit; the smaller coefficients are not such"""
    x, u, _ = cc.sliding_states()
    for mode in (3, 4):
        assert np.array_equal(cc.steps(cc.oracle(mode, cc.MU_STICK), x, u, mode), cc.mode2_steps())
        for mu in cc.MUS:
            assert not np.array_equal(cc.sliding_cases(mode, mu)["step"], cc.mode2_steps())


def test_the_limit_pattern_reaches_every_hinge_at_both_ends():
    x, u = cc.limit_states()
    cls, end = cc.limit_pattern()
    jr = cc.ol.joint_ranges()
    th, v = x[:, 7:cc.NQ], x[:, cc.NQ + 6:]
    for c, n in ((0, 2), (2, 2), (4, 2), (6, 2)):
        assert np.all((cls == c).sum(axis=0) == n)                     # every hinge is in every class, in two states
    assert np.allclose(th[cls == 0], (jr[:, 1] + 0.03 + 0 * th)[cls == 0], atol=1e-15) and np.all(v[cls == 0] == 1.5)
    assert np.allclose(th[cls == 4], (jr[:, 0] - 0.03 + 0 * th)[cls == 4], atol=1e-15) and np.all(v[cls == 4] == -1.5)
    assert np.allclose(th[cls == 2], (jr[:, 1] + 0.03 + 0 * th)[cls == 2], atol=1e-15) and np.all(v[cls == 2] == -0.2)
    on = cls == 6
    assert np.array_equal(th[on & (end > 0)], (jr[:, 1] + 0 * th)[on & (end > 0)]) and np.array_equal(th[on & (end < 0)], (jr[:, 0] + 0 * th)[on & (end < 0)])
    assert np.all(v[on] == 1.5 * end[on]) and (on & (end > 0)).any() and (on & (end < 0)).any()
    xm = dc.mid()[0]
    assert np.array_equal(x[:, :7], xm[:, :7]) and np.array_equal(x[:, 7:cc.NQ][cls % 2 == 1], xm[:, 7:cc.NQ][cls % 2 == 1])
    # the two halves of the per-side range table differ in the shoulder roll and yaw only (hinges 12, 13 against 16, 17): a swapped side
    # shows where one of those is stopped
    differ = [k for k in range(4) if not np.array_equal(jr[11 + k], jr[15 + k])] + [k for k in range(5) if not np.array_equal(jr[k], jr[5 + k])]
    assert differ == [1, 2]


@pytest.mark.parametrize("mode,k", LIMITS)
def test_limit_cases_stay_inside_the_caps(mode, k):
    c = cc.limit_cases(mode, k)
    assert np.all(np.isfinite(c["A"])) and np.all(np.isfinite(c["B"])) and np.all(np.isfinite(c["step"]))
    dropped, stopped, up, lo = cc.check_limit_caps(c["kept"], c["stopped"], (mode, k))
    st = c["stopped"] & c["kept"][:, :, None]
    slow = (st & (c["cls"] == 2)[:, None, :]).sum(); slow_all = c["kept"].sum(axis=1) @ (c["cls"] == 2).sum(axis=1)
    print("mode %d, k %g: %d of %d cases kept; %d hinge-cases stopped, %d distinct hinges at the upper end, %d at the lower; slowly returning "
          "hinges stopped %d of %d; shoulder hinges 12 13 16 17 stopped in %s cases; Jacobian drift %.1e; |A|max %.1f"
          % (mode, k, c["kept"].sum(), c["kept"].size, stopped, up, lo, slow, slow_all, st[:, :, [12, 13, 16, 17]].sum(axis=(0, 1)).tolist(), c["drift"], np.abs(c["A"]).max()))
    assert c["drift"] <= 1e-4
    if mode >= 3:                                                      # limits together with sliding feet
        o2 = cc.oracle(2, None, True, k)
        assert (np.abs(c["step"] - cc.steps(o2, c["x"], c["u"], 2)).max(axis=2) > 1e-6)[:, :3].sum() >= 24


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_the_rows_and_the_restoring_term_move_step_and_jacobians(mode):
    """limits on against limits off, and k = 625 against k = 0, on every kept case with a stopped hinge; the restoring term also decides:
    some slowly returning hinge (class 2) is constrained under k = 625 and free under k = 0"""
    c0, ck = cc.limit_cases(mode, 0.0), cc.limit_cases(mode, cc.K_STIFF[1])
    o = cc.oracle(mode, cc.MU_LIMITS if mode >= 3 else None)
    A_off, off = cc.jacobians(o, c0["x"], c0["u"])[0], cc.steps(o, c0["x"], c0["u"], mode)
    least = {"A, rows on vs off": np.inf, "step, rows on vs off": np.inf, "A, k": np.inf, "step, k": np.inf}
    n = 0
    for i, p in np.argwhere(c0["kept"] & ck["kept"]):
        for c in (c0, ck):
            if c["stopped"][i, p].any():
                least["A, rows on vs off"] = min(least["A, rows on vs off"], np.abs(c["A"][i, p] - A_off[i, p]).max())
                least["step, rows on vs off"] = min(least["step, rows on vs off"], np.abs(c["step"][i, p] - off[i, p]).max())
        if ck["stopped"][i, p].any():
            n += 1
            least["A, k"] = min(least["A, k"], np.abs(ck["A"][i, p] - c0["A"][i, p]).max())
            least["step, k"] = min(least["step, k"], np.abs(ck["step"][i, p] - c0["step"][i, p]).max())
    print("mode %d: %d kept cases with a stopped hinge; the least they move: %s" % (mode, n, ", ".join("%s %.2e" % kv for kv in least.items())))
    assert n >= 12 and min(least.values()) > 1e-3
    decided = (ck["stopped"] & ~c0["stopped"] & (c0["cls"] == 2)[:, None, :]).sum()
    print("mode %d: the restoring term alone constrains %d slowly returning hinge-cases" % (mode, decided))
    assert decided * 16 >= c0["kept"].size                             # (one in sixteen cases: 4 of 64, 1 of 16 in mode 0)


def _spread(o, c, mode, skip_x=None, skip_u=None):
    """(worst error of the AD Jacobians against central differences on the columns where the quotient has converged, the same on the other
    columns, their share), over the kept cases, relative to max(1, max |want|) of [A B]"""
    worst, coarse, n_coarse, n = 0.0, 0.0, 0, 0
    for i, p in np.argwhere(c["kept"]):
        use = np.ones(cc.NX + cc.NU, dtype=bool)
        if skip_x is not None:
            use[:cc.NX] = ~skip_x[i]
        if skip_u is not None:
            use[cc.NX:] = ~skip_u[i]
        want = np.concatenate([c["A"][i, p], c["B"][i, p]], axis=1)
        J, gap = cc.central_differences(o, c["x"][i], c["u"][i], cc.rows(mode)[p])
        e = np.abs(J - want).max(axis=0) / max(1.0, np.abs(want).max())
        ok = gap <= cc.FD_CONVERGED
        worst = max(worst, e[use & ok].max())
        coarse = max(coarse, e[use & ~ok].max(initial=0.0))
        n_coarse += int((use & ~ok).sum()); n += int(use.sum())
    return worst, coarse, n_coarse / n


# Parametrisations in which the difference quotient, not the AD, limits the agreement: the rigid double-support solve of mode 1 is stiff
# (|A|max 340) and the kinetic-friction solve at mu 0.7 less so; the rounding noise of their step, 1e-11 at the worst, is divided by the
# quotient's step.  Measured: 1.4e-9 and 1.6e-10 max(1, |want|).  The Jacobian bound of the GPU tests sits 7 x and 60 x above these instead
# of two orders.  It stays at the project's 1e-8 all the same: the analytic kernels, a third derivation, agree with the AD to 1e-12 there.
QUOTIENT_LIMITED = {("limits", 1, 0.0): 3e-9, ("limits", 1, 625.0): 3e-9, ("sliding", 4, "mid", 0.7): 3e-10}


def _assert_spread(key, tag, c, worst, coarse, share):
    """The bound on the contact Jacobians sits two orders above the spread of the oracle's two derivations wherever the difference quotient
    can tell: on the columns where it has converged (its fourth- and sixth-order forms agree to 1e-11).  On the others -- a branch of the
    step within a few difference steps of the state -- the quotient is the limit, not the AD: they are counted and held to 1e-6, far below
    what a branch flip moves."""
    print("%s: AD vs sixth-order central differences on %d kept cases, worst error relative to max(1, |want|) %.2e on the converged columns; "
          "%.2e on the %.2f %% of columns where the quotient has not converged" % (tag, c["kept"].sum(), worst, coarse, 100.0 * share))
    assert worst <= QUOTIENT_LIMITED.get(key, cc.JAC_TOL / 100.0) and coarse <= 1e-6 and share <= 0.01, (tag, worst, coarse, share)


@pytest.mark.parametrize("mode,variant,mu", SLIDING)
def test_sliding_ad_and_central_differences_agree(mode, variant, mu):
    """clamped: a control exactly ON a limit is the one place the two differ by design -- the difference steps outside, sees the clamp and
    halves the column, where AD and the kernels (strict comparison) return the unclamped one; those columns are left out"""
    c = cc.sliding_cases(mode, mu, variant)
    skip_u = dc.clamp_pattern()[2] if variant == "clamped" else None
    _assert_spread(("sliding", mode, variant, mu), "mode %d, %s, mu %.1f" % (mode, variant, mu), c, *_spread(cc.oracle(mode, mu), c, mode, skip_u=skip_u))


@pytest.mark.parametrize("mode,k", LIMITS)
def test_limit_ad_and_central_differences_agree(mode, k):
    """the angle column of a hinge exactly ON its limit (class 6) is left out: the difference steps past the limit with the hinge moving
    out, where it is stopped, while AD and the kernels differentiate the branch the state is in (strict comparison: free)"""
    c = cc.limit_cases(mode, k)
    skip_x = np.zeros((cc.NS, cc.NX), dtype=bool); skip_x[:, 7:cc.NQ] = c["cls"] == 6
    _assert_spread(("limits", mode, k), "mode %d, k %g" % (mode, k), c, *_spread(cc.oracle(mode, cc.MU_LIMITS if mode >= 3 else None, True, k), c, mode, skip_x=skip_x))
