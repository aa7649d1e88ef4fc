"""The inputs of tests/dynamics_envelope_cases.py can tell a right step / linearisation kernel from a wrong one, and the oracle can be
trusted on them -- checked on the CPU oracle alone, so that the GPU tests built on them (test_gpu_dynamics_envelope.py) cannot pass
vacuously: two independent derivations of the Jacobians agree, forward differences agree coarsely, and every factor the groups are
there for (2 / |q|, the sign of q, the torque clamp, the velocity-product terms, both sides of the small-spin branch, a released
foot) moves the result by far more than the GPU tests' tolerances."""
import numpy as np
import pytest

import dynamics_envelope_cases as dc
import oracle_lib as ol

NQ = dc.NQ


def _relmax(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", dc.FREE_GROUPS)
def test_ad_and_the_tangent_scheme_agree(name):
    x, u = dc.group(name)
    A, B = dc.group_ad(name)
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(B))
    worst = 0.0
    for i in range(dc.NS):
        A2, B2 = ol.tangent_scheme_jacobians(x[i], u[i], dc.H, dc.GRAVITY)
        for got, want in ((A2, A[i]), (B2, B[i])):
            worst = max(worst, _relmax(got, want))
            assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (name, i)
    print("%s: AD vs tangent scheme, worst error relative to max(1, |want|) %.2e; |A|max %.1f" % (name, worst, np.abs(A).max()))


@pytest.mark.parametrize("name", dc.FREE_GROUPS)
def test_ad_and_forward_differences_agree_coarsely(name):
    """eps = 1e-6, 1e-4 of the matrix's largest entry.  A control exactly ON its upper limit is the one place the two differ by design: the
    forward difference steps outside, sees the clamp and returns a zero column, where AD and the kernels (strict comparison: on the limit is
    inside) return the unclamped one -- those columns are left out here and pinned in test_clamped_columns_are_zero..."""
    x, u = dc.group(name)
    A, B = dc.group_ad(name)
    Af, Bf = dc.oracle_jacobians(x, u, jac_mode=1, fd_eps=1e-6)
    cols = np.ones((dc.NS, dc.NU), dtype=bool)
    if name == "clamped":
        cols = ~(dc.clamp_pattern()[2] & (u > 0))
        assert np.abs(Bf[~cols[:, None, :].repeat(51, 1)]).max() == 0.0 and (~cols).sum() >= 4
    worst = 0.0
    for i in range(dc.NS):
        for got, want in ((Af[i], A[i]), (Bf[i][:, cols[i]], B[i][:, cols[i]])):
            r = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, r)
            assert r <= 1e-4, (name, i, r)
    print("%s: AD vs forward differences, worst relative error %.2e" % (name, worst))


@pytest.mark.parametrize("variant", ["mid", "nonunit", "clamped"])
@pytest.mark.parametrize("mode", [1, 2])
def test_contact_ad_and_forward_differences_agree_coarsely_on_the_kept_cases(mode, variant):
    x, u, kept, A, B, beyond = dc.mid_cases(mode, variant)
    Af, Bf = dc.oracle_jacobians(x, u, mode=mode, jac_mode=1, fd_eps=1e-6)
    plus_tie = (dc.clamp_pattern()[2] & (u > 0)) if variant == "clamped" else np.zeros((dc.NS, dc.NU), dtype=bool)
    worst = 0.0
    assert np.all(np.isfinite(A)) and np.all(np.isfinite(B))
    for i, p in np.argwhere(kept):
        c = ~plus_tie[i]
        for got, want in ((Af[i, p], A[i, p]), (Bf[i, p][:, c], B[i, p][:, c])):
            r = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, r)
            assert r <= 1e-4, (mode, variant, i, p, r)
    print("mode %d, %s: AD vs forward differences on %d kept cases, worst relative error %.2e; |A|max %.1f" % (mode, variant, kept.sum(), worst, np.abs(A).max()))


def test_a_non_unit_quaternion_scales_the_quaternion_columns():
    """f(c q) = f(q): the quaternion columns of A at c q are those at q divided by c (the 2 / |q| of Hq), nothing else moves"""
    (xw, _), (xn, _) = dc.group("wide"), dc.group("nonunit")
    assert np.abs(np.linalg.norm(xw[:, 3:7], axis=1) - 1.0).max() < 1e-15
    assert np.abs(np.linalg.norm(xn[:, 3:7], axis=1) - dc.QUAT_SCALE).max() < 1e-15 and np.abs(dc.QUAT_SCALE - 1.0).min() >= 0.05
    (Aw, Bw), (An, Bn) = dc.group_ad("wide"), dc.group_ad("nonunit")
    other = np.r_[0:3, 7:51]
    for i in range(dc.NS):
        assert np.abs(An[i][:, 3:7] - Aw[i][:, 3:7]).max() > 1e-3, i
        assert np.abs(An[i][:, 3:7] * dc.QUAT_SCALE[i] - Aw[i][:, 3:7]).max() <= 1e-12 * np.abs(Aw[i]).max()
        assert np.abs(An[i][:, other] - Aw[i][:, other]).max() <= 1e-12 * np.abs(Aw[i]).max() and np.abs(Bn[i] - Bw[i]).max() <= 1e-12


def test_a_negated_quaternion_flips_the_quaternion_columns():
    """f(-q) = f(q) with q' negated: the quaternion columns and the quaternion rows of A change sign (their 4 x 4 crossing does not)"""
    (xw, _), (xm, _) = dc.group("wide"), dc.group("negq")
    assert (xw[:, 3] > 0).sum() >= 4 and (xw[:, 3] < 0).sum() >= 1 and np.array_equal(xm[:, 3:7], -xw[:, 3:7])
    assert abs(xw[0, 3]) < 1e-3                                       # the rotation next to pi
    (Aw, Bw), (Am, Bm) = dc.group_ad("wide"), dc.group_ad("negq")
    sgn = np.ones(51); sgn[3:7] = -1.0
    flip = sgn[:, None] * sgn[None, :]
    for i in range(dc.NS):
        assert np.abs(Aw[i][:, 3:7]).max() > 1e-3
        assert np.abs(Am[i] - flip * Aw[i]).max() <= 1e-12 * np.abs(Aw[i]).max() and np.abs(Bm[i] - sgn[:, None] * Bw[i]).max() <= 1e-12


def test_clamped_columns_are_zero_live_when_pulled_inside_and_a_control_on_its_limit_is_inside():
    """The oracle's clamp and the kernel's free_u use the same strict comparisons (h1_dynamics.hpp h1_step, h1_linearize_dev.h lin_prologue):
    a control exactly on a limit is inside, its column of B is the unclamped one.  (The reference's own Jacobians are forward differences:
    on the upper limit they see the clamp, on the lower one they do not -- no side of that tie is `the' derivative; oracle and kernel agree.)"""
    x, u, beyond = dc.clamped()
    above, below, on = dc.clamp_pattern()
    assert np.array_equal(beyond, above | below) and above.sum(0).min() >= 1 and below.sum(0).min() >= 1 and on.sum(1).min() >= 1
    assert np.all(u[above] > np.broadcast_to(dc.sc.CTRLRANGE, u.shape)[above]) and np.all(u[below] < -np.broadcast_to(dc.sc.CTRLRANGE, u.shape)[below])
    assert np.array_equal(np.abs(u[on]), np.broadcast_to(dc.sc.CTRLRANGE, u.shape)[on]) and (u[on] > 0).any() and (u[on] < 0).any()
    A, B = dc.group_ad("clamped")
    Ai, Bi = dc.oracle_jacobians(x, dc.pulled_inside(u))
    for i in range(dc.NS):
        assert np.all(B[i][:, beyond[i]] == 0.0)
        assert np.abs(Bi[i][:, beyond[i]]).max(axis=0).min() > 1e-3 and np.abs(B[i][:, ~beyond[i]]).max(axis=0).min() > 1e-3
        assert np.abs(B[i][:, on[i]]).max(axis=0).min() > 1e-3          # the tie: inside
    for mode in (1, 2):                                               # the same through the contact modes
        xm, um, kept, Am, Bm, bey = dc.mid_cases(mode, "clamped")
        Ai, Bi = dc.oracle_jacobians(xm, dc.pulled_inside(um), mode=mode)
        for i, p in np.argwhere(kept):
            assert np.all(Bm[i, p][:, bey[i]] == 0.0) and np.abs(Bi[i, p][:, bey[i]]).max(axis=0).min() > 1e-3


def test_velocity_product_terms_carry_weight():
    x, u = dc.group("wide")
    A, _ = dc.group_ad("wide")
    x0 = x.copy(); x0[:, NQ:] = 0.0
    A0, _ = dc.oracle_jacobians(x0, u)
    d = np.abs(A - A0).reshape(dc.NS, -1).max(axis=1)
    print("zeroing the velocities moves A by %.2f .. %.2f" % (d.min(), d.max()))
    assert d.min() > 1e-3
    # far from zero: every hinge sits beyond 0.3 rad in some state, and a sine of 0.9 occurs
    assert np.abs(x[:, 7:NQ]).max(axis=0).min() > 0.3 and np.abs(np.sin(x[:, 7:NQ])).max() > 0.9
    jr = ol.joint_ranges()
    assert np.all(x[:, 7:NQ] > jr[:, 0]) and np.all(x[:, 7:NQ] < jr[:, 1])


def test_spin_states_sit_on_both_sides_of_the_taylor_threshold():
    x, u = dc.group("spin")
    s = dc.spin_s(x, u)
    assert np.abs(s / dc.SPIN_S - 1.0).max() < 1e-6
    t = dc.SPIN_THRESHOLD
    assert (s < t).sum() >= 4 and (s >= t).sum() >= 4
    assert ((s < t) & (s > t / 2)).any() and ((s >= t) & (s < 2 * t)).any() and (s > 1e-2).any()
    assert dc.spin_s(*dc.group("wide")).min() > 1e-3                 # (the other groups never come near the branch)
    # The quaternion rows beside the quaternion columns, which the GPU test holds to 1e-12 max(1, |A|max): the two derivations agree on
    # them to 1e-14 of that scale, and the dso term of dE -- h w'_i dso 2 h^2 w'_j, dso = -1 / 48 + ... -- is worth far more than the bound
    # just below the threshold: with the sign of 1 / 48 wrong, column w_j of those rows moves by (2 / 48) 2 h s |n_j| (n = w' / |w'|) in
    # norm, so its largest entry by about half of that or more (d w' / d w_j = e_j + O(h)).
    A, _ = dc.group_ad("spin")
    o = dc.oracle()
    for i in range(dc.NS):
        A2, _ = ol.tangent_scheme_jacobians(x[i], u[i], dc.H, dc.GRAVITY)
        assert np.abs(A2[3:7, 7:] - A[i][3:7, 7:]).max() <= 1e-14 * max(1.0, np.abs(A[i]).max()), i
    i = int(np.argmax(np.where(s < t, s, 0.0)))
    n = o.step(x[i], u[i])[NQ + 3:NQ + 6]; n /= np.linalg.norm(n)
    moved = 0.5 * (2.0 / 48.0) * 2.0 * dc.H * s[i] * np.abs(n).max()
    print("spin state %d, s = %.2e: a wrong sign of the first dso coefficient moves a quaternion-row entry by about %.2e or more; bound %.2e"
          % (i, s[i], moved, 1e-12 * np.abs(A[i]).max()))
    assert moved > 10 * 1e-12 * max(1.0, np.abs(A[i]).max())
    xr, ur = dc.rest()
    for g in ((0.0, 0.0, 0.0), dc.GRAVITY):                          # at rest, without torque: free fall -- s is an exact zero
        assert np.all(dc.spin_s(xr, ur, dc.oracle(gravity=g)) == 0.0)
        A, B = dc.oracle_jacobians(xr, ur, gravity=g)
        assert np.all(np.isfinite(A)) and np.all(np.isfinite(B))
        for i in range(len(xr)):
            A2, B2 = ol.tangent_scheme_jacobians(xr[i], ur[i], dc.H, g)
            assert _relmax(A2, A[i]) <= 1e-12 and _relmax(B2, B[i]) <= 1e-12


def test_contact_filter_keeps_nearly_everything_and_mode_2_releases_feet():
    x, u = dc.mid()
    jr = ol.joint_ranges()
    assert np.all(x[:, 7:NQ] > jr[:, 0]) and np.all(x[:, 7:NQ] < jr[:, 1])
    dropped = total = 0
    for mode in (1, 2):
        for variant in ("mid", "nonunit", "clamped"):
            kept = dc.mid_cases(mode, variant)[2]
            if variant == "mid":
                dropped += int((~kept).sum()); total += kept.size
            assert (~kept).sum() <= 0.1 * kept.size, (mode, variant)
    print("contact filter: %d of %d (state, mode, pattern) triples dropped" % (dropped, total))
    assert dropped <= 0.1 * total
    k1, k2 = dc.mid_cases(1)[2], dc.mid_cases(2)[2]
    o1, o2 = dc.oracle(mode=1), dc.oracle(mode=2)
    free = dc.oracle()
    released = 0
    for i, p in np.argwhere(k1 & k2):
        st = dc.STANCE_ROWS[p]
        f1, f2 = o1.step_stance(x[i], u[i], st), o2.step_stance(x[i], u[i], st)
        released += int(st.any() and np.abs(f1 - f2).max() > 1e-6)
        if st.any():
            assert np.abs(f1 - free.step(x[i], u[i])).max() > 1e-3          # the stance rows do something
    print("mode 2 releases a foot in %d kept cases" % released)
    assert released >= 2
