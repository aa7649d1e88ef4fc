"""The inputs of tests/cost_envelope_cases.py can tell a right cost kernel from a wrong one -- checked on the CPU oracle and NumPy
alone, so that the GPU tests built on them (test_gpu_cost_envelope.py) cannot pass vacuously -- and the part of the oracle those
tests lean on that no golden reaches (nonzero u_ref, non-uniform R / Q / Qf, every row of the limit tables) against closed forms."""
import numpy as np
import pytest

import cost_envelope_cases as cc
import oracle_lib as ol

sc = cc.sc
B, N, SEED = 5, 4, 11


def _oracle(prob, b=0):
    o = ol.Oracle(prob["N"], prob["dt"]); o.set_problem(prob, b)
    return o


def _rolled_out(prob, B=B, seed=SEED):
    """synthetic_batch states rolled out with its controls (constraint-free step of the oracle): xs [B,N+1,51], us [B,N,19]"""
    o = _oracle(prob)
    x0, ui = sc.synthetic_batch(B, N, seed, o.grav_comp(sc.standing_state()))
    xs = np.zeros((B, N + 1, 51))
    for b in range(B):
        o.initialize(x0[b], ui[b]); xs[b] = o.get("xbar")
    return xs, ui


def _evaluate(prob, xs, us):
    """(total cost [B], lx [B,N+1,51], lu [B,N,19]) of the oracle, rollout b on reference set b"""
    B = xs.shape[0]
    cost, lx, lu = np.zeros(B), [], []
    for b in range(B):
        o = _oracle(prob, b); o.set_trajectory(xs[b], us[b]); o.cost_quadratics()
        cost[b] = o.total_cost(); lx.append(o.get("lx")); lu.append(o.get("lu"))
    return cost, np.array(lx), np.array(lu)


def _reldiff(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_scrambled_problem_is_what_it_says():
    for nb in (4, 5, 76):
        p = cc.scrambled_problem(nb, N, SEED)
        for key, n in (("Q", 51), ("R", 19), ("Qf", 51)):
            assert p[key].shape == (n,) and np.all(p[key] > 0) and len(np.unique(p[key])) == n
        ratio = p["Qf"] / p["Q"]
        assert len(np.unique(ratio)) == 51                                        # Qf is no multiple of Q
        w = np.array(p["task_weights"])
        assert np.all(w > 0) and len(np.unique(w)) == 6 and p["w_joint"] != p["w_ctrl"] and p["w_joint"] > 0 and p["w_ctrl"] > 0
        u = p["u_ref"]
        assert u.shape == (nb, N, 19) and np.all(u != 0) and np.all(np.abs(u) <= 0.3 * sc.CTRLRANGE) and len(np.unique(u)) == u.size
        x = p["x_ref"]
        assert x.shape == (nb, N + 1, 51) and np.abs(np.linalg.norm(x[..., 3:7], axis=-1) - 1).max() < 1e-15
        moving = [i for i in range(51) if i != 3]                                 # (the quaternion's w is 1 - O(angle^2))
        assert np.abs(x - sc.standing_state())[..., moving].min() > 0 and np.abs(x - sc.standing_state()).max() < 0.25
        for key in ("x_ref", "com_ref", "ee_ref", "com_vel_ref"):
            a = p[key].reshape(nb * (N + 1), -1)
            assert a.shape[0] == len(np.unique(a, axis=0))                        # another row for every rollout and knot
        st = p["stance"]
        assert st.shape == (nb, N + 1, 2) and st.dtype == np.int32
        assert {tuple(r) for r in st.reshape(-1, 2)} == {(1, 1), (1, 0), (0, 1), (0, 0)}
        assert all(not np.array_equal(st[b], st[(b + 1) % nb]) for b in range(nb))


@pytest.mark.parametrize("B,seed", [(5, 11), (4, 17)])       # the problems of the GPU tests: stage by stage, through a solve
def test_scrambled_weights_and_references_matter(B, seed):
    """Every rollout's total cost and gradient (lu; lx where Q is what changes, lu does not read it) move by more than 1e-3 relative
    when u_ref is zeroed, R or the joint block of Q is replaced by its mean, or the rollout reads the next reference set."""
    prob = cc.scrambled_problem(B, N, seed)
    xs, us = _rolled_out(prob, B, seed)
    cost, lx, lu = _evaluate(prob, xs, us)
    no_uref = dict(prob); no_uref["u_ref"] = np.zeros_like(prob["u_ref"])
    flat_R = dict(prob); flat_R["R"] = np.full(19, prob["R"].mean())
    flat_Q = dict(prob); flat_Q["Q"] = prob["Q"].copy(); flat_Q["Q"][7:26] = prob["Q"][7:26].mean()
    shifted = dict(prob)
    for key in ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref"):
        shifted[key] = np.roll(prob[key], -1, axis=0)                             # rollout b on set b + 1
    for label, other, grad in (("u_ref = 0", no_uref, "lu"), ("R -> mean", flat_R, "lu"), ("Q joints -> mean", flat_Q, "lx"), ("set b + 1", shifted, "lx")):
        c2, lx2, lu2 = _evaluate(other, xs, us)
        dc = np.abs(c2 - cost) / np.abs(cost)
        dg = [_reldiff(a, b_) for a, b_ in zip(*((lu2, lu) if grad == "lu" else (lx2, lx)))]
        print("%-17s total cost differs by %.2e .. %.2e relative, %s by %.2e .. %.2e" % (label, dc.min(), dc.max(), grad, min(dg), max(dg)))
        assert dc.min() > 1e-3 and min(dg) > 1e-3, (label, dc, dg)


def test_each_single_term_is_live_and_alone():
    c = cc.cost_golden()
    off = cc.golden_problem(c, N=N)
    assert off["task_weights"] == (0.0,) * 6
    o = _oracle(off)
    for x in c["x"]:
        for t in (3, N):
            for mode in (0, 1):
                lx, lu, lxx, luu = o.knot_quadratics(t, x, np.full(19, 7.0), mode)
                assert not lx.any() and not lu.any() and not lxx.any() and not luu.any()       # every task weight at 0 contributes exactly 0
    seen = set()
    for label, prob, names in cc.single_term_problems(c, N=N):
        w = np.array(prob["task_weights"])
        on = np.flatnonzero(w)
        assert len(on) == 1 and not prob["Q"].any() and not prob["Qf"].any() and not prob["R"].any() and prob["w_joint"] == 0.0 and prob["w_ctrl"] == 0.0
        seen.add(int(on[0]))
        o = _oracle(prob)
        for i, x in enumerate(c["x"]):
            lx, lu, lxx, luu = o.knot_quadratics(3, x, np.zeros(19), 0)
            g = sum(c["grad_" + n][i] for n in names)
            H = sum(c["hess_" + n][i] for n in names)
            if label == "upright" and np.array_equal(x[3:7], [1.0, 0.0, 0.0, 0.0]):
                # golden state 0 is exactly upright: the residual, and with it the gradient, is 0 there; the curvature is not
                assert i == 0 and not lx.any() and np.abs(lxx).max() > 1e-3
            else:
                assert np.abs(lx).max() > 1e-3, (label, i)
            assert np.abs(lx - g).max() <= 1e-9 * max(1.0, np.abs(g).max()) and np.abs(lxx - H).max() <= 1e-9 * max(1.0, np.abs(H).max()), label
            assert not lu.any() and not luu.any()
    assert seen == set(range(6))


def test_tracking_terms_match_the_closed_form():
    prob = cc.tracking_only(cc.scrambled_problem(B, N, SEED))
    xs, us = _rolled_out(prob)
    worst = 0.0
    for b in range(B):
        o = _oracle(prob, b); o.set_trajectory(xs[b], us[b]); o.cost_quadratics()
        lx, lu, lxx, luu, cost = cc.tracking_closed_form(prob, b, xs[b], us[b])
        for name, want in (("lx", lx), ("lu", lu), ("lxx", lxx), ("luu", luu)):
            err = np.abs(o.get(name) - want).max()
            worst = max(worst, err)
            assert err <= 1e-12, (name, b, err)
        assert np.abs(lu - prob["R"] * us[b]).max() > 1e-2 and np.abs(lx[N] - prob["Q"] * (xs[b, N] - prob["x_ref"][b, N])).max() > 1e-2     # u_ref and Qf are in it
        assert abs(o.total_cost() - cost) <= 1e-12 * abs(cost)
    print("tracking terms, oracle vs NumPy: worst absolute error %.2e" % worst)


def test_limit_sweep_is_live_and_matches_the_closed_form():
    c = cc.cost_golden()
    jr, cr = c["jrange"], c["ctrlrange"]
    assert jr.shape == (19, 2) and cr.shape == (19, 2) and np.array_equal(jr, ol.joint_ranges())
    X, U, cases = cc.limit_sweep(N)
    assert X.shape == (76, N + 1, 51) and U.shape == (76, N, 19) and len(cases) == 76
    prob = cc.golden_problem(c, N=N)
    prob["w_joint"], prob["w_ctrl"] = 1300.0, 1700.0
    o = _oracle(prob)
    worst = 0.0
    for r, (kind, j, side, v) in enumerate(cases):
        o.set_trajectory(X[r], U[r]); o.cost_quadratics()
        lx, lu, lxx, luu = o.get("lx"), o.get("lu"), o.get("lxx"), o.get("luu")
        gx = np.zeros((N + 1, 51)); hx = np.zeros((N + 1, 51)); gu = np.zeros((N, 19)); hu = np.zeros((N, 19)); cost = 0.0
        for t in range(N + 1):
            gx[t, 7:26] = cc.pen_grad(X[r, t, 7:26], jr, prob["w_joint"]); hx[t, 7:26] = cc.pen_hess(X[r, t, 7:26], jr, prob["w_joint"])
            cost += cc.pen(X[r, t, 7:26], jr, prob["w_joint"])
            if t < N:
                gu[t] = cc.pen_grad(U[r, t], cr, prob["w_ctrl"]); hu[t] = cc.pen_hess(U[r, t], cr, prob["w_ctrl"])
                cost += cc.pen(U[r, t], cr, prob["w_ctrl"])
        # exactly one entry of the sweep's rollout is active: the one it names, on the side it names
        assert np.count_nonzero(gx) + np.count_nonzero(gu) == 1 and np.count_nonzero(hx) + np.count_nonzero(hu) == 1
        g = gx[1, 7 + j] if kind == "joint" else gu[1, j]
        assert (g < -1.0) if side == 0 else (g > 1.0), (r, kind, j, side, g)
        diag = lxx[:, np.arange(51), np.arange(51)]
        for got, want in ((lx, gx), (lu, gu), (diag, hx), (luu, hu)):
            worst = max(worst, np.abs(got - want).max())
            assert np.abs(got - want).max() <= 1e-10, (r, kind, j, side)
        assert np.count_nonzero(lxx) == np.count_nonzero(hx)                     # nothing off the diagonal
        assert abs(o.total_cost() - cost) <= 1e-12 * cost and cost > 0
    print("limit sweep, oracle vs closed form: worst absolute error %.2e" % worst)
