"""The device-resident plant on the GPU (include/ilqr_hip.h ilqr_hip_plant_*; csrc/plant_kernels.hip).

The yardstick is never the new kernel: it is the composition of entry points that existed before it, TEACHER-FORCED.  Handle A (dt = 0.02)
solves and carries the plant; handle P is created with dt = 0.02 / substeps and the same contact, limit, friction and gravity settings.
After every advance the plant state is downloaded, and the state the advance should have produced is computed from the state it STARTED
from: u = A.compute_control(x), x <- P.step / step_stance / step_geometry(x, u), `substeps` times (u held, or re-evaluated per substep in
feedback mode 1).  Divergence of the closed loop never enters a tolerance.

Tolerances, from the parity tests of these two stages at the parent commit:
  u       np.allclose(rtol=1e-12, atol=1e-12)   tests/test_gpu_parity.py:819 (test_warm_start_mpc_step_and_control_law)
  x_next  1e-11 absolute per plant step          tests/test_gpu_parity.py:90  (test_step_matches_oracle_and_kane_golden), times substeps
Stance flags must agree for every rollout and every step."""
import os

import numpy as np
import pytest

from conftest import load_package

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
pkg = load_package()
sc = pkg.scenario
NX, NU, NQ, NV = 51, 19, 26, 25
DT = 0.02
U_TOL = dict(rtol=1e-12, atol=1e-12)      # tests/test_gpu_parity.py:819
X_TOL_PER_STEP = 1e-11                    # tests/test_gpu_parity.py:90
PER_ROLLOUT = ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref")


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _pair(B, N, substeps, mode=0, limits=False, mu=None, iters=2):
    """(A, P): the solving handle and the handle that supplies the plant step at the physics step"""
    sv = _sv()
    A, P = sv.BatchedILQR(B, N=N, dt=DT), sv.BatchedILQR(B, N=N, dt=DT / substeps)
    for s in (A, P):
        s.set_contact_mode(mode)
        if mu is not None:
            s.set_friction(mu)
        if limits:
            s.set_joint_limits(True)
    A.set_max_iterations(iters)
    return A, P


def _host_advance(A, P, x, alive, substeps, fb, source, mode, flags):
    """what one advance has to produce from the state x it starts from (behind the kick): (x_next, u, stance, alive)"""
    xc, u, st = x.copy(), None, np.asarray(flags, dtype=np.int32).copy()
    for k in range(substeps):
        if k == 0 or fb:
            u = A.compute_control(xc)
            u[~np.isfinite(u).all(axis=1)] = 0.0                      # main/humanoid_mpc.cpp:162-165
        if mode and source == "geometry":
            xc, st = P.step_geometry(xc, u)
        elif mode:
            xn = np.empty_like(xc)
            for l, r in {(int(a), int(b)) for a, b in flags}:        # step_stance takes one flag pair per call
                idx = np.where((flags[:, 0] == l) & (flags[:, 1] == r))[0]
                xn[idx] = P.step_stance(xc[idx], u[idx], l, r)
            xc = xn
        else:
            xc = P.step(xc, u)
    ok = alive.astype(bool) & np.isfinite(x).all(axis=1) & np.isfinite(xc).all(axis=1)
    xc[~ok] = x[~ok]; u = u.copy(); u[~ok] = 0.0
    return xc, u, st, ok.astype(np.int32)


def _closed_loop(A, P, probs, x0, ui, steps, substeps, fb, source="schedule", mode=0, kicks=None, ring=None):
    """teacher-forced closed loop; returns the per-step downloads for further checks"""
    kicks = kicks or {}
    A.plant_configure(substeps, fb, source)
    A.plant_set_history(steps if ring is None else ring)
    A.set_problem(probs[0]); P.set_problem(probs[0])
    A.initialize(x0, ui); A.solve(x0)
    A.plant_reset(x0)
    x_prev, alive = x0.copy(), np.ones(len(x0), dtype=np.int32)
    seen = dict(x=[], u=[], stance=[], worst_x=0.0)
    for k in range(steps):
        if k > 0:
            A.set_problem(probs[k]); P.set_problem(probs[k])
            A.initialize_warm_from_plant(); A.solve(None)
        x_start = x_prev.copy()
        if k in kicks:
            A.plant_kick(kicks[k])
            x_start[:, NQ:] += kicks[k]                               # the host path: add the kick to the state of that step
        st_row = probs[k]["stance"][:, 0] if probs[k]["stance"].shape[0] > 1 else np.repeat(probs[k]["stance"][:1, 0], len(x0), axis=0)
        want_x, want_u, want_st, want_alive = _host_advance(A, P, x_start, alive, substeps, fb, source, mode, st_row)
        A.plant_advance()
        got_x, got_u, got_st, got_alive = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive()
        err = np.abs(got_x - want_x).max()
        print("step %d: |dx| %.3e  |du| %.3e  alive %d/%d" % (k, err, np.abs(got_u - want_u).max(), got_alive.sum(), len(x0)))
        assert np.array_equal(got_alive, want_alive), k
        assert np.allclose(got_u, want_u, **U_TOL), (k, np.abs(got_u - want_u).max())
        assert err < X_TOL_PER_STEP * substeps, (k, err)
        live = want_alive.astype(bool)
        if mode:
            assert np.array_equal(got_st[live], want_st[live]), k      # every live rollout, every step: nothing is left out
        seen["x"].append(x_start); seen["u"].append(got_u); seen["stance"].append(got_st); seen["worst_x"] = max(seen["worst_x"], err)
        x_prev, alive = got_x, got_alive
    seen["final"] = x_prev
    return seen


def _standing(B, N, seed=3, gravity=(0.0, 0.0, -9.81)):
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=gravity)
    ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
    x0, ui = sc.synthetic_batch(B, N, seed, ug)
    return prob, x0, ui


@pytest.mark.parametrize("substeps,fb", [(1, 0), (4, 0), (1, 1), (4, 1)])
def test_free_plant_matches_the_host_composition(substeps, fb):
    B, N, steps = 64, 25, 6
    prob, x0, ui = _standing(B, N)
    A, P = _pair(B, N, substeps)
    seen = _closed_loop(A, P, [prob] * steps, x0, ui, steps, substeps, fb, ring=steps + 5)
    # history: the ring equals the per-step downloads, and asking for more rows than were recorded returns the recorded count
    hx, hu = A.plant_history()
    assert hx.shape == (steps, B, NX) and hu.shape == (steps, B, NU)
    assert np.array_equal(hx, np.array(seen["x"])) and np.array_equal(hu, np.array(seen["u"]))
    assert np.abs(seen["final"] - x0).max() > 1e-3      # the plant moved
    A.close(); P.close()


def test_contact_mode_2_on_the_advancing_schedule():
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    B, N, steps, substeps = 64, 25, 6, 2
    long_prob, x0, ui_long, t0 = sc.walking_batch(B, N + steps, 5, os.path.join(G, "refdata_golden.npz"), sv, rf)
    probs = []
    for k in range(steps):      # receding horizon: the window of step k starts k rows later, the schedule row with it
        p = dict(long_prob); p["N"] = N
        for key in PER_ROLLOUT:
            p[key] = np.ascontiguousarray(long_prob[key][:, k:k + (N if key == "u_ref" else N + 1)])
        probs.append(p)
    rows = np.array([p["stance"][:, 0] for p in probs])
    assert (rows != rows[0]).any() and 0 < rows.sum() < rows.size      # the row advances, and both kinds of flag occur
    A, P = _pair(B, N, substeps, mode=2)
    _closed_loop(A, P, probs, x0, np.ascontiguousarray(ui_long[:, :N]), steps, substeps, 0, mode=2)
    A.close(); P.close()


def _geometry_states(P, count, rng):
    """the initial states of tests/test_gpu_stance_geometry.py (recorded walking rows, raised / lowered / tilted, random velocities); a state
    whose stance flags a 1e-9 perturbation flips on handle P is left out of the INPUT set"""
    r = np.load(os.path.join(G, "refdata_golden.npz"))
    q = r["q_ref2_mj_full"]
    rows = [q]
    for dz in (5e-4, -5e-4, 5e-3, -5e-3):
        qq = q.copy(); qq[:, 2] += dz; rows.append(qq)
    q = np.concatenate(rows)
    x = np.zeros((len(q), NX)); x[:, :NQ] = q
    x = x[rng.choice(len(x), 4 * count, replace=False)]
    x[:, NQ:] = rng.uniform(-0.3, 0.3, size=(len(x), NX - NQ))
    u = np.zeros((len(x), NU))
    base = P.step_geometry(x, u)[1]
    stable = np.ones(len(x), dtype=bool)
    for sign in (1.0, -1.0):
        for cols in ((2,), tuple(range(3, 7)), tuple(range(7, 17))):      # base height, base orientation, leg hinges
            xp = x.copy(); xp[:, list(cols)] += sign * 1e-9
            stable &= (P.step_geometry(xp, u)[1] == base).all(axis=1)
    x = x[stable]
    assert len(x) >= count
    return x[:count]


def test_contact_mode_3_on_geometry_with_joint_limit_rows():
    sv = _sv()
    B, N, steps, substeps = 64, 25, 6, 2
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    A, P = _pair(B, N, substeps, mode=3, limits=True, mu=0.3)
    x0 = _geometry_states(P, B, np.random.default_rng(14))
    ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
    ui = np.tile(ug, (B, N, 1))
    seen = _closed_loop(A, P, [prob] * steps, x0, ui, steps, substeps, 0, source="geometry", mode=3)
    flags = np.array(seen["stance"])
    assert 0 < flags.sum() < flags.size      # feet on the floor and feet in the air both occur
    A.close(); P.close()


def test_warm_start_from_the_plant_is_the_resident_warm_start():
    B, N = 8, 25
    prob, x0, ui = _standing(B, N, seed=4)
    A, P = _pair(B, N, 1)
    _closed_loop(A, P, [prob] * 2, x0, ui, 2, 1, 0)
    xb0, ub0 = A.xbar(), A.ubar()
    A.initialize_warm_from_plant()
    xb1, ub1 = A.xbar(), A.ubar()
    A.set_trajectory(xb0, ub0)                          # back to the solution both warm starts shift
    A.initialize_warm_resident(A.plant_state())
    xb2, ub2 = A.xbar(), A.ubar()
    assert np.array_equal(xb1, xb2) and np.array_equal(ub1, ub2)
    assert np.array_equal(xb1[:, 0], A.plant_state()) and not np.array_equal(xb1, xb0)
    A.close(); P.close()


def test_kick_is_the_host_paths_velocity_push():
    """the push of tests/test_gpu_parity.py:976-978: 0.6 m/s sideways on the pelvis, at step 2"""
    B, N, steps = 64, 25, 4
    prob, x0, ui = _standing(B, N, seed=5)
    A, P = _pair(B, N, 1, mode=2)
    dv = np.zeros((B, NV)); dv[:, 1] = 0.6
    seen = _closed_loop(A, P, [prob] * steps, x0, ui, steps, 1, 0, mode=2, kicks={2: dv})
    hx, hu = A.plant_history()
    assert np.array_equal(hx, np.array(seen["x"]))      # the ring holds the kicked state: what the control law saw
    assert seen["x"][2][:, 27].mean() > 0.3             # ... and it is a push
    # one-shot: the kick is gone after the advance that applied it (step 3 above was checked without one)
    A.close(); P.close()


def test_non_finite_state_freezes_one_rollout_and_no_other():
    B, N, steps, bad = 8, 25, 4, 3
    prob, x0, ui = _standing(B, N, seed=6)
    out = {}
    for poisoned in (False, True):
        sv = _sv()
        A = sv.BatchedILQR(B, N=N, dt=DT); A.set_max_iterations(3)
        A.plant_configure(2, 1, "schedule"); A.plant_set_history(2)
        A.set_problem(prob); A.initialize(x0, ui); A.solve(x0)
        xp = x0.copy()
        if poisoned:
            xp[bad, 9] = np.nan
        A.plant_reset(xp)
        xs, us, al = [], [], []
        for k in range(steps):
            if k > 0:
                A.initialize_warm_from_plant(); A.solve(None)
            A.plant_advance()
            xs.append(A.plant_state()); us.append(A.plant_control()); al.append(A.plant_alive())
        hx, hu = A.plant_history()
        # the ring has two rows: the last two advances, oldest first
        assert hx.shape[0] == 2 and np.array_equal(hx[1], xs[-2], equal_nan=True) and np.array_equal(hu[1], us[-1]) and np.array_equal(hu[0], us[-2])
        out[poisoned] = (np.array(xs), np.array(us), np.array(al))
        A.close()
    xs, us, al = out[True]
    assert np.all(al[:, bad] == 0) and np.all(us[:, bad] == 0.0)
    assert all(np.array_equal(x[bad], np.where(np.arange(NX) == 9, np.nan, x0[bad]), equal_nan=True) for x in xs)      # frozen where it was
    keep = np.arange(B) != bad
    assert np.all(al[:, keep] == 1) and np.all(out[False][2] == 1)
    assert np.array_equal(xs[:, keep], out[False][0][:, keep]) and np.array_equal(us[:, keep], out[False][1][:, keep])      # bit for bit


def test_runner_resident_and_host_visit_the_same_first_state(tmp_path):
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    B, N, steps = 4, 25, 4
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    ug = sv.gravity_compensation(sc.standing_state(), base["gravity"])
    x0, ui = sc.synthetic_batch(B, N, 0, ug)
    res = {}
    for resident in (False, True):
        s = sv.BatchedILQR(B, N=N, dt=DT); s.set_max_iterations(3); s.set_contact_mode(2)
        run = ml.MPCRunner(s, rd, base, log_dir=str(tmp_path / str(resident)), log_rollouts=(0, 2), resident=resident, substeps=1, feedback_mode=0)
        res[resident] = run.run(x0, steps, u_init=ui)
        run.close(); s.close()
    err = np.abs(res[True][0][1] - res[False][0][1]).max()
    print("first-step state, resident vs host: %.3e" % err)
    assert np.array_equal(res[True][0][0], res[False][0][0]) and err < X_TOL_PER_STEP
    assert np.allclose(res[True][1][0], res[False][1][0], **U_TOL)
    assert res[True][0].shape == res[False][0].shape == (steps + 1, B, NX) and np.all(np.isfinite(res[True][0]))
    for b in (0, 2):
        for name in ("mpc_log.csv", "q_optimal.csv", "u_optimal.csv"):
            a = (tmp_path / "False" / ("rollout_%d" % b) / name).read_text().splitlines()
            r = (tmp_path / "True" / ("rollout_%d" % b) / name).read_text().splitlines()
            assert a[0] == r[0] and len(a) == len(r) == steps + 1, (b, name)


def test_gating_of_the_launching_calls():
    sv = _sv()
    B, N = 2, 25
    prob, x0, ui = _standing(B, N, seed=7)
    with env(ILQR_ENV_PER_CALL="1"):
        s = sv.BatchedILQR(B, N=N, dt=DT); s.set_max_iterations(2); s.set_problem(prob)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            s.plant_advance()                                   # neither a solve nor a reset
        s.plant_reset(x0)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            s.plant_advance()                                   # a reset, but no solve yet
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            s.initialize_warm_from_plant()                      # nothing to shift
        s.initialize(x0, ui); s.solve(x0)
        with env(ILQR_BACKWARD="valu"):                         # a family the product library does not hold
            for call in (s.plant_advance, s.initialize_warm_from_plant):
                with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED.*kernel family"):
                    call()
            assert np.array_equal(s.plant_state(), x0) and np.all(s.plant_alive() == 1)      # the getters keep answering
        s.plant_advance()
        assert not np.array_equal(s.plant_state(), x0)
        s.set_contact_mode(1)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            s.plant_configure(1, 0, "geometry")                 # a welded foot never leaves (as ilqr_hip_set_stance_source)
        for bad in ((0, 0, "schedule"), (1, 2, "schedule")):
            with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
                s.plant_configure(*bad)
        s.close()
