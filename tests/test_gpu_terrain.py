"""A floor of its own height under each foot of the resident plant, on the GPU (include/ilqr_hip.h ilqr_hip_plant_set_terrain,
ilqr_hip_step_terrain; csrc/plant_kernels.hip k_plant_follow_t, k_step_t).

The ground truth is in two layers, as for the other tables:
  * ilqr_hip_step_terrain: its flags against the host statement of the rule (ilqr_hip_terrain_stance, held to its definition without a GPU
    in tests/test_terrain_cpu.py), exactly; its x_next against the library's own step under those flags (ilqr_hip_step_stance);
  * the plant kernel against the TEACHER-FORCED composition compute_control -> step_terrain per substep on a handle at DT / SUBSTEPS, every
    interval of a follow(0, 4) held to the composition from the ring row it started from; under all seven tables against
    terrain_stance -> step_joints, with the other tables' chains as tests/test_gpu_joints.py composes them.

Shape: B = 5 rollouts (one partial workgroup at feedback mode 0, one full and one partial at mode 1), N = 6, SUBSTEPS = 3, four intervals;
contact mode 2, and mode 4 with joint-limit rows.  Rollout b starts from envelope state (b + 2) % 16; the plant's contact source is GEOMETRY.

Bounds: the module's step against the library's step cc.STEP_TOL = 1e-9 relative to max(1, max |want|) (the steps of modes 2 and 4 have rows;
tests/test_gpu_joints.py); plant: U_TOL = 1e-12 on the reported control and cc.STEP_TOL x SUBSTEPS = 3e-9 relative on the state per interval.
Decisions: every decision of the step test is made 5 mm from the floor and from the edge (the issue asks for 1 mm at least); the plant tests
print the smallest distance |clearance - floor| and |ankle_x - edge_x| their composition met and require 1e-6 m, over 100 times what a state
within the 3e-9 bound can move either."""
import os
import shutil

import numpy as np
import pytest

import actuator_cases as ac
import contact_envelope_cases as cc
import dynamics_envelope_cases as dc
import joints_cases as jc
import observation_cases as oc
import payload_cases as plc
import wrench_cases as wc
from conftest import load_package
from test_gpu_plant import U_TOL
from test_gpu_wrench import _rel, _same, _snapshot, _step_handle

pytestmark = pytest.mark.gpu

pkg = load_package()
sc = pkg.scenario
NX, NU, NQ = 51, 19, 26
B, N, DT, SUBSTEPS, INTERVALS = 5, 6, 0.02, 3, 4
HANDLE_MU = 0.3
INF = float("inf")
SEED = 0x7E44A1
MARGIN = 5e-3
#            plant mode, limits, states
CASES = {"mode2": (2, False, "mid"), "mode4_limits": (4, True, "limits")}
FLAT3 = np.array([0.0, 0.0, -INF])


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _solver(mode=2, limits=False, fb=0, ring=0, source="geometry"):
    """the solving handle: one iteration per solve, friction HANDLE_MU, stiffness 0, softness 1e-5; the plant finds its own contacts"""
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=dc.GRAVITY)
    A = sv.BatchedILQR(B, N=N, dt=DT)
    A.set_contact_mode(mode); A.set_friction(HANDLE_MU); A.set_joint_limits(limits); A.set_max_iterations(1)
    A.plant_configure(SUBSTEPS, fb, source)
    A.plant_set_history(ring)
    A.set_problem(prob)
    return A


def _states(group):
    x16, u16 = dc.mid() if group == "mid" else cc.limit_states()
    idx = (np.arange(B) + 2) % dc.NS
    return np.ascontiguousarray(x16[idx]), np.ascontiguousarray(np.repeat(u16[idx][:, None, :], N, axis=1))


def _ready(mode, limits, group, fb, ring=0):
    A = _solver(mode, limits, fb=fb, ring=ring)
    x0, ui = _states(group)
    A.initialize(x0, ui); A.solve(x0)
    assert np.all(np.isfinite(A.ubar())) and np.all(np.isfinite(A.gains_K()))
    return A, x0


def _feet(x):
    """(clearance [n, 2], ankle x [n, 2]) of the states x, from the two host functions the rule is defined on"""
    sv = _sv()
    return np.array([sv.foot_clearance(xi[:NQ]) for xi in x]), np.array([sv.reference_kinematics(xi)[1][:, 0] for xi in x])


def _records(x0):
    """one record per rollout, placed by the feet of the state the run starts from so that it FLIPS what the flat floor says of a foot there
    (a foot in the air gets a floor above it, a foot in the ground one below it): flat; the left foot by 2 cm from interval 1; the right
    foot by 2 cm, in front of an edge 5 cm behind its ankle, from the start -- the first substep already differs from the flat floor's --;
    both feet by 5 cm behind an edge no foot reaches; both feet by 15 mm in intervals 1 and 2 only"""
    clr, ax = _feet(x0)
    flip = lambda c, d: c + d if c >= 0 else c - d
    return sc.stack_plant_terrain([dict(),
                                   dict(z_left=flip(clr[1, 0], 0.02), first=1),
                                   dict(z_right=flip(clr[2, 1], 0.02), edge_x=ax[2, 1] - 0.05),
                                   dict(z_left=flip(clr[3, 0], 0.05), z_right=flip(clr[3, 1], 0.05), edge_x=ax[3].max() + 0.5),
                                   dict(z_left=flip(clr[4, 0], 0.015), z_right=flip(clr[4, 1], 0.015), first=1, end=3)], B)


def _floor3(T, j):
    """[B, 3]: what step_terrain takes for the records T in plant interval j -- the record's floor while its window is open, else the flat one"""
    is_open = (T[:, 3] <= j) & (j < T[:, 4])
    return np.ascontiguousarray(np.where(is_open[:, None], T[:, :3], FLAT3[None]))


def _host_flags(x, T, j, track):
    """[n, 2] flags of the host rule for states x under records T in interval j; track: [min |clearance - floor|, min |ankle x - edge|]"""
    sv = _sv()
    out = np.zeros((len(x), 2), dtype=np.int32)
    for b, xb in enumerate(x):
        st, fl = sv.terrain_stance(xb[:NQ], T[b], j)
        out[b] = st
        clr = sv.foot_clearance(xb[:NQ])
        track[0] = min(track[0], float(np.abs(clr - fl).min()))
        if np.isfinite(T[b, 2]) and T[b, 3] <= j < T[b, 4]:
            track[1] = min(track[1], float(np.abs(sv.reference_kinematics(xb)[1][:, 0] - T[b, 2]).min()))
    return out


def _state_err(got, want):
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True))).max())


# ---- 1: the step kernel: flags against the host rule, x_next against the library's step under those flags
@pytest.mark.parametrize("case", sorted(CASES))
def test_step_terrain_decides_as_the_host_rule_and_steps_as_step_stance(case):
    mode, limits, group = CASES[case]
    sv = _sv()
    x16, u16 = dc.mid() if group == "mid" else cc.limit_states()
    clr, ax = _feet(x16)
    xs, us, ts, of = [], [], [], []
    for i in range(dc.NS):
        # each foot put down or lifted by its floor, 5 mm from it; the edge everywhere, 5 mm behind the rear ankle, 5 mm in front of the
        # front one, and between the two where they are 2 cm apart
        sl, sr = (+1, -1)[i & 1], (+1, -1)[(i >> 1) & 1]
        edges = [-INF, ax[i].min() - MARGIN, ax[i].max() + MARGIN] + ([ax[i].min() + MARGIN] if abs(ax[i, 0] - ax[i, 1]) > 4 * MARGIN else [])
        for e in edges:
            xs.append(x16[i]); us.append(u16[i]); ts.append([clr[i, 0] + sl * MARGIN, clr[i, 1] + sr * MARGIN, e]); of.append(i)
    xs.append(x16[0]); us.append(u16[0]); ts.append(list(FLAT3)); of.append(0)      # the flat floor
    assert len(xs) % 32 != 0 and len(xs) > 32                           # a full workgroup and a partial one: padding items
    x, u, t = np.ascontiguousarray(xs), np.ascontiguousarray(us), np.ascontiguousarray(ts)
    P = _step_handle(len(x), DT / SUBSTEPS, dc.GRAVITY, mode, limits, HANDLE_MU)
    got, flags = P.step_terrain(x, u, t)
    want_flags = np.array([sv.terrain_stance(x[k, :NQ], np.r_[t[k], 0.0, INF], 0)[0] for k in range(len(x))])
    assert np.array_equal(flags, want_flags), np.flatnonzero((flags != want_flags).any(axis=1))
    assert {tuple(f) for f in flags} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    flat_flags = (clr < 0).astype(np.int32)[of]                       # what z = 0 says of each item
    assert np.array_equal(flags[-1], flat_flags[-1])
    flipped = flags != flat_flags
    assert flipped[:, 0].any() and flipped[:, 1].any()                 # the floors flip feet of both sides against the flat ground
    worst = 0.0
    for l, r in ((0, 0), (0, 1), (1, 0), (1, 1)):
        idx = np.flatnonzero((flags[:, 0] == l) & (flags[:, 1] == r))
        want = P.step_stance(x[idx], u[idx], l, r)
        err = _rel(got[idx], want)
        print("%s flags %d%d: %2d items, step_terrain against step_stance %.3e (bound %.0e)" % (case, l, r, len(idx), err, cc.STEP_TOL))
        assert np.all(np.isfinite(got[idx])) and err < cc.STEP_TOL, (l, r, err)
        worst = max(worst, err)
    # the flags matter: the same items under the other feet go elsewhere
    other = P.step_stance(x, u, 1, 1)
    moved = np.abs(other - got).max(axis=1) > 1e-9
    assert moved[(flags != 1).any(axis=1)].any()
    print("%s: %d items, worst %.3e" % (case, len(x), worst))
    P.close()


def test_step_terrain_refuses_modes_without_unilateral_rows():
    sv = _sv()
    x16, u16 = dc.mid()
    for mode in (0, 1):
        P = _step_handle(2, DT, dc.GRAVITY, mode, False, HANDLE_MU)
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
            P.step_terrain(x16[:2], u16[:2], np.tile(FLAT3, (2, 1)))
        P.close()


# ---- 2: the plant against the teacher-forced composition
def _held_to_the_composition(A, x0, fb, tag, step, law):
    """follow(0, INTERVALS) in one launch; every interval against the host composition from the ring row it started from.
    step(j, x, t) -> (x_next, flags); law(j, x) -> the substep's (command, torque)"""
    A.plant_reset(x0)
    A.plant_follow(0, INTERVALS)
    hx, hu = A.plant_history()
    assert hx.shape == (INTERVALS, B, NX) and np.array_equal(hx[0], x0) and np.all(A.plant_alive() == 1) and A.plant_intervals() == INTERVALS
    ends = [hx[j + 1] for j in range(INTERVALS - 1)] + [A.plant_state()]
    worst, flags = 0.0, None
    for j in range(INTERVALS):
        xc, u, t = hx[j].copy(), None, None
        for k in range(SUBSTEPS):
            if k == 0 or fb:
                u = law(j, xc)
            xc, flags = step(j, xc, u, k)
        want_u = ac.guard(u)
        ex, eu = _state_err(ends[j], xc), float(np.abs(hu[j] - want_u).max())
        print("%s interval %d: state error %.3e (bound %.1e)  |du| %.3e" % (tag, j, ex, cc.STEP_TOL * SUBSTEPS, eu))
        assert np.all(np.isfinite(xc)), (tag, j)
        assert np.allclose(hu[j], want_u, **U_TOL), (tag, j, eu)
        assert ex < cc.STEP_TOL * SUBSTEPS, (tag, j, ex)
        worst = max(worst, ex)
    assert np.array_equal(A.plant_control(), hu[-1])
    assert np.array_equal(A.plant_stance(), flags)            # the plant reports the flags of its last substep
    return worst


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plant_under_a_terrain_table_matches_the_host_composition(case, fb):
    mode, limits, group = CASES[case]
    A, x0 = _ready(mode, limits, group, fb, ring=INTERVALS)
    P = _step_handle(B, DT / SUBSTEPS, dc.GRAVITY, mode, limits, HANDLE_MU, 1e-5, 0.0)
    T = _records(x0)
    assert np.array_equal(A.plant_get_terrain(), np.tile([0.0, 0.0, -INF, 0.0, 0.0], (B, 1))) and A.plant_num_terrain_sets() == 0
    A.plant_set_terrain(T)
    assert np.array_equal(A.plant_get_terrain(), T) and A.plant_num_terrain_sets() == B
    track, seen, on_flat = [INF, INF], [], []
    flat_T = sc.stack_plant_terrain({}, B)

    def step(j, xc, u, k):
        xn, fl = P.step_terrain(xc, ac.guard(u), _floor3(T, j))
        assert np.array_equal(fl, _host_flags(xc, T, j, track)), (j, k)      # the device's decision is the host rule's
        seen.append(fl); on_flat.append(_host_flags(xc, flat_T, j, [INF, INF]))
        return xn, fl

    tag = "%s fb%d" % (case, fb)
    worst = _held_to_the_composition(A, x0, fb, tag, step, lambda j, xc: A.compute_control(xc, knot=j))
    seen, on_flat = np.array(seen), np.array(on_flat)                          # [INTERVALS * SUBSTEPS, B, 2]
    acted = (seen != on_flat).any(axis=(0, 2))
    print("%s: worst state error under the terrain table %.3e; smallest |clearance - floor| %.3e m, |ankle x - edge| %.3e m; rollouts whose flags differ from the flat floor's on the same states: %s"
          % (tag, worst, track[0], track[1], np.flatnonzero(acted).tolist()))
    assert track[0] > 1e-6 and track[1] > 1e-6
    assert acted[2] and not acted[[0, 3]].any()                                # the records act; a flat record and an edge nobody reaches do not
    A.close(); P.close()


@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_plant_under_all_seven_tables_matches_the_host_composition(case, fb):
    """parameter (the handle's values and a torque gain per rollout), wrench (window from interval 1), payload, observation, actuator, joints,
    terrain: the flags of the host rule, the step of ilqr_hip_step_joints under them"""
    mode, limits, group = CASES[case]
    A, x0 = _ready(mode, limits, group, fb, ring=INTERVALS)
    P = _step_handle(B, DT / SUBSTEPS, dc.GRAVITY, mode, limits, HANDLE_MU, 1e-5, 0.0)
    T = _records(x0)
    J = jc.random_records(B, 4)
    gain = np.linspace(0.8, 1.0, B)
    params = np.tile([dc.GRAVITY[0], dc.GRAVITY[1], dc.GRAVITY[2], HANDLE_MU, 1e-5, 0.0, 1.0], (B, 1)); params[:, 6] = gain
    wrench = np.hstack([wc.random_wrenches(B, 3), np.ones((B, 1)), np.full((B, 1), np.inf)])
    payload = plc.random_payloads(B, 5)
    rec = ac.golden_records(B)
    A.plant_set_params(params); A.plant_set_wrench(wrench); A.plant_set_payload(payload)
    A.plant_set_observation(oc.plant_records(B), seed=SEED + 1)
    A.plant_set_actuator(rec, seed=SEED)
    A.plant_set_joints(J)
    A.plant_set_terrain(T)
    A.plant_reset(x0)
    delta, z, beta = A.plant_observation_errors(0, INTERVALS), A.plant_actuator_draws(0, INTERVALS), A.plant_actuator_blend()
    chain = ac.Chain(rec, beta)
    track = [INF, INF]

    def step(j, xc, u, k):
        t = chain.substep(u, z[j])
        fl = _host_flags(xc, T, j, track)
        w9 = wrench[:, :9] if j >= 1 else np.zeros((B, 9))
        xn = np.empty_like(xc)
        for l, r in {(int(a), int(c)) for a, c in fl}:
            idx = np.flatnonzero((fl[:, 0] == l) & (fl[:, 1] == r))
            xn[idx] = P.step_joints(xc[idx], (gain[:, None] * t)[idx], l, r, J[idx], w9[idx], payload[idx])
        return xn, fl

    tag = "%s fb%d all seven tables" % (case, fb)
    worst = _held_to_the_composition(A, x0, fb, tag, step, lambda j, xc: A.compute_control(oc.boxplus(xc, delta[j]), knot=j))
    print("%s: worst state error %.3e; smallest |clearance - floor| %.3e m, |ankle x - edge| %.3e m" % (tag, worst, track[0], track[1]))
    assert track[0] > 1e-6 and track[1] > 1e-6
    A.close(); P.close()


# ---- 3: bit for bit within the family
def _run(A, x0, calls):
    A.plant_reset(x0)
    for c in calls:
        A.plant_advance() if c is None else A.plant_follow(*c)
    return _snapshot(A)


@pytest.mark.parametrize("fb", [0, 1])
def test_one_record_for_all_is_b_identical_records(fb):
    A, x0 = _ready(4, True, "limits", fb, ring=3)
    rec = _records(x0)[4:5]
    A.plant_set_terrain(rec)
    assert np.array_equal(A.plant_get_terrain(), np.repeat(rec, B, axis=0)) and A.plant_num_terrain_sets() == 1
    one = _run(A, x0, [(0, 3)])
    A.plant_set_terrain(np.repeat(rec, B, axis=0))
    assert _same(one, _run(A, x0, [(0, 3)])) and np.all(one[3] == 1)
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_a_group_of_three_is_the_same_in_one_launch_and_in_three(fb):
    """the windows of rollouts 1 and 4 open inside the group, rollout 4's shuts at its end"""
    A, x0 = _ready(4, True, "limits", fb, ring=3)
    A.plant_set_terrain(_records(x0))
    fused = _run(A, x0, [(0, 3)])
    assert _same(fused, _run(A, x0, [(0, 1), (1, 1), (2, 1)])) and np.all(fused[3] == 1) and A.plant_intervals() == 3
    assert _same(_run(A, x0, [None, None, None]), _run(A, x0, [(0, 1), (0, 1), (0, 1)]))      # an advance is the kernel over one interval
    A.close()


@pytest.mark.parametrize("fb", [0, 1])
def test_a_shut_window_is_a_flat_record_and_clearing_is_a_fresh_handle(fb):
    A, x0 = _ready(2, False, "mid", fb, ring=3)
    calls = [None, (1, 2)]
    fresh = _run(A, x0, calls)                                                                 # no table yet: k_plant_advance, k_plant_follow
    T = _records(x0)
    A.plant_set_terrain(T)
    table = _run(A, x0, calls)
    assert not _same(fresh, table)
    shut = T.copy(); shut[:, 3] = 2.0; shut[:, 4] = 2.0                                        # first == end: the heights stay in the records
    A.plant_set_terrain(shut)
    closed = _run(A, x0, calls)
    A.plant_set_terrain(sc.stack_plant_terrain({}, B))
    flat = _run(A, x0, calls)
    assert _same(closed, flat)
    A.plant_set_terrain(sc.stack_plant_terrain({}, 1))                                         # ... one flat record for all as well
    assert _same(flat, _run(A, x0, calls))
    A.plant_clear_terrain()
    assert A.plant_num_terrain_sets() == 0
    assert _same(fresh, _run(A, x0, calls))
    A.plant_set_terrain(None); A.plant_clear_terrain()                                          # (None clears; clearing twice is fine)
    A.close()
    F, _ = _ready(2, False, "mid", fb, ring=3)                                                  # a handle that never had a table
    assert _same(fresh, _run(F, x0, calls))
    F.close()
    err = _state_err(flat[0], fresh[0])
    print("fb%d: the terrain family under a flat record against the plant without a table: state %.3e, control %.3e" % (fb, err, float(np.abs(flat[1] - fresh[1]).max())))
    assert np.array_equal(flat[2], fresh[2]) and err < cc.STEP_TOL * SUBSTEPS


# ---- 4: the window on a standing robot
@pytest.mark.parametrize("fb", [0, 1])
def test_the_right_floor_gives_way_under_a_standing_robot_from_interval_2(fb):
    sv = _sv()
    A = _solver(2, False, fb=fb, ring=3)
    x0 = np.tile(sc.standing_state(), (B, 1))
    ug = sv.gravity_compensation(sc.standing_state(), dc.GRAVITY)
    A.initialize(x0, np.tile(ug, (B, N, 1))); A.solve(x0)
    assert np.all(sv.foot_clearance(x0[0, :NQ]) < -5e-4)                                       # the soles are 1 mm inside z = 0: both feet stand
    low = 1                                                                                    # the rollout whose floor gives way
    T = sc.stack_plant_terrain([dict(z_right=-0.03, first=2) if b == low else dict() for b in range(B)], B)
    A.plant_set_terrain(sc.stack_plant_terrain({}, B))
    A.plant_reset(x0)
    for _ in range(3):
        A.plant_advance()
    flat = _snapshot(A)
    A.plant_set_terrain(T)
    A.plant_reset(x0)
    right, left = [], []
    for j in range(3):
        A.plant_advance()
        st = A.plant_stance()
        right.append(int(st[low, 1])); left.append(int(st[low, 0]))
        keep = np.arange(B) != low
        assert np.all(st[keep] == 1)
    got = _snapshot(A)
    hx = got[4]
    rule = [int(sv.terrain_stance(hx[j, low, :NQ], T[low], j)[0][1]) for j in range(3)]      # the host rule on the ring's rows
    print("fb%d: right flag of rollout %d after intervals 0, 1, 2: %s; the host rule on the ring rows: %s" % (fb, low, right, rule))
    assert right == [1, 1, 0] and rule == [1, 1, 0] and left == [1, 1, 1]
    keep = np.arange(B) != low
    for g, f in zip(got, flat):                                                                # the rollouts beside it: bit for bit
        g, f = np.asarray(g), np.asarray(f)
        sel = (slice(None), keep) if g.ndim == 3 else (keep,)
        assert np.array_equal(g[sel], f[sel])
    assert np.array_equal(got[4][:, low], flat[4][:, low])                                     # ... and its own first two intervals: the ring rows 0, 1, 2
    assert np.abs(got[0][low] - flat[0][low]).max() > 1e-6                                     # the robot has begun to fall
    A.close()


# ---- 5: a state that overflows freezes its rollout alone
@pytest.mark.parametrize("fb", [0, 1])
def test_an_overflowing_state_freezes_its_rollout_alone(fb):
    bad = 4                                                                                    # in the second workgroup at feedback mode 1
    out = {}
    for poisoned in (False, True):
        A, x0 = _ready(2, False, "mid", fb, ring=2)
        T = _records(x0)
        x = x0.copy()
        if poisoned:
            x[bad, NQ + 6 + 3] = 1e308                                                         # a hinge rate: finite now, not after a step
        A.plant_set_terrain(T)
        A.plant_reset(x)
        A.plant_advance()
        out[poisoned] = A.plant_state(), A.plant_control(), A.plant_stance(), A.plant_alive(), x
        A.close()
    x, u, st, alive, xin = out[True]
    keep = np.arange(B) != bad
    assert alive[bad] == 0 and np.all(u[bad] == 0.0) and np.array_equal(x[bad], xin[bad])         # frozen in the state before the advance
    assert np.all(alive[keep] == 1) and np.all(out[False][3] == 1)
    assert np.array_equal(x[keep], out[False][0][keep]) and np.array_equal(u[keep], out[False][1][keep]) and np.array_equal(st[keep], out[False][2][keep])


# ---- 6: the runner
def test_runner_with_plant_terrain_is_the_call_sequence_made_by_hand():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    from mpc_ilqr_mujoco_amd import references as rf
    sv = _sv()
    Bn, Nn, steps = 4, 25, 3
    base = sc.make_problem(sv.reference_kinematics, N=Nn, gravity=dc.GRAVITY)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.tile(sc.standing_state(), (60, 1))); rd.contact = np.ones((60, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(Bn, Nn, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    T = sc.stack_plant_terrain([dict(), dict(z_right=-0.03, first=1), dict(z_left=-0.02, z_right=-0.02), dict(z_left=0.03, edge_x=2.0)], Bn)
    s = sv.BatchedILQR(Bn, N=Nn, dt=DT); s.set_contact_mode(2); s.set_max_iterations(2)
    xs, us = ml.MPCRunner(s, rd, base, resident=True, substeps=2, plant_contacts="geometry", plant_terrain=T).run(x0, steps, u_init=ui)
    assert np.array_equal(s.plant_get_terrain(), T) and s.plant_intervals() == steps
    s.close()
    h = sv.BatchedILQR(Bn, N=Nn, dt=DT); h.set_contact_mode(2); h.set_max_iterations(2)
    run = ml.MPCRunner(h, rd, base, resident=True, substeps=2, plant_contacts="geometry")
    h.plant_set_terrain(T)                                                                     # (survives the runner's configure and reset)
    xh, uh = run.run(x0, steps, u_init=ui)
    assert np.array_equal(h.plant_get_terrain(), T)
    h.close()
    assert np.array_equal(xs, xh) and np.array_equal(us, uh)
    p = sv.BatchedILQR(Bn, N=Nn, dt=DT); p.set_contact_mode(2); p.set_max_iterations(2)
    xp, _ = ml.MPCRunner(p, rd, base, resident=True, substeps=2, plant_contacts="geometry").run(x0, steps, u_init=ui)
    p.close()
    d = np.abs(np.asarray(xs)[-1] - np.asarray(xp)[-1]).max(axis=1)
    print("last state against the run without a table, per rollout: %s" % d)
    assert d[1] > 1e-6 and d[2] > 1e-6                                                        # a floor that gives way under one foot / under both


# ---- 7: refusals
def test_refusals_on_a_live_handle(tmp_path):
    sv = _sv()
    A, x0 = _ready(2, False, "mid", 0, ring=2)
    for bad in (np.ones((2, 5)), np.ones((B, 4))):
        with pytest.raises(ValueError):
            A.plant_set_terrain(bad)
    T = _records(x0)
    for col, v in ((0, np.nan), (1, np.inf), (2, np.inf), (2, np.nan), (3, -1.0), (3, 0.5), (4, 1.5), (4, -np.inf)):
        q = T.copy(); q[B - 1, col] = v
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
            A.plant_set_terrain(q)
    q = T.copy(); q[0, 3], q[0, 4] = 3.0, 2.0
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_ARG"):
        A.plant_set_terrain(q)
    assert A.plant_num_terrain_sets() == 0
    two = np.ascontiguousarray(T[:2])
    assert A.L.ilqr_hip_plant_set_terrain(A.h, two.ctypes.data_as(sv._dp), 2) == 1              # n neither 1 nor B, past the wrapper
    # a floor nobody consults is refused, before anything is launched
    A.plant_set_terrain(T)
    A.plant_reset(x0)
    A.plant_configure(SUBSTEPS, 0, "schedule")
    assert np.array_equal(A.plant_get_terrain(), T)                                            # survives configure and reset
    for call in (A.plant_advance, lambda: A.plant_follow(0, 2)):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED") as e:
            call()
        assert "SCHEDULE" in str(e.value)
    A.plant_configure(SUBSTEPS, 0, "geometry")
    A.plant_set_model(0, None)                                                                 # the plant's own contact mode: none
    for call in (A.plant_advance, lambda: A.plant_follow(0, 2)):
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED") as e:
            call()
        assert "contact mode" in str(e.value)
    assert A.plant_intervals() == 0 and np.array_equal(A.plant_state(), x0) and len(A.plant_history()[0]) == 0      # nothing ran
    A.plant_set_model(None, None)
    A.plant_advance()                                                                          # mode 2 from the feet: served
    assert A.plant_intervals() == 1 and np.all(A.plant_alive() == 1)
    A.plant_clear_terrain()
    A.plant_configure(SUBSTEPS, 0, "schedule"); A.plant_advance()                              # without a table the schedule is a source again
    A.close()
    # a solver in mode 0 whose plant has no mode of its own: the effective mode is the solver's
    Z = _solver(0, False, source="schedule")
    xz, uz = _states("mid")
    Z.initialize(xz, uz); Z.solve(xz); Z.plant_reset(xz)
    Z.plant_set_terrain(T[:1]); Z.plant_configure(SUBSTEPS, 0, "geometry")
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED"):
        Z.plant_advance()
    Z.plant_set_model(3, None); Z.plant_advance()                                              # ... and the plant's own mode overrides it
    assert Z.plant_intervals() == 1
    Z.close()
    # a library whose directory holds no terrain module: an error that names the path it looked for, never a fall-back
    lonely = tmp_path / "libilqr_hip.so"
    shutil.copyfile(sv.LIB_PATH, lonely)
    P = sv.BatchedILQR(B, N=N, dt=DT, lib_path=str(lonely))
    P.set_contact_mode(2)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED") as e:
        P.plant_set_terrain(T)
    assert os.path.join(str(tmp_path), "libilqr_hip_terrain.so") in str(e.value)
    with pytest.raises(sv.ILQRError, match="ILQR_ERR_UNSUPPORTED") as e:
        P.step_terrain(np.zeros((1, NX)), np.zeros((1, NU)), FLAT3[None])
    assert os.path.join(str(tmp_path), "libilqr_hip_terrain.so") in str(e.value)
    assert P.plant_num_terrain_sets() == 0
    P.close()
