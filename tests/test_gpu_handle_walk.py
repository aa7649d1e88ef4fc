"""A long-lived solver handle that is reconfigured between solves, against fresh handles (builders: handle_walk_cases.py).

The yardstick is a FRESH handle brought straight to the configuration by the shortest setter sequence (hw.recipe), given the same start
and solved.  The WALKED handle arrives at the configuration through other configurations, solves, reads and side work.  Every observable
of the observation must then be equal bit for bit (np.array_equal; NaN equal to NaN in the traces): cost (returned and read), the three
traces, iterations, lambda, xbar, ubar, K, kff, adopt_mismatches() == 0, and with an augmented Lagrangian installed its traces, multipliers
and penalties.  This is the project's own standard (two fresh handles agree bit for bit; every solve order is bit-identical in its
observables), so no tolerance is introduced; the fresh-handle path is what the rest of the suite holds to the oracle, and test 5 anchors
the end of two walks to the oracle with the comparison of test_gpu_parity.py.  Counts that depend on host timing (iterations_enqueued
under the early-exit gate) are not compared; with fixed iterations the order of every iteration and its work lists are.  One yardstick is
stated more narrowly than "initialize + solve(x0) on the fresh handle": where a change between initialize and solve() moves the rollout
itself, the walked handle's first cost entry is, as in the reference, the cost of the trajectory it held before the rollout -- see
cold_start_under_other_dynamics.  lambda survives a solve by design: set_regularization before every observation on both
handles; the multipliers and penalties of an installed augmented Lagrangian likewise (a warm start shifts them), set after the initialiser.

B = 40, N = 6, at most 8 iterations (hw: three k_control workgroups of 16 / 16 / 8, the whole-batch side-by-side order, lists with more
than one workgroup), off-pose states, schedules with swing phases; one case at B = 5, below one control group.  Product library only, no
kernel-family environment switches."""
import numpy as np
import pytest

import handle_walk_cases as hw

pytestmark = pytest.mark.gpu
NX, NU, N = hw.NX, hw.NU, hw.N
NAN_OK = ("trace_cost", "trace_alpha", "trace_lambda", "al_trace", "al_state_trace", "al_task_trace")


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


_data = {}


def data(nb):
    """hw.inputs(nb) with the start on the device (torch buffers, as the gather test hands them over) and the buffers of pack_first_knot_device"""
    if nb not in _data:
        import torch
        D = dict(hw.inputs(nb))
        t = dict(x0=torch.tensor(D["x0"], dtype=torch.float64, device="cuda:0"), ui=torch.tensor(D["ui"], dtype=torch.float64, device="cuda:0"),
                 u0=torch.zeros(nb, NU, dtype=torch.float64, device="cuda:0"), K0=torch.zeros(nb, NU, NX, dtype=torch.float64, device="cuda:0"),
                 cost=torch.zeros(nb, dtype=torch.float64, device="cuda:0"))
        torch.cuda.synchronize()
        D["torch"] = t
        D["pack"] = (t["u0"].data_ptr(), t["K0"].data_ptr(), t["cost"].data_ptr())
        _data[nb] = D
    return _data[nb]


def fresh(cfg, nb):
    s = _sv().BatchedILQR(nb, N=N, dt=hw.dc.H)
    hw.recipe(s, cfg, nb)
    return s


def set_multipliers(s, cfg, nb):
    """the state of an installed augmented Lagrangian that survives a solve by design, set explicitly: zero multipliers, the initial penalties"""
    al = cfg["al"]
    if al is None:
        return
    a = hw.al_install_args(cfg, nb)
    s.set_al_multipliers(np.zeros((nb, N + 1, NU, 2)), np.zeros((nb, N, NU, 2)), np.tile([a["rho_joint0"], a["rho_ctrl0"]], (nb, 1)))
    if al["st"] is not None:
        s.set_al_state_multipliers(np.zeros((nb, N + 1, 28, 2)), np.full(nb, hw.AL_STATE[0]))
    if al["tk"]:
        s.set_al_task_multipliers(np.zeros((nb, N + 1, 9, 2)), np.full(nb, hw.AL_TASK[0]))


def solved(s, cost, cfg):
    """the observables of a solve, in the order they are compared"""
    tc, ta, tl = s.trace()
    out = dict(cost=cost, cost_read=s.cost(), trace_cost=tc, trace_alpha=ta, trace_lambda=tl, iterations=s.iterations(), lambdas=s.lambdas(),
               xbar=s.xbar(), ubar=s.ubar(), K=s.gains_K(), kff=s.gains_kff(), adopt_mismatches=np.array(s.adopt_mismatches()))
    if not cfg["early_exit"]:
        # fixed iterations: the order every iteration was enqueued in and the lists it ran from hang on no host timing
        out["orders"] = np.array(s.iteration_orders())
        for it in range(cfg["max_iter"]):
            try:
                out["changed_%d" % it], out["retried_%d" % it] = s.iteration_lists(it)
            except _sv().ILQRError as e:                                 # (the solve kept no lists: the documented refusal, on both handles)
                assert "ILQR_ERR_STATE" in str(e)
                out["changed_%d" % it] = out["retried_%d" % it] = np.array([-1])
    al = cfg["al"]
    if al is not None:
        mj, mc = s.al_multipliers()
        out.update(al_trace=s.al_trace(), al_mu_joint=mj, al_mu_ctrl=mc, al_rho=s.al_penalties())
        if al["st"] is not None:
            out.update(al_state_trace=s.al_state_trace(), al_state_mu=s.al_state_multipliers(), al_state_rho=s.al_state_penalties())
        if al["tk"]:
            out.update(al_task_trace=s.al_task_trace(), al_task_mu=s.al_task_multipliers(), al_task_rho=s.al_task_penalties())
    return out


def staged(s, cfg, D):
    """observation kind (e): the stage API on the cold start, with its getters"""
    s.initialize(D["x0"], D["ui"])
    set_multipliers(s, cfg, D["B"])
    s.stage_linearize(); s.stage_cost_quadratics(); s.stage_backward_pass()
    out = dict(K=s.gains_K(), kff=s.gains_kff())
    out["Vx"], out["Vxx"] = s.value_function()
    out["A"], out["Bm"] = s.linearization()
    out["lx"], out["lu"], out["lxx"], out["luu"] = s.quadratics()
    s.stage_backward_pass()                                              # (again, behind the getters' conversions)
    out["K_again"], out["kff_again"] = s.gains_K(), s.gains_kff()
    # the getters' conversions and the pass's own back are exact round trips: the same pass on the same data, on THIS handle
    assert np.array_equal(out["K_again"], out["K"]) and np.array_equal(out["kff_again"], out["kff"]), "the backward pass behind the getters' layout conversions"
    imp, c, a = s.stage_line_search()
    out.update(improved=imp, ls_cost=c, ls_alpha=a, total_cost=s.stage_total_cost(), xbar=s.xbar(), ubar=s.ubar())
    return out


def observe(s, kind, cfg, D, prev=None, walked=True):
    """one observation of kind a / c1 / c2 / cp / d / e on a handle; prev = (X, U): the previous solution a fresh handle is given"""
    nb = D["B"]
    s.set_regularization(hw.LAMBDA0)
    if kind == "e":
        return staged(s, cfg, D)
    if kind == "a":
        s.initialize(D["x0"], D["ui"]); set_multipliers(s, cfg, nb)
        return solved(s, s.solve(D["x0"]), cfg)
    if kind == "d":
        s.initialize_device(D["torch"]["x0"].data_ptr(), D["torch"]["ui"].data_ptr()); set_multipliers(s, cfg, nb)
        s.solve_async(); s.synchronize()
        return solved(s, s.cost(), cfg)
    if not walked:
        s.set_trajectory(*prev)
    if kind == "cp" and walked:
        s.plant_reset(D["x_warm"]); s.initialize_warm_from_plant(1); set_multipliers(s, cfg, nb)
        return solved(s, s.solve(), cfg)
    s.initialize_warm_resident(D["x_warm"], shift=2 if kind == "c2" else 1); set_multipliers(s, cfg, nb)
    return solved(s, s.solve(D["x_warm"]), cfg)


def first_difference(got, want):
    assert list(got) == list(want)
    for k in got:
        if not np.array_equal(got[k], want[k], equal_nan=k in NAN_OK):
            return k
    return None


COST_KEYS = ("cost", "cost_read", "trace_cost")


def cold_start_under_other_dynamics(got, cold, x_cold, cfg, D, where):
    """A (b) block whose change moves the rollout itself (dynamics, schedule).  The walked handle holds a trajectory that was rolled out
    under the configuration BEFORE the change; like the reference (ilqr.cpp:540, then :551 / :563) the solve takes its first cost entry
    from that trajectory and only then rolls out from x0.  So against `cold` -- the fresh handle's initialize + solve(x0) under the new
    configuration -- everything the rolled-out trajectory decides must be equal bit for bit: accepted alphas, the lambda schedule,
    iterations, xbar, ubar, gains, the augmented Lagrangian's records, and the cost entries from a rollout's first accepted step on.  What
    is left, the cost entries that still carry the pre-rollout trajectory, is held bit for bit to a fresh handle that is GIVEN that
    trajectory (set_trajectory: never a re-roll aside) and solves with solve(x0); its observation is returned as the yardstick of the full
    comparison.  (Under the convergence exit with the wide tolerance |J1 - J0| < tol may end a rollout's solve on the first entry: the
    first comparison is then left to the second.)"""
    nb = D["B"]
    if not (cfg["early_exit"] and cfg["tol"] != hw.TOL[0]):
        for k in got:
            if k not in COST_KEYS:
                assert np.array_equal(got[k], cold[k], equal_nan=k in NAN_OK), "%s: %s differs from the fresh handle's initialize + solve(x0)" % (where, k)
        accepted = np.nan_to_num(cold["trace_alpha"]) != 0.0
        since = np.concatenate([np.zeros((nb, 1), dtype=bool), np.cumsum(accepted, axis=1) > 0], axis=1)      # [nb, max_iter + 1]: an accepted step at or before entry i
        assert since[:, 1:].any(), where
        assert np.array_equal(got["trace_cost"][since], cold["trace_cost"][since], equal_nan=True), "%s: trace_cost behind the first accepted step" % where
        assert np.array_equal(got["cost"][since[:, -1]], cold["cost"][since[:, -1]]), "%s: cost of the rollouts that accepted a step" % where
    return given_trajectory(x_cold, D["ui"], cfg, D, with_state=True)


def given_trajectory(X, U, cfg, D, with_state):
    """the observation of a handle of its own, fresh, that is GIVEN a trajectory and solves: set_trajectory, no initialize; with_state:
    solve(x0), else solve() -- the state is knot 0 of the trajectory"""
    nb = D["B"]
    f = fresh(cfg, nb)
    try:
        f.set_regularization(hw.LAMBDA0)
        f.set_trajectory(X, U); set_multipliers(f, cfg, nb)
        return solved(f, f.solve(D["x0"]) if with_state else f.solve(), cfg)
    finally:
        f.close()


def run(seq, nb, tag):
    """Walk one handle through the sequence; at every observation build the fresh handle of the configuration, observe both, compare.
    Returns (the walked handle, its last observation, the last configuration)."""
    D = data(nb)
    w = fresh(hw.START, nb)
    names, last, in_b, b_rollout, b_given = [], None, False, False, False
    try:
        for i, (step, old, new, label) in enumerate(hw.replay(seq)):
            if step[0] == "T":
                t = hw.TRANSITIONS[step[1]]
                t.apply(w, old, new, D)
                names.append(step[1])
                b_rollout = b_rollout or (in_b and t.rollout)
                b_given = b_given or (in_b and t.trajectory)
                continue
            if step[0] == "B0":
                w.set_regularization(hw.LAMBDA0); w.initialize(D["x0"], D["ui"])
                x_cold = w.xbar()                                        # (a read: the cold start under the configuration before the changes)
                names.append("(b: initialize"); in_b, b_rollout, b_given = True, False, False
                continue
            kind = "b" if step[0] == "B1" else step[1]
            names.append("solve())" if kind == "b" else "observe " + kind)
            f = fresh(new, nb)
            try:
                if kind == "b":
                    # the walked handle initialised BEFORE the transitions and solves without a state: the cold start may be re-rolled aside
                    set_multipliers(w, new, nb); got = solved(w, w.solve(), new)
                    in_b = False
                    if b_given:
                        # the block handed the walked handle a trajectory of the caller's: the yardstick never initialises, it is given the
                        # same trajectory and solves -- a trajectory that is no rollout has to be rolled out from x0 before iteration 0
                        want = given_trajectory(D["x_given"], D["u_given"], new, D, with_state=False)
                        assert not np.array_equal(got["xbar"], D["x_given"])
                    else:
                        f.set_regularization(hw.LAMBDA0); f.initialize(D["x0"], D["ui"]); set_multipliers(f, new, nb)
                        want = solved(f, f.solve(D["x0"]) if b_rollout else f.solve(), new)
                        if b_rollout:
                            want = cold_start_under_other_dynamics(got, want, x_cold, new, D, "%s: step %d, after %s" % (tag, i, " > ".join(names)))
                else:
                    prev = (w.xbar(), w.ubar()) if kind in ("c1", "c2", "cp") else None
                    got = observe(w, kind, new, D)
                    want = observe(f, kind, new, D, prev, walked=False)
            finally:
                f.close()
            k = first_difference(got, want)
            assert k is None, "%s: step %d, after %s: %s differs from the fresh handle's (max |diff| %.3e)" % (
                tag, i, " > ".join(names), k, np.nanmax(np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(want[k], dtype=np.float64))))
            assert kind == "e" or got["adopt_mismatches"] == 0
            assert all(np.isfinite(v).all() for kk, v in got.items() if kk not in NAN_OK), (tag, i, names)
            last = got
    except Exception:
        w.close()
        raise
    return w, last, new


# ------------------------------------------------------------------------------------------------------------------------- 1. directed
DIRECTED = hw.directed()


@pytest.mark.parametrize("family, name", [(f, n) for f, n, _ in DIRECTED])
def test_directed_sequence(family, name):
    seq = next(s for f, n, s in DIRECTED if (f, n) == (family, name))
    w, last, cfg = run(seq, hw.B, "%s/%s" % (family, name))
    w.close()


@pytest.mark.parametrize("family, name", [("side_work", "dynamics_walk"), ("installed_removed", "one_set_and_B_sets"), ("layouts", "stage_api_after_a_full_solve")])
def test_directed_sequence_below_one_control_group(family, name):
    seq = next(s for f, n, s in DIRECTED if (f, n) == (family, name))
    w, last, cfg = run(seq, hw.B_SMALL, "B=%d %s/%s" % (hw.B_SMALL, family, name))
    w.close()


# ------------------------------------------------------------------------------------------------------------------------- 2. seeded walks
@pytest.mark.parametrize("seed", hw.WALK_SEEDS)
def test_seeded_random_walk(seed):
    seq = hw.random_walks()[seed]
    w, last, cfg = run(seq, hw.B, "seed %d" % seed)
    w.close()


# --------------------------------------------------------------------------------------------- fresh handles tell the configurations apart
_fresh_obs = {}


def fresh_observation(cfg):
    """observation (a) of a fresh handle, remembered by the configuration's items"""
    key = str(sorted(cfg.items(), key=str))
    if key not in _fresh_obs:
        f = fresh(cfg, hw.B)
        try:
            _fresh_obs[key] = observe(f, "a", cfg, data(hw.B))
        finally:
            f.close()
    return _fresh_obs[key]


@pytest.mark.parametrize("name", sorted(hw.DISCRIMINATING) + sorted(hw.GPU_ONLY_DISCRIMINATING))
def test_fresh_handles_of_differing_configurations_observe_different_things(name):
    """the discrimination check of test_handle_walk_cpu.py with fresh handles only: a walk that compared two unread settings would pass otherwise"""
    before, after = hw.discriminating_pair(name)
    a, b = fresh_observation(before), fresh_observation(after)
    assert not np.array_equal(a["cost"], b["cost"]), name
    n = (np.abs(a["cost"] - b["cost"]) > hw.DISCRIMINATION_MARGIN * np.abs(a["cost"])).sum()
    print(name, "rollouts whose cost differs by more than 1e-6 relative:", int(n))
    assert 2 * n > hw.B                                                  # (most of the batch; a third of it shares one set's references, half starts inside the joint limits)


@pytest.mark.parametrize("field", hw.ORDER_FIELDS)
def test_fresh_handles_under_the_order_switches_observe_the_same(field):
    """every observable of the solve; the order each iteration was enqueued in and the lists it ran from are what these switches move
    (set_relinearize_unchanged keeps no lists at all), so they are compared between a walked and a fresh handle of ONE configuration only"""
    def results(obs):
        return {k: v for k, v in obs.items() if k != "orders" and not k.startswith(("changed_", "retried_"))}
    for base in (hw.START, dict(hw.START, early_exit=False), dict(hw.START, early_exit=False, mode=2)):
        for name in (n for n in hw.TRANSITIONS if n.split(":")[0] == field):
            cfg = hw.TRANSITIONS[name].step(base)
            if cfg is not None:
                got, want = results(fresh_observation(cfg)), results(fresh_observation(base))
                assert len(got) >= 12 and first_difference(got, want) is None, (name, base, first_difference(got, want))


# ------------------------------------------------------------------------------------------------------------------------- 3. refused calls
def _refusals():
    track = hw.sc.stack_al_task_bounds(dict(swing_clearance=0.05), 1, N + 4)[0]
    return [
        ("al_onto_weight_sets", ["wsets:True"], lambda s, nb: s.set_augmented_lagrangian(**hw.al_install_args(hw.START, nb)), "ILQR_ERR_UNSUPPORTED"),
        ("weight_sets_onto_al", ["al:on", "al_jc:table"], lambda s, nb: s.set_weight_sets(*hw.weight_table(hw.START, nb)), "ILQR_ERR_UNSUPPORTED"),
        ("contact_mode_1_under_geometry", ["mode:2", "source:geometry"], lambda s, nb: s.set_contact_mode(1), "ILQR_ERR_UNSUPPORTED"),
        ("geometry_under_contact_mode_1_is_never_reached", ["mode:2"], lambda s, nb: (s.set_stance_source("geometry"), s.set_contact_mode(1)), "ILQR_ERR_UNSUPPORTED"),
        ("task_track_without_a_task_family", ["mode:2", "al:on", "al_st:table"], lambda s, nb: s.set_al_task_bounds_track(track), "ILQR_ERR_STATE"),
        ("window_from_track_past_the_last_row", ["mode:2", "track:on"], lambda s, nb: s.window_from_track(hw.walking_track().x_ref.shape[0], True), "ILQR_ERR_ARG"),
    ]


REFUSALS = ("al_onto_weight_sets", "weight_sets_onto_al", "contact_mode_1_under_geometry", "geometry_under_contact_mode_1_is_never_reached",
            "task_track_without_a_task_family", "window_from_track_past_the_last_row")


@pytest.mark.parametrize("case", REFUSALS)
def test_refused_call_changes_nothing(case):
    sv = _sv()
    assert [r[0] for r in _refusals()] == list(REFUSALS)
    name, before, call, code = next(r for r in _refusals() if r[0] == case)
    nb, D = hw.B, data(hw.B)
    w, last, cfg = run(hw.T(*before) + hw.O("a"), nb, name)
    try:
        with pytest.raises(sv.ILQRError, match=code):
            call(w, nb)
        if name.startswith("geometry_under"):
            w.set_stance_source("schedule")                              # (the accepted half of the pair; the refused half left the mode at 2)
        for kind in ("c1", "a"):
            f = fresh(cfg, nb)
            try:
                prev = (w.xbar(), w.ubar())
                got, want = observe(w, kind, cfg, D), observe(f, kind, cfg, D, prev, walked=False)
            finally:
                f.close()
            assert first_difference(got, want) is None, (name, kind, first_difference(got, want))
    finally:
        w.close()


def test_warm_start_before_any_initialise_is_refused_and_changes_nothing():
    sv = _sv()
    nb, D = hw.B, data(hw.B)
    w = fresh(hw.START, nb)
    try:
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            w.initialize_warm_resident(D["x_warm"])
        with pytest.raises(sv.ILQRError, match="ILQR_ERR_STATE"):
            w.initialize_warm_resident(D["x_warm"], shift=2)
        assert first_difference(observe(w, "a", hw.START, D), fresh_observation(hw.START)) is None
    finally:
        w.close()


# ------------------------------------------------------------------------------------------------------------------------- 4. device pointers
class _DeviceArray:
    """a device pointer of the C ABI as an object torch.as_tensor reads (the CUDA array interface)"""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr="<f8", data=(int(ptr), False), version=2, strides=None)


def through_torch(ptr, shape):
    import torch
    return torch.as_tensor(_DeviceArray(ptr, shape), device="cuda:0")


@pytest.mark.parametrize("gate", [True, False])
@pytest.mark.parametrize("early_exit", [True, False])
def test_device_pointer_path_is_the_host_path(gate, early_exit):
    import torch
    nb, D = hw.B, data(hw.B)
    cfg = dict(hw.START, mode=2, gate=gate, early_exit=early_exit)
    want = fresh_observation(cfg)                                        # initialize + solve(x0)
    s = fresh(cfg, nb)
    try:
        got = observe(s, "d", cfg, D)
        assert first_difference(got, want) is None, first_difference(got, want)
        # the gather payload, into caller-owned buffers and through the handle's own
        t = D["torch"]
        for b in (t["u0"], t["K0"], t["cost"]):
            b.fill_(-1.0)
        torch.cuda.synchronize()
        s.pack_first_knot_device(*D["pack"])
        assert np.array_equal(t["u0"].cpu().numpy(), want["ubar"][:, 0]) and np.array_equal(t["K0"].cpu().numpy(), want["K"][:, 0])
        assert np.array_equal(t["cost"].cpu().numpy(), want["cost"])
        u0, K0, c = s.first_knot_device()
        assert u0 and K0 and c
        assert np.array_equal(through_torch(u0, (nb, NU)).cpu().numpy(), want["ubar"][:, 0])
        assert np.array_equal(through_torch(K0, (nb, NU, NX)).cpu().numpy(), want["K"][:, 0])
        assert np.array_equal(through_torch(c, (nb,)).cpu().numpy(), want["cost"])
        # the plant state on the device
        s.plant_reset(D["x_warm"]); s.plant_advance(); s.synchronize()
        p = s.plant_state_device()
        assert p and np.array_equal(through_torch(p, (nb, NX)).cpu().numpy(), s.plant_state())
        assert not np.array_equal(s.plant_state(), D["x_warm"])
        # a copy enqueued on the handle's stream is ordered behind solve_async: the cost read without a host synchronise of the handle
        assert s.stream
        ext = torch.cuda.ExternalStream(s.stream)
        cost_dev, out = through_torch(c, (nb,)), torch.full((nb,), -1.0, dtype=torch.float64, device="cuda:0")
        # the handle's cost buffer still holds this very cost from the solve above: overwritten first, so that only a copy that ran
        # BEHIND the new solve on the stream the handle names can read it
        cost_dev.fill_(-2.0)
        torch.cuda.synchronize()
        assert np.all(s.cost() == -2.0)
        s.set_regularization(hw.LAMBDA0)
        s.initialize_device(t["x0"].data_ptr(), t["ui"].data_ptr()); s.solve_async()
        with torch.cuda.stream(ext):
            out.copy_(cost_dev, non_blocking=True)
            ev = torch.cuda.Event(); ev.record(ext)
        ev.synchronize()
        assert np.array_equal(out.cpu().numpy(), want["cost"])
        s.synchronize()
    finally:
        s.close()


def test_stage_rollout_is_the_cold_start_and_reset_starts_the_loop_again():
    sv = _sv()
    nb, D = hw.B, data(hw.B)
    cfg = dict(hw.START, mode=2)
    f = fresh(cfg, nb); f.initialize(D["x0"], D["ui"]); want = f.xbar(); f.close()
    s = fresh(cfg, nb)
    try:
        X = np.repeat(D["x0"][:, None, :], N + 1, axis=1)                # (only knot 0 is a state of the rollout)
        s.set_trajectory(X, D["ui"]); s.stage_rollout()
        assert np.array_equal(s.xbar(), want) and np.array_equal(s.ubar(), D["ui"]) and not np.array_equal(want, X)
        # BatchedMPC.reset: the next step is a cold start again
        refs = hw.reference_arrays("a", 1, nb)
        mpc = sv.BatchedMPC(s, lambda t: refs)
        s.set_regularization(hw.LAMBDA0)
        u_first = mpc.step_once(D["x0"]); first = solved(s, mpc.last_solve_cost, cfg)
        mpc.step_once(D["x_warm"])
        assert mpc.t_idx == 2 and mpc.has_prev
        mpc.reset()
        assert mpc.t_idx == 0 and not mpc.has_prev
        s.set_regularization(hw.LAMBDA0)
        u_again = mpc.step_once(D["x0"])
        assert np.array_equal(u_again, u_first) and first_difference(solved(s, mpc.last_solve_cost, cfg), first) is None
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------------- 5. the oracle
def rel(a, b):
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


@pytest.mark.parametrize("name", sorted(hw.ANCHOR_TAILS))
def test_end_of_a_walk_matches_the_oracle(name):
    """the comparison of test_gpu_parity.test_full_solve_parity_trace_and_gains, tolerances included, on the last solve of a walk: the
    walks end in configurations the oracle models, so the fresh-handle yardstick does not compare two wrong answers"""
    nb, D = hw.B, data(hw.B)
    w, got, cfg = run(hw.ANCHOR_TAILS[name], nb, "anchor " + name)
    w.close()
    assert cfg["mode"] == (2 if name == "contact2" else 0)
    tc, ta, tl, it = got["trace_cost"], got["trace_alpha"], got["trace_lambda"], got["iterations"]
    for b in range(nb):
        o = hw.oracle_of(cfg, b)
        o.initialize(D["x0"][b], D["ui"][b])
        ok, c = o.solve(D["x0"][b])
        n, oc, oa, olam = o.trace()
        assert n == it[b], (b, n, it[b])
        assert np.allclose(tc[b, : n + 1], oc[: n + 1], rtol=1e-5, atol=0), (b, tc[b, : n + 1], oc[: n + 1])
        assert np.array_equal(ta[b, :n], oa[:n]) and np.allclose(tl[b, :n], olam[:n], rtol=1e-12), (b, ta[b, :n], oa[:n])
        assert abs(got["cost"][b] - c) <= 1e-5 * abs(c)
        assert rel(got["K"][b], o.get("K")) < 1e-5 and rel(got["kff"][b], o.get("kff")) < 1e-5, (b, rel(got["K"][b], o.get("K")), rel(got["kff"][b], o.get("kff")))
        assert rel(got["xbar"][b], o.get("xbar")) < 1e-5 and rel(got["ubar"][b], o.get("ubar")) < 1e-5
        assert abs(got["lambdas"][b] - o.get_lambda()) < 1e-18
