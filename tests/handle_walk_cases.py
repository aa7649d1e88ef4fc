"""Builders for the walks of a long-lived solver handle (test_handle_walk_cpu.py, test_gpu_handle_walk.py).  NumPy, the CPU oracle and
the host-only entry points of the library; no GPU code: everything here acts on whatever object it is handed -- a BatchedILQR, or the
recording stand-in of test_handle_walk_cpu.py.

A CONFIGURATION is a flat dict (START is what the walks begin with; HANDLE_DEFAULT is what ilqr_hip_create leaves).  A TRANSITION
(TRANSITIONS[name]) either moves one field of it -- name "field:value", visit label "field:old>new" -- or is side work between solves
(names "read:*" / "side:*"): reads, single steps, the plant, the stage setters.  recipe(cfg) is the shortest setter sequence that brings a
FRESH handle to a configuration, the yardstick of every comparison: a walked handle that arrives there through other configurations,
solves and reads must observe what the fresh handle observes, bit for bit.

A SEQUENCE is a list of steps:
    ("T", name)          a transition
    ("O", kind)          an observation: "a" initialize + solve(x0); "c1" / "c2" initialize_warm_resident(shift) + solve(x); "cp" the same
                         start taken from the plant state; "d" initialize_device + solve_async + synchronize; "e" the stage API
    ("B0",) ... ("B1",)  observation kind (b): initialize, then the transitions in between, then solve() -- the first_aside path
directed() lists the directed sequences, one per remembered fact of the handle; random_walk(seed) draws legal transitions only, the
least visited first, with an observation after every second one.

Shape: B = 40 (three k_control workgroups of 16 / 16 / 8, the whole-batch side-by-side order, lists with more than one workgroup), N = 6,
six iterations; one case at B_SMALL = 5.  Start: the sixteen dynamics_envelope_cases.mid() states (velocities scaled by 0.3, as
solve_envelope_cases.tame) repeated over the batch with a seeded offset per rollout, every other rollout with the left knee past its upper
limit and moving out, every fourth with the right elbow past its lower one (work_list_cases.py); schedules with swing phases."""
import ctypes as C
import functools

import numpy as np

import dynamics_envelope_cases as dc
import oracle_lib as ol
from conftest import load_package

pkg = load_package()
sc = pkg.scenario
NX, NU, NQ = 51, 19, 26
B, N, ITERS, B_SMALL = 40, 6, 6, 5
LAMBDA0 = 1e-6
FD_EPS = 1e-2                       # (forward differences at 1e-5 move the final cost by less than 1e-6 of the analytic solve's, at 1e-3 in some rollouts: no discrimination)
SEED = 97
EARTH, LOW = (0.0, 0.0, -9.81), (0.3, 0.0, -6.0)
SOFT = (1e-5, 1e-3)
MU = (1.0, 0.3)
LIM_K = (0.0, 625.0)
TOL = (1e-4, 500.0)                 # (an absolute cost decrease: the off-pose costs are in the thousands)
MAX_ITERS = (6, 3, 8)               # the cycle 6 -> 3 -> 8 -> 6
TRACK = ((0, False), (2, True))     # (step, follow_schedule) of the two track cuts
STAGES = ("iLQR_backwardPass", "iLQR_lineSearch")
SCHEDULES = {"a": np.array([[1, 1], [1, 0], [1, 0], [1, 1], [0, 1], [0, 1], [1, 1]], dtype=np.int32),
             "b": np.array([[0, 1], [0, 1], [1, 1], [1, 1], [1, 0], [1, 1], [1, 1]], dtype=np.int32),
             "c": np.array([[1, 1], [1, 1], [0, 1], [1, 1], [1, 1], [1, 0], [1, 0]], dtype=np.int32)}
AL_ARGS = dict(rounds=2, growth=10.0, rho_max_factor=1e4, margin=0.1, tol_joint=1e-3, tol_ctrl=1e-2)
AL_STATE = (1.0, 1e-3)              # rho_state0, tol_state
AL_TASK = (10.0, 1e-3)              # rho_task0, tol_task
AL_CUT_STEP = 1
KINDS = ("a", "b", "c1", "c2", "cp", "d", "e")

# what ilqr_hip_create leaves behind
HANDLE_DEFAULT = dict(mode=0, soft=SOFT[0], mu=MU[0], limits=False, lim_k=LIM_K[0], source="schedule", gravity="earth",
                      refs_var="a", refs_sets=1, sched_var="a", sched_sets=1, track=None, weights="a", wsets=False,
                      jac=0, early_exit=True, gate=True, max_iter=10, tol=TOL[0], dedup=True, relin=False, repass=False, reroll=False, listed=True,
                      al=None, profiling=False, stages=None)
START = dict(HANDLE_DEFAULT, max_iter=ITERS)
# the fields a solve's observables do not depend on: launch orders, the gate, verification and profiling switches
ORDER_FIELDS = ("gate", "dedup", "relin", "repass", "reroll", "listed", "profiling", "stages")


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs
@functools.lru_cache(maxsize=None)
def inputs(nb=B):
    """dict: x0 [nb,51], ui [nb,N,19], x_warm [nb,51] (the state of the warm starts), xs / us (the items of the single steps);
    read-only.  The first nb rollouts of the B = 40 batch."""
    rng = np.random.default_rng(SEED)
    xm = dc.mid()[0].copy()
    xm[:, NQ:] *= 0.3
    x0 = xm[np.arange(B) % dc.NS].copy()
    x0[:, 7:NQ] += rng.uniform(-0.02, 0.02, (B, NQ - 7))
    x0[:, NQ:] += rng.uniform(-0.05, 0.05, (B, NX - NQ))
    x0[1::2, 7 + 3] = 2.09; x0[1::2, 32 + 3] = 1.5
    x0[3::4, 7 + 18] = -1.29; x0[3::4, 32 + 18] = 0.1
    o = ol.Oracle(N, dc.H); o.set_problem(dc.problem(N, SCHEDULES["a"], EARTH))
    ug = o.grav_comp(sc.standing_state())
    ui = np.clip(ug[None, None, :] + rng.uniform(-1.0, 1.0, (B, N, NU)), -0.8 * sc.CTRLRANGE, 0.8 * sc.CTRLRANGE)
    x_warm = x0.copy()
    x_warm[:, NQ:] += rng.uniform(-0.05, 0.05, (B, NX - NQ))
    # a trajectory that is no rollout of anything: knot 0 is x0, the hinges drift by 0.01 rad a knot, the velocities fade; 0.9 of the controls
    x_given = np.repeat(x0[:, None, :], N + 1, axis=1)
    t = np.arange(N + 1)[None, :, None]
    x_given[:, :, 7:NQ] += 0.01 * t
    x_given[:, :, NQ:] *= 1.0 - 0.05 * t
    out = dict(x0=x0[:nb].copy(), ui=ui[:nb].copy(), x_warm=x_warm[:nb].copy(), xs=x0[:4].copy(), us=ui[:4, 0].copy(),
               x_given=x_given[:nb].copy(), u_given=0.9 * ui[:nb])
    for v in out.values():
        v.setflags(write=False)
    out["B"] = nb
    return out


def _poses():
    """three reference poses: standing; knees bent with the pelvis lowered; arms raised and the pelvis turned"""
    p0 = sc.standing_state()
    p1 = p0.copy(); p1[2] -= 0.03; p1[7 + 3] += 0.25; p1[7 + 8] += 0.25; p1[7 + 2] -= 0.12; p1[7 + 7] -= 0.12
    p2 = p0.copy(); p2[7 + 11] += 0.3; p2[7 + 15] += 0.3; p2[3:7] = sc._axis_angle_quat(np.array([0.0, 0.0, 0.15]))
    return p0, p1, p2


@functools.lru_cache(maxsize=None)
def _reference_sets():
    """per pose: (x_ref [N+1,51], u_ref [N,19], com_ref [N+1,3], ee [2,3])"""
    o = ol.Oracle(N, dc.H); o.set_problem(dc.problem(N, SCHEDULES["a"], EARTH))
    out = []
    for k, p in enumerate(_poses()):
        com, ee = ol.reference_kinematics(p)
        u = np.tile(0.5 * k * o.grav_comp(p), (N, 1))
        out.append((np.tile(p, (N + 1, 1)), u, np.tile(com, (N + 1, 1)), ee))
    return out


def reference_arrays(var, sets, nb):
    """(x_ref, u_ref, com_ref) with a leading axis of `sets` (1 or nb): variant "a" is pose b % 3 per rollout (pose 0 as one set),
    variant "b" pose (b + 1) % 3 (pose 1 as one set)"""
    off = {"a": 0, "b": 1}[var]
    rs = _reference_sets()
    idx = [off] if sets == 1 else [(b + off) % 3 for b in range(nb)]
    return tuple(np.stack([rs[i][k] for i in idx]) for k in range(3))


def schedule_arrays(var, sets, nb):
    """(stance [sets,N+1,2], ee_ref [sets,N+1,2,3], com_vel_ref [sets,N+1,3]): variant "a" is schedule "a" ("a", "b", "c" in turn per
    rollout), variant "b" schedule "b" ("b", "c", "a" in turn); the foot references are the standing pose's with a swing foot 5 cm up"""
    names = ("a", "b", "c")
    off = {"a": 0, "b": 1}[var]
    ee0 = _reference_sets()[0][3]
    idx = [off] if sets == 1 else [(b + off) % 3 for b in range(nb)]
    st = np.stack([SCHEDULES[names[i]] for i in idx])
    ee = np.tile(ee0, (len(idx), N + 1, 1, 1))
    ee[..., 2] += 0.05 * (st == 0)
    cv = np.tile(np.array([0.05, -0.02, 0.01]) * (1 + off), (len(idx), N + 1, 1))
    return st, ee, cv


def weight_scale(nb):
    return np.array([(1.0, 1.5, 0.6)[b % 3] for b in range(nb)])


@functools.lru_cache(maxsize=None)
def walking_track():
    import reference_track_cases as rc
    return rc.track()


def track_starts(nb):
    return np.array([(7 * b) % 150 for b in range(nb)], dtype=np.int32)


def base_problem(cfg, nb):
    """the problem dict set_problem takes for the configuration, the track left aside"""
    prob = sc.make_problem(ol.reference_kinematics, N=N, gravity={"earth": EARTH, "low": LOW}[cfg["gravity"]])
    prob["dt"] = dc.H
    prob["x_ref"], prob["u_ref"], prob["com_ref"] = reference_arrays(cfg["refs_var"], cfg["refs_sets"], nb)
    prob["stance"], prob["ee_ref"], prob["com_vel_ref"] = schedule_arrays(cfg["sched_var"], cfg["sched_sets"], nb)
    if cfg["weights"] == "b":
        prob["Q"], prob["Qf"], prob["R"] = prob["Q"] * 1.3, prob["Qf"] * 0.8, prob["R"] * 2.0
    if cfg["wsets"]:
        prob = sc.stack_weight_sets(prob, [dict(Q=prob["Q"] * w, Qf=prob["Qf"] * w) for w in weight_scale(nb)])
    return prob


def problem(cfg, nb):
    """the problem the configuration solves: base_problem, or under a track the windows of references.problem_at_starts"""
    prob = base_problem(cfg, nb)
    if cfg["track"] is not None:
        step, follow = cfg["track"]
        prob = walking_track().problem_at_starts(track_starts(nb), step, N, prob, follow_schedule=follow)
    return prob


def weight_table(cfg, nb):
    return _sv().weight_sets_of(base_problem(dict(cfg, wsets=True), nb), nb)


# ---- augmented-Lagrangian bounds
def al_install_args(cfg, nb):
    prob = base_problem(dict(cfg, wsets=False), nb)
    return dict(AL_ARGS, rho_joint0=2 * prob["w_joint"], rho_ctrl0=2 * prob["w_ctrl"])


def al_jc_table(nb):
    return sc.stack_al_bounds([dict(torque_scale=0.5 + 0.05 * (b % 5), joint_hi={3: 1.9 - 0.01 * (b % 3)}) for b in range(nb)], nb, margin=AL_ARGS["margin"])


def al_jc_window(nb):
    return sc.stack_al_knot_bounds([dict(torque_scale=[(0, 3, 0.6), (3, N + 1, 0.4 + 0.05 * (b % 4))], joint_lo=(2, 5, {18: -1.0})) for b in range(nb)], nb, N, margin=AL_ARGS["margin"])


def al_jc_track():
    return sc.stack_al_knot_bounds(dict(torque_scale=[(0, 4, 0.7), (4, 9, 0.45), (9, N + 7, 0.55)]), 1, N + 6, margin=AL_ARGS["margin"])[0]


def al_track_starts(nb):
    return np.array([b % 3 for b in range(nb)], dtype=np.int32)


def al_jc_cut(nb):
    """what the cut of al_jc_track() at AL_CUT_STEP writes: rollout b, knot t reads row min(start[b] + step + t, rows - 1)"""
    tr = al_jc_track()
    rows = np.minimum(al_track_starts(nb)[:, None] + AL_CUT_STEP + np.arange(N + 1)[None, :], tr.shape[0] - 1)
    return tr[rows]


def al_state_table(nb):
    return sc.stack_al_state_bounds([dict(joint_speed=1.0 + 0.1 * (b % 4), pelvis_z=(0.95, 1.08)) for b in range(nb)], nb)


def al_state_window(nb):
    return sc.stack_al_state_knot_bounds([dict(joint_speed=[(0, 3, 2.0), (3, N + 1, 0.8 + 0.1 * (b % 3))], pelvis_lin_vel=(1, N + 1, (-0.3, 0.3))) for b in range(nb)], nb, N)


def al_task_window(nb):
    return sc.stack_al_task_bounds([dict(swing_clearance=0.08 + 0.01 * (b % 3), com_xy=((-0.03, -0.03), (0.03, 0.03))) for b in range(nb)], nb, N)


# ---------------------------------------------------------------------------------------------------------------------------------------
# setter calls
def set_schedule(s, cfg, nb):
    """the contact schedule and the foot / CoM-velocity references of the configuration, by the two C entry points set_problem uses"""
    st, ee, cv = schedule_arrays(cfg["sched_var"], cfg["sched_sets"], nb)
    st = np.ascontiguousarray(st, dtype=np.int32); ee = np.ascontiguousarray(ee); cv = np.ascontiguousarray(cv)
    s._chk(s.L.ilqr_hip_set_contact_schedule(s.h, st.ctypes.data_as(C.POINTER(C.c_int)), int(st.shape[0])))
    s._chk(s.L.ilqr_hip_set_ee_references(s.h, ee.ctypes.data_as(C.POINTER(C.c_double)), cv.ctypes.data_as(C.POINTER(C.c_double)), int(ee.shape[0])))


def set_track(s, cfg, nb, upload):
    step, follow = cfg["track"]
    if upload:
        s.set_reference_track(walking_track())
        s.set_track_starts(track_starts(nb))
    s.window_from_track(step, follow)


def set_al_jc(s, kind, nb, was=None):
    if was == "cut" and kind != "cut":
        s.clear_al_bounds_track()
    if kind is None:
        s.clear_al_bounds()
    elif kind == "table":
        s.set_al_bounds(al_jc_table(nb))
    elif kind == "window":
        s.set_al_knot_bounds(al_jc_window(nb))
    else:
        s.set_al_bounds_track(al_jc_track(), None); s.set_al_bounds_track_starts(al_track_starts(nb)); s.al_bounds_window_from_track(AL_CUT_STEP)


def set_al_st(s, kind, nb):
    if kind is None:
        s.clear_al_state_bounds()
    elif kind == "table":
        s.set_al_state_bounds(al_state_table(nb), *AL_STATE)
    else:
        s.set_al_state_knot_bounds(al_state_window(nb), *AL_STATE)


def set_al_tk(s, on, nb):
    if on:
        s.set_al_task_bounds(al_task_window(nb), *AL_TASK)
    else:
        s.clear_al_task_bounds()


AL_EMPTY = dict(jc=None, st=None, tk=False)


def recipe(s, cfg, nb):
    """The shortest setter sequence from a fresh handle (HANDLE_DEFAULT) to `cfg`: one set_problem, then one call per field that differs."""
    d = HANDLE_DEFAULT
    s.set_problem(base_problem(cfg, nb))
    if cfg["track"] is not None:
        set_track(s, cfg, nb, True)
    if (cfg["mode"], cfg["soft"]) != (d["mode"], d["soft"]):
        s.set_contact_mode(cfg["mode"], cfg["soft"])
    if cfg["mu"] != d["mu"]:
        s.set_friction(cfg["mu"])
    if cfg["limits"]:
        s.set_joint_limits(True)
    if cfg["lim_k"] != d["lim_k"]:
        s.set_joint_limit_stiffness(cfg["lim_k"])
    if cfg["source"] != d["source"]:
        s.set_stance_source(cfg["source"])
    if (cfg["jac"], cfg["early_exit"]) != (d["jac"], d["early_exit"]):
        s.set_options(jacobian_mode=cfg["jac"], fd_eps=FD_EPS, early_exit=cfg["early_exit"])
    if cfg["gate"] != d["gate"]:
        s.set_early_exit_gate(cfg["gate"])
    if cfg["max_iter"] != d["max_iter"]:
        s.set_max_iterations(cfg["max_iter"])
    if cfg["tol"] != d["tol"]:
        s.set_tolerance(cfg["tol"])
    for field, setter in (("dedup", "set_dedup_saturated_retry"), ("relin", "set_relinearize_unchanged"), ("repass", "set_repeat_first_pass"),
                          ("reroll", "set_reroll_nominal"), ("listed", "set_listed_spec")):
        if cfg[field] != d[field]:
            getattr(s, setter)(cfg[field])
    if cfg["al"] is not None:
        s.set_augmented_lagrangian(**al_install_args(cfg, nb))
        if cfg["al"]["jc"] is not None:
            set_al_jc(s, cfg["al"]["jc"], nb)
        if cfg["al"]["st"] is not None:
            set_al_st(s, cfg["al"]["st"], nb)
        if cfg["al"]["tk"]:
            set_al_tk(s, True, nb)
    if cfg["profiling"]:
        s.enable_profiling(True)
    if cfg["stages"] is not None:
        s.set_profiled_stages(list(cfg["stages"]))


def recipe_calls(cfg):
    """the method names recipe() may call for `cfg` and no others (test_handle_walk_cpu.py holds the recorded calls against it)"""
    d, out = HANDLE_DEFAULT, ["set_problem"]
    if cfg["track"] is not None:
        out += ["set_reference_track", "set_track_starts", "window_from_track"]
    out += ["set_contact_mode"] * ((cfg["mode"], cfg["soft"]) != (d["mode"], d["soft"]))
    for field, setter in (("mu", "set_friction"), ("limits", "set_joint_limits"), ("lim_k", "set_joint_limit_stiffness"), ("source", "set_stance_source")):
        out += [setter] * (cfg[field] != d[field])
    out += ["set_options"] * ((cfg["jac"], cfg["early_exit"]) != (d["jac"], d["early_exit"]))
    for field, setter in (("gate", "set_early_exit_gate"), ("max_iter", "set_max_iterations"), ("tol", "set_tolerance"), ("dedup", "set_dedup_saturated_retry"),
                          ("relin", "set_relinearize_unchanged"), ("repass", "set_repeat_first_pass"), ("reroll", "set_reroll_nominal"), ("listed", "set_listed_spec")):
        out += [setter] * (cfg[field] != d[field])
    if cfg["al"] is not None:
        out += ["set_augmented_lagrangian"]
        out += {None: [], "table": ["set_al_bounds"], "window": ["set_al_knot_bounds"],
                "cut": ["set_al_bounds_track", "set_al_bounds_track_starts", "al_bounds_window_from_track"]}[cfg["al"]["jc"]]
        out += {None: [], "table": ["set_al_state_bounds"], "window": ["set_al_state_knot_bounds"]}[cfg["al"]["st"]]
        out += ["set_al_task_bounds"] * bool(cfg["al"]["tk"])
    out += ["enable_profiling"] * bool(cfg["profiling"])
    out += ["set_profiled_stages"] * (cfg["stages"] is not None)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# transitions
class Transition:
    """name; group (of the issue's table); step(cfg) -> the new configuration (None: side work); apply(s, old, new, D) the calls on the
    handle; legal(cfg, state); in_b: may stand between initialize and solve() (it leaves the nominal trajectory alone);
    rollout: it changes the rollout itself -- dynamics or schedule -- so that a (b) block holds a cold start rolled out under the
    configuration before it (test_gpu_handle_walk.cold_start_under_other_dynamics: the fresh handle then solves with solve(x0))"""

    def __init__(self, name, group, step, apply, legal=None, in_b=True, rollout=False, needs_solved=False, trajectory=False):
        self.name, self.group, self.step, self.apply, self._legal, self.in_b, self.rollout, self.needs_solved = name, group, step, apply, legal, in_b, rollout, needs_solved
        self.trajectory = trajectory      # it hands the handle a trajectory of the caller's (a (b) block's fresh handle is then given it too, without initialize)

    def legal(self, cfg, state):
        if self.needs_solved and not state["solved"]:
            return False
        if self.step is not None and self.step(cfg) is None:
            return False
        return self._legal is None or bool(self._legal(cfg))

    def label(self, old, new):
        if self.step is None:
            return self.name
        f = self.name.split(":")[0]
        key = {"al_jc": lambda c: c["al"] and c["al"]["jc"], "al_st": lambda c: c["al"] and c["al"]["st"], "al_tk": lambda c: bool(c["al"] and c["al"]["tk"]),
               "al": lambda c: c["al"] is not None, "problem": lambda c: (c["refs_sets"], c["sched_sets"]), "track": lambda c: c["track"]}.get(f, lambda c: c[f])
        return "%s:%s>%s" % (f, key(old), key(new))


TRANSITIONS = {}


def _add(t):
    assert t.name not in TRANSITIONS
    TRANSITIONS[t.name] = t


def _field(field, values, group, apply, legal=None, chain=False, cycle=False, rollout=False):
    """one transition per target value of a field; chain: only between neighbours of `values`; cycle: only to the next value"""
    for i, v in enumerate(values):
        def step(cfg, v=v, i=i):
            cur = cfg[field]
            if cur == v:
                return None
            if chain and abs(values.index(cur) - i) != 1:
                return None
            if cycle and (values.index(cur) + 1) % len(values) != i:
                return None
            return dict(cfg, **{field: v})
        _add(Transition("%s:%s" % (field, v), group, step, apply, legal, rollout=rollout))


no_track = lambda c: c["track"] is None
_field("mode", (0, 2, 3, 4), "dynamics", lambda s, o, n, D: s.set_contact_mode(n["mode"], n["soft"]), chain=True, rollout=True)
_field("soft", SOFT, "dynamics", lambda s, o, n, D: s.set_contact_mode(n["mode"], n["soft"]), rollout=True)
_field("mu", MU, "dynamics", lambda s, o, n, D: s.set_friction(n["mu"]), rollout=True)
_field("limits", (False, True), "dynamics", lambda s, o, n, D: s.set_joint_limits(n["limits"]), rollout=True)
_field("lim_k", LIM_K, "dynamics", lambda s, o, n, D: s.set_joint_limit_stiffness(n["lim_k"]), rollout=True)
_field("source", ("schedule", "geometry"), "dynamics", lambda s, o, n, D: s.set_stance_source(n["source"]), rollout=True)
_field("gravity", ("earth", "low"), "dynamics",
       lambda s, o, n, D: s.set_problem(base_problem(n, D["B"])) if n["track"] is None else s.set_problem_constants(base_problem(n, D["B"])), rollout=True)
_field("refs_sets", (1, B), "problem", lambda s, o, n, D: s.set_references(*reference_arrays(n["refs_var"], n["refs_sets"], D["B"])), no_track)
_field("refs_var", ("a", "b"), "problem", lambda s, o, n, D: s.set_references(*reference_arrays(n["refs_var"], n["refs_sets"], D["B"])), no_track)
_field("sched_sets", (1, B), "problem", lambda s, o, n, D: set_schedule(s, n, D["B"]), no_track, rollout=True)
_field("sched_var", ("a", "b"), "problem", lambda s, o, n, D: set_schedule(s, n, D["B"]), no_track, rollout=True)
for _n in (1, B):
    _add(Transition("problem:%d" % _n, "problem",
                    lambda cfg, _n=_n: None if (cfg["refs_sets"], cfg["sched_sets"]) == (_n, _n) else dict(cfg, refs_sets=_n, sched_sets=_n),
                    lambda s, o, n, D: s.set_problem(base_problem(n, D["B"])), no_track, rollout=True))
_add(Transition("track:on", "problem", lambda c: dict(c, track=TRACK[0]) if c["track"] is None else None, lambda s, o, n, D: set_track(s, n, D["B"], True), rollout=True))
_add(Transition("track:step", "problem", lambda c: dict(c, track=TRACK[1 - TRACK.index(c["track"])]) if c["track"] is not None else None,
                lambda s, o, n, D: set_track(s, n, D["B"], False), rollout=True))
_add(Transition("track:off", "problem", lambda c: dict(c, track=None) if c["track"] is not None else None,
                lambda s, o, n, D: (s.clear_reference_track(), s.set_problem(base_problem(n, D["B"]))), rollout=True))
_field("weights", ("a", "b"), "problem", lambda s, o, n, D: s.set_problem_constants(base_problem(n, D["B"])), lambda c: not c["wsets"])
_add(Transition("wsets:True", "problem", lambda c: None if c["wsets"] else dict(c, wsets=True), lambda s, o, n, D: s.set_weight_sets(*weight_table(n, D["B"])), lambda c: c["al"] is None))
_add(Transition("wsets:False", "problem", lambda c: dict(c, wsets=False) if c["wsets"] else None, lambda s, o, n, D: s.clear_weight_sets()))
_options = lambda s, o, n, D: s.set_options(jacobian_mode=n["jac"], fd_eps=FD_EPS, early_exit=n["early_exit"])
_field("jac", (0, 1), "control", _options)
_field("early_exit", (True, False), "control", _options)
_field("gate", (True, False), "control", lambda s, o, n, D: s.set_early_exit_gate(n["gate"]))
_field("max_iter", MAX_ITERS, "control", lambda s, o, n, D: s.set_max_iterations(n["max_iter"]), cycle=True)
_field("tol", TOL, "control", lambda s, o, n, D: s.set_tolerance(n["tol"]))
_field("dedup", (True, False), "control", lambda s, o, n, D: s.set_dedup_saturated_retry(n["dedup"]))
_field("relin", (False, True), "control", lambda s, o, n, D: s.set_relinearize_unchanged(n["relin"]))
_field("repass", (False, True), "control", lambda s, o, n, D: s.set_repeat_first_pass(n["repass"]))
_field("reroll", (False, True), "control", lambda s, o, n, D: s.set_reroll_nominal(n["reroll"]))
_field("listed", (True, False), "control", lambda s, o, n, D: s.set_listed_spec(n["listed"]))
_field("profiling", (False, True), "reads", lambda s, o, n, D: s.enable_profiling(n["profiling"]))
_field("stages", (None, STAGES), "reads", lambda s, o, n, D: s.set_profiled_stages(None if n["stages"] is None else list(n["stages"])))
_add(Transition("al:on", "al", lambda c: dict(c, al=dict(AL_EMPTY)) if c["al"] is None else None,
                lambda s, o, n, D: s.set_augmented_lagrangian(**al_install_args(n, D["B"])), lambda c: not c["wsets"]))
_add(Transition("al:off", "al", lambda c: dict(c, al=None) if c["al"] is not None else None, lambda s, o, n, D: s.clear_augmented_lagrangian()))


def _al_part(part, v):
    def step(c):
        if c["al"] is None or c["al"][part] == v:
            return None
        return dict(c, al=dict(c["al"], **{part: v}))
    return step


for _v in (None, "table", "window", "cut"):
    _add(Transition("al_jc:%s" % _v, "al", _al_part("jc", _v), lambda s, o, n, D: set_al_jc(s, n["al"]["jc"], D["B"], o["al"]["jc"])))
for _v in (None, "table", "window"):
    _add(Transition("al_st:%s" % _v, "al", _al_part("st", _v), lambda s, o, n, D: set_al_st(s, n["al"]["st"], D["B"])))
for _v in (False, True):
    _add(Transition("al_tk:%s" % _v, "al", _al_part("tk", _v), lambda s, o, n, D: set_al_tk(s, n["al"]["tk"], D["B"])))


# ---- reads and side work between solves: the configuration stays
def _getters(s, o, n, D):
    s.cost(), s.trace(), s.iterations(), s.lambdas(), s.xbar(), s.ubar(), s.gains_K(), s.gains_kff(), s.adopt_mismatches()
    if n["al"] is not None:
        s.al_trace(), s.al_multipliers()


def _set_what_was_read(s, o, n, D):
    A, Bm = s.linearization()
    q = s.quadratics()
    s.set_linearization(A, Bm); s.set_quadratics(*q)
    s.stage_backward_pass()


def _plant(s, o, n, D):
    s.plant_configure(substeps=2, feedback_mode=1)
    s.plant_reset(D["x_warm"])
    s.plant_advance(); s.plant_follow(1, 2)
    s.plant_state(); s.plant_state_device()


def _plant_table(s, o, n, D):
    s.plant_reset(D["x_warm"])
    s.plant_set_params(sc.stack_plant_params(D["B"], friction=[0.5 + 0.01 * b for b in range(D["B"])]))
    s.plant_advance(); s.plant_state()
    s.plant_clear_params()
    s.plant_advance(); s.plant_state()


def _warm_from_plant(s, o, n, D):
    s.plant_reset(D["x_warm"]); s.plant_advance()
    s.initialize_warm_from_plant(2)
    s.synchronize()


def _lists(s, o, n, D):
    s.iteration_orders()
    try:
        s.iteration_lists(0)
    except _sv().ILQRError:
        pass                                # (the last solve kept no lists: ILQR_ERR_STATE, documented)


def _side(name, apply, in_b=True, needs_solved=True, trajectory=False):
    _add(Transition(name, "reads", None, apply, None, in_b, needs_solved=needs_solved, trajectory=trajectory))


_side("read:getters", _getters)
_side("read:linearization", lambda s, o, n, D: s.linearization())
_side("read:quadratics", lambda s, o, n, D: s.quadratics())
_side("read:value_function", lambda s, o, n, D: s.value_function())
_side("read:iteration_lists", _lists)
_side("read:stage_ms", lambda s, o, n, D: s.stage_ms())
_side("side:set_what_was_read", _set_what_was_read)
_side("side:step", lambda s, o, n, D: s.step(D["xs"], D["us"]), needs_solved=False)
_side("side:step_stance", lambda s, o, n, D: s.step_stance(D["xs"], D["us"], 1, 0), needs_solved=False)
_side("side:step_geometry", lambda s, o, n, D: s.step_geometry(D["xs"], D["us"]), needs_solved=False)
_side("side:compute_control", lambda s, o, n, D: (s.compute_control(D["x_warm"], 0), s.compute_control(D["x_warm"], 2)))
_side("side:first_knot_device", lambda s, o, n, D: s.first_knot_device())
_side("side:pack_first_knot_device", lambda s, o, n, D: s.pack_first_knot_device(*D["pack"]) if "pack" in D else s.first_knot_device())
_side("side:plant", _plant)
_side("side:plant_table", _plant_table)
_side("side:warm_from_plant", _warm_from_plant, in_b=False)      # (it replaces the nominal trajectory)
# a trajectory of the caller's that is no rollout: between initialize and solve() the solve must roll out from x0 first, not keep it
_side("side:set_trajectory", lambda s, o, n, D: s.set_trajectory(D["x_given"], D["u_given"]), needs_solved=False, trajectory=True)
# the backward pass ALONE on whatever layouts the last solve and the getters since have left S.A, S.Bm and S.lxx in
_side("side:stage_backward_pass", lambda s, o, n, D: s.stage_backward_pass())


def replay(seq, cfg=None):
    """[(step, configuration before, configuration after, label or None)] of a sequence, from START; asserts every transition is legal"""
    cfg = dict(START) if cfg is None else cfg
    state = dict(solved=False, in_b=False)
    out = []
    for step in seq:
        new, label = cfg, None
        if step[0] == "T":
            t = TRANSITIONS[step[1]]
            assert t.legal(cfg, state), (step, cfg)
            assert t.in_b or not state["in_b"], step
            new = t.step(cfg) if t.step is not None else cfg
            label = t.label(cfg, new)
        elif step[0] == "B0":
            assert not state["in_b"]; state["in_b"] = True
        elif step[0] == "B1":
            assert state["in_b"]; state["in_b"] = False; state["solved"] = True
        else:
            assert step[0] == "O" and step[1] in KINDS and step[1] != "b" and not state["in_b"]
            assert state["solved"] or step[1] in ("a", "d", "e"), step      # a warm start needs a solution
            if step[1] != "e":
                state["solved"] = True
        out.append((step, cfg, new, label))
        cfg = new
    assert not state["in_b"]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# which configurations must observe different things
def result_key(cfg):
    """the part of a configuration a solve's observables depend on: two configurations with equal keys must observe the same bits, two with
    different keys are meant to differ (DISCRIMINATING holds the bases at which every field carries weight)"""
    k = {f: v for f, v in cfg.items() if f not in ORDER_FIELDS}
    if k["mode"] < 3:
        k["mu"] = None
    if k["mode"] < 2:
        k["soft"] = k["source"] = None
    if not k["limits"]:
        k["lim_k"] = None
    if not k["early_exit"]:
        k["tol"] = None
    if k["track"] is not None:
        k["refs_var"] = k["refs_sets"] = k["sched_var"] = k["sched_sets"] = None
    k["al"] = None if k["al"] is None else tuple(sorted(k["al"].items(), key=str))
    return tuple(sorted(k.items()))


# the base (overrides of START) at which the transition into the named value changes the result; the oracle can state all but the last group
DISCRIMINATING = {
    "mode:2": {}, "mode:3": dict(mode=2, mu=MU[1]), "mode:4": dict(mode=3, mu=MU[1]), "soft:%s" % SOFT[1]: dict(mode=2), "mu:%s" % MU[1]: dict(mode=4),
    "limits:True": {}, "lim_k:%s" % LIM_K[1]: dict(limits=True), "gravity:low": {}, "refs_var:b": {}, "refs_sets:%d" % B: {}, "sched_var:b": dict(mode=2),
    "sched_sets:%d" % B: dict(mode=2), "problem:%d" % B: dict(mode=2), "track:on": {}, "track:step": dict(track=TRACK[0]), "weights:b": {}, "wsets:True": {},
    "jac:1": {}, "max_iter:3": dict(mode=2, gravity="low", early_exit=False), "tol:%s" % TOL[1]: dict(mode=2, gravity="low"),
    "early_exit:False": dict(mode=2, gravity="low", tol=TOL[1]),
}
GPU_ONLY_DISCRIMINATING = {"source:geometry": dict(mode=2), "al:on": {}, "al_jc:table": dict(al=dict(AL_EMPTY)), "al_st:table": dict(al=dict(AL_EMPTY)),
                           "al_tk:True": dict(al=dict(AL_EMPTY), mode=2)}
ORACLE_ROLLOUTS = (1, 11, 19, 29, 35, 37)      # two per k_control workgroup of the B = 40 batch: odd (past a joint limit), no multiple of 3 (sets differ)
DISCRIMINATION_MARGIN = 1e-6


def discriminating_pair(name):
    """(configuration before, configuration after) of a transition of DISCRIMINATING / GPU_ONLY_DISCRIMINATING"""
    before = dict(START, **{**DISCRIMINATING, **GPU_ONLY_DISCRIMINATING}[name])
    t = TRANSITIONS[name]
    assert t.legal(before, dict(solved=True)), name
    return before, t.step(before)


def oracle_of(cfg, b, nb=B):
    """the oracle under a configuration it can state (no stance geometry, no augmented Lagrangian), for rollout b"""
    assert cfg["source"] == "schedule" and cfg["al"] is None
    prob = problem(dict(cfg, wsets=False), nb)
    if cfg["wsets"]:
        w = weight_scale(nb)[b]
        prob = dict(prob, Q=prob["Q"] * w, Qf=prob["Qf"] * w)
    o = ol.Oracle(N, prob["dt"]); o.set_problem(prob, b)
    o.set_contact_mode(cfg["mode"], cfg["soft"]); o.set_friction(cfg["mu"])
    o.set_joint_limits(cfg["limits"]); o.set_joint_limit_stiffness(cfg["lim_k"])
    o.set_options(lam=LAMBDA0, max_iter=cfg["max_iter"], tol=cfg["tol"], jac_mode=cfg["jac"], fd_eps=FD_EPS, early_exit=int(cfg["early_exit"]))
    return o


_oracle_costs = {}


def oracle_cost(cfg, b):
    """final cost of the oracle's cold solve of rollout b of the B = 40 start under `cfg`; remembered by result_key"""
    key = (result_key(cfg), b)
    if key not in _oracle_costs:
        D = inputs(B)
        o = oracle_of(cfg, b)
        o.initialize(D["x0"][b], D["ui"][b])
        _oracle_costs[key] = o.solve(D["x0"][b])[1]
    return _oracle_costs[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# sequences
def T(*names):
    return [("T", n) for n in names]


def O(kind):
    return [("O", kind)]


def Bk(*names):
    """observation kind (b): initialize, the transitions, solve()"""
    return [("B0",)] + T(*names) + [("B1",)]


def directed():
    """[(family of facts, name, sequence)]: one sequence per remembered fact, named after it"""
    s1, k1, m1, t1 = SOFT[1], LIM_K[1], MU[1], TOL[1]
    out = []
    # ---- xbar_rolled / rolled_variant / rolled_dyn / first_aside: a cold start, ONE change, solve()
    aside = [("schedule", ["sched_var:b"], ["mode:2"]), ("schedule_sets", ["sched_sets:%d" % B], ["mode:2"]), ("contact_mode", ["mode:2"], []),
             ("softness", ["soft:%s" % s1], ["mode:2"]), ("friction", ["mu:%s" % m1], ["mode:2", "mode:3"]), ("gravity", ["gravity:low"], []),
             ("joint_limits", ["limits:True"], []), ("limit_stiffness", ["lim_k:%s" % k1], ["limits:True"]), ("stance_source", ["source:geometry"], ["mode:2"]),
             ("references", ["refs_var:b"], []), ("reference_sets", ["refs_sets:%d" % B], []), ("weights", ["weights:b"], []),
             ("weight_set_table", ["wsets:True"], []), ("weight_set_table_cleared", ["wsets:False"], ["wsets:True"]),
             ("al_installed", ["al:on"], []), ("al_cleared", ["al:off"], ["al:on", "al_jc:table"]), ("track_window", ["track:on"], ["mode:2"]),
             ("reroll_nominal", ["reroll:True"], []), ("nothing", [], [])]
    for name, change, before in aside:
        out.append(("cold_start_aside", name, T(*before) + O("a") + Bk(*change) + O("c1")))
    out.append(("cold_start_aside", "set_trajectory", O("a") + Bk("side:set_trajectory") + O("c1")))
    out.append(("cold_start_aside", "set_trajectory_on_a_handle_that_never_solved", Bk("side:set_trajectory") + T("mode:2") + Bk("side:set_trajectory") + O("c2")))
    out.append(("cold_start_aside", "nothing_behind_warm_starts", O("a") + O("c1") + Bk() + O("c2")))
    # ---- lxx_layout / ab_packed / ab_pads_clean / packed_h / lin_fold_h
    out.append(("layouts", "linearization_read_then_warm_solve", O("a") + T("read:linearization") + O("c1") + T("read:linearization", "read:quadratics") + O("d")))
    out.append(("layouts", "quadratics_read_backward_pass_then_warm_solve", O("a") + T("read:quadratics", "side:stage_backward_pass") + O("c1")
                + T("read:quadratics", "side:stage_backward_pass", "read:getters") + O("c2") + T("mode:2") + O("a") + T("read:quadratics", "side:stage_backward_pass") + O("c1")))
    out.append(("layouts", "linearization_read_backward_pass_then_warm_solve", O("a") + T("read:linearization", "side:stage_backward_pass") + O("c1")
                + T("side:stage_backward_pass", "read:linearization", "read:quadratics", "side:stage_backward_pass") + O("c2") + T("side:stage_backward_pass") + O("e")))
    out.append(("layouts", "backward_pass_alone_between_analytic_and_forward_difference_solves", O("a") + T("side:stage_backward_pass", "jac:1") + O("a")
                + T("read:quadratics", "side:stage_backward_pass", "jac:0") + O("c1") + Bk("read:linearization", "side:stage_backward_pass")))
    out.append(("layouts", "what_was_read_set_again_then_warm_solve", O("a") + T("read:quadratics", "side:set_what_was_read") + O("c1")))
    out.append(("layouts", "analytic_forward_difference_analytic", O("a") + T("jac:1") + O("a") + T("jac:0") + O("a") + T("jac:1") + O("c1") + T("jac:0") + O("c2")))
    out.append(("layouts", "stage_api_after_a_full_solve", O("e") + O("a") + O("e") + T("jac:1") + O("a") + O("e") + T("jac:0") + O("e")))
    out.append(("layouts", "set_linearization_of_unknown_origin_then_analytic_solve", O("a") + T("side:set_what_was_read") + O("a") + T("side:set_what_was_read") + O("e")))
    out.append(("layouts", "contact_mode_changes_the_backward_kernel", O("a") + T("mode:2") + O("e") + T("mode:3", "mu:%s" % m1) + O("a") + T("mode:2", "mode:0") + O("e")))
    # ---- buffers sized by an earlier solve
    out.append(("buffers", "max_iterations_6_3_8_6", T("early_exit:False") + O("a") + T("read:iteration_lists", "max_iter:3") + O("a") + T("read:iteration_lists", "max_iter:8") + O("c1")
                + T("read:iteration_lists", "max_iter:6") + O("a") + T("read:iteration_lists") + O("c2")))
    out.append(("buffers", "max_iterations_with_the_convergence_exit", O("a") + T("max_iter:3") + O("a") + T("max_iter:8", "tol:%s" % t1) + O("a") + T("max_iter:6") + O("c1")))
    out.append(("buffers", "no_twin_then_twin", T("jac:1", "early_exit:False") + O("a") + T("jac:0") + O("a") + T("jac:1") + O("c1")))
    out.append(("buffers", "twin_then_no_twin", T("early_exit:False") + O("a") + T("jac:1") + O("a") + T("jac:0") + O("c1")))
    out.append(("buffers", "profiling_on_between_two_solves_and_off", O("a") + T("profiling:True") + O("a") + T("read:stage_ms", "stages:%s" % (STAGES,)) + O("c1")
                + T("read:stage_ms", "profiling:False") + O("a") + T("stages:None") + O("d")))
    out.append(("buffers", "orders_switched_between_solves", T("early_exit:False") + O("a") + T("listed:False", "dedup:False") + O("a") + T("relin:True", "repass:True") + O("c1")
                + T("reroll:True", "gate:False") + O("a") + T("listed:True", "dedup:True", "relin:False", "repass:False", "reroll:False", "gate:True") + O("c2")))
    out.append(("buffers", "gate_and_exit", O("a") + T("gate:False") + O("a") + T("early_exit:False") + O("c1") + T("gate:True", "early_exit:True") + O("a")))
    # ---- installed and removed
    out.append(("installed_removed", "weight_sets", O("a") + T("wsets:True") + O("a") + T("wsets:False") + O("a") + T("weights:b", "wsets:True") + O("c1") + T("wsets:False") + O("c2") + T("weights:a") + O("a")))
    out.append(("installed_removed", "reference_track", T("mode:2") + O("a") + T("track:on") + O("a") + T("track:step") + O("c1") + T("gravity:low", "track:step") + O("a") + T("track:off") + O("a")
                + T("gravity:earth", "problem:%d" % B) + O("c1") + T("track:on") + O("a") + T("track:step", "track:off", "problem:1") + O("a")))
    out.append(("installed_removed", "one_set_and_B_sets", O("a") + T("refs_sets:%d" % B) + O("a") + T("sched_sets:%d" % B, "mode:2") + O("c1") + T("refs_sets:1") + O("a")
                + T("sched_sets:1") + O("a") + T("problem:%d" % B) + O("a") + T("refs_var:b", "sched_var:b") + O("c2") + T("problem:1") + O("a") + T("refs_var:a", "sched_var:a") + O("a")))
    out.append(("installed_removed", "augmented_lagrangian_families", T("mode:2", "early_exit:False", "al:on") + O("a") + T("al_tk:True", "al_st:table") + O("a") + T("al_jc:table") + O("c1")
                + T("al_jc:window", "al_st:window") + O("a") + T("al_tk:False", "al_jc:cut") + O("a") + T("al_st:None", "al_jc:table") + O("d") + T("al_jc:None") + O("e")
                + T("al_jc:cut", "al_tk:True") + O("c1") + T("al:off") + O("a") + T("al:on", "al_st:window") + O("a") + T("al_st:table", "al_jc:window", "al_jc:None") + Bk("al_st:None") + T("al:off", "mode:0") + O("a")))
    out.append(("installed_removed", "plant_table", O("a") + T("side:plant_table") + O("c1") + T("side:plant", "side:plant_table") + O("cp") + T("side:plant_table") + O("a")))
    # ---- side work between initialize and solve(), and between a solve and its warm start
    out.append(("side_work", "between_a_solve_and_its_warm_start", O("a") + T("side:plant", "side:step", "side:step_stance", "side:step_geometry", "side:compute_control") + O("c1")
                + T("side:first_knot_device", "side:pack_first_knot_device", "read:getters", "read:value_function") + O("c2") + T("side:warm_from_plant") + O("c1") + T("side:warm_from_plant") + O("a")))
    out.append(("side_work", "between_initialize_and_solve", O("a") + Bk("side:plant", "side:step", "side:compute_control") + Bk("side:step_stance", "side:step_geometry", "read:getters")
                + T("mode:2") + Bk("side:plant", "side:first_knot_device", "side:pack_first_knot_device", "read:linearization", "read:quadratics") + O("cp") + O("d")))
    out.append(("side_work", "dynamics_walk", O("a") + T("mode:2") + O("a") + T("soft:%s" % s1) + O("c1") + T("mode:3", "mu:%s" % m1) + O("a") + T("mode:4") + O("c2") + T("limits:True") + O("a")
                + T("lim_k:%s" % k1, "source:geometry") + O("a") + T("mode:3", "source:schedule") + O("d") + T("limits:False", "mu:%s" % MU[0]) + O("a") + T("mode:2", "soft:%s" % SOFT[0], "lim_k:%s" % LIM_K[0]) + O("c1")
                + T("mode:0", "tol:%s" % t1) + O("a") + T("tol:%s" % TOL[0]) + O("a")))
    return out


WALK_SEEDS = (11, 12, 13, 14, 15, 16)
WALK_TRANSITIONS = 12


def random_walks(seeds=WALK_SEEDS, n=WALK_TRANSITIONS):
    """{seed: sequence}: per seed n transitions from START, drawn among the legal ones with the fewest visits so far (over the walks in the
    order of `seeds`: the generator is one deterministic function of the seeds), an observation after every second; the observation kinds in
    turn, (b) blocks with the two transitions inside"""
    visits, out = {}, {}
    for w, seed in enumerate(seeds):
        rng = np.random.default_rng(seed)
        cfg, state, seq = dict(START), dict(solved=False), []
        for pair in range(n // 2):
            kind = KINDS[(w + pair) % len(KINDS)] if state["solved"] else ("a", "d")[w % 2]
            in_b = kind == "b"
            drawn = []
            for _ in range(2):
                legal = [t for t in TRANSITIONS.values() if t.legal(cfg, state) and (t.in_b or not in_b)]
                new_of = {t.name: (t.step(cfg) if t.step is not None else cfg) for t in legal}
                fewest = min(visits.get(t.label(cfg, new_of[t.name]), 0) for t in legal)
                pool = sorted(t.name for t in legal if visits.get(t.label(cfg, new_of[t.name]), 0) == fewest)
                name = pool[int(rng.integers(len(pool)))]
                lab = TRANSITIONS[name].label(cfg, new_of[name])
                visits[lab] = visits.get(lab, 0) + 1
                drawn.append(name); cfg = new_of[name]
            seq += Bk(*drawn) if in_b else T(*drawn) + O(kind)
            state["solved"] = state["solved"] or kind != "e"
        out[seed] = seq
    return out


# the two walks whose last solve is held to the oracle: one free, one in contact mode 2; each ends with a cold observation (a) in a
# configuration the oracle states
ANCHOR_TAILS = {"free": T("early_exit:False", "refs_var:b") + O("a") + T("gravity:low", "jac:1") + O("c1") + T("jac:0", "max_iter:3") + O("a") + T("max_iter:8", "max_iter:6", "refs_sets:%d" % B) + O("a"),
                "contact2": T("early_exit:False", "mode:2") + O("a") + T("sched_var:b", "soft:%s" % SOFT[1]) + O("c2") + T("sched_sets:%d" % B, "limits:True") + O("a") + T("limits:False", "wsets:True") + O("a")}


def required_labels():
    """the visit labels the sequences must cover between them: every transition, every two-valued one in both directions"""
    need = set()
    for field, values in (("soft", SOFT), ("mu", MU), ("limits", (False, True)), ("lim_k", LIM_K), ("source", ("schedule", "geometry")), ("gravity", ("earth", "low")),
                          ("refs_sets", (1, B)), ("refs_var", ("a", "b")), ("sched_sets", (1, B)), ("sched_var", ("a", "b")), ("weights", ("a", "b")), ("wsets", (False, True)),
                          ("jac", (0, 1)), ("early_exit", (True, False)), ("gate", (True, False)), ("tol", TOL), ("dedup", (True, False)), ("relin", (False, True)),
                          ("repass", (False, True)), ("reroll", (False, True)), ("listed", (True, False)), ("profiling", (False, True)), ("stages", (None, STAGES)),
                          ("al", (False, True)), ("al_tk", (False, True))):
        need |= {"%s:%s>%s" % (field, values[0], values[1]), "%s:%s>%s" % (field, values[1], values[0])}
    for a, b in ((0, 2), (2, 3), (3, 4)):
        need |= {"mode:%d>%d" % (a, b), "mode:%d>%d" % (b, a)}
    for i, v in enumerate(MAX_ITERS):
        need.add("max_iter:%d>%d" % (v, MAX_ITERS[(i + 1) % 3]))
    need |= {"problem:(1, 1)>(%d, %d)" % (B, B), "problem:(%d, %d)>(1, 1)" % (B, B)}
    need |= {"track:None>%s" % (TRACK[0],), "track:%s>%s" % TRACK, "track:%s>%s" % TRACK[::-1], "track:%s>None" % (TRACK[0],), "track:%s>None" % (TRACK[1],)}
    for part, values in (("al_jc", (None, "table", "window", "cut")), ("al_st", (None, "table", "window"))):
        for v in values:                                                 # each bounds source installed and left at least once
            need.add(("into", part, v)); need.add(("out of", part, v))
    need |= {t.name for t in TRANSITIONS.values() if t.step is None}
    return need


def covered_labels(sequences):
    got = set()
    for seq in sequences:
        for step, old, new, label in replay(seq):
            if label is None:
                continue
            got.add(label)
            f = label.split(":")[0]
            if f in ("al_jc", "al_st") and old["al"] is not None and new["al"] is not None:
                part = f[3:]
                got.add(("into", f, new["al"][part])); got.add(("out of", f, old["al"][part]))
    return got


def all_sequences():
    return [seq for _, _, seq in directed()] + list(random_walks().values()) + list(ANCHOR_TAILS.values())
