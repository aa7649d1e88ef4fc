"""Closed-loop batched MPC on loaded references, with the reference's CSV logs -- SURVEY.md 8(f) row f3.

Mirrors (host side; the solve itself is the HIP library):
  * runSimulation / MPC::stepOnce       /root/reference/main/humanoid_mpc.cpp:126-190, src/ilqr/mpc.cpp:40-127
      per step: reference window -> warm start (shifted previous solution) -> solve -> u = ubar0 + K0 (x - xbar0)
      -> plant step.  The plant here is the same dynamics as the model (`BatchedILQR.step`, or `step_stance` with the
      stance flags of the current schedule row when the solver is in contact mode); the
      reference steps MuJoCo with contacts and clobbers its plant state while solving
       -- neither is reproduced.
  * MPC::initCSVLog / logCurrentStep    src/ilqr/mpc.cpp:181-262   main log, one row per step
  * MPC::logAppliedOptimal              src/ilqr/mpc.cpp:271-343   q_optimal.csv, u_optimal.csv
      (`step,time_sec,q_0..q_25` / `step,time_sec,u_0..u_18`, first knot of the optimised trajectory; the step index
      is the one AFTER the increment in stepOnce, i.e. 1-based), so plotter.py-style tooling keeps working.
  * profiler keys and table             include/common/profiler.hpp, main/humanoid_mpc.cpp:195-226
      `MPCRunner.prof[key]` = list of milliseconds per call for MPC_stepOnce, MPC_extractReference, MPC_warmStart,
      MPC_iLQR_solve, MPC_computeControl (host clock, as the reference measures them) and, with `profile_stages=True`, the
      iLQR_* keys from the device events of the solve; `profiling_table()` formats them as `printProfilingResults` does.
One log set per logged rollout (`log_rollouts`), the reference being single-trajectory.

`MPCRunner(..., resident=True)` keeps the plant in the solver handle (include/ilqr_hip.h "device-resident plant"): after the cold start
of the first step every step is  set_problem -> initialize_warm_from_plant -> solve(None) -> plant_advance,  with no upload of x, no
download of u or x_next and no synchronisation but the solve's own.  `substeps` plant steps of dt / substeps per MPC step
(physics_steps_per_mpc, main/humanoid_mpc.cpp:128,168-170) and `feedback_mode` 1 (u = ubar0 + K0 (x - xbar0) re-evaluated before every
substep) exist on that path only.  States and controls come back from the history ring in one download when the run ends, and the CSV
logs are written then, in the same formats (a logged run also fetches the first knot of the solution once per step: q_optimal.csv /
u_optimal.csv hold it).  `run(..., kicks={step: dv})` adds dv [B,25] to the plant's qvel in that step, between the solve and the control
law: the solver meets the push one step later, as a controller meets a push that arrives between measurement and actuation.

`MPCRunner(..., solve_every=m)`, m > 1, solves before every m-th plant interval only and follows the time-varying policy
u = ubar_j + K_j (x - xbar_j), j = 0..m-1, in between (the reference solves every step and only ever uses knot 0).  Groups are counted from
the start of each `run`; the warm start shifts by the number of intervals applied since the last solve.  Resident path, per group:
set_problem -> initialize_warm_from_plant(shift=m) -> solve(None) -> plant_follow(0, m), t_idx += m; a kick is supported before the first
interval of a group only.  Host path: compute_control(x, knot=j) and today's plant step per interval, the stance taken from row j of the
group's window.  The logs keep one main row per plant interval, the solve cost and time repeated over the group.

`MPCRunner(..., resident=True, score={...})` installs the closed-loop score of the plant (BatchedILQR.plant_set_score; the dict holds its
arguments) before the plant is reset: every plant call then adds the cost terms of its intervals, under the score's own weights, to a
record per rollout on the device, and `runner.score()` returns it [B, 8] after `run`.  `history_rows=r` sizes the history ring to r rows
instead of the whole run (r >= solve_every: a plant call must fit); `run` then returns the last min(r, steps) states and controls the ring
still holds -- with a score, a run of any length is judged without keeping its history.

`MPCRunner(..., resident=True, device_refs=True, track_starts=None)` cuts the reference windows on the device too: the first `run` sets the
weights and gravity of `base_problem` and uploads the whole of `refs` as a track (BatchedILQR.set_reference_track) with one start row per
rollout (`track_starts` [B]; None or one entry: one shared start, 0 by default), and every group calls
`window_from_track(t_idx, follow_schedule)` where the host path calls problem_at + set_problem -- one kernel, nothing uploaded, no
synchronisation; rollout b then tracks the rows from track_starts[b] + t_idx on (ReferenceData.problem_at_starts is the same rule on the
host).  While the solver handle has a bounds track of either kind (BatchedILQR.set_al_bounds_track, set_al_task_bounds_track) every solve of
either loop also calls `al_bounds_window_from_track` with the step index its reference windows use, and `track_starts` feeds the tracks' shared
start rows as well; without a bounds track there is no new call.  `MPCRunner(..., resident=True, task_score=tol)` installs the task score of the
plant (BatchedILQR.plant_set_task_score) before the plant is reset: every plant call then scores its intervals against the task window the
handle holds, and `runner.task_score()` returns the record [B, 8] after `run`.  MPC_extractReference times the enqueue only.  The logged reference rows come from the host's copy of the rule, for the logged
rollouts alone, and `last_stance0` from the host's contact table (rollout 0).

`MPCRunner(..., resident=True, plant_model=(contact_mode, joint_limits), plant_params=P)` runs closed loops in which the plant is not the
solver's model: `plant_model` gives the plant its own contact mode and joint-limit option (either None: the solver's;
BatchedILQR.plant_set_model), `plant_params` [1, 7] or [B, 7] (scenario.stack_plant_params) its own gravity, friction, softness,
joint-limit stiffness and torque gain, one set for all rollouts or one per rollout (BatchedILQR.plant_set_params).  Both are installed
before the plant is reset and stay on the handle after the run; the solve keeps the solver's model throughout.

`MPCRunner(..., resident=True, plant_wrench=W)` pushes the plant: W [1, 11] or [B, 11] (scenario.stack_plant_wrench) is a sustained external
wrench on the pelvis per rollout -- force, torque, point of application and the window of plant intervals it acts in, counted from the
reset of the run (BatchedILQR.plant_set_wrench).  Installed behind the parameter sets, in front of the reset; the solve does not know of it.

`MPCRunner(..., resident=True, plant_payload=P)` loads the plant: P [1, 10] or [B, 10] (scenario.stack_plant_payload) is a rigid payload fixed
to the pelvis per rollout -- mass, centre of mass and rotational inertia, carried over the whole run (BatchedILQR.plant_set_payload).  Installed
beside the wrench, in front of the reset; the solve keeps the unloaded model.

`MPCRunner(..., resident=True, plant_observation=O, observation_seed=S, observation_stream0=0)` blurs what the controller is told: O [1, 100]
or [B, 100] (scenario.stack_plant_observation) is a bias and a noise level per tangent coordinate and rollout; the warm starts and the
plant's control law read the plant state with that error, drawn once per plant interval on the device (BatchedILQR.plant_set_observation).
The cold first step initialises from plant_get_observed(); physics, ring and score stay on the true state.

`MPCRunner(..., resident=True, plant_actuator=A, actuator_seed=S, actuator_stream0=0)` puts an actuator between the control law and the
joints: A [1, 39] or [B, 39] (scenario.stack_plant_actuator) is a delay in plant substeps, a lag time constant and a torque noise level per
joint and rollout (BatchedILQR.plant_set_actuator).  The log and the score keep the commanded torque; the solve knows of none of it.

`MPCRunner(..., resident=True, plant_joints=J)` gives every rollout's plant joints of its own: J [1, 76] or [B, 76]
(scenario.stack_plant_joints) is a torque gain, a scale on the torque range, a damping and an armature per joint and rollout
(BatchedILQR.plant_set_joints), installed in front of the reset.  The log and the score keep the commanded torque; the solve keeps the model's joints.

`MPCRunner(..., resident=True, plant_contacts="geometry", plant_terrain=T)` puts a floor of its own height under each rollout's feet: T [1, 5]
or [B, 5] (scenario.stack_plant_terrain) is a height under the left and the right foot, an edge in x behind which the height holds and the
window of plant intervals it holds in, counted from the reset of the run (BatchedILQR.plant_set_terrain), installed behind the joints, in
front of the reset.  The plant's feet land and lift against that floor; the solve and the score's schedule know nothing of it.

`MPCRunner(..., resident=True, starts=G, start_sigma=S, start_hold=1, start_seed=0)` spends the batch on B / G robots: the batch is cut into
solve groups of G consecutive rollouts (BatchedILQR.set_groups) that share x0, references and plant tables -- the caller repeats them with
scenario.repeat_for_groups -- and every solve runs  warm start -> group_perturb -> solve -> group_select -> group_adopt -> plant call:  the
members g >= 1 start from the shifted previous solution plus S o z (S a scalar, [19] or [G, 19], scenario.stack_group_sigma; one draw per
`start_hold` knots), member 0 from the shifted solution itself, and the member with the lowest solve cost drives all G plants of its group,
which therefore stay bit-identical.  The cold start is perturbed too, behind `initialize`.  Nothing synchronises but the solve; the winners of
every solve are logged on the device and `runner.winners` [solves, B / G] (global rollout indices) is downloaded once when the run ends.
starts > 1 is refused on the host-plant path and together with plant_observation / plant_actuator, whose streams are per rollout: the members of
a group would measure different states.  starts = 1: exactly the calls of a runner without it.
"""
import os
import time

import numpy as np

NQ, NV, NX, NU = 26, 25, 51, 19


class MPCLogs:
    """The three CSV files of one rollout, in the reference's formats."""

    def __init__(self, directory, dt, log_name="mpc_log.csv"):
        os.makedirs(directory, exist_ok=True)
        self.dt = dt
        self.main = open(os.path.join(directory, log_name), "w")
        self.q = open(os.path.join(directory, "q_optimal.csv"), "w")
        self.u = open(os.path.join(directory, "u_optimal.csv"), "w")
        self.main.write("time_index,time_sec,solve_cost,solve_time_ms" + "".join(",x_%d" % i for i in range(NX)) + "".join(",u_%d" % i for i in range(NU))
                        + "".join(",x_ref_%d" % i for i in range(NX)) + "".join(",u_ref_%d" % i for i in range(NU)) + "\n")
        self.q.write("step,time_sec" + "".join(",q_%d" % i for i in range(NQ)) + "\n")
        self.u.write("step,time_sec" + "".join(",u_%d" % i for i in range(NU)) + "\n")

    @staticmethod
    def _fmt(v):
        return "%.6g" % v          # std::ostream default formatting (6 significant digits)

    def log(self, t_idx, solve_cost, solve_ms, x_measured, u_applied, x_ref0, u_ref0, x_opt0, u_opt0):
        f = self._fmt
        self.main.write(",".join([str(t_idx), f(t_idx * self.dt), f(solve_cost), f(solve_ms)] + [f(v) for v in x_measured] + [f(v) for v in u_applied]
                                 + [f(v) for v in x_ref0] + [f(v) for v in u_ref0]) + "\n")
        self.q.write(",".join([str(t_idx), f(t_idx * self.dt)] + [f(v) for v in x_opt0[:NQ]]) + "\n")
        self.u.write(",".join([str(t_idx), f(t_idx * self.dt)] + [f(v) for v in u_opt0]) + "\n")

    def close(self):
        for fh in (self.main, self.q, self.u):
            fh.flush(); fh.close()


class MPCRunner:
    """Batched closed loop: `solver` = BatchedILQR, `refs` = ReferenceData, `base_problem` = weights etc. (scenario.make_problem)."""

    def __init__(self, solver, refs, base_problem, log_dir=None, log_rollouts=(0,), follow_schedule=False, profile_stages=False, plant_contacts="schedule",
                 resident=False, substeps=1, feedback_mode=0, solve_every=1, score=None, history_rows=None,
                 device_refs=False, track_starts=None, task_score=None, plant_params=None, plant_model=None, plant_wrench=None, plant_payload=None,
                 plant_observation=None, observation_seed=0, observation_stream0=0, plant_actuator=None, actuator_seed=0, actuator_stream0=0, plant_joints=None,
                 plant_terrain=None, starts=1, start_sigma=None, start_hold=1, start_seed=0):
        self.starts = int(starts)
        if self.starts < 1:
            raise ValueError("starts must be >= 1 and divide the batch")
        if self.starts > 1:
            if solver.B % self.starts:
                raise ValueError("starts must be >= 1 and divide the batch")
            if not resident:
                raise ValueError("starts > 1 needs the device-resident plant (resident=True)")
            if plant_observation is not None or plant_actuator is not None:
                raise ValueError("starts > 1 together with plant_observation / plant_actuator is not supported: their streams are per rollout, the members of a group would measure different states")
            if start_sigma is None:
                raise ValueError("starts > 1 needs start_sigma (a scalar, [19] or [starts, 19]: scenario.stack_group_sigma)")
            start_sigma = np.asarray(start_sigma, dtype=np.float64)
            start_sigma = np.broadcast_to(start_sigma, (1, NU)).copy() if start_sigma.ndim < 2 else start_sigma
            if start_sigma.shape not in ((1, NU), (self.starts, NU)) or int(start_hold) < 1:
                raise ValueError("start_sigma must be a scalar, [19], [1, 19] or [starts, 19], start_hold >= 1")
        self.start_sigma, self.start_hold, self.start_seed = start_sigma, int(start_hold), int(start_seed)
        self.winners = None
        if plant_contacts not in ("schedule", "geometry"):
            raise ValueError("plant_contacts must be 'schedule' or 'geometry'")
        if not resident and (int(substeps) != 1 or int(feedback_mode) != 0):
            raise ValueError("substeps / feedback_mode need the device-resident plant (resident=True)")
        if int(solve_every) < 1 or (int(solve_every) > 1 and int(solve_every) > solver.N - 1):
            raise ValueError("solve_every must be in 1 .. N - 1")
        if not resident and (score is not None or history_rows is not None or task_score is not None):
            raise ValueError("score / task_score / history_rows need the device-resident plant (resident=True)")
        if history_rows is not None and int(history_rows) < int(solve_every):
            raise ValueError("history_rows must be at least solve_every (the ring holds the intervals of one plant call)")
        if not resident and (device_refs or track_starts is not None):
            raise ValueError("device_refs / track_starts need the device-resident plant (resident=True)")
        if track_starts is not None and not device_refs:
            raise ValueError("track_starts need device_refs=True (the host path cuts one shared window, problem_at)")
        if not resident and (plant_params is not None or plant_model is not None):
            raise ValueError("plant_params / plant_model need the device-resident plant (resident=True)")
        if plant_model is not None and len(tuple(plant_model)) != 2:
            raise ValueError("plant_model must be (contact_mode, joint_limits), either None to follow the solver")
        if plant_params is not None:
            plant_params = np.atleast_2d(np.asarray(plant_params, dtype=np.float64))
            if plant_params.ndim != 2 or plant_params.shape[1] != 7 or plant_params.shape[0] not in (1, solver.B):
                raise ValueError("plant_params must be [1, 7] or [B, 7] (scenario.stack_plant_params)")
        self.plant_params, self.plant_model = plant_params, None if plant_model is None else tuple(plant_model)
        if not resident and plant_wrench is not None:
            raise ValueError("plant_wrench needs the device-resident plant (resident=True)")
        if plant_wrench is not None:
            plant_wrench = np.atleast_2d(np.asarray(plant_wrench, dtype=np.float64))
            if plant_wrench.ndim != 2 or plant_wrench.shape[1] != 11 or plant_wrench.shape[0] not in (1, solver.B):
                raise ValueError("plant_wrench must be [1, 11] or [B, 11] (scenario.stack_plant_wrench)")
        self.plant_wrench = plant_wrench
        if not resident and plant_payload is not None:
            raise ValueError("plant_payload needs the device-resident plant (resident=True)")
        if plant_payload is not None:
            plant_payload = np.atleast_2d(np.asarray(plant_payload, dtype=np.float64))
            if plant_payload.ndim != 2 or plant_payload.shape[1] != 10 or plant_payload.shape[0] not in (1, solver.B):
                raise ValueError("plant_payload must be [1, 10] or [B, 10] (scenario.stack_plant_payload)")
        self.plant_payload = plant_payload
        if not resident and plant_observation is not None:
            raise ValueError("plant_observation needs the device-resident plant (resident=True)")
        if plant_observation is not None:
            plant_observation = np.atleast_2d(np.asarray(plant_observation, dtype=np.float64))
            if plant_observation.ndim != 2 or plant_observation.shape[1] != 100 or plant_observation.shape[0] not in (1, solver.B):
                raise ValueError("plant_observation must be [1, 100] or [B, 100] (scenario.stack_plant_observation)")
        self.plant_observation, self.observation_seed, self.observation_stream0 = plant_observation, int(observation_seed), int(observation_stream0)
        if not resident and plant_actuator is not None:
            raise ValueError("plant_actuator needs the device-resident plant (resident=True)")
        if plant_actuator is not None:
            plant_actuator = np.atleast_2d(np.asarray(plant_actuator, dtype=np.float64))
            if plant_actuator.ndim != 2 or plant_actuator.shape[1] != 39 or plant_actuator.shape[0] not in (1, solver.B):
                raise ValueError("plant_actuator must be [1, 39] or [B, 39] (scenario.stack_plant_actuator)")
        self.plant_actuator, self.actuator_seed, self.actuator_stream0 = plant_actuator, int(actuator_seed), int(actuator_stream0)
        if not resident and plant_joints is not None:
            raise ValueError("plant_joints needs the device-resident plant (resident=True)")
        if plant_joints is not None:
            plant_joints = np.atleast_2d(np.asarray(plant_joints, dtype=np.float64))
            if plant_joints.ndim != 2 or plant_joints.shape[1] != 76 or plant_joints.shape[0] not in (1, solver.B):
                raise ValueError("plant_joints must be [1, 76] or [B, 76] (scenario.stack_plant_joints)")
        self.plant_joints = plant_joints
        if not resident and plant_terrain is not None:
            raise ValueError("plant_terrain needs the device-resident plant (resident=True)")
        if plant_terrain is not None:
            if plant_contacts != "geometry":
                raise ValueError("plant_terrain needs plant_contacts='geometry': with the schedule as the contact source nothing consults the floor")
            plant_terrain = np.atleast_2d(np.asarray(plant_terrain, dtype=np.float64))
            if plant_terrain.ndim != 2 or plant_terrain.shape[1] != 5 or plant_terrain.shape[0] not in (1, solver.B):
                raise ValueError("plant_terrain must be [1, 5] or [B, 5] (scenario.stack_plant_terrain)")
        self.plant_terrain = plant_terrain
        self.device_refs, self.track_ready = bool(device_refs), False
        self.track_starts_given, self.bounds_starts_for = track_starts is not None, None
        self.track_starts = np.zeros(1, dtype=np.int64) if track_starts is None else np.atleast_1d(np.asarray(track_starts)).astype(np.int64)
        self.score_args = None if score is None else dict(score)
        self.task_score_tol = None if task_score is None else float(task_score)
        self.history_rows = None if history_rows is None else int(history_rows)
        self.resident, self.substeps, self.feedback_mode = bool(resident), int(substeps), int(feedback_mode)
        self.solve_every, self.since_solve = int(solve_every), 1      # since_solve: plant intervals applied since the last solve (the next warm start's shift)
        self.s, self.refs, self.base = solver, refs, base_problem
        # "geometry": the plant finds its contacts from the foot hulls (BatchedILQR.step_geometry, the solver's contact mode), as mj_step
        # does in the reference's plant (robot_utils.cpp:106-117); "schedule": the stance flags of the current schedule row
        self.plant_contacts = plant_contacts
        self.plant_stance = []
        self.prof = {}
        self.profile_stages = profile_stages
        if profile_stages:
            solver.enable_profiling(True)
        self.follow_schedule = follow_schedule
        self.t_idx, self.has_prev = 0, False
        self.logs = {b: MPCLogs(os.path.join(log_dir, "rollout_%d" % b), base_problem["dt"]) for b in log_rollouts} if log_dir else {}
        self.last_cost = None

    def _add(self, key, t_a, t_b):
        self.prof.setdefault(key, []).append(1e3 * (t_b - t_a))

    def profiling_table(self):
        """The table of printProfilingResults (main/humanoid_mpc.cpp:195-226): Function, Calls, Total / Avg / Min / Max in ms."""
        lines = ["", "=== Performance Profiling ===", "", "--- Timing Summary ---",
                 "%-20s%8s%12s%12s%12s%12s" % ("Function", "Calls", "Total(ms)", "Avg(ms)", "Min(ms)", "Max(ms)"), "-" * 76]
        for key in sorted(self.prof):
            t = self.prof[key]
            if t:
                lines.append("%-20s%8d%12.2f%12.2f%12.2f%12.2f" % (key, len(t), sum(t), sum(t) / len(t), min(t), max(t)))
        return "\n".join(lines)

    def _add_stage_ms(self):
        ms, _ = self.s.stage_ms()
        for key, val in (("iLQR_forwardRollout", ms["iLQR_computeCost+forwardRollout"]), ("iLQR_linearization", ms["iLQR_linearization"]),
                         ("iLQR_costQuadratics", ms["iLQR_costQuadratics"]), ("iLQR_backwardPass", ms["iLQR_backwardPass"] + ms["iLQR_backwardPass_retry"]),
                         ("iLQR_lineSearch", ms["iLQR_lineSearch"] + ms["iLQR_lineSearch_retry"])):
            self.prof.setdefault(key, []).append(float(val))

    def _bounds_window(self, step):
        """While the solver handle has a bounds track of either kind (BatchedILQR.set_al_bounds_track, set_al_task_bounds_track), the bounds
        windows of the solve at loop step `step`, beside its reference windows: one kernel, nothing uploaded.  `track_starts` feeds the
        tracks' shared start rows too, once per pair of tracks."""
        track_rows = getattr(self.s, "al_bounds_track_rows", None)      # (a solver stand-in without bounds tracks has none)
        task_rows = getattr(self.s, "al_task_bounds_track_rows", None)
        rows = (track_rows() if track_rows else 0, task_rows() if task_rows else 0)
        if not any(rows):
            self.bounds_starts_for = None
            return
        if self.bounds_starts_for != rows and self.track_starts_given:
            self.s.set_al_bounds_track_starts(self.track_starts)
        self.bounds_starts_for = rows
        self.s.al_bounds_window_from_track(step)

    def step_once(self, x_measured, u_init=None, kick=None):
        t0 = time.perf_counter()
        prob = self.refs.problem_at(self.t_idx, self.s.N, self.base, follow_schedule=self.follow_schedule)   # extractReferenceWindow
        self.s.set_problem(prob)
        self._bounds_window(self.t_idx)
        t1 = time.perf_counter(); self._add("MPC_extractReference", t0, t1)
        self.last_stance0 = prob["stance"][0, 0]
        if self.has_prev and self.since_solve == 1:
            self.s.initialize_warm_resident(x_measured)       # ilqr.cpp:68-80
        elif self.has_prev:
            self.s.initialize_warm_resident(x_measured, shift=self.since_solve)
        else:
            self.s.initialize(x_measured, u_init)            # cold start, ilqr.cpp:82-116
        t2 = time.perf_counter(); self._add("MPC_warmStart", t1, t2)
        self.last_cost = self.s.solve(x_measured)
        t3 = time.perf_counter(); self._add("MPC_iLQR_solve", t2, t3)
        if self.profile_stages:
            self._add_stage_ms()
        if kick is not None:                                  # a push between measurement and actuation (see run)
            x_measured = np.array(x_measured, dtype=np.float64); x_measured[:, NQ:] += kick
        self.last_x_applied = x_measured
        u = self.s.compute_control(x_measured)                # mpc.cpp:97-101
        t4 = time.perf_counter(); self._add("MPC_computeControl", t3, t4)
        self.has_prev = True
        self.since_solve = 1
        self.t_idx += 1
        if self.logs:
            ms = 1e3 * (time.perf_counter() - t0)
            xb, ub = self.s.xbar(), self.s.ubar()
            for b, lg in self.logs.items():
                lg.log(self.t_idx, self.last_cost[b], ms, x_measured[b], u[b], prob["x_ref"][0, 0], prob["u_ref"][0, 0], xb[b, 0], ub[b, 0])
            self._group = (prob, ms, xb, ub)
        elif self.solve_every > 1:
            self._group = (prob, 0.0, None, None)
        self._add("MPC_stepOnce", t0, time.perf_counter())
        return u

    def follow_once(self, x_measured, kick=None):
        """A plant interval WITHOUT a solve (solve_every > 1): the control of knot j = since_solve of the last solve's policy."""
        t3 = time.perf_counter()
        j = self.since_solve
        prob, ms, xb, ub = self._group
        self.last_stance0 = prob["stance"][0, j]
        if kick is not None:
            x_measured = np.array(x_measured, dtype=np.float64); x_measured[:, NQ:] += kick
        self.last_x_applied = x_measured
        u = self.s.compute_control(x_measured, knot=j)
        self._add("MPC_computeControl", t3, time.perf_counter())
        self.since_solve += 1
        self.t_idx += 1
        for b, lg in self.logs.items():
            lg.log(self.t_idx, self.last_cost[b], ms, x_measured[b], u[b], prob["x_ref"][0, j], prob["u_ref"][0, j], xb[b, j], ub[b, j])
        return u

    def run(self, x0, steps, u_init=None, kicks=None):
        """`steps` closed-loop steps from x0 [B,51]; returns the visited states [steps+1,B,51] and controls [steps,B,19].
        kicks: {step index: dv [B,25]} velocity kicks; the state recorded for such a step is the kicked one (what the control law saw)."""
        kicks = {} if kicks is None else {int(k): np.asarray(v, dtype=np.float64) for k, v in kicks.items()}
        if self.resident:
            return self._run_resident(np.array(x0, dtype=np.float64), steps, u_init, kicks)
        x = np.array(x0, dtype=np.float64)
        xs, us = [x.copy()], []
        for k in range(steps):
            kick = kicks.get(k)
            if k % self.solve_every == 0:                # (groups count from the start of the run)
                u = self.step_once(x, u_init, kick=kick)
            else:
                u = self.follow_once(x, kick=kick)
            if kick is not None:
                x = self.last_x_applied; xs[-1] = x.copy()
            if self.plant_contacts == "geometry":
                x, st = self.s.step_geometry(x, u)
                self.plant_stance.append(st)
            elif getattr(self.s, "contact_mode", 0):    # contact row: the plant holds the feet in stance now
                st = np.asarray(self.last_stance0).reshape(-1)
                x = self.s.step_stance(x, u, int(st[0]), int(st[1]))
            else:
                x = self.s.step(x, u)
            xs.append(x.copy()); us.append(u.copy())
        return np.array(xs), np.array(us)

    def _run_resident(self, x0, steps, u_init, kicks):
        """The same loop with the plant in the handle: nothing of the state crosses the host between the cold start and the end of the run.
        One difference from the host path besides the crossings: with a per-rollout contact schedule (`follow_schedule` windows stacked per
        rollout) the resident plant steps every rollout with row 0 of ITS OWN set, as ilqr_hip_plant_configure documents; the host path
        steps the whole batch with row 0 of set 0 (`last_stance0`).  With a shared schedule, which `problem_at` produces, the two agree."""
        s, m = self.s, self.solve_every
        off = sorted(k for k in kicks if k % m != 0)
        if off:
            raise ValueError("resident plant: a kick is supported before the first interval of a group only (solve_every = %d, kicks at %s)" % (m, off))
        if self.plant_model is not None:
            s.plant_set_model(*self.plant_model)             # (in front of plant_configure: the stance source is checked against the plant's mode)
        s.plant_configure(self.substeps, self.feedback_mode, self.plant_contacts)
        if self.plant_params is not None:
            s.plant_set_params(self.plant_params)
        if self.plant_wrench is not None:
            s.plant_set_wrench(self.plant_wrench)
        if self.plant_payload is not None:
            s.plant_set_payload(self.plant_payload)
        if self.plant_observation is not None:
            s.plant_set_observation(self.plant_observation, seed=self.observation_seed, stream0=self.observation_stream0)
        if self.plant_actuator is not None:
            s.plant_set_actuator(self.plant_actuator, seed=self.actuator_seed, stream0=self.actuator_stream0)
        if self.plant_joints is not None:
            s.plant_set_joints(self.plant_joints)
        if self.plant_terrain is not None:
            s.plant_set_terrain(self.plant_terrain)
        s.plant_set_history(steps if self.history_rows is None else self.history_rows)
        if self.score_args is not None:
            s.plant_set_score(**self.score_args)             # (empties the record: it covers this run)
        if self.task_score_tol is not None:
            s.plant_set_task_score(self.task_score_tol)      # (the same)
        s.plant_reset(x0)                                    # the only upload of a state (besides the cold start's x0)
        if self.device_refs and not self.track_ready:        # once: weights and gravity, the track, the start rows
            s.set_problem_constants(self.base)
            s.set_reference_track(self.refs)
            s.set_track_starts(self.track_starts)
            self.track_ready = True
        start_of = lambda b: int(self.track_starts[b if len(self.track_starts) > 1 else 0])
        rows = []                                            # per plant interval: (cost, ms, x_ref_j, u_ref_j, x_opt_j, u_opt_j)
        win_log = None
        if self.starts > 1:                                  # solve groups: the perturbation, and one row of winners per solve on the device
            import torch
            s.set_groups(self.starts)
            s.group_set_perturbation(self.start_sigma, hold=self.start_hold, seed=self.start_seed)
            win_log = torch.zeros(((steps + m - 1) // m, s.num_groups()), dtype=torch.int32, device="cuda:%d" % getattr(s, "device", 0))
            torch.cuda.synchronize()                         # (torch's stream is not the handle's: the zeros are there before the first copy)
        for k in range(0, steps, m):
            cnt = min(m, steps - k)                          # plant intervals of this group
            t0 = time.perf_counter()
            t_solve = self.t_idx
            if self.device_refs:
                s.window_from_track(t_solve, self.follow_schedule)       # enqueued: nothing uploaded, no synchronisation
            else:
                prob = self.refs.problem_at(t_solve, s.N, self.base, follow_schedule=self.follow_schedule)
                s.set_problem(prob)
            self._bounds_window(t_solve)
            t1 = time.perf_counter(); self._add("MPC_extractReference", t0, t1)
            if self.device_refs:
                r0 = start_of(0) + t_solve if self.follow_schedule else 0
                self.last_stance0 = np.array([1 if self.refs.is_stance(e, r0) else 0 for e in range(2)], dtype=np.int32)
            else:
                self.last_stance0 = prob["stance"][0, 0]
            if self.has_prev:
                if self.since_solve == 1:
                    s.initialize_warm_from_plant()           # ilqr.cpp:68-80, x0 from the plant on the device
                else:
                    s.initialize_warm_from_plant(shift=self.since_solve)
                if win_log is not None:
                    s.group_perturb()
                t2 = time.perf_counter(); self._add("MPC_warmStart", t1, t2)
                self.last_cost = s.solve(None)
            else:                                            # the gravity-compensation guess is computed on the host from x0
                xm = x0 if self.plant_observation is None else s.plant_get_observed()      # (the measurement of interval 0: the plant was reset to x0)
                s.initialize(xm, u_init)
                if win_log is not None:
                    s.group_perturb()
                t2 = time.perf_counter(); self._add("MPC_warmStart", t1, t2)
                self.last_cost = s.solve(xm)
            if win_log is not None:                          # enqueued behind the solve: the winner's solution drives every plant of its group
                s.group_select()
                s.group_adopt()
                s.group_copy_winners_device(win_log[k // m].data_ptr())
            t3 = time.perf_counter(); self._add("MPC_iLQR_solve", t2, t3)
            if self.profile_stages:
                self._add_stage_ms()
            if k in kicks:
                s.plant_kick(kicks[k])
            if m == 1:
                s.plant_advance()                            # mpc.cpp:97-101 + main:162-170, enqueued behind the solve
            else:
                s.plant_follow(0, cnt)                       # the same over the knots 0 .. cnt - 1 of the policy, one kernel
            t4 = time.perf_counter(); self._add("MPC_plantAdvance", t3, t4)
            self.has_prev = True
            self.since_solve = cnt
            self.t_idx += cnt
            if self.logs:
                xb, ub = s.xbar(), s.ubar()
                ms = 1e3 * (time.perf_counter() - t0)
                if self.device_refs:                         # the host's copy of the rule, for the logged rollouts only
                    logged = list(self.logs)
                    lp = self.refs.problem_at_starts([start_of(b) for b in logged], t_solve, s.N, self.base, follow_schedule=self.follow_schedule)
                for j in range(cnt):
                    if self.device_refs:
                        xr, ur = ({b: lp[key][i, j].copy() for i, b in enumerate(logged)} for key in ("x_ref", "u_ref"))
                    else:
                        xr, ur = prob["x_ref"][0, j].copy(), prob["u_ref"][0, j].copy()
                    rows.append((self.last_cost.copy(), ms, xr, ur, xb[:, j].copy(), ub[:, j].copy()))
            self._add("MPC_stepOnce", t0, time.perf_counter())
        hx, hu = s.plant_history()                           # ONE download for the whole run
        if win_log is not None:
            self.winners = win_log.cpu().numpy()             # (behind plant_history's synchronisation of the handle's stream)
        xs = np.concatenate([hx, s.plant_state()[None]], axis=0)
        t_first = self.t_idx - steps
        gone = steps - len(hx)                               # intervals a ring of history_rows < steps has overwritten: not logged
        for k, (cost, ms, xr0, ur0, xo0, uo0) in enumerate(rows):
            for b, lg in self.logs.items():
                if k >= gone:
                    lg.log(t_first + k + 1, cost[b], ms, hx[k - gone, b], hu[k - gone, b], xr0[b] if isinstance(xr0, dict) else xr0, ur0[b] if isinstance(ur0, dict) else ur0,
                           xo0[b], uo0[b])
        return xs, hu

    def score(self):
        """The closed-loop score record [B, 8] of the last `run` (columns solver.PLANT_SCORE_TERMS); needs MPCRunner(..., score=...)."""
        if self.score_args is None:
            raise ValueError("no score was asked for (MPCRunner(..., resident=True, score={...}))")
        return self.s.plant_score()

    def task_score(self):
        """The task score record [B, 8] of the last `run` (columns solver.PLANT_TASK_SCORE_TERMS); needs MPCRunner(..., task_score=tol)."""
        if self.task_score_tol is None:
            raise ValueError("no task score was asked for (MPCRunner(..., resident=True, task_score=tol))")
        return self.s.plant_task_score()

    def close(self):
        for lg in self.logs.values():
            lg.close()
