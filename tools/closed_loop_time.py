#!/usr/bin/env python3
"""Milliseconds per closed-loop step of mpc_loop.MPCRunner with the plant on the host path (resident=False: four host crossings per MPC
step) against the device-resident plant (resident=True), on one GPU, alternating:
   python tools/closed_loop_time.py [--batch 4096] [--horizon 25] [--iters 10] [--steps 6] [--rounds 3] [--substeps 1] [--feedback-mode 0] [--solve-every 1] [--score]
Ten fixed iterations per solve (no convergence exit), standing scenario.  --substeps / --feedback-mode configure the resident plant only
(the host path has neither: its figure stays the one-step, held-control loop).  --solve-every M goes to both runners: a solve before every
M-th plant interval, the policy followed in between; the timed run is lengthened to the next multiple of M intervals (whole groups), and
the figures stay milliseconds per PLANT interval.  --score installs the closed-loop score on the resident runner (the problem's own Q, R and
unit weights on the four scalar terms; the two score kernels then run behind every plant call).  Prints one JSON line; not part of bench.py.

   python tools/closed_loop_time.py --device-refs [--per-rollout-starts] [--contact-mode 2] ...
compares, instead, two ways of giving the RESIDENT runner a moving reference, alternating on one box: (a) the windows of every step cut
on the host (ReferenceData.problem_at_starts) and uploaded through the three reference setters, (b) the windows cut on the device from a
track uploaded once (MPCRunner(device_refs=True)).  The track is the 200 walking rows of tests/golden/refdata_golden.npz prepared as
scenario.walking_batch prepares them, on the advancing schedule; one shared start of 0, or with --per-rollout-starts one start per
rollout drawn so that start + steps + horizon < 200.  Also reports the time the host spends in MPC_extractReference per step on either
path and the duration of the window kernel alone (events on the handle's stream around 50 launches) beside the bytes it writes.

   python tools/closed_loop_time.py --plant-params {shared,per-rollout} [--solve-every M] ...
compares, instead, the RESIDENT runner without a plant parameter table against the same runner with one installed
(MPCRunner(plant_params=...): one set for all rollouts, or one per rollout with friction, softness, gravity and torque gain spread over the
batch), alternating on one box, and times the plant kernel alone -- events on the handle's stream around 50 back-to-back plant_advance
calls under one solve -- for the free plant and for plant contact mode 2 (ilqr_hip_plant_set_model), with and without the table.

   python tools/closed_loop_time.py --wrench [--contact-mode 2] [--solve-every M] ...
compares, instead, the RESIDENT runner without a wrench table against the same runner with one installed (MPCRunner(plant_wrench=...): a
lateral push of 20 to 60 N per rollout, at the pelvis inertial offset, over the whole run), alternating on one box, the plant in the
given contact mode.

   python tools/closed_loop_time.py --payload [--contact-mode 2] [--solve-every M] ...
compares, instead, the RESIDENT runner without a payload table against the same runner with one installed (MPCRunner(plant_payload=...): a
rigid payload of 0 to 20 kg per rollout at the fixed offset (-0.1, 0, 0.3) in the pelvis frame, a backpack at torso height, over the whole
run), alternating on one box, the plant in the given contact mode.

   python tools/closed_loop_time.py --observation [--contact-mode 0] [--solve-every M] ...
compares, instead, the RESIDENT runner without an observation table against the same runner with one installed
(MPCRunner(plant_observation=...): per rollout a pelvis position bias of up to 1 cm, 2 mrad of joint encoder noise and 0.05 rad/s of gyro
noise), alternating on one box, the plant in the given contact mode.

   python tools/closed_loop_time.py --actuator [--contact-mode 0] [--solve-every M] ...
compares, instead, the RESIDENT runner without an actuator table against the same runner with one installed (MPCRunner(plant_actuator=...):
per rollout a delay of 0 to 2 plant substeps, a lag of 5 to 20 ms and 0.5 N m of torque noise per joint), alternating on one box, the plant
in the given contact mode; then the plant call alone, events around 50 back-to-back advances.

   python tools/closed_loop_time.py --joints [--contact-mode 0] [--solve-every M] ...
compares, instead, the RESIDENT runner without a joint table against the same runner with one installed (MPCRunner(plant_joints=...): per
rollout and joint a gain of 0.8 to 1, a range scale of 0.7 to 1, a damping of 0.5 to 2 and an armature of 0.05 to 0.2), alternating on one
box, the plant in the given contact mode; then the plant call alone, events around 50 back-to-back advances: without a table, under the
actuator table of --actuator alone (the family the joints family widens) and under the joint table alone.

   python tools/closed_loop_time.py --terrain [--contact-mode 2] ...
times the plant call alone, events around 50 back-to-back advances, three repetitions from the same plant state, the plant in the given
contact mode (2, 3 or 4): without a table and under the joint table of --joints with the schedule as the contact source, the same two with
the plant's own feet as the source, and under a terrain table alone (MPCRunner's plant_terrain: per rollout a floor of -2 to 2 cm under
each foot from interval 1 on) -- which needs that source.  A library without the terrain entry points (ILQR_HIP_LIB naming an older build)
times the first four: run the tool under both libraries in turn to compare the families on one box."""
import argparse, importlib.util, json, os, sys, time
import numpy as np
import torch      # first HIP runtime of the process (as tests/conftest.py): behind the product library, torch finds "no HIP GPUs" when it is asked for the device name
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_package():
    name, path = "mpc_ilqr_mujoco_amd", os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096); ap.add_argument("--horizon", type=int, default=25); ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=6); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--substeps", type=int, default=1); ap.add_argument("--feedback-mode", type=int, default=0, choices=(0, 1))
    ap.add_argument("--solve-every", type=int, default=1); ap.add_argument("--score", action="store_true")
    ap.add_argument("--plant-params", choices=("shared", "per-rollout"), default=None)
    ap.add_argument("--wrench", action="store_true")
    ap.add_argument("--payload", action="store_true")
    ap.add_argument("--observation", action="store_true")
    ap.add_argument("--actuator", action="store_true")
    ap.add_argument("--joints", action="store_true")
    ap.add_argument("--terrain", action="store_true")
    ap.add_argument("--device-refs", action="store_true"); ap.add_argument("--per-rollout-starts", action="store_true"); ap.add_argument("--contact-mode", type=int, default=2)
    a = ap.parse_args()
    if a.per_rollout_starts and not a.device_refs:
        ap.error("--per-rollout-starts needs --device-refs")
    pkg = load_package()
    from mpc_ilqr_mujoco_amd import mpc_loop as ml, references as rf, solver as sv
    sc = pkg.scenario
    B, N = a.batch, a.horizon
    a.steps = -(-a.steps // a.solve_every) * a.solve_every      # whole groups
    if a.device_refs:
        return device_refs_main(a, sc, ml, rf, sv)
    if a.plant_params:
        return plant_params_main(a, sc, ml, rf, sv)
    if a.wrench:
        return wrench_main(a, sc, ml, rf, sv)
    if a.payload:
        return payload_main(a, sc, ml, rf, sv)
    if a.observation:
        return observation_main(a, sc, ml, rf, sv)
    if a.actuator:
        return actuator_main(a, sc, ml, rf, sv)
    if a.joints:
        return joints_main(a, sc, ml, rf, sv)
    if a.terrain:
        return terrain_main(a, sc, ml, rf, sv)
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rows = a.steps + N + 10
    rd.set_states(np.tile(sc.standing_state(), (rows, 1))); rd.contact = np.ones((rows, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    score = dict(Q=base["Q"], R=base["R"], upright=1.0, balance=1.0, joint_limits=1.0, control_limits=1.0) if a.score else None
    ms = {False: [], True: []}
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for resident in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
            run = ml.MPCRunner(s, rd, base, resident=resident, substeps=a.substeps if resident else 1, feedback_mode=a.feedback_mode if resident else 0,
                                   solve_every=a.solve_every, score=score if resident else None)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)              # (ends with the downloads of the run: the history ring, or the last plant step)
            dt = time.perf_counter() - t0
            s.close()
            if rnd:
                ms[resident].append(1e3 * dt / a.steps)
    print(json.dumps({"tool": "closed_loop_time", "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "iterations": a.iters, "steps": a.steps,
                      "resident_substeps": a.substeps, "resident_feedback_mode": a.feedback_mode, "solve_every": a.solve_every, "score": bool(a.score),
                      "ms_per_step_host_plant": float(np.median(ms[False])), "ms_per_step_resident_plant": float(np.median(ms[True])),
                      "samples_host": ms[False], "samples_resident": ms[True]}))


def plant_params_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rows = a.steps + N + 10
    rd.set_states(np.tile(sc.standing_state(), (rows, 1))); rd.contact = np.ones((rows, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    rng = np.random.default_rng(1)
    if a.plant_params == "shared":
        table = sc.stack_plant_params(1, friction=0.7, softness=2e-5, torque_gain=0.9)
    else:
        table = sc.stack_plant_params(B, gravity=np.array([0.0, 0.0, -9.81]) + rng.uniform(-0.3, 0.3, (B, 3)), friction=rng.uniform(0.3, 1.0, B),
                                      softness=rng.uniform(1e-5, 1e-4, B), limit_stiffness=rng.uniform(0.0, 625.0, B), torque_gain=rng.uniform(0.8, 1.0, B))
    ms = {False: [], True: []}
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for tab in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
            run = ml.MPCRunner(s, rd, base, resident=True, substeps=a.substeps, feedback_mode=a.feedback_mode, solve_every=a.solve_every, plant_params=table if tab else None)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)
            dt = time.perf_counter() - t0
            s.close()
            if rnd:
                ms[tab].append(1e3 * dt / a.steps)
    # the plant kernel alone: 50 back-to-back advances under one solve, three repetitions from the same plant state
    kernel_us, alive = {}, {}
    for mode in (0, 2):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
        s.set_problem(base); s.initialize(x0, ui); s.solve(x0)
        s.plant_set_model(mode, None); s.plant_configure(a.substeps, a.feedback_mode, "schedule")
        st = torch.cuda.ExternalStream(s.stream)
        for tab in (False, True):
            if tab:
                s.plant_set_params(table)
            us = []
            for rep_ in range(4):                        # (the first repetition warms up)
                s.plant_reset(x0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(50):
                    s.plant_advance()
                e1.record(st); e1.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 50)
            key = "mode%d_%s" % (mode, "table" if tab else "no_table")
            kernel_us[key], alive[key] = us[1:], int(s.plant_alive().sum())
        s.close()
    print(json.dumps({"tool": "closed_loop_time", "mode": "plant_params", "plant_params": a.plant_params, "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N,
                      "iterations": a.iters, "steps": a.steps, "substeps": a.substeps, "feedback_mode": a.feedback_mode, "solve_every": a.solve_every,
                      "ms_per_step_resident_plant": float(np.median(ms[False])), "ms_per_step_resident_plant_with_table": float(np.median(ms[True])),
                      "samples_no_table": ms[False], "samples_table": ms[True],
                      "plant_kernel_us": {k: float(np.median(v)) for k, v in kernel_us.items()}, "plant_kernel_samples_us": kernel_us, "alive_after_50_advances": alive}))


def wrench_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rows = a.steps + N + 10
    rd.set_states(np.tile(sc.standing_state(), (rows, 1))); rd.contact = np.ones((rows, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    force = np.zeros((B, 3)); force[:, 1] = np.random.default_rng(1).uniform(20.0, 60.0, B)
    table = sc.stack_plant_wrench(B, force=force, point=sv.pelvis_inertial_offset())
    ms, alive = {False: [], True: []}, {}
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for tab in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
            s.set_contact_mode(a.contact_mode)
            run = ml.MPCRunner(s, rd, base, resident=True, substeps=a.substeps, feedback_mode=a.feedback_mode, solve_every=a.solve_every, plant_wrench=table if tab else None)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)
            dt = time.perf_counter() - t0
            alive[tab] = int(s.plant_alive().sum())
            s.close()
            if rnd:
                ms[tab].append(1e3 * dt / a.steps)
    print(json.dumps({"tool": "closed_loop_time", "mode": "wrench", "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "iterations": a.iters, "steps": a.steps,
                      "substeps": a.substeps, "feedback_mode": a.feedback_mode, "solve_every": a.solve_every, "contact_mode": a.contact_mode,
                      "ms_per_step_resident_plant": float(np.median(ms[False])), "ms_per_step_resident_plant_with_wrench": float(np.median(ms[True])),
                      "samples_no_wrench": ms[False], "samples_wrench": ms[True], "alive_no_wrench": alive[False], "alive_wrench": alive[True]}))


def payload_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rows = a.steps + N + 10
    rd.set_states(np.tile(sc.standing_state(), (rows, 1))); rd.contact = np.ones((rows, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    mass = np.random.default_rng(1).uniform(0.0, 20.0, B)
    table = sc.stack_plant_payload(B, mass, com=(-0.1, 0.0, 0.3), inertia=np.outer(mass / 20.0, (0.4, 0.3, 0.3, 0.0, 0.0, 0.0)))
    ms, alive = {False: [], True: []}, {}
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for tab in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
            s.set_contact_mode(a.contact_mode)
            run = ml.MPCRunner(s, rd, base, resident=True, substeps=a.substeps, feedback_mode=a.feedback_mode, solve_every=a.solve_every, plant_payload=table if tab else None)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)
            dt = time.perf_counter() - t0
            alive[tab] = int(s.plant_alive().sum())
            s.close()
            if rnd:
                ms[tab].append(1e3 * dt / a.steps)
    print(json.dumps({"tool": "closed_loop_time", "mode": "payload", "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "iterations": a.iters, "steps": a.steps,
                      "substeps": a.substeps, "feedback_mode": a.feedback_mode, "solve_every": a.solve_every, "contact_mode": a.contact_mode,
                      "ms_per_step_resident_plant": float(np.median(ms[False])), "ms_per_step_resident_plant_with_payload": float(np.median(ms[True])),
                      "samples_no_payload": ms[False], "samples_payload": ms[True], "alive_no_payload": alive[False], "alive_payload": alive[True]}))


def observation_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rows = a.steps + N + 10
    rd.set_states(np.tile(sc.standing_state(), (rows, 1))); rd.contact = np.ones((rows, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    table = sc.stack_plant_observation(B, position_bias=np.random.default_rng(1).uniform(-0.01, 0.01, (B, 3)), joints_noise=0.002, angular_velocity_noise=0.05)
    ms, alive = {False: [], True: []}, {}
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for tab in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
            s.set_contact_mode(a.contact_mode)
            run = ml.MPCRunner(s, rd, base, resident=True, substeps=a.substeps, feedback_mode=a.feedback_mode, solve_every=a.solve_every, plant_observation=table if tab else None,
                               observation_seed=2024)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)
            dt = time.perf_counter() - t0
            alive[tab] = int(s.plant_alive().sum())
            s.close()
            if rnd:
                ms[tab].append(1e3 * dt / a.steps)
    # the plant call alone (with a table: the draw and the plant kernel): 50 back-to-back advances under one solve, three repetitions from the same plant state
    kernel_us, alive_k = {}, {}
    for mode in (0, 2):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
        s.set_problem(base); s.initialize(x0, ui); s.solve(x0)
        s.plant_set_model(mode, None); s.plant_configure(a.substeps, a.feedback_mode, "schedule")
        st = torch.cuda.ExternalStream(s.stream)
        for tab in (False, True):
            if tab:
                s.plant_set_observation(table, seed=2024)
            us = []
            for rep_ in range(4):                        # (the first repetition warms up)
                s.plant_reset(x0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(50):
                    s.plant_advance()
                e1.record(st); e1.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 50)
            key = "mode%d_%s" % (mode, "table" if tab else "no_table")
            kernel_us[key], alive_k[key] = us[1:], int(s.plant_alive().sum())
        s.close()
    print(json.dumps({"tool": "closed_loop_time", "mode": "observation", "plant_call_us": {k: float(np.median(v)) for k, v in kernel_us.items()}, "plant_call_samples_us": kernel_us,
                      "alive_after_50_advances": alive_k, "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "iterations": a.iters, "steps": a.steps,
                      "substeps": a.substeps, "feedback_mode": a.feedback_mode, "solve_every": a.solve_every, "contact_mode": a.contact_mode,
                      "ms_per_step_resident_plant": float(np.median(ms[False])), "ms_per_step_resident_plant_with_observation": float(np.median(ms[True])),
                      "samples_no_observation": ms[False], "samples_observation": ms[True], "alive_no_observation": alive[False], "alive_observation": alive[True]}))


def actuator_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rows = a.steps + N + 10
    rd.set_states(np.tile(sc.standing_state(), (rows, 1))); rd.contact = np.ones((rows, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    rng = np.random.default_rng(1)
    table = sc.stack_plant_actuator(B, delay=rng.integers(0, 3, B), tau=rng.uniform(0.005, 0.02, (B, 19)), sigma=0.5)
    ms, alive = {False: [], True: []}, {}
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for tab in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
            s.set_contact_mode(a.contact_mode)
            run = ml.MPCRunner(s, rd, base, resident=True, substeps=a.substeps, feedback_mode=a.feedback_mode, solve_every=a.solve_every, plant_actuator=table if tab else None,
                               actuator_seed=2024)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)
            dt = time.perf_counter() - t0
            alive[tab] = int(s.plant_alive().sum())
            s.close()
            if rnd:
                ms[tab].append(1e3 * dt / a.steps)
    # the plant call alone (with a table: the draw and the plant kernel): 50 back-to-back advances under one solve, three repetitions from the same plant state
    kernel_us, alive_k = {}, {}
    for mode in (0, 2):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
        s.set_problem(base); s.initialize(x0, ui); s.solve(x0)
        s.plant_set_model(mode, None); s.plant_configure(a.substeps, a.feedback_mode, "schedule")
        st = torch.cuda.ExternalStream(s.stream)
        for tab in (False, True):
            if tab:
                s.plant_set_actuator(table, seed=2024)
            us = []
            for rep_ in range(4):                        # (the first repetition warms up)
                s.plant_reset(x0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(50):
                    s.plant_advance()
                e1.record(st); e1.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 50)
            key = "mode%d_%s" % (mode, "table" if tab else "no_table")
            kernel_us[key], alive_k[key] = us[1:], int(s.plant_alive().sum())
        s.close()
    print(json.dumps({"tool": "closed_loop_time", "mode": "actuator", "plant_call_us": {k: float(np.median(v)) for k, v in kernel_us.items()}, "plant_call_samples_us": kernel_us,
                      "alive_after_50_advances": alive_k, "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "iterations": a.iters, "steps": a.steps,
                      "substeps": a.substeps, "feedback_mode": a.feedback_mode, "solve_every": a.solve_every, "contact_mode": a.contact_mode,
                      "ms_per_step_resident_plant": float(np.median(ms[False])), "ms_per_step_resident_plant_with_actuator": float(np.median(ms[True])),
                      "samples_no_actuator": ms[False], "samples_actuator": ms[True], "alive_no_actuator": alive[False], "alive_actuator": alive[True]}))


def joints_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rows = a.steps + N + 10
    rd.set_states(np.tile(sc.standing_state(), (rows, 1))); rd.contact = np.ones((rows, 2), dtype=np.int32)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    rng = np.random.default_rng(1)
    table = sc.stack_plant_joints([dict(gain=rng.uniform(0.8, 1.0, 19), range_scale=rng.uniform(0.7, 1.0, 19), damping=rng.uniform(0.5, 2.0, 19), armature=rng.uniform(0.05, 0.2, 19))
                                   for _ in range(B)], B)
    act = sc.stack_plant_actuator(B, delay=rng.integers(0, 3, B), tau=rng.uniform(0.005, 0.02, (B, 19)), sigma=0.5)
    ms, alive = {False: [], True: []}, {}
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for tab in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
            s.set_contact_mode(a.contact_mode)
            run = ml.MPCRunner(s, rd, base, resident=True, substeps=a.substeps, feedback_mode=a.feedback_mode, solve_every=a.solve_every, plant_joints=table if tab else None)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)
            dt = time.perf_counter() - t0
            alive[tab] = int(s.plant_alive().sum())
            s.close()
            if rnd:
                ms[tab].append(1e3 * dt / a.steps)
    # the plant call alone: 50 back-to-back advances under one solve, three repetitions from the same plant state
    kernel_us, alive_k = {}, {}
    for mode in (0, 2):
        s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
        s.set_problem(base); s.initialize(x0, ui); s.solve(x0)
        s.plant_set_model(mode, None); s.plant_configure(a.substeps, a.feedback_mode, "schedule")
        st = torch.cuda.ExternalStream(s.stream)
        for tab in ("no_table", "actuator_table", "joint_table"):
            s.plant_clear_actuator(); s.plant_clear_joints()
            if tab == "actuator_table":
                s.plant_set_actuator(act, seed=2024)
            if tab == "joint_table":
                s.plant_set_joints(table)
            us = []
            for rep_ in range(4):                        # (the first repetition warms up)
                s.plant_reset(x0)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(50):
                    s.plant_advance()
                e1.record(st); e1.synchronize()
                us.append(1e3 * e0.elapsed_time(e1) / 50)
            key = "mode%d_%s" % (mode, tab)
            kernel_us[key], alive_k[key] = us[1:], int(s.plant_alive().sum())
        s.close()
    print(json.dumps({"tool": "closed_loop_time", "mode": "joints", "plant_call_us": {k: float(np.median(v)) for k, v in kernel_us.items()}, "plant_call_samples_us": kernel_us,
                      "alive_after_50_advances": alive_k, "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "iterations": a.iters, "steps": a.steps,
                      "substeps": a.substeps, "feedback_mode": a.feedback_mode, "solve_every": a.solve_every, "contact_mode": a.contact_mode,
                      "ms_per_step_resident_plant": float(np.median(ms[False])), "ms_per_step_resident_plant_with_joints": float(np.median(ms[True])),
                      "samples_no_joints": ms[False], "samples_joints": ms[True], "alive_no_joints": alive[False], "alive_joints": alive[True]}))


def terrain_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    if a.contact_mode not in (2, 3, 4):
        raise SystemExit("--terrain needs --contact-mode 2, 3 or 4")
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), base["gravity"]))
    rng = np.random.default_rng(1)
    joints = sc.stack_plant_joints([dict(gain=rng.uniform(0.8, 1.0, 19), range_scale=rng.uniform(0.7, 1.0, 19), damping=rng.uniform(0.5, 2.0, 19), armature=rng.uniform(0.05, 0.2, 19))
                                    for _ in range(B)], B)
    floors = rng.uniform(-0.02, 0.02, (B, 2))
    terrain = sc.stack_plant_terrain([dict(z_left=floors[b, 0], z_right=floors[b, 1], first=1) for b in range(B)], B)
    has_terrain = hasattr(sv.load_library(), "ilqr_hip_plant_set_terrain")
    kernel_us, alive_k = {}, {}
    s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False)
    s.set_problem(base); s.initialize(x0, ui); s.solve(x0)
    s.plant_set_model(a.contact_mode, None)
    st = torch.cuda.ExternalStream(s.stream)
    cases = [("no_table", "schedule"), ("joint_table", "schedule"), ("no_table", "geometry"), ("joint_table", "geometry")] + ([("terrain_table", "geometry")] if has_terrain else [])
    for tab, source in cases:
        s.plant_clear_joints()
        if has_terrain:
            s.plant_clear_terrain()
        s.plant_configure(a.substeps, a.feedback_mode, source)
        if tab == "joint_table":
            s.plant_set_joints(joints)
        if tab == "terrain_table":
            s.plant_set_terrain(terrain)
        us = []
        for rep_ in range(4):                        # (the first repetition warms up)
            s.plant_reset(x0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(50):
                s.plant_advance()
            e1.record(st); e1.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / 50)
        key = "mode%d_%s_%s" % (a.contact_mode, tab, source)
        kernel_us[key], alive_k[key] = us[1:], int(s.plant_alive().sum())
    s.close()
    print(json.dumps({"tool": "closed_loop_time", "mode": "terrain", "library": sv.LIB_PATH, "plant_call_us": {k: float(np.median(v)) for k, v in kernel_us.items()},
                      "plant_call_samples_us": kernel_us, "alive_after_50_advances": alive_k, "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N,
                      "iterations": a.iters, "substeps": a.substeps, "feedback_mode": a.feedback_mode, "contact_mode": a.contact_mode}))


class HostWindows:
    """the parent's path for per-rollout windows: problem_at for MPCRunner, cut by problem_at_starts on the host"""

    def __init__(self, rd, starts):
        self.rd, self.starts = rd, starts

    def problem_at(self, t0, N, base, follow_schedule=False):
        return self.rd.problem_at_starts(self.starts, t0, N, base, follow_schedule=follow_schedule)


def device_refs_main(a, sc, ml, rf, sv):
    B, N = a.batch, a.horizon
    r = np.load(os.path.join(ROOT, "tests", "golden", "refdata_golden.npz"))
    q_mj = rf.pinocchio_to_mujoco(r["walking_pin_rows"])
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.concatenate([q_mj, rf.differentiate_positions(q_mj, float(r["dt"]))], axis=1)); rd.contact = rf.contact_schedule(q_mj, sv.foot_clearance)
    T = rd.x_ref.shape[0]
    total = 1 + a.steps                                   # the cold step and the timed ones run on one step counter
    if total + N >= T:
        raise SystemExit("steps + horizon must stay below the track's %d rows" % T)
    rng = np.random.default_rng(0)
    starts = rng.integers(0, T - N - total, size=B) if a.per_rollout_starts else np.zeros(1, dtype=np.int64)
    base = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -1.0))
    x0 = rd.x_ref[np.broadcast_to(starts, (B,))].copy()      # scenario.walking_batch's initial states
    x0[:, 7:26] += rng.uniform(-0.02, 0.02, (B, 19)); x0[:, 0:3] += rng.uniform(-0.01, 0.01, (B, 3)); x0[:, 26:] *= 0.5
    ui = np.tile(sv.gravity_compensation(sc.standing_state(), base["gravity"]), (B, N, 1)) + rng.uniform(-0.5, 0.5, (B, N, 19))
    ms, extract = {False: [], True: []}, {False: [], True: []}
    kernel_us = []
    for rnd in range(a.rounds + 1):                      # round 0 warms up (first launches, allocations)
        for dev in (False, True):
            s = sv.BatchedILQR(B, N=N, dt=base["dt"]); s.set_max_iterations(a.iters); s.set_options(early_exit=False); s.set_contact_mode(a.contact_mode)
            kw = dict(follow_schedule=True, resident=True, substeps=a.substeps, feedback_mode=a.feedback_mode, solve_every=a.solve_every)
            run = ml.MPCRunner(s, rd, base, device_refs=True, track_starts=starts, **kw) if dev else ml.MPCRunner(s, HostWindows(rd, starts), base, **kw)
            run.run(x0, 1, u_init=ui)                    # the cold start is not what is compared: every timed step is a warm one
            s.synchronize()
            run.prof.clear()
            t0 = time.perf_counter()
            run.run(x0, a.steps, u_init=ui)
            dt = time.perf_counter() - t0
            if rnd:
                ms[dev].append(1e3 * dt / a.steps); extract[dev].append(float(np.median(run.prof["MPC_extractReference"])))
            if dev and rnd == a.rounds:                  # the kernel alone, on the handle's stream
                st = torch.cuda.ExternalStream(s.stream)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for rep_ in range(3):
                    e0.record(st)
                    for _ in range(50):
                        s.window_from_track(1, True)
                    e1.record(st); e1.synchronize()
                    kernel_us.append(1e3 * e0.elapsed_time(e1) / 50)
            s.close()
    n1, sets = N + 1, len(starts)
    nbytes = sets * ((n1 * 51 + N * 19 + n1 * 3) * 8 + n1 * 9 * 8 + n1 * 2 * 4)
    k_us = float(np.median(kernel_us))
    print(json.dumps({"tool": "closed_loop_time", "mode": "device_refs", "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "iterations": a.iters, "steps": a.steps,
                      "contact_mode": a.contact_mode, "substeps": a.substeps, "solve_every": a.solve_every, "per_rollout_starts": bool(a.per_rollout_starts), "track_rows": int(T),
                      "ms_per_step_host_windows": float(np.median(ms[False])), "ms_per_step_device_windows": float(np.median(ms[True])),
                      "samples_host_windows": ms[False], "samples_device_windows": ms[True],
                      "extract_reference_ms_host_windows": float(np.median(extract[False])), "extract_reference_ms_device_windows": float(np.median(extract[True])),
                      "window_bytes_per_step": int(nbytes), "window_kernel_us": k_us, "window_kernel_samples_us": kernel_us,
                      "window_kernel_fraction_of_6TBps": float(nbytes / (k_us * 1e-6) / 6e12)}))


if __name__ == "__main__":
    main()
