#!/usr/bin/env python3
"""Milliseconds per closed-loop step of mpc_loop.MPCRunner with the plant on the host path (resident=False: four host crossings per MPC
step) against the device-resident plant (resident=True), on one GPU, alternating:
   python tools/closed_loop_time.py [--batch 4096] [--horizon 25] [--iters 10] [--steps 6] [--rounds 3] [--substeps 1] [--feedback-mode 0] [--solve-every 1] [--score]
Ten fixed iterations per solve (no convergence exit), standing scenario.  --substeps / --feedback-mode configure the resident plant only
(the host path has neither: its figure stays the one-step, held-control loop).  --solve-every M goes to both runners: a solve before every
M-th plant interval, the policy followed in between; the timed run is lengthened to the next multiple of M intervals (whole groups), and
the figures stay milliseconds per PLANT interval.  --score installs the closed-loop score on the resident runner (the problem's own Q, R and
unit weights on the four scalar terms; the two score kernels then run behind every plant call).  Prints one JSON line; not part of bench.py."""
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
    a = ap.parse_args()
    pkg = load_package()
    from mpc_ilqr_mujoco_amd import mpc_loop as ml, references as rf, solver as sv
    sc = pkg.scenario
    B, N = a.batch, a.horizon
    a.steps = -(-a.steps // a.solve_every) * a.solve_every      # whole groups
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


if __name__ == "__main__":
    main()
