#!/usr/bin/env python3
"""Cost of the augmented-Lagrangian joint and torque limits (ilqr_hip_set_augmented_lagrangian) against the plain penalties on ONE handle,
on one GPU, the two alternating:
   python tools/al_time.py [--batch 4096] [--horizon 25] [--calls 20] [--rounds 5] [--iters 10] [--bounds] [--state] [--knot] [--task] [--task-track [--follow M]]
  * ms per call of the two cost stages (stage_cost_quadratics: k_quad_kin + k_cost_quadratics; stage_total_cost: k_traj_knot_cost +
    k_traj_cost_sum) and, per launch inside a solve, of the cost quadratics (ilqr_hip_get_stage_ms, stage 2);
  * ms per call of the update kernel alone (ilqr_hip_al_update: k_al_update, one memset, one synchronisation);
  * one solve under the plain penalties and one three-round AL solve, fixed iteration count (what bench.py times), cold start each.
Each stage sample is the wall time of `calls` back-to-back calls (every call synchronises the handle's stream) divided by `calls`;
medians over the rounds are reported and no threshold is applied.  Prints one JSON line; not part of bench.py.
--bounds adds two modes to the alternation on the same handle: AL under a one-record table of bounds (ilqr_hip_set_al_bounds, n_sets = 1)
and under a per-rollout table (n_sets = batch).  Both tables hold the bounds the installation has without a table, so the three AL modes
do the same arithmetic on the same values and differ in where the bounds come from.
--state (implies --bounds) adds a fifth mode: the per-rollout table plus a per-rollout table of state bounds (ilqr_hip_set_al_state_bounds,
n_sets = batch; every bound +-1e3, none active) -- the state instantiation of k_cost_quadratics and k_al_state_knot_cost behind
k_traj_knot_cost against the AL_TABLE instantiations of the mode before it.
--knot (implies --state) adds two modes: per-rollout WINDOWS of the same bounds (ilqr_hip_set_al_knot_bounds, n_sets = batch: every knot its own
five lines) against the per-rollout table, and both families as windows (ilqr_hip_set_al_state_knot_bounds) against the two tables -- the per-knot
instantiations of libilqr_hip_alknot.so against the table instantiations, the same arithmetic on the same values.  It also times
ilqr_hip_al_bounds_window_from_track itself (both parts of a track of 2 (N + 1) rows, one start per rollout, `calls` enqueues and one
synchronisation, per call): "window_from_track" in the output.
--task (implies --knot) adds one mode: the per-rollout windows of joint / torque bounds plus a per-rollout window of task bounds
(ilqr_hip_set_al_task_bounds, n_sets = batch; every bound +-1e3 m, none active; the stance schedule is the problem's) -- the task
instantiations of k_quad_kin, k_cost_quadratics and k_al_update and k_al_task_knot_cost against the per-knot instantiations of "al_knot_B".
--task-track (implies --knot; with --cut-only nothing else runs) times the cut once more with a task track of the same rows installed beside the
other two parts (ilqr_hip_set_al_task_bounds_track): "window_from_track_task", with the bytes each cut writes; and a plant_follow of --follow M
intervals (default 1) on the same handle without and with the task score (ilqr_hip_plant_set_task_score), `calls` enqueues and one
synchronisation, alternating: "plant_follow"."""
import argparse, importlib.util, json, os, sys, time
import numpy as np
import torch      # first HIP runtime of the process (as tests/conftest.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_package():
    name, path = "mpc_ilqr_mujoco_amd", os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096); ap.add_argument("--horizon", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bounds", action="store_true", help="also time AL under a one-record and under a per-rollout table of bounds")
    ap.add_argument("--state", action="store_true", help="also time AL under a per-rollout table of bounds plus a per-rollout table of state bounds")
    ap.add_argument("--knot", action="store_true", help="also time AL under per-rollout windows of bounds (per knot), and the track cut")
    ap.add_argument("--task", action="store_true", help="also time AL under per-rollout windows of bounds plus a per-rollout window of task bounds")
    ap.add_argument("--cut-only", action="store_true", help="with --knot: time the track cut alone")
    ap.add_argument("--task-track", action="store_true", help="also time the cut with a task track, and plant_follow without and with the task score")
    ap.add_argument("--follow", type=int, default=1, help="with --task-track: intervals of the timed plant_follow")
    a = ap.parse_args()
    a.knot = a.knot or a.task or a.task_track
    a.state = a.state or a.knot
    a.bounds = a.bounds or a.state
    pkg = load_package()
    from mpc_ilqr_mujoco_amd import solver as sv
    sc = pkg.scenario
    B, N = a.batch, a.horizon
    prob = sc.make_problem(sv.reference_kinematics, N=N)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), prob["gravity"]))
    s = sv.BatchedILQR(B, N=N, dt=prob["dt"]); s.set_problem(prob)
    s.set_options(early_exit=False); s.set_max_iterations(a.iters)
    al = dict(rounds=3, rho_joint0=2 * prob["w_joint"], rho_ctrl0=2 * prob["w_ctrl"], growth=10.0, rho_max_factor=1e4, margin=0.1, tol_joint=0.0, tol_ctrl=0.0)
    modes = ("plain", "al") + (("al_bounds_1", "al_bounds_B") if a.bounds else ()) + (("al_bounds_B_state_B",) if a.state else ()) + (("al_knot_B", "al_knot_B_state_knot_B") if a.knot else ()) + (("al_knot_B_task_B",) if a.task else ())
    ms = {m: {"quadratics": [], "total_cost": [], "solve": [], "quadratics_per_launch_in_solve": []} for m in modes}
    for m in modes[1:]:
        ms[m]["update"] = []
    record = sv.al_default_bounds(al["margin"])
    state_record = np.concatenate([np.full(sv.AL_STATE_COORDS, -1e3), np.full(sv.AL_STATE_COORDS, 1e3)])
    task_row = np.concatenate([np.full(sv.AL_TASK_COORDS, -1e3), np.full(sv.AL_TASK_COORDS, 1e3)])

    def timed(fn, calls):
        fn()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return 1e3 * (time.perf_counter() - t0) / calls

    for rnd in range(0 if a.cut_only else a.rounds + 1):      # round 0 warms up
        for m in modes:
            if m == "plain":
                s.clear_augmented_lagrangian()
            else:
                s.set_augmented_lagrangian(**al)
                if m == "al":
                    s.clear_al_bounds()
                elif m.startswith("al_knot"):
                    s.set_al_knot_bounds(np.tile(record, (B, N + 1, 1)))
                else:
                    s.set_al_bounds(record if m == "al_bounds_1" else np.tile(record, (B, 1)))
                if m == "al_bounds_B_state_B":
                    s.set_al_state_bounds(np.tile(state_record, (B, 1)), 2 * prob["w_joint"], 0.0)
                elif m == "al_knot_B_state_knot_B":
                    s.set_al_state_knot_bounds(np.tile(state_record, (B, N + 1, 1)), 2 * prob["w_joint"], 0.0)
                else:
                    s.clear_al_state_bounds()
                if m == "al_knot_B_task_B":
                    s.set_al_task_bounds(np.tile(task_row, (B, N + 1, 1)), 2 * prob["w_joint"], 0.0)
                else:
                    s.clear_al_task_bounds()
                assert s.num_al_task_bound_sets() == (B if "task" in m else 0)
                assert s.num_al_bound_sets() == (0 if m == "al" else 1 if m == "al_bounds_1" else B)
                assert s.num_al_state_bound_sets() == (B if "state" in m else 0)
                assert s.al_bounds_per_knot() == {"al_knot_B": 1, "al_knot_B_state_knot_B": 3, "al_knot_B_task_B": 1}.get(m, 0)
            s.initialize(x0, ui)
            s.enable_profiling(True)
            t0 = time.perf_counter(); s.solve(None); dt = 1e3 * (time.perf_counter() - t0)
            st, launches = s.stage_ms()
            s.enable_profiling(False)
            row = {"solve": dt, "quadratics_per_launch_in_solve": float(st["iLQR_costQuadratics"] / max(1.0, launches["iLQR_costQuadratics"])),
                   "quadratics": timed(s.stage_cost_quadratics, a.calls), "total_cost": timed(s.stage_total_cost, a.calls)}
            if m != "plain":
                row["update"] = timed(lambda: s.al_update(0), a.calls)
            if rnd:
                for k, v in row.items():
                    ms[m][k].append(v)
    cut = cut_task = follow = None

    def time_cut():
        samples = []
        for rnd in range(a.rounds + 1):
            s.al_bounds_window_from_track(0); s.al_violation()      # (al_violation synchronises the stream and copies [B][2] doubles)
            t0 = time.perf_counter()
            for k in range(a.calls):
                s.al_bounds_window_from_track(k)
            s.al_violation()
            samples.append(1e3 * (time.perf_counter() - t0) / a.calls)
        return samples[1:]

    if a.knot:                                           # the track cut alone: enqueues back to back, one synchronisation
        s.set_augmented_lagrangian(**al)
        s.set_al_state_bounds(state_record, 2 * prob["w_joint"], 0.0)
        s.set_al_bounds_track(np.tile(record, (2 * (N + 1), 1)), np.tile(state_record, (2 * (N + 1), 1)))
        s.set_al_bounds_track_starts(np.arange(B) % (N + 1))
        samples = time_cut()
        # bytes a cut writes: B windows of N + 1 padded rows per part (80 + 64 doubles; the task part adds 32); it reads as many, mostly from cache
        cut = {"ms_median": float(np.median(samples)), "samples": samples, "bytes_written": 8 * B * (N + 1) * (80 + 64)}
    if a.task_track:
        s.set_al_task_bounds(task_row[None, None, :].repeat(N + 1, axis=1), 2 * prob["w_joint"], 0.0)
        s.set_al_task_bounds_track(np.tile(task_row, (2 * (N + 1), 1)))      # (installing it resets the shared starts)
        s.set_al_bounds_track_starts(np.arange(B) % (N + 1))
        samples = time_cut()
        cut_task = {"ms_median": float(np.median(samples)), "samples": samples, "bytes_written": 8 * B * (N + 1) * (80 + 64 + 32)}
        assert s.num_al_task_bound_sets() == B and s.al_bounds_per_knot() == 3
        # plant_follow without and with the task score: the ring row of every interval is read once ([B][51] doubles), with the interval's window
        # and schedule rows ([B][32] doubles, [B][2] ints); term rows [M][B][8] written and read, the record [B][8] read and written
        M = a.follow
        s.clear_al_bounds_track(); s.clear_al_task_bounds_track()
        s.initialize(x0, ui); s.solve(None)
        s.plant_configure(1, 0, "schedule"); s.plant_set_history(M); s.plant_reset(x0)
        rows = {"without": [], "with": []}
        for rnd in range(a.rounds + 1):
            for how in ("without", "with"):
                if how == "with":
                    s.plant_set_task_score(0.0)
                else:
                    s.plant_clear_task_score()
                s.plant_reset(x0)
                s.plant_follow(0, M); s.plant_alive()              # (plant_alive synchronises the stream and copies [B] ints)
                s.plant_reset(x0)
                t0 = time.perf_counter()
                for k in range(a.calls):
                    s.plant_follow(0, M)
                s.plant_alive()
                if rnd:
                    rows[how].append(1e3 * (time.perf_counter() - t0) / a.calls)
        follow = {"intervals": M, "ms_median": {k: float(np.median(v)) for k, v in rows.items()}, "samples": rows,
                  "score_bytes": 8 * B * (M * (51 + 32 + 8 + 8) + 16) + 4 * 2 * B * M}
    s.close()
    print(json.dumps({"tool": "al_time", "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "calls": a.calls, "rounds": a.rounds, "iters": a.iters,
                      "al": al, "window_from_track": cut, "window_from_track_task": cut_task, "plant_follow": follow, "ms_median": {m: {k: float(np.median(v)) if v else None for k, v in d.items()} for m, d in ms.items()}, "samples": ms}))


if __name__ == "__main__":
    main()
