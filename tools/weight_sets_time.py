#!/usr/bin/env python3
"""Milliseconds per call of the two cost stages (stage_cost_quadratics: k_quad_kin + k_cost_quadratics; stage_total_cost:
k_traj_knot_cost + k_traj_cost_sum) under shared weights, a one-set table and a B-set table whose sets all hold the shared values,
on one GPU, the three alternating:
   python tools/weight_sets_time.py [--batch 4096] [--horizon 25] [--calls 20] [--rounds 5] [--lib PATH --shared-only]
Each sample is the wall time of `calls` back-to-back stage calls (every call synchronises the handle's stream) divided by `calls`;
medians over the rounds are reported and no threshold is applied.  --lib PATH --shared-only times the shared path of another build of
the library (a parent commit's, which has no weight sets): that figure, not this build's own, is what the tables are compared with.
Prints one JSON line; not part of bench.py."""
import argparse, ctypes as C, importlib.util, json, os, sys, time
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
    ap.add_argument("--batch", type=int, default=4096); ap.add_argument("--horizon", type=int, default=25)
    ap.add_argument("--calls", type=int, default=20); ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib", default=None); ap.add_argument("--shared-only", action="store_true")
    a = ap.parse_args()
    pkg = load_package()
    from mpc_ilqr_mujoco_amd import solver as sv
    sc = pkg.scenario
    B, N = a.batch, a.horizon
    prob = sc.make_problem(sv.reference_kinematics, N=N)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), prob["gravity"]))
    s = sv.BatchedILQR(B, N=N, dt=prob["dt"], lib_path=a.lib)
    # (the shared setters and the references directly: set_problem asks the library for its table, which another build may not have)
    dp = C.POINTER(C.c_double)
    keep = [np.ascontiguousarray(prob[k], dtype=np.float64) for k in ("Q", "R", "Qf")]
    s._chk(s.L.ilqr_hip_set_cost_weights(s.h, *[k.ctypes.data_as(dp) for k in keep]))
    s._chk(s.L.ilqr_hip_set_task_weights(s.h, *[C.c_double(float(v)) for v in prob["task_weights"]]))
    s._chk(s.L.ilqr_hip_set_constraint_weights(s.h, C.c_double(prob["w_joint"]), C.c_double(prob["w_ctrl"])))
    st = np.ascontiguousarray(prob["stance"], dtype=np.int32)
    s._chk(s.L.ilqr_hip_set_contact_schedule(s.h, st.ctypes.data_as(C.POINTER(C.c_int)), 1))
    ee, cv = np.ascontiguousarray(prob["ee_ref"]), np.ascontiguousarray(prob["com_vel_ref"])
    s._chk(s.L.ilqr_hip_set_ee_references(s.h, ee.ctypes.data_as(dp), cv.ctypes.data_as(dp), 1))
    s.set_references(prob["x_ref"], prob["u_ref"], prob["com_ref"])
    s.initialize(x0, ui)
    one = (prob["Q"][None], prob["R"][None], prob["Qf"][None], np.array([prob["task_weights"]], dtype=np.float64), np.array([[prob["w_joint"], prob["w_ctrl"]]], dtype=np.float64))
    modes = ["shared"] if a.shared_only else ["shared", "one_set", "b_sets"]
    ms = {m: {"quadratics": [], "total_cost": []} for m in modes}
    for rnd in range(a.rounds + 1):                      # round 0 warms up
        for m in modes:
            if m == "shared":
                if not a.shared_only:
                    s.clear_weight_sets()
            elif m == "one_set":
                s.set_weight_sets(*one)
            else:
                s.set_weight_sets(*[np.repeat(x, B, axis=0) for x in one])
            for stage, fn in (("quadratics", s.stage_cost_quadratics), ("total_cost", s.stage_total_cost)):
                fn()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                if rnd:
                    ms[m][stage].append(1e3 * (time.perf_counter() - t0) / a.calls)
    s.close()
    print(json.dumps({"tool": "weight_sets_time", "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "calls": a.calls, "rounds": a.rounds, "library": a.lib or sv.LIB_PATH,
                      "ms_per_call_median": {m: {k: float(np.median(v)) for k, v in d.items()} for m, d in ms.items()}, "samples": ms}))


if __name__ == "__main__":
    main()
