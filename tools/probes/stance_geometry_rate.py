#!/usr/bin/env python3
"""Iterations per second of the contact leg's batch (bench.py: synthetic standing batch under gravity [0, 0, -9.81], contact mode 2,
analytic Jacobians, fixed iterations) with the stance source SCHEDULE and GEOMETRY (include/ilqr_hip.h ilqr_hip_set_stance_source),
alternated on the same handle and box:
    python tools/probes/stance_geometry_rate.py [B=4096] [N=25] [iters=10] [rounds=3]
Prints one JSON line: the rate of each source (best of the rounds), their ratio, and the stance flags the final nominals hold."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
pkg = ge._load_package()
sc = pkg.scenario
from mpc_ilqr_mujoco_amd import solver as sv
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
N = int(sys.argv[2]) if len(sys.argv) > 2 else 25
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -9.81))
ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
x0, ui = sc.synthetic_batch(B, N, 0, ug)
s = sv.BatchedILQR(B, N=N, dt=prob["dt"]); s.set_problem(prob); s.set_contact_mode(2)
s.set_options(jacobian_mode=sv.JAC_ANALYTIC, early_exit=False); s.set_max_iterations(iters)


def one():
    s.initialize(x0, ui)
    t0 = time.perf_counter(); s.solve(x0); dt = time.perf_counter() - t0
    assert np.all(s.iterations() == iters) and np.all(np.isfinite(s.cost()))
    return B * iters / dt


best = {"schedule": 0.0, "geometry": 0.0}
stance = {}
for src in ("schedule", "geometry"):
    s.set_stance_source(src); one()          # warm-up
for _ in range(rounds):
    for src in ("schedule", "geometry"):
        s.set_stance_source(src)
        best[src] = max(best[src], one())
        stance[src] = s.stance()
s.close()
print(json.dumps({"batch": B, "horizon": N, "iters": iters, "rounds": rounds, "unit": "iterations/s",
                  "schedule": round(best["schedule"], 1), "geometry": round(best["geometry"], 1),
                  "ratio_geometry_to_schedule": round(best["geometry"] / best["schedule"], 4),
                  "geometry_knots_in_stance": float(stance["geometry"].mean()), "schedule_knots_in_stance": float(stance["schedule"].mean())}))
