#!/usr/bin/env python3
"""Milliseconds per call of the three solve-group operations alone (include/ilqr_hip.h ilqr_hip_group_select, ilqr_hip_group_adopt,
ilqr_hip_group_perturb; csrc/group_kernels.hip), on one GPU:
   python tools/group_time.py [--batch 4096] [--horizon 25] [--groups 2,8,32] [--samples 20] [--al]
Each sample is one call between two device events on the handle's stream (the calls only enqueue); the median of --samples is reported
after two warm-up calls per operation and G.  adopt's bytes are computed from the shapes -- per group the winner's slabs are read once and
written to the G - 1 other members (with a winner that is member 0 of no group: the key puts it at member 1) -- and divided by its time.
--al installs the augmented Lagrangian (joint / torque family) so that its multiplier store is among the slabs.  No threshold is applied.
Prints one JSON line; not part of bench.py."""
import argparse, importlib.util, json, os, sys
import numpy as np
import torch      # first HIP runtime of the process (as tests/conftest.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NX, NU = 51, 19


def load_package():
    name, path = "mpc_ilqr_mujoco_amd", os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(name, path, submodule_search_locations=[os.path.dirname(path)])
    mod = importlib.util.module_from_spec(spec); sys.modules[name] = mod; spec.loader.exec_module(mod)
    return mod


def slab_bytes(N, al):
    """bytes of one rollout's solution state: x0, xbar, ubar, K, kff, cost, lambda, iterations (+ the joint / torque multiplier row, violation, done)"""
    b = 8 * (NX + (N + 1) * NX + N * NU + N * NU * NX + N * NU + 1 + 1) + 4
    if al:
        b += 8 * (8 + (N + 1) * 80 + 2) + 4      # (upper estimate of the store's row: header + N + 1 knot records of at most 80 doubles)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096); ap.add_argument("--horizon", type=int, default=25)
    ap.add_argument("--groups", default="2,8,32"); ap.add_argument("--samples", type=int, default=20); ap.add_argument("--al", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("group_time.py needs a GPU: a timing without one says nothing")
    pkg = load_package()
    from mpc_ilqr_mujoco_amd import solver as sv
    sc = pkg.scenario
    B, N = a.batch, a.horizon
    prob = sc.make_problem(sv.reference_kinematics, N=N)
    x0, ui = sc.synthetic_batch(B, N, 0, sv.gravity_compensation(sc.standing_state(), prob["gravity"]))
    s = sv.BatchedILQR(B, N=N, dt=prob["dt"])
    s.set_problem(prob); s.set_max_iterations(1)
    if a.al:
        s.set_augmented_lagrangian(rounds=1, rho_joint0=2 * prob["w_joint"], rho_ctrl0=2 * prob["w_ctrl"])
    s.initialize(x0, ui); s.solve(None)
    stream = torch.cuda.ExternalStream(s.stream, device="cuda:0")

    def timed(fn):
        for _ in range(2):
            fn()
        s.synchronize()
        out = []
        for _ in range(a.samples):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    res = {}
    for G in [int(g) for g in a.groups.split(",")]:
        s.set_groups(G)
        keys = np.ones(B); keys[1::G] = 0.5                                # member 1 wins every group: G - 1 members are written
        kt = torch.tensor(keys, dtype=torch.float64, device="cuda:0"); torch.cuda.synchronize()
        s.group_set_perturbation(sc.stack_group_sigma(G, 1e-3, ladder=np.ones(G - 1)), hold=1, seed=1)
        ms = dict(select=timed(lambda: s.group_select(kt)), adopt=timed(s.group_adopt), perturb=timed(s.group_perturb))
        moved = (B // G) * G * slab_bytes(N, a.al)                          # read once + written G - 1 times, per group
        med = {k: float(np.median(v)) for k, v in ms.items()}
        res[str(G)] = dict(ms_median=med, ms_min={k: float(np.min(v)) for k, v in ms.items()}, ms_max={k: float(np.max(v)) for k, v in ms.items()},
                           adopt_bytes=int(moved), adopt_written_bytes=int((B // G) * (G - 1) * slab_bytes(N, a.al)), adopt_TB_per_s=moved / (med["adopt"] * 1e-3) / 1e12)
    s.close()
    print(json.dumps({"tool": "group_time", "device": torch.cuda.get_device_name(0), "batch": B, "horizon": N, "samples": a.samples, "al": bool(a.al), "groups": res}))


if __name__ == "__main__":
    main()
