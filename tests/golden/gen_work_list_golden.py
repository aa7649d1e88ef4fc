#!/usr/bin/env python3
"""work_list_traces.npz: what the CPU oracle (tests/oracle_lib.py) decides in the batches of tests/work_list_cases.py -- per case, solve and
rollout the iteration count, the cost, alpha and lambda traces and the final lambda.  The alpha traces fix the lists of the linearisation
cache and of the first-pass skip in every iteration (work_list_cases.predicted_counts); a GPU test compares its device traces and its two
counters with them without solving on the CPU.

standing40 (three k_control workgroups): three solves on one handle, a convergence-exit solve, and three warm-started chains of three MPC
steps (shift 1, shift 2, shift 1 with a disturbed plant) with the states the chains visit; `tie_free` says that all of that keeps every
accept decision of all 40 rollouts when x0 is scaled by (1 +- 1e-9).

Mode cases (B = 24, two workgroups): the first seed in 0..15 whose traces hold an iteration >= 1 with both listed and skipped rollouts and a
list with entries from both workgroups -- here a seed is taken only if one iteration is both --, and whose two checked rollouts (the first
of either workgroup) are tie-free.  A case without such a seed is left out, and printed.

   python tests/golden/gen_work_list_golden.py          (about three minutes on eight cores; needs the built library and oracle)
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import work_list_cases as wl      # noqa: E402


def put(out, case, runs):
    for run, rec in runs.items():
        for k, v in rec.items():
            out["%s/%s/%s" % (case, run, k)] = v


def main():
    out = {}
    t0 = time.time()
    case = wl.standing40()
    res = wl.pool_map(lambda b: wl.standing_runs(case, b), range(case.B))
    runs = wl.stack([r[0] for r in res])
    put(out, case.name, runs)
    for chain in wl.CHAINS:
        out["%s/%s_x" % (case.name, chain)] = np.array([r[1][chain] for r in res]).transpose(1, 0, 2)      # [step, rollout, 51]
    for run in wl.STANDING_RUNS:
        a, it = runs[run]["alpha"], runs[run]["it"]
        print("standing40 %-8s lists %s, iterations %d..%d" % (run, wl.predicted_counts(a, it, run == "exit")[4], it.min(), it.max()))
    a, it = runs["fixed0"]["alpha"], runs["fixed0"]["it"]
    print("standing40 iteration 5 per workgroup", wl.per_group(a, it, 5), "mixed / spread", wl.occurrence(a, it), "%.0f s" % (time.time() - t0))
    free = wl.pool_map(lambda b: wl.tie_free(case, b, res[b][0]), range(case.B))
    print("standing40 tie-free rollouts: %d of %d  %.0f s" % (sum(free), case.B, time.time() - t0))
    out["standing40/tie_free"] = np.array(all(free))

    left_out = []
    for name in wl.MODE_CASES:
        for seed in wl.SEEDS:
            case = wl.mode_case(name, seed)
            res = wl.pool_map(lambda b: wl.mode_runs(case, b)[0], range(case.B))
            runs = wl.stack(res)
            a, it = runs["fixed0"]["alpha"], runs["fixed0"]["it"]
            mixed, spread = wl.occurrence(a, it)
            lists = wl.predicted_counts(a, it, False)[4]
            ok = any(i in spread for i in mixed)
            free = ok and all(wl.pool_map(lambda b: wl.tie_free(case, b, res[b]), (0, wl.GROUP)))
            print("%-12s seed %2d: lists %s, mixed %s, spread %s, tie-free %s  %.0f s" % (name, seed, lists, mixed, spread, free, time.time() - t0))
            if ok and free:
                put(out, name, runs)
                out[name + "/seed"] = np.array(seed)
                break
        else:
            left_out.append(name)
    print("left out:", left_out)
    np.savez_compressed(wl.FIXTURE, **out)
    print("wrote %s: %d bytes" % (wl.FIXTURE, os.path.getsize(wl.FIXTURE)))


if __name__ == "__main__":
    main()
