"""Rollouts that enter the lambda-retry pass, per iteration, in the fixed-iteration headline mode (from the solve traces), and how many of
them are saturated repeats -- retries at the lambda cap, which the solve skips by default (ilqr_hip_set_dedup_saturated_retry)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge
pkg = ge._load_package()
from mpc_ilqr_mujoco_amd import solver as sv
sc = pkg.scenario
B, N = 4096, 25
prob = sc.make_problem(sv.reference_kinematics, N=N)
ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
x0, ui = sc.synthetic_batch(B, N, 0, ug)
s = sv.BatchedILQR(B, N=N); s.set_problem(prob); s.set_options(early_exit=False)
for step in range(2):      # (bench.py solves on one handle again and again: lambda survives a solve)
    s.initialize(x0, ui)
    lam = s.lambdas()      # regularisation at the start of iteration 0
    s.solve(x0)
    tc, ta, tl = s.trace()
    print("solve %d: %d rollouts enter at the lambda cap; retry passes executed %d, first passes %d of %d" % (step + 1, (lam == 1e-3).sum(), s.retry_pass_rollouts(), s.first_pass_rollouts(), B * ta.shape[1]))
    # the launch order the device took per iteration, and the lists the iteration started from (listed side-by-side order: chg = accepted in
    # the previous iteration -- first pass on the solve's buffers, retry speculated into the twin --, kr = known retries)
    orders = s.iteration_orders()
    print("         listed side by side in %d iterations: %s" % (s.listed_spec_iterations(), " ".join(sv.BatchedILQR.ORDER_NAMES[o] for o in orders)))
    for i in range(ta.shape[1]):
        used = tl[:, i]
        retried = (ta[:, i] == 0.0) | (used != lam)
        saturated = (ta[:, i] == 0.0) & (lam == 1e-3)
        chg, kr = s.iteration_lists(i)
        side = i < len(orders) and orders[i] == 4
        print("iteration %d: first search failed for %4d rollouts (both passes failed: %4d), %4d of them at the lambda cap: retry list %4d; chg %4d kr %4d%s"
              % (i, retried.sum(), (ta[:, i] == 0.0).sum(), saturated.sum(), (retried & ~saturated).sum(), len(chg), len(kr),
                 "  SIDE BY SIDE: %d retries speculated, %d slots" % (len(chg), 2 * len(chg) + len(kr)) if side else ""))
        lam = np.where(ta[:, i] > 0.0, np.maximum(used / 2.0, 1e-6), used)
