"""One solve in one of the launch orders of csrc/solve_order.h, on the smallest batch at which the order occurs (the standing40 case of
tests/work_list_cases.py, thresholds lowered through the environment as the GPU tests do), for a kernel trace:

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/solve_order_trace.py CONFIG
  python3 tools/solve_order_trace.py CONFIG report
  python3 tools/launch_summary.py DIR/.../*_kernel_trace.csv

CONFIG: listed (fixed iterations, the listed pair from iteration 1 on), twin (B <= ILQR_SPEC_MAX), exit_gate (convergence exit with the gate,
twin -> dual -> sequential), exit_split (convergence exit with the default early-continuation split), slices (two slices with stagger).
A second argument `report` prints the orders and counters the handle reports (a run of its own, not traced)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIGS = dict(
    listed=(dict(ILQR_SPEC_MAX="0", ILQR_SPLIT="0", ILQR_SPEC_LIST_FROM="1", ILQR_SPEC_LIST_MAX="30"), False, 40),
    twin=(dict(), False, 40),
    exit_gate=(dict(ILQR_SPEC="1", ILQR_SPEC_MAX="6", ILQR_SPLIT="0"), True, 40),
    exit_split=(dict(ILQR_SPEC="0"), True, 40),
    slices=(dict(ILQR_SLICES="2", ILQR_SPEC="0", ILQR_SPLIT="0"), False, 128),
)


def main():
    envs, early_exit, B = CONFIGS[sys.argv[1]]
    os.environ.update(envs)
    import __graft_entry__ as ge
    ge._load_package()
    import test_gpu_work_lists as twl
    import work_list_cases as wl
    case = wl.standing40()
    tile = np.arange(B) % 40
    s = twl.open_handle(case, twl.DEFAULTS, early_exit=early_exit, tile=tile)
    s.initialize(case.x0[tile], case.ui[tile])
    cost = s.solve(case.x0[tile])
    if sys.argv[2:] == ["report"]:      # (not under a trace: the getters read the lists back, which shows as copy kernels behind the solve)
        print(sys.argv[1], "slices", s.num_slices(), "orders", s.iteration_orders(), "first_pass", s.first_pass_rollouts(), "retry_pass", s.retry_pass_rollouts(),
              "linearized", s.linearized_rollouts(), "listed", s.listed_spec_iterations(), "cost sum %.17g" % float(np.sum(cost)))
    s.close()


if __name__ == "__main__":
    main()
