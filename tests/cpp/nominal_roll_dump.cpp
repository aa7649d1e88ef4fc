// Prints nominal_roll / splits_next (csrc/solve_order.h) for tests/test_nominal_roll_cpu.py: one text line per combination of
// reuse_rollout, overlap_rollout, first_aside, can_split, L.reroll_aside, L.cold_start_aside and iter in {0, 1, 2} of a solve of 3 iterations:
//   reuse overlap first_aside can_split reroll_aside cold_start_aside iter rolls_aside nominal_roll splits_next
// The SolveOrder is filled field by field: the two functions read nothing else of it (resolve_solve_order copies the three switches
// from the settings, tests/test_solve_order_cpu.py).
#include <cstdio>

#include "solve_order.h"

using namespace ilqr;

int main() {
  std::printf("reuse overlap first_aside can_split reroll_aside cold_start_aside iter rolls_aside nominal_roll splits_next\n");
  for (int bits = 0; bits < 64; ++bits) for (int iter = 0; iter < 3; ++iter) {
    SolveOrder o{};
    o.reuse_rollout = bits & 1; o.overlap_rollout = bits & 2; o.first_aside = bits & 4; o.can_split = bits & 8;
    LaunchPlan L{};
    L.reroll_aside = bits & 16; L.cold_start_aside = bits & 32;
    std::printf("%d %d %d %d %d %d %d %d %d %d\n", (int)o.reuse_rollout, (int)o.overlap_rollout, (int)o.first_aside, (int)o.can_split, (int)L.reroll_aside, (int)L.cold_start_aside, iter,
                (int)rolls_aside(o, L, iter), (int)nominal_roll(o, L, iter), (int)splits_next(o, L, iter, 3));
  }
  return 0;
}
