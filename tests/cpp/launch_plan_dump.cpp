// Prints resolve_plan / plan_supported (csrc/launch_plan.h) over every combination of the kernel-family switches, contact mode,
// joint-limit option and Jacobian mode: one line of name=value tokens per combination (tests/test_launch_plan_cpu.py).
#include <cstdio>

#include "launch_plan.h"

int main() {
  using namespace ilqr;
  for (int scalar = 0; scalar < 2; ++scalar) for (int rs = 0; rs < 2; ++rs) for (int ls = 0; ls < 2; ++ls)
  for (int bw = 0; bw < 3; ++bw) for (int fold = 0; fold < 3; ++fold) for (int one = 0; one < 2; ++one)
  for (int contact = 0; contact < 5; ++contact) for (int limits = 0; limits < 2; ++limits) for (int jac = 0; jac < 2; ++jac) {
    const Variants V{scalar, rs, ls, bw, fold, one};
    const LaunchPlan p = resolve_plan(V, contact, limits, jac);
    std::printf("scalar_dyn=%d rollout_split=%d ls_split=%d backward=%d fold=%d lin_one_knot=%d contact=%d limits=%d jac_mode=%d", scalar, rs, ls, bw, fold, one, contact, limits, jac);
    std::printf(" p.rollout=%d p.line_search=%d p.step=%d p.step_kind=%d", p.rollout, p.line_search, p.step, p.step_kind);
    std::printf(" p.lin=%d p.primal_dump=%d p.lin_contact_tangent=%d p.lin_friction=%d p.limits=%d p.lin_stance_prepass=%d", p.lin, p.primal_dump, p.lin_contact_tangent, p.lin_friction, p.limits,
                p.lin_stance_prepass);
    std::printf(" p.backward_foldable=%d p.backward_plain=%d p.folds_h=%d p.backward=%d p.pack=%d p.lxx_layout=%d", p.backward_foldable, p.backward_plain, p.folds_h, p.backward(), p.pack, p.lxx_layout);
    std::printf(" p.ls_costs_per_knot=%d p.spec_dual=%d p.lin_lists=%d p.reroll_aside=%d p.cold_start_aside=%d", p.ls_costs_per_knot, p.spec_dual, p.lin_lists, p.reroll_aside, p.cold_start_aside);
    std::printf(" p.weight_sets=%d p.stance_geometry=%d p.cone_and_limits=%d p.analytic_full=%d", p.weight_sets, p.stance_geometry, p.cone_and_limits, p.analytic_full);
    std::printf(" supported=%d supported_legacy=%d\n", plan_supported(V, false), plan_supported(V, true));
  }
  return 0;
}
