// Prints resolve_al_plan (csrc/al_plan.h) over every combination of the augmented Lagrangian on / off and, per family, {nothing, table of 1,
// table of B, window of 1, window of B}: one line of name=value tokens per combination (tests/test_al_plan_cpu.py).  launcher= is al_variant
// fed the pointer-nullness the plan's sources imply.
#include <cstdio>

#include "al_plan.h"

int main() {
  using namespace ilqr;
  const int B = 3;
  const AlInstalled inst[5] = {{0, false}, {1, false}, {B, false}, {1, true}, {B, true}};
  for (int on = 0; on < 2; ++on) for (int jc = 0; jc < 5; ++jc) for (int st = 0; st < 5; ++st) {
    const AlPlan p = resolve_al_plan(on != 0, inst[jc], inst[st]);
    const bool alb = p.jc.source != AL_SRC_NONE && p.jc.source != AL_SRC_MODEL_RANGES, alsb = p.st.source != AL_SRC_NONE;
    std::printf("on=%d jc=%d st=%d", on, jc, st);
    std::printf(" p.variant=%d p.jc.source=%d p.jc.shared=%d p.jc.per_knot=%d p.st.source=%d p.st.shared=%d p.st.per_knot=%d", p.variant, (int)p.jc.source, p.jc.shared, p.jc.per_knot,
                (int)p.st.source, p.st.shared, p.st.per_knot);
    std::printf(" p.upload_model=%d p.expand_jc=%d p.expand_st=%d p.module=%d launcher=%d\n", p.upload_model, p.expand_jc, p.expand_st, p.module, al_variant(on != 0, alb, alsb, p.jc.per_knot));
  }
  return 0;
}
