// Prints resolve_plant_plan (csrc/plant_plan.h) over every combination of installed tables, joints_nominal and follow: one line of
// name=value tokens per combination (tests/test_plant_plan_cpu.py).
#include <cstdio>

#include "plant_plan.h"

int main() {
  using namespace ilqr;
  for (int params = 0; params < 2; ++params) for (int wrench = 0; wrench < 2; ++wrench) for (int payload = 0; payload < 2; ++payload)
  for (int obs = 0; obs < 2; ++obs) for (int act = 0; act < 2; ++act) for (int joints = 0; joints < 2; ++joints)
  for (int nominal = 0; nominal < 2; ++nominal) for (int follow = 0; follow < 2; ++follow) {
    const PlantTables t{params != 0, wrench != 0, payload != 0, obs != 0, act != 0, joints != 0, nominal != 0};
    const PlantPlan p = resolve_plant_plan(t, follow != 0);
    std::printf("params=%d wrench=%d payload=%d observation=%d actuator=%d joints=%d joints_nominal=%d follow=%d", params, wrench, payload, obs, act, joints, nominal, follow);
    std::printf(" p.family=%d p.modules=%u p.draw_observation=%d p.draw_actuator=%d p.self_params=%d p.pass_joints=%d\n", (int)p.family, p.modules, p.draw_observation, p.draw_actuator, p.self_params, p.pass_joints);
  }
  return 0;
}
