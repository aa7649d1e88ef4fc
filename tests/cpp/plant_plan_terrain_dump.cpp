// Prints resolve_plant_plan (csrc/plant_plan.h) over every combination of the seven installed tables, joints_nominal and follow -- 512
// lines of name=value tokens (tests/test_terrain_cpu.py).  tests/cpp/plant_plan_dump.cpp prints the 256 of them without a terrain table.
#include <cstdio>

#include "plant_plan.h"

int main() {
  using namespace ilqr;
  static_assert(PLANT_TERRAIN == PLANT_JOINTS + 1 && MOD_TERRAIN == MOD_JOINTS + 1 && PLANT_MODULES == MOD_TERRAIN + 1, "the terrain family is the highest");
  for (int terrain = 0; terrain < 2; ++terrain)
  for (int params = 0; params < 2; ++params) for (int wrench = 0; wrench < 2; ++wrench) for (int payload = 0; payload < 2; ++payload)
  for (int obs = 0; obs < 2; ++obs) for (int act = 0; act < 2; ++act) for (int joints = 0; joints < 2; ++joints)
  for (int nominal = 0; nominal < 2; ++nominal) for (int follow = 0; follow < 2; ++follow) {
    PlantTables t{params != 0, wrench != 0, payload != 0, obs != 0, act != 0, joints != 0, nominal != 0};
    t.terrain = terrain != 0;
    const PlantPlan p = resolve_plant_plan(t, follow != 0);
    std::printf("terrain=%d params=%d wrench=%d payload=%d observation=%d actuator=%d joints=%d joints_nominal=%d follow=%d", terrain, params, wrench, payload, obs, act, joints, nominal, follow);
    std::printf(" p.family=%d p.modules=%u p.draw_observation=%d p.draw_actuator=%d p.self_params=%d p.pass_joints=%d\n", (int)p.family, p.modules, p.draw_observation, p.draw_actuator, p.self_params, p.pass_joints);
  }
  return 0;
}
