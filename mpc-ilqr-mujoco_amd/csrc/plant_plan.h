// Which kernel family a plant call (ilqr_hip_plant_advance / ilqr_hip_plant_follow) launches, which modules it calls into and which draws
// run in front of it -- resolved in ONE place from the tables a handle has installed.  Host-only C++17 without a HIP include, as
// launch_plan.h: the C ABI (ilqr_capi.hip) resolves one per call, loads every module of PlantPlan::modules and switches on the family;
// neither the entry points nor enqueue_plant test a table themselves.  Nothing is cached: resolve_plant_plan is a few comparisons.
#pragma once

namespace ilqr {

// Each family from PARAMS on is the superset of the one before it (every table below its own may be absent), so the family is decided by
// the highest table installed.  WRENCH .. TERRAIN live in modules of their own (csrc/Makefile), ADVANCE .. PARAMS in the library.
enum PlantFamily {
  PLANT_ADVANCE = 0,        // k_plant_advance: no table, one interval
  PLANT_FOLLOW,             // k_plant_follow: no table, several intervals
  PLANT_PARAMS,             // k_plant_follow_p
  PLANT_WRENCH,             // k_plant_follow_w
  PLANT_PAYLOAD,            // k_plant_follow_m
  PLANT_OBSERVE,            // k_plant_follow_o behind the draw of the call's error rows
  PLANT_ACTUATOR,           // k_plant_follow_a behind the draw of the call's normals
  PLANT_JOINTS,             // k_plant_follow_j
  PLANT_TERRAIN             // k_plant_follow_t
};
// the modules, in the order of their families; a bit of PlantPlan::modules each
enum PlantModule { MOD_WRENCH = 0, MOD_PAYLOAD, MOD_OBSERVE, MOD_ACTUATOR, MOD_JOINTS, MOD_TERRAIN, PLANT_MODULES };

// which tables are installed; joints_nominal: the joint table holds the model's own joints in every record -- such a table is no table
// (terrain is the last member: an initialiser that names the seven above leaves it false)
struct PlantTables { bool params, wrench, payload, observation, actuator, joints, joints_nominal, terrain; };
struct PlantPlan {
  PlantFamily family;
  unsigned modules;         // bit PlantModule of every module the call calls into
  bool draw_observation;    // the observation module's draw runs in front of the family's kernel
  bool draw_actuator;       // the actuator module's draw does
  bool self_params;         // the kernels read the handle's own parameter record (plant_self_params): a module family without a parameter table
  bool pass_joints;         // the kernel is handed the joint table: installed and not all-nominal (only the joints family and above read it)
};

inline PlantPlan resolve_plant_plan(const PlantTables& t, bool follow) {
  PlantPlan p{};
  p.pass_joints = t.joints && !t.joints_nominal;
  p.family = t.terrain ? PLANT_TERRAIN : p.pass_joints ? PLANT_JOINTS : t.actuator ? PLANT_ACTUATOR : t.observation ? PLANT_OBSERVE : t.payload ? PLANT_PAYLOAD
           : t.wrench ? PLANT_WRENCH : t.params ? PLANT_PARAMS : follow ? PLANT_FOLLOW : PLANT_ADVANCE;
  p.draw_observation = t.observation && p.family >= PLANT_OBSERVE;
  p.draw_actuator = t.actuator && p.family >= PLANT_ACTUATOR;
  if (p.family >= PLANT_WRENCH) p.modules |= 1u << (p.family - PLANT_WRENCH);
  if (p.draw_observation) p.modules |= 1u << MOD_OBSERVE;
  if (p.draw_actuator) p.modules |= 1u << MOD_ACTUATOR;
  // (an all-nominal joint table counts here: the record is uploaded although no family reads it)
  p.self_params = (t.wrench || t.payload || t.observation || t.actuator || t.joints || t.terrain) && !t.params;
  return p;
}

}  // namespace ilqr
