// Where the augmented-Lagrangian limit terms take their bounds from and which instantiation of the cost kernels reads them -- resolved in
// ONE place from what a handle has installed.  Host-only C++17 without a HIP include, as launch_plan.h and plant_plan.h: the C ABI
// (ilqr_capi.hip al_point_bounds) resolves a plan, does the work it names and writes the pointers it names; the launchers ask al_variant for
// the same variant from those pointers and switch on it.  Nothing is cached: resolve_al_plan is a few comparisons.
//
// The rules.  Augmented Lagrangian off: the plain penalties, no bounds.  On, no window installed: the joint / torque family reads its table;
// without one the model's ranges at the installed margin, formed in the kernels (a null pointer) -- or, while a state family is installed,
// ONE record of those same doubles (h1host::al_default_bounds): the state instantiations take every bound from a record, there is no
// AL_MODEL_STATE.  The state family reads its table.  A window of either family installed: both families read windows, a family that has none
// gets its record (the table's, or the model's) repeated over the knots, so that two per-knot instantiations serve every combination; those
// live in the per-knot module (ilqr_kernels.h AlKnotModule).  One set serves every rollout through a set stride of 0.  A window of the task
// family (the last function below) counts as a window installed.
#pragma once

namespace h1 {
// The AL template axis of the cost kernels (values fixed: they are part of the kernels' names).  AL_OFF: the plain penalties.  AL_MODEL the
// model's ranges at ProblemDev::al_margin, AL_TABLE rollout b's record of ProblemDev::alb, AL_TABLE_STATE: AL_TABLE with the state family
// (ProblemDev::als, alsb) on top.  AL_KNOT_TABLE / AL_KNOT_TABLE_STATE: the bounds of knot t taken from row t of rollout b's window
// (ProblemDev::alb_knot, alsb_knot); there is no mixed one.
enum { AL_OFF = 0, AL_MODEL = 1, AL_TABLE = 2, AL_TABLE_STATE = 3, AL_KNOT_TABLE = 4, AL_KNOT_TABLE_STATE = 5 };
}  // namespace h1

namespace ilqr {

enum AlSource {
  AL_SRC_NONE = 0,          // the family is not installed
  AL_SRC_MODEL_RANGES,      // null pointer: the model's ranges at the margin, formed in the kernels (joint / torque family only)
  AL_SRC_MODEL_RECORD,      // the one model record at the installed margin
  AL_SRC_TABLE,             // the installed table
  AL_SRC_WINDOW,            // the installed window
  AL_SRC_TABLE_EXPANDED,    // the window buffer, filled from the table
  AL_SRC_MODEL_EXPANDED     // the window buffer, filled from the model record
};
// what a family has installed: sets 0 = nothing, else the records (1 or B) of its table or, with `window`, of its window
struct AlInstalled { int sets; bool window; };
struct AlFamilyPlan {
  AlSource source;
  bool shared;              // set stride 0: one record / window serves every rollout
  bool per_knot;            // knot stride set: the pointer is a window
};
struct AlPlan {
  int variant;              // h1::AL_*
  AlFamilyPlan jc, st;      // joint / torque family, state family
  bool upload_model;        // the model record has to be formed and uploaded
  bool expand_jc, expand_st;   // the family's record has to be repeated over the knots of its window buffer
  bool module;              // the per-knot module is called into
};

// the variant from what a launcher holds: ProblemDev::al, alb, alsb, alb_knot (AlDev: store, bounds, sbounds, bounds_knot) as booleans
constexpr int al_variant(bool al, bool alb, bool alsb, bool alb_knot) {
  return !al ? h1::AL_OFF : (alb && alb_knot) ? (alsb ? h1::AL_KNOT_TABLE_STATE : h1::AL_KNOT_TABLE) : (alb && alsb) ? h1::AL_TABLE_STATE : alb ? h1::AL_TABLE : h1::AL_MODEL;
}

// other_window: a family that is not one of the two has a window installed (the task family, below)
inline AlPlan resolve_al_plan_beside(bool on, AlInstalled jc, AlInstalled st, bool other_window) {
  AlPlan p{};
  p.jc.shared = p.st.shared = true;      // (a family without a pointer has no stride)
  if (!on) return p;        // (AL_OFF, AL_SRC_NONE and no work are the zeros)
  const bool state = st.sets > 0, knot = (jc.sets > 0 && jc.window) || (state && st.window) || other_window;
  p.module = knot;
  p.jc.source = (jc.sets > 0 && jc.window) ? AL_SRC_WINDOW : jc.sets > 0 ? (knot ? AL_SRC_TABLE_EXPANDED : AL_SRC_TABLE)
              : knot ? AL_SRC_MODEL_EXPANDED : state ? AL_SRC_MODEL_RECORD : AL_SRC_MODEL_RANGES;
  p.jc.shared = jc.sets <= 1;
  p.jc.per_knot = knot;
  if (state) p.st = {st.window ? AL_SRC_WINDOW : knot ? AL_SRC_TABLE_EXPANDED : AL_SRC_TABLE, st.sets == 1, knot};
  p.upload_model = p.jc.source == AL_SRC_MODEL_RECORD || p.jc.source == AL_SRC_MODEL_EXPANDED;
  p.expand_jc = p.jc.source == AL_SRC_TABLE_EXPANDED || p.jc.source == AL_SRC_MODEL_EXPANDED;
  p.expand_st = p.st.source == AL_SRC_TABLE_EXPANDED;
  p.variant = al_variant(true, p.jc.source != AL_SRC_MODEL_RANGES, state, knot);
  return p;
}
inline AlPlan resolve_al_plan(bool on, AlInstalled jc, AlInstalled st) { return resolve_al_plan_beside(on, jc, st, false); }

// The task family (ilqr_hip_set_al_task_bounds: bounds on the CoM and the ankle origins, al_task_dev.h) on top.  Its bounds are always a window,
// so installing it counts as "a window is installed": the other two families then read windows through the expansions above and the per-knot
// module is called into.  An axis of its own, orthogonal to the variant: `task` selects the task instantiations of the two per-knot variants
// (the launchers read it off ProblemDev::altb / AlDev::tbounds).  Without a task window the base is resolve_al_plan(on, jc, st) field for field.
struct AlTaskPlan {
  AlPlan base;
  AlFamilyPlan tk;          // source AL_SRC_WINDOW or AL_SRC_NONE
  bool task;
};
inline AlTaskPlan resolve_al_plan(bool on, AlInstalled jc, AlInstalled st, AlInstalled tk) {
  const bool task = on && tk.sets > 0;
  AlTaskPlan p{resolve_al_plan_beside(on, jc, st, task), {AL_SRC_NONE, true, false}, task};
  if (task) p.tk = {AL_SRC_WINDOW, tk.sets == 1, true};
  return p;
}

}  // namespace ilqr
