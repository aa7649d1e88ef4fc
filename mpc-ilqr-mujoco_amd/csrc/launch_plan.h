// Which kernel runs each stage, and what follows from that choice -- resolved in ONE place from the kernel-family switches of a handle
// (Variants: the environment, read_variants), its contact mode, its joint-limit option and its Jacobian mode.  Host-only C++17 without a
// HIP include: the launchers (ilqr_kernels.hip) switch on a LaunchPlan's fields, the C ABI (ilqr_capi.hip) resolves one per call
// (plan_of) and reads its capabilities; neither tests a switch itself.  Nothing is cached: resolve_plan is a few comparisons.
#pragma once

namespace ilqr {

// kernel variants (ILQR_DYN / ILQR_ROLLOUT / ILQR_LS / ILQR_BACKWARD / ILQR_LINT): read from the environment ONCE per handle
// (ilqr_hip_create; read_variants, ilqr_kernels.hip, where every switch is described) and kept there.
// backward: 0 four-wave MFMA, 1 LDS + VALU, 2 one wave per rollout; fold: 0 never, 1 the folded kernel on the standard layout, 2 the
// operand-layout kernel
struct Variants {
  int scalar_dyn, rollout_split, ls_split, backward, fold, lin_one_knot;
};

// The CONTACT / CK / KIND template argument of the two-lane kernels (dyn_step_shared.h step_any).  The numbers are part of kernel names,
// documents and test names: they stay.
enum StepKind {
  STEP_FREE = 0,            // constraint-free
  STEP_STANCE = 1,          // stance rows (contact modes 1-3)
  STEP_KINETIC = 2,         // stance rows with kinetic friction on sliding feet (contact mode 4)
  STEP_STANCE_LIMITS = 3,   // as 1, with joint-limit rows
  STEP_KINETIC_LIMITS = 4,  // as 2, with joint-limit rows
  STEP_LIMITS = 5           // joint-limit rows on the constraint-free plant
};
constexpr int step_kind_of(int contact, int limits) {
  return (contact == 0 && limits == 0) ? STEP_FREE : (contact == 0 ? STEP_LIMITS : (contact == 4 ? STEP_KINETIC : STEP_STANCE) + (limits ? 2 : 0));
}

// (the values of DynFamily are what a handle remembers of the kernel that rolled its cold start out: LaunchPlan::rollout)
enum DynFamily { DYN_ONE_LANE = 0, DYN_TWO_LANE = 1, DYN_SCALAR = 2 };      // dyn_kernels.hip _r / dyn_split_kernels.hip _s / the scalar scratch-resident cross-check
enum LinKernel {
  LIN_ANALYTIC_TWO_KNOT,    // primal dump + k_lin_tangent2 / k_lin_tangent2c
  LIN_ANALYTIC_ONE_KNOT,    // primal dump + k_lin_tangent / k_lin_tangent_c (ILQR_LINT=1)
  LIN_FD_TWO_LANE,          // forward differences on the two-lane step (any contact mode)
  LIN_FD_SCALAR             // forward differences on the scalar step
};
enum BackwardKernel {
  BWD_PACK,                 // one wave per rollout on the operand layout (riccati_pack.hip)
  BWD_WAVE_GENERIC,         // one wave per rollout, standard layout, no fold (riccati_wave.hip)
  BWD_WAVE_FOLDED,          // the same with the hinge-position rows folded (ILQR_BACKWARD=wave-fold)
  BWD_FOUR_WAVE,            // riccati_mfma.hip (ILQR_BACKWARD=wg)
  BWD_VALU                  // LDS + VALU cross-check (ILQR_BACKWARD=valu)
};
// what the kernel reads of lxx: 0 whole matrices, 1 the tiles I >= J of the knots t < N, 2 the operand layout of riccati_pack.h
constexpr int lxx_layout_of(BackwardKernel k) { return k == BWD_PACK ? 2 : (k == BWD_WAVE_GENERIC || k == BWD_WAVE_FOLDED) ? 1 : 0; }

struct LaunchPlan {
  // ---- dynamics stages
  DynFamily rollout;        // nominal rollout (launch_rollout)
  DynFamily line_search;    // launch_line_search
  DynFamily step;           // single step and last knot of the warm start; launch_step goes to the two-lane kernel whenever it is given st_out,
                            // launch_warm_tail has no scalar kernel and re-rolls by the default family's under DYN_SCALAR
  int step_kind;            // StepKind of the two-lane kernels
  // ---- linearisation
  LinKernel lin;
  DynFamily primal_dump;    // analytic modes: one lane or two lanes per knot (under ILQR_DYN=s the one-lane dump feeds the free tangent kernel)
  bool lin_contact_tangent; // analytic modes: the contact tangent kernels instead of the free ones
  int lin_friction;         // contact tangent: 0 sticking feet only, 1 / 2 the Coulomb-limit branch of contact mode 3 / 4
  bool limits;              // joint-limit rows in the tangent kernels
  bool lin_stance_prepass;  // stance source GEOMETRY: the nominal knots' stance is decided first -- if ProblemDev::stance_geom is on and
                            // launch_linearize is given its scratch buffer
  // ---- backward pass
  BackwardKernel backward_foldable, backward_plain;      // on Jacobians whose hinge-position rows are e_k + h * the hinge-velocity rows (the
                                                         // analytic tangent kernels write those) / on any others: launch_backward's fold_h says which
  bool folds_h;             // this plan's own linearisation leaves foldable Jacobians AND the backward kernel uses that: fold_h = folds_h * h
  BackwardKernel backward() const { return folds_h ? backward_foldable : backward_plain; }      // inside a solve
  bool pack;                // inside a solve the producers write A_t, B_t, lxx~_t in the operand layout (backward() == BWD_PACK)
  int lxx_layout;           // what the cost quadratics of a solve must leave: lxx_layout_of(backward())
  // ---- capabilities
  bool ls_costs_per_knot;   // the line search leaves per-knot costs behind and k_control sums them
  bool spec_dual;           // both speculative orders can be enqueued side by side (list-driven two-lane line search, one-wave backward)
  bool lin_lists;           // the linearisation takes work lists (linearisation cache, early continuation)
  bool reroll_aside;        // the re-rollout of an accepted candidate reproduces it bit for bit: it may run beside the linearisation
  bool cold_start_aside;    // ... in iteration 0 as well, if the nominal trajectory is a cold start by LaunchPlan::rollout
  bool weight_sets;         // per-rollout cost weights: in the cost kernels of the default family only
  bool stance_geometry;     // stance from the foot hulls
  bool cone_and_limits;     // contact modes 3 / 4 and joint-limit rows
  bool analytic_full;       // the analytic Jacobians carry the Coulomb-limit branch and the joint-limit rows
};

inline LaunchPlan resolve_plan(const Variants& V, int contact, int limits, int jac_mode) {
  const bool constrained = contact != 0 || limits != 0, scalar = V.scalar_dyn != 0;
  LaunchPlan p{};
  // contact mode and joint-limit rows run on the two-lane kernels (the one-lane register kernels are constraint-free only)
  p.rollout = scalar ? DYN_SCALAR : (V.rollout_split || constrained) ? DYN_TWO_LANE : DYN_ONE_LANE;
  p.line_search = scalar ? DYN_SCALAR : (V.ls_split || constrained) ? DYN_TWO_LANE : DYN_ONE_LANE;
  p.step = scalar ? DYN_SCALAR : constrained ? DYN_TWO_LANE : DYN_ONE_LANE;
  p.step_kind = step_kind_of(contact, limits);
  // the scalar family's analytic kernels are constraint-free only: in contact it differentiates its own step
  const bool analytic = jac_mode == 0 && (!scalar || contact == 0);
  p.lin = analytic ? (V.lin_one_knot ? LIN_ANALYTIC_ONE_KNOT : LIN_ANALYTIC_TWO_KNOT) : (scalar ? LIN_FD_SCALAR : LIN_FD_TWO_LANE);
  p.primal_dump = scalar ? DYN_ONE_LANE : p.rollout;
  p.lin_contact_tangent = analytic && contact != 0;
  p.lin_friction = contact == 3 ? 1 : contact == 4 ? 2 : 0;
  p.limits = limits != 0;
  p.lin_stance_prepass = jac_mode == 0 && !scalar && contact != 0;
  p.backward_plain = V.backward == 1 ? BWD_VALU : V.backward == 2 ? BWD_WAVE_GENERIC : BWD_FOUR_WAVE;
  p.backward_foldable = V.backward != 2 ? p.backward_plain : V.fold == 2 ? BWD_PACK : V.fold == 1 ? BWD_WAVE_FOLDED : BWD_WAVE_GENERIC;
  p.folds_h = analytic && V.fold != 0 && V.backward == 2;
  p.pack = p.backward() == BWD_PACK;
  p.lxx_layout = lxx_layout_of(p.backward());
  p.ls_costs_per_knot = p.line_search == DYN_TWO_LANE;
  p.spec_dual = p.line_search == DYN_TWO_LANE && V.backward == 2;
  p.lin_lists = analytic;
  // (by the switches, under ILQR_DYN=s too, where both stages are the scalar kernels whatever they say)
  p.reroll_aside = constrained || V.ls_split == V.rollout_split;
  p.cold_start_aside = p.reroll_aside && !scalar;
  p.weight_sets = !scalar && V.rollout_split && V.ls_split;
  p.stance_geometry = !scalar;
  p.cone_and_limits = !scalar;
  p.analytic_full = !scalar && !V.lin_one_knot;
  return p;
}

// The cross-check families -- scalar dynamics, one-lane rollout / line search, the VALU / four-wave / folded Riccati kernels, the one-knot
// tangent kernels -- are compiled into the test library only (legacy_build: -DILQR_LEGACY_KERNELS); the product library holds the default
// family alone.
inline bool plan_supported(const Variants& V, bool legacy_build) {
  return legacy_build || (!V.scalar_dyn && V.rollout_split && V.ls_split && V.backward == 2 && V.fold != 1 && !V.lin_one_knot);
}

}  // namespace ilqr
