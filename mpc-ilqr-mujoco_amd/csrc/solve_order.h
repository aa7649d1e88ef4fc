// In which order the launches of a solve are enqueued -- resolved in ONE place from a handle's effective switches, its sizes, what its
// LaunchPlan can do and which of the optional buffers it holds.  Host-only C++17 without a HIP include, like launch_plan.h: the C ABI
// (ilqr_capi.hip) fills a SolveSettings from the handle (solve_settings), resolves one SolveOrder per enqueue (enqueue_solve) and asks
// iteration_order once per iteration; neither it nor its getters test a switch themselves.  Nothing is cached: every function here is a
// few comparisons.  tests/cpp/solve_order_dump.cpp prints them, tests/test_solve_order_cpu.py restates the rules (nominal_roll and splits_next:
// tests/cpp/nominal_roll_dump.cpp, tests/test_nominal_roll_cpu.py).
#pragma once

#include "launch_plan.h"

namespace ilqr {

// Everything the decisions below read.  The switches are the EFFECTIVE ones: where the environment sets one it overrides the handle's own
// setting (diagnostics, tests) -- ilqr_capi.hip effective() is the one place that rule is written.
struct SolveSettings {
  bool early_exit;          // convergence exit (ilqr_hip_set_options)
  bool early_exit_gate;     // ilqr_hip_set_early_exit_gate / ILQR_EE_GATE
  bool split;               // ILQR_SPLIT, else on with the convergence exit (SolveOrder::can_split)
  bool spec;                // ILQR_SPEC
  bool spec_dual;           // ILQR_SPEC_DUAL
  int spec_max;             // ILQR_SPEC_MAX
  bool spec_lists;          // ILQR_SPEC_LISTS
  bool listed_spec;         // ilqr_hip_set_listed_spec
  int spec_list_max;        // ILQR_SPEC_LIST_MAX
  int spec_list_from;       // ILQR_SPEC_LIST_FROM
  bool dedup;               // ilqr_hip_set_dedup_saturated_retry / ILQR_DEDUP_RETRY
  bool relin;               // ilqr_hip_set_relinearize_unchanged / ILQR_RELIN
  bool repass;              // ilqr_hip_set_repeat_first_pass / ILQR_REPASS=1 (either one is enough)
  bool overlap_rollout;     // ILQR_OVERLAP_ROLLOUT
  bool reuse_rollout;       // not ilqr_hip_set_reroll_nominal / ILQR_REUSE_ROLLOUT (on unless either asks for the re-roll: nominal_roll)
  int max_iter;
  int B;                    // rollouts of the view that is enqueued (the batch, or one slice of it)
  int slices;               // batch slices of the solve (1: the whole batch on one stream set)
  bool analytic_jacobians;  // ILQR_JAC_ANALYTIC
  bool first_aside;         // the nominal trajectory is a cold start by LaunchPlan::rollout under the present dynamics parameters
  // ---- which of the optional buffers / streams / events the enqueued view holds
  bool lists;               // DevState::order (the compacted lists index the whole batch: slices have none)
  bool chg, chg_f;          // DevState::chg / chg_f
  bool kr;                  // DevState::kr and kr_n
  bool ls_list, ls_kind;    // DevState::ls_list / ls_kind
  bool lgate;               // the gate words of the listed order (d_lgate)
  bool grp_a;               // DevState::grp_a
  bool stream_a;            // group A's stream
  bool adopt_events;        // ev_lin and ev_adopt of the lanes the solve is enqueued on (a slice has none)
  bool twin;                // the twin view is allocated
};

// One iteration's launch order.  TWIN: both lambda passes side by side for every active rollout (k_control_spec).  DUAL: the pair (twin,
// sequential) is enqueued and the device takes one (launch_spec_gate).  SEQUENTIAL: first pass, then the lambda retry -- the first pass
// from DevState::chg where first_listed, and behind the listed side-by-side order where pair (launch_listed_prologue takes one of the two
// on the device).
enum OrderKind { ORDER_SEQUENTIAL = 0, ORDER_TWIN = 1, ORDER_DUAL = 2 };
struct IterationOrder {
  OrderKind kind;
  bool first_listed;
  bool pair;
};
// what a handle remembers of each iteration of its last solve, for the getters (ilqr_capi.hip read_iteration_counts): the order as enqueued
using IterationRecord = IterationOrder;

struct SolveOrder {
  // without the convergence exit every rollout stays active: the per-knot kernels then skip the selection altogether (MASK_ALL instead of
  // MASK_ACTIVE)
  bool sel_active;
  // With the convergence exit on, the launches of an iteration nobody needs are pure latency (17 launches that find nothing to
  // do): the count of rollouts active after iteration i (DevState::order_n, maintained by k_control) follows iteration i to the
  // host, which enqueues iteration i only after it has seen the count left by iteration i - 2 -- one full iteration stays
  // queued on the device meanwhile, so the device never waits for the host.  (ILQR_EE_GATE=0: always enqueue max_iter.)
  bool gate;
  // ilqr_hip_set_dedup_saturated_retry (on by default): bit 1 of k_control's early_exit argument (the sequential orders; the side-by-side
  // order has both passes in flight before either outcome is known).  A retry at the lambda cap repeats its rollout's last executed pass
  // -- the first pass of the same iteration, or, where that one was skipped, the pass it repeats in turn; iteration 0 of every solve runs
  // the full first pass, so the chain never leaves the solve
  int dedup_bit;            // 0 or 2
  // Linearisation cache: from iteration 1 on the per-knot kernels of the region (stance decisions, primal dump, tangent sweeps, kinematics
  // record, cost quadratics) run from DevState::chg -- the active rollouts whose previous iteration accepted a candidate.  A rollout
  // whose two line searches both failed enters the iteration with the nominal trajectory it had, bit for bit (k_control copies nothing),
  // and S.A, S.Bm, S.lx, S.lu, S.lxx, S.luu are functions of that trajectory and the problem data alone (not of lambda) that nothing
  // between two regions writes: the backward kernels and the twin view read them, the control / adoption kernels never touch them,
  // the in-place layout conversions belong to the getters and the stage API, outside a solve.  Iteration 0 takes every rollout.  Not for
  // the forward-difference kernels (they select by S.active and use S.A / S.Bm as scratch) nor for batch slices (no lists);
  // ilqr_hip_set_relinearize_unchanged / ILQR_RELIN=1: the full pass in every iteration.
  bool cache;
  bool lin_listed;          // the region of every iteration runs from list (it, 0) (convergence exit, whole batch), else from no list
  // Early continuation: the rollouts whose first line search of iteration i accepted a step are done with iteration i; their share of
  // iteration i + 1's concurrent region (group A) starts right behind the first control pass, on streams of its own, while the
  // others take their lambda retry (ilqr.cpp:619-644); those follow as group R behind the second control pass, and both groups meet again at
  // the backward pass.  The retry of an early iteration keeps a fraction of the chip busy for two latency-bound passes: the time it
  // left idle is what this recovers.  Same kernels on the same data in the same per-rollout order: results are bit-identical
  // (GPU test).  ILQR_SPLIT=0 / 1 forces one / two groups; by default with the convergence exit only -- measured on one MI355X, executed
  // iterations/s with / without: constraint-free B = 4096 +1.5 %, contact B = 4096 +9 %, contact B = 1024 +5 %, configs[4] +4 %; with a
  // fixed iteration count most rollouts retry in most iterations, the early group is small, and its kernels only take SIMDs from the
  // one-wave-per-SIMD kernels of the retry (headline -3 %, contact +3 % / -3.5 % at B = 4096 / 1024).
  // (analytic Jacobians only: the forward-difference launchers select by S.active, not by the group's list, and use S.A / S.Bm as
  // scratch that k_fd_finish rewrites in place -- group A's pass would rewrite the Jacobians the retry's backward pass is reading)
  bool can_split;
  // First-pass skip: a rollout whose two line searches of iteration i both failed enters iteration i + 1 with its nominal trajectory, its
  // Jacobians and quadratics (cache) AND its lambda unchanged -- the reference `continue`s with the raised lambda, so the first pass of i + 1
  // runs at the lambda of the retry of i (ilqr.cpp:619-646) -- and S.Jbase is the cost of a bit-identical re-roll.  Its first backward pass,
  // line search and candidate costs would rewrite S.K, S.kff, S.Vx, S.Vxx, S.xcand, S.ucand, S.cand_knot with what its last executed pass
  // (that retry; with the dedup option the first pass that saturated) left there, and fail again.  In the sequential order the first
  // pass of iterations >= 1 therefore runs from the list of the rollouts that accepted a candidate, DevState::chg -- the cache's list --,
  // the candidates' knot costs from the same set as flags (DevState::chg_f).  k_control phase 0 still runs for every active rollout: for a
  // skipped one it reads the costs that pass left and decides acc = -1 again from them and S.Jbase -- nothing a skipped launch writes.
  // Not inside the side-by-side orders or the early-continuation split (they keep the full pass: a full pass is always valid), nor
  // without lists (batch slices, forward differences).  ilqr_hip_set_repeat_first_pass / ILQR_REPASS=1: the full first pass everywhere.
  bool skip_first;
  // The retry's line search in the sequential order: from its list (iter, 1), a few hundred rollouts in the early iterations and, with the
  // saturated retries gone, in the late ones -- one rollout per wave where the list holds at most ILQR_LS_LIST_MAX, decided on the device
  // as for the first pass's list; the candidates' knot costs stay selected by need_retry.  Not with the early-continuation split: there the
  // retry runs beside group A's region, and a wave per rollout takes SIMDs from it (the early_exit object of bench.py lost 2 %)
  bool retry_gated;
  // Speculative lambda retry: while at most spec_max rollouts are in a pass (the whole batch, or -- convergence exit with the gate --
  // the count the host has seen), two Riccati passes / line searches of that many one-wave rollouts fit on the chip's 1024 SIMDs side by
  // side.  ILQR_SPEC=0 switches it off (sequential retry as for large passes), ILQR_SPEC_MAX moves the threshold (diagnostics, tests).
  bool twin_order;          // ORDER_TWIN wherever pass_bound <= spec_max
  // The host's count is one iteration old: between spec_max and 4 spec_max the pass may or may not have shrunk below the
  // threshold by now.  Both orders are enqueued and the device takes one (launch_spec_gate): the twin's launches and the
  // one-rollout-per-wave line search see a count of zero unless the list holds <= spec_max rollouts, the sequential first line
  // search and bookkeeping see zero if it does; the lambda-retry launches find an empty retry list behind k_control_spec.
  bool dual_order;          // ORDER_DUAL wherever spec_max < pass_bound <= 4 spec_max
  int spec_max;
  // Listed side-by-side order: what a handle's settings must allow before a fixed-iteration solve enqueues it -- the lists it rests on
  // (linearisation cache, first-pass skip, saturated-retry skip: not with ILQR_RELIN=1, ILQR_REPASS=1, ILQR_DEDUP_RETRY=0 or their setters),
  // analytic Jacobians, the whole batch on one stream set, no early-continuation split, no convergence exit (that path has the orders above)
  bool listed_wanted;
  // From iteration listed_from on, the pair (listed side by side, sequential from the lists) is enqueued and the device takes one by the
  // lists' lengths (launch_listed_prologue).  k_control and k_control_listed both leave order, chg, chg_f and kr behind, so either order
  // may follow either.
  bool listed;
  // (the pair costs ~60 us of empty launches per iteration where the lists stay long -- the early iterations of any solve, every iteration of
  // a batch that keeps accepting: measured, DESIGN 9 -- so it starts with the last two fifths of the iterations unless ILQR_SPEC_LIST_FROM
  // says otherwise: iteration 3 max_iter / 5, a fixed rule)
  int listed_from;
  // The twin is allocated by the first solve that can take a side-by-side order: B <= spec_max, or the convergence exit with its gate on
  // (the late passes of any batch shrink below the threshold), or the listed order.  ILQR_SPEC=0 keeps a handle from ever allocating it.
  bool twin_wanted;
  bool overlap_rollout, reuse_rollout, first_aside;      // rolls_aside, nominal_roll
};

inline SolveOrder resolve_solve_order(const SolveSettings& s, const LaunchPlan& L) {
  SolveOrder o{};
  o.sel_active = s.early_exit;
  o.gate = s.early_exit && s.lists && s.early_exit_gate;
  o.dedup_bit = s.dedup ? 2 : 0;
  o.cache = !s.relin && s.lists && s.chg && L.lin_lists;
  o.lin_listed = s.early_exit && s.lists;
  o.can_split = s.split && s.lists && s.grp_a && s.adopt_events && s.stream_a && s.analytic_jacobians;
  o.skip_first = !s.repass && s.lists && s.chg && s.chg_f && L.lin_lists && L.spec_dual && !o.can_split;
  o.retry_gated = s.lists && L.line_search == DYN_TWO_LANE && !o.can_split;
  o.twin_order = s.twin && s.spec && s.lists;
  o.dual_order = o.twin_order && s.spec_dual && o.gate && L.spec_dual;
  o.spec_max = s.spec_max;
  o.listed_wanted = s.spec && s.spec_lists && s.listed_spec && s.spec_list_max > 0 && !s.early_exit && s.slices <= 1 && s.max_iter > 1 &&
                    s.analytic_jacobians && L.lin_lists && L.spec_dual && s.dedup && !s.relin && !s.repass && !s.split && s.B > s.spec_max &&
                    s.kr && s.ls_list && s.ls_kind && s.lgate;
  o.listed = o.listed_wanted && s.twin && o.skip_first && o.cache && !o.gate;
  o.listed_from = s.spec_list_from >= 1 ? s.spec_list_from : (3 * s.max_iter / 5 > 1 ? 3 * s.max_iter / 5 : 1);
  o.twin_wanted = s.spec && s.slices <= 1 && (s.B <= s.spec_max || (s.early_exit && s.early_exit_gate) || o.listed_wanted);
  o.overlap_rollout = s.overlap_rollout; o.reuse_rollout = s.reuse_rollout; o.first_aside = s.first_aside;
  return o;
}

// The nominal re-rollout of iteration iter runs beside the linearisation -- where it runs at all (nominal_roll below: the verification
// mode, ILQR_REUSE_ROLLOUT=0 / ilqr_hip_set_reroll_nominal).  From the second iteration on the nominal trajectory already is a
// rollout from x0 (the accepted line-search candidate, or the unchanged previous nominal), so the re-rollout reproduces it bit for bit
// (ilqr_hip_get_adopt_mismatches): it runs beside the linearisation and is adopted (with its cost, the line-search baseline) once the
// linearisation and the cost quadratics have read the old copy; the backward pass reads neither, only the line search waits for the
// adoption.  ILQR_OVERLAP_ROLLOUT=0 puts it in front of the region instead.  (only while the line search and the rollout run the same step
// implementation; iteration 0 as well when the nominal trajectory is itself a rollout by this very kernel -- the cold start,
// initializeWithReference ilqr.cpp:113-115; a warm-shifted or caller-supplied trajectory is rolled out BEFORE the linearisation, as the
// reference does)
inline bool rolls_aside(const SolveOrder& o, const LaunchPlan& L, int iter) {
  return (iter > 0 ? L.reroll_aside : (o.first_aside && L.cold_start_aside)) && !o.reuse_rollout && o.overlap_rollout;
}

// THE rule for the nominal rollout of iteration iter (ilqr.cpp:551,563), for every launch order and every augmented-Lagrangian round: not
// at all, in front of the region on the solve's own stream, or beside the region into the shadow buffer with adoption and mismatch count.
// With o.reuse_rollout (the default; ILQR_REUSE_ROLLOUT=0 or ilqr_hip_set_reroll_nominal(ctx, 1) clear it) a rollout whose result the
// buffers already hold is not launched:
//   iterations >= 1, L.reroll_aside -- the nominal trajectory is the previous one or an accepted line-search candidate, both rollouts from
//     x0 by the step implementation the rollout kernel runs, so S.xbar holds the bits the re-roll would write; k_control, k_control_spec and
//     k_control_listed have written S.Jbase = Jn on acceptance, summed along the knots in k_traj_cost_sum's order, so S.Jbase does too;
//   iteration 0, o.first_aside and L.cold_start_aside -- S.xbar is a cold start by this very kernel under the present dynamics parameters
//     (in rounds >= 2 of an augmented-Lagrangian solve: the trajectory the previous round left), and the cost-only call at the top of
//     enqueue_solve has just written S.Jbase under the present weights and multipliers.
// Everywhere else the rollout computes something new and runs BEFORE the region: a warm-shifted or caller-supplied trajectory, a new x0 or
// schedule in iteration 0; every iteration of the mixed cross-check families of the test library, whose line search and rollout run
// different step implementations (!L.reroll_aside).  Without o.reuse_rollout: what rolls_aside says, ASIDE or BEFORE, in every iteration.
enum NominalRoll { ROLL_NONE = 0, ROLL_BEFORE = 1, ROLL_ASIDE = 2 };
inline NominalRoll nominal_roll(const SolveOrder& o, const LaunchPlan& L, int iter) {
  if (!o.reuse_rollout) return rolls_aside(o, L, iter) ? ROLL_ASIDE : ROLL_BEFORE;
  return (iter > 0 ? L.reroll_aside : (o.first_aside && L.cold_start_aside)) ? ROLL_NONE : ROLL_BEFORE;
}
// The early-continuation split of iteration iter + 1 (SolveOrder::can_split) needs what the bit-identity rests on, not the re-rollout
// itself: a group's region may start from S.xbar as the first control pass left it only where a re-roll would reproduce it.  Whether a
// group's region launches a rollout is nominal_roll(o, L, iter + 1) -- ROLL_ASIDE or ROLL_NONE here, never ROLL_BEFORE (iter + 1 >= 1).
// (ILQR_OVERLAP_ROLLOUT=0 without reuse: one group, as before)
inline bool splits_next(const SolveOrder& o, const LaunchPlan& L, int iter, int max_iter) {
  return o.can_split && iter + 1 < max_iter && L.reroll_aside && nominal_roll(o, L, iter + 1) != ROLL_BEFORE;
}

// pass_bound: an upper bound of the rollouts in this iteration's passes -- with the gate the count the host has seen at the start of
// iteration iter - 1 (the active set only shrinks), else the batch; prev_seq: the previous iteration ran in the sequential order (k_control
// has written chg_f for this one)
inline IterationOrder iteration_order(const SolveOrder& o, int iter, int pass_bound, bool prev_seq) {
  if (o.twin_order && pass_bound <= o.spec_max) return IterationOrder{ORDER_TWIN, false, false};
  if (o.dual_order && pass_bound <= 4 * o.spec_max) return IterationOrder{ORDER_DUAL, false, false};
  const bool first_listed = o.skip_first && iter > 0 && prev_seq;
  return IterationOrder{ORDER_SEQUENTIAL, first_listed, o.listed && first_listed && iter >= o.listed_from};
}

}  // namespace ilqr
