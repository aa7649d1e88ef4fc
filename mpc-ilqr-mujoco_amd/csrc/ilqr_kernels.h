// Device-state descriptor and kernel launchers shared by ilqr_kernels.hip and ilqr_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "launch_plan.h"

namespace h1 {
struct ProblemDev;
struct DynParams;
}  // namespace h1

namespace ilqr {

enum { MASK_ALL = 0, MASK_ACTIVE = 1, MASK_RETRY = 2 };

// All pointers are device pointers; rollout-major, row-major inside.
struct DevState {
  int B, N, max_iter;
  double* x0;          // [B][51]
  double* xbar;        // [B][N+1][51]
  double* ubar;        // [B][N][19]
  double* xcand;       // [B][8][N+1][51]   line-search candidates
  double* ucand;       // [B][8][N][19]
  double* cand_cost;   // [B][8]
  double* cand_knot;   // [B][8][N+1]       per-knot costs of the line-search candidates (summed in knot order)
  double* A;           // [B][N][51][51]
  double* Bm;          // [B][N][51][19]
  double* lx;          // [B][N+1][51]
  double* lu;          // [B][N][19]
  double* lxx;         // [B][N+1][51][51]  (inside a solve with the one-wave Riccati kernel: knots t < N hold the 16 x 16 tiles I >= J only)
  double* luu;         // [B][N][19]        diagonal
  double* K;           // [B][N][19][51]
  double* kff;         // [B][N][19]
  double* lin_dump;    // [B][N][sizeof(KnotDump)/8] primal per-body quantities of every knot
  double* quad_rec;    // per-knot records of the cost quadratics (k_quad_kin -> k_cost_quadratics; quad_rec_doubles(B (N + 1)), four knots per line in runs of four fields)
  long quad_knot0;     // index of this view's first knot in quad_rec (batch slices share the handle's buffer)
  double* Vx;          // [B][51]           value gradient at knot 0
  double* Vxx;         // [B][51][51]
  double* J;           // [B] current cost
  double* Jbase;       // [B] cost of the nominal trajectory (line-search baseline)
  double* ls_cost;     // [B] stage API: cost after the line search
  double* lambda;      // [B]
  int* active;         // [B]
  int* need_retry;     // [B]
  int* iters;          // [B]
  int* improved;       // [B]
  int* alpha_idx;      // [B]
  double* trace_cost;  // [B][max_iter+1]
  double* trace_alpha; // [B][max_iter]
  double* trace_lambda;// [B][max_iter]
  // Compacted work lists, rebuilt on the device by k_control (null: not in use, e.g. batch slices): list (it, 0) = rollouts
  // active at the start of iteration it, list (it, 1) = rollouts that take the lambda retry of iteration it.  A launch whose
  // blocks are one rollout each (k_backward_wave) takes rollout order[...][blockIdx] for blockIdx < order_n[...]: the selected
  // rollouts then occupy the FIRST blocks of the grid and spread evenly over the shader engines (workgroups are dealt to them
  // round-robin by index: with a scattered selection one engine needs an extra 0.5 ms round of the one-wave-per-SIMD kernel).
  int* order;          // [2 (max_iter + 1)][B]
  int* order_n;        // [2 (max_iter + 1)]
  // Early continuation (solve_order.h SolveOrder::can_split; ilqr_capi.hip enqueue_sequential_iteration): the rollouts whose FIRST line search of iteration it - 1 accepted a step start
  // the linearisation / cost quadratics / re-rollout of iteration it while the others still take their lambda retry.  Group A =
  // the first order_an[it] entries of list (it, 0) (k_control phase 0 fills that list first; the count is snapshot after it), group R =
  // order_r[0 .. order_rn[it]) (filled by phase 1); grp_a / grp_r: the same two sets as per-rollout flags for the kernels that select
  // by mask (rollout, trajectory cost, adoption).  Null: not in use.
  int* grp_a;          // [B]
  int* grp_r;          // [B]
  int* order_r;        // [B]
  int* order_rn;       // [max_iter + 2]
  int* order_an;       // [max_iter + 2]
  // Linearisation cache (solve_order.h SolveOrder::cache): list it = the rollouts active in iteration it that ACCEPTED a candidate in iteration
  // it - 1 (k_control / k_control_spec: acc >= 0, the condition under which xbar / ubar are overwritten), in the order of list (it, 0)
  // restricted to them.  The other active rollouts enter iteration it with the nominal trajectory of iteration it - 1 bit for bit: A_t,
  // B_t, lxx~_t, lx_t, lu_t, luu_t depend on that trajectory and the problem data only, so the per-knot kernels of the concurrent region
  // run from this list.  Early continuation: group A = the first chg_an[it] entries (phase 0 fills the list first), group R = chg_r[0 ..
  // chg_rn[it]) (phase 1).  Null: not in use.
  int* chg;            // [max_iter + 1][B]
  int* chg_n;          // [max_iter + 1]
  int* chg_r;          // [B]
  int* chg_rn;         // [max_iter + 2]
  int* chg_an;         // [max_iter + 2]
  // First-pass skip (solve_order.h SolveOrder::skip_first): chg_f[b] = 1 while rollout b is on list it of the iteration to come (k_control writes it
  // beside the list), for the kernels that select by mask (the candidates' knot costs).  Null: not in use.
  int* chg_f;          // [B]
  // Listed side-by-side order (solve_order.h SolveOrder::listed; ilqr_capi.hip enqueue_listed_pair): kr list it = the rollouts active in iteration it whose two line searches of
  // iteration it - 1 both failed and whose lambda is below its cap (min(10 lambda, 1e-3) != lambda): their first pass of it is skipped and
  // fails by construction, their retry is known before the iteration starts.  Written by the control kernel that closes iteration it - 1,
  // compacted like chg; disjoint from chg by construction (chg: accepted, kr: failed).  ls_list: chg ++ kr of the iteration at hand, ls_kind[b]:
  // 0 = neither (stuck at the cap: no pass), 1 = on chg, 2 = on kr -- both written by k_listed_prologue.  Null: not in use.
  int* kr;             // [max_iter + 1][B]
  int* kr_n;           // [max_iter + 1]
  int* ls_list;        // [B]
  int* ls_kind;        // [B]
};

// compacted list of the rollouts of a pass inside a solve (DevState::order), or nulls: MASK_ACTIVE at iteration iter -> list (iter, 0), MASK_RETRY -> (iter, 1)
struct WorkList { const int* list; const int* count; };
inline WorkList work_list(const DevState& S, int mode, int iter) {
  if (!S.order || iter < 0 || mode == MASK_ALL) return WorkList{nullptr, nullptr};
  const int slot = 2 * iter + (mode == MASK_RETRY ? 1 : 0);
  return WorkList{S.order + (size_t)slot * S.B, S.order_n + slot};
}

// ---- ilqr_kernels.hip: the launchers that choose between kernel families.  L: the handle's LaunchPlan (launch_plan.h), resolved by the
// caller from its switches (read_variants: the environment, once per handle), contact mode, joint-limit option and Jacobian mode.
Variants read_variants();
void launch_rollout(const LaunchPlan& L, const DevState& S, const h1::ProblemDev& P, int mode, int do_roll, int count_iter, double* cost_out, hipStream_t st);
// geom / st_out: stance from each item's own feet (ProblemDev::stance_geom) / the flags it decided, [count][2] (two-lane kernels only)
void launch_step(const LaunchPlan& L, int count, const double* x, const double* u, const h1::DynParams& dyn, double* xn, hipStream_t st, int stance_l = 1, int stance_r = 1, int geom = 0, int* st_out = nullptr);
void launch_last_step(const LaunchPlan& L, const DevState& S, const h1::ProblemDev& P, hipStream_t st);
// the warm start shifted by `shift` knots (1 <= shift <= N - 1): the copies (launch_warm_shift_m), then ONE kernel that re-rolls
// xbar[N - shift + 1 .. N] with the state in registers
void launch_warm_tail(const LaunchPlan& L, const DevState& S, const h1::ProblemDev& P, int shift, hipStream_t st);
// phases: 1 = primal dump only, 2 = tangent sweeps / FD only, 3 = both.  pack != 0 (a solve under LaunchPlan::pack; the stage API asks
// for the standard layout): A_t, B_t in the layout of riccati_pack.h (the two-knot analytic kernels write it themselves, any other producer
// is followed by the conversion kernel).  stance_dyn: [S.B][N][2] scratch of the stance source GEOMETRY (LaunchPlan::lin_stance_prepass)
void launch_linearize(const LaunchPlan& L, const DevState& S, const h1::ProblemDev& P, int mode, double eps, hipStream_t st, int phases = 3, int iter = -1, int pack = 0, const WorkList* wl = nullptr,
                      int* stance_dyn = nullptr);
// fold_h: the step size h if S.A / S.Bm hold foldable Jacobians (LaunchPlan::backward_foldable runs), else 0 (backward_plain)
void launch_backward(const LaunchPlan& L, const DevState& S, int mode, hipStream_t st, double fold_h = 0.0, int iter = -1);
void launch_backward_list(const LaunchPlan& L, const DevState& S, hipStream_t st, double fold_h, const int* list, const int* count);
// max_rollouts: upper bound of the rollouts this pass can select (the batch, or -- with the early-exit gate -- the count of
// still-active rollouts the host saw two iterations ago): at most 1024 -> one rollout per wave in the two-lane line search
void launch_line_search(const LaunchPlan& L, const DevState& S, const h1::ProblemDev& P, int mode, hipStream_t st, int iter = -1, int max_rollouts = -1);
// ---- ilqr_kernels.hip: one kernel whatever the family
void launch_line_search_list(const DevState& S, const h1::ProblemDev& P, hipStream_t st, const int* list, const int* count, int max_rollouts);      // (LaunchPlan::spec_dual)
// The line search of a list whose length only the device knows: one rollout per wave if it holds <= threshold rollouts, else four per wave
// (same results either way).  Both launches are enqueued behind k_list_gate, which hands the list's count to one of them and zero to the other
// (g[0] / g[1]); max_rollouts (< 0: the batch) bounds the length from the host -- a bound <= threshold needs neither gate nor second launch,
// threshold <= 0 means four per wave always.  An empty list costs the launches.
void launch_line_search_gated(const DevState& S, const h1::ProblemDev& P, hipStream_t st, const int* list, const int* count, int threshold, int max_rollouts, int* g);
void launch_control(const DevState& S, int phase, int iter, double tol, int early_exit, hipStream_t st, int sum_knots = 0, const int* gate = nullptr);
// speculative lambda retry (k_control_spec): T = the twin view whose K, kff, Vx, Vxx, candidates and lambda are its own
void launch_spec_lambda(const DevState& S, double* lambda2, hipStream_t st);
void launch_control_spec(const DevState& S, const DevState& T, int iter, double tol, int early_exit, hipStream_t st, int sum_knots, const int* gate = nullptr);
// Device-side choice between the two orders (the host's count of active rollouts is one iteration old): g[0] = n if n <= max else 0 (count of
// the speculative launches), g[1] = 0 / 1 (gate of the sequential bookkeeping), g[2] = 0 / n (count of the sequential first line search), with
// n = the length of list (iter, 0).  The list-driven launchers take an explicit list / count.
void launch_spec_gate(const DevState& S, int iter, int max, int* g, hipStream_t st);
// Listed side-by-side order.  launch_listed_prologue decides on the device: taken while 2 chg_n[iter] + kr_n[iter] <= max (max <= 0: never) --
// g[0] = chg_n / 0 (the twin's launches), g[1] = 0 / 1 (gate of the sequential order's bookkeeping and candidate costs), g[2] = 0 / chg_n (count
// of the sequential first pass), g[3] = chg_n + kr_n / 0 (the launches on S), g[4] = 1 / 0 (gate of the order's own kernels; read back by the
// getters): taken / not taken -- and, where taken, writes lambda of the known retries and of the twin, S.ls_list and S.ls_kind.
// launch_control_listed (gate g + 4): ilqr.cpp:619-655 for every active rollout by its kind.
void launch_listed_prologue(const DevState& S, double* lambda2, int iter, int max, int* g, hipStream_t st);
void launch_control_listed(const DevState& S, const DevState& T, int iter, hipStream_t st, int sum_knots, const int* g);
void launch_solve_begin(const DevState& S, hipStream_t st);
// ---- al_kernels.h (the tail of ilqr_kernels.hip): the augmented-Lagrangian outer loop (ilqr_hip_set_augmented_lagrangian).  All pointers are device pointers of the whole batch.
struct AlDev {
  double* store; long stride;      // the multiplier store (h1_cost_dev.h: ProblemDev::al points at the same records)
  double margin, growth, tol_joint, tol_ctrl, rho_joint_max, rho_ctrl_max;
  double* viol;                    // [B][2] joint, control violation of the nominal trajectory at the last update
  int* done;                       // [B]
  double* trace;                   // [rounds][B][5]
  int* left;                       // [rounds] rollouts not done after each round (zeroed ahead of the round's update)
  const double* bounds; long bounds_stride;      // the bounds table (ProblemDev::alb, the same records; stride 0: one record for all); null: the model's ranges at `margin`
  // the state family (ilqr_hip_set_al_state_bounds); sbounds null: not installed, nothing below is read.  Appended: nothing above moves
  const double* sbounds; long sbounds_stride;    // its bounds table (ProblemDev::alsb, the same records)
  double* sstore; long sstride;                  // its multiplier store (ProblemDev::als points at the same records)
  double rho_state0, rho_state_max, tol_state;
  double* sviol;                   // [B] state violation of the nominal trajectory at the last update
  double* strace;                  // [rounds][B][2] violation, rho_state the round ran with
  // windows of bounds (ProblemDev::alb_knot, alsb_knot, the same values): 0 one record per set, else the doubles from knot t's record to knot
  // t + 1's inside a set's window, and bounds_stride / sbounds_stride the doubles of one set's window.  Appended: nothing above moves
  long bounds_knot, sbounds_knot;
  // the task family (ilqr_hip_set_al_task_bounds; al_task_dev.h); tbounds null: not installed, nothing below is read.  Appended: nothing above moves
  const double* tbounds; long tbounds_stride, tbounds_knot;      // its window of bounds (ProblemDev::altb, the same rows)
  double* tstore; long tstride;                  // its multiplier store (ProblemDev::alt points at the same records)
  double rho_task0, rho_task_max, tol_task;
  double* tviol;                   // [B] task violation of the nominal trajectory at the last update (knots 1..N, swing rows of the feet)
  double* ttrace;                  // [rounds][B][2] violation, rho_task the round ran with
  const int* stance; long stance_stride;         // the contact schedule (ProblemDev::stance): a foot's rows are off where it stands
};
// The kernels that read windows of bounds live in a module of their own, libilqr_hip_alknot.so beside the library (csrc/Makefile; opened by
// ilqr_capi.hip on the first call that installs a window, as the plant kernels' modules are): the per-knot instantiations of
// k_cost_quadratics, k_traj_knot_cost, k_al_state_knot_cost and k_al_update and the kernels that write the windows, compiled from the same sources with -DAL_KNOT_MODULE, so that
// the library holds the instantiations it held and nothing more.  Its entry points, C linkage (ilqr_alknot_module_<name>; ilqr_alknot_module() returns this table of them); the library's
// launchers call them for the per-knot variants of al_variant (al_plan.h), which a handle's pointers name only once the table below is filled (AlPlan::module).
struct AlBoundsTrackDev;
struct AlBoundsWindowDev;      // (al_bounds_track_kernels.h)
struct PlantTaskScoreDev;      // (plant_task_score_kernels.h)
struct AlKnotModule {
  void (*knot_cost)(const DevState* S, const h1::ProblemDev* P, int mode, const double* xsrc, const double* usrc, int cshift, int oshift, const int* gate, hipStream_t st);
  void (*state_knot_cost)(const DevState* S, const h1::ProblemDev* P, int mode, const double* xsrc, int cshift, int oshift, const int* gate, hipStream_t st);
  void (*cost_quadratics)(const DevState* S, const h1::ProblemDev* P, int mode, const int* list, const int* count, int lower, hipStream_t st);
  void (*al_update)(const DevState* S, const AlDev* A, int round, int masked, hipStream_t st);
  // al_bounds_track_kernels.hip: launch_al_bounds_window_from_track, launch_al_bounds_expand (a code object of their own in the library
  // costs it ~25 KB of headers and metadata for two copy kernels)
  void (*window_from_track)(const AlBoundsTrackDev* T, const AlBoundsWindowDev* W, const int* start, int n_sets, int step, int N, hipStream_t st);
  void (*expand)(const double* rec, long rec_stride, double* win, int width, int n_sets, int N, hipStream_t st);
  // the task family (al_task_dev.h), whose every kernel lives here: its terms added to the knot costs (behind knot_cost and state_knot_cost,
  // ahead of the sum), the warm-start shift of its store, and the nine points of the nominal trajectories into out [B][N+1][9].  cost_quadratics
  // and al_update above launch their task instantiations where ProblemDev::altb / AlDev::tbounds is set.  Appended: nothing above moves
  void (*task_knot_cost)(const DevState* S, const h1::ProblemDev* P, int mode, const double* xsrc, int cshift, int oshift, const int* gate, hipStream_t st);
  void (*task_shift)(const AlDev* A, int B, int N, int shift, hipStream_t st);
  void (*task_points)(const DevState* S, double* out, hipStream_t st);
  // plant_task_score_kernels.hip: launch_plant_task_score (ilqr_hip_plant_set_task_score).  Appended: nothing above moves
  void (*plant_task_score)(const PlantTaskScoreDev* T, int B, const double* hist_x, long hist_row0, long hist_cap, int knot0, int count, double* terms, double* record, hipStream_t st);
  // the velocities of the task family's nine coordinates at every knot of the nominal trajectories into out [B][N+1][9]
  // (ilqr_hip_get_al_task_velocities; al_task_dev.h al_task_velocities).  Appended: nothing above moves
  void (*task_velocities)(const DevState* S, double* out, hipStream_t st);
};
extern AlKnotModule g_al_knot;      // (ilqr_capi.hip)
// masked: the convergence exit is on -- a rollout that was done when the round began did not run and gets no trace row
void launch_al_update(const DevState& S, const AlDev& A, int round, int masked, hipStream_t st);
// shift > N: every multiplier becomes zero (cold start); the penalties are reset to the given values (the state family's to A.rho_state0),
// done flags and violations cleared
void launch_al_shift(const AlDev& A, int B, int N, int shift, double rho_joint, double rho_ctrl, hipStream_t st);
// launch_solve_begin with active = !done (done: of S's rollouts)
void launch_solve_begin_al(const DevState& S, const int* done, hipStream_t st);
void launch_adopt_rollout(const DevState& S, const double* shadow, int mode, unsigned long long* mismatches, hipStream_t st);
void launch_warm_shift(const DevState& S, const double* prev_x, const double* prev_u, hipStream_t st);
void launch_warm_shift_m(const DevState& S, const double* prev_x, const double* prev_u, int shift, hipStream_t st);
void launch_compute_control(const DevState& S, const double* x_meas, double* u_out, hipStream_t st);
void launch_compute_control_at(const DevState& S, int knot, const double* x_meas, double* u_out, hipStream_t st);
void launch_pack_first_knot(const DevState& S, double* u0, double* K0, hipStream_t st);
void launch_pack_payload(const DevState& S, int with_gains, double* out, hipStream_t st);
void launch_mirror_lxx(const DevState& S, hipStream_t st);   // fill the strictly upper tiles of lxx_t, t < N, from the lower ones
int backward_needs_lds_attr();
size_t lin_dump_doubles();
// ---- quad_kernels.hip
// lower = 1: knots t < N get only the tiles I >= J of lxx (what k_backward_wave loads); 2: every knot in the operand layout of
// riccati_pack.h (lx in row / column "aug"); the stage API always asks for the full matrix (0)
void launch_cost_quadratics(const DevState& S, const h1::ProblemDev& P, int mode, hipStream_t st, int iter = -1, int lower = 0, const WorkList* wl = nullptr);
size_t quad_rec_doubles(size_t knots);
// ---- dyn_kernels.hip: one lane per rollout / candidate, and the cost kernels of the two-lane family
void launch_rollout_r(const DevState& S, const h1::ProblemDev& P, int mode, int do_roll, int count_iter, double* cost_out, hipStream_t st);
void launch_step_r(int count, const double* x, const double* u, const h1::DynParams& dyn, double* xn, hipStream_t st);
void launch_last_step_r(const DevState& S, const h1::ProblemDev& P, hipStream_t st);
void launch_warm_tail_r(const DevState& S, const h1::ProblemDev& P, int shift, hipStream_t st);
void launch_line_search_r(const DevState& S, const h1::ProblemDev& P, int mode, hipStream_t st);
void launch_lin_primal_r(const DevState& S, const h1::ProblemDev& P, int mode, hipStream_t st);
void launch_cand_costs(const DevState& S, const h1::ProblemDev& P, int mode, hipStream_t st, bool with_sum = true, const int* gate = nullptr);
void launch_nominal_costs(const DevState& S, const h1::ProblemDev& P, int mode, double* cost_out, hipStream_t st);
int dyn_kernels_set_attr();
// ---- dyn_split_kernels.hip: two lanes per rollout / candidate, the StepKind instantiation picked from the dynamics parameters
void launch_rollout_s(const DevState& S, const h1::ProblemDev& P, int mode, int do_roll, int count_iter, double* cost_out, hipStream_t st);
void launch_step_s(int count, const double* x, const double* u, const h1::DynParams& dyn, double* xn, hipStream_t st, int stance_l, int stance_r, int geom, int* st_out);
void launch_last_step_s(const DevState& S, const h1::ProblemDev& P, hipStream_t st);
void launch_warm_tail_s(const DevState& S, const h1::ProblemDev& P, int shift, hipStream_t st);
// rpw: 0 = rollouts per wave chosen from max_rollouts, 1 / 4 = as given (1: a grid of max_rollouts waves)
void launch_line_search_s(const DevState& S, const h1::ProblemDev& P, int mode, hipStream_t st, const int* list = nullptr, const int* count = nullptr, int max_rollouts = -1, int rpw = 0);
void launch_lin_primal_s(const DevState& S, const h1::ProblemDev& P, int mode, hipStream_t st, const int* list = nullptr, const int* count = nullptr);
// stance flags of the nominal knots t = 0..N-1 from the feet of xbar (out[B][N][2]); rollouts selected as by launch_lin_primal_s
void launch_stance_geom_s(const DevState& S, int mode, const int* list, const int* count, int* out, hipStream_t st);
void launch_linearize_fd_s(const DevState& S, const h1::ProblemDev& P, int mode, double eps, hipStream_t st);
int dyn_split_kernels_set_attr();
// ---- plant_kernels.hip: the closed-loop plant resident in the handle (include/ilqr_hip.h ilqr_hip_plant_*); all device pointers.
// Always the two-lane step, whatever the handle's family.
struct PlantDev {
  double* x;        // [B][51] plant state
  double* u;        // [B][19] control applied in the last substep of the last advance (zero for a rollout that is not alive)
  double* dv;       // [B][25] pending velocity kick
  int* stance;      // [B][2]  stance flags of the last substep
  int* alive;       // [B]     0 once a rollout's state was or became non-finite
  double* hist_x;   // [rows][B][51] history ring (null: none): the state each advance started from, behind its kick
  double* hist_u;   // [rows][B][19]                            and the control it wrote to u
};
// one MPC interval of the plant under the policy of the last solve (first knot of S.xbar / S.ubar / S.K): `substeps` steps of dyn.h (the
// caller passes the plant's parameters, h = dt / substeps); sched / sched_stride: row 0 of each set is the stance of this interval, geom:
// from the feet instead; kick != 0: apply Pl.dv first; hist_row >= 0: fill that row of the ring
void launch_plant_advance(const DevState& S, const PlantDev& Pl, const h1::DynParams& dyn, const int* sched, long sched_stride, int geom, int substeps, int feedback_mode, int kick, long hist_row,
                          hipStream_t st);
int plant_kernels_set_attr();
// ---- the followed plant: `count` consecutive intervals in one launch under the policy knots first_knot .. first_knot + count - 1 (schedule
// rows likewise); the kick before the first interval only; ring rows (hist_row0 + j) % hist_cap, hist_cap = 0: no ring.  (first_knot, count)
// = (0, 1) is the advance: with a table there is no kernel of its own for it.
struct PlantFollowArgs { const int* sched; long sched_stride; int geom, substeps, feedback_mode, kick, first_knot, count; long hist_row0, hist_cap; };
// The tables of the eight followed kernel families (plant_plan.h PlantFamily), each family the superset of the one before it.  In every
// table rollout b reads record b * rec_stride of `records`: rec_stride the record's size, or 0: ONE record that every rollout reads.  A
// table that is not installed has null `records`; a family ignores the tables above its own.
// plant parameter table (ilqr_hip_plant_set_params): g[3], mu, soft, lim_k, torque gain, padding; 8 doubles -- in the place of those fields
// of dyn, and gain * u in the place of u.  dyn still supplies h, the contact mode and the limits switch.  Every family from the parameter
// family on reads T: without a parameter table the caller passes ONE record of the handle's own values with gain 1 (rec_stride 0).
struct PlantTable {
  const double* records;
  int rec_stride;
};
// external wrench on the pelvis (ilqr_hip_plant_set_wrench): F[3], T[3] (world), r[3] (pelvis frame), first, end, padding; 16 doubles.  The
// rollout steps under it in the plant intervals first <= interval0 + j < end.
struct WrenchTable {
  const double* records;
  int rec_stride;
  long interval0;      // plant intervals run since ilqr_hip_plant_reset when this launch starts; set whether or not there is a wrench table (the terrain's window counts from it too)
};
// rigid payload on the pelvis (ilqr_hip_plant_set_payload): mass, centre of mass c[3] (pelvis frame), Ixx, Iyy, Izz, Ixy, Ixz, Iyz about c,
// padding; 16 doubles -- in every substep
struct PayloadTable {
  const double* records;
  int rec_stride;
};
// observation table (ilqr_hip_plant_set_observation): bias[50], sigma[50] in tangent order; 100 doubles; the rollout's stream of the
// generator is stream0 + b.  The followed kernel does not read the table itself: its control law reads x [+] delta, delta the error rows
// PlantCall::dobs [count][B][51] of the call's intervals as ilqr_observe_module_draw wrote them from the table.
struct ObservationTable {
  const double* records;
  int rec_stride;
  unsigned long long seed, stream0;
};
// an actuator between the control law and the joints (ilqr_hip_plant_set_actuator): per substep the law's output -- the COMMAND, which
// stays what the plant reports -- goes through a delay line, a first-order lag and additive noise, and the step takes the result.
// Record: delay, tau[19], sigma[19]; 39 doubles -- and row b * blend_stride of `blend`, beta[19] = -expm1(-h / tau) as the host computed it
// (rec_stride 39 / blend_stride 19, or both 0: one record for all).  z: the normals [count][B][19] of the call's intervals as
// ilqr_actuator_module_draw wrote them.  The actuator's state is the handle's and persists across launches: fifo [B][9][19], y [B][19];
// applied [B][19] takes the torque of the launch's last substep.  substep0: substeps run since the state was primed; 0 primes it (every
// slot and y take the first command).
struct ActuatorTable {
  const double* records;
  int rec_stride;
  const double* blend;
  int blend_stride;
  const double* z;
  double* fifo;
  double* y;
  double* applied;
  long substep0;
};
// the joints of each rollout (ilqr_hip_plant_set_joints): gain[19], range scale[19], damping[19], armature[19], four doubles of padding; 80 doubles
struct JointTable {
  const double* records;
  int rec_stride;
};
// a floor of each rollout's own height (ilqr_hip_plant_set_terrain): z_left, z_right, edge_x, first, end, three doubles of padding; 8
// doubles; the rollout decides its stance flags per substep against that floor.  The window is counted from W.interval0.
struct TerrainTable {
  const double* records;
  int rec_stride;
};
// ONE call record for every followed family, in the library and across the module boundary: everything any family reads.  dobs: the
// observation's error rows, null without an observation table.
struct PlantCall {
  PlantFollowArgs a;
  PlantTable T;
  WrenchTable W;
  PayloadTable M;
  const double* dobs;
  ActuatorTable A;
  JointTable J;
  TerrainTable R;
};
// the library's two families: without a table (reads C.a alone) and with the parameter table (C.a and C.T)
void launch_plant_follow(const DevState& S, const PlantDev& Pl, const h1::DynParams& dyn, const PlantCall& C, hipStream_t st);
void launch_plant_follow_params(const DevState& S, const PlantDev& Pl, const h1::DynParams& dyn, const PlantCall& C, hipStream_t st);
// The six families above live in a module each, libilqr_hip_<stem>.so (plant_kernels.hip compiled with -DPLANT_<STEM>_MODULE; stems wrench,
// payload, observe, actuator, joints, terrain), which the C API opens on first use.  Entry points, C linkage, of every module:
//   int  ilqr_<stem>_module_set_attr()                          plant_set_attr_fn: the LDS attributes of its kernels on the current device
//   void ilqr_<stem>_module_follow(S, Pl, dyn, call, stream)    plant_follow_fn: the module's followed plant kernel
// and beside them
//   wrench, payload, joints   void ilqr_<stem>_module_step(count, x, u, dyn, xn, stance_l, stance_r, wrench[count][9], payload[count][10], joints[count][76], stream)
//                             plant_step_fn: one two-lane step per item (launch_step_s with explicit stance flags) under the item's wrench (F, T,
//                             r), payload and joint record.  A module ignores the arrays its kernel does not take (wrench: payload and joints;
//                             payload: joints); in the payload module wrench may be null, in the joints module wrench and payload: none.
//   terrain                   void ilqr_terrain_module_step(count, x, u, dyn, xn, terrain[count][3] (z_left, z_right, edge_x), stance_out[count][2], stream)
//   observe                   void ilqr_observe_module_draw(B, O, interval0, count, delta[count][B][51], stream)     the errors of intervals interval0 .. + count - 1
//                             void ilqr_observe_module_apply(B, x[B][51], delta[B][51], out[B][51], stream)          out = x [+] delta
//   actuator                  void ilqr_actuator_module_draw(B, seed, stream0, interval0, count, z[count][B][19], stream)     the normals of intervals interval0 .. + count - 1
typedef int (*plant_set_attr_fn)();
typedef void (*plant_follow_fn)(const DevState*, const PlantDev*, const h1::DynParams*, const PlantCall*, hipStream_t);
typedef void (*plant_step_fn)(int, const double*, const double*, const h1::DynParams*, double*, int, int, const double*, const double*, const double*, hipStream_t);
typedef void (*terrain_step_fn)(int, const double*, const double*, const h1::DynParams*, double*, const double*, int*, hipStream_t);
typedef void (*observe_draw_fn)(int, const ObservationTable*, long, int, double*, hipStream_t);
typedef void (*observe_apply_fn)(int, const double*, const double*, double*, hipStream_t);
typedef void (*actuator_draw_fn)(int, unsigned long long, unsigned long long, long, int, double*, hipStream_t);
// ---- riccati_mfma.hip (four waves per rollout) / riccati_wave.hip (one wave per rollout, standard layout)
void launch_backward_mfma(const DevState& S, int mode, hipStream_t st);
int backward_mfma_set_attr();
void launch_backward_wave(const DevState& S, int mode, hipStream_t st, double fold_h, const int* list, const int* count);
// ---- riccati_pack.hip: the one-wave kernel on the operand layout of riccati_pack.h and the conversions between that layout and the
// standard one (in place, per knot region)
void launch_backward_pack(const DevState& S, int mode, hipStream_t st, double fold_h, const int* list, const int* count);
void launch_pack_ab(const DevState& S, hipStream_t st, int mode = MASK_ALL, const int* list = nullptr, const int* count = nullptr);
void launch_pack_zero_pads(const DevState& S, hipStream_t st);
void launch_unpack_ab(const DevState& S, double h, hipStream_t st);
void launch_pack_lxx(const DevState& S, hipStream_t st);
void launch_unpack_lxx(const DevState& S, hipStream_t st);

}  // namespace ilqr
