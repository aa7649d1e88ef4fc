// C-ABI of the batched HIP iLQR (include/ilqr_hip.h): context, device buffers, problem data and the
// host-side orchestration of iLQR::solve (reference src/ilqr/ilqr.cpp:521-660) as a fixed stream of
// kernel launches with per-rollout masks on the device -- no host round trip inside a solve.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl is opened lazily (ilqr_hip_comm_*), never linked
#include <dlfcn.h>
#include <cstdlib>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ilqr_hip.h"
#include "al_task_dev.h"
#include "h1_cost_dev.h"
#include "h1_host_model.h"
#include "ilqr_kernels.h"
#include "plant_plan.h"
#include "group_kernels.h"
#include "solve_order.h"
#include "plant_score_kernels.h"
#include "plant_task_score_kernels.h"
#include "reference_track_kernels.h"
#include "al_bounds_track_kernels.h"

using ilqr::DevState;

// Environment switches (diagnostics, tests): ONE pass over the environment when a handle is created, kept in the handle; no getenv on
// the call path.  ILQR_ENV_PER_CALL=1 (itself read at creation) restores the re-read at the top of every C-ABI call -- the test
// suite and the tools that switch kernel families within one process set it (tests/conftest.py); ilqr_hip_reload_environment
// re-reads on demand.
struct Knobs {
  ilqr::Variants var;
  int dedup_retry;      // ILQR_DEDUP_RETRY (-1: the handle's own setting, ilqr_hip_set_dedup_saturated_retry)
  int relin;            // ILQR_RELIN (-1: the handle's own setting, ilqr_hip_set_relinearize_unchanged)
  int repass;           // ILQR_REPASS=1: the full first pass in every iteration (as ilqr_hip_set_repeat_first_pass; either one is enough)
  int ls_list_max;      // ILQR_LS_LIST_MAX: a first-pass list of at most this many rollouts takes the one-rollout-per-wave line search (1024: one wave per SIMD)
  int slices, stagger, overlap_rollout, reuse_rollout /* -1: the handle's own setting, ilqr_hip_set_reroll_nominal */, ee_gate /* -1: the handle's own setting */, split /* -1: on with the convergence exit */, spec, spec_dual, spec_max;
  int spec_lists;       // ILQR_SPEC_LISTS=0: never the listed side-by-side order (as ilqr_hip_set_listed_spec(ctx, 0); either one is enough)
  int spec_list_max;    // ILQR_SPEC_LIST_MAX: the order is taken while 2 chg_n + kr_n is at most this many one-wave-per-SIMD slots
  int spec_list_from;   // ILQR_SPEC_LIST_FROM: first iteration that enqueues the pair of orders (0: iteration 3 max_iter / 5, a fixed rule -- the empty launches of the order not taken cost time where the lists are long)
  bool per_call;
};
#ifndef SPEC_LIST_MAX_DEFAULT
#define SPEC_LIST_MAX_DEFAULT 1024
#endif
#ifndef SPEC_LIST_FROM_DEFAULT
#define SPEC_LIST_FROM_DEFAULT 0
#endif
static Knobs read_knobs() {
  Knobs k;
  auto geti = [](const char* n, int d) { const char* e = getenv(n); return e ? atoi(e) : d; };
  k.var = ilqr::read_variants();
#ifndef SLICES_DEFAULT
#define SLICES_DEFAULT 1
#endif
  k.slices = geti("ILQR_SLICES", SLICES_DEFAULT);
  k.stagger = geti("ILQR_STAGGER", 1);
  k.dedup_retry = geti("ILQR_DEDUP_RETRY", -1);
  k.relin = geti("ILQR_RELIN", -1);
  k.repass = geti("ILQR_REPASS", 0);
  k.ls_list_max = geti("ILQR_LS_LIST_MAX", 1024);
  k.overlap_rollout = geti("ILQR_OVERLAP_ROLLOUT", 1);
  k.reuse_rollout = geti("ILQR_REUSE_ROLLOUT", -1);
  k.ee_gate = geti("ILQR_EE_GATE", -1);
  k.split = geti("ILQR_SPLIT", -1);
  k.spec = geti("ILQR_SPEC", 1);
  k.spec_dual = geti("ILQR_SPEC_DUAL", 1);
  k.spec_max = geti("ILQR_SPEC_MAX", 512);
  k.spec_lists = geti("ILQR_SPEC_LISTS", 1);
  k.spec_list_max = geti("ILQR_SPEC_LIST_MAX", SPEC_LIST_MAX_DEFAULT);
  k.spec_list_from = geti("ILQR_SPEC_LIST_FROM", SPEC_LIST_FROM_DEFAULT);
  k.per_call = geti("ILQR_ENV_PER_CALL", 0) != 0;
  return k;
}
struct ilqr_hip_ctx {
  int device = 0, B = 0, N = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;          // cost quadratics run here, concurrently with the linearisation
  hipStream_t stream3 = nullptr;          // nominal re-rollout of iterations >= 1, concurrently with both
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_roll = nullptr;
  hipEvent_t ev_lin = nullptr, ev_adopt = nullptr;   // adoption of the re-rolled trajectory beside the backward pass (enqueue_region, wait_adoption)
  double* d_shadowx = nullptr;            // [B][N+1][51] target of the concurrent re-rollout: allocated by the first solve that re-rolls aside (ensure_shadow)
  // ilqr_hip_set_reroll_nominal: 1 = the verification mode, every nominal rollout the reference runs (solve_order.h nominal_roll); nominal_rollouts:
  // rollouts the nominal-rollout launches of the last solve were enqueued for, all rounds and slices (ilqr_hip_get_nominal_rollouts)
  int reroll_nominal = 0;
  long long nominal_rollouts = 0;
  DevState S{};
  h1::ProblemDev P{};
  // reference sets on the device
  double *d_xref = nullptr, *d_uref = nullptr, *d_comref = nullptr, *d_eeref = nullptr, *d_comvelref = nullptr;
  int* d_stance = nullptr;
  int* d_stance_dyn = nullptr;            // [B][N][2] stance flags decided from the feet of xbar (stance source GEOMETRY: linearisation, ilqr_hip_get_stance)
  int* d_stance_out = nullptr;            // [step_cap][2] flags decided by ilqr_hip_step_geometry
  int n_xref = 0, n_stance = 0, n_ee = 0;
  double* d_wsets = nullptr;              // [B][WS_STRIDE] weight-set table (ilqr_hip_set_weight_sets; allocated by its first call); installed while P.wsets points at it
  int n_wsets = 0;                        // 0: shared weights, else the installed table's n_sets
  // Augmented Lagrangian (ilqr_hip_set_augmented_lagrangian): installed while P.al points at al.jc.store; every buffer is kept by the handle once
  // allocated and freed by ilqr_hip_destroy.  Which pointers ProblemDev / AlDev get from all this: al_point_bounds, by the plan of al_plan.h.
  // One record per family of bounds -- jc the hinges and actuators (ilqr_hip_set_al_bounds ...), st the 28 box coordinates
  // (ilqr_hip_set_al_state_bounds ...), tk the nine task coordinates (ilqr_hip_set_al_task_bounds: a window always, no table; a track of its own, ilqr_hip_set_al_task_bounds_track) -- which the bodies behind the two families' entry points take as their parameter:
  struct AlFamily {
    int fields, width;        // doubles of a bounds record in the interface (76 / 56) and on the device (ALB_STRIDE / ALSB_STRIDE)
    int blocks, per;          // a bounds record is `blocks` blocks of lo[per], hi[per] (2 x 19 / 1 x 28); so is a knot's multiplier record:
    int knot_rec, block_at[2];   // its doubles and the offset of each block in it (h1_cost_dev.h); block 1 (the actuators) has no knot N
    double* store = nullptr;  // [B][AL_HDR + (N+1) knot_rec] the multiplier store: penalty `g` of the record at [g], allocated with the family
    double *table = nullptr, *window = nullptr, *track = nullptr;   // bounds [B][width], [B][N+1][width], [rows][width] (null: the track has no such part)
    int sets = 0;             // 0: nothing installed (jc: the model's ranges at the installed margin), else the n_sets of the table or window
    bool knot = false;        // the installed bounds are a window (host is then stale)
    std::vector<double> host; // the installed table as the caller gave it, [sets][fields]
  };
  struct Al {
    int rounds = 0, trace_cap = 0, round = 0, rounds_run = 0;      // round: the one enqueue_solve is enqueuing; rounds_run: rounds the last solve enqueued
    double rho0[2] = {0, 0}, growth = 1.0, max_factor = 1.0, tol[2] = {0, 0}, srho0 = 0.0, stol = 0.0, trho0 = 0.0, ttol = 0.0;
    // viol [B][2], done [B], trace [trace_cap][B][5], left [trace_cap] rollouts not done after each round and its pinned copy h_left (the host's
    // read between two rounds, as the early-exit gate reads its counts); sviol [B], strace [trace_cap][B][2] the state family's
    // tviol [B], ttrace [trace_cap][B][2] the task family's; tpoints [B][N+1][9] the getter's buffer (ilqr_hip_get_al_task_points, allocated by its first call)
    double *viol = nullptr, *trace = nullptr, *sviol = nullptr, *strace = nullptr, *tviol = nullptr, *ttrace = nullptr, *tpoints = nullptr;
    int *done = nullptr, *left = nullptr, *h_left = nullptr;
    hipEvent_t ev = nullptr;
    AlFamily jc{ILQR_AL_BOUNDS, h1::ALB_STRIDE, 2, 19, h1::AL_KNOT, {h1::AL_JLO, h1::AL_ULO}};
    AlFamily st{ILQR_AL_STATE_BOUNDS, h1::ALSB_STRIDE, 1, ILQR_AL_STATE_COORDS, h1::ALS_KNOT, {h1::ALS_LO, 0}};
    AlFamily tk{ILQR_AL_TASK_BOUNDS, h1::ALTB_STRIDE, 1, ILQR_AL_TASK_COORDS, h1::ALT_KNOT, {h1::ALT_LO, 0}};
    double* model = nullptr;  // [ALB_STRIDE] the model's bounds at the installed margin as one record (AlPlan::upload_model)
    // the bounds tracks (ilqr_hip_set_al_bounds_track: jc and st `track`, track_rows; ilqr_hip_set_al_task_bounds_track: tk `track`,
    // task_track_rows): the start rows [B] on the device that both share, allocated with the first track of either kind
    int* track_start = nullptr;
    int track_rows = 0, track_sets = 1, task_track_rows = 0;
  } al;
  // scratch
  double *d_tmpx = nullptr, *d_tmpu = nullptr, *d_prevx = nullptr, *d_prevu = nullptr, *d_u0 = nullptr, *d_K0 = nullptr, *d_cost_tmp = nullptr;
  double *d_stepx = nullptr, *d_stepu = nullptr, *d_stepn = nullptr;   // ilqr_hip_step* scratch, grown on demand
  size_t step_cap = 0;
  unsigned long long* d_mismatch = nullptr;   // elements in which a concurrent re-rollout differed from the trajectory it replaced
  // multi-GPU: RCCL communicator of this handle's rank and the packed first-knot payload it sends
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0;
  double* d_payload = nullptr;
  size_t payload_cap = 0;
  int max_iter = 10;
  double tol = 1e-4;
  int jac_mode = ILQR_JAC_ANALYTIC;
  double fd_eps = 1e-5;
  int early_exit = 1;
  int ee_gate = 1;            // early-exit gate (ilqr_hip_set_early_exit_gate): solve_async waits for iteration i - 2 before it enqueues iteration i
  bool initialized = false, refs_set = false;
  // early-exit gate: the number of rollouts still active after each iteration travels to this pinned array behind the
  // iteration; the host stays one iteration ahead of the device and stops enqueuing once the batch has converged
  int* h_active = nullptr;
  std::vector<hipEvent_t> ev_active;
  int iterations_enqueued = 0;
  // S.xbar is a rollout of (S.x0, S.ubar) by `rolled_variant` under `rolled_dyn` (the cold start): iteration 0 of the next solve
  // may then re-roll it beside the linearisation like every later iteration (solve_order.h rolls_aside); cleared by anything that changes
  // the trajectory or x0 without a rollout
  bool xbar_rolled = false, first_aside = false;
  int rolled_variant = -1;
  h1::DynParams rolled_dyn{};
  // Layouts the last writer left behind (riccati_pack.h).  lxx: 0 whole matrices, 1 the tiles I >= J of the knots t < N only (getters
  // mirror them), 2 operand layout; ab_packed: S.A / S.Bm in the operand layout; ab_pads_clean: the slots of those images that the
  // tangent kernels never write are zeros (true after k_pack_zero_pads or a whole-batch k_pack_ab, false once anything wrote the
  // standard layout over them).  The stage API and the getters convert on demand (in place, per knot region).
  int lxx_layout = 0;
  bool ab_packed = false, ab_pads_clean = false;
  int dedup_retry = 1;          // ilqr_hip_set_dedup_saturated_retry: on unless the caller or ILQR_DEDUP_RETRY=0 asks for the full retry
  // linearisation cache (solve_order.h SolveOrder::cache): relin = ilqr_hip_set_relinearize_unchanged; what the last solve did, for
  // ilqr_hip_get_linearized_rollouts: lin_iterations (0: no solve, or its lists are gone), lin_cached = iterations >= 1 ran from
  // DevState::chg, lin_listed = the region of every iteration ran from list (it, 0) (convergence exit, whole batch), else from no list
  int relin = 0, lin_iterations = 0;
  bool lin_cached = false, lin_listed = false;
  // first-pass skip (solve_order.h SolveOrder::skip_first): repass = ilqr_hip_set_repeat_first_pass; d_fp_gate [4]: device-side choice of the
  // line-search kernel (launch_line_search_gated) -- words 0, 1 for the first pass, words 2, 3 for the lambda retry
  int repass = 0;
  int* d_fp_gate = nullptr;
  // record[it]: the order iteration it of the last solve was enqueued in (enqueue_solve; sized once per solve), for the getters
  // (read_iteration_counts).  first_listed: its first pass ran from DevState::chg (ilqr_hip_get_first_pass_rollouts); kind: what its retry ran
  // for (ilqr_hip_get_retry_pass_rollouts) -- ORDER_SEQUENTIAL the retry list (it, 1), ORDER_TWIN every active rollout (side by side),
  // ORDER_DUAL whichever of the two the device chose; pair: it enqueued the listed pair (word 4 of its gate words says whether the device
  // took the side-by-side order)
  std::vector<ilqr::IterationRecord> record;
  bool env_refused = false;     // ILQR_ENV_PER_CALL: the last re-read selected a family this library does not hold (enter, enter_launching)
  double packed_h = 0.0;        // step size h of the packed image while ab_packed (k_unpack_ab rebuilds the position rows from it)
  Knobs knobs = read_knobs();   // (constructed in ilqr_hip_create)
  double lin_fold_h = 0.0;   // step size h while S.A / S.Bm hold the analytic Jacobians (folded backward kernel), else 0
  std::string err;
  // profiling
  int profiling = 0;
  unsigned prof_mask = 0xFFu;             // stages that get event pairs while profiling is on (ilqr_hip_set_profiled_stages)
  struct Span { int stage; hipEvent_t a, b; };
  std::vector<Span> spans;
  std::vector<hipEvent_t> pool;
  size_t pool_next = 0;
  double stage_ms[8] = {0}, stage_launches[8] = {0};
  // batch slices: the solve of each contiguous slice of the batch is enqueued on its own pair of streams, so that the
  // latency-bound stages of one slice (line search: 8 waves per 64 rollouts, nominal rollout) overlap with the
  // throughput-bound stages of the others (ILQR_SLICES, default SLICES_DEFAULT; 1 = whole batch on one stream pair)
  struct Slice { hipStream_t st = nullptr, st2 = nullptr, st3 = nullptr; hipEvent_t fork = nullptr, join = nullptr, done = nullptr, lead = nullptr, roll = nullptr; };
  std::vector<Slice> slices;
  hipEvent_t ev_begin = nullptr;
  int n_slices = 1;
  // speculative lambda retry (ilqr_kernels.hip k_control_spec): the twin view's own buffers, allocated by the first solve that can use them
  DevState T{};
  bool twin = false, twin_failed = false;
  hipEvent_t ev_spec_fork = nullptr, ev_spec_join = nullptr;
  int spec_iterations = 0;    // iterations of the last solve that enqueued both passes side by side
  int* d_spec_gate = nullptr; // [4] device-side choice of the order (launch_spec_gate)
  // listed side-by-side order (ilqr_kernels.hip k_control_listed): listed_spec = ilqr_hip_set_listed_spec; d_lgate [max_iter][8] the gate words of
  // every iteration (launch_listed_prologue; word 4 = taken), read back by the getters
  int listed_spec = 1;
  int* d_lgate = nullptr;
  // early continuation (solve_order.h SolveOrder::can_split): streams / events of the group that starts the next iteration behind the first control pass
  hipStream_t a1 = nullptr;     // (its cost quadratics and re-rollout share streams 2 and 3 with the other group, see group_a_lanes)
  hipEvent_t evA_fork = nullptr, evA_join = nullptr, evA_roll = nullptr, evA_lin = nullptr, evA_adopt = nullptr;
  int split_iterations = 0;   // iterations of the last solve whose concurrent region ran in two groups
  // device-resident plant (ilqr_hip_plant_*; plant_kernels.hip): every buffer is owned here and freed by ilqr_hip_destroy
  ilqr::PlantDev plant{};
  bool plant_set = false;     // ilqr_hip_plant_reset has given it a state
  bool solved = false;        // a solve has been enqueued: the first knot of xbar / ubar / K is a policy
  bool plant_kick = false;    // plant.dv holds a kick for the next advance
  int plant_substeps = 1, plant_feedback = 0, plant_source = ILQR_STANCE_SCHEDULE;
  // the plant's own model (ilqr_hip_plant_set_model): -1 follows the solver's contact mode / joint-limit option, else the plant's
  int plant_mode = -1, plant_limits = -1;
  // Per-rollout tables of the plant, one TableBuf each: [sets][record] doubles on the device, sets = 1 or B; d null: none installed
  // (table_install / table_clear / table_read).  While any is installed the plant calls launch the family resolve_plant_plan names.
  //   pparams (ilqr_hip_plant_set_params; k_plant_follow_p): records of 8 doubles
  //   wrench  (ilqr_hip_plant_set_wrench; k_plant_follow_w): records of WRENCH_REC doubles
  //   payload (ilqr_hip_plant_set_payload; k_plant_follow_m): records of PAYLOAD_REC doubles
  //   obs     (ilqr_hip_plant_set_observation; k_plant_follow_o): records of 100 doubles
  //   act     (ilqr_hip_plant_set_actuator; k_plant_follow_a): records of 39 doubles
  //   joints  (ilqr_hip_plant_set_joints; k_plant_follow_j): records of JOINT_REC doubles
  //   terrain (ilqr_hip_plant_set_terrain; k_plant_follow_t): records of TERRAIN_REC doubles
  struct TableBuf { double* d = nullptr; int sets = 0; };
  TableBuf pparams, wrench, payload, obs, act, joints, terrain;
  // d_self_params: the ONE parameter record the module families read while no parameter table is installed -- the handle's own values with
  // gain 1, uploaded again whenever they differ from self_params
  double* d_self_params = nullptr;
  double self_params[ILQR_PLANT_PARAMS + 1] = {0};
  unsigned module_attr_set = 0;   // bit ilqr::PlantModule: that module's kernels have their LDS attributes on this handle's device
  // scratch of the single-step calls beside d_stepx / d_stepu / d_stepn: [cap][9] wrenches, [cap][10] payloads, [cap][76] joint records,
  // 4 doubles per item of floors: [count][3] doubles, then the flags that come back, [count][2] ints
  double *d_stepw = nullptr, *d_stepm = nullptr, *d_stepj = nullptr, *d_stept = nullptr;
  size_t step_w_cap = 0, step_m_cap = 0, step_j_cap = 0, step_t_cap = 0;
  // Observation: the plant calls run behind a draw of the call's error rows into d_obs_delta [N][B][51] (a follow never exceeds N intervals),
  // and the warm starts hand the solve Pl.x [+] delta of the current interval.
  unsigned long long obs_seed = 0, obs_stream0 = 0;
  double* d_obs_delta = nullptr;
  double* d_obs_x = nullptr;      // [B][51] the measured state of ilqr_hip_plant_get_observed
  // Actuator: the plant calls run behind a draw of the call's normals into d_act_z [N][B][19].  act_rec is the host's copy of the table, from
  // which d_act_beta [sets][19] is derived again when plant_configure changes the substeps.  The actuator's state -- delay line [B][9][19], lag
  // output [B][19] -- and the applied torque of the last substep [B][19] persist across the calls; act_substeps counts the substeps run since
  // the state was primed (0: the next substep primes it).
  unsigned long long act_seed = 0, act_stream0 = 0;
  std::vector<double> act_rec, act_beta;
  double* d_act_beta = nullptr;
  double* d_act_z = nullptr;
  double* d_act_fifo = nullptr;
  double* d_act_y = nullptr;
  double* d_act_applied = nullptr;
  long act_substeps = 0;
  // Joints: a table whose every record is the model's own joints is no table (joints_nominal, decided on the host when it is installed)
  bool joints_nominal = false;
  long plant_intervals = 0;   // plant intervals run since the last ilqr_hip_plant_reset (the history cursor only counts while a ring exists)
  int hist_cap = 0;           // rows of the history ring (0: none)
  long hist_n = 0;            // advances recorded since the last reset / set_history
  // closed-loop score of the plant (ilqr_hip_plant_set_score; plant_score_kernels.hip): the record [B][8], the term rows of one plant call
  // [N][B][8] and the scoring weights (Q, R, upright, balance, joint limits, control limits), all independent of P's and of the weight sets
  double *d_score = nullptr, *d_score_terms = nullptr;
  bool score_on = false;
  // task score of the plant (ilqr_hip_plant_set_task_score; plant_task_score_kernels.hip in the per-knot module): the record [B][8], the term
  // rows of one plant call [N][B][8], the tolerance of the counts; installed while d_tscore is set
  double *d_tscore = nullptr, *d_tscore_terms = nullptr, tscore_tol = 0.0;
  double score_Q[ILQR_NX] = {0}, score_R[ILQR_NU] = {0}, score_w[4] = {0};
  // reference track (ilqr_hip_set_reference_track; reference_track_kernels.hip): ONE allocation [rows][51 | 19 | 3 | 6 | 3] doubles array by
  // array, then [contact_rows][2] ints; the start rows [B] on the device (allocated with the first track) and their maximum here, for the
  // range check of ilqr_hip_window_from_track
  double* d_track = nullptr;
  int* d_track_start = nullptr;
  int track_rows = 0, track_contact_rows = 0, track_sets = 1, track_max_start = 0;
  // solve groups (ilqr_hip_set_groups; group_kernels.hip in the module libilqr_hip_groups.so): G consecutive rollouts solve one problem from G
  // starts.  G = 1: off, no buffer.  winner [M] the global rollout index of each group's winner and rec [M][4] its record (k_group_select;
  // selected: one has run since the groups were set); sigma [sets][19] on the device while a perturbation is installed (sets 1 or G), with the
  // hold, seed, first stream and draw counter of k_group_perturb.  All of it is the handle's own: nothing here enters ProblemDev or DevState.
  struct Groups {
    int G = 1, sets = 0, hold = 1;
    int *winner = nullptr, *mask = nullptr;      // mask [B]: 1 for the members g >= 1 (the rollouts group_perturb re-rolls), 0 for the incumbents
    double *rec = nullptr, *sigma = nullptr;
    unsigned long long seed = 0, stream0 = 0;
    long draws = 0;
    bool selected = false;
  } grp;
};

// A failed HIP call: "<the call>: <HIP's message>" into the handle, ILQR_ERR_HIP to the caller.  The message is built out of line: built
// in place it was ~200 bytes of string handling per use, 250 uses, and the product library has to stay under 0.8 x the test library
// (test_product_library_holds_the_default_kernel_family_only)
__attribute__((noinline, cold)) static int hip_failed(ilqr_hip_ctx* c, const char* what, hipError_t e) {
  c->err = std::string(what) + ": " + hipGetErrorString(e);
  return ILQR_ERR_HIP;
}
#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_failed((ctx), #call, e_); } while (0)
#define HIPCHK_S(ctx, call) HIPCHK(ctx, call)

template <class T> static int dalloc(ilqr_hip_ctx* c, T** p, size_t count) {
  HIPCHK(c, hipMalloc((void**)p, count * sizeof(T)));
  HIPCHK(c, hipMemsetAsync(*p, 0, count * sizeof(T), c->stream));
  return ILQR_OK;
}
#define TRY(x) do { int r_ = (x); if (r_ != ILQR_OK) return r_; } while (0)

static hipEvent_t next_event(ilqr_hip_ctx* c) {
  if (c->pool_next == c->pool.size()) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) { c->err = "hipEventCreate failed (profiling events)"; return nullptr; }
    c->pool.push_back(e);
  }
  return c->pool[c->pool_next++];
}
struct StageTimer {
  ilqr_hip_ctx* c; int stage; hipStream_t st; hipEvent_t a{}, b{};
  StageTimer(ilqr_hip_ctx* c_, int s, hipStream_t st_ = nullptr) : c(c_), stage(s), st(st_ ? st_ : c_->stream) { if (c->profiling && ((c->prof_mask >> s) & 1u)) { a = next_event(c); b = next_event(c); if (a && b) hipEventRecord(a, st); } }
  ~StageTimer() { if (a && b) { hipEventRecord(b, st); c->spans.push_back({stage, a, b}); } }
};

#ifdef ILQR_LEGACY_KERNELS
static constexpr bool LEGACY_BUILD = true;
#else
static constexpr bool LEGACY_BUILD = false;
#endif
// Which kernel runs each stage of this handle and what that family can do (launch_plan.h): resolved from the handle's state whenever an
// entry point needs it, behind its prologue -- never stored, so no setter has anything to invalidate.
static ilqr::LaunchPlan plan_of(const ilqr_hip_ctx* c) { return ilqr::resolve_plan(c->knobs.var, c->P.dyn.contact, c->P.dyn.limits, c->jac_mode); }
// Prologue of every entry point that touches the device, called after its argument checks.  The kernel family is c->knobs.var and
// nothing else: whatever depends on it takes an ilqr::LaunchPlan argument.  An entry point uses enter_launching if it calls, directly or
// through a static helper, a function that takes one; so does ilqr_hip_plant_advance, whose kernel exists in one family only (the
// two-lane step, whatever the handle's family: on a scalar-dynamics handle of the test library the plant and ilqr_hip_step therefore run
// different kernels) -- it steps the model, and a handle whose environment names an absent family has no model to speak of.  Every other
// entry point uses enter and never refuses.
static inline void enter(ilqr_hip_ctx* c) {
  hipSetDevice(c->device);
  if (c->knobs.per_call) {
    // an unsupported selection keeps the previous one AND is recorded: the calls that launch family-dependent kernels refuse until the
    // environment selects a family this library holds again -- a test that switches families on a product handle must not pass vacuously
    const Knobs k = read_knobs();
    if (ilqr::plan_supported(k.var, LEGACY_BUILD)) { c->knobs = k; c->env_refused = false; }
    else { c->env_refused = true; c->err = "ILQR_ENV_PER_CALL: the environment selects a kernel family this library does not hold (see ilqr_hip_create)"; }
  }
}
// weight sets exist in the cost kernels of the default family; a family whose rollout / line-search kernels evaluate the cost themselves reads the shared values
static const char* weight_sets_refusal(const ilqr_hip_ctx* c) {
  if (!plan_of(c).weight_sets) return "weight sets exist in the default family's cost kernels only; unset ILQR_DYN=s / ILQR_ROLLOUT=r / ILQR_LS=r";
  return nullptr;
}
// the augmented-Lagrangian terms live in the same two cost kernels: the same rule
static const char* al_refusal(const ilqr_hip_ctx* c) {
  if (!plan_of(c).weight_sets) return "the augmented-Lagrangian terms exist in the default family's cost kernels only; unset ILQR_DYN=s / ILQR_ROLLOUT=r / ILQR_LS=r";
  return nullptr;
}
static inline int enter_launching(ilqr_hip_ctx* c) {
  enter(c);
  if (c->env_refused) return ILQR_ERR_UNSUPPORTED;
  if (c->P.wsets) if (const char* why = weight_sets_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  if (c->P.al) if (const char* why = al_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  return ILQR_OK;
}
// libilqr_hip_<stem>.so in the directory this library was loaded from
__attribute__((noinline, minsize)) static std::string module_path(const char* stem) {
  Dl_info info;
  std::string dir = ".";
  if (dladdr((const void*)&ilqr_hip_al_default_bounds, &info) && info.dli_fname) {
    const std::string self = info.dli_fname;
    const size_t slash = self.rfind('/');
    if (slash != std::string::npos) dir = self.substr(0, slash);
  }
  return dir + "/libilqr_hip_" + stem + ".so";
}
// One way to open a module: libilqr_hip_<stem>.so, opened once per process, on first use, from the directory this library was loaded from,
// and handed to `resolve`, which looks its entry points up and says whether all are there.  `name`: of the kernels, in the messages.
struct ModuleLib { std::once_flag once; bool ok = false; std::string why; };
__attribute__((noinline)) static bool open_module(ModuleLib& m, const char* stem, const char* name, bool (*resolve)(void* lib, int which), int which) {
  std::call_once(m.once, [&] {
    const std::string path = module_path(stem);
    void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib) { m.why = std::string("the ") + name + " kernels' module is missing: " + path + " (csrc/Makefile builds it beside the library)"; return; }
    m.ok = resolve(lib, which);
    if (!m.ok) m.why = std::string("the ") + name + " kernels' module lacks an entry point: " + path;
  });
  return m.ok;
}
// n rows of `fields` doubles onto the device as rows of `width` doubles, padded with zeros; returns behind the copy
__attribute__((noinline, minsize)) static int upload_rows(ilqr_hip_ctx* c, double* dst, const double* src, size_t n, int fields, int width) {
  std::vector<double> padded;
  if (width != fields) {
    padded.assign(n * width, 0.0);
    for (size_t r = 0; r < n; ++r) std::memcpy(padded.data() + r * width, src + r * fields, sizeof(double) * fields);
    src = padded.data();
  }
  HIPCHK(c, hipMemcpyAsync(dst, src, n * width * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
// The per-knot instantiations of the cost kernels and of k_al_update live in libilqr_hip_alknot.so (ilqr_kernels.h AlKnotModule), opened by the
// first call that may install a window.  Missing module or entry point: ILQR_ERR_UNSUPPORTED.
namespace ilqr { AlKnotModule g_al_knot = {}; }
using AlFamily = ilqr_hip_ctx::AlFamily;
// the module and the two window buffers: what every call that may install a window needs, before it touches the handle's state
__attribute__((noinline, minsize)) static int al_knot_ready(ilqr_hip_ctx* c) {
  static ModuleLib lib;
  // one exported symbol: the table of the module's entry points (al_knot_kernels.hip)
  const auto resolve = [](void* so, int) { const auto table = (const ilqr::AlKnotModule* (*)())dlsym(so, "ilqr_alknot_module"); if (table) ilqr::g_al_knot = *table(); return table != nullptr; };
  if (!open_module(lib, "alknot", "per-knot bounds", resolve, 0)) { c->err = lib.why; return ILQR_ERR_UNSUPPORTED; }
  for (AlFamily* f : {&c->al.jc, &c->al.st, &c->al.tk}) if (!f->window) TRY(dalloc(c, &f->window, (size_t)c->B * (c->N + 1) * f->width));
  return ILQR_OK;
}
// Points ProblemDev at the bounds: resolves the plan of what is installed (al_plan.h states the rules), does the work it names -- the model's
// record, the expansions (k_al_bounds_expand, device to device; a plan that names one has the module loaded) -- and writes each family's
// pointer and strides as the plan names them.
__attribute__((noinline, minsize)) static int al_point_bounds(ilqr_hip_ctx* c) {
  const ilqr::AlTaskPlan tplan = ilqr::resolve_al_plan(c->P.al != nullptr, {c->al.jc.sets, c->al.jc.knot}, {c->al.st.sets, c->al.st.knot}, {c->al.tk.sets, true});
  const ilqr::AlPlan& plan = tplan.base;
  if (plan.upload_model) {
    double rec[h1::ALB_STRIDE] = {0};
    h1host::al_default_bounds(c->P.al_margin, rec);
    if (!c->al.model) TRY(dalloc(c, &c->al.model, (size_t)h1::ALB_STRIDE));
    TRY(upload_rows(c, c->al.model, rec, 1, h1::ALB_STRIDE, h1::ALB_STRIDE));
  }
  const auto point = [&](const AlFamily& f, const ilqr::AlFamilyPlan& fp, bool expand, const double*& ptr, long& stride, long& knot) {
    const double* rec = (fp.source == ilqr::AL_SRC_MODEL_RECORD || fp.source == ilqr::AL_SRC_MODEL_EXPANDED) ? c->al.model : f.table;
    if (expand) ilqr::g_al_knot.expand(rec, fp.shared ? 0 : f.width, f.window, f.width, f.sets ? f.sets : 1, c->N, c->stream);
    ptr = (fp.source == ilqr::AL_SRC_NONE || fp.source == ilqr::AL_SRC_MODEL_RANGES) ? nullptr : fp.per_knot ? f.window : rec;
    stride = fp.shared ? 0 : fp.per_knot ? (long)(c->N + 1) * f.width : (long)f.width;
    knot = fp.per_knot ? f.width : 0;
  };
  point(c->al.jc, plan.jc, plan.expand_jc, c->P.alb, c->P.alb_stride, c->P.alb_knot);
  point(c->al.st, plan.st, plan.expand_st, c->P.alsb, c->P.alsb_stride, c->P.alsb_knot);
  point(c->al.tk, tplan.tk, false, c->P.altb, c->P.altb_stride, c->P.altb_knot);
  if (plan.module) HIPCHK(c, hipGetLastError());
  return ILQR_OK;
}
__attribute__((noinline, minsize)) static ilqr::AlDev al_view(const ilqr_hip_ctx* c) {
  ilqr::AlDev A{};
  A.store = c->al.jc.store; A.stride = h1::al_record_doubles(c->N);
  A.margin = c->P.al_margin; A.growth = c->al.growth; A.tol_joint = c->al.tol[0]; A.tol_ctrl = c->al.tol[1];
  A.rho_joint_max = c->al.rho0[0] * c->al.max_factor; A.rho_ctrl_max = c->al.rho0[1] * c->al.max_factor;
  A.viol = c->al.viol; A.done = c->al.done; A.trace = c->al.trace; A.left = c->al.left;
  A.bounds = c->P.alb; A.bounds_stride = c->P.alb_stride;
  A.sbounds = c->P.alsb; A.sbounds_stride = c->P.alsb_stride;
  A.sstore = c->al.st.store; A.sstride = h1::als_record_doubles(c->N);
  A.rho_state0 = c->al.srho0; A.rho_state_max = c->al.srho0 * c->al.max_factor; A.tol_state = c->al.stol;
  A.sviol = c->al.sviol; A.strace = c->al.strace;
  A.bounds_knot = c->P.alb_knot; A.sbounds_knot = c->P.alsb_knot;
  A.tbounds = c->P.altb; A.tbounds_stride = c->P.altb_stride; A.tbounds_knot = c->P.altb_knot;
  A.tstore = c->al.tk.store; A.tstride = h1::alt_record_doubles(c->N);
  A.rho_task0 = c->al.trho0; A.rho_task_max = c->al.trho0 * c->al.max_factor; A.tol_task = c->al.ttol;
  A.tviol = c->al.tviol; A.ttrace = c->al.ttrace;
  A.stance = c->P.stance; A.stance_stride = c->P.stance_stride;
  return A;
}
// the multipliers follow the trajectory: shifted by the knots it is shifted by (shift > N: a cold start, all zero), penalties back to their
// initial values -- enqueued on the handle's stream by every initialiser while AL is installed
static void al_follow_initialize(ilqr_hip_ctx* c, int shift) {
  if (c->P.al) ilqr::launch_al_shift(al_view(c), c->B, c->N, shift, c->al.rho0[0], c->al.rho0[1], c->stream);
}

// The wrench, payload, observation, actuator, joints and terrain families of the plant kernels are modules of their own (csrc/Makefile PLANT_MODULE;
// plant_kernels.hip says why), each opened on first use from the directory this library was loaded from, as RCCL is opened on first use: a
// process that never uses a family never loads it.  A module that is missing or lacks an entry point is an error of the call that needs it
// (ILQR_ERR_UNSUPPORTED).
namespace {
enum ModuleFn { FN_SET_ATTR = 0, FN_FOLLOW, FN_STEP, FN_DRAW = FN_STEP, FN_APPLY, MODULE_FNS };
// stem: of the file (libilqr_hip_<stem>.so) and of the symbols (ilqr_<stem>_module_<entry>); name: in the messages; entry: by ModuleFn
struct ModuleDesc { const char *stem, *name; const char* entry[MODULE_FNS]; };
const ModuleDesc MODULE_DESC[ilqr::PLANT_MODULES] = {
  {"wrench", "wrench", {"set_attr", "follow", "step", nullptr}},
  {"payload", "payload", {"set_attr", "follow", "step", nullptr}},
  {"observe", "observation", {"set_attr", "follow", "draw", "apply"}},
  {"actuator", "actuator", {"set_attr", "follow", "draw", nullptr}},
  {"joints", "joints", {"set_attr", "follow", "step", nullptr}},
  {"terrain", "terrain", {"set_attr", "follow", "step", nullptr}},
};
struct PlantModuleLib : ModuleLib { void* fn[MODULE_FNS] = {nullptr}; };
PlantModuleLib g_plant_module[ilqr::PLANT_MODULES];
bool resolve_plant_module(void* lib, int which) {
  const ModuleDesc& d = MODULE_DESC[which];
  bool ok = true;
  for (int i = 0; i < MODULE_FNS && d.entry[i]; ++i) {
    g_plant_module[which].fn[i] = dlsym(lib, (std::string("ilqr_") + d.stem + "_module_" + d.entry[i]).c_str());
    ok = ok && g_plant_module[which].fn[i];
  }
  return ok;
}
// opened and resolved once per process and module
PlantModuleLib& plant_module(int which) {
  open_module(g_plant_module[which], MODULE_DESC[which].stem, MODULE_DESC[which].name, resolve_plant_module, which);
  return g_plant_module[which];
}
// entry point `slot` of a module that need_module has checked, as its typedef of ilqr_kernels.h
template <class Fn> Fn module_fn(int which, ModuleFn slot) { return (Fn)plant_module(which).fn[slot]; }
}  // namespace
// the module, with its kernels' LDS attributes set on this handle's device (once per handle)
static int need_module(ilqr_hip_ctx* c, int which) {
  const PlantModuleLib& m = plant_module(which);
  if (!m.ok) { c->err = m.why; return ILQR_ERR_UNSUPPORTED; }
  if (!((c->module_attr_set >> which) & 1u)) {
    if (module_fn<ilqr::plant_set_attr_fn>(which, FN_SET_ATTR)() != 0) { c->err = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed on the ") + MODULE_DESC[which].name + " kernels"; return ILQR_ERR_HIP; }
    c->module_attr_set |= 1u << which;
  }
  return ILQR_OK;
}

extern "C" {

// (once per handle, as ilqr_hip_destroy; like the getters and setters marked minsize below it is compiled for size, which is what the
// library-size check of tests/test_gpu_configs.py weighs)
__attribute__((minsize)) int ilqr_hip_create(ilqr_hip_ctx** out, int device, int batch, int horizon, double dt) {
  if (!out || batch <= 0 || horizon <= 0 || !(dt > 0.0)) return ILQR_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return ILQR_ERR_NO_DEVICE;
  ilqr_hip_ctx* c = new ilqr_hip_ctx();
  c->device = device; c->B = batch; c->N = horizon;
  if (!ilqr::plan_supported(c->knobs.var, LEGACY_BUILD)) {
    // (the handle is returned so that ilqr_hip_last_error can say why; the caller destroys it)
    c->err = "the environment selects a cross-check kernel family (ILQR_BACKWARD / ILQR_LS / ILQR_ROLLOUT / ILQR_DYN / ILQR_LINT) that this library does not hold: "
             "they are compiled into the test library only (make ../lib/libilqr_hip_legacy.so, -DILQR_LEGACY_KERNELS)";
    *out = c;
    return ILQR_ERR_UNSUPPORTED;
  }
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream) != hipSuccess || hipStreamCreate(&c->stream2) != hipSuccess || hipStreamCreate(&c->stream3) != hipSuccess || hipEventCreateWithFlags(&c->ev_roll, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_lin, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->ev_adopt, hipEventDisableTiming) != hipSuccess) { delete c; return ILQR_ERR_NO_DEVICE; }
  const size_t B = batch, N = horizon, n = ILQR_NX, m = ILQR_NU;
  DevState& S = c->S;
  S.B = batch; S.N = horizon; S.max_iter = c->max_iter;
  int rc = ILQR_OK;
  auto A = [&](int r) { if (rc == ILQR_OK) rc = r; };
  A(dalloc(c, &S.x0, B * n)); A(dalloc(c, &S.xbar, B * (N + 1) * n)); A(dalloc(c, &S.ubar, B * N * m));
  A(dalloc(c, &S.xcand, B * 8 * (N + 1) * n)); A(dalloc(c, &S.ucand, B * 8 * N * m)); A(dalloc(c, &S.cand_cost, B * 8)); A(dalloc(c, &S.cand_knot, B * 8 * (N + 1)));
  A(dalloc(c, &S.A, B * N * n * n + 32)); A(dalloc(c, &S.Bm, B * N * n * m + 32));   // slack: riccati_wave.hip stages 16-byte pairs that may straddle the end of the last row
  A(dalloc(c, &S.lx, B * (N + 1) * n)); A(dalloc(c, &S.lu, B * N * m)); A(dalloc(c, &S.lxx, B * (N + 1) * n * n)); A(dalloc(c, &S.luu, B * N * m));
  A(dalloc(c, &S.lin_dump, B * N * ilqr::lin_dump_doubles()));
  A(dalloc(c, &S.quad_rec, ilqr::quad_rec_doubles(B * (N + 1)))); S.quad_knot0 = 0;
  A(dalloc(c, &S.K, B * N * m * n + 32)); /* slack: the line search stages K_t in 16-byte pairs, the last one ends one double past the knot */ A(dalloc(c, &S.kff, B * N * m)); A(dalloc(c, &S.Vx, B * n)); A(dalloc(c, &S.Vxx, B * n * n));
  A(dalloc(c, &S.J, B)); A(dalloc(c, &S.Jbase, B)); A(dalloc(c, &S.ls_cost, B)); A(dalloc(c, &S.lambda, B));
  A(dalloc(c, &S.active, B)); A(dalloc(c, &S.need_retry, B)); A(dalloc(c, &S.iters, B)); A(dalloc(c, &S.improved, B)); A(dalloc(c, &S.alpha_idx, B));
  A(dalloc(c, &S.trace_cost, B * (c->max_iter + 1))); A(dalloc(c, &S.trace_alpha, B * c->max_iter)); A(dalloc(c, &S.trace_lambda, B * c->max_iter));
  A(dalloc(c, &S.order, B * 2 * (c->max_iter + 1))); A(dalloc(c, &S.order_n, 2 * (size_t)(c->max_iter + 1)));
  A(dalloc(c, &S.grp_a, B)); A(dalloc(c, &S.grp_r, B)); A(dalloc(c, &S.order_r, B)); A(dalloc(c, &S.order_rn, (size_t)c->max_iter + 2)); A(dalloc(c, &S.order_an, (size_t)c->max_iter + 2));
  A(dalloc(c, &S.chg, B * (c->max_iter + 1))); A(dalloc(c, &S.chg_n, (size_t)c->max_iter + 2)); A(dalloc(c, &S.chg_r, B)); A(dalloc(c, &S.chg_rn, (size_t)c->max_iter + 2)); A(dalloc(c, &S.chg_an, (size_t)c->max_iter + 2));
  A(dalloc(c, &S.chg_f, B)); A(dalloc(c, &c->d_fp_gate, 4));
  A(dalloc(c, &S.kr, B * (c->max_iter + 1))); A(dalloc(c, &S.kr_n, (size_t)c->max_iter + 1)); A(dalloc(c, &S.ls_list, B)); A(dalloc(c, &S.ls_kind, B)); A(dalloc(c, &c->d_lgate, 8 * (size_t)c->max_iter));
  if (rc == ILQR_OK && (hipStreamCreate(&c->a1) != hipSuccess ||
      hipEventCreateWithFlags(&c->evA_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->evA_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evA_roll, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->evA_lin, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->evA_adopt, hipEventDisableTiming) != hipSuccess)) { c->err = "stream / event creation failed (early continuation)"; rc = ILQR_ERR_HIP; }
  A(dalloc(c, &c->d_tmpx, B * (N + 1) * n)); A(dalloc(c, &c->d_tmpu, B * N * m));
  A(dalloc(c, &c->d_prevx, B * (N + 1) * n)); A(dalloc(c, &c->d_prevu, B * N * m));
  A(dalloc(c, &c->d_u0, B * m)); A(dalloc(c, &c->d_K0, B * m * n)); A(dalloc(c, &c->d_cost_tmp, B)); A(dalloc(c, &c->d_mismatch, 1));
  // shared reference sets sized for per-rollout use
  A(dalloc(c, &c->d_xref, B * (N + 1) * n)); A(dalloc(c, &c->d_uref, B * N * m)); A(dalloc(c, &c->d_comref, B * (N + 1) * 3));
  A(dalloc(c, &c->d_eeref, B * (N + 1) * 6)); A(dalloc(c, &c->d_comvelref, B * (N + 1) * 3)); A(dalloc(c, &c->d_stance, B * (N + 1) * 2));
  A(dalloc(c, &c->d_stance_dyn, B * N * 2));
  A(dalloc(c, &c->plant.x, B * n)); A(dalloc(c, &c->plant.u, B * m)); A(dalloc(c, &c->plant.dv, B * ILQR_NV)); A(dalloc(c, &c->plant.stance, B * 2)); A(dalloc(c, &c->plant.alive, B));
  if (rc != ILQR_OK) { *out = c; return rc; }
  if (ilqr::backward_needs_lds_attr() != 0 || ilqr::plant_kernels_set_attr() != 0) { c->err = "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed"; *out = c; return ILQR_ERR_HIP; }
  h1::ProblemDev& P = c->P;
  P.N = horizon; P.dyn.h = dt; P.dyn.g[0] = 0; P.dyn.g[1] = 0; P.dyn.g[2] = -9.81; P.dyn.contact = 0; P.dyn.soft = 1e-5; P.dyn.mu = 1.0; P.dyn.limits = 0; P.dyn.lim_k = 0.0;
  for (int i = 0; i < ILQR_NX; ++i) { P.Q[i] = 1.0; P.Qf[i] = 1.0; }
  for (int i = 0; i < ILQR_NU; ++i) P.R[i] = 1.0;
  P.w_com = P.w_com_vel = P.w_ee_pos = P.w_ee_vel = P.w_upright = P.w_balance = 0.0;
  P.w_joint = 500.0; P.w_ctrl = 1000.0;  // RobotUtils ctor defaults, robot_utils.cpp:10
  P.x_ref = c->d_xref; P.u_ref = c->d_uref; P.com_ref = c->d_comref; P.stance = c->d_stance; P.ee_ref = c->d_eeref; P.com_vel_ref = c->d_comvelref;
  P.x_ref_stride = P.u_ref_stride = P.com_ref_stride = P.stance_stride = P.ee_ref_stride = P.com_vel_ref_stride = 0;
  P.wsets = nullptr; P.wsets_stride = 0;
  P.al = nullptr; P.al_stride = 0; P.al_margin = 0.0; P.alb = nullptr; P.alb_stride = 0;
  P.als = nullptr; P.als_stride = 0; P.alsb = nullptr; P.alsb_stride = 0; P.alb_knot = 0; P.alsb_knot = 0;
  P.alt = nullptr; P.alt_stride = 0; P.altb = nullptr; P.altb_stride = 0; P.altb_knot = 0;
  // default: stance everywhere (RobotUtils::isStance default, robot_utils.cpp:494-504), lambda = 1e-6 (ilqr.cpp:16)
  std::vector<int> ones((N + 1) * 2, 1);
  hipMemcpyAsync(c->d_stance, ones.data(), ones.size() * sizeof(int), hipMemcpyHostToDevice, c->stream);
  std::vector<double> lam(B, 1e-6);
  hipMemcpyAsync(S.lambda, lam.data(), B * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "stream sync failed in create"; *out = c; return ILQR_ERR_HIP; }
  if (getenv("ILQR_DEBUG_PTRS")) {   // diagnostic: device address ranges, to place the address of a reported memory access fault
    auto pr = [&](const char* name, const void* p, size_t bytes) { std::fprintf(stderr, "[ilqr_hip] %-10s %p .. %p\n", name, p, (const void*)((const char*)p + bytes)); };
    pr("x0", S.x0, B * n * 8); pr("xbar", S.xbar, B * (N + 1) * n * 8); pr("ubar", S.ubar, B * N * m * 8);
    pr("xcand", S.xcand, B * 8 * (N + 1) * n * 8); pr("ucand", S.ucand, B * 8 * N * m * 8); pr("K", S.K, (B * N * m * n + 32) * 8); pr("kff", S.kff, B * N * m * 8);
    pr("A", S.A, (B * N * n * n + 32) * 8); pr("Bm", S.Bm, (B * N * n * m + 32) * 8); pr("lxx", S.lxx, B * (N + 1) * n * n * 8); pr("lin_dump", S.lin_dump, B * N * ilqr::lin_dump_doubles() * 8);
    pr("active", S.active, B * 4); pr("cand_knot", S.cand_knot, B * 8 * (N + 1) * 8);
  }
  *out = c;
  return ILQR_OK;
}

__attribute__((minsize)) int ilqr_hip_destroy(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  DevState& S = c->S;
  void* ptrs[] = {S.cand_knot, S.lin_dump, S.quad_rec, S.x0, S.xbar, S.ubar, S.xcand, S.ucand, S.cand_cost, S.A, S.Bm, S.lx, S.lu, S.lxx, S.luu, S.K, S.kff, S.Vx, S.Vxx, S.J, S.Jbase, S.ls_cost,
                  S.lambda, S.active, S.need_retry, S.iters, S.improved, S.alpha_idx, S.trace_cost, S.trace_alpha, S.trace_lambda, S.order, S.order_n, c->d_tmpx, c->d_tmpu,
                  c->d_prevx, c->d_prevu, c->d_shadowx, c->d_u0, c->d_K0, c->d_cost_tmp, c->d_stepx, c->d_stepu, c->d_stepn, c->d_mismatch, c->d_payload, c->d_xref, c->d_uref, c->d_comref, c->d_eeref, c->d_comvelref, c->d_stance, c->d_stance_dyn, c->d_stance_out, c->d_wsets, c->al.viol, c->al.trace, c->al.done, c->al.left, c->al.sviol, c->al.strace, c->al.model, c->al.track_start, c->al.tviol, c->al.ttrace, c->al.tpoints};
  for (void* p : ptrs) if (p) hipFree(p);
  for (const AlFamily* f : {&c->al.jc, &c->al.st, &c->al.tk}) for (void* p : {(void*)f->store, (void*)f->table, (void*)f->window, (void*)f->track}) if (p) hipFree(p);
  if (c->al.h_left) (void)hipHostFree(c->al.h_left);
  if (c->al.ev) hipEventDestroy(c->al.ev);
  if (c->twin) { void* tw[] = {c->T.K, c->T.kff, c->T.Vx, c->T.Vxx, c->T.xcand, c->T.ucand, c->T.cand_cost, c->T.cand_knot, c->T.lambda, c->d_spec_gate}; for (void* p : tw) if (p) hipFree(p); }
  { void* gp[] = {S.grp_a, S.grp_r, S.order_r, S.order_rn, S.order_an, S.chg, S.chg_n, S.chg_r, S.chg_rn, S.chg_an, S.chg_f, c->d_fp_gate, S.kr, S.kr_n, S.ls_list, S.ls_kind, c->d_lgate}; for (void* p : gp) if (p) hipFree(p); }
  { void* pl[] = {c->plant.x, c->plant.u, c->plant.dv, c->plant.stance, c->plant.alive, c->plant.hist_x, c->plant.hist_u, c->d_score, c->d_score_terms, c->d_tscore, c->d_tscore_terms, c->d_track, c->d_track_start, c->d_self_params, c->d_stepw, c->d_stepm, c->d_stepj, c->d_stept, c->d_obs_delta, c->d_obs_x, c->d_act_beta, c->d_act_z, c->d_act_fifo, c->d_act_y, c->d_act_applied}; for (void* p : pl) if (p) hipFree(p); }
  for (ilqr_hip_ctx::TableBuf* t : {&c->pparams, &c->wrench, &c->payload, &c->obs, &c->act, &c->joints, &c->terrain}) if (t->d) hipFree(t->d);
  for (void* p : {(void*)c->grp.winner, (void*)c->grp.rec, (void*)c->grp.sigma, (void*)c->grp.mask}) if (p) hipFree(p);
  for (hipEvent_t e : {c->evA_fork, c->evA_join, c->evA_roll, c->evA_lin, c->evA_adopt}) if (e) hipEventDestroy(e);
  if (c->a1) hipStreamDestroy(c->a1);
  if (c->ev_spec_fork) hipEventDestroy(c->ev_spec_fork);
  if (c->ev_spec_join) hipEventDestroy(c->ev_spec_join);
  if (c->comm) ilqr_hip_comm_destroy(c);
  for (hipEvent_t e : c->pool) hipEventDestroy(e);
  for (hipEvent_t e : c->ev_active) hipEventDestroy(e);
  if (c->h_active) (void)hipHostFree(c->h_active);
  for (auto& sl : c->slices) { hipEventDestroy(sl.fork); hipEventDestroy(sl.join); hipEventDestroy(sl.done); hipEventDestroy(sl.lead); hipEventDestroy(sl.roll); hipStreamDestroy(sl.st3); hipStreamDestroy(sl.st2); hipStreamDestroy(sl.st); }
  if (c->ev_begin) hipEventDestroy(c->ev_begin);
  if (c->ev_fork) hipEventDestroy(c->ev_fork);
  if (c->ev_join) hipEventDestroy(c->ev_join);
  if (c->ev_roll) hipEventDestroy(c->ev_roll);
  if (c->ev_lin) hipEventDestroy(c->ev_lin);
  if (c->ev_adopt) hipEventDestroy(c->ev_adopt);
  if (c->stream3) hipStreamDestroy(c->stream3);
  if (c->stream2) hipStreamDestroy(c->stream2);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
  return ILQR_OK;
}
const char* ilqr_hip_last_error(const ilqr_hip_ctx* c) { return c ? c->err.c_str() : "null context"; }
int ilqr_hip_batch(const ilqr_hip_ctx* c) { return c ? c->B : -1; }
int ilqr_hip_horizon(const ilqr_hip_ctx* c) { return c ? c->N : -1; }
void* ilqr_hip_stream(ilqr_hip_ctx* c) { return c ? (void*)c->stream : nullptr; }

int ilqr_hip_set_cost_weights(ilqr_hip_ctx* c, const double* Q, const double* R, const double* Qf) {
  if (!c || !Q || !R || !Qf) return ILQR_ERR_ARG;
  std::memcpy(c->P.Q, Q, sizeof(c->P.Q)); std::memcpy(c->P.R, R, sizeof(c->P.R)); std::memcpy(c->P.Qf, Qf, sizeof(c->P.Qf));
  return ILQR_OK;
}
int ilqr_hip_set_task_weights(ilqr_hip_ctx* c, double w_com, double w_com_vel, double w_ee_pos, double w_ee_vel, double w_upright, double w_balance) {
  if (!c) return ILQR_ERR_ARG;
  c->P.w_com = w_com; c->P.w_com_vel = w_com_vel; c->P.w_ee_pos = w_ee_pos; c->P.w_ee_vel = w_ee_vel; c->P.w_upright = w_upright; c->P.w_balance = w_balance;
  return ILQR_OK;
}
int ilqr_hip_set_constraint_weights(ilqr_hip_ctx* c, double wj, double wc) { if (!c) return ILQR_ERR_ARG; c->P.w_joint = wj; c->P.w_ctrl = wc; return ILQR_OK; }
int ilqr_hip_set_gravity(ilqr_hip_ctx* c, double gx, double gy, double gz) { if (!c) return ILQR_ERR_ARG; c->P.dyn.g[0] = gx; c->P.dyn.g[1] = gy; c->P.dyn.g[2] = gz; return ILQR_OK; }

static int check_sets(const ilqr_hip_ctx* c, int n_sets) { return (n_sets == 1 || n_sets == c->B) ? ILQR_OK : ILQR_ERR_ARG; }

int ilqr_hip_set_weight_sets(ilqr_hip_ctx* c, const double* Q, const double* R, const double* Qf, const double* task, const double* constraint, int n_sets) {
  if (!c || !Q || !R || !Qf || !task || !constraint || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  if (const char* why = weight_sets_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  if (c->P.al) { c->err = "weight sets together with the augmented Lagrangian are not supported: ilqr_hip_clear_augmented_lagrangian first"; return ILQR_ERR_UNSUPPORTED; }
  if (!c->d_wsets) TRY(dalloc(c, &c->d_wsets, (size_t)c->B * h1::WS_STRIDE));
  std::vector<double> rec((size_t)n_sets * h1::WS_STRIDE, 0.0);
  for (int s = 0; s < n_sets; ++s) {
    double* r = rec.data() + (size_t)s * h1::WS_STRIDE;
    std::memcpy(r + h1::WS_Q, Q + (size_t)s * ILQR_NX, sizeof(double) * ILQR_NX); std::memcpy(r + h1::WS_QF, Qf + (size_t)s * ILQR_NX, sizeof(double) * ILQR_NX);
    std::memcpy(r + h1::WS_R, R + (size_t)s * ILQR_NU, sizeof(double) * ILQR_NU); std::memcpy(r + h1::WS_TASK, task + (size_t)s * 6, sizeof(double) * 6);
    r[h1::WS_W_JOINT] = constraint[2 * s]; r[h1::WS_W_CTRL] = constraint[2 * s + 1];
  }
  HIPCHK(c, hipMemcpyAsync(c->d_wsets, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->P.wsets = c->d_wsets; c->P.wsets_stride = n_sets == 1 ? 0 : (long)h1::WS_STRIDE;
  c->n_wsets = n_sets;
  return ILQR_OK;
}
int ilqr_hip_clear_weight_sets(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  c->P.wsets = nullptr; c->P.wsets_stride = 0; c->n_wsets = 0;      // (the buffer stays with the handle for the next table)
  return ILQR_OK;
}
int ilqr_hip_num_weight_sets(const ilqr_hip_ctx* c) { return c ? c->n_wsets : -1; }

// ---------------------------------------------------------------- augmented-Lagrangian joint and torque limits
__attribute__((minsize)) int ilqr_hip_set_augmented_lagrangian(ilqr_hip_ctx* c, int rounds, double rho_joint0, double rho_ctrl0, double growth, double rho_max_factor, double margin,
                                      double tol_joint, double tol_ctrl) {
  if (!c || rounds < 1 || !(rho_joint0 > 0.0) || !(rho_ctrl0 > 0.0) || !(growth >= 1.0) || !(rho_max_factor >= 1.0) || !(margin >= 0.0) || !(margin < 0.5) ||
      !(tol_joint >= 0.0) || !(tol_ctrl >= 0.0) || !std::isfinite(rho_joint0) || !std::isfinite(rho_ctrl0) || !std::isfinite(growth) || !std::isfinite(rho_max_factor)) return ILQR_ERR_ARG;
  enter(c);
  if (const char* why = al_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  if (c->P.wsets) { c->err = "the augmented Lagrangian together with weight sets is not supported: ilqr_hip_clear_weight_sets first"; return ILQR_ERR_UNSUPPORTED; }
  const size_t B = c->B;
  if (!c->al.jc.store) { TRY(dalloc(c, &c->al.jc.store, B * (size_t)h1::al_record_doubles(c->N))); TRY(dalloc(c, &c->al.viol, B * 2)); TRY(dalloc(c, &c->al.done, B)); }
  if (!c->al.sviol) TRY(dalloc(c, &c->al.sviol, B));
  if (!c->al.tviol) TRY(dalloc(c, &c->al.tviol, B));
  if (!c->al.ev) HIPCHK_S(c, hipEventCreateWithFlags(&c->al.ev, hipEventDisableTiming));
  if (rounds > c->al.trace_cap) {
    HIPCHK_S(c, hipStreamSynchronize(c->stream));
    if (c->al.trace) (void)hipFree(c->al.trace);
    if (c->al.left) (void)hipFree(c->al.left);
    if (c->al.h_left) (void)hipHostFree(c->al.h_left);
    if (c->al.strace) (void)hipFree(c->al.strace);
    if (c->al.ttrace) (void)hipFree(c->al.ttrace);
    c->al.trace = nullptr; c->al.left = nullptr; c->al.h_left = nullptr; c->al.strace = nullptr; c->al.ttrace = nullptr; c->al.trace_cap = 0;
    TRY(dalloc(c, &c->al.trace, (size_t)rounds * B * 5)); TRY(dalloc(c, &c->al.left, (size_t)rounds)); TRY(dalloc(c, &c->al.strace, (size_t)rounds * B * 2));
    TRY(dalloc(c, &c->al.ttrace, (size_t)rounds * B * 2));
    HIPCHK_S(c, hipHostMalloc((void**)&c->al.h_left, sizeof(int) * (size_t)rounds, hipHostMallocDefault));
    c->al.trace_cap = rounds;
  }
  c->al.rounds = rounds; c->al.rho0[0] = rho_joint0; c->al.rho0[1] = rho_ctrl0; c->al.growth = growth; c->al.max_factor = rho_max_factor;
  c->al.tol[0] = tol_joint; c->al.tol[1] = tol_ctrl; c->al.rounds_run = 0;
  c->P.al = c->al.jc.store; c->P.al_stride = h1::al_record_doubles(c->N); c->P.al_margin = margin;
  TRY(al_point_bounds(c));      // (a state table without a bounds table: the model's record at the new margin)
  HIPCHK_S(c, hipMemsetAsync(c->al.trace, 0xFF, (size_t)rounds * B * 5 * sizeof(double), c->stream));      // (all bits set: NaN)
  HIPCHK_S(c, hipMemsetAsync(c->al.strace, 0xFF, (size_t)rounds * B * 2 * sizeof(double), c->stream));
  HIPCHK_S(c, hipMemsetAsync(c->al.ttrace, 0xFF, (size_t)rounds * B * 2 * sizeof(double), c->stream));
  al_follow_initialize(c, c->N + 1);
  HIPCHK_S(c, hipGetLastError());
  HIPCHK_S(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
__attribute__((minsize)) int ilqr_hip_clear_augmented_lagrangian(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  c->P.al = nullptr; c->P.al_stride = 0; c->P.al_margin = 0.0; c->al.rounds = 0; c->al.rounds_run = 0;      // (the buffers stay with the handle for the next call)
  c->P.als = nullptr; c->P.als_stride = 0; c->P.alt = nullptr; c->P.alt_stride = 0;
  // the tables and windows of every family go with it: a fresh installation starts on the model's ranges (the bounds track stays with the handle)
  for (AlFamily* f : {&c->al.jc, &c->al.st, &c->al.tk}) { f->sets = 0; f->knot = false; }
  return al_point_bounds(c);      // (nothing installed: null pointers, no work)
}
int ilqr_hip_augmented_lagrangian_rounds(const ilqr_hip_ctx* c) { return c ? (c->P.al ? c->al.rounds : 0) : -1; }
// what every entry point below needs first
__attribute__((noinline)) static int al_installed(ilqr_hip_ctx* c) {
  if (c->P.al) return ILQR_OK;
  c->err = "no augmented Lagrangian installed";
  return ILQR_ERR_STATE;
}
// ---- the bounds, one body per operation for both families (ilqr_hip_ctx::AlFamily).  Joint / torque family: one record of ILQR_AL_BOUNDS doubles per
// set, joint lo, joint hi, ctrl lo, ctrl hi; state family: the 28 box coordinates (pelvis position, pelvis velocity, joint velocities), one
// record lo[28], hi[28] per set.  Windows [n_sets][N+1][fields] hold one such record per knot; the bounds track they can be cut from on the
// device: al_bounds_track_kernels.hip.
static_assert(h1::ALB_FIELDS == ILQR_AL_BOUNDS && h1::ALB_JHI == 19 && h1::ALB_ULO == 38 && h1::ALB_UHI == 57, "the interface's record is the device record without its padding");
static_assert(h1::ALSB_FIELDS == ILQR_AL_STATE_BOUNDS && h1::ALS_COORDS == ILQR_AL_STATE_COORDS && h1::ALSB_HI == 28, "the interface's record is the device record without its padding");
static_assert(h1::AL_JHI == h1::AL_JLO + 19 && h1::AL_UHI == h1::AL_ULO + 19 && h1::ALS_HI == h1::ALS_LO + 28 && h1::AL_HDR == h1::ALS_HDR && h1::AL_RHO_JOINT == 0 && h1::AL_RHO_CTRL == 1 && h1::ALS_RHO == 0,
              "a knot's multiplier record: per block the lower bounds' multipliers, then the upper bounds'; the penalties lead the store's header");
int ilqr_hip_al_default_bounds(double margin, double* bounds) {
  if (!bounds || !(margin >= 0.0) || !(margin < 0.5)) return ILQR_ERR_ARG;
  h1host::al_default_bounds(margin, bounds);
  return ILQR_OK;
}
int ilqr_hip_al_state_slot(int k) { return (k >= 0 && k < ILQR_AL_STATE_COORDS) ? h1::als_slot(k) : -1; }
// the old getters' refusal while their family's bounds are a window
static const char* const AL_WINDOW_ERR = "per-knot bounds: ilqr_hip_get_al_knot_bounds";
// the family exists: the joint / torque family with the installation, the state family with its bounds
static bool al_family_absent(const ilqr_hip_ctx* c, const AlFamily& f) { return &f != &c->al.jc && !f.sets; }
// every pair of n records: no NaN, lo <= hi, lo < +inf, hi > -inf (lo = -inf / hi = +inf switch that side off)
__attribute__((noinline, minsize)) static bool al_bounds_ok(const AlFamily& f, const double* v, size_t n) {
  for (size_t r = 0; r < n; ++r)
    for (int g = 0; g < f.blocks; ++g)
      for (int i = 0; i < f.per; ++i) {
        const double lo = v[r * f.fields + 2 * f.per * g + i], hi = v[r * f.fields + 2 * f.per * g + f.per + i];
        if (!(lo <= hi) || lo == HUGE_VAL || hi == -HUGE_VAL) return false;      // (a NaN fails lo <= hi)
      }
  return true;
}
// what a family without bounds is solved with: the model's ranges at the installed margin / every side switched off
__attribute__((noinline)) static void al_no_bounds(const ilqr_hip_ctx* c, const AlFamily& f, double* rec) {
  if (&f == &c->al.jc) h1host::al_default_bounds(c->P.al_margin, rec);
  else for (int i = 0; i < f.fields; ++i) rec[i] = i < f.per ? -HUGE_VAL : HUGE_VAL;
}
static size_t al_store_doubles(const ilqr_hip_ctx* c, const AlFamily& f) { return h1::AL_HDR + (size_t)f.knot_rec * (c->N + 1); }
// the state (or the task) family's multiplier store, for a table or a window of bounds: zero where none was installed; bounds that replace
// others keep the multipliers.  rho_state (rho_task) starts at rho_state0 (rho_task0) either way
__attribute__((noinline, minsize)) static int al_state_store_install(ilqr_hip_ctx* c, AlFamily& f, double rho_state0, double tol_state) {
  const bool task = &f == &c->al.tk;
  const size_t B = c->B, rec_d = al_store_doubles(c, f);
  if (!f.store) TRY(dalloc(c, &f.store, B * rec_d));
  std::vector<double> st(B * rec_d, 0.0);
  HIPCHK_S(c, hipStreamSynchronize(c->stream));
  if (f.sets) HIPCHK_S(c, hipMemcpy(st.data(), f.store, st.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; ++b) st[b * rec_d + h1::ALS_RHO] = rho_state0;
  HIPCHK_S(c, hipMemcpy(f.store, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
  if (!f.sets) HIPCHK_S(c, hipMemset(task ? c->al.tviol : c->al.sviol, 0, B * sizeof(double)));
  if (task) { c->P.alt = f.store; c->P.alt_stride = (long)rec_d; c->al.trho0 = rho_state0; c->al.ttol = tol_state; return ILQR_OK; }
  c->P.als = f.store; c->P.als_stride = (long)rec_d;
  c->al.srho0 = rho_state0; c->al.stol = tol_state;
  return ILQR_OK;
}
// a table (one record per set) or a window (N + 1 records per set) of a family's bounds, behind the caller's argument checks: the later call
// wins within a family.  state: rho_state0 and tol_state of the state family, whose store comes with its bounds
__attribute__((noinline, minsize)) static int al_install(ilqr_hip_ctx* c, AlFamily& f, const double* bounds, int n_sets, bool window, const double* state = nullptr) {
  enter(c);
  const size_t rows = (size_t)n_sets * (window ? c->N + 1 : 1);
  if (window) TRY(al_knot_ready(c));
  else if (!f.table) TRY(dalloc(c, &f.table, (size_t)c->B * f.width));
  TRY(upload_rows(c, window ? f.window : f.table, bounds, rows, f.fields, f.width));
  if (state) TRY(al_state_store_install(c, f, state[0], state[1]));
  if (!window) f.host.assign(bounds, bounds + rows * f.fields);
  f.sets = n_sets; f.knot = window;
  return al_point_bounds(c);
}
// both setters' argument checks; rows: records per set
__attribute__((noinline, minsize)) static int al_set_bounds(ilqr_hip_ctx* c, AlFamily& f, const double* bounds, int n_sets, bool window, const double* state = nullptr) {
  TRY(al_installed(c));
  if (!bounds || check_sets(c, n_sets) || (state && (!(state[0] > 0.0) || !std::isfinite(state[0]) || !(state[1] >= 0.0))) || !al_bounds_ok(f, bounds, (size_t)n_sets * (window ? c->N + 1 : 1))) return ILQR_ERR_ARG;
  return al_install(c, f, bounds, n_sets, window, state);
}
// table or window; the buffers stay with the handle for the next one
__attribute__((noinline, minsize)) static int al_clear_bounds(ilqr_hip_ctx* c, AlFamily& f) {
  TRY(al_installed(c));
  f.sets = 0; f.knot = false;
  if (&f == &c->al.st) { c->P.als = nullptr; c->P.als_stride = 0; }
  if (&f == &c->al.tk) { c->P.alt = nullptr; c->P.alt_stride = 0; }
  enter(c);
  return al_point_bounds(c);
}
// the whole-horizon getter: the record each rollout is solved with
__attribute__((noinline, minsize)) static int al_get_bounds(ilqr_hip_ctx* c, AlFamily& f, double* bounds) {
  if (!bounds) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  if (f.knot) { c->err = AL_WINDOW_ERR; return ILQR_ERR_STATE; }
  double none[ILQR_AL_BOUNDS];
  if (!f.sets) al_no_bounds(c, f, none);
  for (int b = 0; b < c->B; ++b) std::memcpy(bounds + (size_t)b * f.fields, f.sets ? f.host.data() + (size_t)(f.sets == 1 ? 0 : b) * f.fields : none, sizeof(double) * f.fields);
  return ILQR_OK;
}
int ilqr_hip_set_al_bounds(ilqr_hip_ctx* c, const double* bounds, int n_sets) { return c ? al_set_bounds(c, c->al.jc, bounds, n_sets, false) : ILQR_ERR_ARG; }
int ilqr_hip_set_al_knot_bounds(ilqr_hip_ctx* c, const double* bounds, int n_sets) { return c ? al_set_bounds(c, c->al.jc, bounds, n_sets, true) : ILQR_ERR_ARG; }
int ilqr_hip_set_al_state_bounds(ilqr_hip_ctx* c, const double* bounds, int n_sets, double rho_state0, double tol_state) {
  const double state[2] = {rho_state0, tol_state};
  return c ? al_set_bounds(c, c->al.st, bounds, n_sets, false, state) : ILQR_ERR_ARG;
}
int ilqr_hip_set_al_state_knot_bounds(ilqr_hip_ctx* c, const double* bounds, int n_sets, double rho_state0, double tol_state) {
  const double state[2] = {rho_state0, tol_state};
  return c ? al_set_bounds(c, c->al.st, bounds, n_sets, true, state) : ILQR_ERR_ARG;
}
int ilqr_hip_clear_al_bounds(ilqr_hip_ctx* c) { return c ? al_clear_bounds(c, c->al.jc) : ILQR_ERR_ARG; }
int ilqr_hip_clear_al_state_bounds(ilqr_hip_ctx* c) { return c ? al_clear_bounds(c, c->al.st) : ILQR_ERR_ARG; }
int ilqr_hip_num_al_bound_sets(const ilqr_hip_ctx* c) { return c ? c->al.jc.sets : -1; }
int ilqr_hip_num_al_state_bound_sets(const ilqr_hip_ctx* c) { return c ? c->al.st.sets : -1; }
int ilqr_hip_get_al_bounds(ilqr_hip_ctx* c, double* bounds) { return c ? al_get_bounds(c, c->al.jc, bounds) : ILQR_ERR_ARG; }
int ilqr_hip_get_al_state_bounds(ilqr_hip_ctx* c, double* bounds) { return c ? al_get_bounds(c, c->al.st, bounds) : ILQR_ERR_ARG; }
int ilqr_hip_al_bounds_per_knot(const ilqr_hip_ctx* c) { return c ? ((c->P.al && c->al.jc.knot) ? 1 : 0) | ((c->P.al && c->al.st.knot) ? 2 : 0) : -1; }
// what the kernels read at every knot, whoever wrote it: the windows (knot stride set), a table's records, or nothing (al_no_bounds)
__attribute__((noinline, minsize)) static int al_get_knot_bounds(ilqr_hip_ctx* c, double* joint_ctrl, double* state, double* task) {
  if (!c) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  enter(c);
  const size_t B = c->B, n1 = (size_t)c->N + 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const struct { const AlFamily& f; double* out; const double* dev; long stride, knot; } fams[3] = {
    {c->al.jc, joint_ctrl, c->P.alb, c->P.alb_stride, c->P.alb_knot}, {c->al.st, state, c->P.alsb, c->P.alsb_stride, c->P.alsb_knot},
    {c->al.tk, task, c->P.altb, c->P.altb_stride, c->P.altb_knot}};
  for (int i = 0; i < 3; ++i) {
    const auto& v = fams[i];
    if (!v.out) continue;
    const size_t F = v.f.fields, W = v.f.width, per_set = (v.knot ? n1 : 1) * W;
    std::vector<double> img(v.dev ? (v.stride ? B : 1) * per_set : F);
    if (v.dev) HIPCHK(c, hipMemcpy(img.data(), v.dev, img.size() * sizeof(double), hipMemcpyDeviceToHost));
    else al_no_bounds(c, v.f, img.data());
    for (size_t b = 0; b < B; ++b)
      for (size_t t = 0; t < n1; ++t)
        std::memcpy(v.out + (b * n1 + t) * F, v.dev ? img.data() + (v.stride ? b : 0) * per_set + (v.knot ? t : 0) * W : img.data(), sizeof(double) * F);
  }
  return ILQR_OK;
}
int ilqr_hip_get_al_knot_bounds(ilqr_hip_ctx* c, double* joint_ctrl, double* state) { return al_get_knot_bounds(c, joint_ctrl, state, nullptr); }
// ---- the task family's entry points: the bodies above on the third family record.  Its bounds are a window always
static_assert(h1::ALTB_FIELDS == ILQR_AL_TASK_BOUNDS && h1::ALT_COORDS == ILQR_AL_TASK_COORDS && h1::ALTB_HI == 9 && h1::ALT_HI == h1::ALT_LO + 9 && h1::ALT_HDR == h1::AL_HDR && h1::ALT_RHO == 0,
              "the interface's row is the device row without its padding; the store's layout is the one al_convert walks");
__attribute__((minsize)) int ilqr_hip_set_al_task_bounds(ilqr_hip_ctx* c, const double* bounds, int n_sets, double rho_task0, double tol_task) {
  const double state[2] = {rho_task0, tol_task};
  return c ? al_set_bounds(c, c->al.tk, bounds, n_sets, true, state) : ILQR_ERR_ARG;
}
int ilqr_hip_clear_al_task_bounds(ilqr_hip_ctx* c) { return c ? al_clear_bounds(c, c->al.tk) : ILQR_ERR_ARG; }
int ilqr_hip_num_al_task_bound_sets(const ilqr_hip_ctx* c) { return c ? c->al.tk.sets : -1; }
int ilqr_hip_get_al_task_bounds(ilqr_hip_ctx* c, double* bounds) { return bounds ? al_get_knot_bounds(c, nullptr, nullptr, bounds) : ILQR_ERR_ARG; }

// ---- the multiplier stores.  Host image of a family's store <-> the interface's arrays, one pass: block g of a knot's record <-> mu[g]
// [B][N+1][per][2] (lower, upper; block 1, the actuators: [B][N][per][2]), the penalties <-> rho [B][blocks]; to_store = false reads the image
// into the arrays, true writes them into it (any pointer may be null; knot 0 of block 0 is stored as zero: x_0 is given, its multipliers stay zero)
__attribute__((noinline, minsize)) static void al_convert(const ilqr_hip_ctx* c, const AlFamily& f, double* st, double* const mu[2], double* rho, bool to_store) {
  const size_t N = c->N, rec = al_store_doubles(c, f);
  for (size_t b = 0; b < (size_t)c->B; ++b) {
    double* r = st + b * rec;
    for (int g = 0; g < f.blocks; ++g) {
      if (rho) { if (to_store) r[g] = rho[f.blocks * b + g]; else rho[f.blocks * b + g] = r[g]; }
      if (!mu[g]) continue;
      const size_t T = g ? N : N + 1;
      for (size_t t = 0; t < T; ++t)
        for (int i = 0; i < 2 * f.per; ++i) {
          double& s = r[h1::AL_HDR + t * f.knot_rec + f.block_at[g] + i];
          double& o = mu[g][((b * T + t) * f.per + i % f.per) * 2 + i / f.per];
          if (to_store) s = (g == 0 && t == 0) ? 0.0 : o; else o = s;
        }
    }
  }
}
// doubles of mu[g] and of rho
static size_t al_mu_doubles(const ilqr_hip_ctx* c, const AlFamily& f, int g) { return (size_t)c->B * (g ? c->N : c->N + 1) * f.per * 2; }
// reads the store (set: installs the caller's arrays in its image and writes it back).  Without a state family its getters give zero
// multipliers and rho_state 0 (nothing is constrained) and its setter refuses
__attribute__((noinline, minsize)) static int al_store_io(ilqr_hip_ctx* c, AlFamily& f, double* const mu[2], double* rho, bool set) {
  TRY(al_installed(c));
  if (al_family_absent(c, f)) {
    if (set) { c->err = &f == &c->al.tk ? "no task bounds installed" : "no state bounds installed"; return ILQR_ERR_STATE; }
    for (int g = 0; g < f.blocks; ++g) if (mu[g]) std::fill(mu[g], mu[g] + al_mu_doubles(c, f, g), 0.0);
    if (rho) std::fill(rho, rho + (size_t)c->B * f.blocks, 0.0);
    return ILQR_OK;
  }
  if (set) {
    auto ok = [](const double* v, size_t n, bool positive) { if (v) for (size_t e = 0; e < n; ++e) if (!std::isfinite(v[e]) || v[e] < 0.0 || (positive && v[e] == 0.0)) return false; return true; };
    for (int g = 0; g < f.blocks; ++g) if (!ok(mu[g], al_mu_doubles(c, f, g), false)) return ILQR_ERR_ARG;
    if (!ok(rho, (size_t)c->B * f.blocks, true)) return ILQR_ERR_ARG;
  }
  enter(c);
  std::vector<double> st((size_t)c->B * al_store_doubles(c, f));
  HIPCHK_S(c, hipStreamSynchronize(c->stream));
  HIPCHK_S(c, hipMemcpy(st.data(), f.store, st.size() * sizeof(double), hipMemcpyDeviceToHost));
  al_convert(c, f, st.data(), mu, rho, set);
  if (set) HIPCHK_S(c, hipMemcpy(f.store, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
  return ILQR_OK;
}
int ilqr_hip_get_al_multipliers(ilqr_hip_ctx* c, double* joint, double* ctrl) { double* const mu[2] = {joint, ctrl}; return c ? al_store_io(c, c->al.jc, mu, nullptr, false) : ILQR_ERR_ARG; }
int ilqr_hip_get_al_penalties(ilqr_hip_ctx* c, double* rho) { double* const mu[2] = {nullptr, nullptr}; return c && rho ? al_store_io(c, c->al.jc, mu, rho, false) : ILQR_ERR_ARG; }
int ilqr_hip_set_al_multipliers(ilqr_hip_ctx* c, const double* joint, const double* ctrl, const double* rho) {
  double* const mu[2] = {const_cast<double*>(joint), const_cast<double*>(ctrl)};
  return c ? al_store_io(c, c->al.jc, mu, const_cast<double*>(rho), true) : ILQR_ERR_ARG;
}
int ilqr_hip_get_al_state_multipliers(ilqr_hip_ctx* c, double* m) { double* const mu[2] = {m, nullptr}; return c && m ? al_store_io(c, c->al.st, mu, nullptr, false) : ILQR_ERR_ARG; }
int ilqr_hip_get_al_state_penalties(ilqr_hip_ctx* c, double* rho) { double* const mu[2] = {nullptr, nullptr}; return c && rho ? al_store_io(c, c->al.st, mu, rho, false) : ILQR_ERR_ARG; }
int ilqr_hip_set_al_state_multipliers(ilqr_hip_ctx* c, const double* m, const double* rho) {
  double* const mu[2] = {const_cast<double*>(m), nullptr};
  return c ? al_store_io(c, c->al.st, mu, const_cast<double*>(rho), true) : ILQR_ERR_ARG;
}
int ilqr_hip_get_al_task_multipliers(ilqr_hip_ctx* c, double* m) { double* const mu[2] = {m, nullptr}; return c && m ? al_store_io(c, c->al.tk, mu, nullptr, false) : ILQR_ERR_ARG; }
int ilqr_hip_get_al_task_penalties(ilqr_hip_ctx* c, double* rho) { double* const mu[2] = {nullptr, nullptr}; return c && rho ? al_store_io(c, c->al.tk, mu, rho, false) : ILQR_ERR_ARG; }
int ilqr_hip_set_al_task_multipliers(ilqr_hip_ctx* c, const double* m, const double* rho) {
  double* const mu[2] = {const_cast<double*>(m), nullptr};
  return c ? al_store_io(c, c->al.tk, mu, const_cast<double*>(rho), true) : ILQR_ERR_ARG;
}
// ---- the observables of the update
__attribute__((minsize)) int ilqr_hip_get_al_violation(ilqr_hip_ctx* c, double* viol, int* done) {
  if (!c) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  enter(c);
  HIPCHK_S(c, hipStreamSynchronize(c->stream));
  if (viol) HIPCHK_S(c, hipMemcpy(viol, c->al.viol, (size_t)c->B * 2 * sizeof(double), hipMemcpyDeviceToHost));
  if (done) HIPCHK_S(c, hipMemcpy(done, c->al.done, (size_t)c->B * sizeof(int), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
__attribute__((noinline, minsize)) static int al_get_family_violation(ilqr_hip_ctx* c, const AlFamily& f, const double* dev, double* viol) {
  if (!viol) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  if (al_family_absent(c, f)) { std::fill(viol, viol + c->B, 0.0); return ILQR_OK; }
  enter(c);
  HIPCHK_S(c, hipStreamSynchronize(c->stream));
  HIPCHK_S(c, hipMemcpy(viol, dev, (size_t)c->B * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_get_al_state_violation(ilqr_hip_ctx* c, double* viol) { return c ? al_get_family_violation(c, c->al.st, c->al.sviol, viol) : ILQR_ERR_ARG; }
int ilqr_hip_get_al_task_violation(ilqr_hip_ctx* c, double* viol) { return c ? al_get_family_violation(c, c->al.tk, c->al.tviol, viol) : ILQR_ERR_ARG; }
// the trace of the last solve: `width` doubles per round and rollout
__attribute__((noinline, minsize)) static int al_get_trace(ilqr_hip_ctx* c, const double* trace, int width, double* out) {
  if (!c || !out) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  enter(c);
  HIPCHK_S(c, hipStreamSynchronize(c->stream));
  HIPCHK_S(c, hipMemcpy(out, trace, (size_t)c->al.rounds * c->B * width * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_get_al_trace(ilqr_hip_ctx* c, double* out) { return al_get_trace(c, c ? c->al.trace : nullptr, 5, out); }
int ilqr_hip_get_al_state_trace(ilqr_hip_ctx* c, double* out) { return al_get_trace(c, c ? c->al.strace : nullptr, 2, out); }
int ilqr_hip_get_al_task_trace(ilqr_hip_ctx* c, double* out) { return al_get_trace(c, c ? c->al.ttrace : nullptr, 2, out); }
// the nine task coordinates of the resident nominal trajectory, by the kernel the cost kernels and the update share their arithmetic with
// (velocities: the velocities of the same nine coordinates, by their kernel, through the same buffer)
__attribute__((noinline, minsize)) static int al_get_task_coords(ilqr_hip_ctx* c, double* out, bool velocities) {
  if (!c || !out) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  if (!c->initialized) return ILQR_ERR_STATE;
  enter(c);
  TRY(al_knot_ready(c));
  const size_t n = (size_t)c->B * (c->N + 1) * ILQR_AL_TASK_COORDS;
  if (!c->al.tpoints) TRY(dalloc(c, &c->al.tpoints, n));
  (velocities ? ilqr::g_al_knot.task_velocities : ilqr::g_al_knot.task_points)(&c->S, c->al.tpoints, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, c->al.tpoints, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_get_al_task_points(ilqr_hip_ctx* c, double* out) { return al_get_task_coords(c, out, false); }
int ilqr_hip_get_al_task_velocities(ilqr_hip_ctx* c, double* out) { return al_get_task_coords(c, out, true); }
static_assert(ILQR_AL_TASK_VEL_COORDS == ILQR_AL_TASK_COORDS && h1::ALV_COORDS == ILQR_AL_TASK_VEL_COORDS, "one buffer for both getters");
int ilqr_hip_al_update(ilqr_hip_ctx* c, int round) {
  if (!c || round < 0) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  if (round >= c->al.rounds) return ILQR_ERR_ARG;
  if (!c->initialized) return ILQR_ERR_STATE;
  enter(c);
  HIPCHK_S(c, hipMemsetAsync(c->al.left + round, 0, sizeof(int), c->stream));
  ilqr::launch_al_update(c->S, al_view(c), round, c->early_exit, c->stream);
  HIPCHK_S(c, hipGetLastError());
  HIPCHK_S(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}

// ---- the bounds tracks: the joint / torque and state parts (one row count) and the task part (a row count of its own); one body per
// operation, `task` naming the kind.  The start rows are shared
static const char* const AL_TRACK_STATE_ERR = "the track's state part needs an installed state family";
static const char* const AL_TRACK_TASK_ERR = "the task track needs an installed task family";
static const char* const AL_NO_TRACK_ERR = "no bounds track installed";
// (behind a synchronisation: a window kernel in flight still reads the track)
__attribute__((noinline, minsize)) static int al_track_free(ilqr_hip_ctx* c, bool task) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (AlFamily* f : {&c->al.jc, &c->al.st, &c->al.tk}) if ((f == &c->al.tk) == task) { if (f->track) hipFree(f->track); f->track = nullptr; }
  (task ? c->al.task_track_rows : c->al.track_rows) = 0;
  if (!c->al.track_rows && !c->al.task_track_rows) c->al.track_sets = 1;
  return ILQR_OK;
}
// part[3]: the joint / torque, state and task rows; the parts of the other kind are null
__attribute__((noinline, minsize)) static int al_track_install(ilqr_hip_ctx* c, int rows, const double* const part[3], bool task) {
  if (!c) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  AlFamily* const fam[3] = {&c->al.jc, &c->al.st, &c->al.tk};
  if (rows < 1 || (!part[0] && !part[1] && !part[2])) return ILQR_ERR_ARG;
  for (int i = 0; i < 3; ++i) if (part[i] && !al_bounds_ok(*fam[i], part[i], rows)) return ILQR_ERR_ARG;
  for (int i = 1; i < 3; ++i) if (part[i] && !fam[i]->sets) { c->err = i == 1 ? AL_TRACK_STATE_ERR : AL_TRACK_TASK_ERR; return ILQR_ERR_STATE; }
  enter(c);
  TRY(al_knot_ready(c));
  TRY(al_track_free(c, task));
  if (!c->al.track_start) TRY(dalloc(c, &c->al.track_start, (size_t)c->B));
  HIPCHK(c, hipMemsetAsync(c->al.track_start, 0, (size_t)c->B * sizeof(int), c->stream));      // one shared start of 0
  c->al.track_sets = 1;
  for (int i = 0; i < 3; ++i) if (part[i]) { TRY(dalloc(c, &fam[i]->track, (size_t)rows * fam[i]->width)); TRY(upload_rows(c, fam[i]->track, part[i], rows, fam[i]->fields, fam[i]->width)); }
  (task ? c->al.task_track_rows : c->al.track_rows) = rows;
  return ILQR_OK;
}
int ilqr_hip_set_al_bounds_track(ilqr_hip_ctx* c, int rows, const double* joint_ctrl, const double* state) {
  const double* const part[3] = {joint_ctrl, state, nullptr};
  return al_track_install(c, rows, part, false);
}
int ilqr_hip_set_al_task_bounds_track(ilqr_hip_ctx* c, int rows, const double* task) {
  const double* const part[3] = {nullptr, nullptr, task};
  return al_track_install(c, rows, part, true);
}
int ilqr_hip_clear_al_bounds_track(ilqr_hip_ctx* c) { return al_track_free(c, false); }
int ilqr_hip_clear_al_task_bounds_track(ilqr_hip_ctx* c) { return al_track_free(c, true); }
int ilqr_hip_al_bounds_track_rows(const ilqr_hip_ctx* c) { return c ? c->al.track_rows : -1; }
int ilqr_hip_al_task_bounds_track_rows(const ilqr_hip_ctx* c) { return c ? c->al.task_track_rows : -1; }
__attribute__((minsize)) int ilqr_hip_set_al_bounds_track_starts(ilqr_hip_ctx* c, const int* start, int n_sets) {
  if (!c || !start || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  for (int b = 0; b < n_sets; ++b) if (start[b] < 0) return ILQR_ERR_ARG;
  if (!c->al.track_rows && !c->al.task_track_rows) { c->err = AL_NO_TRACK_ERR; return ILQR_ERR_STATE; }
  enter(c);
  HIPCHK(c, hipMemcpyAsync(c->al.track_start, start, (size_t)n_sets * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->al.track_sets = n_sets;
  return ILQR_OK;
}
__attribute__((minsize)) int ilqr_hip_al_bounds_window_from_track(ilqr_hip_ctx* c, int step) {
  if (!c || step < 0) return ILQR_ERR_ARG;
  TRY(al_installed(c));
  if (!c->al.track_rows && !c->al.task_track_rows) { c->err = AL_NO_TRACK_ERR; return ILQR_ERR_STATE; }
  if (c->al.st.track && !c->al.st.sets) { c->err = AL_TRACK_STATE_ERR; return ILQR_ERR_STATE; }
  if (c->al.tk.track && !c->al.tk.sets) { c->err = AL_TRACK_TASK_ERR; return ILQR_ERR_STATE; }
  enter(c);
  const int n_sets = c->al.track_sets;
  const ilqr::AlBoundsTrackDev T{c->al.jc.track, c->al.st.track, c->al.track_rows, c->al.tk.track, c->al.task_track_rows};
  const ilqr::AlBoundsWindowDev W{c->al.jc.window, c->al.st.window, c->al.tk.window};
  ilqr::g_al_knot.window_from_track(&T, &W, c->al.track_start, n_sets, step, c->N, c->stream);
  HIPCHK(c, hipGetLastError());
  // the state the knot setters leave; the pointers move only where that state changes (the first cut, or other starts)
  bool same = c->P.alb_knot != 0;
  for (AlFamily* f : {&c->al.jc, &c->al.st, &c->al.tk}) if (f->track) { same = same && f->knot && f->sets == n_sets; f->knot = true; f->sets = n_sets; }
  return same ? ILQR_OK : al_point_bounds(c);      // asynchronous on the handle's stream
}

int ilqr_hip_set_contact_schedule(ilqr_hip_ctx* c, const int* stance, int n_sets) {
  if (!c || !stance || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  const size_t per = (size_t)(c->N + 1) * 2;
  HIPCHK(c, hipMemcpyAsync(c->d_stance, stance, per * n_sets * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->P.stance_stride = n_sets == 1 ? 0 : (long)per;
  c->xbar_rolled = false;      // (contact mode: the schedule is part of the dynamics)
  return ILQR_OK;
}
int ilqr_hip_set_ee_references(ilqr_hip_ctx* c, const double* ee_ref, const double* com_vel_ref, int n_sets) {
  if (!c || !ee_ref || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  const size_t per = (size_t)(c->N + 1);
  HIPCHK(c, hipMemcpyAsync(c->d_eeref, ee_ref, per * 6 * n_sets * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (com_vel_ref) HIPCHK(c, hipMemcpyAsync(c->d_comvelref, com_vel_ref, per * 3 * n_sets * sizeof(double), hipMemcpyHostToDevice, c->stream));
  else HIPCHK(c, hipMemsetAsync(c->d_comvelref, 0, per * 3 * n_sets * sizeof(double), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->P.ee_ref_stride = n_sets == 1 ? 0 : (long)(per * 6);
  c->P.com_vel_ref_stride = n_sets == 1 ? 0 : (long)(per * 3);
  return ILQR_OK;
}
int ilqr_hip_set_references(ilqr_hip_ctx* c, const double* x_ref, const double* u_ref, const double* com_ref, int n_sets) {
  if (!c || !x_ref || !u_ref || !com_ref || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  const size_t N = c->N;
  HIPCHK(c, hipMemcpyAsync(c->d_xref, x_ref, (N + 1) * ILQR_NX * n_sets * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_uref, u_ref, N * ILQR_NU * n_sets * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_comref, com_ref, (N + 1) * 3 * n_sets * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->P.x_ref_stride = n_sets == 1 ? 0 : (long)((N + 1) * ILQR_NX);
  c->P.u_ref_stride = n_sets == 1 ? 0 : (long)(N * ILQR_NU);
  c->P.com_ref_stride = n_sets == 1 ? 0 : (long)((N + 1) * 3);
  c->refs_set = true;
  return ILQR_OK;
}

// ---- reference windows from a track on the device (reference_track_kernels.hip)
static const size_t TRACK_ROW = ILQR_NX + ILQR_NU + 3 + 6 + 3;      // doubles per row of the track, all five arrays
static ilqr::TrackDev track_view(const ilqr_hip_ctx* c) {
  const size_t T = c->track_rows;
  ilqr::TrackDev t;
  t.x = c->d_track; t.u = t.x + T * ILQR_NX; t.com = t.u + T * ILQR_NU; t.ee = t.com + T * 3; t.com_vel = t.ee + T * 6;
  t.contact = c->track_contact_rows ? (const int*)(t.com_vel + T * 3) : nullptr;
  t.rows = c->track_rows; t.contact_rows = c->track_contact_rows;
  return t;
}
int ilqr_hip_set_reference_track(ilqr_hip_ctx* c, int rows, const double* x_ref, const double* u_ref, const double* com_ref, const double* ee_ref, const double* com_vel_ref,
                                 const int* contact, int contact_rows) {
  if (!c || rows < 1 || !x_ref || !com_ref || !ee_ref || contact_rows < 0) return ILQR_ERR_ARG;
  if (!contact) contact_rows = 0;
  enter(c);
  const size_t T = rows, nd = T * TRACK_ROW, bytes = nd * sizeof(double) + (size_t)contact_rows * 2 * sizeof(int);
  std::vector<double> host((bytes + sizeof(double) - 1) / sizeof(double), 0.0);      // (u_ref / com_vel_ref NULL: their rows stay zero)
  double* p = host.data();
  std::memcpy(p, x_ref, T * ILQR_NX * sizeof(double)); p += T * ILQR_NX;
  if (u_ref) std::memcpy(p, u_ref, T * ILQR_NU * sizeof(double));
  p += T * ILQR_NU;
  std::memcpy(p, com_ref, T * 3 * sizeof(double)); p += T * 3;
  std::memcpy(p, ee_ref, T * 6 * sizeof(double)); p += T * 6;
  if (com_vel_ref) std::memcpy(p, com_vel_ref, T * 3 * sizeof(double));
  p += T * 3;
  if (contact_rows) std::memcpy(p, contact, (size_t)contact_rows * 2 * sizeof(int));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (a window kernel in flight still reads the track this call replaces)
  if (c->d_track) { hipFree(c->d_track); c->d_track = nullptr; c->track_rows = c->track_contact_rows = 0; }
  if (!c->d_track_start) HIPCHK(c, hipMalloc((void**)&c->d_track_start, (size_t)c->B * sizeof(int)));
  HIPCHK(c, hipMalloc((void**)&c->d_track, host.size() * sizeof(double)));
  HIPCHK(c, hipMemcpyAsync(c->d_track, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->d_track_start, 0, (size_t)c->B * sizeof(int), c->stream));      // one shared start of 0
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->track_rows = rows; c->track_contact_rows = contact_rows; c->track_sets = 1; c->track_max_start = 0;
  return ILQR_OK;
}
int ilqr_hip_clear_reference_track(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (a window kernel in flight still reads it)
  if (c->d_track) hipFree(c->d_track);
  c->d_track = nullptr; c->track_rows = c->track_contact_rows = 0; c->track_sets = 1; c->track_max_start = 0;
  return ILQR_OK;
}
int ilqr_hip_reference_track_rows(const ilqr_hip_ctx* c) { return c ? c->track_rows : -1; }
int ilqr_hip_set_track_starts(ilqr_hip_ctx* c, const int* start, int n_sets) {
  if (!c || !start || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  int mx = 0;
  for (int b = 0; b < n_sets; ++b) { if (start[b] < 0) return ILQR_ERR_ARG; mx = start[b] > mx ? start[b] : mx; }
  if (!c->d_track) { c->err = "set_track_starts without a reference track (ilqr_hip_set_reference_track)"; return ILQR_ERR_STATE; }
  enter(c);
  HIPCHK(c, hipMemcpyAsync(c->d_track_start, start, (size_t)n_sets * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->track_sets = n_sets; c->track_max_start = mx;
  return ILQR_OK;
}
int ilqr_hip_window_from_track(ilqr_hip_ctx* c, int step, int follow_schedule) {
  if (!c || step < 0) return ILQR_ERR_ARG;
  if (!c->d_track) { c->err = "window_from_track without a reference track (ilqr_hip_set_reference_track)"; return ILQR_ERR_STATE; }
  // ee_ref / com_vel_ref have no end clamp (robot_utils.cpp:525-549 throws): the largest row any set would read, from the stored maximum start
  const long r_last = (follow_schedule ? (long)c->track_max_start + step : 0L) + c->N;
  if (r_last >= c->track_rows) {
    c->err = "window_from_track: foot / CoM-velocity reference row " + std::to_string(r_last) + " is beyond the track's " + std::to_string(c->track_rows) + " rows";
    return ILQR_ERR_ARG;
  }
  enter(c);
  const int n_sets = c->track_sets, sched_sets = follow_schedule ? n_sets : 1;
  const ilqr::WindowDev W{c->d_xref, c->d_uref, c->d_comref, c->d_eeref, c->d_comvelref, c->d_stance};
  ilqr::launch_window_from_track(track_view(c), W, c->d_track_start, n_sets, sched_sets, step, follow_schedule ? 1 : 0, c->N, c->stream);
  HIPCHK(c, hipGetLastError());
  const long n1 = c->N + 1, per = n_sets == 1 ? 0 : 1, sper = sched_sets == 1 ? 0 : 1;
  c->P.x_ref_stride = per * n1 * ILQR_NX; c->P.u_ref_stride = per * (long)c->N * ILQR_NU; c->P.com_ref_stride = per * n1 * 3;
  c->P.ee_ref_stride = sper * n1 * 6; c->P.com_vel_ref_stride = sper * n1 * 3; c->P.stance_stride = sper * n1 * 2;
  c->refs_set = true;
  c->xbar_rolled = false;      // (contact mode: the schedule is part of the dynamics)
  return ILQR_OK;      // asynchronous on the handle's stream
}
__attribute__((minsize)) int ilqr_hip_get_reference_windows(ilqr_hip_ctx* c, double* x_ref, double* u_ref, double* com_ref, double* ee_ref, double* com_vel_ref, int* stance) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t B = c->B, N = c->N;
  // one array: `per` elements per set; the device holds B sets (stride != 0) or one, the caller gets B
  auto fetch = [&](void* out, const void* dev, size_t per_bytes, long stride) -> hipError_t {
    if (!out) return hipSuccess;
    hipError_t e = hipMemcpy(out, dev, per_bytes * (stride ? B : 1), hipMemcpyDeviceToHost);
    if (e == hipSuccess && !stride) for (size_t b = 1; b < B; ++b) std::memcpy((char*)out + b * per_bytes, out, per_bytes);
    return e;
  };
  HIPCHK(c, fetch(x_ref, c->d_xref, (N + 1) * ILQR_NX * sizeof(double), c->P.x_ref_stride));
  HIPCHK(c, fetch(u_ref, c->d_uref, N * ILQR_NU * sizeof(double), c->P.u_ref_stride));
  HIPCHK(c, fetch(com_ref, c->d_comref, (N + 1) * 3 * sizeof(double), c->P.com_ref_stride));
  HIPCHK(c, fetch(ee_ref, c->d_eeref, (N + 1) * 6 * sizeof(double), c->P.ee_ref_stride));
  HIPCHK(c, fetch(com_vel_ref, c->d_comvelref, (N + 1) * 3 * sizeof(double), c->P.com_vel_ref_stride));
  HIPCHK(c, fetch(stance, c->d_stance, (N + 1) * 2 * sizeof(int), c->P.stance_stride));
  return ILQR_OK;
}

int ilqr_hip_set_regularization(ilqr_hip_ctx* c, double lambda) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  std::vector<double> lam(c->B, lambda);
  HIPCHK(c, hipMemcpyAsync(c->S.lambda, lam.data(), c->B * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_set_max_iterations(ilqr_hip_ctx* c, int max_iter) {
  if (!c || max_iter <= 0) return ILQR_ERR_ARG;
  enter(c);
  if (max_iter != c->max_iter) {
    hipFree(c->S.trace_cost); hipFree(c->S.trace_alpha); hipFree(c->S.trace_lambda); hipFree(c->S.order); hipFree(c->S.order_n);
    c->S.trace_cost = c->S.trace_alpha = c->S.trace_lambda = nullptr; c->S.order = c->S.order_n = nullptr;
    c->max_iter = max_iter; c->S.max_iter = max_iter;
    TRY(dalloc(c, &c->S.trace_cost, (size_t)c->B * (max_iter + 1))); TRY(dalloc(c, &c->S.trace_alpha, (size_t)c->B * max_iter)); TRY(dalloc(c, &c->S.trace_lambda, (size_t)c->B * max_iter));
    TRY(dalloc(c, &c->S.order, (size_t)c->B * 2 * (max_iter + 1))); TRY(dalloc(c, &c->S.order_n, 2 * (size_t)(max_iter + 1)));
    if (c->S.order_rn) hipFree(c->S.order_rn);
    if (c->S.order_an) hipFree(c->S.order_an);
    c->S.order_rn = c->S.order_an = nullptr;
    TRY(dalloc(c, &c->S.order_rn, (size_t)max_iter + 2)); TRY(dalloc(c, &c->S.order_an, (size_t)max_iter + 2));
    { void* cp[] = {c->S.chg, c->S.chg_n, c->S.chg_rn, c->S.chg_an}; for (void* p : cp) if (p) hipFree(p); }
    c->S.chg = c->S.chg_n = c->S.chg_rn = c->S.chg_an = nullptr; c->lin_iterations = 0;
    TRY(dalloc(c, &c->S.chg, (size_t)c->B * (max_iter + 1))); TRY(dalloc(c, &c->S.chg_n, (size_t)max_iter + 2)); TRY(dalloc(c, &c->S.chg_rn, (size_t)max_iter + 2)); TRY(dalloc(c, &c->S.chg_an, (size_t)max_iter + 2));
    { void* kp[] = {c->S.kr, c->S.kr_n, c->d_lgate}; for (void* p : kp) if (p) hipFree(p); }
    c->S.kr = c->S.kr_n = c->d_lgate = nullptr; c->record.clear();
    TRY(dalloc(c, &c->S.kr, (size_t)c->B * (max_iter + 1))); TRY(dalloc(c, &c->S.kr_n, (size_t)max_iter + 1)); TRY(dalloc(c, &c->d_lgate, 8 * (size_t)max_iter));
  }
  return ILQR_OK;
}
int ilqr_hip_set_tolerance(ilqr_hip_ctx* c, double tol) { if (!c) return ILQR_ERR_ARG; c->tol = tol; return ILQR_OK; }
int ilqr_hip_set_options(ilqr_hip_ctx* c, int jacobian_mode, double fd_eps, int early_exit) {
  if (!c || (jacobian_mode != ILQR_JAC_ANALYTIC && jacobian_mode != ILQR_JAC_FD_FORWARD) || !(fd_eps > 0.0)) return ILQR_ERR_ARG;
  c->jac_mode = jacobian_mode; c->fd_eps = fd_eps; c->early_exit = early_exit ? 1 : 0;
  return ILQR_OK;
}
int ilqr_hip_set_early_exit_gate(ilqr_hip_ctx* c, int on) { if (!c) return ILQR_ERR_ARG; c->ee_gate = on ? 1 : 0; return ILQR_OK; }

// ---------------------------------------------------------------- initializeWithReference
// Iteration 0 of a solve may re-roll a cold start BESIDE the linearisation only if it is the very kernel that rolled it out
// (LaunchPlan::rollout, kept in rolled_variant) under these very dynamics parameters (bit-identical result); compared field by field,
// not by memcmp (padding bytes).
static bool same_dyn(const h1::DynParams& a, const h1::DynParams& b) {
  return a.h == b.h && a.g[0] == b.g[0] && a.g[1] == b.g[1] && a.g[2] == b.g[2] && a.contact == b.contact && a.soft == b.soft && a.mu == b.mu && a.limits == b.limits && a.lim_k == b.lim_k;
}
static int cold_start_device(ilqr_hip_ctx* c, const double* x0_dev, const double* uinit_dev) {
  const size_t B = c->B, N = c->N;
  HIPCHK(c, hipMemcpyAsync(c->S.x0, x0_dev, B * ILQR_NX * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->S.ubar, uinit_dev, B * N * ILQR_NU * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  const ilqr::LaunchPlan L = plan_of(c);
  al_follow_initialize(c, c->N + 1);      // (ahead of the rollout: its cost is the augmented one)
  ilqr::launch_rollout(L, c->S, c->P, ilqr::MASK_ALL, 1, 0, c->S.Jbase, c->stream);  // N rollouts (ilqr.cpp:113-115)
  HIPCHK(c, hipGetLastError());
  c->initialized = true;
  c->xbar_rolled = true;
  c->rolled_variant = L.rollout; c->rolled_dyn = c->P.dyn;
  return ILQR_OK;
}
int ilqr_hip_initialize_device(ilqr_hip_ctx* c, const double* x0_device, const double* u_init_device) {
  if (!c || !x0_device || !u_init_device) return ILQR_ERR_ARG;
  TRY(enter_launching(c));
  return cold_start_device(c, x0_device, u_init_device);
}
int ilqr_hip_initialize(ilqr_hip_ctx* c, const double* x0, const double* u_init, const double* prev_xbar, const double* prev_ubar) {
  if (!c || !x0) return ILQR_ERR_ARG;
  TRY(enter_launching(c));
  const size_t B = c->B, N = c->N;
  if (prev_xbar && prev_ubar) {
    HIPCHK(c, hipMemcpyAsync(c->S.x0, x0, B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_prevx, prev_xbar, B * (N + 1) * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_prevu, prev_ubar, B * N * ILQR_NU * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ilqr::launch_warm_shift(c->S, c->d_prevx, c->d_prevu, c->stream);
    ilqr::launch_last_step(plan_of(c), c->S, c->P, c->stream);
    al_follow_initialize(c, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->initialized = true;
    c->xbar_rolled = false;
    return ILQR_OK;
  }
  std::vector<double> ug;
  const double* uh = u_init;
  if (!uh) {  // gravity compensation evaluated at each rollout's x0 (computeGravComp uses the plant state)
    ug.resize(B * N * ILQR_NU);
    for (size_t b = 0; b < B; ++b) {
      double u1[ILQR_NU]; h1host::gravity_compensation(x0 + b * ILQR_NX, c->P.dyn.g, u1);
      for (size_t t = 0; t < N; ++t) std::memcpy(&ug[(b * N + t) * ILQR_NU], u1, sizeof(u1));
    }
    uh = ug.data();
  }
  HIPCHK(c, hipMemcpyAsync(c->d_tmpx, x0, B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_tmpu, uh, B * N * ILQR_NU * sizeof(double), hipMemcpyHostToDevice, c->stream));
  TRY(cold_start_device(c, c->d_tmpx, c->d_tmpu));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_initialize_warm_resident(ilqr_hip_ctx* c, const double* x0) {
  if (!c || !x0) return ILQR_ERR_ARG;
  if (!c->initialized) return ILQR_ERR_STATE;
  TRY(enter_launching(c));
  const size_t B = c->B, N = c->N;
  HIPCHK(c, hipMemcpyAsync(c->S.x0, x0, B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_prevx, c->S.xbar, B * (N + 1) * ILQR_NX * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_prevu, c->S.ubar, B * N * ILQR_NU * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  ilqr::launch_warm_shift(c->S, c->d_prevx, c->d_prevu, c->stream);
  ilqr::launch_last_step(plan_of(c), c->S, c->P, c->stream);
  al_follow_initialize(c, 1);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->xbar_rolled = false;
  return ILQR_OK;
}
// the warm start shifted by `shift` knots on the resident solution (S.x0 already holds x0): copies, shift, tail re-roll -- enqueued
static int warm_shifted(ilqr_hip_ctx* c, int shift) {
  const size_t B = c->B, N = c->N;
  HIPCHK(c, hipMemcpyAsync(c->d_prevx, c->S.xbar, B * (N + 1) * ILQR_NX * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_prevu, c->S.ubar, B * N * ILQR_NU * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  ilqr::launch_warm_shift_m(c->S, c->d_prevx, c->d_prevu, shift, c->stream);
  ilqr::launch_warm_tail(plan_of(c), c->S, c->P, shift, c->stream);
  al_follow_initialize(c, shift);
  HIPCHK(c, hipGetLastError());
  c->xbar_rolled = false;
  return ILQR_OK;
}
int ilqr_hip_initialize_warm_resident_shifted(ilqr_hip_ctx* c, const double* x0, int shift) {
  if (!c || !x0 || shift < 1 || shift > c->N - 1) return ILQR_ERR_ARG;
  if (!c->initialized) return ILQR_ERR_STATE;
  TRY(enter_launching(c));
  HIPCHK(c, hipMemcpyAsync(c->S.x0, x0, (size_t)c->B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  TRY(warm_shifted(c, shift));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}

// ---------------------------------------------------------------- solve
static void collect_profile(ilqr_hip_ctx* c) {
  for (int i = 0; i < 8; ++i) { c->stage_ms[i] = 0; c->stage_launches[i] = 0; }
  for (auto& s : c->spans) { float ms = 0; hipEventElapsedTime(&ms, s.a, s.b); c->stage_ms[s.stage] += ms; c->stage_launches[s.stage] += 1; }
  c->spans.clear(); c->pool_next = 0;
}

static int slices_wanted(const ilqr_hip_ctx* c, int B) {
  int k = c->knobs.slices;
  if (k < 1) k = 1;
  if (k > 32) k = 32;
  while (k > 1 && B / k < 64) --k;   // a slice is at least one wave of the widest kernels
  return k;
}
// view of rollouts [b0, b0 + Bs) of the batch (every array is rollout-major)
static DevState slice_state(const DevState& S, size_t b0, int Bs) {
  DevState T = S;
  const size_t N = S.N, n = ILQR_NX, m = ILQR_NU, mi = S.max_iter;
  T.B = Bs;
  T.x0 += b0 * n; T.xbar += b0 * (N + 1) * n; T.ubar += b0 * N * m;
  T.xcand += b0 * 8 * (N + 1) * n; T.ucand += b0 * 8 * N * m; T.cand_cost += b0 * 8; T.cand_knot += b0 * 8 * (N + 1);
  T.A += b0 * N * n * n; T.Bm += b0 * N * n * m;
  T.lx += b0 * (N + 1) * n; T.lu += b0 * N * m; T.lxx += b0 * (N + 1) * n * n; T.luu += b0 * N * m;
  T.K += b0 * N * m * n; T.kff += b0 * N * m; T.lin_dump += b0 * N * ilqr::lin_dump_doubles();
  T.quad_knot0 = S.quad_knot0 + (long)(b0 * (N + 1));      // (the record buffer is indexed by knot, four to a line: not a pointer offset)
  T.Vx += b0 * n; T.Vxx += b0 * n * n;
  T.J += b0; T.Jbase += b0; T.ls_cost += b0; T.lambda += b0;
  T.active += b0; T.need_retry += b0; T.iters += b0; T.improved += b0; T.alpha_idx += b0;
  T.trace_cost += b0 * (mi + 1); T.trace_alpha += b0 * mi; T.trace_lambda += b0 * mi;
  T.order = nullptr; T.order_n = nullptr;      // the compacted lists index the whole batch: not used by slices
  T.grp_a = T.grp_r = T.order_r = T.order_rn = T.order_an = nullptr;
  T.chg = T.chg_n = T.chg_r = T.chg_rn = T.chg_an = nullptr; T.chg_f = nullptr;
  T.kr = T.kr_n = T.ls_list = T.ls_kind = nullptr;
  return T;
}
static h1::ProblemDev slice_problem(const h1::ProblemDev& P, long b0) {
  h1::ProblemDev T = P;
  T.x_ref += b0 * P.x_ref_stride; T.u_ref += b0 * P.u_ref_stride; T.com_ref += b0 * P.com_ref_stride;
  T.stance += b0 * P.stance_stride; T.ee_ref += b0 * P.ee_ref_stride; T.com_vel_ref += b0 * P.com_vel_ref_stride;
  if (P.wsets) T.wsets += b0 * P.wsets_stride;
  if (P.al) T.al += b0 * P.al_stride;
  if (P.alb) T.alb += b0 * P.alb_stride;
  if (P.alsb) { T.als += b0 * P.als_stride; T.alsb += b0 * P.alsb_stride; }
  if (P.altb) { T.alt += b0 * P.alt_stride; T.altb += b0 * P.altb_stride; }
  return T;
}
static int ensure_slices(ilqr_hip_ctx* c, int k) {
  if (!c->ev_begin) HIPCHK(c, hipEventCreateWithFlags(&c->ev_begin, hipEventDisableTiming));
  while ((int)c->slices.size() < k) {
    ilqr_hip_ctx::Slice sl;
    HIPCHK(c, hipStreamCreate(&sl.st)); HIPCHK(c, hipStreamCreate(&sl.st2)); HIPCHK(c, hipStreamCreate(&sl.st3));
    HIPCHK(c, hipEventCreateWithFlags(&sl.roll, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&sl.fork, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&sl.join, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&sl.lead, hipEventDisableTiming));
    c->slices.push_back(sl);
  }
  return ILQR_OK;
}
// a switch that the handle has a setting of its own for (`own`: its setter's value): the environment, when set, overrides it (diagnostics, tests)
static int effective(int knob, int own) { return knob >= 0 ? knob : own; }
static int early_exit_gate(const ilqr_hip_ctx* c) { return effective(c->knobs.ee_gate, c->ee_gate); }      // ilqr_hip_set_early_exit_gate
static int ensure_gate(ilqr_hip_ctx* c) {
  if ((int)c->ev_active.size() >= c->max_iter + 2 && c->h_active) return ILQR_OK;
  if (c->h_active) { (void)hipHostFree(c->h_active); c->h_active = nullptr; }
  HIPCHK(c, hipHostMalloc((void**)&c->h_active, sizeof(int) * (size_t)(c->max_iter + 2), hipHostMallocDefault));
  while ((int)c->ev_active.size() < c->max_iter + 2) { hipEvent_t e; HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->ev_active.push_back(e); }
  return ILQR_OK;
}
// The streams and events one launch sequence is enqueued on -- m: the sequence itself and the linearisation, q: cost quadratics (and the
// twin's passes of a side-by-side order), r: the nominal re-rollout and its adoption (lin / adopt: null where the adoption waits on m
// instead).  Values built from the fields of their owners (the handle, a slice): nothing changes hands.
struct Lanes { hipStream_t m, q, r; hipEvent_t fork, join, roll, lin, adopt; };
static Lanes main_lanes(const ilqr_hip_ctx* c) { return Lanes{c->stream, c->stream2, c->stream3, c->ev_fork, c->ev_join, c->ev_roll, c->ev_lin, c->ev_adopt}; }
static Lanes slice_lanes(const ilqr_hip_ctx::Slice& sl) { return Lanes{sl.st, sl.st2, sl.st3, sl.fork, sl.join, sl.roll, nullptr, nullptr}; }
// (group A's cost quadratics and re-rollout share the second and third stream with group R -- idle while the retry runs, and R's
// work comes behind A's anyway --, only its linearisation has a stream of its own: the runtime maps streams onto four hardware
// queues by default, and streams that share a queue serialise)
static Lanes group_a_lanes(const ilqr_hip_ctx* c, const Lanes& G) { return Lanes{c->a1, G.q, G.r, c->evA_fork, c->evA_join, c->evA_roll, c->evA_lin, c->evA_adopt}; }
// what solve_order.h decides from, for the view S of the batch enqueued on G: the effective switches, the sizes and which buffers exist
static ilqr::SolveSettings solve_settings(const ilqr_hip_ctx* c, const DevState& S, const Lanes& G) {
  const Knobs& k = c->knobs;
  ilqr::SolveSettings s{};
  s.early_exit = c->early_exit != 0; s.early_exit_gate = early_exit_gate(c) != 0; s.split = effective(k.split, c->early_exit) != 0;
  s.spec = k.spec != 0; s.spec_dual = k.spec_dual != 0; s.spec_max = k.spec_max;
  s.spec_lists = k.spec_lists != 0; s.listed_spec = c->listed_spec != 0; s.spec_list_max = k.spec_list_max; s.spec_list_from = k.spec_list_from;
  s.dedup = effective(k.dedup_retry, c->dedup_retry) != 0; s.relin = effective(k.relin, c->relin) != 0; s.repass = k.repass || c->repass;
  s.overlap_rollout = k.overlap_rollout != 0; s.reuse_rollout = effective(k.reuse_rollout, !c->reroll_nominal) != 0;
  s.max_iter = c->max_iter; s.B = S.B; s.slices = c->n_slices; s.analytic_jacobians = c->jac_mode == ILQR_JAC_ANALYTIC; s.first_aside = c->first_aside;
  s.lists = S.order != nullptr; s.chg = S.chg != nullptr; s.chg_f = S.chg_f != nullptr; s.kr = S.kr && S.kr_n;
  s.ls_list = S.ls_list != nullptr; s.ls_kind = S.ls_kind != nullptr; s.lgate = c->d_lgate != nullptr;
  s.grp_a = S.grp_a != nullptr; s.stream_a = c->a1 != nullptr; s.adopt_events = G.lin && G.adopt; s.twin = c->twin;
  return s;
}
// The shadow buffer of the re-rollout beside the region, 0.01 MB per rollout at N = 25 (43 MB at B = 4096, 344 MB at B = 32 768): allocated by
// the first solve any iteration or round of which re-rolls aside (first_aside: rounds >= 2 of an augmented-Lagrangian solve set it), as the
// twin below.  A handle that never re-rolls never holds it.  Unlike the twin it is what the caller asked for: failing to get it fails the solve.
static int ensure_shadow(ilqr_hip_ctx* c, const ilqr::LaunchPlan& L) {
  if (c->d_shadowx) return ILQR_OK;
  ilqr::SolveSettings s = solve_settings(c, c->S, main_lanes(c));
  s.first_aside = true;
  const ilqr::SolveOrder O = ilqr::resolve_solve_order(s, L);
  if (ilqr::nominal_roll(O, L, 0) != ilqr::ROLL_ASIDE && ilqr::nominal_roll(O, L, 1) != ilqr::ROLL_ASIDE) return ILQR_OK;
  return dalloc(c, &c->d_shadowx, (size_t)c->B * (c->N + 1) * ILQR_NX);
}
static int alloc_twin(ilqr_hip_ctx* c);
// (the side-by-side order is an optimisation: a handle that cannot get the memory keeps the sequential order instead of failing the solve)
// Memory: the twin is indexed by rollout like everything else, so it is a full-batch copy of K, k, Vx, Vxx, the eight candidates and
// their knot costs -- 0.33 MB per rollout at N = 25 (1.3 GB at B = 4096, 10.7 GB at B = 32 768), allocated by the first solve that can
// take the side-by-side order: B <= ILQR_SPEC_MAX, or the convergence exit with its gate on (the late passes of any batch shrink below
// the threshold).  ILQR_SPEC=0 keeps a handle from ever allocating it.
static int ensure_twin(ilqr_hip_ctx* c) {
  if (c->twin || c->twin_failed) return ILQR_OK;
  if (alloc_twin(c) != ILQR_OK) {
    void* tw[] = {c->T.K, c->T.kff, c->T.Vx, c->T.Vxx, c->T.xcand, c->T.ucand, c->T.cand_cost, c->T.cand_knot, c->T.lambda, c->d_spec_gate};
    for (void* p : tw) if (p) (void)hipFree(p);
    c->T = DevState{}; c->d_spec_gate = nullptr; c->twin = false; c->twin_failed = true;
    (void)hipGetLastError();
    c->err.clear();      // (the failed allocation is not an error of the call: the sequential order runs instead)
  }
  return ILQR_OK;
}
static int alloc_twin(ilqr_hip_ctx* c) {
  const size_t B = c->B, N = c->N, n = ILQR_NX, m = ILQR_NU;
  DevState& T = c->T;
  T = c->S;
  T.K = T.kff = T.Vx = T.Vxx = T.xcand = T.ucand = T.cand_cost = T.cand_knot = T.lambda = nullptr;
  c->twin = true;       // (from here on destroy frees whatever was allocated)
  TRY(dalloc(c, &T.K, B * N * m * n + 32)); TRY(dalloc(c, &T.kff, B * N * m)); TRY(dalloc(c, &T.Vx, B * n)); TRY(dalloc(c, &T.Vxx, B * n * n));
  TRY(dalloc(c, &T.xcand, B * 8 * (N + 1) * n)); TRY(dalloc(c, &T.ucand, B * 8 * N * m)); TRY(dalloc(c, &T.cand_cost, B * 8)); TRY(dalloc(c, &T.cand_knot, B * 8 * (N + 1)));
  TRY(dalloc(c, &T.lambda, B));
  TRY(dalloc(c, &c->d_spec_gate, 4));
  if (!c->ev_spec_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_spec_fork, hipEventDisableTiming));
  if (!c->ev_spec_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_spec_join, hipEventDisableTiming));
  return ILQR_OK;
}
// the twin view of (a slice of) the batch: everything of S, with the twin's own gains, value function, candidates and lambda
static DevState twin_view(const ilqr_hip_ctx* c, const DevState& S) {
  DevState T = S;
  const DevState& W = c->T; const DevState& F = c->S;
  T.K = W.K + (S.K - F.K); T.kff = W.kff + (S.kff - F.kff); T.Vx = W.Vx + (S.Vx - F.Vx); T.Vxx = W.Vxx + (S.Vxx - F.Vxx);
  T.xcand = W.xcand + (S.xcand - F.xcand); T.ucand = W.ucand + (S.ucand - F.ucand); T.cand_cost = W.cand_cost + (S.cand_cost - F.cand_cost);
  T.cand_knot = W.cand_knot + (S.cand_knot - F.cand_knot); T.lambda = W.lambda + (S.lambda - F.lambda);
  return T;
}
// What the functions that enqueue one solve share: the handle, the view of the batch and its problem data, the plan and the order resolved
// for them, the lanes, and the iteration at hand.
struct SolveCtx {
  ilqr_hip_ctx* c;
  const DevState& S;
  const h1::ProblemDev& P;
  ilqr::LaunchPlan L;       // (the per-call re-read happened in the caller's prologue: the plan cannot change under a solve)
  ilqr::SolveOrder O;
  Lanes G, GA;              // the solve's own lanes (group R's where an iteration runs in two groups) and group A's
  hipEvent_t lead;
  double* shadow;           // target of the concurrent re-rollout: same rollouts as S.xbar, in the shadow buffer
  int* stance_dyn;          // (same rollouts as S)
  // step size h while launch_linearize writes Jacobians whose hinge-position rows are exactly e_k + h * the hinge-velocity rows (the
  // analytic tangent kernels, lin_column) and the backward kernel uses that (riccati_wave.hip fold_rows); else 0
  double fold_h;
  DevState Tw;              // the twin view of S (S itself while the handle has no twin: no order reads it then)
  // ---- the iteration at hand
  int iter;
  int ls_bound;             // with the gate the host has seen how many rollouts were still active at the start of iteration iter - 1: an upper
                            // bound for this iteration's passes -- the active set only shrinks; else -1
  bool adopt_aside;         // the re-rolled trajectory is adopted on G.r, beside the backward pass
  bool a_adopts;            // ... and group A's on GA.r: the regions of iterations >= 1 re-roll aside (one answer per solve, solve_order.h nominal_roll)
  bool prev_split;          // group A of the iteration at hand is already enqueued
};
// One group's share of the concurrent region of an iteration -- linearisation (:576) on G.m, cost quadratics (:588) on G.q, and where
// roll is ROLL_ASIDE the nominal re-rollout (:551,563) into the shadow buffer and its adoption on G.r (solve_order.h nominal_roll) --
// behind an event recorded on fork_src.  G.lin is recorded behind the linearisation wherever somebody waits for it: the adoption, or the
// solve's own stream for a group whose linearisation runs on a stream of its own (group A).
// Sm: the view the mask-selected kernels (rollout, trajectory cost, adoption) get -- S, or S with a group's flags as `active`;
// wl: the group's compacted list for the per-knot kernels (null: the iteration's own list / mask, as knot_mode and iter_l say).
static int enqueue_region(const SolveCtx& X, const Lanes& G, hipStream_t fork_src, const DevState& Sm, int knot_mode, int iter_l, const ilqr::WorkList* wl, ilqr::NominalRoll roll) {
  ilqr_hip_ctx* c = X.c;
  const bool concurrent_roll = roll == ilqr::ROLL_ASIDE;
  HIPCHK(c, hipEventRecord(G.fork, fork_src));
  if (G.m != fork_src) HIPCHK(c, hipStreamWaitEvent(G.m, G.fork, 0));
  HIPCHK(c, hipStreamWaitEvent(G.q, G.fork, 0));
  if (concurrent_roll) {
    HIPCHK(c, hipStreamWaitEvent(G.r, G.fork, 0));
    DevState Sr = Sm; Sr.xbar = X.shadow;
    { StageTimer T(c, 0, G.r); ilqr::launch_rollout(X.L, Sr, X.P, ilqr::MASK_ACTIVE, 1, 0, X.S.Jbase, G.r); }
    c->nominal_rollouts += Sr.B;
    HIPCHK(c, hipEventRecord(G.roll, G.r));
  }
  { StageTimer T(c, 2, G.q); ilqr::launch_cost_quadratics(X.S, X.P, knot_mode, G.q, iter_l, X.L.lxx_layout, wl); }
  HIPCHK(c, hipEventRecord(G.join, G.q));
  { StageTimer T(c, 1, G.m); ilqr::launch_linearize(X.L, X.S, X.P, knot_mode, c->fd_eps, G.m, 3, iter_l, X.L.pack ? 1 : 0, wl, X.stance_dyn); }
  const bool adopt_aside = concurrent_roll && G.lin && G.adopt;
  if (G.lin && (adopt_aside || G.m != fork_src)) HIPCHK(c, hipEventRecord(G.lin, G.m));
  if (adopt_aside) {
    HIPCHK(c, hipStreamWaitEvent(G.r, G.lin, 0)); HIPCHK(c, hipStreamWaitEvent(G.r, G.join, 0));
    ilqr::launch_adopt_rollout(Sm, X.shadow, ilqr::MASK_ACTIVE, c->d_mismatch, G.r);
    HIPCHK(c, hipEventRecord(G.adopt, G.r));
  }
  return ILQR_OK;
}
// t goes on only behind the adoption of the re-rolled trajectory (the line search reads it; the backward pass does not)
static int wait_adoption(const SolveCtx& X, hipStream_t t) {
  if (X.adopt_aside) HIPCHK(X.c, hipStreamWaitEvent(t, X.G.adopt, 0));
  if (X.prev_split && X.a_adopts) HIPCHK(X.c, hipStreamWaitEvent(t, X.GA.adopt, 0));
  return ILQR_OK;
}
// a side-by-side pass: the second stream starts behind what G.m holds so far, and G.m goes on behind what the second stream was given
static int fork_second(const SolveCtx& X) {
  HIPCHK(X.c, hipEventRecord(X.c->ev_spec_fork, X.G.m));
  HIPCHK(X.c, hipStreamWaitEvent(X.G.q, X.c->ev_spec_fork, 0));
  return ILQR_OK;
}
static int join_second(const SolveCtx& X) {
  HIPCHK(X.c, hipEventRecord(X.c->ev_spec_join, X.G.q));
  HIPCHK(X.c, hipStreamWaitEvent(X.G.m, X.c->ev_spec_join, 0));
  return ILQR_OK;
}
// with the gate: the count of rollouts still active behind this iteration travels to the host (SolveOrder::gate)
static int publish_active(const SolveCtx& X) {
  if (!X.O.gate) return ILQR_OK;
  HIPCHK(X.c, hipMemcpyAsync(&X.c->h_active[X.iter + 1], X.S.order_n + 2 * (X.iter + 1), sizeof(int), hipMemcpyDeviceToHost, X.G.m));
  HIPCHK(X.c, hipEventRecord(X.c->ev_active[X.iter], X.G.m));
  return ILQR_OK;
}
// ORDER_TWIN: both passes of ilqr.cpp:601-646 side by side (k_control_spec), the twin on the second stream
static int enqueue_twin_iteration(const SolveCtx& X) {
  ilqr_hip_ctx* c = X.c; const DevState& S = X.S; const DevState& Tw = X.Tw;
  const hipStream_t st = X.G.m, st2 = X.G.q;
  ++c->spec_iterations;
  TRY(fork_second(X));
  ilqr::launch_spec_lambda(S, Tw.lambda, st2);
  { StageTimer T(c, 3, st); ilqr::launch_backward(X.L, S, ilqr::MASK_ACTIVE, st, X.fold_h, X.iter); }
  { StageTimer T(c, 6, st2); ilqr::launch_backward(X.L, Tw, ilqr::MASK_ACTIVE, st2, X.fold_h, X.iter); }
  TRY(wait_adoption(X, st)); TRY(wait_adoption(X, st2));
  if (X.iter == 0 && X.lead) HIPCHK(c, hipEventRecord(X.lead, st));
  { StageTimer T(c, 4, st); ilqr::launch_line_search(X.L, S, X.P, ilqr::MASK_ACTIVE, st, X.iter, X.ls_bound); }
  { StageTimer T(c, 7, st2); ilqr::launch_line_search(X.L, Tw, X.P, ilqr::MASK_ACTIVE, st2, X.iter, X.ls_bound); }
  TRY(join_second(X));
  { StageTimer T(c, 5, st); ilqr::launch_control_spec(S, Tw, X.iter, c->tol, c->early_exit, st, X.L.ls_costs_per_knot); }
  return publish_active(X);
}
// ORDER_DUAL: both orders are enqueued and the device takes one (SolveOrder::dual_order)
static int enqueue_dual_iteration(const SolveCtx& X) {
  ilqr_hip_ctx* c = X.c; const DevState& S = X.S; const DevState& Tw = X.Tw;
  const hipStream_t st = X.G.m, st2 = X.G.q;
  const int iter = X.iter, spec_max = X.O.spec_max;
  const int* list = S.order + (size_t)(2 * iter) * S.B;
  int* g = c->d_spec_gate;
  ++c->spec_iterations;
  ilqr::launch_spec_gate(S, iter, spec_max, g, st);
  TRY(fork_second(X));
  ilqr::launch_spec_lambda(S, Tw.lambda, st2);
  { StageTimer T(c, 3, st); ilqr::launch_backward(X.L, S, ilqr::MASK_ACTIVE, st, X.fold_h, iter); }
  { StageTimer T(c, 6, st2); ilqr::launch_backward_list(X.L, Tw, st2, X.fold_h, list, g); }
  TRY(wait_adoption(X, st)); TRY(wait_adoption(X, st2));
  { StageTimer T(c, 4, st);
    ilqr::launch_line_search_list(S, X.P, st, list, g, spec_max);
    ilqr::launch_line_search_list(S, X.P, st, list, g + 2, X.ls_bound);
    ilqr::launch_cand_costs(S, X.P, ilqr::MASK_ACTIVE, st, false); }
  { StageTimer T(c, 7, st2); ilqr::launch_line_search_list(Tw, X.P, st2, list, g, spec_max); ilqr::launch_cand_costs(Tw, X.P, ilqr::MASK_ACTIVE, st2, false, g); }
  TRY(join_second(X));
  { StageTimer T(c, 5, st);
    ilqr::launch_control_spec(S, Tw, iter, c->tol, c->early_exit, st, X.L.ls_costs_per_knot, g);
    ilqr::launch_control(S, 0, iter, c->tol, c->early_exit | X.O.dedup_bit, st, X.L.ls_costs_per_knot, g + 1); }
  { StageTimer T(c, 6, st); ilqr::launch_backward(X.L, S, ilqr::MASK_RETRY, st, X.fold_h, iter); }
  { StageTimer T(c, 7, st); ilqr::launch_line_search(X.L, S, X.P, ilqr::MASK_RETRY, st, iter, X.ls_bound); }
  { StageTimer T(c, 5, st); ilqr::launch_control(S, 1, iter, c->tol, c->early_exit, st, X.L.ls_costs_per_knot); }
  return publish_active(X);
}
// The listed side-by-side order in front of the sequential one (SolveOrder::listed): the twin runs the first pass of the changed rollouts
// (wf, the iteration's chg list), the solve's own buffers the known retries.  The sequential order behind it sees an empty first-pass list
// (wf->count) and closed gates (*gseq: the gate of its bookkeeping) where the device took this order -- its retry list stays empty: nobody
// ran phase 0.
static int enqueue_listed_pair(const SolveCtx& X, ilqr::WorkList* wf, const int** gseq) {
  ilqr_hip_ctx* c = X.c; const DevState& S = X.S; const DevState& Tw = X.Tw;
  const hipStream_t st = X.G.m, st2 = X.G.q;
  int* g = c->d_lgate + 8 * (size_t)X.iter;
  const int slots = c->knobs.spec_list_max < S.B ? c->knobs.spec_list_max : S.B;      // (either list holds at most this many rollouts where the order is taken)
  DevState Su = S; Su.active = S.ls_kind;       // the candidates' knot costs select by mask: chg and kr as flags on S, chg on the twin
  DevState Tf = Tw; Tf.active = S.chg_f;
  ilqr::launch_listed_prologue(S, Tw.lambda, X.iter, c->knobs.spec_list_max, g, st);
  TRY(fork_second(X));
  { StageTimer T(c, 3, st); ilqr::launch_backward_list(X.L, S, st, X.fold_h, S.ls_list, g + 3); }
  { StageTimer T(c, 6, st2); ilqr::launch_backward_list(X.L, Tw, st2, X.fold_h, wf->list, g); }
  TRY(wait_adoption(X, st)); TRY(wait_adoption(X, st2));
  { StageTimer T(c, 4, st); ilqr::launch_line_search_s(S, X.P, ilqr::MASK_ACTIVE, st, S.ls_list, g + 3, slots, 1); ilqr::launch_cand_costs(Su, X.P, ilqr::MASK_ACTIVE, st, false, g + 4); }
  { StageTimer T(c, 7, st2); ilqr::launch_line_search_s(Tw, X.P, ilqr::MASK_ACTIVE, st2, wf->list, g, slots, 1); ilqr::launch_cand_costs(Tf, X.P, ilqr::MASK_ACTIVE, st2, false, g + 4); }
  TRY(join_second(X));
  { StageTimer T(c, 5, st); ilqr::launch_control_listed(S, Tw, X.iter, st, X.L.ls_costs_per_knot, g); }
  wf->count = g + 2; *gseq = g + 1;
  return ILQR_OK;
}
// ORDER_SEQUENTIAL: first pass (:601-620), lambda retry (:637-646); with or without lists, behind the listed pair where ord.pair.
// *split_next: group A of the next iteration has been enqueued behind the first control pass (SolveOrder::can_split)
static int enqueue_sequential_iteration(const SolveCtx& X, const ilqr::IterationOrder& ord, bool* split_next) {
  ilqr_hip_ctx* c = X.c; const DevState& S = X.S; const h1::ProblemDev& P = X.P; const ilqr::LaunchPlan& L = X.L;
  const hipStream_t st = X.G.m;
  const int iter = X.iter, ls_bound = X.ls_bound;
  ilqr::WorkList wf{S.chg + (size_t)iter * S.B, S.chg_n + iter};
  const int* gseq = nullptr;
  if (ord.pair) TRY(enqueue_listed_pair(X, &wf, &gseq));
  { StageTimer T(c, 3, st);                                                                                              // :601
    if (ord.first_listed) ilqr::launch_backward_list(L, S, st, X.fold_h, wf.list, wf.count);
    else ilqr::launch_backward(L, S, ilqr::MASK_ACTIVE, st, X.fold_h, iter); }
  TRY(wait_adoption(X, st));
  if (iter == 0 && X.lead) HIPCHK(c, hipEventRecord(X.lead, st));
  { StageTimer T(c, 4, st);                                                                                              // :616
    if (ord.first_listed) {
      DevState Sf = S; Sf.active = S.chg_f;      // (the candidates' knot costs select by mask: the list as flags; every other rollout's cand_knot stays)
      ilqr::launch_line_search_gated(S, P, st, wf.list, wf.count, c->knobs.ls_list_max, ls_bound, c->d_fp_gate);
      ilqr::launch_cand_costs(Sf, P, ilqr::MASK_ACTIVE, st, false, gseq);
    } else ilqr::launch_line_search(L, S, P, ilqr::MASK_ACTIVE, st, iter, ls_bound); }
  { StageTimer T(c, 5, st); ilqr::launch_control(S, 0, iter, c->tol, c->early_exit | X.O.dedup_bit, st, L.ls_costs_per_knot, gseq); }      // :619-620,645-655
  *split_next = ilqr::splits_next(X.O, L, iter, c->max_iter);
  if (*split_next) {
    // group A of iteration iter + 1: the first entries of its list, as many as the first control pass has just put there
    HIPCHK(c, hipMemcpyAsync(S.order_an + iter + 1, S.order_n + 2 * (iter + 1), sizeof(int), hipMemcpyDeviceToDevice, st));
    DevState Sg = S; Sg.active = S.grp_a;
    if (X.O.cache) HIPCHK(c, hipMemcpyAsync(S.chg_an + iter + 1, S.chg_n + iter + 1, sizeof(int), hipMemcpyDeviceToDevice, st));
    const ilqr::WorkList wa = X.O.cache ? ilqr::WorkList{S.chg + (size_t)(iter + 1) * S.B, S.chg_an + iter + 1} : ilqr::WorkList{S.order + (size_t)(2 * (iter + 1)) * S.B, S.order_an + iter + 1};
    TRY(enqueue_region(X, X.GA, st, Sg, ilqr::MASK_ACTIVE, -1, &wa, ilqr::nominal_roll(X.O, L, iter + 1)));
  }
  { StageTimer T(c, 6, st); ilqr::launch_backward(L, S, ilqr::MASK_RETRY, st, X.fold_h, iter); }                                // :637
  { StageTimer T(c, 7, st);                                                                                              // :638
    if (X.O.retry_gated) {
      const ilqr::WorkList wr = ilqr::work_list(S, ilqr::MASK_RETRY, iter);
      ilqr::launch_line_search_gated(S, P, st, wr.list, wr.count, c->knobs.ls_list_max, ls_bound, c->d_fp_gate + 2);
      ilqr::launch_cand_costs(S, P, ilqr::MASK_RETRY, st, false, gseq);
    } else ilqr::launch_line_search(L, S, P, ilqr::MASK_RETRY, st, iter, ls_bound); }
  { StageTimer T(c, 5, st); ilqr::launch_control(S, 1, iter, c->tol, c->early_exit, st, L.ls_costs_per_knot, gseq); }                    // :640-646
  return publish_active(X);
}
// the launch sequence of iLQR::solve (ilqr.cpp:521-660) for one slice on its streams; `wait_lead` (optional) delays the
// first throughput-bound stage until the previous slice has finished its first backward pass, `lead` is recorded there.
// Which order each iteration takes is decided in solve_order.h; every order has a function of its own above.
static int enqueue_solve(ilqr_hip_ctx* c, const DevState& S, const h1::ProblemDev& P, const Lanes& G, hipEvent_t wait_lead, hipEvent_t lead) {
  const hipStream_t st = G.m;
  const ilqr::LaunchPlan L = plan_of(c);
  const ilqr::SolveOrder O = ilqr::resolve_solve_order(solve_settings(c, S, G), L);
  SolveCtx X{c, S, P, L, O, G, group_a_lanes(c, G), lead,
             c->d_shadowx ? c->d_shadowx + (S.xbar - c->S.xbar) : nullptr, c->d_stance_dyn + (S.xbar - c->S.xbar) / ((long)(c->N + 1) * ILQR_NX) * 2L * c->N,
             L.folds_h ? P.dyn.h : 0.0, c->twin ? twin_view(c, S) : S, 0, -1, false, ilqr::nominal_roll(O, L, 1) == ilqr::ROLL_ASIDE, false};
  { StageTimer T(c, 0, st); ilqr::launch_rollout(L, S, P, ilqr::MASK_ALL, 0, 0, S.Jbase, st);
    // (rounds >= 2 of an augmented-Lagrangian solve with the convergence exit: the rollouts that are done enter inactive)
    if (P.al && c->al.round > 0 && c->early_exit) ilqr::launch_solve_begin_al(S, c->al.done + (S.active - c->S.active), st);
    else ilqr::launch_solve_begin(S, st); }  // ilqr.cpp:540
  // the operand-layout Riccati kernel (analytic Jacobians, riccati_pack.hip) has its producers write A_t, B_t and lxx~_t in its own
  // layout; the generic one-wave kernel reads only the tiles I >= J of lxx_t (t < N): the cost quadratics then leave the others unwritten
  // (iteration 0 rewrites A_t, B_t, lxx_t of every rollout: a solve leaves one layout behind; ilqr_hip_solve_async has prepared the padding)
  c->lxx_layout = L.lxx_layout;
  c->ab_packed = L.pack;
  c->lin_fold_h = X.fold_h;      // what S.A / S.Bm hold after this solve; assigned with the layout flags (an early return above leaves all of them alone)
  if (L.pack) c->packed_h = X.fold_h;
  if (!L.pack) c->ab_pads_clean = false;
  if (O.gate) TRY(ensure_gate(c));
  c->iterations_enqueued = c->max_iter;
  c->lin_cached = O.cache; c->lin_listed = O.lin_listed;
  c->record.assign((size_t)c->max_iter, ilqr::IterationRecord{ilqr::ORDER_SEQUENTIAL, false, false});
  const int sel_mode = O.sel_active ? ilqr::MASK_ACTIVE : ilqr::MASK_ALL;
  bool prev_seq = false;        // the previous iteration ran in the sequential order (k_control has written chg_f for this one)
  for (int iter = 0; iter < c->max_iter; ++iter) {
    if (O.gate && iter >= 2) {
      HIPCHK(c, hipEventSynchronize(c->ev_active[iter - 2]));
      if (c->h_active[iter - 1] == 0) { c->iterations_enqueued = iter; break; }     // nobody was active in iteration iter - 1
    }
    X.iter = iter;
    X.ls_bound = (O.gate && iter >= 2) ? c->h_active[iter - 1] : -1;
    const ilqr::NominalRoll roll = ilqr::nominal_roll(O, L, iter);
    const bool concurrent_roll = roll == ilqr::ROLL_ASIDE;
    if (!X.prev_split) {
      if (roll == ilqr::ROLL_BEFORE) { StageTimer T(c, 0, st); ilqr::launch_rollout(L, S, P, ilqr::MASK_ACTIVE, 1, 0, S.Jbase, st); c->nominal_rollouts += S.B; }
      if (iter == 0 && wait_lead) HIPCHK(c, hipStreamWaitEvent(st, wait_lead, 0));
      const ilqr::WorkList wc{S.chg + (size_t)iter * S.B, S.chg_n + iter};
      TRY(enqueue_region(X, G, st, S, sel_mode, iter, (O.cache && iter > 0) ? &wc : nullptr, roll));
    } else {
      DevState Sg = S; Sg.active = S.grp_r;      // (the mask-selected kernels: every rollout of the group, changed or not)
      const ilqr::WorkList wr = O.cache ? ilqr::WorkList{S.chg_r, S.chg_rn + iter} : ilqr::WorkList{S.order_r, S.order_rn + iter};
      TRY(enqueue_region(X, G, st, Sg, ilqr::MASK_ACTIVE, -1, &wr, roll));      // (ROLL_ASIDE or ROLL_NONE: solve_order.h splits_next)
      ++c->split_iterations;
    }
    X.adopt_aside = concurrent_roll && G.lin && G.adopt;
    HIPCHK(c, hipStreamWaitEvent(st, G.join, 0));
    if (X.prev_split) { HIPCHK(c, hipStreamWaitEvent(st, X.GA.join, 0)); HIPCHK(c, hipStreamWaitEvent(st, X.GA.lin, 0)); }
    if (concurrent_roll && !X.adopt_aside) { HIPCHK(c, hipStreamWaitEvent(st, G.roll, 0)); ilqr::launch_adopt_rollout(S, X.shadow, ilqr::MASK_ACTIVE, c->d_mismatch, st); }
    const ilqr::IterationOrder ord = ilqr::iteration_order(O, iter, X.ls_bound >= 0 ? X.ls_bound : S.B, prev_seq);
    bool split_next = false;
    switch (ord.kind) {
      case ilqr::ORDER_TWIN: TRY(enqueue_twin_iteration(X)); break;
      case ilqr::ORDER_DUAL: TRY(enqueue_dual_iteration(X)); break;
      case ilqr::ORDER_SEQUENTIAL: TRY(enqueue_sequential_iteration(X, ord, &split_next)); break;
    }
    c->record[iter] = ord;
    X.prev_split = split_next; prev_seq = ord.kind == ilqr::ORDER_SEQUENTIAL;
  }
  if (X.prev_split) {      // (the convergence exit ended the loop behind a group A that found nothing to do: its streams rejoin)
    HIPCHK(c, hipStreamWaitEvent(st, X.GA.join, 0)); HIPCHK(c, hipStreamWaitEvent(st, X.GA.lin, 0));
    if (X.a_adopts) HIPCHK(c, hipStreamWaitEvent(st, X.GA.adopt, 0));
  }
  c->lin_iterations = c->iterations_enqueued;
  return ILQR_OK;
}
int ilqr_hip_set_relinearize_unchanged(ilqr_hip_ctx* c, int on) { if (!c) return ILQR_ERR_ARG; c->relin = on ? 1 : 0; return ILQR_OK; }
int ilqr_hip_set_repeat_first_pass(ilqr_hip_ctx* c, int on) { if (!c) return ILQR_ERR_ARG; c->repass = on ? 1 : 0; return ILQR_OK; }
int ilqr_hip_set_listed_spec(ilqr_hip_ctx* c, int on) { if (!c) return ILQR_ERR_ARG; c->listed_spec = on ? 1 : 0; return ILQR_OK; }
int ilqr_hip_set_reroll_nominal(ilqr_hip_ctx* c, int on) { if (!c) return ILQR_ERR_ARG; c->reroll_nominal = on ? 1 : 0; return ILQR_OK; }
long long ilqr_hip_get_nominal_rollouts(const ilqr_hip_ctx* c) { return c ? c->nominal_rollouts : -1; }
// What the lists of the last solve held, iteration by iteration, read ONCE behind the handle's stream for the getters below: act[2 it] /
// act[2 it + 1] the rollouts active at the start of iteration it / in its lambda retry (DevState::order_n), chg[it] and kr[it] the lengths of
// its chg and kr lists, took[it] = 1 where it enqueued the listed pair and the device took the side-by-side order (word 4 of its gate
// words).  A buffer the handle does not hold reads as zeros.  On failure "<who>: reading <what> failed" is the handle's error.
struct IterationCounts { std::vector<int> act, chg, kr, took; };
static int read_iteration_counts(ilqr_hip_ctx* c, const char* who, const char* what, IterationCounts* n) {
  const size_t mi = (size_t)c->max_iter;
  n->act.assign(2 * (mi + 1), 0); n->chg.assign(mi + 1, 0); n->kr.assign(mi + 1, 0); n->took.assign(mi, 0);
  std::vector<int> g(c->d_lgate ? 8 * mi : 0);
  auto fetch = [](std::vector<int>& v, const int* dev) { return !dev || v.empty() || hipMemcpy(v.data(), dev, v.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess; };
  if (hipStreamSynchronize(c->stream) != hipSuccess || !fetch(n->act, c->S.order_n) || !fetch(n->chg, c->S.chg_n) || !fetch(n->kr, c->S.kr_n) || !fetch(g, c->d_lgate)) {
    c->err = std::string(who) + ": reading " + what + " failed";
    return ILQR_ERR_HIP;
  }
  for (size_t it = 0; it < mi && it < c->record.size() && !g.empty(); ++it) n->took[it] = (c->record[it].pair && g[8 * it + 4]) ? 1 : 0;
  return ILQR_OK;
}
// the order iteration it of the last solve was enqueued in
static ilqr::IterationRecord recorded(const ilqr_hip_ctx* c, int it) {
  return (size_t)it < c->record.size() ? c->record[it] : ilqr::IterationRecord{ilqr::ORDER_SEQUENTIAL, false, false};
}
long long ilqr_hip_get_linearized_rollouts(ilqr_hip_ctx* c) {
  if (!c) return -1;
  enter(c);
  const int n = c->lin_iterations;
  if (n <= 0) return 0;
  if (!c->lin_cached && !c->lin_listed) return (long long)c->B * n;
  IterationCounts k;
  if (read_iteration_counts(c, "ilqr_hip_get_linearized_rollouts", "the list counts", &k) != ILQR_OK) return -1;
  long long total = 0;
  for (int it = 0; it < n; ++it) total += (it > 0 && c->lin_cached) ? k.chg[it] : (c->lin_listed ? k.act[2 * it] : c->B);
  return total;
}
long long ilqr_hip_get_first_pass_rollouts(ilqr_hip_ctx* c) {
  if (!c) return -1;
  enter(c);
  const int n = c->lin_iterations;
  if (n <= 0) return 0;
  IterationCounts k;
  if (read_iteration_counts(c, "ilqr_hip_get_first_pass_rollouts", "the list counts", &k) != ILQR_OK) return -1;
  long long total = 0;
  for (int it = 0; it < n; ++it) total += recorded(c, it).first_listed ? k.chg[it] : (c->lin_listed ? k.act[2 * it] : c->B);
  return total;
}
int ilqr_hip_get_listed_spec_iterations(ilqr_hip_ctx* c) {
  if (!c) return -1;
  enter(c);
  IterationCounts k;
  if (read_iteration_counts(c, "ilqr_hip_get_listed_spec_iterations", "the gate words", &k) != ILQR_OK) return -1;
  int total = 0;
  for (int it = 0; it < c->lin_iterations && it < c->max_iter; ++it) total += k.took[it];
  return total;
}
int ilqr_hip_get_iteration_lists(ilqr_hip_ctx* c, int iter, int* chg, int* kr, int* counts) {
  if (!c || !counts || iter < 0 || iter >= c->max_iter) return ILQR_ERR_ARG;
  enter(c);
  if (c->lin_iterations <= 0 || !c->S.chg || !c->S.kr || !c->lin_cached) { c->err = "ilqr_hip_get_iteration_lists: the last solve kept no lists"; return ILQR_ERR_STATE; }
  IterationCounts k;
  TRY(read_iteration_counts(c, "ilqr_hip_get_iteration_lists", "the list counts", &k));
  counts[0] = k.chg[iter]; counts[1] = k.kr[iter];
  if (iter == 0) counts[0] = counts[1] = 0;      // (iteration 0 runs every rollout and reads neither list)
  if (chg && counts[0] > 0) HIPCHK(c, hipMemcpy(chg, c->S.chg + (size_t)iter * c->B, sizeof(int) * (size_t)counts[0], hipMemcpyDeviceToHost));
  if (kr && counts[1] > 0) HIPCHK(c, hipMemcpy(kr, c->S.kr + (size_t)iter * c->B, sizeof(int) * (size_t)counts[1], hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_get_iteration_orders(ilqr_hip_ctx* c, int* out) {
  if (!c || !out) return -1;
  enter(c);
  const int n = c->lin_iterations;
  if (n <= 0) return 0;
  IterationCounts k;
  if (read_iteration_counts(c, "ilqr_hip_get_iteration_orders", "the gate words", &k) != ILQR_OK) return -1;
  for (int it = 0; it < n; ++it) {
    const ilqr::OrderKind kind = recorded(c, it).kind;
    if (k.took[it]) out[it] = ILQR_ORDER_LISTED_SPEC;
    else if (kind == ilqr::ORDER_TWIN) out[it] = ILQR_ORDER_TWIN;
    else if (kind == ilqr::ORDER_DUAL) out[it] = k.act[2 * it] <= c->knobs.spec_max ? ILQR_ORDER_DUAL_TWIN : ILQR_ORDER_DUAL_SEQUENTIAL;
    else out[it] = ILQR_ORDER_SEQUENTIAL;
  }
  return n;
}
long long ilqr_hip_get_retry_pass_rollouts(ilqr_hip_ctx* c) {
  if (!c) return -1;
  enter(c);
  const int n = c->lin_iterations;
  if (n <= 0) return 0;
  if (c->n_slices > 1 || !c->S.order) return (long long)c->B * n;      // (batch slices keep no lists: the retry launches cover the slice)
  IterationCounts k;
  if (read_iteration_counts(c, "ilqr_hip_get_retry_pass_rollouts", "the list counts", &k) != ILQR_OK) return -1;
  long long total = 0;
  for (int it = 0; it < n; ++it) {
    // listed side by side: the twin ran for the changed rollouts, the known retries on the solve's own buffers
    if (k.took[it]) { total += k.chg[it] + k.kr[it]; continue; }
    const ilqr::OrderKind kind = recorded(c, it).kind;
    // side by side the twin pass runs for every active rollout; where both orders were enqueued the device took the twin for a list of at most spec_max
    const bool twin = kind == ilqr::ORDER_TWIN || (kind == ilqr::ORDER_DUAL && k.act[2 * it] <= c->knobs.spec_max);
    total += twin ? k.act[2 * it] : k.act[2 * it + 1];
  }
  return total;
}
int ilqr_hip_get_split_iterations(const ilqr_hip_ctx* c) { return c ? c->split_iterations : -1; }
int ilqr_hip_get_speculative_iterations(const ilqr_hip_ctx* c) { return c ? c->spec_iterations : -1; }
int ilqr_hip_set_dedup_saturated_retry(ilqr_hip_ctx* c, int on) { if (!c) return ILQR_ERR_ARG; c->dedup_retry = on ? 1 : 0; return ILQR_OK; }
int ilqr_hip_reload_environment(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  const Knobs k = read_knobs();
  if (!ilqr::plan_supported(k.var, LEGACY_BUILD)) { c->err = "the environment selects a kernel family this library does not hold (see ilqr_hip_create)"; return ILQR_ERR_UNSUPPORTED; }
  const bool pc = c->knobs.per_call; c->knobs = k; c->knobs.per_call = k.per_call || pc;
  return ILQR_OK;
}
int ilqr_hip_num_slices(const ilqr_hip_ctx* c) { return c ? slices_wanted(c, c->B) : -1; }
// The analytic Jacobians differentiate the constrained step with the active set and the sliding decisions held fixed.  The sliding
// branch (contact modes 3 / 4: the normal row and the normal force turn with the foot, kinetic friction follows the sticking
// solution) is carried by the two-knot tangent kernel only (k_lin_tangent2c<., 1 / 2>): the one-knot and scalar cross-check families
// refuse it.
static int jacobians_available(ilqr_hip_ctx* c) {
  if (c->jac_mode != ILQR_JAC_ANALYTIC || plan_of(c).analytic_full) return ILQR_OK;
  if (c->P.dyn.limits) {
    c->err = "joint-limit rows (ilqr_hip_set_joint_limits): analytic Jacobians are not available in this kernel family (ILQR_LIN / ILQR_DYN), select ILQR_JAC_FD_FORWARD with ilqr_hip_set_options";
    return ILQR_ERR_UNSUPPORTED;
  }
  if (c->P.dyn.contact >= ILQR_CONTACT_FRICTION_STANCE) {
    c->err = "contact modes 3 / 4 (Coulomb limit): analytic Jacobians are not available in this kernel family (ILQR_LIN / ILQR_DYN), select ILQR_JAC_FD_FORWARD with ilqr_hip_set_options";
    return ILQR_ERR_UNSUPPORTED;
  }
  return ILQR_OK;
}
// one inner solve of the whole batch on the handle's stream: one launch sequence, or one per batch slice behind ev_begin
__attribute__((noinline)) static int enqueue_batch(ilqr_hip_ctx* c, int k) {
  hipStream_t st = c->stream;
  const DevState& S = c->S; const h1::ProblemDev& P = c->P;
  if (k <= 1) {
    TRY(enqueue_solve(c, S, P, main_lanes(c), nullptr, nullptr));
  } else {
    TRY(ensure_slices(c, k));
    HIPCHK_S(c, hipEventRecord(c->ev_begin, st));
    const int per = (c->B + k - 1) / k;
    const bool stagger = c->knobs.stagger != 0;
    for (int i = 0; i < k; ++i) {
      const int b0 = i * per, Bs = (b0 + per <= c->B) ? per : (c->B - b0);
      if (Bs <= 0) continue;
      auto& sl = c->slices[i];
      HIPCHK_S(c, hipStreamWaitEvent(sl.st, c->ev_begin, 0));
      const DevState Ss = slice_state(S, (size_t)b0, Bs);
      const h1::ProblemDev Ps = slice_problem(P, b0);
      TRY(enqueue_solve(c, Ss, Ps, slice_lanes(sl), (stagger && i > 0) ? c->slices[i - 1].lead : nullptr, sl.lead));
      HIPCHK_S(c, hipEventRecord(sl.done, sl.st));
      HIPCHK_S(c, hipStreamWaitEvent(st, sl.done, 0));
    }
  }
  return ILQR_OK;
}
// Augmented Lagrangian: up to al_rounds rounds, each the inner solve as it stands followed by the update kernel on the handle's stream.
// A round after the first starts from the nominal trajectory its predecessor left -- iteration 0 of that round rolled it out from x0 with
// LaunchPlan::rollout, or the line search produced it: the nominal of an iteration >= 1, so its iteration 0 re-rolls it aside under the rule
// of those iterations (first_aside).  The baseline cost, every Jacobian and every quadratic are recomputed by iteration 0 under the new
// multipliers, and no list survives k_solve_begin: the linearisation cache and the two skips see nothing of the round before.
__attribute__((noinline)) static int enqueue_al_rounds(ilqr_hip_ctx* c, int k) {
  hipStream_t st = c->stream;
  const int rounds = c->al.rounds;
  const bool al_stop = c->early_exit && early_exit_gate(c);      // the host reads the count of rollouts left between two rounds
  HIPCHK_S(c, hipMemsetAsync(c->al.done, 0, (size_t)c->B * sizeof(int), st));
  HIPCHK_S(c, hipMemsetAsync(c->al.left, 0, (size_t)rounds * sizeof(int), st));
  HIPCHK_S(c, hipMemsetAsync(c->al.trace, 0xFF, (size_t)rounds * c->B * 5 * sizeof(double), st));      // (all bits set: NaN)
  HIPCHK_S(c, hipMemsetAsync(c->al.strace, 0xFF, (size_t)rounds * c->B * 2 * sizeof(double), st));
  HIPCHK_S(c, hipMemsetAsync(c->al.ttrace, 0xFF, (size_t)rounds * c->B * 2 * sizeof(double), st));
  c->al.rounds_run = 0;
  int rc = ILQR_OK;
  for (int round = 0; round < rounds && rc == ILQR_OK; ++round) {
    c->al.round = round;
    if (round > 0) { c->first_aside = true; c->spec_iterations = 0; c->split_iterations = 0; }
    rc = enqueue_batch(c, k);
    if (rc != ILQR_OK) break;
    ilqr::launch_al_update(c->S, al_view(c), round, c->early_exit, st);
    c->al.rounds_run = round + 1;
    if (al_stop && round + 1 < rounds) {
      hipError_t e = hipMemcpyAsync(&c->al.h_left[round], c->al.left + round, sizeof(int), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipEventRecord(c->al.ev, st);
      if (e == hipSuccess) e = hipEventSynchronize(c->al.ev);
      if (e != hipSuccess) rc = hip_failed(c, "reading the count of rollouts left between two rounds", e);
      else if (c->al.h_left[round] == 0) break;      // every rollout is done
    }
  }
  c->al.round = 0;
  return rc;
}
int ilqr_hip_solve_async(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  if (!c->initialized || !c->refs_set) { c->err = "solve before initialize/set_references"; return ILQR_ERR_STATE; }
  TRY(enter_launching(c));
  TRY(jacobians_available(c));
  hipStream_t st = c->stream;
  const DevState& S = c->S; const h1::ProblemDev& P = c->P; const ilqr::LaunchPlan L = plan_of(c);
  c->spans.clear(); c->pool_next = 0;
  HIPCHK(c, hipMemsetAsync(c->d_mismatch, 0, sizeof(unsigned long long), st));
  const int k = slices_wanted(c, c->B);
  c->n_slices = k;
  c->spec_iterations = 0; c->split_iterations = 0; c->nominal_rollouts = 0;
  TRY(ensure_shadow(c, L));
  if (!c->twin && ilqr::resolve_solve_order(solve_settings(c, S, main_lanes(c)), L).twin_wanted) TRY(ensure_twin(c));
  if (L.pack && !c->ab_pads_clean) { ilqr::launch_pack_zero_pads(S, st); c->ab_pads_clean = true; }
  c->first_aside = c->xbar_rolled && c->rolled_variant == L.rollout && same_dyn(c->rolled_dyn, P.dyn);
  c->xbar_rolled = false;                                   // after this solve xbar is an accepted line-search candidate
  if (P.al) TRY(enqueue_al_rounds(c, k));
  else TRY(enqueue_batch(c, k));
  HIPCHK(c, hipGetLastError());
  c->solved = true;
  return ILQR_OK;
}
int ilqr_hip_synchronize(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->profiling) collect_profile(c);
  return ILQR_OK;
}
int ilqr_hip_solve(ilqr_hip_ctx* c, const double* x0, double* cost_out) {
  if (!c) return ILQR_ERR_ARG;
  TRY(enter_launching(c));
  if (x0) {      // (a new x0: the nominal trajectory is rolled out from it before the linearisation, as the reference does)
    HIPCHK(c, hipMemcpyAsync(c->S.x0, x0, (size_t)c->B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->xbar_rolled = false;
  }
  TRY(ilqr_hip_solve_async(c));
  TRY(ilqr_hip_synchronize(c));
  if (cost_out) HIPCHK(c, hipMemcpy(cost_out, c->S.J, (size_t)c->B * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}

// ---------------------------------------------------------------- accessors
#define GETTER(name, ptr, count, type)                                                                          \
  int name(ilqr_hip_ctx* c, type* out) {                                                                        \
    if (!c || !out) return ILQR_ERR_ARG;                                                                        \
    enter(c);                                                                                    \
    HIPCHK(c, hipStreamSynchronize(c->stream));                                                                 \
    HIPCHK(c, hipMemcpy(out, c->S.ptr, (size_t)(count) * sizeof(type), hipMemcpyDeviceToHost));                 \
    return ILQR_OK;                                                                                             \
  }
GETTER(ilqr_hip_get_xbar, xbar, (size_t)c->B*(c->N + 1) * ILQR_NX, double)
GETTER(ilqr_hip_get_ubar, ubar, (size_t)c->B* c->N* ILQR_NU, double)
GETTER(ilqr_hip_get_gains_K, K, (size_t)c->B* c->N* ILQR_NU* ILQR_NX, double)
GETTER(ilqr_hip_get_gains_kff, kff, (size_t)c->B* c->N* ILQR_NU, double)
GETTER(ilqr_hip_get_cost, J, c->B, double)
GETTER(ilqr_hip_get_iterations, iters, c->B, int)
GETTER(ilqr_hip_get_lambda, lambda, c->B, double)

int ilqr_hip_get_trace(ilqr_hip_ctx* c, double* cost, double* alpha, double* lambda) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (cost) HIPCHK(c, hipMemcpy(cost, c->S.trace_cost, (size_t)c->B * (c->max_iter + 1) * sizeof(double), hipMemcpyDeviceToHost));
  if (alpha) HIPCHK(c, hipMemcpy(alpha, c->S.trace_alpha, (size_t)c->B * c->max_iter * sizeof(double), hipMemcpyDeviceToHost));
  if (lambda) HIPCHK(c, hipMemcpy(lambda, c->S.trace_lambda, (size_t)c->B * c->max_iter * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_first_knot_device(ilqr_hip_ctx* c, const double** u0, const double** K0, const double** cost) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  ilqr::launch_pack_first_knot(c->S, c->d_u0, c->d_K0, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (u0) *u0 = c->d_u0;
  if (K0) *K0 = c->d_K0;
  if (cost) *cost = c->S.J;
  return ILQR_OK;
}
int ilqr_hip_pack_first_knot_device(ilqr_hip_ctx* c, double* u0_out, double* K0_out, double* cost_out) {
  if (!c || !u0_out) return ILQR_ERR_ARG;
  enter(c);
  ilqr::launch_pack_first_knot(c->S, u0_out, K0_out ? K0_out : c->d_K0, c->stream);
  HIPCHK(c, hipGetLastError());
  if (cost_out) HIPCHK(c, hipMemcpyAsync(cost_out, c->S.J, (size_t)c->B * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_compute_control(ilqr_hip_ctx* c, const double* x_measured, double* u_apply) {
  if (!c || !x_measured || !u_apply) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipMemcpyAsync(c->d_tmpx, x_measured, (size_t)c->B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  ilqr::launch_compute_control(c->S, c->d_tmpx, c->d_u0, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(u_apply, c->d_u0, (size_t)c->B * ILQR_NU * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_compute_control_at(ilqr_hip_ctx* c, int knot, const double* x_measured, double* u_apply) {
  if (!c || !x_measured || !u_apply || knot < 0 || knot >= c->N) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipMemcpyAsync(c->d_tmpx, x_measured, (size_t)c->B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  ilqr::launch_compute_control_at(c->S, knot, c->d_tmpx, c->d_u0, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(u_apply, c->d_u0, (size_t)c->B * ILQR_NU * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}

// ---------------------------------------------------------------- stage entry points
int ilqr_hip_set_trajectory(ilqr_hip_ctx* c, const double* xbar, const double* ubar) {
  if (!c || !xbar || !ubar) return ILQR_ERR_ARG;
  enter(c);
  const size_t B = c->B, N = c->N;
  HIPCHK(c, hipMemcpyAsync(c->S.xbar, xbar, B * (N + 1) * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->S.ubar, ubar, B * N * ILQR_NU * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpy2DAsync(c->S.x0, ILQR_NX * sizeof(double), c->S.xbar, (N + 1) * ILQR_NX * sizeof(double), ILQR_NX * sizeof(double), B, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->initialized = true;
  c->xbar_rolled = false;
  return ILQR_OK;
}
#define STAGE_CHECK if (!c) return ILQR_ERR_ARG; if (!c->initialized) return ILQR_ERR_STATE
#define STAGE_POST HIPCHK(c, hipGetLastError()); HIPCHK(c, hipStreamSynchronize(c->stream)); return ILQR_OK
int ilqr_hip_stage_rollout(ilqr_hip_ctx* c) { STAGE_CHECK; TRY(enter_launching(c)); ilqr::launch_rollout(plan_of(c), c->S, c->P, ilqr::MASK_ALL, 1, 0, c->S.Jbase, c->stream); STAGE_POST; }
int ilqr_hip_stage_linearize(ilqr_hip_ctx* c) {
  STAGE_CHECK; TRY(enter_launching(c)); TRY(jacobians_available(c));
  const ilqr::LaunchPlan L = plan_of(c);
  ilqr::launch_linearize(L, c->S, c->P, ilqr::MASK_ALL, c->fd_eps, c->stream, 3, -1, 0, nullptr, c->d_stance_dyn);
  c->lin_fold_h = L.folds_h ? c->P.dyn.h : 0.0; c->ab_packed = false; c->ab_pads_clean = false;
  STAGE_POST;
}
int ilqr_hip_stage_cost_quadratics(ilqr_hip_ctx* c) { STAGE_CHECK; enter(c); if (!c->refs_set) return ILQR_ERR_STATE; ilqr::launch_cost_quadratics(c->S, c->P, ilqr::MASK_ALL, c->stream); c->lxx_layout = 0; STAGE_POST; }
// layout conversions on demand (in place): what a consumer of the standard layout (getters, any kernel family but the operand-layout
// one) or of the operand layout (stage API on riccati_pack.hip) calls first
static void want_standard_ab(ilqr_hip_ctx* c) { if (c->ab_packed) { ilqr::launch_unpack_ab(c->S, c->packed_h, c->stream); c->ab_packed = false; c->ab_pads_clean = false; } }
static void want_standard_lxx(ilqr_hip_ctx* c, bool whole) {
  if (c->lxx_layout == 2) { ilqr::launch_unpack_lxx(c->S, c->stream); c->lxx_layout = 0; }
  if (c->lxx_layout == 1 && whole) { ilqr::launch_mirror_lxx(c->S, c->stream); c->lxx_layout = 0; }
}
int ilqr_hip_stage_backward_pass(ilqr_hip_ctx* c) {
  STAGE_CHECK; TRY(enter_launching(c));
  const ilqr::LaunchPlan L = plan_of(c);
  const int layout = ilqr::lxx_layout_of(c->lin_fold_h != 0.0 ? L.backward_foldable : L.backward_plain);      // (of the kernel launch_backward picks)
  if (layout == 2) {
    // analytic Jacobians and the operand-layout kernel (riccati_pack.hip): convert in place what is not yet in its layout
    if (!c->ab_packed) { ilqr::launch_pack_ab(c->S, c->stream); c->ab_packed = true; c->packed_h = c->lin_fold_h; c->ab_pads_clean = true; }
    if (c->lxx_layout != 2) { want_standard_lxx(c, true); ilqr::launch_pack_lxx(c->S, c->stream); c->lxx_layout = 2; }
  } else {
    // any other family reads the standard layout (the one-wave kernel: the tiles I >= J of lxx_t, t < N, suffice)
    want_standard_ab(c);
    want_standard_lxx(c, layout == 0);
  }
  ilqr::launch_backward(L, c->S, ilqr::MASK_ALL, c->stream, c->lin_fold_h);
  STAGE_POST;
}
int ilqr_hip_stage_total_cost(ilqr_hip_ctx* c, double* cost) {
  STAGE_CHECK; TRY(enter_launching(c)); if (!cost || !c->refs_set) return ILQR_ERR_ARG;
  ilqr::launch_rollout(plan_of(c), c->S, c->P, ilqr::MASK_ALL, 0, 0, c->d_cost_tmp, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(cost, c->d_cost_tmp, (size_t)c->B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_stage_line_search(ilqr_hip_ctx* c, int* improved, double* new_cost, double* alpha) {
  STAGE_CHECK; TRY(enter_launching(c)); if (!c->refs_set) return ILQR_ERR_STATE;
  const ilqr::LaunchPlan L = plan_of(c);
  ilqr::launch_rollout(L, c->S, c->P, ilqr::MASK_ALL, 0, 0, c->S.Jbase, c->stream);   // baseline = computeTotalCost(xbar, ubar), ilqr.cpp:317
  ilqr::launch_line_search(L, c->S, c->P, ilqr::MASK_ALL, c->stream);
  ilqr::launch_control(c->S, 2, 0, c->tol, 0, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t B = c->B;
  std::vector<int> ai(B);
  HIPCHK(c, hipMemcpy(ai.data(), c->S.alpha_idx, B * sizeof(int), hipMemcpyDeviceToHost));
  static const double alphas[8] = {1.0, 0.8, 0.6, 0.4, 0.2, 0.1, 0.05, 0.01};
  for (size_t b = 0; b < B; ++b) { if (improved) improved[b] = ai[b] >= 0; if (alpha) alpha[b] = ai[b] >= 0 ? alphas[ai[b]] : 0.0; }
  if (new_cost) HIPCHK(c, hipMemcpy(new_cost, c->S.ls_cost, B * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_get_linearization(ilqr_hip_ctx* c, double* A, double* Bm) {
  if (!c) return ILQR_ERR_ARG; enter(c);
  const size_t B = c->B, N = c->N;
  want_standard_ab(c); HIPCHK(c, hipGetLastError());      // (the last solve may have left the operand layout behind)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (A) HIPCHK(c, hipMemcpy(A, c->S.A, B * N * ILQR_NX * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost));
  if (Bm) HIPCHK(c, hipMemcpy(Bm, c->S.Bm, B * N * ILQR_NX * ILQR_NU * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_set_linearization(ilqr_hip_ctx* c, const double* A, const double* Bm) {
  if (!c || !A || !Bm) return ILQR_ERR_ARG; enter(c);
  const size_t B = c->B, N = c->N;
  HIPCHK(c, hipMemcpy(c->S.A, A, B * N * ILQR_NX * ILQR_NX * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->S.Bm, Bm, B * N * ILQR_NX * ILQR_NU * sizeof(double), hipMemcpyHostToDevice));
  c->initialized = true;
  c->lin_fold_h = 0.0;      // Jacobians of unknown origin: generic backward kernel
  c->ab_packed = false; c->ab_pads_clean = false;
  return ILQR_OK;
}
int ilqr_hip_get_quadratics(ilqr_hip_ctx* c, double* lx, double* lu, double* lxx, double* luu) {
  if (!c) return ILQR_ERR_ARG; enter(c);
  const size_t B = c->B, N = c->N;
  if (lxx) { want_standard_lxx(c, false); HIPCHK(c, hipGetLastError()); }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (lx) HIPCHK(c, hipMemcpy(lx, c->S.lx, B * (N + 1) * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost));
  if (lu) HIPCHK(c, hipMemcpy(lu, c->S.lu, B * N * ILQR_NU * sizeof(double), hipMemcpyDeviceToHost));
  if (lxx) {
    HIPCHK(c, hipMemcpy(lxx, c->S.lxx, B * (N + 1) * ILQR_NX * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost));
    if (c->lxx_layout == 1) {   // the last solve stored the tiles I >= J of the knots t < N only (quad_kernels.hip): lxx is symmetric
      for (size_t k = 0; k < B * (N + 1); ++k) {
        if (k % (N + 1) == N) continue;
        double* H = lxx + k * ILQR_NX * ILQR_NX;
        for (int i = 0; i < ILQR_NX; ++i) for (int j = 16 * (i / 16 + 1); j < ILQR_NX; ++j) H[i * ILQR_NX + j] = H[j * ILQR_NX + i];
      }
    }
  }
  if (luu) HIPCHK(c, hipMemcpy(luu, c->S.luu, B * N * ILQR_NU * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_set_quadratics(ilqr_hip_ctx* c, const double* lx, const double* lu, const double* lxx, const double* luu) {
  if (!c || !lx || !lu || !lxx || !luu) return ILQR_ERR_ARG; enter(c);
  const size_t B = c->B, N = c->N;
  HIPCHK(c, hipMemcpy(c->S.lx, lx, B * (N + 1) * ILQR_NX * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->S.lu, lu, B * N * ILQR_NU * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->S.lxx, lxx, B * (N + 1) * ILQR_NX * ILQR_NX * sizeof(double), hipMemcpyHostToDevice));
  c->lxx_layout = 0;
  HIPCHK(c, hipMemcpy(c->S.luu, luu, B * N * ILQR_NU * sizeof(double), hipMemcpyHostToDevice));
  return ILQR_OK;
}
int ilqr_hip_get_value_function(ilqr_hip_ctx* c, double* Vx, double* Vxx) {
  if (!c) return ILQR_ERR_ARG; enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (Vx) HIPCHK(c, hipMemcpy(Vx, c->S.Vx, (size_t)c->B * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost));
  if (Vxx) HIPCHK(c, hipMemcpy(Vxx, c->S.Vxx, (size_t)c->B * ILQR_NX * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_step_stance(ilqr_hip_ctx* c, int count, const double* x, const double* u, int stance_left, int stance_right, double* x_next);
int ilqr_hip_step(ilqr_hip_ctx* c, int count, const double* x, const double* u, double* x_next) {
  return ilqr_hip_step_stance(c, count, x, u, 1, 1, x_next);
}
int ilqr_hip_set_contact_mode(ilqr_hip_ctx* c, int mode, double softness) {
  if (!c || (mode != ILQR_CONTACT_NONE && mode != ILQR_CONTACT_RIGID_STANCE && mode != ILQR_CONTACT_UNILATERAL_STANCE && mode != ILQR_CONTACT_FRICTION_STANCE && mode != ILQR_CONTACT_KINETIC_FRICTION_STANCE)) return ILQR_ERR_ARG;
  enter(c);
  if (mode >= ILQR_CONTACT_FRICTION_STANCE && !plan_of(c).cone_and_limits) { c->err = "contact modes 3 / 4 (Coulomb limit) exist on the two-lane kernels only; unset ILQR_DYN=s"; return ILQR_ERR_UNSUPPORTED; }
  if (mode == ILQR_CONTACT_RIGID_STANCE && c->P.stance_geom) { c->err = "contact mode 1 (bilateral weld) with the stance source GEOMETRY: a welded foot never leaves the floor; use mode 2, 3 or 4"; return ILQR_ERR_UNSUPPORTED; }
  c->P.dyn.contact = mode;
  if (softness > 0.0) c->P.dyn.soft = softness;
  return ILQR_OK;
}
int ilqr_hip_set_joint_limits(ilqr_hip_ctx* c, int on) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  if (on && !plan_of(c).cone_and_limits) { c->err = "joint-limit rows exist on the two-lane kernels only; unset ILQR_DYN=s"; return ILQR_ERR_UNSUPPORTED; }
  c->P.dyn.limits = on ? 1 : 0;     // (a nominal rolled under the other setting is recognised by same_dyn)
  return ILQR_OK;
}
int ilqr_hip_set_joint_limit_stiffness(ilqr_hip_ctx* c, double k) {
  if (!c || !(k >= 0.0) || !std::isfinite(k)) return ILQR_ERR_ARG;
  c->P.dyn.lim_k = k;          // (a nominal rolled under another stiffness is recognised by same_dyn)
  return ILQR_OK;
}
int ilqr_hip_set_friction(ilqr_hip_ctx* c, double mu) {
  if (!c || !(mu >= 0.0)) return ILQR_ERR_ARG;
  c->P.dyn.mu = mu;            // (a nominal rolled under another mu is recognised by same_dyn)
  return ILQR_OK;
}
// grows a scratch buffer of the single-step calls to `count` rows of `width` doubles
static int grow_step_buffer(ilqr_hip_ctx* c, double** p, size_t* cap, size_t count, size_t width) {
  if (count <= *cap) return ILQR_OK;
  if (*p) hipFree(*p);
  *p = nullptr; *cap = 0;
  HIPCHK(c, hipMalloc((void**)p, count * width * sizeof(double)));
  *cap = count;
  return ILQR_OK;
}
// the scratch every single-step call uses -- states, controls, next states and the stance flags out -- owned by the context and grown on
// demand (the closed loop steps the plant every MPC step)
static int grow_step_scratch(ilqr_hip_ctx* c, int count) {
  if ((size_t)count <= c->step_cap) return ILQR_OK;
  if (c->d_stepx) hipFree(c->d_stepx);
  if (c->d_stepu) hipFree(c->d_stepu);
  if (c->d_stepn) hipFree(c->d_stepn);
  if (c->d_stance_out) hipFree(c->d_stance_out);
  c->d_stepx = c->d_stepu = c->d_stepn = nullptr; c->d_stance_out = nullptr; c->step_cap = 0;
  HIPCHK(c, hipMalloc((void**)&c->d_stepx, (size_t)count * ILQR_NX * sizeof(double)));
  HIPCHK(c, hipMalloc((void**)&c->d_stepu, (size_t)count * ILQR_NU * sizeof(double)));
  HIPCHK(c, hipMalloc((void**)&c->d_stepn, (size_t)count * ILQR_NX * sizeof(double)));
  HIPCHK(c, hipMalloc((void**)&c->d_stance_out, (size_t)count * 2 * sizeof(int)));
  c->step_cap = (size_t)count;
  return ILQR_OK;
}
// the plant step of ilqr_hip_step_stance / ilqr_hip_step_geometry (geom: stance from each item's own feet, stance_out [count][2] nullable)
static int plant_step(ilqr_hip_ctx* c, int count, const double* x, const double* u, int stance_left, int stance_right, int geom, int* stance_out, double* x_next) {
  TRY(grow_step_scratch(c, count));
  HIPCHK(c, hipMemcpyAsync(c->d_stepx, x, (size_t)count * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_stepu, u, (size_t)count * ILQR_NU * sizeof(double), hipMemcpyHostToDevice, c->stream));
  ilqr::launch_step(plan_of(c), count, c->d_stepx, c->d_stepu, c->P.dyn, c->d_stepn, c->stream, stance_left, stance_right, geom, geom ? c->d_stance_out : nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(x_next, c->d_stepn, (size_t)count * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (geom && stance_out) HIPCHK(c, hipMemcpyAsync(stance_out, c->d_stance_out, (size_t)count * 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_step_stance(ilqr_hip_ctx* c, int count, const double* x, const double* u, int stance_left, int stance_right, double* x_next) {
  if (!c || count <= 0 || !x || !u || !x_next) return ILQR_ERR_ARG;
  TRY(enter_launching(c));
  return plant_step(c, count, x, u, stance_left, stance_right, 0, nullptr, x_next);
}
// ---------------------------------------------------------------- stance from the foot hulls
static const char* geometry_refusal(const ilqr_hip_ctx* c) {
  if (!plan_of(c).stance_geometry) return "the stance source GEOMETRY exists on the two-lane kernels only; unset ILQR_DYN=s";
  if (c->P.dyn.contact == ILQR_CONTACT_RIGID_STANCE) return "contact mode 1 (bilateral weld) with the stance source GEOMETRY: a welded foot never leaves the floor; use mode 2, 3 or 4";
  return nullptr;
}
int ilqr_hip_set_stance_source(ilqr_hip_ctx* c, int source) {
  if (!c || (source != ILQR_STANCE_SCHEDULE && source != ILQR_STANCE_GEOMETRY)) return ILQR_ERR_ARG;
  enter(c);
  if (source == ILQR_STANCE_GEOMETRY) {
    if (const char* why = geometry_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  }
  if (c->P.stance_geom != source) c->xbar_rolled = false;      // (the nominal trajectory was rolled under the other source)
  c->P.stance_geom = source;
  return ILQR_OK;
}
int ilqr_hip_step_geometry(ilqr_hip_ctx* c, int count, const double* x, const double* u, double* x_next, int* stance_out) {
  if (!c || count <= 0 || !x || !u || !x_next) return ILQR_ERR_ARG;
  TRY(enter_launching(c));
  if (const char* why = geometry_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  return plant_step(c, count, x, u, 1, 1, 1, stance_out, x_next);
}
int ilqr_hip_get_stance(ilqr_hip_ctx* c, int* stance) {
  if (!c || !stance) return ILQR_ERR_ARG;
  const size_t B = c->B, N = c->N;
  if (c->P.stance_geom) {      // (the two-lane family's kernel decides: this branch launches by family, the schedule's does not)
    TRY(enter_launching(c));
    if (const char* why = geometry_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
    ilqr::launch_stance_geom_s(c->S, ilqr::MASK_ALL, nullptr, nullptr, c->d_stance_dyn, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(stance, c->d_stance_dyn, B * N * 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ILQR_OK;
  }
  // the schedule's rows t = 0..N-1 (one shared set or one per rollout)
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t per = (N + 1) * 2;
  std::vector<int> sched(c->P.stance_stride ? B * per : per);
  HIPCHK(c, hipMemcpy(sched.data(), c->d_stance, sched.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; ++b)
    std::memcpy(stance + b * N * 2, sched.data() + (c->P.stance_stride ? b * per : 0), N * 2 * sizeof(int));
  return ILQR_OK;
}
// ---------------------------------------------------------------- device-resident plant (plant_kernels.hip)
// the task score's record before the first scored interval: zeros (nothing to do while none is installed); returns behind the stream
__attribute__((noinline, minsize)) static int task_score_empty(ilqr_hip_ctx* c) {
  if (c->d_tscore) HIPCHK(c, hipMemsetAsync(c->d_tscore, 0, (size_t)c->B * ILQR_PLANT_TASK_SCORE_TERMS * sizeof(double), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
// the record of ilqr_hip_plant_set_score before the first scored interval: sums and count zero, minimum height +inf (empty while no score is installed)
static std::vector<double> empty_score(const ilqr_hip_ctx* c) {
  std::vector<double> r(c->score_on ? (size_t)c->B * ILQR_PLANT_SCORE_TERMS : 0, 0.0);
  for (size_t i = 6; i < r.size(); i += ILQR_PLANT_SCORE_TERMS) r[i] = std::numeric_limits<double>::infinity();
  return r;
}
// Scores the `count` ring rows the plant kernel just enqueued fills (from ring row row0 on, against the reference rows knot0 + j), directly
// behind it on the handle's stream: the score kernels see the reference buffers that kernel saw.  Their problem descriptor is the handle's
// with the scoring weights in the place of the shared ones and no weight-set table.
static void enqueue_score(ilqr_hip_ctx* c, long row0, int knot0, int count) {
  if (!c->score_on) return;
  h1::ProblemDev Ps = c->P;
  std::memcpy(Ps.Q, c->score_Q, sizeof(Ps.Q)); std::memcpy(Ps.R, c->score_R, sizeof(Ps.R));
  Ps.w_upright = c->score_w[0]; Ps.w_balance = c->score_w[1]; Ps.w_joint = c->score_w[2]; Ps.w_ctrl = c->score_w[3];
  Ps.wsets = nullptr; Ps.wsets_stride = 0; Ps.al = nullptr; Ps.al_stride = 0; Ps.alb = nullptr; Ps.alb_stride = 0; Ps.als = nullptr; Ps.als_stride = 0; Ps.alsb = nullptr; Ps.alsb_stride = 0; Ps.alb_knot = 0; Ps.alsb_knot = 0; Ps.altb = nullptr;
  ilqr::launch_plant_score(Ps, c->B, c->plant.hist_x, c->plant.hist_u, row0, c->hist_cap, knot0, count, c->d_score_terms, c->d_score, c->stream);
}
// What a plant call of `count` intervals needs while a score of either kind is installed, checked before anything is launched or counted: the
// ring rows the score kernels read, and for the task score (ilqr_hip_plant_set_task_score) a task window to score against
__attribute__((noinline, minsize)) static int plant_scores_ready(ilqr_hip_ctx* c, int count) {
  if ((c->score_on || c->d_tscore) && count > c->hist_cap) {
    c->err = "plant call with a score installed: " + std::to_string(count) + " intervals exceed the history ring's " + std::to_string(c->hist_cap) + " rows (ilqr_hip_plant_set_history: the score kernels read the ring's rows)";
    return ILQR_ERR_STATE;
  }
  if (c->d_tscore && !c->P.altb) { c->err = "plant call with a task score installed and no task family"; return ILQR_ERR_STATE; }
  return ILQR_OK;
}
// the same for the task score, behind the cost score's kernels: the rows knot0 + j of the task window and of the schedule the handle holds now
static void enqueue_task_score(ilqr_hip_ctx* c, long row0, int knot0, int count) {
  if (!c->d_tscore) return;
  const ilqr::PlantTaskScoreDev T{c->P.altb, c->P.altb_stride, c->P.altb_knot, c->P.stance, c->P.stance_stride, c->tscore_tol};
  ilqr::g_al_knot.plant_task_score(&T, c->B, c->plant.hist_x, row0, c->hist_cap, knot0, count, c->d_tscore_terms, c->d_tscore, c->stream);
}
// The plant's dynamics parameters: the handle's at the physics step (main/humanoid_mpc.cpp:99,128), under the plant's own contact mode and
// joint-limit option where ilqr_hip_plant_set_model has given it one.  (With a parameter table the kernels replace g, mu, soft and lim_k per rollout.)
constexpr int WRENCH_REC = 16;      // doubles of a wrench record on the device (128 B): the ILQR_PLANT_WRENCH values and padding
constexpr int PAYLOAD_REC = 16;     // doubles of a payload record on the device (128 B): the ILQR_PLANT_PAYLOAD values and padding
constexpr int JOINT_REC = 80;       // doubles of a joint record on the device (640 B): the ILQR_PLANT_JOINTS values and padding
constexpr int TERRAIN_REC = 8;      // doubles of a terrain record on the device (64 B): the ILQR_PLANT_TERRAIN values and padding
static h1::DynParams plant_dyn(const ilqr_hip_ctx* c) {
  h1::DynParams dyn = c->P.dyn;
  dyn.h = c->P.dyn.h / c->plant_substeps;
  if (c->plant_mode >= 0) dyn.contact = c->plant_mode;
  if (c->plant_limits >= 0) dyn.limits = c->plant_limits;
  return dyn;
}
// geometry_refusal for the plant: against the contact mode the plant would step with
static const char* plant_geometry_refusal(const ilqr_hip_ctx* c, int plant_mode) {
  if (!plan_of(c).stance_geometry) return "the stance source GEOMETRY exists on the two-lane kernels only; unset ILQR_DYN=s";
  if ((plant_mode >= 0 ? plant_mode : c->P.dyn.contact) == ILQR_CONTACT_RIGID_STANCE) return "plant contact mode 1 (bilateral weld) with the stance source GEOMETRY: a welded foot never leaves the floor; use mode 2, 3 or 4";
  return nullptr;
}
// What a plant call launches (plant_plan.h): resolved from the installed tables behind the call's prologue, never stored.
static ilqr::PlantPlan plant_plan_of(const ilqr_hip_ctx* c, bool follow) {
  return ilqr::resolve_plant_plan({c->pparams.d != nullptr, c->wrench.d != nullptr, c->payload.d != nullptr, c->obs.d != nullptr, c->act.d != nullptr, c->joints.d != nullptr, c->joints_nominal, c->terrain.d != nullptr}, follow);
}
// The module families always read a parameter record: the parameter table's, or (PlantPlan::self_params) this ONE record of the handle's own
// values with gain 1, uploaded again whenever the handle's values have changed.
static int plant_self_params(ilqr_hip_ctx* c) {
  const h1::DynParams& d = c->P.dyn;
  const double rec[ILQR_PLANT_PARAMS + 1] = {d.g[0], d.g[1], d.g[2], d.mu, d.soft, d.lim_k, 1.0, 0.0};
  if (c->d_self_params && std::memcmp(rec, c->self_params, sizeof(rec)) == 0) return ILQR_OK;
  if (!c->d_self_params) HIPCHK(c, hipMalloc((void**)&c->d_self_params, sizeof(rec)));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (a plant call in flight may still read the record this one replaces)
  HIPCHK(c, hipMemcpy(c->d_self_params, rec, sizeof(rec), hipMemcpyHostToDevice));
  std::memcpy(c->self_params, rec, sizeof(rec));
  return ILQR_OK;
}
static ilqr::ObservationTable observation_table(const ilqr_hip_ctx* c) {
  return ilqr::ObservationTable{c->obs.d, c->obs.sets == 1 ? 0 : ILQR_PLANT_OBSERVATION, c->obs_seed, c->obs_stream0};
}
static void enqueue_observation_draw(ilqr_hip_ctx* c, long interval0, int count) {
  const ilqr::ObservationTable O = observation_table(c);
  module_fn<ilqr::observe_draw_fn>(ilqr::MOD_OBSERVE, FN_DRAW)(c->B, &O, interval0, count, c->d_obs_delta, c->stream);
}
static void enqueue_actuator_draw(ilqr_hip_ctx* c, long interval0, int count) {
  module_fn<ilqr::actuator_draw_fn>(ilqr::MOD_ACTUATOR, FN_DRAW)(c->B, c->act_seed, c->act_stream0, interval0, count, c->d_act_z, c->stream);
}
// What a warm start hands the solve as x0: the plant's state, or -- under an observation table -- its measurement in the current interval,
// Pl.x [+] delta(plant_intervals): a one-row draw and the apply in the place of the device copy.
static int enqueue_measured_x0(ilqr_hip_ctx* c, double* out) {
  if (!c->obs.d) {
    HIPCHK(c, hipMemcpyAsync(out, c->plant.x, (size_t)c->B * ILQR_NX * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return ILQR_OK;
  }
  TRY(need_module(c, ilqr::MOD_OBSERVE));
  enqueue_observation_draw(c, c->plant_intervals, 1);
  module_fn<ilqr::observe_apply_fn>(ilqr::MOD_OBSERVE, FN_APPLY)(c->B, c->plant.x, c->d_obs_delta, out, c->stream);
  HIPCHK(c, hipGetLastError());
  return ILQR_OK;
}
// beta = -expm1(-h / tau), h = dt / substeps, of every record of the actuator table, in double on the host -> d_act_beta.  tau == 0 (no lag: the
// kernel selects y = a) is never computed; its beta reads 1.
static int upload_actuator_blend(ilqr_hip_ctx* c) {
  const double h = c->P.dyn.h / c->plant_substeps;      // (the plant's step: plant_dyn)
  c->act_beta.assign((size_t)c->act.sets * ILQR_NU, 1.0);
  for (int s = 0; s < c->act.sets; ++s)
    for (int i = 0; i < ILQR_NU; ++i) {
      const double tau = c->act_rec[(size_t)s * ILQR_PLANT_ACTUATOR + 1 + i];
      if (tau != 0.0) c->act_beta[(size_t)s * ILQR_NU + i] = -std::expm1(-h / tau);
    }
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (a plant call in flight may still read the rows this one replaces)
  HIPCHK(c, hipMemcpy(c->d_act_beta, c->act_beta.data(), c->act_beta.size() * sizeof(double), hipMemcpyHostToDevice));
  return ILQR_OK;
}
// The plant kernel of one call: without a table exactly the launch without the feature; with one, the followed kernel of the plan's family
// with the tables' records -- for an advance over the one interval (0, 1), which is an advance bit for bit -- behind the draws the plan names.
// Every followed family gets the same call record (ilqr_kernels.h PlantCall) with every table of the handle in it and reads its own and the
// ones before it, any of which may be null but the parameter record: the parameter table's or the handle's own (plant_self_params).  row: the advance's ring row (-1: no ring) or the follow's first ring row.  The caller has loaded
// plan.modules.
static void enqueue_plant(ilqr_hip_ctx* c, const ilqr::PlantPlan& plan, const h1::DynParams& dyn, int geom, int first_knot, int count, long row) {
  const int g = (geom && dyn.contact != 0) ? 1 : 0, kick = c->plant_kick ? 1 : 0;
  const bool one = c->act.sets == 1;
  ilqr::PlantCall call{};
  call.a = {c->d_stance, c->P.stance_stride, g, c->plant_substeps, c->plant_feedback, kick, first_knot, count, row < 0 ? 0L : row, (long)c->hist_cap};
  call.T = c->pparams.d ? ilqr::PlantTable{c->pparams.d, c->pparams.sets == 1 ? 0 : ILQR_PLANT_PARAMS + 1} : ilqr::PlantTable{c->d_self_params, 0};
  call.W = {c->wrench.d, c->wrench.sets == 1 ? 0 : WRENCH_REC, c->plant_intervals};
  call.M = {c->payload.d, c->payload.sets == 1 ? 0 : PAYLOAD_REC};
  call.dobs = plan.draw_observation ? c->d_obs_delta : nullptr;
  call.A = {c->act.d, one ? 0 : ILQR_PLANT_ACTUATOR, c->d_act_beta, one ? 0 : ILQR_NU, c->d_act_z, c->d_act_fifo, c->d_act_y, c->d_act_applied, c->act_substeps};
  if (plan.pass_joints) call.J = {c->joints.d, c->joints.sets == 1 ? 0 : JOINT_REC};      // (an all-nominal joint table is no table to any family)
  call.R = {c->terrain.d, c->terrain.sets == 1 ? 0 : TERRAIN_REC};
  if (plan.draw_observation) enqueue_observation_draw(c, c->plant_intervals, count);
  if (plan.draw_actuator) enqueue_actuator_draw(c, c->plant_intervals, count);
  switch (plan.family) {
    case ilqr::PLANT_ADVANCE: ilqr::launch_plant_advance(c->S, c->plant, dyn, c->d_stance, c->P.stance_stride, g, c->plant_substeps, c->plant_feedback, kick, row, c->stream); break;
    case ilqr::PLANT_FOLLOW: ilqr::launch_plant_follow(c->S, c->plant, dyn, call, c->stream); break;
    case ilqr::PLANT_PARAMS: ilqr::launch_plant_follow_params(c->S, c->plant, dyn, call, c->stream); break;
    default: module_fn<ilqr::plant_follow_fn>(plan.family - ilqr::PLANT_WRENCH, FN_FOLLOW)(&c->S, &c->plant, &dyn, &call, c->stream);      // the family's own module (plant_plan.h: in the order of the families)
  }
  if (plan.draw_actuator) c->act_substeps += (long)count * c->plant_substeps;
}
// a terrain table is a floor somebody has to consult: the plant decides its own contacts (source GEOMETRY) in a mode with unilateral rows
static const char* terrain_refusal(const ilqr_hip_ctx* c) {
  if (c->plant_source != ILQR_STANCE_GEOMETRY) return "a terrain table is installed and the plant's contact source is SCHEDULE: nothing would consult the floor; ilqr_hip_plant_configure(..., ILQR_STANCE_GEOMETRY) or ilqr_hip_plant_clear_terrain";
  const int mode = c->plant_mode >= 0 ? c->plant_mode : c->P.dyn.contact;
  if (mode == ILQR_CONTACT_NONE || mode == ILQR_CONTACT_RIGID_STANCE) return "a terrain table is installed and the plant's contact mode is 0 or 1: no foot lands or lifts by its height; use mode 2, 3 or 4 or ilqr_hip_plant_clear_terrain";
  return nullptr;
}
// what ilqr_hip_plant_advance and ilqr_hip_plant_follow do in front of enqueue_plant: the handle's own parameter record and every module of the plan
static int prepare_plant(ilqr_hip_ctx* c, const ilqr::PlantPlan& plan) {
  if (plan.family == ilqr::PLANT_TERRAIN) if (const char* why = terrain_refusal(c)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  if (plan.self_params) TRY(plant_self_params(c));
  for (int m = 0; m < ilqr::PLANT_MODULES; ++m) if ((plan.modules >> m) & 1u) TRY(need_module(c, m));
  return ILQR_OK;
}
int ilqr_hip_plant_reset(ilqr_hip_ctx* c, const double* x) {
  if (!c || !x) return ILQR_ERR_ARG;
  enter(c);
  const size_t B = c->B;
  const std::vector<int> ones(B, 1);
  HIPCHK(c, hipMemcpyAsync(c->plant.x, x, B * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->plant.alive, ones.data(), B * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(c->plant.u, 0, B * ILQR_NU * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(c->plant.stance, 0, B * 2 * sizeof(int), c->stream));
  const std::vector<double> empty = empty_score(c);      // (outlives the copy: the synchronisation below)
  if (c->score_on) HIPCHK(c, hipMemcpyAsync(c->d_score, empty.data(), empty.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  TRY(task_score_empty(c));      // (synchronises: the caller's buffers are free on return)
  c->plant_set = true; c->plant_kick = false; c->hist_n = 0; c->plant_intervals = 0;
  c->act_substeps = 0;      // (the actuator's state is primed again by the next substep)
  return ILQR_OK;
}
int ilqr_hip_plant_configure(ilqr_hip_ctx* c, int substeps, int feedback_mode, int contact_source) {
  if (!c || substeps < 1 || (feedback_mode != 0 && feedback_mode != 1) || (contact_source != ILQR_STANCE_SCHEDULE && contact_source != ILQR_STANCE_GEOMETRY)) return ILQR_ERR_ARG;
  enter(c);
  if (contact_source == ILQR_STANCE_GEOMETRY) {
    if (const char* why = plant_geometry_refusal(c, c->plant_mode)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  }
  const bool new_h = substeps != c->plant_substeps;
  c->plant_substeps = substeps; c->plant_feedback = feedback_mode; c->plant_source = contact_source;
  c->act_substeps = 0;      // (the actuator's state is primed again by the next substep)
  if (c->act.d && new_h) TRY(upload_actuator_blend(c));      // (beta depends on h = dt / substeps)
  return ILQR_OK;
}
int ilqr_hip_plant_kick(ilqr_hip_ctx* c, const double* dv) {
  if (!c || !dv) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipMemcpyAsync(c->plant.dv, dv, (size_t)c->B * ILQR_NV * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->plant_kick = true;
  return ILQR_OK;
}
int ilqr_hip_plant_advance(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  if (!c->solved || !c->plant_set) { c->err = "plant_advance before a solve / before ilqr_hip_plant_reset"; return ILQR_ERR_STATE; }
  TRY(enter_launching(c));
  const bool geom = c->plant_source == ILQR_STANCE_GEOMETRY;
  if (geom) {      // (the contact mode or the family may have changed since plant_configure)
    if (const char* why = plant_geometry_refusal(c, c->plant_mode)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  }
  TRY(plant_scores_ready(c, 1));
  const ilqr::PlantPlan plan = plant_plan_of(c, false);
  TRY(prepare_plant(c, plan));
  const h1::DynParams dyn = plant_dyn(c);
  const long row = c->hist_cap > 0 ? c->hist_n % c->hist_cap : -1L;
  enqueue_plant(c, plan, dyn, geom ? 1 : 0, 0, 1, row);
  enqueue_score(c, row, 0, 1);
  enqueue_task_score(c, row, 0, 1);
  HIPCHK(c, hipGetLastError());
  c->plant_kick = false;
  c->plant_intervals += 1;
  if (row >= 0) c->hist_n += 1;
  return ILQR_OK;      // asynchronous on the handle's stream
}
int ilqr_hip_initialize_warm_from_plant(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  if (!c->initialized || !c->plant_set) return ILQR_ERR_STATE;
  TRY(enter_launching(c));
  const size_t B = c->B, N = c->N;
  TRY(enqueue_measured_x0(c, c->S.x0));
  HIPCHK(c, hipMemcpyAsync(c->d_prevx, c->S.xbar, B * (N + 1) * ILQR_NX * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_prevu, c->S.ubar, B * N * ILQR_NU * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  ilqr::launch_warm_shift(c->S, c->d_prevx, c->d_prevu, c->stream);      // (k_warm_shift reads x0 from S.x0: the plant's state by the copy above)
  ilqr::launch_last_step(plan_of(c), c->S, c->P, c->stream);
  al_follow_initialize(c, 1);
  HIPCHK(c, hipGetLastError());
  c->xbar_rolled = false;
  return ILQR_OK;      // asynchronous on the handle's stream
}
int ilqr_hip_plant_follow(ilqr_hip_ctx* c, int first_knot, int count) {
  if (!c || first_knot < 0 || count < 1 || count > c->N - first_knot) return ILQR_ERR_ARG;
  if (!c->solved || !c->plant_set) { c->err = "plant_follow before a solve / before ilqr_hip_plant_reset"; return ILQR_ERR_STATE; }
  TRY(enter_launching(c));
  const bool geom = c->plant_source == ILQR_STANCE_GEOMETRY;
  if (geom) {      // (as ilqr_hip_plant_advance)
    if (const char* why = plant_geometry_refusal(c, c->plant_mode)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  }
  TRY(plant_scores_ready(c, count));
  const ilqr::PlantPlan plan = plant_plan_of(c, true);
  TRY(prepare_plant(c, plan));
  const h1::DynParams dyn = plant_dyn(c);
  const long row0 = c->hist_cap > 0 ? c->hist_n % c->hist_cap : 0L;
  enqueue_plant(c, plan, dyn, geom ? 1 : 0, first_knot, count, row0);
  enqueue_score(c, row0, first_knot, count);
  enqueue_task_score(c, row0, first_knot, count);
  HIPCHK(c, hipGetLastError());
  c->plant_kick = false;
  c->plant_intervals += count;
  if (c->hist_cap > 0) c->hist_n += count;
  return ILQR_OK;      // asynchronous on the handle's stream
}
int ilqr_hip_initialize_warm_from_plant_shifted(ilqr_hip_ctx* c, int shift) {
  if (!c || shift < 1 || shift > c->N - 1) return ILQR_ERR_ARG;
  if (!c->initialized || !c->plant_set) return ILQR_ERR_STATE;
  TRY(enter_launching(c));
  TRY(enqueue_measured_x0(c, c->S.x0));
  return warm_shifted(c, shift);      // asynchronous on the handle's stream
}
int ilqr_hip_plant_set_history(ilqr_hip_ctx* c, int steps) {
  if (!c || steps < 0) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (an advance in flight may still write the ring)
  if (c->plant.hist_x) hipFree(c->plant.hist_x);
  if (c->plant.hist_u) hipFree(c->plant.hist_u);
  c->plant.hist_x = c->plant.hist_u = nullptr; c->hist_cap = 0; c->hist_n = 0;
  if (steps > 0) {
    HIPCHK(c, hipMalloc((void**)&c->plant.hist_x, (size_t)steps * c->B * ILQR_NX * sizeof(double)));
    HIPCHK(c, hipMalloc((void**)&c->plant.hist_u, (size_t)steps * c->B * ILQR_NU * sizeof(double)));
    c->hist_cap = steps;
  }
  return ILQR_OK;
}
int ilqr_hip_plant_get_history(ilqr_hip_ctx* c, double* x, double* u, int* steps_recorded) {
  if (!c || !steps_recorded) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const long cap = c->hist_cap, rec = c->hist_n < cap ? c->hist_n : cap;
  *steps_recorded = (int)rec;
  // oldest row first.  A ring that has not wrapped is one contiguous run; one that has is two: rows [first, cap) then [0, first)
  const long first = c->hist_n > cap ? c->hist_n % cap : 0;
  const long head = rec - first;      // rows of the first run
  const size_t rx = (size_t)c->B * ILQR_NX, ru = (size_t)c->B * ILQR_NU;
  if (x && head > 0) HIPCHK(c, hipMemcpy(x, c->plant.hist_x + first * rx, head * rx * sizeof(double), hipMemcpyDeviceToHost));
  if (x && first > 0) HIPCHK(c, hipMemcpy(x + head * rx, c->plant.hist_x, first * rx * sizeof(double), hipMemcpyDeviceToHost));
  if (u && head > 0) HIPCHK(c, hipMemcpy(u, c->plant.hist_u + first * ru, head * ru * sizeof(double), hipMemcpyDeviceToHost));
  if (u && first > 0) HIPCHK(c, hipMemcpy(u + head * ru, c->plant.hist_u, first * ru * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
#define PLANT_GETTER(name, ptr, count, type)                                                                    \
  int name(ilqr_hip_ctx* c, type* out) {                                                                        \
    if (!c || !out) return ILQR_ERR_ARG;                                                                        \
    if (!c->plant_set) return ILQR_ERR_STATE;                                                                   \
    enter(c);                                                                                                   \
    HIPCHK(c, hipStreamSynchronize(c->stream));                                                                 \
    HIPCHK(c, hipMemcpy(out, c->plant.ptr, (size_t)(count) * sizeof(type), hipMemcpyDeviceToHost));             \
    return ILQR_OK;                                                                                             \
  }
PLANT_GETTER(ilqr_hip_plant_get_state, x, (size_t)c->B * ILQR_NX, double)
PLANT_GETTER(ilqr_hip_plant_get_control, u, (size_t)c->B * ILQR_NU, double)
PLANT_GETTER(ilqr_hip_plant_get_stance, stance, (size_t)c->B * 2, int)
PLANT_GETTER(ilqr_hip_plant_get_alive, alive, c->B, int)
int ilqr_hip_plant_state_device(ilqr_hip_ctx* c, const double** x_device) {
  if (!c || !x_device) return ILQR_ERR_ARG;
  *x_device = c->plant.x;
  return ILQR_OK;
}
// ---- the plant's own model and its parameter sets (plant_kernels.hip k_plant_follow_p)
int ilqr_hip_plant_set_model(ilqr_hip_ctx* c, int contact_mode, int joint_limits) {
  if (!c || contact_mode < -1 || contact_mode > ILQR_CONTACT_KINETIC_FRICTION_STANCE || joint_limits < -1 || joint_limits > 1) return ILQR_ERR_ARG;
  enter(c);
  if (c->plant_source == ILQR_STANCE_GEOMETRY) {
    if (const char* why = plant_geometry_refusal(c, contact_mode)) { c->err = why; return ILQR_ERR_UNSUPPORTED; }
  }
  c->plant_mode = contact_mode; c->plant_limits = joint_limits;
  return ILQR_OK;
}
// ---- what the entry points of the seven tables share (ilqr_hip_ctx::TableBuf); their argument checks, their no-table values and whatever else is
// specific to a table stay with them
using TableBuf = ilqr_hip_ctx::TableBuf;
// installs n_sets records of `values` doubles, padded with zeros to `rec` doubles on the device
static int table_install(ilqr_hip_ctx* c, TableBuf* t, const double* v, int n_sets, int values, int rec) {
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (a plant call in flight may still read the table this one replaces)
  if (t->d && t->sets != n_sets) { hipFree(t->d); t->d = nullptr; t->sets = 0; }
  if (!t->d) HIPCHK(c, hipMalloc((void**)&t->d, (size_t)n_sets * rec * sizeof(double)));
  t->sets = n_sets;
  return upload_rows(c, t->d, v, n_sets, values, rec);
}
static int table_clear(ilqr_hip_ctx* c, TableBuf* t) {
  if (t->d) {
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (a plant call in flight may still read it)
    hipFree(t->d);
  }
  t->d = nullptr; t->sets = 0;
  return ILQR_OK;
}
// the installed table as [B][values]: one record for all is repeated
static int table_read(ilqr_hip_ctx* c, const TableBuf& t, double* out, int values, int rec) {
  std::vector<double> r((size_t)t.sets * rec);
  HIPCHK(c, hipMemcpyAsync(r.data(), t.d, r.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < c->B; ++b) std::memcpy(out + (size_t)b * values, r.data() + (size_t)(t.sets == 1 ? 0 : b) * rec, values * sizeof(double));
  return ILQR_OK;
}
int ilqr_hip_plant_set_params(ilqr_hip_ctx* c, const double* params, int n_sets) {
  if (!c || !params || n_sets < 1 || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  constexpr int P = ILQR_PLANT_PARAMS;
  for (size_t i = 0; i < (size_t)n_sets * P; ++i) if (!std::isfinite(params[i])) return ILQR_ERR_ARG;
  for (int s = 0; s < n_sets; ++s) {
    const double* r = params + (size_t)s * P;
    if (r[3] < 0.0 || !(r[4] > 0.0) || r[5] < 0.0 || r[6] < 0.0) return ILQR_ERR_ARG;
  }
  enter(c);
  return table_install(c, &c->pparams, params, n_sets, P, P + 1);      // (64-byte records: the seven values and one double of padding)
}
int ilqr_hip_plant_clear_params(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  return table_clear(c, &c->pparams);
}
int ilqr_hip_plant_num_param_sets(const ilqr_hip_ctx* c) { return c ? c->pparams.sets : -1; }
int ilqr_hip_plant_get_params(ilqr_hip_ctx* c, double* params) {
  if (!c || !params) return ILQR_ERR_ARG;
  enter(c);
  constexpr int P = ILQR_PLANT_PARAMS;
  if (!c->pparams.d) {
    const h1::DynParams& d = c->P.dyn;
    for (int b = 0; b < c->B; ++b) {
      double* r = params + (size_t)b * P;
      r[0] = d.g[0]; r[1] = d.g[1]; r[2] = d.g[2]; r[3] = d.mu; r[4] = d.soft; r[5] = d.lim_k; r[6] = 1.0;
    }
    return ILQR_OK;
  }
  return table_read(c, c->pparams, params, P, P + 1);
}
// ---- external wrench on the pelvis per rollout (plant_kernels.hip k_plant_follow_w, k_step_w)
// the checks of a wrench record that need no handle: every entry finite but end = +inf, first / end non-negative integers, first <= end
static bool wrench_values_ok(const double* r, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(r[i]) && !(n == ILQR_PLANT_WRENCH && i == 10 && r[i] > 0.0 && std::isinf(r[i]))) return false;
  if (n == ILQR_PLANT_WRENCH) {
    if (r[9] < 0.0 || r[10] < 0.0 || r[9] != std::floor(r[9]) || (std::isfinite(r[10]) && r[10] != std::floor(r[10])) || r[10] < r[9]) return false;
  }
  return true;
}
int ilqr_hip_plant_set_wrench(ilqr_hip_ctx* c, const double* wrench, int n_sets) {
  if (!wrench || n_sets < 1) return ILQR_ERR_ARG;
  for (int s = 0; s < n_sets; ++s) if (!wrench_values_ok(wrench + (size_t)s * ILQR_PLANT_WRENCH, ILQR_PLANT_WRENCH)) return ILQR_ERR_ARG;
  if (!c || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  TRY(need_module(c, ilqr::MOD_WRENCH));
  return table_install(c, &c->wrench, wrench, n_sets, ILQR_PLANT_WRENCH, WRENCH_REC);      // (128-byte records: the eleven values and five doubles of padding)
}
int ilqr_hip_plant_clear_wrench(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  return table_clear(c, &c->wrench);
}
int ilqr_hip_plant_num_wrench_sets(const ilqr_hip_ctx* c) { return c ? c->wrench.sets : -1; }
int ilqr_hip_plant_get_wrench(ilqr_hip_ctx* c, double* wrench) {
  if (!c || !wrench) return ILQR_ERR_ARG;
  enter(c);
  if (!c->wrench.d) {      // (no table: no wrench, an empty window)
    std::fill(wrench, wrench + (size_t)c->B * ILQR_PLANT_WRENCH, 0.0);
    return ILQR_OK;
  }
  return table_read(c, c->wrench, wrench, ILQR_PLANT_WRENCH, WRENCH_REC);
}
long ilqr_hip_plant_intervals(const ilqr_hip_ctx* c) { return c ? c->plant_intervals : -1L; }
// ---- rigid payload on the pelvis per rollout (plant_kernels.hip k_plant_follow_m, k_step_m)
// the checks of a payload record that need no handle: every entry finite, m >= 0, Ic positive semidefinite -- its seven principal minors
// non-negative up to rounding (relative to the products they are differences of)
static bool payload_values_ok(const double* r) {
  for (int i = 0; i < ILQR_PLANT_PAYLOAD; ++i) if (!std::isfinite(r[i])) return false;
  if (r[0] < 0.0) return false;
  const double xx = r[4], yy = r[5], zz = r[6], xy = r[7], xz = r[8], yz = r[9];
  const double eps = 1e-12;
  if (xx < 0.0 || yy < 0.0 || zz < 0.0) return false;
  if (xx * yy - xy * xy < -eps * (xx * yy + xy * xy) || xx * zz - xz * xz < -eps * (xx * zz + xz * xz) || yy * zz - yz * yz < -eps * (yy * zz + yz * yz)) return false;
  const double det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
  const double mag = std::fabs(xx * yy * zz) + std::fabs(xx * yz * yz) + std::fabs(xy * xy * zz) + 2.0 * std::fabs(xy * yz * xz) + std::fabs(yy * xz * xz);
  return det >= -eps * mag;
}
int ilqr_hip_plant_set_payload(ilqr_hip_ctx* c, const double* payload, int n_sets) {
  if (!payload || n_sets < 1) return ILQR_ERR_ARG;
  for (int s = 0; s < n_sets; ++s) if (!payload_values_ok(payload + (size_t)s * ILQR_PLANT_PAYLOAD)) return ILQR_ERR_ARG;
  if (!c || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  TRY(need_module(c, ilqr::MOD_PAYLOAD));
  return table_install(c, &c->payload, payload, n_sets, ILQR_PLANT_PAYLOAD, PAYLOAD_REC);      // (128-byte records: the ten values and six doubles of padding)
}
int ilqr_hip_plant_clear_payload(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  return table_clear(c, &c->payload);
}
int ilqr_hip_plant_num_payload_sets(const ilqr_hip_ctx* c) { return c ? c->payload.sets : -1; }
int ilqr_hip_plant_get_payload(ilqr_hip_ctx* c, double* payload) {
  if (!c || !payload) return ILQR_ERR_ARG;
  enter(c);
  if (!c->payload.d) {      // (no table: nothing carried)
    std::fill(payload, payload + (size_t)c->B * ILQR_PLANT_PAYLOAD, 0.0);
    return ILQR_OK;
  }
  return table_read(c, c->payload, payload, ILQR_PLANT_PAYLOAD, PAYLOAD_REC);
}
// ---- noisy and biased state observation per rollout (plant_kernels.hip k_observation_draw, k_observe_apply, k_plant_follow_o)
int ilqr_hip_plant_set_observation(ilqr_hip_ctx* c, const double* obs, int n_sets, unsigned long long seed, unsigned long long stream0) {
  if (!obs || n_sets < 1) return ILQR_ERR_ARG;
  constexpr int R = ILQR_PLANT_OBSERVATION;
  for (size_t i = 0; i < (size_t)n_sets * R; ++i) {
    if (!std::isfinite(obs[i])) return ILQR_ERR_ARG;
    if (i % R >= R / 2 && obs[i] < 0.0) return ILQR_ERR_ARG;      // (sigma)
  }
  if (!c || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  TRY(need_module(c, ilqr::MOD_OBSERVE));
  if (!c->d_obs_delta) HIPCHK(c, hipMalloc((void**)&c->d_obs_delta, (size_t)c->N * c->B * ILQR_NX * sizeof(double)));
  if (!c->d_obs_x) HIPCHK(c, hipMalloc((void**)&c->d_obs_x, (size_t)c->B * ILQR_NX * sizeof(double)));
  TRY(table_install(c, &c->obs, obs, n_sets, R, R));
  c->obs_seed = seed; c->obs_stream0 = stream0;
  return ILQR_OK;
}
int ilqr_hip_plant_clear_observation(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  TRY(table_clear(c, &c->obs));
  c->obs_seed = 0; c->obs_stream0 = 0;
  return ILQR_OK;
}
int ilqr_hip_plant_num_observation_sets(const ilqr_hip_ctx* c) { return c ? c->obs.sets : -1; }
int ilqr_hip_plant_get_observation(ilqr_hip_ctx* c, double* obs, unsigned long long* seed, unsigned long long* stream0) {
  if (!c || !obs) return ILQR_ERR_ARG;
  enter(c);
  constexpr int R = ILQR_PLANT_OBSERVATION;
  if (seed) *seed = c->obs_seed;
  if (stream0) *stream0 = c->obs_stream0;
  if (!c->obs.d) {      // (no table: the controller sees the truth)
    std::fill(obs, obs + (size_t)c->B * R, 0.0);
    return ILQR_OK;
  }
  return table_read(c, c->obs, obs, R, R);
}
int ilqr_hip_plant_observation_errors(ilqr_hip_ctx* c, long interval0, int count, double* delta) {
  if (!c || !delta || interval0 < 0 || count < 1 || count > c->N) return ILQR_ERR_ARG;
  if (!c->obs.d) { c->err = "plant_observation_errors without an observation table (ilqr_hip_plant_set_observation)"; return ILQR_ERR_STATE; }
  TRY(enter_launching(c));
  TRY(need_module(c, ilqr::MOD_OBSERVE));
  enqueue_observation_draw(c, interval0, count);      // (the buffer of the plant calls: they draw again in front of every use)
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(delta, c->d_obs_delta, (size_t)count * c->B * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_plant_get_observed(ilqr_hip_ctx* c, double* x_obs) {
  if (!c || !x_obs) return ILQR_ERR_ARG;
  if (!c->plant_set) return ILQR_ERR_STATE;
  if (!c->obs.d) return ilqr_hip_plant_get_state(c, x_obs);
  TRY(enter_launching(c));
  TRY(enqueue_measured_x0(c, c->d_obs_x));
  HIPCHK(c, hipMemcpyAsync(x_obs, c->d_obs_x, (size_t)c->B * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
// ---- actuator delay, lag and torque noise per rollout (plant_kernels.hip k_actuator_draw, k_plant_follow_a)
int ilqr_hip_plant_set_actuator(ilqr_hip_ctx* c, const double* act, int n_sets, unsigned long long seed, unsigned long long stream0) {
  if (!act || n_sets < 1) return ILQR_ERR_ARG;
  constexpr int R = ILQR_PLANT_ACTUATOR;
  for (size_t i = 0; i < (size_t)n_sets * R; ++i) {
    if (!std::isfinite(act[i]) || act[i] < 0.0) return ILQR_ERR_ARG;      // (delay, tau and sigma are all non-negative)
    if (i % R == 0 && (act[i] > ILQR_PLANT_ACTUATOR_MAX_DELAY || act[i] != std::floor(act[i]))) return ILQR_ERR_ARG;
  }
  if (!c || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  TRY(need_module(c, ilqr::MOD_ACTUATOR));
  const bool resized = c->act.d && c->act.sets != n_sets;
  TRY(table_install(c, &c->act, act, n_sets, R, R));
  if (resized) { hipFree(c->d_act_beta); c->d_act_beta = nullptr; }      // (the blend rows follow the table's size; nothing is in flight behind table_install)
  const size_t bu = (size_t)c->B * ILQR_NU;
  if (!c->d_act_z) HIPCHK(c, hipMalloc((void**)&c->d_act_z, (size_t)c->N * bu * sizeof(double)));
  if (!c->d_act_fifo) HIPCHK(c, hipMalloc((void**)&c->d_act_fifo, (size_t)(ILQR_PLANT_ACTUATOR_MAX_DELAY + 1) * bu * sizeof(double)));
  if (!c->d_act_y) HIPCHK(c, hipMalloc((void**)&c->d_act_y, bu * sizeof(double)));
  if (!c->d_act_applied) { HIPCHK(c, hipMalloc((void**)&c->d_act_applied, bu * sizeof(double))); HIPCHK(c, hipMemsetAsync(c->d_act_applied, 0, bu * sizeof(double), c->stream)); }
  if (!c->d_act_beta) HIPCHK(c, hipMalloc((void**)&c->d_act_beta, (size_t)n_sets * ILQR_NU * sizeof(double)));
  c->act_seed = seed; c->act_stream0 = stream0;
  c->act_rec.assign(act, act + (size_t)n_sets * R);
  c->act_substeps = 0;      // (the actuator's state is primed again by the next substep)
  return upload_actuator_blend(c);      // (synchronises the stream)
}
int ilqr_hip_plant_clear_actuator(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  const bool installed = c->act.d != nullptr;
  TRY(table_clear(c, &c->act));
  if (installed) hipFree(c->d_act_beta);
  c->d_act_beta = nullptr; c->act_seed = 0; c->act_stream0 = 0; c->act_substeps = 0;
  c->act_rec.clear(); c->act_beta.clear();
  return ILQR_OK;
}
int ilqr_hip_plant_num_actuator_sets(const ilqr_hip_ctx* c) { return c ? c->act.sets : -1; }
int ilqr_hip_plant_get_actuator(ilqr_hip_ctx* c, double* act, unsigned long long* seed, unsigned long long* stream0) {
  if (!c || !act) return ILQR_ERR_ARG;
  enter(c);
  constexpr int R = ILQR_PLANT_ACTUATOR;
  if (seed) *seed = c->act_seed;
  if (stream0) *stream0 = c->act_stream0;
  if (!c->act.d) {      // (no table: the command is the torque)
    std::fill(act, act + (size_t)c->B * R, 0.0);
    return ILQR_OK;
  }
  return table_read(c, c->act, act, R, R);
}
int ilqr_hip_plant_get_actuator_blend(ilqr_hip_ctx* c, double* beta) {
  if (!c || !beta) return ILQR_ERR_ARG;
  enter(c);
  if (!c->act.d) { c->err = "plant_get_actuator_blend without an actuator table (ilqr_hip_plant_set_actuator)"; return ILQR_ERR_STATE; }
  return table_read(c, TableBuf{c->d_act_beta, c->act.sets}, beta, ILQR_NU, ILQR_NU);      // (from the device: the rows the kernel reads)
}
int ilqr_hip_plant_actuator_draws(ilqr_hip_ctx* c, long interval0, int count, double* z) {
  if (!c || !z || interval0 < 0 || count < 1 || count > c->N) return ILQR_ERR_ARG;
  if (!c->act.d) { c->err = "plant_actuator_draws without an actuator table (ilqr_hip_plant_set_actuator)"; return ILQR_ERR_STATE; }
  TRY(enter_launching(c));
  TRY(need_module(c, ilqr::MOD_ACTUATOR));
  enqueue_actuator_draw(c, interval0, count);      // (the buffer of the plant calls: they draw again in front of every use)
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(z, c->d_act_z, (size_t)count * c->B * ILQR_NU * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_plant_get_applied(ilqr_hip_ctx* c, double* tau) {
  if (!c || !tau) return ILQR_ERR_ARG;
  if (!c->plant_set) return ILQR_ERR_STATE;
  if (!c->act.d) return ilqr_hip_plant_get_control(c, tau);
  enter(c);
  HIPCHK(c, hipMemcpyAsync(tau, c->d_act_applied, (size_t)c->B * ILQR_NU * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
// ---- joint gain, torque range, damping and armature per rollout (plant_kernels.hip k_plant_follow_j, k_step_j)
static bool joint_values_ok(const double* j, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(j[i]) || j[i] < 0.0) return false;
  return true;
}
int ilqr_hip_plant_set_joints(ilqr_hip_ctx* c, const double* joints, int n_sets) {
  if (!c) return ILQR_ERR_ARG;
  constexpr int P = ILQR_PLANT_JOINTS;
  if (!joints || n_sets == 0) {      // clears
    if (joints || n_sets != 0) return ILQR_ERR_ARG;
    enter(c);
    TRY(table_clear(c, &c->joints));
    c->joints_nominal = false;
    return ILQR_OK;
  }
  if (n_sets < 1 || !joint_values_ok(joints, (size_t)n_sets * P) || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  TRY(need_module(c, ilqr::MOD_JOINTS));
  bool nominal = true;
  for (int s = 0; s < n_sets; ++s) {
    const double* r = joints + (size_t)s * P;
    for (int i = 0; i < ILQR_NU; ++i) nominal = nominal && r[i] == 1.0 && r[ILQR_NU + i] == 1.0 && r[2 * ILQR_NU + i] == 1.0 && r[3 * ILQR_NU + i] == 0.1;
  }
  TRY(table_install(c, &c->joints, joints, n_sets, P, JOINT_REC));      // (640-byte records: the 76 values and four doubles of padding)
  c->joints_nominal = nominal;
  return ILQR_OK;
}
int ilqr_hip_plant_get_joints(ilqr_hip_ctx* c, double* joints) {
  if (!c || !joints) return ILQR_ERR_ARG;
  enter(c);
  constexpr int P = ILQR_PLANT_JOINTS;
  if (!c->joints.d) {      // (no table: the model's joints)
    for (size_t i = 0; i < (size_t)c->B * P; ++i) joints[i] = i % P < 3 * ILQR_NU ? 1.0 : 0.1;
    return ILQR_OK;
  }
  return table_read(c, c->joints, joints, P, JOINT_REC);
}
// ---- a floor of its own height under each foot per rollout (plant_kernels.hip k_plant_follow_t, k_step_t; the rule: h1_host_model.cpp terrain_stance)
// the checks that need no handle: z_left, z_right finite, edge_x finite or -inf, and with n == ILQR_PLANT_TERRAIN the wrench's window
static bool terrain_values_ok(const double* r, int n) {
  if (!std::isfinite(r[0]) || !std::isfinite(r[1]) || !(std::isfinite(r[2]) || (r[2] < 0.0 && std::isinf(r[2])))) return false;
  if (n == ILQR_PLANT_TERRAIN) {
    double w[ILQR_PLANT_WRENCH] = {0};
    w[9] = r[3]; w[10] = r[4];
    return wrench_values_ok(w, ILQR_PLANT_WRENCH);
  }
  return true;
}
int ilqr_hip_plant_set_terrain(ilqr_hip_ctx* c, const double* terrain, int n_sets) {
  if (!terrain || n_sets < 1) return ILQR_ERR_ARG;
  for (int s = 0; s < n_sets; ++s) if (!terrain_values_ok(terrain + (size_t)s * ILQR_PLANT_TERRAIN, ILQR_PLANT_TERRAIN)) return ILQR_ERR_ARG;
  if (!c || check_sets(c, n_sets)) return ILQR_ERR_ARG;
  enter(c);
  TRY(need_module(c, ilqr::MOD_TERRAIN));
  return table_install(c, &c->terrain, terrain, n_sets, ILQR_PLANT_TERRAIN, TERRAIN_REC);      // (64-byte records: the five values and three doubles of padding)
}
int ilqr_hip_plant_clear_terrain(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  enter(c);
  return table_clear(c, &c->terrain);
}
int ilqr_hip_plant_num_terrain_sets(const ilqr_hip_ctx* c) { return c ? c->terrain.sets : -1; }
int ilqr_hip_plant_get_terrain(ilqr_hip_ctx* c, double* terrain) {
  if (!c || !terrain) return ILQR_ERR_ARG;
  enter(c);
  if (!c->terrain.d) {      // (no table: the solver's ground, a window that is shut)
    for (size_t i = 0; i < (size_t)c->B * ILQR_PLANT_TERRAIN; ++i) terrain[i] = i % ILQR_PLANT_TERRAIN == 2 ? -HUGE_VAL : 0.0;
    return ILQR_OK;
  }
  return table_read(c, c->terrain, terrain, ILQR_PLANT_TERRAIN, TERRAIN_REC);
}
int ilqr_hip_step_terrain(ilqr_hip_ctx* c, int count, const double* x, const double* u, const double* terrain, double* x_next, int* stance_out) {
  if (count <= 0 || !x || !u || !terrain || !x_next || !stance_out) return ILQR_ERR_ARG;
  for (int i = 0; i < count; ++i) if (!terrain_values_ok(terrain + (size_t)i * 3, 3)) return ILQR_ERR_ARG;
  if (!c) return ILQR_ERR_ARG;
  if (c->P.dyn.contact == ILQR_CONTACT_NONE || c->P.dyn.contact == ILQR_CONTACT_RIGID_STANCE) {
    c->err = "step_terrain in contact mode 0 or 1: no foot lands or lifts by the floor's height; use mode 2, 3 or 4";
    return ILQR_ERR_UNSUPPORTED;
  }
  TRY(enter_launching(c));
  TRY(need_module(c, ilqr::MOD_TERRAIN));
  const size_t n = (size_t)count;
  TRY(grow_step_buffer(c, &c->d_stept, &c->step_t_cap, n, 4));
  TRY(grow_step_scratch(c, count));
  int* d_flags = (int*)(c->d_stept + n * 3);      // (behind the floors: 2 ints per item)
  HIPCHK(c, hipMemcpyAsync(c->d_stepx, x, n * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_stepu, u, n * ILQR_NU * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_stept, terrain, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  module_fn<ilqr::terrain_step_fn>(ilqr::MOD_TERRAIN, FN_STEP)(count, c->d_stepx, c->d_stepu, &c->P.dyn, c->d_stepn, c->d_stept, d_flags, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(x_next, c->d_stepn, n * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(stance_out, d_flags, n * 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_terrain_stance(const double* qpos, const double* terrain, long interval, int* stance, double* floor) {
  if (!qpos || !terrain || !stance || interval < 0 || !terrain_values_ok(terrain, ILQR_PLANT_TERRAIN)) return ILQR_ERR_ARG;
  for (int i = 0; i < ILQR_NQ; ++i) if (!std::isfinite(qpos[i])) return ILQR_ERR_ARG;
  h1host::terrain_stance(qpos, terrain, interval, stance, floor);
  return ILQR_OK;
}
// ---- single steps under a wrench, a payload and a joint record per item: ONE body behind the argument checks of the three entry points.
// `which` is the entry point's own module, whose step kernel runs (k_step_w / k_step_m / k_step_j); it takes the arrays of the modules before
// it, of which `wrench` and `payload` may be null where the entry point allows it.
static int step_in_module(ilqr_hip_ctx* c, ilqr::PlantModule which, int count, const double* x, const double* u, int stance_left, int stance_right, const double* wrench, const double* payload,
                          const double* joints, double* x_next) {
  TRY(enter_launching(c));
  TRY(need_module(c, which));
  const size_t n = (size_t)count;
  if (wrench) TRY(grow_step_buffer(c, &c->d_stepw, &c->step_w_cap, n, 9));
  if (payload) TRY(grow_step_buffer(c, &c->d_stepm, &c->step_m_cap, n, ILQR_PLANT_PAYLOAD));
  if (joints) TRY(grow_step_buffer(c, &c->d_stepj, &c->step_j_cap, n, ILQR_PLANT_JOINTS));
  TRY(grow_step_scratch(c, count));
  HIPCHK(c, hipMemcpyAsync(c->d_stepx, x, n * ILQR_NX * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_stepu, u, n * ILQR_NU * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (wrench) HIPCHK(c, hipMemcpyAsync(c->d_stepw, wrench, n * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (payload) HIPCHK(c, hipMemcpyAsync(c->d_stepm, payload, n * ILQR_PLANT_PAYLOAD * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (joints) HIPCHK(c, hipMemcpyAsync(c->d_stepj, joints, n * ILQR_PLANT_JOINTS * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const double *w = wrench ? c->d_stepw : nullptr, *m = payload ? c->d_stepm : nullptr;
  module_fn<ilqr::plant_step_fn>(which, FN_STEP)(count, c->d_stepx, c->d_stepu, &c->P.dyn, c->d_stepn, stance_left, stance_right, w, m, joints ? c->d_stepj : nullptr, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(x_next, c->d_stepn, n * ILQR_NX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
int ilqr_hip_step_wrench(ilqr_hip_ctx* c, int count, const double* x, const double* u, int stance_left, int stance_right, const double* wrench, double* x_next) {
  if (count <= 0 || !x || !u || !wrench || !x_next) return ILQR_ERR_ARG;
  for (int i = 0; i < count; ++i) if (!wrench_values_ok(wrench + (size_t)i * 9, 9)) return ILQR_ERR_ARG;
  if (!c) return ILQR_ERR_ARG;
  return step_in_module(c, ilqr::MOD_WRENCH, count, x, u, stance_left, stance_right, wrench, nullptr, nullptr, x_next);
}
int ilqr_hip_step_payload(ilqr_hip_ctx* c, int count, const double* x, const double* u, int stance_left, int stance_right, const double* wrench, const double* payload, double* x_next) {
  if (count <= 0 || !x || !u || !payload || !x_next) return ILQR_ERR_ARG;
  for (int i = 0; i < count; ++i) {
    if (wrench && !wrench_values_ok(wrench + (size_t)i * 9, 9)) return ILQR_ERR_ARG;
    if (!payload_values_ok(payload + (size_t)i * ILQR_PLANT_PAYLOAD)) return ILQR_ERR_ARG;
  }
  if (!c) return ILQR_ERR_ARG;
  return step_in_module(c, ilqr::MOD_PAYLOAD, count, x, u, stance_left, stance_right, wrench, payload, nullptr, x_next);
}
int ilqr_hip_step_joints(ilqr_hip_ctx* c, int count, const double* x, const double* u, int stance_left, int stance_right, const double* wrench, const double* payload, const double* joints,
                         double* x_next) {
  if (count <= 0 || !x || !u || !joints || !x_next) return ILQR_ERR_ARG;
  for (int i = 0; i < count; ++i) {
    if (wrench && !wrench_values_ok(wrench + (size_t)i * 9, 9)) return ILQR_ERR_ARG;
    if (payload && !payload_values_ok(payload + (size_t)i * ILQR_PLANT_PAYLOAD)) return ILQR_ERR_ARG;
  }
  if (!joint_values_ok(joints, (size_t)count * ILQR_PLANT_JOINTS) || !c) return ILQR_ERR_ARG;
  return step_in_module(c, ilqr::MOD_JOINTS, count, x, u, stance_left, stance_right, wrench, payload, joints, x_next);
}
void ilqr_hip_pelvis_inertial_offset(double r[3]) {
  if (r) h1host::pelvis_inertial_offset(r);      // (host table: the model constants of this translation unit are device constants)
}
// ---- closed-loop score of the plant (plant_score_kernels.hip)
__attribute__((minsize)) int ilqr_hip_plant_set_score(ilqr_hip_ctx* c, const double* Q_diag, const double* R_diag, double w_upright, double w_balance, double w_joint_limits, double w_control_limits) {
  if (!c || !Q_diag || !R_diag) return ILQR_ERR_ARG;
  const double w[4] = {w_upright, w_balance, w_joint_limits, w_control_limits};
  for (double v : w) if (!(v >= 0.0) || !std::isfinite(v)) return ILQR_ERR_ARG;
  for (int i = 0; i < ILQR_NX; ++i) if (!(Q_diag[i] >= 0.0) || !std::isfinite(Q_diag[i])) return ILQR_ERR_ARG;
  for (int i = 0; i < ILQR_NU; ++i) if (!(R_diag[i] >= 0.0) || !std::isfinite(R_diag[i])) return ILQR_ERR_ARG;
  enter(c);
  const size_t rec = (size_t)c->B * ILQR_PLANT_SCORE_TERMS;
  if (!c->d_score) HIPCHK(c, hipMalloc((void**)&c->d_score, rec * sizeof(double)));
  if (!c->d_score_terms) HIPCHK(c, hipMalloc((void**)&c->d_score_terms, (size_t)c->N * rec * sizeof(double)));
  std::memcpy(c->score_Q, Q_diag, sizeof(c->score_Q)); std::memcpy(c->score_R, R_diag, sizeof(c->score_R)); std::memcpy(c->score_w, w, sizeof(c->score_w));
  c->score_on = true;
  const std::vector<double> empty = empty_score(c);
  // (on the stream: behind the score kernels of a plant call still in flight, which then scored under the weights of their own call)
  HIPCHK(c, hipMemcpyAsync(c->d_score, empty.data(), rec * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ILQR_OK;
}
// one body per operation for the two records (the cost score's and the task score's: [B][8] each, installed while `rec` is set)
static_assert(ILQR_PLANT_TASK_SCORE_TERMS == ILQR_PLANT_SCORE_TERMS && PLANT_TASK_SCORE_TERMS == ILQR_PLANT_TASK_SCORE_TERMS, "both records are [B][8]");
__attribute__((noinline, minsize)) static int score_free(ilqr_hip_ctx* c, double** rec, double** terms) {
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));      // (score kernels in flight still write the buffers)
  if (*rec) hipFree(*rec);
  if (*terms) hipFree(*terms);
  *rec = *terms = nullptr;
  return ILQR_OK;
}
// out: the record on the host (synchronises), or dev: its device pointer
__attribute__((noinline, minsize)) static int score_read(ilqr_hip_ctx* c, const double* rec, double* out, const double** dev) {
  if (!out && !dev) return ILQR_ERR_ARG;
  if (!rec) return ILQR_ERR_STATE;
  if (dev) { *dev = rec; return ILQR_OK; }
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(out, rec, (size_t)c->B * ILQR_PLANT_SCORE_TERMS * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_plant_clear_score(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  c->score_on = false;
  return score_free(c, &c->d_score, &c->d_score_terms);
}
int ilqr_hip_plant_get_score(ilqr_hip_ctx* c, double* score) { return c ? score_read(c, c->score_on ? c->d_score : nullptr, score, nullptr) : ILQR_ERR_ARG; }
int ilqr_hip_plant_score_device(ilqr_hip_ctx* c, const double** score_device) { return c ? score_read(c, c->score_on ? c->d_score : nullptr, nullptr, score_device) : ILQR_ERR_ARG; }
// ---- task score of the plant (plant_task_score_kernels.hip, in the per-knot module)
__attribute__((minsize)) int ilqr_hip_plant_set_task_score(ilqr_hip_ctx* c, double tol) {
  if (!c || !(tol >= 0.0) || !std::isfinite(tol)) return ILQR_ERR_ARG;
  enter(c);
  const size_t rec = (size_t)c->B * ILQR_PLANT_TASK_SCORE_TERMS;
  if (!c->d_tscore_terms) TRY(dalloc(c, &c->d_tscore_terms, (size_t)c->N * rec));
  if (!c->d_tscore) TRY(dalloc(c, &c->d_tscore, rec));
  c->tscore_tol = tol;      // (kernels of a plant call in flight took their tolerance by value)
  return task_score_empty(c);
}
int ilqr_hip_plant_clear_task_score(ilqr_hip_ctx* c) { return c ? score_free(c, &c->d_tscore, &c->d_tscore_terms) : ILQR_ERR_ARG; }
int ilqr_hip_plant_get_task_score(ilqr_hip_ctx* c, double* score) { return c ? score_read(c, c->d_tscore, score, nullptr) : ILQR_ERR_ARG; }
int ilqr_hip_plant_task_score_device(ilqr_hip_ctx* c, const double** score_device) { return c ? score_read(c, c->d_tscore, nullptr, score_device) : ILQR_ERR_ARG; }
int ilqr_hip_get_iterations_enqueued(const ilqr_hip_ctx* c) { return c ? c->iterations_enqueued : -1; }
int ilqr_hip_get_adopt_mismatches(ilqr_hip_ctx* c, unsigned long long* count) {
  if (!c || !count) return ILQR_ERR_ARG;
  enter(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(count, c->d_mismatch, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return ILQR_OK;
}

// ---------------------------------------------------------------- multi-GPU: the ONE collective of an MPC step
// RCCL (librccl.so.1) is opened on first use; a process that never shards never loads it.
namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string err;
};
Rccl g_rccl;
std::once_flag g_rccl_once;
bool g_rccl_ok = false;
// Opened and resolved exactly once per process, whichever host thread gets there first (the multi-GPU C++ model is one thread
// and one handle per GPU, tests/cpp/cpp_multi_gpu_demo.cpp); the table is published only after every symbol has resolved.
bool rccl_load() {
  std::call_once(g_rccl_once, [] {
    Rccl R;
    const char* names[] = {getenv("ILQR_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* lib = nullptr;
    for (const char* n : names) { if (n && (lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break; }
    if (!lib) { const char* de = dlerror(); g_rccl.err = std::string("cannot open librccl: ") + (de ? de : "?"); return; }
    bool ok = true;
    auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p) { ok = false; g_rccl.err = std::string("librccl lacks ") + n; } return p; };
    R.GetUniqueId = (decltype(R.GetUniqueId))sym("ncclGetUniqueId");
    R.CommInitRank = (decltype(R.CommInitRank))sym("ncclCommInitRank");
    R.CommDestroy = (decltype(R.CommDestroy))sym("ncclCommDestroy");
    R.Send = (decltype(R.Send))sym("ncclSend");
    R.Recv = (decltype(R.Recv))sym("ncclRecv");
    R.GroupStart = (decltype(R.GroupStart))sym("ncclGroupStart");
    R.GroupEnd = (decltype(R.GroupEnd))sym("ncclGroupEnd");
    R.GetErrorString = (decltype(R.GetErrorString))sym("ncclGetErrorString");
    if (!ok) { dlclose(lib); return; }
    R.lib = lib;
    g_rccl = R;
    g_rccl_ok = true;
  });
  return g_rccl_ok;
}
}  // namespace
#define NCCLCHK(ctx, call)                                                                          \
  do {                                                                                              \
    ncclResult_t r_ = (call);                                                                       \
    if (r_ != ncclSuccess) { (ctx)->err = std::string(#call) + ": " + g_rccl.GetErrorString(r_); return ILQR_ERR_HIP; } \
  } while (0)

int ilqr_hip_payload_width(int with_gains) { return ILQR_NU + 1 + (with_gains ? ILQR_NU * ILQR_NX : 0); }
int ilqr_hip_comm_available(void) { return rccl_load() ? 1 : 0; }
int ilqr_hip_comm_get_unique_id(char* id) {
  if (!id) return ILQR_ERR_ARG;
  if (!rccl_load()) return ILQR_ERR_UNSUPPORTED;
  ncclUniqueId u;
  if (g_rccl.GetUniqueId(&u) != ncclSuccess) return ILQR_ERR_HIP;
  std::memcpy(id, u.internal, ILQR_COMM_ID_BYTES);
  return ILQR_OK;
}
int ilqr_hip_comm_init(ilqr_hip_ctx* c, int world, int rank, const char* id) {
  if (!c || world < 1 || rank < 0 || rank >= world || (world > 1 && !id)) return ILQR_ERR_ARG;
  if (c->comm) { c->err = "communicator already initialised"; return ILQR_ERR_STATE; }
  enter(c);
  c->world = world; c->rank = rank;
  if (world == 1) return ILQR_OK;           // one GPU: the gather degenerates to a device copy, RCCL is not needed
  if (!rccl_load()) { c->err = g_rccl.err; return ILQR_ERR_UNSUPPORTED; }
  ncclUniqueId u; std::memcpy(u.internal, id, ILQR_COMM_ID_BYTES);
  NCCLCHK(c, g_rccl.CommInitRank(&c->comm, world, u, rank));
  return ILQR_OK;
}
int ilqr_hip_comm_destroy(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  if (c->comm) { hipSetDevice(c->device); hipStreamSynchronize(c->stream); g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
  c->world = 1; c->rank = 0;
  return ILQR_OK;
}
int ilqr_hip_comm_world(const ilqr_hip_ctx* c) { return c ? c->world : -1; }
int ilqr_hip_comm_rank(const ilqr_hip_ctx* c) { return c ? c->rank : -1; }
int ilqr_hip_gather_first_knot(ilqr_hip_ctx* c, int root, int with_gains, double* recv_device) {
  if (!c || root < 0 || root >= c->world || (c->rank == root && !recv_device)) return ILQR_ERR_ARG;
  if (!c->initialized) return ILQR_ERR_STATE;
  enter(c);
  const size_t W = (size_t)ilqr_hip_payload_width(with_gains), cnt = (size_t)c->B * W;
  if (cnt > c->payload_cap) {
    if (c->d_payload) hipFree(c->d_payload);
    c->d_payload = nullptr; c->payload_cap = 0;
    HIPCHK(c, hipMalloc((void**)&c->d_payload, cnt * sizeof(double)));
    c->payload_cap = cnt;
  }
  // rank r's rollouts are rows [r B, (r + 1) B) of the gathered array: contiguous shards, global rollout order
  double* mine = (c->rank == root) ? recv_device + (size_t)c->rank * cnt : c->d_payload;
  ilqr::launch_pack_payload(c->S, with_gains, mine, c->stream);
  HIPCHK(c, hipGetLastError());
  if (c->world > 1) {
    if (!c->comm) { c->err = "gather before ilqr_hip_comm_init"; return ILQR_ERR_STATE; }
    // a gather as grouped point-to-point transfers: every peer sends to the root over its own xGMI link
    NCCLCHK(c, g_rccl.GroupStart());
    ncclResult_t gr = ncclSuccess;      // an error inside the group still closes it before the call returns
    if (c->rank == root) {
      for (int r = 0; r < c->world && gr == ncclSuccess; ++r) if (r != root) gr = g_rccl.Recv(recv_device + (size_t)r * cnt, cnt, ncclDouble, r, c->comm, c->stream);
    } else {
      gr = g_rccl.Send(c->d_payload, cnt, ncclDouble, root, c->comm, c->stream);
    }
    const ncclResult_t ge = g_rccl.GroupEnd();
    if (gr != ncclSuccess || ge != ncclSuccess) { c->err = std::string("RCCL gather (grouped send/recv): ") + g_rccl.GetErrorString(gr != ncclSuccess ? gr : ge); return ILQR_ERR_HIP; }
  }
  return ILQR_OK;   // asynchronous on the handle's stream: ilqr_hip_synchronize before reading recv_device
}

int ilqr_hip_enable_profiling(ilqr_hip_ctx* c, int on) { if (!c) return ILQR_ERR_ARG; c->profiling = on ? 1 : 0; return ILQR_OK; }
int ilqr_hip_set_profiled_stages(ilqr_hip_ctx* c, unsigned mask) { if (!c) return ILQR_ERR_ARG; c->prof_mask = mask & 0xFFu; return ILQR_OK; }
int ilqr_hip_get_stage_ms(ilqr_hip_ctx* c, double* ms, double* launches) {
  if (!c || !ms) return ILQR_ERR_ARG;
  for (int i = 0; i < 8; ++i) { ms[i] = c->stage_ms[i]; if (launches) launches[i] = c->stage_launches[i]; }
  return ILQR_OK;
}

int ilqr_hip_reference_kinematics(const double* x, double* com, double* ee) {
  if (!x || !com || !ee) return ILQR_ERR_ARG;
  h1host::reference_kinematics(x, com, ee);
  return ILQR_OK;
}
int ilqr_hip_reference_com_velocity(const double* x, double* comvel) {
  if (!x || !comvel) return ILQR_ERR_ARG;
  h1host::reference_com_velocity(x, comvel);
  return ILQR_OK;
}
int ilqr_hip_foot_clearance(const double* qpos, double* clearance) {
  if (!qpos || !clearance) return ILQR_ERR_ARG;
  h1host::foot_clearance(qpos, clearance);
  return ILQR_OK;
}
int ilqr_hip_gravity_compensation(const double* x, const double* gravity, double* u) {
  if (!x || !gravity || !u) return ILQR_ERR_ARG;
  h1host::gravity_compensation(x, gravity, u);
  return ILQR_OK;
}

// ---------------------------------------------------------------- solve groups (group_kernels.hip, libilqr_hip_groups.so)
// The module, opened by the first call that switches groups on.  Missing module or entry point: ILQR_ERR_UNSUPPORTED.
static ilqr::GroupModule g_groups = {};
__attribute__((noinline, minsize)) static int groups_ready(ilqr_hip_ctx* c) {
  static ModuleLib lib;
  const auto resolve = [](void* so, int) { const auto table = (const ilqr::GroupModule* (*)())dlsym(so, "ilqr_groups_module"); if (table) g_groups = *table(); return table != nullptr; };
  if (!open_module(lib, "groups", "solve groups'", resolve, 0)) { c->err = lib.why; return ILQR_ERR_UNSUPPORTED; }
  return ILQR_OK;
}
// what every group call needs first: groups on (and, where asked, a selection)
__attribute__((noinline, minsize)) static int groups_on(ilqr_hip_ctx* c, bool selected) {
  if (c->grp.G < 2) { c->err = "solve groups are off (ilqr_hip_set_groups)"; return ILQR_ERR_STATE; }
  if (selected && !c->grp.selected) { c->err = "no ilqr_hip_group_select since the groups were set"; return ILQR_ERR_STATE; }
  enter(c);
  return ILQR_OK;
}
__attribute__((noinline, minsize)) static int groups_drop_perturbation(ilqr_hip_ctx* c) {
  if (c->grp.sigma) { HIPCHK(c, hipStreamSynchronize(c->stream)); (void)hipFree(c->grp.sigma); }
  c->grp.sigma = nullptr; c->grp.sets = 0; c->grp.hold = 1; c->grp.seed = c->grp.stream0 = 0; c->grp.draws = 0;
  return ILQR_OK;
}
__attribute__((minsize)) int ilqr_hip_set_groups(ilqr_hip_ctx* c, int G) {
  if (!c || G < 1 || c->B % G) return ILQR_ERR_ARG;
  enter(c);
  if (G > 1) TRY(groups_ready(c));
  TRY(groups_drop_perturbation(c));      // (its rows are the old group's members)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (void* p : {(void*)c->grp.winner, (void*)c->grp.rec, (void*)c->grp.mask}) if (p) (void)hipFree(p);
  c->grp.winner = nullptr; c->grp.rec = nullptr; c->grp.mask = nullptr; c->grp.G = 1; c->grp.selected = false;
  if (G == 1) return ILQR_OK;
  TRY(dalloc(c, &c->grp.winner, (size_t)(c->B / G))); TRY(dalloc(c, &c->grp.rec, (size_t)(c->B / G) * 4)); TRY(dalloc(c, &c->grp.mask, (size_t)c->B));
  std::vector<int> mask((size_t)c->B);
  for (int b = 0; b < c->B; ++b) mask[b] = (b % G) != 0;
  HIPCHK(c, hipMemcpyAsync(c->grp.mask, mask.data(), mask.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->grp.G = G;
  return ILQR_OK;
}
int ilqr_hip_num_groups(const ilqr_hip_ctx* c) { return c ? (c->grp.G > 1 ? c->B / c->grp.G : 0) : -1; }
__attribute__((minsize)) int ilqr_hip_group_set_perturbation(ilqr_hip_ctx* c, int n_sets, const double* sigma, int hold, unsigned long long seed, unsigned long long stream0) {
  if (!c || !sigma || hold < 1) return ILQR_ERR_ARG;
  TRY(groups_on(c, false));
  if (n_sets != 1 && n_sets != c->grp.G) return ILQR_ERR_ARG;
  for (int i = 0; i < n_sets * ILQR_NU; ++i) if (!std::isfinite(sigma[i]) || sigma[i] < 0.0 || (n_sets > 1 && i < ILQR_NU && sigma[i] != 0.0)) return ILQR_ERR_ARG;
  if (!c->grp.sigma) HIPCHK(c, hipMalloc((void**)&c->grp.sigma, (size_t)c->grp.G * ILQR_NU * sizeof(double)));
  TRY(upload_rows(c, c->grp.sigma, sigma, (size_t)n_sets, ILQR_NU, ILQR_NU));
  c->grp.sets = n_sets; c->grp.hold = hold; c->grp.seed = seed; c->grp.stream0 = stream0; c->grp.draws = 0;
  return ILQR_OK;
}
int ilqr_hip_group_clear_perturbation(ilqr_hip_ctx* c) { if (!c) return ILQR_ERR_ARG; enter(c); return groups_drop_perturbation(c); }
long ilqr_hip_group_draws(const ilqr_hip_ctx* c) { return c ? c->grp.draws : -1L; }
__attribute__((minsize)) int ilqr_hip_group_perturb(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  if (!c->initialized) { c->err = "group_perturb before initialize"; return ILQR_ERR_STATE; }
  TRY(groups_on(c, false));
  if (!c->grp.sigma) { c->err = "group_perturb without a perturbation (ilqr_hip_group_set_perturbation)"; return ILQR_ERR_STATE; }
  TRY(enter_launching(c));
  const ilqr::GroupPerturbDev Pd{c->grp.sigma, c->grp.sets, c->grp.hold, c->grp.seed, c->grp.stream0, (unsigned long long)c->grp.draws};
  g_groups.perturb(c->S.ubar, &Pd, c->B, c->N, c->grp.G, c->stream);
  // The members g >= 1 are rolled out from their new controls here (the incumbents keep every bit: the mask): iteration 0 of the next solve
  // rolls every rollout out in front of the linearisation anyway (xbar_rolled = false: solve_order.h nominal_roll, ROLL_BEFORE in every launch
  // order), but the cost a solve starts from -- what it reports for a rollout that accepts no step -- is taken from the trajectory as the
  // solve finds it (k_solve_begin, ilqr.cpp:540), and that must be the trajectory of the perturbed controls: group_select reads it.
  DevState Sg = c->S; Sg.active = c->grp.mask;
  ilqr::launch_rollout(plan_of(c), Sg, c->P, ilqr::MASK_ACTIVE, 1, 0, Sg.Jbase, c->stream);
  HIPCHK(c, hipGetLastError());
  ++c->grp.draws;
  c->xbar_rolled = false;
  return ILQR_OK;
}
__attribute__((minsize)) int ilqr_hip_group_select(ilqr_hip_ctx* c, const double* key_device) {
  if (!c) return ILQR_ERR_ARG;
  TRY(groups_on(c, false));
  if (!key_device && !c->solved) { c->err = "group_select on the solve's cost before a solve"; return ILQR_ERR_STATE; }
  g_groups.select(key_device ? key_device : c->S.J, c->B, c->grp.G, c->grp.winner, c->grp.rec, c->stream);
  HIPCHK(c, hipGetLastError());
  c->grp.selected = true;
  return ILQR_OK;
}
__attribute__((minsize)) int ilqr_hip_group_get_winners(ilqr_hip_ctx* c, int* winner, double* rec) {
  if (!c) return ILQR_ERR_ARG;
  TRY(groups_on(c, true));
  const size_t M = (size_t)(c->B / c->grp.G);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (winner) HIPCHK(c, hipMemcpy(winner, c->grp.winner, M * sizeof(int), hipMemcpyDeviceToHost));
  if (rec) HIPCHK(c, hipMemcpy(rec, c->grp.rec, M * 4 * sizeof(double), hipMemcpyDeviceToHost));
  return ILQR_OK;
}
int ilqr_hip_group_winners_device(ilqr_hip_ctx* c, const int** winner_device, const double** rec_device) {
  if (!c) return ILQR_ERR_ARG;
  TRY(groups_on(c, false));
  if (winner_device) *winner_device = c->grp.winner;
  if (rec_device) *rec_device = c->grp.rec;
  return ILQR_OK;
}
int ilqr_hip_group_copy_winners_device(ilqr_hip_ctx* c, int* winner_out_device) {
  if (!c || !winner_out_device) return ILQR_ERR_ARG;
  TRY(groups_on(c, true));
  HIPCHK(c, hipMemcpyAsync(winner_out_device, c->grp.winner, (size_t)(c->B / c->grp.G) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  return ILQR_OK;
}
// The slabs of a rollout's solution state: what a later call reads about a solved rollout.  Not here: linearisation, quadratics, value function,
// candidates, lin_dump (iteration 0 of the next solve recomputes them for every rollout) and the diagnostic history (traces, lists, counters).
__attribute__((minsize)) int ilqr_hip_group_adopt(ilqr_hip_ctx* c) {
  if (!c) return ILQR_ERR_ARG;
  TRY(groups_on(c, true));
  const size_t N = c->N, D = sizeof(double);
  const DevState& S = c->S;
  ilqr::GroupSlabs T{};
  bool ok = true;
  const auto add = [&](void* p, size_t bytes) { ok = ilqr::group_slabs_add(T, p, bytes) && ok; };
  add(S.x0, ILQR_NX * D); add(S.xbar, (N + 1) * ILQR_NX * D); add(S.ubar, N * ILQR_NU * D); add(S.K, N * ILQR_NU * ILQR_NX * D); add(S.kff, N * ILQR_NU * D);
  add(S.J, D); add(S.lambda, D); add(S.iters, sizeof(int));
  if (c->P.al) {
    add(c->al.jc.store, al_store_doubles(c, c->al.jc) * D); add(c->al.viol, 2 * D); add(c->al.done, sizeof(int));
    if (c->P.als) { add(c->al.st.store, al_store_doubles(c, c->al.st) * D); add(c->al.sviol, D); }
    if (c->P.alt) { add(c->al.tk.store, al_store_doubles(c, c->al.tk) * D); add(c->al.tviol, D); }
  }
  if (!ok) { c->err = "group_adopt: the slab table is full"; return ILQR_ERR_HIP; }
  g_groups.adopt(&T, c->grp.winner, c->B, c->grp.G, c->stream);
  HIPCHK(c, hipGetLastError());
  c->xbar_rolled = false;      // (as after a solve: every other host-side fact describes buffers this call does not write)
  return ILQR_OK;
}

}  // extern "C"
