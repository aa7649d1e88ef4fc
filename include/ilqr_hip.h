/*
 * ilqr_hip.h -- C ABI of the MI355X-native batched iLQR solver (libilqr_hip.so).
 *
 * Drop-in boundary for the reference's MPC_iLQR_solve path.  The reference has no FFI; its boundary
 * is the C++ class API of `iLQR` / `MPC` / `RobotUtils`.  Every entry point below cites the
 * reference interface it replaces (paths relative to the reference repository root).
 * A batch of B independent rollouts (same robot, same horizon) is solved per handle; B = 1
 * reproduces the reference call-for-call (see include/ilqr_hip.hpp for the C++ mirror classes).
 *
 * Conventions: row-major doubles in caller-owned HOST buffers unless a name ends in `_device`;
 * state x = [qpos(26): p, quat wxyz, hinge(19) | qvel(25): v_lin world, omega body, hinge rates];
 * nx = 51, nu = 19; N = horizon.  "set" arrays may be shared by all rollouts (n_sets == 1) or
 * given per rollout (n_sets == batch).  All functions return ILQR_OK (0) or an error code;
 * no exceptions cross the ABI; calls on one handle must be serialised by the caller; one handle
 * per GPU.  There is NO CPU fallback: creating a handle without a HIP device fails.
 */
#ifndef ILQR_HIP_H
#define ILQR_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define ILQR_NX 51
#define ILQR_NU 19
#define ILQR_NQ 26
#define ILQR_NV 25

enum ilqr_status {
  ILQR_OK = 0,
  ILQR_ERR_ARG = 1,         /* null pointer / bad size (reference: size check, src/ilqr/ilqr.cpp:526-532) */
  ILQR_ERR_HIP = 2,         /* HIP runtime error, see ilqr_hip_last_error */
  ILQR_ERR_NO_DEVICE = 3,   /* no usable gfx950 device */
  ILQR_ERR_STATE = 4,       /* call order violated (e.g. solve before initialize) */
  ILQR_ERR_UNSUPPORTED = 5
};

enum ilqr_jacobian_mode {
  ILQR_JAC_ANALYTIC = 0,    /* exact derivatives of the dynamics step (north-star mode) */
  ILQR_JAC_FD_FORWARD = 1   /* reference-style forward differences, RobotUtils::linearizeDynamicsFD,
                               src/common/robot_utils.cpp:120-160 (eps default 1e-5, robot_utils.hpp:51-53) */
};

typedef struct ilqr_hip_ctx ilqr_hip_ctx;

/* iLQR::iLQR(RobotUtils&, int N, double dt, urdf) -- include/ilqr/ilqr.hpp:19, src/ilqr/ilqr.cpp:14-48.
   The H1 model constants (h1.xml / h1.urdf) are compiled in.  device = HIP device ordinal. */
int ilqr_hip_create(ilqr_hip_ctx** out, int device, int batch, int horizon, double dt);
int ilqr_hip_destroy(ilqr_hip_ctx* ctx);
/* The diagnostic environment switches (kernel families ILQR_BACKWARD / ILQR_LS / ILQR_ROLLOUT / ILQR_DYN / ILQR_LINT, launch orders
   ILQR_SLICES / ILQR_STAGGER / ILQR_OVERLAP_ROLLOUT / ILQR_REUSE_ROLLOUT / ILQR_EE_GATE / ILQR_SPLIT / ILQR_SPEC* / ILQR_RELIN) are read ONCE, by
   ilqr_hip_create, and kept in the handle: no getenv on the call path, and the handle's copy is the only one -- handles of different
   kernel families may be driven from one host thread in any order.  This call re-reads them for one handle (tests, profiling tools);
   ILQR_ENV_PER_CALL=1 at creation makes every call of the handle do so, and while such a re-read names a kernel family the library
   does not hold, every call that launches a family-dependent kernel (initialize*, solve*, stage_rollout / linearize / backward_pass /
   total_cost / line_search, step*, get_stance with the stance source GEOMETRY) returns ILQR_ERR_UNSUPPORTED; getters, setters and
   the fixed conversion kernels never do.  No reference counterpart. */
int ilqr_hip_reload_environment(ilqr_hip_ctx* ctx);
/* On by default (the solve executes every pass the reference executes on new inputs).  A lambda retry (ilqr.cpp:619-644) whose lambda is
   already saturated -- min(10 lambda, 1e-3) == lambda, the state a rollout reaches after three failed searches -- is not executed:
   it would repeat the backward pass and the line search that have just failed on identical inputs, bit for bit, and fail again.  Its
   bookkeeping (trace entry, iteration count, convergence-exit rule of ilqr.cpp:640-655) is played at once.  Every observable of the solve
   is unchanged (GPU tests).  lambda outlives a solve, so a rollout may enter a later solve at the cap: the pass its skipped retry repeats
   is then the first pass of the same iteration, and iteration 0 of every solve runs that pass for every rollout, on whatever trajectory
   the warm start or ilqr_hip_initialize* left.  on = 0, or environment ILQR_DEDUP_RETRY=0, restores the full retry (comparison,
   profiling; ILQR_DEDUP_RETRY=1 / 0 overrides this call, unset or -1 leaves it in charge).  In the side-by-side order
   (ilqr_hip_get_speculative_iterations) both passes are in flight before either outcome is known: nothing is skipped there, whatever
   the setting.  bench.py's dedup_saturated_retry object therefore repeats its headline.  No reference counterpart: the reference
   recomputes. */
int ilqr_hip_set_dedup_saturated_retry(ilqr_hip_ctx* ctx, int on);
/* Sum over the iterations of the last solve of the number of rollouts whose lambda retry (backward pass and line search) ran: the length
   of the iteration's retry list in the sequential order -- the rollouts whose first search failed, less the saturated repeats above --,
   the rollouts active in the iteration where both passes ran side by side, batch x iterations with batch slices (no lists).  In the
   sequential order, without the early-continuation groups, the retry's line search takes the one-rollout-per-wave kernel once its list
   holds at most 1024 rollouts (decided on the device; environment ILQR_LS_LIST_MAX, as for the first pass).  Synchronises the handle's stream.  0 before the first solve and
   after ilqr_hip_set_max_iterations changed the count, -1 for a null handle or a failed read. */
long long ilqr_hip_get_retry_pass_rollouts(ilqr_hip_ctx* ctx);
const char* ilqr_hip_last_error(const ilqr_hip_ctx* ctx);
int ilqr_hip_batch(const ilqr_hip_ctx* ctx);
int ilqr_hip_horizon(const ilqr_hip_ctx* ctx);
/* Number of contiguous batch slices a solve is enqueued as (each on its own streams, so that the line search of one
   slice overlaps with the Riccati / Jacobian kernels of the others; environment ILQR_SLICES, 1 = one launch sequence
   for the whole batch).  No reference counterpart: the reference solves one trajectory at a time. */
int ilqr_hip_num_slices(const ilqr_hip_ctx* ctx);

/* RobotUtils::setCostWeights -- include/common/robot_utils.hpp:60, src/common/robot_utils.cpp:253-279.
   Q/R/Qf are diagonal by construction (Config::buildCostMatrices, src/common/config.cpp:66-122). */
int ilqr_hip_set_cost_weights(ilqr_hip_ctx* ctx, const double* Q_diag /*51*/, const double* R_diag /*19*/, const double* Qf_diag /*51*/);
/* RobotUtils::set{CoM,CoMVel,EEPos,EEVel,Upright,Balance}Weight -- include/common/robot_utils.hpp:120-129 */
int ilqr_hip_set_task_weights(ilqr_hip_ctx* ctx, double w_com, double w_com_vel, double w_ee_pos, double w_ee_vel, double w_upright, double w_balance);
/* RobotUtils::setConstraintWeights -- src/common/robot_utils.cpp:674-680 */
int ilqr_hip_set_constraint_weights(ilqr_hip_ctx* ctx, double w_joint_limits, double w_control_limits);
/* Per-rollout weight sets (batched weight sweeps): one set of everything the three setters above carry -- Q, R, Qf, the six task weights in
   the order of ilqr_hip_set_task_weights, and constraint = (w_joint_limits, w_control_limits) -- per rollout.  n_sets is 1 or the batch
   (else ILQR_ERR_ARG), every pointer is required.  The sets go into a device table owned by the handle, one 144-double record (nine
   128-byte lines) per set; while it is installed it takes precedence over the three shared setters, which keep storing their values and
   launch nothing new, and the cost kernels run in their weight-set instantiations.  n_sets == 1 installs a one-record table that every
   rollout reads.  Synchronises the handle's stream.  ILQR_ERR_UNSUPPORTED on a handle of the test library whose environment selects a
   family that evaluates the cost inside its own rollout / line-search kernels (ILQR_DYN=s, ILQR_ROLLOUT=r, ILQR_LS=r); while a table is
   installed and an ILQR_ENV_PER_CALL re-read selects such a family, the calls ilqr_hip_reload_environment lists as launching
   family-dependent kernels return it too (ilqr_hip_stage_cost_quadratics is not one of them: its kernels are the same in every family,
   and it keeps running under the table).  No reference counterpart:
   RobotUtils::setCostWeights (robot_utils.cpp:253-279) holds one set. */
int ilqr_hip_set_weight_sets(ilqr_hip_ctx* ctx, const double* Q /*[n_sets][51]*/, const double* R /*[n_sets][19]*/, const double* Qf /*[n_sets][51]*/,
                             const double* task /*[n_sets][6]*/, const double* constraint /*[n_sets][2]*/, int n_sets);
/* Back to the stored shared values (same kernels and kernel arguments as a handle that never had a table). */
int ilqr_hip_clear_weight_sets(ilqr_hip_ctx* ctx);
/* 0: no table installed (shared weights), else the n_sets of the installed table (1 or the batch); -1 for a null handle */
int ilqr_hip_num_weight_sets(const ilqr_hip_ctx* ctx);
/* Augmented-Lagrangian joint and torque limits: an outer loop of up to `rounds` rounds around the solve that ENFORCES the two range tables
   the plain penalties (ilqr_hip_set_constraint_weights) only discourage.  No reference counterpart: RobotUtils::setConstraintWeights
   (robot_utils.cpp:674-680) is all the reference has.
   Constraints, per rollout, all of the form c <= 0: hinge j (state slot 7 + j) at the knots t = 0..N, q - hi_j and lo_j - q; actuator i at
   t = 0..N-1, u - hi_i and lo_i - u; lo = range[0] + margin (range[1] - range[0]), hi = range[1] - margin (...) from the model's joint /
   control ranges.  margin = 0.1 gives the penalties' bounds, margin = 0 the hard range.  With multiplier mu >= 0 and penalty rho > 0 the
   knot cost gets phi = (max(0, mu + rho c)^2 - mu^2) / (2 rho) per constraint IN PLACE of the plain penalties (w_joint_limits /
   w_control_limits are not read while this is installed); one rho per rollout and family, rho_joint and rho_ctrl.  After each inner solve,
   on the accepted nominal trajectory: mu <- max(0, mu + rho c); viol_joint = the largest max(0, c) over hinges, sides and knots t >= 1
   (x_0 is given: knot 0 carries the cost term, its multipliers stay zero and it is left out), viol_ctrl likewise over t = 0..N-1; the
   rollout is done when viol_joint <= tol_joint and viol_ctrl <= tol_ctrl, otherwise rho <- min(rho growth, rho_max_factor rho_0) for both
   families.  A done rollout's multipliers and penalties are frozen for the rest of the call.  Every rule is per rollout.
   With this installed ilqr_hip_solve / ilqr_hip_solve_async run up to `rounds` rounds; each is the solve described there (max_iter, tol,
   lambda persisting from round to round as from solve to solve), a later round starting from its predecessor's nominal trajectory.  With
   the convergence exit (ilqr_hip_set_options early_exit = 1) a done rollout enters the later rounds inactive and, with the early-exit gate
   on, the host stops enqueuing rounds once every rollout is done (one read between two rounds; gate off: all rounds are enqueued, the
   results are the same).  With early_exit = 0 every round runs max_iter iterations on every rollout.  ilqr_hip_get_trace,
   ilqr_hip_get_iterations and ilqr_hip_get_cost then describe, per rollout, the last round that ran for it -- the cost is the augmented
   cost under the multipliers that round ran with --; ilqr_hip_get_linearized_rollouts, _first_pass_rollouts and _retry_pass_rollouts the
   last round enqueued.  The cold initialisers zero the multipliers and reset rho; the warm ones (ilqr_hip_initialize with a previous
   solution, ilqr_hip_initialize_warm_resident[_shifted], ilqr_hip_initialize_warm_from_plant[_shifted]) shift the multipliers by the
   knots the trajectory is shifted by, zero the tail and reset rho.  The stage calls (ilqr_hip_stage_cost_quadratics, _total_cost,
   _line_search, _rollout) use the installed multipliers and penalties.
   rounds >= 1, rho_joint0 > 0, rho_ctrl0 > 0, growth >= 1, rho_max_factor >= 1, 0 <= margin < 0.5, tolerances >= 0, else ILQR_ERR_ARG.
   Allocates the multiplier store on first use ([B] records of 16 + 80 (N + 1) doubles: h1_cost_dev.h), zeroes it, sets rho = rho_0.
   ILQR_ERR_UNSUPPORTED: in the families of the test library that evaluate the cost inside their own rollout / line-search kernels (the rule
   and the ILQR_ENV_PER_CALL behaviour of ilqr_hip_set_weight_sets), and together with an installed weight-set table -- this call while a
   table is installed, ilqr_hip_set_weight_sets while this is.  Synchronises the handle's stream. */
int ilqr_hip_set_augmented_lagrangian(ilqr_hip_ctx* ctx, int rounds, double rho_joint0, double rho_ctrl0, double growth, double rho_max_factor, double margin,
                                      double tol_joint, double tol_ctrl);
/* Back to the plain penalties (same kernels and kernel arguments as a handle that never had it). */
int ilqr_hip_clear_augmented_lagrangian(ilqr_hip_ctx* ctx);
/* 0: not installed, else the `rounds` it was installed with; -1 for a null handle */
int ilqr_hip_augmented_lagrangian_rounds(const ilqr_hip_ctx* ctx);
/* The multipliers, (lower, upper) per coordinate; either pointer may be NULL.  ILQR_ERR_STATE while nothing is installed (all six calls below). */
int ilqr_hip_get_al_multipliers(ilqr_hip_ctx* ctx, double* joint /*[B][N+1][19][2]*/, double* ctrl /*[B][N][19][2]*/);
/* Any pointer may be NULL (that part stays).  Multipliers >= 0, penalties > 0, else ILQR_ERR_ARG; the hinges' knot-0 entries are stored as zero. */
int ilqr_hip_set_al_multipliers(ilqr_hip_ctx* ctx, const double* joint /*[B][N+1][19][2]*/, const double* ctrl /*[B][N][19][2]*/, const double* rho /*[B][2] joint, ctrl*/);
int ilqr_hip_get_al_penalties(ilqr_hip_ctx* ctx, double* rho /*[B][2] joint, ctrl*/);
/* violations of the nominal trajectory at the last update and the done flags; either pointer may be NULL */
int ilqr_hip_get_al_violation(ilqr_hip_ctx* ctx, double* viol /*[B][2] joint, ctrl*/, int* done /*[B]*/);
/* Per round of the last solve and rollout: joint violation, control violation, rho_joint and rho_ctrl the round ran with, inner iterations
   executed.  NaN where the round did not run for the rollout (done before it, convergence exit) or was not run at all. */
int ilqr_hip_get_al_trace(ilqr_hip_ctx* ctx, double* out /*[rounds][B][5]*/);
/* Stage call: the update that follows an inner solve, alone, on the resident nominal trajectory (ilqr_hip_set_trajectory) and the installed
   multipliers; writes row `round` (0 <= round < rounds) of the trace.  Synchronises. */
int ilqr_hip_al_update(ilqr_hip_ctx* ctx, int round);
/* One table of bounds per rollout for the augmented-Lagrangian limits.  A record is ILQR_AL_BOUNDS = 76 doubles: joint_lo[19], joint_hi[19]
   (hinges in the order of the state slots 7..25), ctrl_lo[19], ctrl_hi[19] (actuators in the order of u).  n_sets is 1 (one record that every
   rollout reads) or the batch (rollout b reads record b).  While a table is installed every constraint of ilqr_hip_set_augmented_lagrangian
   takes its lo / hi from rollout b's record: the model's ranges and the margin fraction are not read, and the margin of the installation is
   NOT applied to the table -- the table holds the final bounds.  Everything else of the description above stays as it is: the term phi,
   the update, the violations with the hinges' knot 0 left out, the done rule, rho growth, the rounds, the warm-start shift, the getters.
   A lower bound may be -inf and an upper bound +inf: that side is switched off -- its c is -inf, its term the constant -mu^2 / (2 rho), its
   gradient and curvature 0, its multiplier driven to 0 by the update, its violation 0.
   The table acts on the COST only: the solver's dynamics step keeps clamping u to the model's control range, so a torque bound wider than
   the model's is not a wider actuator; the plant, the score and the plain penalties are untouched.
   ILQR_ERR_STATE while no augmented Lagrangian is installed (all four handle calls).  ILQR_ERR_ARG: a null pointer, n_sets not 1 or the
   batch, a NaN, lo > hi, lo == +inf, hi == -inf; everything is checked before the handle is touched, a refused call leaves a previously
   installed table as it was.  lo == hi is allowed (a dead motor: ctrl_lo = ctrl_hi = 0).  Uploads and synchronises the handle's stream.
   The table survives the cold and warm initialisers, ilqr_hip_set_al_multipliers and a repeated ilqr_hip_set_augmented_lagrangian on a
   handle that has it installed (whose margin is then unused); ilqr_hip_clear_augmented_lagrangian drops it.  The refusals of
   ilqr_hip_set_augmented_lagrangian (cross-check families, weight sets) stay as they are. */
#define ILQR_AL_BOUNDS 76
int ilqr_hip_set_al_bounds(ilqr_hip_ctx* ctx, const double* bounds /*[n_sets][76]*/, int n_sets);
/* Back to the model's ranges at the installed margin (same kernels and kernel arguments as a handle that never had a table). */
int ilqr_hip_clear_al_bounds(ilqr_hip_ctx* ctx);
/* 0: no table installed, else the n_sets of the installed table (1 or the batch); -1 for a null handle */
int ilqr_hip_num_al_bound_sets(const ilqr_hip_ctx* ctx);
/* The record each rollout is solved with: a one-record table expanded; without a table the model's bounds at the installed margin. */
int ilqr_hip_get_al_bounds(ilqr_hip_ctx* ctx, double* bounds /*[B][76]*/);
/* The bounds ilqr_hip_set_augmented_lagrangian(margin) enforces without a table, as one record: lo = range[0] + margin (range[1] - range[0]),
   hi = range[1] - margin (...), the doubles the kernels form.  margin = 0: the model's joint and control ranges.  Host only: no GPU, no
   handle.  0 <= margin < 0.5 and a non-null pointer, else ILQR_ERR_ARG. */
int ilqr_hip_al_default_bounds(double margin, double* bounds /*[76]*/);
/* Augmented-Lagrangian bounds on the other 28 non-quaternion state coordinates, the "box coordinates" k = 0..27: pelvis position in the
   world (k = 0..2, state slots 0..2), pelvis linear velocity in the world (k = 3..5) and angular velocity in the body (k = 6..8), the 19
   joint velocities in the order of u (k = 9..27); k >= 3 is state slot 23 + k (ilqr_hip_al_state_slot).  A record is ILQR_AL_STATE_BOUNDS =
   56 doubles, lo[28] then hi[28]; n_sets is 1 (every rollout reads the one record) or the batch (rollout b reads record b).  The model has no
   ranges for these coordinates: there is no default table, and without a table nothing here is constrained.
   A third family beside the hinges and the actuators of ilqr_hip_set_augmented_lagrangian, rule for rule: the constraints x_slot - hi and
   lo - x_slot at the knots t = 0..N with the term phi per constraint; knot 0 carries the cost term, keeps zero multipliers and is left out of
   the violation (x_0 is given); one penalty rho_state per rollout, starting at rho_state0 and capped at rho_max_factor rho_state0 (the factor
   of the installation); after each inner solve mu <- max(0, mu + rho_state c) and viol_state = the largest max(0, c) over coordinates, sides
   and knots 1..N.  With a table installed a rollout is done only when viol_joint <= tol_joint, viol_ctrl <= tol_ctrl AND viol_state <=
   tol_state; otherwise all three penalties grow.  A done rollout is frozen; the convergence exit, the early-exit gate and the rounds work off
   that one done flag as described above.  ilqr_hip_al_update updates this family too.  The getters above keep their shapes and meaning.
   A lower bound may be -inf and an upper bound +inf: that side is switched off as in ilqr_hip_set_al_bounds (c = -inf, term -mu^2 / (2 rho),
   zero gradient and curvature, multiplier driven to 0, violation 0).  The table acts on the COST only: dynamics, plant and score are untouched.
   It works with or without a joint / torque bounds table.
   ILQR_ERR_STATE while no augmented Lagrangian is installed (every handle call below).  ILQR_ERR_ARG: a null pointer, n_sets not 1 or the
   batch, a NaN, lo > hi, lo == +inf, hi == -inf, rho_state0 <= 0 or not finite, tol_state < 0; everything is checked before the handle is
   touched, a refused call leaves a previously installed table as it was.  Allocates the second multiplier store on first use ([B] records of
   16 + 64 (N + 1) doubles: h1_cost_dev.h).  Installing where no table was installed zeroes the state multipliers; replacing a table keeps
   them; rho_state = rho_state0 either way.  Uploads and synchronises the handle's stream.
   The table survives the cold and warm initialisers, ilqr_hip_set_al_multipliers and a repeated ilqr_hip_set_augmented_lagrangian;
   ilqr_hip_clear_augmented_lagrangian drops it.  The cold initialisers zero the state multipliers and reset rho_state; the warm ones shift
   the state multipliers by the knots the trajectory is shifted by (zero tail, knot 0 zero) and reset rho_state.  The refusals of
   ilqr_hip_set_augmented_lagrangian (cross-check families, weight sets) stay as they are. */
#define ILQR_AL_STATE_COORDS 28
#define ILQR_AL_STATE_BOUNDS 56
int ilqr_hip_set_al_state_bounds(ilqr_hip_ctx* ctx, const double* bounds /*[n_sets][56]*/, int n_sets, double rho_state0, double tol_state);
/* No state family any more (same kernels and kernel arguments as a handle that never had a table). */
int ilqr_hip_clear_al_state_bounds(ilqr_hip_ctx* ctx);
/* 0: no table installed, else the n_sets of the installed table (1 or the batch); -1 for a null handle */
int ilqr_hip_num_al_state_bound_sets(const ilqr_hip_ctx* ctx);
/* The record each rollout is solved with: a one-record table expanded; without a table lo = -inf, hi = +inf in every row. */
int ilqr_hip_get_al_state_bounds(ilqr_hip_ctx* ctx, double* bounds /*[B][56]*/);
/* The state multipliers, (lower, upper) per box coordinate; zeros without a table. */
int ilqr_hip_get_al_state_multipliers(ilqr_hip_ctx* ctx, double* mu /*[B][N+1][28][2]*/);
/* Either pointer may be NULL (that part stays).  Multipliers >= 0, penalties > 0, else ILQR_ERR_ARG; knot-0 entries are stored as zero.
   ILQR_ERR_STATE without a table. */
int ilqr_hip_set_al_state_multipliers(ilqr_hip_ctx* ctx, const double* mu /*[B][N+1][28][2]*/, const double* rho /*[B]*/);
/* rho_state as the store holds it; zeros without a table */
int ilqr_hip_get_al_state_penalties(ilqr_hip_ctx* ctx, double* rho /*[B]*/);
/* viol_state of the nominal trajectory at the last update; zeros without a table (the done flags: ilqr_hip_get_al_violation) */
int ilqr_hip_get_al_state_violation(ilqr_hip_ctx* ctx, double* viol /*[B]*/);
/* Per round of the last solve and rollout: viol_state and the rho_state the round ran with.  NaN where ilqr_hip_get_al_trace has NaN, and
   everywhere without a table. */
int ilqr_hip_get_al_state_trace(ilqr_hip_ctx* ctx, double* out /*[rounds][B][2]*/);
/* The state slot of box coordinate k; -1 outside 0..27.  Host only: no GPU, no handle. */
int ilqr_hip_al_state_slot(int k);
/* Bounds that change from knot to knot: a WINDOW of bounds per set in place of one record per set.  ilqr_hip_set_al_knot_bounds takes
   [n_sets][N+1][76], row t in the field order of ilqr_hip_set_al_bounds; ilqr_hip_set_al_state_knot_bounds takes [n_sets][N+1][56], row t in
   the field order of ilqr_hip_set_al_state_bounds, with that call's rho_state0 and tol_state.  n_sets is 1 (every rollout reads the one
   window) or the batch (rollout b reads window b).  At knot t of rollout b every constraint of the family takes its lo / hi from row t of
   rollout b's window: the hinges and the box coordinates at the knots 0..N, the actuators at the knots 0..N-1 (the torque fields of row N are
   validated like every other row and never read).  Everything else stays word for word what ilqr_hip_set_augmented_lagrangian,
   ilqr_hip_set_al_bounds and ilqr_hip_set_al_state_bounds describe: the term phi, the update mu <- max(0, mu + rho c), knot 0 carrying the
   cost term but zero multipliers and left out of the violation, viol_*, the done rule, rho growth, the rounds, the -inf / +inf "side off"
   rule, and "acts on the COST only" (dynamics, plant, score and the plain penalties are untouched).
   The later call wins within a family: a window replaces a whole-horizon table of that family (multipliers are kept, as when a table
   replaces a table; the state family's rho_state = rho_state0 either way, and its multipliers are zeroed only where no state family was
   installed); ilqr_hip_set_al_bounds / ilqr_hip_set_al_state_bounds replace a window; ilqr_hip_clear_al_bounds /
   ilqr_hip_clear_al_state_bounds drop whichever is installed.  The two families are independent: either may have a window, a table or
   (joint / torque) the model's bounds.  While one family has a window the library itself repeats the other family's record over the knots on
   the device, so that one kernel instantiation serves the mixed cases; the results are those of the record.
   The window is horizon-local: a warm start shifts the multipliers as it does today and does not move the window -- the caller, or the
   bounds track below, writes the next one.  It survives the cold and warm initialisers, ilqr_hip_set_al_multipliers and a repeated
   ilqr_hip_set_augmented_lagrangian; ilqr_hip_clear_augmented_lagrangian drops it.
   ILQR_ERR_STATE while no augmented Lagrangian is installed.  ILQR_ERR_ARG: a null pointer, n_sets not 1 or the batch, a NaN, lo > hi,
   lo == +inf or hi == -inf in any row, rho_state0 <= 0 or not finite, tol_state < 0; everything is checked before the handle is touched, a
   refused call leaves what was installed as it was.  ILQR_ERR_UNSUPPORTED when the kernels that read windows cannot be loaded: they live in
   libilqr_hip_alknot.so beside the library, opened by the first of these calls.  Allocates the two window buffers on first use ([B][N+1]
   records of 80 and of 64 doubles).  Uploads and synchronises the handle's stream.  The refusals of ilqr_hip_set_augmented_lagrangian
   (cross-check families, weight sets) stay as they are. */
int ilqr_hip_set_al_knot_bounds(ilqr_hip_ctx* ctx, const double* bounds /*[n_sets][N+1][76]*/, int n_sets);
int ilqr_hip_set_al_state_knot_bounds(ilqr_hip_ctx* ctx, const double* bounds /*[n_sets][N+1][56]*/, int n_sets, double rho_state0, double tol_state);
/* What each rollout is solved with at each knot, whoever wrote it: a window (of a setter or of ilqr_hip_al_bounds_window_from_track), a
   whole-horizon record repeated over the knots, or without any table the model's bounds at the installed margin (joint_ctrl) and -inf / +inf
   (state).  Either pointer may be NULL.  Synchronises the handle's stream.  ILQR_ERR_STATE while no augmented Lagrangian is installed.
   On a handle with a window of a family, ilqr_hip_get_al_bounds / ilqr_hip_get_al_state_bounds of that family return ILQR_ERR_STATE (one
   record per rollout cannot describe it; the error text names this call); in every other state they behave as before.
   ilqr_hip_num_al_bound_sets / ilqr_hip_num_al_state_bound_sets report the installed n_sets, table or window. */
int ilqr_hip_get_al_knot_bounds(ilqr_hip_ctx* ctx, double* joint_ctrl /*[B][N+1][76] or NULL*/, double* state /*[B][N+1][56] or NULL*/);
/* Bit 0: the joint / torque family has a window; bit 1: the state family has one.  0 without an augmented Lagrangian; -1 for a null handle. */
int ilqr_hip_al_bounds_per_knot(const ilqr_hip_ctx* ctx);
/* A bounds track, cut on the device as the reference windows are (ilqr_hip_set_reference_track): `rows` >= 1 rows on the loop's timeline,
   joint_ctrl [rows][76] and / or state [rows][56] in the field orders above (at least one part; a NULL part is not cut and that family
   stays as installed).  One upload; the handle owns the copy and a new track replaces it.  Installing a track of either kind (this one or
   ilqr_hip_set_al_task_bounds_track) sets the start rows, which both kinds share, back to one shared start of 0.
   A state part needs an installed state family (table or window), else ILQR_ERR_STATE: the track supplies the bounds, the installation
   rho_state0 and tol_state.  Validation as for the setters, row by row (ILQR_ERR_ARG; ILQR_ERR_STATE without an augmented Lagrangian;
   ILQR_ERR_UNSUPPORTED without the module).  Synchronises the handle's stream. */
int ilqr_hip_set_al_bounds_track(ilqr_hip_ctx* ctx, int rows, const double* joint_ctrl /*[rows][76] or NULL*/, const double* state /*[rows][56] or NULL*/);
/* Frees the track; the windows last written stay installed.  Synchronises the handle's stream. */
int ilqr_hip_clear_al_bounds_track(ilqr_hip_ctx* ctx);
/* Rows of the installed bounds track; 0 without one, -1 for a null handle */
int ilqr_hip_al_bounds_track_rows(const ilqr_hip_ctx* ctx);
/* One start row per set, kept on the device: n_sets is 1 (one start for every rollout) or the batch; every start >= 0 (ILQR_ERR_ARG).
   Default: one shared start of 0.  One start buffer on the handle serves the bounds track and the task bounds track: the call is accepted
   while either is installed, ILQR_ERR_STATE without both. */
int ilqr_hip_set_al_bounds_track_starts(ilqr_hip_ctx* ctx, const int* start /*[n_sets]*/, int n_sets);
/* Enqueues one kernel on the handle's stream (al_bounds_track_kernels.hip), no upload, no synchronisation: for set b and t = 0..N it writes
   row min(start[b] + step + t, rows - 1) of each part of the track into row t of set b's window of that part -- the end clamp of x_ref.  A
   pure copy: the windows are bit for bit what the knot setters would upload, and afterwards the handle is in the state those setters
   leave, with n_sets equal to the number of starts (multipliers and penalties untouched).  Where that state differs from the one before --
   the first cut, or after other starts -- and the other family has no window, the same call also enqueues the copy that repeats that
   family's record over the knots.  The same ONE kernel cuts the task bounds track (ilqr_hip_set_al_task_bounds_track) when that is
   installed: window row t of set b is row min(start[b] + step + t, rows_task - 1) of it.  step >= 0, else ILQR_ERR_ARG.  ILQR_ERR_STATE
   without an augmented Lagrangian, without a track of either kind, with a state part while no state family is installed, or with a task
   track while no task family is. */
int ilqr_hip_al_bounds_window_from_track(ilqr_hip_ctx* ctx, int step);
/* Augmented-Lagrangian bounds on POINTS of the robot, the task family: nine task coordinates k = 0..8 in the world frame -- the whole-body
   centre of mass x, y, z (k = 0..2), the left ankle origin (k = 3..5) and the right ankle origin (k = 6..8): the points the cost tracks
   softly (w_com, w_ee_pos).  "Keep the swing foot 3 cm above the floor", "land the foot inside this stone", "keep the centre of mass over
   the support box".  The ankle origins are those of ilqr_hip_reference_kinematics.  The CoM is the one the w_com term tracks -- the URDF
   link masses, because the term's gradient and Hessian are that point's -- which lies about 3 mm from the CoM of the MuJoCo model that
   ilqr_hip_reference_kinematics returns; ilqr_hip_get_al_task_points reports the coordinates the bounds act on.
   The bounds are always a WINDOW, [n_sets][N+1][ILQR_AL_TASK_BOUNDS = 18], row t = lo[9] then hi[9]; n_sets is 1 (every rollout reads the one
   window) or the batch (rollout b reads window b).  A fourth family beside the hinges, the actuators and the box coordinates, rule for rule
   the state family: the constraints p_k - hi and lo - p_k at the knots t = 0..N with the term phi per constraint; knot 0 carries the cost
   term, keeps zero multipliers and is left out of the violation (x_0 is given), the terminal knot is included; one penalty rho_task per
   rollout, starting at rho_task0 and capped at rho_max_factor rho_task0; after each inner solve mu <- max(0, mu + rho_task c) and viol_task =
   the largest max(0, c) over coordinates, sides and knots 1..N, in metres.  A rollout is done only when every installed family is within
   its tolerance (tol_task here); otherwise all penalties grow.  A done rollout is frozen as described above; ilqr_hip_al_update updates this
   family too.  Every other AL getter keeps its shape and meaning.
   STANCE KNOTS: a foot's three rows at a knot where the contact schedule (ilqr_hip_set_contact_schedule) has that foot in stance (flag 1)
   behave as rows with both sides switched off, whatever the window holds: there the stance constraint or the velocity term holds the foot.
   A constant "z >= z_min" on a foot therefore means swing clearance.
   A lower bound may be -inf and an upper bound +inf: that side is switched off as in the other families (c = -inf, term -mu^2 / (2 rho),
   zero gradient and curvature, multiplier driven to 0, violation 0).  The Hessian of the term is exact, second-order part included, as
   the tracking terms' is.  The window acts on the COST only: dynamics, plant and score are untouched.  It works with or without the other
   families' tables and windows; while it is installed the library repeats their records over the knots on the device, as it does when one
   of them has a window.
   ILQR_ERR_STATE while no augmented Lagrangian is installed (every handle call below).  ILQR_ERR_ARG: a null pointer, n_sets not 1 or the
   batch, a NaN, lo > hi, lo == +inf, hi == -inf in any row, rho_task0 <= 0 or not finite, tol_task < 0; everything is checked before the
   handle is touched, a refused call leaves a previously installed window as it was.  ILQR_ERR_UNSUPPORTED when libilqr_hip_alknot.so beside
   the library, which holds every kernel of this family, cannot be loaded.  Allocates the third multiplier store on first use ([B] records
   of 16 + 32 (N + 1) doubles: al_task_dev.h).  Installing where no window was installed zeroes the task multipliers; replacing a window
   keeps them; rho_task = rho_task0 either way.  Uploads and synchronises the handle's stream.
   The window is horizon-local: a warm start shifts the multipliers and does not move it.  It survives the cold and warm initialisers,
   ilqr_hip_set_al_multipliers, the other families coming and going and a repeated ilqr_hip_set_augmented_lagrangian;
   ilqr_hip_clear_augmented_lagrangian drops it.  The cold initialisers zero the task multipliers and reset rho_task; the warm ones shift
   them by the knots the trajectory is shifted by (zero tail, knot 0 zero) and reset rho_task.  The refusals of
   ilqr_hip_set_augmented_lagrangian (cross-check families, weight sets) stay as they are.  ilqr_hip_set_al_bounds_track does not cut this
   family; a track of its own does (ilqr_hip_set_al_task_bounds_track). */
#define ILQR_AL_TASK_COORDS 9
#define ILQR_AL_TASK_BOUNDS 18
int ilqr_hip_set_al_task_bounds(ilqr_hip_ctx* ctx, const double* bounds /*[n_sets][N+1][18]*/, int n_sets, double rho_task0, double tol_task);
/* No task family any more (same kernels and kernel arguments as a handle that never had a window). */
int ilqr_hip_clear_al_task_bounds(ilqr_hip_ctx* ctx);
/* 0: no window installed, else the n_sets of the installed window (1 or the batch); -1 for a null handle */
int ilqr_hip_num_al_task_bound_sets(const ilqr_hip_ctx* ctx);
/* The window each rollout is solved with: a one-set window expanded; without a window lo = -inf, hi = +inf in every row.  (Rows of a foot
   in stance are returned as installed; the kernels do not read them.)  Synchronises the handle's stream. */
int ilqr_hip_get_al_task_bounds(ilqr_hip_ctx* ctx, double* bounds /*[B][N+1][18]*/);
/* The task multipliers, (lower, upper) per task coordinate; zeros without a window. */
int ilqr_hip_get_al_task_multipliers(ilqr_hip_ctx* ctx, double* mu /*[B][N+1][9][2]*/);
/* Either pointer may be NULL (that part stays).  Multipliers >= 0, penalties > 0, else ILQR_ERR_ARG; knot-0 entries are stored as zero.
   ILQR_ERR_STATE without a window. */
int ilqr_hip_set_al_task_multipliers(ilqr_hip_ctx* ctx, const double* mu /*[B][N+1][9][2]*/, const double* rho /*[B]*/);
/* rho_task as the store holds it; zeros without a window */
int ilqr_hip_get_al_task_penalties(ilqr_hip_ctx* ctx, double* rho /*[B]*/);
/* viol_task of the nominal trajectory at the last update; zeros without a window (the done flags: ilqr_hip_get_al_violation) */
int ilqr_hip_get_al_task_violation(ilqr_hip_ctx* ctx, double* viol /*[B]*/);
/* Per round of the last solve and rollout: viol_task and the rho_task the round ran with.  NaN where ilqr_hip_get_al_trace has NaN, and
   everywhere without a window. */
int ilqr_hip_get_al_task_trace(ilqr_hip_ctx* ctx, double* out /*[rounds][B][2]*/);
/* The nine task coordinates of every knot of the resident nominal trajectory, as the kernels of this family compute them (each coordinate
   is the same double in the cost, the quadratics and the update): what a user plots against the window.  Needs an installed augmented
   Lagrangian (ILQR_ERR_STATE) and an initialised trajectory (ILQR_ERR_STATE), not a task window; ILQR_ERR_UNSUPPORTED without the module.
   Synchronises the handle's stream. */
int ilqr_hip_get_al_task_points(ilqr_hip_ctx* ctx, double* out /*[B][N+1][9]*/);
/* The VELOCITIES of those nine coordinates at every knot of the resident nominal trajectory, world frame, m/s: the velocity of the
   whole-body centre of mass (k = 0..2), of the left ankle origin (k = 3..5) and of the right ankle origin (k = 6..8) -- the quantities
   R(quat) gamma_s(theta, v) the cost penalises softly (w_com_vel, w_ee_vel), in Pinocchio's velocity convention (the base's linear and
   angular velocity in the body frame), with the rotation polynomial on the raw quaternion and the URDF link masses.  What a user plots
   against a cap on the stance foot's slip or on the speed of the centre of mass; bounds on these velocities are not built.
   Needs an installed augmented Lagrangian (ILQR_ERR_STATE) and an initialised trajectory (ILQR_ERR_STATE), not a task window;
   ILQR_ERR_ARG for a null pointer; ILQR_ERR_UNSUPPORTED without libilqr_hip_alknot.so, which holds the kernel.  Synchronises the handle's
   stream. */
#define ILQR_AL_TASK_VEL_COORDS 9
int ilqr_hip_get_al_task_velocities(ilqr_hip_ctx* ctx, double* out /*[B][N+1][9]*/);
/* The task family's part of the bounds track: `rows` >= 1 rows lo[9], hi[9] on the loop's timeline over the task coordinates above, with a
   row count of its own, independent of ilqr_hip_set_al_bounds_track's (on the device a row is padded to 32 doubles, two whole lines).  One
   upload; the handle owns the copy and a new task track replaces it.  ilqr_hip_al_bounds_window_from_track cuts every installed part in one
   kernel; afterwards the handle is in the state ilqr_hip_set_al_task_bounds(the same window cut on the host, n_sets = the number of starts)
   leaves, multipliers and penalties untouched; the stance rule is unchanged (the kernels keep reading the schedule window).  The track
   supplies bounds only: rho_task0 and tol_task stay the installation's.  The start rows are the ones ilqr_hip_set_al_bounds_track_starts
   sets, shared with the other track; installing either track sets them back to one shared start of 0.
   Validation row by row as in the window setter (ILQR_ERR_ARG: a null pointer, rows < 1, a NaN, lo > hi, lo == +inf, hi == -inf).
   ILQR_ERR_STATE without an augmented Lagrangian or without an installed task family.  ILQR_ERR_UNSUPPORTED without the module.  A refused
   call leaves what was installed as it was.  Synchronises the handle's stream. */
int ilqr_hip_set_al_task_bounds_track(ilqr_hip_ctx* ctx, int rows, const double* task /*[rows][18]*/);
/* Frees the task track; the window last written stays installed.  Synchronises the handle's stream. */
int ilqr_hip_clear_al_task_bounds_track(ilqr_hip_ctx* ctx);
/* Rows of the installed task bounds track; 0 without one, -1 for a null handle */
int ilqr_hip_al_task_bounds_track_rows(const ilqr_hip_ctx* ctx);
/* RobotUtils::setGravity -- src/common/robot_utils.cpp:782-789 */
int ilqr_hip_set_gravity(ilqr_hip_ctx* ctx, double gx, double gy, double gz);
/* RobotUtils::loadContactSchedule / isStance -- src/common/robot_utils.cpp:445-504; horizon-local rows 0..N
   (the reference indexes the schedule with the horizon-local t). stance[n_sets][N+1][2] */
int ilqr_hip_set_contact_schedule(ilqr_hip_ctx* ctx, const int* stance, int n_sets);
/* RobotUtils::getEEReference / getCoMVelReference -- src/common/robot_utils.cpp:525-549.
   ee_ref[n_sets][N+1][2][3] (left, right ankle), com_vel_ref[n_sets][N+1][3] (may be NULL -> zeros) */
int ilqr_hip_set_ee_references(ilqr_hip_ctx* ctx, const double* ee_ref, const double* com_vel_ref, int n_sets);
/* reference window handed to solve(): x_ref[n_sets][N+1][51], u_ref[n_sets][N][19], com_ref[n_sets][N+1][3]
   (MPC::extractReferenceWindow, src/ilqr/mpc.cpp:163-166) */
int ilqr_hip_set_references(ilqr_hip_ctx* ctx, const double* x_ref, const double* u_ref, const double* com_ref, int n_sets);

/* iLQR::setRegularization / setMaxIterations / setTolerance -- include/ilqr/ilqr.hpp:22-24.
   setRegularization resets every rollout's lambda (lambda persists across solves, ilqr.hpp:54). */
int ilqr_hip_set_regularization(ilqr_hip_ctx* ctx, double lambda);
int ilqr_hip_set_max_iterations(ilqr_hip_ctx* ctx, int max_iter);
int ilqr_hip_set_tolerance(ilqr_hip_ctx* ctx, double tol);
/* build-specific options: Jacobian mode, FD step, early_exit (0 = run exactly max_iter iterations) */
int ilqr_hip_set_options(ilqr_hip_ctx* ctx, int jacobian_mode, double fd_eps, int early_exit);

/* iLQR::initializeWithReference -- include/ilqr/ilqr.hpp:40-45, src/ilqr/ilqr.cpp:50-117.
   x0[B][51]; cold start: u_init[B][N][19] or NULL (gravity compensation, RobotUtils::computeGravComp,
   src/common/robot_utils.cpp:844-866 with the correct dof index) followed by N rollouts;
   warm start: prev_xbar[B][N+1][51], prev_ubar[B][N][19] shifted by one knot (ilqr.cpp:68-80). */
int ilqr_hip_initialize(ilqr_hip_ctx* ctx, const double* x0, const double* u_init, const double* prev_xbar, const double* prev_ubar);
/* warm start from the solver's own previous solution kept on the device (MPC::stepOnce, src/ilqr/mpc.cpp:58-60) */
int ilqr_hip_initialize_warm_resident(ilqr_hip_ctx* ctx, const double* x0);
/* The same after `shift` knots of the policy have been applied since the last solve (1 <= shift <= N - 1, else ILQR_ERR_ARG): see
   ilqr_hip_initialize_warm_from_plant_shifted, whose x0 comes from the plant; this one uploads it and synchronises.  Generalises
   ilqr.cpp:68-80 (the reference shifts by one knot, because it solves every step). */
int ilqr_hip_initialize_warm_resident_shifted(ilqr_hip_ctx* ctx, const double* x0, int shift);
/* device-resident variant of the cold start: x0_device[B][51], u_init_device[B][N][19] are HIP device pointers */
int ilqr_hip_initialize_device(ilqr_hip_ctx* ctx, const double* x0_device, const double* u_init_device);

/* iLQR::solve -- include/ilqr/ilqr.hpp:27-31, src/ilqr/ilqr.cpp:521-660.  References are the ones last set
   with ilqr_hip_set_references; x0[B][51] (host) or NULL to reuse the x0 given to initialize.
   cost_out[B] may be NULL.  Runs asynchronously on the handle's stream and synchronises before returning. */
int ilqr_hip_solve(ilqr_hip_ctx* ctx, const double* x0, double* cost_out);
/* enqueue only (nothing copied back); pair with ilqr_hip_synchronize.
   With the reference's convergence exit on (ilqr_hip_set_options early_exit = 1, the default; ilqr.cpp:645-655) AND the
   early-exit gate on (ilqr_hip_set_early_exit_gate, default on) this call BLOCKS the host while it enqueues: it launches
   iteration i only after it has seen how many rollouts were still active after iteration i - 2, and stops once that count is
   zero.  The device never waits (one full iteration stays queued), but a host thread that drives several handles, or overlaps
   its own work with the solve, should turn the gate off for a handle: the call then enqueues all max_iter iterations and
   returns at once (converged rollouts are masked out on the device, results are identical). */
int ilqr_hip_solve_async(ilqr_hip_ctx* ctx);
/* per-handle switch of the early-exit gate described above (1 = on, the default).  The environment variable ILQR_EE_GATE,
   when set, overrides it for every handle of the process (diagnostics). */
int ilqr_hip_set_early_exit_gate(ilqr_hip_ctx* ctx, int on);
int ilqr_hip_synchronize(ilqr_hip_ctx* ctx);

/* accessors: iLQR::xbar/ubar/gainsK/gainsKff -- include/ilqr/ilqr.hpp:34-37 */
int ilqr_hip_get_xbar(ilqr_hip_ctx* ctx, double* xbar /*[B][N+1][51]*/);
int ilqr_hip_get_ubar(ilqr_hip_ctx* ctx, double* ubar /*[B][N][19]*/);
int ilqr_hip_get_gains_K(ilqr_hip_ctx* ctx, double* K /*[B][N][19][51]*/);
int ilqr_hip_get_gains_kff(ilqr_hip_ctx* ctx, double* kff /*[B][N][19]*/);
int ilqr_hip_get_cost(ilqr_hip_ctx* ctx, double* cost /*[B]*/);
int ilqr_hip_get_iterations(ilqr_hip_ctx* ctx, int* iters /*[B]*/);
int ilqr_hip_get_lambda(ilqr_hip_ctx* ctx, double* lambda /*[B]*/);
/* per-iteration trace (parity artefact; the reference keeps these internal):
   cost[B][max_iter+1] (entry 0 = initial cost), alpha[B][max_iter] (0 = no step), lambda[B][max_iter] */
int ilqr_hip_get_trace(ilqr_hip_ctx* ctx, double* cost, double* alpha, double* lambda);
/* first-knot results gathered per MPC step: u0[B][19], K0[B][19][51] (either may be NULL); device pointers */
int ilqr_hip_first_knot_device(ilqr_hip_ctx* ctx, const double** u0_device, const double** K0_device, const double** cost_device);
/* same payload written into CALLER-owned device buffers (the send buffer of the per-step RCCL gather):
   u0_out[B][19], K0_out[B][19][51] (nullable), cost_out[B] (nullable); synchronises the handle's stream */
int ilqr_hip_pack_first_knot_device(ilqr_hip_ctx* ctx, double* u0_out_device, double* K0_out_device, double* cost_out_device);

/* ---- multi-GPU: one handle per GPU, one process or thread per handle.  The reference is single
   process; its consumer of the result is MPC::stepOnce (src/ilqr/mpc.cpp:97-113: u_apply from ubar[0], K[0]).  The global
   batch is cut into contiguous shards, rank r owning rollouts [r B, (r + 1) B); the only exchange is ONE gather per MPC
   step of the first-knot payload row [u0(19) | cost | K0(19 x 51) if with_gains] of every rollout to `root`, in global
   rollout order -- RCCL grouped send/recv over xGMI on the handle's stream.  librccl is opened on first use.
     rank 0: ilqr_hip_comm_get_unique_id(id) -> hand the 128 bytes to every rank (file, socket, MPI, torch.distributed ...)
     all   : ilqr_hip_comm_init(ctx, world, rank, id)        (world == 1: no RCCL, the gather is a device copy)
     step  : solve ...; ilqr_hip_gather_first_knot(ctx, root, with_gains, recv); ilqr_hip_synchronize(ctx)
   recv_device (root only, else NULL): device buffer [world * B][ilqr_hip_payload_width(with_gains)]. */
#define ILQR_COMM_ID_BYTES 128
int ilqr_hip_payload_width(int with_gains);
/* 1 if librccl can be opened and resolves every entry point the gather needs, else 0.  ncclCommInitRank is collective: a rank
   that cannot load the library would leave its peers waiting inside ilqr_hip_comm_init, so a launcher lets every rank check
   this (and agree on the outcome) BEFORE any rank calls ilqr_hip_comm_init with world > 1 (bench.py does). */
int ilqr_hip_comm_available(void);
int ilqr_hip_comm_get_unique_id(char* id /*[ILQR_COMM_ID_BYTES]*/);
int ilqr_hip_comm_init(ilqr_hip_ctx* ctx, int world, int rank, const char* id /*[ILQR_COMM_ID_BYTES], may be NULL when world == 1*/);
int ilqr_hip_comm_destroy(ilqr_hip_ctx* ctx);
int ilqr_hip_comm_world(const ilqr_hip_ctx* ctx);
int ilqr_hip_comm_rank(const ilqr_hip_ctx* ctx);
int ilqr_hip_gather_first_knot(ilqr_hip_ctx* ctx, int root, int with_gains, double* recv_device);

/* MPC::stepOnce control law u = ubar[0] + K[0](x_meas - xbar[0]) -- src/ilqr/mpc.cpp:97-101 */
int ilqr_hip_compute_control(ilqr_hip_ctx* ctx, const double* x_measured /*[B][51]*/, double* u_apply /*[B][19]*/);
/* The law of src/ilqr/mpc.cpp:97-101 on knot `knot` (0 .. N - 1, else ILQR_ERR_ARG) of the policy: u = ubar_knot + K_knot (x - xbar_knot),
   for a caller that keeps the plant itself and solves every m-th interval (the reference solves every step and only ever uses knot 0).
   knot = 0 equals ilqr_hip_compute_control bit for bit. */
int ilqr_hip_compute_control_at(ilqr_hip_ctx* ctx, int knot, const double* x_measured /*[B][51]*/, double* u_apply /*[B][19]*/);

/* ---- stage entry points (one reference function each; used by the parity tests and the bench breakdown) ---- */
int ilqr_hip_set_trajectory(ilqr_hip_ctx* ctx, const double* xbar, const double* ubar);   /* overwrite nominal trajectory */
int ilqr_hip_stage_rollout(ilqr_hip_ctx* ctx);          /* iLQR::forwardRolloutNominal, src/ilqr/ilqr.cpp:119-124 (+ total cost) */
int ilqr_hip_stage_linearize(ilqr_hip_ctx* ctx);        /* iLQR::computeLinearization, src/ilqr/ilqr.cpp:126-131 */
int ilqr_hip_stage_cost_quadratics(ilqr_hip_ctx* ctx);  /* iLQR::computeCostQuadratics, src/ilqr/ilqr.cpp:133-244 */
int ilqr_hip_stage_backward_pass(ilqr_hip_ctx* ctx);    /* iLQR::backwardPass, src/ilqr/ilqr.cpp:250-309 */
int ilqr_hip_stage_line_search(ilqr_hip_ctx* ctx, int* improved /*[B]*/, double* new_cost /*[B]*/, double* alpha /*[B]*/); /* ilqr.cpp:311-361 */
int ilqr_hip_stage_total_cost(ilqr_hip_ctx* ctx, double* cost /*[B]*/);  /* iLQR::computeTotalCost, src/ilqr/ilqr.cpp:363-518 */
int ilqr_hip_get_linearization(ilqr_hip_ctx* ctx, double* A /*[B][N][51][51]*/, double* B /*[B][N][51][19]*/);
int ilqr_hip_set_linearization(ilqr_hip_ctx* ctx, const double* A, const double* B);
int ilqr_hip_get_quadratics(ilqr_hip_ctx* ctx, double* lx /*[B][N+1][51]*/, double* lu /*[B][N][19]*/, double* lxx /*[B][N+1][51][51]*/, double* luu_diag /*[B][N][19]*/);
int ilqr_hip_set_quadratics(ilqr_hip_ctx* ctx, const double* lx, const double* lu, const double* lxx, const double* luu_diag);
int ilqr_hip_get_value_function(ilqr_hip_ctx* ctx, double* Vx /*[B][51]*/, double* Vxx /*[B][51][51]*/); /* at knot 0 after the backward pass */
/* one dynamics step for arbitrary (x,u) pairs: RobotUtils::rolloutOneStep, src/common/robot_utils.cpp:106-117 */
int ilqr_hip_step(ilqr_hip_ctx* ctx, int count, const double* x /*[count][51]*/, const double* u /*[count][19]*/, double* x_next /*[count][51]*/);

/* Contact row.  The reference's plant is MuJoCo with floor contacts (mj_step inside
   RobotUtils::rolloutOneStep, src/common/robot_utils.cpp:106-117).  ILQR_CONTACT_RIGID_STANCE restates the regime its
   scenarios run in: a foot the contact schedule (ilqr_hip_set_contact_schedule, horizon-local rows) marks as stance does
   not move -- velocity-level constraint on the ankle link over one step, solved through the articulated-body
   quantities; `softness` (> 0: set, <= 0: keep, default 1e-5 / kg) regularises the constraint-space inertia.  Rollout, line
   search, warm-start step and plant run on the two-lane register / LDS kernels with the constraint solve in them; the
   Jacobians are analytic (ILQR_JAC_ANALYTIC: derivative of the constrained step with the active set held fixed) or the
   reference's forward differences (ILQR_JAC_FD_FORWARD, robot_utils.cpp:120-160), as ilqr_hip_set_options selects.
   ilqr_hip_step_stance: one step with explicit stance flags (the flags only matter in contact mode).
   ILQR_CONTACT_UNILATERAL_STANCE: the same constraint, but the floor only pushes: a scheduled stance foot whose constraint
   force has a negative component along the world up axis is released for that step and the remaining set solved again.
   ILQR_CONTACT_FRICTION_STANCE: unilateral, and sticking is limited by Coulomb friction, the other half of what MuJoCo's floor
   contacts do inside mj_step: a foot whose constraint force leaves the cone |f_t| <= mu f_n (f_n along the world up axis) slides --
   its two tangential translation rows are dropped (rotation and normal rows stay, no tangential force on a sliding foot) and
   the set is solved again, once.  mu: ilqr_hip_set_friction (default 1, MuJoCo's default sliding friction; the reference's
   robots/h1_description/mjcf model sets none).  Jacobians in this mode: the reference's forward differences, or analytic
   (decisions held fixed; a sliding foot's normal row and normal force turn with the foot: that term is carried).
   ILQR_CONTACT_KINETIC_FRICTION_STANCE: the same decision, but the sliding foot keeps kinetic friction: a tangential force mu f_n along
   the direction in which the sticking solution pulled (the one that opposes the slip); its normal multiplier then acts along
   up + mu t while the constraint row stays the normal one -- an unsymmetric 12 x 12 system, Gaussian elimination with partial
   pivoting for the knots where a foot slides.  Jacobians as mode 3; the analytic ones also carry the tangent of the sticking
   solve, which the friction direction t follows. */
enum ilqr_contact_mode { ILQR_CONTACT_NONE = 0, ILQR_CONTACT_RIGID_STANCE = 1, ILQR_CONTACT_UNILATERAL_STANCE = 2, ILQR_CONTACT_FRICTION_STANCE = 3,
                         ILQR_CONTACT_KINETIC_FRICTION_STANCE = 4 };
int ilqr_hip_set_contact_mode(ilqr_hip_ctx* ctx, int mode, double softness);
int ilqr_hip_set_friction(ilqr_hip_ctx* ctx, double mu);
/* Joint-limit rows of the plant: the reference's plant is mj_step (src/common/robot_utils.cpp:106-117), which
   enforces the hinge ranges of robots/h1_description/mjcf/h1.xml (jnt_range, :55-151) as constraints that are active only when violated;
   the cost side only carries the soft penalty (RobotUtils::constraintCost, robot_utils.cpp:615-672).  Restated here as the rigid,
   velocity-level limit of that constraint, like the stance rows: a hinge past its range that the step would still move outward
   (v_i + h qacc_i points out of the range, qacc of the step without these rows) is stopped over the step, v_i+ = 0 -- its acceleration
   is prescribed, qacc_i = -v_i / h, in a second pass of the articulated-body recursion (Featherstone's hybrid dynamics; the stance
   rows of the contact modes are solved on that system).  A hinge past its range that moves back in is left alone; nothing pushes a
   hinge back unless ilqr_hip_set_joint_limit_stiffness gives the rows a restoring term.  Default off (the constraint-free restatement).
   Rollout, line search, plant step and both Jacobian schemes carry it (two-lane kernels, in instantiations of their own: with the
   option off every kernel keeps its machine code).  Analytic Jacobians: the dumped recursion has the stopped hinges
   acceleration-prescribed and d qacc_i = -1 / h rides the direction of a stopped hinge's own rate (decisions held fixed). */
int ilqr_hip_set_joint_limits(ilqr_hip_ctx* ctx, int on);
/* Restoring stiffness of the joint-limit rows (round 6; mj_step pushes a hinge back into its range, h1.xml:55-151 / robot_utils.cpp:113-114, the
   pure stop above does not).  MuJoCo drives a violated constraint towards the reference acceleration a_ref = -b v - k r (solref: b = 2 /
   (dmax timeconst), k = 1 / (dmax^2 timeconst^2 dampratio^2), timeconst clamped to 2 h); in the hard limit of its impedance the constrained
   hinge takes exactly that acceleration.  With k = stiffness the row prescribes qacc_i = -v_i / h - k r_i (r_i = q_i - hi_i > 0 or q_i - lo_i < 0:
   the violation; b = 1 / h is solref's damping at the clamped time constant), i.e. v_i+ = -h k r_i, and it is active when the step without the
   rows falls short of that acceleration on the outward side -- a hinge that drifts back in too slowly is constrained too, one that returns
   faster is left alone (the row only pushes).  k = 1 / (2 h)^2 (625 at h = 0.02) is solref's default time constant: a quarter of the violation
   per step.  0 (default): the pure stop, bit for bit.  Needs ilqr_hip_set_joint_limits(ctx, 1); carried by the step, rollout, line search and
   both Jacobian schemes (analytic: d qacc_i = -k rides the direction of the constrained hinge's own angle).  k < 0: ILQR_ERR_ARG. */
int ilqr_hip_set_joint_limit_stiffness(ilqr_hip_ctx* ctx, double stiffness);
int ilqr_hip_step_stance(ilqr_hip_ctx* ctx, int count, const double* x, const double* u, int stance_left, int stance_right, double* x_next);
/* Stance source of the dynamics (DESIGN 3.5 "Stance from the foot hulls").  The reference's plant and model are both mj_step
   (src/common/robot_utils.cpp:106-117), which finds contacts from geometry on every step; its cost takes isStance from the schedule
   (src/ilqr/ilqr.cpp:403-404,703).  ILQR_STANCE_SCHEDULE (default): the stance rows of contact modes 2-4 sit on the feet the contact
   schedule marks.  ILQR_STANCE_GEOMETRY: at the start of every dynamics step foot f is in stance iff its ankle-link hull reaches the
   floor, clearance_f(qpos_t) < 0 -- the rule of ilqr_hip_foot_clearance (get_contacts.py:96-147); release, friction and joint-limit rows
   then act as before.  Every step decides for itself: rollout, the line-search candidates, the warm-start step, the plant step and each
   forward-difference step (as mj_step does inside linearizeDynamicsFD, robot_utils.cpp:120-160); the analytic Jacobians hold the nominal
   knot's decisions fixed.  The cost keeps reading the schedule.  Valid with contact modes 2, 3 and 4; mode 1 (a weld: a welded foot never
   leaves) returns ILQR_ERR_UNSUPPORTED from whichever setter would create the combination, as does the scalar family (ILQR_DYN=s); mode 0
   stores the source and ignores it (no stance rows). */
enum ilqr_stance_source { ILQR_STANCE_SCHEDULE = 0, ILQR_STANCE_GEOMETRY = 1 };
int ilqr_hip_set_stance_source(ilqr_hip_ctx* ctx, int source);
/* Plant step with contacts from geometry (RobotUtils::rolloutOneStep, robot_utils.cpp:106-117): every item decides its stance from its
   own x and steps with the handle's contact mode, whatever the handle's stance source; stance_out[count][2] (nullable) = the flags it
   decided (left, right; before the unilateral release). */
int ilqr_hip_step_geometry(ilqr_hip_ctx* ctx, int count, const double* x, const double* u, double* x_next, int* stance_out);
/* The stance flags the dynamics use for the steps t = 0..N-1 of the current nominal trajectories, stance[B][N][2] (left, right):
   decided from xbar under ILQR_STANCE_GEOMETRY (get_contacts.py:96-147 applied to the nominal), the schedule's rows otherwise. */
int ilqr_hip_get_stance(ilqr_hip_ctx* ctx, int* stance);

/* ---- device-resident plant: the closed loop of runSimulation (main/humanoid_mpc.cpp:122-190) without a host round trip per MPC step.
   The reference's loop reads the plant state (:131-132), calls MPC::stepOnce (:143), holds u_apply for physics_steps_per_mpc =
   int(dt / physics_dt) plant steps (:128,167-170; physics_dt: config.yaml:19, main:99) and guards against non-finite states and controls
   (:134-137,162-165).  Here the plant state lives in the handle, one per rollout, and ONE kernel per MPC step advances it under the policy
   the handle has just solved -- the first knot (xbar_0, ubar_0, K_0) of "nominal trajectories + TV-LQR gains" (include/ilqr/ilqr.hpp:10-16).
   The plant is the model's dynamics (contact mode, friction, joint-limit rows, gravity of the handle) at the step dt / substeps.  Per MPC
   step:  set references / schedule -> ilqr_hip_initialize_warm_from_plant -> ilqr_hip_solve(ctx, NULL, cost) -> ilqr_hip_plant_advance;
   the solve's own synchronisation is the only one, provided the references do not change: the three reference setters upload and
   synchronise.  With a reference track on the device (ilqr_hip_set_reference_track, below) the order of MPC step k is
   ilqr_hip_window_from_track(ctx, k, follow_schedule) -> ilqr_hip_initialize_warm_from_plant -> ilqr_hip_solve(ctx, NULL, cost) ->
   ilqr_hip_plant_advance, and the solve's own synchronisation is the only one of the step for a moving reference too.  Solving every
   m-th interval only: ilqr_hip_initialize_warm_from_plant_shifted(ctx, m) -> ilqr_hip_solve -> ilqr_hip_plant_follow(ctx, 0, m), see
   there.  External wrenches on the pelvis: ilqr_hip_plant_set_wrench, below; a plant whose contact model or parameters are not the
   solver's: ilqr_hip_plant_set_model / ilqr_hip_plant_set_params; a plant that carries a load the solver does not know of:
   ilqr_hip_plant_set_payload. */
/* Upload the plant state x[B][51] (robot.getState's counterpart in reverse: RobotUtils::setState).  Every rollout becomes alive, a pending
   kick is dropped, the history cursor returns to 0.  Synchronises the handle's stream. */
int ilqr_hip_plant_reset(ilqr_hip_ctx* ctx, const double* x /*[B][51]*/);
/* substeps >= 1: plant steps per MPC step, each of dt / substeps (main:128).  feedback_mode 0: the reference's loop, u = ubar_0 +
   K_0 (x - xbar_0) evaluated once and held (main:167-170); 1: the same law re-evaluated on (xbar_0, ubar_0, K_0) before every substep --
   the gains tracked at the physics rate.  contact_source: ILQR_STANCE_SCHEDULE -- the stance rows of contact modes 1-4 sit on the feet
   that row 0 of the current contact schedule marks (per set); ILQR_STANCE_GEOMETRY -- every substep decides from the plant's own foot
   hulls, as ilqr_hip_step_geometry does (refused with ILQR_ERR_UNSUPPORTED where ilqr_hip_set_stance_source refuses; contact mode 0 has no
   stance rows and ignores it).  Defaults 1, 0, SCHEDULE.  Anything else: ILQR_ERR_ARG.  Launches nothing. */
int ilqr_hip_plant_configure(ilqr_hip_ctx* ctx, int substeps, int feedback_mode, int contact_source);
/* Arm a one-shot velocity kick dv[B][25] (order of qvel): the next advance adds it to the plant's qvel before it evaluates the control law,
   then it is gone.  Synchronises the handle's stream (the caller's buffer is free on return).  No reference counterpart; a sustained
   force is ilqr_hip_plant_set_wrench. */
int ilqr_hip_plant_kick(ilqr_hip_ctx* ctx, const double* dv /*[B][25]*/);
/* One MPC interval of the plant (main:162-170): kick, control law (src/ilqr/mpc.cpp:97-101; a u with a non-finite entry becomes zero,
   main:162-165; the step clamps u to the control range, the reported u is unclamped), `substeps` plant steps, then x, u (as applied in the
   last substep), the stance flags of the last substep and `alive` are written back, and a row of the history ring if there is one.
   A rollout whose state is or becomes non-finite (main:134-137 breaks the loop) gets alive = 0 and is never advanced again: its state stays
   as it was before that advance, its control reads zero; the other rollouts are not affected by it.  ENQUEUES on the handle's stream and
   returns: no synchronisation.  The plant always runs on the two-lane step (the default family's), also on a handle of the test library
   whose environment selects the scalar dynamics (ILQR_DYN=s), where ilqr_hip_step runs the scalar kernel.
   ILQR_ERR_STATE before the first solve or before ilqr_hip_plant_reset; ILQR_ERR_UNSUPPORTED while an
   ILQR_ENV_PER_CALL re-read names an absent kernel family (see ilqr_hip_reload_environment) or the GEOMETRY source meets contact mode 1. */
int ilqr_hip_plant_advance(ilqr_hip_ctx* ctx);
/* ilqr_hip_initialize_warm_resident with x0 taken from the plant state on the device (MPC::stepOnce, src/ilqr/mpc.cpp:58-60; shift of
   ilqr.cpp:68-80): same kernels, same result bit for bit, nothing uploaded and NO synchronisation.  ILQR_ERR_STATE before a first
   initialize or before ilqr_hip_plant_reset. */
int ilqr_hip_initialize_warm_from_plant(ilqr_hip_ctx* ctx);
/* `count` consecutive MPC intervals of the plant in ONE kernel, under the knots first_knot .. first_knot + count - 1 of the policy of the
   last solve: interval j applies u = ubar_k + K_k (x - xbar_k), k = first_knot + j -- the law of src/ilqr/mpc.cpp:97-101 and the loop body
   of main/humanoid_mpc.cpp:162-170 with the knot index in the place of 0 -- and stands on row k of the contact schedule (or on the foot
   hulls).  The reference itself solves before every interval and never reads more than knot 0 of its gains; this is the deployment in
   which a solve takes longer than the control period.  Everything else is ilqr_hip_plant_advance, `count` times: a pending kick lands
   before the first interval only, every interval fills one row of the history ring (the ring may wrap inside the call), a rollout whose
   state is or becomes non-finite in interval j is frozen there exactly as separate advances would freeze it (its later rows log the frozen
   state and zero control), and x, u, stance, alive are written back once, at the end.  (0, 1) is ilqr_hip_plant_advance.  ENQUEUES only.
   ILQR_ERR_ARG unless first_knot >= 0, count >= 1, first_knot + count <= N; ILQR_ERR_STATE / ILQR_ERR_UNSUPPORTED as the advance. */
int ilqr_hip_plant_follow(ilqr_hip_ctx* ctx, int first_knot, int count);
/* ilqr_hip_initialize_warm_from_plant after `shift` followed intervals, 1 <= shift <= N - 1 (else ILQR_ERR_ARG): the shift of
   ilqr.cpp:68-80 by `shift` knots instead of one -- xbar_0 = the plant state, xbar_t = previous xbar_{t + shift} for 1 <= t <= N - shift,
   ubar_t = previous ubar_{min(t + shift, N - 1)} -- and ONE kernel that re-rolls xbar_{t + 1} = f(xbar_t, ubar_t), t = N - shift .. N - 1,
   under row t of the schedule now set (the reference re-rolls its one last knot, ilqr.cpp:72-80, and solves every step).  shift = 1 gives
   the result of ilqr_hip_initialize_warm_from_plant bit for bit.  On a handle of the test library whose environment selects the scalar
   dynamics the tail still runs on the default family's step, as the plant does.  ENQUEUES only; ILQR_ERR_STATE as the one-knot call. */
int ilqr_hip_initialize_warm_from_plant_shifted(ilqr_hip_ctx* ctx, int shift);
/* History ring of `steps` rows (0: free it): every advance appends the state it started from (behind its kick -- the x the control law
   saw) and the control it reported; the oldest row is overwritten once the ring is full.  Resets the cursor; synchronises. */
int ilqr_hip_plant_set_history(ilqr_hip_ctx* ctx, int steps);
/* x[rows][B][51], u[rows][B][19] (either may be NULL; sized for the ring's rows), oldest first; *steps_recorded = min(advances since the
   last reset / set_history, rows).  ONE synchronisation for the whole run and at most two copies per array (a ring that has wrapped is two
   contiguous runs) -- MPC::logCurrentStep's data, src/ilqr/mpc.cpp:181-262. */
int ilqr_hip_plant_get_history(ilqr_hip_ctx* ctx, double* x, double* u, int* steps_recorded);
/* robot.getState (main:131-132) and the companions of the last advance; each synchronises the handle's stream.  ILQR_ERR_STATE before
   ilqr_hip_plant_reset. */
int ilqr_hip_plant_get_state(ilqr_hip_ctx* ctx, double* x /*[B][51]*/);
int ilqr_hip_plant_get_control(ilqr_hip_ctx* ctx, double* u /*[B][19]*/);
int ilqr_hip_plant_get_stance(ilqr_hip_ctx* ctx, int* stance /*[B][2]*/);
int ilqr_hip_plant_get_alive(ilqr_hip_ctx* ctx, int* alive /*[B]*/);
/* The plant state as a device pointer [B][51], for a caller that chains its own kernels on ilqr_hip_stream; no synchronisation. */
int ilqr_hip_plant_state_device(ilqr_hip_ctx* ctx, const double** x_device);
/* ---- closed-loop score of the plant: which rollout's closed loop did best.  While a score is installed every ilqr_hip_plant_advance /
   ilqr_hip_plant_follow is followed, on the same stream, by two small kernels that evaluate the terms of iLQR::computeTotalCost
   (src/ilqr/ilqr.cpp:363-518) of every interval the call ran and add them to a record of ILQR_PLANT_SCORE_TERMS doubles per rollout:
     0  sum of 1/2 sum_i Q_i (x_i - x_ref[k]_i)^2        1  sum of 1/2 sum_i R_i (u_i - u_ref[k]_i)^2
     2  sum of the upright term (0 while w_upright == 0)
     3  sum of the capture-point term: support point from row k of the contact SCHEDULE and of ee_ref, MuJoCo CoM (0 for a row without a
        stance foot or while w_balance == 0)
     4  sum of the joint-limit soft penalty (10 % margins)   5  sum of the control-limit soft penalty on the reported, unclamped u
     6  minimum of x[2] (pelvis height) over the scored intervals, +inf before the first; a NaN height is ignored
     7  number of intervals scored, as a double
   -- the expressions of a non-terminal knot of the solver's cost, under ONE shared set of scoring weights that is independent of the
   solver's weights (ilqr_hip_set_cost_weights ...) and of an installed weight-set table: in a weight sweep every rollout is measured with
   the same ruler.  (x, u) of an interval are exactly the row the plant appends to the history ring (the state behind the kick, the control
   reported; a frozen rollout scores the rows the ring logs for it, a non-finite row makes that rollout's sums non-finite and touches no
   other rollout).  Reference row k: 0 of the window currently set for ilqr_hip_plant_advance, first_knot + j for interval j of
   ilqr_hip_plant_follow; x_ref, u_ref, ee_ref and the schedule alike, each rollout its own set where the sets are per rollout.
   The record is a pure function of ring rows, reference rows and scoring weights, and is accumulated without atomics in interval order:
   ilqr_hip_plant_follow(0, m) and m calls (j, 1) give the same record bit for bit.
   Ring requirement: the score kernels read the ring, so with a score installed a plant call whose intervals exceed the ring's rows (no
   ring at all; count > rows) returns ILQR_ERR_STATE before anything is launched or counted.  The ring may be as small as the largest
   call: a run of any length is scored without keeping or downloading its history.
   set_score: installs the weights (Q_diag[51], R_diag[19]) and empties the record (calling it again empties it again); synchronises the
   handle's stream.  ILQR_ERR_ARG for a null argument or a negative / non-finite weight.  ilqr_hip_plant_reset empties the record too.
   clear_score: frees it; the plant calls then launch exactly what they launch without it.
   get_score: score[B][8], synchronises the handle's stream; score_device: the record as a device pointer, no synchronisation.  Both
   ILQR_ERR_STATE while no score is installed. */
#define ILQR_PLANT_SCORE_TERMS 8
int ilqr_hip_plant_set_score(ilqr_hip_ctx* ctx, const double* Q_diag /*[51]*/, const double* R_diag /*[19]*/, double w_upright, double w_balance, double w_joint_limits, double w_control_limits);
int ilqr_hip_plant_clear_score(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_get_score(ilqr_hip_ctx* ctx, double* score /*[B][8]*/);
int ilqr_hip_plant_score_device(ilqr_hip_ctx* ctx, const double** score_device);
/* ---- task score of the plant: did the TRUE trajectory obey the task bounds (ilqr_hip_set_al_task_bounds) -- did the foot clear the floor,
   land on the stone, did the centre of mass stay over the box -- under every way the plant can differ from the solver's model.  While it is
   installed every ilqr_hip_plant_advance / ilqr_hip_plant_follow is followed, on the same stream, by two small kernels (behind the cost
   score's when both are installed).  For interval j of the call they read the state row the plant appended to the history ring and score
   it against row k of the task window the handle currently holds, whoever wrote it (a setter or ilqr_hip_al_bounds_window_from_track):
   k = 0 for ilqr_hip_plant_advance, first_knot + j for ilqr_hip_plant_follow.  The stance flags are those of schedule row k, each rollout
   its own set where the sets are per rollout.
   With p the nine points of that state -- the doubles ilqr_hip_get_al_task_points and the solver's kernels form -- the violation of task
   coordinate i is v_i = max(0, p_i - hi_i, lo_i - p_i), written as compares: an infinite side never counts, and a foot's three rows are off
   where the schedule has that foot in stance (the solver's rule: a standing foot below a clearance floor scores nothing).  Groups g = CoM,
   left foot, right foot; V_g = max of v_i over the group.  The record, ILQR_PLANT_TASK_SCORE_TERMS doubles per rollout:
     0, 1, 2  maximum of V_g over the scored intervals, in metres; 0 before the first interval
     3, 4, 5  number of intervals with V_g > tol, as doubles
     6        sum over intervals and coordinates of v_i^2
     7        number of intervals scored, as a double
   An interval with a non-finite point adds NaN to slot 6, is counted in slot 7, is left out of slots 0..5 and touches no other rollout.
   The record is a pure function of ring rows, window rows, schedule rows and tol, accumulated without atomics in interval order:
   ilqr_hip_plant_follow(0, m) and m calls (j, 1) give the same record bit for bit.
   Ring requirement: the score kernels read the ring, so with a score installed a plant call whose intervals exceed the ring's rows (no
   ring at all; count > rows) returns ILQR_ERR_STATE before anything is launched or counted.  So does a plant call while the task score is
   installed and no task family is.
   set_task_score: tol >= 0 and finite (ILQR_ERR_ARG); installs and empties the record (again: empties it again); synchronises the handle's
   stream.  ilqr_hip_plant_reset empties the record too.  clear_task_score: frees it; the plant calls then launch exactly what they launch
   without it.  get_task_score: score[B][8], synchronises; task_score_device: the record as a device pointer, no synchronisation; both
   ILQR_ERR_STATE while none is installed.  Independent of ilqr_hip_plant_set_score: either, both or neither.  Physics, the cost score, the
   solver and the observation path are untouched: the score reads the truth. */
#define ILQR_PLANT_TASK_SCORE_TERMS 8
int ilqr_hip_plant_set_task_score(ilqr_hip_ctx* ctx, double tol);
int ilqr_hip_plant_clear_task_score(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_get_task_score(ilqr_hip_ctx* ctx, double* score /*[B][8]*/);
int ilqr_hip_plant_task_score_device(ilqr_hip_ctx* ctx, const double** score_device);
/* ---- the plant's own model and one parameter set per rollout: closed loops in which the plant is NOT the solver's model.  By default the
   plant steps with the handle's dynamics -- a loop in which the model is perfect; the reference's plant, mj_step, is not its solver's model
   either (main/humanoid_mpc.cpp:99-118 builds the two separately).  Both calls below change what ilqr_hip_plant_advance / _follow step
   with and nothing else: rollout, line search, Jacobians and warm-start tail keep the solver's model, and the solver's setters
   (ilqr_hip_set_gravity, ilqr_hip_set_friction, ilqr_hip_set_contact_mode, ...) keep acting on the solve (and on a plant that follows it).
   plant_set_model: the discrete part, shared by all rollouts.  contact_mode -1 (follow the solver's, the default) or 0..4
   (ILQR_CONTACT_*); joint_limits -1 (follow), 0 or 1; anything else ILQR_ERR_ARG.  The plant kernels then run in the instantiation of
   that pair; schedule row and stance source act as before, on the plant's mode.  The refusal of the stance source GEOMETRY (contact mode
   1; scalar family) is evaluated against the plant's effective mode, here, in ilqr_hip_plant_configure and in the launching calls
   (ILQR_ERR_UNSUPPORTED).  Launches nothing.
   plant_set_params: the continuous part, ILQR_PLANT_PARAMS doubles per set --
     0..2 gravity   3 friction coefficient mu (acts in plant contact modes 3 and 4)   4 contact softness (modes 1-4)
     5 joint-limit stiffness (with the plant's joint-limit rows on)   6 torque gain
   -- n_sets = 1 (one set that every rollout reads) or the batch (rollout b steps with set b), else ILQR_ERR_ARG; ILQR_ERR_ARG also for a
   null pointer, a non-finite entry, mu < 0, softness <= 0, limit_stiffness < 0 or torque_gain < 0.  While a table is installed the set
   replaces gravity, friction, softness and stiffness of the handle in the plant's step; the step size stays dt / substeps.  The torque
   gain is an actuator mismatch: the step receives gain * u, with u the control law's output behind its non-finite guard (main:162-165),
   and clamps to the control range as before; the REPORTED control (ilqr_hip_plant_get_control, the history ring, hence the score) stays
   the law's output, unscaled, as it is unclamped.  The table is a device buffer of 64-byte records owned by the handle; the call uploads
   it and synchronises the handle's stream.  It survives ilqr_hip_plant_reset and ilqr_hip_plant_configure.
   plant_clear_params: frees it; the plant calls then launch exactly what they launch without it.
   plant_num_param_sets: 0 without a table, else n_sets; -1 for a null handle.
   plant_get_params: params[B][7], the values the plant would step rollout b with now -- without a table the handle's and gain 1. */
#define ILQR_PLANT_PARAMS 7   /* gx, gy, gz, mu, softness, limit_stiffness, torque_gain */
int ilqr_hip_plant_set_model(ilqr_hip_ctx* ctx, int contact_mode, int joint_limits);
int ilqr_hip_plant_set_params(ilqr_hip_ctx* ctx, const double* params /*[n_sets][7]*/, int n_sets);
int ilqr_hip_plant_clear_params(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_num_param_sets(const ilqr_hip_ctx* ctx);
int ilqr_hip_plant_get_params(ilqr_hip_ctx* ctx, double* params /*[B][7]*/);
/* ---- sustained external wrench on the pelvis, one per rollout: the push of a robustness sweep.  The reference's plant, mj_step, applies
   xfrc_applied in every substep; its main loop never sets it, so this is a capability of the plant and has no parity row.  Plant only:
   rollout, line search, Jacobians and warm-start tail keep the solver's model -- the push is a disturbance the controller does not know.
   One record of ILQR_PLANT_WRENCH doubles per set:
     0..2  force F, world frame, N          3..5  torque T, world frame, N m
     6..8  point of application r, pelvis frame, m: r = 0 is the origin of the pelvis frame, r = the pelvis inertial offset
           (ilqr_hip_pelvis_inertial_offset) is MuJoCo's xfrc_applied
     9, 10 first, end: the record acts in every substep of plant interval i with first <= i < end, intervals counted from 0 at
           ilqr_hip_plant_reset (ilqr_hip_plant_intervals); integers stored as doubles, end may be +inf
   Per substep, with R0 the pelvis rotation of the state the substep starts from, the generalized force on the free joint is
   Wg = [F ; R0^T T + r x (R0^T F)], conjugate to qvel[0:6] (world linear, body angular).  In the articulated-body recursion it is one term
   of the pelvis solve, IA0 a0 = f - p0, in every pass that solves the pelvis; stance rows and joint-limit rows act on that free solve as
   they do without it, in all six step kinds.
   plant_set_wrench: n_sets = 1 or the batch, else ILQR_ERR_ARG; ILQR_ERR_ARG also for a null pointer, a non-finite entry other than
   end = +inf, a non-integral or negative first / end, or end < first (all checked before the handle is touched).  The table is a device
   buffer of 128-byte records owned by the handle; the call uploads it and synchronises the handle's stream.  It survives
   ilqr_hip_plant_reset and ilqr_hip_plant_configure.  While a table is installed ilqr_hip_plant_advance / _follow launch the wrench family
   of the plant kernel (k_plant_follow_w; an advance is that kernel over one interval) and then the score kernels as before: ring, score,
   alive, kick and the non-finite guards behave as without it, the reported control stays the law's output, a parameter table keeps
   acting.  A wrench that makes a rollout's state non-finite freezes that rollout like any other cause.
   plant_clear_wrench: frees it; the plant calls then launch exactly what they launch without it.
   plant_num_wrench_sets: 0 without a table, else n_sets; -1 for a null handle.
   plant_get_wrench: wrench[B][11], the record of each rollout (zeros without a table).
   plant_intervals: plant intervals run since the last ilqr_hip_plant_reset -- ilqr_hip_plant_advance adds 1, ilqr_hip_plant_follow adds
   count; a counter of its own on the host (the history cursor only counts while a ring exists, and ilqr_hip_plant_set_history does not
   touch this one).  -1 for a null handle.
   step_wrench: ilqr_hip_step_stance with one wrench (entries 0..8: F, T, r) per item, at the handle's dt, contact mode, friction,
   softness and joint-limit options; always the two-lane step.  ILQR_ERR_ARG for a null pointer, count <= 0 or a non-finite entry;
   ILQR_ERR_UNSUPPORTED as ilqr_hip_step_stance under an absent kernel family.
   pelvis_inertial_offset: r[3] = the pelvis body's centre of mass in the pelvis frame (h1.xml inertial pos); host only, no GPU. */
#define ILQR_PLANT_WRENCH 11   /* Fx, Fy, Fz, Tx, Ty, Tz, rx, ry, rz, first, end */
int ilqr_hip_plant_set_wrench(ilqr_hip_ctx* ctx, const double* wrench /*[n_sets][11]*/, int n_sets);
int ilqr_hip_plant_clear_wrench(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_num_wrench_sets(const ilqr_hip_ctx* ctx);
int ilqr_hip_plant_get_wrench(ilqr_hip_ctx* ctx, double* wrench /*[B][11]*/);
long ilqr_hip_plant_intervals(const ilqr_hip_ctx* ctx);
int ilqr_hip_step_wrench(ilqr_hip_ctx* ctx, int count, const double* x, const double* u, int stance_left, int stance_right, const double* wrench /*[count][9]*/, double* x_next);
void ilqr_hip_pelvis_inertial_offset(double r[3]);
/* ---- rigid payload fixed to the pelvis, one per rollout: a plant whose mass distribution is not the solver's -- the robot carries a load
   it did not plan for.  Plant only: rollout, line search, Jacobians, warm-start tail, ilqr_hip_gravity_compensation and the score's
   capture-point centre of mass keep the solver's model.  No reference counterpart (its plant and its solver share one model file).
   One record of ILQR_PLANT_PAYLOAD doubles per set:
     0     mass m, kg                        1..3  centre of mass c, pelvis frame, m (a backpack at torso height: c ~ (-0.1, 0, 0.3))
     4..9  Ixx, Iyy, Izz, Ixy, Ixz, Iyz of the rotational inertia Ic about the payload's own centre of mass, pelvis axes, kg m^2
   The pelvis is the root of the articulated-body recursion, so the payload's spatial inertia about the pelvis origin,
   dI = [[Ic + m (|c|^2 E - c c^T), m [c]x], [-m [c]x, m E]] (angular, then linear), joins the pelvis' own in every substep: in its
   articulated inertia and in its velocity-product force.  Gravity needs no term (the recursion works in the frame that accelerates with
   -g); stance rows, joint-limit rows and the wrench's pelvis solve all read the loaded pelvis, in all six step kinds.  Permanent from set
   to clear: no window.
   plant_set_payload: n_sets = 1 or the batch, else ILQR_ERR_ARG; ILQR_ERR_ARG also for a null pointer, a non-finite entry, m < 0 or an Ic
   that is not positive semidefinite (its seven principal minors >= 0 up to rounding), all checked before the handle is touched.  The table
   is a device buffer of 128-byte records owned by the handle; the call uploads it and synchronises the handle's stream.  It survives
   ilqr_hip_plant_reset and ilqr_hip_plant_configure.  While it is installed ilqr_hip_plant_advance / _follow launch the payload family of
   the plant kernel (k_plant_follow_m of the module libilqr_hip_payload.so, opened from the library's directory on first use -- missing:
   ILQR_ERR_UNSUPPORTED with the path in ilqr_hip_last_error; an advance is that kernel over one interval) and then the score kernels as
   before.  The family carries parameter record, wrench and payload together: ring, score, alive, kick, the non-finite guards, the reported
   control, a parameter table and a wrench table with its window behave as without the payload.
   plant_clear_payload: frees it; the plant calls then launch exactly what they launch without it.
   plant_num_payload_sets: 0 without a table, else n_sets; -1 for a null handle.
   plant_get_payload: payload[B][10], the record of each rollout (zeros without a table).
   step_payload: ilqr_hip_step_wrench with one payload record per item as well; wrench may be NULL (none).  ILQR_ERR_ARG for a null
   x / u / payload / x_next, count <= 0 or a record that plant_set_payload would refuse; ILQR_ERR_UNSUPPORTED as ilqr_hip_step_wrench. */
#define ILQR_PLANT_PAYLOAD 10   /* m, cx, cy, cz, Ixx, Iyy, Izz, Ixy, Ixz, Iyz */
int ilqr_hip_plant_set_payload(ilqr_hip_ctx* ctx, const double* payload /*[n_sets][10]*/, int n_sets);
int ilqr_hip_plant_clear_payload(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_num_payload_sets(const ilqr_hip_ctx* ctx);
int ilqr_hip_plant_get_payload(ilqr_hip_ctx* ctx, double* payload /*[B][10]*/);
int ilqr_hip_step_payload(ilqr_hip_ctx* ctx, int count, const double* x, const double* u, int stance_left, int stance_right, const double* wrench /*[count][9], NULL: none*/,
                          const double* payload /*[count][10]*/, double* x_next);
/* ---- noisy and biased state observation, one model per rollout: a controller that is told a MEASUREMENT of the plant's state, as
   MPC::stepOnce(x_measured, ...) is on a robot -- encoder noise, IMU orientation and rate noise, a drifting pelvis position.  Two places
   read the plant's state for the controller, the warm starts (x0 of the solve) and the plant kernels' control law; under a table both
   read the same measurement x [+] delta.  The physics, the ring, alive and the score stay on the true state; a pending kick is applied
   to the true state in front of the law, as before.
   One record of ILQR_PLANT_OBSERVATION doubles per set: bias[50], then sigma[50], in the tangent order of the Jacobians --
     dp[3] pelvis position (world)   dphi[3] orientation, a rotation vector in the body frame   dq[19] joint positions
     dv[3] linear velocity (world)   domega[3] angular velocity (body)                          dqdot[19] joint velocities
   The error of rollout b in plant interval i (counted as ilqr_hip_plant_intervals counts, from the last ilqr_hip_plant_reset) is
   e = bias + sigma o z, z[50] standard normals, laid out as a state-shaped row delta[51]: delta.p = e.dp, delta.quat = (cos(t/2),
   sin(t/2)/t e.dphi) with t = |e.dphi| (exactly (1, 0, 0, 0) for t == 0), the 44 remaining entries e itself.  The measured state
   x [+] delta is p + delta.p, quat (x) delta.quat (Hamilton product, wxyz, not renormalised), every other entry added.
   The normals come from Philox4x32-10, a counter-based generator, so they depend on (seed, rollout stream, interval) alone -- not on
   launch shape, batch split or call grouping: key (seed & 0xffffffff, seed >> 32), counter (s & 0xffffffff, s >> 32, i & 0xffffffff, k)
   with s = stream0 + b and the block k = 0..24; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85.  With the
   output words w0..w3: u1 = (((w0 << 32 | w1) >> 11) + 0.5) 2^-53, u2 likewise from w2, w3, r = sqrt(-2 log u1), z[2k] = r cos(2 pi u2),
   z[2k + 1] = r sin(2 pi u2), 2 pi the double constant, multiplied once.  Draws are made whatever sigma is: a rollout's stream never
   depends on its record.  stream0 is the first GLOBAL rollout index of a shard, so a sharded batch draws what the global batch draws.
   delta(i) is drawn once per plant interval and held over it: the warm start taken while ilqr_hip_plant_intervals == i, the control law
   of interval i (in every substep at feedback mode 1), and inside ilqr_hip_plant_follow(k0, m) interval i + j with knot k0 + j.
   plant_set_observation: n_sets = 1 (one record that every rollout reads; the streams still differ) or the batch, else ILQR_ERR_ARG;
   ILQR_ERR_ARG also for a null pointer, a non-finite entry or a negative sigma, all checked before the handle is touched.  The table and a
   buffer of N x B x 51 error rows are owned by the handle; the call uploads and synchronises the handle's stream.  It survives
   ilqr_hip_plant_reset and ilqr_hip_plant_configure.  While it is installed ilqr_hip_plant_advance / _follow launch the draw of the call's
   intervals and the observation family of the plant kernel (k_observation_draw, k_plant_follow_o of the module libilqr_hip_observe.so,
   opened from the library's directory on first use -- missing: ILQR_ERR_UNSUPPORTED with the path in ilqr_hip_last_error; an advance is
   that kernel over one interval), which carries parameter record, wrench and payload as the payload family does, each table present or
   not; ilqr_hip_initialize_warm_from_plant[_shifted] write x0 with a one-row draw and k_observe_apply in the place of the device copy.
   plant_clear_observation: frees the table; the plant calls and warm starts then launch exactly what they launch without it.
   plant_num_observation_sets: 0 without a table, else n_sets; -1 for a null handle.
   plant_get_observation: obs[B][100], the record of each rollout (zeros without a table); seed / stream0 (each may be NULL; 0 without).
   plant_observation_errors: delta[count][B][51] of the intervals interval0 .. interval0 + count - 1, a pure function of table, seed,
   stream0 and interval; 1 <= count <= N and interval0 >= 0, else ILQR_ERR_ARG; ILQR_ERR_STATE without a table.
   plant_get_observed: x_obs[B][51] = plant state [+] delta(ilqr_hip_plant_intervals), what a warm start would hand the solve now; the
   plant state itself without a table. */
#define ILQR_PLANT_OBSERVATION 100   /* bias[50], sigma[50] */
int ilqr_hip_plant_set_observation(ilqr_hip_ctx* ctx, const double* obs /*[n_sets][100]*/, int n_sets, unsigned long long seed, unsigned long long stream0);
int ilqr_hip_plant_clear_observation(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_num_observation_sets(const ilqr_hip_ctx* ctx);
int ilqr_hip_plant_get_observation(ilqr_hip_ctx* ctx, double* obs /*[B][100]*/, unsigned long long* seed, unsigned long long* stream0);
int ilqr_hip_plant_observation_errors(ilqr_hip_ctx* ctx, long interval0, int count, double* delta /*[count][B][51]*/);
int ilqr_hip_plant_get_observed(ilqr_hip_ctx* ctx, double* x_obs /*[B][51]*/);
/* ---- actuator delay, lag and torque noise, one model per rollout: between the control law and the joints.  In the reference's loop
   (main/humanoid_mpc.cpp:122-190) the torque the law computes acts in the same substep, exactly; on a robot the solve takes time, the motor
   drivers have a bandwidth and the delivered torque ripples.  One record of ILQR_PLANT_ACTUATOR doubles per set:
     delay      an integer stored as a double, in plant SUBSTEPS, 0 <= delay <= ILQR_PLANT_ACTUATOR_MAX_DELAY
     tau[19]    time constant of a first-order lag per joint, seconds, >= 0; 0: no lag
     sigma[19]  torque noise per joint, N m, >= 0
   With n the plant substeps run since the actuator's state was last primed and h = dt / substeps:
     c_n     the COMMAND: the control law's output for substep n behind the non-finite guard (main:162-165: a command with a non-finite
             entry is zero) -- constant over an interval at feedback mode 0, new in every substep at mode 1.  It stays what the plant
             REPORTS: ilqr_hip_plant_get_control, the ring, hence the score.
     a_n   = c_{n - delay}: a delay line of MAX_DELAY + 1 slots of 19 doubles per rollout, slot n % 9 written, slot (n - delay) % 9 read.
     y_n   = y_{n-1} + beta o (a_n - y_{n-1}), beta_i = -expm1(-h / tau_i), the exact discretisation of tau y' = a - y (as MuJoCo's
             `filterexact` activation dynamics is documented; the reference's h1.xml motors have none, so this is an option, no parity
             claim).  The host computes beta in double when the table is installed and whenever ilqr_hip_plant_configure changes
             `substeps`; the kernel reads it, and the product beta_i (a_i - y_i) is rounded on its own (no fused multiply-add).  For
             tau_i == 0, y_i = a_i by SELECTION, not by arithmetic; its beta is never computed (the getter returns 1).
     t_n   = y_n + sigma o z(i): z(i) 19 standard normals drawn once per plant INTERVAL i (ilqr_hip_plant_intervals) and held over it, as
             the observation error is; sigma_i z_i is rounded on its own; sigma_i == 0 adds nothing, again by selection.
     t_n goes where the control goes without a table: through the torque gain of the parameter record and then the step's clamp.
   So a record of zeros is no table, bit for bit.
   Priming: ilqr_hip_plant_reset, ilqr_hip_plant_configure and ilqr_hip_plant_set_actuator set n = 0; the first substep after that writes
   c_0 into every slot and into y -- the joint was already holding that torque, a standing rollout does not drop for `delay` substeps.
   The delay line and y persist across the plant calls.  A rollout that is frozen (non-finite) is handled as without a table.
   The normals come from the generator of the observation model above, Philox4x32-10 with key (seed lo, seed hi) and counter
   (s lo, s hi, i lo, k), s = stream0 + b, under a seed and stream0 of this call's own, in the blocks k = 32..41: block 32 + q gives the
   normals of joints 2q and 2q + 1 as the observation's block gives z[2k], z[2k + 1]; the second normal of block 41 is discarded.  (The
   observation uses k = 0..24: equal seeds do not correlate the two.)  Draws are made whatever sigma is.
   plant_set_actuator: n_sets = 1 (one record that every rollout reads; the streams still differ) or the batch, else ILQR_ERR_ARG;
   ILQR_ERR_ARG also for a null pointer, a non-finite entry, a negative tau or sigma, or a delay that is not an integer in 0..8, all checked
   before the handle is touched.  The table, the derived beta rows, the actuator's state and a buffer of N x B x 19 normals are owned by the
   handle; the call uploads and synchronises the handle's stream.  The table survives ilqr_hip_plant_reset and ilqr_hip_plant_configure.
   While it is installed ilqr_hip_plant_advance / _follow launch the draw of the call's intervals and the actuator family of the plant
   kernel (k_actuator_draw, k_plant_follow_a of the module libilqr_hip_actuator.so, opened from the library's directory on first use --
   missing: ILQR_ERR_UNSUPPORTED with the path in ilqr_hip_last_error, never a fall-back; an advance is that kernel over one interval),
   which carries parameter record, wrench, payload and observation as the observation family does, each table present or not.
   plant_clear_actuator: frees the table; the plant calls then launch exactly what they launch without it.
   plant_num_actuator_sets: 0 without a table, else n_sets; -1 for a null handle.
   plant_get_actuator: act[B][39], the record of each rollout (zeros without a table); seed / stream0 (each may be NULL; 0 without).
   plant_get_actuator_blend: beta[B][19] as the kernel reads it, to the bit; ILQR_ERR_STATE without a table.
   plant_actuator_draws: z[count][B][19] of the intervals interval0 .. interval0 + count - 1, a pure function of seed, stream0 and
   interval; 1 <= count <= N and interval0 >= 0, else ILQR_ERR_ARG; ILQR_ERR_STATE without a table.
   plant_get_applied: tau[B][19] = t_n of the last substep run under the table, in front of the torque gain and the clamp (zeros before
   the first); without a table the reported control. */
#define ILQR_PLANT_ACTUATOR 39            /* delay, tau[19], sigma[19] */
#define ILQR_PLANT_ACTUATOR_MAX_DELAY 8
int ilqr_hip_plant_set_actuator(ilqr_hip_ctx* ctx, const double* act /*[n_sets][39]*/, int n_sets, unsigned long long seed, unsigned long long stream0);
int ilqr_hip_plant_clear_actuator(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_num_actuator_sets(const ilqr_hip_ctx* ctx);
int ilqr_hip_plant_get_actuator(ilqr_hip_ctx* ctx, double* act /*[B][39]*/, unsigned long long* seed, unsigned long long* stream0);
int ilqr_hip_plant_get_actuator_blend(ilqr_hip_ctx* ctx, double* beta /*[B][19]*/);
int ilqr_hip_plant_actuator_draws(ilqr_hip_ctx* ctx, long interval0, int count, double* z /*[count][B][19]*/);
int ilqr_hip_plant_get_applied(ilqr_hip_ctx* ctx, double* tau /*[B][19]*/);
/* ---- joint gain, torque range, damping and armature, one set per rollout: a joint that is not the model's.  The model's joints have
   armature 0.1, damping 1 and the torque ranges of h1.xml, and the parameter record has ONE torque gain for all 19 motors; rotor inertia
   behind the gearbox and joint friction are the worst-known numbers of a real robot, and a weak, saturating or dead motor is a fault of
   ONE joint.  One record of ILQR_PLANT_JOINTS doubles per set, the joints in the order of u:
     gain[19]     g_i, per-joint torque gain, >= 0
     scale[19]    s_i, scale on the model's torque range [lo_i, hi_i], >= 0; 0: a dead motor
     damping[19]  d_i, N m s / rad, >= 0
     armature[19] a_i, kg m^2, >= 0
   In every plant substep of length h_s, with G the scalar gain of the parameter record (1 without one):
     tau_i = clamp(G g_i u_i, s_i lo_i, s_i hi_i) - d_i v_i
     (M + diag(a) + h_s diag(d)) qacc = tau - bias + J^T lambda + E^T nu      (MuJoCo's Euler step with implicit joint damping)
   g_i acts in front of the clamp, s_i on the clamp.  Everything else of the step is unchanged in all six step kinds: stance rows, unilateral
   and Coulomb decisions, the joint-limit rows' lock decision and second pass (a stopped hinge keeps its prescribed acceleration: nothing of
   the record reaches it), wrench and payload.  The nominal record g = s = d = 1, a = 0.1 is the model: a table whose every record is
   nominal is no table, bit for bit (the plant calls launch what they launch without it).  The plant keeps REPORTING the commanded torque
   (ilqr_hip_plant_get_control, the ring, the score, ilqr_hip_plant_get_applied behind the actuator): the record acts inside the step,
   behind all of them, and the solver does not know of it.
   plant_set_joints: n_sets = 1 (one record that every rollout reads) or the batch, else ILQR_ERR_ARG; ILQR_ERR_ARG also for a non-finite or
   negative entry, checked before the handle is touched.  joints NULL with n_sets 0 clears the table: the plant calls then launch exactly
   what they launch without it.  The table is owned by the handle; the call uploads and synchronises the handle's stream.  It survives
   ilqr_hip_plant_reset and ilqr_hip_plant_configure.  While it is installed ilqr_hip_plant_advance / _follow launch the joints family of
   the plant kernel (k_plant_follow_j of the module libilqr_hip_joints.so, opened from the library's directory on first use -- missing:
   ILQR_ERR_UNSUPPORTED with the path in ilqr_hip_last_error, never a fall-back; an advance is that kernel over one interval), which
   carries parameter record, wrench, payload, observation and actuator as the actuator family does, each table present or not.
   plant_get_joints: joints[B][76], the record of each rollout (the nominal record without a table).
   step_joints: x_next[i] = f(x[i], u[i]) under joints[i], and under wrench[i] (F, T, r) and payload[i] where given, with the handle's
   dynamics parameters and step size, as ilqr_hip_step_payload. */
#define ILQR_PLANT_JOINTS 76   /* gain[19], scale[19], damping[19], armature[19] */
int ilqr_hip_plant_set_joints(ilqr_hip_ctx* ctx, const double* joints /*[n_sets][76]; NULL with n_sets 0: clear*/, int n_sets);
int ilqr_hip_plant_get_joints(ilqr_hip_ctx* ctx, double* joints /*[B][76]*/);
int ilqr_hip_step_joints(ilqr_hip_ctx* ctx, int count, const double* x, const double* u, int stance_left, int stance_right, const double* wrench /*[count][9], NULL: none*/,
                         const double* payload /*[count][10], NULL: none*/, const double* joints /*[count][76]*/, double* x_next);
/* ---- a floor of its own height under each foot, one record per rollout: a ground that is not the solver's.  With the stance source
   GEOMETRY the plant's feet land and lift against z = 0, exactly where the solver's model expects them to; an unexpected ground height -- a
   touchdown a few centimetres early or late, a kerb, a floor that gives way -- is the standard disturbance of a walking controller.  One
   record of ILQR_PLANT_TERRAIN doubles per set:
     z_left, z_right   floor height under the left / right foot, m; finite
     edge_x            m; the height holds for a foot only while the world x of its ankle-link origin is >= edge_x; finite, or -inf: everywhere
     first, end        the record acts in the plant intervals first <= i < end, counted as ilqr_hip_plant_intervals counts them and checked
                       as the wrench's window is (non-negative integers, first <= end, end may be +inf)
   The rule, per plant substep, on the state the substep starts from: foot f is in stance iff clearance_f(qpos) < floor_f, where
   floor_f = z_f while the window is open and ankle_x_f >= edge_x, else 0, and clearance_f is what ilqr_hip_foot_clearance returns.  The
   contact step itself is unchanged: the stance rows weld a touching foot where it is, at whatever height, and release, the Coulomb limit,
   kinetic friction and joint-limit rows act on these flags as on any flags.  What changes is the flags the plant reports
   (ilqr_hip_plant_get_stance, the ring's states follow from them); the score's capture-point term keeps reading the schedule and the solver
   knows nothing of the record.  A record with z = 0, or whose window is shut, is the solver's ground.
   plant_set_terrain: n_sets = 1 (one record that every rollout reads) or the batch, else ILQR_ERR_ARG; ILQR_ERR_ARG also for a value outside
   the ranges above, checked before the handle is touched.  The table is owned by the handle; the call uploads and synchronises the handle's
   stream.  It survives ilqr_hip_plant_reset and ilqr_hip_plant_configure; plant_clear_terrain removes it.  While it is installed
   ilqr_hip_plant_advance / _follow launch the terrain family of the plant kernel (k_plant_follow_t of the module libilqr_hip_terrain.so,
   opened from the library's directory on first use -- missing: ILQR_ERR_UNSUPPORTED with the path in ilqr_hip_last_error, never a fall-back;
   an advance is that kernel over one interval), which carries parameter record, wrench, payload, observation, actuator and joints as the
   joints family does, each table present or not.  A floor nobody consults is refused, not ignored: while the table is installed a plant call
   whose contact source is ILQR_STANCE_SCHEDULE, or whose effective contact mode (ilqr_hip_plant_set_model, else the solver's) is 0 or 1,
   returns ILQR_ERR_UNSUPPORTED before anything is launched.
   plant_get_terrain: terrain[B][5], the record of each rollout (without a table: heights 0, edge -inf, the empty window [0, 0)).
   step_terrain: x_next[i] = f(x[i], u[i]) under the flags the rule gives x[i] on the floor terrain[i] = z_left, z_right, edge_x (no window:
   always open), decided on the device, with the handle's dynamics parameters and step size; the flags in stance_out[i].  Contact mode 0 or
   1: ILQR_ERR_UNSUPPORTED.  Always the two-lane step.
   terrain_stance: the rule itself on the host, no GPU and no handle: stance[2] of qpos[26] under terrain[5] in plant interval `interval`,
   and the floor each foot was held against in floor[2] where it is not NULL. */
#define ILQR_PLANT_TERRAIN 5   /* z_left, z_right, edge_x, first, end */
int ilqr_hip_plant_set_terrain(ilqr_hip_ctx* ctx, const double* terrain /*[n_sets][5]*/, int n_sets);
int ilqr_hip_plant_clear_terrain(ilqr_hip_ctx* ctx);
int ilqr_hip_plant_num_terrain_sets(const ilqr_hip_ctx* ctx);   /* 0: no table */
int ilqr_hip_plant_get_terrain(ilqr_hip_ctx* ctx, double* terrain /*[B][5]*/);
int ilqr_hip_step_terrain(ilqr_hip_ctx* ctx, int count, const double* x, const double* u, const double* terrain /*[count][3]: z_left, z_right, edge_x*/, double* x_next,
                          int* stance_out /*[count][2]*/);
int ilqr_hip_terrain_stance(const double* qpos /*26*/, const double* terrain /*5*/, long interval, int* stance /*2*/, double* floor /*2, NULL: not wanted*/);

/* ---- reference windows from a track on the device.  The reference cuts the window of every MPC step out of RobotUtils' full-length
   arrays on the host (MPC::extractReferenceWindow, src/ilqr/mpc.cpp:163-166) and hands it to the solver; with one window per rollout
   that is the largest host crossing of a resident step.  Here the full-length arrays are uploaded ONCE, one start row per rollout lives
   on the device, and one kernel per step writes every window into the buffers the three reference setters fill.
   set_reference_track: the arrays of RobotUtils::loadReferences / loadContactSchedule (src/common/robot_utils.cpp:281-492) --
   x_ref_full_, u_ref_full_ (NULL: zeros), com_ref_full_, ee_ref_full_ (left, right ankle), com_vel_ref_full_ (NULL: zeros) with `rows`
   rows each, contact_schedule_ with `contact_rows` rows, which may differ from `rows` (NULL: no table).  The handle owns a device copy:
   one upload, one synchronisation of the handle's stream.  rows < 1, contact_rows < 0 or a null required pointer: ILQR_ERR_ARG.  A second
   call replaces the track.  The start rows become one shared start of 0.
   clear_reference_track: frees the track; the windows last written stay installed.
   reference_track_rows: 0 without a track, else its rows; -1 for a null handle. */
int ilqr_hip_set_reference_track(ilqr_hip_ctx* ctx, int rows, const double* x_ref /*[rows][51]*/, const double* u_ref /*[rows][19], NULL: zeros*/,
                                 const double* com_ref /*[rows][3]*/, const double* ee_ref /*[rows][2][3]*/, const double* com_vel_ref /*[rows][3], NULL: zeros*/,
                                 const int* contact /*[contact_rows][2], NULL: none*/, int contact_rows);
int ilqr_hip_clear_reference_track(ilqr_hip_ctx* ctx);
int ilqr_hip_reference_track_rows(const ilqr_hip_ctx* ctx);
/* One start row per set, start[n_sets], n_sets 1 or the batch (else ILQR_ERR_ARG); every start >= 0 (else ILQR_ERR_ARG).  Kept on the
   device; their maximum is kept on the host for the range check of the window call.  Synchronises the handle's stream.  ILQR_ERR_STATE
   without a track. */
int ilqr_hip_set_track_starts(ilqr_hip_ctx* ctx, const int* start, int n_sets);
/* The windows of MPC step `step` >= 0 (else ILQR_ERR_ARG), for every set b with s = start[b] + step (one shared start: one window, read
   by every rollout), t = 0 .. N:
     x_ref, u_ref (t < N), com_ref     row min(s + t, rows - 1)     RobotUtils::getReferenceWindow's end clamp, robot_utils.cpp:422-443
     ee_ref, com_vel_ref, stance       row r = (follow_schedule ? s : 0) + t: the horizon-local index the reference's solver uses
                                       (ilqr.cpp:703,729-734,767-791), or the advancing one
     stance flag                       contact[r][foot] == 1; 1 where r >= contact_rows or no table was given (isStance, :494-504)
   getEEReference / getCoMVelReference have no clamp and throw past the end (:525-549): ILQR_ERR_ARG when the largest r of any set would
   reach `rows`, checked on the host from the stored maximum start before anything is launched (the kernel clamps every row index it
   forms as well).  ENQUEUES one kernel on the handle's stream: no upload, no synchronisation.  A pure copy: the windows are bit for bit
   what the three reference setters would have uploaded, and afterwards the handle is in the state they leave (set strides, references
   set); a later setter simply overwrites what this wrote.  ILQR_ERR_STATE without a track.  No reference counterpart for the batch:
   the reference holds one trajectory. */
int ilqr_hip_window_from_track(ilqr_hip_ctx* ctx, int step, int follow_schedule);
/* The reference windows the solver currently reads, whoever wrote them (a setter or the track), expanded to one per rollout whatever the
   set strides are; every pointer may be NULL.  Synchronises the handle's stream. */
int ilqr_hip_get_reference_windows(ilqr_hip_ctx* ctx, double* x_ref /*[B][N+1][51]*/, double* u_ref /*[B][N][19]*/, double* com_ref /*[B][N+1][3]*/,
                                   double* ee_ref /*[B][N+1][2][3]*/, double* com_vel_ref /*[B][N+1][3]*/, int* stance /*[B][N+1][2]*/);

/* per-stage device time of the last solve in milliseconds, keyed like the reference's profiler
   (src/ilqr/ilqr.cpp:537-639): 0 computeCost/rollout, 1 linearization, 2 costQuadratics, 3 backwardPass,
   4 lineSearch, 5 control, 6 backwardPass (lambda-retry launch), 7 lineSearch (lambda-retry launch);
   requires ilqr_hip_enable_profiling(ctx, 1) before the solve */
int ilqr_hip_enable_profiling(ilqr_hip_ctx* ctx, int on);
/* Restrict the event pairs to the stages whose bit (stage index as above) is set in `mask` (default 0xFF: all).  Every timed
   launch costs two event records on its stream: all eight stages together add 1.3 ms to a 95 ms solve at B = 4096. */
int ilqr_hip_set_profiled_stages(ilqr_hip_ctx* ctx, unsigned mask);
/* Diagnostic of the concurrent nominal re-rollout (with ilqr_hip_set_reroll_nominal, iterations >= 1 of a solve roll the nominal
   trajectory beside the linearisation, ilqr.cpp:563 vs :576): number of trajectory elements of the last solve in which the re-rolled
   trajectory differed bit-wise from the one the linearisation saw.  0 means the launch order is equivalent to the reference's -- and
   that the default, which does not re-roll, computes what the re-roll computes.  0 as well where nothing was re-rolled. */
int ilqr_hip_get_adopt_mismatches(ilqr_hip_ctx* ctx, unsigned long long* count);
/* Nominal re-rollout.  The reference rolls the nominal trajectory out from x0 at the top of every iteration (ilqr.cpp:551,563) and evaluates
   its cost, the line-search baseline.  From iteration 1 on that trajectory is the previous one or the line-search candidate the iteration
   before accepted: a rollout from x0 under the same controls by the same step implementation, which the rollout reproduces bit for bit, and
   whose cost the bookkeeping has stored summed in the same order.  The same holds for iteration 0 of a solve whose trajectory is a cold start
   (ilqr_hip_initialize*) under the dynamics parameters now set, and of rounds >= 2 of an augmented-Lagrangian solve: the cost-only pass at
   the top of every solve and round evaluates the baseline under the weights and multipliers now set.  By default none of these launches
   runs -- the rollout, its knot costs, their sum, the adoption.  A warm-shifted or caller-supplied trajectory, a new x0 (ilqr_hip_solve with
   x0), changed dynamics parameters: iteration 0 rolls out in front of the linearisation, as the reference does.  Every observable of the
   solve is unchanged, bit for bit (GPU test).
   on != 0, or environment ILQR_REUSE_ROLLOUT=0, restores every rollout the reference executes -- the verification mode: beside the
   linearisation into a shadow buffer (0.01 MB per rollout at N = 25, allocated by the first solve that re-rolls) and adopted with
   ilqr_hip_get_adopt_mismatches counting, or in front of it with ILQR_OVERLAP_ROLLOUT=0.  ILQR_REUSE_ROLLOUT=1 / 0 overrides the handle's
   setting (read with the other switches, ilqr_hip_reload_environment).  The cross-check kernel families of the test library whose line
   search and rollout run different step implementations roll out in every iteration whatever the setting.
   bench.py's per-iteration flop budget still charges every iteration a nominal step per knot, as it charges a full linearisation with the
   cache: its rates are algorithmic-equivalent rates.  No reference counterpart: the reference recomputes. */
int ilqr_hip_set_reroll_nominal(ilqr_hip_ctx* ctx, int on);
/* Rollouts the nominal-rollout launches of the last solve were enqueued for: launches x the rollouts of the batch (or slice) each covers,
   all augmented-Lagrangian rounds together; an iteration whose region runs in two groups (ilqr_hip_get_split_iterations) launches once per
   group, each over the batch under the group's flags.  Host-side count, no synchronisation.  By default 0 behind a cold start and batch x 1 behind a warm
   start; batch x iterations enqueued (x rounds) in the verification mode.  -1 for a null handle. */
long long ilqr_hip_get_nominal_rollouts(const ilqr_hip_ctx* ctx);
int ilqr_hip_get_stage_ms(ilqr_hip_ctx* ctx, double* ms /*[8]*/, double* launches /*[8]*/);
/* Iterations whose kernels the last solve enqueued: max_iterations, or fewer when the convergence exit (ilqr.cpp:645-655,
   ilqr_hip_set_options early_exit) is on and every rollout of the batch had left the loop -- the host follows the device-side
   count of active rollouts one iteration behind and stops launching (ilqr_hip_set_early_exit_gate(ctx, 0) turns that off).
   Returns the count, or -1 for a null handle. */
int ilqr_hip_get_iterations_enqueued(const ilqr_hip_ctx* ctx);
/* Iterations of the last solve that ran the lambda retry of ilqr.cpp:619-644 speculatively: while a pass holds at most 512
   rollouts (the whole batch, or -- convergence exit -- the count of rollouts still active the host has seen), the Riccati pass and
   the line search for lambda and for min(10 lambda, 1e-3) run side by side on two streams and the bookkeeping of :619-655 is
   played once with both outcomes known; results (gains, value function, trajectory, lambda, trace) are those of the sequential
   order, one pass of latency sooner.  Counted: the iterations that ENQUEUED the side-by-side passes -- while the host's count (one iteration
   old) is between 512 and 2048 both orders are enqueued and the device takes one by the length of the work list (ILQR_SPEC_DUAL=0: host
   count alone).  Environment ILQR_SPEC=0 keeps the sequential order.  Returns the count, -1 for a null handle. */
int ilqr_hip_get_speculative_iterations(const ilqr_hip_ctx* ctx);
/* Listed side-by-side order (on by default): in a fixed-iteration solve of a batch above ILQR_SPEC_MAX the late iterations' lists are short
   and the chip is nearly empty, yet each iteration is a chain of two latency-bound passes.  From iteration 3 max_iterations / 5 on (environment
   ILQR_SPEC_LIST_FROM moves the start, at least 1) the device then takes, per iteration and by the lengths of its lists, the order that runs
   them side by side: the first pass of the rollouts that accepted a candidate
   in the previous iteration (list chg), their lambda retry speculatively into the twin buffers, and -- on the solve's own buffers -- the retry
   of the rollouts whose two searches of the previous iteration both failed below the lambda cap (list kr: their first pass is skipped and
   fails by construction, so the retry is known before the iteration starts).  Taken while 2 chg_n + kr_n <= ILQR_SPEC_LIST_MAX (environment,
   default 1024 one-wave-per-SIMD slots); both orders are enqueued and the one not taken sees empty lists.  Every observable of the solve is
   that of the sequential order (GPU tests).  Not counted by ilqr_hip_get_speculative_iterations.  Off with on = 0, ILQR_SPEC_LISTS=0 or
   ILQR_SPEC=0 (the parent's launch order exactly), and wherever the lists do not exist: convergence exit, batch slices, forward-difference
   Jacobians, the early-continuation split, ILQR_REPASS=1, ILQR_RELIN=1, ILQR_DEDUP_RETRY=0 and their setters.  The twin buffers (0.33 MB per
   rollout) are allocated by the first solve that can take the order; a failed allocation keeps the sequential order.
   ilqr_hip_get_first_pass_rollouts / _retry_pass_rollouts keep counting the rollouts whose pass ran: chg_n for the first pass and
   chg_n + kr_n for the retry side of an iteration taken in this order. */
int ilqr_hip_set_listed_spec(ilqr_hip_ctx* ctx, int on);
/* Iterations of the last solve in which the device took the listed side-by-side order (read from the per-iteration gate words).
   Synchronises the handle's stream.  -1 for a null handle or a failed read. */
int ilqr_hip_get_listed_spec_iterations(ilqr_hip_ctx* ctx);
/* One code per enqueued iteration of the last solve into out[0 .. max_iterations): returns the count, -1 for a null argument or a failed
   read.  Synchronises the handle's stream. */
enum {
  ILQR_ORDER_SEQUENTIAL = 0,      /* first pass, bookkeeping, lambda retry, bookkeeping */
  ILQR_ORDER_TWIN = 1,            /* both passes side by side for every active rollout (ilqr_hip_get_speculative_iterations) */
  ILQR_ORDER_DUAL_SEQUENTIAL = 2, /* both of the above enqueued, the device took the sequential one */
  ILQR_ORDER_DUAL_TWIN = 3,       /* ... the side-by-side one */
  ILQR_ORDER_LISTED_SPEC = 4      /* listed side by side (above); an iteration that enqueued the pair and took the sequential order reports 0 */
};
int ilqr_hip_get_iteration_orders(ilqr_hip_ctx* ctx, int* out);
/* The two lists iteration `iter` (0 <= iter < max_iterations) of the last solve started from, as the device left them (diagnostics, tests):
   counts[0] rollouts into chg (batch entries; may be NULL) -- those that accepted a candidate in iteration iter - 1 --, counts[1] into kr
   (likewise) -- those whose two searches of iter - 1 failed below the lambda cap.  Disjoint; an active rollout on neither is stuck at the
   cap and runs no pass.  Iteration 0 runs every rollout: both counts 0.  The order within a list is not defined.  Synchronises the handle's
   stream.  ILQR_ERR_STATE when the last solve kept no lists (none yet, batch slices, forward differences, ILQR_RELIN=1). */
int ilqr_hip_get_iteration_lists(ilqr_hip_ctx* ctx, int iter, int* chg, int* kr, int* counts);
/* Iterations of the last solve whose concurrent region (linearisation, cost quadratics, nominal re-rollout: ilqr.cpp:551-588) ran in
   two groups: the rollouts whose first line search of the previous iteration accepted a step start right behind that iteration's first
   bookkeeping pass, beside the lambda retry (:619-644) of the others, which follow behind the second; both meet at the backward pass.
   Bit-identical results.  On by default when the convergence exit is enabled (where it pays; with a fixed iteration count nearly every
   rollout retries and the early group is small); environment ILQR_SPLIT=0 / 1 forces it off / on.  Returns the count, -1 for a null handle. */
int ilqr_hip_get_split_iterations(const ilqr_hip_ctx* ctx);
/* Linearisation cache.  A rollout whose two line searches of an iteration both fail (ilqr.cpp:640-655, the failing branch) keeps its
   nominal trajectory bit for bit, and A_t, B_t, lx, lu, lxx, luu are functions of that trajectory and of the problem data alone -- not
   of lambda: the next iteration's linearisation (:576) and cost quadratics (:588) would rewrite the values the buffers hold.  By default
   they run, from iteration 1 on, only for the rollouts that accepted a candidate in the previous iteration (a list k_control builds on the
   device); iteration 0 of every solve takes every rollout.  Every pass, decision, trace entry and lambda update stays where it is and
   every observable of the solve is unchanged, bit for bit (GPU test).  on != 0 restores the full pass in every iteration (comparison,
   profiling); environment ILQR_RELIN=1 / 0 overrides the handle's setting (read with the other switches, ilqr_hip_reload_environment).
   The full pass is also what runs, whatever the setting, with forward-difference Jacobians, with batch slices and in the stage API.
   bench.py's whole_iteration_frac* figures charge every iteration a full linearisation and cost-quadratics pass: with the cache they are
   algorithmic-equivalent rates.  No reference counterpart: the reference recomputes. */
int ilqr_hip_set_relinearize_unchanged(ilqr_hip_ctx* ctx, int on);
/* Sum over the iterations of the last solve of the number of rollouts whose linearisation and cost quadratics ran: batch x iterations
   with ilqr_hip_set_relinearize_unchanged set and a fixed iteration count (with the convergence exit: the rollouts still active, per
   iteration), the executed count with the cache.  Synchronises the handle's stream.  0 before the first solve and after
   ilqr_hip_set_max_iterations changed the count, -1 for a null handle or a failed read.  No reference counterpart: the reference
   recomputes. */
long long ilqr_hip_get_linearized_rollouts(ilqr_hip_ctx* ctx);
/* First-pass skip.  The same rollout -- both line searches of iteration i failed -- also enters iteration i + 1 with the lambda of the
   retry of i (the reference `continue`s with the raised lambda, ilqr.cpp:619-646) and with a baseline cost that is the cost of the same
   trajectory: the first backward pass (:601), line search (:616) and candidate costs of i + 1 would recompute, from identical inputs, the
   gains, value function, candidates and candidate costs that its last executed pass left in the buffers, and fail again.  By default, in
   the sequential order of a solve (the order of large batches with a fixed iteration count), the first pass of iterations >= 1 runs only
   for the rollouts that accepted a candidate in the previous iteration -- the list of the linearisation cache; the line search takes the
   one-rollout-per-wave kernel once that list holds at most 1024 rollouts (decided on the device; environment ILQR_LS_LIST_MAX moves the
   threshold).  The bookkeeping (:619-620) still runs for every active rollout, from the costs that pass left.
   Invariant: every decision, trace entry, lambda update and every observable of the solve is unchanged, bit for bit (GPU test); nothing
   the bookkeeping reads is written by a skipped launch.  on != 0, or environment ILQR_REPASS=1, restores the full first pass in every
   iteration (comparison, profiling: the per-launch figures of bench.py --full then are full-batch figures again).  The full pass is also
   what runs, whatever the setting, in the side-by-side orders (ilqr_hip_get_speculative_iterations), with the early-continuation groups
   (ilqr_hip_get_split_iterations), with forward-difference Jacobians and with batch slices.  Independent of
   ilqr_hip_set_relinearize_unchanged and ilqr_hip_set_dedup_saturated_retry; with the latter on (the default), a rollout stuck at the
   lambda cap costs neither pass.  No reference counterpart: the reference recomputes. */
int ilqr_hip_set_repeat_first_pass(ilqr_hip_ctx* ctx, int on);
/* Sum over the iterations of the last solve of the number of rollouts whose first pass ran: the batch for iteration 0, the rollouts
   active in the iteration where the full pass ran (the batch without the convergence exit), the list's length where it was skipped.
   Synchronises the handle's stream.  0 before the first solve and after ilqr_hip_set_max_iterations changed the count, -1 for a null
   handle or a failed read. */
long long ilqr_hip_get_first_pass_rollouts(ilqr_hip_ctx* ctx);

/* ---- solve groups: several starts per problem, the best one adopted on the device.  iLQR is a local method: after a push, a late touchdown
   or a bound that has just become active the shifted previous solution can be a poor start.  A handle's batch can be cut into M = B / G
   groups of G consecutive rollouts; a group stands for ONE problem (one robot) solved from G starting trajectories.  The members of a group
   share x0, references, schedule and plant tables: that is the caller's business (scenario.repeat_for_groups repeats any per-rollout table
   member-minor), and so are per-rollout weight sets and bound tables inside a group -- nothing is refused for them; a caller whose members
   differ in their cost passes a key of its own to group_select.  Member 0 of every group is the incumbent: it is never perturbed, so before
   the selection it is exactly the plain solve, and a group never does worse per solve than the handle without groups.  One step is
       warm start -> group_perturb -> solve -> group_select -> group_adopt -> plant_advance / plant_follow
   and the three group calls are enqueued on the handle's stream and never synchronise.  Their kernels (k_group_perturb, k_group_select,
   k_group_adopt) live in the module libilqr_hip_groups.so, opened from the library's directory by the first set_groups with G > 1 --
   missing: ILQR_ERR_UNSUPPORTED with the path in ilqr_hip_last_error, the only refusal of this family.  No reference counterpart.
   set_groups: G >= 1 and G divides the batch, else ILQR_ERR_ARG.  G = 1 switches the feature off and frees its buffers; G > 1 allocates
   winner[M] and group_rec[M][4].  Launches no kernel; removes an installed perturbation and forgets the last selection.
   num_groups: M, 0 while the feature is off, -1 for a null handle.
   group_set_perturbation: sigma[n_sets][19], one standard deviation per actuator, n_sets = 1 (every member g >= 1 reads row 0) or G (member
   g reads row g; row 0, the incumbent's, must be all zeros), else ILQR_ERR_ARG; ILQR_ERR_ARG also for a null pointer, an entry that is
   not finite or negative, or hold < 1; ILQR_ERR_STATE while groups are off.  Uploads, synchronises and sets the draw counter to 0.
   group_clear_perturbation: removes it (the counter returns to 0).
   group_draws: the draw counter -- group_perturb calls since the perturbation was installed; -1 for a null handle.
   group_perturb: for every rollout b with g = b mod G >= 1, every knot t and actuator j
       ubar[b][t][j] += sigma[row(g)][j] * z(b, floor(t / hold), j),
   z a standard normal of Philox4x32-10 with key (seed lo, seed hi) and counter (s lo, s hi, draw, k), s = stream0 + b, draw the counter
   in front of the call: block k gives the normals 2k and 2k + 1 of the sequence index i = floor(t / hold) * 19 + j by the Box-Muller
   construction of the plant's observation model above.  The product is rounded on its own and then added; a sigma of exactly 0 adds
   nothing, by selection.  The counter then advances by one.  It is a counter of this family's own: the draws are independent of the
   plant's observation and actuator streams whatever the seeds, and no plant call moves it.  The call then rolls the members
   g >= 1 out from (x0, ubar), so that the cost the next solve starts from -- what it reports for a rollout that accepts no step, and what
   group_select reads -- is the cost of the perturbed controls; the incumbents keep every bit.  Iteration 0 of the next solve rolls every
   rollout out from (x0, ubar) in front of the linearisation again, in every launch order, as behind a warm start.
   ILQR_ERR_STATE before an initialize, while groups are off or while no perturbation is installed.
   group_select: the key of rollout b is key_device[b] (a device array [B] of the caller's) or, with NULL, the cost of the last solve --
   what ilqr_hip_get_cost reports.  Per group the winner is the member with the smallest finite key, among equal keys the lowest member;
   NaN and +-inf never win; without a finite key the winner is member 0.  Writes winner[m], a global rollout index, and group_rec[m] =
   {the winner's key, member 0's key, the number of finite keys, the largest finite key (NaN without one)}.  ILQR_ERR_STATE while groups
   are off, or with NULL before a solve.
   group_get_winners: synchronises the handle's stream; winner[M], rec[M][4], either may be NULL.  ILQR_ERR_STATE before a select.
   group_winners_device: the two device arrays, without synchronising (either pointer may be NULL).
   group_copy_winners_device: enqueues a copy of winner[M] into a device array of the caller's (a row of a per-step log, read once when
   the run ends); never synchronises.  ILQR_ERR_STATE before a select.
   group_adopt: every member of a group receives, bit for bit, the winner's solution state -- what a later call reads about a solved
   rollout: x0, xbar, ubar, K, kff, the cost, lambda and the iteration count as their getters report them and, per installed family of the
   augmented Lagrangian, its whole row of the multiplier store (the header with the penalties and every knot record) with its violation
   and done words.  The diagnostic history stays the member's own: the per-iteration traces, the round traces of the augmented
   Lagrangian, the work lists and the counters.  Linearisation, quadratics, value function and candidates are not copied: iteration 0 of
   the next solve recomputes them for every rollout.  Afterwards the handle is in the state "after a solve".  A group whose winner is
   member 0 keeps every bit.  ILQR_ERR_STATE before a select. */
int ilqr_hip_set_groups(ilqr_hip_ctx* ctx, int G);
int ilqr_hip_num_groups(const ilqr_hip_ctx* ctx);
int ilqr_hip_group_set_perturbation(ilqr_hip_ctx* ctx, int n_sets, const double* sigma /*[n_sets][19]*/, int hold, unsigned long long seed, unsigned long long stream0);
int ilqr_hip_group_clear_perturbation(ilqr_hip_ctx* ctx);
long ilqr_hip_group_draws(const ilqr_hip_ctx* ctx);
int ilqr_hip_group_perturb(ilqr_hip_ctx* ctx);
int ilqr_hip_group_select(ilqr_hip_ctx* ctx, const double* key_device /*[B] or NULL*/);
int ilqr_hip_group_get_winners(ilqr_hip_ctx* ctx, int* winner /*[M]*/, double* rec /*[M][4]*/);
int ilqr_hip_group_winners_device(ilqr_hip_ctx* ctx, const int** winner_device, const double** rec_device);
int ilqr_hip_group_copy_winners_device(ilqr_hip_ctx* ctx, int* winner_out_device /*[M]*/);
int ilqr_hip_group_adopt(ilqr_hip_ctx* ctx);

/* ---- host-side model helpers (no GPU needed) ---- */
/* reference construction as RobotUtils::loadReferences does it (src/common/robot_utils.cpp:369-403):
   whole-body CoM (MuJoCo masses) and world positions of the two ankle bodies */
int ilqr_hip_reference_kinematics(const double* x /*51*/, double* com /*3*/, double* ee /*[2][3]*/);
/* CoM-velocity reference of the same loader (mj_jacSubtreeCom(root) * qvel, src/common/robot_utils.cpp:383-391) */
int ilqr_hip_reference_com_velocity(const double* x /*51*/, double* comvel /*3*/);
/* offline contact-schedule tool (get_contacts.py:96-147): height of the lowest point of each foot's collision hull
   (ankle-link mesh, h1.xml:81,116) above the floor plane z = 0 for the configuration qpos; the tool's stance flag is
   clearance < 0 (MuJoCo reports a floor contact, margin 0).  clearance[0] left, [1] right */
int ilqr_hip_foot_clearance(const double* qpos /*26*/, double* clearance /*2*/);
/* RobotUtils::computeGravComp (src/common/robot_utils.cpp:844-866, correct dof index): qfrc_bias[6+i] at v = 0 */
int ilqr_hip_gravity_compensation(const double* x /*51*/, const double* gravity /*3*/, double* u /*19*/);

/* the HIP stream the handle launches on (as void*), for event timing by the caller */
void* ilqr_hip_stream(ilqr_hip_ctx* ctx);
/* name/duration of the dominant kernel of the last profiled solve are reported by bench.py via hipEvents */

#ifdef __cplusplus
}
#endif
#endif /* ILQR_HIP_H */
