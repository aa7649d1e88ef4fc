// Augmented-Lagrangian outer loop of the batched solve (ilqr_hip_set_augmented_lagrangian; no reference counterpart): the kernels that run
// between two inner solves.  The cost side -- the AL instantiations of k_traj_knot_cost and k_cost_quadratics -- is in dyn_kernels.hip,
// quad_kernels.hip and h1_cost_dev.h, which also states the layout of the multiplier store.
//   k_al_update        multiplier update, violations, done flag, penalty growth, trace row and the count of rollouts left, one pass over
//                      the nominal trajectory, one wave per rollout; <true>: the bounds are rollout b's record of the bounds table
//                      (ilqr_hip_set_al_bounds), <false> the model's ranges at the installed margin; <., true>: and the state family
//                      (ilqr_hip_set_al_state_bounds: the second store, AlDev::sstore) -- a third loop, a third maximum, the done rule over
//                      all three families, the growth of rho_state and the state trace row
//                      <., ., true>: the bounds of knot t are row t of the rollout's windows (ilqr_hip_set_al_knot_bounds ...); instantiated
//                      in libilqr_hip_alknot.so only (al_knot_kernels.hip includes this file with -DAL_KNOT_MODULE: the kernel alone)
//                      <., ., true, true>: and the task family (ilqr_hip_set_al_task_bounds: the third store, AlDev::tstore) -- a fourth loop on
//                      the points of the nominal trajectory (al_task_dev.h), one lane per knot, a fourth maximum, the done rule over all four
//                      families, the growth of rho_task and the task trace row; per-knot instantiations only, in the module
//   k_al_shift         warm-start shift of the multipliers by the knots the trajectory is shifted by (zero tail; shift > N: all zero), penalties reset
//   k_al_state_shift   the same for the state family's store: every column shifts as a hinge column does (knot 0 stays zero)
//   k_al_task_shift    the same for the task family's store; k_al_task_points: the nine task coordinates of the nominal trajectories (module only)
//   k_al_task_velocities  the velocities of those nine coordinates (al_task_dev.h al_task_velocities; module only)
//   k_solve_begin_al   k_solve_begin with active = !done: the prologue of the rounds >= 2 of a solve with the convergence exit
// Every rule is per rollout: nothing here reads another rollout's data, and the one shared word (AlDev::left) is a count.
// Compiled as the tail of ilqr_kernels.hip, beside k_solve_begin and k_warm_shift (a code object of their own for three small kernels cost
// each library ~25 KB of headers and metadata).
#pragma once
#include "al_task_dev.h"
#include "h1_cost_dev.h"
#include "ilqr_kernels.h"

namespace ilqr {

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const double o = __shfl_xor(v, m); v = o > v ? o : v; }
  return v;
}

// Constraint e of a knot's record, e in [0, 38): side = e / 19 (0 lower, 1 upper bound), coordinate e % 19.  The multiplier sits at
// base + e for both families (AL_JHI = AL_JLO + 19, AL_UHI = AL_ULO + 19).
// KNOT: the bounds of knot t are row t of the rollout's windows (AlDev::bounds_knot, sbounds_knot); instantiated in the per-knot module only
// TASK: the task family's window (AlDev::tbounds) on top of the per-knot instantiations
template <bool TABLE, bool STATE, bool KNOT = false, bool TASK = false>
__global__ void __launch_bounds__(64) k_al_update(DevState S, AlDev A, int round, int masked) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, lane = threadIdx.x;
  const double* bd = A.bounds + (long)b * A.bounds_stride;      // (TABLE only: an infinite side gives c = -inf, mu = 0 and no violation)
  const int N = S.N;
  double* rec = A.store + (long)b * A.stride;
  const double rho_j = rec[AL_RHO_JOINT], rho_c = rec[AL_RHO_CTRL];
  const int was_done = A.done[b];
  const int iters = S.iters[b];
  const double* xb = S.xbar + (size_t)b * (N + 1) * H1_NX;
  const double* ub = S.ubar + (size_t)b * N * H1_NU;
  double vj = 0.0, vc = 0.0;
  // hinges, knots 1..N (x_0 is given: its multipliers stay zero and it is left out of the violation)
  for (int e = lane; e < N * 2 * H1_NJ; e += 64) {
    const int t = 1 + e / (2 * H1_NJ), r = e % (2 * H1_NJ), side = r / H1_NJ, j = r % H1_NJ;
    double lo, hi;
    if constexpr (KNOT) { const double* bk = bd + (long)t * A.bounds_knot; lo = bk[ALB_JLO + j]; hi = bk[ALB_JHI + j]; }
    else if constexpr (TABLE) { lo = bd[ALB_JLO + j]; hi = bd[ALB_JHI + j]; } else al_bounds(H1_JRANGE[j], A.margin, lo, hi);
    const double q = xb[t * H1_NX + 7 + j];
    const double c = side ? q - hi : lo - q;
    vj = c > vj ? c : vj;
    if (!was_done) {
      double* mu = rec + AL_HDR + (long)t * AL_KNOT + AL_JLO + r;
      const double s = *mu + rho_j * c;
      *mu = s > 0.0 ? s : 0.0;
    }
  }
  // actuators, knots 0..N-1
  for (int e = lane; e < N * 2 * H1_NU; e += 64) {
    const int t = e / (2 * H1_NU), r = e % (2 * H1_NU), side = r / H1_NU, i = r % H1_NU;
    double lo, hi;
    if constexpr (KNOT) { const double* bk = bd + (long)t * A.bounds_knot; lo = bk[ALB_ULO + i]; hi = bk[ALB_UHI + i]; }
    else if constexpr (TABLE) { lo = bd[ALB_ULO + i]; hi = bd[ALB_UHI + i]; } else al_bounds(H1_CTRLRANGE[i], A.margin, lo, hi);
    const double u = ub[t * H1_NU + i];
    const double c = side ? u - hi : lo - u;
    vc = c > vc ? c : vc;
    if (!was_done) {
      double* mu = rec + AL_HDR + (long)t * AL_KNOT + AL_ULO + r;
      const double s = *mu + rho_c * c;
      *mu = s > 0.0 ? s : 0.0;
    }
  }
  // box coordinates (STATE), knots 1..N as the hinges: entry r of a knot's record is side r / 28 of coordinate r % 28 (ALS_HI = ALS_LO + 28)
  double vs = 0.0, rho_s = 0.0;
  double* srec = nullptr;
  if constexpr (STATE) {
    srec = A.sstore + (long)b * A.sstride;
    rho_s = srec[ALS_RHO];
    const double* sb = A.sbounds + (long)b * A.sbounds_stride;
    for (int e = lane; e < N * 2 * ALS_COORDS; e += 64) {
      const int t = 1 + e / (2 * ALS_COORDS), r = e % (2 * ALS_COORDS), side = r / ALS_COORDS, k = r % ALS_COORDS;
      const double v = xb[t * H1_NX + als_slot(k)];
      const double* sk = KNOT ? sb + (long)t * A.sbounds_knot : sb;
      const double c = side ? v - sk[ALSB_HI + k] : sk[ALSB_LO + k] - v;
      vs = c > vs ? c : vs;
      if (!was_done) {
        double* mu = srec + ALS_HDR + (long)t * ALS_KNOT + ALS_LO + r;
        const double s = *mu + rho_s * c;
        *mu = s > 0.0 ? s : 0.0;
      }
    }
  }
  // task coordinates (TASK), knots 1..N as the hinges, lane = knot: the nine points of the knot's state once, then its 18 sides; a foot's rows
  // are off where the schedule has it in stance (c = -inf: the multiplier goes to 0, no violation)
  double vt = 0.0, rho_t = 0.0;
  double* trec = nullptr;
  if constexpr (TASK) {
    trec = A.tstore + (long)b * A.tstride;
    rho_t = trec[ALT_RHO];
    const double* tb = A.tbounds + (long)b * A.tbounds_stride;
    const int* stn = A.stance + b * A.stance_stride;
    for (int t = 1 + lane; t <= N; t += 64) {
      double p[ALT_COORDS]; al_task_points(xb + t * H1_NX, p);
      const double* tk = tb + (long)t * A.tbounds_knot;
      const int stf[2] = {stn[2 * t], stn[2 * t + 1]};
      double* mu = trec + ALT_HDR + (long)t * ALT_KNOT;
#pragma unroll
      for (int i = 0; i < ALT_COORDS; ++i) {
        const bool off = al_task_row_off(i, stf);
        const double lo = off ? -__builtin_inf() : tk[ALTB_LO + i], hi = off ? __builtin_inf() : tk[ALTB_HI + i];
        const double ch = p[i] - hi, cl = lo - p[i];
        vt = ch > vt ? ch : vt; vt = cl > vt ? cl : vt;
        if (!was_done) {
          const double sh = al_task_side(ch, mu[ALT_HI + i], rho_t), sl = al_task_side(cl, mu[ALT_LO + i], rho_t);
          mu[ALT_HI + i] = sh > 0.0 ? sh : 0.0; mu[ALT_LO + i] = sl > 0.0 ? sl : 0.0;
        }
      }
    }
  }
  vj = wave_max(vj); vc = wave_max(vc);
  if constexpr (STATE) vs = wave_max(vs);
  if constexpr (TASK) vt = wave_max(vt);
  if (lane != 0) return;
  A.viol[2 * b] = vj; A.viol[2 * b + 1] = vc;
  if constexpr (STATE) A.sviol[b] = vs;
  if constexpr (TASK) A.tviol[b] = vt;
  if (was_done && masked) return;          // (the round did not run for this rollout: its trace row stays NaN)
  double* tr = A.trace + ((size_t)round * S.B + b) * 5;
  tr[0] = vj; tr[1] = vc; tr[2] = rho_j; tr[3] = rho_c; tr[4] = (double)iters;
  if constexpr (STATE) { double* ts = A.strace + ((size_t)round * S.B + b) * 2; ts[0] = vs; ts[1] = rho_s; }
  if constexpr (TASK) { double* tt = A.ttrace + ((size_t)round * S.B + b) * 2; tt[0] = vt; tt[1] = rho_t; }
  if (was_done) return;
  if (vj <= A.tol_joint && vc <= A.tol_ctrl && (!STATE || vs <= A.tol_state) && (!TASK || vt <= A.tol_task)) { A.done[b] = 1; return; }
  const double gj = rho_j * A.growth, gc = rho_c * A.growth;
  rec[AL_RHO_JOINT] = gj < A.rho_joint_max ? gj : A.rho_joint_max;
  rec[AL_RHO_CTRL] = gc < A.rho_ctrl_max ? gc : A.rho_ctrl_max;
  if constexpr (STATE) { const double gs = rho_s * A.growth; srec[ALS_RHO] = gs < A.rho_state_max ? gs : A.rho_state_max; }
  if constexpr (TASK) { const double gt = rho_t * A.growth; trec[ALT_RHO] = gt < A.rho_task_max ? gt : A.rho_task_max; }
  atomicAdd(A.left + round, 1);
}

#ifdef AL_KNOT_MODULE
// The task family's store under the walk of k_al_state_shift (below, in the library): every column is one side of a task coordinate at the
// knots 0..N, kept for 1 <= t and t + shift <= N; rho_task back to rho_task0.  The window of bounds is horizon-local and does not move.
__global__ void __launch_bounds__(64) k_al_task_shift(AlDev A, int N, int shift) {
  const int b = blockIdx.x, e = threadIdx.x;
  double* rec = A.tstore + (long)b * A.tstride;
  if (e == 0) { rec[ALT_RHO] = A.rho_task0; A.tviol[b] = 0.0; }
  if (e >= 2 * ALT_COORDS) return;
  double* k = rec + ALT_HDR + ALT_LO;
  for (int t = 0; t <= N; ++t) {
    const long ts = (long)t + shift;
    const bool keep = t >= 1 && ts <= N;
    const double v = k[(ts <= N ? ts : (long)N) * ALT_KNOT + e];      // (index clamped into the record, masked below)
    k[(long)t * ALT_KNOT + e] = keep ? v : 0.0;
  }
}
// the nine task coordinates of every knot of the nominal trajectories as the cost kernels and the update form them: one lane per (rollout, knot)
__global__ void __launch_bounds__(64) k_al_task_points(DevState S, double* out) {
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long)S.B * (S.N + 1)) return;
  double p[ALT_COORDS]; al_task_points(S.xbar + idx * H1_NX, p);
#pragma unroll
  for (int i = 0; i < ALT_COORDS; ++i) out[idx * ALT_COORDS + i] = p[i];
}
// the nine velocities of the same points at every knot of the nominal trajectories (al_task_dev.h al_task_velocities): one lane per (rollout, knot)
__global__ void __launch_bounds__(64) k_al_task_velocities(DevState S, double* out) {
  const long idx = (long)blockIdx.x * 64 + threadIdx.x;
  if (idx >= (long)S.B * (S.N + 1)) return;
  double v[ALV_COORDS]; al_task_velocities(S.xbar + idx * H1_NX, v);
#pragma unroll
  for (int i = 0; i < ALV_COORDS; ++i) out[idx * ALV_COORDS + i] = v[i];
}
#else
// Each lane owns one column of the knot records and walks the knots upwards: it reads knot t + shift after it has written every knot < t, so
// the shift is in place without a barrier.
__global__ void __launch_bounds__(128) k_al_shift(AlDev A, int N, int shift, double rho_joint, double rho_ctrl) {
  const int b = blockIdx.x, e = threadIdx.x;
  double* rec = A.store + (long)b * A.stride;
  if (e == 0) { rec[AL_RHO_JOINT] = rho_joint; rec[AL_RHO_CTRL] = rho_ctrl; A.done[b] = 0; A.viol[2 * b] = 0.0; A.viol[2 * b + 1] = 0.0; }
  if (e >= AL_KNOT) return;
  const bool joint = e < AL_ULO;
  double* k = rec + AL_HDR;
  for (int t = 0; t <= N; ++t) {
    const long ts = (long)t + shift;
    const bool keep = joint ? (t >= 1 && ts <= N) : (ts <= N - 1);
    const double v = k[(ts <= N ? ts : (long)N) * AL_KNOT + e];      // (index clamped into the record, masked below)
    k[(long)t * AL_KNOT + e] = keep ? v : 0.0;
  }
}

// The state family's store under the same walk: every column is a box coordinate's bound at the knots 0..N, kept for 1 <= t and t + shift <= N.
__global__ void __launch_bounds__(64) k_al_state_shift(AlDev A, int N, int shift) {
  const int b = blockIdx.x, e = threadIdx.x;
  double* rec = A.sstore + (long)b * A.sstride;
  if (e == 0) { rec[ALS_RHO] = A.rho_state0; A.sviol[b] = 0.0; }
  if (e >= 2 * ALS_COORDS) return;
  double* k = rec + ALS_HDR + ALS_LO;
  for (int t = 0; t <= N; ++t) {
    const long ts = (long)t + shift;
    const bool keep = t >= 1 && ts <= N;
    const double v = k[(ts <= N ? ts : (long)N) * ALS_KNOT + e];      // (index clamped into the record, masked below)
    k[(long)t * ALS_KNOT + e] = keep ? v : 0.0;
  }
}

// One wave: the rollouts not yet done enter list (0, 0) in order.  A done rollout is inactive and keeps what its last round left in the
// per-rollout observables (cost, iteration count, traces): the existing getters describe the last round that ran for it.
__global__ void __launch_bounds__(64) k_solve_begin_al(DevState S, const int* done) {
  const int lane = threadIdx.x;
  int n = 0;
  for (int b0 = 0; b0 < S.B; b0 += 64) {
    const int b = b0 + lane;
    const bool in = b < S.B;
    const bool act = in && done[b] == 0;
    const unsigned long long m = __ballot(act);
    if (in) {
      S.active[b] = act ? 1 : 0; S.need_retry[b] = 0;
      if (S.grp_a) { S.grp_a[b] = 0; S.grp_r[b] = 0; }
    }
    if (act) {
      if (S.order) S.order[n + __popcll(m & ((1ull << lane) - 1ull))] = b;
      S.iters[b] = 0;
      const double J0 = S.Jbase[b];
      S.J[b] = J0;
      for (int i = 0; i <= S.max_iter; ++i) S.trace_cost[(size_t)b * (S.max_iter + 1) + i] = (i == 0) ? J0 : __builtin_nan("");
      for (int i = 0; i < S.max_iter; ++i) { S.trace_alpha[(size_t)b * S.max_iter + i] = __builtin_nan(""); S.trace_lambda[(size_t)b * S.max_iter + i] = __builtin_nan(""); }
    }
    n += __popcll(m);
  }
  if (lane == 0) {
    if (S.order) { S.order_n[0] = n; for (int i = 1; i < 2 * (S.max_iter + 1); ++i) S.order_n[i] = 0; }
    if (S.grp_a) for (int i = 0; i < S.max_iter + 2; ++i) { S.order_rn[i] = 0; S.order_an[i] = 0; }
    if (S.kr) for (int i = 0; i <= S.max_iter; ++i) S.kr_n[i] = 0;
    if (S.chg) for (int i = 0; i < S.max_iter + 2; ++i) { if (i <= S.max_iter) S.chg_n[i] = 0; S.chg_rn[i] = 0; S.chg_an[i] = 0; }
  }
}

void launch_al_update(const DevState& S, const AlDev& A, int round, int masked, hipStream_t st) {
  switch (al_variant(true, A.bounds, A.sbounds, A.bounds_knot)) {      // (al_plan.h: the variant of the cost kernels)
    case AL_KNOT_TABLE: case AL_KNOT_TABLE_STATE: g_al_knot.al_update(&S, &A, round, masked, st); break;      // (windows: the module's instantiations)
    case AL_TABLE_STATE: hipLaunchKernelGGL((k_al_update<true, true>), dim3(S.B), dim3(64), 0, st, S, A, round, masked); break;
    case AL_TABLE: hipLaunchKernelGGL((k_al_update<true, false>), dim3(S.B), dim3(64), 0, st, S, A, round, masked); break;
    default: hipLaunchKernelGGL((k_al_update<false, false>), dim3(S.B), dim3(64), 0, st, S, A, round, masked); break;
  }
}
void launch_al_shift(const AlDev& A, int B, int N, int shift, double rho_joint, double rho_ctrl, hipStream_t st) {
  hipLaunchKernelGGL(k_al_shift, dim3(B), dim3(128), 0, st, A, N, shift, rho_joint, rho_ctrl);
  if (A.sbounds) hipLaunchKernelGGL(k_al_state_shift, dim3(B), dim3(64), 0, st, A, N, shift);
  if (A.tbounds) g_al_knot.task_shift(&A, B, N, shift, st);      // (the task family's kernels: the module's)
}
void launch_solve_begin_al(const DevState& S, const int* done, hipStream_t st) { hipLaunchKernelGGL(k_solve_begin_al, dim3(1), dim3(64), 0, st, S, done); }
#endif      // AL_KNOT_MODULE

}  // namespace ilqr
