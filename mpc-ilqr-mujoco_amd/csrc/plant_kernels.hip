// The closed-loop plant kept on the device (include/ilqr_hip.h "device-resident plant"): ONE fused kernel per MPC step that does what the
// reference's runSimulation does between two calls of MPC::stepOnce (main/humanoid_mpc.cpp:122-190) with the policy the handle has just solved:
//   k_plant_advance  pending velocity kick -> u = ubar_0 + K_0 (x - xbar_0) (src/ilqr/mpc.cpp:97-101; a non-finite u becomes zero,
//                    main:162-165) -> `substeps` plant steps of h = dt / substeps (main:128,168-170) -> x, u, stance, alive (main:134-137)
//                    and the history ring
//   k_plant_follow   the same over `count` consecutive intervals under the policy knots k0 .. k0 + count - 1 of ONE solve (the caller
//                    solves every count-th interval only; the reference itself solves every step): the state stays in LDS / registers
//                    between the intervals, only the rows of the history ring are written on the way
// Two lanes per rollout as in dyn_split_kernels.hip (the step itself is that file's step_any, dyn_step_shared.h), one wave per workgroup.
// A translation unit of its own: no kernel of the solve shares a compilation with it.  k_plant_follow is plant_follow_body.h, included
// seven times: without a table, with a plant parameter table (k_plant_follow_p), with a parameter and a wrench table (k_plant_follow_w),
// with parameter, wrench and payload tables (k_plant_follow_m), with those three under an observation table (k_plant_follow_o), and with
// those four under an actuator table (k_plant_follow_a), and with those five under a joint table (k_plant_follow_j); an eighth time, with
// those six under a terrain table (k_plant_follow_t), by the terrain module.
// The host side is written once, at the end of the file: every family is launched from one call record (ilqr_kernels.h PlantCall) by one
// launcher, its dynamic LDS and the kernel arguments behind the common ones built up family by family (follow_lds, follow_tail), and a
// module exports the same entry points under its own stem.
#include <hip/hip_runtime.h>

#include <tuple>

#include "h1_cost_dev.h"
#define ABA_FENCE          // as dyn_split_kernels.hip: the step is compiled under the same switches there and here
#include "h1_aba_split.h"
#include "h1_foot_contact_dev.h"
#include "ilqr_kernels.h"

using namespace h1;

namespace ilqr {

// This file is compiled eight times (csrc/Makefile): into the library, as everything but the wrench family; and with -DPLANT_WRENCH_MODULE into
// libilqr_hip_wrench.so, as the wrench family alone (k_plant_follow_w, k_step_w and the wrench-carrying copies of the non-inlined steps),
// which the C API opens on first use (ilqr_capi.hip MODULE_DESC). The family is 1.0 MB of code that both the product and the test
// library would carry; the product library has to stay below 0.8 of the test library (tests/test_gpu_configs.py), which 0.17 MB would
// have used up.  One module serves both libraries: the plant runs on the two-lane step whatever the handle's family.
// A third compilation, -DPLANT_PAYLOAD_MODULE into libilqr_hip_payload.so, is the payload family alone (k_plant_follow_m, k_step_m and the
// same copies of the non-inlined steps instantiated with the payload as well), opened on first use in the same way and for the same reason.
#ifdef PLANT_WRENCH_MODULE
#define DYN_STEP_WRENCH      // the wrench-carrying copies of the non-inlined steps: compiled in the module alone
#endif
// A fourth compilation, -DPLANT_OBSERVE_MODULE into libilqr_hip_observe.so, is the observation family alone (k_plant_follow_o, the superset of
// the payload family whose control law reads a measured state, k_observation_draw and k_observe_apply), opened in the same way.
// A fifth compilation, -DPLANT_ACTUATOR_MODULE into libilqr_hip_actuator.so, is the actuator family alone (k_plant_follow_a, the superset of
// the observation family whose step takes a delayed, lagged and noisy torque, and k_actuator_draw), opened in the same way.
// A sixth compilation, -DPLANT_JOINTS_MODULE into libilqr_hip_joints.so, is the joints family alone (k_plant_follow_j, the superset of the
// actuator family whose step reads gain, torque range, damping and armature of every joint from a record, and k_step_j), opened in the same way.
// A seventh compilation, -DPLANT_TERRAIN_MODULE into libilqr_hip_terrain.so, is the terrain family alone (k_plant_follow_t, the superset of the
// joints family that decides each rollout's stance flags against a floor of the rollout's own height, and k_step_t), opened in the same way.
#ifdef PLANT_TERRAIN_MODULE
#define PLANT_LOWER_FAMILIES      // a family above the joints': everything the families below it are made of, none of their kernels
#endif
#if defined(PLANT_PAYLOAD_MODULE) || defined(PLANT_OBSERVE_MODULE) || defined(PLANT_ACTUATOR_MODULE) || defined(PLANT_JOINTS_MODULE) || defined(PLANT_LOWER_FAMILIES)
#define DYN_STEP_WRENCH
#define DYN_STEP_PAYLOAD     // ... carrying the payload too
#endif
#if defined(PLANT_JOINTS_MODULE) || defined(PLANT_LOWER_FAMILIES)
#define DYN_STEP_JOINTS      // ... and the copies that read a joint record as well
#endif
#if defined(PLANT_WRENCH_MODULE) || defined(PLANT_PAYLOAD_MODULE) || defined(PLANT_OBSERVE_MODULE) || defined(PLANT_ACTUATOR_MODULE) || defined(PLANT_JOINTS_MODULE) || defined(PLANT_LOWER_FAMILIES)
#define PLANT_MODULE         // a module: none of the library's own kernels and launchers
#endif
// What a module compilation holds, named ONCE for the launchers at the end of this file: the number of its followed family (the
// PLANT_TABLE of plant_follow_body.h), that kernel, the stem of its exported symbols ilqr_<stem>_module_<entry>, and -- where it has a
// per-item step kernel under explicit stance flags -- that kernel, its LDS bytes and what it takes of the entry point's (wrench, payload,
// joints).  The library holds families 0 and 1 and the advance.
#if defined(PLANT_WRENCH_MODULE)
#define PLANT_FAMILY 2
#define PLANT_FOLLOW_KERNEL k_plant_follow_w
#define PLANT_STEM wrench
#define PLANT_STEP_KERNEL k_step_w
#define PLANT_STEP_LDS_BYTES STEP_W_LDS_BYTES
#define PLANT_STEP_TAIL wrench
#elif defined(PLANT_PAYLOAD_MODULE)
#define PLANT_FAMILY 3
#define PLANT_FOLLOW_KERNEL k_plant_follow_m
#define PLANT_STEM payload
#define PLANT_STEP_KERNEL k_step_m
#define PLANT_STEP_LDS_BYTES STEP_M_LDS_BYTES
#define PLANT_STEP_TAIL wrench, payload
#elif defined(PLANT_OBSERVE_MODULE)
#define PLANT_FAMILY 4
#define PLANT_FOLLOW_KERNEL k_plant_follow_o
#define PLANT_STEM observe
#elif defined(PLANT_ACTUATOR_MODULE)
#define PLANT_FAMILY 5
#define PLANT_FOLLOW_KERNEL k_plant_follow_a
#define PLANT_STEM actuator
#elif defined(PLANT_JOINTS_MODULE)
#define PLANT_FAMILY 6
#define PLANT_FOLLOW_KERNEL k_plant_follow_j
#define PLANT_STEM joints
#define PLANT_STEP_KERNEL k_step_j
#define PLANT_STEP_LDS_BYTES STEP_J_LDS_BYTES
#define PLANT_STEP_TAIL wrench, payload, joints
#elif defined(PLANT_TERRAIN_MODULE)
#define PLANT_FAMILY 7
#define PLANT_FOLLOW_KERNEL k_plant_follow_t
#define PLANT_STEM terrain
#define PLANT_STEP_KERNEL k_step_t      // (decides its own stance flags: an entry point of its own shape, no PLANT_STEP_TAIL)
#define PLANT_STEP_LDS_BYTES STEP_T_LDS_BYTES
#endif
// sizes of the tables' records in doubles, for the kernels that stage them and for follow_lds (h1s::DIST_REC and h1s::JOINT_REC: h1_aba_split.h)
#define PLANT_REC 8
#define WRENCH_REC 16
#define TERRAIN_REC 8
#include "dyn_step_shared.h"

// LDS of a workgroup, in doubles: the dynamics scratch of the step (LDS_SLOTS x 64, at the base: the non-inlined steps address it there),
// then per rollout of the wave the state x (51), xbar_0 (51), ubar_0 (19), the control u (19) and -- feedback mode 1 -- K_0 (19 x 51).
// RPW rollouts per wave: 32 (a lane pair each, as k_last_step_s) while K_0 is read once, from memory; 4 in feedback mode 1, where the
// wave's K_0 stay in LDS across the substeps (4 x 7.6 KB; 32 of them are 248 KB and fit nowhere on the chip).
#define PLANT_NX H1_NX
#define PLANT_NU H1_NU
template <int FB> struct PlantLayout {
  static constexpr int RPW = FB ? 4 : 32;
  static constexpr int XS = h1s::LDS_SLOTS * 64, XB = XS + RPW * PLANT_NX, UB = XB + RPW * PLANT_NX, US = UB + RPW * PLANT_NU, KS = US + RPW * PLANT_NU;
  static constexpr int DOUBLES = KS + (FB ? RPW * PLANT_NU * PLANT_NX : 0);
};

DEVFN bool finite_half(const h1s::HalfX& h) {
  bool f = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) f = f && isfinite(h.p[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) f = f && isfinite(h.quat[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) f = f && isfinite(h.vb[k]);
  f = f && isfinite(h.q.th11) && isfinite(h.q.qd11);
#pragma unroll
  for (int k = 0; k < 5; ++k) f = f && isfinite(h.q.thL[k]) && isfinite(h.q.qdL[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) f = f && isfinite(h.q.thA[k]) && isfinite(h.q.qdA[k]);
  return f;
}
DEVFN bool finite_half_u(const h1s::HalfU& u) {
  bool f = isfinite(u.u11);
#pragma unroll
  for (int k = 0; k < 5; ++k) f = f && isfinite(u.uL[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) f = f && isfinite(u.uA[k]);
  return f;
}
// this lane's hinges of a control vector (the torso's by the even lane)
DEVFN void store_half_u(bool side, const h1s::HalfU& u, double* o) {
  if (!side) o[10] = u.u11;
#pragma unroll
  for (int k = 0; k < 5; ++k) o[h1s::jleg(side, k)] = u.uL[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[h1s::jarm(side, k)] = u.uA[k];
}
// qvel += dv (dv in the order of qvel: linear (world), angular (body), the 19 hinge rates)
DEVFN void kick_half(bool side, h1s::HalfX& h, const double* dv) {
#pragma unroll
  for (int k = 0; k < 6; ++k) h.vb[k] += dv[k];
  h.q.qd11 += dv[6 + 10];
#pragma unroll
  for (int k = 0; k < 5; ++k) h.q.qdL[k] += dv[6 + h1s::jleg(side, k)];
#pragma unroll
  for (int k = 0; k < 4; ++k) h.q.qdA[k] += dv[6 + h1s::jarm(side, k)];
}
// LDS operations of a wave execute in order and the workgroup is one wave: only the compiler has to be kept from moving them
DEVFN void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// u = ubar_k + K_k (x - xbar_k) for the wave's rollouts (k = knot; 0 in k_plant_advance), x / xbar_k / ubar_k in LDS -> u in LDS.  The arithmetic of k_compute_control
// (ilqr_kernels.hip): one accumulator per row, started at ubar_0, the 51 terms in index order.  The 64 lanes deal the RPW x 19 rows out;
// nothing of the dynamics is live here (the state sits in LDS), so the step's register budget is its own.
// XOFF >= 0: the law reads its state from the rows at that LDS offset instead of XS (k_plant_follow_o: the observed rows).
template <int FB, int XOFF = -1>
DEVFN void control_law(const DevState& S, double* lds, int b0, int knot = 0) {
  typedef PlantLayout<FB> Lay;
  constexpr int n = PLANT_NX, m = PLANT_NU;
  for (int it = threadIdx.x; it < Lay::RPW * m; it += 64) {
    const int r = it / m, row = it - r * m;
    const int b = b0 + r < S.B ? b0 + r : S.B - 1;
    const double* Kr = FB ? lds + Lay::KS + (r * m + row) * n : S.K + ((size_t)b * S.N * m + (size_t)knot * m + row) * n;
    const double* x = lds + (XOFF >= 0 ? XOFF : Lay::XS) + r * n;
    const double* xb = lds + Lay::XB + r * n;
    double s = lds[Lay::UB + r * m + row];
    for (int j = 0; j < n; ++j) s += Kr[j] * (x[j] - xb[j]);
    lds[Lay::US + r * m + row] = s;
  }
}

#ifndef PLANT_MODULE
// KIND: the CONTACT value of step_any (step_kind(dyn)); FB: feedback mode -- 0 the reference's loop, u held over the MPC interval; 1 the
// control law re-evaluated on (xbar_0, ubar_0, K_0) before every substep.  dyn: the PLANT's parameters (h = dt / substeps).
// sched / sched_stride: the contact schedule (row 0 of each set is the stance of this MPC step); geom: stance from the feet instead.
// kick: a velocity kick Pl.dv is pending; hist_row >= 0: row of the history ring to fill.
template <int KIND, int FB>
__global__ void __launch_bounds__(64) k_plant_advance(DevState S, PlantDev Pl, DynParams dyn, const int* sched, long sched_stride, int geom, int substeps, int kick, long hist_row) {
  extern __shared__ double lds[];
  typedef PlantLayout<FB> Lay;
  constexpr int n = PLANT_NX, m = PLANT_NU, RPW = Lay::RPW;
  const int tid = threadIdx.x;
  const int pr = tid >> 1;
  const bool side = (tid & 1) != 0;
  const int b0 = blockIdx.x * RPW;
  const bool owner = pr < RPW && b0 + pr < S.B;      // (lane pairs stay together: every flag below is the same on both lanes of a pair)
  const int b = owner ? b0 + pr : S.B - 1;
  const int N = S.N;
  // ---- first knot of the policy -> LDS, consecutive lanes on consecutive doubles
  for (int r = 0; r < RPW; ++r) {
    const int br = b0 + r < S.B ? b0 + r : S.B - 1;
    const double* xb = S.xbar + (size_t)br * (N + 1) * n;
    const double* ub = S.ubar + (size_t)br * N * m;
    if (tid < n) lds[Lay::XB + r * n + tid] = xb[tid];
    if (tid < m) lds[Lay::UB + r * m + tid] = ub[tid];
    if constexpr (FB != 0) {
      const double* K0 = S.K + (size_t)br * N * m * n;
      for (int e = tid; e < m * n; e += 64) lds[Lay::KS + r * m * n + e] = K0[e];
    }
  }
  // ---- plant state, kick, the guards of main:134-137
  h1s::HalfX h; h1s::load_half(side, Pl.x + (size_t)b * n, h);
  const bool was_alive = owner && Pl.alive[b] != 0;
  if (owner && hist_row >= 0 && !was_alive) h1s::store_half(side, h, Pl.hist_x + ((size_t)hist_row * S.B + b) * n);      // (a frozen rollout logs the state it stopped in)
  if (kick && was_alive) kick_half(side, h, Pl.dv + (size_t)b * H1_NV);
  bool fin = finite_half(h);
  fin = h1s::xch_flag(fin) && fin;
  bool run = was_alive && fin;
  if (owner && hist_row >= 0 && was_alive) h1s::store_half(side, h, Pl.hist_x + ((size_t)hist_row * S.B + b) * n);       // x the control law sees (after the kick)
  if (pr < RPW) h1s::store_half(side, h, lds + Lay::XS + pr * n);
  int st[2] = {1, 1};
  if (owner) { st[0] = sched[b * sched_stride]; st[1] = sched[b * sched_stride + 1]; }
  h1s::HalfU u;
  for (int k = 0; k < substeps; ++k) {
    // The one piece that is not plain C++: an EMPTY asm statement (no instruction) that makes the lane index opaque per substep, as in
    // k_rollout_s.  Without it the per-lane body constants `side ? right : left` are hoisted out of the substep loop and spilled: the free
    // plant's frame grows from 228 to 728 B (120 -> 191 spilled registers), the joint-limit plant's from 1208 to 1720 B (158 -> 225).
    int lane = tid; asm volatile("" : "+v"(lane));
    const bool side_t = (lane & 1) != 0;
    const int prt = lane >> 1;
    if (FB != 0 || k == 0) {
      wave_lds_fence();
      control_law<FB>(S, lds, b0);
      wave_lds_fence();
    }
    const int pc = prt < RPW ? prt : 0;
    load_half_u(side_t, lds + Lay::US + pc * m, u);
    bool ufin = finite_half_u(u);
    ufin = h1s::xch_flag(ufin) && ufin;
    if (!ufin) { u.u11 = 0.0; for (int q = 0; q < 5; ++q) u.uL[q] = 0.0; for (int q = 0; q < 4; ++q) u.uA[q] = 0.0; }      // main:162-165
    wave_lds_fence();      // (the odd lane reads the shared coordinates its partner stored at the end of the previous substep)
    if (run) {
      const h1s::LaneLds L{lds, 64, lane};
      h1s::load_half(side_t, lds + Lay::XS + prt * n, h);
      if constexpr (KIND >= 1 && KIND <= 4) {
        if (geom) h1s::geom_stance(side_t, h, st[0], st[1]);      // (reported; the step decides again behind its call boundary, on the same state with the same machine code)
      }
      step_any<KIND>(side_t, h, u, dyn, st, L, geom);
      wave_lds_fence();      // (the step's LDS scratch and the state rows are different words; the fence orders the row against the next control law)
      h1s::store_half(side_t, h, lds + Lay::XS + prt * n);
    }
  }
  // ---- write-back: a rollout whose state is or became non-finite keeps its state and stance, reports zero control and is never advanced again
  fin = finite_half(h);
  fin = h1s::xch_flag(fin) && fin;
  run = run && fin;
  if (!owner) return;
  if (!run) { u.u11 = 0.0; for (int q = 0; q < 5; ++q) u.uL[q] = 0.0; for (int q = 0; q < 4; ++q) u.uA[q] = 0.0; }
  store_half_u(side, u, Pl.u + (size_t)b * m);
  if (hist_row >= 0) store_half_u(side, u, Pl.hist_u + ((size_t)hist_row * S.B + b) * m);
  if (run) {
    h1s::store_half(side, h, Pl.x + (size_t)b * n);
    if (!side) { Pl.stance[2 * (size_t)b] = st[0]; Pl.stance[2 * (size_t)b + 1] = st[1]; }
  }
  if (!side) Pl.alive[b] = run ? 1 : 0;
}

#endif
// ---- k_plant_follow: `count` intervals in one launch.  Per interval j exactly what k_plant_advance does with knot k0 + j in the place of
// knot 0, row k0 + j of the schedule and row (hist_row0 + j) % hist_cap of the ring; the kick before interval 0 only.  What an advance
// leaves in memory for the next one stays on the chip: the state in the rollout's LDS row (the next interval loads it from there as an
// advance loads Pl.x: the even lane's shared coordinates), alive in `run`, and -- for the one case in which an advance does NOT write its
// state back, a rollout that is or becomes non-finite -- the state its interval started from in a keep row XK, from which the rollout is
// restored and then frozen (interval 0: from Pl.x, which holds the state in front of the kick and is not written before the end).
// FB = 0: xbar_k is dead once the interval's one control law has run, the keep row takes its place; FB = 1: a row of its own (4 x 408 B).
template <int FB> struct FollowLayout : PlantLayout<FB> {
  typedef PlantLayout<FB> Base;
  static constexpr int XK = FB ? Base::DOUBLES : Base::XB;
  static constexpr int DOUBLES = Base::DOUBLES + (FB ? Base::RPW * PLANT_NX : 0);
};
DEVFN void zero_half_u(h1s::HalfU& u) {
  u.u11 = 0.0;
#pragma unroll
  for (int q = 0; q < 5; ++q) u.uL[q] = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) u.uA[q] = 0.0;
}
#ifndef PLANT_MODULE
#define PLANT_TABLE 0
#include "plant_follow_body.h"
#endif

// ---- plant parameter table (include/ilqr_hip.h ilqr_hip_plant_set_params): k_plant_follow_p.  One record of PLANT_REC doubles per rollout
// -- g[3], mu, soft, lim_k, torque gain, one double of padding (64 B) -- or ONE record that every rollout reads (rec_stride = 0).  The wave
// stages the records of its RPW rollouts in LDS once, behind the layout of the kernel: RPW x 8 consecutive doubles of the table,
// consecutive lanes on consecutive doubles (2 KB at FB = 0, 256 B at FB = 1).  Each substep reads its seven values from there behind the
// opaque lane index, right before the step: nothing of the record is live across the control law or from one substep to the next.
// There is no k_plant_advance_p: with a table an advance is the followed kernel over one interval, which is an advance bit for bit
// (GPU tests of plant_follow); a second family of twelve kernels would be a further 0.5 MB of code for a path that is not the fast one.
template <int RPW>
DEVFN void stage_plant_records(const DevState& S, double* rows, int b0, const double* ptab, int rec_stride) {
  for (int e = threadIdx.x; e < RPW * PLANT_REC; e += 64) {
    const int r = e / PLANT_REC;
    const int br = b0 + r < S.B ? b0 + r : S.B - 1;      // (a wave's unowned rows read the last rollout's record, as they read its policy)
    rows[e] = ptab[(size_t)br * rec_stride + (e - r * PLANT_REC)];
  }
}
// one plant step with the record `rec` in the place of g, mu, soft and lim_k of `dyn` (h stays the kernel argument: wave-uniform, as the
// inlined steps need it behind their "+s" constraint) and gain * u in the place of u -- behind the non-finite guard, in front of the
// step's clamp; the caller's u, which is what it reports, stays the law's output
// WR: under the external wrench at LDS offset wro (step_any_w)
template <int KIND, bool WR = false>
DEVFN void plant_step_table(bool side, h1s::HalfX& h, const h1s::HalfU& u, const DynParams& dyn, const int* st, const h1s::LaneLds& L, int geom, const double* rec, int wro = 0) {
  DynParams dl = dyn;
  dl.g[0] = rec[0]; dl.g[1] = rec[1]; dl.g[2] = rec[2]; dl.mu = rec[3]; dl.soft = rec[4]; dl.lim_k = rec[5];
  const double gain = rec[6];
  h1s::HalfU us;
  us.u11 = gain * u.u11;
#pragma unroll
  for (int q = 0; q < 5; ++q) us.uL[q] = gain * u.uL[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) us.uA[q] = gain * u.uA[q];
#ifdef PLANT_MODULE
  if constexpr (WR) step_any_w<KIND>(side, h, us, dl, st, L, geom, wro);
  else
#endif
  step_any<KIND>(side, h, us, dl, st, L, geom);
}
#ifndef PLANT_MODULE
#define PLANT_TABLE 1
#include "plant_follow_body.h"
#endif

#ifdef PLANT_WRENCH_MODULE
// ---- wrench table (include/ilqr_hip.h ilqr_hip_plant_set_wrench): k_plant_follow_w.  One record of WRENCH_REC doubles (128 B) per rollout
// -- force F[3] and torque T[3] in the world frame, point of application r[3] in the pelvis frame, the window [first, end) in plant
// intervals, five doubles of padding -- or ONE record that every rollout reads (wr_stride = 0).  Staged in LDS once per launch behind the
// parameter rows, consecutive lanes on consecutive doubles (4 KB at FB = 0, 512 B at FB = 1), followed by one row of zeros: the wrench of
// an interval outside the window.  A substep hands the step the offset of one of the two rows, so the window costs no second code path
// and a wrench of zero is the arithmetic of a table whose window is shut.  The kernel always reads a parameter record: without a
// parameter table the caller passes one record of the handle's own values with gain 1.
template <int RPW>
DEVFN void stage_wrench_records(const DevState& S, double* rows, int b0, const double* wtab, int wr_stride) {
  for (int e = threadIdx.x; e < (RPW + 1) * WRENCH_REC; e += 64) {
    const int r = e / WRENCH_REC;
    const int br = b0 + r < S.B ? b0 + r : S.B - 1;
    rows[e] = r < RPW ? wtab[(size_t)br * wr_stride + (e - r * WRENCH_REC)] : 0.0;
  }
}
#define PLANT_TABLE 2
#include "plant_follow_body.h"

// ---- one step under a wrench per item (ilqr_hip_step_wrench): k_step_s of dyn_split_kernels.hip with the wrench-carrying step; the 32
// items of a workgroup stage their nine values behind the dynamics scratch
#define STEP_W_LDS_BYTES ((h1s::LDS_SLOTS * 64 + 32 * 9) * sizeof(double))
template <int CK>
__global__ void __launch_bounds__(64) k_step_w(int count, const double* x, const double* u, DynParams dyn, double* xn, int st_l, int st_r, const double* wrench) {
  extern __shared__ double lds[];
  constexpr int WR0 = h1s::LDS_SLOTS * 64;
  const int i0 = blockIdx.x * 32;
  for (int e = threadIdx.x; e < 32 * 9; e += 64) {
    const int r = e / 9;
    const int ir = i0 + r < count ? i0 + r : count - 1;
    lds[WR0 + e] = wrench[(size_t)ir * 9 + (e - r * 9)];
  }
  wave_lds_fence();
  const int i = i0 + ((int)threadIdx.x >> 1);
  const bool side = (threadIdx.x & 1) != 0;
  if (i >= count) return;
  const h1s::LaneLds L{lds, 64, (int)threadIdx.x};
  h1s::HalfX h; h1s::load_half(side, x + (size_t)i * H1_NX, h);
  h1s::HalfU uu; load_half_u(side, u + (size_t)i * H1_NU, uu);
  int st[2] = {st_l, st_r};
  step_any_w<CK>(side, h, uu, dyn, st, L, 0, WR0 + ((int)threadIdx.x >> 1) * 9);
  h1s::store_half(side, h, xn + (size_t)i * H1_NX);
}

#endif

#if defined(PLANT_PAYLOAD_MODULE) || defined(PLANT_OBSERVE_MODULE) || defined(PLANT_ACTUATOR_MODULE) || defined(PLANT_JOINTS_MODULE) || defined(PLANT_LOWER_FAMILIES)
// ---- payload table (include/ilqr_hip.h ilqr_hip_plant_set_payload): k_plant_follow_m.  A rollout has two disturbance rows of h1s::DIST_REC doubles
// in LDS behind the parameter rows, staged once per launch, consecutive lanes on consecutive doubles (12 KB at FB = 0, 1.5 KB at FB = 1):
//   row r        the wrench record (F, T, r, first, end; zeros without a wrench table, wtab null), the payload record, padding
//   row RPW + r  zeros, the same payload record, padding: the row of an interval outside the wrench's window
// (the layout of a row: h1_aba_split.h, at PAYLOAD_AT)
// A substep hands the step the offset of one of the two, as k_plant_follow_w does with its zero row; the payload is in both, so it acts in
// every substep.  Records of the tables: wrench 16 doubles (WRENCH_REC of the wrench module), payload PAYLOAD_REC = 16 doubles (ten values
// and padding, 128 B); a stride of 0 is ONE record that every rollout reads.
// MNULL: mtab may be null as well (k_plant_follow_o): no payload, zeros
template <int RPW, bool MNULL = false>
DEVFN void stage_disturbance_records(const DevState& S, double* rows, int b0, const double* wtab, int wr_stride, const double* mtab, int m_stride) {
  for (int e = threadIdx.x; e < 2 * RPW * h1s::DIST_REC; e += 64) {
    const int r2 = e / h1s::DIST_REC, k = e - r2 * h1s::DIST_REC;
    const int r = r2 < RPW ? r2 : r2 - RPW;
    const int br = b0 + r < S.B ? b0 + r : S.B - 1;      // (a wave's unowned rows read the last rollout's records)
    double v = 0.0;
    if (k < h1s::PAYLOAD_AT) { if (r2 < RPW && wtab) v = wtab[(size_t)br * wr_stride + k]; }
    else if (k < h1s::PAYLOAD_AT + h1s::PAYLOAD_VALS) { if (!MNULL || mtab) v = mtab[(size_t)br * m_stride + (k - h1s::PAYLOAD_AT)]; }
    rows[e] = v;
  }
}
#endif
#ifdef PLANT_PAYLOAD_MODULE
#define PLANT_TABLE 3
#include "plant_follow_body.h"

// ---- one step under a wrench and a payload per item (ilqr_hip_step_payload): k_step_w with the widened row; wrench null: none
#define STEP_M_LDS_BYTES ((h1s::LDS_SLOTS * 64 + 32 * h1s::DIST_REC) * sizeof(double))
template <int CK>
__global__ void __launch_bounds__(64) k_step_m(int count, const double* x, const double* u, DynParams dyn, double* xn, int st_l, int st_r, const double* wrench, const double* payload) {
  extern __shared__ double lds[];
  constexpr int WR0 = h1s::LDS_SLOTS * 64;
  const int i0 = blockIdx.x * 32;
  for (int e = threadIdx.x; e < 32 * h1s::DIST_REC; e += 64) {
    const int r = e / h1s::DIST_REC, k = e - r * h1s::DIST_REC;
    const int ir = i0 + r < count ? i0 + r : count - 1;
    double v = 0.0;
    if (k < h1s::DIST_WRENCH_VALS) { if (wrench) v = wrench[(size_t)ir * h1s::DIST_WRENCH_VALS + k]; }
    else if (k >= h1s::PAYLOAD_AT && k < h1s::PAYLOAD_AT + h1s::PAYLOAD_VALS) v = payload[(size_t)ir * h1s::PAYLOAD_VALS + (k - h1s::PAYLOAD_AT)];
    lds[WR0 + e] = v;
  }
  wave_lds_fence();
  const int i = i0 + ((int)threadIdx.x >> 1);
  const bool side = (threadIdx.x & 1) != 0;
  if (i >= count) return;
  const h1s::LaneLds L{lds, 64, (int)threadIdx.x};
  h1s::HalfX h; h1s::load_half(side, x + (size_t)i * H1_NX, h);
  h1s::HalfU uu; load_half_u(side, u + (size_t)i * H1_NU, uu);
  int st[2] = {st_l, st_r};
  step_any_w<CK>(side, h, uu, dyn, st, L, 0, WR0 + ((int)threadIdx.x >> 1) * h1s::DIST_REC);
  h1s::store_half(side, h, xn + (size_t)i * H1_NX);
}

#endif

#if defined(PLANT_OBSERVE_MODULE) || defined(PLANT_ACTUATOR_MODULE) || defined(PLANT_JOINTS_MODULE) || defined(PLANT_LOWER_FAMILIES)
// ---- observation table (include/ilqr_hip.h ilqr_hip_plant_set_observation): what the controller is told of the state.  One record of
// OBS_REC = 100 doubles per rollout -- bias[50], sigma[50] in the tangent order of the Jacobians (dp, dphi, dq, dv, domega, dqdot) -- or ONE
// record that every rollout reads (stride 0).  The error of rollout b in plant interval i is e = bias + sigma o z(seed, stream0 + b, i),
// laid out as a state-shaped row delta[51] (the rotation vector as a unit quaternion); the measured state is x [+] delta.
//   k_observation_draw  delta[count][B][51] of the intervals interval0 .. interval0 + count - 1: a pure function of its arguments
//   k_observe_apply     out = x [+] delta for B rows (the warm starts' x0, ilqr_hip_plant_get_observed)
//   k_plant_follow_o    plant_follow_body.h a fifth time: the control law on XO = XS [+] delta_j
// observe_entry is the ONE statement of [+]: entry e of the measured row.  Both users compile it in this translation unit under
// -ffp-contract=on, where the front end alone decides what is fused, so the solve's x0 and the law's x agree to the bit.
#define OBS_NT 50
#define OBS_REC 100
DEVFN double observe_entry(const double* x, const double* d, int e) {
  if (e < 3 || e > 6) return x[e] + d[e];
  const double aw = x[3], ax = x[4], ay = x[5], az = x[6], bw = d[3], bx = d[4], by = d[5], bz = d[6];      // Hamilton product, wxyz, not renormalised
  if (e == 3) return aw * bw - ax * bx - ay * by - az * bz;
  if (e == 4) return aw * bx + ax * bw + ay * bz - az * by;
  if (e == 5) return aw * by - ax * bz + ay * bw + az * bx;
  return aw * bz + ax * by - ay * bx + az * bw;
}
// the wave's RPW rows: xs in LDS, the error rows of the interval in memory (rows without a rollout read the last rollout's, as they read its policy)
template <int RPW>
DEVFN void observe_rows(const DevState& S, const double* xs, const double* drow, int b0, double* xo) {
  constexpr int n = PLANT_NX;
  for (int it = threadIdx.x; it < RPW * n; it += 64) {
    const int r = it / n, e = it - r * n;
    const int br = b0 + r < S.B ? b0 + r : S.B - 1;
    xo[it] = observe_entry(xs + r * n, drow + (size_t)br * n, e);
  }
}
#ifdef PLANT_OBSERVE_MODULE
#define PLANT_TABLE 4
#include "plant_follow_body.h"
#endif

// Philox4x32-10, the counter-based generator of the draws below (philox_dev.h: the group kernels share the body)
#include "philox_dev.h"
#endif
#ifdef PLANT_OBSERVE_MODULE
// One lane per (rollout, Philox block): 25 blocks -- counter (stream lo, stream hi, interval lo, block), key (seed lo, seed hi) -- make a
// rollout's 50 normals by Box-Muller, the fp64 log and sincos being the cost.  OBS_RPB rollouts per workgroup of 256 lanes (250 busy); the
// tangent errors and then the state-shaped rows are assembled in LDS and leave in one coalesced run of OBS_RPB x 51 consecutive doubles:
// the rows of one interval are contiguous over the rollouts.  grid (ceil(B / OBS_RPB), count).  Draws are made whatever sigma is.
#define OBS_RPB 10
__global__ void __launch_bounds__(256) k_observation_draw(int B, const double* records, int rec_stride, unsigned long long seed, unsigned long long stream0, long interval0, double* out) {
  __shared__ double er[OBS_RPB * OBS_NT];
  __shared__ double dr[OBS_RPB * PLANT_NX];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * OBS_RPB;
  const int rows = B - b0 < OBS_RPB ? B - b0 : OBS_RPB;
  const unsigned long long iv = (unsigned long long)(interval0 + (long)blockIdx.y);
  const int r = tid / 25, k = tid - r * 25;
  if (r < rows) {
    const unsigned long long s = stream0 + (unsigned long long)(b0 + r);
    unsigned w[4];
    philox4x32_10((unsigned)s, (unsigned)(s >> 32), (unsigned)iv, (unsigned)k, (unsigned)seed, (unsigned)(seed >> 32), w);
    const double u1 = ((double)((((unsigned long long)w[0] << 32) | w[1]) >> 11) + 0.5) * 0x1p-53;
    const double u2 = ((double)((((unsigned long long)w[2] << 32) | w[3]) >> 11) + 0.5) * 0x1p-53;
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    double sn, cs;
    sincos(ang, &sn, &cs);
    const double* rec = records + (size_t)(b0 + r) * rec_stride;
    // (the product rounded on its own, then the sum: no fused multiply-add between a record and its draw)
    const double z0 = rad * cs, z1 = rad * sn;
    const double s0 = rec[OBS_NT + 2 * k] * z0, s1 = rec[OBS_NT + 2 * k + 1] * z1;
    er[r * OBS_NT + 2 * k] = rec[2 * k] + s0;
    er[r * OBS_NT + 2 * k + 1] = rec[2 * k + 1] + s1;
  }
  __syncthreads();
  for (int it = tid; it < rows * PLANT_NX; it += 256) {
    const int rr = it / PLANT_NX, e = it - rr * PLANT_NX;
    const double* ev = er + rr * OBS_NT;
    double v;
    if (e < 3) v = ev[e];
    else if (e > 6) v = ev[e - 1];
    else {
      const double xx = ev[3] * ev[3], yy = ev[4] * ev[4], zz = ev[5] * ev[5];
      const double sum = xx + yy;
      const double th = sqrt(sum + zz);
      if (th == 0.0) v = e == 3 ? 1.0 : 0.0;
      else if (e == 3) v = cos(0.5 * th);
      else { const double f = sin(0.5 * th) / th; v = f * ev[e - 1]; }
    }
    dr[it] = v;
  }
  __syncthreads();
  double* o = out + ((size_t)blockIdx.y * B + b0) * PLANT_NX;
  for (int it = tid; it < rows * PLANT_NX; it += 256) o[it] = dr[it];
}
// out[b] = x[b] [+] delta[b], one lane per entry
__global__ void __launch_bounds__(256) k_observe_apply(int B, const double* x, const double* delta, double* out) {
  const long it = (long)blockIdx.x * 256 + threadIdx.x;
  if (it >= (long)B * PLANT_NX) return;
  const int b = (int)(it / PLANT_NX), e = (int)(it - (long)b * PLANT_NX);
  out[it] = observe_entry(x + (size_t)b * PLANT_NX, delta + (size_t)b * PLANT_NX, e);
}
#endif

#if defined(PLANT_ACTUATOR_MODULE) || defined(PLANT_JOINTS_MODULE) || defined(PLANT_LOWER_FAMILIES)
// ---- actuator table (include/ilqr_hip.h ilqr_hip_plant_set_actuator): what the joints get of the law's command.  One record of ACT_REC = 39
// doubles per rollout -- delay (plant substeps, an integer 0..8), tau[19] (s), sigma[19] (N m) -- or ONE record that every rollout reads
// (stride 0), and beside it the rows beta[19] = -expm1(-h / tau) that the host derived from it.  In substep n (counted from the priming)
// the command c_n -- the law's row US behind the guard of main:162-165 -- becomes
//   a_n = c_{n - delay}                                      a delay line of ACT_SLOTS = 9 slots per rollout: slot n % 9 written, (n - delay) % 9 read
//   y_n = y_{n-1} + beta o (a_n - y_{n-1})                   the product rounded on its own; tau_i == 0: y_i = a_i by selection
//   t_n = y_n + sigma o z                                    z the interval's normals; the product rounded on its own; sigma_i == 0: t_i = y_i by selection
// and t_n is the row UA the step loads.  n == 0 primes: every slot and y take c_0.
//   k_actuator_draw    z[count][B][19] of the intervals interval0 .. interval0 + count - 1: a pure function of its arguments
//   k_plant_follow_a   plant_follow_body.h a sixth time
#define ACT_REC 39
#define ACT_SLOTS 9
// One entry (rollout row r, joint i) per lane and turn, dealt out as control_law deals its rows; an entry belongs to the same lane in every
// substep of a launch, so the lane that wrote a slot of the delay line or y is the one that reads it: program order is all the ordering
// it needs (between launches: the stream).  The rows a wave does not own have no state in memory: they pass the command through.
template <int FB>
DEVFN void actuator_stage(const DevState& S, double* lds, int b0, int ua0, const double* atab, int a_stride, const double* abeta, int ab_stride, const double* zrow, double* fifo, double* yst,
                          double* applied, long nsub, bool last) {
  typedef PlantLayout<FB> Lay;
  constexpr int m = PLANT_NU;
  const int slot_w = (int)(nsub % ACT_SLOTS);
  for (int it = threadIdx.x; it < Lay::RPW * m; it += 64) {
    const int r = it / m, i = it - r * m;
    const double* us = lds + Lay::US + r * m;
    bool fin = true;
    for (int q = 0; q < m; ++q) fin = fin && isfinite(us[q]);
    const double c = fin ? us[i] : 0.0;      // main:162-165: a command with a non-finite entry is zero, all of it
    double t = c;
    if (b0 + r < S.B) {
      const size_t b = (size_t)(b0 + r);
      const double* rec = atab + b * a_stride;
      const int delay = (int)rec[0];
      const double tau = rec[1 + i], sigma = rec[1 + m + i];
      double* f = fifo + b * (ACT_SLOTS * m) + i;
      double* yp = yst + b * m + i;
      double y;
      if (nsub == 0) {      // (wave-uniform) priming: the joint was already holding this torque
        for (int s = 0; s < ACT_SLOTS; ++s) f[s * m] = c;
        y = c;
      } else {
        f[slot_w * m] = c;
        const double a = delay == 0 ? c : f[(int)((nsub - delay + ACT_SLOTS) % ACT_SLOTS) * m];
        if (tau == 0.0) y = a;
        else {
          const double yo = *yp;
          const double d = abeta[b * ab_stride + i] * (a - yo);
          y = yo + d;
        }
      }
      *yp = y;
      const double s = sigma * zrow[b * m + i];
      t = sigma == 0.0 ? y : y + s;
      if (last) applied[b * m + i] = t;
    }
    lds[ua0 + it] = t;
  }
}
#endif
#if defined(PLANT_JOINTS_MODULE) || defined(PLANT_LOWER_FAMILIES)
// ---- joint table (include/ilqr_hip.h ilqr_hip_plant_set_joints): k_plant_follow_j.  One record of h1s::JOINT_REC = 80 doubles (640 B) per rollout --
// gain[19], range scale[19], damping[19], armature[19] in the order of u, four doubles of padding -- or ONE record that every rollout reads
// (j_stride = 0).  Staged in LDS once per launch behind the rows of the actuator family, consecutive lanes on consecutive doubles (20 KB at
// FB = 0, 2.5 KB at FB = 1): ONE copy per rollout, which both disturbance rows of the rollout share.  A substep hands the step the offset of
// the record; the step reads each value where it uses it (h1_aba_split.h stance_prepare_j).
template <int RPW>
DEVFN void stage_joint_records(const DevState& S, double* rows, int b0, const double* jtab, int j_stride) {
  for (int e = threadIdx.x; e < RPW * h1s::JOINT_REC; e += 64) {
    const int r = e / h1s::JOINT_REC;
    const int br = b0 + r < S.B ? b0 + r : S.B - 1;      // (a wave's unowned rows read the last rollout's record)
    rows[e] = jtab[(size_t)br * j_stride + (e - r * h1s::JOINT_REC)];
  }
}
// plant_step_table<KIND, true> with the joint record at LDS offset jro: the scalar gain of the parameter record in front, as there
template <int KIND>
DEVFN void plant_step_table_j(bool side, h1s::HalfX& h, const h1s::HalfU& u, const DynParams& dyn, const int* st, const h1s::LaneLds& L, int geom, const double* rec, int wro, int jro) {
  DynParams dl = dyn;
  dl.g[0] = rec[0]; dl.g[1] = rec[1]; dl.g[2] = rec[2]; dl.mu = rec[3]; dl.soft = rec[4]; dl.lim_k = rec[5];
  const double gain = rec[6];
  h1s::HalfU us;
  us.u11 = gain * u.u11;
#pragma unroll
  for (int q = 0; q < 5; ++q) us.uL[q] = gain * u.uL[q];
#pragma unroll
  for (int q = 0; q < 4; ++q) us.uA[q] = gain * u.uA[q];
  step_any_j<KIND>(side, h, us, dl, st, L, geom, wro, jro);
}
#endif
#ifdef PLANT_JOINTS_MODULE
#define PLANT_TABLE 6
#include "plant_follow_body.h"

// ---- one step under a joint record per item, with an optional wrench and payload (ilqr_hip_step_joints): k_step_m with the record behind the
// widened rows; wrench / payload null: none
#define STEP_J_LDS_BYTES ((h1s::LDS_SLOTS * 64 + 32 * h1s::DIST_REC + 32 * h1s::JOINT_REC) * sizeof(double))
template <int CK>
__global__ void __launch_bounds__(64) k_step_j(int count, const double* x, const double* u, DynParams dyn, double* xn, int st_l, int st_r, const double* wrench, const double* payload,
                                               const double* joints) {
  extern __shared__ double lds[];
  constexpr int WR0 = h1s::LDS_SLOTS * 64, JR0 = WR0 + 32 * h1s::DIST_REC;
  const int i0 = blockIdx.x * 32;
  for (int e = threadIdx.x; e < 32 * h1s::DIST_REC; e += 64) {
    const int r = e / h1s::DIST_REC, k = e - r * h1s::DIST_REC;
    const int ir = i0 + r < count ? i0 + r : count - 1;
    double v = 0.0;
    if (k < h1s::DIST_WRENCH_VALS) { if (wrench) v = wrench[(size_t)ir * h1s::DIST_WRENCH_VALS + k]; }
    else if (k >= h1s::PAYLOAD_AT && k < h1s::PAYLOAD_AT + h1s::PAYLOAD_VALS) { if (payload) v = payload[(size_t)ir * h1s::PAYLOAD_VALS + (k - h1s::PAYLOAD_AT)]; }
    lds[WR0 + e] = v;
  }
  for (int e = threadIdx.x; e < 32 * h1s::JOINT_REC; e += 64) {
    const int r = e / h1s::JOINT_REC, k = e - r * h1s::JOINT_REC;
    const int ir = i0 + r < count ? i0 + r : count - 1;
    lds[JR0 + e] = k < h1s::JOINT_VALS ? joints[(size_t)ir * h1s::JOINT_VALS + k] : 0.0;
  }
  wave_lds_fence();
  const int i = i0 + ((int)threadIdx.x >> 1);
  const bool side = (threadIdx.x & 1) != 0;
  if (i >= count) return;
  const h1s::LaneLds L{lds, 64, (int)threadIdx.x};
  h1s::HalfX h; h1s::load_half(side, x + (size_t)i * H1_NX, h);
  h1s::HalfU uu; load_half_u(side, u + (size_t)i * H1_NU, uu);
  int st[2] = {st_l, st_r};
  step_any_j<CK>(side, h, uu, dyn, st, L, 0, WR0 + ((int)threadIdx.x >> 1) * h1s::DIST_REC, JR0 + ((int)threadIdx.x >> 1) * h1s::JOINT_REC);
  h1s::store_half(side, h, xn + (size_t)i * H1_NX);
}
#endif
#ifdef PLANT_ACTUATOR_MODULE
#define PLANT_TABLE 5
#include "plant_follow_body.h"

// One lane per (rollout, Philox block): the blocks ACT_BLK0 .. ACT_BLK0 + 9 of the rollout's stream -- behind the observation's 0..24, so equal
// seeds do not correlate the two -- make 20 normals by the observation's Box-Muller, of which the first 19 are the joints'.  ACT_RPB rollouts
// per workgroup of 256 lanes (250 busy); the rows are assembled in LDS and leave in one coalesced run of ACT_RPB x 19 consecutive doubles.
// grid (ceil(B / ACT_RPB), count).
#define ACT_RPB 25
#define ACT_BLK 10
#define ACT_BLK0 32
__global__ void __launch_bounds__(256) k_actuator_draw(int B, unsigned long long seed, unsigned long long stream0, long interval0, double* out) {
  __shared__ double zr[ACT_RPB * 2 * ACT_BLK];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * ACT_RPB;
  const int rows = B - b0 < ACT_RPB ? B - b0 : ACT_RPB;
  const unsigned long long iv = (unsigned long long)(interval0 + (long)blockIdx.y);
  const int r = tid / ACT_BLK, q = tid - r * ACT_BLK;
  if (r < rows) {
    const unsigned long long s = stream0 + (unsigned long long)(b0 + r);
    unsigned w[4];
    philox4x32_10((unsigned)s, (unsigned)(s >> 32), (unsigned)iv, (unsigned)(ACT_BLK0 + q), (unsigned)seed, (unsigned)(seed >> 32), w);
    const double u1 = ((double)((((unsigned long long)w[0] << 32) | w[1]) >> 11) + 0.5) * 0x1p-53;
    const double u2 = ((double)((((unsigned long long)w[2] << 32) | w[3]) >> 11) + 0.5) * 0x1p-53;
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    double sn, cs;
    sincos(ang, &sn, &cs);
    zr[r * 2 * ACT_BLK + 2 * q] = rad * cs;
    zr[r * 2 * ACT_BLK + 2 * q + 1] = rad * sn;
  }
  __syncthreads();
  double* o = out + ((size_t)blockIdx.y * B + b0) * PLANT_NU;
  for (int it = tid; it < rows * PLANT_NU; it += 256) {
    const int rr = it / PLANT_NU, i = it - rr * PLANT_NU;
    o[it] = zr[rr * 2 * ACT_BLK + i];
  }
}
#endif

#ifdef PLANT_TERRAIN_MODULE
// ---- terrain table (include/ilqr_hip.h ilqr_hip_plant_set_terrain): k_plant_follow_t.  One record of TERRAIN_REC = 8 doubles (64 B) per rollout --
// z_left, z_right (the floor's height under each foot), edge_x (the height holds for a foot whose ankle-link origin has world x >= edge_x;
// -inf: everywhere), the window [first, end) in plant intervals, three doubles of padding -- or ONE record that every rollout reads (t_stride = 0).
// Staged in LDS once per launch behind the joint rows, consecutive lanes on consecutive doubles (2 KB at FB = 0, 256 B at FB = 1).
template <int RPW>
DEVFN void stage_terrain_records(const DevState& S, double* rows, int b0, const double* ttab, int t_stride) {
  for (int e = threadIdx.x; e < RPW * TERRAIN_REC; e += 64) {
    const int r = e / TERRAIN_REC;
    const int br = b0 + r < S.B ? b0 + r : S.B - 1;      // (a wave's unowned rows read the last rollout's record, as stage_plant_records)
    rows[e] = ttab[(size_t)br * t_stride + (e - r * TERRAIN_REC)];
  }
}
// Stance flags (left, right) of a substep from the pair's own state and the record `rec` in plant interval iv: foot f touches iff
// clearance_f < floor_f, floor_f = z_f while the window is open and the foot's ankle-link origin is at x >= edge_x, else 0.  Each lane asks
// h1s::foot_contact for its own foot at the base height pz - floor_own -- the link heights are sums that start from pz, so lowering the base
// by the floor's height is the test against that floor, and with floor = 0 the subtraction is exact: the decision of h1s::geom_stance -- and
// the pair swaps the answers as geom_stance does (both lanes of the pair must be active).  The ankle's x comes from the chain the height
// comes from: h1s::leg_row2 with row 0 of the pelvis rotation and p_x in the place of row 2 and p_z.
DEVFN void terrain_stance(bool side, const h1s::HalfX& hx, const double* rec, double iv, int& st_left, int& st_right) {
  const double qw = hx.quat[0], qx = hx.quat[1], qy = hx.quat[2], qz = hx.quat[3];
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  const double w = qw / qn, x = qx / qn, y = qy / qn, z = qz / qn;
  double r[3] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)};      // row 0 of the pelvis rotation (h1host quat_R)
  double ax = hx.p[0];
  h1s::leg_row2<0>(side, r, ax, hx.q.thL[0]);
  h1s::leg_row2<1>(side, r, ax, hx.q.thL[1]);
  h1s::leg_row2<2>(side, r, ax, hx.q.thL[2]);
  h1s::leg_row2<3>(side, r, ax, hx.q.thL[3]);
  h1s::leg_row2<4>(side, r, ax, hx.q.thL[4]);
  const bool open = rec[3] <= iv && iv < rec[4];
  const double zf = side ? rec[1] : rec[0];
  const double floor_own = (open && ax >= rec[2]) ? zf : 0.0;
  const bool own = h1s::foot_contact(side, hx.p[2] - floor_own, qw, qx, qy, qz, hx.q.thL[0], hx.q.thL[1], hx.q.thL[2], hx.q.thL[3], hx.q.thL[4]) != 0;
  const bool par = h1s::xch_flag(own);
  st_left = (side ? par : own) ? 1 : 0;
  st_right = (side ? own : par) ? 1 : 0;
}
#define PLANT_TABLE 7
#include "plant_follow_body.h"

// ---- one step on a floor per item (ilqr_hip_step_terrain): k_step_s of dyn_split_kernels.hip behind the decision of terrain_stance -- the 32
// items of a workgroup stage a record each behind the dynamics scratch, z_left, z_right, edge_x of the item under a window that is always
// open -- and the flags it stepped with in stance_out[count][2].  CK 0 / 5 (no stance rows) decide nothing; the C API refuses them.
#define STEP_T_LDS_BYTES ((h1s::LDS_SLOTS * 64 + 32 * TERRAIN_REC) * sizeof(double))
template <int CK>
__global__ void __launch_bounds__(64) k_step_t(int count, const double* x, const double* u, DynParams dyn, double* xn, const double* terrain, int* stance_out) {
  extern __shared__ double lds[];
  constexpr int TR0 = h1s::LDS_SLOTS * 64;
  const int i0 = blockIdx.x * 32;
  for (int e = threadIdx.x; e < 32 * TERRAIN_REC; e += 64) {
    const int r = e / TERRAIN_REC, k = e - r * TERRAIN_REC;
    const int ir = i0 + r < count ? i0 + r : count - 1;
    lds[TR0 + e] = k < 3 ? terrain[(size_t)ir * 3 + k] : k == 4 ? __builtin_inf() : 0.0;
  }
  wave_lds_fence();
  const int i = i0 + ((int)threadIdx.x >> 1);
  const bool side = (threadIdx.x & 1) != 0;
  if (i >= count) return;
  const h1s::LaneLds L{lds, 64, (int)threadIdx.x};
  h1s::HalfX h; h1s::load_half(side, x + (size_t)i * H1_NX, h);
  h1s::HalfU uu; load_half_u(side, u + (size_t)i * H1_NU, uu);
  int st[2] = {1, 1};
  if constexpr (CK >= 1 && CK <= 4) terrain_stance(side, h, lds + TR0 + ((int)threadIdx.x >> 1) * TERRAIN_REC, 0.0, st[0], st[1]);
  step_any<CK>(side, h, uu, dyn, st, L, 0);
  h1s::store_half(side, h, xn + (size_t)i * H1_NX);
  if (!side) { stance_out[2 * (size_t)i] = st[0]; stance_out[2 * (size_t)i + 1] = st[1]; }
}
#endif

// ---- The host side of the followed kernels, ONE of each piece for the eight families.  FAMILY is the PLANT_TABLE the kernel was included
// with; a family is the one below it plus its own rows of LDS and its own kernel arguments, and both are written down that way.
// Dynamic LDS of a workgroup in bytes, term by term as plant_follow_body.h lays the rows out behind FollowLayout.
template <int FAMILY, int FB> static constexpr size_t follow_lds() {
  constexpr int RPW = FollowLayout<FB>::RPW;
  int d = FollowLayout<FB>::DOUBLES;
  if (FAMILY >= 1) d += RPW * PLANT_REC;                  // the parameter records
  if (FAMILY == 2) d += (RPW + 1) * WRENCH_REC;           // the wrench records and the zero row
  if (FAMILY >= 3) d += 2 * RPW * h1s::DIST_REC;          // in their place, two disturbance rows per rollout
  if (FAMILY >= 4) d += RPW * PLANT_NX;                   // the observed rows XO
  if (FAMILY >= 5) d += RPW * PLANT_NU;                   // the applied rows UA
  if (FAMILY >= 6) d += RPW * h1s::JOINT_REC;             // the joint records
  if (FAMILY >= 7) d += RPW * TERRAIN_REC;                // the terrain records
  return d * sizeof(double);
}
// A slip in the sum above is an access outside the workgroup's LDS and not a failing test, so every family's bytes are pinned, {FB 0, FB 1}.
template <int FAMILY> static constexpr bool follow_lds_is(size_t fb0, size_t fb1) { return follow_lds<FAMILY, 0>() == fb0 && follow_lds<FAMILY, 1>() == fb1 && fb0 <= 160 * 1024 && fb1 <= 160 * 1024; }
static_assert(follow_lds_is<0>(76800, 78080) && follow_lds_is<1>(78848, 78336) && follow_lds_is<2>(83072, 78976) && follow_lds_is<3>(91136, 79872), "k_plant_follow .. _m: the workgroup's LDS");
static_assert(follow_lds_is<4>(104192, 81504) && follow_lds_is<5>(109056, 82112) && follow_lds_is<6>(129536, 84672) && follow_lds_is<7>(131584, 84928), "k_plant_follow_o .. _t: the workgroup's LDS");
// the kernel: a compilation holds the library's two families or one module's
template <int FAMILY, int KIND, int FB> static constexpr auto follow_kernel() {
#ifdef PLANT_MODULE
  static_assert(FAMILY == PLANT_FAMILY, "a module holds one family");
  return &PLANT_FOLLOW_KERNEL<KIND, FB>;
#else
  static_assert(FAMILY == 0 || FAMILY == 1, "the library holds the table-free and the parameter family");
  if constexpr (FAMILY == 0) return &k_plant_follow<KIND, FB>;
  else return &k_plant_follow_p<KIND, FB>;
#endif
}
// the kernel arguments behind hist_cap (PLANT_TABLE_PARAMS of plant_follow_body.h)
template <int FAMILY> static auto follow_tail(const PlantCall& c) {
  if constexpr (FAMILY == 0) return std::tuple<>{};
  else {
    const auto below = follow_tail<FAMILY - 1>(c);
    if constexpr (FAMILY == 1) return std::tuple_cat(below, std::make_tuple(c.T.records, c.T.rec_stride));
    else if constexpr (FAMILY == 2) return std::tuple_cat(below, std::make_tuple(c.W.records, c.W.rec_stride, c.W.interval0));
    else if constexpr (FAMILY == 3) return std::tuple_cat(below, std::make_tuple(c.M.records, c.M.rec_stride));
    else if constexpr (FAMILY == 4) return std::tuple_cat(below, std::make_tuple(c.dobs));
    else if constexpr (FAMILY == 5) return std::tuple_cat(below, std::make_tuple(c.A.records, c.A.rec_stride, c.A.blend, c.A.blend_stride, c.A.z, c.A.fifo, c.A.y, c.A.applied, c.A.substep0));
    else if constexpr (FAMILY == 6) return std::tuple_cat(below, std::make_tuple(c.J.records, c.J.rec_stride));
    else return std::tuple_cat(below, std::make_tuple(c.R.records, c.R.rec_stride));
  }
}
template <class... Tail> using follow_kernel_fn = void (*)(DevState, PlantDev, DynParams, const int*, long, int, int, int, int, int, long, long, Tail...);
template <int FAMILY, int KIND, int FB>
static void follow_launch(const DevState& S, const PlantDev& Pl, const DynParams& dyn, const PlantCall& c, hipStream_t st) {
  const dim3 grid((unsigned)((S.B + FollowLayout<FB>::RPW - 1) / FollowLayout<FB>::RPW));
  const PlantFollowArgs& a = c.a;
  std::apply([&](auto... tail) {
    constexpr auto kernel = follow_kernel<FAMILY, KIND, FB>();
    static_assert(std::is_same_v<decltype(kernel), const follow_kernel_fn<decltype(tail)...>>, "follow_tail: not the kernel's argument list");
    hipLaunchKernelGGL(kernel, grid, dim3(64), (follow_lds<FAMILY, FB>()), st, S, Pl, dyn, a.sched, a.sched_stride, a.geom, a.substeps, a.kick, a.first_knot, a.count, a.hist_row0, a.hist_cap, tail...);
  }, follow_tail<FAMILY>(c));
}
template <int FAMILY>
static void launch_follow(const DevState& S, const PlantDev& Pl, const DynParams& dyn, const PlantCall& c, hipStream_t st) {
  with_step_kind(dyn, [&](auto K) {
    if (c.a.feedback_mode) follow_launch<FAMILY, K(), 1>(S, Pl, dyn, c, st);
    else follow_launch<FAMILY, K(), 0>(S, Pl, dyn, c, st);
  });
}
static int lds_attr(const void* kernel, size_t bytes) { return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess; }
template <int FAMILY, int KIND, int FB> static int follow_attr() { return lds_attr((const void*)follow_kernel<FAMILY, KIND, FB>(), follow_lds<FAMILY, FB>()); }
// the LDS attributes of every kernel of this compilation: per step kind its followed kernels at both feedback modes (the library: behind
// the advance of that mode), then its step kernel where it has one.  This is the first use of every kernel in the file, so the order here
// is the order of the kernels in the code object.
#ifndef PLANT_MODULE
template <int KIND, int FB> static int advance_attr() { return lds_attr((const void*)k_plant_advance<KIND, FB>, PlantLayout<FB>::DOUBLES * sizeof(double)); }
int plant_kernels_set_attr() {
#else
static int module_kernels_set_attr() {      // (exported with C linkage, below)
#endif
  int rc = 0;
  for_each_step_kind([&](auto K) {
#ifndef PLANT_MODULE
    rc |= advance_attr<K(), 0>(); rc |= follow_attr<0, K(), 0>(); rc |= advance_attr<K(), 1>(); rc |= follow_attr<0, K(), 1>();
    rc |= follow_attr<1, K(), 0>(); rc |= follow_attr<1, K(), 1>();
#else
    rc |= follow_attr<PLANT_FAMILY, K(), 0>(); rc |= follow_attr<PLANT_FAMILY, K(), 1>();
#endif
#ifdef PLANT_STEP_KERNEL
    rc |= lds_attr((const void*)PLANT_STEP_KERNEL<K()>, PLANT_STEP_LDS_BYTES);
#endif
  });
  return rc;
}
#ifndef PLANT_MODULE
template <int KIND, int FB>
static void plant_launch(const DevState& S, const PlantDev& Pl, const DynParams& dyn, const int* sched, long sched_stride, int geom, int substeps, int kick, long hist_row, hipStream_t st) {
  typedef PlantLayout<FB> Lay;
  const dim3 grid((unsigned)((S.B + Lay::RPW - 1) / Lay::RPW));
  hipLaunchKernelGGL((k_plant_advance<KIND, FB>), grid, dim3(64), Lay::DOUBLES * sizeof(double), st, S, Pl, dyn, sched, sched_stride, geom, substeps, kick, hist_row);
}
void launch_plant_advance(const DevState& S, const PlantDev& Pl, const DynParams& dyn, const int* sched, long sched_stride, int geom, int substeps, int feedback_mode, int kick, long hist_row,
                          hipStream_t st) {
  with_step_kind(dyn, [&](auto K) {
    if (feedback_mode) plant_launch<K(), 1>(S, Pl, dyn, sched, sched_stride, geom, substeps, kick, hist_row, st);
    else plant_launch<K(), 0>(S, Pl, dyn, sched, sched_stride, geom, substeps, kick, hist_row, st);
  });
}
void launch_plant_follow(const DevState& S, const PlantDev& Pl, const DynParams& dyn, const PlantCall& C, hipStream_t st) { launch_follow<0>(S, Pl, dyn, C, st); }
void launch_plant_follow_params(const DevState& S, const PlantDev& Pl, const DynParams& dyn, const PlantCall& C, hipStream_t st) { launch_follow<1>(S, Pl, dyn, C, st); }
#endif

}  // namespace ilqr

// ---- the entry points of a module, C linkage (ilqr_kernels.h): ilqr_<stem>_module_<entry>
#ifdef PLANT_MODULE
#define PLANT_ENTRY_(stem, entry) ilqr_##stem##_module_##entry
#define PLANT_ENTRY_OF(stem, entry) PLANT_ENTRY_(stem, entry)
#define PLANT_ENTRY(entry) PLANT_ENTRY_OF(PLANT_STEM, entry)
extern "C" {
int PLANT_ENTRY(set_attr)() { return ilqr::module_kernels_set_attr(); }
void PLANT_ENTRY(follow)(const ilqr::DevState* S, const ilqr::PlantDev* Pl, const h1::DynParams* dyn, const ilqr::PlantCall* call, hipStream_t st) {
  ilqr::launch_follow<PLANT_FAMILY>(*S, *Pl, *dyn, *call, st);
}
#ifdef PLANT_STEP_TAIL
// one two-lane step per item under explicit stance flags: of (wrench, payload, joints) the kernel takes PLANT_STEP_TAIL
void PLANT_ENTRY(step)(int count, const double* x, const double* u, const h1::DynParams* dyn, double* xn, int stance_l, int stance_r, const double* wrench, const double* payload, const double* joints,
                       hipStream_t st) {
  const dim3 grid((unsigned)((count + 31) / 32));
  ilqr::with_step_kind(*dyn, [&](auto K) { hipLaunchKernelGGL((ilqr::PLANT_STEP_KERNEL<K()>), grid, dim3(64), PLANT_STEP_LDS_BYTES, st, count, x, u, *dyn, xn, stance_l, stance_r, PLANT_STEP_TAIL); });
}
#endif
#ifdef PLANT_TERRAIN_MODULE
void ilqr_terrain_module_step(int count, const double* x, const double* u, const h1::DynParams* dyn, double* xn, const double* terrain, int* stance_out, hipStream_t st) {
  const dim3 grid((unsigned)((count + 31) / 32));
  ilqr::with_step_kind(*dyn, [&](auto K) { hipLaunchKernelGGL((ilqr::k_step_t<K()>), grid, dim3(64), PLANT_STEP_LDS_BYTES, st, count, x, u, *dyn, xn, terrain, stance_out); });
}
#endif
#ifdef PLANT_OBSERVE_MODULE
void ilqr_observe_module_draw(int B, const ilqr::ObservationTable* O, long interval0, int count, double* delta, hipStream_t st) {
  const dim3 grid((unsigned)((B + OBS_RPB - 1) / OBS_RPB), (unsigned)count);
  hipLaunchKernelGGL(ilqr::k_observation_draw, grid, dim3(256), 0, st, B, O->records, O->rec_stride, O->seed, O->stream0, interval0, delta);
}
void ilqr_observe_module_apply(int B, const double* x, const double* delta, double* out, hipStream_t st) {
  const dim3 grid((unsigned)(((long)B * PLANT_NX + 255) / 256));
  hipLaunchKernelGGL(ilqr::k_observe_apply, grid, dim3(256), 0, st, B, x, delta, out);
}
#endif
#ifdef PLANT_ACTUATOR_MODULE
void ilqr_actuator_module_draw(int B, unsigned long long seed, unsigned long long stream0, long interval0, int count, double* z, hipStream_t st) {
  const dim3 grid((unsigned)((B + ACT_RPB - 1) / ACT_RPB), (unsigned)count);
  hipLaunchKernelGGL(ilqr::k_actuator_draw, grid, dim3(256), 0, st, B, seed, stream0, interval0, z);
}
#endif
}
#endif
