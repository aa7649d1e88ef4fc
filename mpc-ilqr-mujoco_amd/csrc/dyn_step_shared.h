// The dynamics step of the two-lane kernels, shared by dyn_split_kernels.hip (rollout, line search, plant step, warm-start step, forward
// differences) and plant_kernels.hip (the device-resident closed-loop plant): the non-inlined constrained steps, step_any<CONTACT> and the
// CONTACT value of a DynParams.  Every translation unit that includes this file compiles its own copy of the non-inlined functions
// (no relocatable device code); build with -ffp-contract=on (csrc/Makefile CONTRACT_ON).
// Include after h1_aba_split.h, h1_foot_contact_dev.h and ilqr_kernels.h, inside namespace ilqr with `using namespace h1`.
#pragma once

// ---- contact row f4 on the two-lane kernels -------------------------------------------------------------------------
// One compiled copy of the stance-constrained step (h1s::step_stance) shared by every kernel of this file: the constraint
// solve (twelve unit-wrench propagations, a 12 x 12 Cholesky) wants the register file to itself, and one machine code for
// the rollout and the line search makes the nominal re-rollout reproduce the accepted candidate bit for bit.
// The constraint-free path (contact mode 0, the headline) keeps its inlined step and is not touched by this.
extern __shared__ double dyn_lds_c[];
__device__ __attribute__((noinline)) void step_stance_shared(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                             double soft, int mode, int st_left, int st_right, double mu, int geom) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  if (geom) h1s::geom_stance(side, h, st_left, st_right);      // (stance source GEOMETRY: the flags of x_t's own feet replace the schedule's)
  h1s::step_stance<false>(side, h, u, dt, grav, L, soft, mode, (side ? st_right : st_left) == 1, (side ? st_left : st_right) == 1, mu);
  *hp = h;
}
// the copy with kinetic friction on sliding feet (contact mode 4), see h1s::stance_correct<KIN>
__device__ __attribute__((noinline)) void step_stance_shared_kin(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                 double soft, int st_left, int st_right, double mu, int geom) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  if (geom) h1s::geom_stance(side, h, st_left, st_right);
  h1s::step_stance<true>(side, h, u, dt, grav, L, soft, 4, (side ? st_right : st_left) == 1, (side ? st_left : st_right) == 1, mu);
  *hp = h;
}
// the step with joint-limit rows (DynParams::limits; h1_aba_split.h "The step with the rows"): only reached when the option is on.
// lim_accelerations is the ONE copy of the constrained accelerations, mask = the hinges it treats as acceleration-prescribed.
struct LimAcc { double qb[6]; h1s::HalfAcc qa; };
template <bool KIN>
__device__ __attribute__((noinline)) void lim_accelerations(const h1s::HalfX* hp, const h1s::HalfU* up, unsigned mask, double dt, double gx, double gy, double gz,
                                                            double soft, int mode, int st_left, int st_right, double mu, double kr, LimAcc* out) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  const h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  double qh[4], R0[9]; h1s::HalfTau tau, add;
  h1s::stance_prepare(side, h, u, qh, R0, tau);
  h1s::apply_lock_mask(side, mask, h.q, dt, kr, tau, add);
  const bool st_own = mode != 0 && (side ? st_right : st_left) == 1, st_par = mode != 0 && (side ? st_left : st_right) == 1;      // (mode 0: no stance rows)
  LimAcc o;
  h1s::stance_accelerations<KIN, true>(side, R0, h, tau, dt, grav, L, soft, mode, st_own, st_par, mu, o.qb, o.qa, &add);
  *out = o;
}
template <bool KIN>
DEVFN void step_lim(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz, double soft, int mode, int st_left, int st_right, double mu, double kr, int geom) {
  const bool side = (threadIdx.x & 1) != 0;
  if (geom) h1s::geom_stance(side, *hp, st_left, st_right);     // (decided once: both passes below run with these flags)
  LimAcc o;
  lim_accelerations<KIN>(hp, up, 0u, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, &o);
  h1s::HalfX h = *hp;
  const unsigned mask = h1s::limit_lock_mask(side, h.q, o.qa, dt, kr);
  const bool any = mask != 0u;
  if (h1s::xch_flag(any) || any) lim_accelerations<KIN>(hp, up, mask, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, &o);      // (the pair runs the recursion together)
  const double qn = sqrt(h.quat[0] * h.quat[0] + h.quat[1] * h.quat[1] + h.quat[2] * h.quat[2] + h.quat[3] * h.quat[3]);
  const double qh[4] = {h.quat[0] / qn, h.quat[1] / qn, h.quat[2] / qn, h.quat[3] / qn};
  h1s::integrate_half(h, qh, o.qb, o.qa, dt);
  *hp = h;
}
__device__ __attribute__((noinline)) void step_stance_shared_lim(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                 double soft, int mode, int st_left, int st_right, double mu, double kr, int geom) {
  step_lim<false>(hp, up, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, geom);
}
__device__ __attribute__((noinline)) void step_stance_shared_kin_lim(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                     double soft, int st_left, int st_right, double mu, double kr, int geom) {
  step_lim<true>(hp, up, dt, gx, gy, gz, soft, 4, st_left, st_right, mu, kr, geom);
}
// ---- joint-limit rows on the constraint-free plant (CONTACT == 5, round 6) ------------------------------------------------------
// With no stance rows the first pass of the step with the rows IS the free step's recursion: it stays inlined, as in the constraint-free
// kernels, and only a lane pair that has a hinge to constrain calls out -- state, controls and the mask cross that call through the
// lane's own LDS column (the dynamics scratch is dead at that point; 44 of its 80 slots), the accelerations come back the same way, so
// the caller keeps no address-taken state (by pointer, the mere presence of such a call cost the constraint-free line search 20 %, round 3).
// Until round 6 this plant ran on CONTACT == 3 -- the shared constrained step, stance code and all: - 19 % on the headline's batch with
// nothing to stop.
DEVFN void lds_put_state(const h1s::LaneLds& L, const h1s::HalfX& h) {
#pragma unroll
  for (int k = 0; k < 3; ++k) L[k] = h.p[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) L[3 + k] = h.quat[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) L[7 + k] = h.vb[k];
  L[13] = h.q.th11; L[14] = h.q.qd11;
#pragma unroll
  for (int k = 0; k < 5; ++k) { L[15 + k] = h.q.thL[k]; L[20 + k] = h.q.qdL[k]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) { L[25 + k] = h.q.thA[k]; L[29 + k] = h.q.qdA[k]; }
}
DEVFN void lds_get_state(const h1s::LaneLds& L, h1s::HalfX& h) {
#pragma unroll
  for (int k = 0; k < 3; ++k) h.p[k] = L[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) h.quat[k] = L[3 + k];
#pragma unroll
  for (int k = 0; k < 6; ++k) h.vb[k] = L[7 + k];
  h.q.th11 = L[13]; h.q.qd11 = L[14];
#pragma unroll
  for (int k = 0; k < 5; ++k) { h.q.thL[k] = L[15 + k]; h.q.qdL[k] = L[20 + k]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) { h.q.thA[k] = L[25 + k]; h.q.qdA[k] = L[29 + k]; }
}
// second pass: the recursion with the hinges of `mask` acceleration-prescribed (no stance rows); in: L[0..32] state, L[33..42] controls,
// L[43] the mask; out: L[0..5] base accelerations, L[6] torso, L[7..11] leg, L[12..15] arm hinge accelerations
__device__ __attribute__((noinline)) void lim_second_pass_lds(double dt, double gx, double gy, double gz, double kr) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h; h1s::HalfU u;
  lds_get_state(L, h);
  u.u11 = L[33];
#pragma unroll
  for (int k = 0; k < 5; ++k) u.uL[k] = L[34 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) u.uA[k] = L[39 + k];
  const unsigned mask = (unsigned)__double_as_longlong(L[43]);
  double qh[4], R0[9]; h1s::HalfTau tau, add;
  h1s::stance_prepare(side, h, u, qh, R0, tau);
  h1s::apply_lock_mask(side, mask, h.q, dt, kr, tau, add);
  double qb[6]; h1s::HalfAcc qa;
  h1s::forward_dynamics<true>(side, R0, h.vb, h.q, tau, h1s::ARMATURE + dt * h1s::DAMPING, grav, L, qb, qa, nullptr, nullptr, &add);
#pragma unroll
  for (int k = 0; k < 6; ++k) L[k] = qb[k];
  L[6] = qa.q11;
#pragma unroll
  for (int k = 0; k < 5; ++k) L[7 + k] = qa.qL[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) L[12 + k] = qa.qA[k];
}
// one step of either kind; `st` = stance flags (left, right) of the knot being stepped
// (compile-time switch: the constraint-free instantiation of a kernel contains no call and no address-taken state -- with a
// run-time branch the mere presence of the call cost the headline's line search 20 %)
DEVFN void pin(double& v) { asm volatile("" : "+v"(v)); }
DEVFN void pin_half(h1s::HalfX& h) {
#pragma unroll
  for (int k = 0; k < 3; ++k) pin(h.p[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) pin(h.quat[k]);
#pragma unroll
  for (int k = 0; k < 6; ++k) pin(h.vb[k]);
  pin(h.q.th11); pin(h.q.qd11);
#pragma unroll
  for (int k = 0; k < 5; ++k) { pin(h.q.thL[k]); pin(h.q.qdL[k]); }
#pragma unroll
  for (int k = 0; k < 4; ++k) { pin(h.q.thA[k]); pin(h.q.qdA[k]); }
}
DEVFN void pin_half_u(h1s::HalfU& u) {
  pin(u.u11);
#pragma unroll
  for (int k = 0; k < 5; ++k) pin(u.uL[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) pin(u.uA[k]);
}
// CONTACT: 0 constraint-free, 1 stance constraints (contact modes 1-3), 2 stance constraints with kinetic friction on sliding feet (mode 4),
// 3 / 4: as 1 / 2 with joint-limit rows (DynParams::limits; 3 also serves the constraint-free plant with them: no stance rows in mode 0).
// Mode 4 has kernels of its own: the private segment of a kernel is the largest frame it can reach, and the constrained kernels lose with
// every kilobyte of it (1.4 -> 1.8 KB per lane: -0.7 % on the contact bench, -> 4 KB: -4 %, same machine code otherwise).
// geom (ProblemDev::stance_geom, wave-uniform): the stance flags come from the feet of x_t (h1_foot_contact_dev.h) instead of `st`; the
// constrained step functions decide, behind their call boundary, so the kernels' own code only gains an argument.  CONTACT 0 / 5 have no
// stance rows and ignore it.
template <int CONTACT>
DEVFN void step_any(bool side, h1s::HalfX& h, const h1s::HalfU& u, const DynParams& dyn, const int* st, const h1s::LaneLds& L, int geom) {
  if constexpr (CONTACT == 5) {
    double dt = dyn.h; asm volatile("" : "+s"(dt));
    h1s::HalfU uo = u;
    pin_half(h); pin_half_u(uo);
    double qh[4], R0[9]; h1s::HalfTau tau;
    h1s::stance_prepare(side, h, uo, qh, R0, tau);
    double qb[6]; h1s::HalfAcc qa;
    h1s::forward_dynamics(side, R0, h.vb, h.q, tau, h1s::ARMATURE + dt * h1s::DAMPING, dyn.g, L, qb, qa);
    const unsigned mask = h1s::limit_lock_mask(side, h.q, qa, dt, dyn.lim_k);
    const bool any = mask != 0u;
    // (inlined in this branch instead, the second pass made a 1.7 KB private segment with 526 spilled registers: measured, dropped)
    if (h1s::xch_flag(any) || any) {      // (the pair runs the recursion together)
      lds_put_state(L, h);
      L[33] = uo.u11;
#pragma unroll
      for (int k = 0; k < 5; ++k) L[34 + k] = uo.uL[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) L[39 + k] = uo.uA[k];
      L[43] = __longlong_as_double((long long)mask);
      lim_second_pass_lds(dt, dyn.g[0], dyn.g[1], dyn.g[2], dyn.lim_k);
#pragma unroll
      for (int k = 0; k < 6; ++k) qb[k] = L[k];
      qa.q11 = L[6];
#pragma unroll
      for (int k = 0; k < 5; ++k) qa.qL[k] = L[7 + k];
#pragma unroll
      for (int k = 0; k < 4; ++k) qa.qA[k] = L[12 + k];
    }
    h1s::integrate_half(h, qh, qb, qa, dt);
    pin_half(h);
  }
  else if constexpr (CONTACT == 4) step_stance_shared_kin_lim(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, st[0], st[1], dyn.mu, dyn.lim_k, geom);
  else if constexpr (CONTACT == 3) step_stance_shared_lim(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, dyn.contact, st[0], st[1], dyn.mu, dyn.lim_k, geom);
  else if constexpr (CONTACT == 2) step_stance_shared_kin(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, st[0], st[1], dyn.mu, geom);
  else if constexpr (CONTACT == 1) step_stance_shared(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, dyn.contact, st[0], st[1], dyn.mu, geom);
  else {
    // (the step size behind an opaque barrier as well: with h a loop invariant the articulated quantities of the chains' leaf
    // bodies -- constants plus the armature term h * damping -- are hoisted out of the knot loop, spilled and reloaded per step)
    double dt = dyn.h; asm volatile("" : "+s"(dt));
    // Opaque boundary around the step: inlined into different kernels the same source is otherwise fused / scheduled together
    // with whatever surrounds it (the feedback law in the line search, plain loads in the rollout), and the re-rollout of an
    // accepted candidate can differ from it in the last bit of a few entries.  With every input and output pinned the step is
    // the same expression graph in every kernel (ilqr_hip_get_adopt_mismatches stays 0; GPU tests).
    h1s::HalfU uo = u;
    pin_half(h); pin_half_u(uo);
    h1s::step(side, h, uo, dt, dyn.g, L);
    pin_half(h);
  }
}

// ---- the same steps under an external wrench on the pelvis (DYN_STEP_WRENCH: plant_kernels.hip alone defines it; k_plant_follow_w and
// k_step_w are the only kernels that reach these copies).  The wrench -- F, T (world), r (pelvis frame), nine doubles -- lives in LDS
// behind the kernel's layout and crosses every call boundary as the offset `wro` of its row from the base of the workgroup's LDS, in
// doubles: the non-inlined steps read it there, next to the dynamics scratch they already address from that base.  Each copy is its
// original with h1s::...<WR = true> in the place of the piece it calls; the originals above keep their text.
// Under DYN_STEP_PAYLOAD as well (the payload module of plant_kernels.hip) the same copies carry the payload of ilqr_hip_plant_set_payload too:
// the row at `wro` is then the widened disturbance row (wrench 0..8, payload from h1s::PAYLOAD_AT), and DYN_WR picks the instantiation.
#ifdef DYN_STEP_WRENCH
#ifdef DYN_STEP_PAYLOAD
#define DYN_WR true, true
#else
#define DYN_WR true
#endif
__device__ __attribute__((noinline)) void step_stance_shared_w(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                               double soft, int mode, int st_left, int st_right, double mu, int geom, int wro) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  if (geom) h1s::geom_stance(side, h, st_left, st_right);
  h1s::step_stance<false, DYN_WR>(side, h, u, dt, grav, L, soft, mode, (side ? st_right : st_left) == 1, (side ? st_left : st_right) == 1, mu, dyn_lds_c + wro);
  *hp = h;
}
__device__ __attribute__((noinline)) void step_stance_shared_kin_w(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                   double soft, int st_left, int st_right, double mu, int geom, int wro) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  if (geom) h1s::geom_stance(side, h, st_left, st_right);
  h1s::step_stance<true, DYN_WR>(side, h, u, dt, grav, L, soft, 4, (side ? st_right : st_left) == 1, (side ? st_left : st_right) == 1, mu, dyn_lds_c + wro);
  *hp = h;
}
template <bool KIN>
__device__ __attribute__((noinline)) void lim_accelerations_w(const h1s::HalfX* hp, const h1s::HalfU* up, unsigned mask, double dt, double gx, double gy, double gz,
                                                              double soft, int mode, int st_left, int st_right, double mu, double kr, int wro, LimAcc* out) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  const h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  double qh[4], R0[9]; h1s::HalfTau tau, add;
  h1s::stance_prepare(side, h, u, qh, R0, tau);
  h1s::apply_lock_mask(side, mask, h.q, dt, kr, tau, add);
  const bool st_own = mode != 0 && (side ? st_right : st_left) == 1, st_par = mode != 0 && (side ? st_left : st_right) == 1;
  LimAcc o;
  h1s::stance_accelerations<KIN, true, DYN_WR>(side, R0, h, tau, dt, grav, L, soft, mode, st_own, st_par, mu, o.qb, o.qa, &add, dyn_lds_c + wro);      // (both passes carry the wrench)
  *out = o;
}
template <bool KIN>
DEVFN void step_lim_w(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz, double soft, int mode, int st_left, int st_right, double mu, double kr, int geom, int wro) {
  const bool side = (threadIdx.x & 1) != 0;
  if (geom) h1s::geom_stance(side, *hp, st_left, st_right);
  LimAcc o;
  lim_accelerations_w<KIN>(hp, up, 0u, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, wro, &o);
  h1s::HalfX h = *hp;
  const unsigned mask = h1s::limit_lock_mask(side, h.q, o.qa, dt, kr);
  const bool any = mask != 0u;
  if (h1s::xch_flag(any) || any) lim_accelerations_w<KIN>(hp, up, mask, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, wro, &o);
  const double qn = sqrt(h.quat[0] * h.quat[0] + h.quat[1] * h.quat[1] + h.quat[2] * h.quat[2] + h.quat[3] * h.quat[3]);
  const double qh[4] = {h.quat[0] / qn, h.quat[1] / qn, h.quat[2] / qn, h.quat[3] / qn};
  h1s::integrate_half(h, qh, o.qb, o.qa, dt);
  *hp = h;
}
__device__ __attribute__((noinline)) void step_stance_shared_lim_w(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                   double soft, int mode, int st_left, int st_right, double mu, double kr, int geom, int wro) {
  step_lim_w<false>(hp, up, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, geom, wro);
}
__device__ __attribute__((noinline)) void step_stance_shared_kin_lim_w(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                       double soft, int st_left, int st_right, double mu, double kr, int geom, int wro) {
  step_lim_w<true>(hp, up, dt, gx, gy, gz, soft, 4, st_left, st_right, mu, kr, geom, wro);
}
// lim_second_pass_lds with the wrench in the pelvis solve of the second pass as well (L[0..43] as there)
__device__ __attribute__((noinline)) void lim_second_pass_lds_w(double dt, double gx, double gy, double gz, double kr, int wro) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h; h1s::HalfU u;
  lds_get_state(L, h);
  u.u11 = L[33];
#pragma unroll
  for (int k = 0; k < 5; ++k) u.uL[k] = L[34 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) u.uA[k] = L[39 + k];
  const unsigned mask = (unsigned)__double_as_longlong(L[43]);
  double qh[4], R0[9]; h1s::HalfTau tau, add;
  h1s::stance_prepare(side, h, u, qh, R0, tau);
  h1s::apply_lock_mask(side, mask, h.q, dt, kr, tau, add);
  double qb[6]; h1s::HalfAcc qa;
  h1s::forward_dynamics<true, DYN_WR>(side, R0, h.vb, h.q, tau, h1s::ARMATURE + dt * h1s::DAMPING, grav, L, qb, qa, nullptr, nullptr, &add, dyn_lds_c + wro);
#pragma unroll
  for (int k = 0; k < 6; ++k) L[k] = qb[k];
  L[6] = qa.q11;
#pragma unroll
  for (int k = 0; k < 5; ++k) L[7 + k] = qa.qL[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) L[12 + k] = qa.qA[k];
}
// step_any under the wrench at LDS offset wro (the comments of step_any hold for every branch)
template <int CONTACT>
DEVFN void step_any_w(bool side, h1s::HalfX& h, const h1s::HalfU& u, const DynParams& dyn, const int* st, const h1s::LaneLds& L, int geom, int wro) {
  if constexpr (CONTACT == 5) {
    double dt = dyn.h; asm volatile("" : "+s"(dt));
    h1s::HalfU uo = u;
    pin_half(h); pin_half_u(uo);
    double qh[4], R0[9]; h1s::HalfTau tau;
    h1s::stance_prepare(side, h, uo, qh, R0, tau);
    double qb[6]; h1s::HalfAcc qa;
    h1s::forward_dynamics<false, DYN_WR>(side, R0, h.vb, h.q, tau, h1s::ARMATURE + dt * h1s::DAMPING, dyn.g, L, qb, qa, nullptr, nullptr, nullptr, L.base + wro);
    const unsigned mask = h1s::limit_lock_mask(side, h.q, qa, dt, dyn.lim_k);
    const bool any = mask != 0u;
    if (h1s::xch_flag(any) || any) {
      lds_put_state(L, h);
      L[33] = uo.u11;
#pragma unroll
      for (int k = 0; k < 5; ++k) L[34 + k] = uo.uL[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) L[39 + k] = uo.uA[k];
      L[43] = __longlong_as_double((long long)mask);
      lim_second_pass_lds_w(dt, dyn.g[0], dyn.g[1], dyn.g[2], dyn.lim_k, wro);
#pragma unroll
      for (int k = 0; k < 6; ++k) qb[k] = L[k];
      qa.q11 = L[6];
#pragma unroll
      for (int k = 0; k < 5; ++k) qa.qL[k] = L[7 + k];
#pragma unroll
      for (int k = 0; k < 4; ++k) qa.qA[k] = L[12 + k];
    }
    h1s::integrate_half(h, qh, qb, qa, dt);
    pin_half(h);
  }
  else if constexpr (CONTACT == 4) step_stance_shared_kin_lim_w(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, st[0], st[1], dyn.mu, dyn.lim_k, geom, wro);
  else if constexpr (CONTACT == 3) step_stance_shared_lim_w(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, dyn.contact, st[0], st[1], dyn.mu, dyn.lim_k, geom, wro);
  else if constexpr (CONTACT == 2) step_stance_shared_kin_w(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, st[0], st[1], dyn.mu, geom, wro);
  else if constexpr (CONTACT == 1) step_stance_shared_w(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, dyn.contact, st[0], st[1], dyn.mu, geom, wro);
  else {
    double dt = dyn.h; asm volatile("" : "+s"(dt));
    h1s::HalfU uo = u;
    pin_half(h); pin_half_u(uo);
    h1s::step<DYN_WR>(side, h, uo, dt, dyn.g, L, L.base + wro);
    pin_half(h);
  }
}
#endif

// ---- the same steps under a joint record per rollout (DYN_STEP_JOINTS: the joints module of plant_kernels.hip alone defines it, with
// DYN_STEP_WRENCH and DYN_STEP_PAYLOAD; k_plant_follow_j and k_step_j are the only kernels that reach these copies).  Each is its `_w` copy
// with the record's torques and per-hinge armature in the place of the model's (h1_aba_split.h stance_prepare_j): every kind runs the PER
// recursion, and a stopped hinge takes LOCK_ARM by selection (apply_lock_mask_j).  The record -- h1s::JOINT_REC doubles -- lives in LDS behind
// the disturbance rows and crosses every call boundary as the offset `jro` of its row, as the disturbance row does as `wro`.  The copies
// above keep their text.
#ifdef DYN_STEP_JOINTS
template <bool KIN>
DEVFN void step_stance_j(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz, double soft, int mode, int st_left, int st_right, double mu, int geom, int wro, int jro) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  if (geom) h1s::geom_stance(side, h, st_left, st_right);
  double qh[4], R0[9]; h1s::HalfTau tau, add;
  h1s::stance_prepare_j(side, h, u, dt, dyn_lds_c + jro, qh, R0, tau, add);
  double qb[6]; h1s::HalfAcc qa;
  h1s::stance_accelerations<KIN, true, DYN_WR>(side, R0, h, tau, dt, grav, L, soft, mode, (side ? st_right : st_left) == 1, (side ? st_left : st_right) == 1, mu, qb, qa, &add, dyn_lds_c + wro);
  h1s::integrate_half(h, qh, qb, qa, dt);
  *hp = h;
}
__device__ __attribute__((noinline)) void step_stance_shared_j(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                               double soft, int mode, int st_left, int st_right, double mu, int geom, int wro, int jro) {
  step_stance_j<false>(hp, up, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, geom, wro, jro);
}
__device__ __attribute__((noinline)) void step_stance_shared_kin_j(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                   double soft, int st_left, int st_right, double mu, int geom, int wro, int jro) {
  step_stance_j<true>(hp, up, dt, gx, gy, gz, soft, 4, st_left, st_right, mu, geom, wro, jro);
}
template <bool KIN>
__device__ __attribute__((noinline)) void lim_accelerations_j(const h1s::HalfX* hp, const h1s::HalfU* up, unsigned mask, double dt, double gx, double gy, double gz,
                                                              double soft, int mode, int st_left, int st_right, double mu, double kr, int wro, int jro, LimAcc* out) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  const h1s::HalfX h = *hp;
  const h1s::HalfU u = *up;
  double qh[4], R0[9]; h1s::HalfTau tau, add;
  h1s::stance_prepare_j(side, h, u, dt, dyn_lds_c + jro, qh, R0, tau, add);
  h1s::apply_lock_mask_j(side, mask, h.q, dt, kr, tau, add);
  const bool st_own = mode != 0 && (side ? st_right : st_left) == 1, st_par = mode != 0 && (side ? st_left : st_right) == 1;
  LimAcc o;
  h1s::stance_accelerations<KIN, true, DYN_WR>(side, R0, h, tau, dt, grav, L, soft, mode, st_own, st_par, mu, o.qb, o.qa, &add, dyn_lds_c + wro);
  *out = o;
}
template <bool KIN>
DEVFN void step_lim_j(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz, double soft, int mode, int st_left, int st_right, double mu, double kr, int geom, int wro, int jro) {
  const bool side = (threadIdx.x & 1) != 0;
  if (geom) h1s::geom_stance(side, *hp, st_left, st_right);
  LimAcc o;
  lim_accelerations_j<KIN>(hp, up, 0u, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, wro, jro, &o);
  h1s::HalfX h = *hp;
  const unsigned mask = h1s::limit_lock_mask(side, h.q, o.qa, dt, kr);
  const bool any = mask != 0u;
  if (h1s::xch_flag(any) || any) lim_accelerations_j<KIN>(hp, up, mask, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, wro, jro, &o);
  const double qn = sqrt(h.quat[0] * h.quat[0] + h.quat[1] * h.quat[1] + h.quat[2] * h.quat[2] + h.quat[3] * h.quat[3]);
  const double qh[4] = {h.quat[0] / qn, h.quat[1] / qn, h.quat[2] / qn, h.quat[3] / qn};
  h1s::integrate_half(h, qh, o.qb, o.qa, dt);
  *hp = h;
}
__device__ __attribute__((noinline)) void step_stance_shared_lim_j(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                   double soft, int mode, int st_left, int st_right, double mu, double kr, int geom, int wro, int jro) {
  step_lim_j<false>(hp, up, dt, gx, gy, gz, soft, mode, st_left, st_right, mu, kr, geom, wro, jro);
}
__device__ __attribute__((noinline)) void step_stance_shared_kin_lim_j(h1s::HalfX* hp, const h1s::HalfU* up, double dt, double gx, double gy, double gz,
                                                                       double soft, int st_left, int st_right, double mu, double kr, int geom, int wro, int jro) {
  step_lim_j<true>(hp, up, dt, gx, gy, gz, soft, 4, st_left, st_right, mu, kr, geom, wro, jro);
}
// lim_second_pass_lds_w under the joint record (L[0..43] as there)
__device__ __attribute__((noinline)) void lim_second_pass_lds_j(double dt, double gx, double gy, double gz, double kr, int wro, int jro) {
  const int lane = threadIdx.x;
  const bool side = (lane & 1) != 0;
  const h1s::LaneLds L{dyn_lds_c, 64, lane};
  const double grav[3] = {gx, gy, gz};
  h1s::HalfX h; h1s::HalfU u;
  lds_get_state(L, h);
  u.u11 = L[33];
#pragma unroll
  for (int k = 0; k < 5; ++k) u.uL[k] = L[34 + k];
#pragma unroll
  for (int k = 0; k < 4; ++k) u.uA[k] = L[39 + k];
  const unsigned mask = (unsigned)__double_as_longlong(L[43]);
  double qh[4], R0[9]; h1s::HalfTau tau, add;
  h1s::stance_prepare_j(side, h, u, dt, dyn_lds_c + jro, qh, R0, tau, add);
  h1s::apply_lock_mask_j(side, mask, h.q, dt, kr, tau, add);
  double qb[6]; h1s::HalfAcc qa;
  h1s::forward_dynamics<true, DYN_WR>(side, R0, h.vb, h.q, tau, h1s::ARMATURE + dt * h1s::DAMPING, grav, L, qb, qa, nullptr, nullptr, &add, dyn_lds_c + wro);
#pragma unroll
  for (int k = 0; k < 6; ++k) L[k] = qb[k];
  L[6] = qa.q11;
#pragma unroll
  for (int k = 0; k < 5; ++k) L[7 + k] = qa.qL[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) L[12 + k] = qa.qA[k];
}
// step_any_w under the joint record at LDS offset jro (the comments of step_any hold for every branch)
template <int CONTACT>
DEVFN void step_any_j(bool side, h1s::HalfX& h, const h1s::HalfU& u, const DynParams& dyn, const int* st, const h1s::LaneLds& L, int geom, int wro, int jro) {
  if constexpr (CONTACT == 5 || CONTACT == 0) {
    double dt = dyn.h; asm volatile("" : "+s"(dt));
    h1s::HalfU uo = u;
    pin_half(h); pin_half_u(uo);
    double qh[4], R0[9]; h1s::HalfTau tau, add;
    h1s::stance_prepare_j(side, h, uo, dt, L.base + jro, qh, R0, tau, add);
    double qb[6]; h1s::HalfAcc qa;
    h1s::forward_dynamics<true, DYN_WR>(side, R0, h.vb, h.q, tau, h1s::ARMATURE + dt * h1s::DAMPING, dyn.g, L, qb, qa, nullptr, nullptr, &add, L.base + wro);
    if constexpr (CONTACT == 5) {
      const unsigned mask = h1s::limit_lock_mask(side, h.q, qa, dt, dyn.lim_k);
      const bool any = mask != 0u;
      if (h1s::xch_flag(any) || any) {
        lds_put_state(L, h);
        L[33] = uo.u11;
#pragma unroll
        for (int k = 0; k < 5; ++k) L[34 + k] = uo.uL[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) L[39 + k] = uo.uA[k];
        L[43] = __longlong_as_double((long long)mask);
        lim_second_pass_lds_j(dt, dyn.g[0], dyn.g[1], dyn.g[2], dyn.lim_k, wro, jro);
#pragma unroll
        for (int k = 0; k < 6; ++k) qb[k] = L[k];
        qa.q11 = L[6];
#pragma unroll
        for (int k = 0; k < 5; ++k) qa.qL[k] = L[7 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) qa.qA[k] = L[12 + k];
      }
    }
    h1s::integrate_half(h, qh, qb, qa, dt);
    pin_half(h);
  }
  else if constexpr (CONTACT == 4) step_stance_shared_kin_lim_j(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, st[0], st[1], dyn.mu, dyn.lim_k, geom, wro, jro);
  else if constexpr (CONTACT == 3) step_stance_shared_lim_j(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, dyn.contact, st[0], st[1], dyn.mu, dyn.lim_k, geom, wro, jro);
  else if constexpr (CONTACT == 2) step_stance_shared_kin_j(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, st[0], st[1], dyn.mu, geom, wro, jro);
  else step_stance_shared_j(&h, &u, dyn.h, dyn.g[0], dyn.g[1], dyn.g[2], dyn.soft, dyn.contact, st[0], st[1], dyn.mu, geom, wro, jro);
}
#endif

#define DYN_LDS_BYTES_S (h1s::LDS_SLOTS * 64 * sizeof(double))
DEVFN void load_half_u(bool side, const double* u, h1s::HalfU& o) {
  o.u11 = u[10];
#pragma unroll
  for (int k = 0; k < 5; ++k) o.uL[k] = u[h1s::jleg(side, k)];
#pragma unroll
  for (int k = 0; k < 4; ++k) o.uA[k] = u[h1s::jarm(side, k)];
}
// CONTACT / CK / KIND of the kernels: the StepKind of the dynamics parameters (launch_plan.h, where the six values have their names)
static inline int step_kind(const DynParams& d) { return step_kind_of(d.contact, d.limits); }
// f(std::integral_constant<int, K>{}) for K = step_kind(d): the ONE place that turns the run-time kind into a template argument; a launcher
// names its kernel as k<K()> inside a generic lambda
template <class F> static inline void with_step_kind(const DynParams& d, F&& f) {
  switch (step_kind(d)) {
    case STEP_LIMITS: f(std::integral_constant<int, STEP_LIMITS>{}); break;
    case STEP_KINETIC_LIMITS: f(std::integral_constant<int, STEP_KINETIC_LIMITS>{}); break;
    case STEP_STANCE_LIMITS: f(std::integral_constant<int, STEP_STANCE_LIMITS>{}); break;
    case STEP_KINETIC: f(std::integral_constant<int, STEP_KINETIC>{}); break;
    case STEP_STANCE: f(std::integral_constant<int, STEP_STANCE>{}); break;
    default: f(std::integral_constant<int, STEP_FREE>{});
  }
}
// f with every kind: the attribute lists (a kernel of the family that is launched by kind is listed here once, for all six)
template <class F> static inline void for_each_step_kind(F&& f) {
  f(std::integral_constant<int, STEP_FREE>{}); f(std::integral_constant<int, STEP_STANCE>{}); f(std::integral_constant<int, STEP_KINETIC>{});
  f(std::integral_constant<int, STEP_STANCE_LIMITS>{}); f(std::integral_constant<int, STEP_KINETIC_LIMITS>{}); f(std::integral_constant<int, STEP_LIMITS>{});
}
