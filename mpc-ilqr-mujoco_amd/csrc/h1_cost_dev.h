// Device-side cost terms of the H1 iLQR (fp64, gfx950).
//
// Replaces, without a symbolic engine on the GPU,
//   iLQR::computeTotalCost          reference src/ilqr/ilqr.cpp:363-518
//   iLQR::computeCostQuadratics     reference src/ilqr/ilqr.cpp:133-244
//   iLQR::add*CostDerivatives       reference src/ilqr/ilqr.cpp:662-800
//   symDerivatives::sym*            reference src/common/derivatives.cpp:525-707 (CasADi gradients and
//                                   exact Hessians of Pinocchio quantities)
//   RobotUtils::constraint*         reference src/common/robot_utils.cpp:615-778
//
// The six task terms are functions of a mass-normalised point set S attached to the URDF tree:
//   c(q)     = mfrac p + R(quat) beta(theta)          (whole-body CoM, or an ankle origin)
//   cdot(q,v)= R(quat) gamma(theta, v)                (its velocity, Pinocchio velocity convention)
// with, per hinge j (all in the pelvis frame): axis z_j, origin p_j, r_j = hsub_j - msub_j p_j,
//   w_j = z_j x r_j = d beta/d theta_j,  Om_j = body angular velocity,  s_j = sum_{k below j} qd_k w_k.
// Every gradient/Hessian entry is then a closed form in these vectors (derivation in DESIGN.md):
//   d2 beta/d theta_a d theta_b = z_lo x w_hi for related joints (lo = ancestor-or-self), else 0
//   d gamma/d theta_k           = Om_k x w_k + z_k x s_k
//   d2 gamma/d theta_a d theta_b= Om_lo x (z_lo x w_hi) + z_lo x ((Om_hi - Om_lo) x w_hi) + z_lo x (z_hi x s_hi)
// Quaternion slots use R = Eigen's toRotationMatrix polynomial on the raw (x,y,z,w) coefficients and
// the reference's slot conventions (permuted state in, un-permuted slots out).
#pragma once
#include "al_plan.h"
#include "h1_dynamics_dev.h"

namespace h1 {

struct ProblemDev {
  int N;
  int stance_geom;           // stance source of the DYNAMICS: 0 the schedule (`stance` below), 1 the feet of x_t (h1_foot_contact_dev.h; the cost
                             // keeps reading `stance`).  Sits in what was padding: the layout of the rest (kernel arguments) does not move
  DynParams dyn;
  double Q[H1_NX], R[H1_NU], Qf[H1_NX];
  double w_com, w_com_vel, w_ee_pos, w_ee_vel, w_upright, w_balance, w_joint, w_ctrl;
  // reference sets: stride 0 when shared by all rollouts
  const double* x_ref;       long x_ref_stride;        // [(N+1)*51]
  const double* u_ref;       long u_ref_stride;        // [N*19]
  const double* com_ref;     long com_ref_stride;      // [(N+1)*3]
  const int* stance;         long stance_stride;       // [(N+1)*2]
  const double* ee_ref;      long ee_ref_stride;       // [(N+1)*2*3]
  const double* com_vel_ref; long com_vel_ref_stride;  // [(N+1)*3]
  // per-rollout weight sets (ilqr_hip_set_weight_sets): null = the shared Q ... w_ctrl above; else one WS_STRIDE record per set, stride 0
  // when one set serves every rollout.  Appended: nothing above moves
  const double* wsets;       long wsets_stride;
  // augmented-Lagrangian joint and torque limits (ilqr_hip_set_augmented_lagrangian): null = the plain penalties w_joint / w_ctrl; else the
  // multiplier store, one record of al_stride doubles per rollout (layout below), and the margin fraction of the bounds.  Appended: nothing above moves
  const double* al;          long al_stride;
  double al_margin;
  // per-rollout bounds of those limits (ilqr_hip_set_al_bounds): null = the model's ranges shrunk by al_margin; else one ALB_STRIDE record per
  // set (layout below), stride 0 when one record serves every rollout, and al_margin is not read.  Appended: nothing above moves
  const double* alb;         long alb_stride;
  // augmented-Lagrangian bounds on the other 28 non-quaternion state coordinates (ilqr_hip_set_al_state_bounds): alsb null = none; else als
  // the second multiplier store, one record of als_stride doubles per rollout, and alsb one ALSB_STRIDE record of bounds per set, stride 0
  // when one record serves every rollout (layouts below).  Read while `al` is installed only.  Appended: nothing above moves
  const double* als;         long als_stride;
  const double* alsb;        long alsb_stride;
  // bounds that change from knot to knot (ilqr_hip_set_al_knot_bounds, ilqr_hip_set_al_state_knot_bounds, ilqr_hip_al_bounds_window_from_track):
  // 0 = one record per set as above; else alb / alsb point at windows, [N+1] records per set, knot-major, knot t's record alb_knot / alsb_knot
  // doubles behind knot 0's (ALB_STRIDE / ALSB_STRIDE) and alb_stride / alsb_stride the doubles of one set's window (0: one window for all).
  // Both are set or both are 0 while a state family is installed (al_plan.h).  Appended: nothing above moves
  long alb_knot, alsb_knot;
  // augmented-Lagrangian bounds on the CoM and the two ankle origins, the task family (ilqr_hip_set_al_task_bounds; al_task_dev.h states the
  // layouts): altb null = none; else alt the third multiplier store, one record of alt_stride doubles per rollout, and altb a window of bounds,
  // [N+1] rows per set altb_knot doubles apart, altb_stride the doubles of one set's window (0: one window for all).  While it is installed the
  // other families read windows too (al_plan.h).  Read while `al` is installed only.  Appended: nothing above moves
  const double* alt;         long alt_stride;
  const double* altb;        long altb_stride, altb_knot;
};
// The multiplier store, in doubles.  Rollout b's record: one 128-byte line of scalars (AL_RHO_JOINT, AL_RHO_CTRL, the rest padding), then one
// record of AL_KNOT = 80 doubles (five whole lines) per knot t = 0..N: the hinges' multipliers of the lower bounds, of the upper bounds, two
// doubles of padding, then the same for the actuators (zeros at t = N).  Knot-major, because k_cost_quadratics reads one knot per workgroup
// with lane = coordinate (two 152-byte runs per wave) and k_traj_knot_cost one knot per lane, each lane using every byte of its knot's five
// lines; the eight candidates of a rollout read the same lines.
enum { AL_RHO_JOINT = 0, AL_RHO_CTRL = 1, AL_HDR = 16, AL_JLO = 0, AL_JHI = H1_NJ, AL_ULO = 40, AL_UHI = 40 + H1_NU, AL_KNOT = 80 };
static_assert(H1_NJ == 19 && H1_NU == 19 && AL_JHI + H1_NJ <= AL_ULO && AL_UHI + H1_NU <= AL_KNOT && AL_KNOT % 16 == 0 && AL_HDR % 16 == 0, "multiplier record: whole 128-byte lines");
inline long al_record_doubles(int N) { return AL_HDR + (long)AL_KNOT * (N + 1); }
// The bounds table, in doubles.  One record per set: the hinges' lower bounds, their upper bounds, the actuators' lower bounds, their upper
// bounds (the order of ilqr_hip_set_al_bounds), padded to five whole 128-byte lines.  Indexed by the rollout b, never by a position in a
// compacted list.  A lower bound may be -inf, an upper bound +inf: the kernels form q - hi, lo - q and mu + rho c only (rho is finite and
// positive), so c = -inf, max(0, mu + rho c) = 0 and no 0 * inf or inf - inf arises.
enum { ALB_JLO = 0, ALB_JHI = H1_NJ, ALB_ULO = 2 * H1_NJ, ALB_UHI = 2 * H1_NJ + H1_NU, ALB_FIELDS = 2 * H1_NJ + 2 * H1_NU, ALB_STRIDE = (ALB_FIELDS + 15) / 16 * 16 };
static_assert(ALB_FIELDS == 76 && ALB_STRIDE == 80, "bounds record: 76 doubles in five 128-byte lines");
// The state family: box coordinate k in [0, 28) is state slot k (pelvis position) for k < 3, else slot 23 + k (pelvis linear and angular
// velocity 26..31, joint velocities 32..50).  Its multiplier store, in doubles: rollout b's record is one 128-byte line of scalars (ALS_RHO,
// the rest padding), then one record of ALS_KNOT = 64 doubles (four whole lines) per knot t = 0..N: the multipliers of the 28 lower bounds, of
// the 28 upper bounds, eight doubles of padding.  Knot-major as the store above, for the same two readers.  Its bounds table: one record per
// set, lo[28] then hi[28] (the order of ilqr_hip_set_al_state_bounds) padded to four lines, indexed by the rollout b; -inf / +inf as above.
enum { ALS_COORDS = 28, ALS_RHO = 0, ALS_HDR = 16, ALS_LO = 0, ALS_HI = ALS_COORDS, ALS_KNOT = 64 };
enum { ALSB_LO = 0, ALSB_HI = ALS_COORDS, ALSB_FIELDS = 2 * ALS_COORDS, ALSB_STRIDE = (ALSB_FIELDS + 15) / 16 * 16 };
static_assert(ALS_HI + ALS_COORDS <= ALS_KNOT && ALS_KNOT % 16 == 0 && ALS_HDR % 16 == 0 && ALSB_STRIDE == 64, "state records: whole 128-byte lines");
static_assert(H1_NX == 51 && H1_NQ == 26, "box coordinates: slots 0..2 and 26..50");
inline long als_record_doubles(int N) { return ALS_HDR + (long)ALS_KNOT * (N + 1); }
constexpr int als_slot(int k) { return k < 3 ? k : 23 + k; }
// The AL template axis (AL_OFF .. AL_KNOT_TABLE_STATE) and which of its values a handle's installation selects: al_plan.h.  A template axis,
// so that the paths without a table keep their machine code, and instantiations of their own per knot, so that the four others keep theirs.
constexpr bool al_table(int AL) { return AL == AL_TABLE || AL == AL_TABLE_STATE || AL == AL_KNOT_TABLE || AL == AL_KNOT_TABLE_STATE; }
constexpr bool al_state(int AL) { return AL == AL_TABLE_STATE || AL == AL_KNOT_TABLE_STATE; }
constexpr bool al_per_knot(int AL) { return AL == AL_KNOT_TABLE || AL == AL_KNOT_TABLE_STATE; }
// Bounds lo = r0 + m (r1 - r0), hi = r1 - m (r1 - r0), each operation rounded once (no contraction): every kernel and the host restatement
// of the tests then hold the same two doubles
DEVFN void al_bounds(const double* range, double m, double& lo, double& hi) {
#pragma clang fp contract(off)
  const double d = range[1] - range[0];
  const double mg = m * d;
  lo = range[0] + mg; hi = range[1] - mg;
}
// One constraint c <= 0 with multiplier mu >= 0 and penalty rho > 0: phi = (max(0, mu + rho c)^2 - mu^2) / (2 rho); its gradient with
// respect to c is max(0, mu + rho c), its second derivative rho where that is positive (exact: c is linear in the coordinate)
// (al_phi2 is 2 rho phi: a family's terms share rho, so their sum is divided once -- an fp64 division is ~30 instructions, and a knot has 76 terms)
DEVFN double al_phi2(double c, double mu, double rho) {
  const double s = mu + rho * c;
  const double sp = s > 0.0 ? s : 0.0;
  return sp * sp - mu * mu;
}
// the two families' terms of knot t of rollout b (x: the knot's state, u: its control), in the order of joint_penalty / ctrl_penalty
template <int AL>
DEVFN double al_joint_term(const ProblemDev& P, int b, int t, const double* x) {
  const double* r = P.al + (long)b * P.al_stride;
  const double* bd = P.alb + (long)b * P.alb_stride;      // (AL_TABLE only)
  if constexpr (al_per_knot(AL)) bd += (long)t * P.alb_knot;
  const double rho = r[AL_RHO_JOINT];
  const double* k = r + AL_HDR + (long)t * AL_KNOT;
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < H1_NJ; ++i) {
    double lo, hi;
    if constexpr (al_table(AL)) { lo = bd[ALB_JLO + i]; hi = bd[ALB_JHI + i]; } else al_bounds(H1_JRANGE[i], P.al_margin, lo, hi);
    const double q = x[7 + i];
    c += al_phi2(q - hi, k[AL_JHI + i], rho);
    c += al_phi2(lo - q, k[AL_JLO + i], rho);
  }
  return c / (2.0 * rho);
}
template <int AL>
DEVFN double al_ctrl_term(const ProblemDev& P, int b, int t, const double* u) {
  const double* r = P.al + (long)b * P.al_stride;
  const double* bd = P.alb + (long)b * P.alb_stride;      // (AL_TABLE only)
  if constexpr (al_per_knot(AL)) bd += (long)t * P.alb_knot;
  const double rho = r[AL_RHO_CTRL];
  const double* k = r + AL_HDR + (long)t * AL_KNOT;
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < H1_NU; ++i) {
    double lo, hi;
    if constexpr (al_table(AL)) { lo = bd[ALB_ULO + i]; hi = bd[ALB_UHI + i]; } else al_bounds(H1_CTRLRANGE[i], P.al_margin, lo, hi);
    c += al_phi2(u[i] - hi, k[AL_UHI + i], rho);
    c += al_phi2(lo - u[i], k[AL_ULO + i], rho);
  }
  return c / (2.0 * rho);
}
// the state family's terms of knot t of rollout b, every knot (the terminal one included); added to the knot cost by a kernel of its own
// (dyn_kernels.hip k_al_state_knot_cost), not by knot_cost_w.  KNOT: the bounds are row t of rollout b's window
template <bool KNOT = false>
DEVFN double al_state_term(const ProblemDev& P, int b, int t, const double* x) {
  const double* r = P.als + (long)b * P.als_stride;
  const double* bd = P.alsb + (long)b * P.alsb_stride;
  if constexpr (KNOT) bd += (long)t * P.alsb_knot;
  const double rho = r[ALS_RHO];
  const double* k = r + ALS_HDR + (long)t * ALS_KNOT;
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < ALS_COORDS; ++i) {
    const double v = x[als_slot(i)];
    c += al_phi2(v - bd[ALSB_HI + i], k[ALS_HI + i], rho);
    c += al_phi2(bd[ALSB_LO + i] - v, k[ALS_LO + i], rho);
  }
  return c / (2.0 * rho);
}
// Record of one weight set, in doubles: every weight the cost reads, padded to whole 128-byte lines (129 fields -> 9 lines)
enum { WS_Q = 0, WS_QF = WS_Q + H1_NX, WS_R = WS_QF + H1_NX, WS_TASK = WS_R + H1_NU /* order of ilqr_hip_set_task_weights */, WS_W_JOINT = WS_TASK + 6, WS_W_CTRL = WS_W_JOINT + 1,
       WS_FIELDS = WS_W_CTRL + 1, WS_STRIDE = (WS_FIELDS + 15) / 16 * 16 };
// The one place a cost kernel takes a weight from: WS = false the shared values in the kernel argument, WS = true rollout b's record
template <bool WS> struct CostWeights {
  const double* w;           // rollout b's record (WS only); the shared values are read from the caller's own P
  DEVFN CostWeights(const ProblemDev& P, int b) : w(WS ? P.wsets + (long)b * P.wsets_stride : nullptr) {}
  DEVFN const double* Qd(const ProblemDev& P, bool term) const { if constexpr (WS) return w + (term ? WS_QF : WS_Q); else return term ? P.Qf : P.Q; }
  DEVFN double R(const ProblemDev& P, int i) const { if constexpr (WS) return w[WS_R + i]; else return P.R[i]; }
  DEVFN double w_com(const ProblemDev& P) const { if constexpr (WS) return w[WS_TASK + 0]; else return P.w_com; }
  DEVFN double w_com_vel(const ProblemDev& P) const { if constexpr (WS) return w[WS_TASK + 1]; else return P.w_com_vel; }
  DEVFN double w_ee_pos(const ProblemDev& P) const { if constexpr (WS) return w[WS_TASK + 2]; else return P.w_ee_pos; }
  DEVFN double w_ee_vel(const ProblemDev& P) const { if constexpr (WS) return w[WS_TASK + 3]; else return P.w_ee_vel; }
  DEVFN double w_upright(const ProblemDev& P) const { if constexpr (WS) return w[WS_TASK + 4]; else return P.w_upright; }
  DEVFN double w_balance(const ProblemDev& P) const { if constexpr (WS) return w[WS_TASK + 5]; else return P.w_balance; }
  DEVFN double w_joint(const ProblemDev& P) const { if constexpr (WS) return w[WS_W_JOINT]; else return P.w_joint; }
  DEVFN double w_ctrl(const ProblemDev& P) const { if constexpr (WS) return w[WS_W_CTRL]; else return P.w_ctrl; }
};

DEVFN void limit_bounds(const double* range, double& lo, double& hi) {
  const double margin = 0.1 * (range[1] - range[0]);
  lo = range[0] + margin; hi = range[1] - margin;
}
template <class W> DEVFN double joint_penalty(const ProblemDev& P, const W& Wt, const double* x) {
  double c = 0.0;
  for (int i = 0; i < H1_NJ; ++i) {
    double lo, hi; limit_bounds(H1_JRANGE[i], lo, hi);
    const double q = x[7 + i];
    if (q > hi) { const double v = q - hi; c += Wt.w_joint(P) * v * v; }
    if (q < lo) { const double v = lo - q; c += Wt.w_joint(P) * v * v; }
  }
  return c;
}
template <class W> DEVFN double ctrl_penalty(const ProblemDev& P, const W& Wt, const double* u) {
  double c = 0.0;
  for (int i = 0; i < H1_NU; ++i) {
    double lo, hi; limit_bounds(H1_CTRLRANGE[i], lo, hi);
    if (u[i] > hi) { const double v = u[i] - hi; c += Wt.w_ctrl(P) * v * v; }
    if (u[i] < lo) { const double v = lo - u[i]; c += Wt.w_ctrl(P) * v * v; }
  }
  return c;
}
DEVFN bool support_point(const ProblemDev& P, int b, int t, double* ps) {
  const int* st = P.stance + b * P.stance_stride + 2 * t;
  const double* ee = P.ee_ref + b * P.ee_ref_stride + t * 6;
  const bool L = st[0] == 1, Rt = st[1] == 1;
  if (L && Rt) { ps[0] = 0.5 * (ee[0] + ee[3]); ps[1] = 0.5 * (ee[1] + ee[4]); return true; }
  if (L) { ps[0] = ee[0]; ps[1] = ee[1]; return true; }
  if (Rt) { ps[0] = ee[3]; ps[1] = ee[4]; return true; }
  return false;
}
// one knot of computeTotalCost (ilqr.cpp:370-443 / 447-510) including its share of the penalties (512-515)
// AL: AL_MODEL / AL_TABLE the augmented-Lagrangian terms of the installed multipliers in place of the two plain penalties
template <bool WS, int AL = AL_OFF, class ComFn>
DEVFN double knot_cost_w(const ProblemDev& P, int b, int t, const double* x, const double* u /*null at t==N*/, ComFn com_fn) {
  const CostWeights<WS> Wt(P, b);
  const bool term = (t == P.N);
  const double* xr = P.x_ref + b * P.x_ref_stride + t * H1_NX;
  const double* Qd = Wt.Qd(P, term);
  double a = 0.0;
  for (int i = 0; i < H1_NX; ++i) { const double e = x[i] - xr[i]; a += e * Qd[i] * e; }
  double c = 0.5 * a;
  if (!term) {
    const double* ur = P.u_ref + b * P.u_ref_stride + t * H1_NU;
    double s = 0.0;
    for (int i = 0; i < H1_NU; ++i) { const double e = u[i] - ur[i]; s += e * Wt.R(P, i) * e; }
    c += 0.5 * s;
  }
  if (Wt.w_upright(P) > 0.0) {
    const double qw = x[3], qx = x[4], qy = x[5], qz = x[6];
    const double zx = 2.0 * (qx * qz + qw * qy), zy = 2.0 * (qy * qz - qw * qx), zz = 1.0 - 2.0 * (qx * qx + qy * qy);
    c += 0.5 * Wt.w_upright(P) * (zx * zx + zy * zy + (zz - 1.0) * (zz - 1.0));
  }
  if (Wt.w_balance(P) > 0.0) {
    double ps[2];
    if (support_point(P, b, t, ps)) {
      double com[3]; com_fn(x, com);
      const double om = sqrt(com[2] / 9.81);
      const double rx = com[0] + x[H1_NQ] * om - ps[0], ry = com[1] + x[H1_NQ + 1] * om - ps[1];
      c += 0.5 * Wt.w_balance(P) * (rx * rx + ry * ry);
    }
  }
  if constexpr (AL != AL_OFF) {
    c += al_joint_term<AL>(P, b, t, x);
    if (!term) c += al_ctrl_term<AL>(P, b, t, u);
  } else {
    c += joint_penalty(P, Wt, x);
    if (!term) c += ctrl_penalty(P, Wt, u);
  }
  return c;
}
template <class ComFn>
DEVFN double knot_cost_t(const ProblemDev& P, int b, int t, const double* x, const double* u, ComFn com_fn) { return knot_cost_w<false, AL_OFF>(P, b, t, x, u, com_fn); }
// The terms of knot_cost_w<false> at a NON-terminal knot, one by one, under the shared weights of P (a caller with weights of its own
// passes a copy of P that holds them): out[0] state, [1] control, [2] upright, [3] balance, [4] joint-limit penalty, [5] control-limit
// penalty -- the same expressions in the same order of operations, so that their sum is knot_cost_w's value up to its own additions
// (csrc/plant_score_kernels.hip; include/ilqr_hip.h ILQR_PLANT_SCORE_TERMS)
template <class ComFn>
DEVFN void knot_cost_terms(const ProblemDev& P, int b, int t, const double* x, const double* u, ComFn com_fn, double* out) {
  const CostWeights<false> Wt(P, b);
  const double* xr = P.x_ref + b * P.x_ref_stride + t * H1_NX;
  const double* Qd = Wt.Qd(P, false);
  double a = 0.0;
  for (int i = 0; i < H1_NX; ++i) { const double e = x[i] - xr[i]; a += e * Qd[i] * e; }
  out[0] = 0.5 * a;
  const double* ur = P.u_ref + b * P.u_ref_stride + t * H1_NU;
  double s = 0.0;
  for (int i = 0; i < H1_NU; ++i) { const double e = u[i] - ur[i]; s += e * Wt.R(P, i) * e; }
  out[1] = 0.5 * s;
  out[2] = 0.0;
  if (Wt.w_upright(P) > 0.0) {
    const double qw = x[3], qx = x[4], qy = x[5], qz = x[6];
    const double zx = 2.0 * (qx * qz + qw * qy), zy = 2.0 * (qy * qz - qw * qx), zz = 1.0 - 2.0 * (qx * qx + qy * qy);
    out[2] = 0.5 * Wt.w_upright(P) * (zx * zx + zy * zy + (zz - 1.0) * (zz - 1.0));
  }
  out[3] = 0.0;
  if (Wt.w_balance(P) > 0.0) {
    double ps[2];
    if (support_point(P, b, t, ps)) {
      double com[3]; com_fn(x, com);
      const double om = sqrt(com[2] / 9.81);
      const double rx = com[0] + x[H1_NQ] * om - ps[0], ry = com[1] + x[H1_NQ + 1] * om - ps[1];
      out[3] = 0.5 * Wt.w_balance(P) * (rx * rx + ry * ry);
    }
  }
  out[4] = joint_penalty(P, Wt, x);
  out[5] = ctrl_penalty(P, Wt, u);
}
struct ComLoop { DEVFN void operator()(const double* x, double* com) const { com_mj(x, com); } };
__device__ inline double knot_cost(const ProblemDev& P, int b, int t, const double* x, const double* u) { return knot_cost_t(P, b, t, x, u, ComLoop()); }

// ------------------------------------------------------------------ closed-form task-term quadratics
DEVFN double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
DEVFN void cross(const double* a, const double* b, double* c) { cross3(a, b, c); }

// dR/dquat_k (k over x,y,z,w) of Eigen's toRotationMatrix polynomial, linear in q
DEVFN void dR_dquat(int k, const double* q, double* D) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  if (k == 0) { D[0] = 0; D[1] = 2 * y; D[2] = 2 * z; D[3] = 2 * y; D[4] = -4 * x; D[5] = -2 * w; D[6] = 2 * z; D[7] = 2 * w; D[8] = -4 * x; }
  else if (k == 1) { D[0] = -4 * y; D[1] = 2 * x; D[2] = 2 * w; D[3] = 2 * x; D[4] = 0; D[5] = 2 * z; D[6] = -2 * w; D[7] = 2 * z; D[8] = -4 * y; }
  else if (k == 2) { D[0] = -4 * z; D[1] = -2 * w; D[2] = 2 * x; D[3] = 2 * w; D[4] = -4 * z; D[5] = 2 * y; D[6] = 2 * x; D[7] = 2 * y; D[8] = 0; }
  else { D[0] = 0; D[1] = -2 * z; D[2] = 2 * y; D[3] = 2 * z; D[4] = 0; D[5] = -2 * x; D[6] = -2 * y; D[7] = 2 * x; D[8] = 0; }
}
DEVFN void d2R_dquat2(int k, int l, double* D) { double e[4] = {0, 0, 0, 0}; e[l] = 1.0; dR_dquat(k, e, D); }

struct PointSetDev {
  double beta[3], gamma[3], mfrac;
  double w[H1_NB][3], s[H1_NB][3], dgam[H1_NB][3];  // dgam = d gamma / d theta_j
  int on[H1_NB];
};
struct KnotKin {
  double xp[H1_NX];
  double R0[9], D[4][9];
  double Rh[H1_NB][9], ph[H1_NB][3], zh[H1_NB][3], Om[H1_NB][3];
  PointSetDev S[3];          // 0 = whole-body CoM (URDF masses), 1 = left ankle origin, 2 = right ankle origin
  double Jc[3][3][H1_NX];    // d c / d x_p
  double Jv[3][3][H1_NX];    // d cdot / d x_p
};
// one weighted linear functional of c or cdot whose Hessian is needed: phi = vec^T c  or  vec^T cdot
struct HessCtx {
  int set, is_vel;
  double scale;
  double vec[3], til[3], Dv[4][3];
};

// serial part: pelvis-frame kinematics of the URDF tree (Pinocchio conventions)
__device__ inline void knot_base_kin(const double* x, KnotKin& K) {
  for (int i = 0; i < H1_NX; ++i) K.xp[i] = x[i];
  K.xp[3] = x[4]; K.xp[4] = x[5]; K.xp[5] = x[6]; K.xp[6] = x[3];   // derivatives.cpp:12-24
  const double qx = K.xp[3], qy = K.xp[4], qz = K.xp[5], qw = K.xp[6];
  {
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    K.R0[0] = 1 - (tyy + tzz); K.R0[1] = txy - twz; K.R0[2] = txz + twy;
    K.R0[3] = txy + twz; K.R0[4] = 1 - (txx + tzz); K.R0[5] = tyz - twx;
    K.R0[6] = txz - twy; K.R0[7] = tyz + twx; K.R0[8] = 1 - (txx + tyy);
  }
  for (int k = 0; k < 4; ++k) dR_dquat(k, K.xp + 3, K.D[k]);
  for (int k = 0; k < 9; ++k) K.Rh[0][k] = (k % 4 == 0) ? 1.0 : 0.0;
  for (int k = 0; k < 3; ++k) { K.ph[0][k] = 0.0; K.zh[0][k] = 0.0; K.Om[0][k] = K.xp[H1_NQ + 3 + k]; }
  for (int i = 1; i < H1_NB; ++i) {
    const int p = H1_PARENT[i], a = H1_AXIS[i];
    double Rj[9]; joint_rot(i, K.xp[7 + i - 1], H1U_RFIX, Rj);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) K.Rh[i][3 * r + c] = K.Rh[p][3 * r] * Rj[c] + K.Rh[p][3 * r + 1] * Rj[3 + c] + K.Rh[p][3 * r + 2] * Rj[6 + c];
    double t[3]; mv3(K.Rh[p], H1U_POS[i], t);
    const double qd = K.xp[H1_NQ + 6 + i - 1];
    for (int k = 0; k < 3; ++k) {
      K.ph[i][k] = K.ph[p][k] + t[k];
      K.zh[i][k] = K.Rh[i][3 * k + a];
      K.Om[i][k] = K.Om[p][k] + K.zh[i][k] * qd;
    }
  }
}
// point set `which`: subtree aggregates, beta, gamma, w, s, dgam
__device__ inline void knot_point_set(KnotKin& K, int which) {
  PointSetDev& S = K.S[which];
  double msub[H1_NB], hsub[H1_NB][3], sw[H1_NB][3];
  double mtot = 0.0;
  if (which == 0) for (int i = 0; i < H1_NB; ++i) mtot += H1U_MASS[i]; else mtot = 1.0;
  const int eb = (which == 1) ? H1_EE_LEFT : H1_EE_RIGHT;
  for (int i = 0; i < H1_NB; ++i) { msub[i] = 0.0; for (int k = 0; k < 3; ++k) { hsub[i][k] = 0.0; sw[i][k] = 0.0; } }
  double mall = 0.0;
  for (int i = H1_NB - 1; i >= 0; --i) {
    const double mu = (which == 0) ? H1U_MASS[i] / mtot : ((i == eb) ? 1.0 : 0.0);
    double ch[3] = {0.0, 0.0, 0.0};
    if (which == 0) mv3(K.Rh[i], H1U_COM[i], ch);
    msub[i] += mu; mall += mu;
    for (int k = 0; k < 3; ++k) hsub[i][k] += mu * (K.ph[i][k] + ch[k]);
    if (i > 0) { const int p = H1_PARENT[i]; msub[p] += msub[i]; for (int k = 0; k < 3; ++k) hsub[p][k] += hsub[i][k]; }
  }
  S.mfrac = mall;
  for (int k = 0; k < 3; ++k) S.beta[k] = hsub[0][k];
  const double* vb = K.xp + H1_NQ; const double* wb = K.xp + H1_NQ + 3;
  double wxb[3]; cross(wb, S.beta, wxb);
  for (int k = 0; k < 3; ++k) S.gamma[k] = S.mfrac * vb[k] + wxb[k];
  S.on[0] = 1;
  for (int i = 1; i < H1_NB; ++i) {
    S.on[i] = msub[i] > 0.0 ? 1 : 0;
    double r[3]; for (int k = 0; k < 3; ++k) r[k] = hsub[i][k] - msub[i] * K.ph[i][k];
    cross(K.zh[i], r, S.w[i]);
    const double qd = K.xp[H1_NQ + 6 + i - 1];
    for (int k = 0; k < 3; ++k) S.gamma[k] += qd * S.w[i][k];
  }
  for (int i = H1_NB - 1; i >= 1; --i) {
    const double qd = K.xp[H1_NQ + 6 + i - 1];
    const int p = H1_PARENT[i];
    for (int k = 0; k < 3; ++k) { S.s[i][k] = sw[i][k]; sw[p][k] += sw[i][k] + qd * S.w[i][k]; }
    double a[3], b[3]; cross(K.Om[i], S.w[i], a); cross(K.zh[i], S.s[i], b);
    for (int k = 0; k < 3; ++k) S.dgam[i][k] = a[k] + b[k];
  }
}
// column `c` (0..50) of the Jacobians of c and cdot for point set `which`
__device__ inline void knot_jac_column(KnotKin& K, int which, int c) {
  const PointSetDev& S = K.S[which];
  double jc[3] = {0, 0, 0}, jv[3] = {0, 0, 0};
  if (c < 3) { jc[c] = S.mfrac; }
  else if (c < 7) { mv3(K.D[c - 3], S.beta, jc); mv3(K.D[c - 3], S.gamma, jv); }
  else if (c < H1_NQ) { const int j = c - 7 + 1; if (S.on[j]) { mv3(K.R0, S.w[j], jc); mv3(K.R0, S.dgam[j], jv); } }
  else {
    const int cv = c - H1_NQ;
    double col[3] = {0, 0, 0};
    if (cv < 3) col[cv] = S.mfrac;
    else if (cv < 6) {  // -[beta]x column
      const int k = cv - 3; const double* b = S.beta;
      if (k == 0) { col[1] = -b[2]; col[2] = b[1]; } else if (k == 1) { col[0] = b[2]; col[2] = -b[0]; } else { col[0] = -b[1]; col[1] = b[0]; }
    } else { const int j = cv - 6 + 1; if (S.on[j]) { col[0] = S.w[j][0]; col[1] = S.w[j][1]; col[2] = S.w[j][2]; } }
    mv3(K.R0, col, jv);
  }
  for (int r = 0; r < 3; ++r) { K.Jc[which][r][c] = jc[r]; K.Jv[which][r][c] = jv[r]; }
}
DEVFN void make_ctx(const KnotKin& K, HessCtx& C, int set, int is_vel, double scale, const double* vec) {
  C.set = set; C.is_vel = is_vel; C.scale = scale;
  for (int k = 0; k < 3; ++k) C.vec[k] = vec[k];
  mtv3(K.R0, vec, C.til);
  for (int k = 0; k < 4; ++k) mtv3(K.D[k], vec, C.Dv[k]);
}
DEVFN bool related(int a, int b, int& lo, int& hi) {
  if (H1_ANC[a - 1][b - 1]) { lo = a; hi = b; return true; }
  if (H1_ANC[b - 1][a - 1]) { lo = b; hi = a; return true; }
  return false;
}
// coordinate classes of x_p: 0 p(0-2) | 1 quat(3-6) | 2 theta(7-25) | 3 v_b(26-28) | 4 omega_b(29-31) | 5 thetadot(32-50)
DEVFN int coord_class(int a) { return a < 3 ? 0 : (a < 7 ? 1 : (a < H1_NQ ? 2 : (a < H1_NQ + 3 ? 3 : (a < H1_NQ + 6 ? 4 : 5)))); }

// d2/dx_a dx_b of phi = vec^T (mfrac p + R0 beta)
DEVFN double hess_pos_entry(const KnotKin& K, const HessCtx& C, int a, int b) {
  const PointSetDev& S = K.S[C.set];
  int ca = coord_class(a), cb = coord_class(b);
  if (ca > cb) { int t = a; a = b; b = t; t = ca; ca = cb; cb = t; }
  if (ca == 1 && cb == 1) { double D2[9], t[3]; d2R_dquat2(a - 3, b - 3, D2); mv3(D2, S.beta, t); return dot3(C.vec, t); }
  if (ca == 1 && cb == 2) { const int j = b - 7 + 1; return S.on[j] ? dot3(C.Dv[a - 3], S.w[j]) : 0.0; }
  if (ca == 2 && cb == 2) {
    const int ja = a - 7 + 1, jb = b - 7 + 1; int lo, hi;
    if (!S.on[ja] || !S.on[jb] || !related(ja, jb, lo, hi)) return 0.0;
    double t[3]; cross(K.zh[lo], S.w[hi], t); return dot3(C.til, t);
  }
  return 0.0;
}
// d2/dx_a dx_b of phi = vec^T R0 gamma
DEVFN double hess_vel_entry(const KnotKin& K, const HessCtx& C, int a, int b) {
  const PointSetDev& S = K.S[C.set];
  int ca = coord_class(a), cb = coord_class(b);
  if (ca > cb) { int t = a; a = b; b = t; t = ca; ca = cb; cb = t; }
  if (ca == 0 || ca >= 3) return 0.0;   // p rows and the v-v block vanish
  if (ca == 1) {
    const int k = a - 3;
    if (cb == 1) { double D2[9], t[3]; d2R_dquat2(k, b - 3, D2); mv3(D2, S.gamma, t); return dot3(C.vec, t); }
    if (cb == 2) { const int j = b - 7 + 1; return S.on[j] ? dot3(C.Dv[k], S.dgam[j]) : 0.0; }
    if (cb == 3) return C.Dv[k][b - H1_NQ] * S.mfrac;
    if (cb == 4) {  // Dv . (-[beta]x e_c) = (beta x Dv)_c
      double t[3]; cross(S.beta, C.Dv[k], t); return t[b - H1_NQ - 3];
    }
    const int j = b - H1_NQ - 6 + 1; return S.on[j] ? dot3(C.Dv[k], S.w[j]) : 0.0;
  }
  // ca == 2
  const int ja = a - 7 + 1;
  if (!S.on[ja]) return 0.0;
  if (cb == 3) return 0.0;
  if (cb == 4) { double t[3]; cross(S.w[ja], C.til, t); return t[b - H1_NQ - 3]; }
  if (cb == 5) {
    const int jb = b - H1_NQ - 6 + 1; int lo, hi;
    if (!S.on[jb] || !related(ja, jb, lo, hi)) return 0.0;
    double t[3]; cross(K.zh[lo], S.w[hi], t); return dot3(C.til, t);
  }
  // theta-theta
  const int jb = b - 7 + 1; int lo, hi;
  if (!S.on[jb] || !related(ja, jb, lo, hi)) return 0.0;
  double zw[3], t1[3], dO[3], t2a[3], t2[3], t3a[3], t3[3];
  cross(K.zh[lo], S.w[hi], zw);
  cross(K.Om[lo], zw, t1);
  for (int r = 0; r < 3; ++r) dO[r] = K.Om[hi][r] - K.Om[lo][r];
  cross(dO, S.w[hi], t2a); cross(K.zh[lo], t2a, t2);
  cross(K.zh[hi], S.s[hi], t3a); cross(K.zh[lo], t3a, t3);
  return C.til[0] * (t1[0] + t2[0] + t3[0]) + C.til[1] * (t1[1] + t2[1] + t3[1]) + C.til[2] * (t1[2] + t2[2] + t3[2]);
}

}  // namespace h1
