// The task family of the augmented Lagrangian (ilqr_hip_set_al_task_bounds; no reference counterpart): bounds on nine points of the robot in
// the world frame -- task coordinate k in [0, 9): 0..2 the whole-body CoM, 3..5 the left ankle origin, 6..8 the right ankle origin -- the three
// point sets the cost tracks softly (h1_cost_dev.h: c = mfrac p + R(quat) beta(theta), Pinocchio conventions, URDF masses).
//   al_task_points   the nine coordinates of one state.  ONE function for every kernel that forms them -- the producer of the cost quadratics
//                    (k_quad_kin<., true>), the knot cost (k_al_task_knot_cost), the update (k_al_update<., ., ., true>) and the getter
//                    (k_al_task_points) -- with every operation rounded once (no contraction; the sine and cosine are written with explicit
//                    fma), so that each coordinate is the same double wherever it is formed: "is this side active" has one answer.
//   al_task_side     s = mu + rho c of one side under the same rule
//   al_task_term     the family's terms of knot t of rollout b, one division
// Layouts (h1_cost_dev.h states the other families'): the multiplier store, rollout b's record: one 128-byte line of scalars (ALT_RHO, the
// rest padding), then ALT_KNOT = 32 doubles (two whole lines) per knot t = 0..N: the multipliers of the nine lower bounds, of the nine upper
// bounds, padding.  The bounds are always a window: row t = lo[9], hi[9] padded to two lines, [N+1] rows per set, indexed by the rollout b and
// the knot t, never by a list position.  A foot's three rows at a knot where the contact schedule has it in stance (flag 1) are rows with both
// sides switched off, whatever the window holds: there the foot's slot in the cost kernels is the velocity functional.
#pragma once
#include "h1_cost_dev.h"
#include "h1_fast_math.h"
#include "h1_model_constexpr.h"

namespace h1 {

enum { ALT_COORDS = 9, ALT_RHO = 0, ALT_HDR = 16, ALT_LO = 0, ALT_HI = ALT_COORDS, ALT_KNOT = 32 };
enum { ALTB_LO = 0, ALTB_HI = ALT_COORDS, ALTB_FIELDS = 2 * ALT_COORDS, ALTB_STRIDE = (ALTB_FIELDS + 15) / 16 * 16 };
static_assert(ALT_HI + ALT_COORDS <= ALT_KNOT && ALT_KNOT % 16 == 0 && ALT_HDR % 16 == 0 && ALTB_STRIDE == 32, "task records: whole 128-byte lines");
inline long alt_record_doubles(int N) { return ALT_HDR + (long)ALT_KNOT * (N + 1); }

// mass fractions of the URDF tree as the cost quadratics' producer forms them (quad_kernels.hip QMASS): mu_i = m_i / sum m, mfrac = sum mu_i
constexpr double alt_mtot() { double m = 0.0; for (int k = 0; k < H1_NB; ++k) m += h1c::CU_MASS[k]; return m; }
constexpr double alt_mu(int i) { return h1c::CU_MASS[i] / alt_mtot(); }
constexpr double alt_mfrac() { double s = 0.0; for (int j = H1_NB - 1; j >= 0; --j) s += alt_mu(j); return s; }

struct AltBody { double R[9], p[3]; };      // body frame in the pelvis frame
template <int I, int r> DEVFN void alt_rj_row(double cs, double sn, double* o) {   // row r of Rfix_I Rot(axis_I, theta)
#pragma clang fp contract(off)
  constexpr double f0 = h1c::CU_RFIX[I][r][0], f1 = h1c::CU_RFIX[I][r][1], f2 = h1c::CU_RFIX[I][r][2];
  constexpr int ax = h1c::C_AXIS[I];
  if constexpr (ax == 0) { o[0] = f0; o[1] = f1 * cs + f2 * sn; o[2] = f2 * cs - f1 * sn; }
  else if constexpr (ax == 1) { o[0] = f0 * cs - f2 * sn; o[1] = f1; o[2] = f2 * cs + f0 * sn; }
  else { o[0] = f0 * cs + f1 * sn; o[1] = f1 * cs - f0 * sn; o[2] = f2; }
}
// body I from its parent; h += mu_I (p_I + R_I com_I), its share of the whole-body CoM
template <int I> DEVFN void alt_step(const AltBody& P, const double* x, AltBody& B, double* h) {
#pragma clang fp contract(off)
  double sn, cs; h1f::sincos_fast(x[7 + I - 1], &sn, &cs);
  double Rj[9];
  alt_rj_row<I, 0>(cs, sn, Rj); alt_rj_row<I, 1>(cs, sn, Rj + 3); alt_rj_row<I, 2>(cs, sn, Rj + 6);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) B.R[3 * r + c] = (P.R[3 * r] * Rj[c] + P.R[3 * r + 1] * Rj[3 + c]) + P.R[3 * r + 2] * Rj[6 + c];
  constexpr double px = h1c::CU_POS[I][0], py = h1c::CU_POS[I][1], pz = h1c::CU_POS[I][2];
  constexpr double c0 = h1c::CU_COM[I][0], c1 = h1c::CU_COM[I][1], c2 = h1c::CU_COM[I][2];
  constexpr double mu = alt_mu(I);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    B.p[k] = P.p[k] + ((P.R[3 * k] * px + P.R[3 * k + 1] * py) + P.R[3 * k + 2] * pz);
    h[k] = h[k] + mu * (B.p[k] + ((B.R[3 * k] * c0 + B.R[3 * k + 1] * c1) + B.R[3 * k + 2] * c2));
  }
}
template <int FIRST, int LEN> DEVFN void alt_chain(const AltBody& par, const double* x, AltBody& last, double* h) {
  AltBody a = par;
  if constexpr (LEN >= 1) { alt_step<FIRST>(a, x, last, h); a = last; }
  if constexpr (LEN >= 2) { alt_step<FIRST + 1>(a, x, last, h); a = last; }
  if constexpr (LEN >= 3) { alt_step<FIRST + 2>(a, x, last, h); a = last; }
  if constexpr (LEN >= 4) { alt_step<FIRST + 3>(a, x, last, h); a = last; }
  if constexpr (LEN >= 5) { alt_step<FIRST + 4>(a, x, last, h); }
}
// x: one state, MuJoCo slot order (quaternion w, x, y, z at 3..6); p[9]: CoM, left ankle origin, right ankle origin, world frame
DEVFN void al_task_points(const double* x, double* p) {
#pragma clang fp contract(off)
  const double qx = x[4], qy = x[5], qz = x[6], qw = x[3];      // (raw coefficients, Eigen's toRotationMatrix polynomial: h1_cost_dev.h knot_base_kin)
  double R0[9];
  {
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R0[0] = 1 - (tyy + tzz); R0[1] = txy - twz; R0[2] = txz + twy;
    R0[3] = txy + twz; R0[4] = 1 - (txx + tzz); R0[5] = tyz - twx;
    R0[6] = txz - twy; R0[7] = tyz + twx; R0[8] = 1 - (txx + tyy);
  }
  AltBody pel;
#pragma unroll
  for (int k = 0; k < 9; ++k) pel.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) pel.p[k] = 0.0;
  constexpr double mu0 = alt_mu(0);
  double h[3] = {mu0 * h1c::CU_COM[0][0], mu0 * h1c::CU_COM[0][1], mu0 * h1c::CU_COM[0][2]};
  AltBody lf, rf, tor, arm;
  alt_chain<1, 5>(pel, x, lf, h);
  alt_chain<6, 5>(pel, x, rf, h);
  alt_chain<11, 1>(pel, x, tor, h);
  alt_chain<12, 4>(tor, x, arm, h);
  alt_chain<16, 4>(tor, x, arm, h);
  constexpr double mfrac = alt_mfrac();
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    p[k] = mfrac * x[k] + ((R0[3 * k] * h[0] + R0[3 * k + 1] * h[1]) + R0[3 * k + 2] * h[2]);
    p[3 + k] = x[k] + ((R0[3 * k] * lf.p[0] + R0[3 * k + 1] * lf.p[1]) + R0[3 * k + 2] * lf.p[2]);
    p[6 + k] = x[k] + ((R0[3 * k] * rf.p[0] + R0[3 * k + 1] * rf.p[1]) + R0[3 * k + 2] * rf.p[2]);
  }
}
// one side of one coordinate: c = p - hi or lo - p (an infinite bound: c = -inf, s = -inf, nothing is active), s = mu + rho c
DEVFN double al_task_side(double c, double mu, double rho) {
#pragma clang fp contract(off)
  return mu + rho * c;
}
// row i of knot t is switched off where its foot stands (st: the knot's two stance flags)
DEVFN bool al_task_row_off(int i, const int* st) { return i >= 3 && st[i >= 6 ? 1 : 0] == 1; }
// The family's terms of knot t of rollout b (x: the knot's state), every knot: sum of (max(0, s)^2 - mu^2) over the 18 sides, divided once
DEVFN double al_task_term(const ProblemDev& P, int b, int t, const double* x) {
#pragma clang fp contract(off)
  double p[ALT_COORDS]; al_task_points(x, p);
  const double* r = P.alt + (long)b * P.alt_stride;
  const double* bd = P.altb + (long)b * P.altb_stride + (long)t * P.altb_knot;
  const int* st = P.stance + b * P.stance_stride + 2 * t;
  const int stf[2] = {st[0], st[1]};
  const double rho = r[ALT_RHO];
  const double* k = r + ALT_HDR + (long)t * ALT_KNOT;
  double c = 0.0;
#pragma unroll
  for (int i = 0; i < ALT_COORDS; ++i) {
    const bool off = al_task_row_off(i, stf);
    const double lo = off ? -__builtin_inf() : bd[ALTB_LO + i], hi = off ? __builtin_inf() : bd[ALTB_HI + i];
    const double mh = k[ALT_HI + i], ml = k[ALT_LO + i];
    const double sh = al_task_side(p[i] - hi, mh, rho), sl = al_task_side(lo - p[i], ml, rho);
    const double ph = sh > 0.0 ? sh : 0.0, pl = sl > 0.0 ? sl : 0.0;
    c += ph * ph - mh * mh;
    c += pl * pl - ml * ml;
  }
  return c / (2.0 * rho);
}

// ---- The VELOCITIES of the same three point sets in the world frame (ilqr_hip_get_al_task_velocities) -- coordinate k in [0, 9): 0..2 the
// velocity of the whole-body CoM, 3..5 of the left ankle origin, 6..8 of the right ankle origin -- the quantities R(quat) gamma_s(theta, v) the
// cost penalises softly (w_com_vel, w_ee_vel; Pinocchio's velocity convention: the base's linear and angular velocity in the body frame, the
// rotation polynomial on the raw quaternion, URDF masses).
//   al_task_velocities  the nine coordinates of one state under al_task_points' rounding rule (no contraction, every operation rounded once):
//                       the one function a family of bounds on these velocities would share between its kernels, as the task family shares
//                       al_task_points.  Today the getter's kernel (k_al_task_velocities) is its only caller.
enum { ALV_COORDS = 9 };

// body frame in the pelvis frame with its motion: origin velocity vp and angular velocity Om, both with the base's own motion included
struct AlvBody { double R[9], p[3], vp[3], Om[3]; };
DEVFN void alv_cross(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
// body I from its parent; hv += mu_I (vp_I + Om_I x R_I com_I), its share of the velocity of the whole-body CoM
template <int I> DEVFN void alv_step(const AlvBody& P, const double* x, AlvBody& B, double* hv) {
#pragma clang fp contract(off)
  constexpr int ax = h1c::C_AXIS[I];
  double sn, cs; h1f::sincos_fast(x[7 + I - 1], &sn, &cs);
  const double qd = x[H1_NQ + 6 + I - 1];
  double Rj[9];
  alt_rj_row<I, 0>(cs, sn, Rj); alt_rj_row<I, 1>(cs, sn, Rj + 3); alt_rj_row<I, 2>(cs, sn, Rj + 6);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) B.R[3 * r + c] = (P.R[3 * r] * Rj[c] + P.R[3 * r + 1] * Rj[3 + c]) + P.R[3 * r + 2] * Rj[6 + c];
  constexpr double px = h1c::CU_POS[I][0], py = h1c::CU_POS[I][1], pz = h1c::CU_POS[I][2];
  constexpr double c0 = h1c::CU_COM[I][0], c1 = h1c::CU_COM[I][1], c2 = h1c::CU_COM[I][2];
  constexpr double mu = alt_mu(I);
  double d[3], cm[3], wd[3], wc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[k] = (P.R[3 * k] * px + P.R[3 * k + 1] * py) + P.R[3 * k + 2] * pz;
    B.p[k] = P.p[k] + d[k];
    B.Om[k] = P.Om[k] + B.R[3 * k + ax] * qd;
    cm[k] = (B.R[3 * k] * c0 + B.R[3 * k + 1] * c1) + B.R[3 * k + 2] * c2;
  }
  alv_cross(P.Om, d, wd); alv_cross(B.Om, cm, wc);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    B.vp[k] = P.vp[k] + wd[k];
    hv[k] = hv[k] + mu * (B.vp[k] + wc[k]);
  }
}
template <int FIRST, int LEN> DEVFN void alv_chain(const AlvBody& par, const double* x, AlvBody& last, double* hv) {
  AlvBody a = par;
  if constexpr (LEN >= 1) { alv_step<FIRST>(a, x, last, hv); a = last; }
  if constexpr (LEN >= 2) { alv_step<FIRST + 1>(a, x, last, hv); a = last; }
  if constexpr (LEN >= 3) { alv_step<FIRST + 2>(a, x, last, hv); a = last; }
  if constexpr (LEN >= 4) { alv_step<FIRST + 3>(a, x, last, hv); a = last; }
  if constexpr (LEN >= 5) { alv_step<FIRST + 4>(a, x, last, hv); }
}
// x: one state, MuJoCo slot order (quaternion w, x, y, z at 3..6; v_b, omega_b of the base in its own frame at H1_NQ .. H1_NQ + 5);
// v[9]: the velocities of the CoM, the left ankle origin and the right ankle origin, world frame
DEVFN void al_task_velocities(const double* x, double* v) {
#pragma clang fp contract(off)
  const double qx = x[4], qy = x[5], qz = x[6], qw = x[3];      // (raw coefficients, as al_task_points)
  double R0[9];
  {
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R0[0] = 1 - (tyy + tzz); R0[1] = txy - twz; R0[2] = txz + twy;
    R0[3] = txy + twz; R0[4] = 1 - (txx + tzz); R0[5] = tyz - twx;
    R0[6] = txz - twy; R0[7] = tyz + twx; R0[8] = 1 - (txx + tyy);
  }
  AlvBody pel;
#pragma unroll
  for (int k = 0; k < 9; ++k) pel.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) { pel.p[k] = 0.0; pel.vp[k] = x[H1_NQ + k]; pel.Om[k] = x[H1_NQ + 3 + k]; }
  constexpr double mu0 = alt_mu(0);
  const double c0[3] = {h1c::CU_COM[0][0], h1c::CU_COM[0][1], h1c::CU_COM[0][2]};
  double w0[3]; alv_cross(pel.Om, c0, w0);
  double hv[3] = {mu0 * (pel.vp[0] + w0[0]), mu0 * (pel.vp[1] + w0[1]), mu0 * (pel.vp[2] + w0[2])};
  AlvBody lf, rf, tor, arm;
  alv_chain<1, 5>(pel, x, lf, hv);
  alv_chain<6, 5>(pel, x, rf, hv);
  alv_chain<11, 1>(pel, x, tor, hv);
  alv_chain<12, 4>(tor, x, arm, hv);
  alv_chain<16, 4>(tor, x, arm, hv);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = (R0[3 * k] * hv[0] + R0[3 * k + 1] * hv[1]) + R0[3 * k + 2] * hv[2];
    v[3 + k] = (R0[3 * k] * lf.vp[0] + R0[3 * k + 1] * lf.vp[1]) + R0[3 * k + 2] * lf.vp[2];
    v[6 + k] = (R0[3 * k] * rf.vp[0] + R0[3 * k + 1] * rf.vp[1]) + R0[3 * k + 2] * rf.vp[2];
  }
}

}  // namespace h1
