// Contact from geometry on the two-lane kernels (DESIGN 3.5 "Stance from the foot hulls"): does the collision hull of this
// lane's foot (even lane: left ankle link, odd lane: right) reach the floor z = 0?  The rule of h1host::foot_clearance
// (h1_host_model.cpp), i.e. of the reference's get_contacts.py:96-147 and of the contacts mj_step finds between the ankle-link
// geoms and the floor (robot_utils.cpp:106-117): the foot touches iff p_z(ankle) + min_v (R_ankle[2, :] . v) < 0 over the hull.
// Include after h1_aba_split.h.
#pragma once

#define H1_FOOT_HULL_QUAL static __constant__
#include "h1_foot_hull_groups.h"
#undef H1_FOOT_HULL_QUAL

namespace h1s {

// hinge K of the lane's leg: z of the link origin and row 2 of the link rotation, from the parent's (host forward_kinematics:
// p_i = p_p + R_p pos_i, R_i = R_p Rfix_i Rot(axis_i, theta_i); only the third row of R ever matters for a height)
template <int K> DEVFN void leg_row2(bool side, double* r, double& z, double th) {
  constexpr int IL = 1 + K, IR = 6 + K;
  static_assert(C_AXIS[IL] == C_AXIS[IR] && rfix_identity<IL>() && rfix_identity<IR>(), "leg links: mirror pairs without a fixed rotation");
  z += dot3z<C_POS[IL][0] == 0.0 && C_POS[IR][0] == 0.0, C_POS[IL][1] == 0.0 && C_POS[IR][1] == 0.0, C_POS[IL][2] == 0.0 && C_POS[IR][2] == 0.0>(
      side ? C_POS[IR][0] : C_POS[IL][0], side ? C_POS[IR][1] : C_POS[IL][1], side ? C_POS[IR][2] : C_POS[IL][2], r[0], r[1], r[2]);
  constexpr int a = C_AXIS[IL], b = (a + 1) % 3, d = (a + 2) % 3;
  double s, c; sincos(th, &s, &c);
  const double rb = r[b] * c + r[d] * s, rd = r[d] * c - r[b] * s;
  r[b] = rb; r[d] = rd;
}

// 1 iff the lane's foot touches the floor at (base height pz, base orientation quat (w, x, y, z), leg hinges th0..th4).
// The hull's vertices come in groups with bounding boxes (h1_foot_hull_groups.h); a group is scanned only if its box reaches
// below a margin of 1e-12 m over the floor.  r . v of a vertex and the box bound carry rounding errors of ~1e-17 m, so every
// vertex of a skipped group is above the floor in the very arithmetic of the scan: the answer is that of the scan of all 918
// vertices, and a lane stops scanning once it has found one below the floor (a swing foot costs the 29 group bounds, a stance
// foot the bounds and usually one group).  Not inlined: the rollout and line-search kernels already run at the register limit,
// and ONE machine code serves every kernel, so that a re-rollout decides exactly as the candidate it re-rolls.
__device__ __attribute__((noinline)) int foot_contact(bool side, double pz, double qw, double qx, double qy, double qz,
                                                     double th0, double th1, double th2, double th3, double th4) {
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  const double w = qw / qn, x = qx / qn, y = qy / qn, z = qz / qn;
  double r[3] = {2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};     // row 2 of the pelvis rotation (h1host quat_R)
  double h = pz;
  leg_row2<0>(side, r, h, th0);
  leg_row2<1>(side, r, h, th1);
  leg_row2<2>(side, r, h, th2);
  leg_row2<3>(side, r, h, th3);
  leg_row2<4>(side, r, h, th4);
  // (h, r): height and row 2 of the ankle link
  int hit = 0;
  for (int g = 0; g < H1_FOOT_HULL_NGROUPS; ++g) {
    const float* bx = H1_FOOT_HULL_BOX[g];
    const double lo = h + fmin(r[0] * (double)bx[0], r[0] * (double)bx[3]) + fmin(r[1] * (double)bx[1], r[1] * (double)bx[4]) +
                      fmin(r[2] * (double)bx[2], r[2] * (double)bx[5]);
    if (!hit && lo < 1e-12) {
#pragma unroll
      for (int k = 0; k < H1_FOOT_HULL_GROUP; ++k) {
        const float* v = H1_FOOT_HULL_G[g * H1_FOOT_HULL_GROUP + k];
        const double zv = r[0] * (double)v[0] + r[1] * (double)v[1] + r[2] * (double)v[2];
        hit |= (h + zv < 0.0) ? 1 : 0;
      }
    }
  }
  return hit;
}

// stance flags (left, right) of a step from the pair's own state: each lane tests its own foot, the pair swaps the answers
// (both lanes of the pair must be active)
DEVFN void geom_stance(bool side, const HalfX& hx, int& st_left, int& st_right) {
  const bool own = foot_contact(side, hx.p[2], hx.quat[0], hx.quat[1], hx.quat[2], hx.quat[3], hx.q.thL[0], hx.q.thL[1], hx.q.thL[2], hx.q.thL[3], hx.q.thL[4]) != 0;
  const bool par = xch_flag(own);
  st_left = (side ? par : own) ? 1 : 0;
  st_right = (side ? own : par) ? 1 : 0;
}

}  // namespace h1s
