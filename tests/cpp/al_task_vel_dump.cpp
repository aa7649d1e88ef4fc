// The oracle's velocity term  w |R0 gamma_s - target|^2  of one point set with a target of the caller's choice (tests/al_task_vel_ref.py):
// oracle/h1_costs.hpp's prepare_terms and its own add_vel_term / jac_vel / hess_vel, nothing else.  The oracle's cost path gives the feet's
// velocity term a fixed zero target; the task-velocity family of the augmented Lagrangian needs the Jacobian rows and the second-order sums of
// the feet's velocities, which a target of choice yields as the CoM's reference yields the CoM's.
// stdin: records of 56 doubles -- point set (0 CoM, 1 left ankle, 2 right ankle), w, the state x[51] (MuJoCo slot order), target[3];
// stdout per record: the velocity R0 gamma_s [3], the gradient [51] and the Hessian [51][51] that add_vel_term ADDS to a zero lx, lxx: the
// slot convention of Oracle.knot_quadratics (the quaternion's derivatives sit in the slots 3..6 in the order x, y, z, w, not un-permuted).
#include <cstdio>
#include <vector>

#include "h1_costs.hpp"

int main() {
  double in[56];
  std::vector<double> out(3 + H1_NX + H1_NX * H1_NX);
  while (std::fread(in, sizeof(double), 56, stdin) == 56) {
    const int set = (int)in[0];
    if (set < 0 || set > 2) return 2;
    orc::TermScratch Z; orc::prepare_terms(in + 2, Z);
    const orc::PointSet& S = set == 0 ? Z.com : Z.ee[set - 1];
    for (double& v : out) v = 0.0;
    orc::mat3_vec(Z.B.R0, S.gamma, out.data());
    orc::add_vel_term(Z.B, S, in + 2 + H1_NX, in[1], out.data() + 3, out.data() + 3 + H1_NX);
    if (std::fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size()) return 3;
  }
  return 0;
}
